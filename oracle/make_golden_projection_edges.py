"""What does the REFERENCE do on the edges of its spherical projection?  TEST INFRASTRUCTURE, build container only:

    python oracle/make_golden_projection_edges.py      # writes tests/golden/projection_edges.npz

Runs the unmodified `SphericalProjector.project_pointcloud` and `build_projection_map` (slam/common/projection.py:11-73,
:331-418) in a child process under the scalar capability (ATEN_CPU_CAPABILITY=default, one thread: the scatter of :415 is
deterministic only then) on the boundary, image-edge, special-row and tie clouds of tests/projection_audit.py at 16 x 128,
field of view (3, -24), and stores per cloud the input rows, the float pixel coordinates and the vertex map — data only.
tests/test_projection_audit.py holds the bit model of the kernels to these recordings wherever the reference's answer does
not hang on the last bit of its float32 atan2 / asin or on its unstable argsort."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "projection_edges.npz")
H, W, UP, DOWN = 16, 128, 3.0, -24.0
CLOUDS = ("boundary", "image_edge", "special", "ties")

CHILD = r'''
import sys, logging
sys.path[:0] = [%(shims)r, "/root/reference", %(tests)r]
logging.disable(logging.WARNING)
import numpy as np, torch
torch.set_num_threads(1)
from slam.common.projection import SphericalProjector
import projection_audit as P
h, w, up, down = %(h)d, %(w)d, %(up)r, %(down)r
out = {"capability": np.array(torch.backends.cpu.get_cpu_capability()), "hw": np.array([h, w]), "fov": np.array([up, down])}
proj = SphericalProjector(h, w, 3, up, down)
for name, pc in P.clouds(h, w, up, down, which=%(clouds)r).items():
    t = torch.from_numpy(pc).unsqueeze(0)
    out[name + "_pc"] = pc
    out[name + "_pix"] = proj.project_pointcloud(t)[0].numpy()
    out[name + "_vmap"] = proj.build_projection_map(t)[0].numpy()
out["special_kind"] = P.special(h, w, up, down)[1]
np.savez_compressed(sys.argv[1], **out)
'''


def main():
    import numpy as np
    src = CHILD % dict(shims=os.path.join(ROOT, "oracle", "shims"), tests=os.path.join(ROOT, "tests"), h=H, w=W, up=UP,
                       down=DOWN, clouds=CLOUDS)
    subprocess.run([sys.executable, "-c", src, OUT], check=True, env=dict(os.environ, ATEN_CPU_CAPABILITY="default"))
    r = np.load(OUT)
    assert "default" in str(r["capability"]).lower(), f"the scalar capability was not honoured (ran as {r['capability']})"
    for name in CLOUDS:
        print(name, r[name + "_pc"].shape, r[name + "_pix"].shape, r[name + "_vmap"].shape)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
