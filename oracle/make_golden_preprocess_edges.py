"""Golden vectors for the preprocessing audit (tests/preprocess_audit.py): the reference's own `voxelise` / `voxel_hashing` /
`sample_from_hashes` / `voxel_normal_distribution` (slam/common/pointcloud.py:13-179) and `Distortion.filter`
(slam/preprocessing.py:144-191), imported from /root/reference through oracle/shims, on the audit's small edge cases:
exact rounding ties, colliding voxels, the voxel whose hash is -1, wrapping full-range hashes, and the de-skew motions
(exact float64 and float32-rounded poses) at n = 4000.  TEST INFRASTRUCTURE.

    python oracle/make_golden_preprocess_edges.py      # writes tests/golden/preprocess_edges.npz

Every input comes from the seeded builders of tests/preprocess_audit.py, so only its sha1 is stored; the outputs are
stored whole, except the de-skewed clouds: the filter runs on all 4000 points and every DESKEW_STRIDE-th row is kept (19
float64 clouds of 4000 rows would not fit the size budget of a fixture).

As in make_golden_distortion.py the rows go to `voxelise` as float64: numba types float32 / float64 as float64, the plain
Python body under the numba stand-in would divide in float32.
"""
import hashlib
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle", "shims"), "/root/reference", os.path.join(ROOT, "pylidar-slam_amd"),
                os.path.join(ROOT, "tests")]
logging.disable(logging.WARNING)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)
from slam.common.pointcloud import sample_from_hashes, voxel_hashing, voxel_normal_distribution, voxelise  # noqa: E402
from slam.preprocessing import Distortion, DistortionConfig  # noqa: E402

import preprocess_audit as P  # noqa: E402

DESKEW_N, DESKEW_STRIDE = 4000, 16


def sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out = {}
    cases = P.tie_cases() + [P.collision_case()] + P.sentinel_cases() + [P.wrap_case()]
    out["grid_cases"] = np.array([c.name for c in cases])
    for c in cases:
        assert c.n <= 4000
        with np.errstate(over="ignore"):
            vox = voxelise(c.points.astype(np.float64), c.voxel)
            hashes = np.zeros(c.n, np.int64)
            voxel_hashing(vox, hashes)
        _, idx = sample_from_hashes(c.points, hashes)
        out[f"{c.name}_sha"] = np.array(sha(c.points))
        out[f"{c.name}_voxels"], out[f"{c.name}_hashes"], out[f"{c.name}_indices"] = vox, hashes, idx.astype(np.int64)
        if not c.f64:  # Voxelization.filter: float32 clouds
            sizes, means, covs, ids = voxel_normal_distribution(c.points, hashes)
            out[f"{c.name}_sizes"], out[f"{c.name}_means"] = np.asarray(sizes, np.int64), np.asarray(means)
            out[f"{c.name}_covs"], out[f"{c.name}_ids"] = np.asarray(covs), np.asarray(ids, np.int64)
        print(c.name, c.n, idx.shape[0])
    pc, ts = P.deskew_points(DESKEW_N), P.deskew_timestamps(DESKEW_N, "epoch")
    out["deskew_sha"] = np.array(sha(pc) + sha(ts))
    out["deskew_stride"] = np.int64(DESKEW_STRIDE)
    for name, rpose in P.deskew_motions().items():
        d = {"numpy_pc": pc, "numpy_pc_timestamps": ts, "init_rpose": rpose}
        Distortion(DistortionConfig(output_key="distorted")).filter(d)
        assert d["distorted"].dtype == np.float64 and d["distorted"].shape == (DESKEW_N, 3)
        out[f"deskew_{name}"] = d["distorted"][::DESKEW_STRIDE]
        out[f"deskew_{name}_rpose"] = rpose
    path = os.path.join(ROOT, "tests", "golden", "preprocess_edges.npz")
    np.savez_compressed(path, **out)
    print("preprocess_edges.npz", os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
