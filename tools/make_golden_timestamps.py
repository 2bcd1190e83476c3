"""Golden vectors for the azimuth time stamps, produced by the reference's own `estimate_timestamps`
(slam/common/geometry.py:443-466, imported from a reference checkout through oracle/shims).  TEST INFRASTRUCTURE.

    python tools/make_golden_timestamps.py [reference checkout]     # writes tests/golden/timestamps_reference.npz

The file holds arrays only: two [4096, 4] float32 scans (seam-safe rows, the last 32 exactly on the seam of the KITTI-360
setting: y = +-0, x < 0), the reference's float32 outputs for them, and the reference-side spread — max |reference(float32
rows) - reference(the same rows as float64)| over both scans and every (direction, phi_0) audited.  The GPU tests, which
cannot see the reference, read it from here.
"""
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
sys.path[:0] = [os.path.join(ROOT, "oracle", "shims"), REF, os.path.join(ROOT, "tests")]
logging.disable(logging.WARNING)

import numpy as np  # noqa: E402

from slam.common.geometry import estimate_timestamps  # noqa: E402

import timestamps_audit as A  # noqa: E402

N, SEAM_ROWS = 4096, 32
SEEDS = (360, 361)


def main():
    scans = [A.make_scan(seed, N, 4, SEAM_ROWS) for seed in SEEDS]
    out = {"scan_a": scans[0], "scan_b": scans[1], "seam_index": np.arange(N - SEAM_ROWS, N),
           "phi_0s": np.array(A.PHI_0S, np.float64)}
    spread = 0.0
    for name, scan in zip("ab", scans):
        assert A.seam_safe(scan)
        for cw in A.DIRECTIONS:
            for k, phi_0 in enumerate(A.PHI_0S):
                r32 = estimate_timestamps(scan[:, :3], clockwise=cw, phi_0=phi_0)
                r64 = estimate_timestamps(scan[:, :3].astype(np.float64), clockwise=cw, phi_0=phi_0)
                assert r32.dtype == np.float32 and r64.dtype == np.float64
                spread = max(spread, A.worst_difference(r32, r64))
                # scan a: every setting; scan b: the KITTI-360 setting (clockwise, phi_0 = pi) — the file stays below 300 KB
                if name == "a" or (cw and k == 1):
                    out[f"ref_{name}_{'cw' if cw else 'ccw'}_{k}"] = r32
    out["spread"] = np.float64(spread)
    path = os.path.join(ROOT, "tests", "golden", "timestamps_reference.npz")
    np.savez_compressed(path, **out)
    print(f"spread {spread:.3e}; {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
