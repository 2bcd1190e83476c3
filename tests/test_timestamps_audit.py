"""CPU: the model the azimuth time stamps are held to (tests/timestamps_audit.py) against the reference's own
`estimate_timestamps` (slam/common/geometry.py:443-466), the committed golden, the KITTI-360 ground truth and loader up to
the point where a GPU is needed, and the comparison helpers against wrong copies.  The reference is imported from
/root/reference through oracle/shims; the tests that need it are skipped where that checkout is absent (the GPU box)."""
import os
import sys

import numpy as np
import pytest

import timestamps_audit as A

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "timestamps_reference.npz")
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "slam")), reason="reference checkout not present")


@pytest.fixture()
def reference_on_path():
    import logging
    logging.disable(logging.WARNING)
    added = [os.path.join(ROOT, "oracle", "shims"), REF]
    sys.path[:0] = added
    yield
    for p in added:
        sys.path.remove(p)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module")
def clouds(golden):
    """the two golden scans and a larger one with an odd row count, xyz only"""
    return [golden["scan_a"][:, :3], golden["scan_b"][:, :3], A.make_scan(362, 40001, 3, 8)]


def _ref_key(name, cw, k):
    return f"ref_{name}_{'cw' if cw else 'ccw'}_{k}"


# ---- the model against the reference ---------------------------------------------------------------------------------
@needs_reference
def test_model_within_the_reference_spread(reference_on_path, clouds, golden):
    """Measures the reference-side spread — max |reference(float32 rows) - reference(the same rows as float64)| — over the
    clouds and every (direction, phi_0), and holds the model within 4 x it of BOTH evaluations (float32 and float64 rows).
    Measured here: spread 1.4e-7, model 1.8e-7 from the float32 evaluation."""
    from slam.common.geometry import estimate_timestamps
    runs = []
    for rows in clouds:
        assert A.seam_safe(rows)
        for cw in A.DIRECTIONS:
            for phi_0 in A.PHI_0S:
                r32 = estimate_timestamps(rows, clockwise=cw, phi_0=phi_0)
                r64 = estimate_timestamps(rows.astype(np.float64), clockwise=cw, phi_0=phi_0)
                assert r32.dtype == np.float32 and r64.dtype == np.float64
                assert r32.min() == 0.0 and r32.max() == 1.0  # Distortion's renormalisation is the identity on these
                runs.append((rows, cw, phi_0, r32, r64))
    spread = max(A.worst_difference(r32, r64) for _, _, _, r32, r64 in runs)
    print(f"reference-side spread {spread:.3e} (recorded with the golden: {float(golden['spread']):.3e})")
    assert 1.0e-8 < spread < 1.0e-6
    worst = 0.0
    for rows, cw, phi_0, r32, r64 in runs:
        m = A.model(rows, cw, phi_0)
        assert m.flagged.sum() <= A.FLAGGED_MAX * rows.shape[0]
        assert m.t.dtype == np.float64 and np.nanmin(m.t) == 0.0 and np.nanmax(m.t) == 1.0
        assert A.same_bits(m.t.astype(np.float32).astype(np.float64), m.t)  # float32 values, widened
        worst = max(worst, A.check_within(m.t, r32, 4 * spread, f"float32 rows, clockwise={cw}, phi_0={phi_0}"))
        worst = max(worst, A.check_within(m.t, r64, 4 * spread, f"float64 rows, clockwise={cw}, phi_0={phi_0}"))
    print(f"model to reference, worst {worst:.3e}")


@needs_reference
def test_golden_is_the_reference(reference_on_path, golden):
    """the recorded outputs are what the reference gives for the recorded scans (within its own spread: numpy's float32
    arctan2 may differ by an ulp between CPUs), and the recorded spread is the one measured on them"""
    from slam.common.geometry import estimate_timestamps
    spread = 0.0
    for name in "ab":
        rows = golden[f"scan_{name}"][:, :3]
        for cw in A.DIRECTIONS:
            for k, phi_0 in enumerate(A.PHI_0S):
                r32 = estimate_timestamps(rows, clockwise=cw, phi_0=phi_0)
                spread = max(spread, A.worst_difference(r32, estimate_timestamps(rows.astype(np.float64), clockwise=cw, phi_0=phi_0)))
                if _ref_key(name, cw, k) in golden.files:
                    A.check_within(golden[_ref_key(name, cw, k)], r32, float(golden["spread"]), _ref_key(name, cw, k))
    assert 0.5 * spread <= float(golden["spread"]) <= 2.0 * spread


@needs_reference
def test_seam_and_nan_cases_exactly(reference_on_path):
    from slam.common.geometry import estimate_timestamps
    rows = A.make_scan(5, 300, 3, 10)
    seam = np.arange(290, 300)
    for cw in A.DIRECTIONS:  # y = +0 -> +-pi, y = -0 -> -+pi: both exactly 0 with phi_0 = pi, whichever way round
        ref = estimate_timestamps(rows, clockwise=cw, phi_0=np.pi)
        m = A.model(rows, cw, np.pi)
        A.check_seam(ref, seam, "reference")
        A.check_seam(m.t, seam, "model")
        assert m.lo == 0.0
    # x = y = 0 (atan2 = 0) and x = -0 (atan2 = +-pi): rows like any other, reference and model agree on them exactly
    odd = rows.copy()
    odd[0, :2] = (0.0, 0.0)
    odd[1, :2] = (-0.0, 0.0)
    odd[2, :2] = (-0.0, -0.0)
    ref, m = estimate_timestamps(odd, clockwise=True, phi_0=np.pi), A.model(odd, True, np.pi)
    assert np.array_equal(ref[:3].astype(np.float64), m.t[:3]) and m.t[1] == 0.0 and m.t[2] == 0.0
    # one row, and rows that share one azimuth: 0 / 0 = NaN for every row, on both sides
    for same in (rows[:1], np.repeat(rows[7:8], 5, axis=0), rows[7:8] * np.array([[1.0], [2.0], [4.0]], np.float32)):
        with np.errstate(invalid="ignore"):
            ref = estimate_timestamps(same, clockwise=True, phi_0=np.pi)
        assert np.isnan(ref).all() and np.isnan(A.model(same, True, np.pi).t).all()
    # a NaN coordinate: the reference's min / max hand it on to every row; the device's fminf / fmaxf — and the model —
    # drop it: that row NaN, the others as without it (the deviation include/icp_mi355x.h documents)
    bad = rows.copy()
    bad[123, 1] = np.nan
    with np.errstate(invalid="ignore"):
        assert np.isnan(estimate_timestamps(bad, clockwise=True, phi_0=np.pi)).all()
    m, without = A.model(bad, True, np.pi), A.model(np.delete(rows, 123, axis=0), True, np.pi)
    assert np.isnan(m.t[123]) and A.same_bits(np.delete(m.t, 123), without.t)
    with pytest.raises(ValueError):  # an empty scan raises in the reference (the library refuses n <= 0)
        estimate_timestamps(rows[:0], clockwise=True, phi_0=np.pi)


# ---- the committed golden, where the reference is not at hand ----------------------------------------------------------
def test_golden_file_and_model(golden):
    assert os.path.getsize(GOLDEN) < 300 * 1024
    spread = float(golden["spread"])
    assert 1.0e-8 < spread < 1.0e-6
    seam = golden["seam_index"]
    assert np.array_equal(golden["phi_0s"], np.array(A.PHI_0S))
    seen = 0
    for name in "ab":
        scan = golden[f"scan_{name}"]
        assert scan.shape == (4096, 4) and scan.dtype == np.float32 and A.seam_safe(scan)
        assert np.all(scan[seam, 1] == 0) and np.all(scan[seam, 0] < 0) and np.signbit(scan[seam, 1]).any()
        for cw in A.DIRECTIONS:
            for k, phi_0 in enumerate(A.PHI_0S):
                m = A.model(scan, cw, phi_0)
                assert not m.flagged.any()  # (the seeds were chosen so: the GPU test holds the kernel to every row)
                if _ref_key(name, cw, k) not in golden.files:
                    continue
                ref = golden[_ref_key(name, cw, k)]
                assert ref.dtype == np.float32
                A.check_within(m.t, ref, 4 * spread, _ref_key(name, cw, k))
                if k == 1:
                    A.check_seam(ref, seam, "reference")
                    A.check_seam(m.t, seam, "model")
                seen += 1
    assert seen == 9


def test_wrong_copies_fail_the_helpers(golden):
    scan, seam = golden["scan_a"], golden["seam_index"]
    m = A.model(scan, True, np.pi)
    A.check_bits(m.t.copy(), m.t)
    A.check_seam(m.t, seam)
    # a seam row flipped to the other end of the turn
    flipped = m.t.copy()
    flipped[seam[3]] = 1.0
    with pytest.raises(AssertionError):
        A.check_seam(flipped, seam)
    with pytest.raises(AssertionError):
        A.check_bits(flipped, m.t)
    with pytest.raises(AssertionError):
        A.check_within(flipped, golden["ref_a_cw_1"], 4 * float(golden["spread"]))
    # one ulp in one row's phi
    phi = m.phi.copy()
    phi[1000] = np.nextafter(phi[1000], np.float32(np.inf))
    with pytest.raises(AssertionError):
        A.check_bits(A.normalise(phi, m.lo, m.hi), m.t)
    # min / max over n - 1 rows: the last row holds the largest phi
    n = scan.shape[0] - seam.size
    rows = A.place_extremes(scan[:n], 0, n - 1, True, 1.0)
    right, short = A.model(rows, True, 1.0), A.model(rows, True, 1.0, minmax_rows=n - 1)
    assert short.hi < right.hi
    with pytest.raises(AssertionError):
        A.check_bits(short.t, right.t)
    # a NaN on one side only is a difference, not a match
    nan = m.t.copy()
    nan[5] = np.nan
    with pytest.raises(AssertionError):
        A.check_bits(nan, m.t)
    assert A.worst_difference(nan, m.t) == np.inf


def test_place_extremes_and_flags():
    rows = A.make_scan(9, 700, 3)
    for lo_at, hi_at in ((0, 699), (699, 0), (255, 256), (256, 255)):
        placed = A.place_extremes(rows, lo_at, hi_at, False, -2.5)
        m = A.model(placed, False, -2.5)
        assert m.t[lo_at] == 0.0 and m.t[hi_at] == 1.0
    # the flag: an angle within two float64 ulp of the middle of two float32 values, and none further away
    a32 = np.float32(0.7)
    mid = (np.float64(a32) + np.float64(np.nextafter(a32, np.float32(1.0)))) / 2
    near = np.array([mid, np.nextafter(mid, 0.0), np.nextafter(mid, 1.0)])
    far = np.array([np.float64(a32), mid + 4 * np.spacing(mid), mid - 4 * np.spacing(mid), np.nan])
    assert A.near_rounding_boundary(near).all() and not A.near_rounding_boundary(far).any()


# ---- KITTI-360: ground truth and loader --------------------------------------------------------------------------------
@needs_reference
def test_kitti360_sequence_poses_against_the_reference(reference_on_path, tmp_path):
    """float64 and the same scipy on both sides: equal to 1e-12 relative (measured here: 0 — bit for bit)."""
    from slam.dataset.kitti_360_dataset import get_sequence_poses
    from pylidar_slam_amd.dataset import kitti360_sequence_poses
    A.write_kitti360_tree(tmp_path, frames=3, rows=8)
    ref = get_sequence_poses(str(tmp_path), 0)
    ours = kitti360_sequence_poses(str(tmp_path), 0)
    assert ref.shape == ours.shape == (3, 4, 4) and ours.dtype == np.float64
    diff = np.abs(ours - ref).max() / np.abs(ref).max()
    print(f"kitti360_sequence_poses against get_sequence_poses: {diff:.3e} relative")
    assert diff <= 1.0e-12
    assert not np.allclose(ours[0], ours[1]) and not np.allclose(ours[1], ours[2])  # the middle frame is interpolated
    assert kitti360_sequence_poses(str(tmp_path), 2) is None  # no poses.txt for that drive


def test_kitti360_loader_up_to_the_gpu(tmp_path):
    from pylidar_slam_amd import eval as our_eval
    from pylidar_slam_amd.dataset import (KITTI360_DRIVES, KITTI360Config, KITTI360DatasetLoader, KITTI360Sequence,
                                          kitti360_sequence_poses)
    A.write_kitti360_tree(tmp_path, frames=3, rows=8)
    cfg = KITTI360Config(root_dir=str(tmp_path), lidar_height=16, lidar_width=256)
    assert cfg.train_sequences == [0, 2, 3, 4, 5, 6, 7, 9, 10] and cfg.test_sequences == [0, 2, 3, 4, 5, 6, 7]
    assert cfg.eval_sequences == [9, 10] and cfg.dataset == "kitti_360"
    loader = KITTI360DatasetLoader(cfg)  # no GPU context yet
    proj = loader.projector()
    assert (proj.height, proj.width) == (16, 256)
    (train, names), (ev, ev_names), (test, test_names), transform = loader.sequences()
    assert names == ["0"] and test_names == ["0"] and ev == [] and ev_names == []
    seq = train[0]
    assert isinstance(seq, KITTI360Sequence) and len(seq) == KITTI360_DRIVES[0] == 11518
    poses = kitti360_sequence_poses(str(tmp_path), 0)
    from_first = np.einsum("ij,njk->nik", np.linalg.inv(poses[0]), poses)
    assert np.array_equal(seq.gt_poses, from_first) and np.allclose(seq.gt_poses[0], np.eye(4), atol=1e-12)
    assert np.array_equal(loader.get_ground_truth("0"), our_eval.compute_relative_poses(from_first))
    assert loader.get_ground_truth("2") is None
    with pytest.raises(AssertionError):
        KITTI360Sequence(str(tmp_path), 1, None)  # KITTI-360 has no drive 1


@needs_reference
def test_kitti_360_registers_with_the_reference(reference_on_path, tmp_path):
    import slam.dataset as ref_dataset
    from omegaconf import DictConfig
    from pylidar_slam_amd import dataset as our_dataset
    from pylidar_slam_amd.register import DATASET_NAMES, register_with_reference
    register_with_reference()
    ds = ref_dataset.DATASET
    assert DATASET_NAMES[-1] == "kitti_360_mi355x" and DATASET_NAMES[:2] == ("synthetic_mi355x", "kitti_mi355x")
    assert "kitti_360_mi355x" in ds.__members__ and "kitti_360" in ds.__members__
    A.write_kitti360_tree(tmp_path, frames=3, rows=8)
    loader = ds.load(DictConfig({"dataset": "kitti_360_mi355x", "root_dir": str(tmp_path), "lidar_width": 512}))
    assert isinstance(loader, our_dataset.KITTI360DatasetLoader) and loader.config.lidar_width == 512
    (train, names), _, _, _ = loader.sequences()
    assert names == ["0"] and train[0].gt_poses.shape == (3, 4, 4)
    # the group file names the same loader and the reference's defaults
    text = open(os.path.join(ROOT, "config", "dataset", "kitti_360_mi355x.yaml")).read()
    assert "dataset: kitti_360_mi355x" in text and "root_dir:" in text
