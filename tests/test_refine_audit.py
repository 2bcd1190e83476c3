"""CPU: the float64 model of the cloud-to-cloud refiner (tests/refine_audit.py) against ground truth, against a float64
cKDTree, against itself under reversed summation, its step by two routes — and nine deliberately wrong readings of the
specification, each caught on a named cloud.

Measured here (and asserted below): the free-running model stops after 4 iterations on both convergent clouds, 2.4e-8 (cube) and
3.3e-9 (lattice) from the truth; summation spread 8.9e-16 / 1.05e-14; the two routes of the step differ by at most 3.6 units of
u * 2 |H|_F / (sigma_2 + s sigma_3)."""
import numpy as np
import pytest

import refine_audit as A


@pytest.mark.parametrize("name", ["cube", "lattice"])
def test_the_model_reaches_the_truth_and_stops_by_its_own_test(name):
    r, truth = A.free_run(name), A.convergent_cases()[name][2]
    assert r["converged"] and 0 < r["iterations"] < 30
    assert np.abs(r["T"] - truth).max() < 1e-6
    assert r["fitness"] == 1.0 and r["rmse"] < 1e-6
    assert len(r["history_T"]) == r["iterations"] + 1 and np.array_equal(r["history_T"][0], np.eye(4))


def test_the_lattice_trap_never_stops_by_its_own_test():
    r, truth = A.free_run("trap"), A.trap_case()[2]
    assert not r["converged"] and r["iterations"] == 30
    assert np.abs(r["T"] - truth).max() > 0.01  # (locked between lattice sites)


@pytest.mark.parametrize("name", ["cube", "lattice"])
def test_summation_spread_is_the_recorded_unit(name):
    a, b = A.free_run(name), A.free_run(name, True)
    assert a["iterations"] == b["iterations"] and a["converged"] == b["converged"]
    spread = np.abs(a["T"] - b["T"]).max()
    print(name, "spread", spread)
    assert spread <= A.SPREAD


def test_the_two_routes_of_the_step_agree_within_the_recorded_units():
    worst = 0.0
    for name in ("cube", "lattice", "trap"):
        for e in A.free_run(name)["evaluations"]:
            H = e.fig[8:].reshape(3, 3)
            unit = A.condition_unit(H)
            assert np.isfinite(unit)
            worst = max(worst, np.abs(A.rotation_svd(H) - A.rotation_horn(H)).max() / unit)
            R = A.rotation_horn(H)
            assert np.abs(R.T @ R - np.eye(3)).max() <= 16 * A.U and np.linalg.det(R) > 0
    print("worst", worst)
    assert 0 < worst <= A.STEP_UNITS
    # a reflection-prone H: both routes return the proper rotation
    H = np.diag([3.0, 2.0, -1.0])
    assert np.abs(A.rotation_svd(H) - A.rotation_horn(H)).max() <= A.STEP_UNITS * A.condition_unit(H)
    assert np.linalg.det(A.rotation_svd(H)) > 0 and np.linalg.det(A.rotation_svd(H, "no_reflection")) < 0


def test_correspondences_equal_a_float64_ckdtree_away_from_ties_and_the_bound():
    from scipy.spatial import cKDTree
    for name in ("cube", "lattice"):
        s, t, _ = A.convergent_cases()[name]
        T = A.rigid(0.02, (0.1, 0.0, 0.05))
        e = A.evaluate(T, s, t, 1.0)
        tree = cKDTree(t.astype(np.float64))
        d, i = tree.query(e.P, k=2, distance_upper_bound=1.0)
        clear = (np.abs(d[:, 0] - 1.0) > 1e-9) & (np.abs(d[:, 1] - d[:, 0]) > 1e-9)  # (no bound edge, no tie)
        want = np.where(np.isfinite(d[:, 0]), i[:, 0], -1)
        assert clear.mean() > 0.95 and np.array_equal(e.corr[clear], want[clear])
        assert (e.corr >= 0).sum() == np.isfinite(d[:, 0]).sum()
        np.testing.assert_allclose(np.sqrt(e.d2[e.corr >= 0]), d[e.corr >= 0, 0], rtol=1e-12)


# ---- wrong readings: each changes a named cloud's result ---------------------------------------------------------------------
def _bound_cloud():
    """sources exactly 1.0 from their only candidate: d2 == r2 is no correspondence"""
    target = np.array([[0, 0, 0], [10, 0, 0]], np.float32)
    source = np.array([[1, 0, 0], [10, 0.5, 0], [0, -1, 0]], np.float32)
    return source, target


def _tie_cloud():
    target = np.array([[1, 0, 0], [-1, 0, 0], [0, 3, 0], [0, 3, 0]], np.float32)
    source = np.array([[0, 0, 0], [0, 3.25, 0]], np.float32)
    return source, target


def test_wrong_bound_inclusive():
    s, t = _bound_cloud()
    assert list(A.evaluate(np.eye(4), s, t, 1.0).corr) == [-1, 1, -1]
    assert list(A.evaluate(np.eye(4), s, t, 1.0, wrong="inclusive").corr) == [0, 1, 0]


def test_wrong_ties_to_the_higher_row():
    s, t = _tie_cloud()
    assert list(A.evaluate(np.eye(4), s, t, 2.0).corr) == [0, 2]
    assert list(A.evaluate(np.eye(4), s, t, 2.0, wrong="ties_high").corr) == [1, 3]


def test_wrong_squared_distance_in_float32():
    # the moved point 999.749999 lies 1e-6 nearer to row 1 (999.5) than to row 0 (1000): float64 sees it, in float32 the point is
    # 999.75, the two distances tie and the lower row wins
    target = np.array([[1000.0, 0, 0], [999.5, 0, 0]], np.float32)
    source = np.array([[999.75, 0, 0]], np.float32)
    T = np.eye(4)
    T[0, 3] = -1e-6
    assert list(A.evaluate(T, source, target, 1.0).corr) == [1]
    assert list(A.evaluate(T, source, target, 1.0, wrong="d2_float32").corr) == [0]


def test_wrong_transform_applied_incrementally():
    s, t, _ = A.cube_case(400, 300, seed=5, offset=(2000.0, -1000.0, 10.0))
    a, b = A.run(s, t), A.run(s, t, wrong="incremental")
    assert np.abs(a["T"] - b["T"]).max() > 1e-7  # (the moved copy is rounded at every move)


def _reflection_cloud():
    """a planar cloud against its mirror image: the best orthogonal map is a reflection"""
    rng = np.random.default_rng(3)
    flat = np.concatenate([rng.uniform(-1, 1, (200, 2)), np.zeros((200, 1))], axis=1)
    target = flat.astype(np.float32)
    source = (flat * np.array([1.0, -1.0, 1.0]) * 0.2 + flat * 0.8).astype(np.float32)
    source[:, 2] = (0.02 * flat[:, 0] * flat[:, 1]).astype(np.float32)
    target[:, 2] = -source[:, 2]
    return source, target


def test_wrong_no_reflection_fix():
    H = np.diag([2.0, 1.0, -0.5])
    fig = np.concatenate([[10.0, 1.0], np.zeros(6), H.reshape(-1)])
    assert np.linalg.det(A.step(fig)[:3, :3]) > 0 and np.linalg.det(A.step(fig, wrong="no_reflection")[:3, :3]) < 0
    s, t = _reflection_cloud()
    e = A.evaluate(np.eye(4), s, t, 1.0)
    good, bad = A.step(e.fig), A.step(e.fig, wrong="no_reflection")
    assert np.linalg.det(good[:3, :3]) > 0.99 and np.linalg.det(bad[:3, :3]) < -0.99


def test_wrong_h_transposed_and_means_kept_and_fitness_only():
    s, t, truth = A.cube_case(500, 300, seed=2)
    good = A.run(s, t)
    assert good["converged"] and np.abs(good["T"] - truth).max() < 1e-6
    transposed = A.run(s, t, wrong="H_transposed")
    assert np.abs(transposed["T"] - truth).max() > 1e-3  # (the rotation goes the wrong way round)
    s2, t2, truth2 = A.cube_case(500, 300, seed=2, offset=(50.0, 20.0, 0.0))
    kept = A.run(s2, t2, wrong="means_kept")
    assert np.abs(A.run(s2, t2)["T"] - truth2).max() < 1e-5 and np.abs(kept["T"] - truth2).max() > 1e-3
    # fitness alone: full overlap from the start, so fitness never moves and the loop stops after one step
    only = A.run(s, t, wrong="fitness_only")
    assert only["iterations"] < good["iterations"] and np.abs(only["T"] - truth).max() > np.abs(good["T"] - truth).max()


def test_wrong_zero_rows_counted_in_the_denominator():
    s, t, _ = A.cube_case(300, 200, seed=4)
    s = np.concatenate([s, np.zeros((50, 3), np.float32), np.full((1, 3), 1e-30, np.float32)])
    a = A.evaluate(np.eye(4), s, t, 1.0, drop_source=True)
    b = A.evaluate(np.eye(4), s, t, 1.0, drop_source=True, wrong="zero_rows_counted")
    assert a.source_left_out == 51 and a.counted == 200 and b.counted == 251 and a.count == b.count
    assert a.fitness == a.count / 200 and b.fitness == a.count / 251
    # without the flag the zero rows are ordinary rows: counted, and matched where a target is near
    c = A.evaluate(np.eye(4), s, t, 1.0)
    assert c.counted == 251 and c.source_left_out == 0


def test_figures_exact_bounds_hold_for_the_models_own_float64_sums():
    for offset in ((0.0, 0.0, 0.0), (10000.0, -10000.0, 50.0)):
        s, t, _ = A.cube_case(600, 400, seed=7, offset=offset)
        e = A.evaluate(np.eye(4), s, t, 1.0)
        fig, tol = A.figures_exact(e, t, A.pivot(t))
        assert fig[0] == e.count and np.all(np.abs(e.fig - fig) <= tol + 64 * A.U * np.abs(fig)), (np.abs(e.fig - fig), tol)
        assert tol[8:].max() < 1e-9  # (about the pivot nothing cancels, 10 km from the origin either)
