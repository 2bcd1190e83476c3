"""`-m gpu`: the cloud-to-cloud refiner (icp_refine_*, IcpContext.cloud_refiner; csrc/refine.hip) against the float64 numpy
model of tests/refine_audit.py, evaluation by evaluation from the kernel's own history: at every recorded T_i the
correspondence of every source row equals the model's brute-force answer BIT FOR BIT (index and the -1s), the count is exact,
fitness and inlier_rmse are bit-equal to the model on the kernel's own count and sum d2, sum d2 / mu / H lie within the
summation bound gamma_n * sum|terms| about the pivot, and T_{i+1} is the model's step from the kernel's own 17 figures within
4 x STEP_UNITS = 14.4 condition units, gross: |T_{i+1} - model| with no allowance for the roundings of the product (degenerate
clouds: R read back through T_{i+1} T_i^-1, a proper rotation to 16 u plus the rounding of that read-back, t = mu_q - R mu_p;
the 16 u on R itself is held on the host build of the same step, tests/test_refine_host.py).  Free-running, the final T
stays within 4 x SPREAD of the free-running model with equal iteration count and `converged`.

No deliberately wrong kernel runs here: the wrong readings of the specification are caught on the CPU
(tests/test_refine_audit.py)."""
import numpy as np
import pytest

import refine_audit as A

pytestmark = pytest.mark.gpu

WORST = [0.0]  # the worst gross step error of the session, in condition units (printed by the last audit)
GRID_ROWS = 2048 * 256  # source rows of a full grid of workgroups (REF_MAX_BLOCKS x REF_THREADS)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    from pylidar_slam_amd.engine import IcpContext
    c = IcpContext(height=16, width=128, max_num_alignments=6, threshold_delta_pose=0.0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _refiner(ctx, target, source_rows, cell=1.0, drop_target=False, room=None):
    r = ctx.cloud_refiner(room or max(len(target), 1), max(source_rows, 1), cell)
    r.set_target(target, drop_zero_rows=drop_target)
    return r


def _degenerate(fig):
    unit = A.condition_unit(fig[8:].reshape(3, 3))
    return fig[0] < 3 or not np.isfinite(unit) or unit > 1e-6


def _audit(r, source, target, res, max_distance=1.0, drop_source=False, drop_target=False, degenerate_ok=False, what=""):
    """every evaluation of the run `res` of refiner `r`, from the kernel's own T_i; returns the worst step error in condition units"""
    hist_T, hist_S = r.history()
    assert len(hist_T) == res.iterations + 1, what
    c = A.pivot(target, drop_target)
    worst = 0.0
    for i, (T, fig) in enumerate(zip(hist_T, hist_S)):
        e = A.evaluate(T, source, target, max_distance, drop_source, drop_target)
        again = r.refine(source, init=T, max_distance=max_distance, max_iteration=0, drop_zero_rows=drop_source)
        assert again.iterations == 0 and not again.converged and np.array_equal(_bits(again.transformation), _bits(T)), (what, i)
        corr = again.correspondences
        assert corr.dtype == np.int32 and np.array_equal(corr, e.corr), (what, i, int((corr != e.corr).sum()))
        assert again.num_correspondences == e.count == int(fig[0]) and again.source_rows == e.counted, (what, i)
        fitness, rmse = A.fitness_rmse(e.count, e.counted, fig[1])
        assert _bits(again.fitness) == _bits(fitness) and _bits(again.inlier_rmse) == _bits(rmse), (what, i)
        exact, tol = A.figures_exact(e, target, c)
        assert np.all(np.abs(fig - exact) <= tol), (what, i, np.abs(fig - exact) / np.maximum(tol, 1e-300))
        if i == len(hist_T) - 1:
            assert np.array_equal(_bits(res.transformation), _bits(T)) and _bits(res.fitness) == _bits(fitness), (what, "final")
            assert _bits(res.inlier_rmse) == _bits(rmse) and res.num_correspondences == e.count
            break
        # T_{i+1} = update T_i: the rotation of the update against the model's step from the kernel's own figures
        nxt = hist_T[i + 1]
        if _degenerate(fig):
            assert degenerate_ok, (what, i, "a degenerate evaluation on a cloud that is not named as such")
            if not fig[0] > 0:
                assert np.array_equal(nxt, T), (what, i)  # the identity update
                continue
            inv = np.linalg.inv(T)
            up = nxt @ inv
            R, t = up[:3, :3], up[:3, 3]
            # (R is read back through T_{i+1} T_i^-1: the 16 u of the rotation, and as much for the two products)
            assert np.abs(R.T @ R - np.eye(3)).max() <= 16 * A.U + 16 * A.U * (np.abs(nxt[:3, :3]) @ np.abs(inv[:3, :3])).max(), (what, i)
            assert np.linalg.det(R) > 0, (what, i)
            size = np.abs(fig[5:8]).max() + np.abs(fig[2:5]).sum() + np.abs(nxt[:3]).sum(axis=1).max() * np.abs(inv).max()
            assert np.abs(t - (fig[5:8] - R @ fig[2:5])).max() <= 64 * A.U * size, (what, i)
            continue
        update = A.step(fig)
        model = A.mul44(update, T)
        unit = A.condition_unit(fig[8:].reshape(3, 3))
        # nxt - model = dR T (+ dt = -dR mu_p in the last column): entry (a, j) moves by at most |dR| (sum_b |T_bj| + [j = 3] sum |mu_p|).
        # GROSS: nothing is taken off for the roundings of the plain product or of t — they come out of the same bar
        lever = np.abs(T[:3]).sum(axis=0) + np.array([0.0, 0.0, 0.0, np.abs(fig[2:5]).sum()])
        err = float((np.abs(nxt - model)[:3] / (unit * np.maximum(lever, 1e-300))).max())
        worst = max(worst, err)
        WORST[0] = max(WORST[0], err)
        assert err <= 4 * A.STEP_UNITS and np.array_equal(nxt[3], [0, 0, 0, 1]), (what, i, err)
    return worst


# ---- the iteration-by-iteration audit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_audit_at_the_workgroup_edges_of_the_source(ctx, n):
    source, target = A.small_case(700, n, seed=n)
    r = _refiner(ctx, target, n)
    res = r.refine(source)
    assert res.source_rows == n and res.target_rows == 700 and res.source_rows_left_out == res.target_rows_left_out == 0
    _audit(r, source, target, res, degenerate_ok=n < 3, what=f"n = {n}")
    r.close()


@pytest.mark.parametrize("m", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025])
def test_audit_at_the_edges_of_the_target(ctx, m):
    source, target = A.small_case(m, 300, seed=50 + m, spread=1.0 if m < 4 else 3.0)
    r = _refiner(ctx, target, 300)  # (capacity exactly reached on both sides)
    res = r.refine(source, max_iteration=6)
    _audit(r, source, target, res, degenerate_ok=m <= 3, what=f"m = {m}")
    r.close()


def test_empty_source_and_empty_target(ctx):
    source, target = A.small_case(100, 50)
    r = _refiner(ctx, target, 50)
    init = A.rigid(0.1, (1.0, 2.0, 3.0))
    res = r.refine(np.zeros((0, 3), np.float32), init=init)
    assert (res.fitness, res.inlier_rmse, res.iterations, res.converged, res.num_correspondences) == (0.0, 0.0, 0, False, 0)
    assert np.array_equal(_bits(res.transformation), _bits(init)) and len(res.correspondences) == 0
    hist_T, hist_S = r.history()
    assert hist_T.shape == (1, 4, 4) and np.array_equal(hist_T[0], init) and not hist_S.any()
    r.set_target(np.zeros((0, 3), np.float32))
    res = r.refine(source)
    assert (res.fitness, res.iterations, res.converged, res.target_rows) == (0.0, 1, True, 0) and (res.correspondences == -1).all()
    r.close()


def test_one_row_beyond_a_full_grid_of_workgroups(ctx):
    rng = np.random.default_rng(9)
    target = np.array([[0.0, 0.0, 0.0], [0.7, 0.1, 0.0], [0.0, 0.9, 0.3]], np.float32)
    source = (target[rng.integers(0, 3, GRID_ROWS + 1)] + rng.normal(0, 0.3, (GRID_ROWS + 1, 3))).astype(np.float32)
    source[-1] = (0.7, 0.1, 0.05)  # the row of the second pass of lane 0
    r = _refiner(ctx, target, GRID_ROWS + 1)
    res = r.refine(source, max_iteration=0)
    e = A.evaluate(np.eye(4), source, target, 1.0)
    assert np.array_equal(res.correspondences, e.corr) and res.correspondences[-1] == 1 and res.num_correspondences == e.count
    exact, tol = A.figures_exact(e, target, A.pivot(target))
    fig = r.history()[1][0]
    assert np.all(np.abs(fig - exact) <= tol)
    r.close()


# ---- free-running ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube", "lattice"])
def test_free_running_result_stays_within_the_summation_spread(ctx, name):
    """measured on an MI355X: max|T - model| 5.6e-16 (cube) and 5.1e-15 (lattice) against the bar 4 x SPREAD = 4.4e-14; 4
    iterations on both, as the model"""
    source, target, truth = A.convergent_cases()[name]
    model = A.free_run(name)
    r = _refiner(ctx, target, len(source))
    res = r.refine(source)
    diff = np.abs(res.transformation - model["T"]).max()
    print(name, "max|T - model| =", diff, "iterations", res.iterations)
    assert res.iterations == model["iterations"] and res.converged == model["converged"]
    assert diff <= 4 * A.SPREAD and np.abs(res.transformation - truth).max() < 1e-6
    assert np.array_equal(res.correspondences, model["corr"])
    # the same call twice: every output bit-equal
    hist = r.history()
    again = r.refine(source)
    assert np.array_equal(_bits(again.transformation), _bits(res.transformation)) and _bits(again.inlier_rmse) == _bits(res.inlier_rmse)
    assert np.array_equal(again.correspondences, res.correspondences)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(hist, r.history()))
    r.close()


def test_the_lattice_trap_runs_all_thirty_iterations(ctx):
    source, target, _ = A.trap_case()
    model = A.free_run("trap")
    r = _refiner(ctx, target, len(source), cell=0.8)
    res = r.refine(source)
    assert res.iterations == 30 and not res.converged and model["iterations"] == 30 and not model["converged"]
    assert len(r.history()[0]) == 31
    _audit(r, source, target, res, what="trap")
    print("worst gross step error of the audits so far, in condition units:", WORST[0])
    r.close()


def test_max_iteration_zero_and_one_and_no_correspondence(ctx):
    source, target = A.small_case(500, 200, seed=3)
    r = _refiner(ctx, target, 200)
    zero = r.refine(source, max_iteration=0)
    assert zero.iterations == 0 and not zero.converged and np.array_equal(zero.transformation, np.eye(4))
    one = r.refine(source, max_iteration=1)
    assert one.iterations == 1 and len(r.history()[0]) == 2
    _audit(r, source, target, one, what="one")
    far = r.refine(source + np.float32(100.0))
    assert (far.iterations, far.converged, far.fitness, far.inlier_rmse) == (1, True, 0.0, 0.0)
    assert np.array_equal(far.transformation, np.eye(4)) and (far.correspondences == -1).all()
    r.close()


# ---- edge clouds -------------------------------------------------------------------------------------------------------------------
def test_pairs_on_the_bound_and_ulps_either_side(ctx):
    """d2 is (dx dx + dy dy) + dz dz of the moved point: pairs along x whose d2 is r2 exactly and 1, 2, 3 ulp either side"""
    r2 = np.float64(1.0)
    shifts = [np.float64(1.0)]
    for k in (1, 2, 3):
        lo, hi = np.float64(1.0), np.float64(1.0)
        for _ in range(k):
            lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, 2.0)
        shifts += [lo, hi, np.sqrt(np.nextafter(r2, 0.0) - (k - 1) * 2.0 ** -53), np.sqrt(r2 + k * 2.0 ** -52)]
    # float32 rows cannot carry a float64 ulp: the translation of T does (dx = p'_x - q_x = T_03, d2 = dx dx)
    target = np.array([[0.0, 50.0 * k, 0.0] for k in range(len(shifts))], np.float32)
    source = target.copy()
    r = _refiner(ctx, target, 1)
    inside = 0
    for k, shift in enumerate(shifts):
        T = np.eye(4)
        T[0, 3] = shift
        e = A.evaluate(T, source[k:k + 1], target, 1.0)
        got = r.refine(source[k:k + 1], init=T, max_iteration=0)
        assert got.correspondences[0] == e.corr[0] == (k if shift * shift < r2 else -1), (k, shift)
        inside += shift * shift < r2
    assert inside >= 3 and len(shifts) - inside >= 4  # (d2 == r2 exactly is among them: no correspondence)
    r.close()


def test_ties_go_to_the_lowest_row(ctx):
    rng = np.random.default_rng(2)
    # 4 096 target rows in one cell: copies of four points; 400 points repeated 23 times
    four = rng.uniform(0.1, 0.9, (4, 3)).astype(np.float32)
    crowd = four[rng.integers(0, 4, 4096)]
    source = (four[rng.integers(0, 4, 300)] + rng.normal(0, 0.05, (300, 3))).astype(np.float32)
    r = _refiner(ctx, crowd, 300)
    res = r.refine(source, max_iteration=0)
    e = A.evaluate(np.eye(4), source, crowd, 1.0)
    assert np.array_equal(res.correspondences, e.corr) and set(res.correspondences) <= {int(np.flatnonzero((crowd == f).all(axis=1))[0]) for f in four}
    r.close()
    base = rng.uniform(-4, 4, (400, 3)).astype(np.float32)
    repeated = np.tile(base, (23, 1))
    source = (base[rng.integers(0, 400, 500)] + rng.normal(0, 0.1, (500, 3))).astype(np.float32)
    r = _refiner(ctx, repeated, 500)
    res = r.refine(source, max_iteration=3)
    assert (res.correspondences < 400).all()
    _audit(r, source, repeated, res, what="repeated")
    r.close()
    # a lattice query in the middle of four sites
    lattice = np.array([[i, j, 0] for i in range(4) for j in range(4)], np.float32)
    mid = np.array([[0.5, 0.5, 0], [1.5, 2.5, 0], [2.5, 0.5, 0.25]], np.float32)
    r = _refiner(ctx, lattice, 3)
    assert list(r.refine(mid, max_iteration=0).correspondences) == [0, 6, 8] == list(A.evaluate(np.eye(4), mid, lattice, 1.0).corr)
    r.close()


@pytest.mark.parametrize("cell,bound", [(1.0, 1.0), (0.4, 0.4), (0.4, 1.48), (0.1, 0.37)])
def test_queries_and_rows_on_cell_faces(ctx, cell, bound):
    """coordinates that are multiples of the cell edge, +-1 ulp: bound = the edge and bound = 3.7 edges"""
    rng = np.random.default_rng(4)
    k = rng.integers(-6, 7, (600, 3)).astype(np.float64) * np.float64(np.float32(cell))
    faces = k.astype(np.float32)
    for a, step in enumerate((np.inf, -np.inf, np.inf)):
        faces[a::6, a] = np.nextafter(faces[a::6, a], np.float32(step))
    target, source = faces[:350], faces[250:] + np.float32(0.0)
    source[::3] += (rng.normal(0, 0.5 * bound, (len(source[::3]), 3))).astype(np.float32)
    r = _refiner(ctx, target, len(source), cell=cell)
    e = A.evaluate(np.eye(4), source, target, bound)
    res = r.refine(source, max_distance=bound, max_iteration=0)
    assert np.array_equal(res.correspondences, e.corr), int((res.correspondences != e.corr).sum())
    assert 0 < e.count < len(source) or bound > cell
    T = A.rigid(0.0, (float(np.float32(cell)), 0.0, 0.0))  # moved by exactly one cell: still on the faces
    e = A.evaluate(T, source, target, bound)
    assert np.array_equal(r.refine(source, init=T, max_distance=bound, max_iteration=0).correspondences, e.corr)
    r.close()


def test_six_grid_and_bound_settings_give_identical_results(ctx):
    source, target, _ = A.cube_case(1500, 800, seed=8)
    runs = {}
    for bound in (1.0, 0.6):
        for cell in (1.0, 0.37, 0.05 if bound == 0.6 else 2.5):  # (0.05: above 7 cells, the exhaustive search)
            r = _refiner(ctx, target, len(source), cell=cell)
            res = r.refine(source, max_distance=bound)
            runs.setdefault(bound, []).append((res, r.history()))
            r.close()
    for bound, rs in runs.items():
        first, hist = rs[0]
        assert first.converged and first.iterations > 1
        for res, h in rs[1:]:
            assert np.array_equal(_bits(res.transformation), _bits(first.transformation)) and res.iterations == first.iterations
            assert np.array_equal(res.correspondences, first.correspondences) and _bits(res.inlier_rmse) == _bits(first.inlier_rmse)
            assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(hist, h))


def test_a_cloud_ten_kilometres_out_keeps_the_same_bars(ctx):
    source, target, truth = A.cube_case(1200, 700, seed=6, offset=(10000.0, -10000.0, 50.0))
    r = _refiner(ctx, target, len(source))
    res = r.refine(source)
    assert res.converged and res.fitness > 0.9
    worst = _audit(r, source, target, res, what="10 km")
    print("10 km: worst gross step error", worst, "; of the audits so far", WORST[0])
    r.close()


def test_non_finite_rows_in_each_cloud(ctx):
    source, target = A.small_case(300, 200, seed=12)
    source, target = source.copy(), target.copy()
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        target[10 + k, k] = v
        source[20 + k, k] = v
    target[5] = source[3]  # (a finite row next to them still matches)
    r = _refiner(ctx, target, 200)
    res = r.refine(source)
    assert res.source_rows == 200 and (res.correspondences[20:23] == -1).all() and not np.isin(res.correspondences, [10, 11, 12]).any()
    assert np.isfinite(res.transformation).all() and res.fitness <= 197 / 200
    _audit(r, source, target, res, what="non-finite")
    r.close()


def test_zero_rows_with_and_without_the_flag(ctx):
    source, target = A.small_case(300, 200, seed=13, spread=1.5)
    tiny = np.float32(1e-30)  # squares underflow to 0: the reference's norm is 0 as well
    source = np.concatenate([source[:100], np.zeros((7, 3), np.float32), [[tiny, -tiny, tiny]], [[1e-20, 0, 0]], source[100:]]).astype(np.float32)
    target = np.concatenate([np.zeros((5, 3), np.float32), target, [[tiny, 0, 0]], [[0, 0, -0.0]]]).astype(np.float32)
    r = _refiner(ctx, target, len(source), drop_target=True)
    res = r.refine(source, drop_zero_rows=True)
    assert (res.source_rows_left_out, res.target_rows_left_out, res.source_rows, res.target_rows) == (8, 7, 201, 300)
    assert (res.correspondences[100:108] == -1).all() and not np.isin(res.correspondences, [0, 1, 2, 3, 4, 305, 306]).any()
    _audit(r, source, target, res, drop_source=True, drop_target=True, what="dropped")
    r.set_target(target)  # without the flag the zero rows are rows: the lowest of the six at the origin wins
    res = r.refine(source, max_iteration=0)
    assert (res.source_rows_left_out, res.target_rows_left_out, res.source_rows) == (0, 0, 209)
    assert (res.correspondences[100:107] == 0).all()
    res = r.refine(source, max_iteration=2)
    _audit(r, source, target, res, what="kept")
    r.close()


def test_targets_outside_the_cell_range_are_reported_at_end(ctx):
    source, target = A.small_case(100, 50, seed=14)
    far = np.concatenate([target, [[3e6, 0, 0]]]).astype(np.float32)
    r = _refiner(ctx, far, 50, cell=1.0)
    r.launch(source)
    with pytest.raises(AssertionError, match="outside"):
        r.end()
    r.close()
    r = _refiner(ctx, far, 50, cell=4.0)  # the same rows within range of a wider cell
    assert np.array_equal(r.refine(source, max_iteration=0).correspondences, A.evaluate(np.eye(4), source, far, 1.0).corr)
    r.close()


# ---- other behaviour -----------------------------------------------------------------------------------------------------------
def test_host_and_device_rows_and_refusals(ctx, torch_cuda):
    torch = torch_cuda
    source, target = A.small_case(400, 300, seed=15)
    r = _refiner(ctx, target, 300)
    host = r.refine(source)
    hist = r.history()
    r2 = ctx.cloud_refiner(400, 300)  # two refiners on one context
    r2.set_target(torch.from_numpy(target).cuda())
    dev = r2.refine(torch.from_numpy(source).cuda())
    assert np.array_equal(_bits(dev.transformation), _bits(host.transformation)) and np.array_equal(dev.correspondences, host.correspondences)
    assert np.array_equal(r2.correspondences_device().cpu().numpy(), host.correspondences)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(hist, r2.history()))
    with pytest.raises(AssertionError, match="exceeds the capacity"):
        r.launch(np.zeros((301, 3), np.float32))
    with pytest.raises(AssertionError, match="exceeds the capacity"):
        r.set_target(np.zeros((401, 3), np.float32))
    with pytest.raises(AssertionError, match="nothing has been launched"):
        r.end()
    r.launch(source)
    with pytest.raises(AssertionError, match="in flight"):
        r.launch(source)
    with pytest.raises(AssertionError, match="in flight"):
        r.set_target(target)
    assert np.array_equal(_bits(r.end().transformation), _bits(host.transformation))
    for bad in (dict(max_distance=0.0), dict(max_distance=np.inf), dict(max_iteration=-1), dict(max_iteration=1001), dict(relative_rmse=-1.0),
                dict(init=np.full((4, 4), np.nan))):
        with pytest.raises(AssertionError, match="icp_refine_launch"):
            r.launch(source, **bad)
    fresh = ctx.cloud_refiner(10, 10)
    with pytest.raises(AssertionError, match="no target"):
        fresh.launch(source[:5])
    for bad in (dict(cell_size=0.0), dict(cell_size=np.nan), dict(max_target_rows=0), dict(max_source_rows=2 ** 31)):
        with pytest.raises(AssertionError, match="icp_refine_create"):
            ctx.cloud_refiner(**{**dict(max_target_rows=5, max_source_rows=5), **bad})
    assert np.array_equal(_bits(r.refine(source).transformation), _bits(host.transformation))
    # host rows are the refiner's once the call returns: overwritten at once, both clouds, the result stays
    t2, s2 = target.copy(), source.copy()
    r.set_target(t2)
    t2[:] = 7.0
    r.launch(s2)
    s2[:] = -7.0
    assert np.array_equal(_bits(r.end().transformation), _bits(host.transformation))
    for x in (r, r2, fresh):
        x.close()


def test_refinement_inside_a_launched_registration_leaves_it_bit_equal(torch_cuda):
    from pylidar_slam_amd.engine import IcpContext
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    scans, _ = make_sequence(SceneConfig(height=16, width=128), 2)
    source, target = A.small_case(400, 300, seed=16)
    results, refined = [], []
    for inside in (False, True):
        c = IcpContext(height=16, width=128, max_num_alignments=6, threshold_delta_pose=0.0)
        c.map_set(scans[0])
        r = c.cloud_refiner(400, 300)
        if not inside:
            r.set_target(target)
            refined.append(r.refine(source))
        c.register_launch(scans[1])
        if inside:
            r.set_target(target)
            refined.append(r.refine(source))
        results.append(c.register_end())
        c.close()
    plain, mixed = results
    u32 = lambda a: np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)  # noqa: E731
    assert plain.iterations == mixed.iterations == 6
    assert np.array_equal(u32(plain.pose), u32(mixed.pose)) and np.array_equal(u32(plain.losses), u32(mixed.losses))
    assert np.array_equal(u32(plain.dx), u32(mixed.dx))
    assert np.array_equal(_bits(refined[0].transformation), _bits(refined[1].transformation)) and refined[0].iterations > 0


def test_elevation_images_passed_directly_equal_their_rows(ctx):
    rng = np.random.default_rng(17)
    ground = np.concatenate([rng.uniform(-15, 15, (6000, 2)), rng.uniform(0.2, 3.0, (6000, 1))], axis=1).astype(np.float32)
    moved = (ground.astype(np.float64) @ A.rigid(0.01, (0.0, 0.0, 0.0))[:3, :3].T + np.array([0.1, 0.05, 0.0])).astype(np.float32)
    table = np.zeros((259, 3), np.uint8)
    images = []
    for rows in (ground, moved):
        img = ctx.elevation_image(100, 100, 0.4, 0.0, 5.0, False, table, 6000)
        img.build(rows)
        images.append(img)
    r = ctx.cloud_refiner(100 * 100, 100 * 100)
    r.set_target(images[0])
    direct = r.refine(images[1])
    pts = [img.points_3d.reshape(-1, 3) for img in images]
    r.set_target(pts[0], drop_zero_rows=True)
    rows = r.refine(pts[1], drop_zero_rows=True)
    assert direct.source_rows_left_out == int(A.zero_rows(pts[1]).sum()) > 0 and direct.target_rows_left_out == int(A.zero_rows(pts[0]).sum())
    assert np.array_equal(_bits(direct.transformation), _bits(rows.transformation)) and direct.iterations == rows.iterations > 0
    assert np.array_equal(direct.correspondences, rows.correspondences) and direct.fitness > 0.3
    for x in (r, *images):
        x.close()


def test_the_drop_in_compute_transform_returns_the_inverse_and_the_clouds(ctx):
    from pylidar_slam_amd import register

    class Config:
        icp_distance_threshold = 1.0

    class Owner:
        config = Config()

    class OnCtx:
        def __init__(self, owner):
            self.r = None

        def refine(self, candidate_pc, target_pc, initial_transform, max_distance):
            self.r = self.r or ctx.cloud_refiner(2048, 2048)
            self.r.set_target(target_pc)
            return self.r.refine(candidate_pc, init=initial_transform, max_distance=max_distance)

    source, target, truth = A.cube_case(1500, 900, seed=18)
    owner = Owner()
    init = A.rigid(0.04, (0.15, -0.1, 0.1))
    inv, a, b = register.compute_transform(owner, init.astype(np.float32), source, target, factory=OnCtx)
    assert a is source and b is target
    want = A.run(source, target, init=init.astype(np.float32).astype(np.float64))
    assert np.abs(np.linalg.inv(inv) - want["T"]).max() <= 4 * A.SPREAD and np.abs(np.linalg.inv(inv) - truth).max() < 1e-6
    owner._mi355x_refiner.r.close()
