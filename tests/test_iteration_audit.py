"""CPU (`-m "not gpu"`): the iteration audit of tests/iteration_audit.py on the oracle alone.  The evidence that the device
tests of tests/test_gpu_iteration_audit.py bite: the records of the oracle's own loop (kd-tree map, float64 sums) on a
16 x 256 scene pass all four checks, and each deliberately wrong copy of them fails the check meant for it; the case
inputs of the device tests exercise what they claim (census by the oracle's own values), and a float32 brute-force search
stays inside the neighbour cap on its own on those inputs."""
from dataclasses import replace

import numpy as np
import pytest
from scipy.spatial import cKDTree

import icp_oracle as O
import iteration_audit as A

F32, F64 = np.float32, np.float64
SCHEME, SIGMA, K = "huber", A.ROW_SIGMA, 4
INIT = O.build_pose_matrix(np.array([0.05, -0.03, 0.01, 0.002, -0.001, 0.005], F32))


@pytest.fixture(scope="module")
def clean():
    scan, model = A.tiny_scene()
    normals = A.oracle_normals(model)
    records = A.oracle_records(scan, model, normals, INIT, K, SCHEME, SIGMA, skip_null=True)
    assert len(records) == K
    return dict(scan=scan, model=model, normals=normals, records=records, tree=cKDTree(model.astype(F64)),
                nref=A.NormalReference(model))


def _audit(c, rec, pose_next=None, normals=None):
    return A.audit_iteration(rec, c["scan"], c["model"], c["normals"] if normals is None else normals, SCHEME, SIGMA,
                             "point_to_plane", True, pose_next, c["nref"], c["tree"])


def _rows(c, rec, ix=None):
    ok = A.valid_rows(c["scan"], True)
    p = A.transform_fma(c["scan"][ok], A.pose44(rec.pose12))
    ix = np.asarray(rec.ix if ix is None else ix)[ok]
    return p, c["model"][ix], c["normals"][ix]


def _with_step(rec, ref, **kw):
    return replace(rec, dx=ref["dx"], loss=ref["loss"], **kw)


def _failed(c, rec, **kw):
    with pytest.raises(A.AuditFailure) as e:
        _audit(c, rec, **kw)
    print(e.value)
    return tuple(sorted(set(e.value.checks)))


def test_clean_records_pass(clean):
    worst = A.Worst("oracle loop")
    A.audit_run("oracle", clean["records"], clean["scan"], clean["model"], clean["normals"], SCHEME, SIGMA, skip_null=True,
                init=INIT, worst=worst)
    print(worst)
    assert worst.n == K and worst.f["ddx"] == 0.0 and worst.f["mismatches"] == 0 and not worst.widened
    for cost in A.COSTS[1:]:
        recs = A.oracle_records(clean["scan"], clean["model"], None, INIT, 3, "neighborhood", 0.3, cost, True)
        A.audit_run("oracle p2p", recs, clean["scan"], clean["model"], None, "neighborhood", 0.3, cost, True, INIT)


def test_one_row_dropped_fails_the_row_count(clean):
    rec = clean["records"][1]
    p, q, n = _rows(clean, rec)
    wrong = _with_step(rec, A.reference_step(p[1:], q[1:], n[1:], SCHEME, SIGMA, "point_to_plane"), num_targets=len(p) - 1)
    assert "row count" in _failed(clean, wrong)


def _second_nearest(c, rec):
    """ix with 0.1 % of the valid rows moved to their second-nearest map point."""
    p, _, _ = _rows(c, rec)
    rows = np.linspace(0, len(p) - 1, int(np.ceil(1e-3 * len(p)))).astype(int)
    second = c["tree"].query(p[rows].astype(F64), k=2)[1][:, 1]
    ix = np.asarray(rec.ix).copy()
    ix[np.nonzero(A.valid_rows(c["scan"], True))[0][rows]] = second
    return ix


def test_second_nearest_neighbours_fail_neighbours_and_rows(clean):
    rec = clean["records"][1]
    ix = _second_nearest(clean, rec)
    ref = A.reference_step(*_rows(clean, rec, ix), SCHEME, SIGMA, "point_to_plane")
    # the sums used them and icp_last_neighbors reports them: the neighbour check
    assert _failed(clean, _with_step(rec, ref, ix=ix)) == ("neighbours",)
    # the sums used them, the reported neighbours are the nearest: the rows no longer follow from them
    assert _failed(clean, _with_step(rec, ref)) == ("rows",)


def test_rows_summed_twice_fail_the_rows(clean):
    rec = clean["records"][1]
    p, q, n = _rows(clean, rec)
    twice = [np.concatenate([a, a[256:384]]) for a in (p, q, n)]
    assert _failed(clean, _with_step(rec, A.reference_step(*twice, SCHEME, SIGMA, "point_to_plane"))) == ("rows",)


@pytest.mark.parametrize("other", ["least_square", "geman_mcclure", "cauchy"])
def test_another_scheme_fails_the_rows(clean, other):
    rec = clean["records"][1]
    sigma = SIGMA if other != "geman_mcclure" else 0.3
    assert _failed(clean, _with_step(rec, A.reference_step(*_rows(clean, rec), other, sigma, "point_to_plane"))) == ("rows",)


def test_flipped_huber_branch_fails_the_rows(clean):
    rec = clean["records"][1]
    p, q, n = _rows(clean, rec)
    res, jac = O.point_to_plane_rows(p, q, n)
    s, a = F32(SIGMA), np.abs(res)
    assert (a >= s).sum() > 0 and (a < s).sum() > 0
    cost = res * res  # the rows with |r| >= sigma take the quadratic branch too (those below sigma already do)
    w = (np.sqrt(cost.astype(F32)) / np.clip(a, F32(1e-4), None)).astype(F32)
    rw, jw = (res * w).astype(F32).astype(F64), (jac * w[:, None]).astype(F32).astype(F64)
    dx = -(np.linalg.inv(jw.T @ jw) @ (jw.T @ rw))
    wrong = replace(rec, dx=dx.astype(F32), loss=float((rw * rw).sum()))
    assert _failed(clean, wrong) == ("rows",)


def test_stale_neighbours_fail_the_neighbours(clean):
    """The neighbours of iteration k taken at the pose of iteration k - 1 (a cache that never refreshes), the sums consistent
    with them."""
    rec, prev = clean["records"][1], clean["records"][0]
    ok = A.valid_rows(clean["scan"], True)
    ix = np.full(len(ok), -1, np.int64)
    ix[ok] = clean["tree"].query(A.transform_fma(clean["scan"][ok], A.pose44(prev.pose12)).astype(F64))[1]
    assert (ix != rec.ix).mean() > A.MISMATCH_CAP
    wrong = _with_step(rec, A.reference_step(*_rows(clean, rec, ix), SCHEME, SIGMA, "point_to_plane"), ix=ix)
    assert _failed(clean, wrong) == ("neighbours",)


def test_masked_rows_with_a_neighbour_fail_the_neighbours(clean):
    scan = clean["scan"].copy()
    scan[100:130] = np.nan
    recs = A.oracle_records(scan, clean["model"], clean["normals"], INIT, 1, SCHEME, SIGMA, skip_null=True)
    c = dict(clean, scan=scan)
    _audit(c, recs[0])
    ix = recs[0].ix.copy()
    ix[110] = 5
    assert "neighbours" in _failed(c, replace(recs[0], ix=ix))


def test_pose_from_the_previous_step_fails_the_pose_chain(clean):
    rec, prev = clean["records"][1], clean["records"][0]
    _audit(clean, rec, pose_next=clean["records"][2].pose12)
    assert _failed(clean, rec, pose_next=A.chain_pose(prev.dx, A.pose44(rec.pose12))) == ("pose chain",)
    assert _failed(clean, rec, pose_next=A.pose44(rec.pose12)) == ("pose chain",)  # (no update at all)


def test_wrong_normals_fail_the_normals(clean):
    rec = clean["records"][1]
    nm = clean["normals"].copy()
    used = np.unique(rec.ix)
    nm[used[::50]] = nm[used[::50]] @ O.euler_to_mat(np.array([0.0, 0.01, 0.0], F32)).T  # 0.01 rad off
    ref = A.reference_step(*_rows(dict(clean, normals=nm), rec), SCHEME, SIGMA, "point_to_plane")
    assert _failed(clean, _with_step(rec, ref), normals=nm) == ("normals",)


def test_status_must_follow_the_oracle(clean):
    """A singular system (a plane over a plane) is an Invalid Jacobian for the oracle: a record that reports a solved step
    fails; fewer rows than unknowns likewise.  An exact subset of the map is the residual guard."""
    pmap, over = A.plane_case(32)
    nm = A.oracle_normals(pmap)
    eye = np.eye(4, dtype=F32)
    recs = A.oracle_records(over, pmap, nm, eye, 3, "geman_mcclure", 0.3)
    assert len(recs) == 1 and recs[0].status == A.ICP_ERR_INVALID_JACOBIAN
    A.audit_iteration(recs[0], over, pmap, nm, "geman_mcclure", 0.3, pose_next=eye)
    with pytest.raises(A.AuditFailure) as e:
        A.audit_iteration(replace(recs[0], status=A.ICP_OK, dx=np.full(6, 1e-3, F32)), over, pmap, nm, "geman_mcclure", 0.3)
    assert "rows" in e.value.checks
    scan, model = clean["scan"], clean["model"]
    for n in (1, 2, 5):
        recs = A.oracle_records(A.subset(scan, n), model, clean["normals"], eye, 2, "geman_mcclure", 0.3)
        assert len(recs) == 1 and recs[0].status == A.ICP_ERR_INVALID_JACOBIAN, n
    sub = np.ascontiguousarray(model[::3])
    recs = A.oracle_records(sub, model, clean["normals"], eye, 3, "geman_mcclure", 0.3)
    assert len(recs) == 1 and recs[0].converged and recs[0].loss == 0.0 and not recs[0].dx.any()
    A.audit_iteration(recs[0], sub, model, clean["normals"], "geman_mcclure", 0.3, pose_next=eye)
    with pytest.raises(A.AuditFailure):
        A.audit_iteration(replace(recs[0], converged=False), sub, model, clean["normals"], "geman_mcclure", 0.3)


def test_tolerance_rule_widens_from_the_reference_only(clean):
    """An ill-conditioned system (everything 10 km away): the allowed |ddx| is 4 x the spread between inv(H) g and the
    Cholesky solve in float64 — whatever the record under test holds."""
    shift = np.array([10000.0, -10000.0, 100.0])
    scan = (A.subset(clean["scan"], 512).astype(F64) + shift).astype(F32)
    model = (clean["model"].astype(F64) + shift).astype(F32)
    nm = A.oracle_normals(model)
    recs = A.oracle_records(scan, model, nm, np.eye(4, dtype=F32), 1, "geman_mcclure", 0.3)
    fig = A.audit_iteration(recs[0], scan, model, nm, "geman_mcclure", 0.3)
    print(f"10 km: reference spread {fig['spread']:.2e}, dx atol {fig['atol']:.2e}")
    assert fig["atol"] == max(A.STEP_ATOL, 4 * fig["spread"])
    off = replace(recs[0], dx=recs[0].dx + F32(10 * fig["atol"] + 1e-3 * np.abs(recs[0].dx).max()))
    with pytest.raises(A.AuditFailure):
        A.audit_iteration(off, scan, model, nm, "geman_mcclure", 0.3)


# ---- the case inputs of the device tests ------------------------------------------------------------------------------
def test_scheme_cases_exercise_both_branches():
    scan, model = A.small_scene()
    eye = np.eye(4, dtype=F32)
    assert set(A.SCHEME_SIGMA) == set(A.SCHEMES)
    for scheme, sigma in A.SCHEME_SIGMA.items():
        got = A.census(scan, model, eye, scheme, sigma)
        print(scheme, sigma, got)
        assert got["valid"] == scan.shape[0] and got["clamped"] > 0
        if scheme not in ("default", "least_square"):
            assert got["quadratic"] > 100 and got["linear"] > 100, (scheme, got)  # |r| < sigma and |r| >= sigma
    assert abs(A.SCHEME_SIGMA["huber"] - A.ROW_SIGMA) < 1e-12
    for scheme, sigma in A.P2P_CASES:  # the point-to-point residual is the distance to the neighbour
        got = A.census(scan, model, eye, scheme, sigma, cost="point_to_point")
        print("point to point", scheme, sigma, got)
        if scheme != "least_square":
            assert got["quadratic"] > 100 and got["linear"] > 100, (scheme, got)


def test_mask_and_far_cases_hold_what_they_claim():
    scan, model = A.small_scene()
    cases = A.mask_cases(scan)
    eye = np.eye(4, dtype=F32)
    blocks = A.census(cases["blocks"], model, eye, "geman_mcclure", 0.3)
    assert blocks["empty_128"] >= 5 and blocks["empty_512"] >= 1 and 0 < blocks["valid"] < scan.shape[0]
    assert np.isnan(cases["blocks"][2047]).all() and np.isnan(cases["blocks"][2048]).all()  # across a border
    one = A.census(cases["one_left"], model, eye, "geman_mcclure", 0.3)
    assert one["single_128"] >= 1 and one["single_512"] >= 1
    assert A.census(cases["all_masked"], model, eye, "geman_mcclure", 0.3)["valid"] == 0
    for c in cases.values():  # both kinds of masked rows
        assert np.isnan(c).any() and (c == 0).all(axis=1).any()
    frame, fmap = A.far_targets()
    far = A.census(frame, fmap, eye, "geman_mcclure", 0.3, skip_null=False)
    print("far", far)
    assert far["valid"] == 6000 and far["far"] >= 50 and far["empty_128"] > 0 and far["single_128"] > 0
    for n in A.SIZES:
        assert A.subset(scan, n).shape == (n, 3)


def _case_input(case):
    """(targets, map, initial pose) of every case input of tests/test_gpu_iteration_audit.py."""
    eye = np.eye(4, dtype=F32)
    kind, _, name = case.partition(":")
    if kind == "tiny":
        return A.tiny_scene() + (eye,)
    if kind == "small":  # sizes, schemes, both costs, live thresholds
        return A.small_scene() + (eye,)
    if kind == "mask":
        scan, model = A.small_scene()
        return A.mask_cases(scan)[name], model, O.build_pose_matrix(np.array([0.05, -0.02, 0.01, 0.001, -0.002, 0.004], F32))
    if kind == "far":
        return A.far_targets() + (eye,)
    if kind == "c2":
        return A.c2_inputs() + (eye,)
    if kind == "variant":
        targets, model, _ = A.full_size_variant(name)
        return targets[-70_000:], model, eye  # (rows_196608: the rows beyond the image)
    if kind == "map":
        return A.map_case(name)
    if kind == "pose":
        targets, init = A.pose_case(name)
        return targets, A.small_scene()[1], init
    if kind == "chained":
        scans, model = A.small_sequence()
        return scans[int(name)], model, eye
    if kind == "subset":
        model = A.small_scene()[1]
        return np.ascontiguousarray(model[::3]), model, eye
    assert kind == "plane"
    pmap, over = A.plane_case()
    return over, pmap, eye


CASE_INPUTS = (["tiny", "small", "mask:blocks", "mask:one_left", "far", "c2", "variant:rows_196608", "variant:no_carry"]
               + [f"map:{c}" for c in A.MAP_CASES] + [f"pose:{c}" for c in A.POSE_CASES]
               + [f"chained:{f}" for f in range(3)] + ["subset", "plane"])


@pytest.mark.parametrize("case", CASE_INPUTS)
def test_float32_brute_force_stays_inside_the_neighbour_cap(case):
    """The cap of the neighbour check (mismatches: squared-distance ties within 2e-6, at most 0.1 % of the rows) against a
    search that is exact in FLOAT32 — what the kernels compute in: it must leave room for that on every case input of the
    device tests, at the pose the first iteration runs with (a strided sample of at most ~4000 valid rows of each; the
    all-masked scan has none)."""
    targets, m, init = _case_input(case)
    t = targets[A.valid_rows(targets, True)]
    q = A.transform_fma(t[::max(1, len(t) // 4000)], np.asarray(init, F32))
    ix = A.brute_force_nn_f32(q, m)
    low = A.lowest_index_of_equal_points(m) if case == "map:duplicates" else None
    rec = A.IterationRecord(1, np.eye(4, dtype=F32)[:3], ix, 0.0, np.zeros(6, F32), len(q), 0, 1, False, np.eye(4, dtype=F32))
    fails, fig = A.check_neighbours(rec, q, m, False, low=low)
    if low is not None:
        fails += A.check_duplicates(rec, low)
    print(case, len(q), fig)
    assert not fails, fails
