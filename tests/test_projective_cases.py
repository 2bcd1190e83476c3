"""CPU (`-m "not gpu"`): the inputs and accounting helpers of tests/projective_cases.py on the oracle alone.  The evidence
that the GPU tests of tests/test_gpu_projective_edges.py bite: every helper passes the oracle's own output (or the CPU
stand-in of the device, `emulate_model`) and reports a deliberately wrong copy of it as unexplained; the caps the inputs
must respect are asserted on every generated case."""
import numpy as np
import pytest

import icp_oracle as O
import projective_cases as PC

F32, F64 = np.float32, np.float64


# ---- A. normal maps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.NORMAL_CASES, ids=PC.case_id)
def test_normal_case_respects_the_cap(case):
    source, h, w, content, ks, accounted = case
    ref = PC.NormalReference(PC.normal_case_input(source, h, w, content), ks)
    got = ref.account(ref.exact.astype(F32))
    assert len(got["unexplained"]) == 0, got["unexplained"][:5]
    assert got["null"] + got["determined"] + got["undetermined"] == h * w  # exactly one class per pixel
    if accounted:
        assert got["undetermined"] <= 0.01 * got["non_null"], (got["undetermined"], got["non_null"], ref.why)
        assert got["determined"] > 0
    if content in ("holes", "mild") and accounted and ks > 1 and h > 3:  # partial support, still three points
        _, _, cnt = PC.window_sums(ref.vmap, ks)
        full = PC.window_sums(np.ones_like(ref.vmap), ks)[2]
        assert ((cnt < full) & ref.determined).sum() > 0


def test_solve_spread_backs_the_tolerance():
    """C_SOLVE is 4 x the largest spread between the adjugate and np.linalg.solve in float64, in units of eps64 cond(A),
    over the accounted cases (largest: 3012, the 64 x 1024 map with holes at kernel size 3 — the adjugate is not backward
    stable: its error grows with cond(A)^2)."""
    worst = 0.0
    for source, h, w, content, ks, accounted in PC.NORMAL_CASES:
        if accounted:
            worst = max(worst, PC.NormalReference(PC.normal_case_input(source, h, w, content), ks).spread())
    print(f"largest spread {worst:.1f} eps64 cond(A); C_SOLVE {PC.C_SOLVE}")
    assert 4.0 * worst <= PC.C_SOLVE < 8.0 * worst, worst


def test_wrong_normal_maps_are_reported():
    v = PC.damage(PC.golden_vmap(0), "holes")
    ref = PC.NormalReference(v, 5)
    good = ref.exact.astype(F32)
    assert len(ref.account(good)["unexplained"]) == 0
    # column 0 zeroed (the golden's column 0 is occupied before the damage: use the dense map)
    dense = PC.NormalReference(PC.golden_vmap(0), 5)
    wrong = dense.exact.astype(F32)
    wrong[:, :, 0] = 0.0
    bad = dense.account(wrong)["unexplained"]
    assert len(bad) == int((dense.determined & ~dense.expect_zero)[:, 0].sum()) > 0 and (bad[:, 1] == 0).all()
    # a window that ignores the zero padding above the top row (replicates row 0 instead)
    padded = np.concatenate([dense.vmap[:, :1], dense.vmap], axis=1)
    wrong = O.compute_normal_map(padded, 5, dtype=F64)[:, 1:].astype(F32)
    bad = dense.account(wrong)["unexplained"]
    assert len(bad) > 0 and (bad[:, 0] <= 1).all(), bad[:5]
    # a non-unit vector, a NaN, a normal at a null pixel
    for poke in (lambda n: n.__setitem__((slice(None), 9, 9), n[:, 9, 9] * F32(1.001)),
                 lambda n: n.__setitem__((0, 9, 9), np.nan),
                 lambda n: n.__setitem__((slice(None), 4, 5), F32(0.5))):
        wrong = good.copy()
        poke(wrong)
        assert len(ref.account(wrong)["unexplained"]) == 1
    assert ref.null[4, 5] and ref.determined[9, 9]


# ---- C. window and model ---------------------------------------------------------------------------------------------
def _run_window(h, w, lms, ks, source, tamper=None):
    calls = PC.window_sequence(h, w, lms, source)
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=lms, normals_kernel_size=ks,
                                 normals_dtype=F64)
    stock = O.ProjectiveLocalMapOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=lms, normals_kernel_size=ks,
                                       normals_dtype=F64)
    total = dict(occupied=0, equal=0, explained=0, unexplained=[])
    inserted = 0
    for n, (pose, v) in enumerate(calls):
        orc.update(pose, v)
        stock.update(pose, v)
        inserted += v is not None
        scale = max(float(np.abs(p).max()) for p in orc.poses + stock.poses)
        drift = max(float(np.abs(a - b).max()) for a, b in zip(orc.poses, stock.poses))
        assert drift <= PC.pose_drift_bound(n + 1, scale), (n, drift)
        mv, mn = PC.emulate_model(orc.vmaps, orc.nmaps, orc.poses, h, w)
        if tamper is not None:
            mv, mn = tamper(n, orc, mv, mn)
        got = PC.account_model(mv, mn, orc.vmaps, orc.nmaps, orc.poses, h, w)
        for key in ("occupied", "equal", "explained"):
            total[key] += got[key]
        total["unexplained"] += [(n,) + u for u in got["unexplained"]]
    assert inserted >= 2 * (lms + 1) + 1  # every storage slot recycled twice
    return total


@pytest.mark.parametrize("h,w,lms,ks,source", [(32, 256, 2, 3, "golden"), (32, 256, 4, 7, "golden"), (17, 33, 1, 7, "scan"),
                                               (64, 1024, 1, 5, "scan")])
def test_float64_projection_stays_inside_the_cap(h, w, lms, ks, source):
    """The float32 oracle against a float64 projection of the same transformed points, over the whole part-C sequence:
    nothing unexplained, explained pixels far below the 0.5 % cap (measured: 2e-5 .. 4e-5 of the occupied ones)."""
    total = _run_window(h, w, lms, ks, source)
    print(h, w, lms, {k: (v if k != "unexplained" else len(v)) for k, v in total.items()})
    assert total["unexplained"] == []
    assert total["explained"] <= 0.005 * total["occupied"]
    assert total["equal"] > 0.99 * total["occupied"]


def test_wrong_models_are_reported():
    h, w, lms = 32, 256, 2
    # one stale pixel: a vertex of an evicted map at a pixel the layer's own map leaves empty
    evicted = {}

    def stale(n, orc, mv, mn):
        empty = np.argwhere(np.abs(mv[0]).max(axis=0) == 0)
        if n == 8 and len(empty):
            r, c = empty[len(empty) // 2]
            mv, mn = mv.copy(), mn.copy()
            mv[0][:, r, c] = PC.golden_vmap(5)[:, 3, 7]
            mn[0][:, r, c] = np.array([0.0, 0.0, 1.0], F32)
            evicted["at"] = (n, 0, int(r), int(c))
        return mv, mn
    total = _run_window(h, w, lms, 5, "golden", tamper=stale)
    assert [u[:4] for u in total["unexplained"]] == [evicted["at"]], total["unexplained"]
    # a normal that is not the winner's: one pixel of one layer
    def wrong_normal(n, orc, mv, mn):
        if n == 5:
            mn = mn.copy()
            r, c = np.argwhere(np.abs(mv[-1]).max(axis=0) > 0)[100]
            mn[-1][:, r, c] = np.roll(mn[-1][:, r, c], 1) + F32(0.25)
        return mv, mn
    assert len(_run_window(h, w, lms, 5, "golden", tamper=wrong_normal)["unexplained"]) == 1
    # a z-buffer that keeps the farther of two points
    def farther(n, orc, mv, mn):
        return PC.emulate_model(orc.vmaps, orc.nmaps, orc.poses, h, w, keep_farther=True)
    total = _run_window(h, w, lms, 5, "golden", tamper=farther)
    assert len(total["unexplained"]) > 100


def test_recorded_reference_model_against_the_oracle():
    """`ls_model_vmap`, the reference's own model after its `ls` run, against the oracle's model of the same updates under
    the library's pose composition: nothing unexplained."""
    import os
    g = np.load(os.path.join(PC.GOLDEN, "projective.npz"))
    h, w = (int(x) for x in g["hw"])
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=4)
    calls = PC.recorded_run_updates(g)
    for pose, v in calls:
        orc.update(pose, v)
    assert len(orc.vmaps) == g["ls_model_vmap"].shape[0] == 4
    scale = max(float(np.abs(p).max()) for p in orc.poses)
    got = PC.account_recorded(g["ls_model_vmap"], orc.vmaps, orc.poses, h, w, PC.pose_drift_bound(len(calls), scale))
    print({k: (v if isinstance(v, int) else len(v)) for k, v in got.items()})
    assert got["unexplained"] == [], got["unexplained"][:8]
    assert got["explained"] <= 0.005 * got["occupied"] and got["equal"] > 0.99 * got["occupied"]
    wrong = g["ls_model_vmap"].copy()
    wrong[1][:, 10, 10] = wrong[0][:, 20, 20]
    assert len(PC.account_recorded(wrong, orc.vmaps, orc.poses, h, w, 1e-5)["unexplained"]) == 1


# ---- D. association --------------------------------------------------------------------------------------------------
def _association_setup(h=32, w=256, lms=2):
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=lms, normals_dtype=F64)
    for pose, v in PC.window_sequence(h, w, lms, "golden")[:5]:
        orc.update(pose, v)
    mv, mn = PC.emulate_model(orc.vmaps, orc.nmaps, orc.poses, h, w)
    pts = PC.association_targets(h, w, PC.window_poses(1, yaw=0.05, step=0.4)[0])
    finite = np.where(np.isfinite(pts).all(axis=1)[:, None], pts, 0).astype(F32)
    _, index = O.build_projection_map(finite, h, w, PC.UP_FOV, PC.DOWN_FOV, return_index=True)
    return orc, mv, mn, pts, index


def test_association_accounting_on_the_oracle():
    orc, mv, mn, pts, index = _association_setup()
    rows = PC.expected_association(mv, mn, pts, index)[:3]
    finite = np.where(np.isfinite(pts).all(axis=1)[:, None], pts, 0).astype(F32)
    model = PC.account_model(mv, mn, orc.vmaps, orc.nmaps, orc.poses, 32, 256)
    got = PC.account_association(rows, mv, mn, pts, index, orc.nearest_neighbor_search(finite), model["explained_pixels"])
    assert got["unexplained"] == [] and got["rows"] == got["expected_rows"] > 1000, got
    assert got["explained"] <= 0.005 * got["rows"]
    # dropped rows, a row too many, swapped order
    for wrong in ([r[:-1] for r in rows], [np.concatenate([r, r[:1]]) for r in rows], [r[::-1] for r in rows]):
        assert PC.account_association(wrong, mv, mn, pts, index)["unexplained"] != []
    # an oracle that matches other targets: reported
    fewer = [r[5:] for r in orc.nearest_neighbor_search(finite)]
    assert len(PC.account_association(rows, mv, mn, pts, index, fewer)["unexplained"]) >= 3


def test_second_layer_on_a_tie_is_reported():
    h, w = 5, 7
    v = (np.round(PC.scan_vmap(h, w) * 64) / 64).astype(F32)  # multiples of 1/64: the offsets below are exact
    pts = O.vertex_map_to_points(v)
    _, index = O.build_projection_map(pts, h, w, PC.UP_FOV, PC.DOWN_FOV, return_index=True)
    assert (index >= 0).sum() > 20
    off = np.array([0.25, 0.0, 0.0], F32).reshape(3, 1, 1)
    tv = O.build_projection_map(pts, h, w, PC.UP_FOV, PC.DOWN_FOV)
    mv = np.stack([tv + off, tv - off, tv + 2 * off]).astype(F32) * (np.abs(tv).max(axis=0) > 0)
    mn = np.stack([np.full_like(tv, 0.1), np.full_like(tv, 0.2), np.full_like(tv, 0.3)])
    rows = PC.expected_association(mv, mn, pts, index)
    assert (rows[1] == F32(0.1)).all()  # exact tie between layers 0 and 1: the first
    assert PC.account_association(rows[:3], mv, mn, pts, index)["unexplained"] == []
    second = (rows[0] - 2 * off.reshape(1, 3), np.full_like(rows[1], 0.2), rows[2])
    bad = PC.account_association(second, mv, mn, pts, index)["unexplained"]
    assert {b[0] for b in bad} == {"neighbour", "normal"}


# ---- E. one iteration's rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,source", [(17, 33, "scan"), (32, 256, "golden")])
def test_iteration_inputs_exercise_every_branch(h, w, source):
    calls, scan, inits = PC.iteration_case(h, w, source)
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=4, normals_dtype=F64)
    for pose, v in calls:
        orc.update(pose, v)
    mv, mn = PC.emulate_model(orc.vmaps, orc.nmaps, orc.poses, h, w)
    for init in inits:
        for skip_null in (False, True):
            targets, planted = PC.iteration_targets(mv, init, scan, skip_null)
            assert planted > 0
            p = PC.moved_targets(targets, init, skip_null)
            _, index = O.build_projection_map(p, h, w, PC.UP_FOV, PC.DOWN_FOV, return_index=True)
            rows = PC.expected_association(mv, mn, p, index)[:3]
            census = PC.residual_census(rows, PC.ROW_SIGMA)
            assert min(census.values()) > 0, census


def test_wrong_huber_branch_for_one_row_is_reported():
    h, w = 17, 33
    calls, scan, inits = PC.iteration_case(h, w, "scan")
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=4, normals_dtype=F64)
    for pose, v in calls:
        orc.update(pose, v)
    mv, mn = PC.emulate_model(orc.vmaps, orc.nmaps, orc.poses, h, w)
    targets, _ = PC.iteration_targets(mv, inits[1], scan, True)
    p = PC.moved_targets(targets, inits[1], True)
    _, index = O.build_projection_map(p, h, w, PC.UP_FOV, PC.DOWN_FOV, return_index=True)
    nb, nn, tg = PC.expected_association(mv, mn, p, index)[:3]
    ref = PC.host_step((nb, nn, tg), "huber", PC.ROW_SIGMA)

    def step(weights):
        res, jac = O.point_to_plane_rows(tg, nb, nn)
        r = (res * weights).astype(F32).astype(F64)
        j = (jac * weights[:, None]).astype(F32).astype(F64)
        return (-np.linalg.solve(j.T @ j, j.T @ r)).astype(F32), float((r * r).sum()), len(r)
    res, _ = O.point_to_plane_rows(tg, nb, nn)
    wts = O.ls_weights("huber", PC.ROW_SIGMA, res)
    PC.assert_step(*step(wts), ref)
    linear = int(np.argmax(np.abs(res)))
    assert abs(res[linear]) >= PC.ROW_SIGMA
    wrong = wts.copy()
    wrong[linear] = 1.0  # the quadratic branch for a row of the linear one
    with pytest.raises(AssertionError):
        PC.assert_step(*step(wrong), ref)
    with pytest.raises(AssertionError):  # a row too few: the count is held exactly
        PC.assert_step(ref[0], ref[1], ref[2] - 1, ref)
