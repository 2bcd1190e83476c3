"""CPU (`-m "not gpu"`): the alignment audit of tests/alignment_audit.py on the oracle alone.  The evidence that the device
tests of tests/test_gpu_alignment_audit.py bite: the oracle's own output passes check_seam / check_procrustes on EVERY case
those tests run, the model reproduces the reference's recorded results, each deliberately wrong copy of the oracle's output
fails by the kinds meant for it and by no other, the inputs exercise what they claim (determinants clear of the guard, the
census of row kinds, which cases the reference leaves undetermined), and every measured spread behind a tolerance constant
is re-measured here."""
import os

import numpy as np
import pytest

import alignment_audit as AA
import icp_oracle as O
import iteration_audit as A

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BIG = AA.STRIDE + 257  # one full stride and a 257-row second turn


def _kinds(out, model):
    fails, _ = AA.check_seam(out, model)
    for k, w in fails:
        print(f"  [{k}] {w}")
    return tuple(sorted({k for k, _ in fails}))


# ----------------------------------------------------------------------------------------------------------------------
# the oracle's output passes, on every case of the device tests
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["sweep", "content", "offsets", "nan", "x0"])
def test_oracle_passes_every_seam_case(family):
    worst = AA.SeamWorst(f"oracle, {family}")
    undetermined = []
    for label, cost, scheme, sigma, ref, tgt, nrm, x0 in AA.seam_cases((family,)):
        model = AA.seam_step(cost, ref, tgt, nrm, x0, scheme, sigma)
        out = AA.oracle_seam(cost, ref, tgt, nrm, x0, scheme, sigma)
        fig = AA.assert_seam(out, model, label)
        worst.add(fig, label)
        if fig["step_undetermined"] or fig["status_undetermined"]:
            undetermined.append(label)
        n = len(ref)
        if x0 is None and n <= 4097 and family != "nan":  # the model IS iteration_audit's at x0 = 0, to the bit
            r = A.reference_step(tgt, ref, nrm, scheme, sigma, cost)
            assert r["status"] == model["ref"]["status"] and r["stopped"] == model["ref"]["stopped"], label
            assert np.array_equal(r["dx"], model["ref"]["dx"]) and abs(r["loss"] - model["ref"]["loss"]) <= 1e-6 * r["loss"], label
            rw, jw, _ = A.weighted_rows(tgt, ref, nrm, scheme, sigma, cost)
            assert np.array_equal(rw, model["rows"]["rw"]) and np.array_equal(jw, model["rows"]["jw"]), label
        if family == "nan":
            assert out["status"] == AA.ICP_ERR_INVALID_JACOBIAN and np.isnan(model["rows"]["rw2"]).sum() == 1, label
    print(worst)
    # the reference leaves the STEP open at pitch = pi / 2 (gimbal lock) and nowhere else; the status nowhere
    assert all("pitch_half_pi" in u for u in undetermined), undetermined
    if family == "x0":
        assert len(undetermined) == len(AA.X0_SIZES) * len(AA.X0_SCHEMES)


def test_robust_weights_are_the_oracles():
    rng = np.random.default_rng(1)
    res = np.concatenate([rng.normal(0, 0.05, 5000), [0.0, 1e-5, -3e-5, 1e-4, 0.05, -0.05]]).astype(F32)
    p, q = rng.normal(size=(len(res), 3)).astype(F32), rng.normal(size=(len(res), 3)).astype(F32)
    d = p - q
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    for scheme in AA.SCHEMES:
        w = AA.robust_weights(scheme, AA.SIGMA[scheme], res, d2)
        assert np.array_equal(w, np.broadcast_to(O.ls_weights(scheme, AA.SIGMA[scheme], res, p, q), w.shape)), scheme


def test_x0_rows_are_the_oracles():
    """seam_rows at x0 != 0 against O.point_to_point_step (numpy matmul for the transform: equal within the float32
    rounding of the three-term sums, and the step within the bars of test_point_to_point_alignment)."""
    for name in ("small", "yaw_3rad", "translation"):
        ref, tgt, x0 = AA.x0_case(name, 257)
        for scheme, sigma in AA.X0_SCHEMES:
            model = AA.seam_step("point_to_point", ref, tgt, None, x0, scheme, sigma)
            _, params, loss = O.point_to_point_step(tgt, ref, x0, scheme, sigma, accumulate=F64)
            np.testing.assert_allclose(model["params"], params, rtol=2e-5, atol=2e-6)
            np.testing.assert_allclose(model["ref"]["loss"], loss, rtol=1e-5)


def test_sweep_inputs_stay_clear_of_the_guard():
    """Every size from 6 up: status determined, both float64 determinants outside [1e-8, 1e-6], no residual guard; 1, 2 and
    5 rows: singular by both formulations (the named guard cases)."""
    for cost, scheme, n in AA.sweep_cases():
        ref, tgt, nrm = AA.sweep_case(cost, n)
        st = AA.seam_step(cost, ref, tgt, nrm, None, scheme, AA.sweep_sigma(scheme, n))["ref"]
        assert not st["stopped"], (cost, scheme, n)
        if n in AA.GUARD_SIZES:  # (a rank-deficient H: the LU determinant is rounding noise, up to 2.5e-8 here)
            assert st["status"] == AA.ICP_ERR_INVALID_JACOBIAN and all(abs(d) < 1e-7 / 3 for d in st["det"]), (cost, scheme, n, st["det"])
        else:
            assert st["status"] == AA.ICP_OK and all(abs(d) > 1e-6 for d in st["det"]), (cost, scheme, n, st["det"])
            assert max(st["spread"], st["order_spread"]) * AA.MARGIN < AA.STEP_ATOL, (cost, scheme, n)  # no case widened


def test_census_of_the_row_content_cases():
    for cost in AA.COSTS:
        ref, tgt, nrm = AA.content_case(cost)
        c = AA.row_census(cost, ref, tgt, nrm)
        print(cost, c)
        assert min(c["quadratic"], c["linear"], c["clamped"], c["zero"], c["coincident"]) >= 1000, c
        if cost == "point_to_plane":
            assert c["zero_normals"] >= 1000 and c["non_unit_normals"] >= 1000, c
        rows = AA.seam_rows(cost, ref, tgt, nrm, None, "huber", AA.SIGMA["huber"])
        same = (ref == tgt).all(axis=1)
        assert not rows["rw2"][same].any()  # r = 0 at both seams
        if cost == "point_to_point":  # p == q: r = 0, J = 0, the weight 0 / 1e-4 = 0
            assert not rows["r"][same].any() and not rows["jw"][same].any() and np.isfinite(rows["jw"]).all()
        for name, shift in AA.OFFSETS.items():
            r2, t2, n2 = AA.content_case(cost, 4097, shift)
            c2 = AA.row_census(cost, r2, t2, n2)
            assert c2["zero"] >= 100 and c2["coincident"] >= 100 and abs(r2[:, 0]).min() > 0.9 * abs(shift[0]), (name, c2)
    ref, tgt, x0 = AA.x0_guard_case()
    st = AA.seam_step("point_to_point", ref, tgt, None, x0, "huber", 0.1)
    assert st["ref"]["stopped"] and not st["rows"]["r"].any() and np.array_equal(st["params"], x0)


def test_tolerance_constants():
    """The spreads behind TRANSCENDENTAL_SPREAD, re-measured over every case of the device tests that runs exp /
    neighborhood / cauchy: the largest relative difference of (w r)^2 between expf / logf in float32 and in float64 rounded
    to float32.  The two evaluations DO differ (the bar is no bit comparison in disguise)."""
    measured = {k: 0.0 for k in AA.TRANSCENDENTAL_SPREAD}
    for label, cost, scheme, sigma, ref, tgt, nrm, x0 in AA.seam_cases():
        if scheme in AA.IEEE_SCHEMES:
            continue
        a = AA.seam_rows(cost, ref, tgt, nrm, x0, scheme, sigma)["rw2"].astype(F64)
        b = AA.seam_rows(cost, ref, tgt, nrm, x0, scheme, sigma, transcendental="f64")["rw2"].astype(F64)
        ok = np.isfinite(a) & (np.abs(a) >= float(np.finfo(F32).tiny))  # (a subnormal result carries no relative precision)
        assert np.array_equal(a[~ok], b[~ok], equal_nan=True) or np.abs(a[~ok] - b[~ok]).max() <= 2e-45 * 8, label
        measured[scheme] = max(measured[scheme], float((np.abs(a - b)[ok] / np.abs(a)[ok]).max()))
    print("measured spreads", measured)
    for scheme, spread in AA.TRANSCENDENTAL_SPREAD.items():
        assert 0.0 < measured[scheme] <= spread, (scheme, measured[scheme], spread)
        assert AA.TRANSCENDENTAL_BOUND[scheme] == AA.MARGIN * spread


def test_trigonometry_spread_at_x0():
    """The bars of the x0 != 0 cases: cos / sin in float32, in float64 rounded, and the oracle's own matrices.  Where the
    three agree to the bit the bit-exact rule applies; otherwise the spread stays far inside the project's 1e-5 loss bar."""
    for name in AA.X0_CASES:
        ref, tgt, x0 = AA.x0_case(name, 257)
        model = AA.seam_step("point_to_point", ref, tgt, None, x0, "least_square", 0.5)
        same = all(np.array_equal(u, v) for t in ("f64", "oracle")
                   for u, v in zip(AA.linearisation(x0, "f32"), AA.linearisation(x0, t)))
        print(name, "bit-exact" if same else f"row bar {model['row_tol'].max():.3e}", "trig_exact", model["trig_exact"])
        assert same == model["trig_exact"] and (model["row_tol"] is None) == same
        if not same:
            assert model["row_tol"].max() <= 1e-5 * np.abs(model["rows"]["rw2"]).max()
        if not np.any(x0[3:] != 0):
            assert same


# ----------------------------------------------------------------------------------------------------------------------
# the reference's recorded results
# ----------------------------------------------------------------------------------------------------------------------
def test_model_reproduces_the_reference():
    g = np.load(os.path.join(GOLDEN, "alignment.npz"))
    for name in ("ls", "huber", "nbh", "gm_svd", "ls_svd"):
        scheme, sigma, svd = g[f"{name}_cfg"]
        x0 = None
        if int(svd):  # alignment.py:170-171: weighted_procrustes(ref_points, tgt_points) — in that argument order
            x0 = O.from_pose_matrix(AA.procrustes_model(g["ref"], g["tgt"])["pose"].astype(F32))
        m = AA.seam_step("point_to_point", g["ref"], g["tgt"], None, x0, str(scheme), float(sigma))
        np.testing.assert_allclose(m["params"], g[f"{name}_params"], rtol=2e-4, atol=2e-5)  # test_point_to_point_alignment
        np.testing.assert_allclose(m["pose"], g[f"{name}_pose"], atol=5e-5)
        np.testing.assert_allclose(m["ref"]["loss"], float(g[f"{name}_loss"]), rtol=1e-4)
    np.testing.assert_allclose(AA.procrustes_model(g["tgt"], g["ref"])["pose"], g["procrustes_np"], atol=2e-6)
    np.testing.assert_allclose(AA.procrustes_model(g["tgt"], g["ref"], g["weights"])["pose"], g["procrustes_np_weighted"],
                               atol=2e-6)  # (the bars of test_weighted_procrustes)
    np.testing.assert_allclose(AA.procrustes_model(g["flat_tgt"], g["flat_ref"])["pose"], g["procrustes_flat"], atol=2e-6)
    c = np.load(os.path.join(GOLDEN, "components.npz"))
    for scheme in AA.SCHEMES:
        sigma = float(c[f"gn_{scheme}_sigma"])
        m = AA.seam_step("point_to_plane", c["nn_points"], c["nn_queries"], c["nn_normals"], None, scheme, sigma)
        np.testing.assert_allclose(m["params"], c[f"gn_{scheme}_dx"], atol=2e-5, rtol=1e-4)  # test_gauss_newton_step
        assert abs(m["ref"]["loss"] - float(c[f"gn_{scheme}_loss"])) <= 1e-4 * abs(float(c[f"gn_{scheme}_loss"]))
        np.testing.assert_allclose(m["pose"], c[f"gn_{scheme}_mat"], atol=2e-5)


# ----------------------------------------------------------------------------------------------------------------------
# wrong copies
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """The huber point-to-plane call at 65 536 + 257 rows and its model."""
    ref, tgt, nrm = AA.sweep_case("point_to_plane", BIG)
    model = AA.seam_step("point_to_plane", ref, tgt, nrm, None, "huber", AA.SIGMA["huber"])
    assert _kinds(AA.output_from_rows(model["rows"]), model) == ()
    return dict(ref=ref, tgt=tgt, nrm=nrm, model=model, rows=model["rows"])


@pytest.fixture(scope="module")
def at_x0():
    """The neighborhood point-to-point call at yaw 3 rad, 257 rows."""
    ref, tgt, x0 = AA.x0_case("yaw_3rad", 257)
    model = AA.seam_step("point_to_point", ref, tgt, None, x0, "neighborhood", 30.0)
    assert _kinds(AA.output_from_rows(model["rows"], x0), model) == ()
    return dict(ref=ref, tgt=tgt, x0=x0, model=model)


@pytest.mark.parametrize("name,keep", [("last row", slice(0, BIG - 1)),
                                       ("one workgroup", np.r_[0:256, 512:BIG]),
                                       ("the stride's second turn", slice(0, AA.STRIDE))])
def test_dropped_rows_fail_the_row_count(big, name, keep):
    """... and where the dropped rows are still COUNTED, the sums and the residual vector (their slots never written)."""
    wrong = AA.output_from_rows(AA.take_rows(big["rows"], keep))
    assert _kinds(wrong, big["model"]) == ("row count",)
    stale = np.zeros(BIG, F32)
    stale[keep] = big["rows"]["rw2"][keep]
    counted = AA.output_from_rows(AA.take_rows(big["rows"], keep), count=BIG, residuals=stale)
    kinds = _kinds(counted, big["model"])
    assert {"normal equations", "residual vector"} <= set(kinds) <= {"normal equations", "residual vector", "step"}, kinds


def test_swapped_jacobian_columns_fail_the_sums_and_the_step(big):
    rows = dict(big["rows"])
    rows["jw"] = rows["jw"][:, [0, 1, 2, 4, 3, 5]]
    assert _kinds(AA.output_from_rows(rows), big["model"]) == ("normal equations", "step")


def test_weight_without_its_clamp_fails():
    ref, tgt, nrm = AA.content_case("point_to_plane")
    model = AA.seam_step("point_to_plane", ref, tgt, nrm, None, "huber", AA.SIGMA["huber"])
    wrong = AA.seam_rows("point_to_plane", ref, tgt, nrm, None, "huber", AA.SIGMA["huber"], clamp=False)
    with np.errstate(all="ignore"):  # (0 / 0 at the r == 0 rows: NaN, as the unclamped weight gives)
        kinds = _kinds(AA.output_from_rows(wrong), model)
    assert {"normal equations", "residual vector"} <= set(kinds), kinds
    # ... on the rows the clamp leaves alone it changes nothing
    ref, tgt, nrm = AA.sweep_case("point_to_plane", 257)
    assert np.abs(AA.seam_rows("point_to_plane", ref, tgt, nrm, None, "huber", 0.05)["r"]).min() >= 1e-4
    model = AA.seam_step("point_to_plane", ref, tgt, nrm, None, "huber", 0.05)
    assert _kinds(AA.output_from_rows(AA.seam_rows("point_to_plane", ref, tgt, nrm, None, "huber", 0.05, clamp=False)), model) == ()


@pytest.mark.parametrize("name", ["r^2 for (w r)^2", "rotated by one row", "one ulp"])
def test_wrong_residual_vectors_fail_the_residual_vector_alone(big, name):
    rw2 = big["rows"]["rw2"]
    if name == "r^2 for (w r)^2":
        wrong = big["rows"]["r2"].copy()
    elif name == "rotated by one row":
        wrong = np.roll(rw2, 1)
    else:
        wrong = rw2.copy()
        wrong[AA.STRIDE + 3] = np.nextafter(wrong[AA.STRIDE + 3], F32(np.inf))
        assert abs(float(wrong.astype(F64).sum()) - float(rw2.astype(F64).sum())) < 1e-9 * float(rw2.astype(F64).sum())
    assert _kinds(AA.output_from_rows(big["rows"], residuals=wrong), big["model"]) == ("residual vector",)


def test_x0_ignored_in_the_rows_fails(at_x0):
    c = at_x0
    wrong = AA.seam_rows("point_to_point", c["ref"], c["tgt"], None, c["x0"], "neighborhood", 30.0, use_x0=False)
    kinds = _kinds(AA.output_from_rows(wrong, c["x0"]), c["model"])
    assert kinds == ("normal equations", "residual vector", "step"), kinds


def test_x0_not_added_to_params_fails_the_params(at_x0):
    c = at_x0
    assert _kinds(AA.output_from_rows(c["model"]["rows"], c["x0"], add_x0=False), c["model"]) == ("params",)


def test_neighborhood_on_the_transformed_target_fails(at_x0):
    c = at_x0
    wrong = AA.seam_rows("point_to_point", c["ref"], c["tgt"], None, c["x0"], "neighborhood", 30.0, neighborhood_on="moved")
    kinds = _kinds(AA.output_from_rows(wrong, c["x0"]), c["model"])
    assert {"normal equations", "residual vector"} <= set(kinds) <= {"normal equations", "residual vector", "step"}, kinds


def test_float32_sums_fail_the_sums(big):
    kinds = _kinds(AA.output_from_rows(big["rows"], dtype=F32), big["model"])
    assert "normal equations" in kinds and set(kinds) <= {"normal equations", "step"}, kinds


# ----------------------------------------------------------------------------------------------------------------------
# Procrustes
# ----------------------------------------------------------------------------------------------------------------------
def _pkinds(pose, model):
    fails, _ = AA.check_procrustes(pose, model)
    for k, w in fails:
        print(f"  [{k}] {w}")
    return tuple(sorted({k for k, _ in fails}))


def test_oracle_passes_every_procrustes_case():
    undetermined, refused = [], []
    for label, tgt, ref, w in AA.procrustes_cases():
        m = AA.procrustes_model(tgt, ref, w)
        if m["refused"]:
            refused.append(label)
            continue
        for pose in (m["pose"], AA.oracle_procrustes(m)):
            fig = AA.assert_procrustes(pose, m, label)
        if m["determined"]:
            assert m["spread"] < 1e-13, (label, m["spread"])  # SVD and Horn's quaternion agree: the model is one
        else:
            undetermined.append(label)
        # the undetermined cases still have a minimiser: any proper rotation about the cloud's own axis
        assert fig["excess"] <= m["err_slack"], label
    print("undetermined:", undetermined)
    assert all("zero_sum" in r for r in refused) and len(refused) == len(AA.PROCRUSTES_SIZES)
    assert all(u.startswith(("n=1 ", "n=2 ", "collinear", "all_equal")) for u in undetermined), undetermined
    assert sum(u.startswith("collinear") for u in undetermined) == 2 and sum(u.startswith("all_equal") for u in undetermined) == 2


def test_procrustes_without_the_reflection_fix_fails_the_rotation():
    tgt, ref = AA.procrustes_shape("mirrored")
    m = AA.procrustes_model(tgt, ref)
    assert m["d"] == -1.0 and m["determined"]
    assert _pkinds(AA.procrustes_model(tgt, ref, reflection_fix=False)["pose"], m) == ("rotation",)


def test_procrustes_with_weights_in_the_covariance_fails_the_pose():
    tgt, ref = AA.procrustes_cloud(257)
    w = AA.procrustes_weights("random", 257)
    m = AA.procrustes_model(tgt, ref, w)
    kinds = _pkinds(AA.procrustes_model(tgt, ref, w, weighted_cov=True)["pose"], m)
    assert "pose" in kinds and set(kinds) <= {"pose", "optimum"}, kinds


def test_procrustes_with_float64_means_fails_the_pose():
    """At a 1 km offset the float32 means sit up to 3e-5 m off the float64 ones; the centred differences follow, and with
    weights (which enter the means alone) so does the rotation — by far more than the bar.  The translation stays within
    the one ulp of the means the check grants, so it is the rotation that tells."""
    tgt, ref = AA.procrustes_shape("offset_1km")
    w = AA.procrustes_weights("random", len(tgt))
    m = AA.procrustes_model(tgt, ref, w)
    kinds = _pkinds(AA.procrustes_model(tgt, ref, w, mean_dtype=F64)["pose"], m)
    assert "pose" in kinds and set(kinds) <= {"pose", "centroid", "optimum"}, kinds
