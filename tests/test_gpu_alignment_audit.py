"""The three stand-alone alignment seams — IcpContext.align_point_to_plane, align_point_to_point, weighted_procrustes and
the plugin classes PointToPlaneAlignment / PointToPointAlignment over them — against the float64 model of
tests/alignment_audit.py, at every block edge of their kernels (k_reduce_given, k_reduce_p2p, k_procrustes_means,
k_procrustes_cov, k_sum_partials with check_done = 0, k_solve_given: no other path runs them).

`reduce_grid` gives min(ceil(n / 256), 256) workgroups of 256 threads, so the grid-stride loop turns a second time from row
65 536 on: the sizes bracket one row, one workgroup, and that turn.  Every call is made with host arrays and with device
tensors (bit-equal to each other), with the residual vector and without, and held to check_seam: the row count exactly, the
status, dx / loss at the project's step rule, each of the 29 sums within its summation bound of the model's, and the residual
vector (w r)^2 bit for bit in every row (exp / neighborhood / cauchy: within 4 x the CPU-measured spread of expf / logf).

tests/test_alignment_audit.py shows on the CPU that the oracle's output passes every case run here and that each
deliberately wrong copy of it fails by the kind meant.  The worst figures of every family are printed and quoted in the
docstrings below (measured on an MI355X).  Library changes this audit needed: the seams are now REFUSED between
register_launch and register_end (test_seam_inside_a_registration_is_refused), and an InvalidJacobianError raised by a
seam carries the outputs the library has written (`result`), as a registration's does.  No kernel changed.  Model
changes the CPU suite forced before the first device run: the spread of the float64 solves also takes a solve of the rows
added in the opposite order, and a step whose bar passes 1e-4 counts as undetermined (the oracle's own output missed
4 x the LU / Cholesky spread at pitch = pi / 2); cauchy runs with sigma 1 at 1, 2 and 5 rows and `neighborhood` with sigma
30 m at x0 != 0 (alignment_audit.sweep_sigma, X0_SCHEMES say why).
"""
import numpy as np
import pytest

import alignment_audit as AA
import iteration_audit as A

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


@pytest.fixture(scope="module")
def contexts(torch_cuda):
    """One context per (scheme, sigma), shared by the whole module: every test also shows that a context that has served
    other sizes and other seams before gives the model's answer."""
    from pylidar_slam_amd.engine import IcpContext
    made = {}

    def get(scheme, sigma):
        key = (scheme, float(sigma))
        if key not in made:
            made[key] = IcpContext(scheme=scheme, sigma=float(sigma))
        return made[key]
    yield get
    for ctx in made.values():
        ctx.close()


def _fresh(scheme, sigma):
    from pylidar_slam_amd.engine import IcpContext
    return IcpContext(scheme=scheme, sigma=float(sigma))


def _seam(ctx, torch, cost, ref, tgt, nrm, x0=None, residuals=True, device=False):
    """One seam call -> AA.seam_output (an Invalid Jacobian: the outputs the error carries)."""
    from pylidar_slam_amd.engine import InvalidJacobianError
    conv = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if device else (lambda a: a)
    status = AA.ICP_OK
    try:
        if cost == "point_to_plane":
            out = ctx.align_point_to_plane(conv(ref), conv(tgt), conv(nrm), with_residuals=residuals)
        else:
            out = ctx.align_point_to_point(conv(ref), conv(tgt), x0, with_residuals=residuals)
    except InvalidJacobianError as e:
        assert "Invalid Jacobian" in str(e) and isinstance(e, RuntimeError) and e.result is not None
        status, out = AA.ICP_ERR_INVALID_JACOBIAN, e.result
    res = None
    if residuals:
        res = out[4]
        assert (isinstance(res, torch.Tensor) and res.is_cuda) if device else isinstance(res, np.ndarray)
        res = res.cpu().numpy() if device else res
    return AA.seam_output(status, out[0], out[1], out[2], out[3], res)


def _same(a, b, residuals=True):
    ok = a["status"] == b["status"] and all(np.array_equal(a[k].view(np.uint32 if a[k].dtype == F32 else np.uint64),
                                                           b[k].view(np.uint32 if b[k].dtype == F32 else np.uint64))
                                            for k in ("pose", "params", "neq"))
    ok = ok and np.array_equal(np.float64(a["loss"]).view(np.uint64), np.float64(b["loss"]).view(np.uint64))
    if residuals and a["residuals"] is not None and b["residuals"] is not None:
        ok = ok and np.array_equal(a["residuals"].view(np.uint32), b["residuals"].view(np.uint32))
    return bool(ok)


def _audit(ctx, torch, worst, label, cost, scheme, sigma, ref, tgt, nrm, x0=None):
    """The four calls of one case (host / device, with / without the residual vector): bit-equal to each other, and the
    host call with residuals held to the model.  Returns (model, output)."""
    model = AA.seam_step(cost, ref, tgt, nrm, x0, scheme, sigma)
    host = _seam(ctx, torch, cost, ref, tgt, nrm, x0, True, False)
    fig = AA.assert_seam(host, model, label)
    worst.add(fig, label)
    for residuals, device in ((True, True), (False, False), (False, True)):
        other = _seam(ctx, torch, cost, ref, tgt, nrm, x0, residuals, device)
        assert _same(host, other), f"{label}: residuals {residuals} / device {device} differs from the host call's bits"
    return model, host


# ----------------------------------------------------------------------------------------------------------------------
# a. sizes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", AA.SWEEP_SCHEMES)
@pytest.mark.parametrize("cost", AA.COSTS)
def test_size_sweep(torch_cuda, contexts, cost, scheme):
    """1, 2, 5 (Invalid Jacobian, dx = 0, the loss still the model's), 6, 7, 63 .. 513, 65 535 / 65 536 / 65 537 (the first
    row of the stride's second turn), 65 536 + 257 and 3 x 65 536 + 100 rows (threads with four rows and with three).
    Measured, 6 x 18 cases: default and huber, both costs: dx equal to the model's in every float32 bit (|ddx| 0), dloss <= 4.4e-16,
    the worst sum at 0.15 of its bound, 4 x 461 114 residual rows bit-compared, none differs; cauchy (logf): |ddx| <= 2.4e-7
    (inside atol + rtol), dloss <= 1.0e-7, 2 x 461 114 rows held to the 2.4e-6 relative bar, the worst at 0.25 of it.  No
    case widened, none undetermined."""
    worst = AA.SeamWorst(f"sweep {cost} {scheme}")
    for n in AA.SWEEP_SIZES:
        ref, tgt, nrm = AA.sweep_case(cost, n)
        sigma = AA.sweep_sigma(scheme, n)
        model, out = _audit(contexts(scheme, sigma), torch_cuda, worst, f"n={n}", cost, scheme, sigma, ref, tgt, nrm)
        if n in AA.GUARD_SIZES:
            assert out["status"] == AA.ICP_ERR_INVALID_JACOBIAN and not out["params"].any(), n
        else:
            assert out["status"] == AA.ICP_OK, n
    print(worst)
    assert not worst.undetermined and not worst.widened


@pytest.mark.parametrize("cost", AA.COSTS)
def test_every_scheme_at_the_block_edges(torch_cuda, contexts, cost):
    """The five schemes the sweep leaves out, at 257 rows (two workgroups) and 65 537 (one row in the second turn).
    Measured, 2 x 10 cases: |ddx| 0, dloss <= 1.4e-8 (exp / neighborhood; 0 without expf), worst sum at 0.010 of its bound,
    2 x 197 382 rows bit-compared, 2 x 131 588 held to the bar (worst at 0.25 of it)."""
    worst = AA.SeamWorst(f"schemes {cost}")
    for scheme in AA.SCHEMES:
        if scheme in AA.SWEEP_SCHEMES:
            continue
        for n in AA.ALL_SCHEME_SIZES:
            ref, tgt, nrm = AA.sweep_case(cost, n)
            _audit(contexts(scheme, AA.SIGMA[scheme]), torch_cuda, worst, f"{scheme} n={n}", cost, scheme, AA.SIGMA[scheme],
                   ref, tgt, nrm)
    print(worst)
    assert not worst.undetermined and not worst.widened


# ----------------------------------------------------------------------------------------------------------------------
# b. row content
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cost", AA.COSTS)
def test_row_content(torch_cuda, contexts, cost):
    """65 537 rows holding r == 0 rows, rows with 0 < |r| < 1e-4 (the clamp), both Huber branches, coincident p == q rows
    (point-to-point: r = 0, J = 0, the weight 0 / 1e-4) and non-unit / zero normals (point-to-plane: taken as given, like the
    reference) — the census is asserted by tests/test_alignment_audit.py.
    Measured, 2 x 3 cases: |ddx| 0, dloss <= 1.4e-9, worst sum at 0.0017 of its bound, 2 x 131 074 rows bit-compared (huber,
    square_geman_mcclure), 2 x 65 537 (neighborhood) at most 0.24 of their bar; every residual finite."""
    worst = AA.SeamWorst(f"content {cost}")
    ref, tgt, nrm = AA.content_case(cost)
    for scheme in AA.CONTENT_SCHEMES:
        _, out = _audit(contexts(scheme, AA.SIGMA[scheme]), torch_cuda, worst, scheme, cost, scheme, AA.SIGMA[scheme], ref, tgt, nrm)
        assert out["status"] == AA.ICP_OK and np.isfinite(out["residuals"]).all()
    print(worst)


@pytest.mark.parametrize("cost", AA.COSTS)
def test_offsets(torch_cuda, contexts, cost):
    """The scene 1 km and 10 km from the origin (4097 rows).  The dx bar widens by the reference-side spread alone (10 km,
    point-to-plane: the float64 solves of the model differ by up to 7.6e-6); the sums and the residual vector keep their bars.
    Measured, 2 x 4 cases: 16 388 rows bit-compared per cost, dloss <= 1.9e-16; |ddx| 0 except point-to-plane at 10 km:
    7.63e-6 (huber; bar 3.05e-5 = 4 x the model's own spread of 7.6e-6), default inside 7.6e-7."""
    worst = AA.SeamWorst(f"offsets {cost}")
    for name, shift in AA.OFFSETS.items():
        ref, tgt, nrm = AA.content_case(cost, 4097, shift)
        for scheme in ("default", "huber"):
            _audit(contexts(scheme, AA.SIGMA[scheme]), torch_cuda, worst, f"{name} {scheme}", cost, scheme, AA.SIGMA[scheme],
                   ref, tgt, nrm)
    print(worst)
    assert not worst.undetermined


@pytest.mark.parametrize("cost", AA.COSTS)
def test_nan_row(torch_cuda, contexts, cost):
    """A NaN target row at the first, a middle and the last position, 257 and 65 537 rows: every sum is NaN and the call
    raises RuntimeError("Invalid Jacobian ...") with dx = 0 — the library's DOCUMENTED DEVIATION from the reference, whose
    `abs(det) < 1e-7` is False for NaN and which would hand back a NaN pose (solve_device.h: `!(fabs(det) >= 1e-7)`, "also
    catches NaN").  The residual vector is NaN exactly in that row and bit-equal to the model's elsewhere."""
    worst = AA.SeamWorst(f"nan {cost}")
    scheme, sigma = "huber", AA.SIGMA["huber"]
    for n in AA.NAN_SIZES:
        for where in ("first", "middle", "last"):
            ref, tgt, nrm, row = AA.nan_case(cost, n, where)
            _, out = _audit(contexts(scheme, sigma), torch_cuda, worst, f"n={n} {where}", cost, scheme, sigma, ref, tgt, nrm)
            assert out["status"] == AA.ICP_ERR_INVALID_JACOBIAN and not out["params"].any()
            bad = np.isnan(out["residuals"])
            assert bad.sum() == 1 and bad[row] and np.isnan(out["loss"])
    print(worst)
    assert worst.f["bit_rows"] == 3 * sum(AA.NAN_SIZES)


def test_no_rows_are_refused(torch_cuda, contexts):
    """n = 0: the invalid-argument error at all three seams; the next call on the context is unaffected."""
    ctx = contexts("huber", AA.SIGMA["huber"])
    ref, tgt, nrm = AA.sweep_case("point_to_plane", 257)
    before = _seam(ctx, torch_cuda, "point_to_plane", ref, tgt, nrm)
    empty = np.zeros((0, 3), F32)
    for call in (lambda: ctx.align_point_to_plane(empty, empty, empty), lambda: ctx.align_point_to_point(empty, empty),
                 lambda: ctx.weighted_procrustes(empty, empty),
                 lambda: ctx.align_point_to_plane(*(torch_cuda.from_numpy(empty).cuda(),) * 3)):
        with pytest.raises(AssertionError):
            call()
        assert _same(before, _seam(ctx, torch_cuda, "point_to_plane", ref, tgt, nrm))


# ----------------------------------------------------------------------------------------------------------------------
# c. the linearisation point
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AA.X0_CASES))
def test_linearisation_point(torch_cuda, contexts, name):
    """Point-to-point at x0 = zero, a small pose, yaw 3 rad, pitch float32(pi / 2) and a translation alone, 257 and 65 537
    rows, least_square / huber / neighborhood (which weighs by the RAW target: sigma 30 m).  Where cos / sin of x0 have one
    float32 answer on the CPU (float32, float64 rounded and the oracle's matrices agree to the bit) the rows are held bit for
    bit; at pitch = pi / 2 (gimbal lock) the reference leaves the STEP undetermined — its own float64 solves differ by
    1e4 rad — and the sums, the residual vector and the loss carry the case.
    Measured, 5 x 6 cases: |ddx| <= 1.2e-7 (half an ulp of params = x0 + dx), dloss <= 1.3e-8, worst sum at 0.0079 of its bound;
    per x0 131 588 rows bit-compared (least_square, huber: the three evaluations of cos / sin agree to the bit at all five
    points) and 65 794 (neighborhood) at most 0.25 of their bar; at pitch = pi / 2 the call's dx is 1.3e5 rad off the
    model's, as the oracle's own is."""
    worst = AA.SeamWorst(f"x0 {name}")
    for n in AA.X0_SIZES:
        ref, tgt, x0 = AA.x0_case(name, n)
        for scheme, sigma in AA.X0_SCHEMES:
            model, out = _audit(contexts(scheme, sigma), torch_cuda, worst, f"{scheme} n={n}", "point_to_point", scheme, sigma,
                                ref, tgt, None, x0)
            assert out["status"] == AA.ICP_OK
            if name == "zero":  # x0 = zeros is x0 = None
                assert _same(out, _seam(contexts(scheme, sigma), torch_cuda, "point_to_point", ref, tgt, None, None))
    print(worst)
    assert bool(worst.undetermined) == (name == "pitch_half_pi")


def test_residual_guard_at_x0(torch_cuda, contexts):
    """Targets already aligned under x0 (every residual exactly 0): the guard returns params == x0 bit for bit, loss 0."""
    ref, tgt, x0 = AA.x0_guard_case()
    worst = AA.SeamWorst("guard")
    model, out = _audit(contexts("huber", 0.1), torch_cuda, worst, "guard", "point_to_point", "huber", 0.1, ref, tgt, None, x0)
    assert model["ref"]["stopped"] and out["status"] == AA.ICP_OK and out["loss"] == 0.0
    assert np.array_equal(out["params"].view(np.uint32), x0.view(np.uint32)) and not out["residuals"].any()


@pytest.mark.parametrize("n", AA.X0_SIZES)
def test_initialize_with_svd(torch_cuda, contexts, n):
    """PointToPointAlignment(initialize_with_svd): x0 = from_pose_matrix(weighted_procrustes(ref, tgt)) — the Procrustes
    seam in the reference's argument order, itself held to its model — and the step at that x0 held to the model of the
    step; the class returns the bits of the IcpContext calls."""
    from pylidar_slam_amd.odometry import PointToPointAlignment, from_pose_matrix
    ref, tgt, _ = AA.x0_case("small", n)
    worst = AA.SeamWorst(f"svd n={n}")
    for scheme, sigma in AA.X0_SCHEMES:
        ctx = contexts(scheme, sigma)
        T = ctx.weighted_procrustes(ref, tgt)
        AA.assert_procrustes(T, AA.procrustes_model(ref, tgt), "x0")
        x0 = from_pose_matrix(T.astype(F32))
        _, out = _audit(ctx, torch_cuda, worst, f"{scheme}", "point_to_point", scheme, sigma, ref, tgt, None, x0)
        pose, params, res = PointToPointAlignment(ctx, initialize_with_svd=True).align(ref, tgt)
        assert np.array_equal(params[0], out["params"]) and np.array_equal(pose[0], out["pose"])
        assert np.array_equal(res[0], out["residuals"])
    print(worst)


# ----------------------------------------------------------------------------------------------------------------------
# d. Procrustes
# ----------------------------------------------------------------------------------------------------------------------
def _procrustes(ctx, torch, label, tgt, ref, w, worst):
    model = AA.procrustes_model(tgt, ref, w)
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    if model["refused"]:
        for call in (lambda: ctx.weighted_procrustes(tgt, ref, w), lambda: ctx.weighted_procrustes(dev(tgt), dev(ref), dev(w))):
            with pytest.raises(AssertionError, match="sum to zero"):
                call()
        return None
    T = ctx.weighted_procrustes(tgt, ref, w)
    Td = ctx.weighted_procrustes(dev(tgt), dev(ref), dev(w))
    assert np.array_equal(T.view(np.uint64), Td.view(np.uint64)), f"{label}: device inputs give other bits"
    fig = AA.assert_procrustes(T, model, label)
    for k in ("drot", "dtrans"):
        worst[k] = max(worst[k], fig[k])
    worst["ratio"] = max(worst["ratio"], fig["drot"] / model["rot_tol"] if model["determined"] else 0.0)
    worst["n"] += 1
    worst["undetermined"] += not model["determined"]
    return T


@pytest.mark.parametrize("n", AA.PROCRUSTES_SIZES)
def test_procrustes_sizes(torch_cuda, contexts, n):
    """n in 1, 2, 3, 255, 256, 257, 65 537, 3 x 65 536 + 100; weights none / uniform / random / one non-zero / with negative
    entries / a zero sum (refused, the context usable afterwards).  n = 1 and 2 leave the rotation undetermined: the
    invariants alone (proper rotation to 1e-12, the centroids mapped, the alignment error at the model's optimum).
    Measured, 34 determined cases: rotation within 4.8e-15 of the model's (at most 0.025 of its bar), translation within
    1.3e-14; 10 undetermined cases (n = 1, 2) meet the invariants; 8 zero sums refused."""
    ctx = contexts("default", 0.5)
    worst = dict(drot=0.0, dtrans=0.0, ratio=0.0, n=0, undetermined=0)
    tgt, ref = AA.procrustes_cloud(n)
    plain = None
    for kind in AA.WEIGHT_KINDS:
        if n > 257 and kind not in ("none", "random", "zero_sum"):
            continue
        T = _procrustes(ctx, torch_cuda, f"n={n} {kind}", tgt, ref, AA.procrustes_weights(kind, n), worst)
        if kind == "none":
            plain = T
        elif kind == "uniform":  # (uniform weights of a power of two: the same float64 sums, scaled)
            assert np.array_equal(T, plain)
    print(f"procrustes n={n}: {worst}")
    assert worst["undetermined"] == (worst["n"] if n < 3 else 0)


@pytest.mark.parametrize("kind", AA.SHAPE_KINDS)
def test_procrustes_shapes(torch_cuda, contexts, kind):
    """Collinear and all-equal clouds (undetermined: the invariants), the coplanar clouds of the golden file, a mirrored
    cloud (the reflection fix), a 180 degree rotation, and a 1 km offset, where the float32 centred differences lose bits —
    the model forms them the same way.
    Measured: rotation within 2.7e-15 (mirrored), translation within 1.7e-12 (1 km offset), at most 0.013 of the bar."""
    ctx = contexts("default", 0.5)
    worst = dict(drot=0.0, dtrans=0.0, ratio=0.0, n=0, undetermined=0)
    tgt, ref = AA.procrustes_shape(kind)
    for wk in ("none", "random"):
        _procrustes(ctx, torch_cuda, f"{kind} {wk}", tgt, ref, AA.procrustes_weights(wk, len(tgt)), worst)
    print(f"procrustes {kind}: {worst}")
    assert worst["undetermined"] == (2 if kind in ("collinear", "all_equal") else 0)


# ----------------------------------------------------------------------------------------------------------------------
# e. the plugin classes
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", AA.ALL_SCHEME_SIZES)
@pytest.mark.parametrize("cost", AA.COSTS)
def test_plugin_classes(torch_cuda, contexts, cost, n):
    """PointToPlaneAlignment.align / PointToPointAlignment.align with [N,3] and [1,N,3] inputs, numpy and cuda: (pose
    [1,4,4], params [1,6], residuals [1,N]) as the reference returns them, where the inputs live, the bits of the IcpContext
    call, which passes check_seam.  The documented refusals stay refusals."""
    from pylidar_slam_amd.odometry import PointToPlaneAlignment, PointToPointAlignment
    torch = torch_cuda
    scheme, sigma = "huber", AA.SIGMA["huber"]
    ctx = contexts(scheme, sigma)
    ref, tgt, nrm = AA.sweep_case(cost, n)
    worst = AA.SeamWorst(f"plugin {cost} n={n}")
    _, out = _audit(ctx, torch, worst, "context", cost, scheme, sigma, ref, tgt, nrm)
    algo = PointToPlaneAlignment(ctx) if cost == "point_to_plane" else PointToPointAlignment(ctx)
    for batched in (False, True):
        for device in (False, True):
            conv = (lambda a: torch.from_numpy(a).cuda()) if device else (lambda a: a)
            args = [conv(a[None] if batched else a) for a in ((ref, tgt, nrm) if cost == "point_to_plane" else (ref, tgt))]
            got = algo.align(args[0], args[1], ref_normals=args[2]) if cost == "point_to_plane" else algo.align(*args)
            for g, shape, want in zip(got, ((1, 4, 4), (1, 6), (1, n)), (out["pose"], out["params"], out["residuals"])):
                assert tuple(g.shape) == shape, (batched, device, g.shape)
                assert (isinstance(g, torch.Tensor) and g.is_cuda) if device else isinstance(g, np.ndarray), (batched, device)
                g = g.cpu().numpy() if device else g
                assert g.dtype == F32 and np.array_equal(g[0].view(np.uint32), want.view(np.uint32)), (batched, device)
    with pytest.raises(AssertionError, match="mask"):
        algo.align(ref, tgt, ref_normals=nrm, mask=np.ones(n, bool)) if cost == "point_to_plane" else \
            algo.align(ref, tgt, mask=np.ones(n, bool))
    if cost == "point_to_plane":
        with pytest.raises(AssertionError, match="initial_estimate"):
            algo.align(ref, tgt, ref_normals=nrm, initial_estimate=np.eye(4, dtype=F32))
        with pytest.raises(AssertionError, match="ref_normals"):
            algo.align(ref, tgt)
    else:  # initial_estimate as a matrix and as parameters: the step at that x0
        x0 = np.array(AA.X0_CASES["small"], F32)
        want = _seam(ctx, torch, cost, ref, tgt, None, x0)
        for est in (x0, AA.O.build_pose_matrix(x0)):
            pose, params, res = algo.align(ref, tgt, initial_estimate=est)
            if est.size == 6:
                assert np.array_equal(params[0], want["params"]) and np.array_equal(res[0], want["residuals"])
            else:  # (from_pose_matrix of the matrix: x0 within float32 rounding)
                np.testing.assert_allclose(params[0], want["params"], atol=2e-6)


# ----------------------------------------------------------------------------------------------------------------------
# f. shared state
# ----------------------------------------------------------------------------------------------------------------------
def test_small_calls_after_a_large_one(torch_cuda):
    """3 x 65 536 + 100 rows, then 5, 257 and 1 row on the same context: exactly what a fresh context gives (no stale partial
    rows — 256 were written, the small calls sum 1 or 2 — and no stale staging), for both costs and for Procrustes."""
    scheme, sigma = "huber", AA.SIGMA["huber"]
    used = _fresh(scheme, sigma)
    for cost in AA.COSTS:
        ref, tgt, nrm = AA.sweep_case(cost, AA.SWEEP_SIZES[-1])
        _seam(used, torch_cuda, cost, ref, tgt, nrm)
        used.weighted_procrustes(tgt, ref)
        for n in (5, 257, 1):
            ref, tgt, nrm = AA.sweep_case(cost, n)
            fresh = _fresh(scheme, sigma)
            for device in (False, True):
                assert _same(_seam(used, torch_cuda, cost, ref, tgt, nrm, device=device),
                             _seam(fresh, torch_cuda, cost, ref, tgt, nrm, device=device)), (cost, n, device)
            assert np.array_equal(used.weighted_procrustes(tgt, ref), fresh.weighted_procrustes(tgt, ref)), (cost, n)
            fresh.close()
    used.close()


def test_interleaved_seams(torch_cuda):
    """The three seams interleaved on one context, sizes going up and down: each call the bits of a fresh context's."""
    scheme, sigma = "geman_mcclure", AA.SIGMA["geman_mcclure"]
    used = _fresh(scheme, sigma)
    for n in (AA.STRIDE + 1, 7, 513, AA.STRIDE + 257, 64):
        for cost in AA.COSTS:
            ref, tgt, nrm = AA.sweep_case(cost, n)
            fresh = _fresh(scheme, sigma)
            w = AA.procrustes_weights("random", n)
            want = (_seam(fresh, torch_cuda, cost, ref, tgt, nrm), fresh.weighted_procrustes(tgt, ref, w))
            got_p = used.weighted_procrustes(tgt, ref, w)
            got = _seam(used, torch_cuda, cost, ref, tgt, nrm, device=(n % 2 == 1))
            assert _same(got, want[0]) and np.array_equal(got_p, want[1]), (n, cost)
            fresh.close()
    used.close()


def _registration_context(k=6):
    from pylidar_slam_amd.engine import IcpContext
    scan, model = A.tiny_scene()
    ctx = IcpContext(height=16, width=256, max_num_alignments=k, threshold_delta_pose=0.0, scheme="huber", sigma=A.ROW_SIGMA)
    ctx.map_set(model)
    init = AA.O.build_pose_matrix(np.array([0.05, -0.03, 0.01, 0.002, -0.001, 0.005], F32))
    return ctx, np.ascontiguousarray(scan), init


def _same_result(a, b):
    return (np.array_equal(a.pose, b.pose) and np.array_equal(a.params, b.params) and a.iterations == b.iterations
            and a.converged == b.converged and a.num_targets == b.num_targets and np.array_equal(a.losses, b.losses)
            and np.array_equal(a.dx, b.dx))


def test_seam_registration_seam(torch_cuda):
    """A seam call, a registration, the same seam call: the registration equals the one of a context that never ran a seam,
    the second seam call the first — for all three seams, host and device inputs."""
    clean, scan, init = _registration_context()
    want = clean.register(scan, init, skip_null=True)
    assert want.iterations == 6 and clean.handoff_fallbacks() == 0
    clean.close()
    for cost in AA.COSTS:
        ref, tgt, nrm = AA.sweep_case(cost, AA.STRIDE + 257)
        for device in (False, True):
            ctx, scan, init = _registration_context()
            first = _seam(ctx, torch_cuda, cost, ref, tgt, nrm, device=device)
            first_p = ctx.weighted_procrustes(tgt, ref)
            got = ctx.register(scan, init, skip_null=True)
            assert _same_result(got, want) and ctx.handoff_fallbacks() == 0, (cost, device)
            assert _same(first, _seam(ctx, torch_cuda, cost, ref, tgt, nrm, device=device)), (cost, device)
            assert np.array_equal(first_p, ctx.weighted_procrustes(tgt, ref)), (cost, device)
            ctx.close()


def test_seam_inside_a_registration_is_refused(torch_cuda):
    """A seam call between register_launch and register_end (one ordinary small registration forced to 6 iterations).

    THE CONTRACT, decided from api.hip: REFUSED with "registration in progress", like icp_map_update and
    icp_nearest_neighbor_search.  The seams stage host inputs into ctx->targets and sum into ctx->partials and ctx->neq, the
    buffers of the enqueued registration.  Stream order protects the launches already enqueued, but not what the host does
    later: the timed-out hand-off path of icp_register_end re-runs the rest of the loop from ctx->tgt_ptr — which a
    host-input seam call has overwritten — a chunked launch solves its next chunk from ctx->partials, and
    normal_equations_tensor() would hold the seam's sums.  The allowed contract cannot be shown safe from the code, so
    icp_align_point_to_plane, icp_align_point_to_point and icp_weighted_procrustes now check `in_registration ||
    result_pending()` (include/icp_mi355x.h says so).  The refusal leaves the pending registration untouched: its result and
    last_neighbors equal the undisturbed ones; afterwards the seams give what an idle context gives."""
    clean, scan, init = _registration_context()
    clean.register_launch(scan, init, skip_null=True)
    want = clean.register_end()
    want_ix, want_pose = clean.last_neighbors(len(scan))
    assert want.iterations == 6 and clean.handoff_fallbacks() == 0
    ref, tgt, nrm = AA.sweep_case("point_to_plane", 513)
    idle = (_seam(clean, torch_cuda, "point_to_plane", ref, tgt, nrm), _seam(clean, torch_cuda, "point_to_point", ref, tgt, None),
            clean.weighted_procrustes(tgt, ref))
    clean.close()
    dev = lambda a: torch_cuda.from_numpy(a).cuda()  # noqa: E731
    ctx, scan, init = _registration_context()
    ctx.register_launch(scan, init, skip_null=True)
    for call in (lambda: ctx.align_point_to_plane(ref, tgt, nrm, with_residuals=True), lambda: ctx.align_point_to_point(ref, tgt),
                 lambda: ctx.weighted_procrustes(tgt, ref), lambda: ctx.align_point_to_plane(dev(ref), dev(tgt), dev(nrm)),
                 lambda: ctx.align_point_to_point(dev(ref), dev(tgt)), lambda: ctx.weighted_procrustes(dev(tgt), dev(ref))):
        with pytest.raises(AssertionError, match="registration in progress"):
            call()
    got = ctx.register_end()
    got_ix, got_pose = ctx.last_neighbors(len(scan))
    assert _same_result(got, want) and ctx.handoff_fallbacks() == 0
    assert np.array_equal(got_ix, want_ix) and np.array_equal(got_pose, want_pose)
    after = (_seam(ctx, torch_cuda, "point_to_plane", ref, tgt, nrm), _seam(ctx, torch_cuda, "point_to_point", ref, tgt, None),
             ctx.weighted_procrustes(tgt, ref))
    assert _same(after[0], idle[0]) and _same(after[1], idle[1]) and np.array_equal(after[2], idle[2])
    # ... and between register_begin and register_end
    ctx.register_begin(scan, init, skip_null=True)
    ctx.iteration_accumulate()
    with pytest.raises(AssertionError, match="registration in progress"):
        ctx.align_point_to_point(ref, tgt)
    ctx.register_end()
    ctx.close()
