"""`-m gpu`: the projective local map pinned pixel by pixel — holes, borders, odd shapes, every window size, recycled
storage slots.  Inputs and accounting: tests/projective_cases.py (its helpers are shown to bite on the CPU in
tests/test_projective_cases.py).  Every test prints its counts; unexplained pixels are never tolerated."""
import numpy as np
import pytest

import projective_cases as PC

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


@pytest.fixture(scope="module")
def O():
    import icp_oracle
    return icp_oracle


def _ctx(**kw):
    from pylidar_slam_amd.engine import IcpContext
    return IcpContext(**kw)


@pytest.fixture(scope="module")
def shared_ctx(torch_cuda):
    """One context per image size for the stateless entry points."""
    made = {}

    def get(h, w):
        if (h, w) not in made:
            made[(h, w)] = _ctx(height=h, width=w)
        return made[(h, w)]
    yield get
    for c in made.values():
        c.close()


# ---- A. normal maps --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PC.NORMAL_CASES, ids=PC.case_id)
def test_normal_map_case(torch_cuda, shared_ctx, case):
    """`icp_compute_normal_map` against the float64 oracle, every pixel in exactly one class decided from the oracle's
    window sums: null -> exactly 0; determined -> same zero / non-zero status and sin(angle) <= 2 float32 ulp +
    C_SOLVE eps64 cond(A); undetermined (fewer than three points in the window, the determinant's rounding bound straddles
    1e-6, or cond(A) puts the tolerance above 1e-4) -> 0 or a unit vector, finite.  Host and device inputs give the same
    bits.

    C_SOLVE = 12048 = 4 x 3012, the largest spread (in eps64 cond(A)) between the oracle's adjugate and np.linalg.solve
    over the accounted cases, measured on the CPU (test_solve_spread_backs_the_tolerance); resulting bounds: 2.4e-7 for
    cond(A) below 1e3 up to 1e-4 at cond(A) = 3.7e7.  Measured on the MI355X: no unexplained pixel in any case; the largest
    determined-pixel error is 4.4e-8 (bounds 2.4e-7 .. 4.0e-7 at those pixels) — the float32 rounding of the oracle's value:
    the kernel adds the same float64 products in the same order and its adjugate differs from the oracle's only in the
    scaling by the determinant.  Undetermined pixels of the accounted cases: 52 of 43146 (holes, 64 x 1024, kernel 3), 9 of
    28358 (keep-50 %, 64 x 1024, kernel 5), none elsewhere.  Unit normals made of rounding noise (windows with one or two
    far returns, as in the reference): 65 of the 2235 undetermined pixels of the x3-far keep-10 % map, 97 of 99 and 19 of
    19 on the one-row image at kernel sizes 3 and 5, 2 on the 64 x 1024 map with holes at kernel size 3."""
    source, h, w, content, ks, accounted = case
    ctx = shared_ctx(h, w)
    v = PC.normal_case_input(source, h, w, content)
    ref = PC.NormalReference(v, ks)
    nm = ctx.compute_normal_map(v, ks)
    dn = ctx.compute_normal_map(torch_cuda.from_numpy(v).cuda(), ks)
    assert dn.is_cuda and np.array_equal(dn.cpu().numpy().view(np.uint32), nm.view(np.uint32))
    got = ref.account(nm)
    print(f"normal map {PC.case_id(case)}: null {got['null']}, determined {got['determined']}, undetermined "
          f"{got['undetermined']} (unit normals of rounding noise: {got['noise_normals']}), unexplained "
          f"{len(got['unexplained'])}; largest determined error {got['worst_sin']:.2e} (bound {got['worst_tol']:.2e})")
    assert len(got["unexplained"]) == 0, got["unexplained"][:8]
    if accounted:
        assert got["undetermined"] <= 0.01 * got["non_null"]


def test_kernel_sizes_are_checked(torch_cuda):
    """Even kernel sizes, 0 and 17 are refused by icp_compute_normal_map, icp_pmap_update and icp_batch_pmap_update; a
    refused update leaves the window and the model as they were."""
    from pylidar_slam_amd.engine import IcpBatch
    h, w = 17, 33
    ctxs = [_ctx(height=h, width=w, local_map_size=2) for _ in range(2)]
    v = PC.scan_vmap(h, w)
    eye = np.eye(4, dtype=F32)
    for c in ctxs:
        c.pmap_init()
        c.pmap_update(eye, v, 3)
    before = [c.pmap_model() for c in ctxs]
    batch = IcpBatch(ctxs)
    for ks in (0, 2, 4, 16, 17, -1):
        with pytest.raises(AssertionError):
            ctxs[0].compute_normal_map(v, ks)
        with pytest.raises(AssertionError):
            ctxs[0].pmap_update(PC.window_poses(1)[0], v, ks)
        with pytest.raises(AssertionError):
            batch.pmap_update([eye, eye], [v, None], ks)
        for c, (mv, mn) in zip(ctxs, before):
            assert c.pmap_num_maps() == 1
            now = c.pmap_model()
            assert np.array_equal(now[0], mv) and np.array_equal(now[1], mn)
    batch.close()
    for c in ctxs:
        c.close()


# ---- B. compute_neighbors --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(32, 256), (17, 33), (5, 7), (1, 300), (3, 3)])
def test_compute_neighbors_edges(torch_cuda, O, shared_ctx, h, w):
    """Bit-exact against O.compute_neighbors: K = 1, 2, 20; duplicate layers (the first wins); distances one float32 ulp
    apart; pixels null in every layer; null target pixels; 0, 1 and 6 field channels; shapes with a partial last block."""
    ctx = shared_ctx(h, w)
    rng = np.random.default_rng(h * 1000 + w)
    flat = lambda a: a.reshape(a.shape[:-2] + (-1,))
    for k in (1, 2, 20):
        for c_fields in (0, 1, 6):
            tgt = rng.normal(size=(3, h, w)).astype(F32)
            ref = rng.normal(size=(k, 3, h, w)).astype(F32)
            fld = rng.normal(size=(k, c_fields, h, w)).astype(F32) if c_fields else None
            t, r = flat(tgt), flat(ref)  # views
            npix = h * w
            p_null_t, p_null_r, p_dup, p_ulp_a, p_ulp_b = 0, npix // 3, npix // 2, npix - 1, npix - 2
            t[:, p_null_t] = 0.0
            r[:, :, p_null_r] = 0.0
            if k > 1:
                r[:, :, p_dup] = r[k - 1, :, p_dup]  # every layer the same point: the first
                for p, order in ((p_ulp_a, (1, 0)), (p_ulp_b, (0, 1))):
                    t[:, p] = np.array([0.25, 0.0, -0.25], F32)
                    r[:, :, p] = (t[:, p] + F32(3.0))[None]
                    r[order[0], :, p] = t[:, p] + np.array([0.5, 0, 0], F32)  # distance 0.5
                    r[order[1], :, p] = t[:, p] + np.array([np.nextafter(F32(0.5), F32(1)), 0, 0], F32)  # one ulp more
            nb, nf = ctx.compute_neighbors(tgt, ref, fld)
            onb, onf = O.compute_neighbors(tgt, ref, fld)
            assert np.array_equal(nb, onb), (k, c_fields)  # (values: the oracle's null pixels are x * 0 = -0.0)
            nbf = flat(nb)
            assert not nbf[:, p_null_t].any() and not nbf[:, p_null_r].any()
            if k > 1:
                assert np.array_equal(nbf[:, p_ulp_a], r[1, :, p_ulp_a]) and np.array_equal(nbf[:, p_ulp_b], r[0, :, p_ulp_b])
            if c_fields:
                assert np.array_equal(nf, onf), (k, c_fields)
                f, nff = flat(fld), flat(nf)
                for p in (p_null_t, p_null_r) + ((p_dup,) if k > 1 else ()):
                    assert np.array_equal(nff[:, p], f[0, :, p])  # index 0's fields
            else:
                assert nf is None


# ---- C. window and model ---------------------------------------------------------------------------------------------
WINDOW_CASES = [(32, 256, 2, 3, "golden"), (32, 256, 4, 7, "golden"), (17, 33, 1, 7, "scan"), (64, 1024, 1, 5, "scan")]


@pytest.mark.parametrize("h,w,lms,ks,source", WINDOW_CASES)
def test_window_and_model(torch_cuda, O, h, w, lms, ks, source):
    """`icp_pmap_update` / `icp_pmap_get_model` against ProjectiveLocalMapOracle over PC.window_sequence: every storage
    slot recycled twice, pose-only updates, a non-identity first pose, sparse maps with holes into the slot a dense one was
    evicted from, yaw steps of a few tenths of a radian.  After EVERY update every pixel of every layer is equal to the
    oracle's (same winning source pixel; vertex within 4 ulp(|x| + |y| + |z| + max|t|), <= 1.9e-6 m at 16 m, of
    O.apply_transformation; vertex and normal bit-equal to the fma chain of that source pixel's vertex and device normal)
    or explained as a coin toss of the reference's own projection or a z-buffer tie.  Unexplained: none; explained at most
    0.5 % of the occupied pixels.  The poses are the library's composition (PC.LibraryWindowOracle) and stay within
    4 ulp(largest entry) per update of the stock oracle's.

    Measured on the MI355X: unexplained 0 in all four sequences; explained 0 of 112920 (32 x 256, window 2), 0 of 273622
    (window 4), 0 of 3405 (17 x 33), 8 of 348146 (64 x 1024); largest vertex difference 0 (bound 1.9e-6: the fma chain and
    the oracle's BLAS product round alike); pose drift from the stock oracle at most 4.8e-7 (bound 1.5e-5).  The float64
    projection of the CPU suite (test_float64_projection_stays_inside_the_cap): explained 2, 4, 0 and 15."""
    ctx = _ctx(height=h, width=w, local_map_size=lms)
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=lms, normals_kernel_size=ks,
                                 nmap_of=lambda v: ctx.compute_normal_map(v, ks))
    stock = O.ProjectiveLocalMapOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=lms, normals_kernel_size=ks,
                                       normals_dtype=F64)
    ctx.pmap_init()
    total = dict(occupied=0, equal=0, explained=0, model_unequal=0, model_compared=0, model_flagged=0)
    worst, drift_max, unexplained = (0.0, 0.0), 0.0, []
    calls = PC.window_sequence(h, w, lms, source)
    for n, (pose, v) in enumerate(calls):
        ctx.pmap_update(pose, v, ks)
        orc.update(pose, v)
        stock.update(pose, v)
        assert ctx.pmap_num_maps() == len(orc.vmaps) == len(stock.vmaps)
        scale = max(float(np.abs(p).max()) for p in orc.poses + stock.poses)
        drift = max(float(np.abs(a - b).max()) for a, b in zip(orc.poses, stock.poses))
        assert drift <= PC.pose_drift_bound(n + 1, scale), (n, drift)
        drift_max = max(drift_max, drift)
        mv, mn = ctx.pmap_model()
        if v is not None:  # the newest layer holds nothing the new map does not hold
            assert (np.abs(mv[-1]).max(axis=0) > 0).sum() <= (np.abs(v).max(axis=0) > 0).sum()
        got = PC.account_model(mv, mn, orc.vmaps, orc.nmaps, orc.poses, h, w)
        for key in total:
            total[key] += got[key]
        worst = max(worst, (got["worst_dv"], got["worst_tol"]))
        unexplained += [(n,) + u for u in got["unexplained"]]
    print(f"window {h}x{w} size {lms} kernel {ks}: {len(calls)} updates, occupied {total['occupied']}, equal "
          f"{total['equal']}, explained {total['explained']}, unexplained {len(unexplained)}; largest vertex difference "
          f"{worst[0]:.2e} (bound {worst[1]:.2e}); pose drift from the stock oracle {drift_max:.2e}")
    assert unexplained == [], unexplained[:8]
    assert total["explained"] <= 0.005 * total["occupied"]
    # beside it, stricter: every pixel of every layer is the winner of the bit model of the projection (no coin toss)
    print(f"window {h}x{w} size {lms}: against the bit model, {total['model_compared']} pixels compared, "
          f"{total['model_unequal']} unequal, {total['model_flagged']} rows flagged")
    assert total["model_unequal"] == 0
    ctx.close()


def test_recorded_reference_model(torch_cuda, O):
    """The reference's own `_model_vmap` / `_model_nmap` after its `ls` run (tests/golden/projective.npz), so far read by no
    test: `pmap_update` driven with the reference's relative poses and key-frame rule.  The device's model equals the
    oracle's (account_model) and the oracle's equals the recorded one (account_recorded) apart from explained pixels; the
    normals at the pixels with the reference's winner sit within the float32-box-filter bars already used for `nmap0`
    (median < 1e-3, p99 < 2e-2).  Measured on the MI355X: device vs oracle explained 0, oracle vs recorded explained 0 of
    28760 occupied, unexplained 0; normals at all 28760 pixels: median 1.7e-4, p99 4.3e-3."""
    import os
    g = np.load(os.path.join(PC.GOLDEN, "projective.npz"))
    h, w = (int(x) for x in g["hw"])
    ctx = _ctx(height=h, width=w, local_map_size=4)
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=4,
                                 nmap_of=lambda v: ctx.compute_normal_map(v, 5))
    calls = PC.recorded_run_updates(g)
    ctx.pmap_init()
    for pose, v in calls:
        ctx.pmap_update(pose, v)
        orc.update(pose, v)
    assert ctx.pmap_num_maps() == g["ls_model_vmap"].shape[0]
    mv, mn = ctx.pmap_model()
    dev = PC.account_model(mv, mn, orc.vmaps, orc.nmaps, orc.poses, h, w)
    scale = max(float(np.abs(p).max()) for p in orc.poses)
    rec = PC.account_recorded(g["ls_model_vmap"], orc.vmaps, orc.poses, h, w, PC.pose_drift_bound(len(calls), scale))
    both = np.stack(rec["same_winner"]) & (np.abs(mv - orc.model_vmap).max(axis=1) == 0) & \
        (np.abs(mn).max(axis=1) > 0) & (np.abs(g["ls_model_nmap"]).max(axis=1) > 0)
    ang = np.linalg.norm(np.cross(mn, g["ls_model_nmap"], axis=1), axis=1)[both]
    print(f"recorded model: device vs oracle explained {dev['explained']}, oracle vs recorded explained {rec['explained']} of "
          f"{rec['occupied']}, unexplained {len(dev['unexplained']) + len(rec['unexplained'])}; normals at {both.sum()} "
          f"pixels: median {np.median(ang):.1e}, p99 {np.percentile(ang, 99):.1e}")
    assert dev["unexplained"] == [] and rec["unexplained"] == [], (dev["unexplained"][:4], rec["unexplained"][:4])
    assert dev["explained"] + rec["explained"] <= 0.005 * rec["occupied"]
    assert dev["model_unequal"] == 0, dev["model_first"]
    assert both.sum() > 0.95 * rec["occupied"]
    assert np.median(ang) < 1e-3 and np.percentile(ang, 99) < 2e-2
    ctx.close()


# ---- D. association --------------------------------------------------------------------------------------------------
def _built_map(ctx, h, w, lms, source, updates, ks=5):
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=lms, normals_kernel_size=ks,
                                 nmap_of=lambda v: ctx.compute_normal_map(v, ks))
    ctx.pmap_init()
    for pose, v in PC.window_sequence(h, w, lms, source)[:updates]:
        ctx.pmap_update(pose, v, ks)
        orc.update(pose, v)
    return orc


def _associate(ctx, orc, pts, h, w):
    """The device's rows for `pts` held to PC.account_association (exact part + the oracle's matched set)."""
    mv, mn = ctx.pmap_model()
    _, index = ctx.project(pts, with_index=True)
    rows = ctx.pmap_nearest_neighbor_search(pts)
    finite = np.where(np.isfinite(pts).all(axis=1)[:, None], pts, 0).astype(F32)
    model = PC.account_model(mv, mn, orc.vmaps, orc.nmaps, orc.poses, h, w)
    assert model["unexplained"] == []
    assert model["model_unequal"] == 0, model["model_first"]
    got = PC.account_association(rows, mv, mn, pts, index, orc.nearest_neighbor_search(finite), model["explained_pixels"])
    assert got["model_unequal"] == 0, got
    return rows, got, index


@pytest.mark.parametrize("h,w,lms,source", [(32, 256, 2, "golden"), (17, 33, 1, "scan"), (64, 1024, 1, "scan"),
                                            (5, 7, 4, "scan")])
def test_association_rows(torch_cuda, O, h, w, lms, source):
    """`icp_pmap_nearest_neighbor_search`: every returned row is, bit for bit, the neighbour and normal of the layer a
    float32 argmin selects in `pmap_model()` at the pixel the device projects the target to, in pixel order, and every
    occupied target pixel with a non-null layer yields a row; the matched targets equal the oracle's apart from coin
    tosses.  Measured on the MI355X: unexplained 0 and explained 0 in all four: 5950 rows (32 x 256), 161 (17 x 33), 15546
    (64 x 1024, a sparse map with holes), 32 (5 x 7)."""
    ctx = _ctx(height=h, width=w, local_map_size=lms)
    orc = _built_map(ctx, h, w, lms, source, 5)
    pts = PC.association_targets(h, w, PC.window_poses(1, yaw=0.05, step=0.4)[0], source=source)
    if (h, w) == (32, 256):  # two targets of equal range in one pixel, nearer than anything else there: the higher index
        pair = np.array([[1.0, 0.002, -0.125], [1.0, -0.002, -0.125]], F32)
        assert PC.range32(pair)[0] == PC.range32(pair)[1]
        pts = np.concatenate([pts, pair])
    rows, got, index = _associate(ctx, orc, pts, h, w)
    print(f"association {h}x{w}: rows {got['rows']}, explained {got['explained']}, unexplained {len(got['unexplained'])}")
    assert got["unexplained"] == [], got["unexplained"][:8]
    assert got["rows"] == got["expected_rows"] > 0
    assert got["explained"] <= max(3, 0.005 * got["rows"])
    if (h, w) == (32, 256):
        assert PC.match_rows(pts[-2:-1], rows[2])[0] < 0
        assert (index == len(pts) - 1).sum() == 1 and not (index == len(pts) - 2).any()
    # device input: the same bits
    dev = ctx.pmap_nearest_neighbor_search(torch_cuda.from_numpy(pts).cuda())
    for a, b in zip(dev, rows):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
    ctx.close()


def test_association_edges(torch_cuda, O):
    """n = 0, n > H*W, K = 1, a pixel empty in all layers, only invalid rows."""
    h, w = 17, 33
    ctx = _ctx(height=h, width=w, local_map_size=1)
    v = PC.damage(PC.scan_vmap(h, w), "holes")
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=1,
                                 nmap_of=lambda m: ctx.compute_normal_map(m, 5))
    ctx.pmap_init()
    ctx.pmap_update(np.eye(4, dtype=F32), v)
    orc.update(np.eye(4, dtype=F32), v)
    assert ctx.pmap_num_maps() == 1
    for pts in (np.zeros((0, 3), F32), np.array([[np.nan, 1, 1], [0, 0, 0], [0.0, 0.0, 9.0]], F32)):
        nb, nn, tg = ctx.pmap_nearest_neighbor_search(pts)
        assert nb.shape == nn.shape == tg.shape == (0, 3)
    big = O.vertex_map_to_points(PC.scan_vmap(64, 1024, frame=1))  # 65536 rows (null ones included) into 561 pixels
    big = big[np.unique(PC._row_keys(big), return_index=True)[1]]
    assert big.shape[0] > 50 * h * w
    rows, got, index = _associate(ctx, orc, big, h, w)
    print(f"association edges: {big.shape[0]} targets -> rows {got['rows']}, explained {got['explained']}")
    assert got["unexplained"] == [] and 0 < got["rows"] == got["expected_rows"]
    # a target pixel whose every layer is empty yields no row: the holes are there
    empty = (np.abs(ctx.pmap_model()[0]).max(axis=(0, 1)) == 0) & (index >= 0)
    assert empty.sum() > 0 and got["rows"] == int(((index >= 0) & ~empty).sum())
    ctx.close()


# ---- E. one iteration's rows -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,source", [(17, 33, "scan"), (64, 1024, "scan")])
def test_one_iteration_rows(torch_cuda, O, h, w, source):
    """`icp_pmap_register` with one forced iteration, all eight schemes, both target modes, identity and non-identity initial
    pose: dx, loss and row count against the normal equations recomputed on the host (float32 rows, float64 sums:
    O.gauss_newton_step) from the DEVICE'S OWN association of the transformed targets (`pmap_nearest_neighbor_search` of
    the fma-chain positions) — dx atol 2e-7 / rtol 2e-5, loss rtol 1e-5 (the bars of test_gauss_newton_step), the row count
    exactly: `pixel_of` (the iteration) and `project_device` (the association seam) assign the same pixels.  The inputs
    hold r == 0 rows, 0 < |r| < 1e-4 rows and both Huber branches at sigma = 0.05 — asserted.  Then five forced iterations
    against the oracle's loop at 1e-4 m / 1e-4 rad.

    Measured on the MI355X (both shapes): largest |dx - host| 9.3e-10, largest relative loss difference 4.7e-8; rows per
    case 523 .. 561 (17 x 33) and 48104 .. 55472 (64 x 1024), 24 of them with r == 0, 1 .. 206 with 0 < |r| < 1e-4, 117 ..
    19854 on the linear Huber branch; five iterations: <= 3.1e-8 m / 7.1e-10 rad (17 x 33), <= 1.0e-5 m / 4.5e-7 rad
    (64 x 1024) from the oracle's loop."""
    calls, scan, inits = PC.iteration_case(h, w, source)
    ctxs = {s: _ctx(height=h, width=w, local_map_size=4, max_num_alignments=1, threshold_delta_pose=0.0, scheme=s,
                    sigma=PC.ROW_SIGMA) for s in PC.SCHEMES}
    for c in ctxs.values():
        c.pmap_init()
        for pose, v in calls:
            c.pmap_update(pose, v)
    first = ctxs["default"]
    mv, mn = first.pmap_model()
    for c in ctxs.values():
        assert np.array_equal(c.pmap_model()[0], mv)
    worst = dict(dx=0.0, loss=0.0)
    for which, init in enumerate(inits):
        for skip_null in (False, True):
            targets, planted = PC.iteration_targets(mv, init, scan, skip_null)
            assert planted > 0
            moved = PC.moved_targets(targets, init, skip_null)
            rows = first.pmap_nearest_neighbor_search(moved)
            census = PC.residual_census(rows, PC.ROW_SIGMA)
            print(f"rows {h}x{w} pose {which} skip_null {skip_null}: {rows[0].shape[0]} rows, {census}")
            assert min(census.values()) > 0, census
            for scheme, c in ctxs.items():
                res = c.pmap_register(targets, init, skip_null=skip_null)
                assert res.iterations == 1
                ref = PC.host_step(rows, scheme, PC.ROW_SIGMA)
                PC.assert_step(res.dx[0], float(res.losses[0]), res.num_targets, ref)
                worst["dx"] = max(worst["dx"], float(np.abs(res.dx[0] - ref[0]).max()))
                worst["loss"] = max(worst["loss"], abs(float(res.losses[0]) - ref[1]) / abs(ref[1]))
    print(f"rows {h}x{w}: largest |dx - host| {worst['dx']:.2e}, largest relative loss difference {worst['loss']:.2e}")
    for c in ctxs.values():
        c.close()
    # five forced iterations
    targets = scan[np.abs(scan).max(axis=1) > 0]
    for scheme in ("default", "huber"):
        ctx = _ctx(height=h, width=w, local_map_size=4, max_num_alignments=5, threshold_delta_pose=0.0, scheme=scheme,
                   sigma=0.5)
        orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=4, normals_dtype=F64)
        ctx.pmap_init()
        for pose, v in calls:
            ctx.pmap_update(pose, v)
            orc.update(pose, v)
        res = ctx.pmap_register(targets, inits[1])
        assert res.iterations == 5
        ref = PC.oracle_registration(orc, targets, inits[1], 5, scheme, 0.5)
        dt, dr = O.pose_error(res.pose, ref)
        print(f"five iterations {h}x{w} {scheme}: {dt:.1e} m / {dr:.1e} rad from the oracle's loop")
        assert dt < 1e-4 and dr < 1e-4, (scheme, dt, dr)
        ctx.close()


# ---- F. the same edges through the batch -----------------------------------------------------------------------------
def test_edges_through_the_batch(torch_cuda):
    """B = 3 members of one image size and different content — dense maps; the recycled-slot sequence with sparse maps and
    holes; a member that mostly gets pose-only updates — through IcpBatch.pmap_update (kernel size 3: the fused
    k_pm_insert_batch) and pmap_register_launch: windows, models, poses, losses and steps bit-equal to three single
    contexts given the same calls."""
    from pylidar_slam_amd.engine import IcpBatch
    from test_gpu_batch_projective import _model_state, _record, _same
    h, w, lms, ks = 32, 256, 2, 3
    kw = dict(height=h, width=w, local_map_size=lms, max_num_alignments=6, threshold_delta_pose=0.0, scheme="huber",
              sigma=0.1)
    ours, refs = [_ctx(**kw) for _ in range(3)], [_ctx(**kw) for _ in range(3)]
    for c in ours + refs:
        c.pmap_init()
    batch = IcpBatch(ours)
    holes = [c for c in PC.window_sequence(h, w, lms, "golden")]
    poses = PC.window_poses(len(holes), yaw=0.1, step=0.5, seed=9)
    for n, (pose, v) in enumerate(holes):
        dense = PC.golden_vmap(n % 6)
        maps = [dense, v, dense if n % 5 == 0 else None]
        rels = [poses[n], pose, poses[-1 - n]]
        batch.pmap_update(rels, maps, ks)
        for c, r, m in zip(refs, rels, maps):
            c.pmap_update(r, m, ks)
        for b in range(3):
            a, r = _model_state(ours[b]), _model_state(refs[b])
            assert a[0] == r[0] and np.array_equal(a[1].view(np.uint32), r[1].view(np.uint32)) and \
                np.array_equal(a[2].view(np.uint32), r[2].view(np.uint32)), f"update {n}, member {b}: window / model"
        if n % 4 == 3:
            scan = O_points(PC.golden_vmap((n + 1) % 6))
            scans = [scan, PC.damage(PC.golden_vmap((n + 2) % 6), "holes").reshape(3, -1).T.copy(), scan[::3].copy()]
            inits = [poses[0], None, poses[1]]
            batch.pmap_register_launch(scans, inits, skip_null=True)
            got = batch.register_end()
            for b, c in enumerate(refs):
                _same(_record(got[b]), _record(c.pmap_register(scans[b], inits[b], skip_null=True)),
                      f"update {n}, member {b}")
    assert [c.pmap_num_maps() for c in ours] == [lms, lms, lms]
    batch.close()
    for c in ours + refs:
        c.close()


def O_points(vmap):
    return np.ascontiguousarray(vmap.reshape(3, -1).T)


# ---- F. the projective kernels round with the projection's function: its boundary cloud through them ---------------------
def _in_band(points, h, w):
    import projection_audit as PA
    row, col, r, _ = PA.coordinates(np.ascontiguousarray(points, F32), h, w, PC.UP_FOV, PC.DOWN_FOV, exact=False)
    with np.errstate(invalid="ignore"):
        return (PA.near_half(row) | PA.near_half(col)) & (r > 0)


def test_boundary_cloud_as_the_window(torch_cuda, O):
    """`k_pm_project` on the refinement branch: the boundary cloud of tests/projection_audit.py (a point on every row and column
    boundary of the 16 x 128 image and its copies 1, 2, 3 ulp either side) planted as the vertex map of a window of size 1, at
    the identity pose and — turned beforehand, so that the layer's pose puts it back on its boundaries — behind one pose-only
    update by a yaw of 0.25 rad.  Every pixel of the layer is the winner of the bit model: no coin toss is granted."""
    import projection_audit as PA
    h, w = 16, 128
    pl = PA.planted(h, w)
    yaw = PA.yaw_pose()
    for what, vmap, updates in (("identity", pl["vmap"], [(np.eye(4, dtype=F32), "vmap")]),
                                ("yaw 0.25 rad", pl["vmap_turned"], [(np.eye(4, dtype=F32), "vmap"), (yaw, None)])):
        ctx = _ctx(height=h, width=w, local_map_size=1)
        orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=1,
                                     nmap_of=lambda v: ctx.compute_normal_map(v, 5))
        ctx.pmap_init()
        for pose, v in updates:
            v = np.array(vmap) if v is not None else None
            ctx.pmap_update(pose, v)
            orc.update(pose, v)
        assert ctx.pmap_num_maps() == 1
        mv, mn = ctx.pmap_model()
        moved = PC.transform_fma(O.vertex_map_to_points(np.array(vmap)), orc.poses[0])
        share = float(_in_band(moved, h, w).mean())
        lv = O.vertex_map_to_points(mv[0])
        unequal, compared, flagged = PC.bit_model_unequal(lv, moved, h, w)
        print(f"boundary cloud as the window, {what}: {share:.0%} of {moved.shape[0]} source pixels in the refinement band, "
              f"{compared} pixels compared with the bit model, {unequal.size} unequal, {flagged} rows flagged")
        assert share > 0.9 and flagged == 0
        assert unequal.size == 0, [(int(p // w), int(p % w)) for p in unequal[:8]]
        got = PC.account_model(mv, mn, orc.vmaps, orc.nmaps, orc.poses, h, w)
        assert got["model_unequal"] == 0 and got["unexplained"] == [], (got["model_first"], got["unexplained"][:4])
        ctx.close()


def test_boundary_cloud_as_the_targets(torch_cuda, O):
    """`k_pm_project_targets` on the refinement branch: one forced iteration of `pmap_register` whose targets are the boundary
    cloud (identity guess), and the cloud turned back by 0.25 rad (guess: that yaw), against a real map.  What the iteration
    associated is visible in its step: the row count equals, and dx and the loss are within the bars of the E tests of, a host
    Gauss-Newton step on the rows the BIT MODEL's pixels give; `pmap_nearest_neighbor_search` on the moved targets returns
    exactly those rows."""
    import projection_audit as PA
    h, w = 16, 128
    pl = PA.planted(h, w)
    ctx = _ctx(height=h, width=w, local_map_size=1, max_num_alignments=1, threshold_delta_pose=0.0, sigma=PC.ROW_SIGMA)
    ctx.pmap_init()
    ctx.pmap_update(np.eye(4, dtype=F32), PC.scan_vmap(h, w))
    mv, mn = ctx.pmap_model()
    for what, targets, init in (("identity", np.array(pl["rows"]), np.eye(4, dtype=F32)),
                                ("yaw 0.25 rad", np.array(pl["back"]), PA.yaw_pose())):
        moved = PC.moved_targets(targets, init, False)
        bit = PA.model(moved, h, w, PC.UP_FOV, PC.DOWN_FOV)
        share = float(_in_band(moved, h, w).mean())
        assert share > 0.9 and not bit.flagged.any(), (what, share)
        want = PC.expected_association(mv, mn, moved, bit.index)[:3]
        rows = ctx.pmap_nearest_neighbor_search(moved)
        for a, b in zip(rows, want):
            assert a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), b.view(np.uint32)), what
        res = ctx.pmap_register(targets, init)
        assert res.iterations == 1
        ref = PC.host_step(want, "default", PC.ROW_SIGMA)
        PC.assert_step(res.dx[0], float(res.losses[0]), res.num_targets, ref)
        print(f"boundary cloud as the targets, {what}: {share:.0%} of {moved.shape[0]} targets in the refinement band, "
              f"{res.num_targets} rows (the bit model: {ref[2]}), |dx| {float(np.abs(ref[0]).max()):.2e}, |dx - host| "
              f"{float(np.abs(res.dx[0] - ref[0]).max()):.2e}")
    ctx.close()
