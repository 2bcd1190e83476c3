"""CPU: the bit model of the spherical projection (tests/projection_audit.py) against everything that can pin it without a
GPU — the reference's recordings, the numpy oracle, an all-float64 evaluation — and nine deliberately wrong copies, each
caught on a named cloud.  tests/test_gpu_projection_audit.py holds the kernels to this model bit for bit.

Measured here: the model reproduces tests/golden/components.npz exactly (0 of 3 636 points in another pixel, 0 of 2 048
pixels of the vertex map differ, coordinates within 2.3e-5 pixel); on the edge clouds recorded from the reference
(tests/golden/projection_edges.npz, 16 x 128) no point outside the reference's coin-toss band lands in another pixel and the
validity of every special row is the reference's; no row of any cloud the GPU file projects is flagged."""
import os

import numpy as np
import pytest

import projection_audit as P
import projective_cases as PC

F32, F64 = np.float32, np.float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def O():
    import icp_oracle
    return icp_oracle


def _half_distance(v):
    with np.errstate(invalid="ignore"):
        return np.abs(v - np.floor(v) - F32(0.5))


def _rounded(row, col, r, h, w):
    with np.errstate(invalid="ignore"):
        pr, pc = np.rint(row), np.rint(col)
        ok = (pr >= 0) & (pr <= h - 1) & (pc >= 0) & (pc <= w - 1) & (r > 0)
    return np.where(ok, np.nan_to_num(pr) * w + np.nan_to_num(pc), -1).astype(np.int64)


# ---- the model against the reference's recordings ------------------------------------------------------------------------
def test_model_reproduces_the_recorded_reference(golden_components, O):
    g = golden_components
    h, w = (int(v) for v in g["proj_hw"])
    up, down = (float(v) for v in g["proj_fov"])
    m = P.model(g["proj_pc"], h, w, up, down)
    ref_r, ref_c = g["proj_pixels"][:, 0], g["proj_pixels"][:, 1]
    band = PC.toss_band(h, w)
    worst = max(float(np.abs(m.row - ref_r).max()), float(np.abs(m.col - ref_c).max()))
    moved = int(((np.rint(m.row) != np.rint(ref_r)) | (np.rint(m.col) != np.rint(ref_c))).sum())
    print(f"components.npz: coordinates within {worst:.2e} pixel (band {band:.2e}), {moved} of {m.n} points in another pixel")
    assert worst <= band
    assert moved == 0
    P.check_bits(m.vmap, g["proj_vmap"], "the recorded vertex map")
    _, oidx = O.build_projection_map(g["proj_pc"], h, w, up, down, return_index=True)
    assert np.array_equal(m.index, oidx.astype(np.int32))
    assert not m.flagged.any()


def test_model_on_the_scan_of_the_spread_recording():
    """tests/golden/projection_spread.npz holds no coordinates of its 64 x 2048 scan, only figures the reference's code paths
    agree on: the 16 smallest distances of a coordinate to a half-integer under the scalar path.  The model's coordinates are
    within the coin-toss band of that path's, so its 16 smallest distances are within the band of the recorded ones (the k-th
    smallest of a set moves by no more than its elements do), and no pixel may change winner between the model and the oracle
    evaluated with float32 libm unless a coin toss explains it."""
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    spread = np.load(os.path.join(GOLDEN, "projection_spread.npz"))
    scan = make_sequence(SceneConfig(height=64, width=2048), 1)[0][0]
    m = P.model(scan, 64, 2048)
    band = PC.toss_band(64, 2048)
    d = np.sort(np.concatenate((_half_distance(m.row[m.r > 0]), _half_distance(m.col[m.r > 0]))))[:16]
    for key in spread.files:
        if key.startswith("scan_") and key.endswith("closest_to_boundary"):
            assert np.abs(d - spread[key]).max() <= band, (key, d, spread[key])
    assert not m.flagged.any()


def test_model_against_the_reference_on_the_edges():
    """tests/golden/projection_edges.npz (oracle/make_golden_projection_edges.py: the unmodified reference, scalar path, on the
    boundary, image-edge, special-row and tie clouds at 16 x 128).  Per point: the float coordinates agree within the
    coin-toss band, NaN where the reference has NaN; a point lands in another pixel than the reference rounded it to only if
    the reference's coordinate is in the band, and then in a neighbouring one.  Per pixel: the vertex map equals the recording
    on every pixel that no in-band point can enter or leave and that holds no range tie for its winner (the reference's argsort
    is not stable).  The validity of every special row is the reference's."""
    g = np.load(os.path.join(GOLDEN, "projection_edges.npz"))
    h, w = (int(v) for v in g["hw"])
    up, down = (float(v) for v in g["fov"])
    band = PC.toss_band(h, w)
    compared = {}
    for name in ("boundary", "image_edge", "special", "ties"):
        pc, pix, vm = g[name + "_pc"], g[name + "_pix"], g[name + "_vmap"]
        assert np.array_equal(pc.view(np.uint32), P.clouds(h, w, up, down, which=(name,))[name].view(np.uint32)), \
            f"{name}: the seeded cloud is no longer the one the reference was run on: re-record"
        m = P.model(pc, h, w, up, down)
        assert not m.flagged.any()
        got = np.stack((m.row, m.col), axis=1)
        assert np.array_equal(np.isnan(got), np.isnan(pix)), name
        with np.errstate(invalid="ignore"):
            worst = float(np.nanmax(np.abs(got - pix)))
        assert worst <= band, (name, worst, band)
        rr = F32(np.sqrt((pc.astype(F64) ** 2).sum(axis=1)))  # (only its sign and zero matter below)
        ref_pixel = _rounded(pix[:, 0], pix[:, 1], np.where(m.r == 0, 0, rr), h, w)
        toss = (_half_distance(pix[:, 0]) <= band) | (_half_distance(pix[:, 1]) <= band)
        moved = ref_pixel != m.pixel
        assert not (moved & ~toss).any(), (name, np.flatnonzero(moved & ~toss)[:5])
        with np.errstate(invalid="ignore"):
            near = (np.abs(np.rint(m.row) - np.rint(pix[:, 0])) <= 1) & (np.abs(np.rint(m.col) - np.rint(pix[:, 1])) <= 1)
        assert near[moved].all(), name
        # pixels the comparison leaves out: those an in-band point is in on either side, and those whose winning range is shared
        out = np.zeros(h * w, bool)
        for p in (m.pixel[toss], ref_pixel[toss]):
            out[p[p >= 0]] = True
        v = np.flatnonzero(m.valid)
        best = m.r[np.maximum(m.index.reshape(-1), 0)]
        share = np.bincount(m.pixel[v], weights=(m.r[v] == best[m.pixel[v]]).astype(F64), minlength=h * w)
        out |= share > 1
        P.check_bits(vm, m.vmap, f"{name}: the reference's vertex map", out.reshape(1, h, w))
        compared[name] = (int((~out & (m.index.reshape(-1) >= 0)).sum()), int((~out).sum()), int(moved.sum()), worst)
    print("edges, (occupied pixels compared, pixels compared, points a coin toss moved, worst coordinate difference):", compared)
    assert compared["image_edge"][0] > 50 and compared["ties"][0] >= 1 and compared["special"][0] >= 5
    # validity of the special rows: NaN, inf, zero, subnormal squares, underflow, -0
    pc, pix, kind = g["special_pc"], g["special_pix"], g["special_kind"]
    m = P.model(pc, h, w, up, down)
    ref_null = (pix[:, 0] == -1) & (pix[:, 1] == -1)
    assert np.array_equal(ref_null, m.r == 0)
    names = np.array(P.SPECIAL_KINDS)[kind]
    assert ref_null[names == "zero"].all() and ref_null[names == "underflow"].all() and ref_null[names == "negative_zero"].all()
    assert not ref_null[names == "subnormal_squares"].any() and m.valid[names == "subnormal_squares"].all()
    assert np.isinf(m.r[names == "overflow"]).all() and m.valid[names == "overflow"].all()
    assert not m.valid[names == "nan"].any()
    # every recorded non-null pixel holds a valid row of the model's, and every valid row's pixel is non-null in the recording
    occupied = np.abs(g["special_vmap"]).max(axis=0).reshape(-1) > 0
    assert np.array_equal(occupied, m.index.reshape(-1) >= 0)
    # the seam and the z axis of the image-edge cloud: y = -0 behind the sensor gives col = W and is dropped, in both
    pc, pix = g["image_edge_pc"], g["image_edge_pix"]
    m = P.model(pc, h, w, up, down)
    seam = (pc[:, 0] < 0) & (pc[:, 1] == 0)
    minus = seam & np.signbit(pc[:, 1])
    assert minus.sum() >= 3 and (pix[minus, 1] == w).all() and (m.col[minus] == w).all() and not m.valid[minus].any()
    assert (pix[seam & ~minus, 1] == 0).all() and (m.col[seam & ~minus] == 0).all()
    axis = (pc[:, 0] == 0) & (pc[:, 1] == 0) & (pc[:, 2] != 0)
    assert axis.sum() == 8 and np.array_equal(pix[axis], np.stack((m.row, m.col), axis=1)[axis])


# ---- the model against the oracle and against float64 -----------------------------------------------------------------------
@pytest.mark.parametrize("h,w", P.IMAGES)
def test_model_against_the_oracle(O, h, w):
    """`oracle.spherical_projection` (float32 libm) on the LiDAR-like clouds: coordinates within the coin-toss band; every
    point the two round to different pixels has its oracle coordinate in the band."""
    band = PC.toss_band(h, w)
    for fov in P.FOVS[:3]:
        for seed in (1, 2, 3):
            pc = P.lidar(seed, 20000, h, w, *fov)
            m = P.model(pc, h, w, *fov)
            orow, ocol, orng = O.spherical_projection(pc, h, w, *fov)
            worst = max(float(np.abs(orow - m.row).max()), float(np.abs(ocol - m.col).max()))
            assert worst <= band, (fov, seed, worst, band)
            moved = _rounded(orow, ocol, orng, h, w) != m.pixel
            toss = (_half_distance(orow) <= band) | (_half_distance(ocol) <= band)
            assert not (moved & ~toss).any(), (fov, seed, np.flatnonzero(moved & ~toss)[:5])


def _float64_coordinates(pc, h, w, up, down):
    p = pc.astype(F64)
    r = np.sqrt((p * p).sum(axis=1))
    a_up, a_down = abs(up) / 180.0 * np.pi, abs(down) / 180.0 * np.pi
    theta, phi = -np.arctan2(p[:, 1], p[:, 0]), np.arcsin(p[:, 2] / r)
    return (1.0 - (phi + a_down) / (a_up + a_down)) * h, 0.5 * (theta / np.pi + 1.0) * w, phi


@pytest.mark.parametrize("h,w", P.IMAGES)
def test_model_against_float64(h, w):
    """The model's coordinates against the same formulas in float64 on the float32 inputs.  With u = 2^-24 (half an ulp,
    relative) the float32 roundings allow:

    column: theta = atan2 rounded once (u |theta|); pi as float32 is 2.8e-8 < u off; the quotient theta / pi rounds (u): at
    most 3 u on a value of magnitude <= 1; adding 1 rounds a sum in [0, 2] (u); halving is exact; the product with W rounds
    (u): |d col| <= (0.5 * 4 u + u) W = 3 u W.

    row: the range carries at most 2.5 u (three squares and two sums, halved by the root, and the root), the quotient q = z / r
    3.5 u, which asin turns into 3.5 u |tan(phi)|; asin rounds once (u |phi|); fov_down rounds (u fov_down); their sum rounds
    (u |phi + fov_down|); fov rounds and the quotient Q by it rounds (2 u |Q|); 1 - Q rounds (u |1 - Q|); the product with H
    rounds (u |1 - Q|):
    |d row| <= H u ((3.5 |tan phi| + |phi| + fov_down + |phi + fov_down|) / fov + 2 |Q| + 2 |1 - Q|).

    Asserted: 4 x these bounds, per point (the factor the other audits use); the worst ratio measured is printed."""
    u = 2.0 ** -24
    worst = [0.0, 0.0]
    for fov in P.FOVS:
        pc = P.lidar(11, 50000, h, w, *fov)
        m = P.model(pc, h, w, *fov)
        row, col, phi = _float64_coordinates(pc, h, w, *fov)
        a_up, a_down = abs(fov[0]) / 180.0 * np.pi, abs(fov[1]) / 180.0 * np.pi
        q = (phi + a_down) / (a_up + a_down)
        with np.errstate(over="ignore"):
            bound_row = h * u * ((3.5 * np.abs(np.tan(phi)) + np.abs(phi) + a_down + np.abs(phi + a_down)) / (a_up + a_down)
                                 + 2.0 * np.abs(q) + 2.0 * np.abs(1.0 - q))
        bound_col = 3.0 * u * w
        ratio_row = float((np.abs(m.row.astype(F64) - row) / bound_row).max())
        ratio_col = float(np.abs(m.col.astype(F64) - col).max() / bound_col)
        worst = [max(worst[0], ratio_row), max(worst[1], ratio_col)]
        assert ratio_row <= 4.0 and ratio_col <= 4.0, (fov, ratio_row, ratio_col)
    print(f"{h} x {w}: model against float64, worst |d row| / bound {worst[0]:.2f}, worst |d col| / bound {worst[1]:.2f} (bar 4)")


# ---- deliberately wrong copies ------------------------------------------------------------------------------------------
WRONG_CASES = (
    # (the wrong copy, image, field of view, the cloud that must show it)
    ("farther_wins", (16, 128), (3.0, -24.0), "lidar"),
    ("tie_lowest_index", (16, 128), (3.0, -24.0), "ties"),
    ("half_away", (16, 128), (3.0, -24.0), "boundary"),
    ("less_than_at_edge", (16, 128), (3.0, -24.0), "image_edge"),
    ("column_band_only", (64, 2048), (3.0, -24.0), "boundary"),
    ("no_refinement", (16, 128), (3.0, -24.0), "boundary"),
    ("fused_range", (16, 128), (3.0, -24.0), "ties"),
    ("fov_float32", (16, 128), (2.0, -24.0), "boundary"),  # (float32(a) + float32(b) = float32(a + b) for the four audited fields)
)


@pytest.mark.parametrize("wrong,image,fov,cloud", WRONG_CASES, ids=[c[0] for c in WRONG_CASES])
def test_wrong_copy_is_caught(wrong, image, fov, cloud):
    h, w = image
    pc = P.clouds(h, w, *fov, which=(cloud,))[cloud]
    right, bad = P.model(pc, h, w, *fov), P.model(pc, h, w, *fov, wrong=wrong)
    moved = int((right.index != bad.index).sum())
    print(f"{wrong}: {moved} pixels of the {cloud} cloud at {h} x {w}, field of view {fov}, get another winner")
    assert moved >= 1
    with pytest.raises(AssertionError):
        P.check_map(bad.index, bad.vmap, bad.rows, right, pc, wrong)


def test_stale_z_buffer_is_caught():
    """a z-buffer that keeps the previous call's keys: the one-pixel cloud projected behind the LiDAR-like cloud at 16 x 128"""
    h, w = P.IMAGES[0]
    cl = P.clouds(h, w, which=("lidar", "one_pixel"))
    first = P.model(cl["lidar"], h, w)
    right = P.model(cl["one_pixel"], h, w)
    bad = P.model(cl["one_pixel"], h, w, wrong="stale_zbuffer", keys=first.keys)
    assert int((right.index != bad.index).sum()) >= 100
    with pytest.raises(AssertionError):
        P.check_map(bad.index, bad.vmap, bad.rows, right, cl["one_pixel"], "stale")


def test_check_bits_and_the_accounting_name_what_differs():
    h, w = P.IMAGES[0]
    pc = P.clouds(h, w, which=("ties",))["ties"]
    m = P.model(pc, h, w)
    assert P.check_map(m.index, m.vmap, m.rows, m, pc) == h * w
    index = m.index.copy()
    p = int(np.flatnonzero(index.reshape(-1) >= 0)[0])
    index.reshape(-1)[p] = -1
    count, lines = P.account(index, m, pc)
    assert count == 1 and f"= {p}:" in lines[0] and "got -1" in lines[0]
    with pytest.raises(AssertionError, match="1 of"):
        P.check_map(index, None, None, m, pc)
    nan = np.array([np.nan, 1.0], F32)
    assert P.check_bits(nan, nan.copy()) == 2
    with pytest.raises(AssertionError, match="first at"):
        P.check_bits(np.array([0.0], F32), np.array([-0.0], F32))


# ---- the stricter accounting of the projective tests ---------------------------------------------------------------------
def test_projective_accounting_against_the_bit_model(O):
    """`model_unequal` of PC.account_model / PC.account_association: 0 for a model layer and an index map built with the bit
    model, 1 for one tampered pixel, many for a z-buffer that keeps the farther point; the coin-toss accounting beside it is
    untouched (it still explains or equals every pixel of the bit model's layer)."""
    h, w = 16, 128
    v = PC.scan_vmap(h, w)
    nm = O.compute_normal_map(v, 5).astype(F32)
    pose = PC.window_poses(1)[0]
    src, src_n = O.vertex_map_to_points(v), O.vertex_map_to_points(nm)
    valid = np.abs(src).max(axis=1) > 0
    pts = np.where(valid[:, None], PC.transform_fma(src, pose), np.nan).astype(F32)
    m = P.model(pts, h, w)
    won = m.index.reshape(-1)
    mn = np.where((won >= 0)[:, None], PC.transform_fma(src_n, pose, translate=False)[np.maximum(won, 0)], 0).astype(F32)
    mv, mn = m.vmap[None], np.ascontiguousarray(mn.T).reshape(1, 3, h, w)
    got = PC.account_model(mv, mn, [v], [nm], [pose], h, w)
    assert got["model_unequal"] == 0 and got["model_compared"] == h * w and got["unexplained"] == []
    bad = mv.copy()
    at = np.argwhere(m.index >= 0)[5]
    bad[0, :, at[0], at[1]] = 0
    assert PC.account_model(bad, mn, [v], [nm], [pose], h, w)["model_unequal"] == 1
    far, far_n = PC.emulate_model([v], [nm], [pose], h, w, keep_farther=True)
    assert PC.account_model(far, far_n, [v], [nm], [pose], h, w)["model_unequal"] > 10
    # association: the index map of the bit model, and its winners as the returned targets
    tg = PC.association_targets(h, w, PC.window_poses(1, yaw=0.05, step=0.4)[0], source="scan")
    t = P.model(tg, h, w)
    rows = PC.expected_association(mv, mn, tg, t.index)[:3]
    assert PC.account_association(rows, mv, mn, tg, t.index)["model_unequal"] == 0
    other = t.index.copy()
    first, second = np.argwhere(t.index >= 0)[:2]
    other[tuple(first)], other[tuple(second)] = t.index[tuple(second)], t.index[tuple(first)]
    wrong_rows = PC.expected_association(mv, mn, tg, other)[:3]
    assert PC.account_association(wrong_rows, mv, mn, tg, other)["model_unequal"] >= 2


def test_planted_boundary_clouds_stay_on_their_boundaries(O):
    """what tests/test_gpu_projective_edges.py plants: behind the fma chain of the pose each kernel applies, every row is in the
    refinement band, none is flagged, and a projection without refinement would move pixels"""
    h, w = 16, 128
    pl = P.planted(h, w)
    eye = np.eye(4, dtype=F32)
    for name, pts, pose in (("window, identity", O.vertex_map_to_points(np.array(pl["vmap"])), eye),
                            ("window, yaw", O.vertex_map_to_points(np.array(pl["vmap_turned"])), PC.invert4(P.yaw_pose())),
                            ("targets, identity", pl["rows"], eye), ("targets, yaw", pl["back"], P.yaw_pose())):
        moved = PC.transform_fma(pts, pose)
        frow, fcol, _, _ = P.coordinates(moved, h, w, 3.0, -24.0, exact=False)
        m = P.model(moved, h, w)
        assert (P.near_half(frow) | P.near_half(fcol)).all() and not m.flagged.any(), name
        assert (P.model(moved, h, w, wrong="no_refinement").index != m.index).sum() >= 20, name


# ---- the clouds ---------------------------------------------------------------------------------------------------------
def test_no_cloud_of_the_gpu_file_has_a_flagged_row():
    rows = cases = 0
    for what, h, w, up, down, cloud in P.every_gpu_case():
        if cloud.shape[0] == 0:
            continue
        _, _, _, flagged = P.coordinates(np.ascontiguousarray(cloud), h, w, up, down)
        assert not flagged.any(), f"{what}: rows {np.flatnonzero(flagged)[:5].tolist()} are flagged: change the seed"
        rows += cloud.shape[0]
        cases += 1
    print(f"{cases} clouds, {rows} rows, none flagged")


def test_the_clouds_are_what_they_claim():
    h, w = P.IMAGES[1]
    cl = P.clouds(h, w)
    m = P.model(cl["boundary"], h, w)
    frow, fcol, _, _ = P.coordinates(cl["boundary"], h, w, 3.0, -24.0, exact=False)
    in_band = P.near_half(frow) | P.near_half(fcol)
    on_half = (_half_distance(m.row) == 0) | (_half_distance(m.col) == 0)
    print(f"boundary cloud at {h} x {w}: {m.n} rows, {int(in_band.sum())} in the refinement band, {int(on_half.sum())} exactly "
          f"on a half")
    assert in_band.all() and on_half.sum() > m.n // 2
    frow, fcol, _, _ = P.coordinates(cl["band_edge"], h, w, 3.0, -24.0, exact=False)
    in_band = P.near_half(frow) | P.near_half(fcol)
    assert 0.2 < in_band.mean() < 0.8  # rows on both sides of the band's edge
    lid = P.model(cl["lidar"], h, w)
    assert (lid.row[lid.r > 0] < -0.5).any() and (lid.row[lid.r > 0] > h - 0.5).any()  # off the top and the bottom
    t = P.model(P.clouds(16, 128, which=("ties",))["ties"], 16, 128)
    counts = np.bincount(t.pixel[t.valid], minlength=16 * 128)
    assert sorted(counts[counts > 0].tolist()) == [2, 3, 19, 257, 4096]
    one = P.model(P.clouds(16, 128, which=("one_pixel",))["one_pixel"], 16, 128)
    assert (one.index >= 0).sum() == 1 and one.valid.all() and one.index.max() == 1000 - 3
    lidar = cl["lidar"]
    for name, c in P.padded_cases(lidar).items():
        v = int(name.split("V")[1])
        assert np.isnan(c[v:]).all() and np.array_equal(c[:v], lidar[:v])
