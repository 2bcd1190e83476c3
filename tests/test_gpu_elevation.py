"""`-m gpu`: the elevation image (icp_elevation_*, IcpContext.elevation_image, AggregatedMap.elevation; csrc/elevation.hip)
against the numpy bit model of tests/elevation_audit.py — BIT FOR BIT, no tolerance, on every array (colour, theta, the
float32 point and the row behind every pixel) and every counter, for float32 and float64 rows: the workgroup edges of n, five
image shapes, every pixel boundary ± 3 ulp, the image edges, the clip bounds ± 1 ulp, ±inf and the two zeros, ties of up to
4 096 rows, heights below float32 resolution, flip and three z_min, NaN in each coordinate, host and device rows and outputs,
reuse, two images on one context, a build inside a launched registration, windows of an aggregated map and the drop-in
`build_image`.  No deliberately wrong kernel runs here: the wrong readings of the specification are caught on the CPU
(tests/test_elevation_audit.py).

Measured on an MI355X: 50 tests in 3 s, no array or counter differs from the model."""
import numpy as np
import pytest

import aggmap_audit as G
import elevation_audit as A

pytestmark = pytest.mark.gpu

TABLE = A.random_table(3)
DTYPES = [np.float32, np.float64]
SHAPES = {(1, 1): 30.0, (1, 300): 0.4, (5, 7): 8.0, (255, 1): 0.4, (400, 400): 0.4}  # image -> pixel size


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
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _image(ctx, spec, rows=70000, table=TABLE):
    return ctx.elevation_image(spec.height, spec.width, spec.pixel_size, spec.z_min, spec.z_max, spec.flip, table, rows)


def _same(img, want, what=""):
    """every array and counter of the device image equals the model's, bit for bit"""
    st = img.stats()
    assert st == want["stats"], (what, st, want["stats"])
    index = img.indices
    assert index.dtype == np.int32 and np.array_equal(index, want["index"]), (what, "indices", int((index != want["index"]).sum()))
    theta = img.theta
    assert theta.dtype == np.float32 and np.array_equal(_bits(theta), _bits(want["theta"])), (what, "theta")
    points = img.points_3d
    assert points.dtype == np.float32 and np.array_equal(_bits(points), _bits(want["points"])), (what, "points")
    rgb = img.rgb
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, want["rgb"]), (what, "rgb")


def _check(ctx, spec, points, what="", rows=70000):
    img = _image(ctx, spec, rows)
    img.build(points)
    want = A.build(points, spec, TABLE)
    _same(img, want, what)
    img.close()
    return want


# ---- sizes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 65537])
def test_row_counts_and_image_shapes(ctx, n, dtype):
    cloud = A.tied_cloud(n, 100 + n, dtype)
    filled = 0
    for (h, w), pixel in SHAPES.items():
        want = _check(ctx, A.Spec(h, w, pixel, 0.0, 5.0, False), cloud, (n, h, w))
        filled += want["stats"]["filled_pixels"]
    assert filled == 0 if n == 0 else (n == 1 or filled > 0)


# ---- pixel boundaries and image edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(5, 7), (400, 400), (1, 300)])
def test_every_pixel_boundary_and_its_neighbours(ctx, shape, dtype):
    spec = A.Spec(shape[0], shape[1], 0.4, 0.0, 5.0, False)
    cloud = A.boundary_cloud(spec, dtype)
    want = _check(ctx, spec, cloud, shape)
    assert want["stats"]["rows_outside"] > 0 and want["stats"]["rows_in_image"] > 0
    exact = A.Spec(shape[0], shape[1], 0.5, 0.0, 5.0, False)  # (k + 0.5 - half) * 0.5 and its quotient are exact: true half-way cases
    _check(ctx, exact, A.boundary_cloud(exact, dtype), (shape, "exact"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", [6, 7])
def test_image_edges(ctx, h, dtype):
    """rows that round to -1, 0, H - 1, H; -0.5 rounds to -0 and is pixel 0; H - 0.5 is outside for even H, pixel H - 1 for odd"""
    spec = A.Spec(h, 3, 0.5, 0.0, 5.0, False)
    cells = np.array([-1.0, -0.5, -0.25, 0.0, h - 1.0, h - 0.5, h - 0.0, -0.75, h - 0.75])
    p = np.zeros((len(cells), 3), dtype)
    p[:, 0] = (cells - h // 2) * 0.5
    p[:, 2] = [1.0, 1.1, 1.2, 1.3, 2.0, 3.0, 1.0, 1.0, 1.5]
    want = _check(ctx, spec, p, h)
    assert want["index"][0, 1] == 3 and want["index"][h - 1, 1] == (5 if h % 2 else 4)
    assert want["stats"]["rows_outside"] == (3 if h % 2 else 4) and want["stats"]["filled_pixels"] == 2
    q = p[:, [1, 0, 2]].copy()  # the same along the columns of a [3, h] image
    _check(ctx, A.Spec(3, h, 0.5, 0.0, 5.0, False), q, (h, "columns"))


# ---- heights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flip", [False, True])
def test_clip_bounds_infinities_and_zeros(ctx, flip, dtype):
    dt = np.dtype(dtype).type
    lo, hi = dt(-2.0), dt(5.0)
    zs = [lo, np.nextafter(lo, dt(np.inf)), np.nextafter(lo, dt(-np.inf)), dt(-7.0), hi, np.nextafter(hi, dt(-np.inf)),
          np.nextafter(hi, dt(np.inf)), dt(9.0), dt(np.inf), dt(-np.inf), dt(0.0), dt(-0.0)]
    rows = [(k, z) for k, z in enumerate(zs)]                       # every height alone in a pixel
    base = len(zs)
    pairs = [(10, 11), (11, 10), (8, 6), (6, 8), (9, 3), (3, 9), (0, 2), (2, 0), (4, 5), (1, 0), (8, 4), (9, 0)]
    for j, (a, b) in enumerate(pairs):                               # and in pairs: both orders decide the tie by the row
        rows += [(base + j, zs[a]), (base + j, zs[b])]
    p = np.zeros((len(rows), 3), dtype)
    p[:, 1] = (np.array([r[0] for r in rows]) - 15) * 0.5
    p[:, 2] = np.array([r[1] for r in rows], dtype)
    spec = A.Spec(3, 31, 0.5, -2.0, 5.0, flip)
    want = _check(ctx, spec, p, flip)
    row = want["index"][1]
    assert row[base + 0] == base + 1 and row[base + 1] == base + 3  # -0.0 and +0.0 tie: the higher row, whichever zero it holds
    assert row[base + 2] == base + 5 and row[base + 3] == base + 7  # +inf and a finite height beyond z_max tie at z_max
    assert want["stats"]["filled_pixels"] == base + len(pairs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ties_of_many_rows_and_a_cloud_clipped_to_one_height(ctx, dtype):
    rng = np.random.default_rng(5)
    spec = A.Spec(5, 7, 0.4, 0.0, 5.0, False)
    parts = []
    for k, count in enumerate((2, 257, 4096)):  # equal raw heights, equal clipped heights above z_max, and below z_min
        p = np.zeros((count, 3), dtype)
        p[:, 1] = (k - 1) * 0.4
        p[:, 2] = (2.5, 6.0, -4.0)[k] + (rng.uniform(0, 3, count) if k else 0.0)
        parts.append(p)
    cloud = np.concatenate(parts)[rng.permutation(2 + 257 + 4096)]
    for flip in (False, True):
        want = _check(ctx, A.Spec(5, 7, 0.4, 0.0, 5.0, flip), cloud, flip)
        for k in range(3):
            mine = np.flatnonzero(np.isclose(cloud[:, 1], (k - 1) * 0.4))
            assert want["index"][2, 2 + k] == mine.max()
    high = A.tied_cloud(5000, 9, dtype)
    high[:, 2] = np.abs(high[:, 2]) + 5.5
    want = _check(ctx, A.Spec(400, 400, 0.4, 0.0, 5.0, False), high, "all at z_max")
    assert np.all(want["theta"][want["index"] >= 0] == 1.0) and want["stats"]["filled_pixels"] > 3000


def test_float64_heights_that_differ_below_float32_resolution(ctx):
    points, spec = A.edge_clouds(np.float64)["below_float32"]
    want = _check(ctx, spec, points)
    assert want["index"][2, 3] == 0 and want["index"][3, 3] == 4
    assert np.unique(points[:, 2].astype(np.float32)).size == 1
    flipped = A.Spec(spec.height, spec.width, spec.pixel_size, spec.z_min, spec.z_max, True)
    assert _check(ctx, flipped, points)["index"][3, 3] == 3


# ---- configurations --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("z_min", [-2.0, 0.0, 0.5])
def test_flip_z_min_and_nan_in_each_coordinate(ctx, z_min, flip, dtype):
    cloud = A.tied_cloud(20000, 21, dtype)
    cloud[::97, 0] = np.nan
    cloud[1::97, 1] = np.nan
    cloud[2::97, 2] = np.nan
    cloud[3::97, 0], cloud[4::97, 1] = np.inf, -np.inf
    cloud[5::97] = np.nan
    want = _check(ctx, A.Spec(300, 200, 0.4, z_min, 5.0, flip), cloud, (z_min, flip))
    st = want["stats"]
    assert st["rows_nan_z"] > 100 and st["rows_outside"] > 800 and sum(st[k] for k in ("rows_in_image", "rows_outside", "rows_nan_z")) == 20000
    assert np.all(want["theta"][want["index"] < 0] == np.float32(z_min))


# ---- memory, reuse, contexts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_and_device_rows_and_outputs(ctx, torch_cuda, dtype):
    torch = torch_cuda
    spec = A.Spec(400, 400, 0.4, 0.0, 5.0, False)
    cloud = A.tied_cloud(30000, 31, dtype)
    want = A.build(cloud, spec, TABLE)
    img = _image(ctx, spec)
    img.build(torch.from_numpy(cloud).to(ctx.device))
    _same(img, want, "device rows")
    rgb, theta, points, index = img.device()
    assert rgb.is_cuda and rgb.dtype == torch.uint8 and index.dtype == torch.int32 and tuple(points.shape) == (400, 400, 3)
    assert np.array_equal(rgb.cpu().numpy(), want["rgb"]) and np.array_equal(index.cpu().numpy(), want["index"])
    assert np.array_equal(_bits(theta.cpu().numpy()), _bits(want["theta"])) and np.array_equal(_bits(points.cpu().numpy()), _bits(want["points"]))
    (only,) = img.device("indices")
    assert np.array_equal(only.cpu().numpy(), want["index"])
    img.build(cloud)
    _same(img, want, "host rows")
    img.close()


def test_a_sparse_build_after_a_dense_one_and_two_images_on_one_context(ctx):
    spec_a, spec_b = A.Spec(400, 400, 0.4, 0.0, 5.0, False), A.Spec(101, 203, 0.7, -2.0, 3.0, True)
    a, b = _image(ctx, spec_a), _image(ctx, spec_b)
    _same(a, A.build(np.zeros((0, 3), np.float32), spec_a, TABLE), "never built")
    dense, sparse = A.tied_cloud(60000, 41), A.gaussian_cloud(50, 42)
    a.build(dense)
    b.build(dense.astype(np.float64))
    _same(a, A.build(dense, spec_a, TABLE), "a dense")
    a.build(sparse.astype(np.float64))
    _same(b, A.build(dense.astype(np.float64), spec_b, TABLE), "b dense")
    _same(a, A.build(sparse.astype(np.float64), spec_a, TABLE), "a sparse")
    b.build(sparse)
    a.build(np.zeros((0, 3), np.float32))
    _same(b, A.build(sparse, spec_b, TABLE), "b sparse")
    _same(a, A.build(np.zeros((0, 3), np.float32), spec_a, TABLE), "a empty")
    a.close()
    b.close()


def test_refusals_before_any_launch(ctx, torch_cuda):
    from pylidar_slam_amd.engine import IcpContext
    spec = A.Spec(5, 7, 0.4, 0.0, 5.0, False)
    img = _image(ctx, spec, rows=64)
    cloud = A.gaussian_cloud(64, 1, spread=1.0)
    img.build(cloud)
    with pytest.raises(AssertionError, match="exceeds max_rows"):
        img.build(A.gaussian_cloud(65, 1))
    other = IcpContext(height=16, width=128)
    foreign = other.aggregated_map(0.5, 100, 64)
    mine = ctx.aggregated_map(0.5, 100, 64)
    with pytest.raises(AssertionError, match="another context"):
        img.build_from(foreign, 0, 1, np.eye(4))
    with pytest.raises(AssertionError, match="non-finite"):
        img.build_from(mine, 0, 1, np.full((4, 4), np.inf))
    with pytest.raises(AssertionError, match="frame_lo"):
        img.build_from(mine, 2, 1, np.eye(4))
    for bad in (dict(pixel_size=0.0), dict(pixel_size=np.nan), dict(z_min=5.0), dict(z_max=np.inf), dict(height=0), dict(width=0),
                dict(height=1 << 16, width=1 << 15), dict(max_rows=0)):
        with pytest.raises(AssertionError, match="icp_elevation_create"):
            ctx.elevation_image(**{**dict(height=5, width=7, color_map=TABLE), **bad})
    _same(img, A.build(cloud, spec, TABLE), "after the refusals")
    img.close()
    other.close()
    mine.close()


def test_build_inside_a_launched_registration_leaves_it_bit_equal(torch_cuda):
    from pylidar_slam_amd.engine import IcpContext
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    scans, _ = make_sequence(SceneConfig(height=16, width=128), 2)
    spec = A.Spec(400, 400, 0.4, -2.0, 5.0, False)
    results = []
    for with_build in (False, True):
        c = IcpContext(height=16, width=128, max_num_alignments=6, threshold_delta_pose=0.0)
        c.map_set(scans[0])
        img = _image(c, spec)
        c.register_launch(scans[1])
        if with_build:
            img.build(scans[1])
            img.build(scans[1].astype(np.float64))
        res = c.register_end()
        _same(img, A.build(scans[1].astype(np.float64) if with_build else np.zeros((0, 3), np.float32), spec, TABLE), "inside")
        results.append(res)
        c.close()
    plain, mixed = results
    assert plain.iterations == mixed.iterations == 6
    assert np.array_equal(_bits(plain.pose), _bits(mixed.pose)) and np.array_equal(_bits(plain.losses), _bits(mixed.losses))
    assert np.array_equal(_bits(plain.dx), _bits(mixed.dx))


# ---- windows of an aggregated map --------------------------------------------------------------------------------------------
def _pose(yaw=0.0, pitch=0.0, t=(0.0, 0.0, 0.0)):
    cz, sz, cy, sy = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    m = np.eye(4)
    m[:3, :3] = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    m[:3, 3] = t
    return m


def _moved(w, pose):
    m, out = np.asarray(pose, np.float64).reshape(4, 4), np.empty(w.shape, np.float64)
    for i in range(3):
        out[:, i] = ((m[i, 0] * w[:, 0] + m[i, 1] * w[:, 1]) + m[i, 2] * w[:, 2]) + m[i, 3]
    return out


@pytest.mark.parametrize("far", [False, True])
def test_windows_of_a_map_of_six_inserts(ctx, far):
    """empty, single-frame and full windows; the identity and a 10 km pose; every filled pixel's point is submap's row"""
    anchor = _pose(0.7, 0.05, (10000.0, -10000.0, 50.0)) if far else np.eye(4)
    gm, model = ctx.aggregated_map(0.3, 30000, 4096), G.AggMapModel(0.3, 30000, 4096)
    frames = [5, 2, 9, 2, 7, 0]
    rng = np.random.default_rng(8)
    for k, f in enumerate(frames):
        p = (rng.standard_normal((4000, 3)) * np.array([25.0, 25.0, 2.0]) + np.array([0.4 * k, 0.0, 1.5])).astype(np.float32)
        pose = anchor @ _pose(0.1 * k, 0.0, (0.5 * k, 0.0, 0.0))
        gm.insert(p, pose, f)
        model.insert(p, pose, f)
    spec = A.Spec(200, 301, 0.4, 0.0, 5.0, False)
    img = _image(ctx, spec)
    back = np.linalg.inv(anchor @ _pose(0.2, 0.0, (1.0, 0.0, 0.0)))
    for lo, hi in ((3, 3), (2, 3), (0, 10), (6, 9), (10, 50)):
        assert gm.elevation(lo, hi, back, img) is img
        keep = (model.first_frame >= lo) & (model.first_frame < hi)
        want = A.build(_moved(model.w, back), spec, TABLE, keep=keep)
        _same(img, want, (lo, hi))
        xyz, idx = gm.submap(lo, hi, back)
        rows = np.full((model.size, 3), np.nan, np.float32)
        rows[idx] = xyz
        index, points = img.indices, img.points_3d
        filled = index >= 0
        assert np.array_equal(_bits(points[filled]), _bits(rows[index[filled]])), (lo, hi)
        assert want["stats"]["rows_in_image"] + want["stats"]["rows_outside"] == int(keep.sum()) == len(idx)
        assert (want["stats"]["filled_pixels"] > 1000) == ((lo, hi) in ((2, 3), (0, 10), (6, 9)))
    gm.insert(np.zeros((1, 3), np.float32), anchor, 2)  # the map grows: the next window reads the new size on the device
    model.insert(np.zeros((1, 3), np.float32), anchor, 2)
    img.build_from(gm, 2, 3, back)
    _same(img, A.build(_moved(model.w, back), spec, TABLE, keep=(model.first_frame == 2)), "after another insert")
    img.close()
    gm.close()


# ---- drop-in ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_build_image_returns_what_the_reference_returns(ctx, dtype):
    spec = A.Spec(400, 400, 0.4, 0.0, 5.0, False)
    cloud = A.tied_cloud(40000, 51, dtype)
    img = _image(ctx, spec)
    image, extra = img.build_image(cloud)
    want = A.build(cloud, spec, TABLE)
    assert sorted(extra) == ["pc_indices", "points_3D"]
    assert image.dtype == np.uint8 and image.shape == (400, 400, 3) and np.array_equal(image, want["rgb"])
    assert extra["pc_indices"].dtype == np.int64 and extra["pc_indices"].shape == (400, 400) and np.array_equal(extra["pc_indices"], want["index"])
    assert extra["points_3D"].dtype == np.float32 and np.array_equal(_bits(extra["points_3D"]), _bits(want["points"]))
    img.close()
