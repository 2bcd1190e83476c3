"""`-m gpu`: the spherical projection and its z-buffer (csrc/projection.hip, csrc/projection_device.h) against the bit model of
tests/projection_audit.py — float coordinates, index map, vertex map and rows, BIT FOR BIT, no tolerance, on every entry
point: `project_pixels` (the exact path), `project` with the index (host arrays and device tensors), `project_rows` (padded
input), the batch (`IcpBatch.project` / `project_rows`, 1, 3 and 32 members), frame 0 of `frame_launch` and
`pmap_frame_launch`, and every step of one sequence that walks the z-buffer through each of its states.

The clouds (projection_audit): LiDAR-like rows that fall off the top and the bottom of the image; a point on every row and
column boundary k + 0.5 with copies 1, 2, 3 ulp either side (all in the refinement band, most exactly on a half: half to even);
points 1e-4 .. 1e-2 pixel off every boundary (the edge of the band); the image's own edges, the +-pi seam and the z axis; NaN,
inf, overflowing, subnormal and zero rows; range ties of 2, 257 and 4 096 points; NaN-padded frames.  The model flags no row
of any of them (asserted on the CPU by tests/test_projection_audit.py).

The large images (128 x 4096 / 8192 / 16384) decide whether the ABSOLUTE refinement band of 2e-3 pixel still covers the error
of the fast float32 path where one ulp of a column is 4.9e-4 or 9.8e-4 pixel: every pixel must equal the model, which
refines everywhere.

Measured on an MI355X: 35 tests in 3 s, NO coordinate, index, vertex or row differs from the model, 0 flagged.  Compared:
`project_pixels` 820 824 rows; `project` 377 034 rows and 491 520 pixels from host arrays and as many from device tensors,
46 528 rows on the small images either way; `project_rows` 95 870 rows, 940 032 pixels; 135 200 / 266 272 / 528 416 rows
and every pixel at 128 x 4096 / 8192 / 16384 (the constant band holds at all three widths: DESIGN.md, section 4);
`IcpBatch.project` and `project_rows` 179 060 rows each; the z-buffer sequence 36 321 rows over 90 112 pixels; frame 0 of the
two frame calls 9 450 rows each.  Rows whose sum of squares is subnormal are kept, as in the reference: the device does not
flush them.  A kernel trace of one run of this file names k_project (236 launches), k_project_resolve (246),
k_project_batch (28), k_project_resolve_batch (30), k_project_pixels (96) and k_zbuf_clear (67), and of the projective side
k_pm_project, k_pm_resolve, k_pm_project_targets and k_pm_iterate.
"""
import numpy as np
import pytest

import projection_audit as P

pytestmark = pytest.mark.gpu

FIGURES = {}
_CTX = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _ctx(h, w, up=3.0, down=-24.0, fresh=False, **kw):
    from pylidar_slam_amd.engine import IcpContext
    if fresh or kw:
        return IcpContext(height=h, width=w, up_fov=up, down_fov=down, **kw)
    key = (h, w, up, down)
    if key not in _CTX:
        _CTX[key] = IcpContext(height=h, width=w, up_fov=up, down_fov=down)
    return _CTX[key]


def _count(path, rows, pixels):
    f = FIGURES.setdefault(path, {"rows": 0, "pixels": 0})
    f["rows"] += int(rows)
    f["pixels"] += int(pixels)


def _hold_map(path, what, m, cloud, index=None, vmap=None, rows=None):
    def host(a):
        return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()
    pixels = P.check_map(host(index), host(vmap), host(rows), m, cloud, f"{path}, {what}")
    _count(path, m.n, pixels)


@pytest.fixture(scope="module", autouse=True)
def figures():
    yield
    for path, f in FIGURES.items():
        print(f"projection audit, {path}: {f['rows']} rows, {f['pixels']} pixels compared, 0 differ, 0 flagged")


# ---- project_pixels: the exact path -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fov", P.FOVS, ids=lambda f: f"fov{f[0]:g}_{f[1]:g}")
@pytest.mark.parametrize("h,w", P.IMAGES)
def test_project_pixels(torch_cuda, h, w, fov):
    ctx = _ctx(h, w, *fov)
    for name, cloud in P.pixel_cases(h, w, *fov).items():
        cloud = np.array(cloud, np.float32)  # (a writable copy: the clouds are shared and frozen)
        row, col, _, flagged = P.coordinates(cloud, h, w, *fov)
        got_row, got_col = ctx.project_pixels(cloud)
        P.check_bits(got_row, row, f"{h} x {w}, field of view {fov}, {name}: rows", flagged)
        P.check_bits(got_col, col, f"{h} x {w}, field of view {fov}, {name}: columns", flagged)
        _count("project_pixels", cloud.shape[0], 0)


# ---- project with the index -----------------------------------------------------------------------------------------------
def _project_both_ways(torch, ctx, path, what, cloud, h, w, up=3.0, down=-24.0):
    cloud = np.array(cloud, np.float32)  # (a writable copy: the clouds are shared and frozen)
    m = P.model(cloud, h, w, up, down)
    vmap, index = ctx.project(cloud, with_index=True)
    _hold_map(path + ", host arrays", what, m, cloud, index, vmap)
    dv, di = ctx.project(torch.from_numpy(cloud).cuda(), with_index=True)
    assert dv.is_cuda and di.is_cuda
    _hold_map(path + ", device tensors", what, m, cloud, di, dv)
    return m


@pytest.mark.parametrize("fov", P.FOVS, ids=lambda f: f"fov{f[0]:g}_{f[1]:g}")
def test_project_every_cloud(torch_cuda, fov):
    h, w = P.IMAGES[0]
    ctx = _ctx(h, w, *fov)
    for name, cloud in P.pixel_cases(h, w, *fov).items():
        _project_both_ways(torch_cuda, ctx, "project", f"{h} x {w}, field of view {fov}, {name}", cloud, h, w, *fov)


def test_project_boundaries_at_64x2048(torch_cuda):
    h, w = P.IMAGES[1]
    ctx = _ctx(h, w)
    for name, cloud in P.map_cases(h, w).items():
        _project_both_ways(torch_cuda, ctx, "project", f"{h} x {w}, {name}", cloud, h, w)


@pytest.mark.parametrize("h,w", P.SMALL_IMAGES)
def test_project_small_images(torch_cuda, h, w):
    """1 x 1, single rows and single columns; 255, 256 and 257 pixels: the edge of the resolve grid"""
    ctx = _ctx(h, w)
    for name, cloud in P.map_cases(h, w).items():
        _project_both_ways(torch_cuda, ctx, "project, small images", f"{h} x {w}, {name}", cloud, h, w)
    empty = np.zeros((0, 3), np.float32)
    vmap, index = ctx.project(empty, with_index=True)
    assert not vmap.any() and (index == -1).all() and vmap.shape == (3, h, w)


def test_project_no_points(torch_cuda):
    h, w = P.IMAGES[0]
    ctx = _ctx(h, w)
    empty = np.zeros((0, 3), np.float32)
    m = P.model(empty, h, w)
    lidar = np.array(P.map_cases(h, w)["lidar"])
    ctx.project(lidar)
    vmap, index = ctx.project(empty, with_index=True)
    _hold_map("project, n = 0", "behind a full cloud", m, empty, index, vmap)
    dv, di = ctx.project(torch_cuda.zeros((0, 3), dtype=torch_cuda.float32, device="cuda"), with_index=True)
    _hold_map("project, n = 0", "device tensor", m, empty, di, dv)
    vm, rows = ctx.project_rows(torch_cuda.zeros((0, 3), dtype=torch_cuda.float32, device="cuda"))
    _hold_map("project, n = 0", "project_rows", m, empty, None, vm, rows)


# ---- project_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", P.IMAGES)
def test_project_rows(torch_cuda, h, w):
    ctx = _ctx(h, w)
    cases = dict(P.map_cases(h, w))
    cases.update(P.padded_cases(P.pixel_cases(h, w, 3.0, -24.0)["lidar"]))
    for name, cloud in cases.items():
        cloud = np.array(cloud, np.float32)  # (a writable copy: the clouds are shared and frozen)
        m = P.model(cloud, h, w)
        t = torch_cuda.from_numpy(cloud).cuda()
        vmap, rows = ctx.project_rows(t)
        _hold_map("project_rows", f"{h} x {w}, {name}", m, cloud, None, vmap, rows)
        assert np.array_equal(vmap.cpu().numpy().view(np.uint32), ctx.project(t).cpu().numpy().view(np.uint32)), name
    # a padded frame with nothing in front of its NaN rows leaves an empty image
    assert not ctx.project_rows(torch_cuda.from_numpy(np.array(cases["padded_V0"])).cuda())[1].any()


# ---- large images: is the absolute band wide enough? ---------------------------------------------------------------------
@pytest.mark.parametrize("h,w", P.LARGE_IMAGES)
def test_large_images(torch_cuda, h, w):
    ctx = _ctx(h, w, fresh=True)
    for name, cloud in P.large_cases(h, w).items():
        cloud = np.array(cloud, np.float32)  # (a writable copy: the clouds are shared and frozen)
        m = P.model(cloud, h, w)
        dv, di = ctx.project(torch_cuda.from_numpy(cloud).cuda(), with_index=True)
        _hold_map(f"project at {h} x {w}", name, m, cloud, di, dv)
    ctx.close()


# ---- the batch --------------------------------------------------------------------------------------------------------------
def _batch(count):
    from pylidar_slam_amd.engine import IcpBatch
    h, w = P.IMAGES[0]
    ctxs = [_ctx(h, w, fresh=True) for _ in range(count)]
    return IcpBatch(ctxs), ctxs


def _hold_batch(torch, batch, clouds, models, what):
    h, w = P.IMAGES[0]
    dev = [torch.from_numpy(np.array(c, np.float32)).cuda() for c in clouds]
    outs = [torch.full((3, h, w), 7.0, dtype=torch.float32, device="cuda") for _ in clouds]
    batch.project(dev, outs)
    for b, (m, c, o) in enumerate(zip(models, clouds, outs)):
        _hold_map("batch.project", f"{what}, member {b}", m, c, None, o)
    for b, (m, c, (vm, rows)) in enumerate(zip(models, clouds, batch.project_rows(dev))):
        _hold_map("batch.project_rows", f"{what}, member {b}", m, c, None, vm, rows)


@pytest.mark.parametrize("count", (1, 3, 32))
def test_batch(torch_cuda, count):
    """members of different lengths — one empty, one of NaN rows only, the longest last — twice in a row, and once more after
    one member has projected alone"""
    h, w = P.IMAGES[0]
    clouds = P.batch_members(count)
    models = [P.model(c, h, w) for c in clouds]
    batch, ctxs = _batch(count)
    _hold_batch(torch_cuda, batch, clouds, models, f"B = {count}, first")
    _hold_batch(torch_cuda, batch, clouds, models, f"B = {count}, again")
    alone = count // 2
    lidar = np.array(P.map_cases(h, w)["lidar"])
    vmap, index = ctxs[alone].project(lidar, with_index=True)
    _hold_map("project of a batch member", f"B = {count}", P.model(lidar, h, w), lidar, index, vmap)
    _hold_batch(torch_cuda, batch, clouds, models, f"B = {count}, after a single projection")
    # the members in reverse order: every z-buffer meets another cloud than the one it saw last
    back = clouds[::-1] if count > 1 else [np.array(P.map_cases(h, w)["ties"])]
    _hold_batch(torch_cuda, batch, back, [P.model(c, h, w) for c in back], f"B = {count}, other clouds")
    batch.close()


def test_batch_of_empty_members(torch_cuda):
    h, w = P.IMAGES[0]
    batch, ctxs = _batch(3)
    clouds = P.batch_members(3)
    _hold_batch(torch_cuda, batch, clouds, [P.model(c, h, w) for c in clouds], "before")
    empty = [np.zeros((0, 3), np.float32)] * 3
    _hold_batch(torch_cuda, batch, empty, [P.model(c, h, w) for c in empty], "every member empty")
    batch.close()


# ---- the z-buffer through its states ---------------------------------------------------------------------------------------
def test_z_buffer_states(torch_cuda):
    """One context, one sequence, every projection held to the model: (1) a dense cloud, (2) a 10-point cloud, (3) with the
    index, (4) pmap_update + pmap_register with threshold 0 (the projective iteration leaves its keys in the z-buffer),
    (5) a sparse cloud that wins no pixel against those keys, (6) the same context as a member of a batch, (7) alone again,
    (8) pmap_nearest_neighbor_search (keys again), (9) project."""
    from pylidar_slam_amd.engine import IcpBatch
    torch = torch_cuda
    h, w = P.STATE_IMAGE
    cl = {k: np.array(v) for k, v in P.state_clouds().items()}
    models = {k: P.model(v, h, w) for k, v in cl.items()}
    dev = {k: torch.from_numpy(v).cuda() for k, v in cl.items()}
    kw = dict(max_num_alignments=5, threshold_delta_pose=0.0, local_map_size=3)
    ctx, other = _ctx(h, w, **kw), _ctx(h, w, **kw)

    def hold(step, name, index=None, vmap=None, rows=None):
        _hold_map("z-buffer sequence", f"step {step}, {name}", models[name], cl[name], index, vmap, rows)
    vm0 = ctx.project(dev["scan0"])                                      # 1
    hold(1, "scan0", None, vm0)
    hold(2, "ten", None, ctx.project(dev["ten"]))                        # 2
    vmap, index = ctx.project(cl["scan1"], with_index=True)              # 3
    hold(3, "scan1", index, vmap)
    ctx.pmap_init()                                                      # 4
    ctx.pmap_update(np.eye(4, dtype=np.float32), vm0)
    ctx.pmap_register(dev["scan1"], None)
    vmap, index = ctx.project(cl["sparse"], with_index=True)             # 5
    hold(5, "sparse", index, vmap)
    ctx.pmap_register(dev["scan1"], None)
    batch = IcpBatch([other, ctx])                                       # 6
    outs = [torch.empty((3, h, w), dtype=torch.float32, device="cuda") for _ in range(2)]
    batch.project([dev["scan2"], dev["sparse"]], outs)
    hold(6, "scan2", None, outs[0])
    hold(6, "sparse", None, outs[1])
    (v0, r0), (v1, r1) = batch.project_rows([dev["ten"], dev["scan0"]])
    hold(6, "ten", None, v0, r0)
    hold(6, "scan0", None, v1, r1)
    vmap, index = ctx.project(dev["ten"], with_index=True)               # 7
    hold(7, "ten", index, vmap)
    ctx.pmap_nearest_neighbor_search(dev["scan2"])                       # 8
    vmap, rows = ctx.project_rows(dev["sparse"])                         # 9
    hold(9, "sparse", None, vmap, rows)
    vmap, index = ctx.project(cl["ten"], with_index=True)
    hold(9, "ten", index, vmap)
    batch.close()


# ---- frame 0 of the frame calls ----------------------------------------------------------------------------------------------
def _row_keys(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))
    return np.sort(a.view(np.dtype((np.void, 12))).reshape(-1))


@pytest.mark.parametrize("cloud", ("image_edge", "ties"))
@pytest.mark.parametrize("device_rows", (False, True), ids=("numpy", "cuda"))
def test_frame_0_holds_the_models_pixels(torch_cuda, cloud, device_rows):
    """frame 0 of `frame_launch` (targets = pixels) and of `pmap_frame_launch`, rows in: the map holds exactly the model's
    occupied pixels"""
    h, w = P.IMAGES[0]
    pts = np.array(P.map_cases(h, w)[cloud])
    m = P.model(pts, h, w)
    frame = torch_cuda.from_numpy(pts).cuda() if device_rows else pts
    ctx = _ctx(h, w, fresh=True)
    ctx.odometry_init(targets=1)
    ctx.frame_launch(frame)
    r = ctx.frame_end()
    assert r.frame_index == 0
    want = m.rows[m.index.reshape(-1) >= 0]
    got = ctx.map_points()
    assert got.shape == want.shape and np.array_equal(_row_keys(got), _row_keys(want)), (cloud, got.shape, want.shape)
    _count("frame 0, frame_launch", m.n, h * w)
    ctx.close()
    ctx = _ctx(h, w, fresh=True)
    ctx.pmap_odometry_init(targets=1)
    ctx.pmap_frame_launch(frame)
    r = ctx.pmap_frame_end()
    assert r.frame_index == 0 and ctx.pmap_num_maps() == 1
    P.check_bits(ctx.pmap_model()[0][0], m.vmap, f"pmap frame 0, {cloud}")
    _count("frame 0, pmap_frame_launch", m.n, h * w)
    ctx.close()
