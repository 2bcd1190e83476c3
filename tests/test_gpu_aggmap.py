"""`-m gpu`: the aggregated world map (icp_aggmap_*, IcpContext.aggregated_map, the plugin's `aggregate_map_voxel`;
csrc/aggmap.hip) against the numpy bit model of tests/aggmap_audit.py — BIT FOR BIT, no tolerance, on every array (float64
world points, float32 points, hits, first and last frames, submap rows and indices) and every counter: the wave and
workgroup edges of n, the voxel layouts, half-to-even ties, the poses, the rows set aside, probe chains built through the
model's slot function, the capacity, several inserts and windows, host and device memory, two maps on one context, an
insert inside a launched registration, and the plugin paths.  No deliberately wrong kernel runs here: the wrong readings of
the specification are caught on the CPU (tests/test_aggmap_audit.py).

Measured on an MI355X: 31 tests in 3 s, no array or counter differs from the model."""
import numpy as np
import pytest

import aggmap_audit as A

pytestmark = pytest.mark.gpu

EYE = np.eye(4)


def _pose(yaw=0.0, pitch=0.0, t=(0.0, 0.0, 0.0)):
    cz, sz, cy, sy = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    m = np.eye(4)
    m[:3, :3] = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    m[:3, 3] = t
    return m


YAW3 = _pose(3.0)
FAR = _pose(0.7, 0.05, (10000.0, -10000.0, 50.0))


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


def _same(gm, model, origin=None, what=""):
    """every array and counter of the device map equals the model's, bit for bit"""
    st = gm.stats()
    assert st == model.stats(), (what, st, model.stats())
    w = gm.points(dtype=np.float64)
    assert w.dtype == np.float64 and w.shape == model.w.shape and np.array_equal(_bits(w), _bits(model.w)), (what, "world points")
    xyz, hits, first, last = gm._get(origin)
    want = model.points(origin)
    assert xyz.dtype == np.float32 and np.array_equal(_bits(xyz), _bits(want)), (what, "float32 points")
    assert hits.dtype == np.uint32 and np.array_equal(hits, model.hits), (what, "hits")
    assert first.dtype == np.int32 and np.array_equal(first, model.first_frame), (what, "first_frame")
    assert last.dtype == np.int32 and np.array_equal(last, model.last_frame), (what, "last_frame")


def _pair(ctx, voxel, capacity, rows):
    return ctx.aggregated_map(voxel, capacity, rows), A.AggMapModel(voxel, capacity, rows)


def _both(gm, model, points, pose, frame):
    gm.insert(points, pose, frame)
    model.insert(points, pose, frame)


def _cloud(n, seed, spread=20.0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * np.array([spread, spread, 2.0])).astype(np.float32)


# ---- row counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1025, 65537])
def test_row_counts(ctx, n):
    """wave, workgroup and multi-workgroup edges of one insert; a second insert of the same size overlaps the first"""
    gm, model = _pair(ctx, 0.5, 140000, 65537)
    _both(gm, model, _cloud(n, 1), YAW3, 3)
    _same(gm, model, what=("first", n))
    _both(gm, model, np.concatenate([_cloud(n, 2)[: n // 2], _cloud(n, 1)[n // 2:]]), YAW3, 1)
    _same(gm, model, what=("second", n))
    assert (model.size > n // 2 or n == 0) and model.stats() == dict(model.stats(), inserts=2, dropped=0, nonfinite=0)
    gm.close()


def test_more_rows_than_the_map_takes_are_refused_before_any_launch(ctx):
    gm, model = _pair(ctx, 0.5, 100, 64)
    _both(gm, model, _cloud(64, 3), EYE, 0)
    with pytest.raises(AssertionError, match="exceeds max_insert_rows"):
        gm.insert(_cloud(65, 3), EYE, 1)
    with pytest.raises(AssertionError, match="non-finite"):
        gm.insert(_cloud(5, 3), np.full((4, 4), np.nan), 1)
    with pytest.raises(AssertionError, match="frame_lo"):
        gm.submap(3, 2, EYE)
    _same(gm, model)
    gm.close()


# ---- voxel layouts ---------------------------------------------------------------------------------------------------------
def _layout(name):
    rng = np.random.default_rng(11)
    if name == "one_voxel":  # 1 000 different points of one voxel
        return (np.array([4.0, -6.0, 1.0]) + rng.uniform(-0.24, 0.24, (1000, 3))).astype(np.float32)
    if name == "own_voxels":  # every row a voxel of its own
        g = np.stack(np.meshgrid(np.arange(10), np.arange(10), np.arange(10), indexing="ij"), -1).reshape(-1, 3)
        return (rng.permutation(g) * 0.5 + rng.uniform(-0.2, 0.2, (1000, 3))).astype(np.float32)
    if name == "first_and_last_row":  # the same voxel at row 0 and at row n - 1, five workgroups apart
        p = (np.arange(1025)[:, None] * np.array([0.5, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, (1025, 3))).astype(np.float32)
        p[-1] = p[0] + np.float32(0.01)
        return p
    if name == "straddling_groups":  # runs of 7 and of 100 rows per voxel: groups cut by wave and workgroup edges
        runs = np.concatenate([np.repeat(np.arange(100), 7), np.repeat(np.arange(100, 110), 100), np.repeat(np.arange(50), 3)])
        return (runs[:, None] * np.array([0.5, 0.5, 0.0]) + rng.uniform(-0.2, 0.2, (len(runs), 3))).astype(np.float32)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["one_voxel", "own_voxels", "first_and_last_row", "straddling_groups"])
def test_voxel_layouts(ctx, name):
    gm, model = _pair(ctx, 0.5, 4096, 4096)
    p = _layout(name)
    _both(gm, model, p, EYE, 0)
    _same(gm, model, what=name)
    if name == "one_voxel":
        assert model.size == 1 and model.hits[0] == 1000 and np.array_equal(model.w[0], p[0].astype(np.float64))
    if name == "own_voxels":
        assert model.size == 1000 and np.array_equal(model.w, p.astype(np.float64))
    if name == "first_and_last_row":
        assert model.size == 1024 and model.hits[0] == 2
    _both(gm, model, p[::-1].copy(), EYE, 1)  # the same voxels again, in reverse: nothing is created, every voxel is hit
    _same(gm, model, what=(name, "reversed"))
    gm.close()


# ---- rounding --------------------------------------------------------------------------------------------------------------
def test_half_to_even_ties_and_their_neighbours(ctx):
    """points exactly on (k + 0.5) voxels (voxel 0.5: the quotient is exact), with copies 1 to 3 ulp either side, on every
    axis; positive and negative k, -0.5 and +0.5 among them"""
    rows = []
    for k in (-1001, -1000, -3, -2, -1, 0, 1, 2, 1000, 1001):
        tie = np.float32((k + 0.5) * 0.5)
        near = [tie]
        lo = hi = tie
        for _ in range(3):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            near += [lo, hi]
        for axis in range(3):
            for v in near:
                row = np.array([0.1, 0.1, 0.1], np.float32)
                row[axis] = v
                rows.append(row)
    p = np.array(rows, np.float32)
    c = A.voxel_coords_real(A.world_points(p, EYE), 0.5)
    assert {-1.0, 0.0} <= set(c[:, 0]) and np.any(c[:, 0] == -1000.0) and np.any(c[:, 0] == 1002.0)  # ties went to the even side
    gm, model = _pair(ctx, 0.5, 1024, 1024)
    _both(gm, model, p, EYE, 0)
    _same(gm, model)
    gm.close()


# ---- poses -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["identity", "yaw3", "far"])
def test_poses(ctx, name):
    pose = {"identity": EYE, "yaw3": YAW3, "far": FAR}[name]
    gm, model = _pair(ctx, 0.2, 8192, 4096)
    _both(gm, model, _cloud(3000, 5), pose, 4)
    _both(gm, model, _cloud(3000, 5) + np.float32(0.05), pose, 5)
    _same(gm, model, origin=pose[:3, 3], what=name)
    xyz, idx = gm.submap(4, 5, np.linalg.inv(pose))
    want_xyz, want_idx = model.submap(4, 5, np.linalg.inv(pose))
    assert np.array_equal(_bits(xyz), _bits(want_xyz)) and np.array_equal(idx, want_idx) and len(idx) > 2000
    gm.close()


# ---- special rows ----------------------------------------------------------------------------------------------------------
def test_rows_set_aside(ctx):
    """NaN and infinite rows, the range edges -2^20 and 2^20 - 1 and one beyond (voxel 1), ties at the edges, and a pose that
    makes finite rows overflow or cancel to NaN"""
    e = float(1 << 20)
    p = np.array([[np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1, 2, 3],
                  [-e, 0, 0], [e - 1, 0, 0], [e, 0, 0], [-e - 1, 0, 0], [0, -e, e - 1], [0, e, 0], [0, 0, -e - 1],
                  [e - 0.5, 5, 5], [-e - 0.5, 5, 5], [e - 1.5, 6, 6], [1, 2, 3.2], [3.0e38, 0, 0]], np.float32)
    gm, model = _pair(ctx, 1.0, 64, 64)
    _both(gm, model, p, EYE, 0)
    _same(gm, model, what="identity")
    st = model.stats()
    assert st["nonfinite"] == 3 and st["out_of_range"] == 6 and st["size"] == 6 and model.hits.sum() == 7
    big = np.eye(4)
    big[0, 0], big[1, 0], big[1, 1] = 1.0e300, 1.0e300, -1.0e300
    q = np.array([[1.0e30, 0, 0], [1.0e30, 1.0e30, 0], [0, 0, 1], [1.0e-30, 0, 2]], np.float32)
    _both(gm, model, q, big, 1)
    _same(gm, model, what="overflow")
    assert model.stats()["nonfinite"] == 5 and model.stats()["out_of_range"] == 7
    tiny, tiny_model = _pair(ctx, 1.0e-300, 8, 8)  # (a quotient that overflows is out of range, not undefined)
    _both(tiny, tiny_model, np.array([[1, 1, 1], [0, 0, 0]], np.float32), EYE, 0)
    _same(tiny, tiny_model, what="tiny voxel")
    assert tiny_model.stats()["out_of_range"] == 1 and tiny_model.size == 1
    gm.close()
    tiny.close()


# ---- probing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["chain", "wrap", "wave"])
def test_probe_chains_built_through_the_slot_function(ctx, case):
    """small maps (C = 8 .. 64, R = 64: 256 slots) whose keys start their probe chains in ONE slot: a chain of 12, a chain that
    wraps past the last slot, and a 64-lane wave whose 64 keys all land in one slot"""
    capacity, count, target = {"chain": (16, 12, 77), "wrap": (8, 7, 255), "wave": (64, 64, 130)}[case]
    slots = A.slot_count(capacity, 64)
    assert slots == 256
    c = A.colliding_keys(slots, target, count)
    assert len(np.unique(A.pack_keys(c))) == count and np.all(A.slot_of_keys(A.pack_keys(c), slots) == target)
    gm, model = _pair(ctx, 1.0, capacity, 64)
    p = A.voxel_centres(c, 1.0)
    assert np.array_equal(A.voxel_coords_real(p.astype(np.float64), 1.0), c)
    _both(gm, model, p, EYE, 0)
    _same(gm, model, what=case)
    assert model.size == min(count, capacity) and model.stats()["error"] == 0
    _both(gm, model, p[::-1].copy(), EYE, 1)  # every key is found again at the end of its chain
    _same(gm, model, what=(case, "again"))
    assert np.all(model.hits == 2) and np.all(model.last_frame == 1)
    gm.close()


# ---- capacity --------------------------------------------------------------------------------------------------------------
def _voxel_rows(ids, per, seed):
    """`per` rows in each of the voxels `ids` (voxel 1, along x and y), shuffled"""
    rng = np.random.default_rng(seed)
    ids = np.repeat(np.asarray(ids), per)
    p = np.stack([ids % 37, ids // 37, np.zeros_like(ids)], 1) + rng.uniform(-0.4, 0.4, (len(ids), 3))
    return rng.permutation(p).astype(np.float32)


def test_capacity_edges_full_map_clear_and_reuse(ctx):
    gm, model = _pair(ctx, 1.0, 100, 1024)
    _both(gm, model, _voxel_rows(range(99), 3, 1), EYE, 10)      # ends at C - 1
    _same(gm, model, what="C - 1")
    assert model.size == 99
    _both(gm, model, _voxel_rows(range(98, 100), 2, 2), EYE, 11)  # ends at C
    _same(gm, model, what="C")
    assert model.size == 100 and model.stats()["dropped"] == 0
    # three more inserts into the full map: stored voxels keep counting, unknown ones are dropped
    _both(gm, model, _voxel_rows(range(90, 120), 4, 3), EYE, 12)
    _both(gm, model, _voxel_rows(range(0, 10), 5, 4), EYE, 3)
    _both(gm, model, _voxel_rows(range(100, 300), 1, 5), EYE, 13)
    _same(gm, model, what="full")
    assert model.stats()["dropped"] == 20 * 4 + 200 and int(model.hits.sum()) == 99 * 3 + 4 + 10 * 4 + 10 * 5
    assert model.last_frame.max() == 12 and np.sum(model.last_frame == 10) == 90 and np.all(model.first_frame[:99] == 10)
    gm.clear()
    model.clear()
    _same(gm, model, what="cleared")
    # an insert that crosses C in its middle: the first voxels in row order are stored, the others stay unstored for good
    _both(gm, model, _voxel_rows(range(60), 2, 6), EYE, 0)
    crossing = _voxel_rows(range(30, 130), 3, 7)
    _both(gm, model, crossing, EYE, 1)
    _same(gm, model, what="crossing")
    assert model.size == 100 and model.stats()["dropped"] == 30 * 3 and len(model.unstored) == 30
    _both(gm, model, crossing[::-1].copy(), EYE, 2)  # rows in the unstored voxels are dropped again
    _same(gm, model, what="after crossing")
    assert model.stats()["dropped"] == 2 * 30 * 3
    gm.close()


# ---- several inserts, windows, origin --------------------------------------------------------------------------------------
def test_six_overlapping_inserts_windows_and_origin(ctx):
    gm, model = _pair(ctx, 0.3, 30000, 4096)
    frames = [5, 2, 9, 2, 7, 0]
    for k, f in enumerate(frames):
        _both(gm, model, _cloud(4000, 20 + k % 4, spread=6.0) + np.float32(0.4 * k), _pose(0.1 * k, 0.0, (0.5 * k, 0.0, 0.0)), f)
    _same(gm, model, origin=(1.5, -2.25, 0.125), what="six inserts")
    assert model.stats()["inserts"] == 6 and set(model.first_frame) == set(frames) and np.any(model.last_frame > model.first_frame)
    back = np.linalg.inv(_pose(0.2, 0.0, (1.0, 0.0, 0.0)))
    for lo, hi in ((3, 3), (0, 10), (2, 3), (9, 10), (10, 50), (-5, 0), (6, 9)):
        xyz, idx = gm.submap(lo, hi, back)
        want_xyz, want_idx = model.submap(lo, hi, back)
        assert xyz.dtype == np.float32 and idx.dtype == np.int32
        assert np.array_equal(idx, want_idx) and np.array_equal(_bits(xyz), _bits(want_xyz)), (lo, hi)
    assert len(model.submap(3, 3, back)[1]) == 0 and len(model.submap(0, 10, back)[1]) == model.size
    assert 0 < len(model.submap(2, 3, back)[1]) < model.size and np.all(np.diff(model.submap(6, 9, back)[1]) > 0)
    gm.close()


# ---- memory and contexts ---------------------------------------------------------------------------------------------------
def test_host_and_device_rows_and_two_maps_on_one_context(ctx, torch_cuda):
    torch = torch_cuda
    a, model_a = _pair(ctx, 0.5, 16384, 4096)
    b, model_b = _pair(ctx, 0.25, 16384, 4096)
    for k in range(4):
        p = _cloud(3000, 30 + k, spread=8.0)
        dev = torch.from_numpy(p).to(ctx.device)
        a.insert(dev if k % 2 else p, YAW3, k)
        b.insert(p if k % 2 else dev, YAW3, k)
        model_a.insert(p, YAW3, k)
        model_b.insert(p, YAW3, k)
    _same(a, model_a, what="map a")
    _same(b, model_b, what="map b")
    assert model_b.size > model_a.size
    a.close()
    b.close()


def test_insert_inside_a_launched_registration_leaves_it_bit_equal(torch_cuda):
    from pylidar_slam_amd.engine import IcpContext
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    scans, _ = make_sequence(SceneConfig(height=16, width=128), 2)
    results = []
    for with_insert in (False, True):
        c = IcpContext(height=16, width=128, max_num_alignments=6, threshold_delta_pose=0.0)
        c.map_set(scans[0])
        gm, model = _pair(c, 0.2, 8192, 4096)
        c.register_launch(scans[1])
        if with_insert:
            _both(gm, model, scans[1], YAW3, 1)
        res = c.register_end()
        _same(gm, model, what="inside a registration")
        results.append(res)
        c.close()
    plain, mixed = results
    assert plain.iterations == mixed.iterations == 6
    assert np.array_equal(_bits(plain.pose), _bits(mixed.pose)) and np.array_equal(_bits(plain.losses), _bits(mixed.losses))
    assert np.array_equal(_bits(plain.dx), _bits(mixed.dx))


# ---- plugin ----------------------------------------------------------------------------------------------------------------
DRIVE_FRAMES = 12


def _drive(seed=1234):
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    return make_sequence(SceneConfig(height=16, width=128, seed=seed), DRIVE_FRAMES)[0]


def _plugin_config(**over):
    from pylidar_slam_amd.odometry import MI355XICPConfig
    kw = dict(max_num_alignments=6, threshold_delta_pose=0.0, threshold_trans=0.7, threshold_rot=10.0, data_key="numpy_pc",
              local_map=dict(type="kdtree_local_map", local_map_size=3, num_neighbors_normals=10))
    kw.update(over)
    return MI355XICPConfig(**kw)


def _model_of_run(dicts, absolute_poses, voxel, capacity, rows):
    model = A.AggMapModel(voxel, capacity, rows)
    for f, d in enumerate(dicts):
        if "odometry_pc" in d:
            model.insert(d["odometry_pc"], absolute_poses[f], f)
    return model


def _run_single(torch, scans, as_tensor=False, **over):
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    odo = our.MI355XICPFrameToModel(_plugin_config(**over), projector=our.SphericalProjector(16, 128), device=dev)
    odo.init()
    dicts = []
    for s in scans:
        d = {over.get("data_key", "numpy_pc"): torch.from_numpy(s).to(dev) if as_tensor else s}
        odo.process_next_frame(d)
        dicts.append(d)
    return odo, dicts


PROJECTIVE = dict(local_map=dict(type="projective_local_map", local_map_size=3, normals_kernel_size=5))


@pytest.mark.parametrize("path", ["per_call", "one_call_frame", "one_call_projective_frame"])
def test_plugin_map_equals_the_model_fed_with_its_own_outputs(torch_cuda, path):
    scans = _drive()
    flag = {"per_call": {}, "one_call_frame": dict(one_call_frame=True),
            "one_call_projective_frame": dict(one_call_projective_frame=True, **PROJECTIVE)}[path]
    on, dicts = _run_single(torch_cuda, scans, aggregate_map_voxel=0.25, aggregate_map_capacity=30000, **flag)
    off, _ = _run_single(torch_cuda, scans, **flag)
    assert off.aggregated_map is None and on.aggregated_map is not None
    assert np.array_equal(_bits(np.stack(on.absolute_poses)), _bits(np.stack(off.absolute_poses)))
    assert np.array_equal(_bits(on.get_relative_poses()), _bits(off.get_relative_poses()))
    model = _model_of_run(dicts, on.absolute_poses, 0.25, 30000, on.aggregated_map.max_insert_rows)
    _same(on.aggregated_map, model, what=path)
    st = model.stats()
    assert st["inserts"] == DRIVE_FRAMES - 1 and st["size"] > 2048 and st["dropped"] == 0 and st["nonfinite"] == 0
    assert set(model.first_frame) == set(range(1, DRIVE_FRAMES))


def test_batched_plugin_gives_every_member_the_map_of_its_single_run(torch_cuda):
    torch = torch_cuda
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    drives = [_drive(1234 + b) for b in range(3)]
    over = dict(aggregate_map_voxel=0.25, aggregate_map_capacity=30000, data_key="input_data")
    batch = our.MI355XICPFrameToModelBatch(_plugin_config(**over), 3, projector=our.SphericalProjector(16, 128), device=dev)
    batch.init()
    for f in range(DRIVE_FRAMES):
        batch.process_next_frames([{"input_data": torch.from_numpy(drives[b][f]).to(dev)} for b in range(3)])
    for b in range(3):
        single, dicts = _run_single(torch, drives[b], as_tensor=True, **over)
        member = batch.members[b]
        assert np.array_equal(_bits(np.stack(member.absolute_poses)), _bits(np.stack(single.absolute_poses))), b
        model = _model_of_run(dicts, single.absolute_poses, 0.25, 30000, single.aggregated_map.max_insert_rows)
        _same(single.aggregated_map, model, what=("single", b))
        _same(member.aggregated_map, model, what=("member", b))
        assert model.size > 2048
