"""`-m gpu`: one library call per odometry frame (icp_odometry_init / icp_frame_launch / icp_frame_end,
include/icp_mi355x.h) against the per-call plugin `MI355XICPFrameToModel` on the same frames — bit for bit: the new calls
compose the plugin's own steps in the plugin's order — against the reference's loop (tests/golden/loop_reference.npz, the
bars of tests/test_gpu_loop.py), and on the edges and refusals of the new calls.

The drives and their key-frame thresholds live in tests/frame_cases.py; tests/test_frame_host.py checks on the CPU that no
frame of a drive sits near a threshold (so the float32 4x4 product of the library and numpy's cannot decide differently).

The plugin's preprocessing chain here is the device-resident one of config/slam/preprocessing/grid_sample_mi355x.yaml
(ToDevice -> Distortion -> GridSample(padded) -> ToTensor(float32)) with ONE change: Distortion writes to `deskewed`, not
`distorted`, so that the plugin copies the rows it registered out as `odometry_pc` (with a `distorted` entry it hands that
entry on instead, icp_odometry.py:210-211) — the copy-out is one of the ten steps the new calls replace."""
import numpy as np
import pytest

import frame_cases as FC
from test_loop_reference import golden_loop, loop_scans, published_config, trajectory_metrics  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


# ---- the two paths ---------------------------------------------------------------------------------------------------
def _filters(d, dev):
    from pylidar_slam_amd import odometry as our
    if d.targets == 0:
        return []
    return [our.ToDevice(our.ToDeviceConfig(device=str(dev)), device=dev),
            our.Distortion(our.DistortionConfig(pointcloud_key="pc_device", timestamps_key="timestamps_device",
                                                output_key="deskewed")),
            our.GridSample(our.GridSampleConfig(voxel_size=d.voxel_size, pointcloud_key="deskewed", padded=True)),
            our.ToTensor(our.ToTensorConfig(device=str(dev), keys={"sample_points": "input_data"}, dtype="float32"),
                         device=dev)]


def _frame_dict(d, f, scan=None):
    data = {"numpy_pc": d.scans[f] if scan is None else scan}
    if d.timestamps:
        data["numpy_pc_timestamps"] = d.stamps[f]
    return data


def _record(kind, **kw):
    return dict(kind=kind, **kw)


def _plugin_step(odo, filters, init, data, explicit_init=None):
    """One frame through the per-call (or one_call_frame) plugin: what the frame returned, or the error it raised."""
    from pylidar_slam_amd.engine import InvalidJacobianError
    init.next_frame(data)  # slam/slam.py:126-127
    if explicit_init is not None:
        data["init_rpose"] = explicit_init
    for flt in filters:
        flt.filter(data)
    first = odo._iter == 0
    try:
        odo.process_next_frame(data)
    except InvalidJacobianError as e:
        return _record("invalid_jacobian", num_targets=e.result.num_targets, iterations=e.result.iterations,
                       losses=e.result.losses)
    if first:
        return _record("first")
    init.save_real_motion(data["odometry_pose"], data)  # :139-140
    res = odo.last_result
    key = np.array_equal(odo._delta_since_map_update, EYE)  # (__update_map resets it on a key frame, :376)
    return _record("frame", pose=data["odometry_pose"], params=res.params, iterations=res.iterations, losses=res.losses,
                   dx=res.dx, key_frame=key, inserted=odo.local_map._last_count if key else 0,
                   odometry_pc=data["odometry_pc"])


def _library_step(ctx, scan, stamps=None, init_pose=None, **end):
    from pylidar_slam_amd.engine import InvalidJacobianError
    ctx.frame_launch(scan, stamps, init_pose)
    try:
        r = ctx.frame_end(**end)
    except InvalidJacobianError as e:
        return _record("invalid_jacobian", num_targets=e.result.num_targets, iterations=e.result.iterations,
                       losses=e.result.losses)
    if r.frame_index == 0:
        assert r.register.iterations == 0 and np.array_equal(r.pose, EYE) and r.key_frame and r.points is None
        return _record("first", samples=r.samples, inserted=r.inserted)
    g = r.register
    return _record("frame", pose=g.pose, params=g.params, iterations=g.iterations, losses=g.losses, dx=g.dx,
                   key_frame=r.key_frame, inserted=r.inserted, odometry_pc=r.points, samples=r.samples,
                   frame_index=r.frame_index)


def _make_plugin(torch, d, **over):
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    odo = our.MI355XICPFrameToModel(FC.plugin_config(d, **over), projector=our.SphericalProjector(d.height, d.width), device=dev)
    init = our.ConstantVelocityInitialization()
    odo.init()
    init.init()
    return odo, _filters(d, dev), init


def _make_context(d):
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(height=d.height, width=d.width, max_num_alignments=d.max_num_alignments,
                     threshold_delta_pose=d.threshold_delta_pose, local_map_size=d.local_map_size, num_neighbors_normals=10)
    ctx.set_cost(d.cost)
    return ctx


def _init_sequence(ctx, d, **over):
    kw = dict(voxel_size=d.voxel_size, threshold_trans=FC.THRESHOLD_TRANS, threshold_rot=FC.THRESHOLD_ROT,
              constant_velocity=True, targets=d.targets)
    kw.update(over)
    ctx.odometry_init(**kw)


def _same(a, b, what, skip=()):
    assert a["kind"] == b["kind"], (what, a["kind"], b["kind"])
    if a["kind"] == "invalid_jacobian":  # (the result up to and including the failing iteration)
        assert a["num_targets"] == b["num_targets"] and a["iterations"] == b["iterations"], (what, a, b)
        assert np.array_equal(a["losses"], b["losses"]), (what, a["losses"], b["losses"])
    if a["kind"] != "frame":
        return
    for k in ("pose", "params", "losses", "dx", "odometry_pc"):
        if k in skip:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(x, y), (what, k, np.abs(x.astype(np.float64) - y.astype(np.float64)).max())
    for k in ("iterations", "key_frame", "inserted"):
        assert a[k] == b[k], (what, k, a[k], b[k])


_PLUGIN_RUNS = {}


def _plugin_run(torch, name):
    """The drive through the per-call plugin, once per module: per-frame records, the final map and its cloud count."""
    if name not in _PLUGIN_RUNS:
        d = FC.drive(name)
        odo, filters, init = _make_plugin(torch, d)
        recs = [_plugin_step(odo, filters, init, _frame_dict(d, f)) for f in range(d.frames)]
        _PLUGIN_RUNS[name] = (recs, odo.ctx.map_points().copy(), odo.ctx.map_num_clouds(), odo.get_relative_poses(),
                              np.stack(odo.absolute_poses))
    return _PLUGIN_RUNS[name]


def _compare_drive(torch, name, min_each):
    d = FC.drive(name)
    want, want_map, want_clouds, _, _ = _plugin_run(torch, name)
    ctx = _make_context(d)
    _init_sequence(ctx, d)
    got = [_library_step(ctx, d.scans[f], d.stamps[f] if d.timestamps else None) for f in range(d.frames)]
    for f, (a, b) in enumerate(zip(got, want)):
        _same(a, b, (name, f))
        if f > 0:
            assert a["frame_index"] == f
            if d.voxel_size > 0:
                assert a["samples"] == a["odometry_pc"].shape[0] < d.scans[f].shape[0]
    keys = sum(1 for r in got[1:] if r["key_frame"])
    assert keys >= min_each and len(got) - 1 - keys >= min_each, (name, keys)
    assert np.array_equal(ctx.map_points(), want_map) and ctx.map_num_clouds() == want_clouds
    return got, ctx


# ---- 1-4: bit-equal to the per-call plugin -----------------------------------------------------------------------------
def test_sampled_drive_equals_the_plugin_bit_for_bit(torch_cuda):
    """32x1024, 10 frames from host arrays, grid sample 0.4 m, 8 forced iterations, a window of 3 clouds (evictions within
    the drive), targets = the pixels of the vertex map: per frame pose, parameters, iteration count, losses, steps,
    insertion, key-frame decision and odometry_pc; at the end the map and its cloud count.  At least two key frames and
    two pose-only frames."""
    got, ctx = _compare_drive(torch_cuda, "sampled", 2)
    assert all(r["iterations"] == 8 for r in got[1:])
    assert ctx.map_num_clouds() == 3 and sum(1 for r in got[1:] if r["key_frame"]) + 1 > 3  # evictions happened
    assert ctx.handoff_fallbacks() == 0


def test_live_stop_drive_equals_the_plugin_bit_for_bit(torch_cuda):
    """The same drive with the stop test live (|dx| < 1e-4, at most 15 iterations): chunked launches under the new calls."""
    got, _ = _compare_drive(torch_cuda, "sampled_live", 2)
    assert all(1 <= r["iterations"] <= 15 for r in got[1:]) and any(r["iterations"] < 15 for r in got[1:])


@pytest.mark.parametrize("name", ["raw", "raw_p2p"])
def test_raw_rows_drive_equals_the_plugin_bit_for_bit(torch_cuda, name):
    """No grid sample, targets = the frame's rows, 16x512 host arrays (8192 rows), 6 frames; both costs."""
    got, _ = _compare_drive(torch_cuda, name, 1)
    assert all(r["samples"] == 8192 and r["odometry_pc"].shape == (8192, 3) for r in got[1:])


def test_deskewed_drive_equals_the_plugin_bit_for_bit(torch_cuda):
    """Per-point timestamps: de-skew by the constant-velocity guess -> grid sample of the float64 rows -> float32, against
    the plugin behind Distortion -> GridSample -> ToTensor; 5 frames."""
    _compare_drive(torch_cuda, "deskew", 1)
    # (the de-skew moved something: the same frames without timestamps give other poses from frame 2 on)
    plain = _plugin_run(torch_cuda, "sampled")[0]
    skewed = _plugin_run(torch_cuda, "deskew")[0]
    assert not np.array_equal(plain[2]["pose"], skewed[2]["pose"])


# ---- 5: against the reference -------------------------------------------------------------------------------------------
def test_published_loop_through_the_frame_calls_matches_the_reference(torch_cuda, golden_loop, loop_scans):
    """The published configuration's 36-frame loop (tests/test_gpu_loop.py) through icp_frame_launch / icp_frame_end, with
    that file's bars against tests/golden/loop_reference.npz: every frame within 1e-4 m / 1e-4 rad (one iteration more or
    less only where the reference's own stop was within 2 % of the threshold, then off by at most that step more), map sizes
    within 2 points, 30 clouds at the end, ATE / ARE / tr_err equal to 2e-5."""
    import os
    import icp_oracle as O
    from conftest import GOLDEN
    from pylidar_slam_amd.engine import IcpContext
    g = golden_loop
    spread = np.load(os.path.join(GOLDEN, "loop_spread.npz"))
    assert bool(spread["base_reproduces_loop_reference"])
    scans, gt_abs = loop_scans
    ctx = IcpContext(height=64, width=2048, max_num_alignments=20, threshold_delta_pose=1.0e-4, scheme="neighborhood",
                     sigma=0.2, local_map_size=30, num_neighbors_normals=10)
    ctx.odometry_init(voxel_size=0.4, threshold_trans=0.1, threshold_rot=0.3, constant_velocity=True, targets=1)
    rel, flips, worst = [], [], (0.0, 0.0)
    for f, scan in enumerate(scans):
        ctx.frame_launch(scan)
        r = ctx.frame_end()
        assert r.samples == int(g["samples"][f]) and r.frame_index == f
        rel.append(r.pose)
        if f == 0:
            continue
        dt, dr = O.pose_error(r.pose, g["rel"][f])
        worst = (max(worst[0], dt), max(worst[1], dr))
        ours, theirs = int(r.register.iterations), int(g["iters"][f])
        bound = 1e-4
        if ours != theirs:
            margin = float(spread["stop_margin"][f])
            step = float(spread["base_dx_norm"][f, min(ours, theirs) - 1])
            flips.append((f, ours, theirs, margin, step, dt))
            assert abs(ours - theirs) == 1 and margin < 0.02, (f, ours, theirs, margin)
            bound = 1e-4 + step
        assert dt < bound and dr < 1e-4, (f, dt, dr, ours, theirs)
        assert abs(ctx.map_size() - int(g["map_sizes"][f])) <= 2, (f, ctx.map_size(), int(g["map_sizes"][f]))
        assert r.key_frame and r.points.shape[0] == r.samples == r.inserted
    assert ctx.map_num_clouds() == 30 and ctx.handoff_fallbacks() == 0
    ate, are, tr, rot, n = trajectory_metrics(np.stack(rel), gt_abs, g["segments"])
    print(f"frame calls, published loop: worst frame {worst[0]:.1e} m / {worst[1]:.1e} rad vs the reference; ATE {ate:.4e} "
          f"(reference {g['ate'][0]:.4e}) m, tr_err {tr:.4e} ({g['kitti'][0]:.4e}) m/m; flips {flips}")
    assert n == int(g["num_segments"])
    assert abs(ate - g["ate"][0]) < 2e-5 and abs(are - g["are"][0]) < 2e-5
    assert abs(tr - g["kitti"][0]) < 2e-5
    assert rot < 1e-3 and len(flips) <= 3


# ---- 6: the plugin's flag -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sampled", "raw"])
def test_one_call_frame_flag_equals_the_default_path(torch_cuda, name):
    """`one_call_frame=True` against `False` on the same dicts: every entry of every frame's dict and both pose lists."""
    torch = torch_cuda
    d = FC.drive(name)
    _, want_map, want_clouds, want_rel, want_abs = _plugin_run(torch, name)
    ref_odo, ref_filters, ref_init = _make_plugin(torch, d)
    odo, filters, init = _make_plugin(torch, d, one_call_frame=True)
    for f in range(d.frames):
        a, b = _frame_dict(d, f), _frame_dict(d, f)
        ra = _plugin_step(odo, filters, init, a)
        rb = _plugin_step(ref_odo, ref_filters, ref_init, b)
        assert ra["kind"] == rb["kind"] == ("first" if f == 0 else "frame")
        assert set(a) == set(b), (f, sorted(a), sorted(b))
        for k in a:
            x = a[k].detach().cpu().numpy() if isinstance(a[k], torch.Tensor) else np.asarray(a[k])
            y = b[k].detach().cpu().numpy() if isinstance(b[k], torch.Tensor) else np.asarray(b[k])
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (f, k)
        if f > 0:
            assert odo.last_result.iterations == ref_odo.last_result.iterations
            assert np.array_equal(odo.last_result.losses, ref_odo.last_result.losses)
    assert np.array_equal(odo.get_relative_poses(), want_rel) and np.array_equal(np.stack(odo.absolute_poses), want_abs)
    assert np.array_equal(odo.ctx.map_points(), want_map) and odo.ctx.map_num_clouds() == want_clouds


# ---- 7: edges -----------------------------------------------------------------------------------------------------------
def test_edges_equal_the_plugin_and_refusals_leave_the_context_registering(torch_cuda):
    """Raw 16x512 sequence from host arrays.  Frame 2: ONE valid row among NaN rows; frame 3: an explicit init_pose.  The
    library run alone also meets: `cap` below the row count (frame 1: ICP_ERR_INVALID_ARGUMENT with the count, the frame
    completed), a second icp_frame_launch before icp_frame_end (frame 3), icp_frame_end with nothing launched (behind frame
    3) — and still equals the plugin, frame by frame and in its final map."""
    torch = torch_cuda
    from pylidar_slam_amd.synthetic import pose_matrix
    d = FC.drive("raw")
    lonely = np.full_like(d.scans[2], np.nan)
    lonely[4097] = d.scans[2][4097]
    guess = pose_matrix(np.array([0.35, 0.01, 0.0, 0.0, 0.0, 0.008])).astype(np.float32)
    frames = [(d.scans[0], None), (d.scans[1], None), (lonely, None), (d.scans[2], guess), (d.scans[3], None),
              (d.scans[4], None)]
    odo, filters, init = _make_plugin(torch, d)
    want = [_plugin_step(odo, filters, init, {"numpy_pc": s}, explicit_init=g) for s, g in frames]
    ctx = _make_context(d)
    _init_sequence(ctx, d)
    got = []
    for f, (s, g) in enumerate(frames):
        if f == 1:  # cap below the row count: refused with the count, the frame completed all the same
            ctx.frame_launch(s, None, g)
            with pytest.raises(AssertionError, match="fewer rows") as raised:
                ctx.frame_end(cap=100)
            assert raised.value.rows == 8192 and raised.value.result.frame_index == 1
            reg = raised.value.register  # (the registration's own result; no row was written: odometry_pc is not compared)
            got.append(_record("frame", pose=reg.pose, params=reg.params, iterations=reg.iterations, losses=reg.losses,
                               dx=reg.dx, key_frame=bool(raised.value.result.key_frame),
                               inserted=int(raised.value.result.inserted), odometry_pc=None))
            continue
        if f == 3:
            ctx.frame_launch(s, None, g)
            with pytest.raises(AssertionError, match="already launched"):
                ctx.frame_launch(s, None, g)
            r = ctx.frame_end()
            got.append(_record("frame", pose=r.pose, params=r.params, iterations=r.register.iterations,
                               losses=r.register.losses, dx=r.register.dx, key_frame=r.key_frame, inserted=r.inserted,
                               odometry_pc=r.points))
            with pytest.raises(AssertionError, match="no frame launched"):
                ctx.frame_end()
            continue
        got.append(_library_step(ctx, s, None, g))
    for f, (a, b) in enumerate(zip(got, want)):
        _same(a, b, ("edges", f), skip=("odometry_pc",) if f == 1 else ())
    # the lonely frame: ONE row took part on both paths — one row cannot determine six parameters: an Invalid Jacobian, raised
    # before the map was touched; every other frame registered
    assert got[2]["kind"] == "invalid_jacobian" and got[2]["num_targets"] == 1 and want[2]["num_targets"] == 1
    assert [r["kind"] for r in got] == ["first", "frame", "invalid_jacobian", "frame", "frame", "frame"]
    assert np.array_equal(ctx.map_points(), odo.ctx.map_points()) and ctx.map_num_clouds() == odo.ctx.map_num_clouds()


def test_tiny_grid_sample_equals_the_plugin(torch_cuda):
    """A frame whose grid sample leaves fewer than 10 rows (8 occupied voxels), inside the sampled drive."""
    torch = torch_cuda
    d = FC.drive("sampled")
    rng = np.random.default_rng(7)
    picks = d.scans[2][np.linspace(0, d.scans[2].shape[0] - 1, 8).astype(int)]
    centres = np.round(picks / 0.4) * 0.4  # (a voxel is round(p / 0.4), slam/common/pointcloud.py:54-79: its centre k * 0.4)
    assert len({tuple(c) for c in np.round(centres / 0.4).astype(int)}) == 8
    tiny = (np.repeat(centres, 50, axis=0) + rng.uniform(-0.05, 0.05, size=(400, 3))).astype(np.float32)
    frames = [d.scans[0], d.scans[1], tiny, d.scans[2], d.scans[3]]
    odo, filters, init = _make_plugin(torch, d)
    want = [_plugin_step(odo, filters, init, {"numpy_pc": s}) for s in frames]
    ctx = _make_context(d)
    _init_sequence(ctx, d)
    got = [_library_step(ctx, s) for s in frames]
    for f, (a, b) in enumerate(zip(got, want)):
        _same(a, b, ("tiny", f))
    # the tiny frame registered (8 targets determine the pose) and its 8 samples are what came back and went into the map
    assert [r["kind"] for r in got] == ["first"] + ["frame"] * 4
    assert got[2]["samples"] == 8 and got[2]["odometry_pc"].shape == (8, 3)
    assert got[2]["inserted"] == (8 if got[2]["key_frame"] else 0)
    assert np.array_equal(ctx.map_points(), odo.ctx.map_points()) and ctx.map_num_clouds() == odo.ctx.map_num_clouds()


def test_projective_context_is_refused_and_keeps_working(torch_cuda):
    from pylidar_slam_amd.engine import IcpContext
    d = FC.drive("raw")
    ctx = IcpContext(height=d.height, width=d.width, max_num_alignments=4, threshold_delta_pose=0.0, local_map_size=3)
    ctx.pmap_init()
    ctx.pmap_update(EYE, ctx.project(d.scans[0]))
    with pytest.raises(AssertionError, match="projective map"):
        ctx.odometry_init()
    with pytest.raises(AssertionError, match="icp_odometry_init first"):
        ctx.frame_launch(d.scans[1])
    assert ctx.pmap_num_maps() == 1
    res = ctx.pmap_register(d.scans[1])
    assert res.iterations == 4 and np.isfinite(res.pose).all()


def test_exchange_profiling_and_batch_hold_are_refused_and_lifted(torch_cuda):
    """The other refusals of the scope: an exchange switched on, profiling on, a context held by a batch that still holds
    iterations back.  Each is ICP_ERR_INVALID_ARGUMENT with its reason; with the condition lifted the same context runs the
    drive with the poses of a context that never met it."""
    from pylidar_slam_amd.engine import IcpBatch
    d = FC.drive("raw")
    fresh = _make_context(d)
    _init_sequence(fresh, d)
    want = [_library_step(fresh, d.scans[f]) for f in range(3)]

    def runs_like_fresh(ctx, what):
        _init_sequence(ctx, d)
        for f in range(3):
            _same(_library_step(ctx, d.scans[f]), want[f], (what, f))

    ctx = _make_context(d)
    ctx.profile_enable(1)
    with pytest.raises(AssertionError, match="profiling"):
        _init_sequence(ctx, d)
    ctx.profile_enable(0)
    runs_like_fresh(ctx, "profiling off again")
    ctx.profile_enable(1)  # ... and switched on in the middle of a sequence
    with pytest.raises(AssertionError, match="profiling"):
        ctx.frame_launch(d.scans[3])
    ctx.profile_enable(0)

    ctx = _make_context(d)
    ctx.exchange_connect([ctx.exchange_create(0, 1)])  # (a world of one rank: the exchange is on)
    with pytest.raises(AssertionError, match="exchange"):
        _init_sequence(ctx, d)
    ctx.exchange_destroy()
    runs_like_fresh(ctx, "exchange destroyed")

    live = FC.drive("sampled_live")  # (a live stop threshold: the batch enqueues a first chunk and holds the rest back)
    a, b = _make_context(live), _make_context(live)
    for c in (a, b):
        c.map_set(live.scans[0])
    batch = IcpBatch([a, b])
    batch.register_launch([live.scans[1], live.scans[1]])
    with pytest.raises(AssertionError, match="held by a batch"):
        a.odometry_init()
    results = batch.register_end()
    assert all(1 <= r.iterations <= live.max_num_alignments for r in results)
    batch.close()
    a.odometry_init(threshold_trans=FC.THRESHOLD_TRANS, threshold_rot=FC.THRESHOLD_ROT, targets=0)
    a.frame_launch(live.scans[0])
    assert a.frame_end().frame_index == 0
    a.frame_launch(live.scans[1])
    assert a.frame_end().register.iterations >= 1


def test_odometry_init_restarts_the_sequence(torch_cuda):
    """icp_odometry_init in the middle of a drive — behind a collected frame, and behind a frame launched and never ended —
    starts over: the second run's poses equal a fresh context's."""
    d = FC.drive("raw")
    fresh = _make_context(d)
    _init_sequence(fresh, d)
    want = [_library_step(fresh, d.scans[f]) for f in range(4)]
    ctx = _make_context(d)
    _init_sequence(ctx, d)
    for f in range(3):
        _library_step(ctx, d.scans[f])
    ctx.frame_launch(d.scans[3])  # never ended
    _init_sequence(ctx, d)
    got = [_library_step(ctx, d.scans[f]) for f in range(4)]
    for f, (a, b) in enumerate(zip(got, want)):
        _same(a, b, ("restart", f))
    assert np.array_equal(ctx.map_points(), fresh.map_points()) and ctx.map_num_clouds() == fresh.map_num_clouds()


# ---- 8: the error path ----------------------------------------------------------------------------------------------------
def test_invalid_jacobian_through_frame_end_leaves_the_map_where_it_was(torch_cuda):
    """The degenerate input of tests/test_gpu_pipeline.py::test_failed_registration_leaves_the_map_where_it_was — a map on
    the plane z = 0 and targets right above it: J^T J is singular — through icp_frame_end: the status comes back
    (InvalidJacobianError), the map is unchanged, the sequence has not advanced, and the next icp_odometry_init + frames
    work."""
    from pylidar_slam_amd.engine import IcpContext, InvalidJacobianError
    d = FC.drive("raw")
    ctx = IcpContext(height=d.height, width=d.width, max_num_alignments=4, threshold_delta_pose=0.0, local_map_size=3)
    ctx.odometry_init(threshold_trans=FC.THRESHOLD_TRANS, threshold_rot=FC.THRESHOLD_ROT, targets=0)
    ctx.frame_launch(d.scans[0])
    assert ctx.frame_end().frame_index == 0
    xs, ys = np.meshgrid(np.arange(40, dtype=np.float32) * 0.1, np.arange(40, dtype=np.float32) * 0.1)
    plane = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size, np.float32)], axis=1)
    ctx.map_set(plane)
    before = ctx.map_points().copy()
    targets = plane[::3] + np.array([0.013, 0.007, 0.05], np.float32)
    ctx.frame_launch(targets)
    with pytest.raises(InvalidJacobianError) as raised:
        ctx.frame_end()
    assert raised.value.result is not None and raised.value.result.iterations >= 1
    np.testing.assert_array_equal(ctx.map_points(), before)
    assert ctx.map_num_clouds() == 0  # (icp_map_set keeps no cloud bookkeeping: nothing was appended either)
    with pytest.raises(AssertionError, match="no frame launched"):
        ctx.frame_end()
    # the sequence has not advanced: the next frame is frame 1 again; then a fresh sequence equals a fresh context's
    ctx.odometry_init(threshold_trans=FC.THRESHOLD_TRANS, threshold_rot=FC.THRESHOLD_ROT, targets=0)
    got = [_library_step(ctx, d.scans[f]) for f in range(3)]
    fresh = IcpContext(height=d.height, width=d.width, max_num_alignments=4, threshold_delta_pose=0.0, local_map_size=3)
    fresh.odometry_init(threshold_trans=FC.THRESHOLD_TRANS, threshold_rot=FC.THRESHOLD_ROT, targets=0)
    want = [_library_step(fresh, d.scans[f]) for f in range(3)]
    for f, (a, b) in enumerate(zip(got, want)):
        _same(a, b, ("after the error", f))
    assert got[1]["iterations"] == 4 and got[1]["frame_index"] == 1
