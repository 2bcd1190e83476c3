"""`-m gpu`: one library call per odometry frame against the projective local map (icp_pmap_odometry_init /
icp_pmap_frame_launch / icp_pmap_frame_end, include/icp_mi355x.h) and the enqueued registration behind it
(icp_pmap_register_launch) — against the per-call entry point `icp_pmap_register` and the per-call plugin
`MI355XICPFrameToModel` with `projective_local_map` on the same frames, bit for bit: the new calls compose the plugin's own
steps in the plugin's order.

The drives and their key-frame thresholds live in tests/pmap_frame_cases.py; tests/test_pmap_frame_host.py checks on the CPU
that no frame of a drive sits near a threshold (so the float32 4x4 product of the library and numpy's cannot decide
differently)."""
import ctypes as C

import numpy as np
import pytest

import pmap_frame_cases as PC

pytestmark = pytest.mark.gpu

EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


# ---- contexts, inputs ------------------------------------------------------------------------------------------------------
def _make_context(d, **over):
    from pylidar_slam_amd.engine import IcpContext
    kw = dict(height=d.height, width=d.width, max_num_alignments=d.max_num_alignments,
              threshold_delta_pose=d.threshold_delta_pose, scheme=d.scheme, sigma=d.sigma, local_map_size=d.local_map_size)
    kw.update(over)
    return IcpContext(**kw)


_INPUTS = {}


def _inputs(torch, d):
    """What a frame of the drive is, per frame: cuda [3,H,W] vertex maps (the library's own projection of the scans), cuda
    [N,3] rows, or the numpy scans themselves."""
    if d.name not in _INPUTS:
        if d.kind == "vmap":
            ctx = _make_context(d)
            _INPUTS[d.name] = [ctx.project(torch.from_numpy(s).cuda()).clone() for s in d.scans]
            torch.cuda.synchronize()
            ctx.close()
        elif d.kind == "rows_cuda" and not d.timestamps:
            _INPUTS[d.name] = [torch.from_numpy(s).cuda() for s in d.scans]
        else:
            _INPUTS[d.name] = list(d.scans)
    return _INPUTS[d.name]


# ---- the raw registration calls ----------------------------------------------------------------------------------------------
def _raw_result(ctx, rc, res, losses, dxs):
    k = int(res.iterations)
    return dict(rc=int(rc), status=int(res.status), pose=np.array(res.pose, np.float32), params=np.array(res.params, np.float32),
                iterations=k, converged=int(res.converged), num_targets=int(res.num_targets),
                losses=np.array(losses[:k], np.float64), dx=np.array(dxs, np.float32)[:6 * k])


def _register(ctx, points, init, skip_null, launched):
    """icp_pmap_register, or icp_pmap_register_launch + icp_register_end, straight through the C ABI: every field of the
    result, the histories and the return code."""
    from pylidar_slam_amd import _lib
    from pylidar_slam_amd.engine import _pose16, _ptr_mem
    ctx._bind(points)
    p, mem, keep = _ptr_mem(points)
    n = int(keep.shape[0])
    cap = max(1, int(ctx.config.max_num_alignments))
    losses, dxs, res = (C.c_double * cap)(), (C.c_float * (6 * cap))(), _lib.IcpRegisterResult()
    mode = _lib.TARGETS_SKIP_NULL if skip_null else _lib.TARGETS_ALL
    if not launched:
        rc = ctx._lib.icp_pmap_register(ctx._h, p, n, mem, mode, _pose16(init), C.byref(res), losses, dxs)
    else:
        rc = ctx._lib.icp_pmap_register_launch(ctx._h, p, n, mem, mode, _pose16(init))
        assert rc == 0, ctx._lib.icp_last_error(ctx._h)
        rc = ctx._lib.icp_register_end(ctx._h, C.byref(res), losses, dxs)
    return _raw_result(ctx, rc, res, losses, dxs)


def _same_registration(a, b, what):
    for k in ("rc", "status", "iterations", "converged", "num_targets"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in ("pose", "params", "losses", "dx"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True), (what, k, a[k], b[k])


def _mapped_context(torch, d, vmaps, **over):
    """A context whose projective map holds frames 0 and 1 of the drive (the second one step ahead)."""
    from pylidar_slam_amd.synthetic import pose_matrix
    ctx = _make_context(d, **over)
    ctx.pmap_init()
    ctx.pmap_update(EYE, vmaps[0])
    ctx.pmap_update(pose_matrix(np.array([0.4, 0.0, 0.0, 0.0, 0.0, 0.01])).astype(np.float32), vmaps[1])
    return ctx


# ---- 1. icp_pmap_register_launch == icp_pmap_register ----------------------------------------------------------------------------
def test_register_launch_equals_pmap_register_forced_iterations(torch_cuda):
    """8 forced iterations against a window of two maps (16x512): 1, 63, 64, 65 and 257 target rows from device and host
    memory, and all 8192 pixels of a vertex map with ICP_TARGETS_SKIP_NULL — every field, the losses, the steps, the status
    and the return code (a single row cannot determine six parameters: both report it alike)."""
    torch = torch_cuda
    from pylidar_slam_amd import _lib
    d = PC.drive("vmap")
    vmaps = _inputs(torch, d)
    ctx = _mapped_context(torch, d, vmaps)
    rows = d.scans[2]
    rows = rows[~np.isnan(rows).any(axis=1)]  # (rows with a NaN take no part: counted out of num_targets)
    pick = np.linspace(0, rows.shape[0] - 1, 257).astype(int)
    seen = set()
    for n in (1, 63, 64, 65, 257):
        for where in ("host", "device"):
            pts = np.ascontiguousarray(rows[pick[:n]])
            pts = torch.from_numpy(pts).cuda() if where == "device" else pts
            want = _register(ctx, pts, EYE, False, launched=False)
            got = _register(ctx, pts, EYE, False, launched=True)
            _same_registration(got, want, (n, where))
            assert 0 <= want["num_targets"] <= n  # (the rows of the last iteration: targets that found a map pixel)
            seen.add(want["status"])
    assert seen == {0, _lib.ICP_ERR_INVALID_JACOBIAN}  # (63 rows determine a pose, one row does not)
    pixels = vmaps[2].permute(1, 2, 0).reshape(-1, 3).contiguous()
    want = _register(ctx, pixels, EYE, True, launched=False)
    got = _register(ctx, pixels, EYE, True, launched=True)
    _same_registration(got, want, "pixels")
    assert want["rc"] == 0 and want["iterations"] == 8 and 0 < want["num_targets"] < 8192
    assert np.abs(want["pose"].reshape(4, 4)[:3, 3]).max() > 0.1  # (the registration moved: 0.4 m per frame)


def test_register_launch_equals_pmap_register_live_stop(torch_cuda):
    """|dx| < 1e-4 live, at most 15 iterations, `neighborhood` / 0.2: the per-call loop polls the host every 4 iterations,
    the launched one decides on the device — the same iteration count and histories.  Then the guess = the converged pose:
    both stop in the first iteration."""
    torch = torch_cuda
    d = PC.drive("live")
    vmaps = _inputs(torch, d)
    ctx = _mapped_context(torch, d, vmaps)
    pixels = vmaps[2].permute(1, 2, 0).reshape(-1, 3).contiguous()
    want = _register(ctx, pixels, EYE, True, launched=False)
    got = _register(ctx, pixels, EYE, True, launched=True)
    _same_registration(got, want, "live")
    assert want["rc"] == 0 and want["converged"] == 1 and 1 < want["iterations"] < 15
    converged = want["pose"].reshape(4, 4)
    first = _register(ctx, pixels, converged, True, launched=False)
    again = _register(ctx, pixels, converged, True, launched=True)
    _same_registration(again, first, "from the converged pose")
    assert first["rc"] == 0 and first["iterations"] == 1 and first["converged"] == 1


def _few_pixels(torch, vmap):
    """The vertex map with all but three of its non-null pixels zeroed: three rows cannot determine six parameters."""
    flat = vmap.reshape(3, -1)
    valid = torch.nonzero(flat.abs().amax(dim=0) > 0).reshape(-1)
    keep = valid[torch.linspace(0, valid.numel() - 1, 5).long()[1:4]]
    out = torch.zeros_like(flat)
    out[:, keep] = flat[:, keep]
    return out.reshape(vmap.shape).contiguous()


def test_register_launch_degenerate_frames_end_alike_and_the_context_goes_on(torch_cuda):
    """An all-null frame: no row at all, so the residual-norm guard of the Gauss-Newton step (optimization.py:323-327) ends the
    loop in its first iteration with the guess unchanged — icp_pmap_register's own answer, status ICP_OK — and the launched
    form gives the same.  Three pixels: `Invalid Jacobian` (|det H| < 1e-7, :334-336) from both, the same status, return code
    and histories.  The context registers normally afterwards."""
    torch = torch_cuda
    from pylidar_slam_amd import _lib
    d = PC.drive("vmap")
    vmaps = _inputs(torch, d)
    ctx = _mapped_context(torch, d, vmaps)
    pixels = vmaps[2].permute(1, 2, 0).reshape(-1, 3).contiguous()
    before = _register(ctx, pixels, EYE, True, launched=True)
    null = torch.zeros_like(pixels)
    want = _register(ctx, null, EYE, True, launched=False)
    got = _register(ctx, null, EYE, True, launched=True)
    _same_registration(got, want, "all null")
    assert want["rc"] == want["status"] == 0 and want["num_targets"] == 0 and want["iterations"] == 1 and want["converged"] == 1
    assert np.array_equal(want["pose"].reshape(4, 4), EYE)
    few = _few_pixels(torch, vmaps[2]).permute(1, 2, 0).reshape(-1, 3).contiguous()
    want = _register(ctx, few, EYE, True, launched=False)
    got = _register(ctx, few, EYE, True, launched=True)
    _same_registration(got, want, "three pixels")
    assert want["rc"] == want["status"] == _lib.ICP_ERR_INVALID_JACOBIAN and 1 <= want["num_targets"] <= 3
    assert b"Invalid Jacobian" in ctx._lib.icp_last_error(ctx._h)
    after = _register(ctx, pixels, EYE, True, launched=True)
    _same_registration(after, before, "behind the failure")
    assert after["rc"] == 0 and ctx.pmap_num_maps() == 2


def test_entry_points_between_launch_and_end_run_in_call_order(torch_cuda):
    """Between icp_pmap_register_launch and icp_register_end: a second launch is refused; the model read-back, the window
    size and the association seam (which shares the context's z-buffer with the iterations) run behind the registration in
    call order — they return what they return without one, and the registration's result is what it is without them."""
    torch = torch_cuda
    d = PC.drive("vmap")
    vmaps = _inputs(torch, d)
    ctx = _mapped_context(torch, d, vmaps)
    pixels = vmaps[2].permute(1, 2, 0).reshape(-1, 3).contiguous()
    model = ctx.pmap_model()
    as_np = lambda a: a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    assoc = [as_np(a) for a in ctx.pmap_nearest_neighbor_search(d.scans[2])]  # (before any registration ran on the context)
    assert assoc[0].shape[0] > 1000
    want = _register(ctx, pixels, EYE, True, launched=True)
    ctx.pmap_register_launch(pixels, EYE, skip_null=True)
    with pytest.raises(AssertionError, match="awaits icp_register_end"):
        ctx.pmap_register_launch(pixels, EYE, skip_null=True)
    assert ctx.pmap_num_maps() == 2
    between = ctx.pmap_model()
    assoc_between = [as_np(a) for a in ctx.pmap_nearest_neighbor_search(d.scans[2])]  # (over the iterations' z-buffer keys)
    res = ctx.register_end()
    assert np.array_equal(between[0], model[0]) and np.array_equal(between[1], model[1])
    for a, b in zip(assoc_between, assoc):
        assert a.shape == b.shape and np.array_equal(a, b)
    assert np.array_equal(res.pose.reshape(-1), want["pose"]) and res.iterations == want["iterations"]
    assert np.array_equal(res.losses, want["losses"]) and np.array_equal(res.dx.reshape(-1), want["dx"])
    with pytest.raises(AssertionError):  # nothing left to collect
        ctx.register_end()


# ---- the two paths of a drive ------------------------------------------------------------------------------------------------
def _filters(d, dev):
    from pylidar_slam_amd import odometry as our
    if not d.timestamps:
        return []
    return [our.ToDevice(our.ToDeviceConfig(device=str(dev)), device=dev),
            our.Distortion(our.DistortionConfig(pointcloud_key="pc_device", timestamps_key="timestamps_device",
                                                output_key="deskewed")),
            our.GridSample(our.GridSampleConfig(voxel_size=d.voxel_size, pointcloud_key="deskewed", padded=True)),
            our.ToTensor(our.ToTensorConfig(device=str(dev), keys={"sample_points": "input_data"}, dtype="float32"),
                         device=dev)]


def _frame_dict(d, frame, f):
    if d.timestamps:
        return {"numpy_pc": frame, "numpy_pc_timestamps": d.stamps[f]}
    return {"input_data": frame}


def _make_plugin(torch, d, **over):
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    odo = our.MI355XICPFrameToModel(PC.plugin_config(d, **over), projector=our.SphericalProjector(d.height, d.width), device=dev)
    init = our.ConstantVelocityInitialization()
    odo.init()
    init.init()
    return odo, _filters(d, dev), init


def _model(ctx):
    mv, mn = ctx.pmap_model()
    return ctx.pmap_num_maps(), mv, mn


def _plugin_step(odo, filters, init, data):
    """One frame through the plugin (either path): what the frame returned, and the window and model behind it."""
    from pylidar_slam_amd.engine import InvalidJacobianError
    init.next_frame(data)  # slam/slam.py:126-127
    for flt in filters:
        flt.filter(data)
    first = odo._iter == 0
    try:
        odo.process_next_frame(data)
    except InvalidJacobianError:
        return dict(kind="invalid_jacobian", model=_model(odo.ctx))
    if first:
        return dict(kind="first", model=_model(odo.ctx))
    init.save_real_motion(data["odometry_pose"], data)  # :139-140
    res = odo.last_result
    key = np.array_equal(odo._delta_since_map_update, EYE)  # (__update_map resets it on a key frame, :376)
    return dict(kind="frame", pose=data["odometry_pose"], params=res.params, iterations=res.iterations, losses=res.losses,
                dx=res.dx, key_frame=bool(key), odometry_pc=data["odometry_pc"], model=_model(odo.ctx))


def _library_step(ctx, frame, stamps=None, init_pose=None, **end):
    from pylidar_slam_amd.engine import InvalidJacobianError
    ctx.pmap_frame_launch(frame, stamps, init_pose)
    try:
        r = ctx.pmap_frame_end(**end)
    except InvalidJacobianError as e:
        assert e.result is not None
        return dict(kind="invalid_jacobian", model=_model(ctx), num_targets=e.result.num_targets)
    if r.frame_index == 0:
        assert r.register.iterations == 0 and np.array_equal(r.pose, EYE) and r.key_frame and r.points is None
        assert r.inserted == 1
        return dict(kind="first", model=_model(ctx), samples=r.samples)
    g = r.register
    return dict(kind="frame", pose=g.pose, params=g.params, iterations=g.iterations, losses=g.losses, dx=g.dx,
                key_frame=r.key_frame, inserted=r.inserted, odometry_pc=r.points, samples=r.samples,
                frame_index=r.frame_index, model=_model(ctx))


def _same(a, b, what, skip=()):
    assert a["kind"] == b["kind"], (what, a["kind"], b["kind"])
    ka, kb = a["model"], b["model"]
    assert ka[0] == kb[0], (what, "pmap_num_maps", ka[0], kb[0])
    assert np.array_equal(ka[1], kb[1]) and np.array_equal(ka[2], kb[2]), (what, "pmap_model")
    if a["kind"] != "frame":
        return
    for k in ("pose", "params", "losses", "dx", "odometry_pc"):
        if k in skip:
            continue
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (what, k, x.shape, y.shape, x.dtype, y.dtype)
        assert np.array_equal(x, y), (what, k, np.abs(x.astype(np.float64) - y.astype(np.float64)).max())
    for k in ("iterations", "key_frame"):
        assert a[k] == b[k], (what, k, a[k], b[k])


_PLUGIN_RUNS = {}


def _plugin_run(torch, name):
    """The drive through the per-call plugin, once per module: per-frame records and both pose lists."""
    if name not in _PLUGIN_RUNS:
        d = PC.drive(name)
        frames = _inputs(torch, d)
        odo, filters, init = _make_plugin(torch, d)
        recs = [_plugin_step(odo, filters, init, _frame_dict(d, frames[f], f)) for f in range(d.frames)]
        _PLUGIN_RUNS[name] = (recs, odo.get_relative_poses(), np.stack(odo.absolute_poses))
        odo.ctx.close()
    return _PLUGIN_RUNS[name]


def _init_sequence(ctx, d, **over):
    kw = dict(voxel_size=d.voxel_size, threshold_trans=PC.THRESHOLD_TRANS, threshold_rot=PC.THRESHOLD_ROT,
              constant_velocity=False, targets=d.targets, normals_kernel_size=5)
    kw.update(over)
    ctx.pmap_odometry_init(**kw)


def _library_run(torch, d, frames, count=None, ctx=None, **over):
    """The drive through the bare calls with the plugin's `init_rpose` chain handed over explicitly: the identity for
    frames 0 and 1, then the last pose."""
    ctx = ctx or _make_context(d)
    _init_sequence(ctx, d, **over)
    got, last = [], EYE
    for f in range(d.frames if count is None else count):
        got.append(_library_step(ctx, frames[f], d.stamps[f] if d.timestamps else None, last))
        if got[-1]["kind"] == "frame":
            last = got[-1]["pose"]
    return got, ctx


# ---- 2. every drive: the bare calls == the per-call plugin ---------------------------------------------------------------------
@pytest.mark.parametrize("name", PC.NAMES)
def test_drive_through_the_bare_calls_equals_the_plugin_bit_for_bit(torch_cuda, name):
    """Per frame pose, parameters, iteration count, losses, steps, key-frame decision and odometry_pc; behind every frame the
    window size and the model (`pmap_num_maps`, `pmap_model`).  Both kinds of update in every drive; `vmap` and `rows_pixels`
    evict; `live` stops early; `deskew` de-skews by the guess and grid-samples inside the library, against the plugin behind
    ToDevice -> Distortion -> GridSample(padded) -> ToTensor."""
    torch = torch_cuda
    d = PC.drive(name)
    frames = _inputs(torch, d)
    want, _, _ = _plugin_run(torch, name)
    got, ctx = _library_run(torch, d, frames)
    npix = d.height * d.width
    for f, (a, b) in enumerate(zip(got, want)):
        _same(a, b, (name, f))
        if f > 0:
            assert a["frame_index"] == f and a["inserted"] == (1 if a["key_frame"] else 0)
            if d.voxel_size > 0:
                assert a["samples"] == a["odometry_pc"].shape[0] < npix
            else:
                assert a["samples"] == npix and 0 < a["odometry_pc"].shape[0] <= npix
    keys = [f for f, r in enumerate(got) if f > 0 and r["key_frame"]]
    assert len(keys) >= 1 and d.frames - 1 - len(keys) >= 1, (name, keys)
    if name in ("vmap", "rows_pixels"):
        assert len(keys) + 1 > d.local_map_size and ctx.pmap_num_maps() == d.local_map_size  # evictions happened
    if d.threshold_delta_pose > 0:
        assert all(1 <= r["iterations"] <= d.max_num_alignments for r in got[1:])
        assert any(r["iterations"] < d.max_num_alignments for r in got[1:])
    else:
        assert all(r["iterations"] == d.max_num_alignments for r in got[1:])
    if d.kind == "vmap":  # null pixels were dropped from odometry_pc, in pixel order
        px = frames[1].permute(1, 2, 0).reshape(-1, 3).cpu().numpy()
        assert np.array_equal(got[1]["odometry_pc"], px[np.abs(px).max(axis=1) > 0])


def test_constant_velocity_without_init_pose_equals_the_plugin_fed_its_last_pose(torch_cuda):
    torch = torch_cuda
    d = PC.drive("vmap")
    frames = _inputs(torch, d)
    want, _, _ = _plugin_run(torch, "vmap")
    ctx = _make_context(d)
    _init_sequence(ctx, d, constant_velocity=True)
    for f in range(d.frames):
        _same(_library_step(ctx, frames[f]), want[f], ("constant velocity", f))
    # ... and it matters: without a guess the same frames give other poses from frame 2 on
    _init_sequence(ctx, d, constant_velocity=False)
    plain = [_library_step(ctx, frames[f]) for f in range(3)]
    assert np.array_equal(plain[1]["pose"], want[1]["pose"]) and not np.array_equal(plain[2]["losses"], want[2]["losses"])


def test_device_and_host_rows_give_the_same_frames(torch_cuda):
    """`rows_numpy`'s scans as cuda tensors (targets = 0 kept): the upload through the pinned slots changes nothing; and the
    output capacity: `cap` below the row count is refused with the count, the frame completed all the same."""
    torch = torch_cuda
    d = PC.drive("rows_numpy")
    want, _, _ = _plugin_run(torch, "rows_numpy")
    got, ctx = _library_run(torch, d, [torch.from_numpy(s).cuda() for s in d.scans], count=3)
    for f in range(3):
        _same(got[f], want[f], ("device rows", f))
    ctx.pmap_frame_launch(d.scans[3], None, got[2]["pose"])
    with pytest.raises(AssertionError, match="fewer rows") as raised:
        ctx.pmap_frame_end(cap=100)
    assert raised.value.rows == d.scans[3].shape[0] and raised.value.result.frame_index == 3
    assert np.array_equal(raised.value.register.pose, want[3]["pose"])
    assert np.array_equal(ctx.pmap_model()[0], want[3]["model"][1])


# ---- 3. a failed frame ------------------------------------------------------------------------------------------------------------
def test_failed_frame_leaves_the_sequence_where_it_was(torch_cuda):
    """A vertex map of three pixels between frames 2 and 3 of `vmap`: Invalid Jacobian out of icp_pmap_frame_end, the window,
    the model and the sequence state untouched — the frames behind it equal the run that never saw it."""
    torch = torch_cuda
    d = PC.drive("vmap")
    frames = _inputs(torch, d)
    want, _, _ = _plugin_run(torch, "vmap")
    ctx = _make_context(d)
    _init_sequence(ctx, d)
    last = EYE
    for f in range(d.frames):
        if f == 3:
            bad = _library_step(ctx, _few_pixels(torch, frames[f]), None, last)
            assert bad["kind"] == "invalid_jacobian" and 1 <= bad["num_targets"] <= 3
            assert bad["model"][0] == want[2]["model"][0] and np.array_equal(bad["model"][1], want[2]["model"][1])
            with pytest.raises(AssertionError, match="no frame launched"):
                ctx.pmap_frame_end()
        got = _library_step(ctx, frames[f], None, last)
        _same(got, want[f], ("behind a failed frame", f))
        if f > 0:
            assert got["frame_index"] == f
            last = got["pose"]


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason_and_leave_the_context_usable(torch_cuda):
    """Every refusal of the header: ICP_ERR_INVALID_ARGUMENT (AssertionError) with its reason; with the condition lifted the
    same context runs the head of `vmap` like a fresh one."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch
    d = PC.drive("vmap")
    frames = _inputs(torch, d)
    want, _, _ = _plugin_run(torch, "vmap")

    def runs_like_fresh(ctx, what):
        got, _ = _library_run(torch, d, frames, count=3, ctx=ctx)
        for f in range(3):
            _same(got[f], want[f], (what, f))

    ctx = _make_context(d)
    with pytest.raises(AssertionError, match="icp_pmap_odometry_init first"):
        ctx.pmap_frame_launch(frames[0])
    with pytest.raises(AssertionError, match="no frame launched"):
        ctx.pmap_frame_end()
    for ks in (0, 4, 17):
        with pytest.raises(AssertionError, match="normals_kernel_size"):
            _init_sequence(ctx, d, normals_kernel_size=ks)
    with pytest.raises(AssertionError, match="targets is 0 or 1"):
        _init_sequence(ctx, d, targets=2)
    ctx.set_cost("point_to_point_gauss_newton")
    with pytest.raises(AssertionError, match="point-to-point"):
        _init_sequence(ctx, d)
    ctx.set_cost("point_to_plane_gauss_newton")
    ctx.profile_enable(1)
    with pytest.raises(AssertionError, match="profiling"):
        _init_sequence(ctx, d)
    ctx.profile_enable(0)
    ctx.exchange_connect([ctx.exchange_create(0, 1)])  # (a world of one rank: the exchange is on)
    with pytest.raises(AssertionError, match="exchange"):
        _init_sequence(ctx, d)
    ctx.exchange_destroy()
    runs_like_fresh(ctx, "conditions lifted")
    # in the middle of a sequence
    ctx.profile_enable(1)
    with pytest.raises(AssertionError, match="profiling"):
        ctx.pmap_frame_launch(frames[3])
    ctx.profile_enable(0)
    ctx.pmap_frame_launch(frames[3], None, want[2]["pose"])
    with pytest.raises(AssertionError, match="already launched"):
        ctx.pmap_frame_launch(frames[3], None, want[2]["pose"])
    _same(dict(_library_end(ctx)), want[3], ("behind a refused second launch", 3))
    # the vertex-map layout: n = H*W, no timestamps, no grid sample
    with pytest.raises(AssertionError, match="H\\*W"):
        ctx.pmap_frame_launch(frames[4][:, :8].contiguous(), None, want[3]["pose"])
    from pylidar_slam_amd import _lib
    stamps = torch.zeros(d.height * d.width, dtype=torch.float64, device="cuda")
    rc = ctx._lib.icp_pmap_frame_launch(ctx._h, frames[4].data_ptr(), d.height * d.width, _lib.MEM_DEVICE, _lib.FRAME_VERTEX_MAP,
                                        stamps.data_ptr(), None)
    assert rc == _lib.ICP_ERR_INVALID_ARGUMENT and b"timestamps" in ctx._lib.icp_last_error(ctx._h)
    rc = ctx._lib.icp_pmap_frame_launch(ctx._h, frames[4].data_ptr(), d.height * d.width, _lib.MEM_DEVICE, 7, None, None)
    assert rc == _lib.ICP_ERR_INVALID_ARGUMENT and b"layout" in ctx._lib.icp_last_error(ctx._h)
    _same(_library_step(ctx, frames[4], None, want[3]["pose"]), want[4], ("behind refused layouts", 4))
    _init_sequence(ctx, d, voxel_size=0.4)
    with pytest.raises(AssertionError, match="grid sample"):
        ctx.pmap_frame_launch(frames[0])
    runs_like_fresh(ctx, "grid sample off again")
    # a context that holds a projective map is still none for the kd-tree frame calls
    with pytest.raises(AssertionError, match="projective map"):
        ctx.odometry_init()
    # ... and a context that runs a kd-tree sequence is none for these; the kd-tree sequence goes on
    kd = _make_context(d)
    kd.odometry_init(threshold_trans=PC.THRESHOLD_TRANS, threshold_rot=PC.THRESHOLD_ROT, targets=0)
    kd.frame_launch(d.scans[0])
    assert kd.frame_end().frame_index == 0
    with pytest.raises(AssertionError, match="kd-tree sequence"):
        _init_sequence(kd, d)
    kd.frame_launch(d.scans[1])
    assert kd.frame_end().register.iterations == d.max_num_alignments
    # a context held by a batch that still holds kd-tree iterations back (a live stop: chunks)
    live = PC.drive("live")
    a, b = _make_context(live), _make_context(live)
    for c in (a, b):
        c.map_set(live.scans[0])
    batch = IcpBatch([a, b])
    batch.register_launch([live.scans[1], live.scans[1]])
    with pytest.raises(AssertionError, match="held by a batch"):
        _init_sequence(a, live)
    batch.register_end()
    batch.close()
    got, _ = _library_run(torch, live, _inputs(torch, live), count=3, ctx=a)
    live_want, _, _ = _plugin_run(torch, "live")
    for f in range(3):
        _same(got[f], live_want[f], ("batch hold lifted", f))


def _library_end(ctx):
    r = ctx.pmap_frame_end()
    g = r.register
    return dict(kind="frame", pose=g.pose, params=g.params, iterations=g.iterations, losses=g.losses, dx=g.dx,
                key_frame=r.key_frame, inserted=r.inserted, odometry_pc=r.points, samples=r.samples,
                frame_index=r.frame_index, model=_model(ctx))


def test_pmap_odometry_init_restarts_the_sequence(torch_cuda):
    """icp_pmap_odometry_init behind a frame launched and never ended starts over: the second run equals a fresh one."""
    torch = torch_cuda
    d = PC.drive("vmap")
    frames = _inputs(torch, d)
    want, _, _ = _plugin_run(torch, "vmap")
    got, ctx = _library_run(torch, d, frames, count=3)
    ctx.pmap_frame_launch(frames[3], None, got[2]["pose"])  # never ended
    got, _ = _library_run(torch, d, frames, count=4, ctx=ctx)
    for f in range(4):
        _same(got[f], want[f], ("restart", f))


# ---- 5. the plugin's flag ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["vmap", "rows_pixels", "rows_numpy"])
def test_one_call_projective_frame_flag_equals_the_default_path(torch_cuda, name):
    """`one_call_projective_frame=True` against `False` on the same dicts: every entry of every frame's dict, both pose
    lists, and the window and model behind every frame.  `vmap` frames go in as [1,3,H,W] on odd frames."""
    torch = torch_cuda
    d = PC.drive(name)
    frames = _inputs(torch, d)
    want, want_rel, want_abs = _plugin_run(torch, name)
    odo, filters, init = _make_plugin(torch, d, one_call_projective_frame=True)
    ref_odo, ref_filters, ref_init = _make_plugin(torch, d)
    for f in range(d.frames):
        x = frames[f].unsqueeze(0) if (d.kind == "vmap" and f % 2) else frames[f]
        a, b = _frame_dict(d, x, f), _frame_dict(d, x, f)
        ra = _plugin_step(odo, filters, init, a)
        rb = _plugin_step(ref_odo, ref_filters, ref_init, b)
        _same(ra, rb, (name, "flag", f))
        _same(ra, want[f], (name, "flag vs the recorded run", f))
        last_a, last_b = odo.local_map.get_last_frame(), ref_odo.local_map.get_last_frame()  # (the newest stored map's pixels)
        assert np.array_equal(np.asarray(last_a.cpu()), np.asarray(last_b.cpu())), (name, "get_last_frame", f)
        assert set(a) == set(b), (f, sorted(a), sorted(b))
        for k in a:
            u = a[k].detach().cpu().numpy() if isinstance(a[k], torch.Tensor) else np.asarray(a[k])
            v = b[k].detach().cpu().numpy() if isinstance(b[k], torch.Tensor) else np.asarray(b[k])
            assert u.shape == v.shape and u.dtype == v.dtype and np.array_equal(u, v, equal_nan=True), (f, k)
    assert np.array_equal(odo.get_relative_poses(), want_rel) and np.array_equal(np.stack(odo.absolute_poses), want_abs)
