"""`-m gpu`: the projective frame calls for B sequences (icp_batch_pmap_odometry_init / icp_batch_pmap_frame_launch /
icp_batch_pmap_frame_end, include/icp_mi355x.h) against the single calls (icp_pmap_frame_launch / icp_pmap_frame_end) on the
same frames, per member and bit for bit: pose, parameters, iteration count, losses, steps, key-frame decision, samples,
odometry_pc, and the window and model behind every step.  A schedule is a list of steps, a step a list with one frame per
member (None: the member sits the step out); the reference of a member is a single context fed its frames in order."""
import numpy as np
import pytest

import pmap_frame_cases as PC

pytestmark = pytest.mark.gpu

H, W, ITERS, LMS = 16, 512, 6, 2
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _ctx(**over):
    from pylidar_slam_amd.engine import IcpContext
    kw = dict(height=H, width=W, max_num_alignments=ITERS, threshold_delta_pose=0.0, local_map_size=LMS)
    kw.update(over)
    return IcpContext(**kw)


_SCANS = {}


def _scans(seed, frames=9):
    """0.4 m per frame (the key-frame rhythm of tests/pmap_frame_cases.py), another scene per seed."""
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    if seed not in _SCANS:
        _SCANS[seed] = make_sequence(SceneConfig(height=H, width=W, seed=seed), frames)[0]
    return _SCANS[seed]


_VMAPS = {}


def _vmaps(torch, seed):
    if seed not in _VMAPS:
        ctx = _ctx()
        _VMAPS[seed] = [ctx.project(torch.from_numpy(s).cuda()).clone() for s in _scans(seed)]
        torch.cuda.synchronize()
        ctx.close()
    return _VMAPS[seed]


def _few_pixels(torch, vmap):
    flat = vmap.reshape(3, -1)
    valid = torch.nonzero(flat.abs().amax(dim=0) > 0).reshape(-1)
    keep = valid[torch.linspace(0, valid.numel() - 1, 5).long()[1:4]]
    out = torch.zeros_like(flat)
    out[:, keep] = flat[:, keep]
    return out.reshape(vmap.shape).contiguous()


INIT = dict(threshold_trans=PC.THRESHOLD_TRANS, threshold_rot=PC.THRESHOLD_ROT, constant_velocity=True, normals_kernel_size=5)


def _model(ctx):
    mv, mn = ctx.pmap_model()
    return ctx.pmap_num_maps(), mv, mn


def _rec(r, ctx):
    if r is None:
        return dict(kind="invalid", model=_model(ctx))
    g = r.register
    return dict(kind="first" if r.frame_index == 0 else "frame", pose=g.pose, params=g.params, iterations=g.iterations,
                losses=g.losses, dx=g.dx, key_frame=r.key_frame, inserted=r.inserted, samples=r.samples, frame_index=r.frame_index,
                points=r.points, model=_model(ctx))


def _single_step(ctx, frame):
    from pylidar_slam_amd.engine import InvalidJacobianError
    ctx.pmap_frame_launch(frame)
    try:
        return _rec(ctx.pmap_frame_end(), ctx)
    except InvalidJacobianError:
        return _rec(None, ctx)


def _batch_step(batch, step):
    from pylidar_slam_amd.engine import InvalidJacobianError
    skip = [f is None for f in step]
    batch.pmap_frame_launch(step, skip=skip)
    try:
        results = batch.pmap_frame_end()
    except InvalidJacobianError as e:
        results = e.results
        assert e.failed and all(results[i] is None and not skip[i] for i in e.failed)
    return [None if sk else _rec(r, c) for r, c, sk in zip(results, batch.contexts, skip)]


def _same(a, b, what):
    assert a["kind"] == b["kind"], (what, a["kind"], b["kind"])
    assert a["model"][0] == b["model"][0], (what, "pmap_num_maps")
    assert np.array_equal(a["model"][1], b["model"][1]) and np.array_equal(a["model"][2], b["model"][2]), (what, "pmap_model")
    if a["kind"] == "invalid":
        return
    for k in ("pose", "params", "losses", "dx"):
        assert np.array_equal(a[k], b[k]), (what, k)
    for k in ("iterations", "key_frame", "inserted", "samples", "frame_index"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert (a["points"] is None) == (b["points"] is None), (what, "points")
    if a["points"] is not None:
        assert a["points"].shape == b["points"].shape and np.array_equal(a["points"], b["points"]), (what, "odometry_pc")


def _run_schedule(schedule, init=INIT, **ctx_over):
    """The schedule through one batch, and every member's frames through a single context of its own: both record lists per
    member.  Returns (batched, single, batch contexts)."""
    from pylidar_slam_amd.engine import IcpBatch
    count = len(schedule[0])
    ctxs = [_ctx(**ctx_over) for _ in range(count)]
    batch = IcpBatch(ctxs)
    batch.pmap_odometry_init(**init)
    got = [[] for _ in range(count)]
    for step in schedule:
        for b, r in enumerate(_batch_step(batch, step)):
            if r is not None:
                got[b].append(r)
    want = []
    for b in range(count):
        ctx = _ctx(**ctx_over)
        ctx.pmap_odometry_init(**init)
        want.append([_single_step(ctx, step[b]) for step in schedule if step[b] is not None])
        ctx.close()
    return got, want, batch


def _compare(got, want, label):
    for b, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), (label, b)
        for f, (x, y) in enumerate(zip(g, w)):
            _same(x, y, (label, "member", b, "frame", f))


def _kinds(records):
    return [r["kind"] for r in records]


# ---- 1. whole drives ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [3, 1])
def test_batched_drives_equal_the_single_calls(torch_cuda, count):
    """B = 3 (three scenes) and B = 1, vertex maps in, 7 frames, a window of 2: key frames, pose-only frames and evictions."""
    seqs = [_vmaps(torch_cuda, 4100 + 111 * b) for b in range(count)]
    got, want, batch = _run_schedule([[s[f] for s in seqs] for f in range(7)])
    _compare(got, want, f"B = {count}")
    for g in got:
        keys = [r["key_frame"] for r in g[1:]]
        assert any(keys) and not all(keys) and sum(keys) + 1 > LMS and g[-1]["model"][0] == LMS
        assert all(r["iterations"] == ITERS and r["points"].shape[0] > 0 for r in g[1:])


def test_offset_members_mix_insertions_and_pose_only_updates(torch_cuda):
    """Member b joins b steps late: its key frames fall on other steps than its neighbours', so every step from the third on
    has insertions and pose-only updates in ONE icp_batch_pmap_update — and first frames beside registering members."""
    v = [_vmaps(torch_cuda, 4100 + 111 * b) for b in range(3)]
    schedule = [[v[b][f - b] if 0 <= f - b < 7 else None for b in range(3)] for f in range(8)]
    got, want, _ = _run_schedule(schedule)
    _compare(got, want, "offset")
    mixed = 0
    for f in range(2, 7):
        keys = {got[b][f - b]["key_frame"] for b in range(3) if 1 <= f - b < len(got[b])}
        mixed += keys == {True, False}
    assert mixed >= 3


def test_skipping_late_and_restarted_members(torch_cuda):
    """Member 1 sits steps 2 and 3 out and comes back; member 2 starts at step 3 (frame 0 beside registering members)."""
    v = [_vmaps(torch_cuda, 4100 + 111 * b) for b in range(3)]
    schedule = [[v[0][0], v[1][0], None], [v[0][1], v[1][1], None], [v[0][2], None, None], [v[0][3], None, v[2][0]],
                [v[0][4], v[1][2], v[2][1]], [v[0][5], v[1][3], v[2][2]]]
    got, want, _ = _run_schedule(schedule)
    _compare(got, want, "skip / late")
    assert [len(g) for g in got] == [6, 4, 3]


def test_degenerate_members_beside_healthy_ones(torch_cuda):
    """Step 3: member 0 gets an all-null vertex map (no row: the residual-norm guard ends its loop with ICP_OK and the guess,
    as on the single call), member 2 three pixels (Invalid Jacobian: its map and sequence stay, the call reports it after
    the others have completed); every member's later frames equal the single run that met the same frames."""
    torch = torch_cuda
    v = [_vmaps(torch, 4100 + 111 * b) for b in range(3)]
    schedule = [[s[f] for s in v] for f in range(3)]
    schedule.append([torch.zeros_like(v[0][3]), v[1][3], _few_pixels(torch, v[2][3])])
    schedule += [[s[f] for s in v] for f in range(3, 6)]
    got, want, _ = _run_schedule(schedule)
    _compare(got, want, "degenerate")
    assert _kinds(got[2])[3] == "invalid" and _kinds(got[0])[3] == "frame" and got[0][3]["iterations"] == 1
    assert got[2][4]["frame_index"] == 3 and got[1][4]["frame_index"] == 4


def test_nine_member_masks_at_b4_evict_an_inner_batch(torch_cuda):
    """B = 4, nine distinct sets of registering members in a row (the cache of inner batches holds 8), then the first set
    again (created anew)."""
    v = [_vmaps(torch_cuda, 4100 + 111 * b) for b in range(4)]
    masks = [0b0011, 0b0101, 0b1001, 0b0110, 0b1010, 0b1100, 0b0111, 0b1011, 0b1101, 0b0011]
    nxt = [1] * 4
    schedule = [[s[0] for s in v]]
    for m in masks:
        step = []
        for b in range(4):
            take = bool(m >> b & 1) and nxt[b] < 9
            step.append(v[b][nxt[b]] if take else None)
            nxt[b] += take
        schedule.append(step)
    assert len({tuple(f is None for f in s) for s in schedule[1:]}) == 9
    got, want, _ = _run_schedule(schedule)
    _compare(got, want, "masks")
    assert all(len(g) >= 5 for g in got)


def test_member_stepped_single_then_batch_then_single(torch_cuda):
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch
    v = [_vmaps(torch, 4100 + 111 * b) for b in range(2)]
    ctxs = [_ctx(), _ctx()]
    batch = IcpBatch(ctxs)
    batch.pmap_odometry_init(**INIT)
    got = [[], []]
    for f in range(7):
        if f in (1, 2, 5):  # alone, member by member
            for b in range(2):
                got[b].append(_single_step(ctxs[b], v[b][f]))
        else:
            for b, r in enumerate(_batch_step(batch, [v[0][f], v[1][f]])):
                got[b].append(r)
    for b in range(2):
        ctx = _ctx()
        ctx.pmap_odometry_init(**INIT)
        for f in range(7):
            _same(got[b][f], _single_step(ctx, v[b][f]), ("hand-over", b, f))
    # a frame the batch has launched is the batch's to end
    batch.pmap_odometry_init(**INIT)
    batch.pmap_frame_launch([v[0][0], v[1][0]])
    with pytest.raises(AssertionError, match="launched by a batch"):
        ctxs[0].pmap_frame_end()
    assert all(r.frame_index == 0 for r in batch.pmap_frame_end())


@pytest.mark.parametrize("kind", ["rows_host", "rows_device", "rows_device_sampled"])
def test_rows_layout_from_host_and_device_equals_the_single_calls(torch_cuda, kind):
    """[N,3] rows: host arrays through the batch's ONE pinned arena (targets = the rows), cuda tensors (targets = the pixels),
    and cuda tensors behind the batched grid sample (0.4 m)."""
    torch = torch_cuda
    seqs = [_scans(4100 + 111 * b) for b in range(3)]
    if kind != "rows_host":
        seqs = [[torch.from_numpy(s).cuda() for s in seq] for seq in seqs]
    init = dict(INIT, targets=0 if kind == "rows_host" else 1, voxel_size=0.4 if kind == "rows_device_sampled" else 0.0)
    got, want, _ = _run_schedule([[s[f] for s in seqs] for f in range(5)], init=init)
    _compare(got, want, kind)
    for g in got:
        assert any(r["key_frame"] for r in g[1:]) and not all(r["key_frame"] for r in g[1:])
        if kind == "rows_device_sampled":
            assert all(r["samples"] == r["points"].shape[0] < H * W for r in g[1:])


def test_refusals_change_nothing(torch_cuda):
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch
    v = [_vmaps(torch, 4100 + 111 * b) for b in range(2)]
    ctxs = [_ctx(), _ctx()]
    batch = IcpBatch(ctxs)
    with pytest.raises(AssertionError, match=r"member 0: no sequence .*nothing was changed"):
        batch.pmap_frame_launch([v[0][0], v[1][0]])
    with pytest.raises(AssertionError, match="no step launched"):
        batch.pmap_frame_end()
    with pytest.raises(AssertionError, match="normals_kernel_size"):
        batch.pmap_odometry_init(**dict(INIT, normals_kernel_size=4))
    batch.pmap_odometry_init(**INIT)
    with pytest.raises(AssertionError, match="every member is skipped"):
        batch.pmap_frame_launch([None, None], skip=[True, True])
    with pytest.raises(AssertionError, match=r"member 1: a vertex map has n = H\*W"):
        batch.pmap_frame_launch([v[0][0], v[1][0][:, :8].contiguous()])
    ctxs[1].pmap_odometry_init(**dict(INIT, normals_kernel_size=3))
    with pytest.raises(AssertionError, match="member 1: normals_kernel_size differs"):
        batch.pmap_frame_launch([v[0][0], v[1][0]])
    ctxs[1].pmap_odometry_init(**INIT)
    ctxs[1].set_cost("point_to_point_gauss_newton")
    with pytest.raises(AssertionError, match="member 1: the member runs point-to-point"):
        batch.pmap_frame_launch([v[0][0], v[1][0]])
    ctxs[1].set_cost("point_to_plane_gauss_newton")
    batch.pmap_frame_launch([v[0][0], v[1][0]])
    with pytest.raises(AssertionError, match="a step is already launched"):
        batch.pmap_frame_launch([v[0][1], v[1][1]])
    assert all(r.frame_index == 0 for r in batch.pmap_frame_end())
    # after all of it the batch runs the drive like a fresh one
    got = [[], []]
    for f in range(1, 4):
        for b, r in enumerate(_batch_step(batch, [v[0][f], v[1][f]])):
            got[b].append(r)
    for b in range(2):
        ctx = _ctx()
        ctx.pmap_odometry_init(**INIT)
        _single_step(ctx, v[b][0])
        for f in range(1, 4):
            _same(got[b][f - 1], _single_step(ctx, v[b][f]), ("behind the refusals", b, f))
    # a member on a kd-tree sequence is none for the projective step, and the kd-tree batch calls still refuse a projective map
    kd = _ctx()
    kd.odometry_init(targets=0)
    mixed = IcpBatch([ctxs[0], kd])
    with pytest.raises(AssertionError, match="member 1: a kd-tree sequence"):
        mixed.pmap_frame_launch([v[0][4], v[1][4]])
    with pytest.raises(AssertionError, match="projective map"):
        batch.odometry_init()


def test_one_pending_step_per_batch_whatever_its_kind(torch_cuda):
    """A batch over a projective and a kd-tree member: while a step of one kind awaits its end, a launch of the other kind is
    refused with nothing changed — the pending step is then ended by its own end call, and the other kind runs."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch
    v = _vmaps(torch, 4100)
    rows = [torch.from_numpy(s).cuda() for s in _scans(4211)[:2]]
    pm, kd = _ctx(), _ctx()
    pm.pmap_odometry_init(**INIT)
    kd.odometry_init(targets=0)
    mixed = IcpBatch([pm, kd])
    mixed.pmap_frame_launch([v[0], None], skip=[False, True])
    with pytest.raises(AssertionError, match=r"icp_batch_frame_launch: a projective step of this batch awaits "
                                             r"icp_batch_pmap_frame_end \(nothing was changed\)"):
        mixed.frame_launch([None, rows[0]], skip=[True, False])
    with pytest.raises(AssertionError, match="no step launched"):
        mixed.frame_end()
    first = mixed.pmap_frame_end()
    assert first[0].frame_index == 0 and first[1] is None
    mixed.frame_launch([None, rows[0]], skip=[True, False])
    with pytest.raises(AssertionError, match=r"icp_batch_pmap_frame_launch: a kd-tree step of this batch awaits "
                                             r"icp_batch_frame_end \(nothing was changed\)"):
        mixed.pmap_frame_launch([v[1], None], skip=[False, True])
    first = mixed.frame_end()
    assert first[0] is None and first[1].frame_index == 0
    # both members go on from where they stood
    mixed.pmap_frame_launch([v[1], None], skip=[False, True])
    assert mixed.pmap_frame_end()[0].frame_index == 1
    mixed.frame_launch([None, rows[1]], skip=[True, False])
    assert mixed.frame_end()[1].frame_index == 1
    mixed.close()
    for c in (pm, kd):
        c.close()


# ---- the plugins' flag ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["vmap", "rows_device", "rows_host"])
def test_batch_plugin_flag_equals_the_single_plugin_without_it(torch_cuda, kind):
    """`MI355XICPFrameToModelBatch` with `one_call_projective_frame` (B = 3) against per-call single plugins on the same dicts
    (the per-call batch plugin takes no numpy frames; tests/test_gpu_batch_projective.py holds it to the single plugin): every
    entry of every dict, both pose lists, `get_last_frame`, windows and models."""
    torch = torch_cuda
    from pylidar_slam_amd import odometry as our
    d = PC.drive("vmap")
    dev = torch.device("cuda:0")
    if kind == "vmap":
        seqs = [_vmaps(torch, 4100 + 111 * b) for b in range(3)]
    elif kind == "rows_device":
        seqs = [[torch.from_numpy(s).cuda() for s in _scans(4100 + 111 * b)] for b in range(3)]
    else:
        seqs = [_scans(4100 + 111 * b) for b in range(3)]
    cfg = lambda **over: PC.plugin_config(d, max_num_alignments=ITERS, **over)
    proj = our.SphericalProjector(H, W)
    flagged = our.MI355XICPFrameToModelBatch(cfg(one_call_projective_frame=True), 3, projector=proj, device=dev)
    singles = [our.MI355XICPFrameToModel(cfg(), projector=proj, device=dev) for _ in range(3)]
    flagged.init()
    for m in singles:
        m.init()
    last = [None] * 3
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    for f in range(6):
        a = [{"input_data": s[f], "init_rpose": last[b]} for b, s in enumerate(seqs)]
        bb = [{"input_data": s[f], "init_rpose": last[b]} for b, s in enumerate(seqs)]
        flagged.process_next_frames(a)
        for m, x in zip(singles, bb):
            m.process_next_frame(x)
        for b in range(3):
            assert set(a[b]) == set(bb[b]), (f, b)
            for k in a[b]:
                if a[b][k] is None:
                    assert bb[b][k] is None
                    continue
                u, w = as_np(a[b][k]), as_np(bb[b][k])
                assert u.shape == w.shape and u.dtype == w.dtype and np.array_equal(u, w, equal_nan=True), (f, b, k)
            fm, sm = flagged.members[b], singles[b]
            assert fm.ctx.pmap_num_maps() == sm.ctx.pmap_num_maps()
            assert all(np.array_equal(x, y) for x, y in zip(fm.ctx.pmap_model(), sm.ctx.pmap_model())), (f, b, "model")
            assert np.array_equal(as_np(fm.local_map.get_last_frame()), as_np(sm.local_map.get_last_frame())), (f, b, "get_last_frame")
            if f > 0:
                last[b] = a[b]["odometry_pose"]
                assert np.array_equal(fm.last_result.losses, sm.last_result.losses)
    for b in range(3):
        assert np.array_equal(flagged.get_relative_poses(b), singles[b].get_relative_poses())
        assert np.array_equal(np.stack(flagged.members[b].absolute_poses), np.stack(singles[b].absolute_poses))
