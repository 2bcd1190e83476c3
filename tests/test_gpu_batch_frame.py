"""`-m gpu`: the frame loop of B drives behind two calls (icp_batch_odometry_init / icp_batch_frame_launch /
icp_batch_frame_end, include/icp_mi355x.h).  The yardstick is B single contexts running icp_frame_launch / icp_frame_end on
the same frames: per member and per step pose, parameters, iteration count, losses, steps, key-frame decision, samples,
inserted and odometry_pc, at the end `map_points()` and `map_num_clouds()` — bit for bit.

The drives live in tests/batch_frame_cases.py (three members of different scene and speed, so that one step mixes
insertions with pose-only updates); tests/test_batch_frame_host.py checks on the CPU that no frame of theirs sits within
10 % of a key-frame threshold."""
import numpy as np
import pytest

import batch_frame_cases as BC
import frame_cases as FC
import test_gpu_frame as TF  # (its helpers; the module object is not collected here)
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
def _context(d):
    from pylidar_slam_amd.engine import IcpContext
    return IcpContext(height=d.height, width=d.width, max_num_alignments=d.max_num_alignments,
                      threshold_delta_pose=d.threshold_delta_pose, local_map_size=d.local_map_size, num_neighbors_normals=10)


def _sequence_kw(d, **over):
    kw = dict(voxel_size=d.voxel_size, threshold_trans=FC.THRESHOLD_TRANS, threshold_rot=FC.THRESHOLD_ROT,
              constant_velocity=True, targets=d.targets)
    kw.update(over)
    return kw


def _inputs(torch, d, device):
    """[member][frame] scans and timestamps as the calls take them: host arrays, or cuda tensors made once."""
    if not device:
        return d.scans, d.stamps
    dev = torch.device("cuda:0")
    scans = [[torch.from_numpy(s).to(dev) for s in member] for member in d.scans]
    stamps = None
    if d.stamps:
        stamps = [[torch.from_numpy(t).to(dev) for t in member] if member is not None else None for member in d.stamps]
    return scans, stamps


def _record(r):
    if r is None:
        return None
    if r.frame_index == 0:
        assert r.register.iterations == 0 and np.array_equal(r.pose, EYE) and r.key_frame and r.points is None
        return dict(kind="first", samples=r.samples, inserted=r.inserted, frame_index=0)
    g = r.register
    return dict(kind="frame", pose=g.pose, params=g.params, iterations=g.iterations, losses=g.losses, dx=g.dx,
                key_frame=r.key_frame, inserted=r.inserted, odometry_pc=r.points, samples=r.samples,
                frame_index=r.frame_index)


def _batch_step(batch, scans, stamps=None, inits=None, skip=None, **end):
    batch.frame_launch(scans, stamps, inits, skip)
    return [_record(r) for r in batch.frame_end(**end)]


def _same(a, b, what, skip=()):
    TF._same(a, b, what, skip=skip)
    for k in ("samples", "frame_index", "inserted"):
        if k in a and k in b:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _stamp(stamps, b, f):
    return stamps[b][f] if (stamps and stamps[b] is not None) else None


_SINGLES = {}


def _singles(torch, name, device, members=None):
    """Every member of the drive on a context of its own through icp_frame_launch / icp_frame_end, once per module:
    per member (records, final map, cloud count)."""
    key = (name, device, members)
    if key not in _SINGLES:
        d = BC.drive(name, members)
        scans, stamps = _inputs(torch, d, device)
        out = []
        for b in range(d.members):
            ctx = _context(d)
            ctx.odometry_init(**_sequence_kw(d))
            recs = [TF._library_step(ctx, scans[b][f], _stamp(stamps, b, f)) for f in range(d.frames)]
            assert ctx.handoff_fallbacks() == 0
            out.append((recs, ctx.map_points().copy(), ctx.map_num_clouds()))
            ctx.close()
        _SINGLES[key] = out
    return _SINGLES[key]


def _make_batch(d):
    from pylidar_slam_amd.engine import IcpBatch
    ctxs = [_context(d) for _ in range(d.members)]
    return ctxs, IcpBatch(ctxs)


def _compare_drive(torch, name, device, members=None):
    d = BC.drive(name, members)
    want = _singles(torch, name, device, members)
    scans, stamps = _inputs(torch, d, device)
    ctxs, batch = _make_batch(d)
    batch.odometry_init(**_sequence_kw(d))
    steps = []
    for f in range(d.frames):
        got = _batch_step(batch, [scans[b][f] for b in range(d.members)],
                          [_stamp(stamps, b, f) for b in range(d.members)] if stamps else None)
        for b in range(d.members):
            _same(got[b], want[b][0][f], (name, "member", b, "frame", f))
        steps.append(got)
    for b, ctx in enumerate(ctxs):
        assert np.array_equal(ctx.map_points(), want[b][1]) and ctx.map_num_clouds() == want[b][2], (name, b)
        assert ctx.handoff_fallbacks() == 0
    batch.close()
    return d, steps, ctxs


# ---- 1-4: whole drives ---------------------------------------------------------------------------------------------------
def test_sampled_drives_from_device_tensors_equal_the_single_calls(torch_cuda):
    """Three 32x1024 drives of 10 frames from cuda tensors, grid sample 0.4 m, targets = the pixels of the vertex map, 8
    forced iterations, a window of 3 clouds (evictions within the drive).  At least one step mixes insertions with pose-only
    updates, and one has every member insert."""
    d, steps, ctxs = _compare_drive(torch_cuda, "sampled", True)
    keys = [[bool(r["key_frame"]) for r in step] for step in steps[1:]]
    assert any(0 < sum(k) < d.members for k in keys) and any(all(k) for k in keys), keys
    assert [[f for f, k in enumerate(keys, start=1) if k[b]] for b in range(d.members)] == [list(k) for k in BC.KEY_FRAMES]
    assert all(r["iterations"] == 8 for step in steps[1:] for r in step)
    assert all(c.map_num_clouds() == 3 for c in ctxs)  # (4 or 5 insertions each: evictions happened)
    assert all(r["samples"] == r["odometry_pc"].shape[0] < d.scans[0][0].shape[0] for step in steps[1:] for r in step)


def test_live_stop_drives_equal_the_single_calls(torch_cuda):
    """The same drives with the stop test live (|dx| < 1e-4, at most 15 iterations): chunked batched launches."""
    _, steps, _ = _compare_drive(torch_cuda, "sampled_live", True)
    its = [r["iterations"] for step in steps[1:] for r in step]
    assert all(1 <= i <= 15 for i in its) and any(i < 15 for i in its)


@pytest.mark.parametrize("members", [2, 1])
def test_raw_rows_from_host_arrays_equal_the_single_calls(torch_cuda, members):
    """No grid sample, targets = the frame's rows, 16x512 host arrays (8192 rows) through the batch's one upload, 6 frames;
    B = 2 and B = 1."""
    _, steps, _ = _compare_drive(torch_cuda, "raw", False, members)
    assert all(r["samples"] == 8192 and r["odometry_pc"].shape == (8192, 3) for step in steps[1:] for r in step)


def test_deskewed_members_beside_a_plain_one_equal_the_single_calls(torch_cuda):
    """Timestamps on members 0 and 2 only (host arrays): those are de-skewed by the library's own constant-velocity guess
    inside the batched preprocessing, member 1 passes through; 5 frames."""
    _compare_drive(torch_cuda, "deskew", False)
    plain = _singles(torch_cuda, "sampled", True)
    skewed = _singles(torch_cuda, "deskew", False)
    assert not np.array_equal(plain[0][0][2]["pose"], skewed[0][0][2]["pose"])  # (the de-skew moved something)
    assert np.array_equal(plain[1][0][2]["pose"], skewed[1][0][2]["pose"])      # (member 1 has no timestamps)


# ---- 5: partial steps ------------------------------------------------------------------------------------------------------
def test_partial_steps_equal_singles_fed_the_same_frames(torch_cuda):
    """Ten steps of the sampled drives: member 1 sits steps 3 and 4 out; member 2 is restarted alone with icp_odometry_init
    behind step 4 and begins another drive at frame 0 while the others register.  Every member equals a single context fed
    the same per-member frame list."""
    torch = torch_cuda
    d = BC.drive("sampled")
    scans, _ = _inputs(torch, d, True)
    ctxs, batch = _make_batch(d)
    kw = _sequence_kw(d)
    batch.odometry_init(**kw)
    fed = [[], [], []]       # per member: ("init",) or ("frame", scan)
    got = [[], [], []]
    cursor = [0, 0, 0]
    source = [scans[0], scans[1], scans[2]]
    for step in range(10):
        skip = [False, step in (3, 4), False]
        if step == 5:
            ctxs[2].odometry_init(**kw)
            fed[2].append(("init",))
            source[2], cursor[2] = scans[1], 0  # (another drive: member 1's scene)
        frames = [None if skip[b] else source[b][cursor[b]] for b in range(3)]
        out = _batch_step(batch, frames, skip=skip)
        for b in range(3):
            if skip[b]:
                assert out[b] is None
                continue
            fed[b].append(("frame", frames[b]))
            got[b].append(out[b])
            cursor[b] += 1
        if step == 5:
            assert out[2]["kind"] == "first" and out[0]["kind"] == out[1]["kind"] == "frame"
    for b in range(3):
        ctx = _context(d)
        ctx.odometry_init(**kw)
        want = []
        for item in fed[b]:
            if item[0] == "init":
                ctx.odometry_init(**kw)
            else:
                want.append(TF._library_step(ctx, item[1]))
        assert len(want) == len(got[b]) == (8 if b == 1 else 10)
        for f, (a, w) in enumerate(zip(got[b], want)):
            _same(a, w, ("partial", "member", b, "its frame", f))
        assert np.array_equal(ctxs[b].map_points(), ctx.map_points()) and ctxs[b].map_num_clouds() == ctx.map_num_clouds()
        ctx.close()
    batch.close()


# ---- 6: hand-over ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched_first", [True, False], ids=["batch_alone_batch", "alone_batch_alone"])
def test_hand_over_between_the_batch_and_the_single_calls(torch_cuda, batched_first):
    """Frames 0-2, 3-5 and 6-9 alternate between the batched calls and every member alone: the sequence state is the
    member's own."""
    torch = torch_cuda
    d = BC.drive("sampled")
    want = _singles(torch, "sampled", True)
    scans, _ = _inputs(torch, d, True)
    ctxs, batch = _make_batch(d)
    batch.odometry_init(**_sequence_kw(d))
    for f in range(d.frames):
        batched = (f < 3 or f >= 6) == batched_first
        if batched:
            got = _batch_step(batch, [scans[b][f] for b in range(3)])
        else:
            got = [TF._library_step(ctxs[b], scans[b][f]) for b in range(3)]
        for b in range(3):
            _same(got[b], want[b][0][f], ("hand-over", batched_first, "member", b, "frame", f))
    for b, ctx in enumerate(ctxs):
        assert np.array_equal(ctx.map_points(), want[b][1]) and ctx.map_num_clouds() == want[b][2]
    batch.close()


# ---- 7: a failure beside healthy members --------------------------------------------------------------------------------------
def test_a_failing_member_leaves_its_sequence_and_costs_the_others_nothing(torch_cuda):
    """The plane-over-plane input of tests/test_gpu_batch_direct.py::_plane on member 1 at step 2: InvalidJacobianError
    behind the completed step with `.failed == [1]`; member 1's map and sequence are where they were, members 0 and 2 equal
    their singles; the next step — member 1 on a healthy map again — equals a single context that went the same way."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import InvalidJacobianError
    from test_gpu_batch_direct import _plane
    d = BC.drive("raw", 3)
    want = _singles(torch, "raw", False, 3)
    plane, above = _plane()
    ctxs, batch = _make_batch(d)
    batch.odometry_init(**_sequence_kw(d))
    for f in range(2):
        got = _batch_step(batch, [d.scans[b][f] for b in range(3)])
        for b in range(3):
            _same(got[b], want[b][0][f], ("failure", b, f))
    ctxs[1].map_set(plane)
    before = ctxs[1].map_points().copy()
    batch.frame_launch([d.scans[0][2], above, d.scans[2][2]])
    with pytest.raises(InvalidJacobianError) as raised:
        batch.frame_end()
    e = raised.value
    assert e.failed == [1] and e.results[1] is None and e.result.iterations >= 1
    for b in (0, 2):
        _same(_record(e.results[b]), want[b][0][2], ("failure", b, 2))
    np.testing.assert_array_equal(ctxs[1].map_points(), before)
    assert ctxs[1].map_num_clouds() == 0  # (icp_map_set keeps no cloud bookkeeping: nothing was appended either)
    with pytest.raises(AssertionError, match="no step launched"):
        batch.frame_end()
    # the same way on a context alone
    alone = _context(d)
    alone.odometry_init(**_sequence_kw(d))
    for f in range(2):
        TF._library_step(alone, d.scans[1][f])
    alone.map_set(plane)
    failed = TF._library_step(alone, above)
    assert failed["kind"] == "invalid_jacobian" and failed["iterations"] == e.result.iterations
    assert np.array_equal(failed["losses"], e.result.losses)
    alone.map_set(d.scans[1][1])
    want_1 = TF._library_step(alone, d.scans[1][2])
    ctxs[1].map_set(d.scans[1][1])
    got = _batch_step(batch, [d.scans[0][3], d.scans[1][2], d.scans[2][3]])
    assert got[1]["frame_index"] == 2  # (the failed frame did not advance the sequence)
    _same(got[1], want_1, ("failure", 1, "behind the failure"))
    for b in (0, 2):
        _same(got[b], want[b][0][3], ("failure", b, 3))
    assert np.array_equal(ctxs[1].map_points(), alone.map_points()) and ctxs[1].map_num_clouds() == alone.map_num_clouds()
    batch.close()


# ---- 8: refusals and capacity overflow ----------------------------------------------------------------------------------------
def test_refusals_change_nothing_and_overflow_completes_the_step(torch_cuda):
    """Every refusal of the header; behind each group of them a proper step that equals the singles.  `cap` below a member's
    rows: AssertionError with the count, nothing written for that member, every frame completed."""
    torch = torch_cuda
    d = BC.drive("raw_long")
    want = _singles(torch, "raw_long", False)
    kw = _sequence_kw(d)
    ctxs, batch = _make_batch(d)
    frame = [0]

    def proper(skip=None):
        f = frame[0]
        got = _batch_step(batch, [d.scans[b][f] for b in range(3)], skip=skip)
        for b in range(3):
            if skip and skip[b]:
                assert got[b] is None
            else:
                _same(got[b], want[b][0][f], ("refusals", "member", b, "frame", f))
        frame[0] += 1

    def refused(match, skip=None):
        f = frame[0]
        with pytest.raises(AssertionError, match=match):
            batch.frame_launch([d.scans[b][f] for b in range(3)], skip=skip)
        with pytest.raises(AssertionError, match="no step launched"):  # (nothing was launched)
            batch.frame_end()

    def alone(b):
        f = frame[0]
        _same(TF._library_step(ctxs[b], d.scans[b][f]), want[b][0][f], ("refusals", "member", b, "alone", f))

    # ---- before and at frame 0
    refused("member 0: no sequence")
    batch.odometry_init(**kw)
    refused("every member is skipped", skip=[True] * 3)
    ctxs[1].odometry_init(**dict(kw, voxel_size=0.4))
    refused("member 1: voxel_size differs")
    ctxs[1].odometry_init(**dict(kw, targets=1))
    refused("member 1: targets differs")
    ctxs[1].odometry_init(**kw)
    ctxs[2].frame_launch(d.scans[2][0])  # frame 0 launched alone: no registration, a frame of its own
    refused("member 2: a frame of the member's own awaits icp_frame_end")
    r = ctxs[2].frame_end()
    assert r.frame_index == 0 and r.inserted == want[2][0][0]["inserted"]
    proper(skip=[False, False, True])  # frame 0 of members 0 and 1
    # ---- frame 1
    ctxs[2].set_cost("point_to_point_gauss_newton")
    refused("member 2: the member runs point-to-point")
    ctxs[2].set_cost("point_to_plane_gauss_newton")
    proper()
    # ---- frame 2: a second launch, and the batch ends what it launched
    batch.frame_launch([d.scans[b][2] for b in range(3)])
    with pytest.raises(AssertionError, match="a step is already launched"):
        batch.frame_launch([d.scans[b][2] for b in range(3)])
    with pytest.raises(AssertionError, match="launched by a batch"):
        ctxs[0].frame_end()
    with pytest.raises(AssertionError, match="launched by a batch"):
        ctxs[0].odometry_init(**kw)
    got = [_record(r) for r in batch.frame_end()]
    for b in range(3):
        _same(got[b], want[b][0][2], ("refusals", "member", b, "frame", 2))
    frame[0] = 3
    # ---- frames 3-6: the states of a member's context
    ctxs[0].pmap_init()
    ctxs[0].pmap_update(EYE, ctxs[0].project(d.scans[0][0]))
    refused("member 0: the member holds a projective map")
    ctxs[0].pmap_init()
    proper()
    ctxs[1].exchange_connect([ctxs[1].exchange_create(0, 1)])
    refused("member 1: a multi-GPU exchange")
    ctxs[1].exchange_destroy()
    proper()
    ctxs[2].profile_enable(1)
    refused("member 2: profiling")
    ctxs[2].profile_enable(0)
    proper()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ctxs[1].use_torch_stream()
    refused("member 1: the members must enqueue on one stream")
    ctxs[1].use_torch_stream()
    proper()
    # ---- frame 7: `cap` below member 0's rows: the count comes back, nothing is written for it, every frame is completed
    batch.frame_launch([d.scans[b][7] for b in range(3)])
    with pytest.raises(AssertionError, match="member 0: odometry_pc_out holds fewer rows") as raised:
        batch.frame_end(cap=[100, 8192, 8192])
    e = raised.value
    assert e.rows == [8192, 8192, 8192] and e.failed == [] and e.results[0].points is None
    for b in range(3):
        _same(_record(e.results[b]), want[b][0][7], ("overflow", b), skip=("odometry_pc",) if b == 0 else ())
    frame[0] = 8
    # ---- frame 8: a member in a registration of its own, then with a frame of its own behind frame 0 (which IS a registration
    # that awaits its end): refused; that frame is ended alone and the member sits the step out
    ctxs[2].register_launch(d.scans[2][8])
    refused("member 2: a registration of the member's own")
    ctxs[2].register_end()
    ctxs[2].frame_launch(d.scans[2][8])
    refused("member 2: a registration of the member's own")
    _same(TF._record("frame", **{k: v for k, v in _record(ctxs[2].frame_end()).items() if k != "kind"}), want[2][0][8],
          ("refusals", "member 2 alone", 8))
    proper(skip=[False, False, True])
    proper()  # frame 9
    assert frame[0] == d.frames
    for b, ctx in enumerate(ctxs):
        assert np.array_equal(ctx.map_points(), want[b][1]) and ctx.map_num_clouds() == want[b][2]
    batch.close()


# ---- 9: the plugin's flag ------------------------------------------------------------------------------------------------------
def _dict_values_equal(torch, a, b, what):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        x = a[k].detach().cpu().numpy() if isinstance(a[k], torch.Tensor) else np.asarray(a[k])
        y = b[k].detach().cpu().numpy() if isinstance(b[k], torch.Tensor) else np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True), (what, k)


@pytest.mark.parametrize("kind", ["cuda", "numpy"])
def test_batched_plugin_flag_equals_the_default_path(torch_cuda, kind):
    """`MI355XICPFrameToModelBatch(one_call_frame=True)` on the same dicts as its default path: every entry of every
    frame's dict (`odometry_pose`, `odometry_pc`, ...), the relative and absolute poses and the maps, bit for bit.  cuda
    frames (the device-resident grid sample in front): against the per-call batched plugin.  numpy frames, which the
    per-call batched plugin does not take: against the per-call single plugin on every member's frames — the path the
    batched plugin is itself held to (tests/test_gpu_batch_loop.py)."""
    torch = torch_cuda
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    d = BC.drive("sampled" if kind == "cuda" else "raw", 3)
    singles = [BC.single_drive(d, b) for b in range(3)]
    cfg = FC.plugin_config(singles[0])
    proj = our.SphericalProjector(d.height, d.width)
    flagged = our.MI355XICPFrameToModelBatch(FC.plugin_config(singles[0], one_call_frame=True), 3, projector=proj, device=dev)
    flagged.init()
    if kind == "cuda":
        plain = our.MI355XICPFrameToModelBatch(cfg, 3, projector=proj, device=dev)
        plain.init()
        plain_members = plain.members
    else:
        plain_members = [our.MI355XICPFrameToModel(cfg, projector=proj, device=dev) for _ in range(3)]
        for m in plain_members:
            m.init()
    chains = []
    for _ in range(2):  # (filters and initialisation modules of each path's own)
        inits = [our.ConstantVelocityInitialization() for _ in range(3)]
        for i in inits:
            i.init()
        chains.append(([TF._filters(singles[b], dev) for b in range(3)], inits))
    for f in range(d.frames):
        dicts = []
        for filters, inits in chains:
            step = []
            for b in range(3):
                data = {"numpy_pc": d.scans[b][f]}
                inits[b].next_frame(data)
                for flt in filters[b]:
                    flt.filter(data)
                step.append(data)
            dicts.append(step)
        flagged.process_next_frames(dicts[0])
        if kind == "cuda":
            plain.process_next_frames(dicts[1])
        else:
            for m, data in zip(plain_members, dicts[1]):
                m.process_next_frame(data)
        for b in range(3):
            _dict_values_equal(torch, dicts[0][b], dicts[1][b], (kind, "member", b, "frame", f))
            if f > 0:
                for (_, inits), step in zip(chains, dicts):
                    inits[b].save_real_motion(step[b]["odometry_pose"], step[b])
                a, w = flagged.members[b].last_result, plain_members[b].last_result
                assert a.iterations == w.iterations and np.array_equal(a.losses, w.losses) and np.array_equal(a.dx, w.dx)
                assert "odometry_pc" in dicts[0][b] and "odometry_pose" in dicts[0][b]
    keys = 0
    for b in range(3):
        assert np.array_equal(flagged.get_relative_poses(b), plain_members[b].get_relative_poses())
        assert np.array_equal(np.stack(flagged.members[b].absolute_poses), np.stack(plain_members[b].absolute_poses))
        assert np.array_equal(flagged.members[b].ctx.map_points(), plain_members[b].ctx.map_points())
        assert flagged.members[b].ctx.map_num_clouds() == plain_members[b].ctx.map_num_clouds()
        keys += flagged.members[b].ctx.map_num_clouds()
    assert keys >= 6


# ---- 10: the published loop ------------------------------------------------------------------------------------------------------
def test_published_loop_for_two_drives_matches_the_reference_and_the_single_calls(torch_cuda, golden_loop, loop_scans):
    """B = 2 on the published configuration's 36-frame loop: member 0 runs the frames of tests/test_gpu_loop.py and is held
    to tests/golden/loop_reference.npz with that file's bars (every frame within 1e-4 m / 1e-4 rad — one iteration more or
    less only where the reference's own stop was within 2 % of the threshold, then off by at most that step more — map sizes
    within 2 points, 30 clouds at the end, ATE / ARE / tr_err equal to 2e-5); member 1 runs another scene.  Both members are
    bit-equal to single frame calls."""
    import os
    import icp_oracle as O
    from conftest import GOLDEN
    from pylidar_slam_amd.engine import IcpBatch, IcpContext
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    g = golden_loop
    spread = np.load(os.path.join(GOLDEN, "loop_spread.npz"))
    assert bool(spread["base_reproduces_loop_reference"])
    scans, gt_abs = loop_scans
    other = make_sequence(SceneConfig(height=64, width=2048, seed=2234), len(scans))[0]
    drives = [scans, other]

    def context():
        return IcpContext(height=64, width=2048, max_num_alignments=20, threshold_delta_pose=1.0e-4, scheme="neighborhood",
                          sigma=0.2, local_map_size=30, num_neighbors_normals=10)

    kw = dict(voxel_size=0.4, threshold_trans=0.1, threshold_rot=0.3, constant_velocity=True, targets=1)
    want = []
    for drive in drives:
        ctx = context()
        ctx.odometry_init(**kw)
        want.append(([TF._library_step(ctx, s) for s in drive], ctx.map_points().copy(), ctx.map_num_clouds()))
        ctx.close()
    ctxs = [context(), context()]
    batch = IcpBatch(ctxs)
    batch.odometry_init(**kw)
    rel, flips, worst = [], [], (0.0, 0.0)
    for f in range(len(scans)):
        batch.frame_launch([drives[0][f], drives[1][f]])
        res = batch.frame_end()
        for b in range(2):
            _same(_record(res[b]), want[b][0][f], ("published loop", "member", b, "frame", f))
        r = res[0]
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
        assert abs(ctxs[0].map_size() - int(g["map_sizes"][f])) <= 2, (f, ctxs[0].map_size(), int(g["map_sizes"][f]))
        assert r.key_frame and r.points.shape[0] == r.samples == r.inserted
    assert ctxs[0].map_num_clouds() == 30 and all(c.handoff_fallbacks() == 0 for c in ctxs)
    for b in range(2):
        assert np.array_equal(ctxs[b].map_points(), want[b][1]) and ctxs[b].map_num_clouds() == want[b][2]
    ate, are, tr, rot, n = trajectory_metrics(np.stack(rel), gt_abs, g["segments"])
    print(f"batched frame calls, published loop: worst frame {worst[0]:.1e} m / {worst[1]:.1e} rad vs the reference; ATE "
          f"{ate:.4e} (reference {g['ate'][0]:.4e}) m, tr_err {tr:.4e} ({g['kitti'][0]:.4e}) m/m; flips {flips}")
    assert n == int(g["num_segments"])
    assert abs(ate - g["ate"][0]) < 2e-5 and abs(are - g["are"][0]) < 2e-5
    assert abs(tr - g["kitti"][0]) < 2e-5
    assert rot < 1e-3 and len(flips) <= 3
    batch.close()
