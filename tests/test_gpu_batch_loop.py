"""`-m gpu`: the batched published-configuration loop — `MI355XICPFrameToModelBatch` and `icp_batch_map_update_staged`.

B sequences advance together: one launch per ICP iteration for all B registrations (`icp_batch_register_launch`) and
ONE map update for all B maps — key-frame insertion, eviction, grid rebuild, neighbourhood lists and eager normals
(ICPFrameToModel.__update_map, slam/odometry/icp_odometry.py:360-380; KdTreeLocalMap.update, local_map.py:302-362).
Per sequence everything must be what the single plugin / the single context computes on the same frames, bit for bit:
poses, iteration counts, losses, steps, maps, windows and normals."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_loop import _filters
from test_loop_reference import golden_loop, loop_scans, published_config  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

H, W = 64, 2048


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _scans(seed, step, frames, yaw_rate=0.01, with_motion=False):
    """A synthetic drive; with_motion: also the ground-truth relative pose of every frame in its predecessor's frame."""
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    scans, gt = make_sequence(SceneConfig(height=H, width=W, seed=seed, step=step, yaw_rate=yaw_rate), frames)
    if not with_motion:
        return scans
    rel = [np.eye(4, dtype=np.float32)] + [(np.linalg.inv(gt[k - 1]) @ gt[k]).astype(np.float32) for k in range(1, frames)]
    return scans, rel


@pytest.fixture(scope="module")
def other_sequences():
    """Three more 36-frame drives: other seeds, other speeds."""
    return [_scans(2234, 0.3, 36), _scans(3234, 0.5, 36), _scans(4234, 0.25, 36)]


@pytest.fixture(scope="module")
def mixed_sequences():
    """One slow drive (2 cm and 0.06 degrees per frame: most frames stay below both key-frame thresholds, 0.1 m / 0.3
    degrees) and two fast ones, 16 frames each."""
    return [_scans(5234, 0.02, 16, yaw_rate=0.001), _scans(6234, 0.4, 16), _scans(7234, 0.35, 16)]


def _record(res):
    return (res.pose.copy(), int(res.iterations), res.losses.copy(), res.dx.copy())


def _run_single(torch, scans, cfg, options, probe=None):
    """The sequence through MI355XICPFrameToModel alone (device-resident preprocessing): per frame (pose, iterations,
    losses, steps), the map, the window size and the plugin's trajectory.  `probe(0, ctx, f)`: called on the live
    context behind every registered frame f (the update of the map by that frame included)."""
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    odo = our.MI355XICPFrameToModel(cfg, projector=our.SphericalProjector(H, W), device=dev)
    for k, v in options.items():
        odo.ctx.set_option(k, v)
    filters = _filters("device", dev)
    init = our.ConstantVelocityInitialization()
    odo.init()
    init.init()
    out = []
    for f, scan in enumerate(scans):
        d = {"numpy_pc": scan}
        init.next_frame(d)
        for flt in filters:
            flt.filter(d)
        odo.process_next_frame(d)
        if f > 0:
            init.save_real_motion(d["odometry_pose"], d)
            assert np.array_equal(d["odometry_pose"], odo.last_result.pose)
            out.append(_record(odo.last_result))
            if probe is not None:
                probe(0, odo.ctx, f)
    result = (out, odo.ctx.map_points(), odo.ctx.map_num_clouds(), odo.get_relative_poses())
    odo.ctx.close()
    return result


def _run_batch(torch, sequences, cfg, options, probe=None):
    """The same sequences through MI355XICPFrameToModelBatch: per member what _run_single returns.  `probe(b, ctx, f)`:
    called on every member's live context behind every registered frame f."""
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    count = len(sequences)
    odo = our.MI355XICPFrameToModelBatch(cfg, count, projector=our.SphericalProjector(H, W), device=dev)
    for m, opts in zip(odo.members, options):
        for k, v in opts.items():
            m.ctx.set_option(k, v)
    filters = [_filters("device", dev) for _ in range(count)]
    inits = [our.ConstantVelocityInitialization() for _ in range(count)]
    odo.init()
    for i in inits:
        i.init()
    out = [[] for _ in range(count)]
    for f in range(len(sequences[0])):
        dicts = []
        for b in range(count):
            d = {"numpy_pc": sequences[b][f]}
            inits[b].next_frame(d)
            for flt in filters[b]:
                flt.filter(d)
            dicts.append(d)
        odo.process_next_frames(dicts)
        if f == 0:
            assert all("odometry_pose" not in d for d in dicts)
            continue
        for b, d in enumerate(dicts):
            inits[b].save_real_motion(d["odometry_pose"], d)
            assert d["odometry_pc"] is d["distorted"]  # icp_odometry.py:210-211, as the single plugin
            res = odo.members[b].last_result
            assert np.array_equal(d["odometry_pose"], res.pose)
            out[b].append(_record(res))
        if probe is not None:
            for b in range(count):
                probe(b, odo.members[b].ctx, f)
    result = [(out[b], odo.members[b].ctx.map_points(), odo.members[b].ctx.map_num_clouds(), odo.get_relative_poses(b))
              for b in range(count)]
    odo.batch.close()
    return result


def _assert_same_run(single, batched, label):
    (s_frames, s_map, s_clouds, s_rel), (b_frames, b_map, b_clouds, b_rel) = single, batched
    assert len(s_frames) == len(b_frames)
    for f, (s, b) in enumerate(zip(s_frames, b_frames), start=1):
        assert np.array_equal(s[0], b[0]), (label, f, "pose")
        assert s[1] == b[1], (label, f, "iterations", s[1], b[1])
        assert np.array_equal(s[2], b[2]), (label, f, "losses")
        assert np.array_equal(s[3], b[3]), (label, f, "steps")
    assert s_clouds == b_clouds, (label, s_clouds, b_clouds)
    assert np.array_equal(s_map, b_map), (label, "map")
    assert np.array_equal(s_rel, b_rel), (label, "trajectory")


def test_published_loop_batched_equals_single(torch_cuda, loop_scans, other_sequences):
    """Four drives of the published configuration (live 1e-4 stop, window 30: evictions from frame 30 on) — the golden
    loop's frames and three others — batched: every frame of every member equal to the member's drive alone."""
    scans0, _ = loop_scans
    seqs = [scans0] + other_sequences
    cfg = published_config()
    batched = _run_batch(torch_cuda, seqs, cfg, [{}] * 4)
    for b, seq in enumerate(seqs):
        single = _run_single(torch_cuda, seq, cfg, {})
        _assert_same_run(single, batched[b], f"member {b}")
        assert single[2] == 30  # the window is full: clouds were evicted


def test_batched_forced_loop_matches_the_reference_run(torch_cuda, golden_loop, loop_scans, other_sequences):
    """Member 0 with the stop test off (threshold 0, the fixture's forced iteration count) within 1e-4 m / 1e-4 rad of the
    reference's run on every frame (the bound tests/test_gpu_loop.py applies to the single plugin)."""
    import icp_oracle as O
    g = golden_loop
    scans0, _ = loop_scans
    cfg = published_config(max_num_alignments=int(g["forced_iters_per_frame"]), threshold_delta_pose=0.0)
    batched = _run_batch(torch_cuda, [scans0, other_sequences[0]], cfg, [{}] * 2)
    frames, _, clouds, _ = batched[0]
    for f, (pose, iters, _, _) in enumerate(frames, start=1):
        dt, dr = O.pose_error(pose, g["forced_rel"][f])
        assert dt < 1e-4 and dr < 1e-4, (f, dt, dr)
        assert iters == int(g["forced_iters"][f])
    assert clouds == 30


@pytest.mark.parametrize("carry_normals", [1, 0])
def test_mixed_key_frame_decisions_in_one_update(torch_cuda, mixed_sequences, carry_normals):
    """A slow member (mostly pose-only updates) beside two fast ones (an insertion per frame): single map updates that
    mix inserting and pose-only members, bit-equal to the single plugins — with the normals carried through pose-only
    updates and with the reference's schedule (every rebuild clears them)."""
    cfg = published_config(local_map=dict(type="kdtree_local_map", local_map_size=8, num_neighbors_normals=10))
    opts = {"carry_normals": carry_normals}
    batched = _run_batch(torch_cuda, mixed_sequences, cfg, [opts] * 3)
    singles = [_run_single(torch_cuda, seq, cfg, opts) for seq in mixed_sequences]
    for b in range(3):
        _assert_same_run(singles[b], batched[b], f"member {b}")
    # the calls were mixed: the slow member inserted on few frames, the fast ones on every frame (window of 8 full)
    assert singles[0][2] < 8 and singles[1][2] == 8 and singles[2][2] == 8, [s[2] for s in singles]


def test_fallback_members_beside_batched_ones(torch_cuda, mixed_sequences):
    """Members whose eager normals another kernel computes — the straggler list (normals_list = 1), four lanes per point
    (knn_lanes = 2) — take their own launches inside the batched update, beside a member on the batched kernels, and
    stay bit-equal to their single plugins."""
    cfg = published_config(local_map=dict(type="kdtree_local_map", local_map_size=8, num_neighbors_normals=10))
    seqs = [mixed_sequences[1], mixed_sequences[2], mixed_sequences[1]]
    opts = [{}, {"normals_list": 1}, {"knn_lanes": 2}]
    batched = _run_batch(torch_cuda, seqs, cfg, opts)
    for b in range(3):
        _assert_same_run(_run_single(torch_cuda, seqs[b], cfg, opts[b]), batched[b], f"member {b} {opts[b]}")


# ---- the C entry point on its own -------------------------------------------------------------------------------------
def _grid_clouds(torch, scans):
    """Grid-sampled frames (0.4 m voxels, as the published configuration): [n, 3] float32 host arrays."""
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(height=H, width=W)
    out = [ctx.grid_sample(s, 0.4)[0] for s in scans]
    ctx.close()
    return [np.ascontiguousarray(c, np.float32) for c in out]


def _contexts(count, **kw):
    from pylidar_slam_amd.engine import IcpContext
    cfg = dict(height=H, width=W, max_num_alignments=20, threshold_delta_pose=1e-4, scheme="neighborhood", sigma=0.2,
               local_map_size=30, num_neighbors_normals=10)
    cfg.update(kw)
    return [IcpContext(**cfg) for _ in range(count)]


def test_refused_calls_leave_every_member_untouched(torch_cuda):
    """Every refusal of icp_batch_map_update_staged (a member on another stream, an inserting member without a staged
    cloud, rel_poses = NULL before an inserting member's registration was collected, rel_poses = NULL on a member that
    never registered) changes nothing: maps, windows and staged clouds stay, and the run goes on exactly like a twin run
    that never made the refused calls."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch
    drives = [_scans(9234 + 1000 * b, 0.3 + 0.05 * b, 4, with_motion=True) for b in range(3)]
    clouds = [_grid_clouds(torch, scans) for scans, _ in drives]
    motion = [rel for _, rel in drives]
    dev = [[torch.from_numpy(c).cuda() for c in cl] for cl in clouds]
    runs = []
    for refuse in (True, False):
        ctxs = _contexts(3)
        batch = IcpBatch(ctxs)
        batch.use_torch_stream()
        for c, cl, rel in zip(ctxs, clouds, motion):
            c.map_update(rel[0], cl[0])
            c.map_update(rel[1], cl[1])

        def snapshot():
            return [(c.map_points(), c.map_num_clouds()) for c in ctxs]

        def unchanged(before):
            for (m0, n0), c in zip(before, ctxs):
                assert c.map_num_clouds() == n0 and np.array_equal(c.map_points(), m0)

        if refuse:  # no member has registered yet
            before = snapshot()
            with pytest.raises(AssertionError, match="previous registration"):
                batch.map_update_staged([0, 0, 0], None)
            unchanged(before)
        for b in (0, 2):  # member 1 stages nothing
            ctxs[b].map_stage_cloud(dev[b][2])
        batch.register_launch([dev[b][2] for b in range(3)], [motion[b][2] for b in range(3)])
        if refuse:  # an inserting member's registration is still pending
            before = snapshot()
            with pytest.raises(AssertionError, match="collect the pending registration"):
                batch.map_update_staged([1, 0, 1], None)
            unchanged(before)
        results = batch.register_end()
        poses = [r.pose for r in results]
        if refuse:
            before = snapshot()
            with pytest.raises(AssertionError, match="no staged cloud"):
                batch.map_update_staged([1, 1, 1], poses)  # member 1 has nothing staged
            unchanged(before)
            other = torch.cuda.Stream()
            ctxs[2]._lib.icp_set_stream(ctxs[2]._h, C.c_void_p(other.cuda_stream))
            ctxs[2]._bound_stream = other.cuda_stream
            with pytest.raises(AssertionError, match="one stream"):
                batch.map_update_staged([1, 0, 1], poses)
            unchanged(before)
            batch.use_torch_stream()
        inserted = batch.map_update_staged([1, 0, 1], poses)  # the staged clouds of members 0 and 2 are still there
        queries = torch.from_numpy(np.ascontiguousarray(clouds[1][3][::3])).cuda()
        normals = [c.nearest_neighbor_search(queries, with_normals=True)[1].cpu().numpy() for c in ctxs]
        for b in range(3):
            ctxs[b].map_stage_cloud(dev[b][3])
        batch.register_launch([dev[b][3] for b in range(3)], poses)
        nxt = batch.register_end()
        runs.append((inserted, [_record(r) for r in results], snapshot(), normals, [_record(r) for r in nxt]))
        batch.close()
        for c in ctxs:
            c.close()
    (ins_a, res_a, maps_a, nrm_a, nxt_a), (ins_b, res_b, maps_b, nrm_b, nxt_b) = runs
    assert ins_a == ins_b and ins_a[0] > 0 and ins_a[1] == 0 and ins_a[2] > 0
    for x, y in zip(res_a + nxt_a, res_b + nxt_b):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])
    for (ma, na), (mb, nb) in zip(maps_a, maps_b):
        assert na == nb and np.array_equal(ma, mb)
    for a, b in zip(nrm_a, nrm_b):
        assert np.array_equal(a, b)


def test_full_windows_at_benchmark_size(torch_cuda):
    """Eight members with full 30-cloud windows (~180 000 map points each): one batched insertion (with eviction, by the
    device-resident poses) equals the insertion on each context alone — the map, the window, every normal (through
    nearest_neighbor_search on a fixed query set) and the next registration."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch
    scans, rel = _scans(8234, 0.3, 39, with_motion=True)  # member b: frames b .. b + 31 of one drive
    clouds = _grid_clouds(torch, scans)
    assert sum(c.shape[0] for c in clouds[:30]) > 150_000
    dev = [torch.from_numpy(c).cuda() for c in clouds]
    queries = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds[36:39])[::2])).cuda()
    runs = []
    for batched in (False, True):
        ctxs = _contexts(8)
        batch = IcpBatch(ctxs)
        batch.use_torch_stream()
        for b, c in enumerate(ctxs):  # member b's window: frames b .. b + 29, then frame b + 30 registered and staged
            for k in range(b, b + 30):
                c.map_update(rel[k] if k > b else np.eye(4, dtype=np.float32), dev[k])
            c.register(dev[b + 30], rel[b + 30])
            c.map_stage_cloud(dev[b + 30])
        if batched:
            inserted = batch.map_update_staged([1] * 8, None)
        else:
            inserted = [c.map_update_staged(None) for c in ctxs]
        state = [(c.map_points(), c.map_num_clouds(), c.nearest_neighbor_search(queries, with_normals=True)[1].cpu().numpy())
                 for c in ctxs]
        batch.register_launch([dev[b + 31] for b in range(8)], [rel[b + 31] for b in range(8)])
        nxt = [_record(r) for r in batch.register_end()]
        runs.append((inserted, state, nxt))
        batch.close()
        for c in ctxs:
            c.close()
    (ins_a, st_a, nxt_a), (ins_b, st_b, nxt_b) = runs
    assert ins_a == ins_b and min(ins_a) > 0
    for b, ((ma, na, nma), (mb, nb, nmb)) in enumerate(zip(st_a, st_b)):
        assert na == nb == 30 and ma.shape[0] > 150_000, (b, na, nb, ma.shape)
        assert np.array_equal(ma, mb), b
        assert np.array_equal(nma, nmb), b
    for b, (x, y) in enumerate(zip(nxt_a, nxt_b)):
        assert np.array_equal(x[0], y[0]) and x[1] == y[1] and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3]), b
