"""`-m gpu`: the projective local map, B sequences per launch — `icp_batch_pmap_register_launch`, `icp_batch_pmap_update`
and `MI355XICPFrameToModelBatch` with `local_map.type = projective_local_map` (ProjectiveLocalMap, the reference's
slam/odometry/local_map.py:91-240).  Per member everything must be what the single plugin / the single context computes
on the same frames, bit for bit: poses, iteration counts, losses, steps, windows and models."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def golden():
    from conftest import GOLDEN
    return np.load(os.path.join(GOLDEN, "projective.npz")), np.load(os.path.join(GOLDEN, "projective_spread.npz"))


def _scans(h, w, seed, step, frames, yaw_rate=0.01):
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    scans, _ = make_sequence(SceneConfig(height=h, width=w, seed=seed, step=step, yaw_rate=yaw_rate), frames)
    return scans


def _vmaps(torch, h, w, scans):
    """[3,H,W] cuda vertex maps of the scans (the library's own projection)."""
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(height=h, width=w)
    out = [ctx.project(torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).cuda()).clone() for s in scans]
    torch.cuda.synchronize()
    ctx.close()
    return out


def _config(iters, threshold, lms, scheme="neighborhood", sigma=0.2):
    from pylidar_slam_amd.odometry import MI355XICPConfig
    return MI355XICPConfig(max_num_alignments=int(iters), threshold_delta_pose=float(threshold), data_key="vertex_map",
                           local_map=dict(type="projective_local_map", local_map_size=int(lms)),
                           alignment=dict(mode="point_to_plane_gauss_newton",
                                          gauss_newton_config=dict(max_iters=1, scheme=scheme, sigma=float(sigma))))


def _record(res):
    return (res.pose.copy(), int(res.iterations), res.losses.copy(), res.dx.copy())


def _same(a, b, what):
    assert np.array_equal(a[0], b[0]), f"{what}: pose"
    assert a[1] == b[1], f"{what}: iterations {a[1]} vs {b[1]}"
    assert np.array_equal(a[2], b[2]), f"{what}: losses"
    assert np.array_equal(a[3], b[3]), f"{what}: steps"


def _run_single(torch, frames, cfg, h, w):
    """One sequence through MI355XICPFrameToModel: per frame (pose, iterations, losses, steps), then the window size
    and the model.  Initial estimate of every frame: the previous relative pose."""
    from pylidar_slam_amd import odometry as our
    odo = our.MI355XICPFrameToModel(cfg, projector=our.SphericalProjector(h, w), device=torch.device("cuda:0"))
    odo.init()
    out, last = [], None
    for f, x in enumerate(frames):
        d = {"vertex_map": x, "init_rpose": last}
        odo.process_next_frame(d)
        if f > 0:
            last = d["odometry_pose"]
            out.append(_record(odo.last_result))
    result = (out, odo.ctx.pmap_num_maps(), odo.ctx.pmap_model())
    odo.ctx.close()
    return result


def _run_batch(torch, seqs, cfg, h, w):
    """The sequences through one MI355XICPFrameToModelBatch: the same records per member."""
    from pylidar_slam_amd import odometry as our
    odo = our.MI355XICPFrameToModelBatch(cfg, len(seqs), projector=our.SphericalProjector(h, w),
                                         device=torch.device("cuda:0"))
    odo.init()
    out = [[] for _ in seqs]
    last = [None] * len(seqs)
    for f in range(len(seqs[0])):
        ds = [{"vertex_map": s[f], "init_rpose": last[b]} for b, s in enumerate(seqs)]
        odo.process_next_frames(ds)
        if f > 0:
            for b, (m, d) in enumerate(zip(odo.members, ds)):
                assert np.array_equal(d["odometry_pose"], m.last_result.pose)
                last[b] = d["odometry_pose"]
                out[b].append(_record(m.last_result))
    result = [(out[b], m.ctx.pmap_num_maps(), m.ctx.pmap_model()) for b, m in enumerate(odo.members)]
    odo.batch.close()
    for m in odo.members:
        m.ctx.close()
    return result


def _compare(single, batched, label):
    (s_rec, s_k, (s_mv, s_mn)), (b_rec, b_k, (b_mv, b_mn)) = single, batched
    assert len(s_rec) == len(b_rec)
    for f, (a, b) in enumerate(zip(s_rec, b_rec)):
        _same(a, b, f"{label} frame {f + 1}")
    assert s_k == b_k, f"{label}: window {s_k} vs {b_k}"
    assert np.array_equal(s_mv, b_mv) and np.array_equal(s_mn, b_mn), f"{label}: model"


# ---- 1. batched == single, per member and frame ----------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [0.0, 1.0e-4])
@pytest.mark.parametrize("form", ["vertex_map", "cloud"])
def test_batched_equals_single(torch_cuda, threshold, form):
    torch = torch_cuda
    h, w, frames = 32, 256, 12
    drives = [_scans(h, w, 8101, 0.3, frames), _scans(h, w, 8202, 0.5, frames, yaw_rate=0.02),
              _scans(h, w, 8303, 0.15, frames, yaw_rate=0.005)]
    if form == "vertex_map":
        seqs = [_vmaps(torch, h, w, s) for s in drives]
    else:
        seqs = [[torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda() for x in s] for s in drives]
    cfg = _config(15, threshold, 4)
    singles = [_run_single(torch, s, cfg, h, w) for s in seqs]
    batched = _run_batch(torch, seqs, cfg, h, w)
    for b in range(len(seqs)):
        _compare(singles[b], batched[b], f"member {b}")
    assert all(k == 4 for _, k, _ in singles), "the windows are expected full (evictions happened)"
    if threshold > 0:  # the members stop at different iterations
        iters = {tuple(r[1] for r in rec) for rec, _, _ in singles}
        assert len(iters) > 1 and min(r[1] for rec, _, _ in singles for r in rec) < 15


# ---- 2. against the reference's own run --------------------------------------------------------------------------------
@pytest.mark.parametrize("run", ["ls", "nbh"])
def test_golden_member(torch_cuda, O, golden, run):
    torch = torch_cuda
    g, sp = golden
    h, w = (int(v) for v in g["hw"])
    scheme, sigma, iters, thr = (str(v) for v in g[f"{run}_cfg"])
    frames = len(g["vmaps"])
    cfg = _config(int(iters), float(thr), 4, scheme=scheme, sigma=float(sigma))
    gold = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in g["vmaps"]]
    seqs = [_vmaps(torch, h, w, _scans(h, w, 8404, 0.3, frames)), gold, _vmaps(torch, h, w, _scans(h, w, 8505, 0.4, frames))]
    batched = _run_batch(torch, seqs, cfg, h, w)
    _compare(_run_single(torch, gold, cfg, h, w), batched[1], f"golden member ({run})")
    for f, rec in enumerate(batched[1][0], start=1):
        assert rec[1] == int(g[f"{run}_iters"][f]), (run, f, rec[1])
        for name, ref in (("reference", g[f"{run}_rel"][f]), ("reference_f64conv", sp[f"{run}_float64_rel"][f])):
            dt, dr = O.pose_error(rec[0], ref)
            assert dt < 1e-4 and dr < 1e-4, (name, run, f, dt, dr)


# ---- 3. mixed updates in one call ----------------------------------------------------------------------------------------
def _contexts(h, w, count, **kw):
    from pylidar_slam_amd.engine import IcpContext
    base = dict(height=h, width=w, max_num_alignments=12, threshold_delta_pose=0.0, scheme="neighborhood", sigma=0.2,
                local_map_size=2)
    base.update(kw)
    return [IcpContext(**base) for _ in range(count)]


def _rel(k):
    from pylidar_slam_amd.odometry import build_pose_matrix
    return build_pose_matrix(np.array([0.3 + 0.05 * k, 0.02, -0.01, 0.002, -0.001, 0.01 * (k + 1)], np.float32))


def _model_state(ctx):
    mv, mn = ctx.pmap_model()
    return ctx.pmap_num_maps(), mv, mn


def test_mixed_updates(torch_cuda):
    from pylidar_slam_amd.engine import IcpBatch
    torch = torch_cuda
    h, w = 32, 256
    vm = _vmaps(torch, h, w, _scans(h, w, 8606, 0.3, 6))
    ours, refs = _contexts(h, w, 3), _contexts(h, w, 3)
    for c in ours + refs:
        c.pmap_init()
    # member 0: empty; member 1: a full window (the insertion evicts); member 2: one map (pose-only update)
    for group in (ours, refs):
        group[1].pmap_update(np.eye(4, dtype=np.float32), vm[0])
        group[1].pmap_update(_rel(0), vm[1])
        group[2].pmap_update(np.eye(4, dtype=np.float32), vm[2])
    batch = IcpBatch(ours)
    rels = [np.eye(4, dtype=np.float32), _rel(1), _rel(2)]
    maps = [vm[3], vm[4], None]
    batch.pmap_update(rels, maps)
    for c, r, m in zip(refs, rels, maps):
        c.pmap_update(r, m)
    for b in range(3):
        a, r = _model_state(ours[b]), _model_state(refs[b])
        assert a[0] == r[0] and np.array_equal(a[1], r[1]) and np.array_equal(a[2], r[2]), f"member {b}: window / model"
    assert [c.pmap_num_maps() for c in ours] == [1, 2, 1]
    # the next registration of every member, bit for bit
    scans = [vm[5].permute(1, 2, 0).reshape(-1, 3).contiguous()] * 3
    inits = [_rel(3), None, _rel(1)]
    batch.pmap_register_launch(scans, inits, skip_null=True)
    got = batch.register_end()
    for b, c in enumerate(refs):
        _same(_record(got[b]), _record(c.pmap_register(scans[b], inits[b], skip_null=True)), f"member {b}")
    batch.close()
    for c in ours + refs:
        c.close()


# ---- 4. refused calls change nothing -------------------------------------------------------------------------------------
def test_refusals_change_nothing(torch_cuda):
    from pylidar_slam_amd.engine import IcpBatch
    torch = torch_cuda
    h, w = 32, 256
    scans_np = _scans(h, w, 8707, 0.3, 3)
    vm = _vmaps(torch, h, w, scans_np)
    pts = vm[2].permute(1, 2, 0).reshape(-1, 3).contiguous()

    def fresh(count=2, **kw):
        ctxs = _contexts(h, w, count, **kw)
        for c in ctxs:
            c.pmap_init()
            c.pmap_update(np.eye(4, dtype=np.float32), vm[0])
            c.pmap_update(_rel(0), vm[1])
        return ctxs

    refs = fresh()
    expected = [_record(c.pmap_register(pts, _rel(1), skip_null=True)) for c in refs]

    def check_unchanged(ctxs, batch):
        assert [c.pmap_num_maps() for c in ctxs] == [2, 2]
        batch.pmap_register_launch([pts, pts], [_rel(1), _rel(1)], skip_null=True)
        for b, res in enumerate(batch.register_end()):
            _same(_record(res), expected[b], f"member {b} after a refused call")

    def refused(fn, exc=AssertionError):
        with pytest.raises(exc):
            fn()

    ctxs = fresh()
    batch = IcpBatch(ctxs)
    eye = np.eye(4, dtype=np.float32)
    # another scheme; another image size
    odd = _contexts(h, w, 1, scheme="huber")[0]
    odd.pmap_init()
    odd.pmap_update(eye, vm[0])
    small = _contexts(16, 256, 1)[0]
    small.pmap_init()
    small.pmap_update(eye, torch.ones((3, 16, 256), device="cuda"))
    for other in (odd, small):
        mixed = IcpBatch([ctxs[0], other])
        refused(lambda: mixed.pmap_register_launch([pts, pts], [_rel(1), _rel(1)], skip_null=True))
        if other is small:
            refused(lambda: mixed.pmap_update([_rel(2), _rel(2)], [vm[2], None]))
        mixed.close()
    check_unchanged(ctxs, batch)
    # another stream
    batch.use_torch_stream()
    side = torch.cuda.Stream()
    assert ctxs[1]._lib.icp_set_stream(ctxs[1]._h, C.c_void_p(side.cuda_stream)) == 0
    refused(lambda: batch.pmap_register_launch([pts, pts], [_rel(1), _rel(1)], skip_null=True))
    refused(lambda: batch.pmap_update([_rel(2), _rel(2)], [vm[2], None]))
    assert ctxs[1]._lib.icp_set_stream(ctxs[1]._h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    check_unchanged(ctxs, batch)
    # a member without a projective map
    empty = _contexts(h, w, 1)[0]
    empty.pmap_init()
    with_empty = IcpBatch([ctxs[0], empty])
    with pytest.raises(RuntimeError, match="empty"):
        with_empty.pmap_register_launch([pts, pts], None, skip_null=True)
    refused(lambda: with_empty.pmap_update([_rel(2), _rel(2)], [vm[2], None]))  # (an empty map needs a vertex map)
    with_empty.close()
    check_unchanged(ctxs, batch)
    # a pending result
    batch.pmap_register_launch([pts, pts], [_rel(1), _rel(1)], skip_null=True)
    refused(lambda: batch.pmap_register_launch([pts, pts], [_rel(1), _rel(1)], skip_null=True))
    refused(lambda: batch.pmap_update([_rel(2), _rel(2)], [vm[2], None]))
    for b, res in enumerate(batch.register_end()):
        _same(_record(res), expected[b], f"member {b}: the pending registration")
    check_unchanged(ctxs, batch)
    batch.close()
    # kd-tree iterations held back by a batched kd-tree registration in chunks (live threshold)
    ctxs = fresh(threshold_delta_pose=1.0e-4, max_num_alignments=12)
    kd_refs = fresh(threshold_delta_pose=1.0e-4, max_num_alignments=12)
    expected = [_record(c.pmap_register(pts, _rel(1), skip_null=True)) for c in kd_refs]
    cloud = torch.from_numpy(np.ascontiguousarray(scans_np[0], dtype=np.float32)).cuda()
    for c in ctxs:
        c.map_update(np.eye(4, dtype=np.float32), cloud)
    batch = IcpBatch(ctxs)
    batch.register_launch([cloud, cloud], None)
    refused(lambda: batch.pmap_register_launch([pts, pts], [_rel(1), _rel(1)], skip_null=True))
    refused(lambda: batch.pmap_update([_rel(2), _rel(2)], [None, None]))
    batch.register_end()
    check_unchanged(ctxs, batch)
    batch.close()
    for c in refs + ctxs + kd_refs + [empty, odd, small]:
        c.close()


# ---- 5. benchmark size ---------------------------------------------------------------------------------------------------
def test_benchmark_size(torch_cuda):
    """B = 8 drives of the PF2M configuration at 64 x 1024 (local_map_size 20, 15 alignments, neighborhood / 0.2, stop
    at 1e-4), 24 frames: full windows; batched == single per member."""
    torch = torch_cuda
    h, w, frames = 64, 1024, 24
    seqs = [_vmaps(torch, h, w, _scans(h, w, 9000 + 101 * b, 0.2 + 0.05 * b, frames, yaw_rate=0.004 * (b + 1)))
            for b in range(8)]
    cfg = _config(15, 1.0e-4, 20)
    batched = _run_batch(torch, seqs, cfg, h, w)
    for b in range(8):
        _compare(_run_single(torch, seqs[b], cfg, h, w), batched[b], f"member {b}")
