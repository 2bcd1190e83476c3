"""`-m gpu`: what the begins of a registration refuse, and what a refused begin leaves behind — `pmap_register`,
`pmap_register_launch` and `IcpBatch.pmap_register_launch` against an empty projective map or (batched) without a pose to
start from, `register_launch` and `IcpBatch.register_launch` with two results pending.  Every refusal is an argument check:
the text is today's, nothing reaches the device, and the calls that follow give the poses of a run that never made the
refused call, bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W = 16, 64
KW = dict(height=H, width=W, max_num_alignments=2, threshold_delta_pose=0.0, scheme="neighborhood", sigma=0.2, local_map_size=2)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


@pytest.fixture(scope="module")
def frames(torch_cuda):
    """Four scans of a 16 x 64 sensor (cuda, every other return: a few hundred points), the vertex maps of the full scans, and
    an initial guess near the truth.  Computed once, shared and left unchanged."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpContext
    from pylidar_slam_amd.odometry import build_pose_matrix
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    full, _ = make_sequence(SceneConfig(height=H, width=W, seed=4117, step=0.2, yaw_rate=0.01), 4)
    full = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).cuda() for s in full]
    ctx = IcpContext(height=H, width=W)
    vmaps = [ctx.project(s).clone() for s in full]
    torch.cuda.synchronize()
    ctx.close()
    scans = [s[::2].contiguous() for s in full]
    assert all(200 <= int(s.shape[0]) <= 600 for s in scans), [int(s.shape[0]) for s in scans]
    init = build_pose_matrix(np.array([0.2, 0.0, 0.0, 0.0, 0.0, 0.01], np.float32))
    return scans, vmaps, init


def _contexts(count):
    from pylidar_slam_amd.engine import IcpContext
    return [IcpContext(**KW) for _ in range(count)]


def _close(*things):
    for t in things:
        t.close()


def _same(a, b, what):
    assert np.array_equal(a.pose, b.pose), f"{what}: pose"
    assert a.iterations == b.iterations == 2, f"{what}: iterations {a.iterations} vs {b.iterations}"
    assert np.array_equal(a.losses, b.losses) and np.array_equal(a.dx, b.dx), f"{what}: losses / steps"


def _launched(ctx, scan, init):
    ctx.pmap_register_launch(scan, init, skip_null=True)
    return ctx.register_end()


SINGLE = {"pmap_register": lambda ctx, scan, init: ctx.pmap_register(scan, init, skip_null=True),
          "pmap_register_launch": _launched}


# ---- an empty projective map -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", sorted(SINGLE))
def test_empty_projective_map_is_refused_and_the_next_call_is_a_fresh_one(torch_cuda, frames, call):
    scans, vmaps, init = frames
    eye = np.eye(4, dtype=np.float32)
    fresh, ctx = _contexts(2)
    fresh.pmap_init()
    fresh.pmap_update(eye, vmaps[0])
    want = SINGLE[call](fresh, scans[1], init)
    ctx.pmap_init()
    with pytest.raises(RuntimeError, match=r"libicp_mi355x: the local map is empty \(") as refused:
        SINGLE[call](ctx, scans[1], init)
    assert not isinstance(refused.value, AssertionError)
    ctx.pmap_update(eye, vmaps[0])
    _same(SINGLE[call](ctx, scans[1], init), want, call)
    _close(fresh, ctx)


def test_batched_empty_projective_map_is_refused_and_the_next_call_is_a_fresh_one(torch_cuda, frames):
    from pylidar_slam_amd.engine import IcpBatch
    scans, vmaps, init = frames
    eye = np.eye(4, dtype=np.float32)
    fresh = _contexts(2)
    for b, c in enumerate(fresh):
        c.pmap_init()
        c.pmap_update(eye, vmaps[b])
    want = [c.pmap_register(scans[b + 1], init, skip_null=True) for b, c in enumerate(fresh)]
    ctxs = _contexts(2)
    for c in ctxs:
        c.pmap_init()
    ctxs[0].pmap_update(eye, vmaps[0])  # (member 0 has a map: the refusal names member 1)
    batch = IcpBatch(ctxs)
    with pytest.raises(RuntimeError) as refused:
        batch.pmap_register_launch([scans[1], scans[2]], [init, init], skip_null=True)
    assert "batched projective registration, member 1: the projective local map is empty" in str(refused.value)
    assert [c.pmap_num_maps() for c in ctxs] == [1, 0]
    ctxs[1].pmap_update(eye, vmaps[1])
    batch.pmap_register_launch([scans[1], scans[2]], [init, init], skip_null=True)
    for b, res in enumerate(batch.register_end()):
        _same(res, want[b], f"member {b}")
    _close(batch, *fresh, *ctxs)


# ---- from_last without a previous registration, batched projective path --------------------------------------------------
def test_batched_projective_from_last_without_a_pose_is_refused_and_the_members_stay_usable(torch_cuda, frames):
    from pylidar_slam_amd.engine import IcpBatch
    scans, vmaps, init = frames
    eye = np.eye(4, dtype=np.float32)
    fresh, ctxs = _contexts(2), _contexts(2)
    for b in range(2):
        for c in (fresh[b], ctxs[b]):
            c.pmap_init()
            c.pmap_update(eye, vmaps[b])
    want = [c.pmap_register(scans[b + 1], init, skip_null=True) for b, c in enumerate(fresh)]
    batch = IcpBatch(ctxs)
    with pytest.raises(AssertionError) as refused:
        batch.pmap_register_launch([scans[1], scans[2]], "last", skip_null=True)
    assert str(refused.value) == "batched projective registration, member 0: no previous registration to start from"
    assert [c.pmap_num_maps() for c in ctxs] == [1, 1]
    batch.pmap_register_launch([scans[1], scans[2]], [init, init], skip_null=True)
    first = batch.register_end()
    for b, res in enumerate(first):
        _same(res, want[b], f"member {b}")
    # ... and now there is a pose to start from: the same call goes through, and is the single registration from that pose
    batch.pmap_register_launch([scans[2], scans[3]], "last", skip_null=True)
    for b, res in enumerate(batch.register_end()):
        _same(res, fresh[b].pmap_register(scans[b + 2], want[b].pose, skip_null=True), f"member {b} from its last pose")
    _close(batch, *fresh, *ctxs)


# ---- two results pending ----------------------------------------------------------------------------------------------------
def test_third_launch_with_two_results_pending_is_refused_and_both_are_collected(torch_cuda, frames):
    scans, _, init = frames
    eye = np.eye(4, dtype=np.float32)
    fresh, ctx = _contexts(2)
    for c in (fresh, ctx):
        c.map_update(eye, scans[0])
        c.register_launch(scans[1], init)
        c.register_launch(scans[2], "last")
    with pytest.raises(AssertionError) as refused:
        ctx.register_launch(scans[3], "last")
    assert str(refused.value) == "two results are already pending"
    for k in range(2):
        _same(ctx.register_end(), fresh.register_end(), f"pending result {k}")
    _close(fresh, ctx)


def test_batched_third_launch_with_two_results_pending_is_refused_and_both_are_collected(torch_cuda, frames):
    from pylidar_slam_amd.engine import IcpBatch
    scans, _, init = frames
    eye = np.eye(4, dtype=np.float32)
    fresh, ctxs = _contexts(2), _contexts(2)
    for b in range(2):
        fresh[b].map_update(eye, scans[b])
        fresh[b].register_launch(scans[b + 1], init)
        fresh[b].register_launch(scans[b + 2], "last")
        ctxs[b].map_update(eye, scans[b])
    batch = IcpBatch(ctxs)
    batch.register_launch([scans[1], scans[2]], [init, init])
    batch.register_launch([scans[2], scans[3]], "last")
    with pytest.raises(AssertionError) as refused:
        batch.register_launch([scans[3], scans[0]], "last")
    assert str(refused.value) == "two results are already pending"
    for k in range(2):
        got = batch.register_end()
        for b in range(2):
            _same(got[b], fresh[b].register_end(), f"member {b}, pending result {k}")
    _close(batch, *fresh, *ctxs)
