"""The frame boundary of one context — `register_launch / map_update(None) / register_end` — under the schedule switches
"clear_ahead" (the next hash table emptied beside the final solve) and "move_on_insert" (move, carried normals and seeds in
the insertion launch): each switch alone and both together give the bits of the run with both 0.  (A third part, the pose
delivered through a polled ticket, was measured and taken out — DESIGN.md §0.8 — and its cases with it.)

16 x 256 scans (4096 points), 12 forced iterations, geman_mcclure / 0.3; maps of 2999 points (more seeds than map points: the
insertion launch is sized by the seeds; no multiple of 256) and of 9001 points (more points than seeds)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, ITERS = 16, 256, 12
KW = dict(height=H, width=W, max_num_alignments=ITERS, threshold_delta_pose=0.0, scheme="geman_mcclure", sigma=0.3)
OFF = {"clear_ahead": 0, "move_on_insert": 0}
ALL = {"clear_ahead": 1, "move_on_insert": 1}
VARIANTS = {
    "clear_ahead": {**OFF, "clear_ahead": 1},        # the spare is used, the clearing launch keeps the per-point work
    "move_on_insert": {**OFF, "move_on_insert": 1},  # (alone it finds no clean table: the clearing path)
    "all": ALL,
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


@functools.lru_cache(maxsize=None)
def _scene():
    from pylidar_slam_amd.synthetic import SceneConfig, make_fixed_map, make_sequence
    cfg = SceneConfig(height=H, width=W)
    scans, poses = make_sequence(cfg, 12)
    maps = {m: make_fixed_map(cfg, scans[:4], poses[:4], ref_frame=3, num_points=m, voxel=0.1) for m in (2999, 9001)}
    return scans, maps


def _context(options, **kw):
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(**{**KW, **kw})
    for k, v in options.items():
        ctx.set_option(k, v)
    return ctx


def _record(r):
    return dict(pose=r.pose.copy(), params=r.params.copy(), losses=r.losses.copy(), dx=r.dx.copy(), iterations=r.iterations)


def _final(ctx, scan, neighbors=True):
    """What the grid holds at the end: the map, the neighbours and normals of a subsample of `scan` and — `icp_last_neighbors`
    reads the NN cache of a registration against the CURRENT grid — the neighbours one more registration of `scan`, with no
    update behind it, ends on (and its result)."""
    nb, nm, ix = ctx.nearest_neighbor_search(np.ascontiguousarray(scan[::7]), with_normals=True, with_index=True)
    out = dict(map=ctx.map_points().copy(), nb=nb, normals=nm, index=ix, last=np.zeros(0, np.int32))
    if neighbors:
        ctx.register_launch(scan, None)
        out.update({"extra_" + k: v for k, v in _record(ctx.register_end()).items()})
        out["last"] = ctx.last_neighbors(scan.shape[0])[0]
    out["fallbacks"] = ctx.handoff_fallbacks()
    return out


def _same(got, want, label):
    recs_a, fin_a = got
    recs_b, fin_b = want
    assert len(recs_a) == len(recs_b), label
    for f, (a, b) in enumerate(zip(recs_a, recs_b)):
        for k in ("pose", "params", "losses", "dx"):
            assert np.array_equal(a[k], b[k]), (label, f, k)
        assert a["iterations"] == b["iterations"], (label, f)
    assert sorted(fin_a) == sorted(fin_b), label
    for k in sorted(fin_a):
        assert np.array_equal(fin_a[k], fin_b[k]), (label, k)
    assert fin_a["fallbacks"] == 0 and fin_b["fallbacks"] == 0, label


def _chain(options, m, carry, frames=5):
    """`frames` chained frames of register_launch / map_update(None) / register_end on the m-point map."""
    scans, maps = _scene()
    ctx = _context({**options, "carry_normals": carry})
    ctx.map_set(maps[m])
    recs, last = [], None
    for f in range(4, 4 + frames):
        ctx.register_launch(scans[f], last)
        ctx.map_update(None, None)
        r = ctx.register_end()
        recs.append(_record(r))
        last = r.pose
    return recs, _final(ctx, scans[4 + frames - 1])


@functools.lru_cache(maxsize=None)
def _chain_reference(m, carry):
    return _chain(OFF, m, carry)


@pytest.mark.parametrize("carry", [1, 0])
@pytest.mark.parametrize("m", [2999, 9001])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_option_variants_equal_the_schedule_without_them(torch_cuda, variant, m, carry):
    """Five chained frames under each switch alone and both together, with and without carried normals: poses, parameters, losses, steps, iteration counts,
    the final map, the neighbours, normals and indices of a subsample and the NN cache equal the run with both switches 0."""
    _same(_chain(VARIANTS[variant], m, carry), _chain_reference(m, carry), (variant, m, carry))


def test_two_registrations_in_a_row_leave_the_current_grid_alone(torch_cuda):
    """Two launched registrations without an update between them: the first one's final solve empties the spare table, the
    second finds it clean — and searches a grid nobody touched: its result is the one a fresh context gives on the same map.
    Then an update and a third frame, against the reference schedule."""
    scans, maps = _scene()

    def run(options):
        ctx = _context(options)
        ctx.map_set(maps[2999])
        ctx.register_launch(scans[4], None)
        a = ctx.register_end()
        ctx.register_launch(scans[5], None)
        b = ctx.register_end()
        ctx.map_update(None, None)
        ctx.register_launch(scans[6], b.pose)
        ctx.map_update(None, None)
        c = ctx.register_end()
        return [_record(a), _record(b), _record(c)], _final(ctx, scans[6])

    got, want = run(ALL), run(OFF)
    _same(got, want, "two registrations")
    fresh = _context(ALL)
    fresh.map_set(maps[2999])
    fresh.register_launch(scans[5], None)
    alone = _record(fresh.register_end())
    for k in ("pose", "params", "losses", "dx"):
        assert np.array_equal(got[0][1][k], alone[k]), k


def test_host_pose_update_and_table_growth_take_the_clearing_path(torch_cuda):
    """An update by a host pose with no registration in front of it, and an insertion that takes the map across a table-size
    step (tsize = next_pow2(m + m / 4): 800 -> more than 819 points is 1024 -> 2048 slots), find no clean spare of their size
    and clear their own table; the frames behind them use the fast path again.  All against the reference schedule."""
    scans, maps = _scene()
    step = np.eye(4, dtype=np.float32)
    step[0, 3] = 0.05

    def run(options):
        ctx = _context(options, local_map_size=4)
        ctx.map_init()
        ctx.map_update(np.eye(4, dtype=np.float32), np.ascontiguousarray(maps[9001][::11][:800]))
        recs = []
        ctx.map_update(step, None)                       # a host pose, nothing registered yet
        ctx.register_launch(scans[4], None)
        ctx.map_update(None, None)                       # behind a registration: the spare
        recs.append(_record(ctx.register_end()))
        assert ctx.map_update(recs[-1]["pose"], np.ascontiguousarray(maps[9001][5::11][:200])) == 200
        assert ctx.map_size() == 1000                    # 800 -> 1000 points: the table grows
        ctx.register_launch(scans[5], recs[-1]["pose"])
        ctx.map_update(None, None)
        recs.append(_record(ctx.register_end()))
        ctx.map_update(step, None)                       # a host pose behind a collected registration
        ctx.register_launch(scans[6], recs[-1]["pose"])
        ctx.map_update(None, None)
        recs.append(_record(ctx.register_end()))
        return recs, _final(ctx, scans[6])

    _same(run(ALL), run(OFF), "host pose / growth")


def test_two_frames_in_flight(torch_cuda):
    """`register_launch(scan, "last")` twice, then `register_end` twice, over six frames."""
    scans, maps = _scene()

    def run(options):
        ctx = _context(options)
        ctx.map_set(maps[9001])
        recs = []
        ctx.register_launch(scans[4], None)
        ctx.map_update(None, None)
        recs.append(_record(ctx.register_end()))
        for f in (5, 7, 9):
            ctx.register_launch(scans[f], "last")
            ctx.map_update(None, None)
            ctx.register_launch(scans[f + 1], "last")
            ctx.map_update(None, None)
            recs.append(_record(ctx.register_end()))
            recs.append(_record(ctx.register_end()))
        return recs[:6], _final(ctx, scans[10])

    _same(run(ALL), run(OFF), "in flight")


def test_failed_registration_moves_nothing(torch_cuda):
    """A registration that ends with an Invalid Jacobian (two target rows) moves nothing, on either path: the map behind the
    pose-only update is the map in front of it, and the next frame runs as on the reference schedule."""
    from pylidar_slam_amd.engine import InvalidJacobianError
    scans, maps = _scene()

    def run(options):
        ctx = _context(options)
        ctx.map_set(maps[2999])
        ctx.register_launch(scans[4], None)
        ctx.map_update(None, None)
        first = _record(ctx.register_end())
        before = ctx.map_points().copy()
        ctx.register_launch(np.ascontiguousarray(scans[5][:2]), None)
        ctx.map_update(None, None)
        with pytest.raises(InvalidJacobianError):
            ctx.register_end()
        assert np.array_equal(ctx.map_points(), before)
        ctx.register_launch(scans[5], first["pose"])
        ctx.map_update(None, None)
        return [first, _record(ctx.register_end())], _final(ctx, scans[5])

    _same(run(ALL), run(OFF), "failed registration")


def test_frame_calls_with_a_sliding_window(torch_cuda):
    """Eight frames of frame_launch / frame_end with a grid sample and a window of three key frames: insertions and evictions
    (the clearing path, tables of changing size) between pose-only updates (the spare)."""
    scans, _ = _scene()

    def run(options):
        ctx = _context(options, local_map_size=3)
        ctx.odometry_init(voxel_size=0.4, threshold_trans=0.7, threshold_rot=10.0, constant_velocity=True, targets=0)
        recs, keys = [], []
        for f in range(8):
            ctx.frame_launch(scans[f])
            r = ctx.frame_end()
            recs.append(_record(r.register))
            keys.append((bool(r.key_frame), int(r.inserted), int(r.samples)))
        return (recs, _final(ctx, scans[7], neighbors=False)), keys

    got, keys_got = run(ALL)
    want, keys_want = run(OFF)
    assert keys_got == keys_want
    _same(got, want, "frame calls")
    later = [k for k, _, _ in keys_want[1:]]
    assert any(later) and not all(later), keys_want  # both kinds of update occurred
