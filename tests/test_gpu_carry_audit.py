"""The CARRIED map normals of the library against the bit model of tests/carry_audit.py, read back with
`IcpContext.map_normals_peek()` (the normal cache as it stands: nothing is estimated by looking).

With "carry_normals" (the default) a pose-only map update rotates the normals of the old grid into the new frame; every
point-to-plane row of the next registration on a non-key frame is built from them.  Here every path that carries — the clearing
launch behind a host pose, the insertion launch behind an enqueued registration ("move_on_insert" on a table "clear_ahead"
emptied), their batch forms, the frame calls — is held, row by row, to the model applied to the device's OWN previous read-back:
(A) the flags, (B) the bits of every flagged row (the only latitude: which of the five admissible rsqrtf values scaled a
renormalised row), (C) the length, and over chains (D) the direction against the float64 rotation.  tests/test_carry_audit.py
shows on the CPU that each check reports the wrong copy meant for it.

What the model had to learn from the source, and what was changed:
  * an update behind which `map_update_finish` estimates the whole map eagerly (a registered context, "eager_normals_limit",
    normals missing) OVERWRITES the carried rows as well: the cache is then the estimator's model on the moved map, every row.
  * a cache filled by searches (not by the eager estimation of a registration) is estimated AGAIN by the next registration,
    carried or not: the consumer test fills it by a registration, as the product does.
  * a carried normal whose squared length overflows (2e19 u) came out as a FLAGGED ZERO normal; carry_normal now tests its
    result.  Against the library built from the grid unit as it was before (plus the read-back) the three planted-rows cases
    fail at that row ("[flag census] ... 1 rows are flagged that the model leaves unestimated") and the other 55 tests pass: writing
    the arithmetic out with __fmul_rn / __fadd_rn moved no bit.

Measured on an MI355X (58 tests, 7 s together, the slowest — the chain — 1.2 s): 1.29 million flagged rows held to the bit over
1 560 carries, none differing.  rsqrtf census over the 67 600 renormalised rows: the correctly rounded value 91 %, one step low
9 %, never high, never two steps off.  Worst | |n|^2 - 1 | 0.82 of the bound of its branch (the chain).  The chain: renormalised
share 0 at the first step, 1.0 % at the second, 2.3 - 19.5 % (mean 10.8 %) from the third on; the worst angle to the float64
rotation 5.2e-7 / 2.1e-6 / 1.0e-5 / 3.9e-5 rad after 10 / 40 / 200 / 1 000 steps = 0.121 / 0.121 / 0.116 / 0.090 of the derived
bound.  Behind a timed-out hand-off the repeated update applies the carry ONCE.  The consumer: |ddx| 0, dloss 5.3e-16, no
neighbour mismatch, min |dot| 0.9999998 — what the audit gives for estimated normals.  A kernel trace of this file
(profiles/carry_audit_kernel_trace.txt) names k_grid_clear, k_grid_insert2_ride, k_grid_clear_batch, k_grid_insert2_batch and
both rows-scatter kernels.  Every test prints its figures."""
import numpy as np
import pytest

import carry_audit as C
import iteration_audit as A
import map_lifecycle as L

pytestmark = pytest.mark.gpu
F32 = np.float32
KW = dict(height=16, width=512, max_num_alignments=L.K_REG, threshold_delta_pose=0.0, scheme=L.SCHEME, sigma=L.SIGMA,
          local_map_size=3)
OPTIONS = ((), (("cell_lists", 1),), (("insert_by_cell", 0),), (("overlap_map_update", 1),), (("hoods", 0),), (("frame_seed", 0),))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _ctx(options=(), **kw):
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(**{**KW, **kw})
    for name, value in options:
        ctx.set_option(name, value)
    return ctx


class Figures:
    """what a test saw: the rsqrtf census, the renormalised and flagged rows, the worst ratio to the length bound"""

    def __init__(self):
        self.census = {s: 0 for s in C.RSQ_STEPS}
        self.renormalised = self.flagged = self.steps = 0
        self.length = 0.0

    def add(self, fig):
        for s, n in fig["census"].items():
            self.census[s] += n
        self.renormalised += fig["renormalised"]
        self.flagged += fig["flagged"]
        self.length = max(self.length, fig["length_ratio"])
        self.steps += 1

    def __str__(self):
        return (f"{self.steps} carries, {self.flagged} flagged rows held to the bit, {self.renormalised} of them renormalised "
                f"(rsqrtf census by steps off the correctly rounded value: {self.census}); worst | |n|^2 - 1 | "
                f"{self.length:.3f} of its bound")


def _searched(ctx, pts):
    """the map set and every map point searched: the cache holds the normal of every point that is its own neighbour"""
    ctx.map_set(pts)
    ctx.nearest_neighbor_search(pts)
    return ctx.map_normals_peek()


def _host_step(ctx, rel, before, tag, figs):
    assert ctx.map_update(rel, None) == 0
    after = ctx.map_normals_peek()
    figs.add(C.check_step(tag, before, after, C.transform_of(rel)))
    return after


def _device_step(ctx, scan, init, before, tag, figs):
    """register_launch / map_update(None, None) / register_end: the update reads the pose on the device (on a table the solving
    launch emptied: the insertion launch carries); the model takes the returned pose"""
    ctx.register_launch(scan, init, skip_null=True)
    with pytest.raises(AssertionError, match="registration in progress"):
        ctx.map_normals_peek()
    assert ctx.map_update(None, None) == 0
    rc, res = A.raw_register_end(ctx)
    after = ctx.map_normals_peek()
    figs.add(C.check_step(tag, before, after, C.transform_of(res.pose, ok=rc == A.ICP_OK)))
    return after, rc, res


def _registered(ctx, pts, scan):
    """the map set and one collected registration against it: every normal estimated (map <= 2 x scan), none missing"""
    ctx.map_set(pts)
    rc, res = A.raw_register(ctx, scan, None, True)
    assert rc == A.ICP_OK
    before = ctx.map_normals_peek()
    assert (before[:, 3] == 1).all(), f"{(before[:, 3] != 1).sum()} normals missing behind an eager estimation"
    return before, res


# ---- the read-back itself --------------------------------------------------------------------------------------------------
def test_peek_estimates_nothing_and_refuses(torch_cuda):
    ctx = _ctx()
    with pytest.raises(RuntimeError, match="empty"):
        ctx.map_normals_peek()
    pts = C.cloud("lidar", 1025)
    ctx.map_set(pts)
    assert not ctx.map_normals_peek().any()                     # nothing searched yet: looking estimated nothing
    rows = np.arange(0, 1025, 3)
    _, nm, ix = ctx.nearest_neighbor_search(np.ascontiguousarray(pts[rows]), with_index=True)
    assert np.array_equal(ix, rows)
    a, b = ctx.map_normals_peek(), ctx.map_normals_peek()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(np.flatnonzero(a[:, 3] == 1), rows)   # by ORIGINAL index, exactly the searched points
    assert np.array_equal(a[rows, :3].view(np.uint32), nm.view(np.uint32))
    assert not a[a[:, 3] != 1].any()
    C.check_estimated("peek", a, pts, rows=rows)                # ... with the estimator's bits
    ctx.close()


# ---- sizes x poses through the clearing launch -----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,m", [("lidar", m) for m in C.SIZES] + [("lattice", m) for m in C.SIZES if m <= 4097])
def test_sizes_and_poses(torch_cuda, kind, m):
    """Every workgroup edge of the clear and scatter launches x every pose, two carries each (the second one meets rows the
    first moved off unit length).  Measured: 25 maps x 18 carries, 0.55 million flagged rows, none differing; the identity
    (with and without the translation) moves no bit; up to 72 rows per map renormalise, all on the correctly rounded rsqrtf;
    worst | |n|^2 - 1 | 0.755 of its bound."""
    pts, figs, ctx = C.cloud(kind, m), Figures(), _ctx()
    for name, rel in C.poses().items():
        before = _searched(ctx, pts)
        assert (before[:, 3] == 1).all()
        if name.startswith("identity"):
            same = _host_step(ctx, rel, before, f"{kind} {m} {name}", figs)
            assert np.array_equal(same.view(np.uint32), before.view(np.uint32)), f"{kind} {m} {name}: the identity moved a bit"
            continue
        mid = _host_step(ctx, rel, before, f"{kind} {m} {name}", figs)
        _host_step(ctx, rel, mid, f"{kind} {m} {name}, second carry", figs)
    ctx.close()
    print(f"{kind} {m}: {figs}")
    assert figs.flagged > 0


# ---- the options, on both carrying launches --------------------------------------------------------------------------------
@pytest.mark.parametrize("options", OPTIONS, ids=lambda o: "default" if not o else f"{o[0][0]}={o[0][1]}")
@pytest.mark.parametrize("m", C.OPTION_SIZES)
def test_options_give_the_models_bits(torch_cuda, m, options):
    """Each option alone: a host-pose update (the clearing launch) and two enqueued frames register_launch / map_update(None,
    None) / register_end ("clear_ahead" and "move_on_insert" are on by default: the second frame finds the spare table the
    first one's solving launch emptied, and its insertion launch carries).  Every one gives the model's bits, hence each
    other's."""
    pts, scan, figs = C.cloud("lidar", m), C.scans()[3], Figures()
    ctx = _ctx(options)
    before, res = _registered(ctx, pts, scan)
    after = _host_step(ctx, C.poses()["small"], before, f"{m} {options} host pose", figs)
    for f in range(3):
        after, rc, res = _device_step(ctx, scan, res.pose, after, f"{m} {options} enqueued frame {f}", figs)
        assert rc == A.ICP_OK and (after[:, 3] == 1).all()
    assert ctx.handoff_fallbacks() == 0
    ctx.close()
    print(f"{m} {options}: {figs}")


@pytest.mark.parametrize("m", C.OPTION_SIZES)
def test_the_schedule_switches_off_give_the_same_bits(torch_cuda, m):
    """"clear_ahead" 0 and "move_on_insert" 0 (every build clears its own table: the clearing launch carries behind a device pose
    too) against the default schedule: the same read-back after every frame."""
    pts, scan = C.cloud("lidar", m), C.scans()[3]
    seen = {}
    for name, options in (("off", (("clear_ahead", 0), ("move_on_insert", 0))), ("default", ())):
        ctx, figs = _ctx(options), Figures()
        after, res = _registered(ctx, pts, scan)
        seen[name] = []
        for f in range(3):
            after, rc, res = _device_step(ctx, scan, res.pose, after, f"{m} {name} frame {f}", figs)
            seen[name].append(after)
        ctx.close()
    for a, b in zip(seen["off"], seen["default"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- the other entry points ------------------------------------------------------------------------------------------------
def test_entry_points_behind_a_registration(torch_cuda):
    """`map_update(None, None)` behind a collected `register`, `map_update_staged` with nothing staged (refused: nothing moves)
    and with an empty staged cloud (a cloud: the cache is cleared, not carried)."""
    pts, scan, figs = C.cloud("lidar", 4097), C.scans()[3], Figures()
    ctx = _ctx()
    before, res = _registered(ctx, pts, scan)
    assert ctx.map_update(None, None) == 0
    after = ctx.map_normals_peek()
    figs.add(C.check_step("behind register", before, after, C.transform_of(res.pose)))
    with pytest.raises(AssertionError, match="no staged cloud"):
        ctx.map_update_staged(C.poses()["small"])
    again = ctx.map_normals_peek()
    assert np.array_equal(again.view(np.uint32), after.view(np.uint32))
    ctx.set_option("eager_normals_limit", 0)  # (4 097 <= 2 x 8 192 all the same: the eager rule runs behind the insertion)
    ctx.map_stage_cloud(np.zeros((0, 3), F32))
    assert ctx.map_update_staged(C.poses()["small"]) == 0
    cleared = ctx.map_normals_peek()
    n = C.check_never_carried("an empty staged cloud", after, cleared, C.transform_of(C.poses()["small"]),
                              map_points=ctx.map_points())
    ctx.close()
    print(f"entry points: {figs}; behind the empty staged cloud {n} rows re-estimated, none carried")


def test_batch_updates(torch_cuda):
    """`IcpBatch.map_update()` and `map_update_staged(insert = 0)` with three members of 1 025, 1 and 257 points, the last one
    behind a registration that fails (two target rows: Invalid Jacobian — it is carried by the identity)."""
    from pylidar_slam_amd.engine import IcpBatch, InvalidJacobianError
    scan, figs = C.scans()[3], Figures()
    sizes = (1025, 1, 257)
    scans = [scan, scan, np.ascontiguousarray(scan[A.valid_rows(scan, True)][:2])]
    ctxs = [_ctx() for _ in sizes]
    for ctx, m in zip(ctxs, sizes):
        _searched(ctx, C.cloud("lidar", m))
    batch = IcpBatch(ctxs)

    def end():
        try:
            return batch.register_end()
        except InvalidJacobianError as e:
            return e.results

    batch.register_launch(scans, None, skip_null=True)
    first = end()
    assert first[0] is not None and first[2] is None, "the two-row member was to fail"
    before = [c.map_normals_peek() for c in ctxs]
    batch.register_launch(scans, [r.pose if r is not None else None for r in first], skip_null=True)
    batch.map_update()
    res = end()
    T = [C.transform_of(r.pose if r is not None else np.eye(4), ok=r is not None) for r in res]
    after = [c.map_normals_peek() for c in ctxs]
    for i, m in enumerate(sizes):
        figs.add(C.check_step(f"batch map_update, member {i} ({m} points)", before[i], after[i], T[i]))
    assert np.array_equal(after[2].view(np.uint32), before[2].view(np.uint32))  # the failed member: every bit where it was
    assert batch.map_update_staged([0, 0, 0]) == [0, 0, 0]
    again = [c.map_normals_peek() for c in ctxs]
    for i, m in enumerate(sizes):
        figs.add(C.check_step(f"batch map_update_staged, member {i} ({m} points)", after[i], again[i], T[i]))
    batch.close()
    for c in ctxs:
        c.close()
    print(f"batch: {figs}; failed members {[i for i, r in enumerate(res) if r is None]}")


def _frames(torch, batched):
    """six frames of frame_launch / frame_end (a grid sample, a window of three key frames); the non-key frames from the second
    on are carried from the read-back behind the frame before (every normal is there: the eager rule ran behind each update)"""
    from pylidar_slam_amd.engine import IcpBatch
    kw = dict(voxel_size=0.4, threshold_trans=0.7, threshold_rot=10.0, constant_velocity=True, targets=0)
    seq = L._sequence()[0]
    members = 2 if batched else 1
    ctxs = [_ctx(height=L.H, width=L.W) for _ in range(members)]
    drives = [seq[:6], seq[3:9]][:members]
    batch = IcpBatch(ctxs) if batched else None
    (batch or ctxs[0]).odometry_init(**kw)
    figs, audited, keys = Figures(), 0, []
    prev = [None] * members
    for f in range(6):
        if batched:
            batch.frame_launch([d[f] for d in drives])
            results = batch.frame_end()
        else:
            ctxs[0].frame_launch(drives[0][f])
            results = [ctxs[0].frame_end()]
        for i, (ctx, r) in enumerate(zip(ctxs, results)):
            now = ctx.map_normals_peek()
            keys.append(bool(r.key_frame))
            if f >= 2 and not r.key_frame:
                assert (prev[i][:, 3] == 1).all(), f"frame {f}: normals were missing in front of a carried frame"
                figs.add(C.check_step(f"frame {f}, member {i}", prev[i], now, C.transform_of(r.pose)))
                audited += 1
            prev[i] = now
    if batch:
        batch.close()
    for c in ctxs:
        c.close()
    print(f"frames ({'batched' if batched else 'single'}): key frames {keys}; {audited} carried frames audited: {figs}")
    assert audited >= 2 * members


def test_frame_calls(torch_cuda):
    _frames(torch_cuda, False)


def test_batched_frame_calls(torch_cuda):
    _frames(torch_cuda, True)


# ---- partial caches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eager_behind", [0, 1])
def test_partial_flags(torch_cuda, eager_behind):
    """A registration of 2 048 rows against the 8 192-point map with "eager_normals_limit" 0 estimates the normals it touches
    only.  The update behind it carries exactly those (the rest stay zeros) — unless the limit is back above the map by then:
    the eager estimation behind the update then rewrites EVERY row with the estimator's bits on the moved map."""
    pts, scan, figs = C.cloud("lidar", 8192), C.scans()[3], Figures()
    ctx = _ctx((("eager_normals_limit", 0),))
    ctx.map_set(pts)
    rc, res = A.raw_register(ctx, np.ascontiguousarray(scan[:2048]), None, True)
    assert rc == A.ICP_OK
    before = ctx.map_normals_peek()
    have = int((before[:, 3] == 1).sum())
    assert 0 < have < len(pts), have
    if eager_behind:
        ctx.set_option("eager_normals_limit", 1 << 20)
    assert ctx.map_update(None, None) == 0
    after = ctx.map_normals_peek()
    T = C.transform_of(res.pose)
    if eager_behind:
        rows = np.sort(np.random.default_rng(5).choice(len(pts), 512, replace=False))
        assert (after[:, 3] == 1).all()
        n = C.check_estimated("eager behind a partial carry", after, L.move(T, pts), rows=rows)
        print(f"partial flags, eager behind: {have} of {len(pts)} flagged before, all behind; {n} sampled rows with the estimator's bits")
    else:
        fig = C.check_step("partial carry", before, after, T)
        assert fig["after"] == fig["before"] == have
        figs.add(fig)
        print(f"partial flags: {have} of {len(pts)} flagged before and behind: {figs}")
    ctx.close()


# ---- planted normals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose_name", ["identity", "small", "pitch_half_pi+far"])
def test_planted_normals(torch_cuda, pose_name):
    """Rows installed with `map_normals_install`: lengths 1 +- j 2^-24 on both sides of the threshold, exact axes, a zero row,
    an n2 that underflows, a subnormal n2, 1e19 u, 2e19 u (n2 = +inf), a NaN and an infinite component.  Two carries."""
    names, rows = C.planted_rows()
    ctx, figs = _ctx(), Figures()
    ctx.map_set(C.cloud("lidar", len(rows)))
    ctx.map_normals_install(torch_cuda.from_numpy(rows))
    before = ctx.map_normals_peek()
    assert np.array_equal(before[:, :3].view(np.uint32), rows[:, :3].view(np.uint32)) and (before[:, 3] == 1).all()
    rel = C.poses()[pose_name]
    mid = _host_step(ctx, rel, before, f"planted rows at {pose_name}", figs)
    flagged = mid[:, 3] == 1
    assert np.isfinite(mid).all() and mid[flagged, :3].any(axis=1).all(), \
        [n for n, r in zip(names, mid) if r[3] == 1 and not (np.isfinite(r).all() and r[:3].any())]
    _host_step(ctx, rel, mid, f"planted rows at {pose_name}, second carry", figs)
    ctx.close()
    print(f"planted rows at {pose_name}: kept {[n for n, k in zip(names, flagged) if k and not n.startswith(('length', 'axis'))]}, "
          f"dropped {[n for n, k in zip(names, flagged) if not k]}; {figs}")


# ---- failures --------------------------------------------------------------------------------------------------------------
def test_identity_behind_a_failed_registration(torch_cuda):
    """An Invalid Jacobian (two target rows), then `map_update(None, None)` — collected first, and enqueued between launch and
    end: every bit and every flag of the 8 192-point map's cache is as before."""
    from pylidar_slam_amd.engine import InvalidJacobianError
    pts, scan = C.cloud("lidar", 8192), C.scans()[3]
    two = np.ascontiguousarray(scan[A.valid_rows(scan, True)][:2])
    ctx = _ctx()
    before, _ = _registered(ctx, pts, scan)
    with pytest.raises(InvalidJacobianError):
        ctx.register(two)
    assert ctx.map_update(None, None) == 0
    after = ctx.map_normals_peek()
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    ctx.register_launch(two)
    assert ctx.map_update(None, None) == 0
    with pytest.raises(InvalidJacobianError):
        ctx.register_end()
    after = ctx.map_normals_peek()
    assert np.array_equal(after.view(np.uint32), before.view(np.uint32))
    assert np.array_equal(ctx.map_points().view(np.uint32), pts.view(np.uint32))
    ctx.close()


def test_behind_a_timed_out_handoff(torch_cuda):
    """The recipe of test_gpu_parity.test_timed_out_handoff_finishes_on_per_iteration_launches ("lead_timeout_ms" at one tick
    of the clock, register_launch / map_update(None, None) / register_end): the device skips the update enqueued behind the
    cut-short loop and icp_register_end repeats it.  The cache behind it is the model applied ONCE to the normals in front
    of it, or cleared — never applied twice, never the old normals still flagged.  Which of the two is printed."""
    from pylidar_slam_amd.synthetic import SceneConfig, make_fixed_map, make_sequence
    cfg = SceneConfig(height=32, width=1024)
    scans, poses = make_sequence(cfg, 6)
    model = np.ascontiguousarray(make_fixed_map(cfg, scans[:4], poses[:4], ref_frame=3, num_points=30_000), F32)
    ctx = _ctx(height=32, width=1024, max_num_alignments=12)
    ctx.map_set(model)
    first = ctx.register(scans[4])
    before = ctx.map_normals_peek()
    assert (before[:, 3] == 1).all() and ctx.handoff_fallbacks() == 0
    ctx.set_option("lead_timeout_ms", 1.0e-5)
    ctx.register_launch(scans[5], first.pose)
    assert ctx.map_update(None, None) == 0
    res = ctx.register_end()
    assert ctx.handoff_fallbacks() == 1, "the hand-off was to time out"
    after = ctx.map_normals_peek()
    if not (after[:, 3] == 1).any():
        assert not after.any()
        print("timed-out hand-off: the repeated update CLEARED the cache")
    else:
        fig = C.check_step("behind a timed-out hand-off", before, after, C.transform_of(res.pose))
        assert fig["after"] == len(model)
        print(f"timed-out hand-off: the repeated update applied the carry ONCE: {fig}")
    ctx.close()


# ---- the chain -------------------------------------------------------------------------------------------------------------
def test_chain_of_a_thousand_updates(torch_cuda):
    """1 000 host-pose updates alternating the 0.1 degree pose and its transpose on the 600-point chain cloud — a vehicle
    standing at a light: no key frame, no re-estimation.  (A) - (C) at every step from the device's previous read-back, (D)
    free-running at 10, 40, 200 and 1 000 steps."""
    pts, rels, figs = C.chain_cloud(), C.chain_poses(C.CHAIN_STEPS), Figures()
    ctx = _ctx()
    n0 = _searched(ctx, pts)
    assert (n0[:, 3] == 1).all()
    rows, share, direction = n0, [], {}
    for k, rel in enumerate(rels, 1):
        assert ctx.map_update(rel, None) == 0
        now = ctx.map_normals_peek()
        fig = C.check_step(f"chain step {k}", rows, now, C.transform_of(rel))
        figs.add(fig)
        share.append(fig["renormalised"] / len(pts))
        rows = now
        if k in C.CHAIN_MARKS:
            direction[k] = C.check_direction(f"chain, {k} steps", n0, now, rels[:k])
    ctx.close()
    share = np.array(share)
    print(f"chain: {figs}")
    print(f"chain: renormalised share per step: first {share[0]:.4f}, second {share[1]:.4f}, from the third on "
          f"{share[2:].min():.4f} - {share[2:].max():.4f} (mean {share[2:].mean():.4f})")
    for k, (angle, ratio) in direction.items():
        print(f"chain: after {k} steps the worst angle to the float64 rotation is {angle:.3e} rad, {ratio:.3f} of the derived bound")
    assert share[0] == 0.0 and (share[1:] > 0).all() and (share < 1).all()


# ---- updates that must not carry -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["insertion", "eviction", "carry_normals_0", "point_to_point", "map_set"])
def test_never_carried(torch_cuda, case):
    """Behind an inserting update, an evicting one, "carry_normals" 0, the point-to-point cost and `map_set` no row is a rotated
    old normal: the cache is zeros (no registration ran on these contexts: nothing is estimated eagerly)."""
    pts, rel = C.cloud("lidar", 1025), C.poses()["small"]
    ctx = _ctx((("carry_normals", 0),) if case == "carry_normals_0" else (), local_map_size=1 if case == "eviction" else 3)
    if case == "eviction":
        ctx.map_update(np.eye(4, dtype=F32), pts)
        ctx.nearest_neighbor_search(pts)
        before = ctx.map_normals_peek()
    else:
        before = _searched(ctx, pts)
    assert (before[:, 3] == 1).all()
    if case in ("insertion", "eviction"):
        assert ctx.map_update(rel, C.cloud("lidar", 1300)[1025:]) == 275
        assert ctx.map_size() == (275 if case == "eviction" else 1300)
    elif case == "map_set":
        ctx.map_set(L.move(C.transform_of(rel), pts))
    else:
        if case == "point_to_point":
            ctx.set_cost("point_to_point_gauss_newton")
        assert ctx.map_update(rel, None) == 0
    after = ctx.map_normals_peek()
    assert C.check_never_carried(case, before, after, C.transform_of(rel)) == 0
    ctx.close()


# ---- the consumer ----------------------------------------------------------------------------------------------------------
def _audit_with_peeked_normals(ctx, model, scan, init, tag, worst):
    """map_lifecycle.check_registration with the normals READ BACK instead of searched for: the registration estimates nothing
    (the read-back is the same behind it) and its last iteration's rows are built from exactly those bits"""
    peeked = ctx.map_normals_peek()
    assert (peeked[:, 3] == 1).all()
    ctx.set_alignment(L.SCHEME, L.SIGMA, L.K_REG, 0.0)
    rc, res = A.raw_register(ctx, scan, init, True)
    rec, mp, nm = A.observe(ctx, rc, res, int(scan.shape[0]))
    assert rec is not None and rec.ix is not None, f"{tag}: the last iteration was not observable"
    behind = ctx.map_normals_peek()
    assert np.array_equal(behind.view(np.uint32), peeked.view(np.uint32)), f"{tag}: a registration changed the normal cache"
    assert L.first_difference(mp, model.map) is None, tag
    found = ~np.isnan(nm).any(axis=1)
    assert np.array_equal(nm[found].view(np.uint32), peeked[found, :3].view(np.uint32)), f"{tag}: a search returns other normals"
    A.audit_run(tag, [rec], scan, model.map, np.ascontiguousarray(peeked[:, :3]), L.SCHEME, L.SIGMA, "point_to_plane", True, None,
                worst, duplicates=True, k_normals=int(ctx.config.num_neighbors_normals))
    assert ctx.handoff_fallbacks() == 0, tag


def test_the_consumer_uses_the_carried_bits(torch_cuda):
    """Behind the 40th step of the chain, and behind the carrying insertion launch, one registration audited (tests/
    iteration_audit.py, its own bars) with the normals as read back: the rows of its last iteration are built from exactly
    the carried bits."""
    scan = C.scans()[3]
    worst = A.Worst("carried normals")
    pts, rels, figs = C.chain_cloud(), C.chain_poses(40), Figures()
    ctx, model = _ctx(), L.MapModel(3)
    rows, _ = _registered(ctx, pts, scan)  # (estimated all at once: a cache filled by searches is estimated AGAIN by the next registration)
    model.set(pts)
    for k, rel in enumerate(rels, 1):
        rows = _host_step(ctx, rel, rows, f"chain step {k}", figs)
        model.update(rel, None)
    _audit_with_peeked_normals(ctx, model, scan, None, "behind 40 carries", worst)
    ctx.close()
    pts = C.cloud("lidar", 4097)
    ctx, model = _ctx(), L.MapModel(3)
    after, res = _registered(ctx, pts, scan)
    model.set(pts)
    for f in range(2):
        after, rc, res = _device_step(ctx, scan, res.pose, after, f"enqueued frame {f}", figs)
        model.update(res.pose, None)
    _audit_with_peeked_normals(ctx, model, scan, np.eye(4, dtype=F32), "behind the carrying insertion launch", worst)
    ctx.close()
    print(f"the consumer: {figs}")
    print(worst)
