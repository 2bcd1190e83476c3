"""The first-iteration build of the fused kernel (`k_iterate_first`, option "first_build") against the path it replaces.

With "first_build" 1 (the default) the first launch of a launched single-sequence registration packs the scan rows, initialises
the registration state and searches every query without a miss list; with 0 — and under each of the conditions the header lists
— `k_pack_targets` and the generic kernel run.  Both must give the same bits: every case runs the same inputs under 1 and under
0 and compares the NN-cache entries a 1-iteration registration leaves (`last_cache_entries`: candidate set, bound, iteration,
pose history — read through the packed targets) and the whole result of a 20-iteration one (pose, parameters, loss and step
history, counts), asserts which path was taken (`first_build_launches`) and that no hand-off fell back.

The two runs of a case share ONE context and one grid build: the runner-up members of a candidate set are chosen by keys that
carry a candidate's place in its cell, and the order of the points inside a cell is settled by atomics at every grid build — two
builds of the same map may name different runners-up (winner and bound are the same), whichever kernel reads them.

The initial guess reaches the library by value (host), from the device state ("last") or — a device tensor — through the plugin's
`init_rpose`, which is where a tensor enters the product: that case drives `MI355XICPFrameToModel`.  A live stop threshold (the
registration enqueued in chunks) is compared as well.

Shapes: 37 rows (less than a pair of waves), 1000 (a ragged last workgroup, no multiple of 128), 64 x 32 and 64 x 256 scans
(four chunks a quarter-scan apart per workgroup), each with "wide_until" 0 and 3 (512 and 1024 threads per workgroup).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
WIDE = (0, 3)
SCHEME, SIGMA = "geman_mcclure", 0.3
_SCENES = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _scans(h, w):
    """four frames of the synthetic room at h x w rays (rendered once per shape)"""
    if (h, w) not in _SCENES:
        from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
        _SCENES[(h, w)] = make_sequence(SceneConfig(height=h, width=w), 4)[0]
    return _SCENES[(h, w)]


def _context(h, w, iters, opts=None, **kw):
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(height=h, width=w, max_num_alignments=iters, threshold_delta_pose=0.0, scheme=SCHEME, sigma=SIGMA, **kw)
    for name, value in (opts or {}).items():
        ctx.set_option(name, value)
    return ctx


def _same_result(a, b, what):
    # (not `normals_computed`: the first registration against a map estimates its normals, whichever path it takes)
    assert a.iterations == b.iterations and a.num_targets == b.num_targets and a.converged == b.converged, what
    for name in ("pose", "params", "losses", "dx"):
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), f"{what}: {name} differs"


def _same_entries(a, b, what):
    assert a["last"] == b["last"], what
    for name in ("members", "bound", "iteration", "pose_hist"):
        assert np.array_equal(a[name], b[name]), f"{what}: cache {name} differs"


def _launch(ctx, scan, first_build, init=None, skip_null=False, with_entries=True):
    """(result, cache entries, did the first-iteration build run) of one launched registration"""
    before = ctx.first_build_launches()
    ctx.set_option("first_build", first_build)
    ctx.register_launch(scan, init, skip_null=skip_null)
    res = ctx.register_end()
    entries = ctx.last_cache_entries(scan.shape[0]) if with_entries else None  # (unfused iterations write no entries)
    ctx.set_option("first_build", 1)
    assert ctx.handoff_fallbacks() == 0
    return res, entries, ctx.first_build_launches() - before


def _both_paths(h, w, model, scan, what, opts=None, init=None, skip_null=False, expect_first=1, with_entries=True, warm=False):
    """1 iteration (the entries launch 0 leaves) and 20 iterations, "first_build" 1 against 0 on one context; the new run's
    20-iteration result and 1-iteration entries.  warm: a registration in front of the compared ones (normals on demand: the
    first run estimates them, and counts them in its result)"""
    ctx = _context(h, w, 1, opts)
    ctx.map_set(model)
    kept = None
    for iters in (1, 20):
        ctx.set_alignment(SCHEME, SIGMA, iters, 0.0)
        if warm:
            _launch(ctx, scan, 0, init, skip_null, with_entries)
        new, new_entries, took = _launch(ctx, scan, 1, init, skip_null, with_entries)
        old, old_entries, took_old = _launch(ctx, scan, 0, init, skip_null, with_entries)
        again, _, took_again = _launch(ctx, scan, 1, init, skip_null, with_entries)
        assert (took, took_old, took_again) == (expect_first, 0, expect_first), f"{what}: path taken {took} / {took_old} / {took_again}"
        assert new.iterations == iters
        _same_result(new, old, f"{what}, {iters} iterations")
        _same_result(again, old, f"{what}, {iters} iterations, again")
        if with_entries:
            _same_entries(new_entries, old_entries, f"{what}, {iters} iterations")
        if iters == 1 and with_entries:  # every entry with a neighbour was written by launch 0
            assert (new_entries["iteration"][new_entries["members"][:, 0] >= 0] == 0).all(), what
            kept = new_entries
    ctx.close()
    return new, kept


@pytest.mark.parametrize("wide_until", WIDE)
@pytest.mark.parametrize("shape", ["n37", "n1000", "64x32", "64x256"])
def test_shapes(torch_cuda, shape, wide_until):
    h, w = (64, 256) if shape == "64x256" else (64, 32)
    scans = _scans(h, w)
    scan = scans[1]
    if shape.startswith("n"):
        scan = np.ascontiguousarray(scan[:int(shape[1:])])
    res, entries = _both_paths(h, w, scans[0], scan, f"{shape}, wide_until {wide_until}", {"wide_until": wide_until})
    assert res.num_targets == scan.shape[0] and (entries["members"][:, 0] >= 0).all()


@pytest.mark.parametrize("wide_until", WIDE)
def test_masked_rows(torch_cuda, wide_until):
    """NaN rows and null rows (skip_null) scattered over the scan, and all 128 rows of one chunk of a workgroup (rows 512..639
    of 2048: the second chunk of workgroup 0); a masked row has no entry."""
    scans = _scans(64, 32)
    scan = scans[1].copy()
    rng = np.random.default_rng(5)
    nan_rows, null_rows = rng.choice(2048, 60, replace=False), rng.choice(2048, 60, replace=False)
    scan[nan_rows, rng.integers(0, 3, 60)] = np.nan
    scan[null_rows] = 0.0
    scan[512:640] = np.nan
    scan[640:700] = 0.0
    masked = np.isnan(scan).any(axis=1) | (scan == 0.0).all(axis=1)
    res, entries = _both_paths(64, 32, scans[0], scan, f"masked rows, wide_until {wide_until}", {"wide_until": wide_until},
                               skip_null=True)
    assert res.num_targets == int((~masked).sum())
    assert (entries["members"][masked] == -1).all() and (entries["iteration"][masked] == -1).all()
    assert (entries["members"][~masked, 0] >= 0).all()


@pytest.mark.parametrize("wide_until", WIDE)
def test_displaced_scan(torch_cuda, wide_until):
    """a scan 1 m off the map: own cells empty, balls that leave their block, queries handed back to phases BF and B1"""
    scans = _scans(64, 32)
    scan = np.ascontiguousarray(scans[1] + np.array([1.0, -0.3, 0.2], F32))
    _both_paths(64, 32, scans[0], scan, f"displaced, wide_until {wide_until}", {"wide_until": wide_until})
    # ... and a map so sparse that most own cells are empty
    _both_paths(64, 32, np.ascontiguousarray(scans[0][::7]), scan, f"displaced, sparse map, wide_until {wide_until}",
                {"wide_until": wide_until})


@pytest.mark.parametrize("wide_until", WIDE)
def test_frames_with_and_without_seeds(torch_cuda, wide_until):
    """A sequence on one context: frame k registers scan k and inserts it; the map keeps two clouds, so the first frame has
    no frame seeds, the second has them, and from the third on the seeds of evicted points are gone and the others shifted.
    Every frame runs under 1 with the guess "last" (read on the device), under 0 with the same pose by value, and under 1
    again by value — against the same grid — before its cloud goes into the map."""
    scans = _scans(64, 32)
    ctx = _context(64, 32, 3, {"wide_until": wide_until}, local_map_size=2)
    ctx.map_update(np.eye(4, dtype=F32), scans[0])
    last_pose = None
    for k in range(1, 4):
        what = f"frame {k}, wide_until {wide_until}"
        new, new_entries, took = _launch(ctx, scans[k], 1, "last" if k > 1 else None)
        old, old_entries, took_old = _launch(ctx, scans[k], 0, last_pose)
        again, again_entries, took_again = _launch(ctx, scans[k], 1, last_pose)
        assert (took, took_old, took_again) == (1, 0, 1), what
        _same_result(new, old, what)
        _same_entries(new_entries, old_entries, what)
        _same_result(again, old, what + ", by value")
        _same_entries(again_entries, old_entries, what + ", by value")
        last_pose = new.pose
        ctx.map_update(None, scans[k])
    ctx.close()


GUESS = np.array([0.35, -0.02, 0.01, 0.001, -0.002, 0.012])


def test_initial_guess_from_the_host(torch_cuda):
    """the guess by value from the host ("last", read on the device: test_frames_with_and_without_seeds)"""
    from pylidar_slam_amd.synthetic import pose_matrix
    scans = _scans(64, 32)
    by_host, _ = _both_paths(64, 32, scans[0], scans[1], "host guess", init=pose_matrix(GUESS).astype(F32))
    identity, _ = _both_paths(64, 32, scans[0], scans[1], "identity")
    assert not np.array_equal(identity.losses, by_host.losses)  # (the guess is used)


def _plugin_drive(torch, first_build, guess):
    """three frames through the plugin (`MI355XICPFrameToModel.process_next_frame`: the frame calls of the library), the
    initial estimate of every frame handed over as `init_rpose` = `guess(frame)`"""
    from pylidar_slam_amd.odometry import MI355XICPConfig, MI355XICPFrameToModel, SphericalProjector
    scans = _scans(64, 32)
    cfg = MI355XICPConfig(max_num_alignments=8, threshold_delta_pose=0.0, data_key="numpy_pc")
    odo = MI355XICPFrameToModel(cfg, projector=SphericalProjector(64, 32), device=torch.device("cuda:0"))
    odo.init()
    odo.ctx.set_option("first_build", first_build)
    out = []
    for f in range(3):
        d = {"numpy_pc": scans[f], "init_rpose": guess(f)}
        odo.process_next_frame(d)
        if f:
            r = odo.last_result
            out.append((np.array(d["odometry_pose"]), np.array(r.pose), np.array(r.losses), np.array(r.dx), r.iterations))
    took, fallbacks = odo.ctx.first_build_launches(), odo.ctx.handoff_fallbacks()
    odo.ctx.close()
    assert fallbacks == 0
    return out, took


def test_initial_guess_as_a_device_tensor(torch_cuda):
    """`init_rpose` as a CUDA tensor ([1,4,4] float32 and bfloat16: a pose network's output) is where a device tensor enters the
    product: the plugin brings its 16 numbers to the host and the frame call hands them to the library by value.  Under
    "first_build" 1 and 0, and against the same numbers given as a numpy array."""
    from pylidar_slam_amd.synthetic import pose_matrix
    torch = torch_cuda
    pose = pose_matrix(GUESS).astype(F32)
    for dtype in (torch.float32, torch.bfloat16):
        as_tensor = lambda f: torch.from_numpy(pose).to("cuda:0", dtype).reshape(1, 4, 4)  # noqa: E731
        as_array = lambda f: as_tensor(f).to(torch.float32).cpu().numpy()  # noqa: E731  (the same numbers after the cast)
        new, took = _plugin_drive(torch, 1, as_tensor)
        old, took_old = _plugin_drive(torch, 0, as_tensor)
        host, took_host = _plugin_drive(torch, 1, as_array)
        assert (took, took_old, took_host) == (2, 0, 2), f"{dtype}: first-build launches {took} / {took_old} / {took_host}"
        for k, (a, b, c) in enumerate(zip(new, old, host)):
            assert a[4] == b[4] == c[4] == 8
            for x, y, z in zip(a[:4], b[:4], c[:4]):
                assert np.array_equal(x, y) and np.array_equal(x, z), f"{dtype}, frame {k + 1}"
    # (the guess is used: the identity gives other losses)
    ident, _ = _plugin_drive(torch, 1, lambda f: None)
    assert not np.array_equal(ident[0][2], new[0][2])


def test_live_threshold_in_chunks(torch_cuda):
    """the published configuration's path: threshold_delta_pose 1e-4, the registration enqueued in chunks — the first chunk
    begins with the first-iteration build, `register_end` enqueues the later ones, the loop stops on the device.  Two
    registrations per path (the second chunk size follows the iterations the first one ran), 1 against 0 on one context."""
    scans = _scans(64, 32)
    for wide_until in WIDE:
        ctx = _context(64, 32, 20, {"wide_until": wide_until})
        ctx.set_alignment(SCHEME, SIGMA, 20, 1.0e-4)
        ctx.map_set(scans[0])
        runs = [_launch(ctx, scans[1], fb) for fb in (1, 1, 0, 0, 1)]
        assert [r[2] for r in runs] == [1, 1, 0, 0, 1]
        ref, ref_entries, _ = runs[2]
        print(f"live threshold, wide_until {wide_until}: {ref.iterations} iterations, converged {ref.converged}")
        assert ref.iterations >= 1
        for k in (0, 1, 3, 4):
            _same_result(runs[k][0], ref, f"live threshold, wide_until {wide_until}, run {k}")
            _same_entries(runs[k][1], ref_entries, f"live threshold, wide_until {wide_until}, run {k}")
        ctx.close()


# one case per option under which the packing launch and the generic kernel still run
FALLBACKS = {
    "unfused": {"fuse_iteration": 0},
    "lazy_normals": {"lazy_fused": 2},
    "hit_records": {"hit_records": 1},
    "search_stats": {"search_stats": 1},
    "no_ball_search": {"ball_search": 0},
    "dense_shape": {"narrow_from": 3},
    "wide_with_one_lane": {"ball_lanes": 1, "wide_until": 3},
}


@pytest.mark.parametrize("name", list(FALLBACKS))
def test_fall_back_by_option(torch_cuda, name):
    scans = _scans(64, 32)
    _both_paths(64, 32, scans[0], scans[1], name, FALLBACKS[name], expect_first=0, with_entries=name != "unfused",
                warm=name == "lazy_normals")


def test_options_that_keep_the_build(torch_cuda):
    """one lane per query in the 512-thread shape, a resident tail from iteration 1 on (there is none from iteration 0: it
    needs rows to solve), classic launches without a lead, no XCD sectors"""
    scans = _scans(64, 32)
    for what, opts in (("ball_lanes 1, 512 threads", {"ball_lanes": 1, "wide_until": 0}),
                       ("tail from 1", {"resident_tail": 1, "wide_until": 0}),
                       ("no lead launches", {"lead_solve": 0}), ("xcd sectors off", {"xcd_sectors": 0})):
        _both_paths(64, 32, scans[0], scans[1], what, opts)


def test_fall_back_by_call(torch_cuda):
    """the event profile, the in-library exchange, the polled `register` and a batched launch"""
    from pylidar_slam_amd.engine import IcpBatch
    scans = _scans(64, 32)
    ctx = _context(64, 32, 20)
    ctx.map_set(scans[0])
    ref, ref_entries, took = _launch(ctx, scans[1], 0)
    assert took == 0

    def kept(what, expect=0):
        res, entries, took = _launch(ctx, scans[1], 1)
        assert took == expect, what
        _same_result(res, ref, what)
        _same_entries(entries, ref_entries, what)

    ctx.profile_enable(1)
    kept("event profile")
    ctx.profile_enable(0)
    ctx.exchange_connect([ctx.exchange_create(0, 1)])  # (a world of one rank: the exchange is on)
    kept("exchange of one rank")
    ctx.exchange_destroy()
    kept("conditions lifted", 1)
    before = ctx.first_build_launches()
    res = ctx.register(scans[1])   # the host polls: begin + per-iteration launches
    assert ctx.first_build_launches() == before
    _same_result(res, ref, "polled register")
    ctx.close()

    ctxs = [_context(64, 32, 20) for _ in range(2)]
    for c in ctxs:
        c.map_set(scans[0])
    batch = IcpBatch(ctxs)
    batch.register_launch([scans[1], scans[1]])
    for c, res in zip(ctxs, batch.register_end()):
        assert c.first_build_launches() == 0 and c.handoff_fallbacks() == 0
        _same_result(res, ref, "batched launch")
    batch.close()
    for c in ctxs:
        c.close()
