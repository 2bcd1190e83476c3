"""`-m gpu`: the batched mode (`icp_batch_*`, `IcpBatch`, `MI355XICPFrameToModelBatch`) pinned DIRECTLY — on the reference's
own run, on the float64 oracle and on a brute-force search — instead of through "batched == single, single == reference":

 B  the cell lists of the grid build ("cell_lists": what the benchmark's batched leg runs) through maps that grow, evict,
    are replaced and are built once without lists: every query answered as a float64 brute-force search answers it;
 C  a batched launch at the benchmark size against `tests/golden/c2_reference.npz` (the reference's
    `ICPFrameToModel.register_new_frame`, slam/odometry/icp_odometry.py:248-299), with the single test's tolerances;
 D  the options a batch reads from one member on behalf of all (include/icp_mi355x.h, icp_batch_register_launch): a
    difference is refused before any member changes; the options that travel in the member's descriptor may differ;
 E  a member whose system is singular (optimization.py:334-336) beside healthy ones;
 F  sizes: members of a few hundred targets beside full scans, workgroup counts that are no multiple of 8, masked rows,
    one member, the most members.
(A — the benchmark's option set in a batch — lives in tests/test_gpu_batch.py.)"""
import functools
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import GOLDEN
from test_gpu_batch import BENCH_OPTIONS, _assert_same, _benchmark_sequences, _ctx, _sequences
from test_gpu_batch import _run_batch as _reg_batch
from test_gpu_batch import _run_single as _reg_single
from test_gpu_batch_loop import _assert_same_run, _contexts, _grid_clouds, _scans, mixed_sequences  # noqa: F401 (fixture)
from test_gpu_batch_loop import _run_batch as _loop_batch
from test_gpu_batch_loop import _run_single as _loop_single
from test_gpu_parity import _c2_inputs
from test_loop_reference import published_config

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _member(batched, b):
    return [r for r in batched[0][b]], batched[1][b], batched[2][b]


# ---- B. cell lists through a map that changes, against brute force ------------------------------------------------------
def _brute_force(queries, model):
    """icp_oracle.brute_force_nn (float64, exhaustive) over slices of the queries on a few threads."""
    import icp_oracle as O
    step = 256
    with ThreadPoolExecutor(8) as pool:
        parts = list(pool.map(lambda s: O.brute_force_nn(queries[s:s + step], model, chunk=64),
                              range(0, queries.shape[0], step)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def _assert_exact_search(ctx, scan, tag):
    """The context's grid against a float64 brute-force search over `ctx.map_points()`: 1536 rows of `scan` (strided) and
    512 points a few metres off them.  The index `nearest_neighbor_search` returns refers to the row order of
    `map_points()` (asserted: the returned neighbour IS that row), also behind insertions and evictions, so indices are
    compared: EVERY query returns the brute-force index, or a point at the brute-force distance within rtol 2e-6 (an
    equidistant candidate: the bound of test_c2_full_size_registration_vs_reference_and_oracle).  A slot of the cell table
    that was lost, or left behind by an earlier build, shows up here as a neighbour that is too far.  Then 1024 of the map's
    own points: each returns itself, or an exact duplicate with a lower index."""
    model = ctx.map_points()
    m = model.shape[0]
    assert m > 0, tag
    rows = scan[np.isfinite(scan).all(axis=1) & (np.abs(scan).sum(axis=1) > 0)]
    near = rows[::max(1, rows.shape[0] // 1536)][:1536]
    rng = np.random.default_rng(m)
    far = near[::3] + rng.normal(scale=2.0, size=(near[::3].shape[0], 3)) + np.array([2.0, -3.0, 4.0])
    q = np.ascontiguousarray(np.concatenate([near, far]).astype(np.float32))
    nb, _, ix = ctx.nearest_neighbor_search(q, with_normals=False, with_index=True)
    assert ix.min() >= 0 and ix.max() < m, (tag, int(ix.min()), int(ix.max()), m)
    assert np.array_equal(model[ix], nb), (tag, "the index does not refer to the rows of map_points()")
    bi, bd2 = _brute_force(q, model)
    d2 = ((q.astype(np.float64) - model[ix].astype(np.float64)) ** 2).sum(axis=1)
    other = ix != bi
    np.testing.assert_allclose(d2[other], bd2[other], rtol=2e-6, atol=0.0,
                               err_msg=f"{tag}: {int(other.sum())} of {q.shape[0]} queries off the brute-force index")
    own_rows = np.arange(0, m, max(1, m // 1024))
    sub = np.ascontiguousarray(model[own_rows])
    _, _, own = ctx.nearest_neighbor_search(sub, with_normals=False, with_index=True)
    assert np.array_equal(model[own], sub), (tag, "a map point is not its own nearest neighbour")
    assert (own <= own_rows).all(), (tag, "a duplicate with a HIGHER index was returned")
    return int(other.sum())


PROBE_FRAMES = (11, 15)  # window of 8 clouds: full from frame 7 on for a member that inserts every frame; 15 = the last


def _window8():
    return published_config(local_map=dict(type="kdtree_local_map", local_map_size=8, num_neighbors_normals=10))


def _probe(sequences, log):
    def probe(b, ctx, f):
        if f in PROBE_FRAMES:
            log.append((b, f, ctx.map_num_clouds()))
            _assert_exact_search(ctx, sequences[b][f], ("member", b, "frame", f))
    return probe


def test_cell_lists_through_insertions_and_evictions(torch_cuda, mixed_sequences):
    """One context, a fast drive (a key frame per frame, window of 8: evictions from frame 8 on), the published
    configuration, with "cell_lists" 1 and 0: per frame pose, iteration count, losses and steps, the final map, window and
    trajectory equal bit for bit; behind frames 11 (window long full) and 15 (the last) the grid of EACH run answers a
    few thousand queries as the brute-force search over its map does."""
    drive = mixed_sequences[1]
    runs, logs = [], []
    for lists in (1, 0):
        log = []
        runs.append(_loop_single(torch_cuda, drive, _window8(), {"cell_lists": lists}, probe=_probe([drive], log)))
        logs.append(log)
    _assert_same_run(runs[1], runs[0], "cell_lists 1 vs 0")
    assert runs[0][2] == 8
    for log in logs:  # both probes ran, both on a full window: clouds had been evicted
        assert [(f, clouds) for _, f, clouds in log] == [(11, 8), (15, 8)], log


def test_cell_lists_in_a_batch_of_mixed_key_frame_decisions(torch_cuda, mixed_sequences):
    """A batch of three — a slow member (mostly pose-only updates) beside two fast ones (an insertion and, from frame 8 on,
    an eviction per frame) — with cell lists on and off: batched == single, lists == no lists, bit for bit; and behind
    frames 11 and 15 every member's grid, in every run, against the brute-force search."""
    opts = {1: {"cell_lists": 1}, 0: {"cell_lists": 0}}
    logs = {1: [], 0: [], "single": []}
    batched = {k: _loop_batch(torch_cuda, mixed_sequences, _window8(), [opts[k]] * 3, probe=_probe(mixed_sequences, logs[k]))
               for k in (1, 0)}
    singles = [_loop_single(torch_cuda, seq, _window8(), opts[1], probe=_probe([seq], logs["single"]))
               for seq in mixed_sequences]
    for b in range(3):
        _assert_same_run(singles[b], batched[1][b], f"member {b}: batched vs single, cell lists")
        _assert_same_run(batched[0][b], batched[1][b], f"member {b}: cell lists 1 vs 0")
    # the calls were mixed and clouds were evicted (test_mixed_key_frame_decisions_in_one_update)
    assert singles[0][2] < 8 and singles[1][2] == 8 and singles[2][2] == 8, [s[2] for s in singles]
    for k in (1, 0):
        assert len(logs[k]) == 6 and all(clouds == 8 for b, _, clouds in logs[k] if b > 0), logs[k]
        assert all(clouds < 8 for b, _, clouds in logs[k] if b == 0), logs[k]
    assert len(logs["single"]) == 6


def test_cell_lists_behind_a_build_without_them_and_a_smaller_map(torch_cuda):
    """What "the previous build's lists" means when the build in between had none, and when the map is replaced: a context
    that inserts and evicts with cell lists, ONE build with "cell_lists" 0, lists on again (the next build must clear the
    whole table: the lists it would clear through are not those of the table's last contents), then `map_set` of a
    different, smaller cloud, a registration against it and the pose-only rebuild by its pose.  Behind every step the
    brute-force check; the registration equals, bit for bit, the one of a fresh context without cell lists."""
    torch = torch_cuda
    scans, rel = _scans(6234, 0.4, 13, with_motion=True)
    clouds = _grid_clouds(torch, scans)
    dev = [torch.from_numpy(c).cuda() for c in clouds]
    (ctx,) = _contexts(1, local_map_size=8)
    ctx.set_option("cell_lists", 1)
    for k in range(10):
        ctx.map_update(rel[k] if k > 0 else np.eye(4, dtype=np.float32), dev[k])
    assert ctx.map_num_clouds() == 8  # two clouds evicted
    _assert_exact_search(ctx, scans[9], "lists, ten insertions")
    ctx.set_option("cell_lists", 0)
    ctx.map_update(rel[10], dev[10])
    _assert_exact_search(ctx, scans[10], "one build without lists")
    ctx.set_option("cell_lists", 1)
    ctx.map_update(rel[11], dev[11])
    _assert_exact_search(ctx, scans[11], "lists again")
    other = _scans(9911, 0.3, 2)
    small = np.ascontiguousarray(_grid_clouds(torch, other[:1])[0][::2])
    assert 0 < small.shape[0] < ctx.map_size() // 4
    ctx.map_set(small)
    assert ctx.map_size() == small.shape[0]
    _assert_exact_search(ctx, other[0], "map_set of a smaller cloud")
    target = torch.from_numpy(_grid_clouds(torch, other[1:2])[0]).cuda()
    res = ctx.register(target)
    ctx.map_update(res.pose, None)
    _assert_exact_search(ctx, other[1], "pose-only rebuild behind map_set")
    (plain,) = _contexts(1, local_map_size=8)
    plain.set_option("cell_lists", 0)
    plain.map_set(small)
    ref = plain.register(target)
    plain.map_update(ref.pose, None)
    assert res.iterations == ref.iterations and np.array_equal(res.pose, ref.pose)
    assert np.array_equal(res.losses, ref.losses) and np.array_equal(res.dx, ref.dx)
    assert np.array_equal(ctx.map_points(), plain.map_points())
    ctx.close()
    plain.close()


# ---- C. the batched launch against the reference's own run ---------------------------------------------------------------
_C2 = np.load(os.path.join(GOLDEN, "c2_reference.npz"))
_C2_SCHEMES = [str(v) for v in _C2["schemes"]]


@functools.lru_cache(maxsize=None)
def _c2_golden_inputs():
    scan, model = _c2_inputs()
    assert hashlib.sha1(np.ascontiguousarray(scan).tobytes()).hexdigest() == str(_C2["scan_sha"]), \
        "the seeded generator no longer reproduces the scan the reference was run on"
    assert hashlib.sha1(np.ascontiguousarray(model).tobytes()).hexdigest() == str(_C2["model_sha"])
    return scan, model


@pytest.mark.parametrize("options", ["default", "bench_options"])
@pytest.mark.parametrize("scheme", _C2_SCHEMES)
def test_batched_c2_vs_reference(torch_cuda, scheme, options):
    """BASELINE configs[1] in a batch of three: the golden scan and map (tests/golden/c2_reference.npz: the reference's
    `register_new_frame` on them, 20 forced iterations) as member k for the k-th scheme — every position once —, the other
    two members other 64x2048 scenes.  For the golden member exactly what
    test_c2_full_size_registration_vs_reference_and_oracle asserts for the single context, with its tolerances: 20
    iterations, every target used, the pose within 1e-4 m / 1e-4 rad, params atol 1e-4, losses rtol 2e-3, steps atol 2e-5 —
    with the default options and with the option set of the benchmark's batched leg.  Batched must equal single to the bit
    (asserted too); a miss reports the first iteration at which the two differ."""
    import icp_oracle as O
    g = _C2
    position = _C2_SCHEMES.index(scheme)
    sigma = float(g["sigmas"][position])
    scan, model = _c2_golden_inputs()
    seqs = [(sc[:1], m) for sc, m in _benchmark_sequences()[:2]]
    seqs.insert(position, ([scan], model))
    opts = dict(BENCH_OPTIONS) if options == "bench_options" else {}
    kw = dict(height=64, width=2048, max_num_alignments=int(g["iters"]), threshold_delta_pose=0.0, scheme=scheme, sigma=sigma)
    batched = _reg_batch(kw, opts, seqs, 1, "pose", torch_cuda)
    single = _reg_single(kw, opts, seqs[position], 1, "pose", torch_cuda)
    res, alone = batched[0][position][0], single[0][0]
    differ = [i for i in range(min(res.iterations, alone.iterations))
              if res.losses[i] != alone.losses[i] or not np.array_equal(res.dx[i], alone.dx[i])]
    where = f"{scheme} at position {position}, {options}: batched and single first differ at iteration " \
            f"{differ[0] if differ else None}"
    assert res.iterations == 20 and res.num_targets == scan.shape[0], where
    dt, dr = O.pose_error(res.pose, g[f"{scheme}_pose"])
    print(f"batched C2 {scheme} (member {position}, {options}) vs REFERENCE: |dt| = {dt:.2e} m |dr| = {dr:.2e} rad")
    assert dt < 1e-4 and dr < 1e-4, (where, dt, dr)
    np.testing.assert_allclose(res.params, g[f"{scheme}_params"], atol=1e-4, err_msg=where)
    np.testing.assert_allclose(res.losses, g[f"{scheme}_loss"], rtol=2e-3, err_msg=where)
    np.testing.assert_allclose(res.dx, g[f"{scheme}_dx"], atol=2e-5, err_msg=where)
    _assert_same(single, _member(batched, position), where)


# ---- D. members that differ in a registration option ---------------------------------------------------------------------
SMALL_KW = dict(height=32, width=1024, max_num_alignments=8, threshold_delta_pose=0.0, scheme="geman_mcclure", sigma=0.3)


@functools.lru_cache(maxsize=None)
def _small_sequences():
    """Three 32x1024 drives of four frames against 30 000-point maps (the scenes of test_gpu_batch.py)."""
    return tuple(_sequences(3, 32, 1024, 30_000, 4))


# the shared options (include/icp_mi355x.h, icp_batch_register_launch): name -> a value that is not the default
SHARED_OPTIONS = {"threshold_delta_pose": 1.0e-4, "chunked_launch": 0, "lead_after_dense": 0, "hit_records": 1,
                  "late_from": 2, "late_waves": 6, "wide_until": 0, "narrow_from": 1, "nn_cache": 0, "ball_search": 0}


# ... and the defaults (csrc/icp_internal.h; the stop threshold: SMALL_KW's)
SHARED_DEFAULTS = {"threshold_delta_pose": 0.0, "chunked_launch": 1, "lead_after_dense": 1, "hit_records": 0, "late_from": -1,
                   "late_waves": 8, "wide_until": 3, "narrow_from": 0, "nn_cache": 2, "ball_search": 1}


def _set_shared(ctx, name, value):
    if name == "threshold_delta_pose":
        ctx.set_alignment(SMALL_KW["scheme"], SMALL_KW["sigma"], SMALL_KW["max_num_alignments"], value)
    else:
        ctx.set_option(name, value)


def _same_result(a, b, tag):
    assert a.iterations == b.iterations and a.converged == b.converged and a.num_targets == b.num_targets, tag
    assert np.array_equal(a.pose, b.pose) and np.array_equal(a.params, b.params), tag
    assert np.array_equal(a.losses, b.losses) and np.array_equal(a.dx, b.dx), tag


@pytest.mark.parametrize("name", sorted(SHARED_OPTIONS))
def test_members_that_differ_in_a_shared_option_are_refused(torch_cuda, name):
    """Two healthy contexts that differ in ONE option the batch would read from member 0 on behalf of both:
    `register_launch` raises an AssertionError that names the option — BEFORE any member changes: no hand-off fallback, the
    maps as they were, and each member then registers the same scan ALONE with the bits of a twin that was never in a batch.
    With the option made equal, the SAME batch object registers, and equals the twins run alone.
    (Without the check the batch would run member 1 on member 0's schedule — forced iterations for a member with a live
    threshold, the instantiation picked by the last member's "hit_records" — or refuse from inside the frame.)"""
    from pylidar_slam_amd.engine import IcpBatch
    seqs = _small_sequences()[:2]
    dev = [[torch_cuda.from_numpy(s).cuda() for s in sc[:2]] for sc, _ in seqs]

    def pair():
        ctxs = [_ctx(**SMALL_KW), _ctx(**SMALL_KW)]
        for c, (_, model) in zip(ctxs, seqs):
            c.map_set(torch_cuda.from_numpy(model).cuda())
        _set_shared(ctxs[1], name, SHARED_OPTIONS[name])
        return ctxs

    members, twins = pair(), pair()
    batch = IcpBatch(members)
    before = [c.map_points() for c in members]
    with pytest.raises(AssertionError, match=name):
        batch.register_launch([dev[0][0], dev[1][0]])
    for b, (c, t) in enumerate(zip(members, twins)):
        assert c.handoff_fallbacks() == 0
        assert np.array_equal(c.map_points(), before[b]), (name, b, "the refused call moved a map")
        _same_result(c.register(dev[b][0]), t.register(dev[b][0]), (name, b, "alone after the refusal"))
    # ... the option made equal again (member 0 never left the default)
    for c in (members[1], twins[1]):
        _set_shared(c, name, SHARED_DEFAULTS[name])
    batch.register_launch([dev[0][1], dev[1][1]])
    batch.map_update()
    results = batch.register_end()
    for b, (c, t) in enumerate(zip(members, twins)):
        t.register_launch(dev[b][1], None)
        t.map_update(None, None)
        _same_result(results[b], t.register_end(), (name, b, "batched after the option was made equal"))
        assert np.array_equal(c.map_points(), t.map_points()), (name, b)
        assert c.handoff_fallbacks() == 0 and t.handoff_fallbacks() == 0
    batch.close()
    for c in members + twins:
        c.close()


def test_a_refusal_from_inside_the_frame_gives_the_registration_up(torch_cuda):
    """Equal options that no batched instantiation exists for ("ball_search" 0 on both members: the first iteration would
    run the 128-target shape) pass the option check and are refused while the frame's launches are prepared, behind
    `register_begin` of every member.  Nothing has been launched; the batch must give the registration up completely —
    nothing held back (the next call would otherwise enqueue iterations of a dead registration), no member in
    registration or refusing single calls: each member registers alone with the bits of a twin that was never in a batch,
    and with the option back the SAME batch registers and equals the twins."""
    from pylidar_slam_amd.engine import IcpBatch
    seqs = _small_sequences()[:2]
    dev = [[torch_cuda.from_numpy(s).cuda() for s in sc[:2]] for sc, _ in seqs]

    def pair():
        ctxs = [_ctx(**SMALL_KW), _ctx(**SMALL_KW)]
        for c, (_, model) in zip(ctxs, seqs):
            c.map_set(torch_cuda.from_numpy(model).cuda())
            c.set_option("ball_search", 0)
        return ctxs

    members, twins = pair(), pair()
    batch = IcpBatch(members)
    before = [c.map_points() for c in members]
    for _ in range(2):  # (the second call finds nothing of the first)
        with pytest.raises(AssertionError, match="fused shape"):
            batch.register_launch([dev[0][0], dev[1][0]])
    for b, (c, t) in enumerate(zip(members, twins)):
        assert np.array_equal(c.map_points(), before[b]), b
        _same_result(c.register(dev[b][0]), t.register(dev[b][0]), (b, "alone after the refusal"))
    for c in members + twins:
        c.set_option("ball_search", 1)
    batch.register_launch([dev[0][1], dev[1][1]])
    batch.map_update()
    results = batch.register_end()
    for b, (c, t) in enumerate(zip(members, twins)):
        t.register_launch(dev[b][1], None)
        t.map_update(None, None)
        _same_result(results[b], t.register_end(), (b, "batched after the refusal"))
        assert np.array_equal(c.map_points(), t.map_points()), b
        assert c.handoff_fallbacks() == 0 and t.handoff_fallbacks() == 0
    batch.close()
    for c in members + twins:
        c.close()


def test_options_that_travel_in_the_descriptor_may_differ(torch_cuda):
    """The ball / far search options, "wave_misses", "refresh_at", "frame_seed" and "xcd_sectors" are read per member from
    its own descriptor: a batch whose members differ in them equals, bit for bit, the members run alone with the same
    options — four chained frames."""
    options = [{},
               {"ball_lanes": 2, "ball_empty": 0, "far_lanes": 0, "wave_misses": 8, "refresh_at": 3},
               {"ball_max": 64, "far_min": 4, "far_max": 64, "xcd_sectors": 0, "frame_seed": 0, "refresh_margin": 0.0}]
    kw = dict(SMALL_KW, max_num_alignments=12)
    seqs = list(_small_sequences())
    batched = _reg_batch(kw, options, seqs, 4, "pose", torch_cuda)
    for b, seq in enumerate(seqs):
        _assert_same(_reg_single(kw, options[b], seq, 4, "pose", torch_cuda), _member(batched, b), ("descriptor options", b))


def test_projective_batch_refuses_a_shared_option_that_differs(torch_cuda):
    """`icp_batch_pmap_register_launch` applies the same rule: refused with the option's name, nothing changed — the same
    batch registers once the option is equal, and equals the members registered alone."""
    from pylidar_slam_amd.engine import IcpBatch
    from test_gpu_batch_projective import _contexts as _pm_contexts
    from test_gpu_batch_projective import _rel, _scans as _pm_scans, _vmaps
    torch = torch_cuda
    h, w = 32, 256
    vm = _vmaps(torch, h, w, _pm_scans(h, w, 8707, 0.3, 3))
    pts = vm[2].permute(1, 2, 0).reshape(-1, 3).contiguous()

    def fresh():
        ctxs = _pm_contexts(h, w, 2)
        for c in ctxs:
            c.pmap_init()
            c.pmap_update(np.eye(4, dtype=np.float32), vm[0])
            c.pmap_update(_rel(0), vm[1])
        return ctxs

    expected = [c.pmap_register(pts, _rel(1), skip_null=True) for c in fresh()]
    ctxs = fresh()
    ctxs[1].set_option("wide_until", 0)
    batch = IcpBatch(ctxs)
    with pytest.raises(AssertionError, match="wide_until"):
        batch.pmap_register_launch([pts, pts], [_rel(1), _rel(1)], skip_null=True)
    assert [c.pmap_num_maps() for c in ctxs] == [2, 2]
    ctxs[1].set_option("wide_until", 3)
    batch.pmap_register_launch([pts, pts], [_rel(1), _rel(1)], skip_null=True)
    for b, res in enumerate(batch.register_end()):
        _same_result(res, expected[b], ("projective", b))
    batch.close()
    for c in ctxs:
        c.close()


# ---- E. a member that fails ----------------------------------------------------------------------------------------------
TINY_KW = dict(height=16, width=128, max_num_alignments=4, threshold_delta_pose=0.0)


@functools.lru_cache(maxsize=None)
def _tiny_drives():
    """Three healthy 16x128 drives: (map = scan 0, frames = scans 1 and 2)."""
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    out = []
    for b in range(3):
        scans, _ = make_sequence(SceneConfig(height=16, width=128, seed=1234 + 1000 * b, step=0.3 + 0.05 * b), 3)
        out.append((scans[0], [scans[1], scans[2]]))
    return tuple(out)


def _plane():
    """test_failed_registration_leaves_the_map_where_it_was: a map on the plane z = 0 and targets right above it — every
    row has the same normal, J^T J is singular (the oracle raises "Invalid Jacobian in Gauss Newton minimization" on it)."""
    xs, ys = np.meshgrid(np.arange(40, dtype=np.float32) * 0.1, np.arange(40, dtype=np.float32) * 0.1)
    plane = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size, np.float32)], axis=1)
    return plane, np.ascontiguousarray(plane[::3] + np.array([0.013, 0.007, 0.05], np.float32))


@pytest.mark.parametrize("failing", [(1,), (0,), (0, 2)], ids=["member_1", "first_member", "two_members"])
def test_a_failing_member_costs_its_neighbours_nothing(torch_cuda, failing):
    """A batch of three in the order of the engine's asynchronous loop — register_launch, map_update, register_end — with
    singular members (the plane over a plane) beside healthy ones.  `register_end` raises InvalidJacobianError; the failing
    members' maps stay where they were, bit for bit (the reference raises before `__update_map`, icp_odometry.py:192-199);
    the exception carries the healthy members' results (`.results`, None at the `.failed` positions), equal to the same
    registrations run alone, and so are their maps (re-expressed by the device-resident pose: that pins the pose the device
    kept) and their next frame, registered through the same batch from the device-resident pose after the failing members
    were given a healthy map."""
    from pylidar_slam_amd.engine import IcpBatch, InvalidJacobianError
    drives = _tiny_drives()
    plane, above = _plane()
    alone = []
    for model, frames in drives:  # every healthy registration on a context of its own
        c = _ctx(**TINY_KW)
        c.map_set(model)
        steps = []
        for f, init in ((0, None), (1, "last")):
            c.register_launch(frames[f], init)
            c.map_update(None, None)
            steps.append((c.register_end(), c.map_points()))
        alone.append(steps)
        assert c.handoff_fallbacks() == 0
        c.close()
    ctxs = [_ctx(**TINY_KW) for _ in drives]
    for b, c in enumerate(ctxs):
        c.map_set(plane if b in failing else drives[b][0])
    before = [c.map_points() for c in ctxs]
    batch = IcpBatch(ctxs)
    batch.register_launch([above if b in failing else drives[b][1][0] for b in range(3)])
    batch.map_update()
    with pytest.raises(InvalidJacobianError) as raised:
        batch.register_end()
    assert tuple(raised.value.failed) == tuple(failing)
    results = raised.value.results
    assert len(results) == 3
    for b, c in enumerate(ctxs):
        if b in failing:
            assert results[b] is None
            assert np.array_equal(c.map_points(), before[b]), (b, "the map of a failed registration moved")
        else:
            _same_result(results[b], alone[b][0][0], (failing, b, "beside a failing member"))
            assert np.array_equal(c.map_points(), alone[b][0][1]), (failing, b, "map")
    # the next frame through the same batch, every member from its device-resident pose
    for b in failing:
        ctxs[b].map_set(drives[b][0])
    batch.register_launch([drives[b][1][1] for b in range(3)], "last")
    batch.map_update()
    try:
        nxt = batch.register_end()
    except InvalidJacobianError as err:  # (what a member that failed starts from is its own affair)
        assert set(err.failed) <= set(failing), err.failed
        nxt = err.results
    for b, c in enumerate(ctxs):
        if b not in failing:
            _same_result(nxt[b], alone[b][1][0], (failing, b, "next frame"))
            assert np.array_equal(c.map_points(), alone[b][1][1]), (failing, b, "next map")
        assert c.handoff_fallbacks() == 0
    batch.close()
    for c in ctxs:
        c.close()


# ---- F. sizes ------------------------------------------------------------------------------------------------------------
SIZE_KW = dict(height=32, width=1024, max_num_alignments=12, threshold_delta_pose=0.0, scheme="geman_mcclure", sigma=0.3)
FULL = 32 * 1024
# Workgroups per member in a batched launch: 512 targets each — the 512-thread shape gives a target one lane, the 1024-thread
# shape (the first "wide_until" iterations) two, for the same 512 targets (`IT_THREADS`, csrc/search.hip; the 128-target
# shapes of a single context are not batched).  `per_seq`, the stride from one member's workgroups to the next one's, is the
# count of the largest member.
SIZE_CASES = {
    # 1, 1, 2, 9, 41 and 64 workgroups: per_seq = 64, the small members own 55 to 63 idle ones
    "ragged": [257, 511, 513, 4097, 20 * 1024 + 77, FULL],
    # 55 workgroups for the largest member (27 948 targets) at both shapes — 55 = 6 * 8 + 7 —, 1 and 17 for the others
    "odd_workgroups": [300, 27 * 1024 + 300, 8 * 1024 + 1],
    "one_member": [4097],
}


def _strided(scan, n):
    """`n` rows spread over the whole scan (the first n rows are part of one ring: a near-singular system)."""
    return np.ascontiguousarray(scan[::len(scan) // n][:n])


def _oracle_poses(model, frames):
    """The float64-accumulating oracle (as smoke()) on the same chain: identity, then the previous pose, as initial guess;
    the map re-expressed by every pose."""
    import icp_oracle as O
    cfg = O.ICPOracleConfig(max_num_alignments=SIZE_KW["max_num_alignments"], threshold_delta_pose=0.0,
                            scheme=SIZE_KW["scheme"], sigma=SIZE_KW["sigma"], height=32, width=1024, accumulate=np.float64)
    orc = O.ICPFrameToModelOracle(cfg)
    lm = O.KdTreeLocalMapOracle()
    lm.set_map_pointcloud(model)
    orc.local_map = lm
    pose, out = np.eye(4, dtype=np.float32), []
    for frame in frames:
        _, pose = orc.register_new_frame(frame, pose)
        out.append(pose)
        orc.local_map.update(pose, None)
    return out


@pytest.mark.parametrize("case", sorted(SIZE_CASES))
def test_batched_sizes(torch_cuda, case):
    """Members of very different sizes in one batch, two chained frames of 12 forced iterations, every member a strided
    subset of a 32x1024 scan of its own scene against a 30 000-point map.  Binding: batched == single, bit for bit.  And
    every member's poses against the float64 oracle at the project's bar, 1e-4 m / 1e-4 rad, printed first (the batched
    pose IS the single context's, by the assertion before).  Measured on an MI355X: the bar holds at every size, small
    members included — 257 targets 4e-8 / 4e-7 m (first / second frame), 511: 3e-8 / 9e-8, 513: 1e-8 / 3e-7, 4097: 6e-9 /
    8e-8, 20 557: 2e-9 / 6e-8, 27 948: 2e-9 / 1.2e-6, 32 768: 5e-9 / 4e-7 m; rotations at most 2.2e-7 rad."""
    import icp_oracle as O
    sizes = SIZE_CASES[case]
    scenes = _sequences(len(sizes), 32, 1024, 30_000, 2)
    seqs = [([_strided(s, n) for s in sc], m) for (sc, m), n in zip(scenes, sizes)]
    batched = _reg_batch(SIZE_KW, {}, seqs, 2, "pose", torch_cuda)
    for b, seq in enumerate(seqs):
        single = _reg_single(SIZE_KW, {}, seq, 2, "pose", torch_cuda)
        _assert_same(single, _member(batched, b), (case, sizes[b]))
        assert all(r.iterations == 12 and r.num_targets == sizes[b] for r in single[0])
    for b, (frames, model) in enumerate(seqs):
        ref = _oracle_poses(model, frames)
        errs = [O.pose_error(r.pose, p) for r, p in zip(batched[0][b], ref)]
        print(f"sizes[{case}] member {b}: {sizes[b]} targets, vs oracle " +
              ", ".join(f"|dt| = {dt:.2e} m |dr| = {dr:.2e} rad" for dt, dr in errs))
        for f, (dt, dr) in enumerate(errs):
            assert dt < 1e-4 and dr < 1e-4, (case, sizes[b], f, dt, dr)


def test_batched_member_with_masked_rows(torch_cuda):
    """A member whose scan has NaN rows and all-zero rows mixed in (test_register_masks_nan_and_null_rows), beside two
    clean members, `skip_null`: batched == single, the masked member counts exactly the clean rows, and its poses meet the
    oracle run on the clean rows."""
    import icp_oracle as O
    from pylidar_slam_amd.engine import IcpBatch
    scenes = _sequences(3, 32, 1024, 30_000, 2)
    clean = [_strided(s, 6000) for s in scenes[1][0]]
    dirty = [np.concatenate([c[:100], np.full((7, 3), np.nan, np.float32), c[100:4000], np.zeros((5, 3), np.float32),
                             c[4000:], np.full((3, 3), np.nan, np.float32)]) for c in clean]
    frames = [scenes[0][0], dirty, [_strided(s, 513) for s in scenes[2][0]]]
    ctxs, solo = [_ctx(**SIZE_KW) for _ in range(3)], [_ctx(**SIZE_KW) for _ in range(3)]
    for b in range(3):
        ctxs[b].map_set(scenes[b][1])
        solo[b].map_set(scenes[b][1])
    batch = IcpBatch(ctxs)
    inits, poses = None, []
    for f in range(2):
        batch.register_launch([torch_cuda.from_numpy(frames[b][f]).cuda() for b in range(3)], inits, skip_null=True)
        batch.map_update()
        res = batch.register_end()
        for b in range(3):
            solo[b].register_launch(torch_cuda.from_numpy(frames[b][f]).cuda(), None if inits is None else inits[b],
                                    skip_null=True)
            solo[b].map_update(None, None)
            _same_result(res[b], solo[b].register_end(), ("masked rows", f, b))
            assert np.array_equal(ctxs[b].map_points(), solo[b].map_points()), (f, b)
        assert res[1].num_targets == clean[f].shape[0] and res[1].iterations == 12
        inits = [r.pose for r in res]
        poses.append(res[1].pose)
    for f, (pose, ref) in enumerate(zip(poses, _oracle_poses(scenes[1][1], clean))):
        dt, dr = O.pose_error(pose, ref)
        print(f"masked member, frame {f}: vs oracle |dt| = {dt:.2e} m |dr| = {dr:.2e} rad")
        assert dt < 1e-4 and dr < 1e-4, (f, dt, dr)
    batch.close()
    for c in ctxs + solo:
        assert c.handoff_fallbacks() == 0
        c.close()


def test_the_most_members_and_one_too_many(torch_cuda):
    """ICP_BATCH_MAX_SEQUENCES (32) members — the descriptor table, the lead workgroups at the head of the launch
    (`BATCH_LEAD_SLOTS`) and the result slots at their limit — against 8 192-point maps, sizes from 300 targets to a full
    scan: all 32 equal their singles, bit for bit, over two chained frames.  33 contexts are refused."""
    from pylidar_slam_amd import _lib
    from pylidar_slam_amd.engine import IcpBatch
    assert _lib.BATCH_MAX_SEQUENCES == 32
    scenes = _sequences(4, 32, 1024, 8192, 2)
    sizes = [300 + 1047 * b for b in range(31)] + [FULL]  # 300 .. 31 710, then the full scan: 1 .. 64 workgroups
    seqs = [([_strided(s, n) for s in scenes[b % 4][0]], scenes[b % 4][1]) for b, n in enumerate(sizes)]
    batched = _reg_batch(SIZE_KW, {}, seqs, 2, "pose", torch_cuda)
    for b, seq in enumerate(seqs):
        _assert_same(_reg_single(SIZE_KW, {}, seq, 2, "pose", torch_cuda), _member(batched, b), ("32 members", b, sizes[b]))
    ctxs = [_ctx(**SIZE_KW) for _ in range(33)]
    with pytest.raises(AssertionError):
        IcpBatch(ctxs)
    for c in ctxs:
        c.close()
