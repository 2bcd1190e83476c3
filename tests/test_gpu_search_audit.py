"""The exact 1-NN search against its bit model at the faces of its own cells (tests/search_audit.py).

The rest of the suite holds this search to a kd-tree with a tolerance, on random and synthetic clouds, and to itself across
schedule options on one benign scene.  Here every query row of every cloud — face triples found by searching for
configurations in which a strict box-gap prune answers the wrong point, edges and corners, exact ties, empty own cells, the
early exit at rings 1, 2 and 4, the coarse level, coordinates beyond the cell clamp, a cell of 300 points, workgroups with
16 / 17 ... 256 / 257 own-cell-empty rows — is compared with the model INDEX FOR INDEX on every unflagged row (none is
flagged: the CPU suite asserts the cap), through `nearest_neighbor_search`, `knn_query`, the first iteration of the fused
kernel under 21 option sets, the NN cache across six iterations, one `IcpBatch` launch and a three-frame chain.

tests/test_search_audit.py shows on the CPU that each check fails the wrong copy meant for it.
"""
import numpy as np
import pytest

import knn_audit as K
import search_audit as S

pytestmark = pytest.mark.gpu
F32 = np.float32

OPTION_SETS = {
    "defaults": {},
    "no_guard_no_refresh": {"prune_guard": 0.0, "refresh_margin": 0.0},
    "no_cache": {"nn_cache": 0},
    "no_ball_search": {"ball_search": 0},
    "ball_one_lane": {"ball_lanes": 1},
    "no_ball_empty": {"ball_empty": 0},
    "ball_max_16": {"ball_max": 16},
    "no_far_lanes": {"far_lanes": 0},
    "far_min_0": {"far_min": 0},
    "far_max_512": {"far_max": 512},
    "no_wave_search": {"wave_misses": 0, "wave_misses_dense": 0},
    "wave_search_always": {"wave_misses": 128, "wave_misses_dense": 128},
    "never_narrow": {"narrow_from": -1},
    "narrow_always": {"narrow_from": 0},
    "never_wide": {"wide_until": 0},
    "always_wide": {"wide_until": 99},
    "flat_rows_0": {"flat_rows": 0},
    "flat_rows_1": {"flat_rows": 1},
    "hit_records": {"hit_records": 1},
    "late_from_1": {"hit_records": 1, "late_from": 1},
    "unfused": {"fuse_iteration": 0},
}
CACHE_OPTION_SETS = {
    "defaults": {},
    "no_guard_no_refresh": {"prune_guard": 0.0, "refresh_margin": 0.0},
    "cache_no_seed": {"nn_cache": 1},
    "tail_from_1": {"resident_tail": 1, "wide_until": 0},
}
CLOUDS = list(S.CLOUDS)
KNN_CLOUDS = [n for n in CLOUDS if n.startswith(("faces", "corners", "ties", "skew ties", "coarse"))]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _context(cloud, max_rings=2, k=1, opts=None, map_pts=None):
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(height=32, width=1024, max_num_alignments=k, threshold_delta_pose=0.0, scheme="geman_mcclure", sigma=0.3,
                     cell_size=cloud.h, max_rings=max_rings)
    ctx.set_option("xcd_sectors", 0)   # the row order is the block order
    for name, value in (opts or {}).items():
        ctx.set_option(name, value)
    ctx.map_set(cloud.map if map_pts is None else map_pts)
    return ctx


@pytest.mark.parametrize("name", CLOUDS)
def test_nearest_neighbor_search(torch_cuda, name):
    """`nearest_neighbor_search` on every cloud, cell_size = the cloud's h, max_rings 1, 2 and 4, under the defaults and under
    prune_guard 0: the index of every row is the model's, the neighbour returned has the bits of map[index]."""
    cloud = S.cloud(name)
    want = S.model_of(cloud)
    rows = 0
    for max_rings in (1, 2, 4):
        ctx = _context(cloud, max_rings)
        for guard in (None, 0.0):
            if guard is not None:
                ctx.set_option("prune_guard", guard)
            nb, _, ix = ctx.nearest_neighbor_search(cloud.queries, with_normals=False, with_index=True)
            n, _ = S.check_indices(ix, want, f"{name}, max_rings {max_rings}, prune_guard {guard}", nb, cloud.map)
            rows += n
        ctx.close()
    print(f"{name}: {rows} rows compared, {int(want.flagged.sum())} flagged")


@pytest.mark.parametrize("name", KNN_CLOUDS)
def test_knn_query(torch_cuda, name):
    """`knn_query`, k = 1 and 5, on the face, corner, tie and coarse clouds against knn_audit.model_knn_multi: its ring loop
    prunes by the same gaps.  Distances and indices bit for bit; only the adversarial rows and 256 rows of the filler."""
    cloud = S.cloud(name)
    q = np.ascontiguousarray(cloud.queries[cloud.first_adv - 256:])
    want = K.model_knn_multi(cloud.map, q, (1, 5))
    for max_rings in (1, 2):
        ctx = _context(cloud, max_rings)
        for k in (1, 5):
            dist, index = ctx.knn_query(q, k)
            K.check_bits(dist, index, want[k], f"{name}, k {k}, max_rings {max_rings}")
        ctx.close()


UNOBSERVABLE = ("unfused",)   # no fused launch has written the entries `last_neighbors` reads: it refuses


def _first_iteration(cloud, label, opts):
    """(neighbour indices or None, RegisterResult) of one iteration from the identity pose"""
    ctx = _context(cloud, 2, 1, opts)
    res = ctx.register(cloud.queries, None, False)
    if label in UNOBSERVABLE:
        with pytest.raises(AssertionError, match="no fused registration"):
            ctx.last_neighbors(cloud.queries.shape[0])
        ix = None
    else:
        ix, pose = ctx.last_neighbors(cloud.queries.shape[0])
        assert np.array_equal(pose, np.eye(4, dtype=F32)[:3])
    fallbacks = ctx.handoff_fallbacks()
    ctx.close()
    assert res.iterations == 1 and fallbacks == 0
    return ix, res


@pytest.mark.parametrize("name", CLOUDS)
def test_fused_first_iteration(torch_cuda, name):
    """One iteration (max_num_alignments 1, threshold 0) from the identity pose — the transform is exact — with the cloud's
    queries as the scan, then `last_neighbors`, under every option set of OPTION_SETS; no hand-off fallback.
    Every fused set also gives the loss and the step of the default run bit for bit.  `fuse_iteration 0` leaves no entries to
    read neighbours from (`last_neighbors` refuses, asserted): it sums its rows in another order and is held to the default
    run's loss at 1e-6 relative; its search kernel is the one `nearest_neighbor_search` runs, compared index for index in
    test_nearest_neighbor_search."""
    cloud = S.cloud(name)
    want = S.model_of(cloud)
    rows, ref = 0, None
    for label, opts in OPTION_SETS.items():
        ix, res = _first_iteration(cloud, label, opts)
        ref = ref or res
        if ix is not None:
            rows += S.check_indices(ix, want, f"{name}, {label}")[0]
            assert np.array_equal(res.losses, ref.losses) and np.array_equal(res.dx, ref.dx), \
                f"{name}, {label}: not the bits of defaults"
        else:
            np.testing.assert_allclose(res.losses, ref.losses, rtol=1e-6, err_msg=f"{name}, {label}")
    print(f"{name}: {rows} rows compared over {len(OPTION_SETS) - len(UNOBSERVABLE)} option sets")


_POSE_MODELS = {}


def _model_at(cloud, map_pts, scan, pose12, tag=""):
    """the model of `scan` at a pose against a map, computed once per (cloud, pose): the option sets share their poses"""
    key = (cloud.name, tag, np.ascontiguousarray(pose12, F32).tobytes())
    if key not in _POSE_MODELS:
        _POSE_MODELS[key] = S.model_nn(map_pts, scan, pose12)
    return _POSE_MODELS[key]


SHIFT = np.array([1.0e-4, -1.0e-4, 1.0e-4], F32)


@pytest.mark.parametrize("name", list(S.SMALL))
def test_cache_across_iterations(torch_cuda, name):
    """Runs of K = 1 .. 6 iterations at threshold 0 from a scan displaced by 1e-4 m (later iterations move the queries
    across faces by ulps), each run a prefix of the next to the bit; after each run `last_neighbors` against the model at
    the pose of that last iteration.  Defaults, prune_guard 0 with refresh_margin 0, nn_cache 1, and the resident tail."""
    cloud = S.small(name)
    scan = np.ascontiguousarray(cloud.queries + SHIFT)
    rows = flagged = 0
    for label, opts in CACHE_OPTION_SETS.items():
        runs = []
        for k in range(1, 7):
            ctx = _context(cloud, 2, k, opts)
            res = ctx.register(scan, None, False)
            ix, pose = ctx.last_neighbors(scan.shape[0])
            assert ctx.handoff_fallbacks() == 0 and res.iterations == k
            ctx.close()
            runs.append(res)
            n, f = S.check_indices(ix, _model_at(cloud, cloud.map, scan, pose), f"{name}, {label}, iteration {k}")
            rows, flagged = rows + n, flagged + f
        for k, res in enumerate(runs, start=1):
            assert np.array_equal(res.losses, runs[-1].losses[:k]) and np.array_equal(res.dx, runs[-1].dx[:k]), \
                f"{name}, {label}: a run of {k} iterations is no prefix of the run of 6"
    assert flagged <= K.FLAGGED_MAX * (rows + flagged) + 1
    print(f"{name}: {rows} rows compared, {flagged} flagged")


def test_batch_launch(torch_cuda):
    """One `IcpBatch` launch of three contexts with three clouds and cell sizes: one iteration each from the identity."""
    from pylidar_slam_amd.engine import IcpBatch
    clouds = [S.cloud("faces h=0.3"), S.cloud("own cell empty h=0.37"), S.cloud("corners h=0.7")]
    ctxs = [_context(c, 2, 1) for c in clouds]
    batch = IcpBatch(ctxs)
    batch.register_launch([c.queries for c in clouds])
    results = batch.register_end()
    for c, ctx, res in zip(clouds, ctxs, results):
        ix, pose = ctx.last_neighbors(c.queries.shape[0])
        assert res.iterations == 1 and ctx.handoff_fallbacks() == 0 and np.array_equal(pose, np.eye(4, dtype=F32)[:3])
        S.check_indices(ix, S.model_of(c), f"batch, {c.name}")
    batch.close()
    for ctx in ctxs:
        ctx.close()


def test_three_frame_chain(torch_cuda):
    """Three frames, register_launch / map_update(None, None) / register_end with init "last": the pose-only update
    re-expresses the map, so membership is recomputed from moved coordinates.  The neighbours of each frame's last
    iteration against the model on `map_points()` as that frame saw them (a fresh context replays the frames before)."""
    cloud = S.small("faces h=0.3 small")
    rows = flagged = 0
    for f in range(3):
        ctx = _context(cloud, 2, 4)
        for g in range(f):
            ctx.register_launch(np.ascontiguousarray(cloud.queries + SHIFT * F32(g + 1)), "last" if g else None, skip_null=False)
            ctx.map_update(None, None)
            ctx.register_end()
        scan = np.ascontiguousarray(cloud.queries + SHIFT * F32(f + 1))
        mp = ctx.map_points()
        assert f == 0 or not np.array_equal(mp, cloud.map)   # the map was re-expressed
        ctx.register_launch(scan, "last" if f else None, skip_null=False)
        res = ctx.register_end()
        ix, pose = ctx.last_neighbors(scan.shape[0])
        assert res.iterations == 4 and ctx.handoff_fallbacks() == 0
        ctx.close()
        n, fl = S.check_indices(ix, S.model_nn(mp, scan, pose), f"chain, frame {f}")
        rows, flagged = rows + n, flagged + fl
    assert flagged <= K.FLAGGED_MAX * (rows + flagged) + 1
    print(f"chain: {rows} rows compared, {flagged} flagged")
