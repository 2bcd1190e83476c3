"""`-m gpu`: the kNN map normals on every kernel and path against the bit model of tests/normals_audit.py — EVERY map point,
bit for bit, nobody exempt: the sharded kernels (one, two and three ranks), the lazy worklist (4 and 2 lanes, shorter than a
workgroup and longer than its grid), the eager kernels (two lanes with in-launch stragglers, the stragglers in a launch of
their own on either stream, the four-lane list walk, the row walk with 4 and 2 lanes, k = 20), the lazy estimation inside the
fused iteration, the batched launch, every generic k, and the map after an insertion and an eviction.  The k-NN query (another
kernel) must name the same neighbour sets as the model.

The clouds (normals_audit.clouds / tiny_maps / edge_maps): an 8 192-point LiDAR map, the 24 x 24 x 12 lattice, exact duplicates,
isolated points, a 10 km offset, a line, an exact plane, maps of 1, 2, k, k + 1, k + 2 points and maps at the workgroup edges.
The model flags none of their points and none is order-dependent.

Measured on an MI355X: 29 tests in 13 s, NO point differs from the model, 0 flagged, 0 order-dependent.  Points compared:
sharded 416 326 (k = 5, 10, 20; one, two and three ranks, "hoods" 2, 1, 0), lazy worklist 68 598 with 4 lanes and as many with 2,
262 656 / 525 312 on the tiled lattice, each of the five eager forms 68 499, stragglers on the map stream 10 000, lazy in the
registration 16 384 per form (441 / 440 normals by the registration itself), batched 7 817, generic k 205 630, after insertion
and eviction 26 000; 218 536 k-NN rows equal.  Worst float64 ratio of the library's normals 3.13 (k = 32 on the offset cloud; 2.62
for k = 5, 10, 20), bar 12.56.  A kernel trace of one run names every normals kernel of search.hip, k_normals_tail<11 | 6>,
k_normals_hood2_batch<11 | 6> and k_iterate_compact<..., LAZY_KN = 11 | 6> included.  The library has no counter of stragglers
that a test can read without "search_stats", so their number is not printed; a point of a duplicate that is not the lowest
index of its twins is never a search's answer, so the eager and lazy paths are compared on the points a search can return (the
sharded path returns all)."""

import numpy as np
import pytest

import normals_audit as N

pytestmark = pytest.mark.gpu

FIGURES = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _ctx(k, opts=(), iters=1, **kw):
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(height=16, width=512, num_neighbors_normals=k, max_num_alignments=iters, threshold_delta_pose=0.0, **kw)
    for name, value in opts:
        ctx.set_option(name, value)
    return ctx


def _maps(k, tiny=True, edges=True):
    out = dict(N.clouds())
    if tiny:
        out.update(N.tiny_maps(k))
    if edges:
        out.update(N.edge_maps())
    return out


def _hold(path, name, cloud, k, normals, rows=None):
    """`normals` [M, 3] by original index against the model of `cloud` on `rows` (all), bit for bit; the figures of the path"""
    want = N.model(name, cloud, k)
    flagged, dependent = N.check_caps(want, name)
    normals = np.ascontiguousarray(np.asarray(normals)[:, :3], np.float32)
    compared = N.check_bits(normals, want, rows, f"{path}, {name}")
    use = np.flatnonzero(~want.left_out) if rows is None else np.setdiff1d(rows, np.flatnonzero(want.left_out))
    ratio, determined = N.truth_ratio(normals, N.truth(name, cloud, k), use)
    assert ratio <= N.BAR, (path, name, k, ratio)
    f = FIGURES.setdefault(path, {"points": 0, "flagged": 0, "order_dependent": 0, "ratio": 0.0, "determined": 0})
    f["points"] += compared
    f["flagged"] += flagged
    f["order_dependent"] += dependent
    f["determined"] += determined
    f["ratio"] = max(f["ratio"], ratio)
    return compared


def _report(path):
    f = FIGURES.get(path)
    if f:
        print(f"{path}: {f['points']} map points compared bit for bit, {f['flagged']} flagged, {f['order_dependent']} "
              f"order-dependent; worst float64 ratio of the library's normals {f['ratio']:.2f} over {f['determined']} determined")


def _searched(ctx, queries, m):
    """(normals by original index [M, 3] (NaN: not reached), the indices reached, the index per query) through
    nearest_neighbor_search"""
    _, nm, ix = ctx.nearest_neighbor_search(np.ascontiguousarray(queries, np.float32), with_index=True)
    out = np.full((m, 3), np.nan, np.float32)
    out[ix] = nm
    # (two queries with one neighbour got one normal)
    assert np.array_equal(out[ix].view(np.uint32), nm.view(np.uint32))
    return out, np.unique(ix), ix


def _owned(ctx, world, m):
    """the ranks' shares put together (by ownership, not by a sum: -0.0 + 0.0 would lose a sign bit); every point has one owner"""
    parts = [ctx.map_normals_owned(r, world).cpu().numpy() for r in range(world)]
    out = np.zeros((m, 3), np.float32)
    owners = np.zeros(m, np.int32)
    for p in parts:
        mine = p[:, 3] == 1.0
        assert not p[~mine].any(), "a rank wrote a point it does not own"
        owners += mine
        out[mine] = p[mine, :3]
    assert np.array_equal(owners, np.ones(m, np.int32)), (world, np.flatnonzero(owners != 1)[:5])
    return out


# ---- sharded -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", N.GRID_KS)
def test_sharded_normals_of_one_two_and_three_ranks(torch_cuda, k):
    """k_normals_hood2<KN, true> (k = 5, 10) and k_normals_owned<21, 4> (k = 20); on the LiDAR map, the duplicates and the
    edges also k_normals_hood<KN, true> ("hoods" 1) and k_normals_owned<KN, 4> ("hoods" 0)"""
    path = f"sharded k {k}"
    for name, cloud in _maps(k).items():
        m = cloud.shape[0]
        earlier = name in ("lidar", "duplicates", "isolated", "edge63", "edge65", "edge129", f"m{k}", f"m{k + 1}")
        for hoods in (2, 1, 0) if earlier else (2,):
            ctx = _ctx(k, (("hoods", hoods),))
            ctx.map_set(cloud)
            for world in (1, 2, 3) if hoods == 2 else (1, 2):
                _hold(path, name, cloud, k, _owned(ctx, world, m))
            ctx.close()
    _report(path)


# ---- lazy worklist -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [4, 2])
def test_lazy_worklist_normals(torch_cuda, lanes):
    """k_normals<KN, NL>: a bare search on a fresh context estimates the normals of the map points it returns — the whole map
    queried with itself, and ten queries on another fresh context (a worklist shorter than a workgroup)"""
    path = f"lazy worklist, {lanes} lanes"
    for k in N.GRID_KS:
        for name, cloud in _maps(k).items():
            m = cloud.shape[0]
            ctx = _ctx(k, (("knn_lanes", lanes),))
            ctx.map_set(cloud)
            got, rows, ix = _searched(ctx, cloud, m)
            ctx.close()
            # (a map point's nearest neighbour is the first key of its list: itself, or a twin with a lower index)
            assert np.array_equal(ix, N.model(name, cloud, k).keys[:, 0]), name
            _hold(path, name, cloud, k, got, rows)
            if name in ("lidar", "duplicates", "edge65", "edge1025"):
                ctx = _ctx(k, (("knn_lanes", lanes),))
                ctx.map_set(cloud)
                got, rows, _ = _searched(ctx, cloud[m // 2:m // 2 + 10], m)
                ctx.close()
                assert 1 <= rows.size <= 10
                _hold(path, name, cloud, k, got, rows)
    _report(path)


@pytest.mark.parametrize("lanes", [4, 2])
def test_worklist_longer_than_its_grid(torch_cuda, lanes):
    """A worklist of more than worklist_blocks' cap times the points of a workgroup: every workgroup takes a second trip.  The
    map is the lattice tiled (normals_audit.tiled_lattice): the model of the lattice holds for every copy."""
    shapes = N.launch_shapes()
    per_group = shapes["four_lanes"] if lanes == 4 else shapes["two_lanes"]
    base = N.clouds()["lattice"]
    copies = shapes["worklist_blocks_max"] * per_group // base.shape[0] + 1
    cloud, _ = N.tiled_lattice(copies)
    m = cloud.shape[0]
    assert m > shapes["worklist_blocks_max"] * per_group
    k = 10
    want = N.model("lattice", base, k)
    assert not want.left_out.any()
    ctx = _ctx(k, (("knn_lanes", lanes),))
    ctx.map_set(cloud)
    got, rows, _ = _searched(ctx, cloud, m)
    ctx.close()
    assert rows.size == m
    tiled = np.tile(want.normals, (copies, 1))
    bad = np.flatnonzero(np.any(got.view(np.uint32) != tiled.view(np.uint32), axis=1))
    assert bad.size == 0, (f"{bad.size} of {m} points differ from the model, first {bad[0]} (lattice point {bad[0] % base.shape[0]} "
                           f"of copy {bad[0] // base.shape[0]}): {got[bad[0]].tolist()} against {tiled[bad[0]].tolist()}")
    print(f"worklist longer than its grid, {lanes} lanes: {m} map points ({copies} lattices) compared bit for bit")


# ---- eager ---------------------------------------------------------------------------------------------------------------
EAGER = {
    "two lanes + in-launch stragglers (default)": (),
    "stragglers in their own launch (tail16)": (("normals_list", 1),),
    "four lanes over the lists (hoods 1)": (("hoods", 1),),
    "row walk, four lanes (hoods 0)": (("hoods", 0),),
    "row walk, two lanes (knn_lanes 2)": (("knn_lanes", 2),),
}


@pytest.mark.parametrize("form", list(EAGER))
def test_eager_normals(torch_cuda, form):
    """A registration of the whole map against itself estimates every normal at once (k_normals_hood2 / k_normals_tail16 /
    k_normals_hood / k_normals_all<KN, 4> / <KN, 2>; k = 20 is <21, *> under every option), whatever becomes of the alignment;
    read back through a search, which finds them ready."""
    path = f"eager, {form}"
    for k in N.GRID_KS:
        for name, cloud in _maps(k).items():
            m = cloud.shape[0]
            ctx = _ctx(k, EAGER[form])
            ctx.map_set(cloud)
            try:
                res = ctx.register(cloud)
                assert res.normals_computed == m, (name, k, res.normals_computed)   # all of them, at once
            except RuntimeError:
                assert name != "lidar"                                              # (a degenerate alignment: line, plane, M = 1)
            got, rows, _ = _searched(ctx, cloud, m)
            ctx.close()
            _hold(path, name, cloud, k, got, rows)
    _report(path)


def _scan_of(cloud, step):
    return np.ascontiguousarray(cloud[::step])


def _moved(scan):
    """the scan 5 cm and 0.01 rad off the map: a registration with something to do"""
    c, s = np.cos(0.01), np.sin(0.01)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    return np.ascontiguousarray(scan.astype(np.float64) @ rot.T + np.array([0.05, 0.02, 0.01]), np.float32)


@pytest.mark.parametrize("k", [10, 5])
def test_stragglers_on_the_map_stream_behind_an_update(torch_cuda, k):
    """"normals_tail_stream" 1: behind a map update the two-lane kernel lists its stragglers and k_normals_tail finishes them on
    the map stream.  The map is what map_points() says after the update."""
    path = f"eager, stragglers on the map stream (k_normals_tail), k {k}"
    torch = torch_cuda
    lidar = N.lidar()
    ctx = _ctx(k, (("normals_tail_stream", 1),), iters=2, local_map_size=2)
    # (the context's own stream must be another than its map stream: on the default stream the tail stays in the launch)
    with torch.cuda.stream(torch.cuda.Stream()):
        ctx.use_torch_stream()
        ctx.map_update(np.eye(4, dtype=np.float32), torch.tensor(lidar[:3000]).cuda())
        res = ctx.register(torch.tensor(_scan_of(lidar[:3000], 2)).cuda())
        ctx.map_update(res.pose, torch.tensor(lidar[3000:5000]).cuda())
        cloud = ctx.map_points()
        assert cloud.shape[0] == 5000
        got, rows, _ = _searched(ctx, cloud, 5000)
        torch.cuda.current_stream().synchronize()
    ctx.close()
    _hold(path, f"tail_stream_{k}", cloud, k, got, rows)
    _report(path)


# ---- lazy inside the fused iteration -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [2, 0])
def test_lazy_normals_of_a_small_scan(torch_cuda, fused):
    """"eager_normals_limit" 0 and a scan of 300 targets against the 8 192-point map: the registration estimates the normals of
    the map points it touches — inside k_iterate_* ("lazy_fused" 2: lazy_cov_*, normal_from_cov) or through the worklist between
    the iterations (0) — and a search of the whole map the rest.  All equal the model."""
    path = f"lazy in the registration (lazy_fused {fused})"
    lidar = N.lidar()
    for k in (10, 5):
        ctx = _ctx(k, (("eager_normals_limit", 0), ("lazy_fused", fused)), iters=3)
        ctx.map_set(lidar)
        res = ctx.register(_moved(_scan_of(lidar, 27)[:300]))
        assert 0 < res.normals_computed <= 3 * 300 and res.iterations == 3, (res.normals_computed, res.iterations)
        touched = res.normals_computed
        got, rows, _ = _searched(ctx, lidar, lidar.shape[0])
        ctx.close()
        _hold(path, "lidar", lidar, k, got, rows)
        print(f"{path}, k {k}: {touched} normals estimated by the registration, the rest by the search")
    _report(path)


# ---- batched -------------------------------------------------------------------------------------------------------------
def test_batched_map_update_normals(torch_cuda):
    """IcpBatch.map_update_staged on four members with maps of different sizes: k_normals_hood2_batch<11> (two members) and <6>
    (one) in one call, beside a member that takes its own launch ("normals_list" 1)."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch
    path = "batched map update"
    lidar = N.lidar()
    ks = (10, 10, 5, 10)
    first = (1500, 700, 2500, 900)
    second = (1000, 129, 63, 1025)
    ctxs = [_ctx(k, (("normals_list", 1),) if b == 3 else (), iters=2, local_map_size=2) for b, k in enumerate(ks)]
    batch = IcpBatch(ctxs)
    batch.use_torch_stream()
    scans = []
    for c, n0, n1 in zip(ctxs, first, second):
        c.map_update(np.eye(4, dtype=np.float32), torch.tensor(lidar[:n0]).cuda())
        c.map_stage_cloud(torch.tensor(lidar[4000:4000 + n1]).cuda())
        scans.append(torch.tensor(_scan_of(lidar[:n0], 2)).cuda())
    batch.register_launch(scans, None)
    results = batch.register_end()
    inserted = batch.map_update_staged([1, 1, 1, 1], [r.pose for r in results])
    assert inserted == list(second)
    for b, (c, k) in enumerate(zip(ctxs, ks)):
        cloud = c.map_points()
        assert cloud.shape[0] == first[b] + second[b]
        got, rows, _ = _searched(c, cloud, cloud.shape[0])
        _hold(path, f"batch_member_{b}", cloud, k, got, rows)
    batch.close()
    for c in ctxs:
        c.close()
    _report(path)


# ---- generic k -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", N.GENERIC_KS)
def test_generic_k(torch_cuda, k):
    """k_normals_generic (every num_neighbors_normals other than 5, 10, 20): 65-entry lists, an exhaustive scan, plain float32
    sums — through a bare search and through a registration (which leaves a generic k to the worklist) followed by a search;
    maps below, at and above k + 1 points; the sharded entry point refuses them."""
    path = f"generic k {k}"
    maps = _maps(k, edges=False)
    maps.update({n: c for n, c in N.edge_maps().items() if n in ("edge63", "edge64", "edge65", "edge127", "edge128", "edge129")})
    for name, cloud in maps.items():
        m = cloud.shape[0]
        ctx = _ctx(k)
        ctx.map_set(cloud)
        with pytest.raises(AssertionError, match="5, 10 or 20"):
            ctx.map_normals_owned(0, 1)
        got, rows, _ = _searched(ctx, cloud, m)
        ctx.close()
        _hold(path, name, cloud, k, got, rows)
        if name in ("lidar", "duplicates", "isolated", "edge129", f"m{k + 1}", f"m{k + 2}"):
            ctx = _ctx(k, iters=2)
            ctx.map_set(cloud)
            try:
                res = ctx.register(_scan_of(cloud, 3))
                assert 0 < res.normals_computed <= 2 * m
            except RuntimeError:
                pass
            got, rows, _ = _searched(ctx, cloud, m)
            ctx.close()
            _hold(path, name, cloud, k, got, rows)
    _report(path)


# ---- after insertion and eviction ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [10, 5, 20, 7])
def test_normals_after_insertion_and_eviction(torch_cuda, k):
    """A "local_map_size" 2 context: an update that inserts a cloud, one that evicts the oldest.  After each the normals are the
    model's of what map_points() says is there (tests/map_lifecycle.py holds THAT to its own model)."""
    path = f"after insertion and eviction, k {k}"
    lidar = N.lidar()
    parts = (lidar[:2000], lidar[2000:3500], lidar[3500:5000])
    ctx = _ctx(k, iters=2, local_map_size=2)
    ctx.map_update(np.eye(4, dtype=np.float32), parts[0])
    sizes = []
    for step, new in enumerate(parts[1:]):
        res = ctx.register(_scan_of(new, 2))
        ctx.map_update(res.pose, new)
        cloud = ctx.map_points()
        sizes.append(cloud.shape[0])
        got, rows, _ = _searched(ctx, cloud, cloud.shape[0])
        _hold(path, f"lifecycle_{k}_{step}", cloud, k, got, rows)
    ctx.close()
    assert sizes == [3500, 3000], sizes    # (inserted; then the first cloud evicted)
    _report(path)


# ---- the k-NN query names the same sets ----------------------------------------------------------------------------------
def test_knn_query_names_the_models_neighbour_sets(torch_cuda):
    """knn_query(map, k + 1) — k_knn_query, a kernel of its own — returns the model's key lists, the dropped first key
    included: two independent kernels agree with one model about the set (k + 1 <= 32)."""
    rows = 0
    for name, cloud in _maps(10).items():
        ctx = _ctx(10)
        ctx.map_set(cloud)
        for k in (5, 10, 20, 1, 2, 3, 7, 12):
            want = N.model(name, cloud, k)
            _, index = ctx.knn_query(cloud, k + 1)
            use = ~want.flagged
            bad = np.flatnonzero(np.any(index != want.keys, axis=1) & use)
            assert bad.size == 0, (name, k, bad[:5], index[bad[0]].tolist(), want.keys[bad[0]].tolist())
            rows += int(use.sum())
        ctx.close()
    print(f"k-NN query against the model's neighbour lists: {rows} rows equal")
