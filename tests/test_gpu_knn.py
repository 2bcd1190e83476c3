"""`-m gpu`: the k-NN query (icp_knn_query, IcpContext.knn_query, pylidar_slam_amd.kdtree.KDTree; csrc/knn.hip) against the
float32 brute-force model of tests/knn_audit.py — BIT FOR BIT, distances and indices, on every row the model does not flag
(the clouds are chosen so that it flags none): every compiled list length and every round-up, the quad / wave / workgroup
edges of n, maps smaller than k, the coarse level and the exhaustive scan, exact ties, the distance bound, non-finite rows,
the search options, host and device memory, the existing 1-NN, the state a query must leave alone, and the refusals.

Measured on an MI355X: 29 tests in 5 s, no row differs from the model."""

import numpy as np
import pytest

import knn_audit as A

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 8, 9, 11, 12, 16, 17, 31, 32)          # every instantiation and every round-up
SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4097)    # quad, wave, workgroup and second-turn edges for 4 lanes and 1
BOUNDS = (0.05, 0.5, 5.0, np.inf)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    from pylidar_slam_amd.engine import IcpContext
    c = IcpContext(height=16, width=256)
    yield c
    c.close()


def _fresh(**kw):
    from pylidar_slam_amd.engine import IcpContext
    return IcpContext(height=16, width=256, **kw)


@pytest.fixture(scope="module")
def sampled_ctx(ctx):
    """the module's context holding the 6 471-point map (tests that need another map use a fresh context)"""
    ctx.map_set(A.scene()[2])
    return ctx


@pytest.fixture(scope="module")
def mixed_queries():
    """1 024 rows that take every path: rows of the fourth scan, points in the empty cells between the surfaces, points 100 m
    and 10 km from every map point, and one row 256 times"""
    _, queries, sampled = A.scene()
    rng = np.random.default_rng(17)
    lo, hi = sampled.min(axis=0), sampled.max(axis=0)
    between = rng.uniform(lo, hi, (480, 3)).astype(np.float32)
    centre = ((lo + hi) / 2).astype(np.float32)
    far = np.stack([centre + np.array(v, np.float32) for v in
                    ((100, 0, 0), (0, -100, 0), (0, 0, 100), (70, 70, 10), (10000, 0, 0), (0, 10000, 0), (-7000, 7000, 50),
                     (0, 0, -10000))])
    q = np.concatenate((queries[:280], between, far, np.repeat(queries[3000:3001], 256, axis=0)))
    assert q.shape == (1024, 3)
    q = np.ascontiguousarray(q, dtype=np.float32)
    q.setflags(write=False)
    return q


@pytest.fixture(scope="module")
def sweep_models(mixed_queries):
    """{k: model} on the 6 471-point map for the mixed queries, from one evaluation of the distances"""
    models = A.model_knn_multi(A.scene()[2], mixed_queries, KS)
    for r in models.values():
        assert not r.flagged.any()
    return models


def _query(ctx, q, k, **kw):
    dist, index = ctx.knn_query(q, k=k, **kw)
    assert isinstance(dist, np.ndarray) and dist.dtype == np.float32 and dist.shape == (q.shape[0], k)
    assert isinstance(index, np.ndarray) and index.dtype == np.int32 and index.shape == (q.shape[0], k)
    return dist, index


# ---- k and n -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_k_sweep(sampled_ctx, mixed_queries, sweep_models, k):
    dist, index = _query(sampled_ctx, mixed_queries, k)
    A.check_bits(dist, index, sweep_models[k], f"k = {k}")
    # the fallbacks were taken and found neighbours: the far rows are complete, the 256 equal rows are equal
    assert np.all(np.isfinite(dist[760:768])) and np.all(dist[760:768, 0] > 50.0)
    assert np.all(index[768:] == index[768]) and np.all(dist[768:] == dist[768])


def test_size_sweep(sampled_ctx):
    _, queries, sampled = A.scene()
    q = queries[1000:1000 + max(SIZES)]
    want = A.model_knn(sampled, q, 11)
    assert not want.flagged.any()
    for n in SIZES:
        dist, index = _query(sampled_ctx, q[:n], 11)
        A.check_bits(dist, index, A.Knn(want.dist[:n], want.index[:n], want.flagged[:n]), f"n = {n}")
    dist, index = _query(sampled_ctx, q[:0], 11)           # n = 0: nothing written, nothing refused
    assert dist.shape == (0, 11) and index.shape == (0, 11)


@pytest.mark.parametrize("k", (4, 11, 32))
def test_small_maps(torch_cuda, mixed_queries, k):
    _, _, sampled = A.scene()
    c = _fresh()
    try:
        for m in sorted({1, 2, k - 1, k, k + 1}):
            small = np.ascontiguousarray(sampled[::97][:m])
            c.map_set(small)
            dist, index = _query(c, mixed_queries[:300], k)
            want = A.model_knn(small, mixed_queries[:300], k)
            A.check_bits(dist, index, want, f"M = {m}, k = {k}")
            n_found = min(m, k)
            assert np.all(np.isinf(dist[:, n_found:])) and np.all(index[:, n_found:] == m) and np.all(np.isfinite(dist[:, :n_found]))
    finally:
        c.close()


# ---- fallbacks and ties ------------------------------------------------------------------------------------------------------
def test_map_in_one_cell(torch_cuda, mixed_queries):
    rng = np.random.default_rng(23)
    cell = (np.float32(0.2) + rng.uniform(0.0, 0.1, (200, 3))).astype(np.float32)   # inside the cell [0, 0.5)^3
    c = _fresh(cell_size=0.5)
    try:
        c.map_set(cell)
        q = np.ascontiguousarray(np.concatenate((cell[:50], mixed_queries[:200], mixed_queries[756:768])))
        for k in (1, 11, 32):
            dist, index = _query(c, q, k)
            A.check_bits(dist, index, A.model_knn(cell, q, k), f"one cell, k = {k}")
    finally:
        c.close()


@pytest.mark.parametrize("name", ("lattice", "duplicated"))
def test_ties(torch_cuda, name):
    map_pts, queries = getattr(A, name)()
    c = _fresh()
    try:
        c.map_set(map_pts)
        for k in (1, 2, 8, 11, 32):
            dist, index = _query(c, queries, k)
            want = A.model_knn(map_pts, queries, k)
            assert not want.flagged.any()
            A.check_bits(dist, index, want, f"{name}, k = {k}")
            A.check_key_order(map_pts, queries, A.Knn(dist, index, want.flagged), name)
        if name == "lattice":                                # a bound that points sit on exactly: excluded
            dist, index = _query(c, queries, 11, distance_upper_bound=1.0)
            A.check_bits(dist, index, A.model_knn(map_pts, queries, 11, bound=1.0), "lattice, bound 1")
            assert np.all(index[:343, 0] == np.arange(343)) and np.all(index[:343, 1:] == 343)
    finally:
        c.close()


# ---- the distance bound --------------------------------------------------------------------------------------------------------
def test_distance_bound(sampled_ctx, mixed_queries):
    _, _, sampled = A.scene()
    q = mixed_queries
    td, _ = A.truth_knn(sampled, q, 12)
    kinds = set()
    for b in BOUNDS:
        if np.isfinite(b):
            assert not np.any(np.abs(td - b) < 1.0e-6 * b), f"a truth distance lies within 1e-6 of the bound {b}"
        for sqr in (False, True):
            dist, index = _query(sampled_ctx, q, 11, distance_upper_bound=b, sqr_dists=sqr)
            want = A.model_knn(sampled, q, 11, bound=b, sqr=sqr)
            assert not want.flagged.any()
            A.check_bits(dist, index, want, f"bound {b}, sqr_dists = {sqr}")
        found = np.isfinite(dist).sum(axis=1)
        assert np.all((index == 6471) == np.isinf(dist)) and np.all(dist[np.isfinite(dist)] < np.float32(b) * np.float32(b))
        kinds |= {"zero"} if np.any(found == 0) else set()
        kinds |= {"some"} if np.any((found > 0) & (found < 11)) else set()
        kinds |= {"all"} if np.any(found == 11) else set()
        assert np.array_equal(found, (td[:, :11] < b).sum(axis=1))      # the float64 truth agrees on who is inside
    assert kinds == {"zero", "some", "all"}
    # no bound: None, 0 and +inf are the same call
    base = _query(sampled_ctx, q, 11)
    for b in (0.0, np.inf):
        other = _query(sampled_ctx, q, 11, distance_upper_bound=b)
        assert np.array_equal(base[0].view(np.uint32), other[0].view(np.uint32)) and np.array_equal(base[1], other[1])


def test_non_finite_queries(sampled_ctx, mixed_queries):
    q = mixed_queries[:300].copy()
    bad = {5: (0, np.nan), 64: (1, np.inf), 65: (2, -np.inf), 130: (0, -np.inf), 299: (2, np.nan)}
    for row, (axis, v) in bad.items():
        q[row, axis] = v
    clean = A.model_knn(A.scene()[2], mixed_queries[:300], 11)
    for k, bound in ((1, None), (11, None), (11, 0.5), (32, None)):
        dist, index = _query(sampled_ctx, q, k, distance_upper_bound=bound)
        want = A.model_knn(A.scene()[2], q, k, bound=bound)
        A.check_bits(dist, index, want, f"non-finite rows, k = {k}")
        rows = sorted(bad)
        assert np.all(np.isinf(dist[rows])) and np.all(index[rows] == 6471)
        if k == 11 and bound is None:                         # the neighbouring rows are those of the clean call
            keep = np.setdiff1d(np.arange(300), rows)
            A.check_bits(dist, index, clean, "rows beside the non-finite ones", rows=keep)


# ---- options, memory kinds --------------------------------------------------------------------------------------------------------
def test_search_options_never_change_a_result(torch_cuda, mixed_queries, sweep_models):
    _, _, sampled = A.scene()
    q = np.ascontiguousarray(np.concatenate((mixed_queries[:128], mixed_queries[280:408], mixed_queries[756:772])))
    rows = np.concatenate((np.arange(128), np.arange(280, 408), np.arange(756, 772)))
    want = {k: A.Knn(sweep_models[k].dist[rows], sweep_models[k].index[rows], sweep_models[k].flagged[rows]) for k in (11, 32)}
    bounded = A.model_knn(sampled, q, 11, bound=0.5)
    for cell_size in (0.05, 0.0, 5.0):
        for max_rings in (0, 1, 2, 4):
            # icp_create takes max_rings >= 1; what a kNN search reads is the option "knn_rings" — the fine rings it tries before
            # the coarse level, by default min(max_rings, 2) —, which takes 0 (the own cell only) and 4 as well
            c = _fresh(cell_size=cell_size, max_rings=max(max_rings, 1))
            try:
                c.set_option("knn_rings", max_rings)
                c.map_set(sampled)
                what = f"cell_size = {cell_size}, max_rings = {max_rings}"
                for k in (11, 32):
                    dist, index = _query(c, q, k)
                    A.check_bits(dist, index, want[k], what)
                dist, index = _query(c, q, 11, distance_upper_bound=0.5)
                A.check_bits(dist, index, bounded, what + ", bound 0.5")
            finally:
                c.close()


def test_host_and_device_memory_and_single_outputs(torch_cuda, sampled_ctx, mixed_queries, sweep_models):
    torch, c = torch_cuda, sampled_ctx
    q = mixed_queries
    host = _query(c, q, 11)
    dev = c.knn_query(torch.from_numpy(q.copy()).cuda(), k=11)
    assert all(t.is_cuda for t in dev) and dev[0].dtype == torch.float32 and dev[1].dtype == torch.int32
    assert tuple(dev[0].shape) == (1024, 11) and tuple(dev[1].shape) == (1024, 11)
    A.check_bits(dev[0].cpu().numpy(), dev[1].cpu().numpy(), sweep_models[11], "device tensors")
    assert np.array_equal(host[0].view(np.uint32), dev[0].cpu().numpy().view(np.uint32)) and np.array_equal(host[1], dev[1].cpu().numpy())
    empty = c.knn_query(torch.from_numpy(q[:0]).cuda(), k=3)
    assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0, 3)
    # one output only, through the C ABI
    lib, h = c._lib, c._h
    dist, index = np.full((1024, 11), -1.0, np.float32), np.full((1024, 11), -1, np.int32)
    assert lib.icp_knn_query(h, q.ctypes.data, 1024, 0, 11, 0.0, 0, dist.ctypes.data, None, 0) == 0
    assert lib.icp_knn_query(h, q.ctypes.data, 1024, 0, 11, 0.0, 0, None, index.ctypes.data, 0) == 0
    A.check_bits(dist, index, sweep_models[11], "one output per call")
    assert lib.icp_knn_query(h, q.ctypes.data, 1024, 0, 11, 0.0, 0, None, None, 0) == -1
    assert b"both outputs are NULL" in lib.icp_last_error(h)
    assert lib.icp_knn_query(h, q.ctypes.data, -1, 0, 11, 0.0, 0, dist.ctypes.data, None, 0) == -1
    assert lib.icp_knn_query(h, None, 0, 0, 11, 0.0, 0, dist.ctypes.data, None, 0) == 0      # n = 0 writes nothing
    assert np.array_equal(dist.view(np.uint32), sweep_models[11].dist.view(np.uint32))


# ---- beside the rest of the library ---------------------------------------------------------------------------------------------
def test_agrees_with_the_existing_nearest_neighbor_search(torch_cuda):
    map_pts, queries, _ = A.scene()
    c = _fresh()
    try:
        c.map_set(map_pts)
        _, _, nn = c.nearest_neighbor_search(queries, with_normals=False, with_index=True)
        dist, index = _query(c, queries, 1)
        assert np.array_equal(index[:, 0], nn)
        near = (map_pts[nn].astype(np.float64) - queries.astype(np.float64))    # (and the distance is that neighbour's)
        assert A.ulp_error(dist[:, 0], np.sqrt((near ** 2).sum(axis=1))).max() <= A.DIST_BAR_ULP
    finally:
        c.close()


def _two_registrations(with_query):
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    import icp_oracle as O
    scans, _ = make_sequence(SceneConfig(height=16, width=256), 3)
    clouds = [np.ascontiguousarray(O.grid_sample(s, 0.4)[0].astype(np.float32)) for s in scans]
    c = _fresh(max_num_alignments=8)
    try:
        c.map_set(clouds[0])
        out = []
        r = c.register(clouds[1])
        out.append((r.pose.copy(), np.asarray(r.losses).copy(), int(r.iterations)))
        if with_query:
            for k in (1, 11, 32):
                dist, index = _query(c, clouds[2], k)
                A.check_bits(dist, index, A.model_knn(clouds[0], clouds[2], k), f"between two registrations, k = {k}")
        r = c.register(clouds[2], init_pose=out[0][0])
        out.append((r.pose.copy(), np.asarray(r.losses).copy(), int(r.iterations)))
        return out
    finally:
        c.close()


def test_a_query_leaves_the_registration_state_alone(torch_cuda):
    plain, queried = _two_registrations(False), _two_registrations(True)
    for (p0, l0, i0), (p1, l1, i1) in zip(plain, queried):
        assert i0 == i1 and i0 >= 1
        assert np.array_equal(np.asarray(p0).view(np.uint8), np.asarray(p1).view(np.uint8))
        assert np.array_equal(l0.view(np.uint8), l1.view(np.uint8))


def test_indices_follow_the_map_through_updates(torch_cuda, mixed_queries):
    _, queries, sampled = A.scene()
    clouds = [np.ascontiguousarray(sampled[a:a + 1500]) for a in (0, 1500, 3000)]
    pose = np.eye(4, dtype=np.float32)
    pose[:3, 3] = (0.4, -0.1, 0.02)
    pose[:2, :2] = ((np.cos(0.02), -np.sin(0.02)), (np.sin(0.02), np.cos(0.02)))
    q = mixed_queries[:300]
    c = _fresh(local_map_size=2)
    try:
        c.map_init()
        c.map_update(np.eye(4, dtype=np.float32), clouds[0])
        c.map_update(pose, clouds[1])                              # an insertion: the kept points move, the new ones follow them
        held = c.map_points()
        assert held.shape == (3000, 3) and np.array_equal(held[1500:], clouds[1]) and not np.array_equal(held[:1500], clouds[0])
        dist, index = _query(c, q, 11)
        A.check_bits(dist, index, A.model_knn(held, q, 11), "after an insertion")
        c.map_update(pose, clouds[2])                              # ... and an eviction: the first cloud leaves, indices shift down
        held = c.map_points()
        assert held.shape == (3000, 3) and np.array_equal(held[1500:], clouds[2])
        dist, index = _query(c, q, 11)
        A.check_bits(dist, index, A.model_knn(held, q, 11), "after an eviction")
    finally:
        c.close()


def test_refusals_leave_the_context_working(torch_cuda, mixed_queries):
    _, queries, sampled = A.scene()
    q = mixed_queries[:64]
    c = _fresh(max_num_alignments=4)
    try:
        with pytest.raises(RuntimeError, match="empty"):
            c.knn_query(q, k=1)
        c.map_set(sampled)
        for k in (0, 33, -1):
            with pytest.raises(AssertionError, match="outside 1..32"):
                c.knn_query(q, k=k)
        with pytest.raises(AssertionError, match="distance"):
            c.knn_query(q, k=1, distance_upper_bound=-1.0)
        with pytest.raises(AssertionError, match=r"\[n, 3\]"):
            c.knn_query(np.zeros((4, 2), np.float32), k=1)
        c.register_launch(queries[:2000])
        with pytest.raises(AssertionError, match="registration in progress"):
            c.knn_query(q, k=1)
        r = c.register_end()
        assert r.iterations >= 1
        dist, index = _query(c, q, 11)
        A.check_bits(dist, index, A.model_knn(sampled, q, 11), "after the refusals")
    finally:
        c.close()


# ---- the drop-in class -----------------------------------------------------------------------------------------------------------
def test_kdtree_on_the_device(torch_cuda, mixed_queries, sweep_models):
    from pylidar_slam_amd.kdtree import KDTree
    sampled = A.scene()[2]
    tree = KDTree(sampled)                                        # (a private context)
    assert (tree.n, tree.ndim) == (6471, 3)
    d1, i1 = tree.query(mixed_queries)
    assert d1.shape == (1024,) and i1.shape == (1024,) and d1.dtype == np.float32 and i1.dtype == np.uint32
    A.check_bits(d1.reshape(-1, 1), i1.astype(np.int32).reshape(-1, 1), sweep_models[1], "KDTree.query, k = 1")
    d, i = tree.query(mixed_queries, k=11)
    assert d.shape == (1024, 11) and i.dtype == np.uint32
    A.check_bits(d, i.astype(np.int32), sweep_models[11], "KDTree.query, k = 11")
    with pytest.raises(ValueError, match="eps"):
        tree.query(mixed_queries, eps=0.5)
    tree._ctx.close()
    tree._private = False
