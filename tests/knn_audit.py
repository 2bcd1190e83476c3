"""The model the k-NN query is held to (csrc/knn.hip: k_knn_query; icp_knn_query, IcpContext.knn_query,
pylidar_slam_amd.kdtree.KDTree), the clouds it is audited on and the comparison helpers.  TEST INFRASTRUCTURE, never
imported by the package.

`model_knn` is a float32 brute force: for every (query, map point) pair the kernel's own d2,
    dx = m.x - q.x, ...  (float32);   d2 = fma(dz, dz, fma(dy, dy, dx * dx)),
ordered by the 64-bit key (bits of d2, original map index): ascending distance, exact ties to the lower index.  A bound b
keeps d2 < float32(b) * float32(b), strictly.  Entries without a neighbour are (+inf, M).  A query row with a non-finite
coordinate has no neighbours.  The kernel is held to it BIT FOR BIT, distances and indices.

fma.  numpy has no fused multiply-add.  `a * a` of a float32 is exact in float64 (48 significant bits), so
float32(float64(a) * float64(a) + float64(c)) differs from fmaf(a, a, c) only by double rounding: the float64 sum is
itself rounded, and where it lands within one float64 ulp of the middle between two float32 values the second rounding may
go the other way.  (Where the float64 sum is exact — its TwoSum error term is zero, as for the short mantissas of the synthetic
scenes' planes — there is one rounding only, to nearest even like fmaf's, a sum exactly on the middle included.)  Those
candidates are flagged; a ROW is flagged when a flagged candidate is close enough to matter (at or
below the k-th key's distance, or the bound, plus one float32 ulp).  The clouds here are chosen so that no row is; the CPU
suite asserts at most FLAGGED_MAX per case, comparisons leave flagged rows out.

The bar of the model against a float64 truth (`DIST_BAR_ULP`), from the rounding steps, u = 2^-24, first order, all terms
non-negative so relative errors do not amplify:
    dx, dy, dz      one rounding each                          -> (1 + u) each, (1 + 2u) on a square
    dx * dx         product rounding                           -> 3u on the dx^2 term
    fma(dy, dy, .)  one rounding of the sum                    -> dx^2 term 4u, dy^2 term 3u
    fma(dz, dz, .)  one rounding of the sum                    -> dx^2 term 5u, dy^2 term 4u, dz^2 term 3u:  d2 within 5u
    sqrtf           halves the relative error, rounds once     -> 2.5u + u = 3.5u relative
A relative error of u is at most one float32 ulp (ulp(x) >= 2^-24 x), so the distance is within 3.5 ulp of the truth
rounded to nearest; 4 with the second-order terms and the truth's own rounding to float32 for the spacing.  Squared
distances: 5u -> 5 ulp, bar 5.5.
"""
import numpy as np

F32 = np.float32
DIST_BAR_ULP = 4.0
SQR_BAR_ULP = 5.5
FLAGGED_MAX = 1.0e-3     # share of a case's rows the model may flag
AMBIGUOUS_MAX = 1.0e-2   # share of a case's rows whose truth has two neighbours closer than AMBIGUOUS_REL to each other
AMBIGUOUS_REL = 1.0e-6
KS = (1, 2, 11, 16, 32)  # the audited k of the large fixture
MAX_K = 32


class Knn:
    """dist [n, k] float32, index [n, k] int32, flagged [n] bool"""

    def __init__(self, dist, index, flagged):
        self.dist, self.index, self.flagged = dist, index, flagged


# ---- the model ---------------------------------------------------------------------------------------------------------
def _near_f32_midpoint(s64):
    """a non-negative float64 within one float64 ulp of the middle between two float32 values: the 29 mantissa bits a float32
    drops read 0x0fffffff, 0x10000000 or 0x10000001 (below the float32 normal range the dropped bits are others: every such
    sum counts as near)"""
    low = s64.view(np.uint64) & np.uint64(0x1FFFFFFF)
    return ((low - np.uint64(0x0FFFFFFF)) <= np.uint64(2)) | ((s64 > 0.0) & (s64 < 2.0 ** -126))


def _fma_sq(a32, c32):
    """fmaf(a, a, c) for float32 arrays, and where double rounding cannot be excluded"""
    a64 = a32.astype(np.float64)
    p64, c64 = a64 * a64, c32.astype(np.float64)
    s64 = p64 + c64
    unsure = _near_f32_midpoint(s64) & np.isfinite(s64)
    at = np.nonzero(unsure)
    if at[0].size:  # (the error term of the float64 sum, Knuth's TwoSum: zero = the sum is exact, one rounding only)
        p, c, t = p64[at], c64[at], s64[at]
        v = t - p
        unsure[at] = ((p - (t - v)) + (c - v)) != 0.0
    with np.errstate(over="ignore"):
        return s64.astype(F32), unsure


def model_d2(map_pts, queries):
    """d2 [n, M] float32 as point_key computes it, and the candidates whose fma emulation is not certain"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = map_pts[None, :, 0] - queries[:, None, 0]
        dy = map_pts[None, :, 1] - queries[:, None, 1]
        dz = map_pts[None, :, 2] - queries[:, None, 2]
        s, f1 = _fma_sq(dy, dx * dx)
        d2, f2 = _fma_sq(dz, s)
    return d2, f1 | f2


def _top_rows(d2, k):
    """indices [n, k] of the k smallest (d2, index) keys of every row (k <= M)"""
    n, m = d2.shape
    if m <= 2048:
        return np.argsort(d2, axis=1, kind="stable")[:, :k]
    kk = min(m, k + 16)
    part = np.argpartition(d2, kk - 1, axis=1)[:, :kk]
    part.sort(axis=1)                                     # ascending index: a stable sort by d2 is then the key order
    pd = np.take_along_axis(d2, part, axis=1)
    order = np.argsort(pd, axis=1, kind="stable")
    top = np.take_along_axis(part, order, axis=1)[:, :k]
    # a tie that reaches from the k-th key to the edge of the partition may hide a lower index outside it: sort those rows whole
    pds = np.take_along_axis(pd, order, axis=1)
    if kk < m:
        for r in np.flatnonzero(pds[:, k - 1] == pds[:, kk - 1]):
            top[r] = np.argsort(d2[r], kind="stable")[:k]
    return top


def model_knn_multi(map_pts, queries, ks, bound=None, sqr=False, inclusive_bound=False, chunk=128):
    """{k: Knn} for every k of `ks` from ONE evaluation of the distances.  `inclusive_bound`: the wrong copy that keeps a
    point exactly at the bound."""
    map_pts, queries = np.asarray(map_pts), np.asarray(queries)
    assert map_pts.dtype == F32 and queries.dtype == F32 and map_pts.shape[1] == 3 and queries.shape[1] == 3
    m, n = map_pts.shape[0], queries.shape[0]
    b2 = F32(np.inf)
    if bound is not None and bound > 0 and np.isfinite(bound):
        with np.errstate(over="ignore"):
            b2 = F32(bound) * F32(bound)
    out = {k: Knn(np.full((n, k), np.inf, F32), np.full((n, k), m, np.int32), np.zeros(n, bool)) for k in ks}
    kmax = max(ks)
    for lo in range(0, n, chunk):
        q = queries[lo:lo + chunk]
        d2, unsure = model_d2(map_pts, q)
        with np.errstate(invalid="ignore"):
            keep = (d2 <= b2) if inclusive_bound else (d2 < b2)   # (+inf and NaN are never below the bound)
            keep &= np.isfinite(d2)
        d2k = np.where(keep, d2, F32(np.inf))
        kk = min(kmax, m)
        top = _top_rows(d2k, kk)
        td = np.take_along_axis(d2k, top, axis=1)
        for k in ks:
            r = out[k]
            c = min(k, m)
            found = np.isfinite(td[:, :c])
            with np.errstate(invalid="ignore"):
                r.dist[lo:lo + chunk, :c] = np.where(found, td[:, :c] if sqr else np.sqrt(td[:, :c]), F32(np.inf))
            r.index[lo:lo + chunk, :c] = np.where(found, top[:, :c], m)
            # a row is flagged when an unsure candidate could enter or leave its list: at or below the k-th distance (the bound
            # where the list is not full), one float32 ulp allowed for
            kth = td[:, c - 1] if c == k else np.full(q.shape[0], np.inf, F32)
            limit = np.where(np.isfinite(kth), kth, b2)
            with np.errstate(invalid="ignore", over="ignore"):
                limit = np.nextafter(limit, F32(np.inf))
                r.flagged[lo:lo + chunk] = np.any(unsure & (d2 <= limit[:, None]), axis=1)
    return out


def model_knn(map_pts, queries, k, bound=None, sqr=False, inclusive_bound=False):
    return model_knn_multi(map_pts, queries, (k,), bound, sqr, inclusive_bound)[k]


# ---- the float64 truth -------------------------------------------------------------------------------------------------
def truth_knn(map_pts, queries, k):
    """(dist [n, k] float64, index [n, k]) of the finite queries against float64 copies: cKDTree, or brute force for a tiny
    map; entries beyond the map are (inf, M)"""
    m = map_pts.shape[0]
    m64, q64 = map_pts.astype(np.float64), queries.astype(np.float64)
    if m <= 64:
        d = np.sqrt(((m64[None] - q64[:, None]) ** 2).sum(axis=2))
        idx = np.argsort(d, axis=1, kind="stable")[:, :k]
        dist = np.take_along_axis(d, idx, axis=1)
        if k > m:
            dist = np.concatenate((dist, np.full((q64.shape[0], k - m), np.inf)), axis=1)
            idx = np.concatenate((idx, np.full((q64.shape[0], k - m), m)), axis=1)
        return dist, idx
    from scipy.spatial import cKDTree
    dist, idx = cKDTree(m64).query(q64, k=k)
    return dist.reshape(-1, k), idx.reshape(-1, k)


def ambiguous_rows(truth_dist):
    """rows in which two consecutive distances of the truth's list (hand it k + 1 columns) are closer than AMBIGUOUS_REL"""
    t = np.asarray(truth_dist, np.float64)
    if t.shape[1] < 2:
        return np.zeros(t.shape[0], bool)
    a, b = t[:, :-1], t[:, 1:]
    with np.errstate(invalid="ignore"):
        close = (b - a) < AMBIGUOUS_REL * b
    return np.any(close & np.isfinite(b), axis=1)


def ulp_error(got, truth):
    """|got - truth| in float32 ulps of the truth, per entry (both inf: 0)"""
    got, truth = np.asarray(got, np.float64), np.asarray(truth, np.float64)
    both_inf = np.isinf(got) & np.isinf(truth)
    with np.errstate(invalid="ignore", over="ignore"):
        sp = np.spacing(np.abs(truth).astype(F32)).astype(np.float64)
        e = np.abs(got - truth) / sp
    e[both_inf] = 0.0
    e[np.isnan(e)] = np.inf
    return e


# ---- comparison helpers ------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_bits(dist, index, want, what="", rows=None):
    """`dist` / `index` (either may be None) against the model, bit for bit on every unflagged row (of `rows`, when given)"""
    use = ~want.flagged
    if rows is not None:
        sel = np.zeros_like(use)
        sel[rows] = True
        use &= sel
    if dist is not None:
        dist = np.asarray(dist)
        assert dist.dtype == np.float32 and dist.shape == want.dist.shape, (what, dist.dtype, dist.shape, want.dist.shape)
        bad = np.flatnonzero(np.any(_bits(dist) != _bits(want.dist), axis=1) & use)
        assert bad.size == 0, (f"{what}: the distances of {bad.size} of {int(use.sum())} rows differ from the model, first row "
                               f"{bad[0]}: {dist[bad[0]].tolist()} against {want.dist[bad[0]].tolist()}")
    if index is not None:
        index = np.asarray(index)
        assert index.dtype == np.int32 and index.shape == want.index.shape, (what, index.dtype, index.shape, want.index.shape)
        bad = np.flatnonzero(np.any(index != want.index, axis=1) & use)
        assert bad.size == 0, (f"{what}: the indices of {bad.size} of {int(use.sum())} rows differ from the model, first row "
                               f"{bad[0]}: {index[bad[0]].tolist()} against {want.index[bad[0]].tolist()}")


def check_key_order(map_pts, queries, got, what=""):
    """the lists equal np.lexsort((index, d2)) of the model's distances exactly (ties: lattice, duplicated points)"""
    d2, _ = model_d2(map_pts, queries)
    k = got.index.shape[1]
    for r in range(queries.shape[0]):
        order = np.lexsort((np.arange(d2.shape[1]), d2[r]))[:k]
        assert np.array_equal(got.index[r, :order.size], order), (what, r, got.index[r].tolist(), order.tolist())
        assert np.array_equal(_bits(got.dist[r, :order.size]), _bits(np.sqrt(d2[r, order]))), (what, r)


# ---- clouds ------------------------------------------------------------------------------------------------------------
_CACHE = {}


def scene():
    """(map [24 576, 3], queries [8 192, 3], sampled map [6 471, 3]): the valid rows of the first three 32 x 256 scans of the
    seeded synthetic sequence, those of the fourth, and the 0.4 m grid sample of the map"""
    if "scene" not in _CACHE:
        import icp_oracle as O
        from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
        scans, _ = make_sequence(SceneConfig(height=32, width=256), 4)

        def valid(s):
            s = np.asarray(s, F32).reshape(-1, 3)
            return s[np.isfinite(s).all(axis=1) & (np.abs(s).max(axis=1) > 0)]

        map_pts = np.ascontiguousarray(np.concatenate([valid(s) for s in scans[:3]]))
        queries = np.ascontiguousarray(valid(scans[3]))
        sampled = np.ascontiguousarray(O.grid_sample(map_pts, 0.4)[0].astype(F32))
        assert map_pts.shape == (24576, 3) and queries.shape == (8192, 3) and sampled.shape == (6471, 3)
        for a in (map_pts, queries, sampled):
            a.setflags(write=False)
        _CACHE["scene"] = (map_pts, queries, sampled)
    return _CACHE["scene"]


def lattice():
    """(map, queries): the 7 x 7 x 7 integer lattice at spacing 1, queried at its points and at the centres of its cells —
    every distance is exact in float32, so the ties are exact"""
    g = np.arange(7, dtype=F32) - F32(3.0)
    map_pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    c = np.arange(6, dtype=F32) - F32(2.5)
    centres = np.stack(np.meshgrid(c, c, c, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(map_pts), np.ascontiguousarray(np.concatenate((map_pts, centres)))


def duplicated():
    """(map, queries): 600 points of the sampled map, each one twice in a row; queried from the fourth scan"""
    map_pts, queries, sampled = scene()
    return np.ascontiguousarray(np.repeat(sampled[::10][:600], 2, axis=0)), np.ascontiguousarray(queries[::16])
