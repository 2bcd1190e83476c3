// Exact k nearest map points of arbitrary query points against the context's hash grid: the seam of
// pykdtree.kdtree.KDTree.query (slam/odometry/local_map.py:369,385,405).  gfx950 only.
//
// A query is shared by NL lanes (4: a quad; 1: one lane).  Every lane keeps the k smallest (d2, original index) keys of ITS
// share of the candidates in registers (TopK<KN>: compile-time indices only), the lanes' lists are merged at the end of a
// ring by DPP (merge_group), and the search goes fine rings -> coarse level -> exhaustive scan under knn_level's exactness
// rule, as knn_rings does for the map points of the kNN normals.  No distance cap: the answer is the mathematical one for
// the float32 d2 of point_key, ties broken by the lower original index.
//
// Distance bound and missing entries.  The lists do not start at KEY_EMPTY but at a SENTINEL key (b2, index 0), b2 = the
// squared bound (+inf: none).  TopK::insert takes a key only below the list's last one, so
//   - a candidate with d2 >= b2 is never taken (the bound is strict; (b2, 0) itself is refused: not below the sentinel),
//   - a candidate whose d2 is +inf or NaN (a non-finite query) is never taken either: without a bound b2 = +inf,
//   - kth() starts at b2: the ring tests prune with the bound, and the exactness rule settles a query as soon as its rings
//     pass the bound — it never reaches the coarse level or the exhaustive scan for neighbours it could not keep.
// Whatever is still >= the sentinel at the end is a missing entry: dist = +inf, index = M.
#include "icp_internal.h"
#include "knn_device.h"
#include "knn_plan.h"
#include "search_device.h"

namespace icp {

static constexpr int KNN_THREADS = 256;

template <int KN>
__device__ inline void knn_fill(TopK<KN>& t, unsigned long long v) {
#pragma unroll
    for (int k = 0; k < KN; ++k) t.key[k] = v;
}

// a cell's candidates start + sub, start + sub + NL, ...: four independent 16-byte loads in flight (estimate_cov's own-cell
// loop).  `cap`: the last key of the merged list of the rings before — a key at or above it cannot enter the merged list
template <int KN, int NL>
__device__ inline void scan_cell_share(const GridView& g, int start, int count, int sub, float px, float py, float pz,
                                       unsigned long long cap, TopK<KN>& t) {
    const int last = start + count - 1;
    for (int k = start + sub; k <= last; k += 4 * NL) {
        const bool v1 = k + NL <= last, v2 = k + 2 * NL <= last, v3 = k + 3 * NL <= last;
        const float4 q0 = g.pts[k], q1 = g.pts[v1 ? k + NL : k], q2 = g.pts[v2 ? k + 2 * NL : k],
                     q3 = g.pts[v3 ? k + 3 * NL : k];
        const unsigned long long k0 = point_key(q0, px, py, pz), k1 = point_key(q1, px, py, pz),
                                 k2 = point_key(q2, px, py, pz), k3 = point_key(q3, px, py, pz);
        if (k0 < cap) t.insert(k0);
        if (v1 && k1 < cap) t.insert(k1);
        if (v2 && k2 < cap) t.insert(k2);
        if (v3 && k3 < cap) t.insert(k3);
    }
}

// the lanes' lists -> m (the same in all lanes); then lane 0 goes on from m and the others from empty lists
template <int KN, int NL>
__device__ inline void knn_merge_share(TopK<KN>& t, TopK<KN>& m, int sub, unsigned long long sentinel) {
    merge_group<KN, NL>(t, m);
#pragma unroll
    for (int k = 0; k < KN; ++k) t.key[k] = sub == 0 ? m.key[k] : sentinel;
}

// knn_level for NL lanes per query.  m: the merged list (in: all sentinel; out: the k smallest keys of the rings visited);
// true when it is provably exact.  The cell tests prune with the smaller of the lane's own k-th distance and the merged
// list's: both are upper bounds of the final k-th distance.  The ring loop is uniform in the group (its condition comes from
// m), so all NL lanes meet at every merge.
template <int KN, int NL>
__device__ inline bool knn_level_share(const GridView& g, float px, float py, float pz, int max_rings, int sub,
                                       unsigned long long sentinel, TopK<KN>& m) {
    if constexpr (NL == 1) return knn_level<KN>(g, px, py, pz, 0, max_rings, false, m);
    const int cx = cell_coord(px, g.inv_h), cy = cell_coord(py, g.inv_h), cz = cell_coord(pz, g.inv_h);
    const float h = g.h;
    const float hs = slack_h(h);
    const CellOff fx = cell_off(px, cx, h);
    const CellOff fy = cell_off(py, cy, h);
    const CellOff fz = cell_off(pz, cz, h);
    const float edge = cell_edge(fx, fy, fz);
    TopK<KN> t;
    knn_fill<KN>(t, sentinel);
    int start, count;
    if (grid_lookup(g, cx, cy, cz, start, count))
        scan_cell_share<KN, NL>(g, start, count, sub, px, py, pz, sentinel, t);
    bool exact = false;
    for (int r = 1; r <= max_rings && !exact; ++r) {
        const unsigned long long cap = m.key[KN - 1];
        const float capd = key_d2(cap);
        for (int oz = -r; oz <= r; ++oz) {
            const float gz = axis_gap(oz, fz, hs);
            const float gz2 = gz * gz;
            if (gz2 > fminf(t.kth(), capd)) continue;
            const int az = oz < 0 ? -oz : oz;
            for (int oy = -r; oy <= r; ++oy) {
                const float gy = axis_gap(oy, fy, hs);
                const float gyz2 = fmaf(gy, gy, gz2);
                if (gyz2 > fminf(t.kth(), capd)) continue;
                const int ay = oy < 0 ? -oy : oy;
                const int step = ((az == r) || (ay == r)) ? 1 : 2 * r;
                for (int ox = -r; ox <= r; ox += step) {
                    const float gx = axis_gap(ox, fx, hs);
                    if (fmaf(gx, gx, gyz2) > fminf(t.kth(), capd)) continue;
                    if (grid_lookup(g, cx + ox, cy + oy, cz + oz, start, count))
                        scan_cell_share<KN, NL>(g, start, count, sub, px, py, pz, cap, t);
                }
            }
        }
        knn_merge_share<KN, NL>(t, m, sub, sentinel);
        const float bound = ring_bound(r, hs, edge);
        exact = m.kth() <= bound * bound * 0.999999f;
    }
    return exact;
}

// Block = KNN_THREADS / NL queries x NL lanes.  xyz [n,3]; dist / index [n,k] (either may be null); k <= KN: the first k
// entries of the KN-list (both are exact).  b2: the squared distance bound, +inf without one.
template <int KN, int NL>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_query(GridView g, const float* __restrict__ xyz, int n, int k,
                                                           int max_rings, float b2, int sqr_dists,
                                                           float* __restrict__ dist, int* __restrict__ index) {
    const long long gid = (long long)blockIdx.x * KNN_THREADS + threadIdx.x;
    const long long q = gid / NL;
    const int sub = (int)(threadIdx.x & (NL - 1));
    if (q >= n) return;  // (whole groups: KNN_THREADS is a multiple of NL)
    const float px = xyz[q * 3], py = xyz[q * 3 + 1], pz = xyz[q * 3 + 2];
    const unsigned long long sentinel = make_key(b2, 0);
    TopK<KN> m;
    knn_fill<KN>(m, sentinel);
    // a non-finite coordinate makes every d2 +inf or NaN: no key would pass the sentinel and the search would run to the end
    // of the exhaustive scan to find that out.  The row's k entries are missing; the branch is uniform in the group
    const bool finite = fabsf(px) < INFINITY && fabsf(py) < INFINITY && fabsf(pz) < INFINITY;
    if (finite) {
        bool exact = knn_level_share<KN, NL>(g, px, py, pz, max_rings, sub, sentinel, m);
        if (!exact && g.ctable) {
            knn_fill<KN>(m, sentinel);
            exact = knn_level_share<KN, NL>(coarse_view(g), px, py, pz, COARSE_RINGS, sub, sentinel, m);
        }
        if (!exact) {
            knn_fill<KN>(m, sentinel);
            if constexpr (NL == 1) {
                scan_cell_knn<KN>(g, 0, g.m, px, py, pz, m);
            } else {
                TopK<KN> t;
                knn_fill<KN>(t, sentinel);
                scan_cell_share<KN, NL>(g, 0, g.m, sub, px, py, pz, sentinel, t);
                merge_group<KN, NL>(t, m);
            }
        }
    }
    const size_t row = (size_t)q * (size_t)k;
#pragma unroll
    for (int j = 0; j < KN; ++j) {
        if (j >= k || (j & (NL - 1)) != sub) continue;
        const unsigned long long key = m.key[j];
        const bool missing = !(key < sentinel);
        const float d2 = key_d2(key);
        if (dist) dist[row + j] = missing ? INFINITY : (sqr_dists ? d2 : sqrtf(d2));
        if (index) index[row + j] = missing ? g.m : key_idx(key);
    }
}

template <int KN, int NL>
static void launch_knn_t(icp_ctx* ctx, const float* xyz, int n, int k, float b2, int sqr_dists, float* dist, int32_t* index) {
    const long long threads = (long long)n * NL;
    hipLaunchKernelGGL((k_knn_query<KN, NL>), dim3((unsigned)((threads + KNN_THREADS - 1) / KNN_THREADS)), dim3(KNN_THREADS),
                       0, ctx->stream, grid_view(ctx), xyz, n, k, knn_fine_rings(ctx), b2, sqr_dists, dist, index);
}

// the instantiation a k runs on: the next compiled list length (a longer exact list begins with the shorter one)
int launch_knn_query(icp_ctx* ctx, const float* xyz, int64_t n, int k, float b2, int sqr_dists, float* dist_out,
                     int32_t* index_out) {
    if (n <= 0) return ICP_OK;
    const int nn = (int)n;
    switch (knn_list_length(k)) {
#define ICP_KNN_CASE(KN, NL) \
    case KN: launch_knn_t<KN, NL>(ctx, xyz, nn, k, b2, sqr_dists, dist_out, index_out); break;
        ICP_KNN_CASE(1, 4)
        ICP_KNN_CASE(2, 4)
        ICP_KNN_CASE(4, 4)
        ICP_KNN_CASE(8, 4)
        ICP_KNN_CASE(11, 4)
        ICP_KNN_CASE(16, 4)
        ICP_KNN_CASE(32, 4)
#undef ICP_KNN_CASE
        default: return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_knn_query: k is outside 1..32");
    }
    ICP_HIP(ctx, hipGetLastError());
    return ICP_OK;
}

}  // namespace icp
