// Device-side building blocks of the exact k-nearest-neighbour searches: the 64-bit (distance, index) keys, the sorted
// per-lane lists, the ring search over the hash grid and the merge of the lanes' lists.  Shared by the kNN normals
// (search.hip) and the k-NN query for arbitrary points (knn.hip).
#pragma once
#include "icp_internal.h"
#include "search_device.h"

namespace icp {

// k smallest (distance, original index) pairs as 64-bit keys (d2 bits << 32 | index): d2 >= 0, so the float bits order
// like the values and one unsigned 64-bit compare gives the lexicographic (distance, index) order the search breaks
// ties with.  Sorted ascending; a compare-swap step is 1 compare + 4 selects.
static constexpr unsigned long long KEY_EMPTY = (0x7f800000ull << 32) | 0x7fffffffull;  // (+inf, max index)

__device__ inline unsigned long long make_key(float d2, int idx) {
    return ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(unsigned)idx;
}
__device__ inline float key_d2(unsigned long long k) { return __uint_as_float((unsigned)(k >> 32)); }
__device__ inline int key_idx(unsigned long long k) { return (int)(unsigned)(k & 0xffffffffull); }

__device__ inline unsigned long long point_key(const float4 q, float px, float py, float pz) {
    const float dx = q.x - px, dy = q.y - py, dz = q.z - pz;
    return make_key(fmaf(dz, dz, fmaf(dy, dy, dx * dx)), __float_as_int(q.w));
}

template <int KN>
struct TopK {
    unsigned long long key[KN];
    __device__ inline void init() {
#pragma unroll
        for (int k = 0; k < KN; ++k) key[k] = KEY_EMPTY;
    }
    __device__ inline float kth() const { return key_d2(key[KN - 1]); }
    __device__ inline void insert(unsigned long long c) {
        if (!(c < key[KN - 1])) return;
        key[KN - 1] = c;
#pragma unroll
        for (int k = KN - 1; k > 0; --k) {
            const unsigned long long lo = key[k] < key[k - 1] ? key[k] : key[k - 1];
            const unsigned long long hi = key[k] < key[k - 1] ? key[k - 1] : key[k];
            key[k - 1] = lo;
            key[k] = hi;
        }
    }
};

template <int KN>
__device__ inline void scan_cell_knn(const GridView& g, int start, int count, float px, float py, float pz,
                                     TopK<KN>& t) {
    const int last = start + count - 1;
    for (int k = start; k <= last; k += 4) {
        const int k1 = min(k + 1, last), k2 = min(k + 2, last), k3 = min(k + 3, last);
        const float4 q0 = g.pts[k], q1 = g.pts[k1], q2 = g.pts[k2], q3 = g.pts[k3];
        t.insert(point_key(q0, px, py, pz));
        if (k1 != k) t.insert(point_key(q1, px, py, pz));
        if (k2 != k1) t.insert(point_key(q2, px, py, pz));
        if (k3 != k2) t.insert(point_key(q3, px, py, pz));
    }
}

// hashed ring search on one level from ring `first_ring` on (rings below it were already visited by the caller);
// true when the k-th neighbour is provably exact
template <int KN>
__device__ inline bool knn_level(const GridView& g, float px, float py, float pz, int first_ring, int max_rings,
                                 bool translate, TopK<KN>& t) {
    const int cx = cell_coord(px, g.inv_h), cy = cell_coord(py, g.inv_h), cz = cell_coord(pz, g.inv_h);
    const float h = g.h;
    const float hs = slack_h(h);
    const CellOff fx = cell_off(px, cx, h);
    const CellOff fy = cell_off(py, cy, h);
    const CellOff fz = cell_off(pz, cz, h);
    const float edge = cell_edge(fx, fy, fz);
    int start, count;
    if (first_ring == 0 && grid_lookup(g, cx, cy, cz, start, count)) scan_cell_knn<KN>(g, start, count, px, py, pz, t);
    bool exact = false;
    for (int r = first_ring < 1 ? 1 : first_ring; r <= max_rings && !exact; ++r) {
        for (int oz = -r; oz <= r; ++oz) {
            const float gz = axis_gap(oz, fz, hs);
            const float gz2 = gz * gz;
            if (gz2 > t.kth()) continue;
            const int az = oz < 0 ? -oz : oz;
            for (int oy = -r; oy <= r; ++oy) {
                const float gy = axis_gap(oy, fy, hs);
                const float gyz2 = fmaf(gy, gy, gz2);
                if (gyz2 > t.kth()) continue;
                const int ay = oy < 0 ? -oy : oy;
                const int step = ((az == r) || (ay == r)) ? 1 : 2 * r;
                for (int ox = -r; ox <= r; ox += step) {
                    const float gx = axis_gap(ox, fx, hs);
                    if (fmaf(gx, gx, gyz2) > t.kth()) continue;
                    if (grid_lookup(g, cx + ox, cy + oy, cz + oz, start, count))
                        scan_cell_knn<KN>(g, start, count, px, py, pz, t);
                }
            }
        }
        const float bound = ring_bound(r, hs, edge);
        exact = t.kth() <= bound * bound * 0.999999f;
    }
    (void)translate;  // keys carry original indices: nothing to translate between levels
    return exact;
}

// continuation after the fine ring 1 (rows): fine ring 2.., then the coarse level, then the exhaustive scan
template <int KN>
__device__ inline void knn_rings(const GridView& g, float px, float py, float pz, int first_ring, int max_rings,
                                 TopK<KN>& t) {
    if (knn_level<KN>(g, px, py, pz, first_ring, max_rings, false, t)) return;
    if (g.ctable) {
        t.init();
        if (knn_level<KN>(coarse_view(g), px, py, pz, 0, COARSE_RINGS, true, t)) return;
    }
    t.init();
    scan_cell_knn<KN>(g, 0, g.m, px, py, pz, t);
}

// merge of the NL lanes' sorted lists: k rounds of "group-min of the heads, the winner pops" (t is consumed)
template <int KN, int NL>
__device__ inline void merge_group(TopK<KN>& t, TopK<KN>& m) {
#pragma unroll
    for (int round = 0; round < KN; ++round) {
        unsigned long long best = t.key[0];
        if (NL == 16) {  // a row of 16 lanes: DPP (search_device.h::row16_step)
            unsigned long long other = row16_step<0>(best);
            best = other < best ? other : best;
            other = row16_step<1>(best);
            best = other < best ? other : best;
            other = row16_step<2>(best);
            best = other < best ? other : best;
            other = row16_step<3>(best);
            best = other < best ? other : best;
        } else if (NL == 64) {
            // a whole wave (round 6): the minimum of every row of 16 by DPP, then the four rows' minima read into scalar
            // registers (v_readlane) — 4 x 5 + 8 + 9 VALU instructions where six __shfl_xor steps of a 64-bit key were twelve
            // ds_bpermute round trips through the LDS crossbar (~800 cycles per round, eleven rounds per merge, two or three
            // merges per straggler of the kNN normals).  Every lane of the wave must be active.
            unsigned long long other = row16_step<0>(best);
            best = other < best ? other : best;
            other = row16_step<1>(best);
            best = other < best ? other : best;
            other = row16_step<2>(best);
            best = other < best ? other : best;
            other = row16_step<3>(best);
            best = other < best ? other : best;
            const unsigned blo = (unsigned)(best & 0xffffffffull), bhi = (unsigned)(best >> 32);
            unsigned long long r0 = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)bhi, 0) << 32) |
                                    (unsigned)__builtin_amdgcn_readlane((int)blo, 0);
            const unsigned long long r1 = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)bhi, 16) << 32) |
                                          (unsigned)__builtin_amdgcn_readlane((int)blo, 16);
            const unsigned long long r2 = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)bhi, 32) << 32) |
                                          (unsigned)__builtin_amdgcn_readlane((int)blo, 32);
            const unsigned long long r3 = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)bhi, 48) << 32) |
                                          (unsigned)__builtin_amdgcn_readlane((int)blo, 48);
            r0 = r1 < r0 ? r1 : r0;
            const unsigned long long r23 = r3 < r2 ? r3 : r2;
            best = r23 < r0 ? r23 : r0;
        } else if (NL > 4) {  // (other group sizes: the LDS crossbar)
#pragma unroll
            for (int o = 1; o < NL; o <<= 1) {
                const unsigned lo = __shfl_xor((unsigned)(best & 0xffffffffull), o, 64);
                const unsigned hi = __shfl_xor((unsigned)(best >> 32), o, 64);
                const unsigned long long other = ((unsigned long long)hi << 32) | lo;
                best = other < best ? other : best;
            }
        } else {
            const unsigned lo = (unsigned)quad_xor<1>((int)(best & 0xffffffffull));
            const unsigned hi = (unsigned)quad_xor<1>((int)(best >> 32));
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            best = other < best ? other : best;
        }
        if (NL == 4) {
            const unsigned lo = (unsigned)quad_xor<2>((int)(best & 0xffffffffull));
            const unsigned hi = (unsigned)quad_xor<2>((int)(best >> 32));
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            best = other < best ? other : best;
        }
        m.key[round] = best;
        const bool won = (t.key[0] == best) && (best != KEY_EMPTY);  // original indices are unique: one winner
#pragma unroll
        for (int k = 0; k < KN - 1; ++k) t.key[k] = won ? t.key[k + 1] : t.key[k];
        if (won) t.key[KN - 1] = KEY_EMPTY;
    }
}

}  // namespace icp
