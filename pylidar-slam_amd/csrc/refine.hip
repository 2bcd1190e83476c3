// Cloud-to-cloud refinement: point-to-point ICP of one cloud against another, the step behind the 2-D alignment in the
// reference's loop closure (ElevationImageLoopClosure._compute_transform, slam/loop_closure.py:210-225, called at :237-243 on the
// `points_3D` of two elevation images).  The specification is in include/icp_mi355x.h; tests/refine_audit.py restates it.
//
// A refiner owns its search structure: a hashed uniform grid over the TARGET rows (GridEntry / pack_cell / hash_cell of the
// local map's grid; 64-bit cell keys compared on lookup, so a hash collision never merges two cells), the rows cell-sorted with
// their original index.  icp_refine_set_target builds it in a fixed number of launches with no host read:
//   1. k_ref_clear    the table to free slots, the target block (counters, bounding box, flags) to its start;
//   2. k_ref_count    a thread per row: the filter, the cell, its slot claimed by compare-and-swap, the row's rank in the cell by
//                     an integer atomic add; the bounding box of the kept rows by integer atomic min / max of ordered bits,
//                     combined per workgroup first.
//                     The order of the rows inside a cell depends on arrival — no result does: the winner of a search is the
//                     smallest (d2, row);
//   3. k_ref_offsets  the first sorted position of every cell: a scan of the counts per workgroup, its base from one integer atomic
//                     add on a cursor (the order of the CELLS depends on arrival as well); the pivot = the box's centre;
//   4. k_ref_scatter  a thread per row: the row to start[slot] + rank.
// A target row whose cell coordinate leaves [-2^20, 2^20) raises a flag on the device, which icp_refine_end reads with the
// result and turns into ICP_ERR_INVALID_ARGUMENT (the row is left unmatched meanwhile).
//
// icp_refine_launch enqueues k_ref_begin and then max_iteration + 1 pairs (k_ref_iterate, k_ref_solve):
//   k_ref_iterate  a lane per source row (a stride beyond REF_MAX_BLOCKS workgroups): moves the ORIGINAL row by the current T,
//                  scans the cells within the rings of the bound (a loop; a cell whose box cannot hold a candidate, or a better
//                  one than the best so far, is skipped), writes the correspondence and reduces the 16 sums and 3 counts of its
//                  workgroup — wave shuffles, then LDS, float64 — to ONE partial row, stored with plain vector stores.  The sums
//                  are taken about the pivot, so that a cloud 10 km from the origin cancels nothing;
//   k_ref_solve    one workgroup: adds the partial rows in fixed index order, forms the means and H, appends T and the 17
//                  figures to the history, applies the stop test, and otherwise takes the step (refine_device.h) T <- update T.
// Once `done` is set every later launch returns at its first instruction.  No float atomic anywhere, no workgroup waits for
// another, the host reads nothing until icp_refine_end: two runs of one call give the same bits.
#include <string.h>

#include <new>

#include "icp_internal.h"
#include "refine_device.h"
#include "refine_plan.h"

namespace icp {

// what icp_refine_set_target leaves on the device
struct RefTarget {
    double pivot[3];
    unsigned box_min[3], box_max[3];  // ordered bits of the kept rows' float32 coordinates
    int kept;                         // rows in the grid
    int left_out;                     // rows the zero-row filter took
    int out_of_range;                 // rows whose cell leaves [-2^20, 2^20)
    int cursor;                       // sorted positions handed out so far
};

// the state of a refinement; the result block icp_refine_end copies home
struct RefState {
    double T[16];
    double fitness, rmse;
    long long count, counted, left_out;
    int iter, done, converged, max_iteration;
    double relative_fitness, relative_rmse;
};

struct RefPartial {
    double s[REF_SUMS];
    long long count, counted, left_out, pad;
};
static_assert(sizeof(RefPartial) == 160, "RefPartial: the footprint formula counts 160 bytes");

struct RefSearch {
    const GridEntry* __restrict__ table;
    const float4* __restrict__ pts;
    unsigned mask;
    int rings;  // 0: every kept row is scanned
    double cell, inv_cell, r2;
};

__device__ __forceinline__ unsigned ref_order32(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ref_unorder32(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__global__ __launch_bounds__(REF_THREADS) void k_ref_clear(GridEntry* __restrict__ table, long long slots, RefTarget* __restrict__ tg) {
    const long long s = (long long)blockIdx.x * REF_THREADS + threadIdx.x;
    if (s < slots) {
        GridEntry e;
        e.key = GRID_EMPTY;
        e.start = 0;
        e.count = 0;
        table[s] = e;
    }
    if (s == 0) {
        for (int a = 0; a < 3; ++a) {
            tg->pivot[a] = 0.0;
            tg->box_min[a] = 0xffffffffu;
            tg->box_max[a] = 0u;
        }
        tg->kept = tg->left_out = tg->out_of_range = tg->cursor = 0;
    }
}

// (atomics to ONE address queue up: the counters and the box are combined per workgroup — barrier counts, LDS atomics — and go
// to memory once a workgroup)
__global__ __launch_bounds__(REF_THREADS) void k_ref_count(const float* __restrict__ xyz, int n, int drop_zero, double inv_cell,
                                                           GridEntry* table, unsigned mask, int* __restrict__ slot_of,
                                                           int* __restrict__ rank_of, RefTarget* tg) {
    __shared__ unsigned box_s[6];
    if (threadIdx.x < 6) box_s[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    const long long i = (long long)blockIdx.x * REF_THREADS + threadIdx.x;
    const bool live = i < n;
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) {
        x = xyz[3 * i];
        y = xyz[3 * i + 1];
        z = xyz[3 * i + 2];
    }
    int slot = -1, rank = 0;
    bool dropped = false, outside = false;
    if (live && drop_zero && refine_zero_row(x, y, z)) {
        dropped = true;
    } else if (live && refine_finite3(x, y, z)) {
        const double cx = refine_cell((double)x, inv_cell), cy = refine_cell((double)y, inv_cell), cz = refine_cell((double)z, inv_cell);
        const double lim = (double)REF_CELL_LIMIT;
        if (!(cx >= -lim && cx < lim && cy >= -lim && cy < lim && cz >= -lim && cz < lim)) {
            outside = true;
        } else {
            const unsigned long long key = pack_cell((int)cx, (int)cy, (int)cz);
            unsigned s = hash_cell(key) & mask;
            // (the table has at least twice as many slots as rows: a free slot ends every probe sequence)
            for (unsigned long long probe = 0; probe <= mask; ++probe) {
                unsigned long long seen = __hip_atomic_load(&table[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (seen == GRID_EMPTY) seen = atomicCAS(&table[s].key, GRID_EMPTY, key);
                if (seen == GRID_EMPTY || seen == key) {
                    slot = (int)s;
                    break;
                }
                s = (s + 1) & mask;
            }
            if (slot >= 0) {
                rank = atomicAdd(&table[slot].count, 1);
                atomicMin(&box_s[0], ref_order32(x));
                atomicMin(&box_s[1], ref_order32(y));
                atomicMin(&box_s[2], ref_order32(z));
                atomicMax(&box_s[3], ref_order32(x));
                atomicMax(&box_s[4], ref_order32(y));
                atomicMax(&box_s[5], ref_order32(z));
            }
        }
    }
    if (live) {
        slot_of[i] = slot;
        rank_of[i] = rank;
    }
    const int kept = __syncthreads_count(slot >= 0), left_out = __syncthreads_count(dropped), out_of_range = __syncthreads_count(outside);
    if (threadIdx.x == 0) {
        if (kept) atomicAdd(&tg->kept, kept);
        if (left_out) atomicAdd(&tg->left_out, left_out);
        if (out_of_range) atomicAdd(&tg->out_of_range, out_of_range);
    }
    if (kept && threadIdx.x < 3) atomicMin(&tg->box_min[threadIdx.x], box_s[threadIdx.x]);
    if (kept && threadIdx.x >= 3 && threadIdx.x < 6) atomicMax(&tg->box_max[threadIdx.x - 3], box_s[threadIdx.x]);
}

// the first sorted position of every cell: a workgroup scans the counts of its REF_THREADS x REF_OFFSET_PER slots and takes its
// base from ONE integer atomic add on the cursor.  The order of the cells in the sorted array depends on arrival — no result
// does.  Thread 0 of workgroup 0 also forms the pivot: the centre of the kept rows' bounding box
__global__ __launch_bounds__(REF_THREADS) void k_ref_offsets(GridEntry* table, long long slots, RefTarget* tg) {
    __shared__ int wave_total[REF_THREADS / 64];
    __shared__ int base_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0 && tg->kept > 0)
        for (int a = 0; a < 3; ++a) tg->pivot[a] = 0.5 * ((double)ref_unorder32(tg->box_min[a]) + (double)ref_unorder32(tg->box_max[a]));
    const long long first = ((long long)blockIdx.x * REF_THREADS + threadIdx.x) * REF_OFFSET_PER;
    int c[REF_OFFSET_PER], mine = 0;
#pragma unroll
    for (int k = 0; k < REF_OFFSET_PER; ++k) {
        c[k] = first + k < slots ? table[first + k].count : 0;
        mine += c[k];
    }
    int incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < REF_THREADS / 64; ++w) total += wave_total[w];
        base_s = total ? atomicAdd(&tg->cursor, total) : 0;
    }
    __syncthreads();
    int run = base_s + incl - mine;
    for (int w = 0; w < wave; ++w) run += wave_total[w];
#pragma unroll
    for (int k = 0; k < REF_OFFSET_PER; ++k) {
        if (first + k < slots && c[k]) table[first + k].start = run;
        run += c[k];
    }
}

__global__ __launch_bounds__(REF_THREADS) void k_ref_scatter(const float* __restrict__ xyz, int n, const GridEntry* __restrict__ table,
                                                             const int* __restrict__ slot_of, const int* __restrict__ rank_of,
                                                             float4* __restrict__ pts) {
    const long long i = (long long)blockIdx.x * REF_THREADS + threadIdx.x;
    if (i >= n) return;
    const int slot = slot_of[i];
    if (slot < 0) return;
    pts[table[slot].start + rank_of[i]] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], __int_as_float((int)i));
}

__global__ void k_ref_begin(RefState* st, RefState init) { *st = init; }

struct RefBest {
    double d2, qx, qy, qz;
    int row;
};

// the rows [start, start + count) of the cell-sorted target against the moved point: the smallest (d2, row) strictly inside the bound
__device__ __forceinline__ void ref_scan_rows(const float4* __restrict__ pts, int start, int count, double px, double py, double pz, double r2,
                                              RefBest& best) {
    for (int j = start; j < start + count; ++j) {
        const float4 q = pts[j];
        const double dx = px - (double)q.x, dy = py - (double)q.y, dz = pz - (double)q.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const int row = __float_as_int(q.w);
        if (d2 < r2 && (d2 < best.d2 || (d2 == best.d2 && row < best.row))) {
            best.d2 = d2;
            best.row = row;
            best.qx = (double)q.x;
            best.qy = (double)q.y;
            best.qz = (double)q.z;
        }
    }
}

__device__ __forceinline__ void ref_search(const RefSearch& g, int kept, double px, double py, double pz, RefBest& best) {
    best.d2 = INFINITY;
    best.row = 0x7fffffff;
    best.qx = best.qy = best.qz = 0.0;
    if (g.rings == 0) {
        ref_scan_rows(g.pts, 0, kept, px, py, pz, g.r2, best);
        return;
    }
    const double cx = refine_cell(px, g.inv_cell), cy = refine_cell(py, g.inv_cell), cz = refine_cell(pz, g.inv_cell);
    const double reach = (double)(REF_CELL_LIMIT + g.rings);
    // (a query further out than the rings reach from every cell of the table has no candidate)
    if (!(fabs(cx) <= reach && fabs(cy) <= reach && fabs(cz) <= reach)) return;
    const int ix = (int)cx, iy = (int)cy, iz = (int)cz;
    const int lo = -REF_CELL_LIMIT, hi = REF_CELL_LIMIT - 1;
    const int x0 = max(ix - g.rings, lo), x1 = min(ix + g.rings, hi), y0 = max(iy - g.rings, lo), y1 = min(iy + g.rings, hi);
    const int z0 = max(iz - g.rings, lo), z1 = min(iz + g.rings, hi);
    for (int kz = z0; kz <= z1; ++kz) {
        const double gz = refine_axis_gap(pz, kz, g.cell), gz2 = gz * gz;
        if (refine_gap_floor(gz2) >= g.r2) continue;
        for (int ky = y0; ky <= y1; ++ky) {
            const double gy = refine_axis_gap(py, ky, g.cell), gzy2 = gz2 + gy * gy;
            if (refine_gap_floor(gzy2) >= g.r2) continue;
            for (int kx = x0; kx <= x1; ++kx) {
                const double gx = refine_axis_gap(px, kx, g.cell);
                const double bound = refine_gap_floor(gzy2 + gx * gx);
                // (a tie at the best distance may still bring a lower row: only a cell strictly further is skipped)
                if (bound >= g.r2 || bound > best.d2) continue;
                const unsigned long long key = pack_cell(kx, ky, kz);
                unsigned s = hash_cell(key) & g.mask;
                for (unsigned long long probe = 0; probe <= g.mask; ++probe) {
                    const GridEntry e = g.table[s];
                    if (e.key == key) {
                        ref_scan_rows(g.pts, e.start, e.count, px, py, pz, g.r2, best);
                        break;
                    }
                    if (e.key == GRID_EMPTY) break;
                    s = (s + 1) & g.mask;
                }
            }
        }
    }
}

__device__ __forceinline__ double ref_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;  // (lane 0 holds the sum)
}
__device__ __forceinline__ long long ref_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ __launch_bounds__(REF_THREADS) void k_ref_iterate(const RefState* __restrict__ st, const RefTarget* __restrict__ tg, RefSearch g,
                                                             const float* __restrict__ xyz, int n, int drop_zero, int* __restrict__ corr,
                                                             RefPartial* __restrict__ partial) {
    if (st->done) return;
    __shared__ double sums_s[REF_THREADS / 64][REF_SUMS];
    __shared__ long long counts_s[REF_THREADS / 64][3];
    double T[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = st->T[k];
    const double c0 = tg->pivot[0], c1 = tg->pivot[1], c2 = tg->pivot[2];
    const int kept = tg->kept;
    double s[REF_SUMS];
#pragma unroll
    for (int k = 0; k < REF_SUMS; ++k) s[k] = 0.0;
    long long count = 0, counted = 0, left_out = 0;
    const long long stride = (long long)gridDim.x * REF_THREADS;
    for (long long i = (long long)blockIdx.x * REF_THREADS + threadIdx.x; i < n; i += stride) {
        const float xf = xyz[3 * i], yf = xyz[3 * i + 1], zf = xyz[3 * i + 2];
        if (drop_zero && refine_zero_row(xf, yf, zf)) {
            ++left_out;
            corr[i] = -1;
            continue;
        }
        ++counted;
        const double x = (double)xf, y = (double)yf, z = (double)zf;
        const double px = refine_move(T, 0, x, y, z), py = refine_move(T, 1, x, y, z), pz = refine_move(T, 2, x, y, z);
        RefBest best;
        best.row = 0x7fffffff;
        if (refine_finite3(px, py, pz)) ref_search(g, kept, px, py, pz, best);
        if (best.row == 0x7fffffff) {
            corr[i] = -1;
            continue;
        }
        corr[i] = best.row;
        ++count;
        const double a0 = px - c0, a1 = py - c1, a2 = pz - c2, b0 = best.qx - c0, b1 = best.qy - c1, b2 = best.qz - c2;
        s[0] += best.d2;
        s[1] += a0;
        s[2] += a1;
        s[3] += a2;
        s[4] += b0;
        s[5] += b1;
        s[6] += b2;
        s[7] += b0 * a0;
        s[8] += b0 * a1;
        s[9] += b0 * a2;
        s[10] += b1 * a0;
        s[11] += b1 * a1;
        s[12] += b1 * a2;
        s[13] += b2 * a0;
        s[14] += b2 * a1;
        s[15] += b2 * a2;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < REF_SUMS; ++k) {
        const double v = ref_wave_sum(s[k]);
        if (lane == 0) sums_s[wave][k] = v;
    }
    count = ref_wave_sum(count);
    counted = ref_wave_sum(counted);
    left_out = ref_wave_sum(left_out);
    if (lane == 0) {
        counts_s[wave][0] = count;
        counts_s[wave][1] = counted;
        counts_s[wave][2] = left_out;
    }
    __syncthreads();
    RefPartial* mine = partial + blockIdx.x;
    if (threadIdx.x < REF_SUMS) {
        double v = sums_s[0][threadIdx.x];
        for (int w = 1; w < REF_THREADS / 64; ++w) v += sums_s[w][threadIdx.x];
        mine->s[threadIdx.x] = v;
    } else if (threadIdx.x < REF_SUMS + 3) {
        const int k = threadIdx.x - REF_SUMS;
        long long v = counts_s[0][k];
        for (int w = 1; w < REF_THREADS / 64; ++w) v += counts_s[w][k];
        (&mine->count)[k] = v;
    }
}

// the 19 columns of the partial rows, each added in 8 segments of consecutive rows and the segments in order: a fixed order
constexpr int REF_SOLVE_THREADS = 256, REF_SOLVE_SEGMENTS = 8, REF_SOLVE_COLUMNS = 32;
__global__ __launch_bounds__(REF_SOLVE_THREADS) void k_ref_solve(RefState* st, const RefTarget* __restrict__ tg,
                                                                 const RefPartial* __restrict__ partial, int blocks,
                                                                 double* __restrict__ hist_T, double* __restrict__ hist_S) {
    if (st->done) return;
    __shared__ double sums_s[REF_SOLVE_SEGMENTS][REF_SUMS];
    __shared__ long long counts_s[REF_SOLVE_SEGMENTS][3];
    const int col = threadIdx.x % REF_SOLVE_COLUMNS, seg = threadIdx.x / REF_SOLVE_COLUMNS;
    const int per = (blocks + REF_SOLVE_SEGMENTS - 1) / REF_SOLVE_SEGMENTS;
    const int b0 = seg * per, b1 = min(blocks, b0 + per);
    if (col < REF_SUMS) {
        double v = 0.0;
        for (int b = b0; b < b1; ++b) v += partial[b].s[col];
        sums_s[seg][col] = v;
    } else if (col < REF_SUMS + 3) {
        long long v = 0;
        for (int b = b0; b < b1; ++b) v += (&partial[b].count)[col - REF_SUMS];
        counts_s[seg][col - REF_SUMS] = v;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double s[REF_SUMS];
    long long cnt[3];
    for (int k = 0; k < REF_SUMS; ++k) {
        double v = sums_s[0][k];
        for (int g = 1; g < REF_SOLVE_SEGMENTS; ++g) v += sums_s[g][k];
        s[k] = v;
    }
    for (int k = 0; k < 3; ++k) {
        long long v = counts_s[0][k];
        for (int g = 1; g < REF_SOLVE_SEGMENTS; ++g) v += counts_s[g][k];
        cnt[k] = v;
    }
    // the 17 figures: count, sum d2, mean p' [3], mean q [3], H [9] = sum (q - c)(p' - c)^T / n - (mu_q - c)(mu_p - c)^T
    double fig[REF_FIGURES];
    const double nn = (double)cnt[0];
    fig[0] = nn;
    fig[1] = s[0];
    double ma[3] = {0.0, 0.0, 0.0}, mb[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < 3; ++a) {
        if (cnt[0] > 0) {
            ma[a] = s[1 + a] / nn;
            mb[a] = s[4 + a] / nn;
        }
        fig[2 + a] = cnt[0] > 0 ? tg->pivot[a] + ma[a] : 0.0;
        fig[5 + a] = cnt[0] > 0 ? tg->pivot[a] + mb[a] : 0.0;
    }
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) fig[8 + 3 * a + b] = cnt[0] > 0 ? s[7 + 3 * a + b] / nn - mb[a] * ma[b] : 0.0;
    const int i = st->iter;
    for (int k = 0; k < 16; ++k) hist_T[16 * (long long)i + k] = st->T[k];
    for (int k = 0; k < REF_FIGURES; ++k) hist_S[REF_FIGURES * (long long)i + k] = fig[k];
    const double fitness = (cnt[0] > 0 && cnt[1] > 0) ? nn / (double)cnt[1] : 0.0;
    const double rmse = cnt[0] > 0 ? sqrt(s[0] / nn) : 0.0;
    const bool stop = i > 0 && fabs(fitness - st->fitness) < st->relative_fitness && fabs(rmse - st->rmse) < st->relative_rmse;
    st->fitness = fitness;
    st->rmse = rmse;
    st->count = cnt[0];
    st->counted = cnt[1];
    st->left_out = cnt[2];
    if (stop || i >= st->max_iteration) {
        st->converged = stop ? 1 : 0;
        st->done = 1;
        return;
    }
    double update[16], next[16], now[16];
    refine_step(fig, update);
    for (int k = 0; k < 16; ++k) now[k] = st->T[k];
    refine_mul44(update, now, next);
    for (int k = 0; k < 16; ++k) st->T[k] = next[k];
    st->iter = i + 1;
}

}  // namespace icp

using namespace icp;

struct icp_refine {
    icp_ctx* ctx = nullptr;
    int64_t max_target = 0, max_source = 0, slots = 0;
    double cell = 0.0, inv_cell = 0.0;
    GridEntry* table = nullptr;     // [slots]
    float4* pts = nullptr;          // [max_target] cell-sorted (x, y, z, bits(original row))
    int* slot_of = nullptr;         // [max_target] the slot of a row's cell (-1: not in the grid)
    int* rank_of = nullptr;         // [max_target] its rank inside the cell
    int* corr = nullptr;            // [max_source] the correspondences of the last evaluation
    RefPartial* partial = nullptr;  // [REF_MAX_BLOCKS]
    double* hist_T = nullptr;       // [REF_MAX_ITERATION + 1][16]
    double* hist_S = nullptr;       // [REF_MAX_ITERATION + 1][17]
    RefTarget* target = nullptr;
    RefState* state = nullptr;
    // host rows on their way in: a pinned buffer and a device buffer per cloud, allocated by the first host cloud of its kind
    struct Stage {
        float* dev = nullptr;        // [capacity][3]
        float* host = nullptr;       // ... pinned
        hipEvent_t copied = nullptr; // the last copy has left the pinned rows
    } stage_target, stage_source;
    struct Home {
        RefState st;
        RefTarget tg;
    }* home = nullptr;              // pinned
    int64_t target_n = 0, source_n = 0;
    bool have_target = false, in_flight = false, have_result = false;
    int32_t iterations = 0;
};

namespace {

void refine_free(icp_refine* r) {
    void* dev[] = {r->table, r->pts, r->slot_of, r->rank_of, r->corr, r->partial, r->hist_T, r->hist_S, r->target, r->state,
                   r->stage_target.dev, r->stage_source.dev};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    for (icp_refine::Stage* st : {&r->stage_target, &r->stage_source}) {
        if (st->host) (void)hipHostFree(st->host);
        if (st->copied) (void)hipEventDestroy(st->copied);
    }
    if (r->home) (void)hipHostFree(r->home);
    delete r;
}

// host rows into the pinned buffer (copied before the call returns), from there to the device behind the stream's work
int refine_stage(icp_refine* r, icp_refine::Stage& st, const float* xyz, int64_t n, int64_t capacity, const float** rows) {
    icp_ctx* ctx = r->ctx;
    const size_t cap_bytes = (size_t)capacity * 12, bytes = (size_t)n * 12;
    if (!st.dev) ICP_HIP(ctx, hipMalloc((void**)&st.dev, cap_bytes));
    if (!st.host) ICP_HIP(ctx, hipHostMalloc((void**)&st.host, cap_bytes, hipHostMallocDefault));
    if (!st.copied) ICP_HIP(ctx, hipEventCreateWithFlags(&st.copied, hipEventDisableTiming));
    else ICP_HIP(ctx, hipEventSynchronize(st.copied));  // (the previous copy out of the pinned rows, not the work behind it)
    memcpy(st.host, xyz, bytes);
    ICP_HIP(ctx, hipMemcpyAsync(st.dev, st.host, bytes, hipMemcpyHostToDevice, ctx->stream));
    ICP_HIP(ctx, hipEventRecord(st.copied, ctx->stream));
    *rows = st.dev;
    return ICP_OK;
}

}  // namespace

extern "C" {

void icp_default_refine_params(icp_refine_params* p) {
    if (!p) return;
    p->max_distance = 1.0;
    p->relative_fitness = 1e-6;
    p->relative_rmse = 1e-6;
    p->max_iteration = 30;
    p->flags = 0;
}

int icp_refine_create(icp_ctx* ctx, int64_t max_target_rows, int64_t max_source_rows, double cell_size, icp_refine** out) {
    if (!ctx) return ICP_ERR_INVALID_ARGUMENT;
    char why[160];
    if (refine_create_refusals(max_target_rows, max_source_rows, cell_size, out, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    *out = nullptr;
    DeviceGuard guard(ctx, false);
    icp_refine* r = new (std::nothrow) icp_refine();
    if (!r) return fail(ctx, ICP_ERR_HIP, "icp_refine_create: out of host memory");
    r->ctx = ctx;
    r->max_target = max_target_rows;
    r->max_source = max_source_rows;
    r->slots = refine_table_slots(max_target_rows);
    r->cell = cell_size;
    r->inv_cell = 1.0 / cell_size;
    const size_t hist_rows = (size_t)REF_MAX_ITERATION + 1;
    hipError_t err = hipMalloc((void**)&r->table, (size_t)r->slots * sizeof(GridEntry));
    if (err == hipSuccess) err = hipMalloc((void**)&r->pts, (size_t)max_target_rows * sizeof(float4));
    if (err == hipSuccess) err = hipMalloc((void**)&r->slot_of, (size_t)max_target_rows * sizeof(int));
    if (err == hipSuccess) err = hipMalloc((void**)&r->rank_of, (size_t)max_target_rows * sizeof(int));
    if (err == hipSuccess) err = hipMalloc((void**)&r->corr, (size_t)max_source_rows * sizeof(int));
    if (err == hipSuccess) err = hipMalloc((void**)&r->partial, (size_t)REF_MAX_BLOCKS * sizeof(RefPartial));
    if (err == hipSuccess) err = hipMalloc((void**)&r->hist_T, hist_rows * 16 * sizeof(double));
    if (err == hipSuccess) err = hipMalloc((void**)&r->hist_S, hist_rows * REF_FIGURES * sizeof(double));
    if (err == hipSuccess) err = hipMalloc((void**)&r->target, sizeof(RefTarget));
    if (err == hipSuccess) err = hipMalloc((void**)&r->state, sizeof(RefState));
    if (err == hipSuccess) err = hipHostMalloc((void**)&r->home, sizeof(*r->home), hipHostMallocDefault);
    if (err != hipSuccess) {
        ctx->error = std::string("icp_refine_create: ") + hipGetErrorString(err);
        refine_free(r);
        return ICP_ERR_HIP;
    }
    *out = r;
    return ICP_OK;
}

void icp_refine_destroy(icp_refine* r) {
    if (!r) return;
    DeviceGuard guard(r->ctx, false);
    (void)hipStreamSynchronize(r->ctx->stream);
    refine_free(r);
}

int icp_refine_set_target(icp_refine* r, const float* xyz, int64_t n, int mem, int32_t flags) {
    if (!r) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = r->ctx;
    char why[160];
    if (refine_set_target_refusals(xyz, n, r->max_target, mem, flags, r->in_flight, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    DeviceGuard guard(ctx, false);
    const float* rows = xyz;
    if (mem == ICP_MEM_HOST && n > 0) {
        const int rc = refine_stage(r, r->stage_target, xyz, n, r->max_target, &rows);
        if (rc) return rc;
    }
    const dim3 threads(REF_THREADS);
    hipLaunchKernelGGL(k_ref_clear, dim3((unsigned)refine_blocks(r->slots)), threads, 0, ctx->stream, r->table, (long long)r->slots, r->target);
    if (n > 0)
        hipLaunchKernelGGL(k_ref_count, dim3((unsigned)refine_blocks(n)), threads, 0, ctx->stream, rows, (int)n,
                           (flags & ICP_REFINE_DROP_ZERO_ROWS) ? 1 : 0, r->inv_cell, r->table, (unsigned)(r->slots - 1), r->slot_of, r->rank_of,
                           r->target);
    hipLaunchKernelGGL(k_ref_offsets, dim3((unsigned)refine_offset_blocks(r->slots)), threads, 0, ctx->stream, r->table,
                       (long long)r->slots, r->target);
    if (n > 0)
        hipLaunchKernelGGL(k_ref_scatter, dim3((unsigned)refine_blocks(n)), threads, 0, ctx->stream, rows, (int)n, r->table, r->slot_of,
                           r->rank_of, r->pts);
    ICP_HIP(ctx, hipGetLastError());
    r->target_n = n;
    r->have_target = true;
    return ICP_OK;
}

int icp_refine_launch(icp_refine* r, const float* xyz, int64_t n, int mem, const double init[16], const icp_refine_params* params) {
    if (!r) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = r->ctx;
    char why[160];
    if (refine_launch_refusals(xyz, n, r->max_source, mem, init, params, r->have_target, r->in_flight, why))
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    DeviceGuard guard(ctx, false);
    const float* rows = xyz;
    if (mem == ICP_MEM_HOST && n > 0) {
        const int rc = refine_stage(r, r->stage_source, xyz, n, r->max_source, &rows);
        if (rc) return rc;
    }
    RefState st;
    memset(&st, 0, sizeof(st));
    memcpy(st.T, init, sizeof(st.T));
    st.max_iteration = n > 0 ? params->max_iteration : 0;  // (an empty source is evaluated once: nothing can move it)
    st.relative_fitness = params->relative_fitness;
    st.relative_rmse = params->relative_rmse;
    RefSearch g;
    g.table = r->table;
    g.pts = r->pts;
    g.mask = (unsigned)(r->slots - 1);
    g.rings = refine_rings(params->max_distance, r->cell);
    g.cell = r->cell;
    g.inv_cell = r->inv_cell;
    g.r2 = params->max_distance * params->max_distance;
    const int blocks = refine_iterate_blocks(n), drop = (params->flags & ICP_REFINE_DROP_ZERO_ROWS) ? 1 : 0;
    hipLaunchKernelGGL(k_ref_begin, dim3(1), dim3(1), 0, ctx->stream, r->state, st);
    for (int k = 0; k <= st.max_iteration; ++k) {
        hipLaunchKernelGGL(k_ref_iterate, dim3((unsigned)blocks), dim3(REF_THREADS), 0, ctx->stream, r->state, r->target, g, rows, (int)n, drop,
                           r->corr, r->partial);
        hipLaunchKernelGGL(k_ref_solve, dim3(1), dim3(REF_SOLVE_THREADS), 0, ctx->stream, r->state, r->target, r->partial, blocks, r->hist_T,
                           r->hist_S);
    }
    ICP_HIP(ctx, hipGetLastError());
    r->source_n = n;
    r->in_flight = true;
    r->have_result = false;
    return ICP_OK;
}

int icp_refine_end(icp_refine* r, icp_refine_result* result, int32_t* correspondence_out, int out_mem) {
    if (!r) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = r->ctx;
    char why[160];
    if (refine_end_refusals(r->in_flight, out_mem, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    DeviceGuard guard(ctx, false);
    r->in_flight = false;
    ICP_HIP(ctx, hipMemcpyAsync(&r->home->st, r->state, sizeof(RefState), hipMemcpyDeviceToHost, ctx->stream));
    ICP_HIP(ctx, hipMemcpyAsync(&r->home->tg, r->target, sizeof(RefTarget), hipMemcpyDeviceToHost, ctx->stream));
    if (correspondence_out && r->source_n > 0)
        ICP_HIP(ctx, hipMemcpyAsync(correspondence_out, r->corr, (size_t)r->source_n * sizeof(int),
                                    out_mem == ICP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
    ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const RefState& st = r->home->st;
    const RefTarget& tg = r->home->tg;
    r->iterations = st.iter;
    r->have_result = true;
    if (result) {
        memcpy(result->transformation, st.T, sizeof(st.T));
        result->fitness = st.fitness;
        result->inlier_rmse = st.rmse;
        result->correspondences = st.count;
        result->source_rows = st.counted;
        result->target_rows = r->target_n - tg.left_out;
        result->source_rows_left_out = st.left_out;
        result->target_rows_left_out = tg.left_out;
        result->iterations = st.iter;
        result->converged = st.converged;
    }
    if (tg.out_of_range > 0) {
        snprintf(why, sizeof(why), "icp_refine_end: %d target rows lie outside +-2^20 cells of %g: they were left unmatched", tg.out_of_range,
                 r->cell);
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    }
    return ICP_OK;
}

int icp_refine_image_rows(icp_refine* r, icp_elevation* image, const float** xyz_out, int64_t* n_out) {
    if (!r) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = r->ctx;
    char why[160];
    if (refine_image_rows_refusals(image, image ? elevation_context(image) : nullptr, ctx, xyz_out, n_out, why))
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    *xyz_out = elevation_points_device(image, n_out);
    return ICP_OK;
}

int icp_refine_history(icp_refine* r, double* transforms_out, double* sums_out, int32_t cap) {
    if (!r) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = r->ctx;
    char why[160];
    if (refine_history_refusals(r->have_result, r->iterations, cap, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    DeviceGuard guard(ctx, false);
    const size_t rows = (size_t)r->iterations + 1;
    if (transforms_out) ICP_HIP(ctx, hipMemcpyAsync(transforms_out, r->hist_T, rows * 16 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (sums_out) ICP_HIP(ctx, hipMemcpyAsync(sums_out, r->hist_S, rows * REF_FIGURES * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICP_OK;
}

}  // extern "C"
