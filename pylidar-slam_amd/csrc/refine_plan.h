// What the cloud-to-cloud refiner (refine.hip; icp_refine_* in include/icp_mi355x.h) decides without a device: every refusal, the
// size of its hash table, the grids of its launches, the number of cell rings a bound needs, its footprint.  Plain C++ without
// a HIP dependency, so that it also builds under the host sanitizers (tests/native/refine_plan_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "icp_mi355x.h"

namespace icp {

constexpr int REF_THREADS = 256;
constexpr int REF_MAX_BLOCKS = 2048;             // the iteration launches walk the source rows with a stride beyond this grid
constexpr int REF_MAX_ITERATION = 1000;
constexpr int REF_MAX_RINGS = 8;                 // more rings than this: the search scans every target row instead
constexpr int64_t REF_MAX_INDEX = 2147483647ll;  // rows are numbered by an int32
constexpr int REF_CELL_LIMIT = 1 << 20;          // cell coordinates are in [-2^20, 2^20) (pack_cell)
constexpr int REF_SUMS = 16;                     // sum d2, sum (p' - c) [3], sum (q - c) [3], sum (q - c)(p' - c)^T [9]
constexpr int REF_FIGURES = 17;                  // count, sum d2, mean p' [3], mean q [3], H [9]

// slots of the hash table: the power of two that is at least twice the rows, at least 64 (every probe sequence ends at a free slot)
inline int64_t refine_table_slots(int64_t max_target_rows) {
    int64_t t = 64;
    for (int k = 0; k < 40 && t < 2 * max_target_rows; ++k) t *= 2;
    return t;
}

// a thread per target row or table slot; 0 rows launch nothing
inline int64_t refine_blocks(int64_t count) {
    if (count < 1) return 0;
    return count / REF_THREADS + (count % REF_THREADS ? 1 : 0);
}

// the offsets launch: REF_OFFSET_PER table slots a thread
constexpr int REF_OFFSET_PER = 8;
inline int64_t refine_offset_blocks(int64_t slots) { return refine_blocks(slots / REF_OFFSET_PER + (slots % REF_OFFSET_PER ? 1 : 0)); }

// the iteration launches: a thread per source row up to REF_MAX_BLOCKS workgroups, a stride beyond; never an empty grid (the
// workgroups of an empty source still write their partial sums: zeros)
inline int refine_iterate_blocks(int64_t n) {
    const int64_t b = refine_blocks(n);
    return b < 1 ? 1 : (b > REF_MAX_BLOCKS ? REF_MAX_BLOCKS : (int)b);
}

// Rings of cells around the query's own cell that can hold a row strictly inside `max_distance`: ceil(max_distance / cell_size)
// + 1.  The + 1 is the widening for the rounded product behind a cell coordinate (floor(fl(v * fl(1 / cell)))): a row's
// computed cell can be the neighbour of its exact one, on the query's side as well, and one ring covers both (k - c <
// max_distance / cell + 1 + 2^-30 for coordinates below 2^20 cells).  The box test of the search (refine_device.h) takes the
// widened ring away again wherever the cell cannot hold a candidate.  Above REF_MAX_RINGS the search is exhaustive: 0.
inline int refine_rings(double max_distance, double cell_size) {
    const double ratio = max_distance / cell_size;
    if (!(ratio <= (double)(REF_MAX_RINGS - 1))) return 0;
    return (int)ceil(ratio) + 1;
}

// device memory of a refiner in bytes: per target row the sorted point (16), slot and rank (8); per table slot 16; per source
// row the correspondence (4); the partial sums of REF_MAX_BLOCKS workgroups; REF_MAX_ITERATION + 1 rows of history; the state.
// + 12 per row of either cloud (and as much pinned host memory) once that cloud has been given from host memory.  0 for capacities create refuses
inline uint64_t refine_footprint_bytes(int64_t max_target_rows, int64_t max_source_rows, int host_target, int host_source) {
    if (max_target_rows < 1 || max_source_rows < 1 || max_target_rows > REF_MAX_INDEX || max_source_rows > REF_MAX_INDEX) return 0;
    return (uint64_t)max_target_rows * 24 + (uint64_t)refine_table_slots(max_target_rows) * 16 + (uint64_t)max_source_rows * 4 +
           (uint64_t)REF_MAX_BLOCKS * 160 + (uint64_t)(REF_MAX_ITERATION + 1) * (16 + REF_FIGURES) * 8 + 512 +
           (host_target ? (uint64_t)max_target_rows * 12 : 0) + (host_source ? (uint64_t)max_source_rows * 12 : 0);
}

// ---- refusals: ICP_OK, or ICP_ERR_INVALID_ARGUMENT with the reason in `reason` (at least 160 bytes) ------------------------
inline bool refine_mem_ok(int mem) { return mem == ICP_MEM_HOST || mem == ICP_MEM_DEVICE; }

inline int refine_create_refusals(int64_t max_target_rows, int64_t max_source_rows, double cell_size, const void* out, char* reason) {
    reason[0] = 0;
    if (!out)
        snprintf(reason, 160, "icp_refine_create: out is NULL");
    else if (!(cell_size > 0.0) || !isfinite(cell_size))
        snprintf(reason, 160, "icp_refine_create: cell size %g is not a positive finite number", cell_size);
    else if (max_target_rows < 1 || max_source_rows < 1)
        snprintf(reason, 160, "icp_refine_create: max_target_rows = %lld, max_source_rows = %lld: below 1", (long long)max_target_rows,
                 (long long)max_source_rows);
    else if (max_target_rows > REF_MAX_INDEX || max_source_rows > REF_MAX_INDEX)
        snprintf(reason, 160, "icp_refine_create: a capacity exceeds %lld rows", (long long)REF_MAX_INDEX);
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int refine_rows_refusals(const char* who, const void* xyz, int64_t n, int64_t capacity, int mem, int32_t flags, char* reason) {
    reason[0] = 0;
    if (n < 0)
        snprintf(reason, 160, "%s: n = %lld is negative", who, (long long)n);
    else if (n > capacity)
        snprintf(reason, 160, "%s: n = %lld exceeds the capacity of %lld rows", who, (long long)n, (long long)capacity);
    else if (!refine_mem_ok(mem))
        snprintf(reason, 160, "%s: host or device memory", who);
    else if (flags & ~ICP_REFINE_DROP_ZERO_ROWS)
        snprintf(reason, 160, "%s: unknown flag in %d", who, (int)flags);
    else if (n > 0 && !xyz)
        snprintf(reason, 160, "%s: xyz is NULL", who);
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int refine_set_target_refusals(const void* xyz, int64_t n, int64_t capacity, int mem, int32_t flags, int in_flight, char* reason) {
    if (refine_rows_refusals("icp_refine_set_target", xyz, n, capacity, mem, flags, reason)) return ICP_ERR_INVALID_ARGUMENT;
    if (in_flight) snprintf(reason, 160, "icp_refine_set_target: a refinement is in flight (icp_refine_end collects it)");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int refine_launch_refusals(const void* xyz, int64_t n, int64_t capacity, int mem, const double* init16, const icp_refine_params* p, int have_target,
                                  int in_flight, char* reason) {
    reason[0] = 0;
    if (!p) {
        snprintf(reason, 160, "icp_refine_launch: params is NULL");
        return ICP_ERR_INVALID_ARGUMENT;
    }
    if (refine_rows_refusals("icp_refine_launch", xyz, n, capacity, mem, p->flags, reason)) return ICP_ERR_INVALID_ARGUMENT;
    bool finite = init16 != nullptr;
    for (int i = 0; finite && i < 16; ++i) finite = isfinite(init16[i]);
    if (!(p->max_distance > 0.0) || !isfinite(p->max_distance) || !isfinite(p->max_distance * p->max_distance))
        snprintf(reason, 160, "icp_refine_launch: max_distance %g is not a positive number with a finite square", p->max_distance);
    else if (p->max_iteration < 0 || p->max_iteration > REF_MAX_ITERATION)
        snprintf(reason, 160, "icp_refine_launch: max_iteration = %d is outside 0..%d", (int)p->max_iteration, REF_MAX_ITERATION);
    else if (!(p->relative_fitness >= 0.0) || !(p->relative_rmse >= 0.0))
        snprintf(reason, 160, "icp_refine_launch: relative_fitness = %g, relative_rmse = %g: a threshold is negative or NaN",
                 p->relative_fitness, p->relative_rmse);
    else if (!finite)
        snprintf(reason, 160, "icp_refine_launch: init is NULL or has a non-finite entry");
    else if (!have_target)
        snprintf(reason, 160, "icp_refine_launch: no target has been set (icp_refine_set_target)");
    else if (in_flight)
        snprintf(reason, 160, "icp_refine_launch: a refinement is in flight (icp_refine_end collects it)");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int refine_end_refusals(int in_flight, int out_mem, char* reason) {
    reason[0] = 0;
    if (!in_flight)
        snprintf(reason, 160, "icp_refine_end: nothing has been launched");
    else if (!refine_mem_ok(out_mem))
        snprintf(reason, 160, "icp_refine_end: host or device memory");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int refine_image_rows_refusals(const void* image, const void* image_ctx, const void* refiner_ctx, const void* xyz_out, const void* n_out,
                                      char* reason) {
    reason[0] = 0;
    if (!image)
        snprintf(reason, 160, "icp_refine_image_rows: image is NULL");
    else if (image_ctx != refiner_ctx)
        snprintf(reason, 160, "icp_refine_image_rows: the image belongs to another context");
    else if (!xyz_out || !n_out)
        snprintf(reason, 160, "icp_refine_image_rows: an output is NULL");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int refine_history_refusals(int have_result, int32_t iterations, int32_t cap, char* reason) {
    reason[0] = 0;
    if (!have_result)
        snprintf(reason, 160, "icp_refine_history: no refinement has been collected (icp_refine_end)");
    else if (cap < iterations + 1)
        snprintf(reason, 160, "icp_refine_history: cap = %d is below the %d evaluations of the run", (int)cap, (int)iterations + 1);
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

}  // namespace icp
