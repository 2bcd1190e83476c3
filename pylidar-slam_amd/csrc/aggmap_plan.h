// What the aggregated world map (aggmap.hip; icp_aggmap_* in include/icp_mi355x.h) decides without a device: the exact voxel
// key and its slot, the slot count and the footprint of a (capacity, rows per insert) pair, and every refusal.  Plain C++
// without a HIP dependency, so that it also builds into a stand-alone program under the host sanitizers
// (tests/native/aggmap_plan_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "icp_mi355x.h"

#if defined(__HIPCC__)
#define ICP_AGGMAP_HD __host__ __device__
#else
#define ICP_AGGMAP_HD
#endif

namespace icp {

constexpr long long AGGMAP_COORD_OFFSET = 1ll << 20;       // voxel coordinates lie in [-2^20, 2^20)
constexpr unsigned long long AGGMAP_COORD_MASK = 0x1FFFFFull;
constexpr unsigned long long AGGMAP_EMPTY = ~0ull;         // no key has bit 63 set
constexpr int64_t AGGMAP_MAX_ROWS = 1ll << 30;             // capacity + rows per insert: the table stays below 2^32 slots
constexpr int AGGMAP_ERR_PROBE = 1;                        // bits of the error word: a probe visited every slot

// the exact key of a voxel: three biased 21-bit coordinates in 63 bits (x lowest)
ICP_AGGMAP_HD inline unsigned long long aggmap_pack(long long cx, long long cy, long long cz) {
    return (unsigned long long)(cx + AGGMAP_COORD_OFFSET) | ((unsigned long long)(cy + AGGMAP_COORD_OFFSET) << 21) |
           ((unsigned long long)(cz + AGGMAP_COORD_OFFSET) << 42);
}

ICP_AGGMAP_HD inline void aggmap_unpack(unsigned long long key, long long c[3]) {
    c[0] = (long long)(key & AGGMAP_COORD_MASK) - AGGMAP_COORD_OFFSET;
    c[1] = (long long)((key >> 21) & AGGMAP_COORD_MASK) - AGGMAP_COORD_OFFSET;
    c[2] = (long long)((key >> 42) & AGGMAP_COORD_MASK) - AGGMAP_COORD_OFFSET;
}

// a voxel coordinate (still a double: rint(w / v)) the key has room for; NaN and the infinities are not
ICP_AGGMAP_HD inline bool aggmap_coord_in_range(double c) {
    return c >= -(double)AGGMAP_COORD_OFFSET && c < (double)AGGMAP_COORD_OFFSET;
}

// first slot of a key's probe chain (the next ones follow linearly, wrapping): the mixed key under the table's mask
ICP_AGGMAP_HD inline unsigned long long aggmap_slot(unsigned long long key, unsigned long long mask) {
    unsigned long long x = key;
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    return x & mask;
}

// slots of the table: the power of two at or above 2 (C + R) — at most C stored voxels and, in the one insert that crosses the
// capacity, fewer than R claimed ones that stay unstored: the table is never more than half full.  0: C + R is out of range
inline uint64_t aggmap_slots_for(uint64_t total) {  // total = C + R, 1 .. AGGMAP_MAX_ROWS; 0 otherwise
    if (total < 1 || total > (uint64_t)AGGMAP_MAX_ROWS) return 0;
    uint64_t s = 2;
    while (s < 2 * total) s <<= 1;
    return s;
}

inline uint64_t aggmap_slot_count(int64_t capacity, int64_t max_rows) {
    if (capacity < 1 || max_rows < 1 || capacity > AGGMAP_MAX_ROWS || max_rows > AGGMAP_MAX_ROWS) return 0;
    return aggmap_slots_for((uint64_t)capacity + (uint64_t)max_rows);
}

// rows a workgroup of the count and emit launches walks (consecutive, 256 at a time): at most AGGMAP_MAX_BLOCKS workgroups
constexpr int AGGMAP_THREADS = 256;
constexpr int AGGMAP_MAX_BLOCKS = 1024;
inline int64_t aggmap_rows_per_block(int64_t n) {
    if (n < 1) return AGGMAP_THREADS;
    const int64_t tiles = n / AGGMAP_THREADS + (n % AGGMAP_THREADS ? 1 : 0);  // (no sum that could overflow)
    const int64_t per = tiles / AGGMAP_MAX_BLOCKS + (tiles % AGGMAP_MAX_BLOCKS ? 1 : 0);
    return (per < 1 ? 1 : per) * AGGMAP_THREADS;
}

// device memory of a map in bytes: per slot the key (8) and its record (16: candidate row, stored index, hits, last frame);
// per stored point the float64 point (24), first frame (4) and slot (4); per row of an insert its staged copy (12) and slot
// (4); the workgroup counts; the counters.  0: out of range
inline uint64_t aggmap_footprint_bytes(int64_t capacity, int64_t max_rows) {
    const uint64_t slots = aggmap_slot_count(capacity, max_rows);
    if (!slots) return 0;
    return slots * 24 + (uint64_t)capacity * 32 + (uint64_t)max_rows * 16 + (uint64_t)(AGGMAP_MAX_BLOCKS + 1) * 4 + 64;
}

inline bool aggmap_pose_finite(const double* pose16) {
    if (!pose16) return false;
    for (int i = 0; i < 16; ++i)
        if (!isfinite(pose16[i])) return false;
    return true;
}

inline bool aggmap_mem_ok(int mem) { return mem == ICP_MEM_HOST || mem == ICP_MEM_DEVICE; }

// ICP_OK, or ICP_ERR_INVALID_ARGUMENT with the reason in `reason` (at least 160 bytes)
inline int aggmap_create_refusals(double voxel, int64_t capacity, int64_t max_rows, char* reason) {
    reason[0] = 0;
    if (!(voxel > 0.0) || !isfinite(voxel))
        snprintf(reason, 160, "icp_aggmap_create: voxel size %g is not a positive finite number", voxel);
    else if (capacity < 1)
        snprintf(reason, 160, "icp_aggmap_create: capacity = %lld is below 1", (long long)capacity);
    else if (max_rows < 1)
        snprintf(reason, 160, "icp_aggmap_create: max_insert_rows = %lld is below 1", (long long)max_rows);
    else if (!aggmap_slot_count(capacity, max_rows))
        snprintf(reason, 160, "icp_aggmap_create: capacity + max_insert_rows exceeds %lld", (long long)AGGMAP_MAX_ROWS);
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int aggmap_insert_refusals(int64_t n, int64_t max_rows, const double* pose16, int mem, char* reason) {
    reason[0] = 0;
    if (n < 0)
        snprintf(reason, 160, "icp_aggmap_insert: n = %lld is negative", (long long)n);
    else if (n > max_rows)
        snprintf(reason, 160, "icp_aggmap_insert: n = %lld exceeds max_insert_rows = %lld", (long long)n, (long long)max_rows);
    else if (!aggmap_pose_finite(pose16))
        snprintf(reason, 160, "icp_aggmap_insert: the pose has a non-finite entry");
    else if (!aggmap_mem_ok(mem))
        snprintf(reason, 160, "icp_aggmap_insert: host or device memory");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int aggmap_submap_refusals(int32_t frame_lo, int32_t frame_hi, const double* pose16, int out_mem, char* reason) {
    reason[0] = 0;
    if (frame_lo > frame_hi)
        snprintf(reason, 160, "icp_aggmap_submap: frame_lo = %d is above frame_hi = %d", (int)frame_lo, (int)frame_hi);
    else if (!aggmap_pose_finite(pose16))
        snprintf(reason, 160, "icp_aggmap_submap: the pose has a non-finite entry");
    else if (!aggmap_mem_ok(out_mem))
        snprintf(reason, 160, "icp_aggmap_submap: host or device memory");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int aggmap_get_refusals(int out_mem, char* reason) {
    reason[0] = 0;
    if (!aggmap_mem_ok(out_mem)) snprintf(reason, 160, "icp_aggmap_get: host or device memory");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

}  // namespace icp
