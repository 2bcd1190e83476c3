// What the units that read an aggregated world map share (aggmap.hip builds and serves it; elevation.hip rasterises a frame
// window of it): the records of the table, the pose rows and their float64 arithmetic, and the map object itself.
#pragma once
#include "aggmap_plan.h"
#include "icp_internal.h"

namespace icp {

static constexpr int AGG_NEW = -1;       // the slot's voxel is not numbered yet (free slot, or claimed by the insert in progress)
static constexpr int AGG_UNSTORED = -2;  // claimed beyond the capacity: never stored

struct AggSlot {
    int cand;       // smallest row of the creating insert in this voxel (INT_MAX: none yet)
    int idx;        // stored index, AGG_NEW or AGG_UNSTORED
    unsigned hits;  // rows that fell into the voxel
    int last;       // largest frame id among them
};

struct AggPose {
    double m[12];  // rows 0-2 of the 4x4 pose
};

struct AggCounters {
    int size[2];  // stored points: the cell of the current parity is valid, the emit launch writes the other one
    int error;
    int sub_count;  // rows of the last submap
    unsigned long long dropped, out_of_range, nonfinite;
    unsigned long long pad[4];
};
static_assert(sizeof(AggCounters) == 72, "AggCounters layout");

__device__ __forceinline__ double agg_world(const AggPose& p, int r, double x, double y, double z) {
    return __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(p.m[4 * r], x), __dmul_rn(p.m[4 * r + 1], y)), __dmul_rn(p.m[4 * r + 2], z)),
                     p.m[4 * r + 3]);
}

}  // namespace icp

struct icp_aggmap {
    icp_ctx* ctx = nullptr;
    double voxel = 0.0;
    int64_t capacity = 0, max_rows = 0;
    uint64_t slots = 0;
    int64_t inserts = 0;
    int parity = 0;                      // the size cell the next launch reads
    unsigned long long* keys = nullptr;  // [slots]
    icp::AggSlot* meta = nullptr;             // [slots]
    double* pts = nullptr;               // [capacity][3]
    int* first_frame = nullptr;          // [capacity]
    int* slot_of = nullptr;              // [capacity]
    int* row_slot = nullptr;             // [max_rows]
    int* counts = nullptr;               // [AGGMAP_MAX_BLOCKS + 1]
    icp::AggCounters* cnt = nullptr;
    float* stage_dev = nullptr;          // [max_rows][3]: host rows on their way in (allocated by the first host insert)
    float* stage_host = nullptr;         // ... pinned
    hipEvent_t stage_copied = nullptr;   // the last host insert's copy has left the pinned buffer
    icp::AggCounters* cnt_host = nullptr;     // pinned
    icp::DeviceBuffer out_xyz, out_a, out_b, out_c;  // outputs bound for host memory
};
