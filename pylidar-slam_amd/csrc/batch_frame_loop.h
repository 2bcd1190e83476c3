// The state of a batch's frame calls (batch_frame.hip, batch_pmap_frame.hip) and the stages the kd-tree and the projective
// form share: the inner batches by member mask, the ONE upload stream / pinned arena / pair of device arenas, the batched
// preprocessing and the ONE copy-out stream and pinned arena.
#pragma once
#include <map>
#include <string>

#include "batch_frame_plan.h"
#include "batch_pmap_frame_plan.h"
#include "frame_loop.h"
#include "icp_internal.h"

struct icp_batch_frames {
    // member mask -> a batch over those members (the full mask: the batch itself).  Bounded: a serving loop whose drives end,
    // start and fail in arbitrary slots meets ever new masks, and every inner batch owns pinned descriptor slots, device tables
    // and events — beyond INNER_MAX of them the least recently used one is destroyed (one device synchronisation; a mask that
    // comes back is created again)
    static constexpr size_t INNER_MAX = 8;
    struct Inner {
        icp_batch* batch;
        uint64_t used;
    };
    std::map<uint32_t, Inner> inner;
    uint64_t tick = 0;
    // ---- the step between icp_batch_frame_launch and icp_batch_frame_end
    bool pending = false;
    icp::BatchFramePlan plan;
    int mem = ICP_MEM_DEVICE;
    int64_t n[ICP_BATCH_MAX_SEQUENCES] = {};
    bool sampled[ICP_BATCH_MAX_SEQUENCES] = {};
    bool copied[ICP_BATCH_MAX_SEQUENCES] = {};     // the member's staged rows are on their way to pin_out
    size_t out_offset[ICP_BATCH_MAX_SEQUENCES] = {};  // ... at this offset
    bool copy_started = false;
    // ---- input: ONE pinned arena -> one of two device arenas, on ONE upload stream, whatever the member count
    void* pin_in = nullptr;
    size_t pin_in_bytes = 0;
    hipEvent_t pin_in_free = nullptr;
    bool pin_in_busy = false;
    icp::DeviceBuffer arena[2];
    hipEvent_t arena_read[2] = {nullptr, nullptr};  // the step that read the arena last has been enqueued up to here
    bool arena_used[2] = {false, false};
    int which = 0;
    hipStream_t upload_stream = nullptr;
    // ---- odometry_pc and the sample counts: ONE copy stream, ONE pinned arena (the counts lead it)
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_done = nullptr;
    void* pin_out = nullptr;
    size_t pin_out_bytes = 0;
    int* pin_counts = nullptr;  // [ICP_BATCH_MAX_SEQUENCES]
    // ---- the projective step between icp_batch_pmap_frame_launch and icp_batch_pmap_frame_end (batch_pmap_frame.hip)
    bool p_pending = false;
    icp::BatchPmapFramePlan p_plan;
};


namespace icp {

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
int bf_fail(icp_batch* b, int code, const std::string& msg);
int bf_hip(icp_batch* b, hipError_t e, const char* what);
#define BF_HIP(b, expr)                               \
    do {                                              \
        const int _rc = bf_hip((b), (expr), #expr);   \
        if (_rc) return _rc;                          \
    } while (0)
int bf_member_fail(icp_batch* b, int rc, const char* who, int member);
int pinned_reserve(icp_batch* b, void** ptr, size_t* have, size_t need);
icp_batch_frames* frames_of(icp_batch* b);
// the batch over `members` (indices into b->members, ascending): b itself for all of them, an inner batch (an LRU of 8) otherwise
int subset_batch(icp_batch* b, const int32_t* members, int n, icp_batch** out);
int inner_fail(icp_batch* b, icp_batch* inner, int rc);
int upload(icp_batch* b, icp_batch_frames* s, const icp_batch_frame* frames, const int32_t* who, int n_who, hipStream_t stream,
           const float** rows, const double** ts);
int batch_frames_preprocess(icp_batch* b, icp_batch* rb, icp_batch_frames* s, const char* who, const int32_t* reg, int nr,
                            icp_ctx* const* ctxs, icp_frame_loop* const* loops, double voxel_size, const float* const* guess,
                            const bool* have_guess, const double* const* ts, const float** r_rows, const int64_t* r_n);
int batch_frames_copy_start(icp_batch* b, icp_batch_frames* s, const int32_t* reg, int nr, icp_ctx* const* ctxs,
                            icp_frame_loop* const* loops, const bool* cloud, const int64_t* r_n);
int batch_frames_arena_read(icp_batch* b, icp_batch_frames* s, hipStream_t stream);
// a projective step launched and never ended is collected and dropped (batch_pmap_frame.hip; batch_frames_release calls it)
void batch_pmap_drop_pending(icp_batch* b);

}  // namespace icp
