// The state of a batch's frame calls and what the kd-tree form (batch_frame.hip) and the projective form
// (batch_pmap_frame.hip) share, all of it in batch_frame.hip: the inner batches by member mask, the ONE upload stream / pinned
// arena / pair of device arenas, the batched preprocessing, the ONE copy-out stream and pinned arena, the two ends of a
// launch, the dropping of a pending step and the whole end call.  A form describes itself in a BatchFrameKind.
#pragma once
#include <string.h>

#include <map>
#include <string>

#include "batch_frame_plan.h"
#include "batch_pmap_frame_plan.h"
#include "frame_loop.h"
#include "icp_internal.h"

namespace icp {

// what both loops have: a member's sequence state, its way in and out, its key-frame thresholds
struct BatchFrameMemberLoop {
    icp_frame_seq* seq;  // null: the member has no sequence of this kind
    icp_frame_io* io;
    float threshold_trans, threshold_rot;
};

// what the shared code needs to know of a form: its names for the messages, the way to a member's loop, and its own steps
struct BatchFrameKind {
    const char* launch_name;  // "icp_batch_frame_launch"
    const char* end_name;     // "icp_batch_frame_end"
    BatchFrameMemberLoop (*loop)(icp_ctx* ctx);  // the member's loop of this kind
    void (*forget_pose)(icp_ctx* ctx);  // the member's registration failed or was dropped (null: nothing to forget)
    // frame 0 of a member, rows on the device: the single launch, and the single end call
    int (*first_launch)(icp_ctx* ctx, const float* rows, int64_t n, int layout, const double* ts, const float init_pose[16]);
    int (*single_end)(icp_ctx* ctx, icp_frame_result* result, float* odometry_pc_out, int64_t cap, int64_t* rows_out, int out_mem,
                      double* loss_per_iter_out, float* dx_per_iter_out);
    // ONE batched map update on `ub` (its members: ctxs[0..nu)): rel [nu,16], the key-frame tests; inserted[u] receives what
    // icp_frame_result.inserted reports for a key frame
    int (*update)(icp_batch* ub, icp_ctx* const* ctxs, int nu, const float* rel, const KeyFrameTest* tests, int64_t* inserted);
    const char* (*end_refusal)(bool step_pending);
};

// who takes part in a launched step: the lists of BatchFramePlan / BatchPmapFramePlan
struct BatchFrameStep {
    int32_t n_first = 0, n_registering = 0;
    int32_t first[ICP_BATCH_MAX_SEQUENCES];
    int32_t registering[ICP_BATCH_MAX_SEQUENCES];
};

}  // namespace icp

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
    // ---- the step between a launch and its end (pending: its kind; null: none)
    const icp::BatchFrameKind* pending = nullptr;
    icp::BatchFrameStep step;
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
                            icp_ctx* const* ctxs, icp_frame_io* const* ios, double voxel_size, const float* const* guess,
                            const bool* have_guess, const double* const* ts, const float** r_rows, const int64_t* r_n);
int batch_frames_copy_start(icp_batch* b, icp_batch_frames* s, const int32_t* reg, int nr, icp_ctx* const* ctxs,
                            icp_frame_io* const* ios, const bool* cloud, const int64_t* r_n);
int batch_frames_arena_read(icp_batch* b, icp_batch_frames* s, hipStream_t stream);
// a step launched and never ended: its registrations are collected and dropped, its copies waited for (only: of that kind)
void batch_frames_drop_pending(icp_batch* b, const BatchFrameKind* only = nullptr);
// ---- the two ends of a launch, around the target-building middle of each form
struct BatchFrameLaunch {
    icp_batch* rb = nullptr;  // the batch over the registering members
    icp_ctx* lead = nullptr;
    hipStream_t stream = nullptr;
    const float* rows[ICP_BATCH_MAX_SEQUENCES] = {};  // per member, on the device
    const double* ts[ICP_BATCH_MAX_SEQUENCES] = {};
    bool uploaded = false;
};
// the batch over the registering members, ONE upload for every member that takes part, then the first frames member by member
int batch_frames_launch_begin(icp_batch* b, const BatchFrameKind& kind, const BatchFrameStep& step, const icp_batch_frame* frames,
                              int mem, int layout, BatchFrameLaunch* l);
// the first frames are complete: ended here, as the single end call would (a failure behind them)
void batch_frames_end_first(icp_batch* b, const BatchFrameKind& kind, const BatchFrameStep& step, int upto);
// the step is launched: the first members are the batch's, the arena's readers are marked, the step is stored
int batch_frames_launch_finish(icp_batch* b, const BatchFrameKind& kind, const BatchFrameStep& step, const BatchFrameLaunch& l);
// a HIP call on behalf of one member failed
int bf_member_hip(icp_batch* b, const char* who, int member, hipError_t e, const char* what);
// the launch's host guesses, [n,16]: the member's guess, or the identity where it has none
void batch_frames_init_poses(const float* const* guess, const bool* have_guess, int n, float* init);
// BatchFramePlan / BatchPmapFramePlan: the lists of a plan that may run, the message of one that was refused
template <class Plan>
BatchFrameStep batch_frame_step(const Plan& plan) {
    BatchFrameStep step;
    step.n_first = plan.n_first;
    step.n_registering = plan.n_registering;
    memcpy(step.first, plan.first, sizeof(step.first));
    memcpy(step.registering, plan.registering, sizeof(step.registering));
    return step;
}
template <class Plan>
int batch_frames_refuse(icp_batch* b, const char* who, const Plan& plan) {
    std::string msg = std::string(who);
    if (plan.refused_member >= 0) msg += ", member " + std::to_string(plan.refused_member);
    return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, msg + ": " + plan.reason + " (nothing was changed)");
}
// icp_batch_frame_end / icp_batch_pmap_frame_end
int batch_frames_end(icp_batch* b, const BatchFrameKind& kind, icp_frame_result* results, float* const* odometry_pc_out,
                     const int64_t* cap, int64_t* rows_out, int out_mem, double* loss_per_iter_out, float* dx_per_iter_out);
// the two forms (batch_frame.hip, batch_pmap_frame.hip)
const BatchFrameKind& batch_frame_kd();
const BatchFrameKind& batch_frame_pmap();

}  // namespace icp
