// Who does what in one step of icp_batch_pmap_frame_launch / icp_batch_pmap_frame_end (batch_pmap_frame.hip), and what the
// calls refuse: plain C++ without a HIP dependency, so that it also builds into a stand-alone program under the host sanitizers
// (tests/native/batch_pmap_frame_plan_check.cpp).  The projective counterpart of batch_frame_plan.h, which stays as it is (its
// update list and member mask serve both).  In: per member the skip flag, the frame index, the settings of its projective
// sequence, its frame and the state flags of its context.  Out: the members that sit out, the members on their first frame and
// the members that register — or the first member that cannot take part, and why.
#pragma once
#include <stdint.h>
#include <stdio.h>

namespace icp {

constexpr int BATCH_PMAP_FRAME_MAX_MEMBERS = 32;  // ICP_BATCH_MAX_SEQUENCES

struct BatchPmapFrameMember {
    int32_t skip;            // icp_batch_frame.skip
    int32_t has_sequence;    // icp_pmap_odometry_init has run on the context
    int32_t kd_sequence;     // icp_odometry_init has (the context runs the kd-tree frame loop)
    int32_t frame_index;     // frames completed since icp_pmap_odometry_init
    double voxel_size;       // icp_pmap_frame_config.voxel_size
    int32_t targets;         // icp_pmap_frame_config.targets
    int32_t normals_kernel_size;
    int32_t point_to_point;  // the context's cost is ICP_COST_POINT_TO_POINT
    int32_t exchange;        // a multi-GPU exchange is switched on
    int32_t profiling;       // profiling is switched on
    int32_t registering;     // in a registration, or one awaits its end, or a batch holds iterations back
    int32_t frame_launched;  // a frame of its own awaits icp_pmap_frame_end
    int32_t has_timestamps;  // the frame handed in carries timestamps
    int64_t n;               // its rows (vertex-map layout: its pixels)
    int64_t pixels;          // H * W of the context
    uint64_t stream;         // the stream it enqueues on
};

struct BatchPmapFramePlan {
    int32_t n_skipped, n_first, n_registering;
    int32_t skipped[BATCH_PMAP_FRAME_MAX_MEMBERS];      // member indices, ascending
    int32_t first[BATCH_PMAP_FRAME_MAX_MEMBERS];        // frame index 0: no registration
    int32_t registering[BATCH_PMAP_FRAME_MAX_MEMBERS];  // frame index >= 1
    int32_t vertex_map;                                 // the step's layout
    int32_t refused_member;                             // -1: the refusal concerns the call, not one member
    char reason[160];                                   // empty: the step may run
};

inline bool batch_pmap_frame_refuse(BatchPmapFramePlan* plan, int member, const char* reason) {
    plan->n_skipped = plan->n_first = plan->n_registering = 0;
    plan->refused_member = member;
    snprintf(plan->reason, sizeof(plan->reason), "%s", reason);
    return false;
}

// false: refused (plan->refused_member, plan->reason; the lists are empty).  Every member is looked at before the lists are
// handed out: a refusal changes nothing.  vertex_map: the step's layout is ICP_FRAME_VERTEX_MAP; host: its frames are host arrays.
inline bool batch_pmap_frame_plan(const BatchPmapFrameMember* members, int count, bool step_pending, bool vertex_map, bool host,
                                  BatchPmapFramePlan* plan) {
    plan->n_skipped = plan->n_first = plan->n_registering = 0;
    plan->vertex_map = vertex_map ? 1 : 0;
    plan->refused_member = -1;
    plan->reason[0] = 0;
    if (!members || count < 1 || count > BATCH_PMAP_FRAME_MAX_MEMBERS)
        return batch_pmap_frame_refuse(plan, -1, "1 to 32 members are required");
    if (step_pending) return batch_pmap_frame_refuse(plan, -1, "a step is already launched (icp_batch_pmap_frame_end first)");
    if (vertex_map && host) return batch_pmap_frame_refuse(plan, -1, "vertex maps are taken from device memory");
    int lead = -1;  // the first member that takes part: the others share its settings and stream
    for (int b = 0; b < count; ++b) {
        const BatchPmapFrameMember& m = members[b];
        if (m.skip) continue;
        if (m.kd_sequence) return batch_pmap_frame_refuse(plan, b, "a kd-tree sequence (icp_odometry_init) runs on the member");
        if (!m.has_sequence)
            return batch_pmap_frame_refuse(plan, b, "no sequence (icp_batch_pmap_odometry_init or icp_pmap_odometry_init first)");
        if (m.frame_index < 0) return batch_pmap_frame_refuse(plan, b, "invalid frame index");
        if (m.point_to_point)
            return batch_pmap_frame_refuse(plan, b, "the member runs point-to-point (the projective map registers point-to-plane)");
        if (m.exchange) return batch_pmap_frame_refuse(plan, b, "a multi-GPU exchange is switched on");
        if (m.profiling) return batch_pmap_frame_refuse(plan, b, "profiling is switched on");
        if (m.registering) return batch_pmap_frame_refuse(plan, b, "a registration of the member's own is in progress or awaits its end");
        if (m.frame_launched) return batch_pmap_frame_refuse(plan, b, "a frame of the member's own awaits icp_pmap_frame_end");
        if (m.n < 0 || m.n > INT32_MAX) return batch_pmap_frame_refuse(plan, b, "invalid row count");
        if (vertex_map && m.n != m.pixels) return batch_pmap_frame_refuse(plan, b, "a vertex map has n = H*W pixels");
        if (vertex_map && (m.has_timestamps || m.voxel_size > 0))
            return batch_pmap_frame_refuse(plan, b, "timestamps and a grid sample (voxel_size > 0) go with rows, not with a vertex map");
        if (lead < 0) {
            lead = b;
            continue;
        }
        const BatchPmapFrameMember& l = members[lead];
        if (m.voxel_size != l.voxel_size && !(m.voxel_size <= 0 && l.voxel_size <= 0))
            return batch_pmap_frame_refuse(plan, b, "voxel_size differs from the other members' (one batched preprocessing per step)");
        if (!vertex_map && m.targets != l.targets)
            return batch_pmap_frame_refuse(plan, b, "targets differs from the other members' (one target mode per step)");
        if (m.normals_kernel_size != l.normals_kernel_size)
            return batch_pmap_frame_refuse(plan, b, "normals_kernel_size differs from the other members' (one batched map update per step)");
        if (m.pixels != l.pixels) return batch_pmap_frame_refuse(plan, b, "the members must share height and width");
        if (m.stream != l.stream) return batch_pmap_frame_refuse(plan, b, "the members must enqueue on one stream (icp_batch_set_stream)");
    }
    if (lead < 0) return batch_pmap_frame_refuse(plan, -1, "every member is skipped");
    for (int b = 0; b < count; ++b) {
        const BatchPmapFrameMember& m = members[b];
        if (m.skip) plan->skipped[plan->n_skipped++] = b;
        else if (m.frame_index == 0) plan->first[plan->n_first++] = b;
        else plan->registering[plan->n_registering++] = b;
    }
    return true;
}

// icp_batch_pmap_frame_end with nothing launched is refused (nullptr: the step may be ended)
inline const char* batch_pmap_frame_end_refusal(bool step_pending) {
    return step_pending ? nullptr : "no step launched (icp_batch_pmap_frame_launch first)";
}

}  // namespace icp
