// Who does what in one step of icp_batch_frame_launch / icp_batch_frame_end (batch_frame.hip), and what the calls refuse:
// plain C++ without a HIP dependency, so that it also builds into a stand-alone program under the host sanitizers
// (tests/native/batch_frame_plan_check.cpp).  In: per member the skip flag, the frame index, the settings of its sequence and
// the state flags of its context.  Out: the members that sit out, the members on their first frame and the members that
// register — or the first member that cannot take part, and why; behind the registrations, the members whose map is updated.
#pragma once
#include <stdint.h>
#include <stdio.h>

namespace icp {

constexpr int BATCH_FRAME_MAX_MEMBERS = 32;  // ICP_BATCH_MAX_SEQUENCES

struct BatchFrameMember {
    int32_t skip;            // icp_batch_frame.skip
    int32_t has_sequence;    // icp_odometry_init has run on the context
    int32_t frame_index;     // frames completed since then
    double voxel_size;       // icp_frame_config.voxel_size
    int32_t targets;         // icp_frame_config.targets
    int32_t point_to_point;  // the context's cost is ICP_COST_POINT_TO_POINT
    int32_t projective_map;  // it holds a projective map
    int32_t exchange;        // a multi-GPU exchange is switched on
    int32_t profiling;       // profiling is switched on
    int32_t registering;     // in a registration, or one awaits its icp_register_end / icp_batch_register_end
    int32_t frame_launched;  // a frame of its own awaits icp_frame_end
    uint64_t stream;         // the stream it enqueues on
};

struct BatchFramePlan {
    int32_t n_skipped, n_first, n_registering;
    int32_t skipped[BATCH_FRAME_MAX_MEMBERS];      // member indices, ascending
    int32_t first[BATCH_FRAME_MAX_MEMBERS];        // frame index 0: no registration
    int32_t registering[BATCH_FRAME_MAX_MEMBERS];  // frame index >= 1
    int32_t refused_member;                        // -1: the refusal concerns the call, not one member
    char reason[160];                              // empty: the step may run
};

inline bool batch_frame_refuse(BatchFramePlan* plan, int member, const char* reason) {
    plan->n_skipped = plan->n_first = plan->n_registering = 0;
    plan->refused_member = member;
    snprintf(plan->reason, sizeof(plan->reason), "%s", reason);
    return false;
}

// false: refused (plan->refused_member, plan->reason; the lists are empty).  Every member is looked at before the lists are
// handed out: a refusal changes nothing.
inline bool batch_frame_plan(const BatchFrameMember* members, int count, bool step_pending, BatchFramePlan* plan) {
    plan->n_skipped = plan->n_first = plan->n_registering = 0;
    plan->refused_member = -1;
    plan->reason[0] = 0;
    if (!members || count < 1 || count > BATCH_FRAME_MAX_MEMBERS) return batch_frame_refuse(plan, -1, "1 to 32 members are required");
    if (step_pending) return batch_frame_refuse(plan, -1, "a step is already launched (icp_batch_frame_end first)");
    int lead = -1;  // the first member that takes part: the others share its voxel_size, targets and stream
    for (int b = 0; b < count; ++b) {
        const BatchFrameMember& m = members[b];
        if (m.skip) continue;
        if (!m.has_sequence) return batch_frame_refuse(plan, b, "no sequence (icp_batch_odometry_init or icp_odometry_init first)");
        if (m.frame_index < 0) return batch_frame_refuse(plan, b, "invalid frame index");
        if (m.point_to_point) return batch_frame_refuse(plan, b, "the member runs point-to-point (the batch registers point-to-plane only)");
        if (m.projective_map) return batch_frame_refuse(plan, b, "the member holds a projective map (the frame calls run the kd-tree style map)");
        if (m.exchange) return batch_frame_refuse(plan, b, "a multi-GPU exchange is switched on");
        if (m.profiling) return batch_frame_refuse(plan, b, "profiling is switched on");
        if (m.registering) return batch_frame_refuse(plan, b, "a registration of the member's own is in progress or awaits its end");
        if (m.frame_launched) return batch_frame_refuse(plan, b, "a frame of the member's own awaits icp_frame_end");
        if (lead < 0) {
            lead = b;
            continue;
        }
        const BatchFrameMember& l = members[lead];
        if (m.voxel_size != l.voxel_size && !(m.voxel_size <= 0 && l.voxel_size <= 0))
            return batch_frame_refuse(plan, b, "voxel_size differs from the other members' (one batched preprocessing per step)");
        if (m.targets != l.targets) return batch_frame_refuse(plan, b, "targets differs from the other members' (one target mode per step)");
        if (m.stream != l.stream) return batch_frame_refuse(plan, b, "the members must enqueue on one stream (icp_batch_set_stream)");
    }
    if (lead < 0) return batch_frame_refuse(plan, -1, "every member is skipped");
    for (int b = 0; b < count; ++b) {
        const BatchFrameMember& m = members[b];
        if (m.skip) plan->skipped[plan->n_skipped++] = b;
        else if (m.frame_index == 0) plan->first[plan->n_first++] = b;
        else plan->registering[plan->n_registering++] = b;
    }
    return true;
}

// icp_batch_frame_end with nothing launched is refused (nullptr: the step may be ended)
inline const char* batch_frame_end_refusal(bool step_pending) {
    return step_pending ? nullptr : "no step launched (icp_batch_frame_launch first)";
}

// icp_batch_frame_end: the registering members whose registration ended with status 0 get their map updated, in order; the
// others (ICP_ERR_INVALID_JACOBIAN) keep their map and their place in the sequence.  statuses[i] belongs to registering[i].
// Returns the number of members written to update[]; *first_status: the first non-zero status (0: none).
inline int batch_frame_update_members(const int32_t* registering, const int32_t* statuses, int n_registering, int32_t* update,
                                      int32_t* first_status) {
    int n = 0;
    if (first_status) *first_status = 0;
    for (int i = 0; i < n_registering; ++i) {
        if (statuses[i] == 0) update[n++] = registering[i];
        else if (first_status && *first_status == 0) *first_status = statuses[i];
    }
    return n;
}

// the member mask of a subset (the key of the inner batches partial steps run on)
inline uint32_t batch_frame_mask(const int32_t* members, int n) {
    uint32_t mask = 0;
    for (int i = 0; i < n; ++i) mask |= (uint32_t)1 << (members[i] & 31);
    return mask;
}

}  // namespace icp
