// C ABI of libicp_mi355x.so, B sequences per launch (include/icp_mi355x.h: icp_batch_*).  Host code only: every kernel it
// enqueues lives in the unit of its single-context twin.
// (the entry points take their C linkage from their declarations in include/icp_mi355x.h)
#include <string.h>

#include <string>
#include <vector>

#include "icp_internal.h"
#include "map_move_device.h"
#include "register_plan.h"

using namespace icp;

// ---- the registration ----------------------------------------------------------------------------------------------------
// The descriptor tables of ONE frame — iteration launch after iteration launch, [count] entries each, the summing / solving
// launches in between — are filled in pinned host memory while the frame's launches are PREPARED (all host bookkeeping of
// all iterations of all members first: nothing in it depends on a launch having been issued), travel to the device in one
// copy, and the launches follow.  Three slots in rotation: a slot is rewritten when the registration two frames back has been
// collected (at most two registrations are ever pending per member), so its launches have long finished.
// (struct icp_batch: icp_internal.h — batch_frame.hip composes the entry points below over subsets of its members)

static int batch_fail(icp_batch* b, int code, const std::string& msg) {
    if (b) b->error = msg;
    return code;
}

// a batched registration that could not be enqueued to its end is given up: nothing is held back any more, no member is "in
// registration" or refuses the single-context entry points
static void batch_abandon(icp_batch* b) {
    b->run_active = false;
    b->run_next = b->run_iters;
    for (icp_ctx* ctx : b->members) {
        ctx->batch_hold = false;
        ctx->in_registration = false;
        result_fold_reset(ctx);
    }
}

// what the batched launches leave behind on an error: no member "in registration" or held by the batch (batch_abandon) —
// and, leave_count, no member without a pending result counted among the registering contexts of the device
namespace {
struct BatchUnwind {
    icp_batch* b;
    bool leave_count;
    bool armed = true;
    ~BatchUnwind() {
        if (!armed) return;
        batch_abandon(b);
        if (!leave_count) return;
        for (icp_ctx* ctx : b->members)
            if (ctx->r_count == 0) registering_leave(ctx);
    }
};
}  // namespace

static int batch_hip(icp_batch* b, icp_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return ICP_OK;
    ctx->error = std::string(what) + ": " + hipGetErrorString(e);
    return batch_fail(b, ICP_ERR_HIP, ctx->error);
}

// a filled descriptor table goes to its device twin in ONE copy on the first member's stream; `copied` (recorded behind it)
// frees the pinned slot for its next user
static int table_send(icp_batch* b, icp::DeviceBuffer& dev, const void* host, size_t bytes, hipEvent_t copied) {
    icp_ctx* first = b->members[0];
    const int rc = batch_hip(b, first, hipMemcpyAsync(dev.ptr, host, bytes, hipMemcpyHostToDevice, first->stream),
                             "hipMemcpyAsync(descriptors)");
    return rc ? rc : batch_hip(b, first, hipEventRecord(copied, first->stream), "hipEventRecord(copied)");
}

// the next of the batch's two `done` events, created on first use: ONE event behind the results of a batched registration
static int done_event_take(icp_batch* b, int* index_out) {
    *index_out = b->done_next;
    b->done_next ^= 1;
    hipEvent_t& done = b->done[*index_out];
    return done ? ICP_OK : batch_hip(b, b->members[0], hipEventCreateWithFlags(&done, hipEventDisableTiming), "hipEventCreate(done)");
}

int icp_batch_create(icp_ctx* const* ctxs, int32_t count, icp_batch** out) {
    if (!ctxs || !out || count < 1 || count > ICP_BATCH_MAX_SEQUENCES) return ICP_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    for (int i = 0; i < count; ++i) {
        if (!ctxs[i] || ctxs[i]->cfg.device != ctxs[0]->cfg.device) return ICP_ERR_INVALID_ARGUMENT;
        for (int j = 0; j < i; ++j)
            if (ctxs[j] == ctxs[i]) return ICP_ERR_INVALID_ARGUMENT;
    }
    icp_batch* b = new icp_batch();
    b->members.assign(ctxs, ctxs + count);
    b->device = ctxs[0]->cfg.device;
    *out = b;
    return ICP_OK;
}

void icp_batch_destroy(icp_batch* b) {
    if (!b) return;
    DeviceGuard device_guard(b->device);
    batch_frames_release(b);  // (a step launched and never ended is collected and dropped; the inner batches of partial steps)
    (void)hipDeviceSynchronize();  // (launches that read the tables; members whose result slots wait for the batch's events)
    for (icp_ctx* ctx : b->members) {
        ctx->batch_hold = false;  // (iterations the batch still held back are dropped: the members' results stand as they are)
        for (auto& r : ctx->rslot)
            if (r.wait == b->done[0] || r.wait == b->done[1]) r.wait = r.event;
    }
    for (int k = 0; k < icp_batch::SLOTS; ++k) {
        if (b->host[k]) (void)hipHostFree(b->host[k]);
        b->dev[k].release();
        if (b->copied[k]) (void)hipEventDestroy(b->copied[k]);
        if (b->grid_host[k]) (void)hipHostFree(b->grid_host[k]);
        b->grid_dev[k].release();
        if (b->grid_copied[k]) (void)hipEventDestroy(b->grid_copied[k]);
    }
    for (auto& e : b->done)
        if (e) (void)hipEventDestroy(e);
    delete b;
}

const char* icp_batch_last_error(const icp_batch* b) { return b ? b->error.c_str() : "null batch"; }

int icp_batch_set_stream(icp_batch* b, void* hip_stream) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    for (icp_ctx* ctx : b->members) {
        const int rc = icp_set_stream(ctx, hip_stream);
        if (rc) return batch_fail(b, rc, ctx->error);
    }
    return ICP_OK;
}

// the next pinned descriptor slot (and its device twin) with room for `need` bytes, free to be rewritten: its copy has left
static int table_slot_take(icp_batch* b, size_t need, int* slot_out) {
    icp_ctx* first = b->members[0];
    const int slot = b->slot;
    b->slot = (slot + 1) % icp_batch::SLOTS;
    if (b->host_bytes[slot] < need) {
        if (b->copied[slot]) ICP_HIP(first, hipEventSynchronize(b->copied[slot]));
        if (b->host[slot]) (void)hipHostFree(b->host[slot]);
        b->host[slot] = nullptr;
        b->host_bytes[slot] = 0;
        ICP_HIP(first, hipHostMalloc((void**)&b->host[slot], need, hipHostMallocDefault));
        b->host_bytes[slot] = need;
    }
    ICP_HIP(first, b->dev[slot].reserve(need));
    if (!b->copied[slot]) ICP_HIP(first, hipEventCreateWithFlags(&b->copied[slot], hipEventDisableTiming));
    else ICP_HIP(first, hipEventSynchronize(b->copied[slot]));  // (three chunks ago: long past)
    *slot_out = slot;
    return ICP_OK;
}

// Enqueues the next `chunk` iterations of the batch's registration in progress (all that are left when chunk < 0): their
// descriptor tables into a fresh pinned slot, one copy, the launches; behind the chunk's last iteration a summing / solving
// launch that also delivers every member's result block; ONE event behind it all.  `packs` (first chunk only): the target
// packing / state initialisation of the members, run in front.
static int batch_enqueue(icp_batch* b, int chunk, const PackDesc* packs, bool first_chunk) {
    const int count = (int)b->members.size();
    icp_ctx* const* ctxs = b->members.data();
    icp_ctx* first = ctxs[0];
    const int left = b->run_iters - b->run_next;
    if (chunk < 0 || chunk > left) chunk = left;
    if (chunk <= 0) return ICP_OK;
    const int it_begin = b->run_next, it_end = it_begin + chunk;
    const bool lead = b->run_lead;
    const BatchRegisterLayout lay(sizeof(PackDesc), iterate_desc_bytes(), sum_solve_desc_bytes(), count);  // the packing launch's table leads the slot
    int slot = 0;
    int rc = table_slot_take(b, lay.need(chunk), &slot);
    if (rc) return batch_fail(b, rc, first->error);
    for (int i = 0; i < count; ++i) {
        ctxs[i]->in_registration = true;
        if ((rc = result_fold_begin(ctxs[i], !first_chunk))) return batch_fail(b, rc, ctxs[i]->error);
    }
    struct Op {
        int kind;  // 0: fused iteration, 1: sum + solve
        size_t offset;
        BatchedIteration it;
    };
    std::vector<Op> ops;
    ops.reserve(2 * (size_t)chunk);
    if (packs) memcpy(b->host[slot], packs, sizeof(PackDesc) * (size_t)count);
    size_t used = lay.first_table();
    for (int it = it_begin; it < it_end; ++it) {
        Op op{0, used, BatchedIteration()};
        if ((rc = prepare_iterate_batch(ctxs, count, lead, b->run_prev_rows, b->run_prev_quad, b->host[slot] + used, &op.it))) {
            for (int i = 0; i < count; ++i)
                if (!ctxs[i]->error.empty()) b->error = ctxs[i]->error;
            return rc;
        }
        used += lay.it_bytes;
        ops.push_back(op);
        bool solve = true;
        if (lead) {  // (as enqueue_iterations: the narrow launches solve the iteration before them themselves)
            for (int i = 0; i < count; ++i) {
                b->run_prev_rows[i] = op.it.rows[i];
                b->run_prev_quad[i] = op.it.quad[i];
            }
            solve = it + 1 == it_end || !next_fused_launch_is_narrow(first) || (op.it.quad[0] && !first->lead_after_dense);
        }
        if (solve) {
            Op so{1, used, BatchedIteration()};
            if ((rc = prepare_sum_solve_batch(ctxs, count, op.it.rows, op.it.quad, lead, it + 1 == it_end, b->host[slot] + used)))
                return batch_fail(b, rc, "batched registration: sum + solve");
            used += lay.ss_bytes;
            ops.push_back(so);
            for (int i = 0; i < count; ++i) b->run_prev_rows[i] = 0;
        }
    }
    b->run_next = it_end;
    // ---- one copy, then the launches
    if ((rc = table_send(b, b->dev[slot], b->host[slot], used, b->copied[slot]))) return rc;
    if (packs && (rc = launch_pack_targets_batch(first, packs, b->dev[slot].as<PackDesc>(), count))) return batch_fail(b, rc, first->error);
    for (const Op& op : ops) {
        const char* table = b->dev[slot].as<char>() + op.offset;
        rc = op.kind == 0 ? launch_iterate_batch(first, op.it, table) : launch_sum_solve_batch(first, count, table);
        if (rc) return batch_fail(b, rc, first->error);
    }
    // ---- the results: every member's block lands in its own pinned slot (written by the chunk's last solving launch), ONE
    // event; further chunks of the same registration record the same event again
    if (first_chunk && (rc = done_event_take(b, &b->run_done))) return rc;
    hipEvent_t done = b->done[b->run_done];
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        ctx->batch_hold = it_end < b->run_iters;
        // (nothing "remains" for the member: what the batch still holds back is the batch's, run_next .. run_iters)
        if ((rc = result_hand_over(ctx, ICP_OK, it_end, 0, !first_chunk, done))) return batch_fail(b, rc, ctx->error);
    }
    ICP_HIP(first, hipEventRecord(done, first->stream));
    if (it_end >= b->run_iters) b->run_active = false;
    return ICP_OK;
}

// everything the batch still holds back goes onto the stream (a map update by the device-resident poses, another launch, the
// destruction of the batch follow the WHOLE registration)
static int batch_flush(icp_batch* b) {
    if (!b->run_active) return ICP_OK;
    const int rc = batch_enqueue(b, -1, nullptr, false);
    if (rc) batch_abandon(b);
    b->run_active = false;
    for (icp_ctx* ctx : b->members) ctx->batch_hold = false;
    return rc;
}

// What batch_enqueue, prepare_iterate_batch and launch_iterate_batch read from ONE member on behalf of all (the stop
// threshold and "chunked_launch": how many iterations a chunk holds; "lead_after_dense", "wide_until", "narrow_from",
// "nn_cache", "ball_search", "late_from": which shape an iteration runs in and which launch solves it; "hit_records",
// "late_waves": which instantiation is launched) must be equal across the members: include/icp_mi355x.h,
// icp_batch_register_launch.  Checked before any member changes; the message names the option.  Everything else travels in
// the member's own descriptor.
static int batch_shared_options_check(icp_batch* b, const char* what) {
    const icp_ctx* first = b->members[0];
    for (size_t i = 1; i < b->members.size(); ++i) {
        const icp_ctx* ctx = b->members[i];
        const char* name = nullptr;
        if (ctx->cfg.threshold_delta_pose != first->cfg.threshold_delta_pose) name = "threshold_delta_pose";
        else if (ctx->chunked_launch != first->chunked_launch) name = "chunked_launch";
        else if (ctx->lead_after_dense != first->lead_after_dense) name = "lead_after_dense";
        else if (ctx->hit_records != first->hit_records) name = "hit_records";
        else if (ctx->late_from != first->late_from) name = "late_from";
        else if (ctx->late_waves != first->late_waves) name = "late_waves";
        else if (ctx->wide_until != first->wide_until) name = "wide_until";
        else if (ctx->narrow_from != first->narrow_from) name = "narrow_from";
        else if (ctx->use_nn_cache != first->use_nn_cache) name = "nn_cache";
        else if (ctx->ball_search != first->ball_search) name = "ball_search";
        if (name)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, std::string(what) + ", member " + std::to_string(i) + ": the members must share \"" +
                                                              name + "\" (it differs from member 0's; nothing was changed)");
    }
    return ICP_OK;
}

// What the batched map calls, the staging and the collection refuse before any member changes: a member between
// icp_register_begin and icp_register_end (`begun`: its caller drives the iterations — a batched launch that failed on it would
// abandon that registration, an update would rebuild the grid under it), and a member whose OWN frame is launched (its
// icp_frame_end / icp_pmap_frame_end collects that registration, inserts those staged rows, appends to that window).
static int batch_members_free(icp_batch* b, const char* what, bool begun, bool own_frame) {
    for (size_t i = 0; i < b->members.size(); ++i) {
        const icp_ctx* ctx = b->members[i];
        const std::string who = std::string(what) + ", member " + std::to_string(i) + ": ";
        if (begun && ctx->in_registration && !b->run_active)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "registration in progress (nothing was changed)");
        if (own_frame && own_frame_in_flight(ctx))
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "a frame is launched and awaits its end (nothing was changed)");
    }
    return ICP_OK;
}

int icp_batch_register_launch(icp_batch* b, const float* const* xyz, const int64_t* n, int mem, int target_mode,
                              const float* init_poses, int from_last) {
    if (!b || !xyz || !n) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    icp_ctx* const* ctxs = b->members.data();
    icp_ctx* first = ctxs[0];
    const int iters = first->cfg.max_num_alignments;
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        { DeviceGuard join_map_stream(ctx); }
        if (ctx->stream != first->stream)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched registration: the members must enqueue on one stream (icp_batch_set_stream)");
        if (ctx->cfg.max_num_alignments != iters || ctx->cfg.scheme != first->cfg.scheme || ctx->cfg.sigma != first->cfg.sigma)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched registration: the members must share max_num_alignments, scheme and sigma");
        if (ctx->r_count >= 2) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "two results are already pending");
        if (ctx->exchange_on || ctx->prof.enabled || ctx->search_stats || ctx->cost != ICP_COST_POINT_TO_PLANE)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched registration: point-to-plane registrations without exchange, "
                                                          "profiling or search statistics only");
    }
    if (int rc_options = batch_shared_options_check(b, "batched registration")) return rc_options;
    if (int rc_free = batch_members_free(b, "batched registration", true, false)) return rc_free;
    BatchUnwind unwind{b, true};  // (register_begin counts the members among the registering contexts)
    int rc = ICP_OK;
    if ((rc = batch_flush(b))) return rc;  // (iterations of the previous batched registration still held back go first)
    PackDesc packs[ICP_BATCH_MAX_SEQUENCES];
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        if ((rc = continue_launch(ctx, -1))) return batch_fail(b, rc, ctx->error);  // (an older chunked launch of this member goes first)
        if ((rc = register_begin(ctx, xyz[i], n[i], mem, target_mode, (init_poses && !from_last) ? init_poses + 16 * i : nullptr,
                                 from_last != 0, &packs[i])))
            return batch_fail(b, rc, ctx->error);
        // (register_begin has answered for this member alone: the batch answers for all of them below, and counts then)
        ctx->lead_registrations -= ctx->lead_latched ? 1 : 0;
        ctx->lead_latched = false;
        if (!fused_path(ctx) || ctx->lazy_now)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched registration: the fused iteration path with eagerly estimated "
                                                          "normals only (see icp_set_option: fuse_iteration, lazy_fused, eager_normals_limit)");
    }
    // lead launches (every member's solve in the head of the next launch, by a lead workgroup of its own) unless a context
    // OUTSIDE the batch is registering on the device: the members themselves are counted, and are no strangers
    const int d = b->device >= 0 && b->device < 64 ? b->device : 0;
    int counted = 0;
    bool lead = true;
    for (int i = 0; i < count; ++i) {
        counted += ctxs[i]->counted_registering ? 1 : 0;
        lead = lead && ctxs[i]->lead_solve && !ctxs[i]->handoff_disabled;
    }
    lead = lead && g_registering[d].load() <= counted;
    for (int i = 0; i < count; ++i) {
        ctxs[i]->lead_latched = lead;
        ctxs[i]->lead_registrations += lead ? 1 : 0;
    }
    // ---- the iterations: all of them (forced count), or a first chunk — as many as the slowest member ran last time plus one —
    // with a live stop threshold (icp_batch_register_end enqueues more while a member is still running; launches behind
    // every member's stop would be no-ops that still cost their slot on the stream: a hundred of them with the default
    // max_num_alignments)
    int ran[ICP_BATCH_MAX_SEQUENCES];
    for (int i = 0; i < count; ++i) ran[i] = ctxs[i]->last_iterations;
    const int first_chunk = first_chunk_iterations(iters, first->cfg.threshold_delta_pose, first->chunked_launch, false, ran, count);
    b->run_active = true;
    b->run_lead = lead;
    b->run_next = 0;
    b->run_iters = iters;
    for (int i = 0; i < count; ++i) {
        b->run_prev_rows[i] = 0;
        b->run_prev_quad[i] = 1;
    }
    if ((rc = batch_enqueue(b, first_chunk, packs, true))) return rc;
    unwind.armed = false;
    return ICP_OK;
}

int icp_batch_project(icp_batch* b, const float* const* xyz, const int64_t* n, float* const* vmap_out) {
    if (!b || !xyz || !n || !vmap_out) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    for (int i = 0; i < count; ++i)
        if (n[i] < 0 || (n[i] > 0 && !xyz[i]) || !vmap_out[i] || b->members[i]->stream != b->members[0]->stream)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched projection: device pointers, one stream (icp_batch_set_stream)");
    const int rc = project_batch_device(b->members.data(), count, xyz, n, vmap_out);
    if (rc) return batch_fail(b, rc, b->members[0]->error);
    return ICP_OK;
}

// ---- the stage in front of a batched registration: preprocessing, projection, staging -----------------------------------
// What each of these calls asks of its members before anything is enqueued: one stream, no registration in progress
// (icp_register_begin .. icp_register_end).  `join`: the member's stream first waits for a map update running on the map
// stream (as the single entry point the call replaces does).
static int front_batch_check(icp_batch* b, const char* what, bool join) {
    icp_ctx* first = b->members[0];
    for (size_t i = 0; i < b->members.size(); ++i) {
        icp_ctx* ctx = b->members[i];
        if (join) { DeviceGuard join_map_stream(ctx); }
        const std::string who = std::string(what) + ", member " + std::to_string(i) + ": ";
        if (ctx->stream != first->stream)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "the members must enqueue on one stream (icp_batch_set_stream)");
        if (ctx->in_registration) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "registration in progress");
    }
    return ICP_OK;
}

// ... then iterations the batch or a member still holds back go onto the stream first (stream order = call order)
static int front_batch_flush(icp_batch* b) {
    int rc = batch_flush(b);
    if (rc) return rc;
    for (icp_ctx* ctx : b->members)
        if ((rc = continue_launch(ctx, -1)) || (rc = ensure_state(ctx))) return batch_fail(b, rc, ctx->error);
    return ICP_OK;
}

// Distortion -> GridSample(padded) -> ToTensor(float32) (slam/preprocessing.py:144-191, :207-226, :101-126) for B frames
int icp_batch_preprocess(icp_batch* b, const icp_preprocess_frame* frames, double voxel_size) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!frames || !(voxel_size > 0))
        return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched preprocessing: frames[] and a positive voxel size are required");
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    for (int i = 0; i < count; ++i) {
        const icp_preprocess_frame& f = frames[i];
        const std::string who = "batched preprocessing, member " + std::to_string(i) + ": ";
        if (f.n < 0 || f.n > INT32_MAX) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "invalid row count");
        if (!f.count_out) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "count_out is required");
        if (f.n > 0 && (!f.xyz || !f.samples_f32_out))
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "xyz and samples_f32_out are required");
        if (f.n > 0 && f.timestamps && !f.distorted_out)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "a de-skewed frame needs distorted_out");
        if (!f.timestamps && f.distorted_out)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "distorted_out without timestamps");
    }
    int rc = front_batch_check(b, "batched preprocessing", false);
    if (rc || (rc = front_batch_flush(b))) return rc;
    if ((rc = preprocess_batch_device(b->members.data(), count, frames, voxel_size))) {
        for (icp_ctx* ctx : b->members)
            if (!ctx->error.empty()) return batch_fail(b, rc, ctx->error);
        return batch_fail(b, rc, "batched preprocessing: HIP error");
    }
    return ICP_OK;
}

// estimate_timestamps (slam/common/geometry.py:443-466) for every member in two launches
int icp_batch_estimate_timestamps(icp_batch* b, const float* const* rows, const int64_t* n, int stride, int clockwise,
                                  double phi_0, double* const* timestamps_out) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!rows || !n || !timestamps_out)
        return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched time stamps: rows[], n[] and timestamps_out[] are required");
    if (stride != 3 && stride != 4)
        return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched time stamps: stride is 3 (xyz rows) or 4 (x, y, z, reflectance records)");
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    bool any = false;
    for (int i = 0; i < count; ++i) {
        const std::string who = "batched time stamps, member " + std::to_string(i) + ": ";
        if (n[i] < 0 || n[i] > INT32_MAX) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "invalid row count");
        if (n[i] == 0 || !rows[i]) continue;  // sits out
        if (!timestamps_out[i]) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "timestamps_out is required");
        icp_ctx* ctx = b->members[i];
        if (ctx->result_pending()) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "registration in progress");
        if (frame_in_flight(ctx)) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "a frame is launched and awaits its end");
        any = true;
    }
    if (!any) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched time stamps: every member sits out (n <= 0)");
    int rc = front_batch_check(b, "batched time stamps", false);
    if (rc || (rc = front_batch_flush(b))) return rc;
    if ((rc = estimate_timestamps_batch_device(b->members.data(), count, rows, n, stride, clockwise != 0, phi_0, timestamps_out))) {
        for (icp_ctx* ctx : b->members)
            if (!ctx->error.empty()) return batch_fail(b, rc, ctx->error);
        return batch_fail(b, rc, "batched time stamps: HIP error");
    }
    return ICP_OK;
}

// icp_project_rows (slam/common/projection.py:331-418; icp_odometry.py:319-358) for every member in two launches
int icp_batch_project_rows(icp_batch* b, const float* const* xyz, const int64_t* n, float* const* vmap_out,
                           float* const* rows_out) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!xyz || !n || !vmap_out) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched projection: xyz[], n[] and vmap_out[] are required");
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    for (int i = 0; i < count; ++i)
        if (n[i] < 0 || n[i] > INT32_MAX || (n[i] > 0 && !xyz[i]) || !vmap_out[i])
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched projection, member " + std::to_string(i) +
                                                               ": a device scan and a vertex map are required");
    int rc = front_batch_check(b, "batched projection", false);
    if (rc || (rc = front_batch_flush(b))) return rc;
    if ((rc = project_batch_device(b->members.data(), count, xyz, n, vmap_out, rows_out))) return batch_fail(b, rc, b->members[0]->error);
    return ICP_OK;
}

// icp_map_stage_cloud (the insertion of icp_odometry.py:229-231, prepared in front of the registration) for every member
int icp_batch_stage(icp_batch* b, const float* const* xyz, const int64_t* n, int row_mode) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!xyz || !n) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched staging: xyz[] and n[] are required");
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    icp_ctx* const* ctxs = b->members.data();
    for (int i = 0; i < count; ++i)
        if (n[i] < 0 || (n[i] > 0 && !xyz[i]))
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched staging, member " + std::to_string(i) + ": a device cloud is required");
    int rc = front_batch_check(b, "batched staging", true);
    if (rc || (rc = batch_members_free(b, "batched staging", false, true)) || (rc = front_batch_flush(b))) return rc;
    int* mapped[ICP_BATCH_MAX_SEQUENCES] = {};
    float* out[ICP_BATCH_MAX_SEQUENCES] = {};
    for (int i = 0; i < count; ++i) {  // (as icp_map_stage_cloud, member by member)
        icp_ctx* ctx = ctxs[i];
        if (!ctx->staged_count_host &&
            (rc = batch_hip(b, ctx, hipHostMalloc((void**)&ctx->staged_count_host, sizeof(int), hipHostMallocDefault), "hipHostMalloc")))
            return rc;
        if (!ctx->staged_event &&
            (rc = batch_hip(b, ctx, hipEventCreateWithFlags(&ctx->staged_event, hipEventDisableTiming), "hipEventCreate")))
            return rc;
        // an earlier staged cloud that was never consumed: its count may still be in flight towards the pinned word
        if (ctx->staged_rows >= 0 && (rc = batch_hip(b, ctx, hipEventSynchronize(ctx->staged_event), "hipEventSynchronize")))
            return rc;
        ctx->staged_rows = -1;
        *ctx->staged_count_host = 0;
        if (n[i] > 0) {
            if ((rc = batch_hip(b, ctx, ctx->staged_xyz.reserve((size_t)n[i] * 12), "reserve(staged_xyz)")) ||
                (rc = batch_hip(b, ctx, hipHostGetDevicePointer((void**)&mapped[i], ctx->staged_count_host, 0), "hipHostGetDevicePointer")))
                return rc;
            out[i] = ctx->staged_xyz.as<float>();
        }
    }
    if ((rc = compact_valid_rows_batch(ctxs, count, xyz, n, row_mode == ICP_TARGETS_SKIP_NULL, out, mapped)))
        return batch_fail(b, rc, ctxs[0]->error);
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        if ((rc = batch_hip(b, ctx, hipEventRecord(ctx->staged_event, ctx->stream), "hipEventRecord(staged_event)"))) return rc;
        ctx->staged_rows = n[i];
    }
    return ICP_OK;
}

// the next pinned slot of the map-update descriptors (and its device twin), free to be rewritten: its copy is three updates old
static constexpr size_t GRID_SLOT_BYTES =
    sizeof(GridBuildDesc) * ICP_BATCH_MAX_SEQUENCES + sizeof(NormalsBatchDesc) * ICP_BATCH_MAX_SEQUENCES;
static int grid_slot_take(icp_batch* b, int* slot_out) {
    icp_ctx* first = b->members[0];
    const int slot = b->grid_slot;
    if (!b->grid_host[slot]) {
        ICP_HIP(first, hipHostMalloc((void**)&b->grid_host[slot], GRID_SLOT_BYTES, hipHostMallocDefault));
        ICP_HIP(first, b->grid_dev[slot].reserve(GRID_SLOT_BYTES));
        ICP_HIP(first, hipEventCreateWithFlags(&b->grid_copied[slot], hipEventDisableTiming));
    } else {
        ICP_HIP(first, hipEventSynchronize(b->grid_copied[slot]));  // (three updates ago)
    }
    b->grid_slot = (slot + 1) % icp_batch::SLOTS;
    *slot_out = slot;
    return ICP_OK;
}

int icp_batch_map_update(icp_batch* b) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    icp_ctx* first = b->members[0];
    if (int rc_free = batch_members_free(b, "batched map update", true, true)) return rc_free;
    {   // the pose-only update reads the END of the registration: iterations the batch still holds back go first
        const int rc_flush = batch_flush(b);
        if (rc_flush) return rc_flush;
    }
    bool one_stream = true;
    for (icp_ctx* ctx : b->members) {
        { DeviceGuard join_map_stream(ctx); }
        one_stream = one_stream && ctx->stream == first->stream;
        if (!ctx->have_device_pose)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "rel_pose = NULL needs a previous registration on every member");
    }
    if (!one_stream || count == 1) {  // members on streams of their own: one update each, as icp_map_update
        for (icp_ctx* ctx : b->members) {
            const int rc = icp_map_update(ctx, nullptr, nullptr, 0, ICP_MEM_DEVICE, ICP_TARGETS_ALL, nullptr);
            if (rc) return batch_fail(b, rc, ctx->error);
        }
        return ICP_OK;
    }
    // the host bookkeeping of every member's update (window, jobs of the rebuild, buffers), the launches of the grid builds
    // left out: their arguments travel to the device in one table, four launches build the B grids
    int slot = 0;
    int rc = grid_slot_take(b, &slot);
    if (rc) return batch_fail(b, rc, first->error);
    GridBuildDesc* table = b->grid_host[slot];
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = b->members[i];
        if ((rc = continue_launch(ctx, -1))) return batch_fail(b, rc, ctx->error);
        if ((rc = ensure_state(ctx))) return batch_fail(b, rc, ctx->error);
        if ((rc = map_update_body(ctx, nullptr, nullptr, nullptr, 0, false, nullptr, -1, &table[i])))
            return batch_fail(b, rc, ctx->error);
    }
    if ((rc = table_send(b, b->grid_dev[slot], table, sizeof(GridBuildDesc) * (size_t)count, b->grid_copied[slot]))) return rc;
    if ((rc = launch_grid_build_batch(first, table, b->grid_dev[slot].as<GridBuildDesc>(), count)))
        return batch_fail(b, rc, first->error);
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = b->members[i];
        if ((rc = build_grid_finish(ctx, table[i])) || (rc = map_update_finish(ctx))) return batch_fail(b, rc, ctx->error);
    }
    return ICP_OK;
}

// ICPFrameToModel.__update_map (icp_odometry.py:360-380) for every member: icp_map_update_staged (insert[i] != 0) or the
// pose-only icp_map_update (insert[i] == 0), each member's host bookkeeping as there — map_update_body with its launches
// left out — then ONE copy of the descriptors and the launches for all members: the grid builds (launch_grid_build_batch),
// ONE launch of the neighbourhood lists, ONE launch of the eager normals per neighbourhood size (k_normals_hood2_batch);
// members whose normals another kernel computes (launch_normals_all's other branches) get their own launch, as there.
int icp_batch_map_update_staged(icp_batch* b, const float* rel_poses, const int32_t* insert, int64_t* inserted_out) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!insert) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched map update: insert[] is required");
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    icp_ctx* const* ctxs = b->members.data();
    icp_ctx* first = ctxs[0];
    // ---- every member is checked before any member changes (window, map, jobs, grid): a refused call changes nothing
    if (int rc_free = batch_members_free(b, "batched map update", true, true)) return rc_free;
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        { DeviceGuard join_map_stream(ctx); }
        const std::string who = "batched map update, member " + std::to_string(i) + ": ";
        if (ctx->stream != first->stream)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "the members must enqueue on one stream (icp_batch_set_stream)");
        if (insert[i] && ctx->staged_rows < 0)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "no staged cloud (icp_map_stage_cloud)");
        if (!rel_poses && !ctx->have_device_pose)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "rel_poses = NULL needs a previous registration on every member");
        if (!rel_poses && insert[i] && ctx->result_pending())
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "rel_poses = NULL with a new cloud: collect the pending "
                                                                 "registration (icp_batch_register_end) first");
        const bool first_cloud = ctx->map_m == 0 && ctx->cloud_sizes.empty() && !ctx->grid_valid;  // (the pose is ignored)
        float inv[16];
        if (rel_poses && !first_cloud && !invert4(rel_poses + 16 * i, inv))
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "singular relative pose");
    }
    // ---- what goes first: iterations held back (the update reads the END of the registrations), the staged counts
    int rc = batch_flush(b);
    if (rc) return rc;
    int64_t staged[ICP_BATCH_MAX_SEQUENCES] = {};
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        if ((rc = continue_launch(ctx, -1)) || (rc = ensure_state(ctx))) return batch_fail(b, rc, ctx->error);
        if (insert[i]) {  // (long past when the registration was collected in between)
            if ((rc = batch_hip(b, ctx, hipEventSynchronize(ctx->staged_event), "hipEventSynchronize(staged_event)"))) return rc;
            staged[i] = *ctx->staged_count_host;
        }
    }
    int slot = 0;
    if ((rc = grid_slot_take(b, &slot))) return batch_fail(b, rc, first->error);
    GridBuildDesc* table = b->grid_host[slot];
    NormalsBatchDesc* ntable = reinterpret_cast<NormalsBatchDesc*>(table + ICP_BATCH_MAX_SEQUENCES);
    // a member whose bookkeeping has run but whose grid build never reached the stream must not claim that grid (its map
    // rows are moved by the build's first launch): it reports an empty map until its next update
    auto invalidate = [&](int upto) {
        for (int k = 0; k < upto; ++k) {
            ctxs[k]->grid_valid = false;
            ctxs[k]->hoods_valid = false;
            ctxs[k]->normals_ready = false;
            ctxs[k]->cells_table = nullptr;
        }
    };
    // ---- the host side of every member's update
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        const float* rel = rel_poses ? rel_poses + 16 * i : nullptr;
        int64_t ins = 0;
        if (insert[i]) {
            ctx->staged_rows = -1;  // consumed
            rc = map_update_body(ctx, rel, ctx->staged_xyz.as<float>(), nullptr, staged[i], true, &ins, staged[i], &table[i]);
        } else {
            rc = map_update_body(ctx, rel, nullptr, nullptr, 0, false, &ins, -1, &table[i]);
        }
        if (rc) {
            invalidate(i + 1);
            return batch_fail(b, rc, ctx->error);
        }
        if (inserted_out) inserted_out[i] = ins;
    }
    // ---- the eager normals behind the rebuild: map_update_finish's rule, member by member
    NormalsBatchDesc d11[ICP_BATCH_MAX_SEQUENCES], d6[ICP_BATCH_MAX_SEQUENCES];
    icp_ctx *c11[ICP_BATCH_MAX_SEQUENCES], *c6[ICP_BATCH_MAX_SEQUENCES], *own[ICP_BATCH_MAX_SEQUENCES];
    int n11 = 0, n6 = 0, n_own = 0;
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        ctx->hoods_valid = table[i].with_hoods != 0;  // (as build_grid_finish leaves it: the lists are built ahead of every reader)
        if (!(ctx->have_device_pose && ctx->tgt_n > 0 && wants_eager_normals(ctx, ctx->tgt_n)) || ctx->normals_ready ||
            ctx->map_m <= 0)
            continue;
        if (!normals_batchable(ctx)) {
            own[n_own++] = ctx;  // (launch_normals_all, as the single update: another kernel, or nothing for another k)
        } else if (ctx->cfg.num_neighbors_normals + 1 == 11) {
            normals_batch_desc(ctx, &d11[n11]);
            c11[n11++] = ctx;
        } else {
            normals_batch_desc(ctx, &d6[n6]);
            c6[n6++] = ctx;
        }
    }
    if (n11) memcpy(ntable, d11, sizeof(NormalsBatchDesc) * (size_t)n11);
    if (n6) memcpy(ntable + n11, d6, sizeof(NormalsBatchDesc) * (size_t)n6);
    // ---- one copy, then the launches
    const size_t bytes = n11 + n6 > 0 ? sizeof(GridBuildDesc) * ICP_BATCH_MAX_SEQUENCES + sizeof(NormalsBatchDesc) * (size_t)(n11 + n6)
                                      : sizeof(GridBuildDesc) * (size_t)count;
    const GridBuildDesc* table_dev = b->grid_dev[slot].as<GridBuildDesc>();
    const NormalsBatchDesc* ntable_dev = reinterpret_cast<const NormalsBatchDesc*>(table_dev + ICP_BATCH_MAX_SEQUENCES);
    rc = table_send(b, b->grid_dev[slot], table, bytes, b->grid_copied[slot]);
    if (!rc && (rc = launch_grid_build_batch(first, table, table_dev, count))) batch_fail(b, rc, first->error);
    if (rc) {
        invalidate(count);
        return rc;
    }
    if ((rc = launch_hood_build_batch(first, table, table_dev, count))) {
        for (int i = 0; i < count; ++i) ctxs[i]->hoods_valid = false;  // (the grids stand; their normals are not estimated)
        return batch_fail(b, rc, first->error);
    }
    if ((rc = launch_normals_batch(first, 11, d11, ntable_dev, n11)) || (rc = launch_normals_batch(first, 6, d6, ntable_dev + n11, n6)))
        return batch_fail(b, rc, first->error);
    for (int k = 0; k < n11 + n6; ++k) {  // (as launch_normals_all)
        icp_ctx* ctx = k < n11 ? c11[k] : c6[k - n11];
        ctx->normals_ready = true;
        ctx->normals_eager_count += ctx->map_m;
    }
    for (int k = 0; k < n_own; ++k)
        if ((rc = map_update_finish(own[k]))) return batch_fail(b, rc, own[k]->error);
    return ICP_OK;
}

// ---- the projective local map, B maps per launch -------------------------------------------------------------------
// What every batched projective call asks of its members: one stream, one image geometry (the kernels share the pixel grid
// and the projection), nothing of a registration still open, no kd-tree iterations held back.  Nothing changes on refusal.
static int pmap_batch_check(icp_batch* b, const char* what) {
    icp_ctx* first = b->members[0];
    for (size_t i = 0; i < b->members.size(); ++i) {
        icp_ctx* ctx = b->members[i];
        { DeviceGuard join_map_stream(ctx); }
        const std::string who = std::string(what) + ", member " + std::to_string(i) + ": ";
        if (ctx->stream != first->stream)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "the members must enqueue on one stream (icp_batch_set_stream)");
        if (ctx->cfg.height != first->cfg.height || ctx->cfg.width != first->cfg.width || ctx->cfg.up_fov != first->cfg.up_fov ||
            ctx->cfg.down_fov != first->cfg.down_fov)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "the members must share height, width and field of view");
        if (ctx->in_registration || ctx->result_pending())
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "a registration is still pending: collect it first "
                                                                 "(icp_batch_register_end / icp_register_end)");
        if (ctx->batch_hold || ctx->launch_remaining > 0)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "kd-tree iterations are still held back: collect them first");
    }
    return batch_members_free(b, what, false, true);  // (frame 0 of a member's own frame call: launched, nothing pending)
}

int icp_batch_pmap_register_launch(icp_batch* b, const float* const* xyz, const int64_t* n, int mem, int target_mode,
                                   const float* init_poses, int from_last) {
    if (!b || !xyz || !n) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    icp_ctx* const* ctxs = b->members.data();
    icp_ctx* first = ctxs[0];
    const int iters = first->cfg.max_num_alignments;
    // ---- every member is checked before any member changes
    int rc = pmap_batch_check(b, "batched projective registration");
    if (rc) return rc;
    if ((rc = batch_shared_options_check(b, "batched projective registration"))) return rc;
    int max_n = 0;
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        const std::string who = "batched projective registration, member " + std::to_string(i) + ": ";
        if (n[i] < 0 || (n[i] > 0 && !xyz[i])) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "no scan");
        if (ctx->cfg.max_num_alignments != iters || ctx->cfg.scheme != first->cfg.scheme || ctx->cfg.sigma != first->cfg.sigma)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "the members must share max_num_alignments, scheme and sigma");
        if (ctx->exchange_on || ctx->prof.enabled || ctx->cost != ICP_COST_POINT_TO_PLANE)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "point-to-plane registrations without exchange or profiling only");
        if (ctx->pm_slots.empty()) return batch_fail(b, ICP_ERR_EMPTY_MAP, who + "the projective local map is empty");
        if (from_last && !ctx->pm_have_pose && !ctx->have_device_pose)
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, who + "no previous registration to start from");
        max_n = std::max(max_n, (int)n[i]);
    }
    BatchUnwind unwind{b, false};
    // ---- descriptor slot: [packs | registrations | sum + solve | sum + solve of the last iteration]
    const BatchPmapRegisterLayout lay(sizeof(PackDesc), pmap_reg_desc_bytes(), sum_solve_desc_bytes(), count);
    int slot = 0;
    if ((rc = table_slot_take(b, lay.need(), &slot))) return batch_fail(b, rc, first->error);
    char* host = b->host[slot];
    int rows[ICP_BATCH_MAX_SEQUENCES], quad[ICP_BATCH_MAX_SEQUENCES];
    // ---- every member begins, the packing launch left to the batch
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        const float* init = (init_poses && !from_last) ? init_poses + 16 * i : nullptr;
        if ((rc = pmap_register_begin(ctx, xyz[i], n[i], mem, target_mode, init, from_last != 0,
                                      reinterpret_cast<PackDesc*>(host) + i, false)) ||
            (rc = pmap_register_desc(ctx, host + lay.registrations() + pmap_reg_desc_bytes() * i, &rows[i])))
            return batch_fail(b, rc, ctx->error);
        quad[i] = 1;
        if ((rc = result_fold_begin(ctx, false))) return batch_fail(b, rc, ctx->error);
    }
    prepare_sum_solve_batch(ctxs, count, rows, quad, false, false, host + lay.sum_solve(false));
    if (iters > 0)  // (the last iteration's launch delivers the result blocks; without iterations a copy does)
        prepare_sum_solve_batch(ctxs, count, rows, quad, false, true, host + lay.sum_solve(true));
    // ---- one copy, then the launches: targets + states + z-buffers, and three per iteration
    const char* dev = b->dev[slot].as<char>();
    if ((rc = table_send(b, b->dev[slot], host, lay.need(), b->copied[slot]))) return rc;
    if ((rc = pmap_launch_begin_batch(first, reinterpret_cast<const PackDesc*>(dev), dev + lay.registrations(), count, max_n)))
        return batch_fail(b, rc, first->error);
    for (int it = 0; it < iters; ++it) {
        if ((rc = pmap_launch_iteration_batch(first, dev + lay.registrations(), count, max_n)) ||
            (rc = launch_sum_solve_batch(first, count, dev + lay.sum_solve(it + 1 == iters))))
            return batch_fail(b, rc, first->error);
    }
    // ---- the results: ONE event behind every member's block (icp_batch_register_end)
    int done_slot = 0;
    if ((rc = done_event_take(b, &done_slot))) return rc;
    hipEvent_t done = b->done[done_slot];
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        ctx->batch_hold = false;
        if ((rc = result_hand_over(ctx, ICP_OK, iters, 0, false, done))) return batch_fail(b, rc, ctx->error);
        ctx->pm_have_pose = true;
    }
    ICP_HIP(first, hipEventRecord(done, first->stream));
    unwind.armed = false;
    return ICP_OK;
}

int icp_batch_pmap_update(icp_batch* b, const float* rel_poses, const float* const* vmaps, int mem, int normals_kernel_size) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!rel_poses) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "batched projective map update: rel_poses is required");
    DeviceGuard device_guard(b->device);
    const int count = (int)b->members.size();
    icp_ctx* const* ctxs = b->members.data();
    icp_ctx* first = ctxs[0];
    bool any_insert = false;
    for (int i = 0; i < count; ++i) any_insert = any_insert || (vmaps && vmaps[i]);
    if (any_insert && (normals_kernel_size < 1 || normals_kernel_size > 15 || !(normals_kernel_size & 1)))
        return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "normals_kernel_size must be odd, 1..15");
    // ---- every member is checked before any member changes
    int rc = pmap_batch_check(b, "batched projective map update");
    if (rc) return rc;
    for (int i = 0; i < count; ++i) {
        const char* why = nullptr;
        if ((rc = pmap_window_check(ctxs[i], rel_poses + 16 * i, vmaps && vmaps[i], &why)))
            return batch_fail(b, rc, "batched projective map update, member " + std::to_string(i) + ": " + why);
    }
    // ---- buffers: the new vertex maps on the device, the slot storage (kept), the model layers of the new windows
    const size_t bytes = (size_t)first->cfg.height * first->cfg.width * 12;
    const float* in[ICP_BATCH_MAX_SEQUENCES] = {};
    int slots[ICP_BATCH_MAX_SEQUENCES];
    size_t pairs = 0;
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        if ((rc = ensure_state(ctx))) return batch_fail(b, rc, ctx->error);
        slots[i] = -1;
        if (vmaps && vmaps[i]) {
            const void* p;
            if ((rc = import_buffer(ctx, vmaps[i], bytes, mem, ctx->stage_in, &p)) || (rc = pmap_reserve_store(ctx)))
                return batch_fail(b, rc, ctx->error);
            in[i] = (const float*)p;
            slots[i] = pmap_free_slot(ctx);
            if (slots[i] < 0) return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "no free projective-map slot");
        }
        // the window after pmap_window_step: + the new map, - the oldest beyond local_map_size (never for the first map)
        int k = (int)ctx->pm_slots.size() + (slots[i] >= 0 ? 1 : 0);
        if (!ctx->pm_slots.empty() && k > ctx->cfg.local_map_size) k -= 1;
        pairs += (size_t)k;
    }
    const size_t ins_bytes = pad256(pmap_insert_desc_bytes() * (size_t)count);
    const size_t need = ins_bytes + pmap_pair_desc_bytes() * (pairs > 0 ? pairs : 1);
    int slot = 0;
    if ((rc = table_slot_take(b, need, &slot))) return batch_fail(b, rc, first->error);
    char* host = b->host[slot];
    // ---- the windows (host only, nothing fails from here on but the HIP calls), the descriptors
    int n_ins = 0, n_pairs = 0;
    for (int i = 0; i < count; ++i) {
        icp_ctx* ctx = ctxs[i];
        if (slots[i] >= 0) pmap_insert_desc(ctx, slots[i], in[i], normals_kernel_size, host + pmap_insert_desc_bytes() * n_ins++);
        pmap_window_step(ctx, rel_poses + 16 * i, slots[i]);
    }
    // a member whose window has moved but whose model never reached the stream reports an empty map until its next update
    auto invalidate = [&]() {
        for (int i = 0; i < count; ++i) {
            ctxs[i]->pm_slots.clear();
            ctxs[i]->pm_poses.clear();
        }
    };
    for (int i = 0; i < count; ++i) {
        int k = 0;
        if (n_pairs + ctxs[i]->pm_slots.size() > pairs) {  // (cannot happen: the count above is the window step's)
            invalidate();
            return batch_fail(b, ICP_ERR_INVALID_ARGUMENT, "internal: projective window larger than counted");
        }
        if ((rc = pmap_pair_descs(ctxs[i], host + ins_bytes + pmap_pair_desc_bytes() * n_pairs, &k))) {
            invalidate();
            return batch_fail(b, rc, ctxs[i]->error);
        }
        n_pairs += k;
    }
    // ---- one copy, then the launches: the insertions, the clear, the projection and the resolve of every (member, slot)
    const char* dev = b->dev[slot].as<char>();
    rc = table_send(b, b->dev[slot], host, need, b->copied[slot]);
    if (!rc && (rc = pmap_launch_update_batch(first, dev, n_ins, dev + ins_bytes, n_pairs))) batch_fail(b, rc, first->error);
    if (rc) {
        invalidate();
        return rc;
    }
    if (any_insert && mem == ICP_MEM_HOST) ICP_HIP(first, hipStreamSynchronize(first->stream));
    return ICP_OK;
}

int icp_batch_register_end(icp_batch* b, icp_register_result* results, double* loss_per_iter_out, float* dx_per_iter_out) {
    if (!b || !results) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(b->device);
    // (a member's own frame: its icp_frame_end collects that registration — collected here, the frame could never end)
    if (int rc_free = batch_members_free(b, "icp_batch_register_end", false, true)) return rc_free;
    // a registration enqueued in chunks: wait for what is on the stream; while a member is still running and iterations are
    // held back, the next chunk (four iterations), and look again
    while (b->run_active) {
        icp_ctx* first = b->members[0];
        ICP_HIP(first, hipEventSynchronize(b->done[b->run_done]));
        bool running = false;
        for (icp_ctx* ctx : b->members) {
            if (ctx->r_count <= 0) continue;
            RegState st;
            memcpy(&st, ctx->rslot[(ctx->r_head + ctx->r_count - 1) & 1].host, sizeof(st));  // (the newest pending result: this registration's)
            running = running || (!st.done && st.status == ICP_OK && st.handoff_timeouts == 0);
        }
        if (!running) {
            b->run_active = false;  // (every member has stopped: the rest is never enqueued)
            for (icp_ctx* ctx : b->members) ctx->batch_hold = false;
            break;
        }
        const int rc_chunk = batch_enqueue(b, 4, nullptr, false);
        if (rc_chunk) {
            batch_abandon(b);
            return rc_chunk;
        }
    }
    for (icp_ctx* ctx : b->members) ctx->batch_hold = false;
    int first_rc = ICP_OK;
    const size_t cap = (size_t)b->members[0]->cfg.max_num_alignments;
    for (size_t i = 0; i < b->members.size(); ++i) {
        icp_ctx* ctx = b->members[i];
        const int rc = register_collect(ctx, &results[i], loss_per_iter_out ? loss_per_iter_out + i * cap : nullptr,
                                        dx_per_iter_out ? dx_per_iter_out + i * cap * 6 : nullptr);
        if (rc) results[i].status = rc;  // (whatever ended this member: a caller tells the healthy members by their status)
        if (rc && !first_rc) {
            first_rc = rc;
            b->error = ctx->error;
        }
    }
    return first_rc;
}

