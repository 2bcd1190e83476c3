// C ABI of libicp_mi355x.so, the registration of ONE context: the kd-tree and the projective begin, the iterations (polled by
// the host, or enqueued whole or in chunks), the pinned result slots and icp_register_end.  Host code only: the kernels it
// enqueues live in search.hip, gauss_newton.hip, projective.hip and grid_sample.hip.
// (the entry points take their C linkage from their declarations in include/icp_mi355x.h)
#include <string.h>

#include <vector>

#include "icp_internal.h"
#include "register_plan.h"

using namespace icp;

static bool device_shared_with_another_registration(const icp_ctx* ctx) {
    const int d = ctx->cfg.device >= 0 && ctx->cfg.device < 64 ? ctx->cfg.device : 0;
    return g_registering[d].load() > (ctx->counted_registering ? 1 : 0);
}

// An entry point of the registration that leaves on an error must not leave its context counted among the registering ones
// (every other context of the device then ran without lead launches for the life of the process): on scope exit,
// a context with no registration in progress and no result pending leaves the count.
namespace {
struct RegisteringGuard {
    icp_ctx* ctx;
    explicit RegisteringGuard(icp_ctx* c) : ctx(c) {}
    ~RegisteringGuard() {
        if (ctx && !ctx->in_registration && ctx->r_count == 0) registering_leave(ctx);
    }
};
}  // namespace

// (wants_eager_normals: icp_internal.h — the grid build asks the same question before it builds the neighbourhood lists)
static int enqueue_iterations(icp_ctx* ctx, bool poll_allowed, int first = 0, int count = -1);

// the host looks at RegState.done behind everything the stream holds (it waits for the stream)
static int poll_done(icp_ctx* ctx, int* done) {
    ICP_HIP(ctx, hipMemcpyAsync(done, &reg_state(ctx)->done, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICP_OK;
}

// ---- against the projective map, the host polling for the stop ------------------------------------------------------------
int icp_pmap_register(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16],
                      icp_register_result* result, double* loss_per_iter_out, float* dx_per_iter_out) {
    DeviceGuard device_guard(ctx);
    if (!ctx || !result || n < 0 || (n > 0 && !xyz)) return ICP_ERR_INVALID_ARGUMENT;
    // (icp_register_end below hands out the OLDEST pending result: with one pending it would return that registration as this
    // one's and leave this one uncollected, the context "in registration" for good)
    if (ctx->in_registration || ctx->result_pending())
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_pmap_register: a registration of this context is in progress or awaits "
                                                   "icp_register_end");
    ICP_HELD_FIRST(ctx);  // (a batch that holds iterations back is refused here)
    if (ctx->pm_slots.empty()) return fail(ctx, ICP_ERR_EMPTY_MAP, "the local map is empty");
    int rc = pmap_register_begin(ctx, xyz, n, mem, target_mode, init_pose, false, nullptr, true);
    if (rc) return rc;
    const int iters = ctx->cfg.max_num_alignments;
    const int poll = ctx->cfg.threshold_delta_pose > 0.f ? ctx->cfg.poll_every : 0;
    for (int it = 0; it < iters; ++it) {
        int blocks = 0;
        rc = pmap_iterate(ctx, &blocks);
        if (!rc) rc = launch_sum_solve(ctx, blocks);
        if (rc) {
            ctx->in_registration = false;
            return rc;
        }
        if (poll > 0 && (it + 1) % poll == 0 && it + 1 < iters) {
            int done = 0;
            if ((rc = poll_done(ctx, &done))) {
                ctx->in_registration = false;  // (as every other error exit of the loop: the context is not left "in registration")
                return rc;
            }
            if (done) break;
        }
    }
    return register_collect(ctx, result, loss_per_iter_out, dx_per_iter_out);
}

// ---- registration ---------------------------------------------------------------------------------------------------
// defer_pack: the launch that packs the targets and initialises the state is left to the caller (a batched registration runs
// it for all its members at once)
// hold_pack (icp_register_launch: the iterations are enqueued right behind the begin): with option "first_build", and where the
// first launch of the registration will be a fused iteration of one sequence with its normals at hand, the packing launch is
// held back in ctx->first_pack — launch_iterate_fused folds it into k_iterate_first, or runs it in front of a launch that
// build does not exist for (first_pack_flush: whoever enqueues anything else first)
static bool first_build_wanted(const icp_ctx* ctx, int64_t n) {
    return ctx->first_build && n > 0 && ctx->cfg.max_num_alignments >= 1 &&
           ctx->cost == ICP_COST_POINT_TO_PLANE && ctx->fuse_iteration && (ctx->normals_ready || wants_eager_normals(ctx, n)) &&
           !wants_lazy_fused(ctx, n) && !ctx->exchange_on && !ctx->search_stats && !ctx->prof.enabled && ctx->ball_search &&
           !(ctx->hit_records && ctx->use_nn_cache);
}

int first_pack_flush(icp_ctx* ctx) {
    if (!ctx->first_pending) return ICP_OK;
    ctx->first_pending = false;
    return launch_pack_targets(ctx, ctx->first_pack);
}

int register_begin(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16],
                   bool from_last, PackDesc* defer_pack, bool hold_pack) {
    if (!ctx || n < 0 || (n > 0 && !xyz)) return ICP_ERR_INVALID_ARGUMENT;
    if (ctx->map_m <= 0 || !ctx->grid_valid) return fail(ctx, ICP_ERR_EMPTY_MAP, "the local map is empty");
    if (ctx->in_registration) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "registration in progress");
    if (from_last && !ctx->have_device_pose)
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "no previous registration on this context to start from");
    int rc = ensure_state(ctx);
    if (rc || (rc = stage_targets(ctx, xyz, n, mem, target_mode))) return rc;
    ICP_HIP(ctx, ctx->nn_pos.reserve((size_t)(n > 0 ? n : 1) * 4));
    ctx->first_pending = false;
    const bool hold = hold_pack && !defer_pack && first_build_wanted(ctx, n);
    if ((rc = prepare_targets_and_state(ctx, n, init_pose, from_last, hold ? &ctx->first_pack : defer_pack))) return rc;
    ctx->first_pending = hold;
    if (hold && !ctx->first_pack_preloaded) {  // (once per context: a later fall-back finds the packing kernel loaded)
        pack_targets_preload();
        ctx->first_pack_preloaded = true;
    }
    ctx->have_device_pose = true; ctx->device_pose_epoch += 1;
    // event pairs around the kernels of every `every`-th registration only: a pair costs ~2 us of stream time
    ctx->prof.sample_now = ctx->prof.every <= 1 || (ctx->prof.registrations % ctx->prof.every) == 0;
    ctx->prof.rotate_index = (int)((ctx->prof.registrations / (ctx->prof.every > 1 ? ctx->prof.every : 1)) %
                                   (ctx->cfg.max_num_alignments > 0 ? ctx->cfg.max_num_alignments : 1));
    ctx->prof.registrations += 1;
    // normals: lazily for the map points the scan touches (local_map.py:397-422) when the map is much larger than the
    // scan, all at once otherwise (same values; one dense launch instead of a sparse one per iteration)
    if (!ctx->normals_ready && wants_eager_normals(ctx, n) && (rc = launch_normals_all(ctx))) return rc;
    // ... or on demand inside the fused iteration kernel, where the scan touches a small part of the map ("lazy_fused")
    ctx->lazy_now = !ctx->normals_ready && wants_lazy_fused(ctx, n);
    // (a held packing launch whose registration turns out not to begin with a plain fused iteration after all: now)
    if (ctx->first_pending && (!fused_path(ctx) || ctx->lazy_now) && (rc = first_pack_flush(ctx))) return rc;
    registering_enter(ctx);
    // lead launches or not: decided ONCE per registration (another context of the process starting or ending a
    // registration between two chunks of this one flipped the answer — a chunk without a lead publishes no pose, the next
    // lead chunk then took a stale one from the mailbox)
    ctx->lead_latched = ctx->lead_solve && !ctx->handoff_disabled && !device_shared_with_another_registration(ctx);
    ctx->lead_registrations += ctx->lead_latched ? 1 : 0;
    ctx->in_registration = true;
    ctx->iter_in_registration = 0;
    ctx->cache_fresh = false;
    ctx->searches_in_registration = 0;
    return ICP_OK;
}

// The projective twin: the scan staged, targets packed and the state initialised (defer_pack: that launch left to the batch),
// the context "in registration" against its projective map.  The callers' refusals stand in front of it.  from_last: the
// pose the state holds is the initial guess.  pose_now: the context counts as holding a projective pose from here on — a
// batched launch says so only once its members' results are on their way (an error in between leaves the flag as it was)
int pmap_register_begin(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16],
                        bool from_last, PackDesc* defer_pack, bool pose_now) {
    int rc = ensure_state(ctx);
    if (rc || (rc = stage_targets(ctx, xyz, n, mem, target_mode))) return rc;
    if ((rc = prepare_targets_and_state(ctx, n, init_pose, from_last, defer_pack))) return rc;
    ctx->have_device_pose = false; ctx->device_pose_epoch += 1;  // icp_map_update(rel_pose = NULL) follows a registration against the kd-tree style map only
    if (pose_now) ctx->pm_have_pose = true;
    ctx->in_registration = true;
    return ICP_OK;
}

int icp_register_begin(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode,
                       const float init_pose[16]) {
    DeviceGuard device_guard(ctx);
    if (ctx && ctx->result_pending()) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "collect the pending result first");
    return register_begin(ctx, xyz, n, mem, target_mode, init_pose, false);
}

// the fused search + rows kernel needs every normal it may touch: the eager schedule
bool fused_path(const icp_ctx* ctx) {
    return ctx->cost == ICP_COST_POINT_TO_PLANE && (ctx->normals_ready || ctx->lazy_now) && ctx->fuse_iteration;
}

int icp_iteration_accumulate(icp_ctx* ctx) {
    DeviceGuard device_guard(ctx);
    if (!ctx) return ICP_ERR_INVALID_ARGUMENT;
    if (!ctx->in_registration)
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_iteration_accumulate: no registration in progress (icp_register_begin first)");
    int rc;
    if (fused_path(ctx)) {
        int rows = 0, quad = 1;
        if ((rc = launch_iterate_fused(ctx, &rows, &quad))) return rc;
        return launch_sum_partials(ctx, rows, quad);
    }
    if ((rc = launch_search(ctx))) return rc;
    ctx->iter_in_registration += 1;  // (the fused launch counts itself)
    if (ctx->cost == ICP_COST_POINT_TO_POINT) return launch_reduce_p2p(ctx, false);
    if ((rc = launch_normals(ctx))) return rc;
    return launch_reduce(ctx);
}

int icp_iteration_solve(icp_ctx* ctx) {
    DeviceGuard device_guard(ctx);
    if (!ctx) return ICP_ERR_INVALID_ARGUMENT;
    if (!ctx->in_registration)
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_iteration_solve: no registration in progress (icp_register_begin first)");
    return launch_solve(ctx);
}

// layout of the pinned result block: the device state allocation verbatim (RegState | pad | loss[hist_cap] |
// dx[6 * hist_cap])
static size_t state_bytes(const icp_ctx* ctx) {
    return STATE_BLOCK + (size_t)ctx->hist_cap * (sizeof(double) + 6 * sizeof(float));
}

// the pinned slot the result of the registration being enqueued will land in (refresh = true: the newest pending one again)
static int result_slot(icp_ctx* ctx, bool refresh, icp_ctx::ResultSlot** out) {
    if (!refresh && ctx->r_count >= 2) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "two results are already pending");
    icp_ctx::ResultSlot& r = ctx->rslot[(ctx->r_head + ctx->r_count - (refresh ? 1 : 0)) & 1];
    const size_t need = state_bytes(ctx);
    if (need > r.bytes) {
        if (r.host) (void)hipHostFree(r.host);
        r.host = nullptr;
        r.bytes = 0;
        ICP_HIP(ctx, hipHostMalloc(&r.host, need, hipHostMallocDefault));
        r.bytes = need;
    }
    if (!r.event) ICP_HIP(ctx, hipEventCreateWithFlags(&r.event, hipEventDisableTiming));
    *out = &r;
    return ICP_OK;
}

// no solving launch writes (or has written) a result block into a pinned slot itself
void result_fold_reset(icp_ctx* ctx) {
    ctx->result_fold_to = nullptr;
    ctx->result_folded = false;
}

// call before enqueue_iterations: the last solving launch may then write the result block into the slot itself
int result_fold_begin(icp_ctx* ctx, bool refresh) {
    result_fold_reset(ctx);
    icp_ctx::ResultSlot* r = nullptr;
    const int rc = result_slot(ctx, refresh, &r);
    if (rc) return rc;
    void* mapped = nullptr;
    if (hipHostGetDevicePointer(&mapped, r->host, 0) == hipSuccess && mapped) {
        ctx->result_fold_to = (char*)mapped;
        ctx->result_fold_bytes = state_bytes(ctx);
    }
    return ICP_OK;
}

// refresh = true: the newest pending slot is copied again (a further chunk of its registration has been enqueued)
static int enqueue_result_copy(icp_ctx* ctx, bool refresh = false, hipEvent_t shared_event = nullptr) {
    icp_ctx::ResultSlot* rp = nullptr;
    const int rc_slot = result_slot(ctx, refresh, &rp);
    if (rc_slot) return rc_slot;
    icp_ctx::ResultSlot& r = *rp;
    const size_t sb = state_bytes(ctx);
    char* h = (char*)r.host;
    // state + histories (unless the last solving launch has written them there already)
    if (!ctx->result_folded) ICP_HIP(ctx, hipMemcpyAsync(h, ctx->state.ptr, sb, hipMemcpyDeviceToHost, ctx->stream));
    // (a batched registration: ONE event behind the results of all its members, recorded by the batch — icp_batch_*)
    r.wait = shared_event ? shared_event : r.event;
    if (!shared_event) ICP_HIP(ctx, hipEventRecord(r.event, ctx->stream));
    if (refresh) return ICP_OK;
    // the grid statistics about to be read back belong to the current build; a later build starts a new pending set
    r.stats = ctx->stats_pending;
    r.stats_m = ctx->stats_m_pending;
    r.stats_h = ctx->stats_h_pending;
    ctx->stats_pending = false;
    r.eager_normals = ctx->normals_eager_count;
    ctx->normals_eager_count = 0;
    ctx->r_count += 1;
    return ICP_OK;
}

// The iterations of a registration — or of one more chunk of it: refresh — are on the stream (rc: what enqueuing them
// returned; nothing is copied behind a failure): `enqueued` of them so far and `remaining` held back, the result copy behind
// them (shared_event: the ONE event of a batched registration), the fold given up, the context no longer "in registration"
int result_hand_over(icp_ctx* ctx, int rc, int enqueued, int remaining, bool refresh, hipEvent_t shared_event) {
    ctx->launch_enqueued = enqueued;
    ctx->launch_remaining = remaining;
    if (!rc) rc = enqueue_result_copy(ctx, refresh, shared_event);
    result_fold_reset(ctx);
    ctx->in_registration = false;  // the result waits in its slot
    return rc;
}

// enqueues the iterations a chunked launch has held back (all of them, or the next `count`) and copies the result again
int continue_launch(icp_ctx* ctx, int count) {
    if (ctx->batch_hold)  // (a batched registration of this context is enqueued in chunks: its batch owns what is held back)
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "a batched registration of this context still holds iterations back: "
                                                   "icp_batch_register_end (or icp_batch_map_update) first");
    if (ctx->launch_remaining <= 0) return ICP_OK;
    if (count < 0 || count > ctx->launch_remaining) count = ctx->launch_remaining;
    ctx->in_registration = true;
    int rc = result_fold_begin(ctx, true);
    if (!rc) rc = enqueue_iterations(ctx, false, ctx->launch_enqueued, count);
    return result_hand_over(ctx, rc, ctx->launch_enqueued + count, ctx->launch_remaining - count, true);
}

// A hand-off inside a lead launch / the resident tail ran out of its wall-clock budget (RegState.handoff_timeouts: a
// workgroup the others wait for is not running — the GPU is shared with foreign work).  The launches behind it solved
// nothing more (lead_solve / k_sum_solve stop at the counter), so the state holds the last complete iteration; a pose-only
// map update enqueued behind the registration moved nothing (map_move_prepare).  Here: the context stops using hand-offs
// (per-iteration launches with a solving launch each: "lead_solve" 0), the remaining iterations run on those — the same
// iterations on the same map, hence the same bits — and the skipped map update is repeated with the final pose.
// `block` receives the state + histories (the layout of the pinned result block).
static int recover_handoff(icp_ctx* ctx, RegState& st, std::vector<char>& block) {
    { DeviceGuard join_map_stream(ctx); }  // (a map update on its own stream: everything below follows it)
    ctx->tail_disabled = true;
    ctx->handoff_disabled = true;  // (the user's "lead_solve" stays as set; setting it again re-arms the hand-offs)
    ctx->lead_latched = false;
    ctx->handoff_fallbacks += 1;
    ctx->launch_remaining = 0;
    ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ICP_HIP(ctx, hipMemcpy(&st, ctx->state.ptr, sizeof(st), hipMemcpyDeviceToHost));
    ICP_HIP(ctx, hipMemsetAsync(&reg_state(ctx)->handoff_timeouts, 0, sizeof(int), ctx->stream));
    int rc = ICP_OK;
    if (!st.done && st.status == ICP_OK && st.iter < ctx->cfg.max_num_alignments) {
        ctx->in_registration = true;
        ctx->iter_in_registration = st.iter;
        ctx->cache_fresh = false;  // (a map update in between has rebuilt the grid: the first launch searches everything)
        ctx->searches_in_registration = 0;
        if (!ctx->normals_ready && wants_eager_normals(ctx, ctx->tgt_n) && (rc = launch_normals_all(ctx))) {
            ctx->in_registration = false;  // (register_collect's RegisteringGuard then leaves the count)
            return rc;
        }
        rc = enqueue_iterations(ctx, false, st.iter, -1);
        ctx->in_registration = false;
        if (rc) return rc;
    }
    if (ctx->update_behind_registration) {  // the pose-only update the device skipped, now with the final pose
        ctx->update_behind_registration = false;
        if ((rc = map_update_impl(ctx, nullptr, nullptr, nullptr, 0, false, nullptr))) return rc;
    }
    ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    block.resize(state_bytes(ctx));
    ICP_HIP(ctx, hipMemcpy(block.data(), ctx->state.ptr, block.size(), hipMemcpyDeviceToHost));
    memcpy(&st, block.data(), sizeof(st));
    return ICP_OK;
}

// A frame call owns the registration it launched: icp_frame_end / icp_pmap_frame_end (or the batch's) collect it, read the
// key-frame test off its pose and insert the staged rows.  Collected from outside, the frame could neither end nor be launched
// again (its end fails in frame_collect and leaves the frame launched).  The library's own collectors call register_collect.
int icp_register_end(icp_ctx* ctx, icp_register_result* result, double* loss_per_iter_out, float* dx_per_iter_out) {
    if (ctx && result && frame_in_flight(ctx))
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_register_end: a frame is launched and awaits its end");
    return register_collect(ctx, result, loss_per_iter_out, dx_per_iter_out);
}

int register_collect(icp_ctx* ctx, icp_register_result* result, double* loss_per_iter_out, float* dx_per_iter_out) {
    DeviceGuard device_guard(ctx, false);  // (the pose arrives while the map update runs)
    if (!ctx || !result) return ICP_ERR_INVALID_ARGUMENT;
    if (!ctx->in_registration && !ctx->result_pending())
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_register_end: no registration to collect");
    if (ctx->batch_hold)
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "a batched registration of this context still holds iterations back: "
                                                   "collect it with icp_batch_register_end");
    RegisteringGuard leave_on_exit(ctx);
    RegState st;
    const bool async = ctx->result_pending();
    bool had_stats;
    int64_t stats_m, eager;
    float stats_h;
    const char* pinned = nullptr;
    if (async) {  // copies were enqueued right behind the last iteration: wait for those only (the OLDEST result)
        icp_ctx::ResultSlot& r = ctx->rslot[ctx->r_head];
        ICP_HIP(ctx, hipEventSynchronize(r.wait));
        pinned = (const char*)r.host;
        memcpy(&st, pinned, sizeof(st));
        // a chunked launch (only ever the newest pending registration, here also the oldest): still running and
        // iterations held back -> the next chunk, then look again
        while (ctx->r_count == 1 && ctx->launch_remaining > 0 && !st.done && st.status == ICP_OK) {
            const int rc2 = continue_launch(ctx, 4);
            if (rc2) return rc2;
            ICP_HIP(ctx, hipEventSynchronize(r.wait));
            memcpy(&st, pinned, sizeof(st));
        }
        if (ctx->r_count == 1) ctx->launch_remaining = 0;  // (finished early: the rest is never enqueued)
        ctx->r_head ^= 1;
        ctx->r_count -= 1;
        had_stats = r.stats;
        stats_m = r.stats_m;
        stats_h = r.stats_h;
        eager = r.eager_normals;
    } else {
        ctx->in_registration = false;
        had_stats = ctx->stats_pending;
        stats_m = ctx->stats_m_pending;
        stats_h = ctx->stats_h_pending;
        ctx->stats_pending = false;
        eager = ctx->normals_eager_count;
        ctx->normals_eager_count = 0;
        ICP_HIP(ctx, hipMemcpyAsync(&st, ctx->state.ptr, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
        ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    std::vector<char> recovered;
    if (st.handoff_timeouts > 0 && ctx->r_count == 0) {  // (with a newer registration already enqueued behind it: the error below)
        const int rc_rec = recover_handoff(ctx, st, recovered);
        if (rc_rec) return rc_rec;
        if (async) pinned = recovered.data();
    }
    if (ctx->r_count == 0) ctx->update_behind_registration = false;  // (the guard above leaves the count of registering contexts)
    if (had_stats && st.grid_cells > 0) {
        ctx->occupied_cells = st.grid_cells;
        ctx->stats_m = stats_m;
        ctx->stats_h = stats_h;
    }
    search_stats_report(ctx, st);  // (the developer's "search_stats" dump, when it is on)
    st.normals_computed += eager;
    memcpy(result->pose, st.pose, sizeof(st.pose));
    memcpy(result->params, st.params, sizeof(st.params));
    result->iterations = st.iter;
    ctx->last_iterations = st.iter;
    ctx->last_valid_targets = st.n_targets;
    result->converged = st.converged;
    result->status = st.status;
    result->num_targets = st.n_targets;
    result->normals_computed = st.normals_computed;
    const int k = st.iter < ctx->hist_cap ? st.iter : ctx->hist_cap;
    if (async) {
        const char* lh = pinned + STATE_BLOCK;
        if (k > 0 && loss_per_iter_out) memcpy(loss_per_iter_out, lh, (size_t)k * sizeof(double));
        if (k > 0 && dx_per_iter_out)
            memcpy(dx_per_iter_out, lh + (size_t)ctx->hist_cap * sizeof(double), (size_t)k * 6 * sizeof(float));
    } else {
        if (k > 0 && loss_per_iter_out)
            ICP_HIP(ctx, hipMemcpy(loss_per_iter_out, ctx->loss_hist, (size_t)k * sizeof(double), hipMemcpyDeviceToHost));
        if (k > 0 && dx_per_iter_out)
            ICP_HIP(ctx, hipMemcpy(dx_per_iter_out, ctx->dx_hist, (size_t)k * 6 * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (ctx->prof.enabled) prof_collect(ctx);
    if (st.handoff_timeouts > 0)
        return fail(ctx, ICP_ERR_HIP, "internal: the pose hand-off inside a fused iteration launch timed out");
    if (st.status == ICP_ERR_INVALID_JACOBIAN)
        return fail(ctx, ICP_ERR_INVALID_JACOBIAN, "Invalid Jacobian in Gauss Newton minimization");
    if (st.status == ICP_ERR_EXCHANGE) {
        // the ranks' sequence counters and inbox tags may have diverged (a rank that timed out did not advance, one that
        // received everything did): the exchange is unusable until it is created and connected again
        ctx->exchange_on = false;
        return fail(ctx, ICP_ERR_EXCHANGE, "multi-GPU exchange: a peer did not deliver its normal equations in time; "
                                           "the context left exchange mode (icp_exchange_create / _connect again)");
    }
    return st.status;
}

// enqueues iterations [first, first + count) of the registration in progress (count < 0: all of them)
static int enqueue_iterations(icp_ctx* ctx, bool poll_allowed, int first, int count) {
    int rc = ICP_OK;
    const int iters = count < 0 ? ctx->cfg.max_num_alignments
                                : (first + count < ctx->cfg.max_num_alignments ? first + count : ctx->cfg.max_num_alignments);
    // the loop never converges early when the threshold is <= 0 (forced iteration count): no point polling
    const int poll = (poll_allowed && ctx->cfg.threshold_delta_pose > 0.f) ? ctx->cfg.poll_every : 0;
    // lead launches: the solve of iteration k rides in the head of launch k + 1 (LeadArgs, icp_internal.h); one summing /
    // solving launch remains, behind the last iteration.  Not with the host polling in between (it reads the RegState,
    // which would lag one iteration) and not with the in-library exchange (its solve waits for the peers)
    const bool lead = ctx->lead_latched && fused_path(ctx) && !ctx->exchange_on && poll == 0;
    int prev_rows = 0, prev_quad = 1;  // rows a lead launch still has to solve
    for (int it = first; it < iters; ++it) {
        if (lead && fused_tail_possible(ctx, prev_rows, iters - it)) {
            // the resident tail: every remaining iteration, and the solve behind the last one, in ONE launch
            int rows = 0, quad = 1;
            rc = launch_iterate_fused(ctx, &rows, &quad, true, prev_rows, prev_quad, iters - it);
            if (rc) {
                ctx->in_registration = false;
                return rc;
            }
            break;
        }
        if (lead) {
            // every launch takes its pose from the mailbox; the NARROW ones (late iterations: one workgroup more fits beside
            // the others) also solve the iteration before them, the others follow a summing / solving launch as before
            int rows = 0, quad = 1;
            rc = launch_iterate_fused(ctx, &rows, &quad, true, prev_rows, prev_quad);
            prev_rows = rows;
            prev_quad = quad;
            // (rows of a dense launch: four times as many, a quarter of a microsecond each for ONE lead workgroup — with
            // "lead_after_dense" = 0 they keep their own summing launch and the lead chain starts one iteration later)
            if (!rc && (it + 1 == iters || !next_fused_launch_is_narrow(ctx) || (quad && !ctx->lead_after_dense))) {
                // the rows of this launch: the parity it has just written
                rc = launch_sum_solve(ctx, rows, quad, (const double*)(ctx->partials.as<char>() +
                                                                       (size_t)(ctx->partials_parity ^ 1) * ctx->partials_half),
                                      true, it + 1 == iters);
                prev_rows = 0;
            }
        } else if (fused_path(ctx)) {
            int rows = 0, quad = 1;
            rc = launch_iterate_fused(ctx, &rows, &quad);
            if (!rc) rc = launch_sum_solve(ctx, rows, quad, nullptr, false, it + 1 == iters && poll == 0);
        } else if (ctx->cost == ICP_COST_POINT_TO_POINT) {
            (rc = launch_search(ctx)) || (rc = launch_reduce_p2p(ctx, true));
            ctx->iter_in_registration += 1;  // (the fused launch counts itself)
        } else {
            (rc = launch_search(ctx)) || (rc = launch_normals(ctx)) || (rc = launch_reduce_solve(ctx));
            ctx->iter_in_registration += 1;
        }
        if (rc) {
            ctx->in_registration = false;
            return rc;
        }
        if (poll > 0 && (it + 1) % poll == 0 && it + 1 < iters) {
            int done = 0;
            if ((rc = poll_done(ctx, &done))) {
                // (icp_register's RegisteringGuard leaves the count only for a context that is not "in registration")
                ctx->in_registration = false;
                return rc;
            }
            if (done) break;
        }
    }
    return ICP_OK;
}

static int register_launch(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode,
                           const float init_pose[16], bool from_last) {
    if (!ctx) return ICP_ERR_INVALID_ARGUMENT;
    RegisteringGuard leave_on_error(ctx);
    if (ctx->r_count >= 2) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "two results are already pending");
    int rc = continue_launch(ctx, -1);  // (an older launch still holding iterations back: they come first on the stream)
    if (rc) return rc;
    rc = register_begin(ctx, xyz, n, mem, target_mode, init_pose, from_last, nullptr, true);
    if (rc) return rc;
    // forced iteration count (threshold <= 0): every iteration is enqueued.  Live threshold: a first chunk of as many
    // iterations as the last frame ran plus one (launches behind an early stop would see `done` on the device and return
    // at once — but each still costs its slot on the stream, twenty of them more than the three that do the work);
    // icp_register_end enqueues further chunks while the loop is still running
    const int iters = ctx->cfg.max_num_alignments;
    // (lead launches that end in a resident tail run to the end of the loop on the device: nothing to chunk)
    const bool tail = ctx->lead_latched && fused_path(ctx) && !ctx->exchange_on && fused_tail_planned(ctx, iters);
    const int first_chunk = first_chunk_iterations(iters, ctx->cfg.threshold_delta_pose, ctx->chunked_launch, tail,
                                                   &ctx->last_iterations, 1);
    rc = result_fold_begin(ctx, false);  // (the last solving launch of the chunk delivers the result block itself)
    // (a first chunk holds at least one iteration — first_chunk_iterations — so launch 0 is never held back by the chunking)
    if (!rc) rc = enqueue_iterations(ctx, false, 0, first_chunk);
    if (!rc) rc = first_pack_flush(ctx);  // (nothing unless no fused launch took it over)
    ctx->first_pending = false;
    return result_hand_over(ctx, rc, first_chunk, iters - first_chunk);
}

int icp_register_launch(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16]) {
    DeviceGuard device_guard(ctx);
    return register_launch(ctx, xyz, n, mem, target_mode, init_pose, false);
}

int icp_register_launch_from_last(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode) {
    DeviceGuard device_guard(ctx);
    return register_launch(ctx, xyz, n, mem, target_mode, nullptr, true);
}

int icp_register(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16],
                 icp_register_result* result, double* loss_per_iter_out, float* dx_per_iter_out) {
    DeviceGuard device_guard(ctx);
    if (!ctx || !result) return ICP_ERR_INVALID_ARGUMENT;
    RegisteringGuard leave_on_error(ctx);
    int rc = icp_register_begin(ctx, xyz, n, mem, target_mode, init_pose);
    if (rc) return rc;
    if ((rc = enqueue_iterations(ctx, true))) return rc;
    return register_collect(ctx, result, loss_per_iter_out, dx_per_iter_out);
}

// icp_pmap_register, enqueued: begin + every iteration on the stream, the result block delivered to its pinned slot behind the
// last one, collected by icp_register_end.  The kernels of an iteration behind the stop return at once (RegState.done): no host
// poll decides anything, and the iterations that run are those of icp_pmap_register — the same bits.
int icp_pmap_register_launch(icp_ctx* ctx, const float* xyz, int64_t n, int mem, int target_mode, const float init_pose[16]) {
    DeviceGuard device_guard(ctx);
    if (!ctx || n < 0 || (n > 0 && !xyz)) return ICP_ERR_INVALID_ARGUMENT;
    if (ctx->in_registration || ctx->result_pending())
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_pmap_register_launch: a registration of this context is in progress or "
                                                   "awaits icp_register_end");
    int rc = continue_launch(ctx, -1);  // (refuses a context whose batch still holds iterations back)
    if (rc) return rc;
    if (ctx->pm_slots.empty()) return fail(ctx, ICP_ERR_EMPTY_MAP, "the local map is empty");
    if ((rc = pmap_register_begin(ctx, xyz, n, mem, target_mode, init_pose, false, nullptr, true))) return rc;
    const int iters = ctx->cfg.max_num_alignments;
    rc = result_fold_begin(ctx, false);  // (the last solving launch delivers the result block itself)
    for (int it = 0; !rc && it < iters; ++it) {
        int blocks = 0;
        rc = pmap_iterate(ctx, &blocks);
        if (!rc) rc = launch_sum_solve(ctx, blocks, 1, nullptr, false, it + 1 == iters);
    }
    return result_hand_over(ctx, rc, iters, 0);
}

