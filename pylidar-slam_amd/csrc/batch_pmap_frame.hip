// One call per odometry frame against the projective local map for B sequences: icp_batch_pmap_odometry_init /
// icp_batch_pmap_frame_launch / icp_batch_pmap_frame_end (include/icp_mi355x.h).  icp_pmap_frame_launch / icp_pmap_frame_end
// (pmap_frame.hip) for the members of a batch, the registering members' stages composed from the BATCHED entry points of api.hip
// — icp_batch_preprocess, _project_rows, _stage, _pmap_register_launch, _register_end, _pmap_update — in the single call's
// order.  The sequence state is each member's own icp_pmap_frame_loop (frame_loop.h); who takes part in a step and what is
// refused is decided in batch_pmap_frame_plan.h; the inner batches, the upload and the copy-out are those of batch_frame.hip
// (batch_frame_loop.h).
#include <string.h>

#include <algorithm>
#include <vector>

#include "batch_frame_loop.h"
#include "frame_keyframe.h"

using namespace icp;

static_assert(BATCH_PMAP_FRAME_MAX_MEMBERS == ICP_BATCH_MAX_SEQUENCES, "batch_pmap_frame_plan.h sizes its lists for ICP_BATCH_MAX_SEQUENCES members");

namespace {

void fill_members(icp_batch* b, const icp_batch_frame* frames, BatchPmapFrameMember* out) {
    for (size_t i = 0; i < b->members.size(); ++i) {
        const icp_ctx* ctx = b->members[i];
        const icp_pmap_frame_loop* f = ctx->pframe;
        BatchPmapFrameMember& m = out[i];
        memset(&m, 0, sizeof(m));
        m.skip = frames[i].skip != 0;
        m.has_sequence = f != nullptr;
        m.kd_sequence = ctx->frame != nullptr;
        m.frame_index = f ? f->index : 0;
        m.voxel_size = f ? f->cfg.voxel_size : 0.0;
        m.targets = f ? f->cfg.targets : 0;
        m.normals_kernel_size = f ? f->cfg.normals_kernel_size : 0;
        m.point_to_point = ctx->cost != ICP_COST_POINT_TO_PLANE;
        m.exchange = ctx->exchange_on;
        m.profiling = ctx->prof.enabled != 0;
        m.registering = ctx->in_registration || ctx->result_pending() || ctx->batch_hold;
        m.frame_launched = f && f->launched;
        m.has_timestamps = frames[i].timestamps != nullptr;
        m.n = frames[i].n;
        m.pixels = (int64_t)ctx->cfg.height * ctx->cfg.width;
        m.stream = (uint64_t)(uintptr_t)ctx->stream;
    }
}

int refuse(icp_batch* b, const char* who, const BatchPmapFramePlan& plan) {
    std::string msg = std::string(who);
    if (plan.refused_member >= 0) msg += ", member " + std::to_string(plan.refused_member);
    return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, msg + ": " + plan.reason + " (nothing was changed)");
}

void clear_flags(icp_batch* b, const BatchPmapFramePlan& p) {
    for (int i = 0; i < p.n_registering; ++i) {
        icp_pmap_frame_loop* f = b->members[p.registering[i]]->pframe;
        if (f && f->batched) f->launched = f->registered = f->batched = false;
    }
    for (int i = 0; i < p.n_first; ++i) {
        icp_pmap_frame_loop* f = b->members[p.first[i]]->pframe;
        if (f && f->batched) f->launched = f->registered = f->batched = false;
    }
}

}  // namespace

namespace icp {

// a step launched and never ended: its registrations are collected and dropped, its copies waited for
void batch_pmap_drop_pending(icp_batch* b) {
    icp_batch_frames* s = b ? b->frames : nullptr;
    if (!s || !s->p_pending) return;
    const BatchPmapFramePlan& p = s->p_plan;
    if (p.n_registering > 0) {
        icp_batch* rb = nullptr;
        if (subset_batch(b, p.registering, p.n_registering, &rb) == ICP_OK) {
            icp_register_result regs[ICP_BATCH_MAX_SEQUENCES];
            (void)icp_batch_register_end(rb, regs, nullptr, nullptr);
        }
    }
    if (s->copy_started) (void)hipEventSynchronize(s->copy_done);
    s->copy_started = false;
    clear_flags(b, p);
    s->p_pending = false;
}

}  // namespace icp

extern "C" {

int icp_batch_pmap_odometry_init(icp_batch* b, const icp_pmap_frame_config* cfg) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!cfg) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_odometry_init: a configuration is required");
    DeviceGuard device_guard(b->device);
    // ---- every member is checked before any member changes
    for (size_t i = 0; i < b->members.size(); ++i) {
        const int rc = pmap_frame_init_check(b->members[i], cfg, b->frames != nullptr && b->frames->p_pending);
        if (rc) return bf_member_fail(b, rc, "icp_batch_pmap_odometry_init (nothing was changed)", (int)i);
    }
    batch_pmap_drop_pending(b);
    for (size_t i = 0; i < b->members.size(); ++i) {
        const int rc = icp_pmap_odometry_init(b->members[i], cfg);
        if (rc) return bf_member_fail(b, rc, "icp_batch_pmap_odometry_init", (int)i);
    }
    return ICP_OK;
}

int icp_batch_pmap_frame_launch(icp_batch* b, const icp_batch_frame* frames, int mem, int layout) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!frames || (mem != ICP_MEM_HOST && mem != ICP_MEM_DEVICE) || (layout != ICP_FRAME_ROWS && layout != ICP_FRAME_VERTEX_MAP))
        return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_frame_launch: frames[] in host or device memory and a layout "
                                                    "(ICP_FRAME_ROWS, ICP_FRAME_VERTEX_MAP) are required (nothing was changed)");
    DeviceGuard device_guard(b->device);
    icp_batch_frames* s = frames_of(b);
    const int count = (int)b->members.size();
    const bool from_vmap = layout == ICP_FRAME_VERTEX_MAP;
    // ---- every member is looked at before any member changes
    BatchPmapFrameMember members[ICP_BATCH_MAX_SEQUENCES];
    fill_members(b, frames, members);
    BatchPmapFramePlan plan;
    if (s->pending) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_frame_launch: a kd-tree step of this batch awaits icp_batch_frame_end (nothing was changed)");
    if (!batch_pmap_frame_plan(members, count, s->p_pending, from_vmap, mem == ICP_MEM_HOST, &plan))
        return refuse(b, "icp_batch_pmap_frame_launch", plan);
    for (int i = 0; i < count; ++i)
        if (!frames[i].skip && frames[i].n > 0 && !frames[i].xyz)
            return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_frame_launch, member " + std::to_string(i) +
                                                            ": rows or a vertex map are required (nothing was changed)");
    icp_batch* rb = nullptr;
    int rc = ICP_OK;
    if (plan.n_registering > 0 && (rc = subset_batch(b, plan.registering, plan.n_registering, &rb))) return rc;
    icp_ctx* lead = b->members[plan.n_registering > 0 ? plan.registering[0] : plan.first[0]];
    hipStream_t stream = lead->stream;
    // ---- input: one upload for every member that takes part
    const float* rows[ICP_BATCH_MAX_SEQUENCES] = {};
    const double* ts[ICP_BATCH_MAX_SEQUENCES] = {};
    int32_t active[ICP_BATCH_MAX_SEQUENCES];
    int n_active = 0;
    for (int i = 0; i < count; ++i) {
        if (frames[i].skip) continue;
        active[n_active++] = i;
        rows[i] = frames[i].xyz;
        ts[i] = frames[i].timestamps;
        s->n[i] = frames[i].n;
    }
    bool uploaded = false;
    if (mem == ICP_MEM_HOST) {
        if ((rc = upload(b, s, frames, active, n_active, stream, rows, ts))) return rc;
        uploaded = true;
    }
    s->mem = mem;
    // ---- first frames: icp_pmap_frame_launch's frame 0, member by member (the rows are on the device by now)
    auto end_first = [&](int upto) {  // those frames are complete: ended here, as icp_pmap_frame_end would
        for (int k = 0; k < upto; ++k) {
            icp_frame_result dropped;
            icp_ctx* ctx = b->members[plan.first[k]];
            ctx->pframe->batched = false;
            (void)icp_pmap_frame_end(ctx, &dropped, nullptr, 0, nullptr, ICP_MEM_HOST, nullptr, nullptr);
        }
    };
    for (int k = 0; k < plan.n_first; ++k) {
        const int i = plan.first[k];
        icp_ctx* ctx = b->members[i];
        if ((rc = icp_pmap_frame_launch(ctx, rows[i], frames[i].n, ICP_MEM_DEVICE, layout, frames[i].n > 0 ? ts[i] : nullptr,
                                        frames[i].init_pose))) {
            end_first(k);
            return bf_member_fail(b, rc, "icp_batch_pmap_frame_launch", i);
        }
    }
    s->copy_started = false;
    const int nr = plan.n_registering;
    if (nr > 0) {
        icp_ctx* ctxs[ICP_BATCH_MAX_SEQUENCES];
        icp_pmap_frame_loop* pl[ICP_BATCH_MAX_SEQUENCES];
        icp_frame_loop* loops[ICP_BATCH_MAX_SEQUENCES];
        const float* r_rows[ICP_BATCH_MAX_SEQUENCES];
        int64_t r_n[ICP_BATCH_MAX_SEQUENCES];
        const float* guess[ICP_BATCH_MAX_SEQUENCES];
        bool have_guess[ICP_BATCH_MAX_SEQUENCES];
        const icp_pmap_frame_config c0 = b->members[plan.registering[0]]->pframe->cfg;
        const size_t npix = (size_t)lead->cfg.height * lead->cfg.width;
        for (int k = 0; k < nr; ++k) {
            const int i = plan.registering[k];
            ctxs[k] = b->members[i];
            pl[k] = ctxs[k]->pframe;
            loops[k] = &pl[k]->io;
            const icp_batch_frame& fr = frames[i];
            r_n[k] = fr.n;
            r_rows[k] = fr.n > 0 ? rows[i] : nullptr;
            have_guess[k] = fr.init_pose != nullptr || pl[k]->cfg.constant_velocity != 0;
            guess[k] = fr.init_pose ? fr.init_pose : pl[k]->last_pose;
            s->sampled[i] = false;
            s->copied[i] = false;
        }
        auto member_hip = [&](int k, hipError_t e, const char* what) -> int {
            if (e == hipSuccess) return ICP_OK;
            return bf_fail(b, ICP_ERR_HIP, std::string("icp_batch_pmap_frame_launch, member ") + std::to_string(plan.registering[k]) +
                                               ": " + what + ": " + hipGetErrorString(e));
        };
        auto give_up = [&](int code) {
            end_first(plan.n_first);
            return code;
        };
        const float* targets[ICP_BATCH_MAX_SEQUENCES];
        const float* valid[ICP_BATCH_MAX_SEQUENCES];
        int64_t n_targets[ICP_BATCH_MAX_SEQUENCES];
        float* vmaps[ICP_BATCH_MAX_SEQUENCES];
        float* pix[ICP_BATCH_MAX_SEQUENCES];
        int target_mode = ICP_TARGETS_ALL, valid_mode = ICP_TARGETS_ALL;
        bool project_behind = false;
        if (from_vmap) {
            // ---- the pixels as rows (sample_points :301-308): ONE transposing launch
            for (int k = 0; k < nr && !rc; ++k) {
                rc = member_hip(k, loops[k]->rows.reserve(npix * 12), "reserve(rows)");
                pix[k] = loops[k]->rows.as<float>();
                pl[k]->frame_vmap = r_rows[k];
                targets[k] = valid[k] = pix[k];
                n_targets[k] = (int64_t)npix;
                loops[k]->copy_started = false;
            }
            if (rc) return give_up(rc);
            if ((rc = vmap_rows_batch_device(lead, nr, r_rows, pix))) return give_up(bf_member_fail(b, rc, "icp_batch_pmap_frame_launch", plan.registering[0]));
            target_mode = valid_mode = ICP_TARGETS_SKIP_NULL;
        } else {
            // ---- de-skew -> grid sample -> float32, then the projection (_read_input :319-358)
            if ((rc = batch_frames_preprocess(b, rb, s, "icp_batch_pmap_frame_launch", plan.registering, nr, ctxs, loops, c0.voxel_size,
                                              guess, have_guess, ts, r_rows, r_n)))
                return give_up(rc);
            for (int k = 0; k < nr && !rc; ++k) {
                rc = member_hip(k, loops[k]->vmap.reserve(npix * 12), "reserve(vmap)");
                if (!rc && c0.targets == 1) rc = member_hip(k, loops[k]->rows.reserve(npix * 12), "reserve(rows)");
                vmaps[k] = loops[k]->vmap.as<float>();
                pix[k] = c0.targets == 1 ? loops[k]->rows.as<float>() : nullptr;
                pl[k]->frame_vmap = vmaps[k];
                valid[k] = r_rows[k];
                targets[k] = c0.targets == 1 ? pix[k] : r_rows[k];
                n_targets[k] = c0.targets == 1 ? (int64_t)npix : r_n[k];
            }
            if (rc) return give_up(rc);
            if (c0.targets == 1) {
                if ((rc = icp_batch_project_rows(rb, r_rows, r_n, vmaps, pix))) return give_up(inner_fail(b, rb, rc));
                target_mode = ICP_TARGETS_SKIP_NULL;
            } else {
                project_behind = true;  // (the vertex maps are read by a key frame's insertion only)
            }
        }
        // ---- the valid rows compacted and on their way to the host, then the registration
        if ((rc = icp_batch_stage(rb, valid, r_n, valid_mode))) return give_up(inner_fail(b, rb, rc));
        {
            bool cloud[ICP_BATCH_MAX_SEQUENCES];
            for (int k = 0; k < nr; ++k) cloud[k] = pl[k]->cfg.copy_cloud != 0;
            if ((rc = batch_frames_copy_start(b, s, plan.registering, nr, ctxs, loops, cloud, r_n))) return give_up(rc);
        }
        float init[16 * ICP_BATCH_MAX_SEQUENCES];
        for (int k = 0; k < nr; ++k) {
            if (have_guess[k]) memcpy(init + 16 * k, guess[k], 16 * sizeof(float));
            else pose_identity(init + 16 * k);
        }
        rc = icp_batch_pmap_register_launch(rb, targets, n_targets, ICP_MEM_DEVICE, target_mode, init, 0);
        if (rc) {
            if (s->copy_started) (void)hipEventSynchronize(s->copy_done);
            s->copy_started = false;
            return give_up(inner_fail(b, rb, rc));
        }
        for (int k = 0; k < nr; ++k) {
            icp_pmap_frame_loop* f = pl[k];
            f->n = r_n[k];
            f->sampled = s->sampled[plan.registering[k]];
            f->valid_rows = valid[k];
            f->valid_mode = valid_mode;
            f->staged = true;
            f->launched = f->registered = f->batched = true;
        }
        if (project_behind && (rc = icp_batch_project_rows(rb, r_rows, r_n, vmaps, nullptr))) {
            s->p_plan = plan;
            s->p_pending = true;  // (the registrations are on the stream: the step is dropped like one never ended)
            for (int k = 0; k < plan.n_first; ++k) b->members[plan.first[k]]->pframe->batched = true;
            const std::string why = rb->error;
            batch_pmap_drop_pending(b);
            end_first(plan.n_first);
            return bf_fail(b, rc, why);
        }
    }
    for (int k = 0; k < plan.n_first; ++k) b->members[plan.first[k]]->pframe->batched = true;
    if (uploaded && (rc = batch_frames_arena_read(b, s, stream))) return rc;
    s->p_plan = plan;
    s->p_pending = true;
    return ICP_OK;
}

int icp_batch_pmap_frame_end(icp_batch* b, icp_frame_result* results, float* const* odometry_pc_out, const int64_t* cap,
                             int64_t* rows_out, int out_mem, double* loss_per_iter_out, float* dx_per_iter_out) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!results) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_frame_end: results[] is required (nothing was changed)");
    DeviceGuard device_guard(b->device);
    icp_batch_frames* s = b->frames;
    if (const char* reason = batch_pmap_frame_end_refusal(s && s->p_pending))
        return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, std::string("icp_batch_pmap_frame_end: ") + reason + " (nothing was changed)");
    const int count = (int)b->members.size();
    if (odometry_pc_out && !cap) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_frame_end: odometry_pc_out needs cap[] (nothing was changed)");
    if (odometry_pc_out)
        for (int i = 0; i < count; ++i)
            if (odometry_pc_out[i] && cap[i] < 0) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_frame_end: negative capacity (nothing was changed)");
    const BatchPmapFramePlan plan = s->p_plan;
    for (int i = 0; i < count; ++i) {
        memset(&results[i], 0, sizeof(results[i]));
        results[i].frame_index = -1;  // (a skipped member's stays so)
        if (rows_out) rows_out[i] = 0;
    }
    int rc;
    // ---- first frames: the identity, the vertex map is in the map (icp_pmap_frame_end's frame 0)
    for (int k = 0; k < plan.n_first; ++k) {
        const int i = plan.first[k];
        icp_ctx* ctx = b->members[i];
        ctx->pframe->batched = false;
        if ((rc = icp_pmap_frame_end(ctx, &results[i], nullptr, 0, nullptr, out_mem, nullptr, nullptr))) {
            const std::string why = ctx->error;
            batch_pmap_drop_pending(b);
            return bf_fail(b, rc, "icp_batch_pmap_frame_end, member " + std::to_string(i) + ": " + why);
        }
    }
    const int nr = plan.n_registering;
    icp_batch* rb = nullptr;
    if (nr > 0 && (rc = subset_batch(b, plan.registering, nr, &rb))) {
        const std::string why = b->error;
        batch_pmap_drop_pending(b);
        return bf_fail(b, rc, why);
    }
    s->p_pending = false;  // from here on the step is ended whatever happens
    if (nr == 0) return ICP_OK;
    icp_ctx* ctxs[ICP_BATCH_MAX_SEQUENCES];
    icp_pmap_frame_loop* pl[ICP_BATCH_MAX_SEQUENCES];
    for (int k = 0; k < nr; ++k) {
        ctxs[k] = b->members[plan.registering[k]];
        pl[k] = ctxs[k]->pframe;
    }
    // ---- the registrations: ONE wait for all of them
    const size_t hist = (size_t)ctxs[0]->cfg.max_num_alignments;
    const size_t stride = (size_t)b->members[0]->cfg.max_num_alignments;
    std::vector<double> losses(loss_per_iter_out ? hist * nr : 0);
    std::vector<float> dxs(dx_per_iter_out ? hist * nr * 6 : 0);
    icp_register_result regs[ICP_BATCH_MAX_SEQUENCES];
    memset(regs, 0, sizeof(regs));
    const int rc_reg = icp_batch_register_end(rb, regs, loss_per_iter_out ? losses.data() : nullptr, dx_per_iter_out ? dxs.data() : nullptr);
    if (rc_reg && rb != b) b->error = rb->error;
    int rc_copy = ICP_OK;
    if (s->copy_started) rc_copy = bf_hip(b, hipEventSynchronize(s->copy_done), "hipEventSynchronize(copy_done)");
    s->copy_started = false;
    int32_t statuses[ICP_BATCH_MAX_SEQUENCES], update[ICP_BATCH_MAX_SEQUENCES], first_status = 0;
    for (int k = 0; k < nr; ++k) {
        const int i = plan.registering[k];
        icp_pmap_frame_loop* f = pl[k];
        statuses[k] = rc_reg ? regs[k].status : ICP_OK;
        results[i].reg = regs[k];
        results[i].frame_index = f->index;
        results[i].samples = s->sampled[i] ? (int64_t)s->pin_counts[i] : f->n;
        const size_t its = (size_t)std::max(0, std::min(regs[k].iterations, (int)std::min(hist, stride)));
        if (loss_per_iter_out) memcpy(loss_per_iter_out + (size_t)i * stride, losses.data() + (size_t)k * hist, its * sizeof(double));
        if (dx_per_iter_out) memcpy(dx_per_iter_out + (size_t)i * stride * 6, dxs.data() + (size_t)k * hist * 6, its * 6 * sizeof(float));
        f->launched = f->registered = f->batched = false;
        f->io.copy_started = false;
    }
    if (rc_copy) return rc_copy;
    const int nu = batch_frame_update_members(plan.registering, statuses, nr, update, &first_status);
    if (rc_reg && !first_status) return rc_reg;  // (a failure of the call itself, not of a member's registration)
    // ---- __update_map (:360-380) for the members that registered: the key-frame tests, then ONE batched update
    if (nu > 0) {
        icp_batch* ub = nullptr;
        if ((rc = subset_batch(b, update, nu, &ub))) return rc;
        float rel[16 * ICP_BATCH_MAX_SEQUENCES];
        const float* vmaps[ICP_BATCH_MAX_SEQUENCES];
        KeyFrameTest tests[ICP_BATCH_MAX_SEQUENCES];
        int ks = 5;
        for (int u = 0; u < nu; ++u) {
            const int i = update[u];
            icp_pmap_frame_loop* f = b->members[i]->pframe;
            tests[u] = key_frame_test(f->delta, results[i].reg.pose, f->cfg.threshold_trans, f->cfg.threshold_rot);
            vmaps[u] = tests[u].key_frame ? f->frame_vmap : nullptr;
            memcpy(rel + 16 * u, results[i].reg.pose, 16 * sizeof(float));
            ks = f->cfg.normals_kernel_size;
        }
        if ((rc = icp_batch_pmap_update(ub, rel, vmaps, ICP_MEM_DEVICE, ks))) return inner_fail(b, ub, rc);
        for (int u = 0; u < nu; ++u) {
            const int i = update[u];
            icp_pmap_frame_loop* f = b->members[i]->pframe;
            results[i].key_frame = tests[u].key_frame;
            results[i].inserted = tests[u].key_frame ? 1 : 0;
            if (tests[u].key_frame) pose_identity(f->delta);
            else memcpy(f->delta, tests[u].new_delta, sizeof(f->delta));
            memcpy(f->last_pose, results[i].reg.pose, sizeof(f->last_pose));
            f->index += 1;
        }
    }
    // ---- odometry_pc (:210-213, :243): the valid rows the staging compacted, in order
    int rc_cap = ICP_OK;
    bool wait_stream = false;
    for (int u = 0; u < nu; ++u) {
        const int i = update[u];
        icp_ctx* ctx = b->members[i];
        const int64_t valid = s->n[i] > 0 ? (int64_t)*ctx->staged_count_host : 0;
        if (rows_out) rows_out[i] = valid;
        float* out = odometry_pc_out ? odometry_pc_out[i] : nullptr;
        if (!out) continue;
        if (valid > cap[i]) {
            if (!rc_cap)
                rc_cap = bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_frame_end, member " + std::to_string(i) +
                                                                  ": odometry_pc_out holds fewer rows than the frame has (count in rows_out)");
            continue;
        }
        if (valid <= 0) continue;
        if (out_mem == ICP_MEM_HOST && s->copied[i]) {
            memcpy(out, (char*)s->pin_out + s->out_offset[i], (size_t)valid * 12);
        } else {
            BF_HIP(b, hipMemcpyAsync(out, ctx->staged_xyz.ptr, (size_t)valid * 12,
                                     out_mem == ICP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
            wait_stream = wait_stream || out_mem == ICP_MEM_HOST;
        }
    }
    if (wait_stream) BF_HIP(b, hipStreamSynchronize(ctxs[0]->stream));
    if (first_status) {
        if (rb == b || !b->error.empty()) return first_status;
        return bf_fail(b, first_status, "icp_batch_pmap_frame_end: a member's registration failed (results[b].reg.status)");
    }
    return rc_cap;
}

}  // extern "C"
