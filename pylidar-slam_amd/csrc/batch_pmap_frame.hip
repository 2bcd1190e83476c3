// One call per odometry frame against the projective local map for B sequences: icp_batch_pmap_odometry_init /
// icp_batch_pmap_frame_launch / icp_batch_pmap_frame_end (include/icp_mi355x.h).  icp_pmap_frame_launch / icp_pmap_frame_end
// (pmap_frame.hip) for the members of a batch, the registering members' stages going through the BATCHED entry points of
// api.hip — icp_batch_preprocess, _project_rows, _stage, _pmap_register_launch, _register_end, _pmap_update — stage by stage
// as the single calls do.  The sequence state is each member's own icp_pmap_frame_loop (frame_loop.h); who takes part in a step and what is
// refused is decided in batch_pmap_frame_plan.h.  What is particular to the projective form lives here: its plan, the
// target-building middle of the launch with its failure path behind the registrations, and the batched update; the rest is
// batch_frame.hip's (batch_frame_loop.h), driven by batch_frame_pmap().
#include <string.h>

#include <algorithm>
#include <vector>

#include "batch_frame_loop.h"

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
        m.frame_index = f ? f->seq.index : 0;
        m.voxel_size = f ? f->cfg.voxel_size : 0.0;
        m.targets = f ? f->cfg.targets : 0;
        m.normals_kernel_size = f ? f->cfg.normals_kernel_size : 0;
        m.point_to_point = ctx->cost != ICP_COST_POINT_TO_PLANE;
        m.exchange = ctx->exchange_on;
        m.profiling = ctx->prof.enabled != 0;
        m.registering = ctx->in_registration || ctx->result_pending() || ctx->batch_hold;
        m.frame_launched = f && f->seq.launched;
        m.has_timestamps = frames[i].timestamps != nullptr;
        m.n = frames[i].n;
        m.pixels = (int64_t)ctx->cfg.height * ctx->cfg.width;
        m.stream = (uint64_t)(uintptr_t)ctx->stream;
    }
}

int pmap_first_launch(icp_ctx* ctx, const float* rows, int64_t n, int layout, const double* ts, const float init_pose[16]) {
    return icp_pmap_frame_launch(ctx, rows, n, ICP_MEM_DEVICE, layout, ts, init_pose);
}

// ONE icp_batch_pmap_update: the key frames insert their vertex map, every member's model is rebuilt
int pmap_update(icp_batch* ub, icp_ctx* const* ctxs, int nu, const float* rel, const KeyFrameTest* tests, int64_t* inserted) {
    const float* vmaps[ICP_BATCH_MAX_SEQUENCES];
    int ks = 5;
    for (int u = 0; u < nu; ++u) {
        const icp_pmap_frame_loop* f = ctxs[u]->pframe;
        vmaps[u] = tests[u].key_frame ? f->frame_vmap : nullptr;
        inserted[u] = tests[u].key_frame ? 1 : 0;
        ks = f->cfg.normals_kernel_size;
    }
    return icp_batch_pmap_update(ub, rel, vmaps, ICP_MEM_DEVICE, ks);
}

}  // namespace

namespace icp {

const BatchFrameKind& batch_frame_pmap() {
    static const BatchFrameKind kind = {
        "icp_batch_pmap_frame_launch",
        "icp_batch_pmap_frame_end",
        [](icp_ctx* ctx) {
            icp_pmap_frame_loop* f = ctx->pframe;
            return f ? BatchFrameMemberLoop{&f->seq, &f->io, f->cfg.threshold_trans, f->cfg.threshold_rot} : BatchFrameMemberLoop{};
        },
        nullptr,
        pmap_first_launch,
        icp_pmap_frame_end,
        pmap_update,
        batch_pmap_frame_end_refusal,
    };
    return kind;
}

}  // namespace icp

extern "C" {

int icp_batch_pmap_odometry_init(icp_batch* b, const icp_pmap_frame_config* cfg) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!cfg) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_odometry_init: a configuration is required");
    DeviceGuard device_guard(b->device);
    // ---- every member is checked before any member changes
    for (size_t i = 0; i < b->members.size(); ++i) {
        const int rc = pmap_frame_init_check(b->members[i], cfg, b->frames != nullptr && b->frames->pending == &batch_frame_pmap());
        if (rc) return bf_member_fail(b, rc, "icp_batch_pmap_odometry_init (nothing was changed)", (int)i);
    }
    batch_frames_drop_pending(b, &batch_frame_pmap());
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
    if (s->pending == &batch_frame_kd()) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_frame_launch: a kd-tree step of this batch awaits icp_batch_frame_end (nothing was changed)");
    if (!batch_pmap_frame_plan(members, count, s->pending == &batch_frame_pmap(), from_vmap, mem == ICP_MEM_HOST, &plan))
        return batch_frames_refuse(b, "icp_batch_pmap_frame_launch", plan);
    for (int i = 0; i < count; ++i)
        if (!frames[i].skip && frames[i].n > 0 && !frames[i].xyz)
            return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_pmap_frame_launch, member " + std::to_string(i) +
                                                            ": rows or a vertex map are required (nothing was changed)");
    const BatchFrameStep step = batch_frame_step(plan);
    BatchFrameLaunch l;
    int rc = batch_frames_launch_begin(b, batch_frame_pmap(), step, frames, mem, layout, &l);
    if (rc) return rc;
    icp_batch* rb = l.rb;
    const int nr = step.n_registering;
    if (nr > 0) {
        icp_ctx* ctxs[ICP_BATCH_MAX_SEQUENCES];
        icp_pmap_frame_loop* pl[ICP_BATCH_MAX_SEQUENCES];
        icp_frame_io* ios[ICP_BATCH_MAX_SEQUENCES];
        const float* r_rows[ICP_BATCH_MAX_SEQUENCES];
        int64_t r_n[ICP_BATCH_MAX_SEQUENCES];
        const float* guess[ICP_BATCH_MAX_SEQUENCES];
        bool have_guess[ICP_BATCH_MAX_SEQUENCES];
        const icp_pmap_frame_config c0 = b->members[step.registering[0]]->pframe->cfg;
        const size_t npix = (size_t)l.lead->cfg.height * l.lead->cfg.width;
        for (int k = 0; k < nr; ++k) {
            const int i = step.registering[k];
            ctxs[k] = b->members[i];
            pl[k] = ctxs[k]->pframe;
            ios[k] = &pl[k]->io;
            const icp_batch_frame& fr = frames[i];
            r_n[k] = fr.n;
            r_rows[k] = fr.n > 0 ? l.rows[i] : nullptr;
            have_guess[k] = fr.init_pose != nullptr || pl[k]->cfg.constant_velocity != 0;
            guess[k] = fr.init_pose ? fr.init_pose : pl[k]->seq.last_pose;
            s->sampled[i] = false;
            s->copied[i] = false;
        }
        auto member_hip = [&](int k, hipError_t e, const char* what) {
            return bf_member_hip(b, "icp_batch_pmap_frame_launch", step.registering[k], e, what);
        };
        auto give_up = [&](int code) {  // a failure behind the first frames: those frames are complete
            batch_frames_end_first(b, batch_frame_pmap(), step, step.n_first);
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
                rc = member_hip(k, ios[k]->rows.reserve(npix * 12), "reserve(rows)");
                pix[k] = ios[k]->rows.as<float>();
                pl[k]->frame_vmap = r_rows[k];
                targets[k] = valid[k] = pix[k];
                n_targets[k] = (int64_t)npix;
                ios[k]->copy_started = false;
            }
            if (rc) return give_up(rc);
            if ((rc = vmap_rows_batch_device(l.lead, nr, r_rows, pix))) return give_up(bf_member_fail(b, rc, "icp_batch_pmap_frame_launch", step.registering[0]));
            target_mode = valid_mode = ICP_TARGETS_SKIP_NULL;
        } else {
            // ---- de-skew -> grid sample -> float32, then the projection (_read_input :319-358)
            if ((rc = batch_frames_preprocess(b, rb, s, "icp_batch_pmap_frame_launch", step.registering, nr, ctxs, ios, c0.voxel_size,
                                              guess, have_guess, l.ts, r_rows, r_n)))
                return give_up(rc);
            for (int k = 0; k < nr && !rc; ++k) {
                rc = member_hip(k, ios[k]->vmap.reserve(npix * 12), "reserve(vmap)");
                if (!rc && c0.targets == 1) rc = member_hip(k, ios[k]->rows.reserve(npix * 12), "reserve(rows)");
                vmaps[k] = ios[k]->vmap.as<float>();
                pix[k] = c0.targets == 1 ? ios[k]->rows.as<float>() : nullptr;
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
        bool cloud[ICP_BATCH_MAX_SEQUENCES];
        for (int k = 0; k < nr; ++k) cloud[k] = pl[k]->cfg.copy_cloud != 0;
        if ((rc = batch_frames_copy_start(b, s, step.registering, nr, ctxs, ios, cloud, r_n))) return give_up(rc);
        float init[16 * ICP_BATCH_MAX_SEQUENCES];
        batch_frames_init_poses(guess, have_guess, nr, init);
        rc = icp_batch_pmap_register_launch(rb, targets, n_targets, ICP_MEM_DEVICE, target_mode, init, 0);
        if (rc) {
            if (s->copy_started) (void)hipEventSynchronize(s->copy_done);
            s->copy_started = false;
            return give_up(inner_fail(b, rb, rc));
        }
        for (int k = 0; k < nr; ++k) {
            icp_pmap_frame_loop* f = pl[k];
            f->seq.n = r_n[k];
            f->seq.sampled = s->sampled[step.registering[k]];
            f->valid_rows = valid[k];
            f->valid_mode = valid_mode;
            f->seq.staged = true;
            f->seq.launched = f->seq.registered = f->seq.batched = true;
        }
        if (project_behind && (rc = icp_batch_project_rows(rb, r_rows, r_n, vmaps, nullptr))) {
            // (the registrations are on the stream: the step is stored and dropped like one never ended)
            s->step = step;
            s->pending = &batch_frame_pmap();
            for (int k = 0; k < step.n_first; ++k) b->members[step.first[k]]->pframe->seq.batched = true;
            const std::string why = rb->error;
            batch_frames_drop_pending(b);
            batch_frames_end_first(b, batch_frame_pmap(), step, step.n_first);
            return bf_fail(b, rc, why);
        }
    }
    return batch_frames_launch_finish(b, batch_frame_pmap(), step, l);
}

int icp_batch_pmap_frame_end(icp_batch* b, icp_frame_result* results, float* const* odometry_pc_out, const int64_t* cap,
                             int64_t* rows_out, int out_mem, double* loss_per_iter_out, float* dx_per_iter_out) {
    return batch_frames_end(b, batch_frame_pmap(), results, odometry_pc_out, cap, rows_out, out_mem, loss_per_iter_out, dx_per_iter_out);
}

}  // extern "C"
