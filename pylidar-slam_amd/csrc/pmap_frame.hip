// One call per odometry frame against the projective local map: icp_pmap_odometry_init / icp_pmap_frame_launch /
// icp_pmap_frame_end (include/icp_mi355x.h).  ICPFrameToModel.do_process_next_frame (slam/odometry/icp_odometry.py:157-246) with
// ProjectiveLocalMap (slam/odometry/local_map.py:113-235), composed from the entry points of api.hip in the order
// pylidar_slam_amd/odometry.py::MI355XICPFrameToModel issues them; host code only — every launch is one of theirs.  What is
// particular to the projective map lives here — the refusals, the input section of the launch, the update call; every other
// step of a frame is frame.hip's (frame_loop.h).
#include <string.h>

#include "frame_loop.h"
#include "icp_internal.h"

using namespace icp;

namespace {

int pframe_fail(icp_ctx* ctx, const std::string& msg) { return fail(ctx, ICP_ERR_INVALID_ARGUMENT, msg.c_str()); }

// what the projective frame calls refuse whatever the state of the loop
int pframe_refusals(icp_ctx* ctx, const char* who) {
    if (ctx->cost != ICP_COST_POINT_TO_PLANE)
        return pframe_fail(ctx, std::string(who) + ": the context runs point-to-point (the projective map registers point-to-plane)");
    if (ctx->exchange_on) return pframe_fail(ctx, std::string(who) + ": a multi-GPU exchange is switched on");
    if (ctx->prof.enabled) return pframe_fail(ctx, std::string(who) + ": profiling is switched on");
    if (ctx->batch_hold) return pframe_fail(ctx, std::string(who) + ": the context is held by a batched registration");
    if (ctx->frame)
        return pframe_fail(ctx, std::string(who) + ": a kd-tree sequence (icp_odometry_init) runs on this context");
    return ICP_OK;
}

}  // namespace

namespace icp {

void pmap_frame_loop_release(icp_ctx* ctx) {
    icp_pmap_frame_loop* f = ctx ? ctx->pframe : nullptr;
    if (!f) return;
    frame_buffers_release(&f->io);
    delete f;
    ctx->pframe = nullptr;
}

// what icp_pmap_odometry_init refuses, nothing changed (icp_batch_pmap_odometry_init asks every member first)
int pmap_frame_init_check(icp_ctx* ctx, const icp_pmap_frame_config* cfg, bool own_batch) {
    int rc = pframe_refusals(ctx, "icp_pmap_odometry_init");
    if (rc) return rc;
    if ((cfg->targets != 0 && cfg->targets != 1) || !(cfg->threshold_trans >= 0.f) || !(cfg->threshold_rot >= 0.f))
        return pframe_fail(ctx, "icp_pmap_odometry_init: targets is 0 or 1, the key-frame thresholds are not negative");
    if (cfg->normals_kernel_size < 1 || cfg->normals_kernel_size > 15 || !(cfg->normals_kernel_size & 1))
        return pframe_fail(ctx, "icp_pmap_odometry_init: normals_kernel_size must be odd, 1..15");
    const icp_pmap_frame_loop* f = ctx->pframe;
    if (!own_batch && f && f->seq.launched && f->seq.batched)
        return pframe_fail(ctx, "icp_pmap_odometry_init: a frame launched by a batch awaits icp_batch_pmap_frame_end");
    if ((ctx->in_registration || ctx->result_pending()) && !(f && f->seq.launched && f->seq.registered))
        return pframe_fail(ctx, "icp_pmap_odometry_init: a registration of this context is in progress or awaits icp_register_end");
    return ICP_OK;
}

}  // namespace icp

extern "C" {

void icp_default_pmap_frame_config(icp_pmap_frame_config* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->voxel_size = 0.0;
    cfg->threshold_trans = 0.1f;  // icp_odometry.py:29-64
    cfg->threshold_rot = 0.3f;
    cfg->constant_velocity = 1;
    cfg->targets = 0;
    cfg->normals_kernel_size = 5;  // local_map.py:91-111
    cfg->copy_cloud = 1;
}

int icp_pmap_odometry_init(icp_ctx* ctx, const icp_pmap_frame_config* cfg) {
    if (!ctx || !cfg) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(ctx, false);
    int rc = pmap_frame_init_check(ctx, cfg, false);
    if (rc) return rc;
    icp_pmap_frame_loop* f = ctx->pframe;
    if (!f) f = ctx->pframe = new icp_pmap_frame_loop();
    frame_drop_pending(ctx, &f->seq, &f->io);
    if ((rc = icp_pmap_init(ctx))) return rc;
    f->cfg = *cfg;
    f->seq.index = 0;
    pose_identity(f->seq.delta);
    pose_identity(f->seq.last_pose);
    return ICP_OK;
}

int icp_pmap_frame_launch(icp_ctx* ctx, const float* data, int64_t n, int mem, int layout, const double* timestamps,
                          const float init_pose[16]) {
    if (!ctx) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(ctx, false);
    icp_pmap_frame_loop* f = ctx->pframe;
    if (!f) return pframe_fail(ctx, "icp_pmap_frame_launch: no sequence (icp_pmap_odometry_init first)");
    int rc = pframe_refusals(ctx, "icp_pmap_frame_launch");
    if (rc) return rc;
    if (f->seq.launched) return pframe_fail(ctx, "icp_pmap_frame_launch: a frame is already launched (icp_pmap_frame_end first)");
    const icp_pmap_frame_config& c = f->cfg;
    const int64_t npix = (int64_t)ctx->cfg.height * ctx->cfg.width;
    if (layout != ICP_FRAME_ROWS && layout != ICP_FRAME_VERTEX_MAP)
        return pframe_fail(ctx, "icp_pmap_frame_launch: layout is ICP_FRAME_ROWS or ICP_FRAME_VERTEX_MAP");
    if (n < 0 || n > INT32_MAX || (n > 0 && !data) || (mem != ICP_MEM_HOST && mem != ICP_MEM_DEVICE))
        return pframe_fail(ctx, "icp_pmap_frame_launch: [n,3] rows in host or device memory, or a [3,H,W] vertex map, are required");
    const bool from_vmap = layout == ICP_FRAME_VERTEX_MAP;
    if (from_vmap && (n != npix || !data))
        return pframe_fail(ctx, "icp_pmap_frame_launch: a vertex map has n = H*W pixels (the context's height x width)");
    if (from_vmap && mem != ICP_MEM_DEVICE)
        return pframe_fail(ctx, "icp_pmap_frame_launch: a vertex map is taken from device memory");
    if (from_vmap && (timestamps || c.voxel_size > 0))
        return pframe_fail(ctx, "icp_pmap_frame_launch: timestamps and a grid sample (voxel_size > 0) go with rows, not with a vertex map");
    if (ctx->in_registration || ctx->result_pending())
        return pframe_fail(ctx, "icp_pmap_frame_launch: a registration of this context is in progress or awaits icp_register_end");
    // ---- the initial guess (ConstantVelocityInitialization, slam/initialization.py:103-119)
    const bool have_guess = init_pose != nullptr || c.constant_velocity != 0;
    const float* guess = init_pose ? init_pose : f->seq.last_pose;
    float eye[16];
    pose_identity(eye);
    f->seq.n = n;
    f->seq.sampled = false;
    f->io.copy_started = false;
    f->seq.staged = false;
    // ---- input: the targets, the rows odometry_pc is made of, the vertex map a key frame inserts
    const float* targets = nullptr;
    int64_t n_targets = 0;
    int target_mode = ICP_TARGETS_ALL;
    const float* rows = data;
    bool project_behind = false;
    if (from_vmap) {
        f->frame_vmap = data;
        if (f->seq.index > 0) {  // the pixels as rows (sample_points :301-308)
            ICP_HIP(ctx, f->io.rows.reserve((size_t)npix * 12));
            if ((rc = vmap_rows_device(ctx, data, f->io.rows.as<float>()))) return rc;
        }
        targets = f->valid_rows = f->io.rows.as<float>();
        n_targets = npix;
        target_mode = f->valid_mode = ICP_TARGETS_SKIP_NULL;
    } else {
        const double* ts = timestamps;
        if (n > 0 && mem == ICP_MEM_HOST && (rc = frame_upload(ctx, &f->io, data, timestamps, n, &rows, &ts))) return rc;
        if ((rc = frame_preprocess_device(ctx, &f->io, c.voxel_size, rows, n, ts, have_guess ? guess : nullptr, &rows, &f->seq.sampled)))
            return rc;
        ICP_HIP(ctx, f->io.vmap.reserve((size_t)npix * 12));
        f->frame_vmap = f->io.vmap.as<float>();
        f->valid_rows = rows;
        f->valid_mode = ICP_TARGETS_ALL;
        if (f->seq.index == 0) {
            if ((rc = icp_project(ctx, rows, n, ICP_MEM_DEVICE, f->io.vmap.as<float>(), nullptr, ICP_MEM_DEVICE))) return rc;
        } else if (c.targets == 1) {
            ICP_HIP(ctx, f->io.rows.reserve((size_t)npix * 12));
            if ((rc = icp_project_rows(ctx, rows, n, f->io.vmap.as<float>(), f->io.rows.as<float>()))) return rc;
            targets = f->io.rows.as<float>();
            n_targets = npix;
            target_mode = ICP_TARGETS_SKIP_NULL;
        } else {  // (the vertex map is read by a key frame's insertion only: projected behind the registration)
            targets = rows;
            n_targets = n;
            project_behind = true;
        }
    }
    // ---- frame 0: the vertex map goes into the map (:176)
    if (f->seq.index == 0) {
        if (f->seq.sampled) {  // (collected in icp_pmap_frame_end)
            if (!f->io.pin_count) ICP_HIP(ctx, hipHostMalloc((void**)&f->io.pin_count, sizeof(int), hipHostMallocDefault));
            ICP_HIP(ctx, hipMemcpyAsync(f->io.pin_count, f->io.count.ptr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        }
        if ((rc = icp_pmap_update(ctx, eye, f->frame_vmap, ICP_MEM_DEVICE, c.normals_kernel_size))) return rc;
        f->seq.launched = true;
        f->seq.registered = false;
        return ICP_OK;
    }
    // ---- later frames: the valid rows compacted and on their way to the host, then the registration
    f->seq.staged = n > 0 && (f->seq.sampled || c.copy_cloud != 0);
    if (f->seq.staged && (rc = icp_map_stage_cloud(ctx, f->valid_rows, n, ICP_MEM_DEVICE, f->valid_mode))) return rc;
    if (f->seq.staged && (rc = frame_copy_start(ctx, &f->io, f->seq.sampled, c.copy_cloud != 0, n))) return rc;
    rc = icp_pmap_register_launch(ctx, targets, n_targets, ICP_MEM_DEVICE, target_mode, have_guess ? guess : eye);
    if (rc) {
        if (f->io.copy_started) (void)hipEventSynchronize(f->io.copy_done);
        f->io.copy_started = false;
        return rc;
    }
    f->seq.launched = true;
    f->seq.registered = true;
    if (project_behind && (rc = icp_project(ctx, rows, n, ICP_MEM_DEVICE, f->io.vmap.as<float>(), nullptr, ICP_MEM_DEVICE)))
        return rc;  // (the frame stays launched: icp_pmap_frame_end collects its registration)
    return ICP_OK;
}

int icp_pmap_frame_end(icp_ctx* ctx, icp_frame_result* result, float* odometry_pc_out, int64_t cap, int64_t* rows_out,
                       int out_mem, double* loss_per_iter_out, float* dx_per_iter_out) {
    if (!ctx || !result) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(ctx, false);
    icp_pmap_frame_loop* f = ctx->pframe;
    if (!f || !f->seq.launched) return pframe_fail(ctx, "icp_pmap_frame_end: no frame launched (icp_pmap_frame_launch first)");
    if (ctx->batch_hold) return pframe_fail(ctx, "icp_pmap_frame_end: the context is held by a batched registration");
    if (f->seq.batched) return pframe_fail(ctx, "icp_pmap_frame_end: the frame was launched by a batch (icp_batch_pmap_frame_end ends it)");
    if (odometry_pc_out && cap < 0) return pframe_fail(ctx, "icp_pmap_frame_end: negative capacity");
    icp_frame_seq& s = f->seq;
    memset(result, 0, sizeof(*result));
    result->frame_index = s.index;
    if (rows_out) *rows_out = 0;
    // frame 0: the identity, the vertex map is in the map (nothing has waited for the grid sample's count yet)
    if (!s.registered) return frame_end_first(ctx, &s, &f->io, 1, true, result);
    int rc = frame_collect(ctx, &s, &f->io, result, loss_per_iter_out, dx_per_iter_out);
    if (rc) return rc;
    // ---- __update_map (:360-380) with ProjectiveLocalMap.update (local_map.py:122-174)
    const KeyFrameTest t = key_frame_test(s.delta, result->reg.pose, f->cfg.threshold_trans, f->cfg.threshold_rot);
    result->key_frame = t.key_frame;
    s.launched = s.registered = false;
    rc = icp_pmap_update(ctx, result->reg.pose, t.key_frame ? f->frame_vmap : nullptr, ICP_MEM_DEVICE, f->cfg.normals_kernel_size);
    if (!rc && t.key_frame) result->inserted = 1;
    const bool copied = f->io.copy_started && f->cfg.copy_cloud && s.n > 0;
    f->io.copy_started = false;
    if (rc) return rc;
    frame_advance(&s, t, result->reg.pose);
    return frame_deliver(ctx, "icp_pmap_frame_end", &s, &f->io, copied, !s.staged && odometry_pc_out && s.n > 0, f->valid_rows,
                         f->valid_mode, odometry_pc_out, cap, rows_out, out_mem);
}

}  // extern "C"
