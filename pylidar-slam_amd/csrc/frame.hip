// One call per odometry frame: icp_odometry_init / icp_frame_launch / icp_frame_end (include/icp_mi355x.h).
// ICPFrameToModel.do_process_next_frame (slam/odometry/icp_odometry.py:157-246) composed from the entry points of api.hip in
// the order pylidar_slam_amd/odometry.py::MI355XICPFrameToModel issues them; host code only — every launch is one of theirs.
// Also the steps of a frame that do not depend on the map (frame_loop.h): the upload, the preprocessing chain, the copy-out,
// a pending frame dropped, frame 0's end, the registration collected, the key-frame outcome applied, odometry_pc delivered —
// the projective frame calls (pmap_frame.hip) and the batched ones (batch_frame.hip) go through the same functions.
#include <string.h>

#include "frame_loop.h"
#include "icp_internal.h"

using namespace icp;


namespace {

int frame_fail(icp_ctx* ctx, const std::string& msg) { return fail(ctx, ICP_ERR_INVALID_ARGUMENT, msg.c_str()); }

// what the frame calls refuse whatever the state of the loop
int frame_refusals(icp_ctx* ctx, const char* who) {
    if (!ctx->pm_slots.empty())
        return frame_fail(ctx, std::string(who) + ": the context holds a projective map (the frame calls run the kd-tree style map)");
    if (ctx->exchange_on) return frame_fail(ctx, std::string(who) + ": a multi-GPU exchange is switched on");
    if (ctx->prof.enabled) return frame_fail(ctx, std::string(who) + ": profiling is switched on");
    if (ctx->batch_hold) return frame_fail(ctx, std::string(who) + ": the context is held by a batched registration");
    return ICP_OK;
}

}  // namespace

namespace icp {

// ---- the steps shared with the projective frame calls (pmap_frame.hip) and the batched ones: frame_loop.h
void frame_drop_pending(icp_ctx* ctx, icp_frame_seq* s, icp_frame_io* io) {
    if (!s->launched) return;
    if (s->registered && ctx->result_pending()) {
        icp_register_result r;
        (void)register_collect(ctx, &r, nullptr, nullptr);
    }
    if (io->copy_started) (void)hipEventSynchronize(io->copy_done);
    io->copy_started = false;
    s->launched = s->registered = false;
}

int frame_end_first(icp_ctx* ctx, icp_frame_seq* s, const icp_frame_io* io, int64_t inserted, bool wait_count,
                    icp_frame_result* result) {
    if (wait_count && s->sampled) ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the grid sample's count)
    pose_identity(result->reg.pose);
    result->key_frame = 1;
    result->inserted = inserted;
    result->samples = s->sampled ? (int64_t)*io->pin_count : s->n;
    s->launched = false;
    s->index += 1;
    return ICP_OK;
}

int frame_collect(icp_ctx* ctx, icp_frame_seq* s, icp_frame_io* io, icp_frame_result* result, double* loss_per_iter_out,
                  float* dx_per_iter_out) {
    const int rc = register_collect(ctx, &result->reg, loss_per_iter_out, dx_per_iter_out);
    if (io->copy_started) ICP_HIP(ctx, hipEventSynchronize(io->copy_done));
    result->samples = s->sampled && io->copy_started ? (int64_t)*io->pin_count : s->n;
    if (rc) {
        s->launched = s->registered = false;
        io->copy_started = false;
    }
    return rc;
}

void frame_advance(icp_frame_seq* s, const KeyFrameTest& t, const float pose[16]) {
    if (t.key_frame) pose_identity(s->delta);
    else memcpy(s->delta, t.new_delta, sizeof(s->delta));
    memcpy(s->last_pose, pose, sizeof(s->last_pose));
    s->index += 1;
}

int frame_deliver(icp_ctx* ctx, const char* who, const icp_frame_seq* s, const icp_frame_io* io, bool copied, bool stage_late,
                  const float* rows, int mode, float* odometry_pc_out, int64_t cap, int64_t* rows_out, int out_mem) {
    int rc;
    if (stage_late) {  // (not staged in front of the registration: compacted now)
        if ((rc = icp_map_stage_cloud(ctx, rows, s->n, ICP_MEM_DEVICE, mode))) return rc;
        ICP_HIP(ctx, hipEventSynchronize(ctx->staged_event));
    }
    const int64_t valid = s->n > 0 && (s->staged || odometry_pc_out) ? (int64_t)*ctx->staged_count_host : 0;
    if (rows_out) *rows_out = valid;
    if (!odometry_pc_out) return ICP_OK;
    if (valid > cap)
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT,
                    (std::string(who) + ": odometry_pc_out holds fewer rows than the frame has (count in *rows_out)").c_str());
    if (valid > 0 && out_mem == ICP_MEM_HOST && copied) {
        memcpy(odometry_pc_out, io->pin_out, (size_t)valid * 12);
    } else if (valid > 0) {
        // (not copied ahead, or a device buffer: behind the map update just enqueued, which reads the staged rows and
        // leaves them as they are)
        ICP_HIP(ctx, hipMemcpyAsync(odometry_pc_out, ctx->staged_xyz.ptr, (size_t)valid * 12,
                                    out_mem == ICP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
        if (out_mem == ICP_MEM_HOST) ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return ICP_OK;
}

int pinned_reserve(icp_ctx* ctx, void** ptr, size_t* have, size_t need) {
    if (*ptr && *have >= need) return ICP_OK;
    if (*ptr) ICP_HIP(ctx, hipHostFree(*ptr));
    *ptr = nullptr;
    *have = 0;
    size_t cap = need + need / 2 + 256;
    ICP_HIP(ctx, hipHostMalloc(ptr, cap, hipHostMallocDefault));
    *have = cap;
    return ICP_OK;
}

// host rows (and timestamps) -> pinned buffer -> the next device slot, on the upload stream; the context's stream waits
int frame_upload(icp_ctx* ctx, icp_frame_io* f, const float* xyz, const double* ts, int64_t n, const float** rows_out,
                 const double** ts_out) {
    const size_t row_bytes = ((size_t)n * 12 + 7) & ~(size_t)7;  // (the timestamps behind the rows, 8-byte aligned)
    const size_t bytes = row_bytes + (ts ? (size_t)n * 8 : 0);
    if (f->pin_in_busy) {  // the previous upload has left the staging buffer (long done in practice)
        ICP_HIP(ctx, hipEventSynchronize(f->pin_in_free));
        f->pin_in_busy = false;
    }
    int rc = pinned_reserve(ctx, &f->pin_in, &f->pin_in_bytes, bytes);
    if (rc) return rc;
    memcpy(f->pin_in, xyz, (size_t)n * 12);
    if (ts) memcpy((char*)f->pin_in + row_bytes, ts, (size_t)n * 8);
    if (!f->upload_stream) ICP_HIP(ctx, hipStreamCreateWithFlags(&f->upload_stream, hipStreamNonBlocking));
    if (!f->pin_in_free) ICP_HIP(ctx, hipEventCreateWithFlags(&f->pin_in_free, hipEventDisableTiming));
    // two device slots, alternating: the DMA does not wait for the context's stream, so it must not land in memory that work
    // queued there still reads — the last reader of a slot is the registration of its own frame or, for a key frame that was
    // not staged, the icp_map_update enqueued by its icp_frame_end: both lie on the stream in front of the registration of the
    // frame in between, which icp_frame_end has collected before this upload starts
    f->which ^= 1;
    DeviceBuffer& slot = f->slot[f->which];
    ICP_HIP(ctx, slot.reserve(bytes));
    ICP_HIP(ctx, hipMemcpyAsync(slot.ptr, f->pin_in, bytes, hipMemcpyHostToDevice, f->upload_stream));
    ICP_HIP(ctx, hipEventRecord(f->pin_in_free, f->upload_stream));
    f->pin_in_busy = true;
    ICP_HIP(ctx, hipStreamWaitEvent(ctx->stream, f->pin_in_free, 0));
    *rows_out = slot.as<float>();
    *ts_out = ts ? (const double*)(slot.as<char>() + row_bytes) : nullptr;
    return ICP_OK;
}

// de-skew -> grid sample -> float32 (slam/preprocessing.py:144-191, :207-226, :101-126) of device rows, into the io
// buffers; guess = NULL: no de-skew.  *rows_out: the rows the frame goes on with (the input itself when nothing applies)
int frame_preprocess_device(icp_ctx* ctx, icp_frame_io* f, double voxel_size, const float* rows, int64_t n, const double* ts,
                            const float* guess, const float** rows_out, bool* sampled_out) {
    int rc;
    const bool skew = n > 0 && ts != nullptr && guess != nullptr;
    const bool sample = n > 0 && voxel_size > 0;
    if (skew) {
        double rel[16];
        for (int i = 0; i < 16; ++i) rel[i] = (double)guess[i];
        ICP_HIP(ctx, f->skew64.reserve((size_t)n * 24));
        if ((rc = distort_device(ctx, rows, ts, n, rel, f->skew64.as<double>()))) return rc;
    }
    if (sample || skew) ICP_HIP(ctx, f->samp32.reserve((size_t)n * 12));
    ICP_HIP(ctx, f->count.reserve(64));
    if (sample && skew) {
        ICP_HIP(ctx, f->samp64.reserve((size_t)n * 24));
        if ((rc = icp_grid_sample_padded_f64(ctx, f->skew64.as<double>(), n, voxel_size, nullptr, f->samp64.as<double>(),
                                             f->count.as<int32_t>())))
            return rc;
        if ((rc = rows_to_f32_device(ctx, f->samp64.as<double>(), 3 * n, f->samp32.as<float>()))) return rc;
        rows = f->samp32.as<float>();
    } else if (sample) {
        if ((rc = icp_grid_sample_padded(ctx, rows, n, voxel_size, nullptr, f->samp32.as<float>(), f->count.as<int32_t>())))
            return rc;
        rows = f->samp32.as<float>();
    } else if (skew) {
        if ((rc = rows_to_f32_device(ctx, f->skew64.as<double>(), 3 * n, f->samp32.as<float>()))) return rc;
        rows = f->samp32.as<float>();
    }
    *rows_out = rows;
    *sampled_out = sample;
    return ICP_OK;
}

// the staged rows (and the grid sample's count) towards pinned memory, beside the registration: behind the staging (its
// event), on a stream of the loop's own
int frame_copy_start(icp_ctx* ctx, icp_frame_io* f, bool sample, bool cloud, int64_t n) {
    int rc;
    if (!f->copy_stream) ICP_HIP(ctx, hipStreamCreateWithFlags(&f->copy_stream, hipStreamNonBlocking));
    if (!f->copy_done) ICP_HIP(ctx, hipEventCreateWithFlags(&f->copy_done, hipEventDisableTiming));
    if (!f->pin_count) ICP_HIP(ctx, hipHostMalloc((void**)&f->pin_count, sizeof(int), hipHostMallocDefault));
    ICP_HIP(ctx, hipStreamWaitEvent(f->copy_stream, ctx->staged_event, 0));
    if (sample)
        ICP_HIP(ctx, hipMemcpyAsync(f->pin_count, f->count.ptr, sizeof(int), hipMemcpyDeviceToHost, f->copy_stream));
    if (cloud) {
        if ((rc = pinned_reserve(ctx, &f->pin_out, &f->pin_out_bytes, (size_t)n * 12))) return rc;
        ICP_HIP(ctx, hipMemcpyAsync(f->pin_out, ctx->staged_xyz.ptr, (size_t)n * 12, hipMemcpyDeviceToHost, f->copy_stream));
    }
    ICP_HIP(ctx, hipEventRecord(f->copy_done, f->copy_stream));
    f->copy_started = true;
    return ICP_OK;
}

void frame_buffers_release(icp_frame_io* f) {
    DeviceBuffer* bufs[] = {&f->slot[0], &f->slot[1], &f->skew64, &f->samp64, &f->samp32, &f->vmap, &f->rows, &f->count};
    for (DeviceBuffer* b : bufs) b->release();
    if (f->pin_in) (void)hipHostFree(f->pin_in);
    if (f->pin_out) (void)hipHostFree(f->pin_out);
    if (f->pin_count) (void)hipHostFree(f->pin_count);
    if (f->pin_in_free) (void)hipEventDestroy(f->pin_in_free);
    if (f->copy_done) (void)hipEventDestroy(f->copy_done);
    if (f->upload_stream) (void)hipStreamDestroy(f->upload_stream);
    if (f->copy_stream) (void)hipStreamDestroy(f->copy_stream);
}

// what icp_odometry_init refuses, nothing changed (icp_batch_odometry_init asks every member first; own_batch: the frame a
// batch has launched on the context is that batch's own step, which it drops itself)
int frame_init_check(icp_ctx* ctx, const icp_frame_config* cfg, bool own_batch) {
    int rc = frame_refusals(ctx, "icp_odometry_init");
    if (rc) return rc;
    if ((cfg->targets != 0 && cfg->targets != 1) || !(cfg->threshold_trans >= 0.f) || !(cfg->threshold_rot >= 0.f))
        return frame_fail(ctx, "icp_odometry_init: targets is 0 or 1, the key-frame thresholds are not negative");
    if (!own_batch && ctx->frame && ctx->frame->seq.launched && ctx->frame->seq.batched)
        return frame_fail(ctx, "icp_odometry_init: a frame launched by a batch awaits icp_batch_frame_end");
    return ICP_OK;
}

void frame_loop_release(icp_ctx* ctx) {
    icp_frame_loop* f = ctx ? ctx->frame : nullptr;
    if (!f) return;
    frame_buffers_release(&f->io);
    delete f;
    ctx->frame = nullptr;
}

}  // namespace icp

extern "C" {

void icp_default_frame_config(icp_frame_config* cfg) {
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->voxel_size = 0.0;
    cfg->threshold_trans = 0.1f;  // icp_odometry.py:29-64
    cfg->threshold_rot = 0.3f;
    cfg->constant_velocity = 1;
    cfg->targets = 0;
    cfg->copy_cloud = 1;
    cfg->stage_max_rows = 32768;
}

int icp_odometry_init(icp_ctx* ctx, const icp_frame_config* cfg) {
    if (!ctx || !cfg) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(ctx, false);  // (the entry points composed below join the map stream where they must)
    int rc = frame_init_check(ctx, cfg, false);
    if (rc) return rc;
    if (!ctx->frame) ctx->frame = new icp_frame_loop();
    icp_frame_loop* f = ctx->frame;
    frame_drop_pending(ctx, &f->seq, &f->io);
    if ((rc = icp_map_init(ctx))) return rc;
    f->cfg = *cfg;
    f->seq.index = 0;
    f->pose_epoch = -1;
    pose_identity(f->seq.delta);
    pose_identity(f->seq.last_pose);
    return ICP_OK;
}

int icp_frame_launch(icp_ctx* ctx, const float* xyz, int64_t n, int mem, const double* timestamps,
                     const float init_pose[16]) {
    if (!ctx) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(ctx, false);  // (the entry points composed below join the map stream where they must)
    icp_frame_loop* f = ctx->frame;
    if (!f) return frame_fail(ctx, "icp_frame_launch: no sequence (icp_odometry_init first)");
    int rc = frame_refusals(ctx, "icp_frame_launch");
    if (rc) return rc;
    if (f->seq.launched) return frame_fail(ctx, "icp_frame_launch: a frame is already launched (icp_frame_end first)");
    if (n < 0 || n > INT32_MAX || (n > 0 && !xyz) || (mem != ICP_MEM_HOST && mem != ICP_MEM_DEVICE))
        return frame_fail(ctx, "icp_frame_launch: [n,3] rows in host or device memory are required");
    if (ctx->in_registration || ctx->result_pending())
        return frame_fail(ctx, "icp_frame_launch: a registration of this context is in progress or awaits icp_register_end");
    // ---- input
    const float* rows = xyz;
    const double* ts = timestamps;
    if (n > 0 && mem == ICP_MEM_HOST && (rc = frame_upload(ctx, &f->io, xyz, timestamps, n, &rows, &ts))) return rc;
    return frame_launch_device(ctx, rows, n, ts, init_pose);
}

}  // extern "C"

namespace icp {

// icp_frame_launch behind its checks and its upload: rows / ts in device memory (icp_batch_frame_launch runs the first frame
// of a member through here, behind the batch's own upload)
int frame_launch_device(icp_ctx* ctx, const float* rows, int64_t n, const double* ts, const float init_pose[16]) {
    icp_frame_loop* f = ctx->frame;
    icp_frame_seq& s = f->seq;
    icp_frame_io& io = f->io;
    int rc;
    const icp_frame_config& c = f->cfg;
    // ---- the initial guess (ConstantVelocityInitialization, slam/initialization.py:103-119)
    const bool have_guess = init_pose != nullptr || c.constant_velocity != 0;
    const float* guess = init_pose ? init_pose : s.last_pose;  // (identity without constant_velocity: see below)
    // ---- de-skew -> grid sample -> float32 (slam/preprocessing.py:144-191, :207-226, :101-126)
    bool sample = false;
    if ((rc = frame_preprocess_device(ctx, &io, c.voxel_size, rows, n, ts, have_guess ? guess : nullptr, &rows, &sample))) return rc;
    f->frame_rows = rows;
    s.n = n;
    s.sampled = sample;
    io.copy_started = false;
    const size_t npix = (size_t)ctx->cfg.height * ctx->cfg.width;
    // ---- frame 0: the vertex map goes into the map (:176)
    if (s.index == 0) {
        ICP_HIP(ctx, io.vmap.reserve(npix * 12));
        if (c.targets == 1) {
            ICP_HIP(ctx, io.rows.reserve(npix * 12));
            rc = icp_project_rows(ctx, rows, n, io.vmap.as<float>(), io.rows.as<float>());
        } else {
            rc = icp_project(ctx, rows, n, ICP_MEM_DEVICE, io.vmap.as<float>(), nullptr, ICP_MEM_DEVICE);
        }
        if (rc) return rc;
        if (sample) {  // (the insertion below waits for its own count: this one arrives with it)
            if (!io.pin_count) ICP_HIP(ctx, hipHostMalloc((void**)&io.pin_count, sizeof(int), hipHostMallocDefault));
            ICP_HIP(ctx, hipMemcpyAsync(io.pin_count, io.count.ptr, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        }
        float eye[16];
        pose_identity(eye);
        f->inserted0 = 0;
        if ((rc = icp_map_update_vertex_map(ctx, eye, io.vmap.as<float>(), ICP_MEM_DEVICE, &f->inserted0))) return rc;
        s.launched = true;
        s.registered = false;
        return ICP_OK;
    }
    // ---- later frames: projection (targets = 1), staging, copy-out, registration — the plugin's order
    const float* targets = rows;
    int64_t n_targets = n;
    int target_mode = ICP_TARGETS_ALL;
    if (c.targets == 1) {
        ICP_HIP(ctx, io.vmap.reserve(npix * 12));
        ICP_HIP(ctx, io.rows.reserve(npix * 12));
        if ((rc = icp_project_rows(ctx, rows, n, io.vmap.as<float>(), io.rows.as<float>()))) return rc;
        targets = io.rows.as<float>();
        n_targets = (int64_t)npix;
        target_mode = ICP_TARGETS_SKIP_NULL;
    }
    // (a frame that comes padded from the grid sample — a handful of valid rows among NaN rows — is staged whatever its row
    // count; a large raw frame only when its copy-out needs the compacted rows anyway)
    s.staged = sample || c.stage_max_rows <= 0 || n <= (int64_t)c.stage_max_rows || c.copy_cloud != 0;
    if (s.staged && (rc = icp_map_stage_cloud(ctx, rows, n, ICP_MEM_DEVICE, ICP_TARGETS_ALL))) return rc;
    if (s.staged && (sample || (c.copy_cloud && n > 0))) {
        if ((rc = frame_copy_start(ctx, &io, sample, c.copy_cloud && n > 0, n))) return rc;
    }
    const bool from_last = c.constant_velocity != 0 && !init_pose && s.index >= 2 && ctx->have_device_pose &&
                           f->pose_epoch == ctx->device_pose_epoch;
    if (from_last) {
        rc = icp_register_launch_from_last(ctx, targets, n_targets, ICP_MEM_DEVICE, target_mode);
    } else {
        float eye[16];
        pose_identity(eye);
        rc = icp_register_launch(ctx, targets, n_targets, ICP_MEM_DEVICE, target_mode, have_guess ? guess : eye);
    }
    if (rc) {
        if (io.copy_started) (void)hipEventSynchronize(io.copy_done);
        io.copy_started = false;
        return rc;
    }
    f->pose_epoch = ctx->device_pose_epoch;
    s.launched = true;
    s.registered = true;
    return ICP_OK;
}

}  // namespace icp

extern "C" {

int icp_frame_end(icp_ctx* ctx, icp_frame_result* result, float* odometry_pc_out, int64_t cap, int64_t* rows_out,
                  int out_mem, double* loss_per_iter_out, float* dx_per_iter_out) {
    if (!ctx || !result) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard device_guard(ctx, false);  // (the entry points composed below join the map stream where they must)
    icp_frame_loop* f = ctx->frame;
    if (!f || !f->seq.launched) return frame_fail(ctx, "icp_frame_end: no frame launched (icp_frame_launch first)");
    if (ctx->batch_hold) return frame_fail(ctx, "icp_frame_end: the context is held by a batched registration");
    if (f->seq.batched) return frame_fail(ctx, "icp_frame_end: the frame was launched by a batch (icp_batch_frame_end ends it)");
    if (odometry_pc_out && cap < 0) return frame_fail(ctx, "icp_frame_end: negative capacity");
    icp_frame_seq& s = f->seq;
    memset(result, 0, sizeof(*result));
    result->frame_index = s.index;
    if (rows_out) *rows_out = 0;
    // frame 0: the identity, the vertex map is in the map (the insertion waited for its count)
    if (!s.registered) return frame_end_first(ctx, &s, &f->io, f->inserted0, false, result);
    int rc = frame_collect(ctx, &s, &f->io, result, loss_per_iter_out, dx_per_iter_out);
    if (rc) {
        if (!s.launched) f->pose_epoch = -1;  // (a failed registration; a failed wait leaves the frame launched)
        return rc;
    }
    // ---- __update_map (:360-380)
    const KeyFrameTest t = key_frame_test(s.delta, result->reg.pose, f->cfg.threshold_trans, f->cfg.threshold_rot);
    result->key_frame = t.key_frame;
    s.launched = s.registered = false;
    if (!t.key_frame) rc = icp_map_update(ctx, result->reg.pose, nullptr, 0, ICP_MEM_DEVICE, ICP_TARGETS_ALL, nullptr);
    else if (s.staged) rc = icp_map_update_staged(ctx, result->reg.pose, &result->inserted);
    else  // (n > stage_max_rows > 0: never an empty cloud)
        rc = icp_map_update(ctx, result->reg.pose, f->frame_rows, s.n, ICP_MEM_DEVICE, ICP_TARGETS_ALL, &result->inserted);
    const bool copied = f->io.copy_started && f->cfg.copy_cloud && s.n > 0;
    f->io.copy_started = false;
    if (rc) return rc;
    frame_advance(&s, t, result->reg.pose);
    return frame_deliver(ctx, "icp_frame_end", &s, &f->io, copied, !s.staged && odometry_pc_out, f->frame_rows, ICP_TARGETS_ALL,
                         odometry_pc_out, cap, rows_out, out_mem);
}

}  // extern "C"
