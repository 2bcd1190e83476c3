// The state behind the frame calls — icp_odometry_init / icp_frame_launch / icp_frame_end (frame.hip) and
// icp_pmap_odometry_init / icp_pmap_frame_launch / icp_pmap_frame_end (pmap_frame.hip) — and the steps the two loops share
// (frame.hip).  The batched calls (batch_frame.hip, batch_pmap_frame.hip) advance THIS state of every member, so that a
// member may be stepped alone and by a batch in turn.
#pragma once
#include "frame_keyframe.h"
#include "icp_internal.h"

// where a sequence stands, whatever its map
struct icp_frame_seq {
    int32_t index = 0;        // frames completed since the loop's init call
    bool launched = false;    // a frame awaits its end call
    bool registered = false;  // ... with a registration enqueued (false: frame 0)
    bool batched = false;     // ... launched by a batch: the batch's end call ends it (batch_frame.hip)
    float delta[16];          // `_delta_since_map_update`
    float last_pose[16];      // the last relative pose (the constant-velocity guess)
    int64_t n = 0;            // rows handed in (vertex-map input: H*W)
    bool sampled = false;
    bool staged = false;      // the frame's valid rows were compacted in front of its registration
};

// a frame's way in and out, whatever its map
struct icp_frame_io {
    // ---- input: pinned staging -> one of two device slots, on a stream of its own (odometry.py::_upload)
    void* pin_in = nullptr;
    size_t pin_in_bytes = 0;
    hipEvent_t pin_in_free = nullptr;
    bool pin_in_busy = false;
    icp::DeviceBuffer slot[2];
    int which = 0;
    hipStream_t upload_stream = nullptr;
    // ---- the frame on the device
    icp::DeviceBuffer skew64, samp64, samp32, vmap, rows, count;
    // ---- odometry_pc: the staged rows towards pinned memory, beside the registration
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_done = nullptr;
    void* pin_out = nullptr;
    size_t pin_out_bytes = 0;
    int* pin_count = nullptr;  // the grid sample's count
    bool copy_started = false;
};

// the frame loop against the kd-tree style map
struct icp_frame_loop {
    icp_frame_config cfg;
    icp_frame_seq seq;
    icp_frame_io io;
    const float* frame_rows = nullptr;  // [n,3] float32: what is staged, projected and (targets = 0) registered
    int64_t inserted0 = 0;              // frame 0's insertion
    long long pose_epoch = -1;  // ctx->device_pose_epoch behind the last frame's launch: while it stands, the device pose is that frame's
};

// the frame loop against the projective local map
struct icp_pmap_frame_loop {
    icp_pmap_frame_config cfg;
    icp_frame_seq seq;
    icp_frame_io io;
    const float* frame_vmap = nullptr;  // [3,H,W] on the device: what a key frame inserts (the input itself, or io.vmap)
    const float* valid_rows = nullptr;  // [n,3] on the device: the rows odometry_pc is compacted from ...
    int valid_mode = 0;                 // ... with this icp_target_mode (vertex-map input: null pixels dropped as well)
};

namespace icp {
// ---- a frame's way in and out (frame.hip)
int pinned_reserve(icp_ctx* ctx, void** ptr, size_t* have, size_t need);
// host rows (and timestamps) -> pinned buffer -> the next of two device slots, on the upload stream
int frame_upload(icp_ctx* ctx, icp_frame_io* io, const float* xyz, const double* ts, int64_t n, const float** rows_out,
                 const double** ts_out);
// de-skew (guess != NULL and ts != NULL) -> padded grid sample (voxel_size > 0) -> float32, into the io buffers
int frame_preprocess_device(icp_ctx* ctx, icp_frame_io* io, double voxel_size, const float* rows, int64_t n, const double* ts,
                            const float* guess, const float** rows_out, bool* sampled_out);
// the staged rows (cloud) and the grid sample's count (sample) towards pinned memory, beside the registration
int frame_copy_start(icp_ctx* ctx, icp_frame_io* io, bool sample, bool cloud, int64_t n);
void frame_buffers_release(icp_frame_io* io);
// ---- the steps of a frame that do not depend on the map (frame.hip); `who`: the calling entry point, for the messages
// a frame launched and never ended: its registration is collected and dropped, its copy waited for
void frame_drop_pending(icp_ctx* ctx, icp_frame_seq* s, icp_frame_io* io);
// frame 0's end: the identity, `inserted`; wait_count: the grid sample's count has not been waited for yet
int frame_end_first(icp_ctx* ctx, icp_frame_seq* s, const icp_frame_io* io, int64_t inserted, bool wait_count,
                    icp_frame_result* result);
// icp_register_end, the copy wait, result->samples; a failed registration leaves no frame launched (the reference raises
// before it touches the map, :286: nothing of the sequence moves)
int frame_collect(icp_ctx* ctx, icp_frame_seq* s, icp_frame_io* io, icp_frame_result* result, double* loss_per_iter_out,
                  float* dx_per_iter_out);
// the key-frame outcome on delta, last_pose and index (__update_map :360-380, behind a map update that succeeded)
void frame_advance(icp_frame_seq* s, const KeyFrameTest& t, const float pose[16]);
// odometry_pc (:210-213, :243): the valid rows the staging compacted, in order; stage_late: `rows` are compacted now
int frame_deliver(icp_ctx* ctx, const char* who, const icp_frame_seq* s, const icp_frame_io* io, bool copied, bool stage_late,
                  const float* rows, int mode, float* odometry_pc_out, int64_t cap, int64_t* rows_out, int out_mem);
// what icp_pmap_odometry_init refuses (pmap_frame.hip); own_batch: a frame launched by the asking batch itself is no obstacle
int pmap_frame_init_check(icp_ctx* ctx, const icp_pmap_frame_config* cfg, bool own_batch);
// what icp_odometry_init refuses (frame.hip); own_batch: a frame launched by the asking batch itself is no obstacle
int frame_init_check(icp_ctx* ctx, const icp_frame_config* cfg, bool own_batch);
// icp_frame_launch behind its checks and its upload (frame.hip)
int frame_launch_device(icp_ctx* ctx, const float* rows, int64_t n, const double* ts, const float init_pose[16]);
}  // namespace icp
