// The sequence state behind icp_odometry_init / icp_frame_launch / icp_frame_end (frame.hip), shared with the batched form
// (batch_frame.hip): a member stepped by icp_batch_frame_launch / icp_batch_frame_end advances THIS state, so that it may be
// stepped alone and by the batch in turn.
#pragma once
#include "icp_internal.h"

struct icp_frame_loop {
    icp_frame_config cfg;
    int32_t index = 0;      // frames completed since icp_odometry_init
    bool launched = false;  // a frame awaits its icp_frame_end
    bool registered = false;  // ... with a registration enqueued (false: frame 0)
    bool batched = false;   // ... launched by icp_batch_frame_launch: icp_batch_frame_end ends it (batch_frame.hip)
    float delta[16];        // `_delta_since_map_update`
    float last_pose[16];    // the last relative pose (the constant-velocity guess)
    long long pose_epoch = -1;  // ctx->device_pose_epoch behind the last frame's launch: while it stands, the device pose is that frame's
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
    const float* frame_rows = nullptr;  // [n,3] float32: what is staged, projected and (targets = 0) registered
    int64_t n = 0;
    bool sampled = false;
    bool staged = false;    // the frame's valid rows were compacted in front of its registration
    int64_t inserted0 = 0;  // frame 0's insertion
    // ---- odometry_pc: the staged rows towards pinned memory, beside the registration
    hipStream_t copy_stream = nullptr;
    hipEvent_t copy_done = nullptr;
    void* pin_out = nullptr;
    size_t pin_out_bytes = 0;
    int* pin_count = nullptr;  // the grid sample's count
    bool copy_started = false;
};

// The sequence state behind icp_pmap_odometry_init / icp_pmap_frame_launch / icp_pmap_frame_end (pmap_frame.hip): the frame
// loop against the projective local map.  `io` lends the upload slots, the preprocessing buffers and the copy-out stream of the
// kd-tree loop (its sequence fields stay unused): the helpers below serve both loops.
struct icp_pmap_frame_loop {
    icp_pmap_frame_config cfg;
    icp_frame_loop io;
    int32_t index = 0;        // frames completed since icp_pmap_odometry_init
    bool launched = false;    // a frame awaits its icp_pmap_frame_end
    bool registered = false;  // ... with a registration enqueued (false: frame 0)
    bool batched = false;     // ... launched by icp_batch_pmap_frame_launch: icp_batch_pmap_frame_end ends it
    float delta[16];          // `_delta_since_map_update`
    float last_pose[16];      // the last relative pose (the constant-velocity guess)
    const float* frame_vmap = nullptr;  // [3,H,W] on the device: what a key frame inserts (the input itself, or io.vmap)
    int64_t n = 0;            // rows handed in (vertex-map input: H*W)
    bool sampled = false;
    const float* valid_rows = nullptr;  // [n,3] on the device: the rows odometry_pc is compacted from ...
    int valid_mode = 0;       // ... with this icp_target_mode (vertex-map input: null pixels dropped as well)
    bool staged = false;      // ... compacted and counted in front of the registration (icp_map_stage_cloud)
};

namespace icp {
// ---- shared by the two loops (frame.hip)
int pinned_reserve(icp_ctx* ctx, void** ptr, size_t* have, size_t need);
// host rows (and timestamps) -> pinned buffer -> the next of two device slots, on the loop's upload stream
int frame_upload(icp_ctx* ctx, icp_frame_loop* f, const float* xyz, const double* ts, int64_t n, const float** rows_out,
                 const double** ts_out);
// de-skew (guess != NULL and ts != NULL) -> padded grid sample (voxel_size > 0) -> float32, into the loop's buffers
int frame_preprocess_device(icp_ctx* ctx, icp_frame_loop* f, double voxel_size, const float* rows, int64_t n, const double* ts,
                            const float* guess, const float** rows_out, bool* sampled_out);
// the staged rows (cloud) and the grid sample's count (sample) towards pinned memory, beside the registration
int frame_copy_start(icp_ctx* ctx, icp_frame_loop* f, bool sample, bool cloud, int64_t n);
void frame_buffers_release(icp_frame_loop* f);
// what icp_pmap_odometry_init refuses (pmap_frame.hip); own_batch: a frame launched by the asking batch itself is no obstacle
int pmap_frame_init_check(icp_ctx* ctx, const icp_pmap_frame_config* cfg, bool own_batch);
// what icp_odometry_init refuses (frame.hip); own_batch: a frame launched by the asking batch itself is no obstacle
int frame_init_check(icp_ctx* ctx, const icp_frame_config* cfg, bool own_batch);
// icp_frame_launch behind its checks and its upload (frame.hip)
int frame_launch_device(icp_ctx* ctx, const float* rows, int64_t n, const double* ts, const float init_pose[16]);
}  // namespace icp
