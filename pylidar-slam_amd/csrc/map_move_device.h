// Re-expression of the local map in a new frame (local_map.py:346-348), shared by api.hip (host-side checks) and
// hash_grid.hip (the re-expression rides in the first launch of the grid build).
#pragma once
#include <math.h>

#include "icp_internal.h"

namespace icp {

// general 4x4 inverse in f64 (np.linalg.inv(relative_pose), local_map.py:346); the same code on host and device
// (every loop unrolled and the pivot row exchanged by comparisons against constant row numbers: no index into `a` depends on
// data, so the 32 doubles live in registers — indexed by the pivot they sat in scratch memory, and the one thread per
// workgroup that inverts the pose in front of the map move spent microseconds on round trips to it.  The operations and
// their order are unchanged, hence the bits)
__host__ __device__ inline bool invert4(const float* m, float* out) {
    double a[4][8];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[r][c] = m[4 * r + c];
            a[r][4 + c] = r == c ? 1.0 : 0.0;
        }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        int piv = c;
        double best = fabs(a[c][c]);  // = fabs(a[piv][c])
#pragma unroll
        for (int r = c + 1; r < 4; ++r) {
            const double v = fabs(a[r][c]);
            if (v > best) {
                best = v;
                piv = r;
            }
        }
        if (best == 0.0) return false;
#pragma unroll
        for (int r = c + 1; r < 4; ++r)
            if (piv == r) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const double t = a[c][k];
                    a[c][k] = a[r][k];
                    a[r][k] = t;
                }
            }
        const double inv = 1.0 / a[c][c];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[c][k] *= inv;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (r != c) {
                const double f = a[r][c];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
                for (int k = 0; k < 8; ++k) a[r][k] = __dsub_rn(a[r][k], __dmul_rn(f, a[c][k]));  // no fma: host bits
#else
#pragma unroll
                for (int k = 0; k < 8; ++k) a[r][k] -= f * a[c][k];
#endif
            }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) out[4 * r + c] = (float)a[r][4 + c];
    return true;
}

// (the moved point also comes back in *ox, *oy, *oz: the insertion launch of a grid build hashes what it has just formed)
__device__ inline void move_point(const float* T, const float* __restrict__ in, long long i, float* __restrict__ out,
                                  float* ox = nullptr, float* oy = nullptr, float* oz = nullptr) {
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    // np.einsum("ij,nj->ni", R, map) + t
    const float mx = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[0], x), __fmul_rn(T[1], y)), __fmul_rn(T[2], z)), T[3]);
    const float my = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[4], x), __fmul_rn(T[5], y)), __fmul_rn(T[6], z)), T[7]);
    const float mz = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(T[8], x), __fmul_rn(T[9], y)), __fmul_rn(T[10], z)), T[11]);
    out[3 * i] = mx;
    out[3 * i + 1] = my;
    out[3 * i + 2] = mz;
    if (ox) {
        *ox = mx;
        *oy = my;
        *oz = mz;
    }
}

// Every block inverts the 4x4 once: one arithmetic for both sources of the pose (host value / device-resident result),
// so the two give the same map bit for bit.
// T (LDS, 16 floats) <- the inverse this launch applies; call from one thread, barrier afterwards
__device__ inline void map_move_prepare(const MapMoveJob& job, float* __restrict__ T) {
    float pose[16], inv[16];
    for (int k = 0; k < 16; ++k) pose[k] = job.st ? job.st->pose[k] : job.rel.m[k];
    // a registration that stopped on an error moves nothing: the reference raises before it would touch the map
    // (slam/common/optimization.py:334-336 inside icp_odometry.py:286), the host learns of it in icp_register_end
    // ... and so does one whose loop was cut short by a timed-out hand-off (icp_register_end finishes it on per-iteration
    // launches and repeats this update with the final pose)
    const bool failed = job.st && (job.st->status != ICP_OK || job.st->handoff_timeouts > 0);
    if (failed || !invert4(pose, inv))  // a pose built from Euler angles is never singular; the host path checks
        for (int k = 0; k < 16; ++k) inv[k] = (k % 5 == 0) ? 1.f : 0.f;
    for (int k = 0; k < 16; ++k) T[k] = inv[k];
}

}  // namespace icp
