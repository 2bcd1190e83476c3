// The key-frame arithmetic of ICPFrameToModel.__update_map (slam/odometry/icp_odometry.py:360-380) on the host, as
// icp_frame_end applies it: plain C++ without a HIP dependency, so that it also builds into a stand-alone program under the
// host sanitizers (tests/native/keyframe_check.cpp).  The plugin's version of the same lines is
// pylidar_slam_amd/odometry.py::MI355XICPFrameToModel.__update_map with `from_pose_matrix` (Pose.from_pose_matrix,
// slam/common/pose.py:120-207; euler xyz, R = Rz Ry Rx).
#pragma once
#include <math.h>
#include <string.h>

namespace icp {

struct KeyFrameTest {
    float new_delta[16];  // delta x pose, float32
    float params[6];      // tx, ty, tz, ex, ey, ez of new_delta
    double trans;         // |t|, metres
    double rot_deg;       // |r| 180 / pi, degrees
    int key_frame;        // 1: trans > threshold_trans or rot_deg > threshold_rot
};

inline void pose_identity(float m[16]) {
    memset(m, 0, 16 * sizeof(float));
    m[0] = m[5] = m[10] = m[15] = 1.f;
}

// row-major 4x4 float32 product, each element accumulated in float32 from k = 0 upwards
inline void pose_product(const float a[16], const float b[16], float out[16]) {
    float r[16];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = a[4 * i] * b[j];
            for (int k = 1; k < 4; ++k) s = s + a[4 * i + k] * b[4 * k + j];
            r[4 * i + j] = s;
        }
    memcpy(out, r, sizeof(r));
}

// from_pose_matrix in float32 (eps = 1e-6): the gimbal-lock branch where sqrt(m00^2 + m10^2) is not below eps
inline void pose_to_params(const float m[16], float p[6]) {
    const float sy = sqrtf(m[0] * m[0] + m[4] * m[4]);
    p[0] = m[3];
    p[1] = m[7];
    p[2] = m[11];
    if (!(sy < 1.0e-6f)) {
        p[3] = atan2f(m[9], m[10]);
        p[4] = atan2f(-m[8], sy);
        p[5] = atan2f(m[4], m[0]);
    } else {
        p[3] = atan2f(-m[6], m[5]);
        p[4] = atan2f(-m[8], sy);
        p[5] = 0.f;
    }
}

inline KeyFrameTest key_frame_test(const float delta[16], const float pose[16], float threshold_trans, float threshold_rot) {
    KeyFrameTest t;
    pose_product(delta, pose, t.new_delta);
    pose_to_params(t.new_delta, t.params);
    const float* p = t.params;
    t.trans = sqrtf(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    t.rot_deg = (double)sqrtf(p[3] * p[3] + p[4] * p[4] + p[5] * p[5]) * 180.0 / 3.14159265358979323846;
    t.key_frame = (t.trans > (double)threshold_trans || t.rot_deg > (double)threshold_rot) ? 1 : 0;
    return t;
}

}  // namespace icp
