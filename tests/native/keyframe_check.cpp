// Stand-alone host program around csrc/frame_keyframe.h — the key-frame arithmetic icp_frame_end applies
// (ICPFrameToModel.__update_map, slam/odometry/icp_odometry.py:360-380) — built and run under
// -fsanitize=address,undefined by tests/test_frame_host.py.
//   keyframe_check CASES   CASES: "count thr_trans thr_rot" then per case 32 words: delta[16] pose[16], float32 bit
//                          patterns in hex.  Prints per case: key_frame, new_delta[16] and params[6] as bit patterns,
//                          |t| and |r| in degrees.
// Every array is heap-allocated at its exact size so that the address sanitizer sees an access one element too far.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "frame_keyframe.h"

static float from_bits(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof(f));
    return f;
}

static uint32_t to_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof(u));
    return u;
}

static bool read_floats(FILE* in, float* out, int count) {
    for (int i = 0; i < count; ++i) {
        unsigned int u = 0;
        if (fscanf(in, "%x", &u) != 1) return false;
        out[i] = from_bits((uint32_t)u);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s CASES\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "r");
    if (!in) {
        perror(argv[1]);
        return 2;
    }
    int count = 0;
    float thr[2];
    if (fscanf(in, "%d", &count) != 1 || count < 0 || !read_floats(in, thr, 2)) {
        fprintf(stderr, "bad header\n");
        fclose(in);
        return 2;
    }
    for (int c = 0; c < count; ++c) {
        std::vector<float> delta(16), pose(16);
        if (!read_floats(in, delta.data(), 16) || !read_floats(in, pose.data(), 16)) {
            fprintf(stderr, "case %d: truncated\n", c);
            fclose(in);
            return 2;
        }
        const icp::KeyFrameTest t = icp::key_frame_test(delta.data(), pose.data(), thr[0], thr[1]);
        // the product may be written over its own left operand (icp_frame_end keeps the motion since the last key frame so)
        std::vector<float> alias(delta);
        icp::pose_product(alias.data(), pose.data(), alias.data());
        if (memcmp(alias.data(), t.new_delta, sizeof(t.new_delta)) != 0) {
            fprintf(stderr, "case %d: the in-place product differs\n", c);
            fclose(in);
            return 1;
        }
        printf("%d", t.key_frame);
        for (int i = 0; i < 16; ++i) printf(" %08x", to_bits(t.new_delta[i]));
        for (int i = 0; i < 6; ++i) printf(" %08x", to_bits(t.params[i]));
        printf(" %.9g %.9g\n", t.trans, t.rot_deg);
    }
    fclose(in);
    return 0;
}
