// What icp_knn_query (api.hip, knn.hip) refuses before it touches the device, the list length a k runs on and the squared
// bound of a distance_upper_bound: plain C++ without a HIP dependency, so that it also builds into a stand-alone program
// under the host sanitizers (tests/native/knn_plan_check.cpp).
#pragma once
#include <stdint.h>
#include <math.h>
#include <stdio.h>

#include "icp_mi355x.h"

namespace icp {

constexpr int KNN_MAX_K = 32;
constexpr int KNN_LENGTHS[] = {1, 2, 4, 8, 11, 16, 32};  // the compiled list lengths (k_knn_query<KN, NL>)

// the compiled list length a k runs on: the next one at or above it (an exact longer list begins with the exact shorter
// one); 0: k is refused
inline int knn_list_length(int32_t k) {
    if (k < 1) return 0;
    for (int len : KNN_LENGTHS)
        if (k <= len) return len;
    return 0;
}

// squared distance bound as the kernel compares it (float32 b * b); +inf: no bound (b <= 0, +inf, NaN, or b * b overflows)
inline float knn_squared_bound(float b) {
    if (!(b > 0.f) || isinf(b)) return INFINITY;
    return b * b;
}

// ICP_OK, or ICP_ERR_INVALID_ARGUMENT with the reason in `reason` (at least 160 bytes)
inline int knn_query_refusals(int64_t n, int32_t k, int32_t flags, bool has_dist, bool has_index, int mem, int out_mem,
                              char* reason) {
    reason[0] = 0;
    if (knn_list_length(k) == 0)
        snprintf(reason, 160, "icp_knn_query: k = %d is outside 1..%d", (int)k, KNN_MAX_K);
    else if (n < 0)
        snprintf(reason, 160, "icp_knn_query: n = %lld is negative", (long long)n);
    else if (n > INT32_MAX / 4)
        snprintf(reason, 160, "icp_knn_query: at most %d query rows per call", INT32_MAX / 4);
    else if (!has_dist && !has_index)
        snprintf(reason, 160, "icp_knn_query: both outputs are NULL");
    else if (flags & ~ICP_KNN_SQR_DISTS)
        snprintf(reason, 160, "icp_knn_query: unknown flags 0x%x", (unsigned)flags);
    else if ((mem != ICP_MEM_HOST && mem != ICP_MEM_DEVICE) || (out_mem != ICP_MEM_HOST && out_mem != ICP_MEM_DEVICE))
        snprintf(reason, 160, "icp_knn_query: host or device memory");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

}  // namespace icp
