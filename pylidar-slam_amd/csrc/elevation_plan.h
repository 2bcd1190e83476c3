// What the elevation image (elevation.hip; icp_elevation_* in include/icp_mi355x.h) decides without a device: every refusal,
// the grids of its launches, its footprint — and the arithmetic of one row and of one pixel (cell, clip, theta, colour index,
// the orderable keys of the z-buffer), which the kernels call and a stand-alone program calls as well.  Plain C++ without a
// HIP dependency, so that it also builds under the host sanitizers (tests/native/elevation_plan_check.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "icp_mi355x.h"

#if defined(__HIPCC__)
#define ICP_ELEV_HD __host__ __device__
#else
#define ICP_ELEV_HD
#endif

namespace icp {

constexpr int ELEV_THREADS = 256;
constexpr int ELEV_LUT_ROWS = 259;          // 256 colours, then under, over, bad
constexpr int ELEV_LUT_UNDER = 256, ELEV_LUT_OVER = 257, ELEV_LUT_BAD = 258;
constexpr int64_t ELEV_MAX_INDEX = 2147483647ll;  // rows and pixels are numbered by an int32
constexpr int ELEV_WINDOW_MAX_BLOCKS = 4096;      // the window launches walk the stored points with a stride

// ---- one row -------------------------------------------------------------------------------------------------------------
ICP_ELEV_HD inline float elev_rint(float v) { return rintf(v); }
ICP_ELEV_HD inline double elev_rint(double v) { return rint(v); }

// the image row (column) of a coordinate: round(v / pixel + half), half to even, in the arithmetic of T; false where it falls
// outside [0, extent) — NaN and the infinities do.  -0.5 / pixel gives -0, which is cell 0
template <typename T>
ICP_ELEV_HD inline bool elevation_cell(T v, T pixel, T half, int64_t extent, int* cell) {
    const T r = elev_rint((T)((T)(v / pixel) + half));
    if (!((double)r >= 0.0 && (double)r < (double)extent)) return false;
    *cell = (int)r;
    return true;
}

// np.clip on a z that is no NaN, and one zero: -0.0 becomes +0.0
template <typename T>
ICP_ELEV_HD inline T elevation_clip(T z, T lo, T hi) {
    T c = z < lo ? lo : z;
    c = c > hi ? hi : c;
    return c == (T)0 ? (T)0 : c;
}

// keys that order like the numbers they come from (no NaN reaches them)
ICP_ELEV_HD inline uint32_t elevation_order32(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

ICP_ELEV_HD inline uint64_t elevation_order64(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

// the z-buffer word of a float32 row: the greatest word wins the pixel — the greatest clipped z (the smallest when flipped),
// among equal ones the highest row.  Never 0, the empty pixel: a clipped z is finite
ICP_ELEV_HD inline uint64_t elevation_key32(float clipped, int flip, uint32_t row) {
    const uint32_t o = elevation_order32(clipped);
    return ((uint64_t)(flip ? ~o : o) << 32) | row;
}

ICP_ELEV_HD inline uint64_t elevation_key64(double clipped, int flip) {
    const uint64_t o = elevation_order64(clipped);
    return flip ? ~o : o;
}

// theta of a clipped z, in the arithmetic of T; `den` = T(z_max - z_min), subtracted in float64
template <typename T>
ICP_ELEV_HD inline float elevation_theta(T clipped, T lo, T den) {
    return (float)((T)(clipped - lo) / den);
}

// matplotlib's Colormap.__call__ on a float32 image of a 256-colour map: the row of the table
ICP_ELEV_HD inline int elevation_colour_row(float theta) {
    float t = theta * 256.0f;
    if (t == 256.0f) t = 255.0f;
    if (t != t) return ELEV_LUT_BAD;
    if (t < 0.0f) return ELEV_LUT_UNDER;
    if (t >= 256.0f) return ELEV_LUT_OVER;
    return (int)t;
}

// ---- grids and footprint ---------------------------------------------------------------------------------------------------
// a thread per row or pixel (count <= 2^31 - 1: at most 2^23 workgroups); 0 rows launch nothing
inline int64_t elevation_blocks(int64_t count) {
    if (count < 1) return 0;
    return count / ELEV_THREADS + (count % ELEV_THREADS ? 1 : 0);
}

// the window launches: the map's size is known on the device only, so the grid covers its capacity, up to a bound
inline int64_t elevation_window_blocks(int64_t capacity) {
    const int64_t b = elevation_blocks(capacity);
    return b > ELEV_WINDOW_MAX_BLOCKS ? ELEV_WINDOW_MAX_BLOCKS : b;
}

// device memory of an image in bytes: per pixel the z-buffer word (8), the winning row (4), colour (3), theta (4), point (12)
// and index (4); the table; 64 cache lines of counters; + 24 per row of max_rows (and as much pinned) once host rows have been built from
inline uint64_t elevation_footprint_bytes(int64_t height, int64_t width, int64_t max_rows, int host_rows) {
    if (height < 1 || width < 1 || max_rows < 1 || max_rows > ELEV_MAX_INDEX) return 0;
    if (height > ELEV_MAX_INDEX / width) return 0;
    return (uint64_t)(height * width) * 35 + ELEV_LUT_ROWS * 3 + 64 * 128 + (host_rows ? (uint64_t)max_rows * 24 : 0);
}

// ---- refusals: ICP_OK, or ICP_ERR_INVALID_ARGUMENT with the reason in `reason` (at least 160 bytes) ------------------------
inline bool elevation_mem_ok(int mem) { return mem == ICP_MEM_HOST || mem == ICP_MEM_DEVICE; }

inline int elevation_create_refusals(int64_t height, int64_t width, double pixel, double z_min, double z_max, const void* lut,
                                     int64_t max_rows, char* reason) {
    reason[0] = 0;
    if (!(pixel > 0.0) || !isfinite(pixel))
        snprintf(reason, 160, "icp_elevation_create: pixel size %g is not a positive finite number", pixel);
    else if (!isfinite(z_min) || !isfinite(z_max))
        snprintf(reason, 160, "icp_elevation_create: z_min = %g, z_max = %g: a bound is not finite", z_min, z_max);
    else if (!(z_min < z_max))
        snprintf(reason, 160, "icp_elevation_create: z_min = %g is not below z_max = %g", z_min, z_max);
    else if (!isfinite(z_max - z_min) || !((float)z_min < (float)z_max) || !isfinite((float)z_min) || !isfinite((float)z_max))
        snprintf(reason, 160, "icp_elevation_create: z_min = %g and z_max = %g do not stay apart and finite in float32", z_min, z_max);
    else if (height < 1 || width < 1)
        snprintf(reason, 160, "icp_elevation_create: height = %lld, width = %lld: below 1", (long long)height, (long long)width);
    else if (height > ELEV_MAX_INDEX / width)
        snprintf(reason, 160, "icp_elevation_create: height x width exceeds %lld pixels", (long long)ELEV_MAX_INDEX);
    else if (max_rows < 1)
        snprintf(reason, 160, "icp_elevation_create: max_rows = %lld is below 1", (long long)max_rows);
    else if (max_rows > ELEV_MAX_INDEX)
        snprintf(reason, 160, "icp_elevation_create: max_rows exceeds %lld", (long long)ELEV_MAX_INDEX);
    else if (!lut)
        snprintf(reason, 160, "icp_elevation_create: the colour table is NULL");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int elevation_build_refusals(int64_t n, int64_t max_rows, int mem, int dtype, char* reason) {
    reason[0] = 0;
    if (n < 0)
        snprintf(reason, 160, "icp_elevation_build: n = %lld is negative", (long long)n);
    else if (n > ELEV_MAX_INDEX)
        snprintf(reason, 160, "icp_elevation_build: n = %lld exceeds what an int32 index holds", (long long)n);
    else if (n > max_rows)
        snprintf(reason, 160, "icp_elevation_build: n = %lld exceeds max_rows = %lld", (long long)n, (long long)max_rows);
    else if (!elevation_mem_ok(mem))
        snprintf(reason, 160, "icp_elevation_build: host or device memory");
    else if (dtype != ICP_ELEVATION_F32 && dtype != ICP_ELEVATION_F64)
        snprintf(reason, 160, "icp_elevation_build: float32 or float64 rows, not dtype %d", dtype);
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int elevation_build_aggmap_refusals(const void* image_ctx, const void* map_ctx, int32_t frame_lo, int32_t frame_hi,
                                           const double* pose16, char* reason) {
    reason[0] = 0;
    bool finite = pose16 != nullptr;
    for (int i = 0; finite && i < 16; ++i) finite = isfinite(pose16[i]);
    if (!map_ctx || image_ctx != map_ctx)
        snprintf(reason, 160, "icp_elevation_build_aggmap: the map belongs to another context");
    else if (frame_lo > frame_hi)
        snprintf(reason, 160, "icp_elevation_build_aggmap: frame_lo = %d is above frame_hi = %d", (int)frame_lo, (int)frame_hi);
    else if (!finite)
        snprintf(reason, 160, "icp_elevation_build_aggmap: the pose has a non-finite entry");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

inline int elevation_get_refusals(int out_mem, char* reason) {
    reason[0] = 0;
    if (!elevation_mem_ok(out_mem)) snprintf(reason, 160, "icp_elevation_get: host or device memory");
    return reason[0] ? ICP_ERR_INVALID_ARGUMENT : ICP_OK;
}

}  // namespace icp
