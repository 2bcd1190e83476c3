// Elevation image: a cloud rasterised top-down into H x W pixels of heights, the highest point per pixel kept — the step
// behind the aggregated window in the reference's loop closure and the front end of its elevation-image initialisation
// (ElevationImageRegistration.build_image, slam/common/registration.py:196-241; called at slam/loop_closure.py:294 on the
// window and at slam/initialization.py:176 on every raw scan).
//
//   pixel    row = rint(x / pixel_size + H / 2), column = rint(y / pixel_size + W / 2): half to even, in the arithmetic of the
//            rows (float32 rows: pixel_size rounded to float32, float32 division and sum; float64 rows: float64); H / 2 and
//            W / 2 are floor divisions; a row is kept iff 0 <= row < H and 0 <= column < W (NaN and the infinities are not)
//   height   z clipped to [z_min, z_max] (the bounds rounded to the rows' type), -0.0 made +0.0; the pixel goes to the
//            greatest clipped z (flip: the smallest); among equal clipped z the HIGHEST ROW wins, flipped or not (the rule
//            of the projection's z-buffer; the reference's unstable sort has no rule to match)
//   theta    (clipped z - z_min) / (z_max - z_min): the denominator subtracted in float64 and rounded to the rows' type,
//            subtraction and division in the rows' type, the result stored as float32; an EMPTY pixel holds float32(z_min)
//   colour   matplotlib's rule on a float32 image: t = theta * 256 (float32); t == 256 -> 255; NaN -> row 258 of the table,
//            t < 0 -> 256, t >= 256 -> 257, else trunc(t); the table [259, 3] uint8 is the caller's data
//   deviation a row inside the image whose z is NaN is SET ASIDE and counted (in the reference it wins its pixel — argsort
//            puts NaN last, the order is reversed — and paints it with the bad colour)
//
// A build is a fixed number of launches on the context's stream with no host read:
//   1. k_elev_clear    z-buffer words to 0 (no row's word is 0), winning rows to -1, counters to 0;
//   2. the splat       float32 rows: ONE pass, a 64-bit atomicMax of (orderable bits of the clipped z, inverted when flipped)
//                      << 32 | row.  float64 rows and map windows: 64 bits of z leave no room for the row, and ordering by
//                      float32(z) would crown another row where two heights differ below float32 resolution, so TWO passes:
//                      the pixel's extreme z (atomicMax of its 64 orderable bits), then the highest row among the rows whose
//                      z equals it (atomicMax of an int).  Every atomic is preceded by a plain read of the pixel's word: words
//                      only grow during a splat, so a row that does not beat the word it reads cannot beat a later one.
//                      Atomics to ONE address queue up (about 12 ns each, measured): of the rows of a wave that share a pixel
//                      only the one with the greatest word goes to memory (elev_covered), and the row counters are 64 copies;
//   3. k_elev_resolve  a thread per pixel: theta, colour, the float32 point, the int32 row (-1: empty), the filled count.
// A window of an aggregated map (aggmap.hip) is splat straight from the stored float64 points with
// frame_lo <= first_frame < frame_hi, each moved by the pose with the arithmetic of the submap (agg_world); the row is the
// stored index.  The map's size is read on the device; the window is never materialised.
#include <string.h>

#include <new>

#include "aggmap_device.h"
#include "elevation_plan.h"
#include "icp_internal.h"

namespace icp {

// The counters of a build are ELEV_COUNTER_SHARDS copies, a cache line apart, summed by the host: a workgroup adds to the copy of
// its index, so that the atomics of a launch spread over as many addresses (atomics to ONE address queue up at about 12 ns each:
// 2 048 waves adding to one counter cost more than the splat itself)
constexpr int ELEV_COUNTER_SHARDS = 64;
struct ElevCounters {
    unsigned long long in_image, outside, nan_z, filled;
    unsigned long long pad[12];
};
static_assert(sizeof(ElevCounters) == 128, "ElevCounters: one cache line");

template <typename T>
struct ElevGeom {
    T pixel, half_h, half_w, lo, hi, den;
    int height, width, flip;
};

// float32 / float64 rows of the caller
template <typename T>
struct ElevRows {
    typedef T real;
    static constexpr bool COVER = true;  // rows that follow one another in a scan share their pixel: elev_covered pays
    const T* __restrict__ xyz;
    int n;
    __device__ __forceinline__ int count() const { return n; }
    __device__ __forceinline__ bool fetch(int i, T* p) const {
        p[0] = xyz[3 * (long long)i];
        p[1] = xyz[3 * (long long)i + 1];
        p[2] = xyz[3 * (long long)i + 2];
        return true;
    }
};

// the stored points of an aggregated map that a frame window keeps, moved by a pose
struct ElevWindow {
    typedef double real;
    static constexpr bool COVER = false;  // one point per voxel, in creation order: neighbours in a wave seldom share a pixel
    const double* __restrict__ pts;
    const int* __restrict__ first_frame;
    const int* __restrict__ size_cell;  // the map's size behind everything enqueued before this launch
    int capacity, lo, hi;
    AggPose pose;
    __device__ __forceinline__ int count() const {
        const int s = *size_cell;
        return s < capacity ? s : capacity;
    }
    __device__ __forceinline__ bool fetch(int i, double* p) const {
        const int f = first_frame[i];
        if (f < lo || f >= hi) return false;
        const double x = pts[3 * (long long)i], y = pts[3 * (long long)i + 1], z = pts[3 * (long long)i + 2];
        p[0] = agg_world(pose, 0, x, y, z);
        p[1] = agg_world(pose, 1, x, y, z);
        p[2] = agg_world(pose, 2, x, y, z);
        return true;
    }
};

enum { ELEV_ROW_OUTSIDE = 0, ELEV_ROW_NAN = 1, ELEV_ROW_IN = 2 };

template <typename T>
__device__ __forceinline__ int elev_row(const ElevGeom<T>& g, const T* p, int* pix, T* clipped) {
    int r, c;
    if (!elevation_cell(p[0], g.pixel, g.half_h, (int64_t)g.height, &r) || !elevation_cell(p[1], g.pixel, g.half_w, (int64_t)g.width, &c))
        return ELEV_ROW_OUTSIDE;
    if (p[2] != p[2]) return ELEV_ROW_NAN;
    *pix = r * g.width + c;  // (< height * width <= 2^31 - 1)
    *clipped = elevation_clip(p[2], g.lo, g.hi);
    return ELEV_ROW_IN;
}

__device__ __forceinline__ unsigned elev_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;  // (lane 0 holds the sum)
}

__global__ __launch_bounds__(ELEV_THREADS) void k_elev_clear(unsigned long long* __restrict__ keys, int* __restrict__ rows, int pixels,
                                                             ElevCounters* __restrict__ cnt) {
    const long long p = (long long)blockIdx.x * ELEV_THREADS + threadIdx.x;
    if (p < pixels) {
        keys[p] = 0ull;
        rows[p] = -1;
    }
    if (p < ELEV_COUNTER_SHARDS) cnt[p].in_image = cnt[p].outside = cnt[p].nan_z = cnt[p].filled = 0ull;
}

// true where another lane of the wave holds a greater word for the same pixel (or the same word, in a higher lane): that
// lane's atomic covers this one, so at most one lane of a wave goes to a pixel.  Rows that follow one another in a scan fall
// into the same pixel near the sensor; without this their atomics queue up on one address.  Lanes without a row pass pix < 0
__device__ __forceinline__ bool elev_covered(int pix, unsigned long long word) {
    const int lane = threadIdx.x & 63;
    const unsigned lo = (unsigned)(word & 0xffffffffull), hi = (unsigned)(word >> 32);
    bool covered = false;
#pragma unroll 9
    for (int d = 1; d < 64; ++d) {
        const int j = (lane + d) & 63;
        const int other_pix = __shfl(pix, j, 64);
        const unsigned long long other = ((unsigned long long)__shfl(hi, j, 64) << 32) | __shfl(lo, j, 64);
        covered |= other_pix == pix && (other > word || (other == word && j > lane));
    }
    return covered;
}

// PASS 0: float32 rows, word = z << 32 | row.  PASS 1: float64, word = z.  PASS 2: float64, the highest row among those whose z
// is the pixel's word.  Passes 0 and 1 add the rows to the counters
template <typename Source, int PASS>
__global__ __launch_bounds__(ELEV_THREADS) void k_elev_splat(Source src, ElevGeom<typename Source::real> g,
                                                             unsigned long long* keys, int* rows, ElevCounters* cnt) {
    typedef typename Source::real T;
    const int n = src.count();
    const long long stride = (long long)gridDim.x * ELEV_THREADS;
    unsigned n_in = 0, n_out = 0, n_nan = 0;
    // (the bound of the loop is the workgroup's: every lane of a wave takes part in the shuffles of elev_covered)
    for (long long first = (long long)blockIdx.x * ELEV_THREADS; first < n; first += stride) {
        const long long i = first + threadIdx.x;
        T p[3];
        int pix = -1, kind = -1;
        T zc = (T)0;
        if (i < n && src.fetch((int)i, p)) kind = elev_row(g, p, &pix, &zc);
        n_in += kind == ELEV_ROW_IN;
        n_out += kind == ELEV_ROW_OUTSIDE;
        n_nan += kind == ELEV_ROW_NAN;
        const bool in = kind == ELEV_ROW_IN;
        if (!in) pix = -1;
        if constexpr (PASS == 2) {
            if (in && elevation_key64((double)zc, g.flip) == keys[pix] &&  // (final: the first pass is over)
                (int)i > __hip_atomic_load(&rows[pix], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(&rows[pix], (int)i);
        } else {
            unsigned long long word = 0ull;
            if (in) word = PASS == 0 ? elevation_key32((float)zc, g.flip, (uint32_t)i) : elevation_key64((double)zc, g.flip);
            const bool covered = Source::COVER && elev_covered(pix, word);
            if (in && !covered && word > __hip_atomic_load(&keys[pix], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMax(&keys[pix], word);
        }
    }
    if (PASS == 2) return;
    n_in = elev_wave_sum(n_in);
    n_out = elev_wave_sum(n_out);
    n_nan = elev_wave_sum(n_nan);
    if ((threadIdx.x & 63) == 0) {
        ElevCounters* mine = cnt + (blockIdx.x & (ELEV_COUNTER_SHARDS - 1));
        if (n_in) atomicAdd(&mine->in_image, (unsigned long long)n_in);
        if (n_out) atomicAdd(&mine->outside, (unsigned long long)n_out);
        if (n_nan) atomicAdd(&mine->nan_z, (unsigned long long)n_nan);
    }
}

template <typename Source, bool PACKED>
__global__ __launch_bounds__(ELEV_THREADS) void k_elev_resolve(Source src, ElevGeom<typename Source::real> g,
                                                               const unsigned long long* __restrict__ keys,
                                                               const int* __restrict__ rows, int pixels, float empty_theta,
                                                               const unsigned char* __restrict__ lut, unsigned char* __restrict__ rgb,
                                                               float* __restrict__ theta_out, float* __restrict__ points,
                                                               int* __restrict__ index, ElevCounters* cnt) {
    typedef typename Source::real T;
    const long long px = (long long)blockIdx.x * ELEV_THREADS + threadIdx.x;
    const bool live = px < pixels;
    int row = -1;
    if (live) row = PACKED ? (keys[px] ? (int)(unsigned)(keys[px] & 0xffffffffull) : -1) : rows[px];
    float theta = empty_theta, x = 0.f, y = 0.f, z = 0.f;
    if (row >= 0) {
        T p[3];
        (void)src.fetch(row, p);
        theta = elevation_theta(elevation_clip(p[2], g.lo, g.hi), g.lo, g.den);
        x = (float)p[0];
        y = (float)p[1];
        z = (float)p[2];
    }
    if (live) {
        const int c = elevation_colour_row(theta);
        rgb[3 * px] = lut[3 * c];
        rgb[3 * px + 1] = lut[3 * c + 1];
        rgb[3 * px + 2] = lut[3 * c + 2];
        theta_out[px] = theta;
        points[3 * px] = x;
        points[3 * px + 1] = y;
        points[3 * px + 2] = z;
        index[px] = row;
    }
    const unsigned long long filled = __ballot(row >= 0);
    if ((threadIdx.x & 63) == 0 && filled)
        atomicAdd(&cnt[blockIdx.x & (ELEV_COUNTER_SHARDS - 1)].filled, (unsigned long long)__popcll(filled));
}

}  // namespace icp

using namespace icp;

struct icp_elevation {
    icp_ctx* ctx = nullptr;
    int64_t height = 0, width = 0, max_rows = 0;
    ElevGeom<float> g32{};
    ElevGeom<double> g64{};
    float empty_theta = 0.f;
    unsigned long long* keys = nullptr;  // [H * W] z-buffer words
    int* rows = nullptr;                 // [H * W] winning rows of the two-pass splat
    unsigned char* lut = nullptr;        // [259][3]
    unsigned char* rgb = nullptr;        // [H * W][3]
    float* theta = nullptr;              // [H * W]
    float* points = nullptr;             // [H * W][3]
    int* index = nullptr;                // [H * W]
    ElevCounters* cnt = nullptr;         // [ELEV_COUNTER_SHARDS]
    ElevCounters* cnt_host = nullptr;    // ... pinned
    void* stage_dev = nullptr;           // [max_rows][3] float64: host rows on their way in (allocated by the first host build)
    void* stage_host = nullptr;          // ... pinned
    hipEvent_t stage_copied = nullptr;   // the last host build's copy has left the pinned buffer
};

namespace {

void elevation_free(icp_elevation* e) {
    void* dev[] = {e->keys, e->rows, e->lut, e->rgb, e->theta, e->points, e->index, e->cnt, e->stage_dev};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (e->stage_host) (void)hipHostFree(e->stage_host);
    if (e->cnt_host) (void)hipHostFree(e->cnt_host);
    if (e->stage_copied) (void)hipEventDestroy(e->stage_copied);
    delete e;
}

template <typename T>
ElevGeom<T> make_geom(int64_t height, int64_t width, double pixel, double z_min, double z_max, int flip) {
    ElevGeom<T> g;
    g.pixel = (T)pixel;
    g.half_h = (T)(height / 2);
    g.half_w = (T)(width / 2);
    g.lo = (T)z_min;
    g.hi = (T)z_max;
    g.den = (T)(z_max - z_min);
    g.height = (int)height;
    g.width = (int)width;
    g.flip = flip ? 1 : 0;
    return g;
}

// clear, splat (one pass packed, two otherwise), resolve
template <typename Source, bool PACKED>
int elevation_launch(icp_elevation* e, const Source& src, const ElevGeom<typename Source::real>& g, int64_t splat_blocks) {
    icp_ctx* ctx = e->ctx;
    const int pixels = (int)(e->height * e->width);
    const dim3 pixel_grid((unsigned)elevation_blocks(pixels)), threads(ELEV_THREADS);
    hipLaunchKernelGGL(k_elev_clear, pixel_grid, threads, 0, ctx->stream, e->keys, e->rows, pixels, e->cnt);
    if (splat_blocks > 0) {
        const dim3 grid((unsigned)splat_blocks);
        if constexpr (PACKED) {
            hipLaunchKernelGGL((k_elev_splat<Source, 0>), grid, threads, 0, ctx->stream, src, g, e->keys, e->rows, e->cnt);
        } else {
            hipLaunchKernelGGL((k_elev_splat<Source, 1>), grid, threads, 0, ctx->stream, src, g, e->keys, e->rows, e->cnt);
            hipLaunchKernelGGL((k_elev_splat<Source, 2>), grid, threads, 0, ctx->stream, src, g, e->keys, e->rows, e->cnt);
        }
    }
    hipLaunchKernelGGL((k_elev_resolve<Source, PACKED>), pixel_grid, threads, 0, ctx->stream, src, g, e->keys, e->rows, pixels,
                       e->empty_theta, e->lut, e->rgb, e->theta, e->points, e->index, e->cnt);
    ICP_HIP(ctx, hipGetLastError());
    return ICP_OK;
}

int elevation_home(icp_elevation* e, void* user, const void* dev, size_t bytes, int out_mem) {
    if (!user) return ICP_OK;
    ICP_HIP(e->ctx, hipMemcpyAsync(user, dev, bytes, out_mem == ICP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                   e->ctx->stream));
    return ICP_OK;
}

}  // namespace

namespace icp {

// refine.hip reads the float32 point behind every pixel in place
icp_ctx* elevation_context(icp_elevation* img) { return img->ctx; }
const float* elevation_points_device(icp_elevation* img, int64_t* rows) {
    *rows = img->height * img->width;
    return img->points;
}

}  // namespace icp

extern "C" {

int icp_elevation_create(icp_ctx* ctx, int64_t height, int64_t width, double pixel_size, double z_min, double z_max, int flip,
                         const uint8_t* lut, int64_t max_rows, icp_elevation** out) {
    if (!ctx) return ICP_ERR_INVALID_ARGUMENT;
    if (!out) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_elevation_create: out is NULL");
    *out = nullptr;
    char why[160];
    if (elevation_create_refusals(height, width, pixel_size, z_min, z_max, lut, max_rows, why))
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    DeviceGuard guard(ctx, false);
    icp_elevation* e = new (std::nothrow) icp_elevation();
    if (!e) return fail(ctx, ICP_ERR_HIP, "icp_elevation_create: out of host memory");
    e->ctx = ctx;
    e->height = height;
    e->width = width;
    e->max_rows = max_rows;
    e->g32 = make_geom<float>(height, width, pixel_size, z_min, z_max, flip);
    e->g64 = make_geom<double>(height, width, pixel_size, z_min, z_max, flip);
    e->empty_theta = (float)z_min;
    const size_t pixels = (size_t)(height * width);
    hipError_t err = hipMalloc((void**)&e->keys, pixels * sizeof(unsigned long long));
    if (err == hipSuccess) err = hipMalloc((void**)&e->rows, pixels * sizeof(int));
    if (err == hipSuccess) err = hipMalloc((void**)&e->lut, ELEV_LUT_ROWS * 3);
    if (err == hipSuccess) err = hipMalloc((void**)&e->rgb, pixels * 3);
    if (err == hipSuccess) err = hipMalloc((void**)&e->theta, pixels * sizeof(float));
    if (err == hipSuccess) err = hipMalloc((void**)&e->points, pixels * 3 * sizeof(float));
    if (err == hipSuccess) err = hipMalloc((void**)&e->index, pixels * sizeof(int));
    if (err == hipSuccess) err = hipMalloc((void**)&e->cnt, ELEV_COUNTER_SHARDS * sizeof(ElevCounters));
    if (err == hipSuccess) err = hipHostMalloc((void**)&e->cnt_host, ELEV_COUNTER_SHARDS * sizeof(ElevCounters), hipHostMallocDefault);
    // (the table is the caller's pageable memory: copied before the call returns)
    if (err == hipSuccess) err = hipMemcpy(e->lut, lut, ELEV_LUT_ROWS * 3, hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        ctx->error = std::string("icp_elevation_create: ") + hipGetErrorString(err);
        elevation_free(e);
        return ICP_ERR_HIP;
    }
    // an image that has not been built yet reads as the empty image
    const int rc = elevation_launch<ElevRows<float>, true>(e, ElevRows<float>{nullptr, 0}, e->g32, 0);
    if (rc) {
        elevation_free(e);
        return rc;
    }
    *out = e;
    return ICP_OK;
}

void icp_elevation_destroy(icp_elevation* img) {
    if (!img) return;
    DeviceGuard guard(img->ctx, false);
    (void)hipStreamSynchronize(img->ctx->stream);
    elevation_free(img);
}

int icp_elevation_build(icp_elevation* img, const void* xyz, int64_t n, int mem, int dtype) {
    if (!img) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = img->ctx;
    char why[160];
    if (elevation_build_refusals(n, img->max_rows, mem, dtype, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    if (n > 0 && !xyz) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_elevation_build: xyz is NULL");
    DeviceGuard guard(ctx, false);
    const void* rows = xyz;
    if (mem == ICP_MEM_HOST && n > 0) {
        const size_t cap_bytes = (size_t)img->max_rows * 3 * sizeof(double);
        const size_t bytes = (size_t)n * 3 * (dtype == ICP_ELEVATION_F64 ? sizeof(double) : sizeof(float));
        if (!img->stage_dev) ICP_HIP(ctx, hipMalloc(&img->stage_dev, cap_bytes));
        if (!img->stage_host) ICP_HIP(ctx, hipHostMalloc(&img->stage_host, cap_bytes, hipHostMallocDefault));
        if (!img->stage_copied) ICP_HIP(ctx, hipEventCreateWithFlags(&img->stage_copied, hipEventDisableTiming));
        else ICP_HIP(ctx, hipEventSynchronize(img->stage_copied));  // (the previous copy out of the pinned rows, not its build)
        memcpy(img->stage_host, xyz, bytes);
        ICP_HIP(ctx, hipMemcpyAsync(img->stage_dev, img->stage_host, bytes, hipMemcpyHostToDevice, ctx->stream));
        ICP_HIP(ctx, hipEventRecord(img->stage_copied, ctx->stream));
        rows = img->stage_dev;
    }
    if (dtype == ICP_ELEVATION_F64)
        return elevation_launch<ElevRows<double>, false>(img, ElevRows<double>{(const double*)rows, (int)n}, img->g64, elevation_blocks(n));
    return elevation_launch<ElevRows<float>, true>(img, ElevRows<float>{(const float*)rows, (int)n}, img->g32, elevation_blocks(n));
}

int icp_elevation_build_aggmap(icp_elevation* img, icp_aggmap* map, int32_t frame_lo, int32_t frame_hi, const double pose[16]) {
    if (!img) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = img->ctx;
    if (!map) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_elevation_build_aggmap: map is NULL");
    char why[160];
    if (elevation_build_aggmap_refusals(ctx, map->ctx, frame_lo, frame_hi, pose, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    DeviceGuard guard(ctx, false);
    ElevWindow src;
    src.pts = map->pts;
    src.first_frame = map->first_frame;
    src.size_cell = &map->cnt->size[map->parity];
    src.capacity = (int)map->capacity;
    src.lo = (int)frame_lo;
    src.hi = (int)frame_hi;
    memcpy(src.pose.m, pose, sizeof(src.pose.m));
    return elevation_launch<ElevWindow, false>(img, src, img->g64, elevation_window_blocks(map->capacity));
}

int icp_elevation_get(icp_elevation* img, uint8_t* rgb_out, float* theta_out, float* points_out, int32_t* index_out, int out_mem) {
    if (!img) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = img->ctx;
    char why[160];
    if (elevation_get_refusals(out_mem, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    DeviceGuard guard(ctx, false);
    const size_t pixels = (size_t)(img->height * img->width);
    int rc;
    if ((rc = elevation_home(img, rgb_out, img->rgb, pixels * 3, out_mem))) return rc;
    if ((rc = elevation_home(img, theta_out, img->theta, pixels * sizeof(float), out_mem))) return rc;
    if ((rc = elevation_home(img, points_out, img->points, pixels * 3 * sizeof(float), out_mem))) return rc;
    if ((rc = elevation_home(img, index_out, img->index, pixels * sizeof(int), out_mem))) return rc;
    if (out_mem == ICP_MEM_HOST) ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICP_OK;
}

int icp_elevation_stats(icp_elevation* img, icp_elevation_counters* out) {
    if (!img) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = img->ctx;
    if (!out) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_elevation_stats: out is NULL");
    DeviceGuard guard(ctx, false);
    ICP_HIP(ctx, hipMemcpyAsync(img->cnt_host, img->cnt, ELEV_COUNTER_SHARDS * sizeof(ElevCounters), hipMemcpyDeviceToHost, ctx->stream));
    ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    out->rows_in_image = out->rows_outside = out->rows_nan_z = out->filled_pixels = 0;
    for (int k = 0; k < ELEV_COUNTER_SHARDS; ++k) {
        out->rows_in_image += (int64_t)img->cnt_host[k].in_image;
        out->rows_outside += (int64_t)img->cnt_host[k].outside;
        out->rows_nan_z += (int64_t)img->cnt_host[k].nan_z;
        out->filled_pixels += (int64_t)img->cnt_host[k].filled;
    }
    return ICP_OK;
}

}  // extern "C"
