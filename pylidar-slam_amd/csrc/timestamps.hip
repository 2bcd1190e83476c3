// Time stamps of a rotating sensor's scan from the azimuth of its rows.
//
// Replaces `estimate_timestamps` (slam/common/geometry.py:443-466), the one producer of `numpy_pc_timestamps` the
// reference has for data without per-point times, and — fused with the scan correction — what its KITTI-360 reader does per
// frame (slam/dataset/kitti_360_dataset.py:170-185).  The reference, for the float32 rows of a .bin scan, in float32:
//
//   phis = arctan2(y, x) * (-1 if clockwise else +1)
//   phis -= phi_0                      (phi_0 rounded to float32)
//   phis[phis < 0] += 2 pi             (2 pi rounded to float32)
//   t = (phis - phis.min()) / (phis.max() - phis.min())
//
// numpy's float32 arctan2 is not correctly rounded (one ulp off the rounded float64 value in a third of the rows), so no
// kernel matches it bit for bit.  The device evaluates atan2 in float64 and rounds ONCE to float32 — the correctly rounded
// value, inside the reference's own float32-against-float64 spread — and follows the reference operation by operation from
// there: a numpy model holds the kernels bit for bit (tests/timestamps_audit.py).
//
// Two launches, the stream never waited on: k_azimuth writes phi and the per-workgroup min / max (DISTORT_PARTS workgroups,
// grid-stride; wave shuffle, four waves through LDS — the shape of minmax_f64_body, grid_sample.hip, in float32), then
// k_azimuth_normalise reduces the partials in a fixed order and writes the float32 quotient widened to float64, which is
// what icp_distort and the frame calls take.  fminf / fmaxf drop a NaN: a row with a NaN coordinate gets a NaN time stamp
// and leaves the others alone (numpy's min / max hand it on to every row).  One row, or rows on one azimuth: 0 / 0 = NaN
// for every row, as in the reference.
#include <stdint.h>
#include <string.h>

#include "icp_internal.h"
#include "projection_device.h"

namespace icp {

struct AzimuthParams {
    float sign;    // -1 clockwise, +1 counter-clockwise
    float phi_0;   // rounded to float32 on the host, like numpy's in-place float32 subtraction of a Python float
    float two_pi;  // float32(2 pi)
    int stride;    // floats per row: 3 or 4
};

// (the body of k_azimuth and of k_azimuth_batch)  vec4: stride 4 and a 16-byte aligned scan — one 16-byte load per row.
// xyz_out (may be NULL, uniform): the corrected row of KITTIOdometrySequence.correct_scan from the same load.
__device__ __forceinline__ void azimuth_body(const float* __restrict__ rows, int n, int vec4, const AzimuthParams& p,
                                             float* __restrict__ phi, float* __restrict__ part,
                                             double* __restrict__ xyz_out) {
    __shared__ float smin[4], smax[4];
    float mn = INFINITY, mx = -INFINITY;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        float x, y, z;
        if (vec4) {
            const float4 r = reinterpret_cast<const float4*>(rows)[i];
            x = r.x;
            y = r.y;
            z = r.z;
        } else {
            const float* r = rows + (size_t)i * p.stride;
            x = r[0];
            y = r[1];
            z = r[2];
        }
        float a = (float)atan2((double)y, (double)x);  // correctly rounded float32 (up to the float64 routine's last ulp)
        a = __fmul_rn(a, p.sign);                       // :459
        a = __fsub_rn(a, p.phi_0);                      // :460
        if (a < 0.0f) a = __fadd_rn(a, p.two_pi);       // :461
        phi[i] = a;
        mn = fminf(mn, a);
        mx = fmaxf(mx, a);
        if (xyz_out) kitti_correct_row(x, y, z, xyz_out + 3 * (size_t)i);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fminf(mn, __shfl_down(mn, o, 64));
        mx = fmaxf(mx, __shfl_down(mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        smin[threadIdx.x >> 6] = mn;
        smax[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {  // every workgroup writes its pair (+inf / -inf without rows): no stale partial survives
        part[2 * blockIdx.x] = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
        part[2 * blockIdx.x + 1] = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    }
}

// (the body of k_azimuth_normalise and of k_azimuth_normalise_batch): :463-466 in float32, widened
__device__ __forceinline__ void azimuth_normalise_body(const float* __restrict__ phi, int n,
                                                       const float* __restrict__ part, double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float mn = INFINITY, mx = -INFINITY;
    for (int k = 0; k < DISTORT_PARTS; ++k) {  // a few dozen values, L2-resident, in a fixed order
        mn = fminf(mn, part[2 * k]);
        mx = fmaxf(mx, part[2 * k + 1]);
    }
    out[i] = (double)(__fsub_rn(phi[i], mn) / __fsub_rn(mx, mn));  // correctly rounded float32 division; 0 / 0 = NaN
}

__global__ __launch_bounds__(256) void k_azimuth(const float* __restrict__ rows, int n, int vec4, AzimuthParams p,
                                                 float* __restrict__ phi, float* __restrict__ part,
                                                 double* __restrict__ xyz_out) {
    azimuth_body(rows, n, vec4, p, phi, part, xyz_out);
}

__global__ void k_azimuth_normalise(const float* __restrict__ phi, int n, const float* __restrict__ part,
                                    double* __restrict__ out) {
    azimuth_normalise_body(phi, n, part, out);
}

// B scans per launch: blockIdx.y = the member, its arguments by value in the kernel-argument segment (one small struct per
// kernel, as MinmaxBatchArgs / DistortBatchArgs of grid_sample.hip: the pointers stay global pointers).  n = 0: sits out.
struct AzimuthBatchEntry {
    const float* rows;
    float* phi;
    float* part;
    int n;
    int vec4;
};
struct AzimuthBatchArgs {
    AzimuthBatchEntry e[ICP_BATCH_MAX_SEQUENCES];
    AzimuthParams p;
};
struct AzimuthNormaliseBatchEntry {
    const float* phi;
    const float* part;
    double* out;
    int n;
};
struct AzimuthNormaliseBatchArgs {
    AzimuthNormaliseBatchEntry e[ICP_BATCH_MAX_SEQUENCES];
};
static_assert(sizeof(AzimuthBatchArgs) <= 4096 && sizeof(AzimuthNormaliseBatchArgs) <= 4096,
              "the per-member arguments of a batch kernel must fit the 4 KB kernel-argument segment");

__global__ __launch_bounds__(256) void k_azimuth_batch(AzimuthBatchArgs a) {
    const AzimuthBatchEntry& e = a.e[blockIdx.y];
    if (e.n <= 0) return;  // (uniform in the workgroup: nobody waits at the barrier below)
    azimuth_body(e.rows, e.n, e.vec4, a.p, e.phi, e.part, nullptr);
}

__global__ void k_azimuth_normalise_batch(AzimuthNormaliseBatchArgs a) {
    const AzimuthNormaliseBatchEntry& e = a.e[blockIdx.y];
    azimuth_normalise_body(e.phi, e.n, e.part, e.out);
}

static AzimuthParams azimuth_params(int stride, bool clockwise, double phi_0) {
    AzimuthParams p;
    p.sign = clockwise ? -1.0f : 1.0f;
    p.phi_0 = (float)phi_0;
    p.two_pi = (float)(2.0 * 3.14159265358979323846);
    p.stride = stride;
    return p;
}

static int vec4_rows(const float* rows, int stride) { return stride == 4 && ((uintptr_t)rows & 15u) == 0 ? 1 : 0; }

int estimate_timestamps_device(icp_ctx* ctx, const float* rows_dev, int64_t n, int stride, bool clockwise, double phi_0,
                               double* ts_dev, double* xyz_out_dev) {
    if (n <= 0) return ICP_OK;
    ICP_HIP(ctx, ctx->scan_a.reserve((size_t)n * sizeof(float)));
    ICP_HIP(ctx, ctx->scan_b.reserve((size_t)DISTORT_PARTS * 2 * sizeof(double)));  // (the size the de-skew asks for)
    float* phi = ctx->scan_a.as<float>();
    float* part = ctx->scan_b.as<float>();
    hipLaunchKernelGGL(k_azimuth, dim3(DISTORT_PARTS), dim3(256), 0, ctx->stream, rows_dev, (int)n,
                       vec4_rows(rows_dev, stride), azimuth_params(stride, clockwise, phi_0), phi, part, xyz_out_dev);
    hipLaunchKernelGGL(k_azimuth_normalise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const float*)phi, (int)n, (const float*)part, ts_dev);
    ICP_HIP(ctx, hipGetLastError());
    return ICP_OK;
}

int estimate_timestamps_batch_device(icp_ctx* const* ctxs, int count, const float* const* rows_dev, const int64_t* n,
                                     int stride, bool clockwise, double phi_0, double* const* ts_dev) {
    if (count <= 0 || count > ICP_BATCH_MAX_SEQUENCES) return ICP_OK;
    AzimuthBatchArgs az;
    AzimuthNormaliseBatchArgs nm;
    memset(&az, 0, sizeof(az));
    memset(&nm, 0, sizeof(nm));
    az.p = azimuth_params(stride, clockwise, phi_0);
    icp_ctx* first = ctxs[0];
    int64_t max_n = 0;
    for (int b = 0; b < count; ++b) {
        if (n[b] <= 0 || !rows_dev[b] || !ts_dev[b]) continue;  // sits out (n = 0 in both tables)
        icp_ctx* ctx = ctxs[b];
        ICP_HIP(ctx, ctx->scan_a.reserve((size_t)n[b] * sizeof(float)));
        ICP_HIP(ctx, ctx->scan_b.reserve((size_t)DISTORT_PARTS * 2 * sizeof(double)));
        az.e[b].rows = rows_dev[b];
        az.e[b].phi = ctx->scan_a.as<float>();
        az.e[b].part = ctx->scan_b.as<float>();
        az.e[b].n = (int)n[b];
        az.e[b].vec4 = vec4_rows(rows_dev[b], stride);
        nm.e[b].phi = az.e[b].phi;
        nm.e[b].part = az.e[b].part;
        nm.e[b].out = ts_dev[b];
        nm.e[b].n = (int)n[b];
        max_n = n[b] > max_n ? n[b] : max_n;
    }
    if (max_n <= 0) return ICP_OK;
    hipLaunchKernelGGL(k_azimuth_batch, dim3(DISTORT_PARTS, count), dim3(256), 0, first->stream, az);
    hipLaunchKernelGGL(k_azimuth_normalise_batch, dim3((unsigned)((max_n + 255) / 256), count), dim3(256), 0,
                       first->stream, nm);
    ICP_HIP(first, hipGetLastError());
    return ICP_OK;
}

}  // namespace icp
