// Aggregated world map: one point per voxel of everything a drive has seen, kept on the device and fed frame by frame.
//
// The first step of the reference's loop closure (slam/loop_closure.py:272-291: grid-sample every registered cloud, move it by
// its absolute pose — slam/common/pose.py:40-49 —, concatenate a window of frames, re-express the window in the frame of its
// middle pose), as a persistent structure instead of a per-window concatenation on the host.
//
//   world point   w = ((r0 x + r1 y) + r2 z) + t        float64, every product and sum rounded once (no contraction)
//   voxel         c = rint(w / v)                       half to even: voxel_coord of the grid sample (voxel_device.h)
//   key           the three coordinates, biased, in 63 bits (aggmap_plan.h): EXACT — two voxels never merge
//   creation      a voxel belongs to the first insert that reaches it; its point is the w of the row with the SMALLEST index
//                 among that insert's rows in it; stored points are numbered insert by insert, and within an insert by
//                 ascending index of those rows: the map is a deterministic array
//   updates       every finite in-range row that falls into a stored voxel adds 1 to its hits and raises its last frame
//                 (integer atomics: no order dependence)
//   capacity      voxels beyond the capacity are claimed but stay unstored; their rows — and, in a full map, rows in unknown
//                 voxels — are counted as dropped
//
// One insert = three launches on the context's stream, no host read, whatever the data:
//   1. k_aggmap_claim  a thread per row.  The lanes of a wave that share a key are grouped by ballots (as hash_dedupe_body of
//                      the grid sample does); the leader — the group's lowest row — claims the key's slot (64-bit atomicCAS;
//                      a full map is only looked up), adds the group's size to the slot's hits, raises its last frame and, where
//                      the voxel is new in this insert, lowers the slot's candidate row (atomicMin);
//   2. k_aggmap_count  a row is a WINNER when it is its slot's candidate; every workgroup counts the winners of its rows;
//   3. k_aggmap_emit   every workgroup sums the counts of the workgroups before it, scans its own winners and stores them
//                      at map size + rank: point, first frame, slot.  A winner past the capacity marks its slot unstored and
//                      moves the slot's hits to the dropped counter.  The last workgroup writes the new size into the OTHER
//                      of two size cells (the launches of the next insert read that one).
// Every probe loop ends after as many steps as the table has slots and sets a bit of the error word then (the table is at
// most half full by construction: aggmap_slot_count); nothing in this unit waits for another thread.
#include <limits.h>
#include <string.h>

#include <new>

#include "aggmap_plan.h"
#include "aggmap_device.h"
#include "icp_internal.h"
#include "voxel_device.h"

namespace icp {

__device__ __forceinline__ unsigned long long agg_wave_sum(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned lo = __shfl_down((unsigned)(v & 0xffffffffull), o, 64), hi = __shfl_down((unsigned)(v >> 32), o, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;  // (lane 0 holds the sum)
}

__global__ __launch_bounds__(AGGMAP_THREADS) void k_aggmap_clear(unsigned long long* __restrict__ keys, AggSlot* __restrict__ meta,
                                                                 unsigned long long slots, AggCounters* __restrict__ cnt) {
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long s = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; s < slots; s += stride) {
        keys[s] = AGGMAP_EMPTY;
        AggSlot e;
        e.cand = INT_MAX;
        e.idx = AGG_NEW;
        e.hits = 0u;
        e.last = INT_MIN;
        meta[s] = e;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        cnt->size[0] = cnt->size[1] = 0;
        cnt->error = 0;
        cnt->sub_count = 0;
        cnt->dropped = cnt->out_of_range = cnt->nonfinite = 0ull;
    }
}

__global__ __launch_bounds__(AGGMAP_THREADS) void k_aggmap_claim(const float* __restrict__ xyz, int n, AggPose pose, double voxel,
                                                                 int frame_id, unsigned long long* keys, AggSlot* meta,
                                                                 unsigned long long mask, int capacity, int parity,
                                                                 AggCounters* cnt, int* __restrict__ row_slot) {
    const long long i = (long long)blockIdx.x * AGGMAP_THREADS + threadIdx.x;
    const bool in = i < n;
    bool nonfinite = false, outside = false;
    unsigned long long key = 0;
    if (in) {
        const double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1], z = (double)xyz[3 * i + 2];
        const double wx = agg_world(pose, 0, x, y, z), wy = agg_world(pose, 1, x, y, z), wz = agg_world(pose, 2, x, y, z);
        if (!(isfinite(wx) && isfinite(wy) && isfinite(wz))) {
            nonfinite = true;
        } else {
            // the range is tested on the doubles: the conversion below is always defined
            const double cx = voxel_coord_real(wx, voxel), cy = voxel_coord_real(wy, voxel), cz = voxel_coord_real(wz, voxel);
            if (aggmap_coord_in_range(cx) && aggmap_coord_in_range(cy) && aggmap_coord_in_range(cz))
                key = aggmap_pack((long long)cx, (long long)cy, (long long)cz);
            else
                outside = true;
        }
    }
    const bool active = in && !nonfinite && !outside;
    const int lane = threadIdx.x & 63;
    const unsigned long long n_nonfinite = __ballot(nonfinite), n_outside = __ballot(outside);
    // lanes of the wave with the same key: the lowest lane holds the smallest row (rows ascend with the lane)
    unsigned long long todo = __ballot(active);
    bool leader = false;
    unsigned group = 0;
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        const unsigned lo = __shfl((unsigned)(key & 0xffffffffull), l, 64), hi = __shfl((unsigned)(key >> 32), l, 64);
        const unsigned long long k = ((unsigned long long)hi << 32) | lo;
        const unsigned long long same = __ballot(active && key == k);
        if (lane == l) {
            leader = true;
            group = (unsigned)__popcll(same);
        }
        todo &= ~same;
    }
    int mine = -1;  // the slot of a voxel this insert creates (leaders only: a winner is always its group's leader)
    unsigned long long drop = 0;
    if (leader) {
        const bool full = cnt->size[parity] >= capacity;  // a full map creates nothing: looked up, not claimed
        unsigned long long s = aggmap_slot(key, mask);
        long long found = -1;
        bool unknown = false;
        for (unsigned long long step = 0; step <= mask; ++step) {
            const unsigned long long old = full ? __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                                : atomicCAS(&keys[s], AGGMAP_EMPTY, key);
            if (old == key || (!full && old == AGGMAP_EMPTY)) {
                found = (long long)s;
                break;
            }
            if (old == AGGMAP_EMPTY) {
                unknown = true;
                break;
            }
            s = (s + 1) & mask;
        }
        if (found < 0) {
            if (!unknown) atomicOr(&cnt->error, AGGMAP_ERR_PROBE);  // every slot visited: cannot happen in a half-empty table
            drop = group;
        } else {
            const int idx = meta[found].idx;  // (written by the emit launch only)
            if (idx == AGG_UNSTORED) {
                drop = group;
            } else {
                atomicAdd(&meta[found].hits, group);
                atomicMax(&meta[found].last, frame_id);
                if (idx == AGG_NEW) {
                    atomicMin(&meta[found].cand, (int)i);
                    mine = (int)found;
                }
            }
        }
    }
    if (in) row_slot[i] = mine;
    drop = agg_wave_sum(drop);
    if (lane == 0) {
        if (drop) atomicAdd(&cnt->dropped, drop);
        if (n_nonfinite) atomicAdd(&cnt->nonfinite, (unsigned long long)__popcll(n_nonfinite));
        if (n_outside) atomicAdd(&cnt->out_of_range, (unsigned long long)__popcll(n_outside));
    }
}

__device__ __forceinline__ bool agg_winner(const int* __restrict__ row_slot, const AggSlot* __restrict__ meta, long long i, int n) {
    if (i >= n) return false;
    const int s = row_slot[i];
    return s >= 0 && meta[s].cand == (int)i;
}

// sum of one int per thread over the workgroup (AGGMAP_THREADS threads), returned to every thread; `cell`: four ints of LDS
__device__ __forceinline__ int agg_block_sum(int v, int* cell) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // (the cells may still be read from a previous call)
    if ((threadIdx.x & 63) == 0) cell[threadIdx.x >> 6] = v;
    __syncthreads();
    return cell[0] + cell[1] + cell[2] + cell[3];
}

__global__ __launch_bounds__(AGGMAP_THREADS) void k_aggmap_count(const int* __restrict__ row_slot, const AggSlot* __restrict__ meta,
                                                                 int n, int rows_per_block, int* __restrict__ counts) {
    __shared__ int cell[AGGMAP_THREADS / 64];
    const long long first = (long long)blockIdx.x * rows_per_block;
    int c = 0;
    for (int t = 0; t < rows_per_block; t += AGGMAP_THREADS) c += agg_winner(row_slot, meta, first + t + threadIdx.x, n) ? 1 : 0;
    c = agg_block_sum(c, cell);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

// rank of this thread's flag among the workgroup's flags (threads in order), and the workgroup's total
__device__ __forceinline__ int agg_block_rank(bool flag, int* cell, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long b = __ballot(flag);
    __syncthreads();
    if (lane == 0) cell[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < AGGMAP_THREADS / 64; ++w) {
        if (w < wave) off += cell[w];
        tot += cell[w];
    }
    *total = tot;
    return off + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(AGGMAP_THREADS) void k_aggmap_emit(const float* __restrict__ xyz, int n, AggPose pose, int frame_id,
                                                                const int* __restrict__ row_slot, AggSlot* meta,
                                                                int rows_per_block, const int* __restrict__ counts, int capacity,
                                                                int parity, AggCounters* cnt, double* __restrict__ pts,
                                                                int* __restrict__ first_frame, int* __restrict__ slot_of) {
    __shared__ int cell[AGGMAP_THREADS / 64];
    int before = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += AGGMAP_THREADS) before += counts[b];
    long long run = (long long)cnt->size[parity] + agg_block_sum(before, cell);
    const long long first = (long long)blockIdx.x * rows_per_block;
    unsigned long long drop = 0;
    for (int t = 0; t < rows_per_block; t += AGGMAP_THREADS) {
        const long long i = first + t + threadIdx.x;
        const bool win = agg_winner(row_slot, meta, i, n);
        int total;
        const long long pos = run + agg_block_rank(win, cell, &total);
        run += total;
        if (!win) continue;
        const int s = row_slot[i];
        if (pos < capacity) {
            const double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1], z = (double)xyz[3 * i + 2];
            pts[3 * pos] = agg_world(pose, 0, x, y, z);
            pts[3 * pos + 1] = agg_world(pose, 1, x, y, z);
            pts[3 * pos + 2] = agg_world(pose, 2, x, y, z);
            first_frame[pos] = frame_id;
            slot_of[pos] = s;
            meta[s].idx = (int)pos;
        } else {
            meta[s].idx = AGG_UNSTORED;
            drop += meta[s].hits;  // (final: the claim launch is over)
        }
    }
    drop = agg_wave_sum(drop);
    if ((threadIdx.x & 63) == 0 && drop) atomicAdd(&cnt->dropped, drop);
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) cnt->size[parity ^ 1] = (int)(run < capacity ? run : capacity);
}

// get: float32(w - origin), subtracted in float64 and rounded once, with the voxel's hits and frames; xyz64: w itself
__global__ __launch_bounds__(AGGMAP_THREADS) void k_aggmap_get(const double* __restrict__ pts, const int* __restrict__ first_frame,
                                                               const int* __restrict__ slot_of, const AggSlot* __restrict__ meta,
                                                               int size, double ox, double oy, double oz, float* __restrict__ xyz,
                                                               double* __restrict__ xyz64, unsigned* __restrict__ hits,
                                                               int* __restrict__ first_out, int* __restrict__ last_out) {
    const long long i = (long long)blockIdx.x * AGGMAP_THREADS + threadIdx.x;
    if (i >= size) return;
    const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    if (xyz) {
        xyz[3 * i] = (float)__dsub_rn(x, ox);
        xyz[3 * i + 1] = (float)__dsub_rn(y, oy);
        xyz[3 * i + 2] = (float)__dsub_rn(z, oz);
    }
    if (xyz64) {
        xyz64[3 * i] = x;
        xyz64[3 * i + 1] = y;
        xyz64[3 * i + 2] = z;
    }
    const AggSlot e = meta[slot_of[i]];
    if (hits) hits[i] = e.hits;
    if (first_out) first_out[i] = first_frame[i];
    if (last_out) last_out[i] = e.last;
}

// submap: the ordered compaction of the insert over the stored points with frame_lo <= first_frame < frame_hi
__global__ __launch_bounds__(AGGMAP_THREADS) void k_aggmap_sub_count(const int* __restrict__ first_frame, int size, int lo, int hi,
                                                                     int rows_per_block, int* __restrict__ counts) {
    __shared__ int cell[AGGMAP_THREADS / 64];
    const long long first = (long long)blockIdx.x * rows_per_block;
    int c = 0;
    for (int t = 0; t < rows_per_block; t += AGGMAP_THREADS) {
        const long long i = first + t + threadIdx.x;
        if (i < size) {
            const int f = first_frame[i];
            c += (f >= lo && f < hi) ? 1 : 0;
        }
    }
    c = agg_block_sum(c, cell);
    if (threadIdx.x == 0) counts[blockIdx.x] = c;
}

__global__ __launch_bounds__(AGGMAP_THREADS) void k_aggmap_sub_emit(const double* __restrict__ pts, const int* __restrict__ first_frame,
                                                                    int size, int lo, int hi, AggPose pose, int rows_per_block,
                                                                    const int* __restrict__ counts, long long cap,
                                                                    float* __restrict__ xyz, int* __restrict__ index,
                                                                    AggCounters* cnt) {
    __shared__ int cell[AGGMAP_THREADS / 64];
    int before = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += AGGMAP_THREADS) before += counts[b];
    long long run = agg_block_sum(before, cell);
    const long long first = (long long)blockIdx.x * rows_per_block;
    for (int t = 0; t < rows_per_block; t += AGGMAP_THREADS) {
        const long long i = first + t + threadIdx.x;
        bool keep = false;
        if (i < size) {
            const int f = first_frame[i];
            keep = f >= lo && f < hi;
        }
        int total;
        const long long pos = run + agg_block_rank(keep, cell, &total);
        run += total;
        if (!keep || pos >= cap) continue;
        const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
        xyz[3 * pos] = (float)agg_world(pose, 0, x, y, z);
        xyz[3 * pos + 1] = (float)agg_world(pose, 1, x, y, z);
        xyz[3 * pos + 2] = (float)agg_world(pose, 2, x, y, z);
        index[pos] = (int)i;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) cnt->sub_count = (int)run;
}

}  // namespace icp

using namespace icp;

namespace {

AggPose pose_rows(const double* pose16) {
    AggPose p;
    memcpy(p.m, pose16, sizeof(p.m));
    return p;
}

void aggmap_free(icp_aggmap* m) {
    void* dev[] = {m->keys, m->meta, m->pts, m->first_frame, m->slot_of, m->row_slot, m->counts, m->cnt, m->stage_dev};
    for (void* p : dev)
        if (p) (void)hipFree(p);
    if (m->stage_host) (void)hipHostFree(m->stage_host);
    if (m->cnt_host) (void)hipHostFree(m->cnt_host);
    if (m->stage_copied) (void)hipEventDestroy(m->stage_copied);
    m->out_xyz.release();
    m->out_a.release();
    m->out_b.release();
    m->out_c.release();
    delete m;
}

int aggmap_launch_clear(icp_aggmap* m) {
    icp_ctx* ctx = m->ctx;
    const uint64_t blocks = std::min<uint64_t>((m->slots + AGGMAP_THREADS - 1) / AGGMAP_THREADS, 16384);
    hipLaunchKernelGGL(k_aggmap_clear, dim3((unsigned)blocks), dim3(AGGMAP_THREADS), 0, ctx->stream, m->keys, m->meta,
                       (unsigned long long)m->slots, m->cnt);
    ICP_HIP(ctx, hipGetLastError());
    m->parity = 0;
    m->inserts = 0;
    return ICP_OK;
}

// the counters as they stand behind everything enqueued so far (synchronises)
int aggmap_read_counters(icp_aggmap* m) {
    icp_ctx* ctx = m->ctx;
    ICP_HIP(ctx, hipMemcpyAsync(m->cnt_host, m->cnt, sizeof(AggCounters), hipMemcpyDeviceToHost, ctx->stream));
    ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICP_OK;
}

// where a kernel writes an output of `bytes`: the caller's device memory, or a buffer of the map on its way to the host
int aggmap_out(icp_aggmap* m, void* user, size_t bytes, int out_mem, DeviceBuffer& stage, void** dev) {
    *dev = nullptr;
    if (!user) return ICP_OK;
    if (out_mem == ICP_MEM_DEVICE) {
        *dev = user;
        return ICP_OK;
    }
    ICP_HIP(m->ctx, stage.reserve(bytes ? bytes : 1));
    *dev = stage.ptr;
    return ICP_OK;
}

int aggmap_home(icp_aggmap* m, void* user, const void* dev, size_t bytes, int out_mem) {
    if (!user || out_mem == ICP_MEM_DEVICE || !bytes) return ICP_OK;
    ICP_HIP(m->ctx, hipMemcpyAsync(user, dev, bytes, hipMemcpyDeviceToHost, m->ctx->stream));
    return ICP_OK;
}

}  // namespace

extern "C" {

int icp_aggmap_create(icp_ctx* ctx, double voxel_size, int64_t capacity, int64_t max_insert_rows, icp_aggmap** out) {
    if (!ctx) return ICP_ERR_INVALID_ARGUMENT;
    if (!out) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_aggmap_create: out is NULL");
    *out = nullptr;
    char why[160];
    if (aggmap_create_refusals(voxel_size, capacity, max_insert_rows, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    DeviceGuard guard(ctx, false);
    icp_aggmap* m = new (std::nothrow) icp_aggmap();
    if (!m) return fail(ctx, ICP_ERR_HIP, "icp_aggmap_create: out of host memory");
    m->ctx = ctx;
    m->voxel = voxel_size;
    m->capacity = capacity;
    m->max_rows = max_insert_rows;
    m->slots = aggmap_slot_count(capacity, max_insert_rows);
    hipError_t e = hipMalloc((void**)&m->keys, m->slots * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&m->meta, m->slots * sizeof(AggSlot));
    if (e == hipSuccess) e = hipMalloc((void**)&m->pts, (size_t)capacity * 3 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&m->first_frame, (size_t)capacity * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&m->slot_of, (size_t)capacity * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&m->row_slot, (size_t)max_insert_rows * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&m->counts, (size_t)(AGGMAP_MAX_BLOCKS + 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&m->cnt, sizeof(AggCounters));
    if (e == hipSuccess) e = hipHostMalloc((void**)&m->cnt_host, sizeof(AggCounters), hipHostMallocDefault);
    if (e != hipSuccess) {
        ctx->error = std::string("icp_aggmap_create: ") + hipGetErrorString(e);
        aggmap_free(m);
        return ICP_ERR_HIP;
    }
    const int rc = aggmap_launch_clear(m);
    if (rc) {
        aggmap_free(m);
        return rc;
    }
    *out = m;
    return ICP_OK;
}

void icp_aggmap_destroy(icp_aggmap* map) {
    if (!map) return;
    DeviceGuard guard(map->ctx, false);
    (void)hipStreamSynchronize(map->ctx->stream);
    aggmap_free(map);
}

int icp_aggmap_insert(icp_aggmap* map, const float* xyz, int64_t n, int mem, const double pose[16], int32_t frame_id) {
    if (!map) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = map->ctx;
    char why[160];
    if (aggmap_insert_refusals(n, map->max_rows, pose, mem, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    if (n > 0 && !xyz) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_aggmap_insert: xyz is NULL");
    DeviceGuard guard(ctx, false);
    map->inserts += 1;
    if (n == 0) return ICP_OK;
    const float* rows = xyz;
    if (mem == ICP_MEM_HOST) {
        const size_t cap_bytes = (size_t)map->max_rows * 3 * sizeof(float);
        if (!map->stage_dev) ICP_HIP(ctx, hipMalloc((void**)&map->stage_dev, cap_bytes));
        if (!map->stage_host) ICP_HIP(ctx, hipHostMalloc((void**)&map->stage_host, cap_bytes, hipHostMallocDefault));
        if (!map->stage_copied) ICP_HIP(ctx, hipEventCreateWithFlags(&map->stage_copied, hipEventDisableTiming));
        else ICP_HIP(ctx, hipEventSynchronize(map->stage_copied));  // (the previous copy out of the pinned rows, not its insert)
        memcpy(map->stage_host, xyz, (size_t)n * 3 * sizeof(float));
        ICP_HIP(ctx, hipMemcpyAsync(map->stage_dev, map->stage_host, (size_t)n * 3 * sizeof(float), hipMemcpyHostToDevice,
                                    ctx->stream));
        ICP_HIP(ctx, hipEventRecord(map->stage_copied, ctx->stream));
        rows = map->stage_dev;
    }
    const AggPose p = pose_rows(pose);
    const int rows_per_block = (int)aggmap_rows_per_block(n);
    const unsigned blocks = (unsigned)((n + rows_per_block - 1) / rows_per_block);
    hipLaunchKernelGGL(k_aggmap_claim, dim3((unsigned)((n + AGGMAP_THREADS - 1) / AGGMAP_THREADS)), dim3(AGGMAP_THREADS), 0,
                       ctx->stream, rows, (int)n, p, map->voxel, (int)frame_id, map->keys, map->meta,
                       (unsigned long long)(map->slots - 1), (int)map->capacity, map->parity, map->cnt, map->row_slot);
    hipLaunchKernelGGL(k_aggmap_count, dim3(blocks), dim3(AGGMAP_THREADS), 0, ctx->stream, map->row_slot, map->meta, (int)n,
                       rows_per_block, map->counts);
    hipLaunchKernelGGL(k_aggmap_emit, dim3(blocks), dim3(AGGMAP_THREADS), 0, ctx->stream, rows, (int)n, p, (int)frame_id,
                       map->row_slot, map->meta, rows_per_block, map->counts, (int)map->capacity, map->parity, map->cnt, map->pts,
                       map->first_frame, map->slot_of);
    ICP_HIP(ctx, hipGetLastError());
    map->parity ^= 1;
    return ICP_OK;
}

int icp_aggmap_stats(icp_aggmap* map, icp_aggmap_counters* out) {
    if (!map) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = map->ctx;
    if (!out) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_aggmap_stats: out is NULL");
    DeviceGuard guard(ctx, false);
    const int rc = aggmap_read_counters(map);
    if (rc) return rc;
    const AggCounters& c = *map->cnt_host;
    out->size = c.size[map->parity];
    out->inserts = map->inserts;
    out->dropped = (int64_t)c.dropped;
    out->out_of_range = (int64_t)c.out_of_range;
    out->nonfinite = (int64_t)c.nonfinite;
    out->error = c.error;
    return ICP_OK;
}

static int aggmap_get_impl(icp_aggmap* map, const double* origin, float* xyz_out, double* xyz64_out, uint32_t* hits_out,
                           int32_t* first_out, int32_t* last_out, int64_t cap, int out_mem, int64_t* size_out) {
    if (!map) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = map->ctx;
    char why[160];
    if (aggmap_get_refusals(out_mem, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    if (origin && !(isfinite(origin[0]) && isfinite(origin[1]) && isfinite(origin[2])))
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_aggmap_get: the origin has a non-finite entry");
    DeviceGuard guard(ctx, false);
    int rc = aggmap_read_counters(map);
    if (rc) return rc;
    const int64_t size = map->cnt_host->size[map->parity];
    if (size_out) *size_out = size;
    if (size > cap) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_aggmap_get: the outputs are shorter than the map (see *size_out)");
    if (size == 0) return ICP_OK;
    void *dx = nullptr, *dh = nullptr, *df = nullptr, *dl = nullptr;
    void* xyz_user = xyz64_out ? (void*)xyz64_out : (void*)xyz_out;
    const size_t xyz_bytes = (size_t)size * 3 * (xyz64_out ? sizeof(double) : sizeof(float));
    if ((rc = aggmap_out(map, xyz_user, xyz_bytes, out_mem, map->out_xyz, &dx))) return rc;
    if ((rc = aggmap_out(map, hits_out, (size_t)size * 4, out_mem, map->out_a, &dh))) return rc;
    if ((rc = aggmap_out(map, first_out, (size_t)size * 4, out_mem, map->out_b, &df))) return rc;
    if ((rc = aggmap_out(map, last_out, (size_t)size * 4, out_mem, map->out_c, &dl))) return rc;
    const double ox = origin ? origin[0] : 0.0, oy = origin ? origin[1] : 0.0, oz = origin ? origin[2] : 0.0;
    hipLaunchKernelGGL(k_aggmap_get, dim3((unsigned)((size + AGGMAP_THREADS - 1) / AGGMAP_THREADS)), dim3(AGGMAP_THREADS), 0,
                       ctx->stream, map->pts, map->first_frame, map->slot_of, map->meta, (int)size, ox, oy, oz,
                       xyz64_out ? (float*)nullptr : (float*)dx, xyz64_out ? (double*)dx : (double*)nullptr, (unsigned*)dh,
                       (int*)df, (int*)dl);
    ICP_HIP(ctx, hipGetLastError());
    if ((rc = aggmap_home(map, xyz_user, dx, xyz_bytes, out_mem))) return rc;
    if ((rc = aggmap_home(map, hits_out, dh, (size_t)size * 4, out_mem))) return rc;
    if ((rc = aggmap_home(map, first_out, df, (size_t)size * 4, out_mem))) return rc;
    if ((rc = aggmap_home(map, last_out, dl, (size_t)size * 4, out_mem))) return rc;
    if (out_mem == ICP_MEM_HOST) ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICP_OK;
}

int icp_aggmap_get(icp_aggmap* map, const double origin[3], float* xyz_out, uint32_t* hits_out, int32_t* first_frame_out,
                   int32_t* last_frame_out, int64_t cap, int out_mem, int64_t* size_out) {
    return aggmap_get_impl(map, origin, xyz_out, nullptr, hits_out, first_frame_out, last_frame_out, cap, out_mem, size_out);
}

int icp_aggmap_get_f64(icp_aggmap* map, double* xyz_out, int64_t cap, int out_mem, int64_t* size_out) {
    return aggmap_get_impl(map, nullptr, nullptr, xyz_out, nullptr, nullptr, nullptr, cap, out_mem, size_out);
}

int icp_aggmap_submap(icp_aggmap* map, int32_t frame_lo, int32_t frame_hi, const double pose[16], float* xyz_out,
                      int32_t* index_out, int64_t cap, int out_mem, int64_t* count_out) {
    if (!map) return ICP_ERR_INVALID_ARGUMENT;
    icp_ctx* ctx = map->ctx;
    char why[160];
    if (aggmap_submap_refusals(frame_lo, frame_hi, pose, out_mem, why)) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, why);
    if (!count_out) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_aggmap_submap: count_out is NULL");
    if (cap < 0 || (cap > 0 && (!xyz_out || !index_out)))
        return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_aggmap_submap: outputs for cap rows are needed");
    DeviceGuard guard(ctx, false);
    int rc = aggmap_read_counters(map);
    if (rc) return rc;
    const int64_t size = map->cnt_host->size[map->parity];
    *count_out = 0;
    if (size == 0) return ICP_OK;
    const int64_t room = std::min(cap, size);
    void *dx = nullptr, *di = nullptr;
    if ((rc = aggmap_out(map, xyz_out, (size_t)room * 12, out_mem, map->out_xyz, &dx))) return rc;
    if ((rc = aggmap_out(map, index_out, (size_t)room * 4, out_mem, map->out_a, &di))) return rc;
    const int rows_per_block = (int)aggmap_rows_per_block(size);
    const unsigned blocks = (unsigned)((size + rows_per_block - 1) / rows_per_block);
    hipLaunchKernelGGL(k_aggmap_sub_count, dim3(blocks), dim3(AGGMAP_THREADS), 0, ctx->stream, map->first_frame, (int)size,
                       (int)frame_lo, (int)frame_hi, rows_per_block, map->counts);
    hipLaunchKernelGGL(k_aggmap_sub_emit, dim3(blocks), dim3(AGGMAP_THREADS), 0, ctx->stream, map->pts, map->first_frame, (int)size,
                       (int)frame_lo, (int)frame_hi, pose_rows(pose), rows_per_block, map->counts, (long long)room, (float*)dx,
                       (int*)di, map->cnt);
    ICP_HIP(ctx, hipGetLastError());
    if ((rc = aggmap_read_counters(map))) return rc;
    const int64_t count = map->cnt_host->sub_count;
    *count_out = count;
    if (count > cap) return fail(ctx, ICP_ERR_INVALID_ARGUMENT, "icp_aggmap_submap: the outputs are shorter than the window (see *count_out)");
    if ((rc = aggmap_home(map, xyz_out, dx, (size_t)count * 12, out_mem))) return rc;
    if ((rc = aggmap_home(map, index_out, di, (size_t)count * 4, out_mem))) return rc;
    if (out_mem == ICP_MEM_HOST) ICP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ICP_OK;
}

int icp_aggmap_clear(icp_aggmap* map) {
    if (!map) return ICP_ERR_INVALID_ARGUMENT;
    DeviceGuard guard(map->ctx, false);
    return aggmap_launch_clear(map);
}

}  // extern "C"
