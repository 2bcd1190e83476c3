// One call per odometry frame for B sequences: icp_batch_odometry_init / icp_batch_frame_launch / icp_batch_frame_end
// (include/icp_mi355x.h).  icp_frame_launch / icp_frame_end (frame.hip) for the members of a batch, the registering members'
// stages going through the BATCHED entry points of api.hip — icp_batch_preprocess, _project_rows, _stage, _register_launch,
// _register_end, _map_update_staged — stage by stage as icp_frame_launch / icp_frame_end do; host code only — every launch is one of theirs.  The
// sequence state is each member's own icp_frame_loop (frame_loop.h); who takes part in a step and what is refused is decided
// in batch_frame_plan.h.  A step that leaves members out runs on inner batches over the members at hand, cached by member mask
// (a batch is host bookkeeping plus lazily allocated descriptor tables, and a context may belong to several).
// Also everything the projective form (batch_pmap_frame.hip) goes through as well (batch_frame_loop.h): the upload, the
// preprocessing, the copy-out, the two ends of a launch, the dropping of a pending step and the end call — written once,
// against the BatchFrameKind each form hands in.
#include <string.h>

#include <algorithm>
#include <map>

#include "batch_frame_loop.h"

using namespace icp;

static_assert(BATCH_FRAME_MAX_MEMBERS == ICP_BATCH_MAX_SEQUENCES, "batch_frame_plan.h sizes its lists for ICP_BATCH_MAX_SEQUENCES members");

namespace icp {

// ---- shared with the projective form (batch_pmap_frame.hip): batch_frame_loop.h
int bf_fail(icp_batch* b, int code, const std::string& msg) {
    b->error = msg;
    return code;
}

int bf_hip(icp_batch* b, hipError_t e, const char* what) {
    if (e == hipSuccess) return ICP_OK;
    return bf_fail(b, ICP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
int bf_member_fail(icp_batch* b, int rc, const char* who, int member) {
    return bf_fail(b, rc, std::string(who) + ", member " + std::to_string(member) + ": " + b->members[member]->error);
}
int bf_member_hip(icp_batch* b, const char* who, int member, hipError_t e, const char* what) {
    if (e == hipSuccess) return ICP_OK;
    return bf_fail(b, ICP_ERR_HIP, std::string(who) + ", member " + std::to_string(member) + ": " + what + ": " + hipGetErrorString(e));
}

int pinned_reserve(icp_batch* b, void** ptr, size_t* have, size_t need) {
    if (*ptr && *have >= need) return ICP_OK;
    if (*ptr) BF_HIP(b, hipHostFree(*ptr));
    *ptr = nullptr;
    *have = 0;
    const size_t cap = need + need / 2 + 256;
    BF_HIP(b, hipHostMalloc(ptr, cap, hipHostMallocDefault));
    *have = cap;
    return ICP_OK;
}

icp_batch_frames* frames_of(icp_batch* b) {
    if (!b->frames) b->frames = new icp_batch_frames();
    return b->frames;
}

// the batch over `members` (indices into b->members, ascending): b itself for all of them, an inner batch otherwise
int subset_batch(icp_batch* b, const int32_t* members, int n, icp_batch** out) {
    if (n == (int)b->members.size()) {
        *out = b;
        return ICP_OK;
    }
    icp_batch_frames* s = frames_of(b);
    const uint32_t mask = batch_frame_mask(members, n);
    auto it = s->inner.find(mask);
    if (it != s->inner.end()) {
        it->second.used = ++s->tick;
        *out = it->second.batch;
        return ICP_OK;
    }
    if (s->inner.size() >= icp_batch_frames::INNER_MAX) {
        // (the batches of the step at hand were used last: with INNER_MAX >= 3 they are never the one that goes; nothing of an
        // inner batch is in flight between two steps — its registration is collected, its launches only read its tables, which
        // icp_batch_destroy waits for)
        auto lru = s->inner.begin();
        for (auto k = s->inner.begin(); k != s->inner.end(); ++k)
            if (k->second.used < lru->second.used) lru = k;
        icp_batch_destroy(lru->second.batch);
        s->inner.erase(lru);
    }
    icp_ctx* ctxs[ICP_BATCH_MAX_SEQUENCES];
    for (int i = 0; i < n; ++i) ctxs[i] = b->members[members[i]];
    icp_batch* inner = nullptr;
    const int rc = icp_batch_create(ctxs, n, &inner);
    if (rc) return bf_fail(b, rc, "batched frame: the batch over the members of this step could not be created");
    s->inner[mask] = icp_batch_frames::Inner{inner, ++s->tick};
    *out = inner;
    return ICP_OK;
}

int inner_fail(icp_batch* b, icp_batch* inner, int rc) {
    if (inner != b) b->error = inner->error;
    return rc;
}

// host rows (and timestamps) of the members in `who` -> the pinned arena -> the next device arena, ONE copy on the upload
// stream; the batch's stream waits for it.  rows[] / ts[] receive the device addresses.
int upload(icp_batch* b, icp_batch_frames* s, const icp_batch_frame* frames, const int32_t* who, int n_who, hipStream_t stream,
           const float** rows, const double** ts) {
    size_t offset[ICP_BATCH_MAX_SEQUENCES], ts_offset[ICP_BATCH_MAX_SEQUENCES];
    size_t bytes = 0;
    for (int i = 0; i < n_who; ++i) {
        const icp_batch_frame& fr = frames[who[i]];
        offset[i] = bytes;
        bytes += align_up((size_t)fr.n * 12);
        ts_offset[i] = bytes;
        if (fr.timestamps) bytes += align_up((size_t)fr.n * 8);
    }
    if (bytes == 0) return ICP_OK;
    if (s->pin_in_busy) {  // the previous upload has left the pinned arena (long done in practice)
        BF_HIP(b, hipEventSynchronize(s->pin_in_free));
        s->pin_in_busy = false;
    }
    int rc = pinned_reserve(b, &s->pin_in, &s->pin_in_bytes, bytes);
    if (rc) return rc;
    for (int i = 0; i < n_who; ++i) {
        const icp_batch_frame& fr = frames[who[i]];
        if (fr.n <= 0) continue;
        memcpy((char*)s->pin_in + offset[i], fr.xyz, (size_t)fr.n * 12);
        if (fr.timestamps) memcpy((char*)s->pin_in + ts_offset[i], fr.timestamps, (size_t)fr.n * 8);
    }
    if (!s->upload_stream) BF_HIP(b, hipStreamCreateWithFlags(&s->upload_stream, hipStreamNonBlocking));
    if (!s->pin_in_free) BF_HIP(b, hipEventCreateWithFlags(&s->pin_in_free, hipEventDisableTiming));
    // two device arenas, alternating (as frame_upload's two slots): the DMA does not wait for the batch's stream, so it must not
    // land in memory that work queued there still reads — the last readers of an arena are the launches of the step before
    // last, which the upload stream waits for (arena_read; long finished: the step in between has been collected)
    s->which ^= 1;
    DeviceBuffer& arena = s->arena[s->which];
    if (s->arena_used[s->which]) BF_HIP(b, hipStreamWaitEvent(s->upload_stream, s->arena_read[s->which], 0));
    if (arena.bytes < bytes && s->arena_used[s->which]) BF_HIP(b, hipEventSynchronize(s->arena_read[s->which]));  // (it is freed)
    BF_HIP(b, arena.reserve(bytes));
    BF_HIP(b, hipMemcpyAsync(arena.ptr, s->pin_in, bytes, hipMemcpyHostToDevice, s->upload_stream));
    BF_HIP(b, hipEventRecord(s->pin_in_free, s->upload_stream));
    s->pin_in_busy = true;
    BF_HIP(b, hipStreamWaitEvent(stream, s->pin_in_free, 0));
    for (int i = 0; i < n_who; ++i) {
        const icp_batch_frame& fr = frames[who[i]];
        if (fr.n <= 0) continue;
        rows[who[i]] = (const float*)(arena.as<char>() + offset[i]);
        ts[who[i]] = fr.timestamps ? (const double*)(arena.as<char>() + ts_offset[i]) : nullptr;
    }
    return ICP_OK;
}

// de-skew -> grid sample -> float32 (slam/preprocessing.py:144-191, :207-226, :101-126) of the registering members `reg` (member
// indices; ctxs / ios / guess / have_guess / r_rows / r_n by position k, ts by member index): icp_batch_preprocess on `rb` for
// a step that grid-samples, icp_frame_launch's own two launches for a de-skewed member otherwise.  r_rows[k] becomes what the
// frame goes on with; s->sampled / s->copied are set.
int batch_frames_preprocess(icp_batch* b, icp_batch* rb, icp_batch_frames* s, const char* who, const int32_t* reg, int nr,
                            icp_ctx* const* ctxs, icp_frame_io* const* ios, double voxel_size, const float* const* guess,
                            const bool* have_guess, const double* const* ts, const float** r_rows, const int64_t* r_n) {
    bool skew[ICP_BATCH_MAX_SEQUENCES];
    const bool sample_step = voxel_size > 0;
    for (int k = 0; k < nr; ++k) {
        const int i = reg[k];
        skew[k] = r_n[k] > 0 && ts[i] != nullptr && have_guess[k];
        s->sampled[i] = r_n[k] > 0 && sample_step;
        s->copied[i] = false;
    }
    auto member_hip = [&](int k, hipError_t e, const char* what) { return bf_member_hip(b, who, reg[k], e, what); };
    int rc = ICP_OK;
    for (int k = 0; k < nr && !rc; ++k) {
        icp_frame_io* f = ios[k];
        const size_t n = (size_t)r_n[k];
        if (skew[k]) rc = member_hip(k, f->skew64.reserve(n * 24), "reserve(skew64)");
        if (!rc && (s->sampled[reg[k]] || skew[k])) rc = member_hip(k, f->samp32.reserve(n * 12), "reserve(samp32)");
        if (!rc && s->sampled[reg[k]] && skew[k]) rc = member_hip(k, f->samp64.reserve(n * 24), "reserve(samp64)");
        if (!rc) rc = member_hip(k, f->count.reserve(64), "reserve(count)");
    }
    if (rc) return rc;
    if (sample_step) {
        icp_preprocess_frame pre[ICP_BATCH_MAX_SEQUENCES];
        memset(pre, 0, sizeof(pre));
        for (int k = 0; k < nr; ++k) {
            icp_frame_io* f = ios[k];
            icp_preprocess_frame& p = pre[k];
            p.xyz = r_rows[k];
            p.n = r_n[k];
            p.count_out = f->count.as<int32_t>();
            if (r_n[k] <= 0) continue;
            if (skew[k]) {
                p.timestamps = ts[reg[k]];
                for (int e = 0; e < 16; ++e) p.rel_pose[e] = (double)guess[k][e];
                p.distorted_out = f->skew64.as<double>();
                p.samples_out = f->samp64.as<double>();
            }
            p.samples_f32_out = f->samp32.as<float>();
            r_rows[k] = f->samp32.as<float>();
        }
        if ((rc = icp_batch_preprocess(rb, pre, voxel_size))) return inner_fail(b, rb, rc);
    } else {
        for (int k = 0; k < nr; ++k) {  // (no grid sample: a de-skewed member takes icp_frame_launch's own two launches)
            if (!skew[k]) continue;
            icp_frame_io* f = ios[k];
            double rel[16];
            for (int e = 0; e < 16; ++e) rel[e] = (double)guess[k][e];
            if ((rc = distort_device(ctxs[k], r_rows[k], ts[reg[k]], r_n[k], rel, f->skew64.as<double>())) ||
                (rc = rows_to_f32_device(ctxs[k], f->skew64.as<double>(), 3 * r_n[k], f->samp32.as<float>())))
                return bf_member_fail(b, rc, who, reg[k]);
            r_rows[k] = f->samp32.as<float>();
        }
    }
    for (int k = 0; k < nr; ++k) ios[k]->copy_started = false;
    return ICP_OK;
}

// the copies towards the host, beside the registration: behind the staging, on ONE stream of the batch's own — the staged rows
// of the members with cloud[k] and the sample counts of the sampled ones, into ONE pinned arena
int batch_frames_copy_start(icp_batch* b, icp_batch_frames* s, const int32_t* reg, int nr, icp_ctx* const* ctxs,
                            icp_frame_io* const* ios, const bool* cloud, const int64_t* r_n) {
    size_t bytes = 0;
    bool any = false;
    for (int k = 0; k < nr; ++k) {
        const int i = reg[k];
        s->out_offset[i] = bytes;
        if (cloud[k] && r_n[k] > 0) {
            bytes += align_up((size_t)r_n[k] * 12);
            s->copied[i] = true;
            any = true;
        }
        any = any || s->sampled[i];
    }
    if (!any) return ICP_OK;
    int rc = ICP_OK;
    if (!s->copy_stream) rc = bf_hip(b, hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking), "hipStreamCreate(copy)");
    if (!rc && !s->copy_done) rc = bf_hip(b, hipEventCreateWithFlags(&s->copy_done, hipEventDisableTiming), "hipEventCreate(copy)");
    if (!rc && !s->pin_counts)
        rc = bf_hip(b, hipHostMalloc((void**)&s->pin_counts, sizeof(int) * ICP_BATCH_MAX_SEQUENCES, hipHostMallocDefault),
                    "hipHostMalloc(counts)");
    if (!rc && bytes > 0) rc = pinned_reserve(b, &s->pin_out, &s->pin_out_bytes, bytes);
    // (the members' staging events are recorded one behind the other on the batch's stream: the last one covers all)
    if (!rc) rc = bf_hip(b, hipStreamWaitEvent(s->copy_stream, ctxs[nr - 1]->staged_event, 0), "hipStreamWaitEvent(staged)");
    for (int k = 0; k < nr && !rc; ++k) {
        const int i = reg[k];
        if (s->sampled[i])
            rc = bf_hip(b, hipMemcpyAsync(&s->pin_counts[i], ios[k]->count.ptr, sizeof(int), hipMemcpyDeviceToHost, s->copy_stream),
                        "hipMemcpyAsync(count)");
        if (!rc && s->copied[i])
            rc = bf_hip(b, hipMemcpyAsync((char*)s->pin_out + s->out_offset[i], ctxs[k]->staged_xyz.ptr, (size_t)r_n[k] * 12,
                                          hipMemcpyDeviceToHost, s->copy_stream),
                        "hipMemcpyAsync(odometry_pc)");
    }
    if (!rc) rc = bf_hip(b, hipEventRecord(s->copy_done, s->copy_stream), "hipEventRecord(copy_done)");
    if (rc) {
        if (s->copy_stream) (void)hipStreamSynchronize(s->copy_stream);
        return rc;
    }
    s->copy_started = true;
    return ICP_OK;
}

// what reads the device arena of this step's upload is on the stream: the upload of the step after next waits for it
int batch_frames_arena_read(icp_batch* b, icp_batch_frames* s, hipStream_t stream) {
    hipEvent_t& e = s->arena_read[s->which];
    if (!e) BF_HIP(b, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    BF_HIP(b, hipEventRecord(e, stream));
    s->arena_used[s->which] = true;
    return ICP_OK;
}

void batch_frames_init_poses(const float* const* guess, const bool* have_guess, int n, float* init) {
    for (int k = 0; k < n; ++k) {
        if (have_guess[k]) memcpy(init + 16 * k, guess[k], 16 * sizeof(float));
        else pose_identity(init + 16 * k);
    }
}

void batch_frames_drop_pending(icp_batch* b, const BatchFrameKind* only) {
    icp_batch_frames* s = b ? b->frames : nullptr;
    if (!s || !s->pending || (only && s->pending != only)) return;
    const BatchFrameKind& kind = *s->pending;
    const BatchFrameStep& p = s->step;
    if (p.n_registering > 0) {
        icp_batch* rb = nullptr;
        if (subset_batch(b, p.registering, p.n_registering, &rb) == ICP_OK) {
            icp_register_result regs[ICP_BATCH_MAX_SEQUENCES];
            (void)icp_batch_register_end(rb, regs, nullptr, nullptr);
        }
    }
    if (s->copy_started) (void)hipEventSynchronize(s->copy_done);
    s->copy_started = false;
    for (int i = 0; i < p.n_registering; ++i) {
        icp_ctx* ctx = b->members[p.registering[i]];
        icp_frame_seq* f = kind.loop(ctx).seq;
        if (!f || !f->batched) continue;
        f->launched = f->registered = f->batched = false;
        if (kind.forget_pose) kind.forget_pose(ctx);
    }
    for (int i = 0; i < p.n_first; ++i) {
        icp_frame_seq* f = kind.loop(b->members[p.first[i]]).seq;
        if (f && f->batched) f->launched = f->registered = f->batched = false;
    }
    s->pending = nullptr;
}

void batch_frames_release(icp_batch* b) {
    icp_batch_frames* s = b ? b->frames : nullptr;
    if (!s) return;
    batch_frames_drop_pending(b);
    (void)hipDeviceSynchronize();
    for (auto& kv : s->inner) icp_batch_destroy(kv.second.batch);
    s->arena[0].release();
    s->arena[1].release();
    if (s->pin_in) (void)hipHostFree(s->pin_in);
    if (s->pin_out) (void)hipHostFree(s->pin_out);
    if (s->pin_counts) (void)hipHostFree(s->pin_counts);
    if (s->pin_in_free) (void)hipEventDestroy(s->pin_in_free);
    if (s->copy_done) (void)hipEventDestroy(s->copy_done);
    for (auto& e : s->arena_read)
        if (e) (void)hipEventDestroy(e);
    if (s->upload_stream) (void)hipStreamDestroy(s->upload_stream);
    if (s->copy_stream) (void)hipStreamDestroy(s->copy_stream);
    delete s;
    b->frames = nullptr;
}

void batch_frames_end_first(icp_batch* b, const BatchFrameKind& kind, const BatchFrameStep& step, int upto) {
    for (int k = 0; k < upto; ++k) {
        icp_frame_result dropped;
        icp_ctx* ctx = b->members[step.first[k]];
        kind.loop(ctx).seq->batched = false;
        (void)kind.single_end(ctx, &dropped, nullptr, 0, nullptr, ICP_MEM_HOST, nullptr, nullptr);
    }
}

int batch_frames_launch_begin(icp_batch* b, const BatchFrameKind& kind, const BatchFrameStep& step, const icp_batch_frame* frames,
                              int mem, int layout, BatchFrameLaunch* l) {
    icp_batch_frames* s = frames_of(b);
    const int count = (int)b->members.size();
    int rc = ICP_OK;
    if (step.n_registering > 0 && (rc = subset_batch(b, step.registering, step.n_registering, &l->rb))) return rc;
    l->lead = b->members[step.n_registering > 0 ? step.registering[0] : step.first[0]];
    l->stream = l->lead->stream;
    // ---- input: one upload for every member that takes part
    int32_t active[ICP_BATCH_MAX_SEQUENCES];
    int n_active = 0;
    for (int i = 0; i < count; ++i) {
        if (frames[i].skip) continue;
        active[n_active++] = i;
        l->rows[i] = frames[i].xyz;
        l->ts[i] = frames[i].timestamps;
        s->n[i] = frames[i].n;
    }
    if (mem == ICP_MEM_HOST) {
        if ((rc = upload(b, s, frames, active, n_active, l->stream, l->rows, l->ts))) return rc;
        l->uploaded = true;
    }
    s->mem = mem;
    // ---- first frames: the single launch's frame 0, member by member (the rows are on the device by now)
    for (int k = 0; k < step.n_first; ++k) {
        const int i = step.first[k];
        if ((rc = kind.first_launch(b->members[i], l->rows[i], frames[i].n, layout, frames[i].n > 0 ? l->ts[i] : nullptr,
                                    frames[i].init_pose))) {
            batch_frames_end_first(b, kind, step, k);  // (their maps hold frame 0)
            return bf_member_fail(b, rc, kind.launch_name, i);
        }
    }
    s->copy_started = false;
    return ICP_OK;
}

int batch_frames_launch_finish(icp_batch* b, const BatchFrameKind& kind, const BatchFrameStep& step, const BatchFrameLaunch& l) {
    icp_batch_frames* s = frames_of(b);
    int rc;
    for (int k = 0; k < step.n_first; ++k) kind.loop(b->members[step.first[k]]).seq->batched = true;
    if (l.uploaded && (rc = batch_frames_arena_read(b, s, l.stream))) return rc;
    s->step = step;
    s->pending = &kind;
    return ICP_OK;
}

int batch_frames_end(icp_batch* b, const BatchFrameKind& kind, icp_frame_result* results, float* const* odometry_pc_out,
                     const int64_t* cap, int64_t* rows_out, int out_mem, double* loss_per_iter_out, float* dx_per_iter_out) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    const std::string who = kind.end_name;
    if (!results) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, who + ": results[] is required (nothing was changed)");
    DeviceGuard device_guard(b->device);
    icp_batch_frames* s = b->frames;
    if (const char* reason = kind.end_refusal(s && s->pending == &kind))
        return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, who + ": " + reason + " (nothing was changed)");
    const int count = (int)b->members.size();
    if (odometry_pc_out && !cap) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, who + ": odometry_pc_out needs cap[] (nothing was changed)");
    if (odometry_pc_out)
        for (int i = 0; i < count; ++i)
            if (odometry_pc_out[i] && cap[i] < 0) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, who + ": negative capacity (nothing was changed)");
    const BatchFrameStep step = s->step;
    for (int i = 0; i < count; ++i) {
        memset(&results[i], 0, sizeof(results[i]));
        results[i].frame_index = -1;  // (a skipped member's stays so)
        if (rows_out) rows_out[i] = 0;
    }
    int rc;
    // ---- first frames: the identity, the vertex map is in the map (the single end call's frame 0)
    for (int k = 0; k < step.n_first; ++k) {
        const int i = step.first[k];
        icp_ctx* ctx = b->members[i];
        kind.loop(ctx).seq->batched = false;
        if ((rc = kind.single_end(ctx, &results[i], nullptr, 0, nullptr, out_mem, nullptr, nullptr))) {
            // (the step is given up: the registrations are collected and dropped, no member stays launched by the batch)
            const std::string why = ctx->error;
            batch_frames_drop_pending(b);
            return bf_fail(b, rc, who + ", member " + std::to_string(i) + ": " + why);
        }
    }
    const int nr = step.n_registering;
    icp_batch* rb = nullptr;
    if (nr > 0 && (rc = subset_batch(b, step.registering, nr, &rb))) {
        const std::string why = b->error;
        batch_frames_drop_pending(b);  // (as above; with no batch to collect them through, the members' registrations stay theirs to end)
        return bf_fail(b, rc, why);
    }
    s->pending = nullptr;  // from here on the step is ended whatever happens: every member's flags are cleared below
    if (nr == 0) return ICP_OK;
    icp_ctx* ctxs[ICP_BATCH_MAX_SEQUENCES];
    for (int k = 0; k < nr; ++k) ctxs[k] = b->members[step.registering[k]];
    // ---- the registrations: ONE wait for all of them
    const size_t hist = (size_t)ctxs[0]->cfg.max_num_alignments;            // (the registering members share it)
    const size_t stride = (size_t)b->members[0]->cfg.max_num_alignments;    // (the layout of icp_batch_register_end over ALL members)
    std::vector<double> losses(loss_per_iter_out ? hist * nr : 0);
    std::vector<float> dxs(dx_per_iter_out ? hist * nr * 6 : 0);
    icp_register_result regs[ICP_BATCH_MAX_SEQUENCES];
    memset(regs, 0, sizeof(regs));
    const int rc_reg = icp_batch_register_end(rb, regs, loss_per_iter_out ? losses.data() : nullptr, dx_per_iter_out ? dxs.data() : nullptr);
    if (rc_reg && rb != b) b->error = rb->error;
    int rc_copy = ICP_OK;
    if (s->copy_started) rc_copy = bf_hip(b, hipEventSynchronize(s->copy_done), "hipEventSynchronize(copy_done)");
    s->copy_started = false;
    int32_t statuses[ICP_BATCH_MAX_SEQUENCES], update[ICP_BATCH_MAX_SEQUENCES], first_status = 0;
    for (int k = 0; k < nr; ++k) {
        const int i = step.registering[k];
        icp_frame_seq* f = kind.loop(ctxs[k]).seq;
        statuses[k] = rc_reg ? regs[k].status : ICP_OK;
        results[i].reg = regs[k];
        results[i].frame_index = f->index;
        results[i].samples = s->sampled[i] ? (int64_t)s->pin_counts[i] : f->n;
        const size_t its = (size_t)std::max(0, std::min(regs[k].iterations, (int)std::min(hist, stride)));
        if (loss_per_iter_out) memcpy(loss_per_iter_out + (size_t)i * stride, losses.data() + (size_t)k * hist, its * sizeof(double));
        if (dx_per_iter_out) memcpy(dx_per_iter_out + (size_t)i * stride * 6, dxs.data() + (size_t)k * hist * 6, its * 6 * sizeof(float));
        f->launched = f->registered = f->batched = false;
        kind.loop(ctxs[k]).io->copy_started = false;
        // the reference raises before it touches the map (:286): nothing of the sequence moves
        if (statuses[k] && kind.forget_pose) kind.forget_pose(ctxs[k]);
    }
    if (rc_copy) return rc_copy;
    const int nu = batch_frame_update_members(step.registering, statuses, nr, update, &first_status);
    if (rc_reg && !first_status) return rc_reg;  // (a failure of the call itself, not of a member's registration)
    // ---- __update_map (:360-380) for the members that registered: the key-frame tests, then ONE batched update
    if (nu > 0) {
        icp_batch* ub = nullptr;
        if ((rc = subset_batch(b, update, nu, &ub))) return rc;
        icp_ctx* uctx[ICP_BATCH_MAX_SEQUENCES];
        float rel[16 * ICP_BATCH_MAX_SEQUENCES];
        int64_t inserted[ICP_BATCH_MAX_SEQUENCES] = {};
        KeyFrameTest tests[ICP_BATCH_MAX_SEQUENCES];
        for (int u = 0; u < nu; ++u) {
            uctx[u] = b->members[update[u]];
            const BatchFrameMemberLoop l = kind.loop(uctx[u]);
            tests[u] = key_frame_test(l.seq->delta, results[update[u]].reg.pose, l.threshold_trans, l.threshold_rot);
            memcpy(rel + 16 * u, results[update[u]].reg.pose, 16 * sizeof(float));
        }
        if ((rc = kind.update(ub, uctx, nu, rel, tests, inserted))) return inner_fail(b, ub, rc);
        for (int u = 0; u < nu; ++u) {
            icp_frame_result& r = results[update[u]];
            r.key_frame = tests[u].key_frame;
            r.inserted = inserted[u];
            frame_advance(kind.loop(uctx[u]).seq, tests[u], r.reg.pose);
        }
    }
    // ---- odometry_pc (:210-213, :243): the valid rows the staging compacted, in order
    int rc_cap = ICP_OK;
    bool wait_stream = false;
    for (int u = 0; u < nu; ++u) {
        const int i = update[u];
        icp_ctx* ctx = b->members[i];
        const int64_t valid = s->n[i] > 0 ? (int64_t)*ctx->staged_count_host : 0;
        if (rows_out) rows_out[i] = valid;
        float* out = odometry_pc_out ? odometry_pc_out[i] : nullptr;
        if (!out) continue;
        if (valid > cap[i]) {
            if (!rc_cap)
                rc_cap = bf_fail(b, ICP_ERR_INVALID_ARGUMENT, who + ", member " + std::to_string(i) +
                                                                  ": odometry_pc_out holds fewer rows than the frame has (count in rows_out)");
            continue;
        }
        if (valid <= 0) continue;
        if (out_mem == ICP_MEM_HOST && s->copied[i]) {
            memcpy(out, (char*)s->pin_out + s->out_offset[i], (size_t)valid * 12);
        } else {
            // (not copied ahead, or a device buffer: behind the map update just enqueued, which reads the staged rows and leaves
            // them as they are)
            BF_HIP(b, hipMemcpyAsync(out, ctx->staged_xyz.ptr, (size_t)valid * 12,
                                     out_mem == ICP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
            wait_stream = wait_stream || out_mem == ICP_MEM_HOST;
        }
    }
    if (wait_stream) BF_HIP(b, hipStreamSynchronize(ctxs[0]->stream));
    if (first_status) {
        if (rb == b || !b->error.empty()) return first_status;
        return bf_fail(b, first_status, who + ": a member's registration failed (results[b].reg.status)");
    }
    return rc_cap;
}

}  // namespace icp

// ---- the kd-tree form
namespace {

void fill_members(icp_batch* b, const icp_batch_frame* frames, BatchFrameMember* out) {
    for (size_t i = 0; i < b->members.size(); ++i) {
        const icp_ctx* ctx = b->members[i];
        const icp_frame_loop* f = ctx->frame;
        BatchFrameMember& m = out[i];
        memset(&m, 0, sizeof(m));
        m.skip = frames[i].skip != 0;
        m.has_sequence = f != nullptr;
        m.frame_index = f ? f->seq.index : 0;
        m.voxel_size = f ? f->cfg.voxel_size : 0.0;
        m.targets = f ? f->cfg.targets : 0;
        m.point_to_point = ctx->cost != ICP_COST_POINT_TO_PLANE;
        m.projective_map = !ctx->pm_slots.empty();
        m.exchange = ctx->exchange_on;
        m.profiling = ctx->prof.enabled != 0;
        m.registering = ctx->in_registration || ctx->result_pending() || ctx->batch_hold;
        m.frame_launched = f && f->seq.launched;
        m.stream = (uint64_t)(uintptr_t)ctx->stream;
    }
}

int kd_first_launch(icp_ctx* ctx, const float* rows, int64_t n, int, const double* ts, const float init_pose[16]) {
    return frame_launch_device(ctx, rows, n, ts, init_pose);
}

// ONE icp_batch_map_update_staged: the key frames insert their staged cloud, the others move their map
int kd_update(icp_batch* ub, icp_ctx* const*, int nu, const float* rel, const KeyFrameTest* tests, int64_t* inserted) {
    int32_t insert[ICP_BATCH_MAX_SEQUENCES];
    for (int u = 0; u < nu; ++u) insert[u] = tests[u].key_frame;
    const int rc = icp_batch_map_update_staged(ub, rel, insert, inserted);
    for (int u = 0; u < nu && !rc; ++u)
        if (!tests[u].key_frame) inserted[u] = 0;
    return rc;
}

}  // namespace

namespace icp {

const BatchFrameKind& batch_frame_kd() {
    static const BatchFrameKind kind = {
        "icp_batch_frame_launch",
        "icp_batch_frame_end",
        [](icp_ctx* ctx) {
            icp_frame_loop* f = ctx->frame;
            return f ? BatchFrameMemberLoop{&f->seq, &f->io, f->cfg.threshold_trans, f->cfg.threshold_rot} : BatchFrameMemberLoop{};
        },
        [](icp_ctx* ctx) { ctx->frame->pose_epoch = -1; },
        kd_first_launch,
        icp_frame_end,
        kd_update,
        batch_frame_end_refusal,
    };
    return kind;
}

}  // namespace icp

extern "C" {

int icp_batch_odometry_init(icp_batch* b, const icp_frame_config* cfg) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!cfg) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_odometry_init: a configuration is required");
    DeviceGuard device_guard(b->device);
    // ---- every member is checked before any member changes (a member whose frame THIS batch has launched is fine: the step is dropped below)
    for (size_t i = 0; i < b->members.size(); ++i) {
        const int rc = frame_init_check(b->members[i], cfg, b->frames != nullptr && b->frames->pending == &batch_frame_kd());
        if (rc) return bf_member_fail(b, rc, "icp_batch_odometry_init (nothing was changed)", (int)i);
    }
    batch_frames_drop_pending(b, &batch_frame_kd());  // (as icp_odometry_init: a step launched and not ended is collected and dropped)
    for (size_t i = 0; i < b->members.size(); ++i) {
        const int rc = icp_odometry_init(b->members[i], cfg);
        if (rc) return bf_member_fail(b, rc, "icp_batch_odometry_init", (int)i);
    }
    return ICP_OK;
}

int icp_batch_frame_launch(icp_batch* b, const icp_batch_frame* frames, int mem) {
    if (!b) return ICP_ERR_INVALID_ARGUMENT;
    if (!frames || (mem != ICP_MEM_HOST && mem != ICP_MEM_DEVICE))
        return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_frame_launch: frames[] in host or device memory are required");
    DeviceGuard device_guard(b->device);
    icp_batch_frames* s = frames_of(b);
    const int count = (int)b->members.size();
    // ---- every member is looked at before any member changes
    BatchFrameMember members[ICP_BATCH_MAX_SEQUENCES];
    fill_members(b, frames, members);
    BatchFramePlan plan;
    // (one pending step per batch: a projective one is ended first, as batch_pmap_frame.hip refuses a pending kd-tree one)
    if (s->pending == &batch_frame_pmap()) return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_frame_launch: a projective step of this batch awaits icp_batch_pmap_frame_end (nothing was changed)");
    if (!batch_frame_plan(members, count, s->pending == &batch_frame_kd(), &plan)) return batch_frames_refuse(b, "icp_batch_frame_launch", plan);
    for (int i = 0; i < count; ++i) {
        const icp_batch_frame& fr = frames[i];
        if (!fr.skip && (fr.n < 0 || fr.n > INT32_MAX || (fr.n > 0 && !fr.xyz)))
            return bf_fail(b, ICP_ERR_INVALID_ARGUMENT, "icp_batch_frame_launch, member " + std::to_string(i) +
                                                            ": [n,3] rows in host or device memory are required (nothing was changed)");
    }
    const BatchFrameStep step = batch_frame_step(plan);
    BatchFrameLaunch l;
    int rc = batch_frames_launch_begin(b, batch_frame_kd(), step, frames, mem, ICP_FRAME_ROWS, &l);
    if (rc) return rc;
    icp_batch* rb = l.rb;
    // a failure behind the first frames: those frames are complete, their members have advanced
    auto give_up = [&](int code) {
        batch_frames_end_first(b, batch_frame_kd(), step, step.n_first);
        return code;
    };
    const int nr = step.n_registering;
    if (nr > 0) {
        // ---- the registering members, in icp_frame_launch's order, one call per stage
        icp_ctx* ctxs[ICP_BATCH_MAX_SEQUENCES];
        icp_frame_loop* loops[ICP_BATCH_MAX_SEQUENCES];
        icp_frame_io* ios[ICP_BATCH_MAX_SEQUENCES];
        const float* r_rows[ICP_BATCH_MAX_SEQUENCES];
        int64_t r_n[ICP_BATCH_MAX_SEQUENCES];
        const float* guess[ICP_BATCH_MAX_SEQUENCES];
        bool have_guess[ICP_BATCH_MAX_SEQUENCES];
        const icp_frame_config& c0 = b->members[step.registering[0]]->frame->cfg;
        for (int k = 0; k < nr; ++k) {
            const int i = step.registering[k];
            ctxs[k] = b->members[i];
            loops[k] = ctxs[k]->frame;
            ios[k] = &loops[k]->io;
            const icp_batch_frame& fr = frames[i];
            r_n[k] = fr.n;
            r_rows[k] = fr.n > 0 ? l.rows[i] : nullptr;
            // the initial guess (ConstantVelocityInitialization, slam/initialization.py:103-119): icp_frame_launch's rule
            have_guess[k] = fr.init_pose != nullptr || loops[k]->cfg.constant_velocity != 0;
            guess[k] = fr.init_pose ? fr.init_pose : loops[k]->seq.last_pose;
        }
        auto member_hip = [&](int k, hipError_t e, const char* what) {
            return bf_member_hip(b, "icp_batch_frame_launch", step.registering[k], e, what);
        };
        // ---- de-skew -> grid sample -> float32 (slam/preprocessing.py:144-191, :207-226, :101-126)
        if ((rc = batch_frames_preprocess(b, rb, s, "icp_batch_frame_launch", step.registering, nr, ctxs, ios, c0.voxel_size, guess,
                                          have_guess, l.ts, r_rows, r_n)))
            return give_up(rc);
        for (int k = 0; k < nr; ++k) {
            loops[k]->frame_rows = r_rows[k];
            loops[k]->seq.n = r_n[k];
            loops[k]->seq.sampled = s->sampled[step.registering[k]];
        }
        // ---- projection (targets = 1), staging, copy-out, registration — the plugin's order
        const float* targets[ICP_BATCH_MAX_SEQUENCES];
        int64_t n_targets[ICP_BATCH_MAX_SEQUENCES];
        int target_mode = ICP_TARGETS_ALL;
        for (int k = 0; k < nr; ++k) {
            targets[k] = r_rows[k];
            n_targets[k] = r_n[k];
        }
        if (c0.targets == 1) {
            float* vmaps[ICP_BATCH_MAX_SEQUENCES];
            float* pix[ICP_BATCH_MAX_SEQUENCES];
            rc = ICP_OK;
            for (int k = 0; k < nr && !rc; ++k) {
                const size_t npix = (size_t)ctxs[k]->cfg.height * ctxs[k]->cfg.width;
                rc = member_hip(k, ios[k]->vmap.reserve(npix * 12), "reserve(vmap)");
                if (!rc) rc = member_hip(k, ios[k]->rows.reserve(npix * 12), "reserve(rows)");
                vmaps[k] = ios[k]->vmap.as<float>();
                pix[k] = ios[k]->rows.as<float>();
                targets[k] = pix[k];
                n_targets[k] = (int64_t)npix;
            }
            if (rc) return give_up(rc);
            if ((rc = icp_batch_project_rows(rb, r_rows, r_n, vmaps, pix))) return give_up(inner_fail(b, rb, rc));
            target_mode = ICP_TARGETS_SKIP_NULL;
        }
        // (the batched form always stages: icp_batch_map_update_staged takes staged clouds only)
        if ((rc = icp_batch_stage(rb, r_rows, r_n, ICP_TARGETS_ALL))) return give_up(inner_fail(b, rb, rc));
        for (int k = 0; k < nr; ++k) loops[k]->seq.staged = true;
        // ---- the copies towards the host, beside the registration: behind the staging, on ONE stream of the batch's own
        bool cloud[ICP_BATCH_MAX_SEQUENCES];
        for (int k = 0; k < nr; ++k) cloud[k] = loops[k]->cfg.copy_cloud != 0;
        if ((rc = batch_frames_copy_start(b, s, step.registering, nr, ctxs, ios, cloud, r_n))) return give_up(rc);
        // ---- the registration: from the device-resident poses when every member would do so on its own, the host guesses otherwise
        bool from_last = true;
        for (int k = 0; k < nr; ++k) {
            const icp_frame_loop* f = loops[k];
            from_last = from_last && f->cfg.constant_velocity != 0 && !frames[step.registering[k]].init_pose && f->seq.index >= 2 &&
                        ctxs[k]->have_device_pose && f->pose_epoch == ctxs[k]->device_pose_epoch;
        }
        float init[16 * ICP_BATCH_MAX_SEQUENCES];
        batch_frames_init_poses(guess, have_guess, nr, init);
        rc = icp_batch_register_launch(rb, targets, n_targets, ICP_MEM_DEVICE, target_mode, from_last ? nullptr : init, from_last ? 1 : 0);
        if (rc) {
            if (s->copy_started) (void)hipEventSynchronize(s->copy_done);
            s->copy_started = false;
            return give_up(inner_fail(b, rb, rc));
        }
        for (int k = 0; k < nr; ++k) {
            icp_frame_loop* f = loops[k];
            f->pose_epoch = ctxs[k]->device_pose_epoch;
            f->seq.launched = f->seq.registered = f->seq.batched = true;
        }
    }
    return batch_frames_launch_finish(b, batch_frame_kd(), step, l);
}

int icp_batch_frame_end(icp_batch* b, icp_frame_result* results, float* const* odometry_pc_out, const int64_t* cap,
                        int64_t* rows_out, int out_mem, double* loss_per_iter_out, float* dx_per_iter_out) {
    return batch_frames_end(b, batch_frame_kd(), results, odometry_pc_out, cap, rows_out, out_mem, loss_per_iter_out, dx_per_iter_out);
}

}  // extern "C"
