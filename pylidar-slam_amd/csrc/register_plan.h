// How many iterations the first chunk of a launched registration holds, and where the descriptor tables of a batched
// registration lie in their pinned slot: plain C++ without a HIP dependency, so that it also builds into a stand-alone
// program under the host sanitizers (tests/native/register_plan_check.cpp).  register.hip and batch.hip call it.
#pragma once
#include <stddef.h>

namespace icp {

// a descriptor table begins on a 256-byte boundary of its slot
inline size_t pad256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// Forced iteration count (threshold <= 0), "chunked_launch" off, or a resident tail planned (it runs to the end of the loop
// on the device): every iteration is enqueued.  Otherwise as many as the slowest member ran last time — a member without a
// collected registration (0) counts as 3 — plus one, at most all: icp_register_end / icp_batch_register_end enqueue further
// chunks while the loop is still running (launches behind an early stop would see `done` and return at once, but each
// still costs its slot on the stream)
inline int first_chunk_iterations(int iters, float threshold, int chunked_launch, bool tail_planned, const int* last_iterations,
                                  int count) {
    if (!(threshold > 0.f) || !chunked_launch || tail_planned) return iters;
    int most = 0;
    for (int i = 0; i < count; ++i) {
        const int ran = last_iterations[i] > 0 ? last_iterations[i] : 3;
        if (ran > most) most = ran;
    }
    return most + 1 < iters ? most + 1 : iters;
}

// One chunk of a batched kd-tree registration: [packs | then, per iteration of the chunk, its iterate table and — where a
// summing / solving launch follows it — its sum + solve table].  Only the packing table is padded; `need` has room for a
// solving launch behind every iteration.
struct BatchRegisterLayout {
    size_t pack_bytes, it_bytes, ss_bytes;
    BatchRegisterLayout(size_t pack_desc, size_t iterate_desc, size_t sum_solve_desc, int count)
        : pack_bytes(pad256(pack_desc * (size_t)count)), it_bytes(iterate_desc * (size_t)count),
          ss_bytes(sum_solve_desc * (size_t)count) {}
    size_t first_table() const { return pack_bytes; }
    size_t need(int chunk) const { return pack_bytes + (size_t)chunk * (it_bytes + ss_bytes); }
};

// A batched projective registration: [packs | registrations | sum + solve | sum + solve of the last iteration], each padded
struct BatchPmapRegisterLayout {
    size_t pack_bytes, reg_bytes, ss_bytes;
    BatchPmapRegisterLayout(size_t pack_desc, size_t reg_desc, size_t sum_solve_desc, int count)
        : pack_bytes(pad256(pack_desc * (size_t)count)), reg_bytes(pad256(reg_desc * (size_t)count)),
          ss_bytes(pad256(sum_solve_desc * (size_t)count)) {}
    size_t registrations() const { return pack_bytes; }
    size_t sum_solve(bool last_iteration) const { return pack_bytes + reg_bytes + (last_iteration ? ss_bytes : 0); }
    size_t need() const { return pack_bytes + reg_bytes + 2 * ss_bytes; }
};

}  // namespace icp
