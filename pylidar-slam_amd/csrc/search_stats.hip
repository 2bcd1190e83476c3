// The developer's dump of option "search_stats" (icp_set_option): what the search kernels counted and stamped during the
// registration icp_register_end has just collected, formatted to stderr, and the counters cleared for the next one.  Host
// code only.  The format is compared by eye against old profiles: leave it as it is.
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "icp_internal.h"

using namespace icp;

void search_stats_report(icp_ctx* ctx, const RegState& st) {
    if (ctx->search_stats) {
        std::vector<char> raw(DBG_BYTES);
        if (hipMemcpy(raw.data(), ctx->dbg_counts.ptr, DBG_BYTES, hipMemcpyDeviceToHost) == hipSuccess) {
            const int* c = (const int*)raw.data();
            fprintf(stderr, "[icp stats] N=%lld M=%lld h=%.3f iters=%d ring1=%d need_ring2=%d need_ring3=%d fine_failed=%d exhaustive=%d own_empty=%d misses=%d by-iteration(0-2,3-5,..)=%d,%d,%d,%d,%d,%d,%d knn: beyond ring 1 %d, beyond the fine rings %d\n",
                    (long long)ctx->tgt_n, (long long)ctx->map_m, ctx->cell_h, st.iter, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[8], c[9], c[10], c[11], c[12], c[13], c[14], c[7], c[15]);
            // phase timestamps per iteration launch (100 MHz wall clock -> us)
            const long long* tall = (const long long*)(c + 16);
            const int nb = (int)((ctx->tgt_n * 4 + 511) / 512);
            for (int it = 0; it < st.iter && it < 24 && nb > 0 && nb <= 1024; ++it) {
                const long long* t = tall + 4 * (size_t)it * 1024;
                if (t[0] == 0) continue;
                const long long MASK = (1ll << 48) - 1;
                long long first = t[0], last_start = t[0], last_end = t[3];
                double a = 0, b = 0, r = 0, amax = 0, bmax = 0, rmax = 0;
                int bmax_miss = 0, with_miss = 0, total_miss = 0, b_over2 = 0, b_over5 = 0;
                int seen = 0;
                first &= MASK, last_start &= MASK, last_end &= MASK;
                // (search_stats = 1: the top 16 bits of stamps 0 / 2 / 3 carry the workgroup's queries that went to the
                // coarse level / beyond ring 1 / found their own cell empty)
                struct Blk { double b; int miss, ring2, empty, coarse; };
                std::vector<Blk> blks;
                for (int i = 0; i < nb; ++i) {
                    const long long* q = t + 4 * i;
                    if (q[0] == 0) continue;  // the 512-queries-per-block shape launches a quarter of the blocks
                    if ((q[3] & MASK) == 0) continue;  // (slot 1023 of a lead launch: the LEAD's three stamps, no end stamp — not a workgroup of the iteration)
                    ++seen;
                    const long long t0 = q[0] & MASK, t1 = q[1] & MASK, t2 = q[2] & MASK, t3 = q[3] & MASK;
                    const int miss = (int)(q[1] >> 48);
                    if (t0 < first) first = t0;
                    if (t0 > last_start) last_start = t0;
                    if (t3 > last_end) last_end = t3;
                    const double da = (t1 - t0) * 0.01, db = (t2 - t1) * 0.01, dr = (t3 - t2) * 0.01;
                    blks.push_back(Blk{db, miss, (int)(q[2] >> 48), (int)(q[3] >> 48), (int)(q[0] >> 48)});
                    a += da; b += db; r += dr;
                    if (da > amax) amax = da;
                    if (db > bmax) { bmax = db; bmax_miss = miss; }
                    if (dr > rmax) rmax = dr;
                    with_miss += miss > 0;
                    total_miss += miss;
                    b_over2 += db > 2.0;
                    b_over5 += db > 5.0;
                }
                if (seen < 1023 && t[4 * 1023] != 0) {  // (the lead's stamps carry no counters)  // the lead workgroup of a lead launch left its stamps in slot 1023
                    const long long* q = t + 4 * 1023;
                    fprintf(stderr, "[icp lead] it %2d: starts %.2f us after the first workgroup; rows summed after %.2f, solved "
                                    "and published after %.2f more\n",
                            it, (q[0] - first) * 0.01, (q[1] - q[0]) * 0.01, (q[2] - q[1]) * 0.01);
                }
                if (it < 4 && ctx->search_stats_blocks) {  // dev ("search_stats" 3 | 4): the search phase of every workgroup, by logical block
                    fprintf(stderr, "[icp blocks] it %d:", it);
                    for (int i = 0; i < nb; ++i) {
                        const long long* q = t + 4 * i;
                        if (q[0] == 0) continue;
                        fprintf(stderr, " %d:%lld:%lld:%lld:%d:%d:%d:%d", i, ((q[1] & MASK) - (q[0] & MASK)),
                                ((q[2] & MASK) - (q[1] & MASK)), ((q[3] & MASK) - (q[2] & MASK)), (int)(q[1] >> 48),
                                (int)(q[2] >> 48), (int)(q[3] >> 48), (int)(q[0] >> 48));
                    }
                    fprintf(stderr, "\n");
                }
                fprintf(stderr, "[icp phases] it %2d: start skew %.2f, span %.2f us; A mean %.2f max %.2f; B mean %.2f max %.2f (that block: %d misses), blocks with B > 2 us: %d, > 5 us: %d; misses %d in %d blocks; reduce mean %.2f max %.2f\n",
                        it, (last_start - first) * 0.01, (last_end - first) * 0.01, a / seen, amax, b / seen, bmax, bmax_miss,
                        b_over2, b_over5, total_miss, with_miss, r / seen, rmax);
                if (ctx->search_stats == 1 && it < 8 && blks.size() >= 16) {
                    // what the slow workgroups have that the others do not: deciles of the search phase
                    std::sort(blks.begin(), blks.end(), [](const Blk& x, const Blk& y) { return x.b < y.b; });
                    const size_t nbk = blks.size();
                    fprintf(stderr, "[icp deciles] it %2d (B us: misses / beyond ring 1 / own cell empty / coarse, means):", it);
                    for (int d = 0; d < 10; ++d) {
                        const size_t lo = nbk * d / 10, hi = nbk * (d + 1) / 10;
                        double sb = 0, sm = 0, s2 = 0, se = 0, sc = 0;
                        for (size_t i = lo; i < hi; ++i) {
                            sb += blks[i].b; sm += blks[i].miss; s2 += blks[i].ring2; se += blks[i].empty; sc += blks[i].coarse;
                        }
                        const double k = (double)(hi - lo);
                        fprintf(stderr, " %.1f: %.0f/%.1f/%.1f/%.1f", sb / k, sm / k, s2 / k, se / k, sc / k);
                    }
                    fprintf(stderr, "\n");
                }
            }
            {   // eager normal estimation: 4 stamps per block (start, ring 1 done, stragglers done, eigen done)
                const long long* t = (const long long*)(raw.data() + DBG_ITER_BYTES);
                const int nb = (int)((ctx->map_m + 63) / 64);
                if (nb > 0 && nb <= 8192 && t[0] != 0) {
                    long long first = t[0], last_end = t[3];
                    double a = 0, b = 0, e = 0, amax = 0, bmax = 0;
                    int hist[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                    for (int i = 0; i < nb; ++i) {
                        const long long* q = t + 4 * i;
                        if (q[0] < first) first = q[0];
                        if (q[3] > last_end) last_end = q[3];
                        const double da = (q[1] - q[0]) * 0.01, db = (q[2] - q[1]) * 0.01, de = (q[3] - q[2]) * 0.01;
                        a += da; b += db; e += de;
                        if (da > amax) amax = da;
                        if (db > bmax) bmax = db;
                        int bin = (int)((q[3] - q[0]) * 0.01 / 10.0);
                        hist[bin > 7 ? 7 : bin]++;
                    }
                    long long last_start = first;
                    for (int i = 0; i < nb; ++i) if (t[4 * i] > last_start) last_start = t[4 * i];
                    fprintf(stderr, "[icp normals] blocks=%d span %.1f us (last block starts at %.1f); ring 1 mean %.1f max %.1f; stragglers mean %.1f max %.1f; eigen mean %.1f; block duration histogram (10 us bins): %d %d %d %d %d %d %d %d\n",
                            nb, (last_end - first) * 0.01, (last_start - first) * 0.01, a / nb, amax, b / nb, bmax, e / nb,
                            hist[0], hist[1], hist[2], hist[3], hist[4], hist[5], hist[6], hist[7]);
                }
            }
            (void)hipMemset(ctx->dbg_counts.ptr, 0, DBG_BYTES);
        }
    }
}
