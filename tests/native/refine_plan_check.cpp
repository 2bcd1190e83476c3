// Stand-alone check of csrc/refine_plan.h (what icp_refine_* refuses before it touches the device, the table and grid sizes,
// the ring count of a bound, the footprint) and of csrc/refine_device.h (the row filter, the box bound of a cell, the rigid step
// the solve kernel takes), built with -fsanitize=address,undefined by tests/test_refine_host.py.
// Input (a text file), one case per line; doubles travel as the hexadecimal bits of a float64, floats as those of a float32:
//   C <max_target_rows> <max_source_rows> <cell bits> <out: 0 NULL | 1>                                 icp_refine_create
//   S <n> <capacity> <mem> <flags> <in flight> <xyz: 0 NULL | 1>                                        icp_refine_set_target
//   L <n> <capacity> <mem> <init: 0 NULL | 1 identity | 2 entry `which` = `value bits`> <which> <value bits> <params: 0 NULL | 1>
//     <max_distance bits> <max_iteration> <relative_fitness bits> <relative_rmse bits> <flags> <have target> <in flight> <xyz: 0 NULL | 1>
//                                                                                                       icp_refine_launch
//   E <in flight> <out_mem>                                                                             icp_refine_end
//   Y <have result> <iterations> <cap>                                                                  icp_refine_history
//   I <image: 0 NULL | 1> <same context: 0 | 1> <xyz_out: 0 NULL | 1> <n_out: 0 NULL | 1>               icp_refine_image_rows
//   T <max_target_rows> <max_source_rows> <host target> <host source> <count>     table slots, footprint, workgroups, iteration grid
//   R <max_distance bits> <cell bits>                                             rings
//   Z <x bits32> <y bits32> <z bits32>                                            the zero-row filter
//   G <v bits> <k> <cell bits>                                                    the axis gap of a coordinate to cell k
//   P <17 figure bits>                                                            the step: 16 update bits
// Output, one line per case:
//   C S L E Y I: "ok"  or  "refused <status> <reason>"
//   T: "<slots> <footprint> <workgroups> <iteration workgroups>"   R: "<rings>"   Z: "<0 | 1>"   G: "<gap bits>"   P: 16 hex words
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "refine_device.h"
#include "refine_plan.h"

using namespace icp;

static double from_bits(unsigned long long bits) {
    double v;
    memcpy(&v, &bits, 8);
    return v;
}

static float from_bits32(unsigned long long bits) {
    const uint32_t b = (uint32_t)bits;
    float v;
    memcpy(&v, &b, 4);
    return v;
}

static unsigned long long bits_of(double v) {
    unsigned long long b;
    memcpy(&b, &v, 8);
    return b;
}

static int report(int rc, const char* reason) {
    if (rc == ICP_OK) {
        if (reason[0]) return 4;
        printf("ok\n");
    } else {
        if (!reason[0] || strlen(reason) >= 160) return 4;
        printf("refused %d %s\n", rc, reason);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    char line[2048];
    int bad = 0;
    while (!bad && fgets(line, sizeof(line), f)) {
        // (a reason buffer of exactly the 160 bytes the header promises to stay within)
        char* reason = (char*)malloc(160);
        long long a, b, c, d, e;
        unsigned long long u[17];
        long long g;
        static const float some_rows[3] = {0.f, 0.f, 0.f};
        if (line[0] == 'C' && sscanf(line + 1, "%lld %lld %llx %lld", &a, &b, &u[0], &c) == 4) {
            bad = report(refine_create_refusals(a, b, from_bits(u[0]), c ? (const void*)some_rows : nullptr, reason), reason);
        } else if (line[0] == 'S' && sscanf(line + 1, "%lld %lld %lld %lld %lld %lld", &a, &b, &c, &d, &e, &g) == 6) {
            bad = report(refine_set_target_refusals(g ? some_rows : nullptr, a, b, (int)c, (int32_t)d, (int)e, reason), reason);
        } else if (line[0] == 'I' && sscanf(line + 1, "%lld %lld %lld %lld", &a, &b, &c, &d) == 4) {
            bad = report(refine_image_rows_refusals(a ? (const void*)some_rows : nullptr, b ? (const void*)(some_rows + 1) : (const void*)(some_rows + 2),
                                                    some_rows + 1, c ? (const void*)some_rows : nullptr, d ? (const void*)some_rows : nullptr, reason),
                         reason);
        } else if (line[0] == 'L') {
            long long n, cap, mem, kind, which, have_p, iters, flags, have_t, flying, have_xyz;
            if (sscanf(line + 1, "%lld %lld %lld %lld %lld %llx %lld %llx %lld %llx %llx %lld %lld %lld %lld", &n, &cap, &mem, &kind, &which, &u[0],
                       &have_p, &u[1], &iters, &u[2], &u[3], &flags, &have_t, &flying, &have_xyz) != 15) {
                bad = 3;
            } else {
                double* init = nullptr;
                if (kind) {
                    init = (double*)malloc(16 * sizeof(double));
                    for (int i = 0; i < 16; ++i) init[i] = (i % 5 == 0) ? 1.0 : 0.0;
                    if (kind == 2 && which >= 0 && which < 16) init[which] = from_bits(u[0]);
                }
                icp_refine_params* p = nullptr;
                if (have_p) {
                    p = (icp_refine_params*)malloc(sizeof(icp_refine_params));
                    p->max_distance = from_bits(u[1]);
                    p->max_iteration = (int32_t)iters;
                    p->relative_fitness = from_bits(u[2]);
                    p->relative_rmse = from_bits(u[3]);
                    p->flags = (int32_t)flags;
                }
                bad = report(refine_launch_refusals(have_xyz ? some_rows : nullptr, n, cap, (int)mem, init, p, (int)have_t, (int)flying, reason), reason);
                free(init);
                free(p);
            }
        } else if (line[0] == 'E' && sscanf(line + 1, "%lld %lld", &a, &b) == 2) {
            bad = report(refine_end_refusals((int)a, (int)b, reason), reason);
        } else if (line[0] == 'Y' && sscanf(line + 1, "%lld %lld %lld", &a, &b, &c) == 3) {
            bad = report(refine_history_refusals((int)a, (int32_t)b, (int32_t)c, reason), reason);
        } else if (line[0] == 'T' && sscanf(line + 1, "%lld %lld %lld %lld %lld", &a, &b, &c, &d, &e) == 5) {
            printf("%lld %llu %lld %d\n", (long long)refine_table_slots(a), (unsigned long long)refine_footprint_bytes(a, b, (int)c, (int)d),
                   (long long)refine_blocks(e), refine_iterate_blocks(e));
        } else if (line[0] == 'R' && sscanf(line + 1, "%llx %llx", &u[0], &u[1]) == 2) {
            printf("%d\n", refine_rings(from_bits(u[0]), from_bits(u[1])));
        } else if (line[0] == 'Z' && sscanf(line + 1, "%llx %llx %llx", &u[0], &u[1], &u[2]) == 3) {
            printf("%d\n", refine_zero_row(from_bits32(u[0]), from_bits32(u[1]), from_bits32(u[2])) ? 1 : 0);
        } else if (line[0] == 'G' && sscanf(line + 1, "%llx %lld %llx", &u[0], &a, &u[1]) == 3) {
            printf("%llx\n", bits_of(refine_axis_gap(from_bits(u[0]), (int)a, from_bits(u[1]))));
        } else if (line[0] == 'P') {
            double* fig = (double*)malloc(REF_FIGURES * sizeof(double));
            double* update = (double*)malloc(16 * sizeof(double));
            char* at = line + 1;
            int got = 0;
            for (; got < REF_FIGURES; ++got) {
                char* end;
                const unsigned long long w = strtoull(at, &end, 16);
                if (end == at) break;
                fig[got] = from_bits(w);
                at = end;
            }
            if (got != REF_FIGURES) {
                bad = 3;
            } else {
                refine_step(fig, update);
                for (int i = 0; i < 16; ++i) printf("%llx%c", bits_of(update[i]), i == 15 ? '\n' : ' ');
            }
            free(fig);
            free(update);
        } else {
            bad = 3;
        }
        free(reason);
    }
    fclose(f);
    return bad;
}
