// Stand-alone check of csrc/aggmap_plan.h (what icp_aggmap_* refuses before it touches the device, the slot count and the
// footprint of a map, the key packing and the slot function), built with -fsanitize=address,undefined by
// tests/test_aggmap_host.py.
// Input (a text file), one case per line; doubles travel as the hexadecimal bits of a float64:
//   C <voxel bits> <capacity> <max_rows>                     icp_aggmap_create
//   I <n> <max_rows> <mem> <pose: 0 NULL | 1 identity | 2 entry `which` = `value bits`> <which> <value bits>
//   S <frame_lo> <frame_hi> <out_mem> <pose as for I> <which> <value bits>
//   G <out_mem>
//   T <capacity> <max_rows>                                  slot count, footprint, rows per workgroup of max_rows rows
//   P <capacity + max_rows>                                  slot count of that sum alone
//   K <cx> <cy> <cz> <mask as hexadecimal>                   key, round trip, slot
//   R <coordinate bits>                                      is the (real) voxel coordinate in range
// Output, one line per case:
//   C I S G: "ok"  or  "refused <status> <reason>"
//   T: "<slots> <footprint bytes> <rows per workgroup>"      P: "<slots>"      K: "<key hex> <cx> <cy> <cz> <slot>"      R: "0" | "1"
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "aggmap_plan.h"

using namespace icp;

static double from_bits(unsigned long long bits) {
    double v;
    memcpy(&v, &bits, 8);
    return v;
}

// a heap pose of exactly 16 doubles (a read beyond it is the sanitizer's to find); NULL for kind 0
static double* make_pose(int kind, int which, unsigned long long bits) {
    if (kind == 0) return nullptr;
    double* p = (double*)malloc(16 * sizeof(double));
    for (int i = 0; i < 16; ++i) p[i] = (i % 5 == 0) ? 1.0 : 0.0;
    if (kind == 2 && which >= 0 && which < 16) p[which] = from_bits(bits);
    return p;
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
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    char kind[8];
    while (fscanf(in, "%7s", kind) == 1) {
        char* reason = (char*)malloc(160);  // (heap, exactly the documented size)
        memset(reason, 0x5a, 160);
        int bad = 0;
        if (kind[0] == 'C') {
            unsigned long long vb = 0;
            long long cap = 0, rows = 0;
            if (fscanf(in, "%llx %lld %lld", &vb, &cap, &rows) != 3) return 3;
            bad = report(aggmap_create_refusals(from_bits(vb), cap, rows, reason), reason);
        } else if (kind[0] == 'I') {
            long long n = 0, rows = 0;
            int mem = 0, pk = 0, which = 0;
            unsigned long long bits = 0;
            if (fscanf(in, "%lld %lld %d %d %d %llx", &n, &rows, &mem, &pk, &which, &bits) != 6) return 3;
            double* pose = make_pose(pk, which, bits);
            bad = report(aggmap_insert_refusals(n, rows, pose, mem, reason), reason);
            free(pose);
        } else if (kind[0] == 'S') {
            int lo = 0, hi = 0, mem = 0, pk = 0, which = 0;
            unsigned long long bits = 0;
            if (fscanf(in, "%d %d %d %d %d %llx", &lo, &hi, &mem, &pk, &which, &bits) != 6) return 3;
            double* pose = make_pose(pk, which, bits);
            bad = report(aggmap_submap_refusals(lo, hi, pose, mem, reason), reason);
            free(pose);
        } else if (kind[0] == 'G') {
            int mem = 0;
            if (fscanf(in, "%d", &mem) != 1) return 3;
            bad = report(aggmap_get_refusals(mem, reason), reason);
        } else if (kind[0] == 'T') {
            long long cap = 0, rows = 0;
            if (fscanf(in, "%lld %lld", &cap, &rows) != 2) return 3;
            printf("%" PRIu64 " %" PRIu64 " %lld\n", aggmap_slot_count(cap, rows), aggmap_footprint_bytes(cap, rows),
                   (long long)aggmap_rows_per_block(rows));
        } else if (kind[0] == 'P') {
            unsigned long long total = 0;
            if (fscanf(in, "%llu", &total) != 1) return 3;
            printf("%" PRIu64 "\n", aggmap_slots_for(total));
        } else if (kind[0] == 'K') {
            long long c[3] = {0, 0, 0}, back[3];
            unsigned long long mask = 0;
            if (fscanf(in, "%lld %lld %lld %llx", &c[0], &c[1], &c[2], &mask) != 4) return 3;
            const unsigned long long key = aggmap_pack(c[0], c[1], c[2]);
            aggmap_unpack(key, back);
            printf("%llx %lld %lld %lld %llu\n", key, back[0], back[1], back[2], aggmap_slot(key, mask));
        } else if (kind[0] == 'R') {
            unsigned long long bits = 0;
            if (fscanf(in, "%llx", &bits) != 1) return 3;
            printf("%d\n", aggmap_coord_in_range(from_bits(bits)) ? 1 : 0);
        } else {
            return 3;
        }
        free(reason);
        if (bad) return bad;
    }
    fclose(in);
    return 0;
}
