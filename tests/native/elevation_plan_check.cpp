// Stand-alone check of csrc/elevation_plan.h (what icp_elevation_* refuses before it touches the device, the grids and the
// footprint of an image, and the arithmetic of one row and one pixel that the kernels call), built with
// -fsanitize=address,undefined by tests/test_elevation_host.py.
// Input (a text file), one case per line; doubles travel as the hexadecimal bits of a float64, floats as those of a float32:
//   C <height> <width> <pixel bits> <z_min bits> <z_max bits> <table: 0 NULL | 1 given> <max_rows>     icp_elevation_create
//   B <n> <max_rows> <mem> <dtype>                                                                      icp_elevation_build
//   W <same context: 0 | 1 | 2 map without a context> <frame_lo> <frame_hi> <pose: 0 NULL | 1 identity | 2 entry `which` =
//     `value bits`> <which> <value bits>                                                                icp_elevation_build_aggmap
//   G <out_mem>                                                                                         icp_elevation_get
//   T <height> <width> <max_rows> <host rows> <count> <capacity>       footprint, workgroups of `count`, of a window over `capacity`
//   X <f | d> <value bits> <pixel bits> <half> <extent>                 the cell of a coordinate
//   Z <f | d> <z bits> <lo bits> <hi bits> <den bits> <flip> <row>      clipped z, its z-buffer word, theta, colour row
//   K <theta bits>                                                      the colour row of a float32 theta
// Output, one line per case:
//   C B W G: "ok"  or  "refused <status> <reason>"
//   T: "<footprint bytes> <workgroups> <window workgroups>"      X: "<0 | 1> <cell>"
//   Z: "<clipped bits> <word hex> <theta bits> <colour row>"      K: "<colour row>"
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "elevation_plan.h"

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

static unsigned long long bits_of(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    return b;
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

template <typename T>
static void row_case(T z, T lo, T hi, T den, int flip, unsigned row) {
    const T c = elevation_clip(z, lo, hi);
    const float theta = elevation_theta(c, lo, den);
    const uint64_t word = sizeof(T) == 4 ? elevation_key32((float)c, flip, row) : elevation_key64((double)c, flip);
    printf("%llx %" PRIx64 " %llx %d\n", bits_of(c), word, bits_of(theta), elevation_colour_row(theta));
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
            long long h = 0, w = 0, rows = 0;
            unsigned long long pb = 0, lb = 0, hb = 0;
            int table = 0;
            if (fscanf(in, "%lld %lld %llx %llx %llx %d %lld", &h, &w, &pb, &lb, &hb, &table, &rows) != 7) return 3;
            unsigned char* lut = table ? (unsigned char*)malloc(ELEV_LUT_ROWS * 3) : nullptr;
            bad = report(elevation_create_refusals(h, w, from_bits(pb), from_bits(lb), from_bits(hb), lut, rows, reason), reason);
            free(lut);
        } else if (kind[0] == 'B') {
            long long n = 0, rows = 0;
            int mem = 0, dtype = 0;
            if (fscanf(in, "%lld %lld %d %d", &n, &rows, &mem, &dtype) != 4) return 3;
            bad = report(elevation_build_refusals(n, rows, mem, dtype, reason), reason);
        } else if (kind[0] == 'W') {
            int same = 0, lo = 0, hi = 0, pk = 0, which = 0;
            unsigned long long bits = 0;
            if (fscanf(in, "%d %d %d %d %d %llx", &same, &lo, &hi, &pk, &which, &bits) != 6) return 3;
            double* pose = make_pose(pk, which, bits);
            int a = 0, b = 0;
            bad = report(elevation_build_aggmap_refusals(&a, same == 1 ? (void*)&a : same == 2 ? nullptr : (void*)&b, lo, hi, pose, reason),
                         reason);
            free(pose);
        } else if (kind[0] == 'G') {
            int mem = 0;
            if (fscanf(in, "%d", &mem) != 1) return 3;
            bad = report(elevation_get_refusals(mem, reason), reason);
        } else if (kind[0] == 'T') {
            long long h = 0, w = 0, rows = 0, count = 0, cap = 0;
            int host = 0;
            if (fscanf(in, "%lld %lld %lld %d %lld %lld", &h, &w, &rows, &host, &count, &cap) != 6) return 3;
            printf("%" PRIu64 " %lld %lld\n", elevation_footprint_bytes(h, w, rows, host), (long long)elevation_blocks(count),
                   (long long)elevation_window_blocks(cap));
        } else if (kind[0] == 'X') {
            char type[4];
            unsigned long long vb = 0, pb = 0;
            long long half = 0, extent = 0;
            if (fscanf(in, "%3s %llx %llx %lld %lld", type, &vb, &pb, &half, &extent) != 5) return 3;
            int cell = -1;
            const bool in_image = type[0] == 'f' ? elevation_cell(from_bits32(vb), from_bits32(pb), (float)half, extent, &cell)
                                                 : elevation_cell(from_bits(vb), from_bits(pb), (double)half, extent, &cell);
            printf("%d %d\n", in_image ? 1 : 0, in_image ? cell : -1);
        } else if (kind[0] == 'Z') {
            char type[4];
            unsigned long long zb = 0, lb = 0, hb = 0, db = 0;
            int flip = 0;
            unsigned row = 0;
            if (fscanf(in, "%3s %llx %llx %llx %llx %d %u", type, &zb, &lb, &hb, &db, &flip, &row) != 7) return 3;
            if (type[0] == 'f')
                row_case(from_bits32(zb), from_bits32(lb), from_bits32(hb), from_bits32(db), flip, row);
            else
                row_case(from_bits(zb), from_bits(lb), from_bits(hb), from_bits(db), flip, row);
        } else if (kind[0] == 'K') {
            unsigned long long tb = 0;
            if (fscanf(in, "%llx", &tb) != 1) return 3;
            printf("%d\n", elevation_colour_row(from_bits32(tb)));
        } else {
            return 3;
        }
        free(reason);
        if (bad) return bad;
    }
    fclose(in);
    return 0;
}
