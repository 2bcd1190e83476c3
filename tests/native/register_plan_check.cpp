// Stand-alone check of csrc/register_plan.h (the first chunk of a launched registration, the descriptor-slot layouts of the
// batched registrations), built with -fsanitize=address,undefined by tests/test_register_plan_host.py.
// Input (a text file), one case per line:
//   C <iters> <threshold> <chunked_launch> <tail_planned> <count> <last_iterations x count>
//   K <pack_desc> <iterate_desc> <sum_solve_desc> <count> <chunk>
//   P <pack_desc> <reg_desc> <sum_solve_desc> <count>
// Output, one line per case:
//   C: "<iterations of the first chunk>"
//   K: "<first table> <iterate table bytes> <sum + solve table bytes> <need>"
//   P: "<registrations> <sum + solve> <sum + solve of the last iteration> <need>"
#include <stdio.h>
#include <stdlib.h>

#include "register_plan.h"

using namespace icp;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    char kind[8];
    while (fscanf(in, "%7s", kind) == 1) {
        if (kind[0] == 'C') {
            int iters = 0, chunked = 0, tail = 0, count = 0;
            float threshold = 0.f;
            if (fscanf(in, "%d %f %d %d %d", &iters, &threshold, &chunked, &tail, &count) != 5 || count < 0) return 3;
            int* last = (int*)malloc(sizeof(int) * (size_t)(count > 0 ? count : 1));  // (heap, exactly `count`: a read past it is the sanitizer's to find)
            for (int i = 0; i < count; ++i)
                if (fscanf(in, "%d", &last[i]) != 1) return 3;
            printf("%d\n", first_chunk_iterations(iters, threshold, chunked, tail != 0, last, count));
            free(last);
        } else if (kind[0] == 'K') {
            unsigned long pack = 0, it = 0, ss = 0;
            int count = 0, chunk = 0;
            if (fscanf(in, "%lu %lu %lu %d %d", &pack, &it, &ss, &count, &chunk) != 5) return 3;
            const BatchRegisterLayout lay(pack, it, ss, count);
            printf("%zu %zu %zu %zu\n", lay.first_table(), lay.it_bytes, lay.ss_bytes, lay.need(chunk));
        } else if (kind[0] == 'P') {
            unsigned long pack = 0, reg = 0, ss = 0;
            int count = 0;
            if (fscanf(in, "%lu %lu %lu %d", &pack, &reg, &ss, &count) != 4) return 3;
            const BatchPmapRegisterLayout lay(pack, reg, ss, count);
            printf("%zu %zu %zu %zu\n", lay.registrations(), lay.sum_solve(false), lay.sum_solve(true), lay.need());
        } else {
            return 3;
        }
    }
    fclose(in);
    return 0;
}
