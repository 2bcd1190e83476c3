// Stand-alone check of csrc/knn_plan.h (what icp_knn_query refuses before it touches the device, the list length a k runs
// on, the squared bound), built with -fsanitize=address,undefined by tests/test_knn_host.py.
// Input (a text file), one case per line:
//   Q <n> <k> <flags> <has_dist> <has_index> <mem> <out_mem>
//   B <bound as the hexadecimal bits of a float32>
// Output, one line per case:
//   Q: "ok <list length>"  or  "refused <status> <reason>"
//   B: "<squared bound as hexadecimal bits>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "knn_plan.h"

using namespace icp;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    char kind[8];
    while (fscanf(in, "%7s", kind) == 1) {
        if (kind[0] == 'Q') {
            long long n = 0;
            int k = 0, flags = 0, has_dist = 0, has_index = 0, mem = 0, out_mem = 0;
            if (fscanf(in, "%lld %d %d %d %d %d %d", &n, &k, &flags, &has_dist, &has_index, &mem, &out_mem) != 7) return 3;
            char* reason = (char*)malloc(160);  // (heap, exactly the documented size: a longer message is the sanitizer's to find)
            memset(reason, 0x5a, 160);
            const int rc = knn_query_refusals(n, k, flags, has_dist != 0, has_index != 0, mem, out_mem, reason);
            if (rc == ICP_OK) {
                if (reason[0]) return 4;
                printf("ok %d\n", knn_list_length(k));
            } else {
                if (!reason[0] || strlen(reason) >= 160) return 4;
                printf("refused %d %s\n", rc, reason);
            }
            free(reason);
        } else if (kind[0] == 'B') {
            unsigned bits = 0;
            if (fscanf(in, "%x", &bits) != 1) return 3;
            float b, b2;
            memcpy(&b, &bits, 4);
            b2 = knn_squared_bound(b);
            memcpy(&bits, &b2, 4);
            printf("%08x\n", bits);
        } else {
            return 3;
        }
    }
    fclose(in);
    return 0;
}
