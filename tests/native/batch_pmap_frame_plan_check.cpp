// Stand-alone check of csrc/batch_pmap_frame_plan.h (the member partition and the refusals of icp_batch_pmap_frame_launch /
// icp_batch_pmap_frame_end), built with -fsanitize=address,undefined by tests/test_pmap_frame_host.py.
// Input (a text file), one case per line:
//   P <count> <pending> <vertex_map> <host> then per member: skip has_sequence kd_sequence frame_index voxel_size targets
//       normals_kernel_size point_to_point exchange profiling registering frame_launched has_timestamps n pixels stream
//   E <pending>
// Output, one line per case:
//   P: "ok S <skipped..> F <first..> R <registering..> V <vertex_map>"  or  "refused <member> <reason>"; then "same" or
//      "changed": whether the member table reads as it did before the call
//   E: "ok" or "refused <reason>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "batch_pmap_frame_plan.h"

using namespace icp;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    char kind[8];
    while (fscanf(in, "%7s", kind) == 1) {
        if (kind[0] == 'P') {
            int count = 0, pending = 0, vmap = 0, host = 0;
            if (fscanf(in, "%d %d %d %d", &count, &pending, &vmap, &host) != 4 || count < 0 || count > 64) return 3;
            std::vector<BatchPmapFrameMember> members((size_t)count);  // (heap: reads past `count` are the sanitizer's to find)
            if (count > 0) memset(members.data(), 0, sizeof(BatchPmapFrameMember) * (size_t)count);
            for (int b = 0; b < count; ++b) {
                BatchPmapFrameMember& m = members[(size_t)b];
                unsigned long long stream = 0;
                long long n = 0, pixels = 0;
                if (fscanf(in, "%d %d %d %d %lf %d %d %d %d %d %d %d %d %lld %lld %llu", &m.skip, &m.has_sequence, &m.kd_sequence,
                           &m.frame_index, &m.voxel_size, &m.targets, &m.normals_kernel_size, &m.point_to_point, &m.exchange,
                           &m.profiling, &m.registering, &m.frame_launched, &m.has_timestamps, &n, &pixels, &stream) != 16)
                    return 3;
                m.n = n;
                m.pixels = pixels;
                m.stream = stream;
            }
            const std::vector<BatchPmapFrameMember> before = members;
            BatchPmapFramePlan* plan = new BatchPmapFramePlan;
            memset(plan, 0x5a, sizeof(*plan));
            const bool ok = batch_pmap_frame_plan(count > 0 ? members.data() : nullptr, count, pending != 0, vmap != 0, host != 0, plan);
            if (!ok) {
                if (plan->n_skipped || plan->n_first || plan->n_registering) return 4;  // a refusal hands out no list
                printf("refused %d %s", plan->refused_member, plan->reason);
            } else {
                printf("ok S");
                for (int i = 0; i < plan->n_skipped; ++i) printf(" %d", plan->skipped[i]);
                printf(" F");
                for (int i = 0; i < plan->n_first; ++i) printf(" %d", plan->first[i]);
                printf(" R");
                for (int i = 0; i < plan->n_registering; ++i) printf(" %d", plan->registering[i]);
                printf(" V %d", plan->vertex_map);
            }
            const bool same = count == 0 || memcmp(before.data(), members.data(), sizeof(BatchPmapFrameMember) * (size_t)count) == 0;
            printf(" | %s\n", same ? "same" : "changed");
            delete plan;
        } else if (kind[0] == 'E') {
            int pending = 0;
            if (fscanf(in, "%d", &pending) != 1) return 3;
            const char* reason = batch_pmap_frame_end_refusal(pending != 0);
            if (reason) printf("refused %s\n", reason);
            else printf("ok\n");
        } else {
            return 3;
        }
    }
    fclose(in);
    return 0;
}
