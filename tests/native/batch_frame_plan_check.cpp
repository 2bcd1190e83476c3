// Stand-alone check of csrc/batch_frame_plan.h (the member partition and the refusals of icp_batch_frame_launch /
// icp_batch_frame_end), built with -fsanitize=address,undefined by tests/test_batch_frame_host.py.
// Input (a text file), one case per line:
//   P <count> <pending> then per member: skip has_sequence frame_index voxel_size targets point_to_point projective_map
//                                         exchange profiling registering frame_launched stream
//   U <n> then n pairs: member status
//   E <pending>
// Output, one line per case:
//   P: "ok S <skipped..> F <first..> R <registering..> M <mask of the registering members>"  or  "refused <member> <reason>"
//   U: "update <members..> first <status>"
//   E: "ok" or "refused <reason>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "batch_frame_plan.h"

using namespace icp;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* in = fopen(argv[1], "r");
    if (!in) return 2;
    char kind[8];
    while (fscanf(in, "%7s", kind) == 1) {
        if (kind[0] == 'P') {
            int count = 0, pending = 0;
            if (fscanf(in, "%d %d", &count, &pending) != 2 || count < 0 || count > 64) return 3;
            std::vector<BatchFrameMember> members((size_t)count);  // (heap: reads past `count` are the sanitizer's to find)
            for (int b = 0; b < count; ++b) {
                BatchFrameMember& m = members[(size_t)b];
                unsigned long long stream = 0;
                if (fscanf(in, "%d %d %d %lf %d %d %d %d %d %d %d %llu", &m.skip, &m.has_sequence, &m.frame_index, &m.voxel_size,
                           &m.targets, &m.point_to_point, &m.projective_map, &m.exchange, &m.profiling, &m.registering,
                           &m.frame_launched, &stream) != 12)
                    return 3;
                m.stream = stream;
            }
            BatchFramePlan* plan = new BatchFramePlan;
            memset(plan, 0x5a, sizeof(*plan));
            const bool ok = batch_frame_plan(count > 0 ? members.data() : nullptr, count, pending != 0, plan);
            if (!ok) {
                if (plan->n_skipped || plan->n_first || plan->n_registering) return 4;  // a refusal hands out no list
                printf("refused %d %s\n", plan->refused_member, plan->reason);
            } else {
                printf("ok S");
                for (int i = 0; i < plan->n_skipped; ++i) printf(" %d", plan->skipped[i]);
                printf(" F");
                for (int i = 0; i < plan->n_first; ++i) printf(" %d", plan->first[i]);
                printf(" R");
                for (int i = 0; i < plan->n_registering; ++i) printf(" %d", plan->registering[i]);
                printf(" M %u\n", batch_frame_mask(plan->registering, plan->n_registering));
            }
            delete plan;
        } else if (kind[0] == 'U') {
            int n = 0;
            if (fscanf(in, "%d", &n) != 1 || n < 0 || n > BATCH_FRAME_MAX_MEMBERS) return 3;
            std::vector<int32_t> reg((size_t)n), st((size_t)n), upd((size_t)n);
            for (int i = 0; i < n; ++i)
                if (fscanf(in, "%d %d", &reg[(size_t)i], &st[(size_t)i]) != 2) return 3;
            int32_t first = 77;
            const int nu = batch_frame_update_members(reg.data(), st.data(), n, upd.data(), &first);
            printf("update");
            for (int i = 0; i < nu; ++i) printf(" %d", upd[(size_t)i]);
            printf(" first %d\n", first);
        } else if (kind[0] == 'E') {
            int pending = 0;
            if (fscanf(in, "%d", &pending) != 1) return 3;
            const char* reason = batch_frame_end_refusal(pending != 0);
            if (reason) printf("refused %s\n", reason);
            else printf("ok\n");
        } else {
            return 3;
        }
    }
    fclose(in);
    return 0;
}
