// Stand-alone driver of csrc/grid_tables_plan.h for tests/test_grid_tables_plan_host.py (built under the host sanitizers).
// Reads one event per line and prints one answer per line.  Besides the plan's state it keeps the PHYSICAL truth of two
// tables (id 0 and 1: slots per level, whether every entry is empty, whether the current grid lives there) and aborts when
// a build would insert into a table that is neither empty nor emptied by the build itself, or when a clearing workgroup would
// be handed the table of the current grid.
//   S clear_ahead cell_lists excluded                 the last solving launch of an enqueued registration
//     -> clears realloc cleared_id current_id spare_tsize spare_clean
//   B tsize clear_ahead deferred cell_lists excluded  a grid build of `tsize` slots per level
//     -> use_spare must_clear current_id current_tsize spare_tsize spare_clean
//   L                                                 the spare is lost (allocation failure)
//     -> spare_tsize spare_clean
#include <stdio.h>
#include <stdlib.h>

#include "grid_tables_plan.h"

struct Table {
    unsigned tsize = 0;
    bool empty = false;
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    icp::GridTablesState s;
    Table phys[2];
    int cur = 0;  // the table the current grid lives in
    bool have_grid = false;
    char kind;
    while (fscanf(f, " %c", &kind) == 1) {
        if (kind == 'S') {
            int ca, cl, ex;
            if (fscanf(f, "%d %d %d", &ca, &cl, &ex) != 3) return 3;
            icp::GridTablesMode mode;
            mode.clear_ahead = ca != 0;
            mode.cell_lists = cl != 0;
            mode.excluded = ex != 0;
            bool realloc = false;
            const bool clears = have_grid && icp::solve_clears_spare(s, phys[cur].tsize, mode, &realloc);
            const int spare = cur ^ 1;
            if (clears) {
                if (spare == cur) abort();
                if (realloc) phys[spare].tsize = phys[cur].tsize;
                if (phys[spare].tsize != phys[cur].tsize) abort();  // (a clearing launch over an allocation of another size)
                phys[spare].empty = true;
            }
            printf("%d %d %d %d %u %d\n", clears ? 1 : 0, realloc ? 1 : 0, clears ? spare : -1, cur, s.spare_tsize,
                   s.spare_clean ? 1 : 0);
        } else if (kind == 'B') {
            unsigned tsize;
            int ca, de, cl, ex;
            if (fscanf(f, "%u %d %d %d %d", &tsize, &ca, &de, &cl, &ex) != 5) return 3;
            icp::GridTablesMode mode;
            mode.clear_ahead = ca != 0;
            mode.deferred = de != 0;
            mode.cell_lists = cl != 0;
            mode.excluded = ex != 0;
            const icp::GridBuildTarget t = icp::grid_build_target(s, tsize, have_grid ? phys[cur].tsize : 0u, mode);
            if (t.use_spare) cur ^= 1;
            else phys[cur].tsize = tsize;  // (in place: the current allocation serves, grown where it must)
            if (phys[cur].tsize != tsize) abort();
            if (!t.must_clear && !phys[cur].empty) abort();  // inserting into a table nobody emptied
            phys[cur].empty = false;                         // the grid lives here now
            have_grid = true;
            printf("%d %d %d %u %u %d\n", t.use_spare ? 1 : 0, t.must_clear ? 1 : 0, cur, phys[cur].tsize, s.spare_tsize,
                   s.spare_clean ? 1 : 0);
        } else if (kind == 'L') {
            icp::spare_lost(s);
            phys[cur ^ 1] = Table();
            printf("%u %d\n", s.spare_tsize, s.spare_clean ? 1 : 0);
        } else {
            return 3;
        }
    }
    fclose(f);
    return 0;
}
