// The two hash tables of a context (a current one the grid lives in, a spare the next build may target): the decision rule,
// as plain C++ without a HIP dependency, so that it also builds into a stand-alone program under the host sanitizers
// (tests/native/grid_tables_plan_check.cpp).  hash_grid.hip and gauss_newton.hip call it.
#pragma once
namespace icp {

// spare_tsize: slots per level the spare allocation holds (0: none); spare_clean: every entry of it is empty — or will be
// by the time anything enqueued from now on reads it (the clearing workgroups of a solving launch are on the stream)
struct GridTablesState {
    unsigned spare_tsize = 0;
    bool spare_clean = false;
};

// what rules the spare out altogether: the build or the registration runs in a mode this schedule leaves alone
struct GridTablesMode {
    bool clear_ahead = true;  // option "clear_ahead"
    bool deferred = false;    // a build whose launches the batch layer runs (build_grid(defer)) / a batched solving launch
    bool cell_lists = false;  // a build on cell lists
    bool excluded = false;    // multi-GPU exchange, "overlap_map_update", the event profile, "search_stats"
    bool usable() const { return clear_ahead && !deferred && !cell_lists && !excluded; }
};

// The last solving launch of an enqueued registration, against a grid in a table of `cur_tsize` slots per level: true = it is
// launched with the clearing workgroups over the spare, which must be (re)allocated first where `*realloc` comes back true.
// The spare counts as clean from here on (stream order).  The current table is never the one handed out: the caller passes
// the spare's pointer, and a flip happens only in grid_build_target below.
inline bool solve_clears_spare(GridTablesState& s, unsigned cur_tsize, const GridTablesMode& mode, bool* realloc) {
    *realloc = false;
    if (!mode.usable() || cur_tsize == 0) return false;
    if (s.spare_tsize == cur_tsize && s.spare_clean) return false;  // cleared once, not used since
    *realloc = s.spare_tsize != cur_tsize;
    s.spare_tsize = cur_tsize;
    s.spare_clean = true;
    return true;
}

// the spare could not be (re)allocated, or its clearing launch failed: there is none
inline void spare_lost(GridTablesState& s) {
    s.spare_tsize = 0;
    s.spare_clean = false;
}

struct GridBuildTarget {
    bool use_spare;    // build into the spare, then flip: the old current table (of `cur_tsize` slots) becomes the dirty spare
    bool must_clear;   // the build's own first launch empties its table
};

// A grid build of `tsize` slots per level, the current table holding `cur_tsize` (0: no table yet).
inline GridBuildTarget grid_build_target(GridTablesState& s, unsigned tsize, unsigned cur_tsize, const GridTablesMode& mode) {
    GridBuildTarget t{false, true};
    if (mode.usable() && s.spare_clean && s.spare_tsize == tsize && tsize != 0) {
        t.use_spare = true;
        t.must_clear = false;
        s.spare_tsize = cur_tsize;  // the flip: what was current is the spare now, full of the old grid
        s.spare_clean = false;
    }
    return t;  // (in place otherwise: the spare stays what it was — a clean table stays clean, one of another size is replaced by the next solve)
}

}  // namespace icp
