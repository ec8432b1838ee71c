// idc_grid.h -- the one place that clamps the grid of a grid-stride launch.  Plain C++, no HIP: tools/grid_selftest.cpp includes it alone.
// A launcher whose kernel walks its items in a grid-stride loop asks grid_blocks(tag, want, builtin_cap) for its workgroup count: `want` is
// the count that covers every item in one pass, `builtin_cap` the launcher's own upper bound.  The test hook set_grid_cap(v) (option "grid_cap")
// lowers every such grid to at most v workgroups, so that a test-sized shape runs many passes with a ragged last one; it can never raise a
// grid above the launcher's own cap, and 0 (the default) changes nothing.  Each call records (want, blocks) under its tag -- process-wide,
// the last launch wins, not synchronised with other threads: a diagnostic (idc_grid_last), nothing a launch depends on.
#ifndef IDC_GRID_H
#define IDC_GRID_H

#include <string.h>

namespace idc {

// one tag per capped launch site
#define IDC_FOR_EACH_GRID_TAG(X)                                                                                                      \
    X(head) X(softmax_nchw) X(dist313) X(lab_post) X(pcie_copy) X(upsample_lab2rgb) X(global_stats) X(ingest_rgb) X(fullres_rgb)     \
    X(batch_prologue) X(batch_fullres_rgb) X(ragged_prologue) X(ragged_fullres_rgb) X(ragged_net_truth) X(eval_sse) X(range_audit)    \
    X(splitk_epilogue) X(nchw_to_nhwc) X(nhwc_to_nchw) X(split_to_nchw) X(nchw_to_split)

enum class GridTag : int {
#define X(t) t,
    IDC_FOR_EACH_GRID_TAG(X)
#undef X
    count_
};

constexpr int kGridTags = (int)GridTag::count_;

struct GridRecord {
    long long want = 0;      // 0: the tag never launched
    int blocks = 0;
};

struct GridState {
    int lowered = 0;         // 0 = no lowering
    GridRecord last[kGridTags];
};

inline GridState& grid_state() {
    static GridState s;
    return s;
}

inline void set_grid_cap(int v) { grid_state().lowered = v > 0 ? v : 0; }
inline int grid_cap() { return grid_state().lowered; }

// max(1, min(want, builtin_cap, lowered)); lowered == 0 takes no part
inline int grid_blocks(GridTag tag, long long want, int builtin_cap) {
    GridState& g = grid_state();
    long long b = want < builtin_cap ? want : builtin_cap;
    if (g.lowered > 0 && b > g.lowered) b = g.lowered;
    if (b < 1) b = 1;
    GridRecord& r = g.last[(int)tag];
    r.want = want; r.blocks = (int)b;
    return (int)b;
}

// name of tag i, nullptr past the end
inline const char* grid_tag_name(int i) {
    static const char* const names[kGridTags] = {
#define X(t) #t,
        IDC_FOR_EACH_GRID_TAG(X)
#undef X
    };
    return i >= 0 && i < kGridTags ? names[i] : nullptr;
}

// index of the tag called `name`, -1 when there is none
inline int grid_tag_index(const char* name) {
    if (name == nullptr) return -1;
    for (int i = 0; i < kGridTags; ++i)
        if (strcmp(name, grid_tag_name(i)) == 0) return i;
    return -1;
}

inline GridRecord grid_last(int i) { return grid_state().last[i]; }

}  // namespace idc

#endif  // IDC_GRID_H
