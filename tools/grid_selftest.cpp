// grid_selftest -- csrc/idc_grid.h without a device: the clamp every capped grid-stride launcher asks for its grid, the test hook that lowers
// it and the per-tag record.  No HIP runtime call.  Checked (tests/test_grid_cap_cpu.py runs this; `make grid_selftest SAN=1` builds it under
// ASan + UBSan):
//   1. lowering 0 gives min(want, builtin_cap);
//   2. a lowering above the built-in cap gives the built-in cap: the hook never raises a grid;
//   3. a lowering below want gives the lowered value;
//   4. want = 1 gives 1, and so does want = 0 (a grid is never empty);
//   5. the record holds the last call per tag and leaves every other tag alone; the tag names and their indices round-trip.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "idc_grid.h"

using namespace idc;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

int main() {
    // tags: 21 names, distinct, nullptr past either end, index round-trip
    CHECK(kGridTags == 21);
    for (int i = 0; i < kGridTags; ++i) {
        CHECK(grid_tag_name(i) != nullptr && grid_tag_name(i)[0] != 0);
        CHECK(grid_tag_index(grid_tag_name(i)) == i);
        CHECK(grid_last(i).want == 0 && grid_last(i).blocks == 0);          // never launched
    }
    CHECK(grid_tag_name(kGridTags) == nullptr && grid_tag_name(-1) == nullptr);
    CHECK(grid_tag_index("no_such_tag") == -1 && grid_tag_index(nullptr) == -1 && grid_tag_index("") == -1);
    CHECK(strcmp(grid_tag_name((int)GridTag::head), "head") == 0 && strcmp(grid_tag_name((int)GridTag::nchw_to_split), "nchw_to_split") == 0);

    // 1. no lowering: min(want, builtin)
    CHECK(grid_cap() == 0);
    CHECK(grid_blocks(GridTag::head, 540, 8192) == 540);
    CHECK(grid_blocks(GridTag::head, 8192, 8192) == 8192);
    CHECK(grid_blocks(GridTag::head, 8193, 8192) == 8192);
    CHECK(grid_blocks(GridTag::head, 131072, 8192) == 8192);
    CHECK(grid_blocks(GridTag::nchw_to_nhwc, 5000000000ll, 65535) == 65535);     // want beyond an int

    // 2. a lowering above the built-in cap never raises a grid
    set_grid_cap(100000);
    CHECK(grid_cap() == 100000);
    CHECK(grid_blocks(GridTag::head, 131072, 8192) == 8192);
    CHECK(grid_blocks(GridTag::eval_sse, 1000, 256) == 256);
    CHECK(grid_blocks(GridTag::eval_sse, 100, 256) == 100);
    CHECK(grid_blocks(GridTag::nchw_to_nhwc, 5000000000ll, 65535) == 65535);

    // 3. a lowering below want
    set_grid_cap(7);
    CHECK(grid_blocks(GridTag::head, 540, 8192) == 7);
    CHECK(grid_blocks(GridTag::head, 7, 8192) == 7);
    CHECK(grid_blocks(GridTag::head, 6, 8192) == 6);
    CHECK(grid_blocks(GridTag::head, 131072, 8192) == 7);
    CHECK(grid_blocks(GridTag::head, 540, 3) == 3);                             // the built-in cap still holds below the lowering
    set_grid_cap(1);
    CHECK(grid_blocks(GridTag::dist313, 65536, 16384) == 1);

    // 4. want = 1 (and 0) give 1 under every setting
    for (int cap : {0, 1, 3, 100000}) {
        set_grid_cap(cap);
        CHECK(grid_blocks(GridTag::lab_post, 1, 4096) == 1);
        CHECK(grid_blocks(GridTag::lab_post, 0, 4096) == 1);
    }
    set_grid_cap(-5);                                                           // the setter itself treats a negative value as "off"
    CHECK(grid_cap() == 0);

    // 5. the record: last call per tag, other tags untouched
    set_grid_cap(0);
    GridRecord before[kGridTags];
    for (int i = 0; i < kGridTags; ++i) before[i] = grid_last(i);
    CHECK(grid_last((int)GridTag::pcie_copy).want == 0);                        // still never launched
    CHECK(grid_blocks(GridTag::pcie_copy, 3000, 1024) == 1024);
    CHECK(grid_last((int)GridTag::pcie_copy).want == 3000 && grid_last((int)GridTag::pcie_copy).blocks == 1024);
    set_grid_cap(5);
    CHECK(grid_blocks(GridTag::pcie_copy, 48, 1024) == 5);
    CHECK(grid_last((int)GridTag::pcie_copy).want == 48 && grid_last((int)GridTag::pcie_copy).blocks == 5);
    for (int i = 0; i < kGridTags; ++i)
        if (i != (int)GridTag::pcie_copy) CHECK(grid_last(i).want == before[i].want && grid_last(i).blocks == before[i].blocks);
    CHECK(grid_last((int)GridTag::head).want == 540 && grid_last((int)GridTag::head).blocks == 3);
    CHECK(grid_last((int)GridTag::nchw_to_nhwc).want == 5000000000ll && grid_last((int)GridTag::nchw_to_nhwc).blocks == 65535);
    CHECK(grid_last((int)GridTag::range_audit).want == 0);

    printf("grid_selftest: ok (%d tags)\n", kGridTags);
    return 0;
}
