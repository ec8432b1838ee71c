// idc_motion.h -- the block geometry, candidate order, item dealing and scratch sizes of the block-matched motion compensation of the temporal ab
// filter (idc_set_temporal_motion / idc_temporal_vectors; the rule: include/ideepcolor.h; the kernels: idc_motion.hip).  Plain C++ that makes no
// runtime call: the launchers, the kernels themselves and tools/motion_selftest.cpp, which includes it beside idc_batch.h alone, read the same
// functions.
#ifndef IDC_MOTION_H
#define IDC_MOTION_H

#include <stddef.h>
#include <stdint.h>

#include "idc_temporal.h"

namespace idc {

// Blocks of kMotionBlock x kMotionBlock net-size pixels; H and W are multiples of 8 (idc_create), so the blocks tile the plane exactly.  The
// search kernel works on the diff kernel's tile: kTemporalTileH x kTemporalTileW pixels = 2 x 8 blocks of ONE frame (blockIdx.y), clipped at the
// plane's bottom and right edges (a block is inside the plane wholly or not at all).
constexpr int kMotionBlock = 8;
constexpr int kMotionMaxSearch = 7;
constexpr int kMotionThreads = kTemporalThreads;
constexpr int kMotionTileBlocksY = kTemporalTileH / kMotionBlock, kMotionTileBlocksX = kTemporalTileW / kMotionBlock;
constexpr int kMotionTileBlocks = kMotionTileBlocksY * kMotionTileBlocksX;                 // 16
constexpr int kMotionLanes = kMotionThreads / kMotionTileBlocks;                           // 16 threads share one block's candidates
constexpr int kMotionMaxCandidates = (2 * kMotionMaxSearch + 1) * (2 * kMotionMaxSearch + 1);      // 225
// LDS of the search kernel: the tile, fp32 (4 KiB), and the predecessor's window with an apron of kMotionMaxSearch pixels whatever the call's
// search, (16 + 14) x (64 + 14) fp32 = 9360 bytes; cells outside the plane are filled with zeros and never read (an invalid candidate is skipped)
constexpr int kMotionWinH = kTemporalTileH + 2 * kMotionMaxSearch, kMotionWinW = kTemporalTileW + 2 * kMotionMaxSearch;

// what a pipelined call carries of idc_set_temporal_motion (BatchCall, PipeSlot) and what the launchers take
struct MotionParams { int on; int search; double penalty; };
IDC_TP_FN MotionParams motion_defaults() { return {0, 4, 0.5}; }
// idc_set_temporal_motion's ranges (a NaN fails every comparison and so is outside)
IDC_TP_FN bool motion_params_ok(int on, int search, double penalty) {
    if (on != 0 && on != 1) return false;
    if (search < 0 || search > kMotionMaxSearch) return false;
    if (!(penalty >= 0.0 && penalty <= 1e6)) return false;
    return true;
}

IDC_TP_FN int motion_blocks_y(int H) { return H / kMotionBlock; }
IDC_TP_FN int motion_blocks_x(int W) { return W / kMotionBlock; }
IDC_TP_FN int motion_blocks(int H, int W) { return motion_blocks_y(H) * motion_blocks_x(W); }

// Candidates of search S: index ci = (dy + S) * (2S + 1) + (dx + S), raster order.  The RANK of a candidate is its place in the order
// (dy^2 + dx^2, dy, dx) ascending: rank 0 is (0, 0).
IDC_TP_FN int motion_candidates(int S) { return (2 * S + 1) * (2 * S + 1); }
IDC_TP_FN int motion_cand_dy(int ci, int S) { return ci / (2 * S + 1) - S; }
IDC_TP_FN int motion_cand_dx(int ci, int S) { return ci % (2 * S + 1) - S; }
IDC_TP_FN bool motion_before(int dy0, int dx0, int dy1, int dx1) {        // (dy0, dx0) ranks strictly before (dy1, dx1)
    const int n0 = dy0 * dy0 + dx0 * dx0, n1 = dy1 * dy1 + dx1 * dx1;
    if (n0 != n1) return n0 < n1;
    if (dy0 != dy1) return dy0 < dy1;
    return dx0 < dx1;
}
IDC_TP_FN int motion_rank(int ci, int S) {                                // by counting: (2S + 1)^2 comparisons, once per candidate and workgroup
    const int dy = motion_cand_dy(ci, S), dx = motion_cand_dx(ci, S);
    int r = 0;
    for (int k = 0; k < motion_candidates(S); ++k) r += motion_before(motion_cand_dy(k, S), motion_cand_dx(k, S), dy, dx) ? 1 : 0;
    return r;
}
// a candidate is valid for block (by, bx) iff the displaced block lies wholly inside the plane: nothing is replicated
IDC_TP_FN bool motion_valid(int by, int bx, int dy, int dx, int H, int W) {
    const int j = by * kMotionBlock + dy, i = bx * kMotionBlock + dx;
    return j >= 0 && j + kMotionBlock <= H && i >= 0 && i + kMotionBlock <= W;
}

// The dealing of the search kernel: thread t works for block t / kMotionLanes of the tile (row-major in the tile) and takes the candidates
// ci = t % kMotionLanes + k * kMotionLanes, k = 0 .. motion_rounds - 1, that exist: neighbouring lanes take neighbouring dx of one block, so
// the tile pixel is a broadcast and the window reads are consecutive.
IDC_TP_FN int motion_thread_block(int t) { return t / kMotionLanes; }
IDC_TP_FN int motion_thread_cand(int t, int k) { return t % kMotionLanes + k * kMotionLanes; }
IDC_TP_FN int motion_rounds(int S) { return (motion_candidates(S) + kMotionLanes - 1) / kMotionLanes; }

// scratch of one launch of n frames: the vectors int8 [n, H/8, W/8, 2] (dy, dx), device and pinned
IDC_TP_FN size_t motion_vector_bytes(int n, int H, int W) { return (size_t)n * motion_blocks(H, W) * 2; }

}  // namespace idc

#endif  // IDC_MOTION_H
