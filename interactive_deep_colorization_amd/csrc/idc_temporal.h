// idc_temporal.h -- the tile geometry, partial-sum counts and scratch sizes of the motion-adaptive temporal ab filter (idc_set_temporal_filter /
// idc_temporal_apply; the rule: include/ideepcolor.h; the kernels: idc_temporal.hip).  Plain C++ that makes no runtime call: the launchers, the
// batch plan (idc_batch.h), the kernels themselves and tools/temporal_selftest.cpp, which includes it beside idc_batch.h alone, read the same
// functions.
#ifndef IDC_TEMPORAL_H
#define IDC_TEMPORAL_H

#include <stddef.h>

#if defined(__HIPCC__)
#define IDC_TP_FN __host__ __device__ inline
#else
#define IDC_TP_FN inline
#endif

namespace idc {

// temporal_diff_kernel: one 256-thread workgroup per tile of kTemporalTileH x kTemporalTileW net-size pixels of ONE frame (blockIdx.y), tiles
// counted row-major, clipped at the plane's bottom and right edges.  Thread t owns the 4 neighbouring pixels (t / 16, 4 * (t % 16) .. + 3) of
// the tile: W is a multiple of 8 (idc_create), so a thread's 4 pixels are all inside the plane or all outside, and its 32 bytes of g are two
// aligned 16-byte stores.  The LDS tile of e has an apron of kTemporalMaxRadius pixels whatever the call's radius:
// (16 + 6) x (64 + 6) float64 = 12320 bytes, 13 workgroups to a CU by LDS, 8 by waves: the waves bind.
constexpr int kTemporalThreads = 256;
constexpr int kTemporalTileH = 16, kTemporalTileW = 64;
constexpr int kTemporalMaxRadius = 3;
constexpr int kTemporalLdsH = kTemporalTileH + 2 * kTemporalMaxRadius, kTemporalLdsW = kTemporalTileW + 2 * kTemporalMaxRadius;
constexpr int kTemporalMaxFrames = 65535; // frames of one launch: grid.y of the diff kernel (the launchers refuse more, as launch_ycc420 does)
constexpr int kTemporalFlagChunk = 1024;  // the blend kernel keeps the cut flags of this many frames in LDS at a time, int32 each
// temporal_blend_kernel: one thread per item of kTemporalItemPixels neighbouring pixels of one channel: one 16-byte load and store a frame
constexpr int kTemporalItemPixels = 4;

// what a pipelined call carries of idc_set_temporal_filter (BatchCall, PipeSlot) and what the launchers take: two_sigma2 = 2 sigma^2 and
// cut2 = cut^2 are formed once on the host, in float64
struct TemporalParams { int on; double strength, sigma, cut; int radius; };
IDC_TP_FN TemporalParams temporal_defaults() { return {0, 0.6, 4.0, 12.0, 1}; }

IDC_TP_FN int temporal_tiles_y(int H) { return (H + kTemporalTileH - 1) / kTemporalTileH; }
IDC_TP_FN int temporal_tiles_x(int W) { return (W + kTemporalTileW - 1) / kTemporalTileW; }
// tiles of one frame = grid.x of the diff kernel = partial sums of e one frame leaves behind
IDC_TP_FN int temporal_tiles(int H, int W) { return temporal_tiles_y(H) * temporal_tiles_x(W); }
IDC_TP_FN int temporal_partials(int H, int W) { return temporal_tiles(H, W); }
// items of one frame pair of channels and the workgroups of the blend kernel (exact; the last one may be ragged)
IDC_TP_FN long long temporal_items(int H, int W) { return 2ll * H * W / kTemporalItemPixels; }
IDC_TP_FN int temporal_blend_blocks(int H, int W) { return (int)((temporal_items(H, W) + kTemporalThreads - 1) / kTemporalThreads); }

// scratch of one launch of n frames: g float64 [n,H,W], then the partial sums float64 [n, partials]
IDC_TP_FN size_t temporal_g_bytes(int n, int H, int W) { return (size_t)n * H * W * sizeof(double); }
IDC_TP_FN size_t temporal_part_at(int n, int H, int W) { return temporal_g_bytes(n, H, W); }
IDC_TP_FN size_t temporal_scratch_bytes(int n, int H, int W) {
    return temporal_part_at(n, H, W) + (size_t)n * temporal_partials(H, W) * sizeof(double);
}
// the info block of one launch: D float64 [n] at 0, the cut flags int32 [n] behind them
IDC_TP_FN size_t temporal_info_cut_at(int n) { return (size_t)n * sizeof(double); }
IDC_TP_FN size_t temporal_info_bytes(int n) { return (size_t)n * (sizeof(double) + sizeof(int)); }

// idc_set_temporal_filter's ranges (a NaN fails every comparison and so is outside)
IDC_TP_FN bool temporal_params_ok(int on, double strength, double sigma, int radius, double cut) {
    if (on != 0 && on != 1) return false;
    if (!(strength >= 0.0 && strength <= 0.95)) return false;
    if (!(sigma >= 0.5 && sigma <= 100.0)) return false;
    if (radius < 0 || radius > kTemporalMaxRadius) return false;
    if (!(cut == 0.0 || (cut > 0.0 && cut <= 100.0))) return false;
    return true;
}

}  // namespace idc

#endif  // IDC_TEMPORAL_H
