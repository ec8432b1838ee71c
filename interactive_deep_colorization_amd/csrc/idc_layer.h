// idc_layer.h -- the span and tiling arithmetic of painted hint layers (idc_set_hints_layer / idc_forward_async_layers; the rule:
// include/ideepcolor.h; the kernel: idc_layer.hip).  Plain C++ that makes no runtime call: the launcher, the batch plan (idc_batch.h), the kernel
// itself and tools/layer_selftest.cpp, which includes it beside idc_batch.h alone, read the same functions.
#ifndef IDC_LAYER_H
#define IDC_LAYER_H

#if defined(__HIPCC__)
#define IDC_LY_FN __host__ __device__ inline
#else
#define IDC_LY_FN inline
#endif

namespace idc {

// One 256-thread workgroup works on cells of ONE image (blockIdx.y), in one of two forms chosen from (lh, lw, H, W) alone:
//   thread form   one thread per net cell, which walks its footprint row-major upwards; a workgroup takes kLayerPasses x 256 cells, 256 at a time.
//   wave form     one wave64 per net cell: lane l takes the footprint's row-major pixels l, l + 64, ... upwards and the 64 lanes fold by halves
//                 (32, 16, ... 1); a workgroup takes kLayerPasses x 4 cells, 4 at a time.
// (kLayerPasses cells per thread or wave: a workgroup fills its sRGB table once and adds its count of hinted cells to the image's with ONE
// atomic -- all counts of a call share a cache line, and one atomic per wave of 64 cells was measured at 0.2 ms of serialised traffic.)
// THE THRESHOLD: a layer takes the wave form iff layer_span_bound(lh, H) * layer_span_bound(lw, W) > kLayerThreadMaxPixels (256): no cell's
// footprint of a thread-form layer holds more than 256 pixels.  1024 x 768 on a 256 net: 4 x 3, thread; 1000 x 700 on 64: 17 x 12 = 204, thread;
// 65 x 16384 on 64: 3 x 256 = 768, wave.
constexpr int kLayerThreads = 256;
constexpr int kLayerWave = 64;
constexpr int kLayerPasses = 4;
constexpr int kLayerThreadMaxPixels = 256;
constexpr int kLayerMaxSide = 16384;

// One image of a layer launch: its [h,w,4] uint8 RGBA layer at byte `off` (a multiple of 4) of the packed run; h == 0: the image has no layer.
struct LayerDesc { long long off; int h, w; };

// The layer indices [lo, hi) whose extent overlaps that of net index i, one axis: l layer pixels stretched over `out` net cells, pixel k covering
// [k * out, (k + 1) * out) and cell i covering [i * l, (i + 1) * l) on the common lattice of l * out steps.  Never empty, inside [0, l).
IDC_LY_FN void layer_span(int i, int l, int out, int& lo, int& hi) {
    lo = (int)(((long long)i * l) / out);
    hi = (int)((((long long)i + 1) * l + out - 1) / out);
}

// no span of the axis is longer than this
IDC_LY_FN int layer_span_bound(int l, int out) {
    if (l <= out) return out % l == 0 ? 1 : 2;
    return l % out == 0 ? l / out : l / out + 2;
}

IDC_LY_FN bool layer_wave_form(int lh, int lw, int H, int W) {
    return (long long)layer_span_bound(lh, H) * layer_span_bound(lw, W) > kLayerThreadMaxPixels;
}

// workgroups of one image: grid.x of a launch is the largest of these over its layers (exact: a workgroup past its own image's count returns)
IDC_LY_FN int layer_blocks(int lh, int lw, int H, int W) {
    const int cells = H * W, per = kLayerPasses * (layer_wave_form(lh, lw, H, W) ? kLayerThreads / kLayerWave : kLayerThreads);
    return (cells + per - 1) / per;
}

}  // namespace idc

#endif  // IDC_LAYER_H
