// idc_resample.h -- the window and tiling arithmetic of the antialiased down-scaling pre-pass (idc_set_ingest_filter(IDC_FILTER_ANTIALIAS);
// the rule: include/ideepcolor.h; the kernel: idc_resample.hip).  Plain C++ that makes no runtime call: the launcher, the batch plan
// (idc_batch.h) and tools/resample_selftest.cpp, which includes it alone, read the same functions, and so does the kernel itself.
#ifndef IDC_RESAMPLE_H
#define IDC_RESAMPLE_H

#if defined(__HIPCC__)
#define IDC_RS_FN __host__ __device__ inline
#else
#define IDC_RS_FN inline
#endif

namespace idc {

// One 256-thread workgroup per (image, output row, tile of tw output columns).  The vertical sums t[x] of the source columns a tile's windows
// cover (its span) are staged in LDS as float64, at most kResampleChunkElems of them at a time: THE LDS BUDGET IS 32 KiB per workgroup
// (4096 doubles; five workgroups per CU by LDS).  tw is the largest tile width whose span fits the budget in one piece; a tile of ONE column
// whose window alone is larger (s > 682 with three channels, s > 2047 with one) walks its span in ascending chunks of the budget's size.
constexpr int kResampleThreads = 256;
constexpr int kResampleChunkElems = 4096;
constexpr int kResampleLdsBudget = kResampleChunkElems * 8;
constexpr int kResampleMaxTW = 64;                 // tw * channels <= 192 lanes take one output sample each in the horizontal pass

// One image of a pre-pass launch: the [h,w,C] source at byte src_off of the launch's source base, the [H,W,C] result at byte dst_off of its
// destination base, and the tiling resample_tiling chose for it.
struct ResampleJob { long long src_off, dst_off; int h, w, tw, tiles; };

// the image is brought to the net size by the tent filter (it is down-scaled on an axis); otherwise today's bilinear expressions serve it
IDC_RS_FN bool resample_applies(int h, int w, int H, int W) { return h > H || w > W; }

// s > 1: the taps lo .. hi-1 of output index i.  Never empty, inside [0, in), at most ceil(2 s) + 1 of them.
IDC_RS_FN void resample_window(int i, int in, int out, int& lo, int& hi) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double s = (double)in / (double)out;
    const double c = ((double)i + 0.5) * s;
    const int l = (int)(c - s + 0.5), h = (int)(c + s + 0.5);
    lo = l < 0 ? 0 : l;
    hi = h > in ? in : h;
}

// s <= 1: the two clamped taps of the bilinear rule, w = the weight of t1 (bilinear_taps of idc_colour.hip, the same expressions)
IDC_RS_FN void resample_taps2(int i, int in, int out, int& t0, int& t1, double& w) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double s = ((double)i + 0.5) * ((double)in / (double)out) - 0.5;
    const double fl = (double)(long long)s - ((double)(long long)s > s ? 1.0 : 0.0);      // floor(s)
    w = s - fl;
    const long long i0 = (long long)fl;
    t0 = (int)(i0 < 0 ? 0 : (i0 > in - 1 ? in - 1 : i0));
    t1 = (int)(i0 + 1 < 0 ? 0 : (i0 + 1 > in - 1 ? in - 1 : i0 + 1));
}

// the source indices [c0, c1) the output indices [i0, i1) of one axis read (both rules are monotone in i)
IDC_RS_FN void resample_span(int i0, int i1, int in, int out, int& c0, int& c1) {
    if (in > out) {
        int lo, hi;
        resample_window(i0, in, out, c0, hi);
        resample_window(i1 - 1, in, out, lo, c1);
    } else {
        int t0, t1;
        double w;
        resample_taps2(i0, in, out, c0, t1, w);
        resample_taps2(i1 - 1, in, out, t0, t1, w);
        c1 = t1 + 1;
    }
}

IDC_RS_FN int resample_chunk_cols(int channels) { return kResampleChunkElems / channels; }

// LDS bytes of a workgroup: the staged part of the span, whatever the image
IDC_RS_FN int resample_lds_bytes(int channels) { return resample_chunk_cols(channels) * channels * 8; }

IDC_RS_FN int resample_tile_count(int out, int tw) { return (out + tw - 1) / tw; }

// The tile width of an axis with `in` source and `out` net columns: a tw <= min(out, kResampleMaxTW) for which the span of EVERY tile fits
// resample_chunk_cols; 1 when not even one column's does.  A span of tw columns is at most (tw - 1) s + 2 s + 2 source columns wide (s = in /
// out, or 1 when the axis is not down-scaled): the search starts at the largest tw that bound admits and steps down while a span fails.
inline int resample_tile_width(int in, int out, int channels) {
    const int cols = resample_chunk_cols(channels);
    const double s = in > out ? (double)in / (double)out : 1.0;
    int tw = out < kResampleMaxTW ? out : kResampleMaxTW;
    const double bound = ((double)cols - 2.0 * s - 2.0) / s + 1.0;
    if (bound < (double)tw) tw = bound < 1.0 ? 1 : (int)bound;
    for (; tw > 1; --tw) {
        bool fits = true;
        for (int i0 = 0; i0 < out && fits; i0 += tw) {
            int c0, c1;
            resample_span(i0, i0 + tw < out ? i0 + tw : out, in, out, c0, c1);
            fits = c1 - c0 <= cols;
        }
        if (fits) break;
    }
    return tw;
}

inline ResampleJob resample_job(long long src_off, long long dst_off, int h, int w, int W, int channels) {
    ResampleJob j;
    j.src_off = src_off; j.dst_off = dst_off; j.h = h; j.w = w;
    j.tw = resample_tile_width(w, W, channels);
    j.tiles = resample_tile_count(W, j.tw);
    return j;
}

}  // namespace idc

#endif  // IDC_RESAMPLE_H
