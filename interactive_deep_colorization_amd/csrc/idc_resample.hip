// idc_resample.hip -- the antialiased down-scaling pre-pass of image ingestion (idc_set_ingest_filter(IDC_FILTER_ANTIALIAS); the rule:
// include/ideepcolor.h).  ONE launch writes the net-size lattice image of every down-scaled image of a call into scratch its handle or slot
// owns; the ingestion kernels of idc_colour.hip then read that scratch as a source of the net's own size, where their bilinear rule is the
// identity, so none of their arithmetic is touched.
//   grid      exact: dim3(largest tile count of the call, H, images).  A workgroup owns `tw` output columns of one output row of one image
//             (tw per image: idc_resample.h); workgroups past an image's own tile count return.
//   pass 1    the tile's windows cover the source columns [c0, c1) (its span).  The lanes stride over the contiguous samples of that span,
//             row by row of the vertical window, so a wavefront's loads are consecutive bytes; each lane keeps up to 16 vertical sums
//             t[x] = sum_y wy * f[y][x] in registers (float64, ascending y) and leaves them in LDS.
//   pass 2    after a barrier, lane o < tw * C owns output sample (column o / C, channel o % C): the ascending sum over its window of t.
//   chunks    the span is staged at most kResampleChunkElems (32 KiB of float64) at a time; tw is chosen so that a span is ONE chunk except for
//             one-column tiles of enormous windows, which walk their chunks in ascending order with the sums carried in registers.
//   weights   r_k = max(0, 1 - |k + .5 - c| / s) and tot = sum r_k are evaluated where they are used, with the rule's own expressions; an axis
//             that is not down-scaled contributes the bilinear rule's two clamped taps with (1 - w) and w.
// Everything is float64 with contraction off; the result is floor(v + .5) clamped to the sample type's range.
#include "idc_kernels.h"

#include "idc_resample.h"

namespace idc {

namespace {

// one output index of one axis: its taps and what their weights need
struct AxisTaps {
    int down;            // 1: the tent window lo .. lo + n - 1; 0: the two taps t0 <= t1
    int lo, n, t0, t1;
    double c, s, tot, w;
};

__device__ __forceinline__ double tent(int k, double c, double s) {
#pragma clang fp contract(off)
    return fmax(0.0, 1.0 - fabs(((double)k + 0.5) - c) / s);
}

__device__ __forceinline__ AxisTaps axis_taps(int i, int in, int out) {
#pragma clang fp contract(off)
    AxisTaps a;
    a.down = in > out;
    a.lo = 0; a.n = 2; a.t0 = 0; a.t1 = 0; a.c = 0.0; a.s = 1.0; a.tot = 1.0; a.w = 0.0;
    if (a.down) {
        int hi;
        resample_window(i, in, out, a.lo, hi);
        a.n = hi - a.lo;
        a.s = (double)in / (double)out;
        a.c = ((double)i + 0.5) * a.s;
        double tot = 0.0;
        for (int k = a.lo; k < hi; ++k) tot += tent(k, a.c, a.s);
        a.tot = tot;
    } else {
        resample_taps2(i, in, out, a.t0, a.t1, a.w);
    }
    return a;
}

// tap j of a: its source index and its weight
__device__ __forceinline__ void axis_tap(const AxisTaps& a, int j, int& k, double& wt) {
#pragma clang fp contract(off)
    if (a.down) {
        k = a.lo + j;
        wt = tent(k, a.c, a.s) / a.tot;
    } else {
        k = j == 0 ? a.t0 : a.t1;
        wt = j == 0 ? 1.0 - a.w : a.w;
    }
}

template <typename T> struct SampleRange;
template <> struct SampleRange<unsigned char> { static constexpr double full = 255.0; };
template <> struct SampleRange<unsigned short> { static constexpr double full = 65535.0; };

template <typename T, int C>
__global__ __launch_bounds__(kResampleThreads) void resample_kernel(const unsigned char* __restrict__ src_base, unsigned char* __restrict__ dst_base,
                                                                    const ResampleJob* __restrict__ jobs, int H, int W) {
#pragma clang fp contract(off)
    constexpr int kPerLane = kResampleChunkElems / kResampleThreads;
    __shared__ double t[kResampleChunkElems];
    const ResampleJob job = jobs[blockIdx.z];
    if ((int)blockIdx.x >= job.tiles) return;            // uniform over the workgroup: this image has fewer tiles than the largest
    const int oy = blockIdx.y, lane = threadIdx.x;
    const int i0 = (int)blockIdx.x * job.tw, i1 = i0 + job.tw < W ? i0 + job.tw : W;
    const T* __restrict__ src = (const T*)(src_base + job.src_off);
    T* __restrict__ dst = (T*)(dst_base + job.dst_off);
    int c0, c1;
    resample_span(i0, i1, job.w, W, c0, c1);
    const AxisTaps ay = axis_taps(oy, job.h, H);         // the same for every lane
    // pass 2's owner of output sample (col, ch); idle lanes take no part in it
    const bool owner = lane < (i1 - i0) * C;
    const int col = i0 + lane / C, ch = lane % C;
    AxisTaps ax = {};
    if (owner) ax = axis_taps(col, job.w, W);
    double v = 0.0;
    const int cols = resample_chunk_cols(C);
    for (int cc0 = c0; cc0 < c1; cc0 += cols) {
        const int cc1 = cc0 + cols < c1 ? cc0 + cols : c1, ne = (cc1 - cc0) * C;
        double acc[kPerLane];
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) acc[j] = 0.0;
        for (int jy = 0; jy < ay.n; ++jy) {
            int ky;
            double wy;
            axis_tap(ay, jy, ky, wy);
            const T* __restrict__ row = src + ((long long)ky * job.w + cc0) * C;
#pragma unroll
            for (int j = 0; j < kPerLane; ++j) {
                const int e = lane + j * kResampleThreads;
                if (e < ne) acc[j] += wy * (double)row[e];
            }
        }
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            const int e = lane + j * kResampleThreads;
            if (e < ne) t[e] = acc[j];
        }
        __syncthreads();
        if (owner) {
            for (int jx = 0; jx < ax.n; ++jx) {
                int kx;
                double wx;
                axis_tap(ax, jx, kx, wx);
                if (kx >= cc0 && kx < cc1) v += wx * t[(kx - cc0) * C + ch];
            }
        }
        __syncthreads();
    }
    if (owner) {
        const double r = floor(v + 0.5);
        dst[((long long)oy * W + col) * C + ch] = (T)(r < 0.0 ? 0.0 : (r > SampleRange<T>::full ? SampleRange<T>::full : r));
    }
}

}  // namespace

hipError_t launch_resample(const void* src_base, void* dst_base, const ResampleJob* jobs, int njobs, int max_tiles, int bits, int channels, int H,
                           int W, hipStream_t s) {
    if (njobs <= 0 || max_tiles <= 0 || jobs == nullptr || H <= 0 || W <= 0 || H > 65535 || njobs > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)max_tiles, (unsigned)H, (unsigned)njobs);
    const unsigned char* sb = (const unsigned char*)src_base;
    unsigned char* db = (unsigned char*)dst_base;
    if (bits == 8 && channels == 3)
        hipLaunchKernelGGL((resample_kernel<unsigned char, 3>), grid, dim3(kResampleThreads), 0, s, sb, db, jobs, H, W);
    else if (bits == 8 && channels == 1)
        hipLaunchKernelGGL((resample_kernel<unsigned char, 1>), grid, dim3(kResampleThreads), 0, s, sb, db, jobs, H, W);
    else if (bits == 16 && channels == 1)
        hipLaunchKernelGGL((resample_kernel<unsigned short, 1>), grid, dim3(kResampleThreads), 0, s, sb, db, jobs, H, W);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace idc
