// idc_temporal.hip -- the motion-adaptive temporal ab filter (idc_set_temporal_filter / idc_temporal_apply; the rule: include/ideepcolor.h;
// the geometry: idc_temporal.h): two launches on the compute stream for all n frames of a call, between the network and the Lab -> RGB epilogue.
//   temporal_diff_kernel   grid exact: dim3(tiles of one frame, n).  Frame f's predecessor plane is frame f - 1 of the same launch, or l_prev
//             for f = 0.  The workgroup fills an LDS tile of e = (l - l_prev)^2 with an apron of R pixels (zero outside the plane, never read
//             there: the window below skips what lies outside), writes g = s exp(-m / 2 sigma^2) for its pixels, m the clipped box mean of e,
//             and ONE partial sum of e over its own pixels: 4 pixels per thread in ascending order, __shfl_xor over the wave from 32 down to
//             1, the four waves through LDS in ascending order, one plain store.  No atomic: the same bits for the same two planes always.
//   temporal_blend_kernel  grid exact: ceil(H W / 2 / 256) workgroups.  Every workgroup first adds each frame's partials in ascending order
//             (thread f takes frame f: at most a few hundred adds, done by every workgroup, so no third launch) and keeps the cut flags in
//             LDS, 1024 frames at a time; workgroup 0 also leaves D and the flags behind.  Then one thread per 4 neighbouring pixels of one
//             channel walks frames 0 .. n-1 with y in registers: the loads of x and g of frame f + 1 are issued before frame f's arithmetic, they do not depend on
//             it.  y is written over x; y_prev and l_prev (channel 0's threads) are left behind for the next launch.
//   Everything is float64 with contraction off; every access is a 16-byte vector access from plain C++, in bounds because W is a multiple of
//   8 and every pointer is 16-byte aligned (the launchers check).
#include <hip/hip_runtime.h>

#include "idc_kernels.h"

namespace idc {

namespace {

__global__ __launch_bounds__(kTemporalThreads) void temporal_diff_kernel(const float* __restrict__ L, const float* __restrict__ l_prev, int have,
                                                                         int H, int W, int R, double strength, double two_sigma2,
                                                                         double* __restrict__ g, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double e[kTemporalLdsH][kTemporalLdsW];
    __shared__ double red[kTemporalThreads / 64];
    const int f = blockIdx.y, tile = blockIdx.x, tiles_x = temporal_tiles_x(W);
    const int j0 = (tile / tiles_x) * kTemporalTileH, i0 = (tile % tiles_x) * kTemporalTileW;
    const size_t hw = (size_t)H * W;
    const int t = threadIdx.x, r = t >> 4, c4 = (t & 15) * 4;
    const int j = j0 + r, i = i0 + c4;
    const bool inside = j < H && i < W;                  // i + 3 < W with it: W is a multiple of 4
    double* __restrict__ gp = g + (size_t)f * hw + (size_t)(inside ? j : 0) * W + (inside ? i : 0);
    if (f == 0 && !have) {                               // no predecessor: the frame passes, D = 0 (uniform over the workgroup)
        if (inside) { ((double2*)gp)[0] = make_double2(0.0, 0.0); ((double2*)gp)[1] = make_double2(0.0, 0.0); }
        if (t == 0) part[(size_t)f * gridDim.x + tile] = 0.0;
        return;
    }
    const float* __restrict__ cur = L + (size_t)f * hw;
    const float* __restrict__ prev = f > 0 ? L + (size_t)(f - 1) * hw : l_prev;
    const int lw = kTemporalTileW + 2 * R, cells = (kTemporalTileH + 2 * R) * lw;
    for (int idx = t; idx < cells; idx += kTemporalThreads) {
        const int jj = idx / lw, ii = idx - jj * lw;
        const int gj = j0 - R + jj, gi = i0 - R + ii;
        double v = 0.0;
        if (gj >= 0 && gj < H && gi >= 0 && gi < W) {
            const double d = (double)cur[(size_t)gj * W + gi] - (double)prev[(size_t)gj * W + gi];
            v = d * d;
        }
        e[jj][ii] = v;
    }
    __syncthreads();
    double own = 0.0;
    if (inside) {
        double gv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            own += e[r + R][c4 + k + R];
            double sum = 0.0;
            int taps = 0;
            for (int dj = -R; dj <= R; ++dj) {
                if (j + dj < 0 || j + dj >= H) continue;
                for (int di = -R; di <= R; ++di) {
                    if (i + k + di < 0 || i + k + di >= W) continue;
                    sum += e[r + R + dj][c4 + k + R + di];
                    ++taps;
                }
            }
            const double m = sum / (double)taps;
            gv[k] = strength * exp(-m / two_sigma2);
        }
        ((double2*)gp)[0] = make_double2(gv[0], gv[1]);
        ((double2*)gp)[1] = make_double2(gv[2], gv[3]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) own += __shfl_xor(own, off);
    if ((t & 63) == 0) red[t >> 6] = own;
    __syncthreads();
    if (t == 0) part[(size_t)f * gridDim.x + tile] = ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ float blend1(float x, float yp, double g) {
#pragma clang fp contract(off)
    const double d = (double)yp - (double)x;
    const double gd = g * d;
    return (float)((double)x + gd);
}

__global__ __launch_bounds__(kTemporalThreads) void temporal_blend_kernel(float* __restrict__ x, const double* __restrict__ g,
                                                                          const double* __restrict__ part, const float* __restrict__ L,
                                                                          float* __restrict__ y_prev, float* __restrict__ l_prev, int have, int n,
                                                                          int H, int W, int P, double cut2, double* __restrict__ D,
                                                                          int* __restrict__ cut) {
#pragma clang fp contract(off)
    __shared__ int s_cut[kTemporalFlagChunk];
    const size_t hw = (size_t)H * W;
    const int t = threadIdx.x;
    const size_t quarter = hw / kTemporalItemPixels;     // items of one channel
    const size_t item = (size_t)blockIdx.x * kTemporalThreads + t;
    const bool active = item < 2 * quarter;              // (no early return: the barriers below are the whole workgroup's)
    const int ch = item >= quarter ? 1 : 0;
    const size_t pix = active ? (item - (ch ? quarter : 0)) * kTemporalItemPixels : 0;
    float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active && have) y = *(const float4*)(y_prev + (size_t)ch * hw + pix);
    float* __restrict__ xp = x + (size_t)ch * hw + pix;
    const double* __restrict__ gq = g + pix;
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    double2 g0 = make_double2(0.0, 0.0), g1 = g0;
    if (active) { xv = *(const float4*)xp; g0 = ((const double2*)gq)[0]; g1 = ((const double2*)gq)[1]; }
    for (int f0 = 0; f0 < n; f0 += kTemporalFlagChunk) {         // the flags of kTemporalFlagChunk frames at a time: any n
        const int m = n - f0 < kTemporalFlagChunk ? n - f0 : kTemporalFlagChunk;
        for (int k = t; k < m; k += kTemporalThreads) {
            const int f = f0 + k;
            double sum = 0.0;
            for (int p = 0; p < P; ++p) sum += part[(size_t)f * P + p];
            const double d = sum / (double)hw;
            const int c = ((f == 0 && !have) || (cut2 > 0.0 && d > cut2)) ? 1 : 0;
            s_cut[k] = c;
            if (blockIdx.x == 0) { D[f] = d; cut[f] = c; }
        }
        __syncthreads();
        if (active) {
            for (int k = 0; k < m; ++k) {
                float4 xn = xv;
                double2 n0 = g0, n1 = g1;
                if (f0 + k + 1 < n) {                        // the next frame's loads: independent of y
                    xn = *(const float4*)(xp + 2 * hw);
                    n0 = ((const double2*)(gq + hw))[0]; n1 = ((const double2*)(gq + hw))[1];
                }
                if (s_cut[k]) y = xv;
                else y = make_float4(blend1(xv.x, y.x, g0.x), blend1(xv.y, y.y, g0.y), blend1(xv.z, y.z, g1.x), blend1(xv.w, y.w, g1.y));
                *(float4*)xp = y;
                xp += 2 * hw; gq += hw;
                xv = xn; g0 = n0; g1 = n1;
            }
        }
        __syncthreads();                                 // the flags are read: the next chunk may overwrite them
    }
    if (!active) return;
    *(float4*)(y_prev + (size_t)ch * hw + pix) = y;
    if (ch == 0) *(float4*)(l_prev + pix) = *(const float4*)(L + (size_t)(n - 1) * hw + pix);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

hipError_t launch_temporal_diff(const float* L, const float* l_prev, int have, int n, int H, int W, int radius, double strength, double sigma,
                                double* g, double* part, hipStream_t s) {
    if (!L || !l_prev || !g || !part) return hipErrorInvalidValue;
    if (n <= 0 || n > kTemporalMaxFrames || H <= 0 || W <= 0 || (H % 8) || (W % 8)) return hipErrorInvalidValue;
    if (radius < 0 || radius > kTemporalMaxRadius || !(sigma > 0.0)) return hipErrorInvalidValue;
    if (!aligned16(L) || !aligned16(l_prev) || !aligned16(g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(temporal_diff_kernel, dim3((unsigned)temporal_tiles(H, W), (unsigned)n), dim3(kTemporalThreads), 0, s, L, l_prev, have ? 1 : 0,
                       H, W, radius, strength, 2.0 * sigma * sigma, g, part);
    return hipGetLastError();
}

hipError_t launch_temporal_blend(float* x, const double* g, const double* part, const float* L, float* y_prev, float* l_prev, int have, int n,
                                 int H, int W, double cut, double* D, int* cut_flags, hipStream_t s) {
    if (!x || !g || !part || !L || !y_prev || !l_prev || !D || !cut_flags) return hipErrorInvalidValue;
    if (n <= 0 || n > kTemporalMaxFrames || H <= 0 || W <= 0 || (H % 8) || (W % 8)) return hipErrorInvalidValue;
    if (!aligned16(x) || !aligned16(g) || !aligned16(L) || !aligned16(y_prev) || !aligned16(l_prev)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(temporal_blend_kernel, dim3((unsigned)temporal_blend_blocks(H, W)), dim3(kTemporalThreads), 0, s, x, g,
                       part, L, y_prev, l_prev, have ? 1 : 0, n, H, W, temporal_partials(H, W), cut * cut, D, cut_flags);
    return hipGetLastError();
}

}  // namespace idc
