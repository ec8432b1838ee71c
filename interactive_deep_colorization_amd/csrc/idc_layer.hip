// idc_layer.hip -- painted hint layers (idc_set_hints_layer / idc_forward_async_layers; the rule: include/ideepcolor.h): the post-pass that
// composes an RGBA layer of any size under the rectangles the prologue or raster_hints_kernel has already written.  ONE launch for all n images
// of a call (blockIdx.y = image) over the packed layers and their LayerDesc table; the hint planes are read and written in place.
//   grid      exact: dim3(largest workgroup count among the call's layers, n).  A workgroup past its own image's count, or of an image without
//             a layer (h == 0), returns.
//   forms     idc_layer.h: a layer whose footprints hold at most 256 pixels takes one THREAD per cell, any other one WAVE64 per cell.  The
//             choice reads (lh, lw, H, W) and nothing else, and so does the order of the sum.
//   thread    the footprint is walked row-major upwards into one float64 sum per channel that starts at 0.0.  Adjacent cells read adjacent
//             pixels: a row is read pixel by pixel up to the first 16-byte boundary of the packed run, then four pixels a load.
//   wave      lane l takes the footprint's row-major pixels l, l + 64, ... upwards into its own sum from 0.0 (adjacent lanes, adjacent pixels);
//             the 64 lanes fold by halves (32, 16, ... 1), as reveal_hints_kernel's waves do.
//   pixel     A < alpha_min: skipped before any colour arithmetic.  Else (a, b) of raster_hints_kernel's IDC_HINT_RGB colour: the sRGB table in
//             LDS (prologue_kernel's) and linear_to_lab's expressions.
//   cell      covered by a rectangle (mask != 0: a call with a layer has mask_value != 0): left alone.  Else hinted iff cnt >= 1 and
//             255 * cnt >= cover * tot, in integers: ab = the sum / cnt in float64, rounded once to fp32, mask = mask_value.
//   passes    a workgroup takes kLayerPasses batches of 256 (thread form) or 4 (wave form) consecutive cells, so that the table is filled and
//             the count added once per 1024 or 16 cells.
//   cells     the hinted cells of a workgroup are summed over its lanes (folds by halves, then the four wave sums through LDS) and added to
//             the image's count with ONE integer atomicAdd; the caller zeroes cells[n] on the same stream.  No float atomic.
// The sums are float64 with contraction off: an FMA of linear_to_lab's last product into a sum would change a rounding.
#include <hip/hip_runtime.h>

#include "idc_kernels.h"

namespace idc {

namespace {

// idc_colour.hip's linear_to_lab and srgb8_to_linear, the same expressions in the same order: the colour raster_hints_kernel gives a rectangle
__device__ __forceinline__ void layer_linear_to_lab(const double* lin, double& L, double& a, double& b) {
    const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
    const double white[3] = {0.95047, 1.0, 1.08883};
    double g[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double t = (lin[0] * M[i][0] + lin[1] * M[i][1] + lin[2] * M[i][2]) / white[i];
        g[i] = t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0;
    }
    L = 116.0 * g[1] - 16.0; a = 500.0 * (g[0] - g[1]); b = 200.0 * (g[1] - g[2]);
}

__device__ __forceinline__ double layer_srgb_to_linear(double v) { return v > 0.04045 ? pow((v + 0.055) / 1.055, 2.4) : v / 12.92; }

// one RGBA pixel (little-endian word: R in the low byte, A in the high one) into the cell's count and sums
__device__ __forceinline__ void layer_pixel(unsigned px, int alpha_min, const double* tab, int& cnt, double& sa, double& sb) {
#pragma clang fp contract(off)
    if ((int)(px >> 24) < alpha_min) return;
    const double lin[3] = {tab[px & 255u], tab[(px >> 8) & 255u], tab[(px >> 16) & 255u]};
    double L, a, b;
    layer_linear_to_lab(lin, L, a, b);
    ++cnt;
    sa += a; sb += b;
}

__global__ __launch_bounds__(kLayerThreads) void hint_layer_kernel(const unsigned char* __restrict__ layers, const LayerDesc* __restrict__ descs,
                                                                   int H, int W, int alpha_min, int cover, float mask_value,
                                                                   float* __restrict__ ab, float* __restrict__ mask, int* __restrict__ cells) {
#pragma clang fp contract(off)
    __shared__ double tab[256];
    __shared__ int wave_hits[kLayerThreads / kLayerWave];
    const LayerDesc d = descs[blockIdx.y];
    if (d.h == 0 || (int)blockIdx.x >= layer_blocks(d.h, d.w, H, W)) return;       // uniform over the workgroup
    for (int i = threadIdx.x; i < 256; i += kLayerThreads) tab[i] = layer_srgb_to_linear((double)i / 255.0);
    __syncthreads();
    const int HW = H * W, lw = d.w;
    const long long first = d.off >> 2;                                            // the layer's first pixel in the packed run
    const unsigned* __restrict__ run = (const unsigned*)layers;
    float* __restrict__ abi = ab + (size_t)blockIdx.y * 2 * HW;
    float* __restrict__ mi = mask + (size_t)blockIdx.y * HW;
    int hinted = 0;
    const bool wave_form = layer_wave_form(d.h, d.w, H, W);
    for (int pass = 0; pass < kLayerPasses; ++pass) {
        if (!wave_form) {
            const int p = ((int)blockIdx.x * kLayerPasses + pass) * kLayerThreads + (int)threadIdx.x;
            if (p < HW && mi[p] == 0.f) {
                const int y = p / W, x = p - y * W;
                int r0, r1, c0, c1;
                layer_span(y, d.h, H, r0, r1);
                layer_span(x, lw, W, c0, c1);
                int cnt = 0;
                double sa = 0.0, sb = 0.0;
                for (int r = r0; r < r1; ++r) {
                    long long q = first + (long long)r * lw + c0;
                    int c = c0;
                    for (; c < c1 && (q & 3); ++c, ++q) layer_pixel(run[q], alpha_min, tab, cnt, sa, sb);
                    for (; c + 4 <= c1; c += 4, q += 4) {
                        const uint4 v = *(const uint4*)(run + q);
                        layer_pixel(v.x, alpha_min, tab, cnt, sa, sb);
                        layer_pixel(v.y, alpha_min, tab, cnt, sa, sb);
                        layer_pixel(v.z, alpha_min, tab, cnt, sa, sb);
                        layer_pixel(v.w, alpha_min, tab, cnt, sa, sb);
                    }
                    for (; c < c1; ++c, ++q) layer_pixel(run[q], alpha_min, tab, cnt, sa, sb);
                }
                const long long tot = (long long)(r1 - r0) * (c1 - c0);
                if (cnt >= 1 && 255LL * cnt >= (long long)cover * tot) {
                    abi[p] = (float)(sa / (double)cnt);
                    abi[HW + p] = (float)(sb / (double)cnt);
                    mi[p] = mask_value;
                    ++hinted;
                }
            }
        } else {
            const int p = ((int)blockIdx.x * kLayerPasses + pass) * (kLayerThreads / kLayerWave) + (int)(threadIdx.x / kLayerWave), lane = threadIdx.x % kLayerWave;
            if (p < HW && mi[p] == 0.f) {                                              // uniform over the wave
                const int y = p / W, x = p - y * W;
                int r0, r1, c0, c1;
                layer_span(y, d.h, H, r0, r1);
                layer_span(x, lw, W, c0, c1);
                const int fw = c1 - c0;
                const long long tot = (long long)(r1 - r0) * fw;
                int cnt = 0;
                double sa = 0.0, sb = 0.0;
                for (long long t = lane; t < tot; t += kLayerWave) {
                    const int fr = (int)(t / fw), fc = (int)(t - (long long)fr * fw);
                    layer_pixel(run[first + (long long)(r0 + fr) * lw + (c0 + fc)], alpha_min, tab, cnt, sa, sb);
                }
    #pragma unroll
                for (int o = kLayerWave / 2; o > 0; o >>= 1) {
                    sa += __shfl_down(sa, o); sb += __shfl_down(sb, o); cnt += __shfl_down(cnt, o);
                }
                if (lane == 0 && cnt >= 1 && 255LL * cnt >= (long long)cover * tot) {
                    abi[p] = (float)(sa / (double)cnt);
                    abi[HW + p] = (float)(sb / (double)cnt);
                    mi[p] = mask_value;
                    ++hinted;
                }
            }
        }
    }
#pragma unroll
    for (int o = kLayerWave / 2; o > 0; o >>= 1) hinted += __shfl_down(hinted, o);
    if (threadIdx.x % kLayerWave == 0) wave_hits[threadIdx.x / kLayerWave] = hinted;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = wave_hits[0] + wave_hits[1] + wave_hits[2] + wave_hits[3];
        if (total != 0) atomicAdd(&cells[blockIdx.y], total);
    }
}

}  // namespace

hipError_t launch_hint_layers(const unsigned char* layers, const LayerDesc* descs, int n, int max_blocks, int H, int W, int alpha_min, int cover,
                              float mask_value, float* ab, float* mask, int* cells, hipStream_t s) {
    if (layers == nullptr || descs == nullptr || ab == nullptr || mask == nullptr || cells == nullptr) return hipErrorInvalidValue;
    if (n <= 0 || n > 65535 || max_blocks <= 0 || H <= 0 || W <= 0 || (long long)H * W > (1LL << 28)) return hipErrorInvalidValue;
    if (alpha_min < 1 || alpha_min > 255 || cover < 0 || cover > 255 || ((uintptr_t)layers & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hint_layer_kernel, dim3((unsigned)max_blocks, (unsigned)n), dim3(kLayerThreads), 0, s, layers, descs, H, W, alpha_min, cover,
                       mask_value, ab, mask, cells);
    return hipGetLastError();
}

}  // namespace idc
