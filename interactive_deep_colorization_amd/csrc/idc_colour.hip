// idc_colour.hip -- colour space, display and layout helpers around the forward pass: Lab -> RGB, the fused upsample + Lab -> RGB of the display step,
// the global-statistics extractor, image ingestion (uint8 RGB -> net-size Lab, full-resolution RGB from the resident source, linear or joint bilateral), the global hints of
// reference photographs (statistics of m references of individual sizes, the rows of the net's global input), the colour picker's
// gamut map and colour snapping, the PCIe copy kernel and the NCHW <-> NHWC (split) converters.
#include <stdlib.h>
#include <type_traits>

#include "idc_kernels.h"

#include "idc_layout.h"

#include "idc_common.hip.h"

namespace idc {

// ------------------------------------------------------------------------------------------------
// lab_post: skimage.color.lab2rgb -> uint8 -> skimage.color.rgb2lab, per pixel, in float64 (the reference
// computes this on the host in float64 inside every net_forward: colorize_image.py:20-36,196-198,264-267).
// Same constants and operation order as oracle/colorspace.py.  Elementwise, one thread
// per pixel; 65536 pixels per 256x256 image -- latency-, not bandwidth-relevant (it removes ~10 ms of host
// numpy from the per-click path).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lab_post_kernel(const float* __restrict__ Lp, float l_add, const float* __restrict__ ab,
                                                       unsigned char* __restrict__ rgb, double* __restrict__ lab_q,
                                                       long long npix, int HW) {
    const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
    // inverse of M (numpy.linalg.inv of the matrix above, float64)
    const double Mi[3][3] = {{3.240481343200526, -1.5371515162713185, -0.4985363261688878},
                             {-0.9692549499965682, 1.8759900014898907, 0.04155592655829284},
                             {0.05564663913517716, -0.20404133836651123, 1.0573110696453443}};
    const double white[3] = {0.95047, 1.0, 1.08883};
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const long long n = p / HW, r = p - n * HW;
        const double L = (double)Lp[p] + (double)l_add;
        const double a = (double)ab[(n * 2 + 0) * HW + r], b = (double)ab[(n * 2 + 1) * HW + r];
        double f[3];
        f[1] = (L + 16.0) / 116.0;
        f[0] = a / 500.0 + f[1];
        f[2] = fmax(f[1] - b / 200.0, 0.0);                                  // skimage zeroes negative z
        double xyz[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) xyz[i] = (f[i] > 0.2068966 ? f[i] * f[i] * f[i] : (f[i] - 16.0 / 116.0) / 7.787) * white[i];
        unsigned char q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double lin = xyz[0] * Mi[c][0] + xyz[1] * Mi[c][1] + xyz[2] * Mi[c][2];
            double s = lin > 0.0031308 ? 1.055 * pow(fmax(lin, 0.0), 1.0 / 2.4) - 0.055 : 12.92 * lin;
            s = fmin(fmax(s, 0.0), 1.0);
            q[c] = (unsigned char)(s * 255.0);                               // astype('uint8'): truncation
            rgb[p * 3 + c] = q[c];
        }
        if (lab_q != nullptr) {
            double lin[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double v = (double)q[c] / 255.0;
                lin[c] = v > 0.04045 ? pow((v + 0.055) / 1.055, 2.4) : v / 12.92;
            }
            double g[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double t = (lin[0] * M[i][0] + lin[1] * M[i][1] + lin[2] * M[i][2]) / white[i];
                g[i] = t > 0.008856 ? cbrt(t) : 7.787 * t + 16.0 / 116.0;
            }
            lab_q[(n * 3 + 0) * HW + r] = 116.0 * g[1] - 16.0;
            lab_q[(n * 3 + 1) * HW + r] = 500.0 * (g[0] - g[1]);
            lab_q[(n * 3 + 2) * HW + r] = 200.0 * (g[1] - g[2]);
        }
    }
}

hipError_t launch_lab_post(const float* L, float l_add, const float* ab, unsigned char* rgb, double* lab_q, int N,
                           int H, int W, hipStream_t s) {
    const long long npix = (long long)N * H * W;
    const int blocks = grid_blocks(GridTag::lab_post, (npix + 255) / 256, 4096);
    hipLaunchKernelGGL(lab_post_kernel, dim3(blocks), dim3(256), 0, s, L, l_add, ab, rgb, lab_q, npix, H * W);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// pcie_copy: a click's host <-> device transfers as a KERNEL on the forward's own stream (round 5).  One side of (dst, src) is pinned host
// memory mapped into the device's address space, the other is HBM; 16 bytes per lane, one pass.  hipMemcpyAsync hands the same bytes to a copy
// engine on another queue: two cross-queue hand-overs per copy, which at 0.2-0.8 MB weigh more than the bytes (tools/click_host_breakdown.py:
// 768 KB in, 37 us through the copy engine).  Batches keep the copy engines: there the bytes dominate and the compute units have better things to do.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pcie_copy_kernel(uint4* __restrict__ dst, const uint4* __restrict__ src, unsigned n16) {
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n16; i += gridDim.x * 256u) dst[i] = src[i];
}

hipError_t launch_pcie_copy(void* dst, const void* src, size_t bytes, hipStream_t s) {       // bytes % 16 == 0, both 16-byte aligned
    const unsigned n16 = (unsigned)(bytes / 16);
    if (n16 == 0) return hipSuccess;
    const int blocks = grid_blocks(GridTag::pcie_copy, ((long long)n16 + 255) / 256, 1024);
    hipLaunchKernelGGL(pcie_copy_kernel, dim3(blocks), dim3(256), 0, s, (uint4*)dst, (const uint4*)src, n16);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// upsample_lab2rgb: the display step that follows every net_forward in the GUI (ui/gui_draw.py:280-283):
//     ab_win = cv2.resize(output_ab, (win_w, win_h), interpolation=cv2.INTER_CUBIC); lab2rgb(concat(l_win, ab_win)) -> uint8
// and the full-resolution getters (data/colorize_image.py:123-158): scipy.ndimage.zoom(ab, order=1 | 0) + lab2rgb with
// the full-resolution L.  One thread per OUTPUT pixel: interpolate (a, b) from the resident planes, then the float64
// Lab -> sRGB -> uint8 of lab_post_kernel.
//   interp 0: cv2 INTER_CUBIC as resize.cpp computes it for 64F data -- source coordinate fx = (float)((dx + .5) * scale
//             - .5), taps sx-1 .. sx+2 clamped to the image, float32 Keys coefficients with A = -0.75
//             (interpolateCubic), rows first (four horizontal sums in double, left to right), then the vertical sum;
//   interp 1: scipy.ndimage.zoom(order=1): coordinate = dst * (in - 1) / (out - 1), linear, double;
//   interp 2: scipy.ndimage.zoom(order=0): nearest of the same coordinate (floor(c + .5)).
// ------------------------------------------------------------------------------------------------
// Lab -> sRGB clipped to [0, 1], not quantised: s[3].  lab_to_rgb_u8 truncates it to uint8; the colour picker's snap loop converts it straight back.
__device__ __forceinline__ void lab_to_srgb(double L, double a, double b, double* sv) {
    const double Mi[3][3] = {{3.240481343200526, -1.5371515162713185, -0.4985363261688878},
                             {-0.9692549499965682, 1.8759900014898907, 0.04155592655829284},
                             {0.05564663913517716, -0.20404133836651123, 1.0573110696453443}};
    const double white[3] = {0.95047, 1.0, 1.08883};
    double f[3];
    f[1] = (L + 16.0) / 116.0;
    f[0] = a / 500.0 + f[1];
    f[2] = fmax(f[1] - b / 200.0, 0.0);
    double xyz[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) xyz[i] = (f[i] > 0.2068966 ? f[i] * f[i] * f[i] : (f[i] - 16.0 / 116.0) / 7.787) * white[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double lin = xyz[0] * Mi[c][0] + xyz[1] * Mi[c][1] + xyz[2] * Mi[c][2];
        double s = lin > 0.0031308 ? 1.055 * pow(fmax(lin, 0.0), 1.0 / 2.4) - 0.055 : 12.92 * lin;
        sv[c] = fmin(fmax(s, 0.0), 1.0);
    }
}

__device__ __forceinline__ void lab_to_rgb_u8(double L, double a, double b, unsigned char* q) {
    double s[3];
    lab_to_srgb(L, a, b, s);
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = (unsigned char)(s[c] * 255.0);
}

__device__ __forceinline__ void cubic_coeffs(float x, float* c) {       // cv2 interpolateCubic
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

// scipy.ndimage.zoom's corner-aligned source coordinate of output pixel (dy, dx); an output dimension of 1 reads source coordinate 0
__device__ __forceinline__ void zoom_coords(int dy, int dx, int H, int W, int oh, int ow, double& cyy, double& cxx) {
    const double zy = oh > 1 ? (double)(H - 1) / (double)(oh - 1) : 0.0, zx = ow > 1 ? (double)(W - 1) / (double)(ow - 1) : 0.0;
    cyy = dy * zy; cxx = dx * zx;
}

// interp 2: the source pixel zoom(order=0) reads for output pixel (dy, dx)
__device__ __forceinline__ void zoom_nearest(int dy, int dx, int H, int W, int oh, int ow, int& yy, int& xx) {
    double cyy, cxx;
    zoom_coords(dy, dx, H, W, oh, ow, cyy, cxx);
    yy = (int)floor(cyy + 0.5); xx = (int)floor(cxx + 0.5);
    yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy); xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
}

// (a, b) of output pixel (dy, dx) of an [oh,ow] image from the planes pa, pb [H,W]: the three rules above
template <typename S>
__device__ __forceinline__ void interp_ab(const S* __restrict__ pa, const S* __restrict__ pb, int H, int W, int interp, int dy, int dx,
                                          int oh, int ow, double* ab) {
    if (interp == 0) {
        const double sc_x = (double)W / ow, sc_y = (double)H / oh;
        float fx = (float)((dx + 0.5) * sc_x - 0.5), fy = (float)((dy + 0.5) * sc_y - 0.5);
        const int sx = (int)floorf(fx), sy = (int)floorf(fy);
        fx -= sx; fy -= sy;
        float cx[4], cy[4];
        cubic_coeffs(fx, cx); cubic_coeffs(fy, cy);
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const S* src = ch ? pb : pa;
            double rows[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int yy = sy - 1 + k; yy = yy < 0 ? 0 : (yy > H - 1 ? H - 1 : yy);
                double v = 0.0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int xx = sx - 1 + j; xx = xx < 0 ? 0 : (xx > W - 1 ? W - 1 : xx);
                    v += (double)src[(size_t)yy * W + xx] * (double)cx[j];
                }
                rows[k] = v;
            }
            ab[ch] = rows[0] * (double)cy[0] + rows[1] * (double)cy[1] + rows[2] * (double)cy[2] + rows[3] * (double)cy[3];
        }
    } else if (interp == 2) {
        int yy, xx;
        zoom_nearest(dy, dx, H, W, oh, ow, yy, xx);
        ab[0] = (double)pa[(size_t)yy * W + xx]; ab[1] = (double)pb[(size_t)yy * W + xx];
    } else {
        double cyy, cxx;
        zoom_coords(dy, dx, H, W, oh, ow, cyy, cxx);
        int y0 = (int)floor(cyy), x0 = (int)floor(cxx);
        const double ty = cyy - y0, tx = cxx - x0;
        y0 = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0); x0 = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0);
        const int y1 = y0 + 1 > H - 1 ? H - 1 : y0 + 1, x1 = x0 + 1 > W - 1 ? W - 1 : x0 + 1;   // weight 0 there
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            const S* src = ch ? pb : pa;
            const double v00 = (double)src[(size_t)y0 * W + x0], v01 = (double)src[(size_t)y0 * W + x1];
            const double v10 = (double)src[(size_t)y1 * W + x0], v11 = (double)src[(size_t)y1 * W + x1];
            ab[ch] = v00 * ((1.0 - ty) * (1.0 - tx)) + v01 * ((1.0 - ty) * tx) + v10 * (ty * (1.0 - tx)) + v11 * (ty * tx);
        }
    }
}

template <typename S>
__global__ __launch_bounds__(256) void upsample_lab2rgb_kernel(const S* __restrict__ pa, const S* __restrict__ pb, int H, int W,
                                                               int interp, const double* __restrict__ Lout, int oh, int ow,
                                                               unsigned char* __restrict__ rgb) {
    const long long npix = (long long)oh * ow;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const int dy = (int)(p / ow), dx = (int)(p - (long long)dy * ow);
        double ab[2];
        interp_ab(pa, pb, H, W, interp, dy, dx, oh, ow, ab);
        unsigned char q[3];
        lab_to_rgb_u8(Lout[p], ab[0], ab[1], q);
        rgb[p * 3 + 0] = q[0]; rgb[p * 3 + 1] = q[1]; rgb[p * 3 + 2] = q[2];
    }
}

hipError_t launch_upsample_lab2rgb(const void* a_plane, const void* b_plane, int src_f64, int H, int W, int interp, const double* L_out,
                                   int oh, int ow, unsigned char* rgb, hipStream_t s) {
    const long long npix = (long long)oh * ow;
    if (npix <= 0 || interp < 0 || interp > 2) return hipErrorInvalidValue;
    const int blocks = grid_blocks(GridTag::upsample_lab2rgb, (npix + 255) / 256, 8192);
    if (src_f64)
        hipLaunchKernelGGL(upsample_lab2rgb_kernel<double>, dim3(blocks), dim3(256), 0, s, (const double*)a_plane, (const double*)b_plane, H, W,
                           interp, L_out, oh, ow, rgb);
    else
        hipLaunchKernelGGL(upsample_lab2rgb_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)a_plane, (const float*)b_plane, H, W,
                           interp, L_out, oh, ow, rgb);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// global_stats: the reference's global_stats.prototxt on one reference image -- rgb2lab per pixel (float64, the
// skimage formulas of lab_post_kernel), 4x4 average pool of ab (Pooling AVE k4 s4, :101-111), hard assignment of
// each pooled value to its nearest of the 313 centres (NNEncLayer with NN = 1, caffe_traininglayers.py:161-196),
// counted with integer atomics (deterministic); plus the sum of the HSV saturation (BGR2HSVLayer :53-85).
// One thread per 4x4 block.  A 256x256 image is 4096 blocks: latency-, not bandwidth-relevant.
// ------------------------------------------------------------------------------------------------
// linear RGB -> Lab: the second half of skimage's rgb2lab (after the sRGB -> linear step)
__device__ __forceinline__ void linear_to_lab(const double* lin, double& L, double& a, double& b) {
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

__device__ __forceinline__ double srgb_to_linear(double v) { return v > 0.04045 ? pow((v + 0.055) / 1.055, 2.4) : v / 12.92; }

__device__ __forceinline__ double srgb8_to_linear(int q) { return srgb_to_linear((double)q / 255.0); }

__device__ __forceinline__ void rgb8_to_lab(const unsigned char* q, double& L, double& a, double& b) {
    double lin[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) lin[c] = srgb8_to_linear(q[c]);
    linear_to_lab(lin, L, a, b);
}

__global__ __launch_bounds__(256) void global_stats_kernel(const unsigned char* __restrict__ rgb, const float* __restrict__ centres,
                                                           unsigned* __restrict__ counts, double* __restrict__ sat_sum,
                                                           int N, int H, int W) {
    __shared__ float cc[313 * 2];
    for (int i = threadIdx.x; i < 626; i += blockDim.x) cc[i] = centres[i];
    __syncthreads();
    const int h4 = H >> 2, w4 = W >> 2;
    const long long nblk = (long long)N * h4 * w4;
    for (long long blk = (long long)blockIdx.x * blockDim.x + threadIdx.x; blk < nblk; blk += (long long)gridDim.x * blockDim.x) {
        const int bx = (int)(blk % w4), by = (int)((blk / w4) % h4), n = (int)(blk / ((long long)w4 * h4));
        double sa = 0.0, sb = 0.0, ssat = 0.0;
        for (int dy = 0; dy < 4; ++dy)
            for (int dx = 0; dx < 4; ++dx) {
                const unsigned char* q = rgb + (((size_t)n * H + by * 4 + dy) * W + bx * 4 + dx) * 3;
                double L, a, b;
                rgb8_to_lab(q, L, a, b);
                sa += a; sb += b;
                const double r = q[0] / 255.0, g = q[1] / 255.0, bl = q[2] / 255.0;
                const double mx = fmax(r, fmax(g, bl)), mn = fmin(r, fmin(g, bl));
                ssat += mx > 0.0 ? (mx - mn) / mx : 0.0;                     // skimage rgb2hsv saturation
            }
        const float pa = (float)(sa / 16.0), pb = (float)(sb / 16.0);      // Caffe blobs are fp32
        int best = 0;
        float bd = 3.0e38f;
        for (int k = 0; k < 313; ++k) {
            const float da = pa - cc[2 * k], db = pb - cc[2 * k + 1];
            const float d = da * da + db * db;
            if (d < bd) { bd = d; best = k; }
        }
        atomicAdd(&counts[(size_t)n * 313 + best], 1u);
        atomicAdd(&sat_sum[n], ssat);
    }
}

hipError_t launch_global_stats(const unsigned char* rgb, const float* centres, unsigned* counts, double* sat_sum, int N,
                               int H, int W, hipStream_t s) {
    const long long nblk = (long long)N * (H / 4) * (W / 4);
    const int blocks = grid_blocks(GridTag::global_stats, (nblk + 255) / 256, 1024);
    hipLaunchKernelGGL(global_stats_kernel, dim3(blocks), dim3(256), 0, s, rgb, centres, counts, sat_sum, N, H, W);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// image ingestion: what ColorizeImageBase.load_image / set_image do on the host before the first click (data/colorize_image.py:52-77):
// cv2.resize to the net size, rgb2lab, L - l_cent; and the full-resolution getters (:123-158) from the source kept on the device.
// A uint8 channel has 256 possible sRGB -> linear values: each workgroup fills a 256-entry float64 table in LDS with srgb8_to_linear (the
// per-pixel expression, so the table is bit-identical to it) and reads it -- one transcendental (cbrt) per Lab component left per pixel.
//
// Source formats.  Every kernel of this section is ONE template over SrcFmt<T, C>: C interleaved samples of type T per pixel, whose sRGB value is
// v / 255 (uint8) or v / 65535 (uint16).  RGB8 is the colour image [h,w,3]; Gray8 / Gray16 are the greyscale sources (idc_set_image_gray, and
// idc_fullres_rgb / idc_fullres_ab / idc_fullres_rgb16 on a kept one; the rule: include/ideepcolor.h): one plane [h,w] whose sample stands on all
// three channels.  The image goes out as uint8 or uint16 O (16 only from 16).  All formats run the SAME device functions below, the grey ones on
// their one channel and on {t, t, t}, so a uint8 plane gives the bits of the RGB route fed the plane three times, and a uint16 plane of 257 g
// gives the bits of the uint8 plane g wherever nothing is resized (fl(257 g / 65535) == fl(g / 255): the correctly rounded quotient of the same
// real number).  There is no expanded RGB copy of a plane.
//   sRGB -> linear   uint8: the 256-entry LDS table.  uint16: srgb_to_linear per sample -- one float64 pow beside the three of lab_to_srgb on the
//                    way out and the cbrt of linear_to_lab; a 65 536-entry table in global memory would hold the same bits.  A kernel that needs
//                    no table sizes it [1] and skips the barrier; the prologue always fills it, because a hint's colour is uint8 whatever the
//                    samples are.
//   grids            every kernel walks its items in a grid-stride loop.  The launchers own the policy and state it in the kernel's first
//                    template argument (EXACT, item_stride below): RGB launches are capped through grid_blocks under their tag and launch the
//                    EXACT = false form, which strides by the grid; grey launches are exact -- dim3(want) covers the items, a count past 2^31 - 1
//                    is refused (a 16384^2 source is 2.6e5 workgroups) -- and launch the EXACT = true form, one pass.
// ------------------------------------------------------------------------------------------------
template <typename T>
struct Depth {      // a sample or output type: uint8 | uint16
    static constexpr int qmax = sizeof(T) == 1 ? 255 : 65535;       // full scale
    static constexpr double full = (double)qmax;
};

template <typename T, int C>
struct SrcFmt : Depth<T> {
    typedef T sample;
    static constexpr int channels = C;
    static constexpr bool table = sizeof(T) == 1;                   // sRGB -> linear through the LDS table
    static constexpr int group_dwords = C * (int)sizeof(T);         // a group of 4 pixels
};
typedef SrcFmt<unsigned char, 3> RGB8;
typedef SrcFmt<unsigned char, 1> Gray8;
typedef SrcFmt<unsigned short, 1> Gray16;

__device__ __forceinline__ void fill_srgb_table(double* tab) {      // tab: 256 doubles of LDS; ends with a barrier
    for (int i = threadIdx.x; i < 256; i += blockDim.x) tab[i] = srgb8_to_linear(i);
    __syncthreads();
}

template <typename F>
__device__ __forceinline__ void fill_source_table(double* tab) {    // uniform over the kernel: only the uint8 formats have a table (and its barrier)
    if constexpr (F::table) fill_srgb_table(tab);
}

// One channel of colorspace.resize_bilinear_u8's output pixel from its four (clamped) taps, on the lattice 0..QMAX: float64, the same
// expressions in the same order, contraction off (an FMA would change a rounding) -> floor(out + .5) clamped to 0..QMAX
template <int QMAX>
__device__ __forceinline__ int bilinear_q(double f00, double f01, double f10, double f11, double wx, double wy) {
#pragma clang fp contract(off)
    const double top = f00 * (1.0 - wx) + f01 * wx;
    const double bot = f10 * (1.0 - wx) + f11 * wx;
    const double out = top * (1.0 - wy) + bot * wy;
    const double r = floor(out + 0.5);
    return r < 0.0 ? 0 : (r > (double)QMAX ? QMAX : (int)r);
}

// half-pixel source coordinate of output index i: tap0 / tap1 clamped to 0..in-1, w = the weight of tap1
__device__ __forceinline__ void bilinear_taps(int i, int in, int out, int& t0, int& t1, double& w) {
#pragma clang fp contract(off)
    const double s = ((double)i + 0.5) * ((double)in / (double)out) - 0.5;
    const double fl = floor(s);
    w = s - fl;
    const long long i0 = (long long)fl;
    t0 = (int)(i0 < 0 ? 0 : (i0 > in - 1 ? in - 1 : i0));
    t1 = (int)(i0 + 1 < 0 ? 0 : (i0 + 1 > in - 1 ? in - 1 : i0 + 1));
}

// THE net-size pixel: the C quantised channels q of pixel (y, x) of the [H,W] image resized from img [sh,sw,C] -- four clamped taps, gathered
// sample by sample, so no alignment is asked of an image's start.  Every kernel that brings a source to the net size calls this.
template <typename F>
__device__ __forceinline__ void net_sample(const typename F::sample* __restrict__ img, int sh, int sw, int H, int W, int y, int x, int* q) {
    constexpr int C = F::channels;
    int y0, y1, x0, x1;
    double wy, wx;
    bilinear_taps(y, sh, H, y0, y1, wy);
    bilinear_taps(x, sw, W, x0, x1, wx);
    const typename F::sample* p00 = img + ((long long)y0 * sw + x0) * C; const typename F::sample* p01 = img + ((long long)y0 * sw + x1) * C;
    const typename F::sample* p10 = img + ((long long)y1 * sw + x0) * C; const typename F::sample* p11 = img + ((long long)y1 * sw + x1) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) q[c] = bilinear_q<F::qmax>((double)p00[c], (double)p01[c], (double)p10[c], (double)p11[c], wx, wy);
}

// Lab of the source colour q[C]: sRGB -> linear per sample (the table for uint8, srgb_to_linear(q / full scale) for uint16), a grey sample on
// all three channels, then linear_to_lab
template <typename F>
__device__ __forceinline__ void source_lab(const int* q, const double* tab, double& L, double& a, double& b) {
    constexpr int C = F::channels;
    double t[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        if constexpr (F::table) t[c] = tab[q[c]]; else t[c] = srgb_to_linear((double)q[c] / F::full);
    }
    const double lin[3] = {t[0], t[C == 3 ? 1 : 0], t[C == 3 ? 2 : 0]};
    linear_to_lab(lin, L, a, b);
}

// lab_to_rgb_u8 for either depth: (O)(s * full scale), truncation
template <typename O>
__device__ __forceinline__ void lab_to_rgb_q(double L, double a, double b, O* q) {
    double s[3];
    lab_to_srgb(L, a, b, s);
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = (O)(s[c] * Depth<O>::full);
}

// The step of a kernel's walk over its `items`, by the grid policy its LAUNCHER states in the kernel's first template argument.  EXACT = false: the
// grid may be capped (grid_blocks), the kernel strides by it.  EXACT = true: the launcher promises gridDim.x * blockDim.x >= items, one pass; saying
// so at compile time keeps the loop's invariants out of registers (a strided fullres_kernel<., Gray8, u8, double> takes 168 VGPRs, the single
// pass 74: three workgroups per SIMD against six).  A launcher that caps a grid must launch the EXACT = false form: the other would skip items.
template <bool EXACT>
__device__ __forceinline__ long long item_stride(long long items) {
    return EXACT ? items : (long long)gridDim.x * blockDim.x;
}

// The four pixels of a dword group.  unpack_group: the C samples of pixel k < 4 from the group's C * sizeof(T) source dwords; pack_group: the
// three values of pixel k into the group's 3 * sizeof(O) result dwords (zeroed by the caller).
template <typename F>
__device__ __forceinline__ void unpack_group(const unsigned* in, int k, int* q) {
#pragma unroll
    for (int c = 0; c < F::channels; ++c) {
        const int e = k * F::channels + c;
        if constexpr (sizeof(typename F::sample) == 1) q[c] = (int)((in[e >> 2] >> (8 * (e & 3))) & 255u);
        else q[c] = (int)((in[e >> 1] >> (16 * (e & 1))) & 65535u);
    }
}

template <typename O>
__device__ __forceinline__ void pack_group(unsigned* out, int k, const O* o) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int e = k * 3 + c;
        if constexpr (sizeof(O) == 1) out[e >> 2] |= (unsigned)o[c] << (8 * (e & 3)); else out[e >> 1] |= (unsigned)o[c] << (16 * (e & 1));
    }
}

// The grid policy of the four walking launchers.  bits 0 (RGB): capped -- one launch site per grid tag (idc_grid.h), which hands grid_blocks its
// tag and cap and launches the RGB8 form under the tag's name (the `*_rgb_kernel` / `*_prologue_kernel` aliases below).  bits 8 | 16 (grey):
// exact -- `want` workgroups cover the items in one pass, refused past 2^31 - 1.
static bool exact_grid_ok(long long want) { return want <= 0x7fffffffll; }

// the four (source format, output depth) forms times the two plane types: f(F(), O(), S()) launches its kernel<F, O, S>.  bits 0 = RGB8, whose
// only output is uint8; bits 8 | 16 = Gray8 | Gray16.  WITH_RGB = false: a launcher whose RGB launches have sites of their own (the capped ones)
// leaves the RGB8 forms out, so that no exact-grid RGB8 kernel nobody launches is compiled.
template <bool WITH_RGB, typename Fn>
static hipError_t source_forms(int bits, int out_bits, int src_f64, Fn&& f) {
    typedef unsigned char u8;
    typedef unsigned short u16;
    if (WITH_RGB && bits == 0 && out_bits == 8) {
        if constexpr (WITH_RGB) { if (src_f64) f(RGB8(), u8(), double()); else f(RGB8(), u8(), float()); }
    }
    else if (bits == 8 && out_bits == 8) { if (src_f64) f(Gray8(), u8(), double()); else f(Gray8(), u8(), float()); }
    else if (bits == 16 && out_bits == 8) { if (src_f64) f(Gray16(), u8(), double()); else f(Gray16(), u8(), float()); }
    else if (bits == 16 && out_bits == 16) { if (src_f64) f(Gray16(), u16(), double()); else f(Gray16(), u16(), float()); }
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// One thread per net-size pixel of all n images: srcs[i] = image i's [src_h,src_w,C] source; Lp = the resident L plane of the first slot
// ([n][H*W] fp32, gets L - l_cent); net [n,H,W,C] (the sample type) and lab_net [n,C,H,W] f64 -- (L, a, b) of a colour image, L of a plane --
// may be nullptr.
template <bool EXACT, typename F>
__global__ __launch_bounds__(256) void ingest_kernel(const typename F::sample* const* __restrict__ srcs, long long npix, int src_h, int src_w, int H,
                                                     int W, float l_cent, float* __restrict__ Lp, typename F::sample* __restrict__ net,
                                                     double* __restrict__ lab_net) {
    constexpr int C = F::channels;
    __shared__ double tab[F::table ? 256 : 1];
    fill_source_table<F>(tab);
    const long long HW = (long long)H * W;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += item_stride<EXACT>(npix)) {
        const long long i = p / HW, r = p - i * HW;
        const int y = (int)(r / W), x = (int)(r - (long long)y * W);
        int q[C];
        net_sample<F>(srcs[i], src_h, src_w, H, W, y, x, q);
        double L, a, b;
        source_lab<F>(q, tab, L, a, b);
        Lp[p] = (float)(L - (double)l_cent);
        const double lab[3] = {L, a, b};
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (net != nullptr) net[p * C + c] = (typename F::sample)q[c];
            if (lab_net != nullptr) lab_net[(i * C + c) * HW + r] = lab[c];
        }
    }
}

// (the RGB8 form under the name of its launch site's grid tag: one tag, one launch site, one kernel name -- tests/test_grid_cap_cpu.py reads them)
constexpr auto ingest_rgb_kernel = ingest_kernel<false, RGB8>;

hipError_t launch_ingest(int bits, const void* const* srcs, int n, int src_h, int src_w, int H, int W, float l_cent, float* Lp, void* net,
                         double* lab_net, hipStream_t s) {
    const long long npix = (long long)n * H * W;
    if (npix <= 0 || src_h <= 0 || src_w <= 0) return hipErrorInvalidValue;
    const long long want = (npix + 255) / 256;
    if (bits == 0) {
        const int blocks = grid_blocks(GridTag::ingest_rgb, want, 4096);
        hipLaunchKernelGGL(ingest_rgb_kernel, dim3(blocks), dim3(256), 0, s, (const unsigned char* const*)srcs, npix, src_h, src_w, H, W, l_cent, Lp,
                           (unsigned char*)net, lab_net);
        return hipGetLastError();
    }
    if (!exact_grid_ok(want)) return hipErrorInvalidValue;      // grey: dim3(want) covers every item, hence the EXACT form
    return source_forms<false>(bits, bits, 1, [&](auto f, auto, auto) {
        typedef decltype(f) F; typedef typename F::sample T;
        hipLaunchKernelGGL((ingest_kernel<true, F>), dim3((unsigned)want), dim3(256), 0, s, (const T* const*)srcs, npix, src_h, src_w, H, W, l_cent, Lp, (T*)net,
                           lab_net);
    });
}

// One full-resolution output pixel p of an [oh,ow] image from its own source colour q: L = source_lab(q)'s (mask == nullptr) or
// 50 * nearest(mask) / mask_value (0 when mask_value == 0: no hints were ever rasterised), (a, b) interpolated from pa / pb [H,W]
// (nullptr: a = b = 0), then Lab -> RGB at O's depth.
template <typename F, typename O, typename S>
__device__ __forceinline__ void fullres_pixel(long long p, const int* q, const double* tab, const S* __restrict__ pa, const S* __restrict__ pb,
                                              int H, int W, int interp, const float* __restrict__ mask, float mask_value, int oh, int ow, O* out) {
    const int dy = (int)(p / ow), dx = (int)(p - (long long)dy * ow);
    double L, ab[2] = {0.0, 0.0};
    if (mask == nullptr) {
        double a_, b_;
        source_lab<F>(q, tab, L, a_, b_);
    } else if (mask_value != 0.f) {
        int yy, xx;
        zoom_nearest(dy, dx, H, W, oh, ow, yy, xx);
        L = 50.0 * ((double)mask[(size_t)yy * W + xx] / (double)mask_value);
    } else {
        L = 0.0;
    }
    if (pa != nullptr) interp_ab(pa, pb, H, W, interp, dy, dx, oh, ow, ab);
    lab_to_rgb_q<O>(L, ab[0], ab[1], out);
}

// One image.  A thread takes 4 consecutive pixels of the flattened image: C * sizeof(T) aligned dwords in (RGB8 three, Gray8 one, Gray16 two),
// 3 * sizeof(O) aligned dwords out (three or six); src and rgb are 4-byte aligned (device allocations).  The npix % 4 pixels at the end go one
// per thread of workgroup 0 through narrow accesses.
template <bool EXACT, typename F, typename O, typename S>
__global__ __launch_bounds__(256) void fullres_kernel(const typename F::sample* __restrict__ src, int oh, int ow, const S* __restrict__ pa,
                                                      const S* __restrict__ pb, int H, int W, int interp, const float* __restrict__ mask,
                                                      float mask_value, O* __restrict__ rgb) {
    constexpr int C = F::channels, kIn = F::group_dwords, kOut = 3 * (int)sizeof(O);      // dwords per group of 4 pixels
    __shared__ double tab[F::table ? 256 : 1];
    fill_source_table<F>(tab);
    const long long npix = (long long)oh * ow, ngroups = npix >> 2;
    const unsigned* src4 = (const unsigned*)src;
    unsigned* rgb4 = (unsigned*)rgb;
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += item_stride<EXACT>(ngroups)) {
        unsigned in[kIn], out[kOut];
#pragma unroll
        for (int j = 0; j < kIn; ++j) in[j] = src4[g * kIn + j];
#pragma unroll
        for (int j = 0; j < kOut; ++j) out[j] = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int q[C];
            unpack_group<F>(in, k, q);
            O o[3];
            fullres_pixel<F, O, S>(g * 4 + k, q, tab, pa, pb, H, W, interp, mask, mask_value, oh, ow, o);
            pack_group<O>(out, k, o);
        }
#pragma unroll
        for (int j = 0; j < kOut; ++j) rgb4[g * kOut + j] = out[j];
    }
    if (blockIdx.x == 0) {
        const long long p = ngroups * 4 + threadIdx.x;
        if (p < npix) {
            int q[C];
#pragma unroll
            for (int c = 0; c < C; ++c) q[c] = (int)src[p * C + c];
            O o[3];
            fullres_pixel<F, O, S>(p, q, tab, pa, pb, H, W, interp, mask, mask_value, oh, ow, o);
            rgb[p * 3 + 0] = o[0]; rgb[p * 3 + 1] = o[1]; rgb[p * 3 + 2] = o[2];
        }
    }
}

template <typename S> constexpr auto fullres_rgb_kernel = fullres_kernel<false, RGB8, unsigned char, S>;

hipError_t launch_fullres(int bits, const void* src, int oh, int ow, const void* a_plane, const void* b_plane, int src_f64, int H, int W, int interp,
                          const float* mask, float mask_value, void* rgb, int out_bits, hipStream_t s) {
    const long long npix = (long long)oh * ow;
    if (npix <= 0 || interp < 0 || interp > 2 || (((uintptr_t)src | (uintptr_t)rgb) & 3)) return hipErrorInvalidValue;
    const long long want = (((npix + 3) >> 2) + 255) / 256;
    if (bits == 0) {
        if (out_bits != 8) return hipErrorInvalidValue;
        const int blocks = grid_blocks(GridTag::fullres_rgb, want, 8192);
        if (src_f64)
            hipLaunchKernelGGL(fullres_rgb_kernel<double>, dim3(blocks), dim3(256), 0, s, (const unsigned char*)src, oh, ow, (const double*)a_plane,
                               (const double*)b_plane, H, W, interp, mask, mask_value, (unsigned char*)rgb);
        else
            hipLaunchKernelGGL(fullres_rgb_kernel<float>, dim3(blocks), dim3(256), 0, s, (const unsigned char*)src, oh, ow, (const float*)a_plane,
                               (const float*)b_plane, H, W, interp, mask, mask_value, (unsigned char*)rgb);
        return hipGetLastError();
    }
    if (!exact_grid_ok(want)) return hipErrorInvalidValue;      // grey: dim3(want) covers every item, hence the EXACT form
    return source_forms<false>(bits, out_bits, src_f64, [&](auto f, auto o, auto p) {
        typedef decltype(f) F; typedef decltype(o) O; typedef decltype(p) S;
        hipLaunchKernelGGL((fullres_kernel<true, F, O, S>), dim3((unsigned)want), dim3(256), 0, s, (const typename F::sample*)src, oh, ow, (const S*)a_plane,
                           (const S*)b_plane, H, W, interp, mask, mask_value, (O*)rgb);
    });
}

// ------------------------------------------------------------------------------------------------
// pipelined batches (idc_forward_async_rgb / _images / _gray): what idc_set_image_rgb + idc_set_hints per image do before a blocking forward and
// what idc_fullres_rgb per image does after it, each as ONE launch over a slot's packed arrays.  The per-pixel arithmetic is the device functions
// above on the same operands, so a batch equals the blocking route bit for bit.
// Images of INDIVIDUAL sizes come with a table imgs[0..n] (ImgDesc: byte offset of the image in the packed source, pixels in front of it, h, w;
// entry n closes the run with the totals); imgs == nullptr is a uniform run of n images of sh x sw packed back to back, whose entries are
// computed instead of loaded.  An image's bits do not depend on the route, on its position or on its neighbours.  The table is at most
// max_batch + 1 entries and read-only, so it is read where it lies, through the cache.
// ------------------------------------------------------------------------------------------------
// The hint walk: image-local net-size pixel (y, x) against the image's clipped list hints[lo .. hi) walked last first, raster_hints_kernel's pixel
// -> (a, b, mask) of the last covering hint (0, 0, 0 without one).  An RGB hint goes through the LDS table, whose entries are the per-colour
// expression of raster_hints_kernel.
__device__ __forceinline__ void hint_walk(const HintRect* __restrict__ hints, int lo, int hi, int mode, float mask_value, const double* tab, int y,
                                          int x, float& a, float& b, float& m) {
    int hit = -1;
    for (int k = hi - 1; k >= lo; --k) {
        const HintRect h = hints[k];
        if (y >= h.y0 && y <= h.y1 && x >= h.x0 && x <= h.x1) { hit = k; break; }
    }
    a = 0.f; b = 0.f; m = 0.f;
    if (hit >= 0) {
        const HintRect h = hints[hit];
        m = mask_value;
        if (mode == 0) {
            a = h.c0; b = h.c1;
        } else {
            const double hl[3] = {tab[(unsigned char)h.c0], tab[(unsigned char)h.c1], tab[(unsigned char)h.c2]};
            double hL, da, db;
            linear_to_lab(hl, hL, da, db);
            a = (float)da; b = (float)db;
        }
    }
}

// One thread per net-size pixel of all n images, grid-stride.  L: ingest_kernel's pixel of image i = p / (H*W), which starts at byte imgs[i].off
// of the packed source with its own h x w (uniform: at sample i * sh * sw * C); hints: the walk above over hints[offs[i] .. offs[i+1])
// (offs == nullptr: no image has hints).  The three planes are written as coalesced fp32.
// TABLE (the launcher's: imgs != nullptr) is a template argument, so each run form is a kernel of its own from the one body: in a uniform run the
// source size is the same for every lane and the taps' scale stays a scalar outside the loop, and neither form carries the other's code.
template <bool EXACT, bool TABLE, typename F>
__global__ __launch_bounds__(256) void prologue_kernel(const typename F::sample* __restrict__ src, const ImgDesc* __restrict__ imgs, long long npix,
                                                       int sh, int sw, int H, int W, float l_cent, const int* __restrict__ offs,
                                                       const HintRect* __restrict__ hints, int mode, float mask_value, float* __restrict__ Lp,
                                                       float* __restrict__ ab, float* __restrict__ mask) {
    typedef typename F::sample T;
    constexpr int C = F::channels;
    __shared__ double tab[256];
    fill_srgb_table(tab);
    const long long HW = (long long)H * W;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += item_stride<EXACT>(npix)) {
        const long long i = p / HW, r = p - i * HW;
        const int y = (int)(r / W), x = (int)(r - (long long)y * W);
        const T* img;
        int h, w;
        if constexpr (TABLE) {
            const ImgDesc d = imgs[i];
            img = (const T*)((const unsigned char*)src + d.off); h = d.h; w = d.w;
        } else {
            img = src + i * ((long long)sh * sw * C); h = sh; w = sw;
        }
        int q[C];
        net_sample<F>(img, h, w, H, W, y, x, q);
        double L, a_, b_;
        source_lab<F>(q, tab, L, a_, b_);
        const int lo = offs != nullptr ? offs[i] : 0, hi = offs != nullptr ? offs[i + 1] : 0;
        float a, b, m;
        hint_walk(hints, lo, hi, mode, mask_value, tab, y, x, a, b, m);
        Lp[p] = (float)(L - (double)l_cent);
        ab[(i * 2 + 0) * HW + r] = a;
        ab[(i * 2 + 1) * HW + r] = b;
        mask[p] = m;
    }
}

constexpr auto batch_prologue_kernel = prologue_kernel<false, false, RGB8>, ragged_prologue_kernel = prologue_kernel<false, true, RGB8>;      // uniform run | table

hipError_t launch_prologue(int bits, const void* src, const ImgDesc* imgs, int n, int sh, int sw, int H, int W, float l_cent, const int* offs,
                           const HintRect* hints, int mode, float mask_value, float* Lp, float* ab, float* mask, hipStream_t s) {
    const long long npix = (long long)n * H * W;
    if (npix <= 0 || (imgs == nullptr && (bits != 0 || sh <= 0 || sw <= 0)) || (mode != 0 && mode != 1)) return hipErrorInvalidValue;
    const long long want = (npix + 255) / 256;
    if (bits == 0 && imgs == nullptr) {
        const int blocks = grid_blocks(GridTag::batch_prologue, want, 4096);
        hipLaunchKernelGGL(batch_prologue_kernel, dim3(blocks), dim3(256), 0, s, (const unsigned char*)src, imgs, npix, sh, sw, H, W, l_cent, offs, hints,
                           mode, mask_value, Lp, ab, mask);
        return hipGetLastError();
    }
    if (bits == 0) {
        const int blocks = grid_blocks(GridTag::ragged_prologue, want, 4096);
        hipLaunchKernelGGL(ragged_prologue_kernel, dim3(blocks), dim3(256), 0, s, (const unsigned char*)src, imgs, npix, sh, sw, H, W, l_cent, offs, hints,
                           mode, mask_value, Lp, ab, mask);
        return hipGetLastError();
    }
    if (!exact_grid_ok(want)) return hipErrorInvalidValue;      // grey: dim3(want) covers every item, hence the EXACT form
    return source_forms<false>(bits, bits, 1, [&](auto f, auto, auto) {
        typedef decltype(f) F;
        hipLaunchKernelGGL((prologue_kernel<true, true, F>), dim3((unsigned)want), dim3(256), 0, s, (const typename F::sample*)src, imgs, npix, sh, sw, H, W, l_cent, offs,
                           hints, mode, mask_value, Lp, ab, mask);
    });
}

// The last image of imgs[lo .. hi] that starts at or in front of pixel t of the flat run (imgs[lo].first <= t).
__device__ __forceinline__ int image_of_pixel(const ImgDesc* __restrict__ imgs, int lo, int hi, long long t) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (imgs[mid].first <= t) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// fullres_kernel over a packed batch.  Image i starts at pixel first_i of the run, on any residue mod 4, so neither an aligned pitch nor a
// scalar head and tail per image is used: the `total` pixels are taken as ONE flat run from the 4-byte aligned base of the allocation.  A
// thread takes 4 consecutive pixels of that run = fullres_kernel's aligned dwords in and out; a group may straddle images, and every pixel
// finds its own image and position.  Uniform run: one division per group.  Table: the images a workgroup's 1024 pixels of one step touch are
// bracketed by two searches whose argument does not depend on the lane (the same addresses for every lane: scalar loads); a lane then searches
// between the two, which is no step at all unless an image starts inside those 1024 pixels.  From its first pixel on a group carries into the
// next image whenever the current one is used up -- every image has a pixel, so one carry per pixel is enough, and a group of four 1 x 1 images
// carries four times.  Only the total % 4 pixels at the end of the whole run use narrow accesses.  The arrays stay packed, so they travel as one
// contiguous copy each way.  (a, b) = planes 1 and 2 of image i's lab_q [n,3,H,W].
// TABLE is a template argument as in prologue_kernel: the uniform form has no search and keeps oh x ow and its zoom factors scalar, the table form has
// no division; merged behind a run-time branch the RGB8 form ran 1.5 to 3 % behind either.
template <bool EXACT, bool TABLE, typename F, typename O>
__global__ __launch_bounds__(256) void packed_fullres_kernel(const typename F::sample* __restrict__ src, const ImgDesc* __restrict__ imgs, int n,
                                                             long long total, int oh, int ow, const double* __restrict__ lab_q, int H, int W,
                                                             int interp, O* __restrict__ rgb) {
    constexpr int C = F::channels, kIn = F::group_dwords, kOut = 3 * (int)sizeof(O);
    __shared__ double tab[F::table ? 256 : 1];
    fill_source_table<F>(tab);
    const long long HW = (long long)H * W, ngroups = total >> 2;
    const unsigned* src4 = (const unsigned*)src;
    unsigned* rgb4 = (unsigned*)rgb;
    for (long long g0 = (long long)blockIdx.x * blockDim.x; g0 < ngroups; g0 += item_stride<EXACT>(ngroups)) {
        const long long g = g0 + threadIdx.x;
        int i_lo = 0, i_hi = 0;
        if constexpr (TABLE) {
            const long long last = g0 + blockDim.x < ngroups ? g0 + blockDim.x : ngroups;
            i_lo = image_of_pixel(imgs, 0, n - 1, g0 * 4); i_hi = image_of_pixel(imgs, i_lo, n - 1, last * 4 - 1);
        }
        if (g >= ngroups) continue;
        unsigned in[kIn], out[kOut];
#pragma unroll
        for (int j = 0; j < kIn; ++j) in[j] = src4[g * kIn + j];
#pragma unroll
        for (int j = 0; j < kOut; ++j) out[j] = 0u;
        int i, h = oh, w = ow;
        long long p;
        if constexpr (TABLE) {
            i = image_of_pixel(imgs, i_lo, i_hi, g * 4);
            const ImgDesc d = imgs[i];
            p = g * 4 - d.first; h = d.h; w = d.w;
        } else {
            i = (int)((g * 4) / ((long long)oh * ow)); p = g * 4 - i * ((long long)oh * ow);
        }
        long long npix = (long long)h * w;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int q[C];
            unpack_group<F>(in, k, q);
            O o[3];
            const double* pa = lab_q + ((long long)i * 3 + 1) * HW;
            fullres_pixel<F, O, double>(p, q, tab, pa, pa + HW, H, W, interp, (const float*)nullptr, 0.f, h, w, o);
            pack_group<O>(out, k, o);
            if (++p == npix && k < 3) {      // i + 1 <= n - 1: the group's next pixel is in the run
                p = 0; ++i;
                if constexpr (TABLE) { const ImgDesc d = imgs[i]; h = d.h; w = d.w; npix = (long long)h * w; }
            }
        }
#pragma unroll
        for (int j = 0; j < kOut; ++j) rgb4[g * kOut + j] = out[j];
    }
    if (blockIdx.x == 0) {
        const long long t = ngroups * 4 + threadIdx.x;
        if (t < total) {
            int i, h = oh, w = ow;
            long long p;
            if constexpr (TABLE) {
                i = image_of_pixel(imgs, 0, n - 1, t);
                const ImgDesc d = imgs[i];
                p = t - d.first; h = d.h; w = d.w;
            } else {
                i = (int)(t / ((long long)oh * ow)); p = t - i * ((long long)oh * ow);
            }
            int q[C];
#pragma unroll
            for (int c = 0; c < C; ++c) q[c] = (int)src[t * C + c];
            O o[3];
            const double* pa = lab_q + ((long long)i * 3 + 1) * HW;
            fullres_pixel<F, O, double>(p, q, tab, pa, pa + HW, H, W, interp, (const float*)nullptr, 0.f, h, w, o);
            rgb[t * 3 + 0] = o[0]; rgb[t * 3 + 1] = o[1]; rgb[t * 3 + 2] = o[2];
        }
    }
}

constexpr auto batch_fullres_rgb_kernel = packed_fullres_kernel<false, false, RGB8, unsigned char>,      // uniform run
               ragged_fullres_rgb_kernel = packed_fullres_kernel<false, true, RGB8, unsigned char>;      // table

hipError_t launch_packed_fullres(int bits, const void* src, const ImgDesc* imgs, int n, int oh, int ow, long long total, const double* lab_q, int H,
                                 int W, int interp, void* rgb, int out_bits, hipStream_t s) {
    if (imgs == nullptr) total = (long long)n * oh * ow;
    if (n <= 0 || total < n || (imgs == nullptr && (bits != 0 || oh <= 0 || ow <= 0)) || interp < 0 || interp > 2 ||
        (((uintptr_t)src | (uintptr_t)rgb) & 3))
        return hipErrorInvalidValue;
    const long long want = (((total + 3) >> 2) + 255) / 256;
    if (bits == 0 && out_bits != 8) return hipErrorInvalidValue;
    if (bits == 0 && imgs == nullptr) {
        const int blocks = grid_blocks(GridTag::batch_fullres_rgb, want, 8192);
        hipLaunchKernelGGL(batch_fullres_rgb_kernel, dim3(blocks), dim3(256), 0, s, (const unsigned char*)src, imgs, n, total, oh, ow, lab_q, H, W, interp,
                           (unsigned char*)rgb);
        return hipGetLastError();
    }
    if (bits == 0) {
        const int blocks = grid_blocks(GridTag::ragged_fullres_rgb, want, 8192);
        hipLaunchKernelGGL(ragged_fullres_rgb_kernel, dim3(blocks), dim3(256), 0, s, (const unsigned char*)src, imgs, n, total, oh, ow, lab_q, H, W, interp,
                           (unsigned char*)rgb);
        return hipGetLastError();
    }
    if (!exact_grid_ok(want)) return hipErrorInvalidValue;      // grey: dim3(want) covers every item, hence the EXACT form
    return source_forms<false>(bits, out_bits, 1, [&](auto f, auto o, auto) {
        typedef decltype(f) F; typedef decltype(o) O;
        hipLaunchKernelGGL((packed_fullres_kernel<true, true, F, O>), dim3((unsigned)want), dim3(256), 0, s, (const typename F::sample*)src, imgs, n, total, oh, ow, lab_q,
                           H, W, interp, (O*)rgb);
    });
}

// ------------------------------------------------------------------------------------------------
// joint bilateral ab upsampling (Kopf et al. 2007; include/ideepcolor.h states the rule): the net-size ab planes go to the source size under
// the guidance of the source's own L, so that chroma stops at the edges of the full-resolution image instead of being smeared across them.
// ONE kernel for idc_fullres_rgb(IDC_INTERP_JOINT), idc_fullres_ab (any interp) and the source-size epilogue of the pipelined calls.
//   tile      a workgroup owns 32 x 8 output pixels of one image (blockIdx.y), one per thread; workgroups past the image's own tile count exit.
//   weights   the spatial Gaussian is separable and a tile has 8 rows and 32 columns: (8 + 32)(2R + 1) exps per TILE, kept in LDS, instead of
//             (2R + 1)^2 per pixel.  Only the range weight costs an exp per tap.
//   taps      adjacent pixels share nearly all of their taps, so the tile's net-size footprint of (L_lo, a_lo, b_lo) is staged once in LDS as
//             float64: rows j0(first row) - R .. j0(last row) + R, likewise columns.  j0 advances by at most floor(7 H/h) + 1 over a tile,
//             so when the source is no smaller than the net (the use of an UPsampler) the footprint is at most 18 x 42 = 756 cells at R = 4:
//             3 x 6 KB.  A tile whose footprint is larger (h < H or w < W: several net-size pixels per output pixel) reads its taps from
//             global memory.  The choice is uniform over the workgroup and does not change a bit: both branches hand the same float64
//             operands to the same expressions.
//   LDS       18.1 KB footprint + 2 KB sRGB table (uint8 sources) + 2.8 KB weights + 0.8 KB (uint8 out) or 1.5 KB (uint16 out) result bytes:
//             23.7 KB for RGB8, six workgroups (24 waves) per CU by LDS.
//   stores    the tile's result bytes cross LDS; a row of the tile is 96 (uint8) or 192 (uint16) consecutive bytes of the image that start on
//             any residue mod 4 (an image of the packed run starts at element 3 * first; uint16: an even residue), so each row goes out as up
//             to 3 head bytes (lanes 0..2), up to 24 / 48 aligned dwords (lanes stride the row) and up to 3 tail bytes (lanes 3..5): no dword
//             reaches into a neighbouring tile or image.
// imgs == nullptr: n images of sh x sw packed back to back (the same-size batch; n = 1: the blocking calls); else image i starts at pixel
// imgs[i].first of the run, in src and in rgb alike (the table of the run itself: off = first pixels' bytes; ImgDesc::off is not read).
// ------------------------------------------------------------------------------------------------
constexpr int kJointTW = 32, kJointTH = 8, kJointMaxR = 4, kJointMaxTaps = 2 * kJointMaxR + 1, kInterpJoint = 3;
constexpr int kJointCells = (kJointTH + 2 * kJointMaxR + 2) * (kJointTW + 2 * kJointMaxR + 2);

// half-pixel centre of output index i on an axis of scale sc = in / out: u, and the nearest net-size index floor(u + .5)
__device__ __forceinline__ int joint_centre(int i, double sc, double& u) {
#pragma clang fp contract(off)
    u = ((double)i + 0.5) * sc - 0.5;
    return (int)floor(u + 0.5);
}

template <typename F, typename O, typename S>
__global__ __launch_bounds__(256) void joint_fullres_kernel(const typename F::sample* __restrict__ src, const ImgDesc* __restrict__ imgs, int sh,
                                                            int sw, const S* __restrict__ pa, const S* __restrict__ pb, long long plane_stride,
                                                            const float* __restrict__ Lp, float l_cent, int H, int W, int interp, JointParams jp,
                                                            O* __restrict__ rgb, double* __restrict__ ab_out) {
#pragma clang fp contract(off)
    constexpr int C = F::channels;
    __shared__ double tab[F::table ? 256 : 1];
    __shared__ double sL[kJointCells], sA[kJointCells], sB[kJointCells];
    __shared__ double wys[kJointTH][kJointMaxTaps], wxs[kJointTW][kJointMaxTaps];
    __shared__ __attribute__((aligned(4))) unsigned char outb[kJointTH][kJointTW * 3 * sizeof(O)];
    const int img = blockIdx.y;
    long long first;
    if (imgs != nullptr) { const ImgDesc d = imgs[img]; sh = d.h; sw = d.w; first = d.first; }
    else first = (long long)img * sh * sw;
    const int tiles_x = (sw + kJointTW - 1) / kJointTW, tiles_y = (sh + kJointTH - 1) / kJointTH;
    if ((long long)blockIdx.x >= (long long)tiles_x * tiles_y) return;        // uniform over the workgroup: this image has fewer tiles than the largest
    src += first * C;
    const S* ia = pa != nullptr ? pa + (long long)img * plane_stride : nullptr;
    const S* ib = pa != nullptr ? pb + (long long)img * plane_stride : nullptr;
    if (Lp != nullptr) Lp += (long long)img * H * W;
    fill_source_table<F>(tab);
    const int ty0 = (int)(blockIdx.x / tiles_x) * kJointTH, tx0 = (int)(blockIdx.x % tiles_x) * kJointTW;
    const int tx = threadIdx.x & (kJointTW - 1), ty = threadIdx.x / kJointTW;
    const int y = ty0 + ty, x = tx0 + tx;
    const bool valid = y < sh && x < sw;
    const bool joint = interp == kInterpJoint && ia != nullptr;
    const int R = jp.R, NT = 2 * R + 1;
    const double sy = (double)H / (double)sh, sx = (double)W / (double)sw;
    bool staged = false;
    int fj0 = 0, fi0 = 0, fc = 0;
    if (joint) {
        for (int t = threadIdx.x; t < (kJointTH + kJointTW) * kJointMaxTaps; t += 256) {
            const int r = t / kJointMaxTaps, k = t - r * kJointMaxTaps;
            if (k >= NT) continue;
            double u;
            const int c0 = r < kJointTH ? joint_centre(ty0 + r, sy, u) : joint_centre(tx0 + r - kJointTH, sx, u);
            const double dd = (double)(c0 - R + k) - u;
            const double wgt = exp(-(dd * dd) / jp.two_ss);
            if (r < kJointTH) wys[r][k] = wgt; else wxs[r - kJointTH][k] = wgt;
        }
        double u_;
        const int y_last = ty0 + kJointTH - 1 < sh ? ty0 + kJointTH - 1 : sh - 1, x_last = tx0 + kJointTW - 1 < sw ? tx0 + kJointTW - 1 : sw - 1;
        fj0 = joint_centre(ty0, sy, u_) - R; fi0 = joint_centre(tx0, sx, u_) - R;
        const int fr = joint_centre(y_last, sy, u_) + R - fj0 + 1;
        fc = joint_centre(x_last, sx, u_) + R - fi0 + 1;
        staged = (long long)fr * fc <= kJointCells;
        if (staged) {
            for (int c = threadIdx.x; c < fr * fc; c += 256) {
                const int jj = fj0 + c / fc, ii = fi0 + c % fc;
                if (jj < 0 || jj >= H || ii < 0 || ii >= W) continue;        // a tap outside the image is skipped, so its cell is never read
                const long long g = (long long)jj * W + ii;
                sL[c] = (double)Lp[g] + (double)l_cent; sA[c] = (double)ia[g]; sB[c] = (double)ib[g];
            }
        }
        __syncthreads();
    }
    double L = 0.0, a = 0.0, b = 0.0;
    if (valid) {
        int q[C];
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = (int)src[((long long)y * sw + x) * C + c];
        double a_, b_;
        source_lab<F>(q, tab, L, a_, b_);
        if (joint) {
            double u, v;
            const int j0 = joint_centre(y, sy, u), i0 = joint_centre(x, sx, v);
            double num_a = 0.0, num_b = 0.0, den = 0.0;
            for (int kj = 0; kj < NT; ++kj) {
                const int j = j0 - R + kj;
                if (j < 0 || j >= H) continue;
                const double wy = wys[ty][kj];
                for (int ki = 0; ki < NT; ++ki) {
                    const int i = i0 - R + ki;
                    if (i < 0 || i >= W) continue;
                    double Lc, ac, bc;
                    if (staged) {
                        const int c = (j - fj0) * fc + (i - fi0);
                        Lc = sL[c]; ac = sA[c]; bc = sB[c];
                    } else {
                        const long long g = (long long)j * W + i;
                        Lc = (double)Lp[g] + (double)l_cent; ac = (double)ia[g]; bc = (double)ib[g];
                    }
                    const double ws = wy * wxs[tx][ki], dl = L - Lc;
                    const double wt = ws * (exp(-(dl * dl) / jp.two_sr) + 1e-6);       // IDC_JOINT_EPS
                    num_a += wt * ac; num_b += wt * bc; den += wt;
                }
            }
            a = num_a / den; b = num_b / den;
        } else if (ia != nullptr) {
            double ab[2];
            interp_ab(ia, ib, H, W, interp, y, x, sh, sw, ab);
            a = ab[0]; b = ab[1];
        }
        if (ab_out != nullptr) {
            const long long np = (long long)sh * sw, p = (long long)y * sw + x;
            ab_out[first * 2 + p] = a; ab_out[first * 2 + np + p] = b;
        }
    }
    if (rgb == nullptr) return;
    O o[3] = {0, 0, 0};
    if (valid) lab_to_rgb_q<O>(L, a, b, o);
    O* orow = (O*)outb[ty];
    orow[tx * 3 + 0] = o[0]; orow[tx * 3 + 1] = o[1]; orow[tx * 3 + 2] = o[2];
    __syncthreads();
    if (y >= sh) return;
    const int tw = sw - tx0 < kJointTW ? sw - tx0 : kJointTW, nb = tw * 3 * (int)sizeof(O);
    unsigned char* g = (unsigned char*)(rgb + (first + (long long)y * sw + tx0) * 3);
    const int mis = (int)((4 - ((uintptr_t)g & 3)) & 3), head = mis < nb ? mis : nb;
    const int ndw = (nb - head) >> 2, tail = nb - head - ndw * 4;
    const unsigned char* row = outb[ty];
    for (int k = tx; k < ndw; k += kJointTW) {
        const unsigned char* s4 = row + head + k * 4;
        ((unsigned*)(g + head))[k] = (unsigned)s4[0] | ((unsigned)s4[1] << 8) | ((unsigned)s4[2] << 16) | ((unsigned)s4[3] << 24);
    }
    if (tx < head) g[tx] = row[tx];                                                  // lanes 0..2 the head bytes, 3..5 the tail bytes
    else if (tx >= 3 && tx - 3 < tail) g[head + ndw * 4 + tx - 3] = row[head + ndw * 4 + tx - 3];
}

hipError_t launch_joint_fullres(int bits, const void* src, const ImgDesc* imgs, int n, int sh, int sw, long long max_tiles, const void* a_plane,
                                const void* b_plane, int src_f64, long long plane_stride, const float* Lp, float l_cent, int H, int W, int interp,
                                JointParams jp, void* rgb, int out_bits, double* ab_out, hipStream_t s) {
    if (n <= 0 || n > 65535 || src == nullptr || (imgs == nullptr && ((bits != 0 && n != 1) || sh <= 0 || sw <= 0)) || max_tiles <= 0 ||
        max_tiles > 0x7fffffffll || interp < 0 || interp > kInterpJoint || (rgb == nullptr && ab_out == nullptr) ||
        (a_plane == nullptr) != (b_plane == nullptr) || (out_bits == 16 && ((uintptr_t)rgb & 1)))
        return hipErrorInvalidValue;
    if (interp == kInterpJoint && a_plane != nullptr && (Lp == nullptr || jp.R < 1 || jp.R > kJointMaxR || !(jp.two_ss > 0.0) || !(jp.two_sr > 0.0)))
        return hipErrorInvalidValue;
    return source_forms<true>(bits, out_bits, src_f64, [&](auto f, auto o, auto p) {
        typedef decltype(f) F; typedef decltype(o) O; typedef decltype(p) S;
        hipLaunchKernelGGL((joint_fullres_kernel<F, O, S>), dim3((unsigned)max_tiles, (unsigned)n), dim3(256), 0, s, (const typename F::sample*)src, imgs,
                           sh, sw, (const S*)a_plane, (const S*)b_plane, plane_stride, Lp, l_cent, H, W, interp, jp, (O*)rgb, ab_out);
    });
}

// ------------------------------------------------------------------------------------------------
// evaluation batches (idc_reveal_hints / idc_forward_async_eval): the paper's simulated user and its metric around the unchanged forward.
// reveal: a hint's colour = the mean ground-truth ab of the image under the hint's own rectangle, written into the device list that the
// prologue / raster_hints_kernel then reads in IDC_HINT_AB mode.  net_truth: the net-size uint8 pixels the prologue's L comes from, kept as the
// ground truth of a net-size score.  eval_sse: the exact integer sum of squared uint8 differences per image and channel.
// ------------------------------------------------------------------------------------------------
// One workgroup of 256 threads (four wave64s) per kept, clipped rectangle k of hints[0 .. gridDim.x).  Its image: the single [sh,sw,3] source at
// src (imgs == nullptr), or image i of the packed run, offs[i] <= k < offs[i+1].  Every net-size pixel of the rectangle is ingest_kernel's /
// prologue_kernel's pixel (net_sample and source_lab on the same operands), and a and b are summed in float64 in a FIXED order: a thread walks
// its pixels t, t + 256, ... of the rectangle's row-major index upwards, the 64 lanes of a wave fold by halves (32, 16, ... 1), and thread 0
// adds the four wave sums in wave order.  No float atomic: the mean is a function of the image's bytes, (H, W) and the four corners only, not
// of n, the rectangle's place in the list, the slot or the route.  The sum is divided by the pixel count in float64 and rounded once to fp32.
// Cost: the rectangle's AREA per hint (a 9x9 patch: 81 pixels, one step of the workgroup; the whole 256x256 image: 256 steps), against the
// hint walk's one comparison per hint per pixel.  colours (may be nullptr) [.,2] receives the mean at the rectangle's index in the caller's list.
__global__ __launch_bounds__(256) void reveal_hints_kernel(const unsigned char* __restrict__ src, const ImgDesc* __restrict__ imgs,
                                                           const int* __restrict__ offs, int n, int sh, int sw, int H, int W,
                                                           HintRect* __restrict__ hints, const int* __restrict__ orig,
                                                           float* __restrict__ colours) {
    __shared__ double tab[256];
    __shared__ double part[2][4];
    fill_srgb_table(tab);
    const int k = blockIdx.x;
    const unsigned char* img = src;
    if (imgs != nullptr) {
        int lo = 0, hi = n - 1;                     // the last image whose list starts at or in front of k (images without hints repeat an offset)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (offs[mid] <= k) lo = mid; else hi = mid - 1;
        }
        const ImgDesc d = imgs[lo];
        img = src + d.off; sh = d.h; sw = d.w;
    }
    const HintRect r = hints[k];
    const int rw = r.x1 - r.x0 + 1, cnt = (r.y1 - r.y0 + 1) * rw;
    double sa = 0.0, sb = 0.0;
    for (int t = threadIdx.x; t < cnt; t += 256) {
        const int ry = t / rw, y = r.y0 + ry, x = r.x0 + (t - ry * rw);
        int q[3];
        net_sample<RGB8>(img, sh, sw, H, W, y, x, q);
        double L, a, b;
        source_lab<RGB8>(q, tab, L, a, b);
        sa += a; sb += b;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sa += __shfl_down(sa, o); sb += __shfl_down(sb, o); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = sa; part[1][threadIdx.x >> 6] = sb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double ta = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3], tb = ((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
        const float ma = (float)(ta / (double)cnt), mb = (float)(tb / (double)cnt);
        hints[k].c0 = ma; hints[k].c1 = mb;
        if (colours != nullptr) { colours[2 * orig[k] + 0] = ma; colours[2 * orig[k] + 1] = mb; }
    }
}

hipError_t launch_reveal_hints(const unsigned char* src, const ImgDesc* imgs, const int* offs, int n, int src_h, int src_w, int H, int W,
                               HintRect* hints, int n_rects, const int* orig, float* colours, hipStream_t s) {
    if (n_rects <= 0) return hipSuccess;
    if (src == nullptr || hints == nullptr || (colours != nullptr && orig == nullptr)) return hipErrorInvalidValue;
    if (imgs != nullptr ? (offs == nullptr || n <= 0) : (src_h <= 0 || src_w <= 0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(reveal_hints_kernel, dim3(n_rects), dim3(256), 0, s, src, imgs, offs, n, src_h, src_w, H, W, hints, orig, colours);
    return hipGetLastError();
}

// Distribution scores (idc_dist_score / idc_forward_async_dist_score): the ground-truth colour of every cell of the distribution's grid,
// truth [.][2][npix] fp32 (npix = Hd * Wd, H = Hd * S, W = Wd * S), = what reveal_hints_kernel reports for the cell's S x S rectangle, bit for bit:
// the same device functions on the same operands per net-size pixel, and that kernel's summation order for a rectangle of at most 64 pixels --
// its thread t holds pixel t = dy * S + dx alone (0.0 + a), lanes fold by halves, lanes without a pixel and the other three waves add +0.0.  Here
// one thread owns the cell and folds its S * S values by halves itself (t with t + 8, then + 4, + 2, + 1 for S = 4); the sum is divided by the
// count in float64 and rounded once to fp32.  Contraction is off: an FMA of linear_to_lab's last product into a sum would change a rounding.
// blockIdx.y = image: image i of the packed run (imgs != nullptr), or the single [sh,sw,3] source at src.
template <int S>
__global__ __launch_bounds__(256) void dist_truth_kernel(const unsigned char* __restrict__ src, const ImgDesc* __restrict__ imgs, int sh, int sw,
                                                         int H, int W, int Wd, int npix, float* __restrict__ truth) {
#pragma clang fp contract(off)
    __shared__ double tab[256];
    fill_srgb_table(tab);
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= npix) return;
    const unsigned char* img = src;
    if (imgs != nullptr) {
        const ImgDesc d = imgs[blockIdx.y];
        img = src + d.off; sh = d.h; sw = d.w;
    }
    const int cy = c / Wd, cx = c - cy * Wd;
    double va[S * S], vb[S * S];
#pragma unroll
    for (int t = 0; t < S * S; ++t) {
        const int y = cy * S + t / S, x = cx * S + t % S;
        int q[3];
        net_sample<RGB8>(img, sh, sw, H, W, y, x, q);
        double L, a, b;
        source_lab<RGB8>(q, tab, L, a, b);
        va[t] = 0.0 + a; vb[t] = 0.0 + b;
    }
#pragma unroll
    for (int o = S * S / 2; o > 0; o >>= 1)
#pragma unroll
        for (int t = 0; t < o; ++t) { va[t] += va[t + o]; vb[t] += vb[t + o]; }
    float* dst = truth + (size_t)blockIdx.y * 2 * npix + c;
    dst[0] = (float)(va[0] / (double)(S * S));
    dst[npix] = (float)(vb[0] / (double)(S * S));
}

hipError_t launch_dist_truth(const unsigned char* src, const ImgDesc* imgs, int n, int src_h, int src_w, int H, int W, int s, float* truth,
                             hipStream_t st) {
    if (src == nullptr || truth == nullptr || n <= 0 || (s != 1 && s != 4) || H % s || W % s) return hipErrorInvalidValue;
    if (imgs == nullptr && (n != 1 || src_h <= 0 || src_w <= 0)) return hipErrorInvalidValue;
    const int Wd = W / s, npix = (H / s) * Wd;
    const dim3 grid((npix + 255) / 256, n);
    if (s == 4) hipLaunchKernelGGL(dist_truth_kernel<4>, grid, dim3(256), 0, st, src, imgs, src_h, src_w, H, W, Wd, npix, truth);
    else hipLaunchKernelGGL(dist_truth_kernel<1>, grid, dim3(256), 0, st, src, imgs, src_h, src_w, H, W, Wd, npix, truth);
    return hipGetLastError();
}

// The uint8 half of prologue_kernel's pixel (net_sample): rgb_net [n,H,W,3] = cv2.resize of every image to the net size, one thread per pixel.
__global__ __launch_bounds__(256) void ragged_net_truth_kernel(const unsigned char* __restrict__ src, const ImgDesc* __restrict__ imgs, int n, int H,
                                                               int W, unsigned char* __restrict__ rgb_net) {
    const long long HW = (long long)H * W, npix = (long long)n * HW;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += (long long)gridDim.x * blockDim.x) {
        const long long i = p / HW, r = p - i * HW;
        const int y = (int)(r / W), x = (int)(r - (long long)y * W);
        const ImgDesc d = imgs[i];
        int q[3];
        net_sample<RGB8>(src + d.off, d.h, d.w, H, W, y, x, q);
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb_net[p * 3 + c] = (unsigned char)q[c];
    }
}

hipError_t launch_ragged_net_truth(const unsigned char* src, const ImgDesc* imgs, int n, int H, int W, unsigned char* rgb_net, hipStream_t s) {
    const long long npix = (long long)n * H * W;
    if (npix <= 0 || imgs == nullptr) return hipErrorInvalidValue;
    const int blocks = grid_blocks(GridTag::ragged_net_truth, (npix + 255) / 256, 4096);
    hipLaunchKernelGGL(ragged_net_truth_kernel, dim3(blocks), dim3(256), 0, s, src, imgs, n, H, W, rgb_net);
    return hipGetLastError();
}

// sse[i][c] += sum over the pixels of image i of (res - truth)^2 in channel c, for two packed uint8 arrays of the same layout: image i holds the
// bytes [3 * first_i, 3 * first_{i+1}) of both, first_i = imgs[i].first, or i * hw when imgs == nullptr (n net-size images).  blockIdx.y is the
// image.  An image starts on any residue mod 4, so a thread takes the ALIGNED 12-byte group g (three dwords of each array, from their 4-byte
// aligned bases) and masks the bytes outside its image; a byte's channel is its absolute index mod 3 (every image starts at a multiple of 3),
// which inside a 12-byte group is its position mod 3.  A dword that would reach past the arrays' `bytes` is assembled from byte loads.
// Sums: per thread in 64 bits, wave fold, then ONE 64-bit integer atomic add per workgroup and channel into sse (zeroed by the caller on the
// same stream).  Integer addition: exact in any order.  The worst case, 255^2 * 16384^2 = 1.75e19 for one image, is below 2^64 = 1.84e19.
__device__ __forceinline__ unsigned load_dword_bounded(const unsigned char* __restrict__ p, long long d, long long bytes) {
    if (d * 4 + 4 <= bytes) return ((const unsigned*)p)[d];
    unsigned w = 0u;
    for (int s = 0; s < 4; ++s)
        if (d * 4 + s < bytes) w |= (unsigned)p[d * 4 + s] << (8 * s);
    return w;
}

__global__ __launch_bounds__(256) void eval_sse_kernel(const unsigned char* __restrict__ res, const unsigned char* __restrict__ truth,
                                                       const ImgDesc* __restrict__ imgs, long long hw, long long bytes,
                                                       unsigned long long* __restrict__ sse) {
    __shared__ unsigned long long part[3][4];
    const int i = blockIdx.y;
    const long long lo = 3 * (imgs != nullptr ? imgs[i].first : (long long)i * hw);
    const long long hi = 3 * (imgs != nullptr ? imgs[i + 1].first : (long long)(i + 1) * hw);
    const long long g_lo = lo / 12, g_hi = (hi + 11) / 12;
    if (g_lo + (long long)blockIdx.x * 256 >= g_hi) return;                       // uniform over the workgroup: nothing of this image is ours
    unsigned long long acc[3] = {0ull, 0ull, 0ull};
    for (long long g = g_lo + (long long)blockIdx.x * 256 + threadIdx.x; g < g_hi; g += (long long)gridDim.x * 256) {
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const unsigned a = load_dword_bounded(res, g * 3 + d, bytes), b = load_dword_bounded(truth, g * 3 + d, bytes);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const long long at = g * 12 + d * 4 + s;
                const int diff = (int)((a >> (8 * s)) & 255u) - (int)((b >> (8 * s)) & 255u);
                if (at >= lo && at < hi) acc[(d * 4 + s) % 3] += (unsigned long long)(diff * diff);
            }
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc[c] += __shfl_down(acc[c], o);
        if ((threadIdx.x & 63) == 0) part[c][threadIdx.x >> 6] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int c = threadIdx.x;
        atomicAdd(&sse[(size_t)i * 3 + c], part[c][0] + part[c][1] + part[c][2] + part[c][3]);
    }
}

hipError_t launch_eval_sse(const unsigned char* res, const unsigned char* truth, const ImgDesc* imgs, int n, long long hw, long long max_pixels,
                           long long total_pixels, unsigned long long* sse, hipStream_t s) {
    if (n <= 0 || max_pixels <= 0 || total_pixels < max_pixels || sse == nullptr || (((uintptr_t)res | (uintptr_t)truth) & 3))
        return hipErrorInvalidValue;
    const long long groups = (max_pixels * 3 + 11) / 12 + 1;                      // an image's bytes touch at most this many aligned groups
    const int blocks = grid_blocks(GridTag::eval_sse, (groups + 255) / 256, 256);
    hipLaunchKernelGGL(eval_sse_kernel, dim3(blocks, n), dim3(256), 0, s, res, truth, imgs, hw, total_pixels * 3, sse);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// reference-image global hints: global_stats_kernel for m reference photographs of individual sizes, resized inside the kernel (the notebook
// resizes inside get_global_histogram, DemoGlobalHistogramTransfer.ipynb:176-182), and the kernel that turns the counts into the rows
// glob_branch_kernel reads -- so that a reference goes from its uint8 bytes to the net's global input without visiting the host.
// ------------------------------------------------------------------------------------------------
// A workgroup of a reference takes 16 of its 4x4 blocks per step, one lane per net-size pixel (16 consecutive lanes = one block, dy outer, dx
// inner): ingest_kernel's pixel from the reference's own h x w, then Lab and saturation as global_stats_kernel computes them.  The 16 values
// of a block cross LDS and are added in global_stats_kernel's order, so a net-size reference gives that kernel's bits; the search for the nearest
// centre is shared by the block's 16 lanes.  Counts go to an LDS histogram (integer atomics) that is flushed once; the saturation sums stay in
// each block's first lane across steps and are added in lane order at the end, one plain store per workgroup: no float atomic anywhere, nothing
// depends on arrival order.
constexpr int kRefStatsMaxWg = 64;      // workgroups per reference at most (256x256: 4096 blocks = 64 workgroups x 4 steps)

int ref_stats_workgroups(int H, int W) {
    const int groups = ((H >> 2) * (W >> 2) + 15) / 16;
    return groups < kRefStatsMaxWg ? groups : kRefStatsMaxWg;
}

__global__ __launch_bounds__(256) void ref_stats_kernel(const RefDesc* __restrict__ refs, const unsigned char* __restrict__ packed,
                                                        const float* __restrict__ centres, int H, int W, unsigned* __restrict__ counts,
                                                        double* __restrict__ sat_part) {
    __shared__ double tab[256];
    __shared__ double xa[256], xb[256], xs[256];
    __shared__ float cc[313 * 2];
    __shared__ float cd[256];
    __shared__ int ck[256];
    __shared__ unsigned bins[313];
    for (int i = threadIdx.x; i < 626; i += blockDim.x) cc[i] = centres[i];
    for (int i = threadIdx.x; i < 313; i += blockDim.x) bins[i] = 0u;
    fill_srgb_table(tab);
    const int r = blockIdx.y;
    const RefDesc rd = refs[r];
    const unsigned char* img = packed + rd.off;
    const int w4 = W >> 2, nblk = (H >> 2) * w4;
    const int sub = threadIdx.x >> 4, px = threadIdx.x & 15, dy = px >> 2, dx = px & 3;
    double wsat = 0.0;
    for (int g0 = blockIdx.x * 16; g0 < nblk; g0 += gridDim.x * 16) {           // uniform over the workgroup: every lane meets the barriers
        const int blk = g0 + sub;
        const bool live = blk < nblk;
        double a = 0.0, b = 0.0, sat = 0.0;
        if (live) {
            const int by = blk / w4, bx = blk - by * w4;
            int q[3];
            net_sample<RGB8>(img, rd.h, rd.w, H, W, by * 4 + dy, bx * 4 + dx, q);
            double L;
            source_lab<RGB8>(q, tab, L, a, b);
            const double rr = q[0] / 255.0, gg = q[1] / 255.0, bl = q[2] / 255.0;
            const double mx = fmax(rr, fmax(gg, bl)), mn = fmin(rr, fmin(gg, bl));
            sat = mx > 0.0 ? (mx - mn) / mx : 0.0;                             // skimage rgb2hsv saturation
        }
        xa[threadIdx.x] = a; xb[threadIdx.x] = b; xs[threadIdx.x] = sat;
        __syncthreads();
        if (live) {
            // every lane of the block adds the 16 values in the same order, so all 16 hold the same pooled value, and each searches the
            // centres px, px + 16, ...: a sixteenth of global_stats_kernel's serial walk, which is what a reference costs in time
            const int base = threadIdx.x & ~15;
            double sa = 0.0, sb = 0.0, ssat = 0.0;
            for (int k = 0; k < 16; ++k) { sa += xa[base + k]; sb += xb[base + k]; ssat += xs[base + k]; }
            const float pa = (float)(sa / 16.0), pb = (float)(sb / 16.0);      // Caffe blobs are fp32
            int best = 0;
            float bd = 3.0e38f;
            for (int k = px; k < 313; k += 16) {
                const float da = pa - cc[2 * k], db = pb - cc[2 * k + 1];
                const float d = da * da + db * db;
                if (d < bd) { bd = d; best = k; }
            }
            cd[threadIdx.x] = bd; ck[threadIdx.x] = best;
            if (px == 0) wsat += ssat;
        }
        __syncthreads();            // (the next step's writes to xa / xb / xs lie behind this barrier, those to cd / ck behind the next one)
        if (live && px == 0) {
            // the nearest of the 16 candidates, the lowest index among equal distances: what one lane walking 0..312 with `<` finds
            float bd = cd[threadIdx.x];
            int best = ck[threadIdx.x];
            for (int j = 1; j < 16; ++j) {
                const float d = cd[threadIdx.x + j];
                const int k = ck[threadIdx.x + j];
                if (d < bd || (d == bd && k < best)) { bd = d; best = k; }
            }
            atomicAdd(&bins[best], 1u);
        }
    }
    if (px == 0) xs[sub] = wsat;
    __syncthreads();
    for (int i = threadIdx.x; i < 313; i += blockDim.x)
        if (bins[i] != 0u) atomicAdd(&counts[(size_t)r * 313 + i], bins[i]);
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < 16; ++k) s += xs[k];
        sat_part[(size_t)r * gridDim.x + blockIdx.x] = s;
    }
}

hipError_t launch_ref_stats(const RefDesc* refs, int m, const unsigned char* packed, const float* centres, int H, int W, unsigned* counts,
                            double* sat_part, hipStream_t s) {
    if (m <= 0 || m > 65535 || H < 4 || W < 4 || (H & 3) || (W & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ref_stats_kernel, dim3(ref_stats_workgroups(H, W), m), dim3(256), 0, s, refs, packed, centres, H, W, counts, sat_part);
    return hipGetLastError();
}

// Workgroups 0..n-1: one row of the global-input block each, a lane per value; workgroups n..n+m-1 (only where the caller wants them): the
// histogram and mean saturation of one reference.  The divisions are idc_global_histogram's host expressions.
__device__ __forceinline__ float ref_mean_saturation(const double* __restrict__ sat_part, int r, int G, int HW) {
    double s = 0.0;
    for (int k = 0; k < G; ++k) s += sat_part[(size_t)r * G + k];
    return (float)(s / (double)HW);
}

__global__ __launch_bounds__(320) void glob_rows_kernel(const unsigned* __restrict__ counts, const double* __restrict__ sat_part, int G,
                                                        const int* __restrict__ ref_index, int n, int nblk, int HW, float hist_flag,
                                                        int with_sat, float* __restrict__ rows, float* __restrict__ hist,
                                                        float* __restrict__ s_avg) {
    const int t = threadIdx.x;
    if ((int)blockIdx.x < n) {
        const int i = blockIdx.x, r = ref_index[i];
        float v = 0.f;
        if (r >= 0) {
            if (t < 313) v = (float)((double)counts[(size_t)r * 313 + t] / (double)nblk);
            else if (t == 313) v = hist_flag;
            else if (with_sat && t == 314) v = ref_mean_saturation(sat_part, r, G, HW);
            else if (with_sat && t == 315) v = 1.f;
        }
        if (t < kGlobIn) rows[(size_t)i * kGlobIn + t] = v;
    } else {
        const int r = blockIdx.x - n;
        if (t < 313) hist[(size_t)r * 313 + t] = (float)((double)counts[(size_t)r * 313 + t] / (double)nblk);
        else if (t == 313 && s_avg != nullptr) s_avg[r] = ref_mean_saturation(sat_part, r, G, HW);
    }
}

hipError_t launch_glob_rows(const unsigned* counts, const double* sat_part, const int* ref_index, int n, int m, int H, int W, float hist_flag,
                            int with_sat, float* rows, float* hist, float* s_avg, hipStream_t s) {
    const int extra = hist != nullptr ? m : 0;
    if (n < 0 || m < 0 || n + extra <= 0 || (n > 0 && (ref_index == nullptr || rows == nullptr))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(glob_rows_kernel, dim3(n + extra), dim3(320), 0, s, counts, sat_part, ref_stats_workgroups(H, W), ref_index, n,
                       (H >> 2) * (W >> 2), H * W, hist_flag, with_sat, rows, hist, s_avg);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// colour picker: data/lab_gamut.py, which the GUI runs on the host on every mouse press (ui/gui_draw.py:182-183,195-204).  Latency kernels of
// at most a few hundred workgroups: one thread per grid point / per colour, the float64 conversions above.
// ------------------------------------------------------------------------------------------------
// abGrid.update_gamut (lab_gamut.py:66-78): blockIdx.y = map, point p = i * A + j is (a, b) = (-gamut_size + i D, -gamut_size + j D)
__global__ __launch_bounds__(256) void gamut_map_kernel(const double* __restrict__ Lk, int gamut_size, int D, int A, unsigned char* __restrict__ pts,
                                                        unsigned char* __restrict__ masked, unsigned char* __restrict__ mask) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= A * A) return;
    const int i = p / A, j = p - i * A;
    const double L = Lk[blockIdx.y], a = (double)(i * D - gamut_size), b = (double)(j * D - gamut_size);
    unsigned char q[3];
    lab_to_rgb_u8(L, a, b, q);
    double bl, ba, bb;
    rgb8_to_lab(q, bl, ba, bb);
    const double dl = L - bl, da = a - ba, db = b - bb;
    const bool in = sqrt(dl * dl + da * da + db * db) < 1.0;
    const size_t o = (size_t)blockIdx.y * A * A + p;
    if (pts != nullptr) { pts[o * 3 + 0] = q[0]; pts[o * 3 + 1] = q[1]; pts[o * 3 + 2] = q[2]; }
    if (masked != nullptr) { masked[o * 3 + 0] = in ? q[0] : 255; masked[o * 3 + 1] = in ? q[1] : 255; masked[o * 3 + 2] = in ? q[2] : 255; }
    if (mask != nullptr) mask[o] = in ? 1 : 0;
}

hipError_t launch_gamut_map(const double* L, int n, int gamut_size, int D, int A, unsigned char* pts, unsigned char* masked, unsigned char* mask,
                            hipStream_t s) {
    if (n <= 0 || n > 65535 || A <= 0 || A > 32768) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gamut_map_kernel, dim3((A * A + 255) / 256, n), dim3(256), 0, s, L, gamut_size, D, A, pts, masked, mask);
    return hipGetLastError();
}

// snap_ab (lab_gamut.py:28-52).  As there: L is overwritten only inside a round, so the Lab that leaves the loop carries the round-tripped L;
// old_lab aliases conv_lab, so the difference is taken against the value with L already overwritten
__global__ __launch_bounds__(256) void snap_colors_kernel(const double* __restrict__ Lk, const unsigned char* __restrict__ rgb, int n,
                                                          unsigned char* __restrict__ rgb_out, double* __restrict__ lab_out, int* __restrict__ iters) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const unsigned char q[3] = {rgb[k * 3 + 0], rgb[k * 3 + 1], rgb[k * 3 + 2]};
    const double Lin = Lk[k];
    double L, a, b, s[3];
    rgb8_to_lab(q, L, a, b);
    int t = 0;
    while (t < 20) {
        lab_to_srgb(Lin, a, b, s);
        const double lin[3] = {srgb_to_linear(s[0]), srgb_to_linear(s[1]), srgb_to_linear(s[2])};
        double nl, na, nb;
        linear_to_lab(lin, nl, na, nb);
        const double dif = fabs(nl - Lin) + fabs(na - a) + fabs(nb - b);
        L = nl; a = na; b = nb;
        ++t;
        if (dif < 1.0) break;
    }
    lab_to_srgb(L, a, b, s);
    unsigned char o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (unsigned char)rint(s[c] * 255.0);      // np.round: half to even
    if (rgb_out != nullptr) { rgb_out[k * 3 + 0] = o[0]; rgb_out[k * 3 + 1] = o[1]; rgb_out[k * 3 + 2] = o[2]; }
    if (lab_out != nullptr) {
        rgb8_to_lab(o, L, a, b);
        lab_out[k * 3 + 0] = L; lab_out[k * 3 + 1] = a; lab_out[k * 3 + 2] = b;
    }
    if (iters != nullptr) iters[k] = t;
}

hipError_t launch_snap_colors(const double* L, const unsigned char* rgb, int n, unsigned char* rgb_out, double* lab_out, int* iters, hipStream_t s) {
    if (n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(snap_colors_kernel, dim3((n + 255) / 256), dim3(256), 0, s, L, rgb, n, rgb_out, lab_out, iters);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// layout converters (test entry points / activation dumps only -- not on the hot path)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ void nchw_to_nhwc_kernel(const float* __restrict__ src, T* __restrict__ dst, int N, int C, int H, int W,
                                    int Cpad) {
    const long long total = (long long)N * H * W * Cpad;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const long long pix = i / Cpad;
        const long long hw = (long long)H * W;
        const long long n = pix / hw, r = pix - n * hw;
        const float v = c < C ? src[(n * C + c) * hw + r] : 0.f;
        if (sizeof(T) == 4) ((float*)dst)[i] = v;
        else ((__bf16*)dst)[i] = (__bf16)v;
    }
}

__global__ void nhwc_to_nchw_kernel(const void* __restrict__ src, float* __restrict__ dst, int N, int C, int H, int W,
                                    int Cstride, int src_is_bf16) {
    const long long total = (long long)N * C * H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (long long)gridDim.x * blockDim.x) {
        const long long hw = (long long)H * W;
        const long long r = i % hw;
        const int c = (int)((i / hw) % C);
        const long long n = i / (hw * C);
        const long long sidx = (n * hw + r) * Cstride + c;
        float v;
        if (src_is_bf16) v = __uint_as_float((unsigned)((const unsigned short*)src)[sidx] << 16);
        else v = ((const float*)src)[sidx];
        dst[i] = v;
    }
}

hipError_t launch_nchw_to_nhwc(int precision, const float* src, void* dst, int N, int C, int H, int W, int Cpad,
                               hipStream_t s) {
    const long long total = (long long)N * H * W * Cpad;
    const int blocks = grid_blocks(GridTag::nchw_to_nhwc, (total + 255) / 256, 65535);
    if (precision == 1)
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<__bf16>, dim3(blocks), dim3(256), 0, s, src, (__bf16*)dst, N, C, H, W, Cpad);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, dim3(blocks), dim3(256), 0, s, src, (float*)dst, N, C, H, W, Cpad);
    return hipGetLastError();
}

hipError_t launch_nhwc_to_nchw(int src_is_bf16, const void* src, float* dst, int N, int C, int H, int W, int Cstride,
                               hipStream_t s) {
    const long long total = (long long)N * C * H * W;
    const int blocks = grid_blocks(GridTag::nhwc_to_nchw, (total + 255) / 256, 65535);
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3(blocks), dim3(256), 0, s, src, dst, N, C, H, W, Cstride, src_is_bf16);
    return hipGetLastError();
}

// ---- operand-split tensors (IDC_BF16X3 / IDC_BF16X6 / IDC_FP16X3): a pixel is [parts][Cpad] bf16 (fp16), x = part 0 + part 1 (+ part 2) ----
__device__ __forceinline__ unsigned short bf16_rne_bits(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }

// test entry points / activation dumps only
__global__ void split_to_nchw_kernel(const unsigned short* __restrict__ src, float* __restrict__ dst, int N, int C, int H, int W, int Cpad, int parts, int f16) {
    const long long total = (long long)N * C * H * W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long hw = (long long)H * W;
        const long long r = i % hw;
        const int c = (int)((i / hw) % C);
        const long long n = i / (hw * C);
        float v = 0.f;
        for (int p = 0; p < parts; ++p) {
            const unsigned short q = src[((n * hw + r) * parts + p) * Cpad + c];
            v += f16 ? (float)__builtin_bit_cast(_Float16, q) : __uint_as_float((unsigned)q << 16);
        }
        dst[i] = v;
    }
}

hipError_t launch_split_to_nchw(const void* src, float* dst, int N, int C, int H, int W, int Cpad, int parts, int f16, hipStream_t s) {
    const long long total = (long long)N * C * H * W;
    const int blocks = grid_blocks(GridTag::split_to_nchw, (total + 255) / 256, 65535);
    hipLaunchKernelGGL(split_to_nchw_kernel, dim3(blocks), dim3(256), 0, s, (const unsigned short*)src, dst, N, C, H, W, Cpad, parts, f16);
    return hipGetLastError();
}

__global__ void nchw_to_split_kernel(const float* __restrict__ src, unsigned short* __restrict__ dst, int N, int C, int H, int W, int Cpad, int parts, int f16) {
    const long long total = (long long)N * H * W * Cpad;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cpad);
        const long long pix = i / Cpad;
        const long long hw = (long long)H * W;
        const long long n = pix / hw, r = pix - n * hw;
        float v = c < C ? src[(n * C + c) * hw + r] : 0.f;
        for (int p = 0; p < parts; ++p) {
            unsigned short h;
            if (f16) { const _Float16 q = (_Float16)fminf(fmaxf(v, -65504.f), 65504.f); h = __builtin_bit_cast(unsigned short, q); v -= (float)q; }
            else { h = bf16_rne_bits(v); v -= __uint_as_float((unsigned)h << 16); }
            dst[(pix * parts + p) * Cpad + c] = h;
        }
    }
}

hipError_t launch_nchw_to_split(const float* src, void* dst, int N, int C, int H, int W, int Cpad, int parts, int f16, hipStream_t s) {
    const long long total = (long long)N * H * W * Cpad;
    const int blocks = grid_blocks(GridTag::nchw_to_split, (total + 255) / 256, 65535);
    hipLaunchKernelGGL(nchw_to_split_kernel, dim3(blocks), dim3(256), 0, s, src, (unsigned short*)dst, N, C, H, W, Cpad, parts, f16);
    return hipGetLastError();
}


}  // namespace idc
