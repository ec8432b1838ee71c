// idc_ycc.hip -- YCbCr 4:2:0 output planes (idc_set_batch_output / idc_fullres_ycc / idc_rgb_to_ycc420; the rule: include/ideepcolor.h): the
// post-pass that reads the packed uint8 RGB results an epilogue wrote and writes each image's plane block.  ONE launch for all n images of a
// call (blockIdx.y = image) over the YccDesc table; the RGB is only read, so the planes are a pure function of the RGB image whatever route,
// interp, source format or hint feature made it.
//   grid      exact: dim3(largest workgroup count among the call's images, n).  A workgroup past its own image's count returns.
//   thread    one strip (idc_ycc.h): 2 rows x 8 pixels = 4 chroma blocks, clipped at the image's right and bottom edges: 2 x 24 bytes in,
//             2 x 8 bytes of Y and 4 + 4 bytes of chroma out.  Adjacent threads take adjacent strips of a chroma row: adjacent bytes.
//   loads     an image starts at any byte of the packed run and a row of odd width anywhere: a full row of a strip is read as the 6 or 7
//             ALIGNED dwords that hold its 24 bytes and shifted into place.  A clipped strip, and the last strip of an image (whose closing
//             dword may reach past the image's own bytes), reads bytes.
//   stores    store_run: bytes up to the first 4-byte boundary, dwords, bytes again.  Every run is exactly the bytes the strip owns in ONE row
//             of ONE plane: no store reaches into a neighbouring row, plane or image.  I420 writes 4 + 4 chroma bytes into two planes, NV12 the
//             same 8 interleaved into one: one path, the layout decides the run.
//   integers  16.16 fixed point in int32 (the largest numerator, 4 pixels: 6.8e7); no clamp, the rule's ranges hold by construction.
#include <hip/hip_runtime.h>

#include "idc_kernels.h"

namespace idc {

namespace {

// `count` (0..8) bytes of v, low byte first, to p
__device__ __forceinline__ void store_run(unsigned char* p, unsigned long long v, int count) {
    int k = 0;
    for (; k < count && ((uintptr_t)(p + k) & 3); ++k) p[k] = (unsigned char)(v >> (8 * k));
    for (; k + 4 <= count; k += 4) *(unsigned*)(p + k) = (unsigned)(v >> (8 * k));
    for (; k < count; ++k) p[k] = (unsigned char)(v >> (8 * k));
}

// pixels 0..nx-1 of the row at `row` into px[] as 0x00BBGGRR; the others 0.  `wide`: all 8 are there and the row's closing dword is the image's own
__device__ __forceinline__ void load_row(const unsigned char* __restrict__ row, int nx, bool wide, unsigned* px) {
    if (wide) {
        const int sh = (int)((uintptr_t)row & 3);
        const unsigned* __restrict__ q = (const unsigned*)(row - sh);
        unsigned d[7];
#pragma unroll
        for (int i = 0; i < 6; ++i) d[i] = q[i];
        d[6] = sh ? q[6] : 0u;
        unsigned r[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) r[i] = (unsigned)(((((unsigned long long)d[i + 1]) << 32) | d[i]) >> (8 * sh));
#pragma unroll
        for (int x = 0; x < kYccStripPixels; ++x) {
            unsigned v = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int k = 3 * x + c;
                v |= ((r[k >> 2] >> (8 * (k & 3))) & 255u) << (8 * c);
            }
            px[x] = v;
        }
        return;
    }
#pragma unroll
    for (int x = 0; x < kYccStripPixels; ++x)
        px[x] = x < nx ? (unsigned)row[3 * x] | ((unsigned)row[3 * x + 1] << 8) | ((unsigned)row[3 * x + 2] << 16) : 0u;
}

__device__ __forceinline__ int dot3(const int* m, unsigned px) {
    return m[0] * (int)(px & 255u) + m[1] * (int)((px >> 8) & 255u) + m[2] * (int)((px >> 16) & 255u);
}

__global__ __launch_bounds__(kYccThreads) void ycc420_kernel(const unsigned char* __restrict__ rgb, const YccDesc* __restrict__ descs, int nv12,
                                                             YccMatrix mat, unsigned char* __restrict__ out) {
    const YccDesc d = descs[blockIdx.y];
    if ((int)blockIdx.x >= ycc_blocks(d.h, d.w)) return;                           // uniform over the workgroup
    const long long strip = (long long)blockIdx.x * kYccThreads + threadIdx.x;
    if (strip >= ycc_strips(d.h, d.w)) return;
    const int h = d.h, w = d.w, cw = ycc_chroma_w(w), rs = ycc_row_strips(w);
    const int j = (int)(strip / rs), t = (int)(strip - (long long)j * rs);
    const int y0 = 2 * j, x0 = kYccStripPixels * t;
    const int ny = h - y0 < 2 ? h - y0 : 2, nx = w - x0 < kYccStripPixels ? w - x0 : kYccStripPixels;
    const unsigned char* __restrict__ src = rgb + d.src;
    unsigned char* __restrict__ dst = out + d.dst;
    const size_t img_bytes = (size_t)h * w * 3;
    unsigned px[2][kYccStripPixels];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r < ny) {
            const size_t at = ((size_t)(y0 + r) * w + x0) * 3;
            load_row(src + at, nx, nx == kYccStripPixels && at + 3 * kYccStripPixels + 4 <= img_bytes, px[r]);
        } else {
#pragma unroll
            for (int x = 0; x < kYccStripPixels; ++x) px[r][x] = 0u;
        }
    }
    // luma: one run of nx bytes per row
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        if (r >= ny) break;
        unsigned long long v = 0;
#pragma unroll
        for (int x = 0; x < kYccStripPixels; ++x) {
            const unsigned Y = (unsigned)(((dot3(mat.y, px[r][x]) + 32768) >> 16) + mat.yoff);
            v |= (unsigned long long)(Y & 255u) << (8 * x);
        }
        store_run(dst + (size_t)(y0 + r) * w + x0, v, nx);
    }
    // chroma: block b holds columns 2b and 2b + 1 of both rows, as far as the image goes (k = 1, 2 or 4 pixels: invalid ones are zero and add nothing)
    const int nc = (nx + 1) / 2;
    unsigned cbv = 0, crv = 0;
#pragma unroll
    for (int b = 0; b < kYccStripBlocks; ++b) {
        const int kc = 2 * b + 1 < nx ? 2 : 1, k = kc * ny, lg = k == 4 ? 2 : k == 2 ? 1 : 0;
        const int scb = dot3(mat.cb, px[0][2 * b]) + dot3(mat.cb, px[0][2 * b + 1]) + dot3(mat.cb, px[1][2 * b]) + dot3(mat.cb, px[1][2 * b + 1]);
        const int scr = dot3(mat.cr, px[0][2 * b]) + dot3(mat.cr, px[0][2 * b + 1]) + dot3(mat.cr, px[1][2 * b]) + dot3(mat.cr, px[1][2 * b + 1]);
        const unsigned cb = (unsigned)((scb + k * kYccChromaBias) >> (16 + lg)) & 255u, cr = (unsigned)((scr + k * kYccChromaBias) >> (16 + lg)) & 255u;
        cbv |= cb << (8 * b); crv |= cr << (8 * b);
    }
    const size_t c_at = (size_t)j * cw + (size_t)kYccStripBlocks * t;
    if (nv12) {
        unsigned long long v = 0;
#pragma unroll
        for (int b = 0; b < kYccStripBlocks; ++b)
            v |= ((unsigned long long)((cbv >> (8 * b)) & 255u) << (16 * b)) | ((unsigned long long)((crv >> (8 * b)) & 255u) << (16 * b + 8));
        store_run(dst + ycc_cb_at(h, w) + 2 * c_at, v, 2 * nc);
    } else {
        store_run(dst + ycc_cb_at(h, w) + c_at, cbv, nc);
        store_run(dst + ycc_cr_at(h, w) + c_at, crv, nc);
    }
}

}  // namespace

hipError_t launch_ycc420(const unsigned char* rgb, const YccDesc* descs, int n, int max_blocks, int format, int matrix, unsigned char* out,
                         hipStream_t s) {
    if (rgb == nullptr || descs == nullptr || out == nullptr) return hipErrorInvalidValue;
    if (n <= 0 || n > 65535 || max_blocks <= 0) return hipErrorInvalidValue;
    if ((format != kYccI420 && format != kYccNV12) || matrix < 0 || matrix >= kYccMatrices) return hipErrorInvalidValue;
    if (((uintptr_t)rgb & 3) || ((uintptr_t)out & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ycc420_kernel, dim3((unsigned)max_blocks, (unsigned)n), dim3(kYccThreads), 0, s, rgb, descs, format == kYccNV12 ? 1 : 0,
                       ycc_matrix(matrix), out);
    return hipGetLastError();
}

}  // namespace idc
