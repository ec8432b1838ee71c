// idc_ycc.h -- the sizes, offsets, tiling and matrices of the YCbCr 4:2:0 output planes (idc_set_batch_output / idc_fullres_ycc /
// idc_rgb_to_ycc420; the rule: include/ideepcolor.h; the kernel: idc_ycc.hip).  Plain C++ that makes no runtime call: the launcher, the batch
// plan (idc_batch.h), the kernel itself and tools/ycc_selftest.cpp, which includes it beside idc_batch.h alone, read the same functions.
#ifndef IDC_YCC_H
#define IDC_YCC_H

#include <stddef.h>

#if defined(__HIPCC__)
#define IDC_YC_FN __host__ __device__ inline
#else
#define IDC_YC_FN inline
#endif

namespace idc {

// One thread owns a strip of kYccStripBlocks chroma blocks of one chroma row: 2 rows x 8 pixels of the image, clipped at its right and bottom
// edges.  A 256-thread workgroup takes 256 consecutive strips of ONE image (blockIdx.y), strips counted row-major over the chroma rows.
constexpr int kYccThreads = 256;
constexpr int kYccStripBlocks = 4;
constexpr int kYccStripPixels = 2 * kYccStripBlocks;
constexpr int kYccMaxSide = 16384;
constexpr int kYccFormats = 3;            // IDC_OUT_RGB, IDC_OUT_I420, IDC_OUT_NV12
constexpr int kYccMatrices = 2;           // IDC_YCC_JFIF, IDC_YCC_BT709_VIDEO
constexpr int kYccI420 = 1, kYccNV12 = 2; // the values of IDC_OUT_I420 / IDC_OUT_NV12, for the code that does not see the public header

// 16.16 fixed point: Y = ((y . (R,G,B) + 32768) >> 16) + yoff; chroma of a block of k pixels = (sum of c . (R,G,B) + k * kYccChromaBias) >> (16 + log2 k)
struct YccMatrix { int y[3], cb[3], cr[3], yoff; };
constexpr int kYccChromaBias = (128 << 16) + 32767;

IDC_YC_FN YccMatrix ycc_matrix(int matrix) {
    if (matrix == 1) return {{11966, 40254, 4064}, {-6596, -22189, 28785}, {28784, -26145, -2639}, 16};     // BT.709, limited range
    return {{19595, 38470, 7471}, {-11059, -21709, 32768}, {32768, -27439, -5329}, 0};                       // BT.601 full range (JFIF, libjpeg jccolor.c)
}

// One image of a launch: its [h,w,3] uint8 RGB at byte `src` of the packed results, its plane block at byte `dst` of the packed blocks
struct YccDesc { long long src, dst; int h, w; };

IDC_YC_FN int ycc_chroma_h(int h) { return (h + 1) / 2; }
IDC_YC_FN int ycc_chroma_w(int w) { return (w + 1) / 2; }

// bytes of one image's block: Y [h,w], then Cb [ch,cw] and Cr [ch,cw] (I420) or CbCr [ch,cw,2] (NV12); 0 for a side outside 1..16384
IDC_YC_FN size_t ycc420_bytes(int h, int w) {
    if (h < 1 || h > kYccMaxSide || w < 1 || w > kYccMaxSide) return 0;
    return (size_t)h * w + 2 * (size_t)ycc_chroma_h(h) * ycc_chroma_w(w);
}

// offsets inside a block: Y at 0, Cb (I420) or the interleaved pairs (NV12) at ycc_cb_at, Cr (I420 only) at ycc_cr_at
IDC_YC_FN size_t ycc_cb_at(int h, int w) { return (size_t)h * w; }
IDC_YC_FN size_t ycc_cr_at(int h, int w) { return (size_t)h * w + (size_t)ycc_chroma_h(h) * ycc_chroma_w(w); }

// strips of one chroma row, strips of one image, workgroups of one image: grid.x of a launch is the largest of the last over its images (exact: a
// workgroup past its own image's count returns).  16384 x 16384: 8192 x 2048 strips, 65536 workgroups.
IDC_YC_FN int ycc_row_strips(int w) { return (ycc_chroma_w(w) + kYccStripBlocks - 1) / kYccStripBlocks; }
IDC_YC_FN long long ycc_strips(int h, int w) { return (long long)ycc_chroma_h(h) * ycc_row_strips(w); }
IDC_YC_FN int ycc_blocks(int h, int w) { return (int)((ycc_strips(h, w) + kYccThreads - 1) / kYccThreads); }

}  // namespace idc

#endif  // IDC_YCC_H
