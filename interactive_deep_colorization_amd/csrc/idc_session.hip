// Click-session kernels: the two pieces of per-click host work that surround the
// network in the reference GUI, moved next to the resident planes so that a click sends a few dozen bytes.
//
//  * hint rasterisation -- UIControl.get_input (ui/ui_control.py:177-187: filled rectangles on a black canvas,
//    later edits over earlier ones) + the rgb2lab of that canvas in gui_draw.compute_result (ui/gui_draw.py:273-277),
//    or the notebook's put_point (DemoInteractiveColorization.ipynb:131-139) when the colours are given as ab.
//  * colour suggestions -- ColorizeImageTorchDist.get_ab_reccs (data/colorize_image.py:322-354): inverse-CDF
//    samples of one pixel's predicted distribution, k-means, clusters ordered by occupancy.
//
//  * distribution maps -- ColorizeImageTorchDist / ColorizeImageCaffeDist.compute_entropy (data/colorize_image.py:356-357,
//    545-546) and a mode / sharpened-mean decode of the classifier's belief (what pred_ab does for the 313 net, prototxt
//    :826-850), as one streaming pass each over the resident distribution instead of a copy of it to the host.
//
//  * distribution batches -- get_ab_reccs for many pixels in one launch (suggest_batch_kernel: the same body, a workgroup per query) and the
//    question compute_entropy's map is plotted for, "where is the model least sure", answered on the device (dist_peaks_kernel).
//
//  * distribution scores -- the question the heads were trained on (NNEncode of the ground-truth ab + softmax cross-entropy,
//    caffe_files/color_quantization.py:7-33, caffe_traininglayers.py:161-189): cross-entropy against the soft-encoded truth and the rank of the
//    true bin per cell, top-k hit counts and a fixed-order sum per image (dist_score_kernel, dist_score_finish_kernel).
//
// The first two are latency kernels (one pixel per thread / one workgroup); neither touches HBM beyond the planes it writes.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "idc_kernels.h"

namespace idc {

// skimage rgb2lab of one uint8 colour, float64 (same constants / order as lab_post_kernel and oracle/colorspace.py)
__device__ __forceinline__ void hint_rgb8_to_lab(const unsigned char* q, double& L, double& a, double& b) {
    const double M[3][3] = {{0.412453, 0.357580, 0.180423}, {0.212671, 0.715160, 0.072169}, {0.019334, 0.119193, 0.950227}};
    const double white[3] = {0.95047, 1.0, 1.08883};
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
    L = 116.0 * g[1] - 16.0; a = 500.0 * (g[0] - g[1]); b = 200.0 * (g[1] - g[2]);
}

// One thread per pixel of one image: the LAST hint whose (inclusive, already clipped) rectangle covers the pixel wins,
// as successive cv2.rectangle / slice assignments do.  All lanes walk the same hint list (scalar loads).
__global__ __launch_bounds__(256) void raster_hints_kernel(const HintRect* __restrict__ hints, int n_hints, int mode,
                                                           float mask_value, float* __restrict__ ab,
                                                           float* __restrict__ mask, int H, int W) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= H * W) return;
    const int y = p / W, x = p - y * W;
    int hit = -1;
    for (int i = n_hints - 1; i >= 0; --i) {
        const HintRect r = hints[i];
        if (y >= r.y0 && y <= r.y1 && x >= r.x0 && x <= r.x1) { hit = i; break; }
    }
    float a = 0.f, b = 0.f, m = 0.f;
    if (hit >= 0) {
        const HintRect r = hints[hit];
        m = mask_value;
        if (mode == 0) {
            a = r.c0; b = r.c1;
        } else {
            const unsigned char q[3] = {(unsigned char)r.c0, (unsigned char)r.c1, (unsigned char)r.c2};
            double L, da, db;
            hint_rgb8_to_lab(q, L, da, db);
            a = (float)da; b = (float)db;
        }
    }
    ab[p] = a;
    ab[(size_t)H * W + p] = b;
    mask[p] = m;
}

hipError_t launch_raster_hints(const HintRect* hints, int n_hints, int mode, float mask_value, float* ab, float* mask,
                               int H, int W, hipStream_t s) {
    hipLaunchKernelGGL(raster_hints_kernel, dim3((H * W + 255) / 256), dim3(256), 0, s, hints, n_hints, mode, mask_value,
                       ab, mask, H, W);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Colour suggestions for one pixel.  pdf: B probabilities, element b at pdf[b * stride].
//   1. cmf = cumsum(pdf) (sequential fp32, as numpy's cumsum of the fp32 distribution), / cmf[B-1]
//   2. N draws u_i = lowbias32(seed, i) >> 8 scaled by 2^-24; bin = #{cmf <= u} (numpy.digitize); counts per bin
//   3. weighted k-means over the B bin centres with the counts as weights (== k-means over the N samples):
//      deterministic greedy k-means++ seeding (first centre = most-sampled bin, next = argmax count * D^2),
//      Lloyd until the assignment is stable (max 100 sweeps), ties -> lowest index, float64
//   4. clusters ordered by occupancy (descending, ties -> lower cluster index first); conf = occupancy / N
// One workgroup of 256 threads; B <= kSuggestMaxBins, K <= kSuggestMaxK.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned lowbias32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

__device__ __forceinline__ void suggest_body(const float* __restrict__ pdf, long long stride, int B,
                                             const float* __restrict__ centres, int K, int N, unsigned seed,
                                             double* __restrict__ out_centres, double* __restrict__ out_conf,
                                             unsigned* __restrict__ out_counts) {
#pragma clang fp contract(off)
    __shared__ float cmf[kSuggestMaxBins];
    __shared__ unsigned cnt[kSuggestMaxBins];
    __shared__ float cx[kSuggestMaxBins], cy[kSuggestMaxBins];
    __shared__ int asg[kSuggestMaxBins];
    __shared__ double mx[kSuggestMaxK], my[kSuggestMaxK];
    __shared__ unsigned long long occ[kSuggestMaxK];
    __shared__ int changed, pick;
    __shared__ double red_v[256];
    __shared__ int red_i[256];
    const int t = threadIdx.x;
    for (int b = t; b < B; b += 256) {
        cmf[b] = pdf[(long long)b * stride];
        cnt[b] = 0u;
        cx[b] = centres[2 * b]; cy[b] = centres[2 * b + 1];
        asg[b] = -1;
    }
    __syncthreads();
    if (t == 0) {
        float run = 0.f;
        for (int b = 0; b < B; ++b) { run += cmf[b]; cmf[b] = run; }
        const float tot = run;
        for (int b = 0; b < B; ++b) cmf[b] = cmf[b] / tot;
    }
    __syncthreads();
    for (int i = t; i < N; i += 256) {
        const unsigned h = lowbias32((unsigned)i * 0x9E3779B9u + seed * 0x85EBCA6Bu + 0x165667B1u);
        const float u = (float)(h >> 8) * (1.0f / 16777216.0f);
        int lo = 0, hi = B;                       // first index with cmf > u  ==  #{cmf <= u}
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cmf[mid] <= u) lo = mid + 1; else hi = mid;
        }
        if (lo > B - 1) lo = B - 1;               // u < 1 = cmf[B-1] always; guard against a NaN pdf
        atomicAdd(&cnt[lo], 1u);
    }
    __syncthreads();
    if (out_counts) for (int b = t; b < B; b += 256) out_counts[b] = cnt[b];

    // --- seeding: k-th centre = argmax over bins of count * (squared distance to the nearest chosen centre) ---
    for (int k = 0; k < K; ++k) {
        double best = -1.0; int bi = 0x7fffffff;
        for (int b = t; b < B; b += 256) {
            double d2 = 1.0;
            if (k > 0) {
                d2 = 1.0e300;
                for (int j = 0; j < k; ++j) {
                    const double dx = (double)cx[b] - mx[j], dy = (double)cy[b] - my[j];
                    const double d = dx * dx + dy * dy;
                    if (d < d2) d2 = d;
                }
            }
            const double v = (double)cnt[b] * d2;
            if (v > best) { best = v; bi = b; }    // ascending b within a thread: first maximum kept
        }
        red_v[t] = best; red_i[t] = bi;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) {
                const double v2 = red_v[t + s]; const int i2 = red_i[t + s];
                if (v2 > red_v[t] || (v2 == red_v[t] && i2 < red_i[t])) { red_v[t] = v2; red_i[t] = i2; }
            }
            __syncthreads();
        }
        if (t == 0) { pick = red_i[0]; mx[k] = (double)cx[pick]; my[k] = (double)cy[pick]; }
        __syncthreads();
    }

    // --- Lloyd ---
    for (int it = 0; it < 100; ++it) {
        if (t == 0) changed = 0;
        __syncthreads();
        for (int b = t; b < B; b += 256) {
            int best = 0; double bd = 1.0e300;
            for (int j = 0; j < K; ++j) {
                const double dx = (double)cx[b] - mx[j], dy = (double)cy[b] - my[j];
                const double d = dx * dx + dy * dy;
                if (d < bd) { bd = d; best = j; }
            }
            if (best != asg[b]) { asg[b] = best; if (cnt[b]) changed = 1; }
        }
        __syncthreads();
        // Read the flag HERE, between the barrier behind the assignment pass and the barrier behind the means.  Read behind the last barrier of
        // the sweep it would race with thread 0's reset at the top of the next sweep: a wave that came late would see 0, leave the loop alone
        // and keep stale assignments while the others went on.  Every thread holds the same copy, so the branch below is uniform.
        const int again = changed;
        if (t < K) {                              // fixed-order (ascending bin) weighted mean of cluster t
            double sx = 0.0, sy = 0.0; unsigned long long w = 0ull;
            for (int b = 0; b < B; ++b)
                if (asg[b] == t && cnt[b]) { sx += (double)cnt[b] * (double)cx[b]; sy += (double)cnt[b] * (double)cy[b]; w += cnt[b]; }
            occ[t] = w;
            if (w) { mx[t] = sx / (double)w; my[t] = sy / (double)w; }     // an empty cluster keeps its centre
        }
        __syncthreads();
        if (!again) break;
    }
    if (t == 0) {                                 // order by occupancy, descending, stable
        unsigned used = 0u;
        for (int r = 0; r < K; ++r) {
            int bk = -1;
            for (int k = 0; k < K; ++k)
                if (!((used >> k) & 1u) && (bk < 0 || occ[k] > occ[bk])) bk = k;
            used |= 1u << bk;
            out_centres[2 * r] = mx[bk]; out_centres[2 * r + 1] = my[bk];
            out_conf[r] = (double)occ[bk] / (double)N;
        }
    }
}

__global__ __launch_bounds__(256) void suggest_kernel(const float* __restrict__ pdf, long long stride, int B,
                                                      const float* __restrict__ centres, int K, int N, unsigned seed,
                                                      double* __restrict__ out_centres, double* __restrict__ out_conf,
                                                      unsigned* __restrict__ out_counts) {
    suggest_body(pdf, stride, B, centres, K, N, seed, out_centres, out_conf, out_counts);
}

// The same body for a batch: workgroup q serves query q = {img, y, x, seed} -- from the list, or (peaks != nullptr) peak q of dist_peaks_kernel's
// [n][P][2] buffer with img = q / P and seed = seed0 + q, read where the picker left it -- and finds its pdf by idc_dist_at's rule: cell
// (y / s, x / s) of dist [n][B][Hd][Wd], s = 4 for the 529 head at H/4, 1 for the 313 head.  Query q writes out_centres [q][K][2] and out_conf [q][K].
// The empty query (-1, -1) reads nothing and writes zeros; so does a query outside the batch or the image (the host refuses those: this keeps a
// stray index from reaching memory).  The test is uniform over the workgroup, in front of every barrier.
__global__ __launch_bounds__(256) void suggest_batch_kernel(const float* __restrict__ dist, int n, int B, int Hd, int Wd, int s,
                                                            const DistQuery* __restrict__ queries, const int* __restrict__ peaks, int P,
                                                            unsigned seed0, const float* __restrict__ centres, int K, int N,
                                                            double* __restrict__ out_centres, double* __restrict__ out_conf) {
    const int q = blockIdx.x;
    int img, y, x; unsigned seed;
    if (peaks) { img = q / P; y = peaks[2 * q]; x = peaks[2 * q + 1]; seed = seed0 + (unsigned)q; }
    else { const DistQuery u = queries[q]; img = u.img; y = u.y; x = u.x; seed = u.seed; }
    double* oc = out_centres + (size_t)q * K * 2;
    double* of = out_conf + (size_t)q * K;
    if (img < 0 || img >= n || y < 0 || y >= Hd * s || x < 0 || x >= Wd * s) {
        for (int k = threadIdx.x; k < K; k += 256) { oc[2 * k] = 0.0; oc[2 * k + 1] = 0.0; of[k] = 0.0; }
        return;
    }
    const long long stride = (long long)Hd * Wd;
    suggest_body(dist + (size_t)img * B * stride + (size_t)(y / s) * Wd + (x / s), stride, B, centres, K, N, seed, oc, of, nullptr);
}

hipError_t launch_suggest_batch(const float* dist, int n, int B, int Hd, int Wd, int s, const DistQuery* queries, const int* peaks, int P,
                                unsigned seed0, int nq, const float* centres, int K, int N, double* out_centres, double* out_conf,
                                hipStream_t st) {
    hipLaunchKernelGGL(suggest_batch_kernel, dim3(nq), dim3(256), 0, st, dist, n, B, Hd, Wd, s, queries, peaks, P, seed0, centres, K, N,
                       out_centres, out_conf);
    return hipGetLastError();
}

hipError_t launch_suggest(const float* pdf, long long stride, int B, const float* centres, int K, int N, unsigned seed,
                          double* out_centres, double* out_conf, unsigned* out_counts, hipStream_t s) {
    hipLaunchKernelGGL(suggest_kernel, dim3(1), dim3(256), 0, s, pdf, stride, B, centres, K, N, seed, out_centres, out_conf,
                       out_counts);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Maps of the resident distribution dist [n][B][npix] fp32 (npix = Hd * Wd; a bin's pixels are contiguous).
// Geometry of both kernels: blockIdx.y = image, a workgroup owns kDistPix consecutive pixels (lane = pixel: one
// coalesced 256-byte row per wave load) and its kDistWaves waves split the bins in a FIXED partition -- wave w walks
// bins [w * chunk, min(B, (w + 1) * chunk)), chunk = ceil(B / kDistWaves), ascending -- so that the 529 head's
// 4096 pixels at 256x256 still put 512 waves on the device.  The partials meet in LDS and wave 0 folds them in wave
// order: the result of a pixel is a function of its B values alone (not of n, the grid or the timing).
// One dword per lane on purpose: a wave's load is already one whole 256-byte row, each element costs a logf and an fp64
// multiply-add (about as long as its 4 bytes take from HBM), and 16 bytes per lane would quarter the waves of the small
// head and want a scalar twin for grids that are no multiple of 4 pixels.
// ------------------------------------------------------------------------------------------------
constexpr int kDistWaves = 8, kDistPix = 64;

// ent[i][pix] = sum_q p log p (the reference's sign: MINUS the entropy).  logf of the stored fp32 p, product and sum
// in fp64, one rounding to fp32.  A bin with p == 0 contributes 0 where the reference's numpy expression gives NaN.
__global__ __launch_bounds__(kDistWaves * kDistPix) void dist_entropy_kernel(const float* __restrict__ dist, int B, int npix,
                                                                             float* __restrict__ ent) {
    __shared__ double part[kDistWaves][kDistPix];
    const int lane = threadIdx.x % kDistPix, w = __builtin_amdgcn_readfirstlane(threadIdx.x / kDistPix);   // wave-uniform: bin indices stay scalar
    const int pix = blockIdx.x * kDistPix + lane;
    const bool live = pix < npix;
    const int chunk = (B + kDistWaves - 1) / kDistWaves;
    const int b0 = w * chunk, b1 = min(B, b0 + chunk);
    const float* src = dist + (size_t)blockIdx.y * B * npix + pix;
    double acc = 0.0;
    if (live) {
#pragma unroll 4
        for (int b = b0; b < b1; ++b) {
            const float p = src[(size_t)b * npix];
            if (p != 0.f) acc += (double)p * (double)logf(p);
        }
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w == 0 && live) {
        double s = part[0][lane];
#pragma unroll
        for (int k = 1; k < kDistWaves; ++k) s += part[k][lane];
        ent[(size_t)blockIdx.y * npix + pix] = (float)s;
    }
}

hipError_t launch_dist_entropy(const float* dist, int n, int B, int npix, float* ent, hipStream_t s) {
    hipLaunchKernelGGL(dist_entropy_kernel, dim3((npix + kDistPix - 1) / kDistPix, n), dim3(kDistWaves * kDistPix), 0, s, dist, B, npix, ent);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Uncertainty peaks: where should the next hint go.  ent [n][Hd][Wd] is dist_entropy_kernel's map (MINUS the entropy: the smallest value is
// the least certain cell); mask [n][H][W] (or nullptr) the hint mask, H = Hd * s, W = Wd * s.  One workgroup per image, P rounds of greedy
// non-maximum suppression:
//   candidates = cells whose ent is not NaN and (mask given) whose s x s block of the mask plane is all zero;
//   round k: the candidate with the smallest ent, ties -> the lowest cy * Wd + cx; peaks[i][k] = (cy * s + s / 2, cx * s + s / 2) in net
//            coordinates, peak_ent[i][k] = its ent; every candidate with max(|dy|, |dx|) < radius leaves; no candidate: (-1, -1) and +0.
// The candidate set lives in work [n][Hd * Wd]: the image's ent with NaN where a cell is not (or no longer) a candidate, so a round is one
// strided walk (thread t sees cells t, t + 1024, ...: ascending, strict < keeps the lowest index), a shuffle arg-min per wave, the 16 wave
// results folded by wave 0 through LDS, and the winner's window overwritten with NaN.  The comparison (value, then index) is a total order on
// candidates, so the result is a function of the image's ent and mask values alone: not of n, the grid or timing.  No atomics; P rounds.
// ------------------------------------------------------------------------------------------------
constexpr int kPeakThreads = 1024;

// is (v2, i2) in front of (v1, i1)?  i == INT_MAX: no candidate
__device__ __forceinline__ bool peak_before(float v2, int i2, float v1, int i1) {
    if (i2 == 0x7fffffff) return false;
    if (i1 == 0x7fffffff) return true;
    return v2 < v1 || (v2 == v1 && i2 < i1);
}

__global__ __launch_bounds__(kPeakThreads) void dist_peaks_kernel(const float* __restrict__ ent, const float* __restrict__ mask, int Hd, int Wd,
                                                                  int s, int P, int radius, float* __restrict__ work, int* __restrict__ peaks,
                                                                  float* __restrict__ peak_ent) {
    __shared__ float wv[kPeakThreads / 64];
    __shared__ int wi[kPeakThreads / 64];
    __shared__ int pick_i;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, img = blockIdx.x;
    const int npix = Hd * Wd, W = Wd * s;
    const float* e = ent + (size_t)img * npix;
    float* wk = work + (size_t)img * npix;
    const float* m = mask ? mask + (size_t)img * npix * s * s : nullptr;
    const float gone = __builtin_nanf("");
    for (int c = t; c < npix; c += kPeakThreads) {
        float v = e[c];
        if (m) {
            const int cy = c / Wd, cx = c - cy * Wd;
            bool hinted = false;
            for (int dy = 0; dy < s; ++dy)
                for (int dx = 0; dx < s; ++dx) hinted = hinted || m[(size_t)(cy * s + dy) * W + cx * s + dx] != 0.f;
            if (hinted) v = gone;
        }
        wk[c] = v;
    }
    __threadfence_block();
    __syncthreads();
    for (int k = 0; k < P; ++k) {
        float bv = 0.f; int bi = 0x7fffffff;
        for (int c = t; c < npix; c += kPeakThreads) {
            const float v = wk[c];
            if (v == v && (bi == 0x7fffffff || v < bv)) { bv = v; bi = c; }
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const float v2 = __shfl_down(bv, d, 64); const int i2 = __shfl_down(bi, d, 64);
            if (peak_before(v2, i2, bv, bi)) { bv = v2; bi = i2; }
        }
        if (lane == 0) { wv[wave] = bv; wi[wave] = bi; }
        __syncthreads();
        if (wave == 0) {
            bv = lane < kPeakThreads / 64 ? wv[lane] : 0.f; bi = lane < kPeakThreads / 64 ? wi[lane] : 0x7fffffff;
#pragma unroll
            for (int d = 8; d > 0; d >>= 1) {
                const float v2 = __shfl_down(bv, d, 64); const int i2 = __shfl_down(bi, d, 64);
                if (peak_before(v2, i2, bv, bi)) { bv = v2; bi = i2; }
            }
            if (lane == 0) {
                pick_i = bi;
                const bool none = bi == 0x7fffffff;
                const int cy = none ? 0 : bi / Wd, cx = none ? 0 : bi - cy * Wd;
                int* out = peaks + ((size_t)img * P + k) * 2;
                out[0] = none ? -1 : cy * s + s / 2; out[1] = none ? -1 : cx * s + s / 2;
                if (peak_ent) peak_ent[(size_t)img * P + k] = none ? 0.f : bv;
            }
        }
        __syncthreads();
        const int pi = pick_i;
        if (pi != 0x7fffffff) {         // uniform over the workgroup
            const int cy = pi / Wd, cx = pi - cy * Wd;
            const int y0 = max(cy - radius + 1, 0), y1 = min(cy + radius - 1, Hd - 1), x0 = max(cx - radius + 1, 0), x1 = min(cx + radius - 1, Wd - 1);
            const int ww = x1 - x0 + 1, cells = (y1 - y0 + 1) * ww;
            for (int j = t; j < cells; j += kPeakThreads) {
                const int dy = j / ww, dx = j - dy * ww;
                wk[(y0 + dy) * Wd + x0 + dx] = gone;
            }
        }
        __threadfence_block();
        __syncthreads();                // the window is gone before the next walk, and pick_i is read before wave 0 writes the next one
    }
}

hipError_t launch_dist_peaks(const float* ent, const float* mask, int n, int Hd, int Wd, int s, int P, int radius, float* work, int* peaks,
                             float* peak_ent, hipStream_t st) {
    hipLaunchKernelGGL(dist_peaks_kernel, dim3(n), dim3(kPeakThreads), 0, st, ent, mask, Hd, Wd, s, P, radius, work, peaks, peak_ent);
    return hipGetLastError();
}

// ab[i][2][npix] (+ conf[i][npix] = p_max unless nullptr) from centres [B][2].
//   mode 0 (IDC_DECODE_MODE): the centre of the arg-max bin; equal maxima -> the lowest bin index (strict > inside a
//                             wave's ascending walk, strict > again over the waves in ascending order).
//   mode 1 (IDC_DECODE_MEAN): w_q = expf(gamma * (logf(p_q) - logf(p_max))), 0 for p_q == 0; ab = sum w_q c_q / sum w_q,
//                             the three sums in fp64 (second walk over the same bins: L2 hits).
__global__ __launch_bounds__(kDistWaves * kDistPix) void dist_decode_kernel(const float* __restrict__ dist, int B, int npix, int mode,
                                                                            float gamma, const float* __restrict__ centres,
                                                                            float* __restrict__ ab, float* __restrict__ conf) {
    __shared__ float wmax[kDistWaves][kDistPix];
    __shared__ int warg[kDistWaves][kDistPix];
    __shared__ double part[3][kDistWaves][kDistPix];
    const int lane = threadIdx.x % kDistPix, w = __builtin_amdgcn_readfirstlane(threadIdx.x / kDistPix);   // wave-uniform: bin indices stay scalar
    const int pix = blockIdx.x * kDistPix + lane;
    const bool live = pix < npix;
    const int chunk = (B + kDistWaves - 1) / kDistWaves;
    const int b0 = w * chunk, b1 = min(B, b0 + chunk);
    const float* src = dist + (size_t)blockIdx.y * B * npix + pix;
    float pm = -1.f; int arg = b0;                 // probabilities are >= 0: the first bin of the walk always takes over
    if (live) {
#pragma unroll 4
        for (int b = b0; b < b1; ++b) {
            const float p = src[(size_t)b * npix];
            if (p > pm) { pm = p; arg = b; }
        }
    }
    wmax[w][lane] = pm; warg[w][lane] = arg;
    __syncthreads();
    pm = wmax[0][lane]; arg = warg[0][lane];       // every wave needs p_max for its weights
#pragma unroll
    for (int k = 1; k < kDistWaves; ++k)
        if (wmax[k][lane] > pm) { pm = wmax[k][lane]; arg = warg[k][lane]; }
    float* dst = ab + (size_t)blockIdx.y * 2 * npix + pix;
    if (mode == 0) {
        if (w == 0 && live) {
            dst[0] = centres[2 * arg]; dst[npix] = centres[2 * arg + 1];
            if (conf) conf[(size_t)blockIdx.y * npix + pix] = pm;
        }
        return;
    }
    double sw = 0.0, sa = 0.0, sb = 0.0;
    if (live) {
        const float lpm = logf(pm);
#pragma unroll 4
        for (int b = b0; b < b1; ++b) {
            const float p = src[(size_t)b * npix];
            if (p != 0.f) {
                const double wq = (double)expf(gamma * (logf(p) - lpm));
                sw += wq; sa += wq * (double)centres[2 * b]; sb += wq * (double)centres[2 * b + 1];
            }
        }
    }
    part[0][w][lane] = sw; part[1][w][lane] = sa; part[2][w][lane] = sb;
    __syncthreads();
    if (w == 0 && live) {
        sw = part[0][0][lane]; sa = part[1][0][lane]; sb = part[2][0][lane];
#pragma unroll
        for (int k = 1; k < kDistWaves; ++k) { sw += part[0][k][lane]; sa += part[1][k][lane]; sb += part[2][k][lane]; }
        dst[0] = (float)(sa / sw); dst[npix] = (float)(sb / sw);
        if (conf) conf[(size_t)blockIdx.y * npix + pix] = pm;
    }
}

hipError_t launch_dist_decode(const float* dist, int n, int B, int npix, int mode, float gamma, const float* centres, float* ab,
                              float* conf, hipStream_t s) {
    hipLaunchKernelGGL(dist_decode_kernel, dim3((npix + kDistPix - 1) / kDistPix, n), dim3(kDistWaves * kDistPix), 0, s, dist, B, npix, mode,
                       gamma, centres, ab, conf);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// Distribution scores (idc_dist_score / idc_forward_async_dist_score): how much probability did the head put on the colour the pixel really has.
// The contract, per image i and cell c of dist [n][B][npix] with truth [n][2][npix] = the cell's ground-truth (a*, b*) fp32 (dist_truth_kernel,
// idc_colour.hip: idc_reveal_hints' colour of the cell's rectangle, bit for bit) and centres [B][2] fp32:
//   neighbours q_1 .. q_nn: the nn centres nearest to the truth, d^2 = da * da + db * db in float64 from the fp32 values (no FMA), ascending,
//                           ties to the lower index; t = q_1 is the target bin.  (Ordered by d^2: as by d, but for two d^2 that share a root.)
//   weights    w_j = exp(-d_j^2 / (2 sigma^2)) / sum_k exp(-d_k^2 / (2 sigma^2)), float64, k ascending; exactly 1 for nn == 1
//   xent       = 0 - sum_j w_j * log(max(p[q_j], FLT_MIN)), float64 log, products and sum, j ascending (Caffe's softmax-loss floor: finite)
//   rank       = #{q : p[q] > p[t] || (p[q] == p[t] && q < t)}, 0 .. B - 1
//   hits[i][j] = #{cells of image i : rank < thr[j]}: integer atomics, exact in any order
//   xent[i]    = the cells' values summed in a FIXED order, no float atomics: blocks of 64 consecutive cells (this kernel's workgroups; the last one
//                padded with +0.0) folded by halves (c with c + 32, then + 16, ... + 1) into part [n][nblk]; then dist_score_finish_kernel, one
//                wave per image: lane l adds the block sums l, l + 64, ... in ascending order onto +0.0, and the 64 lanes fold by halves.
// Geometry: dist_entropy_kernel's -- blockIdx.y = image, a workgroup owns kDistPix consecutive cells, lane = cell in the streaming phases.
//   phase 0  the neighbours.  Eight lanes share a cell (thread t: cell t / 8, lane t % 8 walks centres t % 8, + 8, ... held in LDS): nn passes of
//            "the nearest after (d^2, index) of the pass before", each a strided walk and a three-step butterfly over the eight lanes on the total
//            order (d^2, index).  No per-thread array of candidates (a dynamically indexed one would live in scratch); the lists meet in LDS.
//   phase 1  wave w takes the neighbours j = w, w + 8: one gather p[q_j], its log and the exp term, into LDS.
//   phase 2  the streamed count: wave w walks bins [w * chunk, min(B, (w + 1) * chunk)) against p[t], one coalesced 256-byte row per load;
//            the eight counts meet in LDS, wave 0 adds them, forms xent in j order, writes the maps, votes the hits and folds the block sum.
// A workgroup's dead lanes (the last block) read the image's last cell and write nothing.
// ------------------------------------------------------------------------------------------------
constexpr int kScoreMaxNN = 16;

__global__ __launch_bounds__(kDistWaves * kDistPix) void dist_score_kernel(const float* __restrict__ dist, const float* __restrict__ truth,
                                                                           const float* __restrict__ centres, int B, int npix, int nn, float sigma,
                                                                           ScoreRanks ranks, double* __restrict__ part, unsigned* __restrict__ hits,
                                                                           double* __restrict__ xent_map, int* __restrict__ rank_map,
                                                                           int* __restrict__ target) {
#pragma clang fp contract(off)
    __shared__ float cen[2 * kSuggestMaxBins];
    __shared__ int nq[kScoreMaxNN][kDistPix];
    __shared__ double nd[kScoreMaxNN][kDistPix];       // d^2 of neighbour j, then its exp term
    __shared__ double nl[kScoreMaxNN][kDistPix];       // log(max(p[q_j], FLT_MIN))
    __shared__ int cnt[kDistWaves][kDistPix];
    const int tid = threadIdx.x, img = blockIdx.y, pix0 = blockIdx.x * kDistPix;
    for (int i = tid; i < 2 * B; i += kDistWaves * kDistPix) cen[i] = centres[i];
    __syncthreads();
    {
        const int cell = tid >> 3, sub = tid & 7;
        const int pc = min(pix0 + cell, npix - 1);
        const double ta = (double)truth[(size_t)img * 2 * npix + pc], tb = (double)truth[((size_t)img * 2 + 1) * npix + pc];
        double pd = -1.0; int pi = -1;                  // the pass before: every d^2 >= 0 comes after it
        for (int j = 0; j < nn; ++j) {
            double bd = __builtin_inf(); int bi = 0x7fffffff;
            for (int b = sub; b < B; b += 8) {
                const double da = ta - (double)cen[2 * b], db = tb - (double)cen[2 * b + 1];
                const double d = da * da + db * db;
                if ((d > pd || (d == pd && b > pi)) && d < bd) { bd = d; bi = b; }      // ascending b: the first of equals is kept
            }
#pragma unroll
            for (int o = 1; o < 8; o <<= 1) {
                const double od = __shfl_xor(bd, o, 64); const int oi = __shfl_xor(bi, o, 64);
                if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
            }
            if (sub == 0) { nq[j][cell] = bi < B ? bi : B - 1; nd[j][cell] = bd; }       // (no candidate: a NaN truth; keeps the gather inside)
            pd = bd; pi = bi;
        }
    }
    __syncthreads();
    const int lane = tid % kDistPix, w = __builtin_amdgcn_readfirstlane(tid / kDistPix);   // wave-uniform: bin indices stay scalar
    const int pix = pix0 + lane;
    const bool live = pix < npix;
    const float* src = dist + (size_t)img * B * npix + (live ? pix : npix - 1);
    const int t = nq[0][lane];
    const float pt = src[(size_t)t * npix];
    const double two_s2 = 2.0 * ((double)sigma * (double)sigma);
    for (int j = w; j < nn; j += kDistWaves) {
        const float p = src[(size_t)nq[j][lane] * npix];
        nl[j][lane] = log((double)(p > FLT_MIN ? p : FLT_MIN));
        nd[j][lane] = exp(-nd[j][lane] / two_s2);
    }
    const int chunk = (B + kDistWaves - 1) / kDistWaves;
    const int b0 = w * chunk, b1 = min(B, b0 + chunk);
    int c = 0;
#pragma unroll 4
    for (int b = b0; b < b1; ++b) {
        const float p = src[(size_t)b * npix];
        c += (p > pt || (p == pt && b < t)) ? 1 : 0;
    }
    cnt[w][lane] = c;
    __syncthreads();
    if (w != 0) return;
    int rank = cnt[0][lane];
#pragma unroll
    for (int k = 1; k < kDistWaves; ++k) rank += cnt[k][lane];
    double xe;
    if (nn == 1) {
        xe = 0.0 - nl[0][lane];
    } else {
        double sum = 0.0, acc = 0.0;
        for (int j = 0; j < nn; ++j) sum += nd[j][lane];
        for (int j = 0; j < nn; ++j) acc += (nd[j][lane] / sum) * nl[j][lane];
        xe = 0.0 - acc;
    }
    if (live) {
        const size_t at = (size_t)img * npix + pix;
        if (xent_map) xent_map[at] = xe;
        if (rank_map) rank_map[at] = rank;
        if (target) target[at] = t;
    } else {
        xe = 0.0;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (j < ranks.n) {
            const unsigned long long m = __ballot(live && rank < ranks.thr[j]);
            if (lane == 0 && m) atomicAdd(&hits[(size_t)img * ranks.n + j], (unsigned)__popcll(m));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) xe += __shfl_down(xe, o, 64);
    if (lane == 0) part[(size_t)img * gridDim.x + blockIdx.x] = xe;
}

// xent[i] from image i's nblk block sums: lane l of the one wave adds part[l], part[l + 64], ... in ascending order onto +0.0, the lanes fold by halves.
__global__ __launch_bounds__(64) void dist_score_finish_kernel(const double* __restrict__ part, int nblk, double* __restrict__ xent) {
    const double* p = part + (size_t)blockIdx.x * nblk;
    double s = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 64) s += p[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (threadIdx.x == 0) xent[blockIdx.x] = s;
}

hipError_t launch_dist_score(const float* dist, const float* truth, const float* centres, int n, int B, int npix, int nn, float sigma,
                             ScoreRanks ranks, double* part, double* xent, unsigned* hits, double* xent_map, int* rank_map, int* target,
                             hipStream_t st) {
    if (!dist || !truth || !centres || !part || !xent || n <= 0 || npix <= 0 || B < 1 || B > kSuggestMaxBins || nn < 1 || nn > kScoreMaxNN || nn > B ||
        ranks.n < 0 || ranks.n > 8 || (ranks.n > 0 && !hits))
        return hipErrorInvalidValue;
    const int nblk = (npix + kDistPix - 1) / kDistPix;
    if (ranks.n > 0) {
        const hipError_t e = hipMemsetAsync(hits, 0, (size_t)n * ranks.n * sizeof(unsigned), st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(dist_score_kernel, dim3(nblk, n), dim3(kDistWaves * kDistPix), 0, st, dist, truth, centres, B, npix, nn, sigma, ranks, part,
                       hits, xent_map, rank_map, target);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dist_score_finish_kernel, dim3(n), dim3(64), 0, st, (const double*)part, nblk, xent);
    return hipGetLastError();
}

}  // namespace idc
