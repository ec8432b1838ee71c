// idc_motion.hip -- block-matched motion compensation of the temporal ab filter (idc_set_temporal_motion; the rule: include/ideepcolor.h; the
// geometry: idc_motion.h).  With motion on, run_temporal (idc_exec.hip) takes these launches in place of idc_temporal.hip's two:
//   motion_search_kernel   grid exact: dim3(tiles of one frame, n).  Frame f's predecessor plane is frame f - 1 of the same launch, or l_prev
//             for f = 0: the vectors depend on L alone.  The workgroup keeps its 16 x 64 tile (2 x 8 blocks) and the predecessor's window with
//             an apron of S pixels in LDS as fp32.  16 neighbouring lanes work for one block: lane q takes the candidates q, q + 16, .. in
//             raster order (neighbouring dx: the tile pixel is a broadcast, the window reads are consecutive), each the rule's 64-term
//             sequential float64 sum, and keeps the least (J, rank) pair; four __shfl_xor steps join the 16 lanes.  A parallel reduction over
//             (J, rank) pairs is the rule's first minimum in rank order; a NaN never enters it, and a NaN at rank 0 keeps (0, 0) as the
//             sequential walk does.  One plain 2-byte store per block.
//   motion_diff_kernel     temporal_diff_kernel's twin on the warped plane: e = (l[p] - l_prev[p + v(p's block)])^2, the apron pixels with
//             THEIR blocks' vectors; g and one partial of e per tile in the plain kernel's order, so at S = 0 the bits are the plain kernel's.
//   motion_blend_kernel    ONE LAUNCH PER FRAME, in stream order: y_f[p] reads y_{f-1}[p + v] of another pixel, which another workgroup of
//             the previous launch wrote.  Frame f reads the already-filtered x[f - 1] (frame 0: y_prev) and writes x[f]; nothing is written
//             in place, so the state is updated by two stream-ordered device-to-device copies behind the last launch (idc_exec.hip).  Every
//             workgroup adds the frame's partials in ascending order and forms the flag; a passed frame (no predecessor, or a cut) is left
//             as it is: y = x bit for bit.
//   Everything is float64 with contraction off.  No atomic, no persistent loop, no grid barrier.  Every displaced read is inside the plane
//   because only valid candidates are ever chosen; the readers check all the same and fall back to (0, 0).
#include <hip/hip_runtime.h>

#include "idc_kernels.h"

namespace idc {

namespace {

struct Best { double J; int rank, ci; };      // ci < 0: none yet

__device__ __forceinline__ void take_better(Best& a, double J, int rank, int ci) {
    if (ci >= 0 && (a.ci < 0 || J < a.J || (J == a.J && rank < a.rank))) { a.J = J; a.rank = rank; a.ci = ci; }
}

__global__ __launch_bounds__(kMotionThreads) void motion_search_kernel(const float* __restrict__ L, const float* __restrict__ l_prev, int have,
                                                                       int H, int W, int S, double penalty, signed char* __restrict__ v) {
#pragma clang fp contract(off)
    __shared__ __attribute__((aligned(16))) float cur[kTemporalTileH][kTemporalTileW];
    __shared__ float win[kMotionWinH][kMotionWinW];
    __shared__ unsigned char rank_of[kMotionMaxCandidates + 3];
    const int f = blockIdx.y, tile = blockIdx.x, tiles_x = temporal_tiles_x(W);
    const int j0 = (tile / tiles_x) * kTemporalTileH, i0 = (tile % tiles_x) * kTemporalTileW;
    const size_t hw = (size_t)H * W;
    const int t = threadIdx.x, b = motion_thread_block(t), q = t % kMotionLanes;
    const int bj = b / kMotionTileBlocksX, bi = b % kMotionTileBlocksX;
    const int by = j0 / kMotionBlock + bj, bx = i0 / kMotionBlock + bi;
    const bool inside = by < motion_blocks_y(H) && bx < motion_blocks_x(W);
    signed char* __restrict__ vp = v + ((size_t)f * motion_blocks(H, W) + (size_t)(inside ? by : 0) * motion_blocks_x(W) + (inside ? bx : 0)) * 2;
    if (f == 0 && !have) {                               // no predecessor: the vectors are reported as zeros (uniform over the workgroup)
        if (inside && q == 0) *(char2*)vp = make_char2(0, 0);
        return;
    }
    const float* __restrict__ cp = L + (size_t)f * hw;
    const float* __restrict__ pp = f > 0 ? L + (size_t)(f - 1) * hw : l_prev;
    {                                                    // the tile: one 16-byte load a thread (W is a multiple of 8: 4 pixels inside together)
        const int r = t >> 4, c4 = (t & 15) * 4;
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j0 + r < H && i0 + c4 < W) x = *(const float4*)(cp + (size_t)(j0 + r) * W + i0 + c4);
        *(float4*)&cur[r][c4] = x;
    }
    const int ww = kTemporalTileW + 2 * S, cells = (kTemporalTileH + 2 * S) * ww;
    for (int idx = t; idx < cells; idx += kMotionThreads) {          // the window: origin (j0 - S, i0 - S); zeros outside the plane, never read
        const int jj = idx / ww, ii = idx - jj * ww;
        const int gj = j0 - S + jj, gi = i0 - S + ii;
        win[jj][ii] = (gj >= 0 && gj < H && gi >= 0 && gi < W) ? pp[(size_t)gj * W + gi] : 0.f;
    }
    const int side = 2 * S + 1, ncand = side * side;
    if (t < ncand) {                                     // the rank of every candidate, by counting
        const int dy = t / side - S, dx = t % side - S;
        int r = 0;
        for (int a = -S; a <= S; ++a)
            for (int c = -S; c <= S; ++c) r += motion_before(a, c, dy, dx) ? 1 : 0;
        rank_of[t] = (unsigned char)r;
    }
    __syncthreads();
    Best best = {0.0, 0, -1};
    int nan0 = 0;
    if (inside) {
        for (int ci = q; ci < ncand; ci += kMotionLanes) {
            const int dy = ci / side - S, dx = ci % side - S;
            if (!motion_valid(by, bx, dy, dx, H, W)) continue;
            const float* a = &cur[bj * kMotionBlock][bi * kMotionBlock];
            const float* w = &win[bj * kMotionBlock + S + dy][bi * kMotionBlock + S + dx];
            double C = 0.0;
            for (int r = 0; r < kMotionBlock; ++r) {
#pragma unroll
                for (int c = 0; c < kMotionBlock; ++c) {
                    const double d = (double)a[r * kTemporalTileW + c] - (double)w[r * kMotionWinW + c];
                    const double dd = d * d;
                    C = C + dd;
                }
            }
            const double J = C / 64.0 + penalty * (double)(dy * dy + dx * dx);
            if (J != J) { if (dy == 0 && dx == 0) nan0 = 1; continue; }       // a NaN never wins; at rank 0 nothing replaces it
            take_better(best, J, (int)rank_of[ci], ci);
        }
    }
#pragma unroll
    for (int off = kMotionLanes / 2; off >= 1; off >>= 1) {          // the 16 lanes of a block are neighbours: the exchange stays among them
        const double oJ = __shfl_xor(best.J, off);
        const int oR = __shfl_xor(best.rank, off), oC = __shfl_xor(best.ci, off);
        nan0 |= __shfl_xor(nan0, off);
        take_better(best, oJ, oR, oC);
    }
    if (inside && q == 0) {
        int dy = 0, dx = 0;
        if (!nan0 && best.ci >= 0) { dy = best.ci / side - S; dx = best.ci % side - S; }
        *(char2*)vp = make_char2((signed char)dy, (signed char)dx);
    }
}

// the vector of the block pixel (gj, gi) lies in, as an offset into the plane; (0, 0) if it would leave the plane (it never does: see above)
__device__ __forceinline__ long long vector_offset(const signed char* __restrict__ v, int gj, int gi, int H, int W) {
    const int by = gj / kMotionBlock, bx = gi / kMotionBlock;
    const char2 d = *(const char2*)(v + ((size_t)by * motion_blocks_x(W) + bx) * 2);
    if (!motion_valid(by, bx, d.x, d.y, H, W)) return 0;
    return (long long)d.x * W + d.y;
}

__global__ __launch_bounds__(kTemporalThreads) void motion_diff_kernel(const float* __restrict__ L, const float* __restrict__ l_prev,
                                                                       const signed char* __restrict__ v, int have, int H, int W, int R,
                                                                       double strength, double two_sigma2, double* __restrict__ g,
                                                                       double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double e[kTemporalLdsH][kTemporalLdsW];
    __shared__ double red[kTemporalThreads / 64];
    const int f = blockIdx.y, tile = blockIdx.x, tiles_x = temporal_tiles_x(W);
    const int j0 = (tile / tiles_x) * kTemporalTileH, i0 = (tile % tiles_x) * kTemporalTileW;
    const size_t hw = (size_t)H * W;
    const int t = threadIdx.x, r = t >> 4, c4 = (t & 15) * 4;
    const int j = j0 + r, i = i0 + c4;
    const bool inside = j < H && i < W;
    double* __restrict__ gp = g + (size_t)f * hw + (size_t)(inside ? j : 0) * W + (inside ? i : 0);
    if (f == 0 && !have) {
        if (inside) { ((double2*)gp)[0] = make_double2(0.0, 0.0); ((double2*)gp)[1] = make_double2(0.0, 0.0); }
        if (t == 0) part[(size_t)f * gridDim.x + tile] = 0.0;
        return;
    }
    const float* __restrict__ cur = L + (size_t)f * hw;
    const float* __restrict__ prev = f > 0 ? L + (size_t)(f - 1) * hw : l_prev;
    const signed char* __restrict__ vf = v + (size_t)f * motion_blocks(H, W) * 2;
    const int lw = kTemporalTileW + 2 * R, cells = (kTemporalTileH + 2 * R) * lw;
    for (int idx = t; idx < cells; idx += kTemporalThreads) {
        const int jj = idx / lw, ii = idx - jj * lw;
        const int gj = j0 - R + jj, gi = i0 - R + ii;
        double x = 0.0;
        if (gj >= 0 && gj < H && gi >= 0 && gi < W) {    // the pixel's OWN block's vector, also in the apron
            const long long at = (long long)gj * W + gi;
            const double d = (double)cur[at] - (double)prev[at + vector_offset(vf, gj, gi, H, W)];
            x = d * d;
        }
        e[jj][ii] = x;
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

__device__ __forceinline__ float blend_warped(float x, float yp, double g) {
#pragma clang fp contract(off)
    const double d = (double)yp - (double)x;
    const double gd = g * d;
    return (float)((double)x + gd);
}

// one frame: x [2,H,W] this frame's raw map, overwritten by y; yp [2,H,W] the previous frame's filtered map (another buffer); g, part, v this
// frame's; pass = the frame has no predecessor
__global__ __launch_bounds__(kTemporalThreads) void motion_blend_kernel(float* __restrict__ x, const float* __restrict__ yp,
                                                                        const double* __restrict__ g, const double* __restrict__ part,
                                                                        const signed char* __restrict__ v, int pass, int H, int W, int P,
                                                                        double cut2, double* __restrict__ D, int* __restrict__ cut) {
#pragma clang fp contract(off)
    __shared__ double s_part[kTemporalThreads];
    __shared__ int s_cut;
    const size_t hw = (size_t)H * W;
    const int t = threadIdx.x;
    double sum = 0.0;
    for (int p0 = 0; p0 < P; p0 += kTemporalThreads) {   // the partials in ascending order, as the plain kernel adds them
        if (p0 + t < P) s_part[t] = part[p0 + t];
        __syncthreads();
        if (t == 0) {
            const int m = P - p0 < kTemporalThreads ? P - p0 : kTemporalThreads;
            for (int k = 0; k < m; ++k) sum += s_part[k];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double d = sum / (double)hw;
        const int c = (pass || (cut2 > 0.0 && d > cut2)) ? 1 : 0;
        s_cut = c;
        if (blockIdx.x == 0) { *D = d; *cut = c; }
    }
    __syncthreads();
    if (s_cut) return;                                   // y = x bit for bit: x stands where y goes
    const size_t quarter = hw / kTemporalItemPixels;
    const size_t item = (size_t)blockIdx.x * kTemporalThreads + t;
    if (item >= 2 * quarter) return;
    const int ch = item >= quarter ? 1 : 0;
    const size_t pix = (item - (ch ? quarter : 0)) * kTemporalItemPixels;
    const int gj = (int)(pix / W), gi = (int)(pix - (size_t)gj * W);          // the item's 4 pixels lie in one block: one vector
    const float* __restrict__ ys = yp + (size_t)ch * hw + pix + vector_offset(v, gj, gi, H, W);
    float* __restrict__ xp = x + (size_t)ch * hw + pix;
    const float4 xv = *(const float4*)xp;
    const double2 g0 = ((const double2*)(g + pix))[0], g1 = ((const double2*)(g + pix))[1];
    *(float4*)xp = make_float4(blend_warped(xv.x, ys[0], g0.x), blend_warped(xv.y, ys[1], g0.y), blend_warped(xv.z, ys[2], g1.x),
                               blend_warped(xv.w, ys[3], g1.y));
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool plane_ok(int H, int W) { return H > 0 && W > 0 && !(H % 8) && !(W % 8); }

}  // namespace

hipError_t launch_motion_search(const float* L, const float* l_prev, int have, int n, int H, int W, int search, double penalty, int8_t* v,
                                hipStream_t s) {
    if (!L || !l_prev || !v) return hipErrorInvalidValue;
    if (n <= 0 || n > kTemporalMaxFrames || !plane_ok(H, W) || !motion_params_ok(1, search, penalty)) return hipErrorInvalidValue;
    if (!aligned16(L) || !aligned16(l_prev) || ((uintptr_t)v & 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_search_kernel, dim3((unsigned)temporal_tiles(H, W), (unsigned)n), dim3(kMotionThreads), 0, s, L, l_prev, have ? 1 : 0,
                       H, W, search, penalty, (signed char*)v);
    return hipGetLastError();
}

hipError_t launch_motion_diff(const float* L, const float* l_prev, const int8_t* v, int have, int n, int H, int W, int radius, double strength,
                              double sigma, double* g, double* part, hipStream_t s) {
    if (!L || !l_prev || !v || !g || !part) return hipErrorInvalidValue;
    if (n <= 0 || n > kTemporalMaxFrames || !plane_ok(H, W)) return hipErrorInvalidValue;
    if (radius < 0 || radius > kTemporalMaxRadius || !(sigma > 0.0)) return hipErrorInvalidValue;
    if (!aligned16(L) || !aligned16(l_prev) || !aligned16(g) || ((uintptr_t)v & 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_diff_kernel, dim3((unsigned)temporal_tiles(H, W), (unsigned)n), dim3(kTemporalThreads), 0, s, L, l_prev,
                       (const signed char*)v, have ? 1 : 0, H, W, radius, strength, 2.0 * sigma * sigma, g, part);
    return hipGetLastError();
}

hipError_t launch_motion_blend(float* x, const float* y_before, const double* g, const double* part, const int8_t* v, int pass, int H, int W,
                               double cut, double* D, int* cut_flag, hipStream_t s) {
    if (!x || !y_before || !g || !part || !v || !D || !cut_flag || x == y_before) return hipErrorInvalidValue;
    if (!plane_ok(H, W)) return hipErrorInvalidValue;
    if (!aligned16(x) || !aligned16(g) || ((uintptr_t)y_before & 3) || ((uintptr_t)v & 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(motion_blend_kernel, dim3((unsigned)temporal_blend_blocks(H, W)), dim3(kTemporalThreads), 0, s, x, y_before, g, part,
                       (const signed char*)v, pass ? 1 : 0, H, W, temporal_partials(H, W), cut * cut, D, cut_flag);
    return hipGetLastError();
}

}  // namespace idc
