// idc_track.hip -- hints that follow the motion vectors (idc_set_hint_tracking; the rule: include/ideepcolor.h; the walk: idc_track.h).
//   track_hints_kernel   ONE launch for all n frames, grid dim3(track_blocks(H, W), n), one thread per (frame, pixel).  The rule is a recursion
//             over the frames; unrolled, the tracked value of pixel p of frame f is found by walking back from (f, p) along the vectors until
//             an own hint, a failed `tol` or `life` test, or the call's start, where the handle's state (A, M, G) is read at the displaced
//             pixel.  The walk (track_walk) reads only the RAW own planes, the L planes, l_prev, the vectors and the state, and writes the
//             slot's scratch: no thread reads what another wrote, so there is no grid-wide wait and no launch chain.  The state is written by
//             stream-ordered copies BEHIND the launch (idc_exec.hip): frame 0 reads it at displaced pixels.
//             The 64 lanes of a wave hold 64 neighbouring pixels of one row: at most 8 blocks and so a handful of vectors, and a step moves
//             whole runs of them together -- every gather of a step is a few contiguous segments.  A walk costs one 4-byte mask read a frame
//             it passes and, past the first, two L reads and a 2-byte vector; all planes of a batch (32 x 256 x 256: 32 MB) stay in the
//             last-level cache, so the kernel is bound by the latency of these dependent reads, not by HBM: the length of the walks (at
//             most f + 1 links, cut short by `tol`, `life` and every hint met) sets its time.  The four stores are coalesced 4-byte rows.
#include <hip/hip_runtime.h>

#include "idc_kernels.h"

namespace idc {

namespace {

__global__ __launch_bounds__(kTrackThreads) void track_hints_kernel(const float* __restrict__ ab, const float* __restrict__ mask,
                                                                    const float* __restrict__ L, const float* __restrict__ l_prev,
                                                                    const int8_t* __restrict__ v, const float* __restrict__ sA,
                                                                    const float* __restrict__ sM, const int32_t* __restrict__ sG, int have_prev,
                                                                    int have_state, int H, int W, int life, double tol,
                                                                    float* __restrict__ out_ab, float* __restrict__ out_mask,
                                                                    int32_t* __restrict__ out_age) {
    const size_t hw = (size_t)H * W;
    const int f = blockIdx.y;
    const size_t p = (size_t)blockIdx.x * kTrackThreads + threadIdx.x;
    if (p >= hw) return;
    const TrackHit hit = track_walk(ab, mask, L, l_prev, v, sA, sM, sG, have_prev, have_state, f, (int)p, H, W, life, tol);
    out_ab[(size_t)f * 2 * hw + p] = hit.a;
    out_ab[((size_t)f * 2 + 1) * hw + p] = hit.b;
    out_mask[(size_t)f * hw + p] = hit.m;
    out_age[(size_t)f * hw + p] = hit.age;
}

}  // namespace

hipError_t launch_track_hints(const float* ab, const float* mask, const float* L, const float* l_prev, const int8_t* v, const float* state_ab,
                              const float* state_mask, const int32_t* state_age, int have_prev, int have_state, int n, int H, int W, int life,
                              double tol, float* out_ab, float* out_mask, int32_t* out_age, hipStream_t s) {
    if (!ab || !mask || !L || !l_prev || !v || !state_ab || !state_mask || !state_age || !out_ab || !out_mask || !out_age)
        return hipErrorInvalidValue;
    if (n <= 0 || n > kTemporalMaxFrames || H <= 0 || W <= 0 || (H % 8) || (W % 8) || (long long)H * W > 0x7fffffffll || !track_params_ok(1, life, tol))
        return hipErrorInvalidValue;
    if (out_ab == ab || out_mask == mask) return hipErrorInvalidValue;      // the walks read the raw planes of every earlier frame
    hipLaunchKernelGGL(track_hints_kernel, dim3((unsigned)track_blocks(H, W), (unsigned)n), dim3(kTrackThreads), 0, s, ab, mask, L, l_prev, v,
                       state_ab, state_mask, state_age, have_prev ? 1 : 0, (have_prev && have_state) ? 1 : 0, H, W, life, tol, out_ab, out_mask,
                       out_age);
    return hipGetLastError();
}

}  // namespace idc
