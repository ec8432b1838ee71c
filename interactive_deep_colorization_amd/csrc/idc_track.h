// idc_track.h -- the parameter checks, geometry, scratch sizes and the walk itself of the hint tracking along the motion vectors
// (idc_set_hint_tracking / idc_tracked_hints / idc_track_hints_apply; the rule: include/ideepcolor.h; the kernel: idc_track.hip).  Plain C++ that
// makes no runtime call: the launcher, the kernel itself and tools/track_selftest.cpp, which includes it beside idc_batch.h alone, read the same
// functions.
#ifndef IDC_TRACK_H
#define IDC_TRACK_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "idc_motion.h"

namespace idc {

constexpr int kTrackThreads = 256;        // one thread per (frame, pixel): grid dim3(track_blocks(H, W), n), exact up to the last workgroup
constexpr int kTrackMaxLife = 65535;
constexpr int32_t kTrackMaxAge = 0x7fffffff;      // an age stops here instead of wrapping (2^31 frames of one hint)

// what a pipelined call carries of idc_set_hint_tracking (BatchCall, PipeSlot) and what the launcher takes
struct TrackParams { int on; int life; double tol; };
IDC_TP_FN TrackParams track_defaults() { return {0, 0, 8.0}; }
// idc_set_hint_tracking's ranges (a NaN fails every comparison and so is outside)
IDC_TP_FN bool track_params_ok(int on, int life, double tol) {
    if (on != 0 && on != 1) return false;
    if (life < 0 || life > kTrackMaxLife) return false;
    if (!(tol >= 0.0 && tol <= 100.0)) return false;
    return true;
}

IDC_TP_FN int track_blocks(int H, int W) { return (int)(((long long)H * W + kTrackThreads - 1) / kTrackThreads); }

// scratch of one launch of n frames: the tracked ab fp32 [n,2,H,W], mask fp32 [n,H,W] and age int32 [n,H,W], one behind the other; every
// offset is a multiple of 256 bytes (H * W is a multiple of 64)
IDC_TP_FN size_t track_ab_bytes(int n, int H, int W) { return (size_t)n * 2 * H * W * sizeof(float); }
IDC_TP_FN size_t track_mask_at(int n, int H, int W) { return track_ab_bytes(n, H, W); }
IDC_TP_FN size_t track_age_at(int n, int H, int W) { return track_mask_at(n, H, W) + (size_t)n * H * W * sizeof(float); }
IDC_TP_FN size_t track_scratch_bytes(int n, int H, int W) { return track_age_at(n, H, W) + (size_t)n * H * W * sizeof(int32_t); }
// the sequence state (A, M, G) of the last frame: one frame of the same layout
IDC_TP_FN size_t track_state_bytes(int H, int W) { return track_scratch_bytes(1, H, W); }

struct TrackHit { float a, b, m; int32_t age; };

// pixel q = (qj, qi) of a frame whose vectors are vf [H/8, W/8, 2]: q + v(q's block) as an offset into the plane.  A valid vector keeps its
// whole block inside; one that would not (the search never writes one) counts as (0, 0), so no read leaves the plane whatever vf holds
// (a plane has fewer than 2^31 pixels -- the launcher refuses more -- so a pixel index is an int: no 64-bit division in the chain)
IDC_TP_FN int track_step(const int8_t* vf, int q, int H, int W) {
    const int qy = q / W, by = qy / kMotionBlock, bx = (q - qy * W) / kMotionBlock;
    const int8_t* d = vf + ((size_t)by * motion_blocks_x(W) + bx) * 2;
    if (!motion_valid(by, bx, d[0], d[1], H, W)) return q;
    return q + (int)d[0] * W + d[1];
}

// THE WALK of pixel p of frame f: the recursion of the rule unrolled.  Every read is of the RAW own planes ab [n,2,H,W] / mask [n,H,W], the L
// planes, l_prev, the vectors v [n,H/8,W/8,2] and the state (sA [2,H,W], sM, sG [H,W]): nothing another walk writes.
//   have_prev: frame 0 has a predecessor (l_prev and v[0] mean something); have_state: the state does too (it implies have_prev).
// The ages along a chain grow towards frame f, so `life` holds at every link iff it holds at the last one: the walk gives up as soon as the
// steps taken alone exceed it.
IDC_TP_FN TrackHit track_walk(const float* ab, const float* mask, const float* L, const float* l_prev, const int8_t* v, const float* sA,
                              const float* sM, const int32_t* sG, int have_prev, int have_state, int f, int p, int H, int W, int life,
                              double tol) {
    const TrackHit none = {0.f, 0.f, 0.f, 0};
    const size_t hw = (size_t)H * W, vb = (size_t)motion_blocks(H, W) * 2;
    int q = p;
    int steps = 0;
    for (int g = f;; --g) {
        const float m = mask[(size_t)g * hw + q];
        if (m != 0.f) return {ab[(size_t)g * 2 * hw + q], ab[((size_t)g * 2 + 1) * hw + q], m, steps};
        if (g == 0 && !(have_prev && have_state)) return none;
        const int q1 = track_step(v + (size_t)g * vb, q, H, W);
        const float lp = g > 0 ? L[(size_t)(g - 1) * hw + q1] : l_prev[q1];
        const double d = (double)L[(size_t)g * hw + q] - (double)lp;
        if (!(fabs(d) <= tol)) return none;              // a NaN carries nothing
        ++steps;
        if (life && steps > life) return none;
        if (g == 0) {                                    // the call's start: the state at the displaced pixel
            const float ms = sM[q1];
            if (!(ms != 0.f)) return none;
            const long long age = (long long)sG[q1] + steps;
            if (life && age > life) return none;
            return {sA[q1], sA[hw + q1], ms, age > kTrackMaxAge ? kTrackMaxAge : (int32_t)age};
        }
        q = q1;
    }
}

}  // namespace idc

#endif  // IDC_TRACK_H
