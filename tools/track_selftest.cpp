// track_selftest -- csrc/idc_track.h and csrc/idc_batch.h for the hint tracking along the motion vectors, without a device.  Host code only, no
// library, no HIP runtime call (tests/test_track_cpu.py runs this; `make track_selftest SAN=1` builds it under ASan + UBSan, where the
// exactly-sized arrays turn an index past a plane, the vectors or the state into a report).
//   params   idc_set_hint_tracking's ranges, NaN outside.
//   scratch  for every net size H, W in 8, 16 .. 512: the tracked planes of n frames lie one behind the other without a gap, every offset a
//            multiple of 256 bytes, the state is one frame of the same layout, and the grid covers the plane exactly once.
//   walk     track_walk -- the function the kernel runs per (frame, pixel) -- against the RECURSION of the rule, frame by frame from the
//            previous frame's tracked planes, on small hand-made planes: own over carried, tol on either side and exactly at it, a NaN, life
//            1 and 2 and none, the state with and without a predecessor, vectors that differ block by block, a call split in two.
//   plan     a call with tracking off and on against the same call without the field: every plan field and every byte of the metadata block.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "idc_track.h"
#include "idc_batch.h"

using namespace idc;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

static void check_params() {
    const double nan = NAN;
    CHECK(track_params_ok(1, 0, 8.0) && track_params_ok(0, 65535, 100.0) && track_params_ok(1, 1, 0.0));
    CHECK(!track_params_ok(2, 0, 8.0) && !track_params_ok(-1, 0, 8.0));
    CHECK(!track_params_ok(1, -1, 8.0) && !track_params_ok(1, 65536, 8.0));
    CHECK(!track_params_ok(1, 0, -0.001) && !track_params_ok(1, 0, 100.001) && !track_params_ok(1, 0, nan) && !track_params_ok(1, 0, INFINITY));
    const TrackParams d = track_defaults();
    CHECK(d.on == 0 && d.life == 0 && d.tol == 8.0 && kTrackMaxLife == 65535 && kTrackThreads == 256);
}

static long long check_sizes() {
    long long checked = 0;
    for (int H = 8; H <= 512; H += 8)
        for (int W = 8; W <= 512; W += 8, ++checked) {
            const size_t hw = (size_t)H * W;
            for (int n : {1, 5, 32}) {
                CHECK(track_ab_bytes(n, H, W) == n * 2 * hw * 4 && track_mask_at(n, H, W) == track_ab_bytes(n, H, W));
                CHECK(track_age_at(n, H, W) == track_mask_at(n, H, W) + n * hw * 4 && track_scratch_bytes(n, H, W) == n * hw * 16);
                CHECK(track_mask_at(n, H, W) % 256 == 0 && track_age_at(n, H, W) % 256 == 0);
                CHECK(track_scratch_bytes(n, H, W) <= track_scratch_bytes(32, H, W));      // reserved at max_batch: any n fits
            }
            CHECK(track_state_bytes(H, W) == hw * 16);
            const int blocks = track_blocks(H, W);
            CHECK((size_t)blocks * kTrackThreads >= hw && (size_t)(blocks - 1) * kTrackThreads < hw);
        }
    CHECK(track_scratch_bytes(32, 256, 256) == 32u * 65536u * 16u && track_blocks(8, 8) == 1 && track_blocks(40, 72) == 12);
    return checked;
}

// ---- the walk against the recursion
struct Planes {
    int n, H, W;
    std::vector<float> ab, mask, L;
    std::vector<int8_t> v;
    Planes(int n_, int H_, int W_) : n(n_), H(H_), W(W_), ab((size_t)n_ * 2 * H_ * W_, 0.f), mask((size_t)n_ * H_ * W_, 0.f), L((size_t)n_ * H_ * W_, 0.f),
                                     v((size_t)n_ * (H_ / 8) * (W_ / 8) * 2, 0) {}
};
struct State {
    bool have_prev = false, have = false;
    std::vector<float> A, M, l;
    std::vector<int32_t> G;
    explicit State(size_t hw) : A(2 * hw, 0.f), M(hw, 0.f), l(hw, 0.f), G(hw, 0) {}
};

// the rule, one frame from the previous frame's TRACKED planes; returns the new state
static State recursion_frame(const Planes& P, int f, const State& prev, int life, double tol) {
    const int H = P.H, W = P.W;
    const size_t hw = (size_t)H * W;
    State out(hw);
    out.have_prev = out.have = true;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            out.l[p] = P.L[f * hw + p];
            const float m = P.mask[f * hw + p];
            if (m != 0.f) {
                out.A[p] = P.ab[(size_t)f * 2 * hw + p]; out.A[hw + p] = P.ab[((size_t)f * 2 + 1) * hw + p]; out.M[p] = m;
                continue;
            }
            if (!prev.have_prev || !prev.have) continue;
            const int8_t* d = &P.v[((size_t)f * (H / 8) * (W / 8) + (size_t)(y / 8) * (W / 8) + x / 8) * 2];
            const int qy = y + d[0], qx = x + d[1];
            CHECK(qy >= 0 && qy < H && qx >= 0 && qx < W);
            const size_t q = (size_t)qy * W + qx;
            if (!(prev.M[q] != 0.f)) continue;
            if (!(fabs((double)P.L[f * hw + p] - (double)prev.l[q]) <= tol)) continue;
            if (!(life == 0 || prev.G[q] + 1 <= life)) continue;
            out.A[p] = prev.A[q]; out.A[hw + p] = prev.A[hw + q]; out.M[p] = prev.M[q]; out.G[p] = prev.G[q] + 1;
        }
    return out;
}

static bool same_bits(float a, float b) { return memcmp(&a, &b, 4) == 0; }

// frames [f0, f0 + n) of P as ONE call from `start`: every (frame, pixel) by the walk, on exactly-sized copies, against the recursion
static State check_call(const Planes& P, int f0, int n, const State& start, int life, double tol) {
    const int H = P.H, W = P.W;
    const size_t hw = (size_t)H * W, vb = (size_t)(H / 8) * (W / 8) * 2;
    const std::vector<float> ab(P.ab.begin() + f0 * 2 * hw, P.ab.begin() + (f0 + n) * 2 * hw), mask(P.mask.begin() + f0 * hw, P.mask.begin() + (f0 + n) * hw),
        L(P.L.begin() + f0 * hw, P.L.begin() + (f0 + n) * hw);
    const std::vector<int8_t> v(P.v.begin() + f0 * vb, P.v.begin() + (f0 + n) * vb);
    State st = start;
    for (int f = 0; f < n; ++f) {
        const State next = recursion_frame(P, f0 + f, st, life, tol);
        for (size_t p = 0; p < hw; ++p) {
            const TrackHit h = track_walk(ab.data(), mask.data(), L.data(), start.l.data(), v.data(), start.A.data(), start.M.data(), start.G.data(),
                                          start.have_prev ? 1 : 0, start.have ? 1 : 0, f, (int)p, H, W, life, tol);
            CHECK(same_bits(h.a, next.A[p]) && same_bits(h.b, next.A[hw + p]) && same_bits(h.m, next.M[p]) && h.age == next.G[p]);
        }
        st = next;
    }
    return st;
}

static int check_walks() {
    int calls = 0;
    for (const auto& net : {std::pair<int, int>{8, 8}, {8, 24}, {16, 24}, {24, 16}}) {
        const int H = net.first, W = net.second, n = 6;
        const size_t hw = (size_t)H * W;
        Planes P(n, H, W);
        unsigned seed = 12345u + (unsigned)(H * 100 + W);
        auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (seed >> 8) & 0xffff; };
        // L: a texture in steps of 1/4 that drifts little from frame to frame, with jumps above tol, values exactly tol apart, and a NaN
        for (size_t p = 0; p < hw; ++p) P.L[p] = (float)(rnd() % 400) * 0.25f - 50.f;
        for (int f = 1; f < n; ++f)
            for (size_t p = 0; p < hw; ++p) {
                const unsigned r = rnd() % 16;
                P.L[f * hw + p] = P.L[(f - 1) * hw + p] + (r < 10 ? (float)(r % 5) * 0.25f : r < 12 ? 8.f : r < 14 ? -8.25f : 20.f);
            }
        P.L[3 * hw + hw / 2] = NAN;
        // vectors: valid ones that differ block by block and frame by frame
        for (int f = 0; f < n; ++f)
            for (int by = 0; by < H / 8; ++by)
                for (int bx = 0; bx < W / 8; ++bx) {
                    int dy = (int)(rnd() % 7) - 3, dx = (int)(rnd() % 7) - 3;
                    if (!motion_valid(by, bx, dy, 0, H, W)) dy = 0;
                    if (!motion_valid(by, bx, 0, dx, H, W)) dx = 0;
                    CHECK(motion_valid(by, bx, dy, dx, H, W));
                    int8_t* d = &P.v[((size_t)f * (H / 8) * (W / 8) + (size_t)by * (W / 8) + bx) * 2];
                    d[0] = (int8_t)dy; d[1] = (int8_t)dx;
                }
        // hints: a dense patch at frame 0, a sparse sprinkle later (own over carried), two mask values
        for (int f = 0; f < n; ++f)
            for (size_t p = 0; p < hw; ++p) {
                const bool hint = f == 0 ? rnd() % 3 == 0 : rnd() % 23 == 0;
                if (!hint) continue;
                P.ab[(size_t)f * 2 * hw + p] = (float)(rnd() % 160) - 80.f; P.ab[((size_t)f * 2 + 1) * hw + p] = (float)(rnd() % 160) - 80.f;
                P.mask[f * hw + p] = rnd() % 2 ? 1.f : 0.5f;
            }
        for (int life : {0, 1, 2}) {
            for (double tol : {8.0, 0.0, 100.0}) {
                const State none(hw);
                const State whole = check_call(P, 0, n, none, life, tol);       // one call from a fresh sequence
                State st = check_call(P, 0, 2, none, life, tol);                // ... and split 2 + 1 + 3: the state is read at displaced pixels
                st = check_call(P, 2, 1, st, life, tol);
                st = check_call(P, 3, 3, st, life, tol);
                CHECK(memcmp(st.A.data(), whole.A.data(), 2 * hw * 4) == 0 && memcmp(st.M.data(), whole.M.data(), hw * 4) == 0 && st.G == whole.G);
                State dropped = check_call(P, 0, 3, none, life, tol);           // a predecessor whose tracked planes were dropped
                dropped.have = false;
                check_call(P, 3, 3, dropped, life, tol);
                calls += 6;
            }
        }
        // an age that would pass 2^31 - 1 stops there
        State old(hw);
        old.have_prev = old.have = true;
        for (size_t p = 0; p < hw; ++p) { old.M[p] = 1.f; old.G[p] = kTrackMaxAge; old.l[p] = P.L[p]; }
        std::vector<float> no_hint(hw, 0.f), ab0(2 * hw, 0.f);
        std::vector<int8_t> v0((size_t)(H / 8) * (W / 8) * 2, 0);
        const TrackHit h = track_walk(ab0.data(), no_hint.data(), P.L.data(), old.l.data(), v0.data(), old.A.data(), old.M.data(), old.G.data(), 1, 1, 0, 0, H,
                                      W, 0, 8.0);
        CHECK(h.m == 1.f && h.age == kTrackMaxAge);
        // a vector that would leave the plane counts as (0, 0): no read outside, whatever the vectors hold
        v0[0] = -7; v0[1] = -7;
        CHECK(track_step(v0.data(), 0, H, W) == 0);
        v0[0] = 0; v0[1] = 0;
    }
    return calls;
}

// ---- the plan: tracking takes no room in it
static const int H = 8, W = 16, NB = 8;
alignas(4) static uint8_t g_px[16], g_out[16];

struct Call {
    std::vector<idc_ref_image> images;
    std::vector<idc_gray_image> grays;
    std::vector<uint8_t*> outs;
    std::vector<int32_t> offs;
    std::vector<idc_hint> hints;
    BatchCall c;
};
static const int kSizes[][2] = {{5, 7}, {8, 16}, {9, 12}, {8, 13}, {1, 1}, {30, 5}, {3, 40}, {64, 48}};

static Call* ragged(int first, int n, int gray_bits, unsigned flags, int filter) {
    Call* k = new Call();
    for (int i = 0; i < n; ++i) {
        const int* s = kSizes[(first + i) % 8];
        k->images.push_back({g_px, s[0], s[1]});
        k->grays.push_back({g_px, s[0], s[1]});
        k->outs.push_back(g_out);
    }
    k->offs.assign(1, 0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j <= i % 3; ++j) k->hints.push_back({j, i, j + 3, i + 20 * (j == 2), 10.f + i, 20.f + j, 30.f});
        k->offs.push_back((int32_t)k->hints.size());
    }
    k->c.n = n; k->c.ragged = true; k->c.flags = flags; k->c.mode = IDC_HINT_AB; k->c.mask_value = 1.f;
    k->c.images = gray_bits ? nullptr : k->images.data(); k->c.grays = gray_bits ? k->grays.data() : nullptr; k->c.outs = k->outs.data();
    k->c.gray_bits = gray_bits; k->c.out_bits = (flags & IDC_BATCH_OUT_RGB16) ? 16 : 8;
    k->c.hint_offsets = k->offs.data(); k->c.hints = k->hints.data();
    k->c.ingest_filter = filter;
    return k;
}

static Call* same_size(int n, int sh, int sw, unsigned flags) {
    Call* k = new Call();
    k->offs.assign(n + 1, 0);
    k->c.n = n; k->c.src_h = sh; k->c.src_w = sw; k->c.rgb_in = g_px; k->c.rgb_out = g_out; k->c.flags = flags; k->c.mask_value = 1.f;
    k->c.hint_offsets = k->offs.data();
    return k;
}

struct Filled { BatchPlan p; std::vector<unsigned char> meta; };
static Filled run(const BatchCall& c) {
    Filled f;
    std::string why;
    CHECK(plan_batch(c, H, W, NB, &f.p, &why) == IDC_OK);
    f.meta.assign(f.p.meta_bytes, 0xA5);
    fill_batch_meta(c, f.p, H, W, f.meta.data());
    return f;
}

static void check_same(const Filled& a, const Filled& b) {
    const BatchPlan &p = a.p, &q = b.p;
    CHECK(p.want_rgb == q.want_rgb && p.reveal == q.reveal && p.dist == q.dist && p.score == q.score && p.source_out == q.source_out);
    CHECK(p.n_hints == q.n_hints && p.kept == q.kept && p.in_bytes == q.in_bytes && p.rgb_bytes == q.rgb_bytes);
    CHECK(p.table_at == q.table_at && p.hints_at == q.hints_at && p.orig_at == q.orig_at && p.meta_floor == q.meta_floor);
    CHECK(p.cols_at == q.cols_at && p.cols_bytes == q.cols_bytes && p.max_tiles == q.max_tiles && p.max_pixels == q.max_pixels);
    CHECK(p.bpp_in == q.bpp_in && p.bpp_out == q.bpp_out && p.naa == q.naa && p.aa_tiles == q.aa_tiles && p.aa_at == q.aa_at);
    CHECK(p.src_bytes == q.src_bytes && p.view_at == q.view_at && p.jobs_at == q.jobs_at && p.pieces.size() == q.pieces.size());
    CHECK(p.ycc_bytes == q.ycc_bytes && p.ycc_at == q.ycc_at && p.ycc_blocks == q.ycc_blocks && p.meta_bytes == q.meta_bytes);
    for (size_t i = 0; i < p.pieces.size(); ++i)
        CHECK(p.pieces[i].in == q.pieces[i].in && p.pieces[i].out == q.pieces[i].out && p.pieces[i].in_at == q.pieces[i].in_at &&
              p.pieces[i].in_bytes == q.pieces[i].in_bytes && p.pieces[i].out_at == q.pieces[i].out_at && p.pieces[i].out_bytes == q.pieces[i].out_bytes);
    CHECK(a.meta == b.meta);
}

static int check_plans() {
    const unsigned SRC = IDC_BATCH_OUT_SOURCE;
    std::vector<Call*> calls = {
        ragged(0, 8, 0, 0, 0),       ragged(3, 5, 0, SRC, 0),      ragged(1, 7, 8, SRC, 0),      ragged(5, 3, 16, 0, 0),
        ragged(4, 4, 16, SRC | IDC_BATCH_OUT_RGB16, 0),            ragged(2, 6, 0, SRC, IDC_FILTER_ANTIALIAS),
        same_size(3, 5, 7, 0),       same_size(8, 9, 13, SRC),
    };
    for (Call* k : calls) {
        const Filled plain = run(k->c);                  // the field at its default: what a call built without it holds
        BatchCall c = k->c;
        c.track = {1, 3, 2.0};                           // tracking on under a filter that is off: nothing
        check_same(run(c), plain);
        c.temporal = {1, 0.6, 4.0, 12.0, 1};
        c.motion = {1, 4, 0.5};
        c.track = {0, 7, 50.0};                          // filter and motion on, tracking off: the parent's plan
        check_same(run(c), plain);
        c.track = {1, 0, 8.0};                           // all three on: still no plan byte, no block byte
        check_same(run(c), plain);
        delete k;
    }
    return (int)calls.size();
}

int main() {
    check_params();
    const long long nets = check_sizes();
    const int walks = check_walks();
    const int calls = check_plans();
    printf("track_selftest: ok (%lld nets, %d walked calls, %d plans)\n", nets, walks, calls);
    return 0;
}
