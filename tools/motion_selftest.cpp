// motion_selftest -- csrc/idc_motion.h and csrc/idc_batch.h for the motion compensation of the temporal ab filter, without a device.  Host code
// only, no library, no HIP runtime call (tests/test_motion_cpu.py runs this; `make motion_selftest SAN=1` builds it under ASan + UBSan, where the
// exactly-sized arrays turn an index past a plane, the LDS window or the scratch into a report).
//   ranks    for every search 0..7: motion_rank is a permutation of 0 .. candidates-1 that agrees with a sort by (dy^2 + dx^2, dy, dx), rank 0
//            is (0, 0), and the kernel's nested count gives the same rank.
//   valid    for every net size H, W in 8, 16 .. 512 and every search: a candidate is valid for a block iff every pixel of the displaced block
//            is inside the plane ((0, 0) always is); rows and columns separately everywhere, block by block on the small nets.
//   lds      the search kernel's fill loops, indexed as the kernel indexes them, write every cell they touch inside the tile and the window;
//            every cell a valid candidate of a block inside the plane reads was written from a pixel INSIDE the plane, and is the pixel the
//            rule names.
//   dealing  the threads' (block, candidate) items cover every block of the tile and every candidate exactly once; the tiles' blocks cover
//            every block of the plane exactly once.
//   scratch  the vectors take n * H/8 * W/8 * 2 bytes.
//   params   idc_set_temporal_motion's ranges, NaN outside.
//   plan     a call with motion off and on against the same call without the field: every plan field and every byte of the metadata block.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "idc_motion.h"
#include "idc_batch.h"

using namespace idc;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

static void check_ranks() {
    CHECK(kMotionBlock == 8 && kMotionMaxSearch == 7 && kMotionMaxCandidates == 225 && kMotionThreads == 256 && kMotionTileBlocks == 16);
    CHECK(kMotionLanes == 16 && kMotionWinH == 30 && kMotionWinW == 78);
    for (int S = 0; S <= kMotionMaxSearch; ++S) {
        const int n = motion_candidates(S), side = 2 * S + 1;
        CHECK(n == side * side && n <= kMotionMaxCandidates);
        struct Cand { int n2, dy, dx, ci; };
        std::vector<Cand> sorted;
        for (int ci = 0; ci < n; ++ci) {
            const int dy = motion_cand_dy(ci, S), dx = motion_cand_dx(ci, S);
            CHECK(dy >= -S && dy <= S && dx >= -S && dx <= S && (dy + S) * side + (dx + S) == ci);
            sorted.push_back({dy * dy + dx * dx, dy, dx, ci});
        }
        std::sort(sorted.begin(), sorted.end(), [](const Cand& a, const Cand& b) {
            if (a.n2 != b.n2) return a.n2 < b.n2;
            if (a.dy != b.dy) return a.dy < b.dy;
            return a.dx < b.dx;
        });
        std::vector<int> seen((size_t)n, 0);
        for (int r = 0; r < n; ++r) {
            CHECK(motion_rank(sorted[r].ci, S) == r);
            ++seen.at((size_t)motion_rank(sorted[r].ci, S));
            int count = 0;                               // the kernel's nested loops
            for (int a = -S; a <= S; ++a)
                for (int c = -S; c <= S; ++c) count += motion_before(a, c, sorted[r].dy, sorted[r].dx) ? 1 : 0;
            CHECK(count == r && r <= 255);
        }
        for (int r = 0; r < n; ++r) CHECK(seen[r] == 1);
        CHECK(sorted[0].dy == 0 && sorted[0].dx == 0);
        CHECK(!motion_before(0, 0, 0, 0) && motion_before(0, -1, 0, 1) && motion_before(-1, 0, 0, -1) && motion_before(0, 1, 1, 0));
        // the dealing: every (block, candidate) exactly once
        std::vector<int> dealt((size_t)kMotionTileBlocks * n, 0);
        for (int t = 0; t < kMotionThreads; ++t) {
            const int b = motion_thread_block(t);
            CHECK(b >= 0 && b < kMotionTileBlocks);
            for (int k = 0; k < motion_rounds(S); ++k) {
                const int ci = motion_thread_cand(t, k);
                if (ci < n) ++dealt.at((size_t)b * n + ci);
            }
            CHECK(motion_thread_cand(t, motion_rounds(S)) >= n);      // nothing is left behind the last round
        }
        for (size_t i = 0; i < dealt.size(); ++i) CHECK(dealt[i] == 1);
    }
}

static bool inside_by_pixels(int j0, int dj, int extent) {       // every pixel of rows / columns j0 + dj .. j0 + dj + 7 inside 0 .. extent-1
    for (int r = 0; r < kMotionBlock; ++r)
        if (j0 + dj + r < 0 || j0 + dj + r >= extent) return false;
    return true;
}

static void check_valid_axis(int extent) {
    for (int b = 0; b < extent / kMotionBlock; ++b)
        for (int d = -kMotionMaxSearch; d <= kMotionMaxSearch; ++d) {
            const bool want = inside_by_pixels(b * kMotionBlock, d, extent);
            CHECK(motion_valid(b, 0, d, 0, extent, 8) == want && motion_valid(0, b, 0, d, 8, extent) == want);
        }
}

// one tile of the search kernel on an H x W plane at search S: the fill loops and every read, on exactly-sized arrays
// (every: all 64 pixels of every read; else the block's four corners, which bound the rest: the indices are affine in r and c)
static void check_tile(int H, int W, int S, int tile, std::vector<unsigned char>& block_hit, bool every) {
    const int tiles_x = temporal_tiles_x(W);
    const int j0 = (tile / tiles_x) * kTemporalTileH, i0 = (tile % tiles_x) * kTemporalTileW;
    std::vector<int> cur((size_t)kTemporalTileH * kTemporalTileW, -2), win((size_t)kMotionWinH * kMotionWinW, -2);      // -2: never written
    for (int t = 0; t < kMotionThreads; ++t) {           // the tile: 4 pixels a thread, inside together
        const int r = t >> 4, c4 = (t & 15) * 4;
        const bool in = j0 + r < H && i0 + c4 < W;
        for (int k = 0; k < 4; ++k) {
            CHECK(in == (j0 + r < H && i0 + c4 + k < W));
            if (in) CHECK((size_t)(j0 + r) * W + i0 + c4 + k < (size_t)H * W);
            cur.at((size_t)r * kTemporalTileW + c4 + k) = in ? (j0 + r) * W + i0 + c4 + k : -1;
        }
    }
    const int ww = kTemporalTileW + 2 * S, cells = (kTemporalTileH + 2 * S) * ww;
    for (int idx = 0; idx < cells; ++idx) {
        const int jj = idx / ww, ii = idx - jj * ww;
        CHECK(jj < kMotionWinH && ii < kMotionWinW);
        const int gj = j0 - S + jj, gi = i0 - S + ii;
        const bool in = gj >= 0 && gj < H && gi >= 0 && gi < W;
        CHECK(win.at((size_t)jj * kMotionWinW + ii) == -2);
        win.at((size_t)jj * kMotionWinW + ii) = in ? gj * W + gi : -1;
    }
    const int side = 2 * S + 1, ncand = side * side;
    for (int b = 0; b < kMotionTileBlocks; ++b) {
        const int bj = b / kMotionTileBlocksX, bi = b % kMotionTileBlocksX;
        const int by = j0 / kMotionBlock + bj, bx = i0 / kMotionBlock + bi;
        if (!(by < motion_blocks_y(H) && bx < motion_blocks_x(W))) continue;
        ++block_hit.at((size_t)by * motion_blocks_x(W) + bx);
        for (int ci = 0; ci < ncand; ++ci) {
            const int dy = ci / side - S, dx = ci % side - S;
            const bool ok = motion_valid(by, bx, dy, dx, H, W);
            CHECK(ok == (inside_by_pixels(by * kMotionBlock, dy, H) && inside_by_pixels(bx * kMotionBlock, dx, W)));
            if (!ok) continue;
            const int step = every ? 1 : kMotionBlock - 1;
            for (int r = 0; r < kMotionBlock; r += step)
                for (int c = 0; c < kMotionBlock; c += step) {
                    CHECK(cur.at((size_t)(bj * kMotionBlock + r) * kTemporalTileW + bi * kMotionBlock + c) == (by * kMotionBlock + r) * W + bx * kMotionBlock + c);
                    CHECK(win.at((size_t)(bj * kMotionBlock + S + dy + r) * kMotionWinW + bi * kMotionBlock + S + dx + c) ==
                          (by * kMotionBlock + r + dy) * W + bx * kMotionBlock + c + dx);
                }
        }
    }
}

static long long check_nets() {
    long long checked = 0;
    for (int X = 8; X <= 512; X += 8) check_valid_axis(X);
    for (int H = 8; H <= 512; H += 8)
        for (int W = 8; W <= 512; W += 8) {
            CHECK(motion_blocks(H, W) == (H / 8) * (W / 8) && motion_blocks_y(H) * 8 == H && motion_blocks_x(W) * 8 == W);
            // every tile's LDS walk on the small nets and on a sweep, the first and last tile elsewhere
            const bool full = (H <= 40 && W <= 136) || (H == 168 && W % 136 == 0) || (H == 512 && W == 512);
            const int tiles = temporal_tiles(H, W);
            for (int S = 0; S <= kMotionMaxSearch; ++S, ++checked) {
                std::vector<unsigned char> block_hit((size_t)motion_blocks(H, W), 0);
                if (full) {
                    for (int tile = 0; tile < tiles; ++tile) check_tile(H, W, S, tile, block_hit, true);
                    for (size_t b = 0; b < block_hit.size(); ++b) CHECK(block_hit[b] == 1);
                } else if (S == 0 || S == kMotionMaxSearch) {
                    check_tile(H, W, S, 0, block_hit, false);
                    if (tiles > 1) check_tile(H, W, S, tiles - 1, block_hit, false);
                }
            }
            for (int n : {1, 5, 32}) {
                CHECK(motion_vector_bytes(n, H, W) == (size_t)n * (H / 8) * (W / 8) * 2 && motion_vector_bytes(n, H, W) % 2 == 0);
                CHECK(motion_vector_bytes(n, H, W) == (size_t)n * motion_vector_bytes(1, H, W));
            }
        }
    CHECK(motion_vector_bytes(32, 256, 256) == 65536 && motion_vector_bytes(1, 8, 8) == 2 && motion_blocks(40, 72) == 45);
    return checked;
}

static void check_params() {
    const double nan = NAN;
    CHECK(motion_params_ok(1, 4, 0.5) && motion_params_ok(0, 0, 0.0) && motion_params_ok(1, 7, 1e6));
    CHECK(!motion_params_ok(2, 4, 0.5) && !motion_params_ok(-1, 4, 0.5));
    CHECK(!motion_params_ok(1, -1, 0.5) && !motion_params_ok(1, 8, 0.5));
    CHECK(!motion_params_ok(1, 4, -0.001) && !motion_params_ok(1, 4, 1.0000001e6) && !motion_params_ok(1, 4, nan) && !motion_params_ok(1, 4, INFINITY));
    const MotionParams d = motion_defaults();
    CHECK(d.on == 0 && d.search == 4 && d.penalty == 0.5);
}

// ---- the plan: motion takes no room in it
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
        c.motion = {1, 7, 2.0};                          // motion on under a filter that is off: nothing
        check_same(run(c), plain);
        c.temporal = {1, 0.6, 4.0, 12.0, 1};
        c.motion = {0, 3, 0.0};                          // the filter on, motion off
        check_same(run(c), plain);
        c.motion = {1, 4, 0.5};                          // both on: still no plan byte, no block byte
        check_same(run(c), plain);
        delete k;
    }
    return (int)calls.size();
}

int main() {
    check_ranks();
    const long long nets = check_nets();
    check_params();
    const int calls = check_plans();
    printf("motion_selftest: ok (%lld nets x searches, %d calls)\n", nets, calls);
    return 0;
}
