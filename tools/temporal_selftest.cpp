// temporal_selftest -- csrc/idc_temporal.h and csrc/idc_batch.h for the temporal ab filter, without a device.  Host code only, no library, no
// HIP runtime call (tests/test_temporal_cpu.py runs this; `make temporal_selftest SAN=1` builds it under ASan + UBSan, where the exactly-sized
// arrays turn an index past a plane, the LDS tile or the scratch into a report).
//   tiles    for every net size H, W in 8, 16 .. 512 and every radius 0..3: the threads of the diff kernel's workgroups, indexed as the kernel
//            indexes them, cover every pixel of the plane exactly once, each thread's 4 pixels are inside the plane together or outside
//            together, every LDS cell the fill loop and the window touch lies inside the tile, and the window of a pixel has as many taps as
//            the clipped box has; the partial count is the tile count.
//   blend    the items of the blend kernel's exact grid cover every value of the two channels exactly once, in bounds.
//   scratch  g and the partials do not overlap and fill the scratch exactly; the info block holds D [n] and the flags [n].
//   params   idc_set_temporal_filter's ranges, NaN outside.
//   plan     a call with the filter off against the same call without the field: every plan field and every byte of the metadata block; and
//            with it on: the same again (the filter takes no room in either).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "idc_temporal.h"
#include "idc_batch.h"

using namespace idc;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

static void check_net(int H, int W, int R, bool full) {
    const int tiles = temporal_tiles(H, W), tiles_x = temporal_tiles_x(W);
    CHECK(tiles == ((H + 15) / 16) * ((W + 63) / 64) && temporal_partials(H, W) == tiles && tiles >= 1 && tiles <= 65535);
    CHECK(kTemporalThreads == (kTemporalTileH * kTemporalTileW) / 4 && kTemporalLdsH == 22 && kTemporalLdsW == 70);
    std::vector<unsigned char> hit((size_t)H * W, 0);
    const int lw = kTemporalTileW + 2 * R, cells = (kTemporalTileH + 2 * R) * lw;
    for (int tile = 0; tile < tiles; ++tile) {
        const int j0 = (tile / tiles_x) * kTemporalTileH, i0 = (tile % tiles_x) * kTemporalTileW;
        CHECK(j0 < H && i0 < W);
        if (full || tile == 0 || tile == tiles - 1) {
            std::vector<unsigned char> lds((size_t)kTemporalLdsH * kTemporalLdsW, 0);
            for (int idx = 0; idx < cells; ++idx) {                    // the fill loop: every cell of the (16 + 2R) x (64 + 2R) tile once
                const int jj = idx / lw, ii = idx - jj * lw;
                CHECK(jj < kTemporalLdsH && ii < kTemporalLdsW);
                ++lds.at((size_t)jj * kTemporalLdsW + ii);
                const int gj = j0 - R + jj, gi = i0 - R + ii;
                if (gj >= 0 && gj < H && gi >= 0 && gi < W) CHECK((size_t)gj * W + gi < (size_t)H * W);
            }
            for (int t = 0; t < kTemporalThreads; ++t) {
                const int r = t >> 4, c4 = (t & 15) * 4, j = j0 + r, i = i0 + c4;
                if (!(j < H && i < W)) continue;
                for (int k = 0; k < 4; ++k) {
                    int taps = 0;
                    for (int dj = -R; dj <= R; ++dj) {
                        if (j + dj < 0 || j + dj >= H) continue;
                        for (int di = -R; di <= R; ++di) {
                            if (i + k + di < 0 || i + k + di >= W) continue;
                            CHECK(lds.at((size_t)(r + R + dj) * kTemporalLdsW + (c4 + k + R + di)) == 1);     // a cell the fill loop wrote
                            ++taps;
                        }
                    }
                    const int rows = (j + R < H - 1 ? j + R : H - 1) - (j - R > 0 ? j - R : 0) + 1;
                    const int cols = (i + k + R < W - 1 ? i + k + R : W - 1) - (i + k - R > 0 ? i + k - R : 0) + 1;
                    CHECK(taps == rows * cols && taps >= 1);
                }
            }
        }
        if (R != 0) continue;                            // the cover does not depend on the radius
        for (int t = 0; t < kTemporalThreads; ++t) {
            const int r = t >> 4, c4 = (t & 15) * 4, j = j0 + r, i = i0 + c4;
            const bool inside = j < H && i < W;
            for (int k = 0; k < 4; ++k) CHECK(inside == (j < H && i + k < W));      // 4 pixels together
            if (inside)
                for (int k = 0; k < 4; ++k) ++hit.at((size_t)j * W + i + k);
        }
    }
    for (size_t p = 0; p < hit.size(); ++p) CHECK(hit[p] == (R == 0 ? 1 : 0));
}

static void check_blend(int H, int W) {
    const size_t hw = (size_t)H * W, quarter = hw / kTemporalItemPixels;
    CHECK(hw % kTemporalItemPixels == 0 && (size_t)temporal_items(H, W) == 2 * quarter);
    const int blocks = temporal_blend_blocks(H, W);
    CHECK(blocks >= 1 && (size_t)blocks * kTemporalThreads >= 2 * quarter && (size_t)(blocks - 1) * kTemporalThreads < 2 * quarter);
    std::vector<unsigned char> hit(2 * hw, 0);
    for (size_t item = 0; item < (size_t)blocks * kTemporalThreads; ++item) {
        if (item >= 2 * quarter) continue;
        const int ch = item >= quarter ? 1 : 0;
        const size_t pix = (item - (ch ? quarter : 0)) * kTemporalItemPixels;
        for (int k = 0; k < kTemporalItemPixels; ++k) ++hit.at((size_t)ch * hw + pix + k);
    }
    for (size_t p = 0; p < hit.size(); ++p) CHECK(hit[p] == 1);
}

static long long check_nets() {
    long long checked = 0;
    for (int H = 8; H <= 512; H += 8)
        for (int W = 8; W <= 512; W += 8) {
            // every radius everywhere; the LDS walk of every tile on the small nets and on a sweep, of the first and last tile elsewhere
            const bool full = (H <= 64 && W <= 136) || (H % 120 == 0 && W % 136 == 0) || (H == 512 && W == 512);
            for (int R = 0; R <= kTemporalMaxRadius; ++R, ++checked) check_net(H, W, R, full);
            check_blend(H, W);
            for (int n : {1, 5, 32}) {
                CHECK(temporal_g_bytes(n, H, W) == (size_t)n * H * W * 8 && temporal_part_at(n, H, W) == temporal_g_bytes(n, H, W));
                CHECK(temporal_scratch_bytes(n, H, W) == temporal_part_at(n, H, W) + (size_t)n * temporal_partials(H, W) * 8);
                CHECK(temporal_part_at(n, H, W) % 16 == 0);
                CHECK(temporal_info_cut_at(n) == (size_t)n * 8 && temporal_info_bytes(n) == (size_t)n * 12);
            }
        }
    CHECK(temporal_tiles(256, 256) == 64 && temporal_tiles(512, 512) == 256 && temporal_tiles(8, 8) == 1 && temporal_tiles(40, 72) == 6);
    CHECK(temporal_blend_blocks(256, 256) == 128 && temporal_blend_blocks(8, 8) == 1 && temporal_blend_blocks(40, 72) == 6);
    return checked;
}

static void check_params() {
    const double nan = NAN;
    CHECK(temporal_params_ok(1, 0.6, 4.0, 1, 12.0) && temporal_params_ok(0, 0.0, 0.5, 0, 0.0) && temporal_params_ok(1, 0.95, 100.0, 3, 100.0));
    CHECK(!temporal_params_ok(2, 0.6, 4.0, 1, 12.0) && !temporal_params_ok(-1, 0.6, 4.0, 1, 12.0));
    CHECK(!temporal_params_ok(1, -0.01, 4.0, 1, 12.0) && !temporal_params_ok(1, 0.951, 4.0, 1, 12.0) && !temporal_params_ok(1, nan, 4.0, 1, 12.0));
    CHECK(!temporal_params_ok(1, 0.6, 0.49, 1, 12.0) && !temporal_params_ok(1, 0.6, 100.5, 1, 12.0) && !temporal_params_ok(1, 0.6, nan, 1, 12.0));
    CHECK(!temporal_params_ok(1, 0.6, 4.0, -1, 12.0) && !temporal_params_ok(1, 0.6, 4.0, 4, 12.0));
    CHECK(!temporal_params_ok(1, 0.6, 4.0, 1, -1.0) && !temporal_params_ok(1, 0.6, 4.0, 1, 100.5) && !temporal_params_ok(1, 0.6, 4.0, 1, nan));
    const TemporalParams d = temporal_defaults();
    CHECK(d.on == 0 && d.strength == 0.6 && d.sigma == 4.0 && d.radius == 1 && d.cut == 12.0);
}

// ---- the plan: the filter takes no room in it
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
        c.temporal = {0, 0.3, 9.0, 0.0, 3};              // off, whatever the parameters
        check_same(run(c), plain);
        c.temporal = {1, 0.6, 4.0, 12.0, 1};             // on: still no plan byte, no block byte
        check_same(run(c), plain);
        c.out_format = IDC_OUT_NV12;
        if (c.out_bits != 16) {
            BatchCall d = k->c;
            d.out_format = IDC_OUT_NV12;
            check_same(run(c), run(d));
        }
        delete k;
    }
    return (int)calls.size();
}

int main() {
    const long long nets = check_nets();
    check_params();
    const int calls = check_plans();
    printf("temporal_selftest: ok (%lld nets x radii, %d calls)\n", nets, calls);
    return 0;
}
