// layer_selftest -- csrc/idc_layer.h and csrc/idc_batch.h for painted hint layers, without a device.  Host code only, no library, no HIP runtime
// call (tests/test_layer_cpu.py runs this; `make layer_selftest SAN=1` builds it under ASan + UBSan, where the exactly-sized metadata block turns
// a write past meta_bytes into a report).
//   spans   for every layer size 1..16384 against H in {8, 64, 256}: every span is non-empty, inside the layer and exactly the pixels whose
//           extent overlaps the cell's; together the spans cover the layer without a gap; none is longer than layer_span_bound.
//   form    thread or wave from (lh, lw, H, W) alone: the header's examples, the footprint bound of the thread form, and one workgroup count per
//           layer whatever its place in a call and whatever the call's n.
//   free    a call without layers and the same call with a table whose every entry is empty: the same plan fields, pieces and block bytes.
//   layers  the LayerDesc table behind everything else, the packed pieces in image order, the copy runs of mixed pinned / pageable layers.
//   refuse  every refusal the plan makes for layers.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "idc_layer.h"
#include "idc_batch.h"

using namespace idc;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

static const int H = 8, W = 12, NB = 8;      // net size of the plans (not square: an H / W mix-up shows) and max_batch
alignas(4) static uint8_t g_px[16], g_out[16], g_rgba[16];      // any non-null address: the plan never reads the bytes
static int32_t g_cells[8];

static void check_spans() {
    const int nets[3] = {8, 64, 256};
    long long checked = 0;
    for (int out : nets)
        for (int l = 1; l <= kLayerMaxSide; ++l) {
            const int bound = layer_span_bound(l, out);
            int prev_hi = 0, longest = 0;
            for (int i = 0; i < out; ++i) {
                int lo, hi;
                layer_span(i, l, out, lo, hi);
                CHECK(lo < hi && lo >= 0 && hi <= l);
                CHECK(i > 0 ? lo <= prev_hi : lo == 0);                     // no pixel line between neighbours is left out
                // exactly the overlapping pixels: pixel k covers [k * out, (k + 1) * out), cell i covers [i * l, (i + 1) * l)
                const long long c0 = (long long)i * l, c1 = ((long long)i + 1) * l;
                CHECK((long long)lo * out < c1 && ((long long)lo + 1) * out > c0);
                CHECK(((long long)hi - 1) * out < c1 && (long long)hi * out > c0);
                CHECK(lo == 0 || (long long)lo * out <= c0);                // pixel lo - 1 ends at or in front of the cell
                CHECK(hi == l || (long long)hi * out >= c1);                // pixel hi begins at or behind it
                longest = longest > hi - lo ? longest : hi - lo;
                prev_hi = hi;
                ++checked;
            }
            CHECK(prev_hi == l);
            CHECK(longest <= bound && longest >= bound - 1);
        }
    printf("spans: %lld checked\n", checked);
}

static void check_form() {
    CHECK(!layer_wave_form(1024, 768, 256, 256) && layer_span_bound(1024, 256) == 4 && layer_span_bound(768, 256) == 3);
    CHECK(!layer_wave_form(1000, 700, 64, 64) && layer_span_bound(1000, 64) * layer_span_bound(700, 64) == 204);
    CHECK(layer_wave_form(65, 16384, 64, 64) && layer_span_bound(65, 64) * layer_span_bound(16384, 64) == 768);
    CHECK(!layer_wave_form(1, 1, 64, 64) && !layer_wave_form(64, 64, 64, 64) && layer_wave_form(16384, 16384, 256, 256));
    CHECK(layer_blocks(64, 64, 64, 64) == 4 && layer_blocks(65, 16384, 64, 64) == 256 && layer_blocks(3, 3, 8, 12) == 1 && layer_blocks(64, 64, 65, 63) == 4);
    // the thread form's promise: no footprint above kLayerThreadMaxPixels
    const int sides[] = {1, 7, 64, 100, 255, 256, 257, 1000, 1023, 1024, 1025, 4096, 16383, 16384};
    for (int lh : sides)
        for (int lw : sides) {
            if (layer_wave_form(lh, lw, 64, 64)) continue;
            long long worst = 0;
            for (int y = 0; y < 64; ++y)
                for (int x = 0; x < 64; ++x) {
                    int r0, r1, c0, c1;
                    layer_span(y, lh, 64, r0, r1);
                    layer_span(x, lw, 64, c0, c1);
                    worst = worst > (long long)(r1 - r0) * (c1 - c0) ? worst : (long long)(r1 - r0) * (c1 - c0);
                }
            CHECK(worst <= kLayerThreadMaxPixels);
        }
}

struct Call {
    std::vector<idc_ref_image> images;
    std::vector<idc_gray_image> grays;
    std::vector<uint8_t*> outs;
    std::vector<int32_t> offs;
    std::vector<idc_hint> hints;
    std::vector<idc_hint_layer> layers;
    BatchCall c;
};

static const int kSizes[][2] = {{5, 7}, {8, 12}, {9, 12}, {8, 13}, {1, 1}, {30, 5}, {3, 40}, {64, 48}};
static const int kLayerSizes[][2] = {{1, 1}, {3, 5}, {8, 12}, {7, 3}, {200, 2}, {2, 2}, {16, 4000}, {5, 5}};     // their pixel counts: 1, 15, 96, 21, 400, 4, 64000, 25

static Call* ragged(int first, int n, int gray_bits, unsigned flags, int mode, int filter) {
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
    k->c.n = n; k->c.ragged = true; k->c.flags = flags; k->c.mode = mode; k->c.mask_value = 1.f;
    k->c.images = gray_bits ? nullptr : k->images.data(); k->c.grays = gray_bits ? k->grays.data() : nullptr; k->c.outs = k->outs.data();
    k->c.gray_bits = gray_bits; k->c.out_bits = (flags & IDC_BATCH_OUT_RGB16) ? 16 : 8;
    k->c.hint_offsets = k->offs.data(); k->c.hints = k->hints.data();
    k->c.ingest_filter = filter;
    return k;
}

struct Filled { BatchPlan p; std::vector<unsigned char> meta; };

static Filled run(const BatchCall& c) {
    Filled f;
    std::string why;
    CHECK(plan_batch(c, H, W, NB, &f.p, &why) == IDC_OK);
    f.meta.assign(f.p.meta_bytes, 0xA5);      // exactly sized: a write past the end is the sanitizer's to find
    fill_batch_meta(c, f.p, H, W, f.meta.data());
    return f;
}

// today's fields, pieces and block bytes of q in p
static void check_same(const Filled& a, const Filled& b) {
    const BatchPlan &p = a.p, &q = b.p;
    CHECK(p.want_rgb == q.want_rgb && p.reveal == q.reveal && p.dist == q.dist && p.score == q.score && p.source_out == q.source_out);
    CHECK(p.n_hints == q.n_hints && p.kept == q.kept && p.in_bytes == q.in_bytes && p.rgb_bytes == q.rgb_bytes);
    CHECK(p.table_at == q.table_at && p.hints_at == q.hints_at && p.orig_at == q.orig_at && p.meta_floor == q.meta_floor);
    CHECK(p.cols_at == q.cols_at && p.cols_bytes == q.cols_bytes && p.max_tiles == q.max_tiles && p.max_pixels == q.max_pixels);
    CHECK(p.bpp_in == q.bpp_in && p.bpp_out == q.bpp_out && p.naa == q.naa && p.aa_tiles == q.aa_tiles && p.aa_at == q.aa_at);
    CHECK(p.src_bytes == q.src_bytes && p.view_at == q.view_at && p.jobs_at == q.jobs_at && p.pieces.size() == q.pieces.size());
    for (size_t i = 0; i < p.pieces.size(); ++i)
        CHECK(p.pieces[i].in == q.pieces[i].in && p.pieces[i].out == q.pieces[i].out && p.pieces[i].in_at == q.pieces[i].in_at &&
              p.pieces[i].in_bytes == q.pieces[i].in_bytes && p.pieces[i].out_at == q.pieces[i].out_at && p.pieces[i].out_bytes == q.pieces[i].out_bytes);
    CHECK(a.meta.size() >= b.meta.size() && memcmp(a.meta.data(), b.meta.data(), b.meta.size()) == 0);
}

static int check_plans() {
    const unsigned SRC = IDC_BATCH_OUT_SOURCE, R16 = IDC_BATCH_OUT_RGB16;
    std::vector<Call*> calls = {
        ragged(0, 8, 0, 0, IDC_HINT_AB, 0),          ragged(3, 5, 0, SRC, IDC_HINT_RGB, 0),      ragged(0, 2, 0, SRC, IDC_HINT_AB, 0),
        ragged(1, 7, 8, SRC, IDC_HINT_AB, 0),        ragged(0, 8, 16, SRC | R16, IDC_HINT_AB, 0), ragged(5, 3, 16, 0, IDC_HINT_RGB, 0),
        ragged(2, 6, 0, SRC, IDC_HINT_RGB, IDC_FILTER_ANTIALIAS),                                ragged(0, 1, 8, 0, IDC_HINT_AB, IDC_FILTER_ANTIALIAS),
    };
    int ci = 0;
    for (Call* k : calls) {
        const int n = k->c.n;
        const Filled plain = run(k->c);               // the new fields at their defaults
        CHECK(plain.p.n_layers == 0 && plain.p.layer_bytes == 0 && plain.p.layers_at == 0 && plain.p.layer_blocks == 0 && plain.p.layer_pieces.empty());
        // free: a table without a layer
        k->layers.assign(n, idc_hint_layer{nullptr, 0, 0});
        BatchCall c = k->c;
        c.has_layers = true; c.layers = k->layers.data(); c.alpha_min = 128; c.cover = 0; c.cells = g_cells;
        const Filled empty = run(c);
        check_same(empty, plain);
        CHECK(empty.p.meta_bytes == plain.p.meta_bytes && empty.meta == plain.meta && empty.p.n_layers == 0 && empty.p.layer_pieces.empty());
        c.mask_value = 0.f;                           // ... needs no mask_value either
        CHECK(run(c).p.meta_bytes == plain.p.meta_bytes);
        c.mask_value = 1.f;
        // layers: every second image (shifted per call), so that starts fall on every residue of pixels mod 4
        std::vector<int> with;
        for (int i = 0; i < n; ++i)
            if ((i + ci) % 3 != 2) { k->layers[i] = {g_rgba + (i % 2), kLayerSizes[(i + ci) % 8][0], kLayerSizes[(i + ci) % 8][1]}; with.push_back(i); }
        const Filled on = run(c);
        check_same(on, plain);
        const BatchPlan& p = on.p;
        CHECK(p.n_layers == (int)with.size() && p.layer_pieces.size() == with.size());
        CHECK(p.layers_at >= plain.p.meta_bytes && p.layers_at % 16 == 0 && p.layers_at - plain.p.meta_bytes < 16);
        CHECK(p.meta_bytes == p.layers_at + NB * sizeof(LayerDesc));
        const LayerDesc* tab = (const LayerDesc*)(on.meta.data() + p.layers_at);
        size_t at = 0, w = 0;
        int blocks = 0;
        for (int i = 0; i < NB; ++i) {
            if (w < with.size() && with[w] == i) {
                const idc_hint_layer& l = k->layers[i];
                const Piece& q = p.layer_pieces[w];
                CHECK(tab[i].off == (long long)at && tab[i].h == l.h && tab[i].w == l.w && at % 4 == 0);
                CHECK(q.in == l.rgba && q.out == nullptr && q.in_at == at && q.in_bytes == (size_t)l.h * l.w * 4 && q.out_bytes == 0);
                const int b = layer_blocks(l.h, l.w, H, W);
                // the form and the workgroup count are the sizes' alone: the same layer alone in a call of one image plans the same
                Call* one = ragged(0, 1, 0, 0, IDC_HINT_AB, 0);
                one->layers.assign(1, l);
                one->c.has_layers = true; one->c.layers = one->layers.data(); one->c.alpha_min = 1; one->c.cover = 255;
                CHECK(run(one->c).p.layer_blocks == b);
                delete one;
                blocks = blocks > b ? blocks : b;
                at += q.in_bytes;
                ++w;
            } else {
                CHECK(tab[i].off == 0 && tab[i].h == 0 && tab[i].w == 0);
            }
        }
        CHECK(p.layer_bytes == at && p.layer_blocks == blocks && blocks >= 1);
        // copy runs: pinned layers in place, pageable neighbours as one copy
        std::vector<Piece> pcs = p.layer_pieces;
        for (size_t i = 0; i < pcs.size(); ++i) pcs[i].in_pinned = (i % 3 == 1);
        const std::vector<CopyOp> ops = copy_runs(pcs, true);
        size_t covered = 0, i = 0;
        for (const CopyOp& o : ops) {
            CHECK(o.at == covered);
            if (o.piece >= 0) { CHECK((size_t)o.piece == i && pcs[i].in_pinned && o.bytes == pcs[i].in_bytes); ++i; }
            else { size_t b = 0; while (i < pcs.size() && !pcs[i].in_pinned) b += pcs[i++].in_bytes; CHECK(b == o.bytes); }
            covered += o.bytes;
        }
        CHECK(covered == p.layer_bytes && i == pcs.size());
        // refusals
        BatchPlan pb;
        std::string why;
        BatchCall bad = c;
        bad.layers = nullptr;                                        CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        bad = c; bad.alpha_min = 0;                                  CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        bad = c; bad.alpha_min = 256;                                CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        bad = c; bad.cover = -1;                                     CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        bad = c; bad.cover = 256;                                    CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        bad = c; bad.mask_value = 0.f;                               CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        bad = c; bad.mask_value = -0.f;                              CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        bad = c; bad.mask_value = INFINITY;                          CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        bad = c; bad.mask_value = NAN;                               CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        bad = c; bad.mode = IDC_HINT_REVEAL;                         CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        std::vector<idc_hint_layer> ls = k->layers;
        bad = c; bad.layers = ls.data();
        ls[with[0]].h = 0;                                           CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        ls[with[0]].h = 16385;                                       CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        ls[with[0]].h = 5; ls[with[0]].w = 0;                        CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        ls[with[0]].w = 16385;                                       CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        ls[with[0]].h = 16384; ls[with[0]].w = 16384;                // 1 GiB alone: allowed only when it is the one layer of the call
        CHECK(plan_batch(bad, H, W, NB, &pb, &why) == (with.size() > 1 ? IDC_ERR_INVALID_ARG : IDC_OK));
        CHECK(plan_batch(c, H, W, NB, &pb, &why) == IDC_OK);
        delete k;
        ++ci;
    }
    return (int)calls.size();
}

int main() {
    check_spans();
    check_form();
    const int calls = check_plans();
    printf("layer_selftest: ok (%d calls)\n", calls);
    return 0;
}
