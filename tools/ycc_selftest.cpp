// ycc_selftest -- csrc/idc_ycc.h and csrc/idc_batch.h for the YCbCr 4:2:0 output planes, without a device.  Host code only, no library, no HIP
// runtime call (tests/test_ycc_cpu.py runs this; `make ycc_selftest SAN=1` builds it under ASan + UBSan, where the exactly-sized metadata block
// turns a write past meta_bytes into a report).
//   sizes   for every h, w in 1..64 and a sweep up to 16384: the byte count, the plane offsets, and the strips -- each strip's Y and chroma runs
//           lie inside their own row of their own plane, and together the strips of an image write every byte of its block exactly once (small
//           sizes: byte by byte; the sweep: by count); the workgroup count covers the strips and no more than it must.
//   packed  the blocks of a packed call lie back to back in image order and never overlap; the RGB offsets are those of the packed results.
//   off     a call with the format IDC_OUT_RGB: the plan fields, pieces and block bytes of the same call built without the new fields.
//   on      the YccDesc table behind everything else, the pieces' out_at / out_bytes, ycc_bytes, ycc_blocks; net size and source size, same-size
//           and ragged, grey sources, antialiased ingestion and layers in front of it.
//   refuse  an unknown format or matrix, and IDC_BATCH_OUT_RGB16 with a YCbCr format (IDC_ERR_UNSUPPORTED).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "idc_ycc.h"
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

// the bytes the strips of one image write, as the kernel derives them: run = (offset in the block, count)
struct Run { size_t at; int count; };
static void strip_runs(int h, int w, long long strip, bool nv12, std::vector<Run>* runs) {
    const int cw = ycc_chroma_w(w), rs = ycc_row_strips(w);
    const int j = (int)(strip / rs), t = (int)(strip - (long long)j * rs);
    const int y0 = 2 * j, x0 = kYccStripPixels * t;
    const int ny = h - y0 < 2 ? h - y0 : 2, nx = w - x0 < kYccStripPixels ? w - x0 : kYccStripPixels, nc = (nx + 1) / 2;
    CHECK(ny >= 1 && nx >= 1 && j < ycc_chroma_h(h));
    for (int r = 0; r < ny; ++r) {
        runs->push_back({(size_t)(y0 + r) * w + x0, nx});
        CHECK(x0 + nx <= w && y0 + r < h);                                   // inside its own row of the Y plane
    }
    const size_t c_at = (size_t)j * cw + (size_t)kYccStripBlocks * t;
    CHECK(kYccStripBlocks * t + nc <= cw);                                  // inside its own chroma row
    if (nv12) {
        runs->push_back({ycc_cb_at(h, w) + 2 * c_at, 2 * nc});
    } else {
        runs->push_back({ycc_cb_at(h, w) + c_at, nc});
        runs->push_back({ycc_cr_at(h, w) + c_at, nc});
    }
}

static void check_size(int h, int w, bool bytewise) {
    const int ch = (h + 1) / 2, cw = (w + 1) / 2;
    const size_t total = (size_t)h * w + 2 * (size_t)ch * cw;
    CHECK(ycc_chroma_h(h) == ch && ycc_chroma_w(w) == cw && ycc420_bytes(h, w) == total);
    CHECK(ycc_cb_at(h, w) == (size_t)h * w && ycc_cr_at(h, w) == (size_t)h * w + (size_t)ch * cw);
    const long long strips = ycc_strips(h, w);
    CHECK(strips == (long long)ch * ((cw + kYccStripBlocks - 1) / kYccStripBlocks));
    const int blocks = ycc_blocks(h, w);
    CHECK(blocks >= 1 && (long long)blocks * kYccThreads >= strips && (long long)(blocks - 1) * kYccThreads < strips && blocks <= 65536);
    if (!bytewise) {     // by count: the strips of the first, the last and a middle chroma row, and the arithmetic of the whole
        size_t bytes_per_row_pair = 0;
        for (int nv12 = 0; nv12 < 2; ++nv12) {
            const int rs = ycc_row_strips(w);
            const int rows[3] = {0, ch / 2, ch - 1};
            for (int j : rows) {
                std::vector<Run> runs;
                for (int t = 0; t < rs; ++t) strip_runs(h, w, (long long)j * rs + t, nv12 != 0, &runs);
                size_t sum = 0;
                for (const Run& r : runs) { CHECK(r.count >= 1 && r.at + r.count <= total); sum += r.count; }
                const int ny = h - 2 * j < 2 ? h - 2 * j : 2;
                CHECK(sum == (size_t)ny * w + 2 * (size_t)cw);
                bytes_per_row_pair = sum;
            }
        }
        (void)bytes_per_row_pair;
        return;
    }
    for (int nv12 = 0; nv12 < 2; ++nv12) {
        std::vector<unsigned char> hit(total, 0);
        for (long long s = 0; s < strips; ++s) {
            std::vector<Run> runs;
            strip_runs(h, w, s, nv12 != 0, &runs);
            for (const Run& r : runs)
                for (int k = 0; k < r.count; ++k) { CHECK(r.at + k < total); ++hit[r.at + k]; }
        }
        for (size_t i = 0; i < total; ++i) CHECK(hit[i] == 1);                  // every byte of the block once, none twice, none outside
    }
}

static long long check_sizes() {
    long long checked = 0;
    for (int h = 1; h <= 64; ++h)
        for (int w = 1; w <= 64; ++w, ++checked) check_size(h, w, true);
    const int sweep[] = {65, 83, 127, 128, 129, 187, 203, 211, 255, 256, 257, 768, 1000, 1023, 1024, 1025, 4095, 4096, 8191, 16383, 16384};
    for (int h : sweep)
        for (int w : sweep) { check_size(h, w, false); check_size(1, w, false); check_size(h, 1, false); checked += 3; }
    check_size(65, 16384, true); check_size(1, 1000, true); check_size(1000, 1, true); check_size(211, 83, true);
    CHECK(ycc420_bytes(0, 5) == 0 && ycc420_bytes(5, 0) == 0 && ycc420_bytes(16385, 1) == 0 && ycc420_bytes(1, 16385) == 0 && ycc420_bytes(-1, -1) == 0);
    CHECK(ycc420_bytes(1, 1) == 3 && ycc420_bytes(3, 3) == 17 && ycc420_bytes(1024, 768) == 1179648 && ycc420_bytes(16384, 16384) == 402653184u);
    CHECK(ycc_blocks(16384, 16384) == 65536 && ycc_blocks(1, 1) == 1 && ycc_blocks(1024, 768) == 192);
    // the matrices of the header's table
    const YccMatrix j = ycc_matrix(IDC_YCC_JFIF), v = ycc_matrix(IDC_YCC_BT709_VIDEO);
    CHECK(j.y[0] + j.y[1] + j.y[2] == 65536 && v.y[0] + v.y[1] + v.y[2] == 56284 && j.yoff == 0 && v.yoff == 16);
    CHECK(j.cb[0] + j.cb[1] + j.cb[2] == 0 && j.cr[0] + j.cr[1] + j.cr[2] == 0 && v.cb[0] + v.cb[1] + v.cb[2] == 0 && v.cr[0] + v.cr[1] + v.cr[2] == 0);
    CHECK(kYccI420 == IDC_OUT_I420 && kYccNV12 == IDC_OUT_NV12 && kYccChromaBias == (128 << 16) + 32767);
    return checked;
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

static Call* ragged(int first, int n, int gray_bits, unsigned flags, int mode, int filter, bool with_layers) {
    Call* k = new Call();
    for (int i = 0; i < n; ++i) {
        const int* s = kSizes[(first + i) % 8];
        k->images.push_back({g_px, s[0], s[1]});
        k->grays.push_back({g_px, s[0], s[1]});
        k->outs.push_back(g_out);
        k->layers.push_back(i % 2 ? idc_hint_layer{g_rgba, 3 + i, 5} : idc_hint_layer{nullptr, 0, 0});
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
    if (with_layers) { k->c.has_layers = true; k->c.layers = k->layers.data(); k->c.alpha_min = 128; k->c.cover = 0; }
    return k;
}

static Call* same_size(int n, int sh, int sw, unsigned flags, int filter) {
    Call* k = new Call();
    k->offs.assign(n + 1, 0);
    k->c.n = n; k->c.src_h = sh; k->c.src_w = sw; k->c.rgb_in = g_px; k->c.rgb_out = g_out; k->c.flags = flags; k->c.mask_value = 1.f;
    k->c.hint_offsets = k->offs.data(); k->c.ingest_filter = filter;
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

// every field of q that existed before the output format, its pieces but for where they come back, and its block bytes, in p
static void check_same(const Filled& a, const Filled& b, bool outs_too) {
    const BatchPlan &p = a.p, &q = b.p;
    CHECK(p.want_rgb == q.want_rgb && p.reveal == q.reveal && p.dist == q.dist && p.score == q.score && p.source_out == q.source_out);
    CHECK(p.n_hints == q.n_hints && p.kept == q.kept && p.in_bytes == q.in_bytes && p.rgb_bytes == q.rgb_bytes);
    CHECK(p.table_at == q.table_at && p.hints_at == q.hints_at && p.orig_at == q.orig_at && p.meta_floor == q.meta_floor);
    CHECK(p.cols_at == q.cols_at && p.cols_bytes == q.cols_bytes && p.max_tiles == q.max_tiles && p.max_pixels == q.max_pixels);
    CHECK(p.bpp_in == q.bpp_in && p.bpp_out == q.bpp_out && p.naa == q.naa && p.aa_tiles == q.aa_tiles && p.aa_at == q.aa_at);
    CHECK(p.src_bytes == q.src_bytes && p.view_at == q.view_at && p.jobs_at == q.jobs_at && p.pieces.size() == q.pieces.size());
    CHECK(p.n_layers == q.n_layers && p.layer_blocks == q.layer_blocks && p.layer_bytes == q.layer_bytes && p.layers_at == q.layers_at);
    CHECK(p.layer_pieces.size() == q.layer_pieces.size());
    for (size_t i = 0; i < p.pieces.size(); ++i) {
        CHECK(p.pieces[i].in == q.pieces[i].in && p.pieces[i].out == q.pieces[i].out && p.pieces[i].in_at == q.pieces[i].in_at &&
              p.pieces[i].in_bytes == q.pieces[i].in_bytes);
        if (outs_too) CHECK(p.pieces[i].out_at == q.pieces[i].out_at && p.pieces[i].out_bytes == q.pieces[i].out_bytes);
    }
    CHECK(a.meta.size() >= b.meta.size() && memcmp(a.meta.data(), b.meta.data(), b.meta.size()) == 0);
}

static int check_plans() {
    const unsigned SRC = IDC_BATCH_OUT_SOURCE;
    std::vector<Call*> calls = {
        ragged(0, 8, 0, 0, IDC_HINT_AB, 0, false),      ragged(3, 5, 0, SRC, IDC_HINT_RGB, 0, false),   ragged(0, 2, 0, SRC, IDC_HINT_AB, 0, true),
        ragged(1, 7, 8, SRC, IDC_HINT_AB, 0, false),    ragged(5, 3, 16, 0, IDC_HINT_RGB, 0, true),     ragged(4, 4, 16, SRC, IDC_HINT_AB, 0, false),
        ragged(2, 6, 0, SRC, IDC_HINT_RGB, IDC_FILTER_ANTIALIAS, true),                                 ragged(0, 1, 8, 0, IDC_HINT_AB, IDC_FILTER_ANTIALIAS, false),
        same_size(3, 5, 7, 0, 0),                       same_size(8, 9, 13, SRC, 0),                    same_size(2, 64, 48, SRC, IDC_FILTER_ANTIALIAS),
    };
    for (Call* k : calls) {
        const int n = k->c.n;
        // off: the defaults, and the format off under either matrix, are today's plan to the byte
        const Filled plain = run(k->c);
        CHECK(plain.p.ycc_bytes == 0 && plain.p.ycc_at == 0 && plain.p.ycc_blocks == 0);
        BatchCall c = k->c;
        c.out_format = IDC_OUT_RGB; c.out_matrix = IDC_YCC_BT709_VIDEO;
        const Filled off = run(c);
        check_same(off, plain, true);
        CHECK(off.p.meta_bytes == plain.p.meta_bytes && off.meta == plain.meta && off.p.ycc_bytes == 0);
        // ... and so is a call whose images stay on the device (an evaluation batch without rgb_out)
        if (k->c.ragged) {
            BatchCall ev = k->c;
            ev.eval = true; ev.outs = nullptr; ev.sse = (uint64_t*)g_out; ev.out_format = IDC_OUT_I420;
            BatchCall ev0 = ev; ev0.out_format = IDC_OUT_RGB;
            const Filled a = run(ev), b = run(ev0);
            check_same(a, b, true);
            CHECK(a.p.ycc_bytes == 0 && a.p.meta_bytes == b.p.meta_bytes && a.meta == b.meta);
        }
        // on
        for (int format = IDC_OUT_I420; format <= IDC_OUT_NV12; ++format) {
            c = k->c;
            c.out_format = format; c.out_matrix = format == IDC_OUT_NV12 ? IDC_YCC_BT709_VIDEO : IDC_YCC_JFIF;
            const Filled on = run(c);
            check_same(on, plain, false);
            const BatchPlan& p = on.p;
            CHECK(p.ycc_at >= plain.p.meta_bytes && p.ycc_at % 16 == 0 && p.ycc_at - plain.p.meta_bytes < 16);
            CHECK(p.meta_bytes == p.ycc_at + (size_t)n * sizeof(YccDesc));
            const YccDesc* tab = (const YccDesc*)(on.meta.data() + p.ycc_at);
            size_t src = 0, dst = 0;
            int blocks = 0;
            for (int i = 0; i < n; ++i) {
                const bool so = (c.flags & SRC) != 0;
                const int oh = !so ? H : c.ragged ? batch_image(c, i).h : c.src_h, ow = !so ? W : c.ragged ? batch_image(c, i).w : c.src_w;
                CHECK(tab[i].src == (long long)src && tab[i].dst == (long long)dst && tab[i].h == oh && tab[i].w == ow);
                // the RGB lies where today's plan has the piece come back from
                if (c.ragged) {
                    CHECK(plain.p.pieces[i].out_at == src && plain.p.pieces[i].out_bytes == (size_t)oh * ow * 3);
                    CHECK(p.pieces[i].out_at == dst && p.pieces[i].out_bytes == ycc420_bytes(oh, ow));
                }
                blocks = blocks > ycc_blocks(oh, ow) ? blocks : ycc_blocks(oh, ow);
                src += (size_t)oh * ow * 3; dst += ycc420_bytes(oh, ow);           // back to back, in image order: no two blocks overlap
            }
            CHECK(src == plain.p.rgb_bytes && dst == p.ycc_bytes && p.ycc_blocks == blocks && blocks >= 1);
            if (!c.ragged) CHECK(p.pieces.size() == 1 && p.pieces[0].out_at == 0 && p.pieces[0].out_bytes == (size_t)n * ycc420_bytes(tab[0].h, tab[0].w));
            CHECK(2 * p.ycc_bytes >= plain.p.rgb_bytes && p.ycc_bytes <= plain.p.rgb_bytes);          // between 3/2 and 3 bytes a pixel (1 x 1: 3)
            // the copy runs of mixed pinned / pageable destinations cover the blocks once
            std::vector<Piece> pcs = p.pieces;
            for (size_t i = 0; i < pcs.size(); ++i) pcs[i].out_pinned = (i % 3 == 1);
            size_t covered = 0;
            for (const CopyOp& o : copy_runs(pcs, false)) { CHECK(o.at == covered); covered += o.bytes; }
            CHECK(covered == p.ycc_bytes);
        }
        // refusals
        BatchPlan pb;
        std::string why;
        c = k->c; c.out_format = 3;                                      CHECK(plan_batch(c, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        c = k->c; c.out_format = -1;                                     CHECK(plan_batch(c, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        c = k->c; c.out_format = IDC_OUT_I420; c.out_matrix = 2;         CHECK(plan_batch(c, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        c = k->c; c.out_format = IDC_OUT_NV12; c.out_matrix = -1;        CHECK(plan_batch(c, H, W, NB, &pb, &why) == IDC_ERR_INVALID_ARG);
        if (k->c.gray_bits == 16 && (k->c.flags & SRC)) {
            c = k->c; c.flags |= IDC_BATCH_OUT_RGB16; c.out_bits = 16;
            CHECK(plan_batch(c, H, W, NB, &pb, &why) == IDC_OK);
            c.out_format = IDC_OUT_I420;                                 CHECK(plan_batch(c, H, W, NB, &pb, &why) == IDC_ERR_UNSUPPORTED);
        }
        delete k;
    }
    return (int)calls.size();
}

int main() {
    const long long sizes = check_sizes();
    const int calls = check_plans();
    printf("ycc_selftest: ok (%lld sizes, %d calls)\n", sizes, calls);
    return 0;
}
