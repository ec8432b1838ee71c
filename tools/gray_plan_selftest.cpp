// gray_plan_selftest -- csrc/idc_batch.h for greyscale batches (idc_forward_async_gray) without a device: the byte layout of both sample
// widths and both output depths (plan_batch), every refusal the format adds with its text, the copy runs and the image table
// (fill_batch_meta).  Host code only, no library, no HIP runtime call.
//
// Every expectation is a literal written here (sizes: int 4, HintRect 28, ImgDesc 24 bytes), never a value the code under test produced.
// tests/test_gray_cpu.py runs this; `make gray_plan_selftest SAN=1` builds it under ASan + UBSan.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "idc_batch.h"

using namespace idc;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

static_assert(sizeof(HintRect) == 28 && sizeof(ImgDesc) == 24 && sizeof(idc_gray_image) == 16, "the literals below assume these sizes");

static const int H = 8, W = 12, NB = 8;      // net size (not square) and max_batch
alignas(8) static uint8_t g_px[16], g_out[16];       // any non-null, even addresses: the plan never reads them

struct Gray {
    std::vector<idc_gray_image> images;
    std::vector<uint8_t*> outs;
    BatchCall call;
};
// plane i of hs[i] x ws[i]; the pointers into r stay valid as long as r does
static void make_gray(Gray& r, int bits, unsigned flags, const std::vector<int>& hs, const std::vector<int>& ws) {
    r.images.clear(); r.outs.clear();
    for (size_t i = 0; i < hs.size(); ++i) { r.images.push_back({g_px, hs[i], ws[i]}); r.outs.push_back(g_out); }
    r.call = BatchCall();
    r.call.n = (int)hs.size(); r.call.ragged = true; r.call.grays = r.images.data(); r.call.outs = r.outs.data();
    r.call.gray_bits = bits; r.call.flags = flags; r.call.out_bits = (flags & IDC_BATCH_OUT_RGB16) ? 16 : 8;
}

static void refused(const BatchCall& c, const char* text) {
    BatchPlan p;
    std::string err;
    const int rc = plan_batch(c, H, W, NB, &p, &err);
    if (rc != IDC_ERR_INVALID_ARG || err != text) {
        fprintf(stderr, "expected -1 \"%s\", got %d \"%s\"\n", text, rc, err.c_str());
        exit(1);
    }
}

static void accepted(const BatchCall& c, BatchPlan* p) {
    std::string err;
    const int rc = plan_batch(c, H, W, NB, p, &err);
    if (rc != IDC_OK) {
        fprintf(stderr, "expected 0, got %d \"%s\"\n", rc, err.c_str());
        exit(1);
    }
}

static void expect_piece(const Piece& q, size_t in_at, size_t in_bytes, size_t out_at, size_t out_bytes) {
    if (q.in_at != in_at || q.in_bytes != in_bytes || q.out_at != out_at || q.out_bytes != out_bytes) {
        fprintf(stderr, "piece in [%zu,+%zu) out [%zu,+%zu), expected in [%zu,+%zu) out [%zu,+%zu)\n", q.in_at, q.in_bytes, q.out_at, q.out_bytes, in_at,
                in_bytes, out_at, out_bytes);
        exit(1);
    }
}

// ---------------------------------------------------------------------------------------------------------------- layouts
// three planes of 1 x 1, 3 x 5 and 2 x 7 pixels: 1 + 15 + 14 = 30 pixels, image starts at pixels 0, 1, 16
static void check_layouts() {
    const std::vector<int> hs = {1, 3, 2}, ws = {1, 5, 7};
    Gray g;
    BatchPlan p;
    // uint8 in, net-size out: 1 byte a pixel in, H * W * 3 = 288 bytes an image out
    make_gray(g, 8, 0, hs, ws);
    accepted(g.call, &p);
    CHECK(p.bpp_in == 1 && p.bpp_out == 3 && p.in_bytes == 30 && p.rgb_bytes == 864 && !p.source_out && p.want_rgb && p.pieces.size() == 3);
    expect_piece(p.pieces[0], 0, 1, 0, 288); expect_piece(p.pieces[1], 1, 15, 288, 288); expect_piece(p.pieces[2], 16, 14, 576, 288);
    CHECK(p.max_pixels == 15 && p.max_tiles == 1);
    // uint8 in, source-size out: 3 bytes a pixel out
    make_gray(g, 8, IDC_BATCH_OUT_SOURCE, hs, ws);
    accepted(g.call, &p);
    CHECK(p.bpp_in == 1 && p.bpp_out == 3 && p.in_bytes == 30 && p.rgb_bytes == 90 && p.source_out);
    expect_piece(p.pieces[0], 0, 1, 0, 3); expect_piece(p.pieces[1], 1, 15, 3, 45); expect_piece(p.pieces[2], 16, 14, 48, 42);
    // uint16 in, 8-bit source-size out: 2 bytes in, 3 out
    make_gray(g, 16, IDC_BATCH_OUT_SOURCE, hs, ws);
    accepted(g.call, &p);
    CHECK(p.bpp_in == 2 && p.bpp_out == 3 && p.in_bytes == 60 && p.rgb_bytes == 90);
    expect_piece(p.pieces[0], 0, 2, 0, 3); expect_piece(p.pieces[1], 2, 30, 3, 45); expect_piece(p.pieces[2], 32, 28, 48, 42);
    // uint16 in, 16-bit source-size out: 2 bytes in, 6 out
    make_gray(g, 16, IDC_BATCH_OUT_SOURCE | IDC_BATCH_OUT_RGB16, hs, ws);
    accepted(g.call, &p);
    CHECK(p.bpp_in == 2 && p.bpp_out == 6 && p.in_bytes == 60 && p.rgb_bytes == 180);
    expect_piece(p.pieces[0], 0, 2, 0, 6); expect_piece(p.pieces[1], 2, 30, 6, 90); expect_piece(p.pieces[2], 32, 28, 96, 84);
    // uint16 in, net-size out: the net-size result is 8-bit
    make_gray(g, 16, 0, hs, ws);
    accepted(g.call, &p);
    CHECK(p.bpp_in == 2 && p.bpp_out == 3 && p.in_bytes == 60 && p.rgb_bytes == 864);
    expect_piece(p.pieces[2], 32, 28, 576, 288);
    // n = 1 and n = max_batch, both widths and both depths
    for (int bits = 8; bits <= 16; bits += 8)
        for (int deep = 0; deep <= (bits == 16 ? 1 : 0); ++deep) {
            const size_t bi = bits / 8, bo = deep ? 6 : 3;
            make_gray(g, bits, IDC_BATCH_OUT_SOURCE | (deep ? IDC_BATCH_OUT_RGB16 : 0), {3}, {5});
            accepted(g.call, &p);
            CHECK(p.pieces.size() == 1 && p.in_bytes == 15 * bi && p.rgb_bytes == 15 * bo);
            expect_piece(p.pieces[0], 0, 15 * bi, 0, 15 * bo);
            make_gray(g, bits, IDC_BATCH_OUT_SOURCE | (deep ? IDC_BATCH_OUT_RGB16 : 0), std::vector<int>(NB, 3), std::vector<int>(NB, 5));
            accepted(g.call, &p);
            CHECK(p.pieces.size() == 8 && p.in_bytes == 120 * bi && p.rgb_bytes == 120 * bo);
            expect_piece(p.pieces[7], 105 * bi, 15 * bi, 105 * bo, 15 * bo);
        }
    // a distribution batch may keep its images on the device
    make_gray(g, 16, 0, hs, ws);
    g.call.outs = nullptr; g.call.eval = true; g.call.taps_call = true;
    accepted(g.call, &p);
    CHECK(!p.want_rgb && p.dist && !p.reveal && !p.score && p.pieces[1].out == nullptr);
}

// ---------------------------------------------------------------------------------------------------------------- refusals
static void check_refusals() {
    const std::vector<int> hs = {1, 3, 2}, ws = {1, 5, 7};
    Gray g;
    for (int bits : {-1, 1, 12, 24, 32}) {
        make_gray(g, bits, 0, hs, ws);
        char text[64];
        snprintf(text, sizeof(text), "bits %d is neither 8 nor 16", bits);
        refused(g.call, text);
    }
    make_gray(g, 8, 0, hs, ws);
    g.call.grays = nullptr;
    refused(g.call, "null image pointer");
    make_gray(g, 8, 0, hs, ws);
    g.call.outs = nullptr;
    refused(g.call, "null image pointer");
    make_gray(g, 16, 4, hs, ws);
    refused(g.call, "unknown flag bits 0x4");
    make_gray(g, 8, 0, hs, ws);
    g.call.mode = IDC_HINT_REVEAL;
    refused(g.call, "IDC_HINT_REVEAL: a greyscale source has no colour to reveal");
    g.call.eval = true; g.call.taps_call = true;              // ... with taps too
    refused(g.call, "IDC_HINT_REVEAL: a greyscale source has no colour to reveal");
    make_gray(g, 8, IDC_BATCH_OUT_SOURCE | IDC_BATCH_OUT_RGB16, hs, ws);
    refused(g.call, "IDC_BATCH_OUT_RGB16 needs 16-bit samples, not 8-bit ones");
    make_gray(g, 16, IDC_BATCH_OUT_RGB16, hs, ws);
    refused(g.call, "IDC_BATCH_OUT_RGB16 without IDC_BATCH_OUT_SOURCE: the net-size result is 8-bit");
    make_gray(g, 16, 0, hs, ws);
    g.images[1].pix = g_px + 1;
    refused(g.call, "image 1: 16-bit samples at an odd address");
    make_gray(g, 8, 0, hs, ws);                               // (uint8 samples lie anywhere)
    g.images[1].pix = g_px + 1;
    BatchPlan p;
    accepted(g.call, &p);
    make_gray(g, 16, IDC_BATCH_OUT_SOURCE | IDC_BATCH_OUT_RGB16, hs, ws);
    g.outs[2] = g_out + 1;
    refused(g.call, "image 2: 16-bit result at an odd address");
    make_gray(g, 16, IDC_BATCH_OUT_SOURCE, hs, ws);           // (a uint8 result lies anywhere)
    g.outs[2] = g_out + 1;
    accepted(g.call, &p);
    make_gray(g, 16, 0, hs, ws);
    g.images[2].pix = nullptr;
    refused(g.call, "image 2: null image pointer");
    make_gray(g, 16, 0, {1, 0}, {1, 5});
    refused(g.call, "image 1: source size 0x5 outside 1..16384");
    // IDC_BATCH_MAX_SOURCE_BYTES = 2^30 bounds the sources and the results: four planes of 16384^2 uint8 are exactly 2^30 bytes in ...
    make_gray(g, 8, 0, std::vector<int>(4, 16384), std::vector<int>(4, 16384));
    accepted(g.call, &p);
    CHECK(p.in_bytes == ((size_t)1 << 30));
    make_gray(g, 8, 0, std::vector<int>(5, 16384), std::vector<int>(5, 16384));
    refused(g.call, "5 sources hold 1342177280 bytes, more than 1073741824");
    // ... and a source-size result is 3 or 6 bytes a pixel: 8192 x 16384 uint16 pixels are 2^28 bytes in and 6 * 2^27 = 805306368 out,
    // two of them 2^29 in and 1610612736 out
    make_gray(g, 16, IDC_BATCH_OUT_SOURCE | IDC_BATCH_OUT_RGB16, {8192}, {16384});
    accepted(g.call, &p);
    CHECK(p.in_bytes == ((size_t)1 << 28) && p.rgb_bytes == 805306368u);
    make_gray(g, 16, IDC_BATCH_OUT_SOURCE | IDC_BATCH_OUT_RGB16, {8192, 8192}, {16384, 16384});
    refused(g.call, "2 source-size results hold 1610612736 bytes, more than 1073741824");
    make_gray(g, 16, 0, {8192, 8192}, {16384, 16384});        // (the net-size results of the same planes are small)
    accepted(g.call, &p);
    // the RGB calls keep refusing the new flag
    std::vector<idc_ref_image> rgb = {{g_px, 2, 2}};
    std::vector<uint8_t*> outs = {g_out};
    BatchCall c;
    c.n = 1; c.ragged = true; c.images = rgb.data(); c.outs = outs.data(); c.flags = IDC_BATCH_OUT_RGB16;
    refused(c, "unknown flag bits 0x2");
}

// ---------------------------------------------------------------------------------------------------------------- copy runs
static void check_copy_runs() {
    Gray g;
    BatchPlan p;
    make_gray(g, 16, IDC_BATCH_OUT_SOURCE | IDC_BATCH_OUT_RGB16, {1, 3, 2, 1}, {1, 5, 7, 2});        // 1, 15, 14, 2 pixels
    accepted(g.call, &p);
    // everything pageable: one staged copy each way, 64 bytes in and 192 out
    std::vector<CopyOp> ops = copy_runs(p.pieces, true);
    CHECK(ops.size() == 1 && ops[0].piece == -1 && ops[0].at == 0 && ops[0].bytes == 64);
    ops = copy_runs(p.pieces, false);
    CHECK(ops.size() == 1 && ops[0].piece == -1 && ops[0].at == 0 && ops[0].bytes == 192);
    // plane 1 pinned on the way in, result 2 pinned on the way out: the staged neighbours on either side still merge
    p.pieces[1].in_pinned = true; p.pieces[2].out_pinned = true;
    ops = copy_runs(p.pieces, true);
    CHECK(ops.size() == 3 && ops[0].piece == -1 && ops[0].at == 0 && ops[0].bytes == 2 && ops[1].piece == 1 && ops[1].at == 2 && ops[1].bytes == 30 &&
          ops[2].piece == -1 && ops[2].at == 32 && ops[2].bytes == 32);
    ops = copy_runs(p.pieces, false);
    CHECK(ops.size() == 3 && ops[0].piece == -1 && ops[0].at == 0 && ops[0].bytes == 96 && ops[1].piece == 2 && ops[1].at == 96 && ops[1].bytes == 84 &&
          ops[2].piece == -1 && ops[2].at == 180 && ops[2].bytes == 12);
}

// ---------------------------------------------------------------------------------------------------------------- the table
static void check_table() {
    for (int bits = 8; bits <= 16; bits += 8) {
        Gray g;
        BatchPlan p;
        make_gray(g, bits, IDC_BATCH_OUT_SOURCE, {1, 3, 2}, {1, 5, 7});
        accepted(g.call, &p);
        // offsets int[9] -> 36 -> 48; table ImgDesc[9] = 216 -> 224; no hints: 272 bytes
        CHECK(p.table_at == 48 && p.hints_at == 272 && p.meta_bytes == 272);
        std::vector<unsigned char> meta(p.meta_bytes, 0xAB);          // exactly sized: SAN=1 reports a write past it
        fill_batch_meta(g.call, p, H, W, meta.data());
        const ImgDesc* tab = (const ImgDesc*)(meta.data() + 48);
        const long long bi = bits / 8;
        // `first` stays "pixels in front of this image" whatever a pixel weighs; `off` is its byte offset
        CHECK(tab[0].first == 0 && tab[0].off == 0 && tab[0].h == 1 && tab[0].w == 1);
        CHECK(tab[1].first == 1 && tab[1].off == 1 * bi && tab[1].h == 3 && tab[1].w == 5);
        CHECK(tab[2].first == 16 && tab[2].off == 16 * bi && tab[2].h == 2 && tab[2].w == 7);
        CHECK(tab[3].first == 30 && tab[3].off == 30 * bi && tab[3].h == 0 && tab[3].w == 0);
        const int* offs = (const int*)meta.data();
        CHECK(offs[0] == 0 && offs[1] == 0 && offs[2] == 0 && offs[3] == 0);
    }
    // with hints: the second plane has two, one of which is outside the net
    Gray g;
    BatchPlan p;
    make_gray(g, 16, 0, {4, 4}, {4, 4});
    const int32_t offsets[3] = {0, 0, 2};
    const idc_hint hints[2] = {{1, 1, 2, 2, 5.f, 6.f, 0.f}, {20, 20, 30, 30, 1.f, 1.f, 0.f}};
    g.call.hint_offsets = offsets; g.call.hints = hints;
    accepted(g.call, &p);
    CHECK(p.n_hints == 2 && p.kept == 1 && p.meta_bytes == 272 + 28);
    std::vector<unsigned char> meta(p.meta_bytes, 0xAB);
    fill_batch_meta(g.call, p, H, W, meta.data());
    const int* offs = (const int*)meta.data();
    const HintRect* hr = (const HintRect*)(meta.data() + 272);
    CHECK(offs[0] == 0 && offs[1] == 0 && offs[2] == 1 && hr[0].y0 == 1 && hr[0].x1 == 2 && hr[0].c0 == 5.f);
}

int main() {
    check_layouts();
    check_refusals();
    check_copy_runs();
    check_table();
    printf("gray_plan_selftest: ok\n");
    return 0;
}
