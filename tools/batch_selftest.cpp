// batch_selftest -- csrc/idc_batch.h without a device: the hint clipping rule, the argument checks and byte layout of a pipelined batch
// (plan_batch), the metadata block (fill_batch_meta) and the copy runs (copy_runs).  Host code only, no library, no HIP runtime call.
//
// Every expectation is a literal written here (sizes: int 4, HintRect 28, ImgDesc 24 bytes), never a value the code under test produced.
// tests/test_batch_plan_cpu.py runs this; `make batch_selftest SAN=1` builds it under ASan + UBSan, where the exactly-sized metadata block
// of check_meta turns a write past meta_bytes into a report.
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

static_assert(sizeof(HintRect) == 28 && sizeof(ImgDesc) == 24 && sizeof(idc_hint) == 28, "the literals below assume these sizes");

static const int H = 8, W = 12, NB = 8;      // net size (not square: an H / W mix-up shows) and max_batch
static uint8_t g_px[16], g_out[16];          // any non-null image bytes: the plan never reads them
static uint64_t g_sse[3 * 8];

static idc_hint hint(int y0, int x0, int y1, int x1, float c0 = 1.f, float c1 = 2.f, float c2 = 3.f) { return {y0, x0, y1, x1, c0, c1, c2}; }

static void expect_rect(const HintRect& r, int y0, int x0, int y1, int x1) {
    CHECK(r.y0 == y0 && r.x0 == x0 && r.y1 == y1 && r.x1 == x1);
}

static void check_clip() {
    HintRect r;
    CHECK(clip_hint(hint(2, 3, 5, 7, 4.f, 5.f, 6.f), H, W, r));
    expect_rect(r, 2, 3, 5, 7);
    CHECK(r.c0 == 4.f && r.c1 == 5.f && r.c2 == 6.f);
    CHECK(clip_hint(hint(5, 7, 2, 3), H, W, r));             // corners in the other order ...
    expect_rect(r, 2, 3, 5, 7);
    CHECK(clip_hint(hint(2, 7, 5, 3), H, W, r));             // ... and mixed
    expect_rect(r, 2, 3, 5, 7);
    // entirely outside, on each of the four sides: dropped, r filled all the same
    CHECK(!clip_hint(hint(-5, 2, -1, 4, 9.f), H, W, r));
    CHECK(r.c0 == 9.f && r.x0 == 2 && r.x1 == 4);
    CHECK(!clip_hint(hint(8, 2, 11, 4), H, W, r));
    CHECK(!clip_hint(hint(2, -9, 4, -1), H, W, r));
    CHECK(!clip_hint(hint(2, 12, 4, 20), H, W, r));
    // hanging over each edge: clipped to 0 / H-1 / W-1
    CHECK(clip_hint(hint(-3, 2, 1, 4), H, W, r));
    expect_rect(r, 0, 2, 1, 4);
    CHECK(clip_hint(hint(6, 2, 30, 4), H, W, r));
    expect_rect(r, 6, 2, 7, 4);
    CHECK(clip_hint(hint(2, -3, 4, 1), H, W, r));
    expect_rect(r, 2, 0, 4, 1);
    CHECK(clip_hint(hint(2, 10, 4, 30), H, W, r));
    expect_rect(r, 2, 10, 4, 11);
    CHECK(clip_hint(hint(-100, -100, 100, 100), H, W, r));
    expect_rect(r, 0, 0, 7, 11);
    CHECK(clip_hint(hint(7, 11, 7, 11), H, W, r));           // one pixel in the last corner
    expect_rect(r, 7, 11, 7, 11);
    CHECK(!clip_hint(hint(7, 12, 7, 12), H, W, r));          // ... and one past it, each way
    CHECK(!clip_hint(hint(8, 11, 8, 11), H, W, r));
}

// ---------------------------------------------------------------------------------------------------------------- refusals
static BatchCall same_size(int n, int sh = 5, int sw = 7) {
    BatchCall c;
    c.n = n; c.src_h = sh; c.src_w = sw; c.rgb_in = g_px; c.rgb_out = g_out;
    return c;
}

struct Ragged {
    std::vector<idc_ref_image> images;
    std::vector<uint8_t*> outs;
    BatchCall call;
};
// image i of size hs[i] x ws[i]; the pointers into r stay valid as long as r does
static void make_ragged(Ragged& r, const std::vector<int>& hs, const std::vector<int>& ws) {
    r.images.clear(); r.outs.clear();
    for (size_t i = 0; i < hs.size(); ++i) { r.images.push_back({g_px, hs[i], ws[i]}); r.outs.push_back(g_out); }
    r.call = BatchCall();
    r.call.n = (int)hs.size(); r.call.ragged = true; r.call.images = r.images.data(); r.call.outs = r.outs.data();
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

static void check_refusals() {
    BatchPlan p;
    BatchCall c = same_size(2);
    accepted(c, &p);
    c.slot = 2; refused(c, "slot 2 not in 0..1");
    c.slot = -1; refused(c, "slot -1 not in 0..1");
    c = same_size(2); c.rgb_in = nullptr; refused(c, "null image pointer");
    c = same_size(2); c.rgb_out = nullptr; refused(c, "null image pointer");
    c = same_size(2); c.flags = 2; refused(c, "unknown flag bits 0x2");
    c = same_size(2); c.mode = 3; refused(c, "hint mode 3");
    c = same_size(2); c.mode = IDC_HINT_REVEAL; refused(c, "hint mode 2");      // only an evaluation call reveals
    c = same_size(2); c.src_h = 0; refused(c, "source size 0x7 outside 1..16384");
    c = same_size(2); c.src_w = 16385; refused(c, "source size 5x16385 outside 1..16384");
    c = same_size(8, 16384, 16384); refused(c, "8 sources of 16384x16384 are more than 1073741824 bytes");

    Ragged r;
    make_ragged(r, {1, 2}, {3, 4});
    accepted(r.call, &p);
    r.call.images = nullptr; refused(r.call, "null image pointer");
    make_ragged(r, {1, 2}, {3, 4});
    r.call.outs = nullptr; refused(r.call, "null image pointer");
    r.call.eval = true; r.call.sse = g_sse; accepted(r.call, &p);               // ... an evaluation batch may keep its images on the device
    CHECK(!p.want_rgb);
    make_ragged(r, {1, 2}, {3, 4});
    r.images[1].rgb = nullptr; refused(r.call, "image 1: null image pointer");
    make_ragged(r, {1, 2}, {3, 4});
    r.outs[1] = nullptr; refused(r.call, "image 1: null image pointer");
    make_ragged(r, {1, 0}, {3, 4}); refused(r.call, "image 1: source size 0x4 outside 1..16384");
    make_ragged(r, {1, 2}, {16385, 4}); refused(r.call, "image 0: source size 1x16385 outside 1..16384");
    make_ragged(r, {16384, 16384}, {16384, 16384}); refused(r.call, "2 sources hold 1610612736 bytes, more than 1073741824");

    // the evaluation arguments
    make_ragged(r, {1, 2}, {3, 4});
    r.call.eval = true; refused(r.call, "null sse");
    r.call.taps_call = true; accepted(r.call, &p);                               // a distribution batch need not score
    CHECK(p.dist && !p.score);
    make_ragged(r, {1, 2}, {3, 4});
    float cols[4];
    r.call.eval = true; r.call.sse = g_sse; r.call.hint_colours = cols; r.call.mode = IDC_HINT_AB;
    refused(r.call, "hint_colours with hint mode 0: only IDC_HINT_REVEAL reveals colours");
    r.call.mode = IDC_HINT_REVEAL; accepted(r.call, &p);
    CHECK(p.reveal);

    // the hint list
    const idc_hint hs[3] = {hint(0, 0, 1, 1), hint(2, 2, 3, 3, 256.f), hint(-9, -9, -8, -8, 999.f)};
    int32_t offs[3] = {1, 1, 2};
    c = same_size(2); c.hints = hs; c.hint_offsets = offs; refused(c, "hint_offsets[0] is 1, not 0");
    offs[0] = 0; offs[1] = 2; offs[2] = 1; refused(c, "hint_offsets decrease at image 1");
    offs[1] = 0; offs[2] = (1 << 20) + 1; c.hints = nullptr; refused(c, "1048577 hints, more than 1048576");
    offs[2] = 1; refused(c, "null hints with a non-zero offset");
    offs[1] = 1; offs[2] = 3; c.hints = hs; c.mode = IDC_HINT_RGB; refused(c, "hint 1: RGB outside 0..255");
    c.mode = IDC_HINT_AB; accepted(c, &p);                                       // the range is RGB's alone ...
    CHECK(p.n_hints == 3 && p.kept == 2);
    offs[1] = 1; offs[2] = 1; c.mode = IDC_HINT_RGB; accepted(c, &p);
    const idc_hint dropped[2] = {hint(0, 0, 1, 1), hint(-9, -9, -8, -8, 999.f)};
    offs[2] = 2; c.hints = dropped; accepted(c, &p);                             // ... and a hint outside the image is dropped unread
    CHECK(p.kept == 1);
    const idc_hint nan_hint[1] = {hint(0, 0, 1, 1, 0.f, 0.f, __builtin_nanf(""))};
    offs[1] = 1; offs[2] = 1; c.hints = nan_hint; refused(c, "hint 0: RGB outside 0..255");
    c.hint_offsets = nullptr; c.hints = nullptr; accepted(c, &p);                // no list at all
    CHECK(p.n_hints == 0 && p.kept == 0);

    // two violations: the earlier check answers
    c = same_size(2); c.slot = 2; c.flags = 2; refused(c, "slot 2 not in 0..1");
    c = same_size(2); c.flags = 4; c.mode = 7; refused(c, "unknown flag bits 0x4");
    make_ragged(r, {1, 0}, {3, 4});
    r.call.eval = true; refused(r.call, "null sse");
    offs[0] = 5; c = same_size(2, 0, 7); c.hint_offsets = offs; refused(c, "source size 0x7 outside 1..16384");
}

// ---------------------------------------------------------------------------------------------------------------- layout
// image i of the ragged cases: (i + 1) x (2 i + 3), so 9, 30, 63, 108, 165, 234, 315, 408 bytes: 1332 in all
static const int kRagH[8] = {1, 2, 3, 4, 5, 6, 7, 8}, kRagW[8] = {3, 5, 7, 9, 11, 13, 15, 17};
static const size_t kRagAt[9] = {0, 9, 39, 102, 210, 375, 609, 924, 1332};

static void check_layout_case(int n, bool ragged, bool reveal, bool source) {
    // per image three hints: one inside, one entirely outside, one hanging over the corner -> two of three kept
    std::vector<idc_hint> hints;
    std::vector<int32_t> offs(1, 0);
    for (int i = 0; i < n; ++i) {
        hints.push_back(hint(1, 1, 2, 2));
        hints.push_back(hint(8, 0, 9, 3));
        hints.push_back(hint(6, 10, 20, 20));
        offs.push_back(3 * (i + 1));
    }
    Ragged r;
    BatchCall c;
    if (ragged) {
        make_ragged(r, std::vector<int>(kRagH, kRagH + n), std::vector<int>(kRagW, kRagW + n));
        c = r.call;
    } else {
        c = same_size(n);
    }
    c.hints = hints.data(); c.hint_offsets = offs.data();
    c.flags = source ? IDC_BATCH_OUT_SOURCE : 0;
    float cols[2 * 24];
    if (reveal) { c.eval = true; c.sse = g_sse; c.mode = IDC_HINT_REVEAL; c.hint_colours = cols; }
    BatchPlan p;
    accepted(c, &p);
    const size_t kept = 2 * (size_t)n;
    CHECK(p.n_hints == 3 * n && (size_t)p.kept == kept);
    CHECK(p.reveal == reveal && p.source_out == source && p.want_rgb);
    const size_t in_bytes = ragged ? (n == 1 ? 9 : 1332) : (n == 1 ? 105 : 840);           // 5 x 7 x 3 = 105 a same-size image
    const size_t net_bytes = n == 1 ? 288 : 2304;                                         // 8 x 12 x 3 = 288 a net-size image
    CHECK(p.in_bytes == in_bytes);
    CHECK(p.rgb_bytes == (source ? in_bytes : net_bytes));
    // offsets int[9] = 36 bytes -> the table at 48; ImgDesc[9] = 216 -> the hints at 48 + 224
    CHECK(p.table_at == 48 && p.table_at % 16 == 0 && p.hints_at % 16 == 0);
    CHECK(p.hints_at == (ragged ? 272u : 48u));
    CHECK(p.orig_at == p.hints_at + 28 * kept);
    CHECK(p.meta_bytes == p.orig_at + (reveal ? 4 * kept : 0));
    CHECK(p.meta_floor == p.hints_at + 8192);
    // [0, 36) offsets | [table_at, +216) table | [hints_at, +28 kept) hints | [orig_at, +4 kept) places: in this order, none overlapping
    CHECK(36 <= p.table_at && p.table_at + (ragged ? 216 : 0) <= p.hints_at && p.hints_at + 28 * kept <= p.orig_at && p.orig_at <= p.meta_bytes);
    CHECK(p.cols_at == 192 && p.cols_bytes == (reveal ? 8 * 3 * (size_t)n : 0));
    CHECK(p.max_tiles == 1);
    CHECK(p.max_pixels == (ragged ? (n == 1 ? 3 : 136) : 35));
    CHECK(p.pieces.size() == (ragged ? (size_t)n : 1));
    for (size_t i = 0; i < p.pieces.size(); ++i) {
        const Piece& q = p.pieces[i];
        const size_t at = ragged ? kRagAt[i] : 0, bytes = ragged ? kRagAt[i + 1] - kRagAt[i] : in_bytes;
        CHECK(q.in == g_px && q.out == g_out && q.in_at == at && q.in_bytes == bytes);
        CHECK(q.out_at == (source ? at : 288 * i) && q.out_bytes == (source ? bytes : (ragged ? 288 : net_bytes)));
    }
}

static void check_layout() {
    for (int n : {1, 8})
        for (int ragged = 0; ragged < 2; ++ragged)
            for (int reveal = 0; reveal < 2; ++reveal)
                for (int source = 0; source < 2; ++source) check_layout_case(n, ragged != 0, reveal != 0, source != 0);
    Ragged r;                                // 9 x 33: 2 x 2 tiles of 8 x 32, 297 pixels; 17 x 5: 3 x 1 tiles, 85 pixels
    make_ragged(r, {9, 17}, {33, 5});
    BatchPlan p;
    accepted(r.call, &p);
    CHECK(p.max_tiles == 4 && p.max_pixels == 297);
    BatchCall c = same_size(3, 17, 33);      // 3 x 2 tiles, 561 pixels
    accepted(c, &p);
    CHECK(p.max_tiles == 6 && p.max_pixels == 561);
}

// ---------------------------------------------------------------------------------------------------------------- metadata block
static void check_meta() {
    // image 0: in, out, in; image 1: out, out; image 2: in, then three outside -- the list ENDS in hints that are dropped
    const idc_hint hs[9] = {hint(1, 1, 2, 2, 10.f), hint(8, 0, 9, 3, 11.f), hint(6, 10, 20, 20, 12.f), hint(-4, 0, -1, 3, 13.f), hint(0, 12, 3, 15, 14.f),
                            hint(3, 4, 3, 4, 15.f), hint(0, -9, 7, -1, 16.f), hint(50, 50, 60, 60, 17.f), hint(8, 12, 8, 12, 18.f)};
    const int32_t offs[4] = {0, 3, 5, 9};
    BatchCall c = same_size(3);
    c.hints = hs; c.hint_offsets = offs;
    c.eval = true; c.sse = g_sse; c.mode = IDC_HINT_REVEAL;
    BatchPlan p;
    accepted(c, &p);
    CHECK(p.kept == 3 && p.hints_at == 48 && p.orig_at == 48 + 84 && p.meta_bytes == 48 + 84 + 12);
    unsigned char* exact = (unsigned char*)malloc(p.meta_bytes);           // not a byte more: a sanitizer build reports any write behind it
    fill_batch_meta(c, p, H, W, exact);
    std::vector<unsigned char> buf(p.meta_bytes + 64, 0xA5);
    fill_batch_meta(c, p, H, W, buf.data());
    for (size_t i = p.meta_bytes; i < buf.size(); ++i) CHECK(buf[i] == 0xA5);
    CHECK(memcmp(exact, buf.data(), 16) == 0);
    free(exact);
    const int* m_offs = (const int*)buf.data();
    CHECK(m_offs[0] == 0 && m_offs[1] == 2 && m_offs[2] == 2 && m_offs[3] == 3);      // per image, over the kept hints only
    const HintRect* m = (const HintRect*)(buf.data() + 48);
    expect_rect(m[0], 1, 1, 2, 2);
    expect_rect(m[1], 6, 10, 7, 11);
    expect_rect(m[2], 3, 4, 3, 4);
    CHECK(m[0].c0 == 10.f && m[1].c0 == 12.f && m[2].c0 == 15.f);
    const int* orig = (const int*)(buf.data() + 132);
    CHECK(orig[0] == 0 && orig[1] == 2 && orig[2] == 5);                              // back to the caller's indices
    // without reveal the block ends behind the hints
    c.mode = IDC_HINT_AB;
    accepted(c, &p);
    CHECK(p.meta_bytes == 132);
    std::vector<unsigned char> plain(p.meta_bytes + 64, 0xA5);
    fill_batch_meta(c, p, H, W, plain.data());
    for (size_t i = p.meta_bytes; i < plain.size(); ++i) CHECK(plain[i] == 0xA5);
    CHECK(memcmp(plain.data() + 48, buf.data() + 48, 84) == 0);
    // no list: offsets all zero, nothing else written
    c.hints = nullptr; c.hint_offsets = nullptr;
    accepted(c, &p);
    CHECK(p.meta_bytes == 48);
    std::vector<unsigned char> none(p.meta_bytes + 64, 0xA5);
    fill_batch_meta(c, p, H, W, none.data());
    m_offs = (const int*)none.data();
    CHECK(m_offs[0] == 0 && m_offs[1] == 0 && m_offs[2] == 0 && m_offs[3] == 0);
    for (size_t i = 16; i < none.size(); ++i) CHECK(none[i] == 0xA5);
}

static void check_ragged_table() {
    Ragged r;                                // 3, 6, 9, 12 bytes: every residue mod 4
    make_ragged(r, {1, 1, 1, 2}, {1, 2, 3, 2});
    const idc_hint hs[1] = {hint(0, 0, 0, 0)};
    const int32_t offs[5] = {0, 0, 0, 1, 1};
    r.call.hints = hs; r.call.hint_offsets = offs;
    BatchPlan p;
    accepted(r.call, &p);
    CHECK(p.in_bytes == 30 && p.hints_at == 272 && p.meta_bytes == 300);
    std::vector<unsigned char> buf(p.meta_bytes + 64, 0xA5);
    fill_batch_meta(r.call, p, H, W, buf.data());
    for (size_t i = p.meta_bytes; i < buf.size(); ++i) CHECK(buf[i] == 0xA5);
    const ImgDesc* t = (const ImgDesc*)(buf.data() + 48);
    const long long off[5] = {0, 3, 9, 18, 30}, first[5] = {0, 1, 3, 6, 10};
    const int hh[5] = {1, 1, 1, 2, 0}, ww[5] = {1, 2, 3, 2, 0};                       // entry 4 closes the run
    for (int i = 0; i < 5; ++i) CHECK(t[i].off == off[i] && t[i].first == first[i] && t[i].h == hh[i] && t[i].w == ww[i]);
    for (size_t i = 48 + 5 * 24; i < 272; ++i) CHECK(buf[i] == 0xA5);                 // the rest of the table's room is not touched
    const int* m_offs = (const int*)buf.data();
    CHECK(m_offs[0] == 0 && m_offs[1] == 0 && m_offs[2] == 0 && m_offs[3] == 1 && m_offs[4] == 1);
    expect_rect(*(const HintRect*)(buf.data() + 272), 0, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------------- copy runs
static std::vector<Piece> five(const char* in_pins, const char* out_pins, bool source) {
    const size_t at[6] = {0, 10, 30, 60, 100, 150};
    std::vector<Piece> v;
    for (int i = 0; i < 5; ++i)
        v.push_back({g_px, g_out, at[i], at[i + 1] - at[i], source ? at[i] : 288 * (size_t)i, source ? at[i + 1] - at[i] : 288, in_pins[i] == 'P',
                     out_pins[i] == 'P'});
    return v;
}

static void expect_ops(const std::vector<CopyOp>& got, const std::vector<CopyOp>& want) {
    CHECK(got.size() == want.size());
    for (size_t i = 0; i < got.size(); ++i) CHECK(got[i].piece == want[i].piece && got[i].at == want[i].at && got[i].bytes == want[i].bytes);
}

static void check_runs() {
    // to the device
    expect_ops(copy_runs(five("PPPPP", "SSSSS", true), true), {{0, 0, 10}, {1, 10, 20}, {2, 30, 30}, {3, 60, 40}, {4, 100, 50}});
    expect_ops(copy_runs(five("SSSSS", "PPPPP", true), true), {{-1, 0, 150}});
    expect_ops(copy_runs(five("PSSPS", "PPPPP", true), true), {{0, 0, 10}, {-1, 10, 50}, {3, 60, 40}, {-1, 100, 50}});
    expect_ops(copy_runs(five("SPSSP", "PPPPP", true), true), {{-1, 0, 10}, {1, 10, 20}, {-1, 30, 70}, {4, 100, 50}});
    // from the device, source-size offsets (the input's own) ...
    expect_ops(copy_runs(five("SSSSS", "PPPPP", true), false), {{0, 0, 10}, {1, 10, 20}, {2, 30, 30}, {3, 60, 40}, {4, 100, 50}});
    expect_ops(copy_runs(five("PPPPP", "SSSSS", true), false), {{-1, 0, 150}});
    expect_ops(copy_runs(five("PPPPP", "PSSPS", true), false), {{0, 0, 10}, {-1, 10, 50}, {3, 60, 40}, {-1, 100, 50}});
    // ... and net-size offsets, i x 288
    expect_ops(copy_runs(five("SSSSS", "PPPPP", false), false), {{0, 0, 288}, {1, 288, 288}, {2, 576, 288}, {3, 864, 288}, {4, 1152, 288}});
    expect_ops(copy_runs(five("PPPPP", "SSSSS", false), false), {{-1, 0, 1440}});
    expect_ops(copy_runs(five("PPPPP", "PSSPS", false), false), {{0, 0, 288}, {-1, 288, 576}, {3, 864, 288}, {-1, 1152, 288}});
    // a single piece, and none
    std::vector<Piece> one = {{g_px, g_out, 0, 105, 0, 288, true, false}};
    expect_ops(copy_runs(one, true), {{0, 0, 105}});
    expect_ops(copy_runs(one, false), {{-1, 0, 288}});
    expect_ops(copy_runs(std::vector<Piece>(), true), {});
}

int main() {
    check_clip();
    check_refusals();
    check_layout();
    check_meta();
    check_ragged_table();
    check_runs();
    printf("batch_selftest: ok\n");
    return 0;
}
