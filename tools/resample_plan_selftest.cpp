// resample_plan_selftest -- csrc/idc_batch.h with the ingest filter, without a device.  Host code only, no library, no HIP runtime call
// (tests/test_resample_cpu.py runs this; `make resample_plan_selftest SAN=1` builds it under ASan + UBSan, where the exactly-sized metadata
// block turns a write past meta_bytes into a report).
//   off   for each call of the list below with IDC_FILTER_BILINEAR, one line: the plan's fields and FNV-1a hashes of its pieces and of the
//         metadata block fill_batch_meta writes.  tests/golden/resample_plan_off.txt holds the lines the tree printed BEFORE the filter
//         existed (this file built with -DRESAMPLE_PLAN_BASELINE against that tree's headers): the test compares them byte for byte.
//   on    with IDC_FILTER_ANTIALIAS: everything in front of the appended blocks is the filter-off plan and block, byte for byte; the ingestion
//         view holds one (H, W) entry per down-scaled image, pointing at its net-size image behind the packed sources, and the original entry
//         otherwise, closing entry included; the jobs name the down-scaled images in order, with idc_resample.h's tiling; a call without a
//         down-scaled image is the filter-off plan altogether.
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

static const int H = 8, W = 12, NB = 8;      // net size (not square: an H / W mix-up shows) and max_batch
alignas(4) static uint8_t g_px[16], g_out[16];          // any non-null, even image address: the plan never reads the bytes
static uint64_t g_sse[3 * 8];
static float g_cols[64];

struct Call {
    const char* name;
    std::vector<idc_ref_image> images;
    std::vector<idc_gray_image> grays;
    std::vector<uint8_t*> outs;
    std::vector<int32_t> offs;
    std::vector<idc_hint> hints;
    BatchCall c;
};

static const int kSizes[][2] = {{5, 7}, {8, 12}, {9, 12}, {8, 13}, {1, 1}, {30, 5}, {3, 40}, {64, 48}};   // four of the eight are larger than the net on an axis

static void add_hints(Call& k, int n) {
    k.offs.assign(1, 0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j <= i % 3; ++j) k.hints.push_back({j, i, j + 3, i + 20 * (j == 2), 10.f + i, 20.f + j, 30.f});     // (some hang over, one is outside)
        if (i == 1) k.hints.push_back({50, 50, 60, 60, 1.f, 2.f, 3.f});
        k.offs.push_back((int32_t)k.hints.size());
    }
    k.c.hint_offsets = k.offs.data(); k.c.hints = k.hints.data();
}

static Call* same_size(const char* name, int n, int sh, int sw, unsigned flags, bool hints) {
    Call* k = new Call();
    k->name = name;
    k->c.n = n; k->c.src_h = sh; k->c.src_w = sw; k->c.rgb_in = g_px; k->c.rgb_out = g_out; k->c.flags = flags; k->c.mode = IDC_HINT_RGB;
    if (hints) add_hints(*k, n);
    return k;
}

static Call* ragged(const char* name, int first, int n, int gray_bits, unsigned flags, int mode, bool eval) {
    Call* k = new Call();
    k->name = name;
    for (int i = 0; i < n; ++i) {
        const int* s = kSizes[(first + i) % 8];
        k->images.push_back({g_px, s[0], s[1]});
        k->grays.push_back({g_px, s[0], s[1]});
        k->outs.push_back(g_out);
    }
    k->c.n = n; k->c.ragged = true; k->c.flags = flags; k->c.mode = mode;
    k->c.images = gray_bits ? nullptr : k->images.data(); k->c.grays = gray_bits ? k->grays.data() : nullptr; k->c.outs = k->outs.data();
    k->c.gray_bits = gray_bits; k->c.out_bits = (flags & IDC_BATCH_OUT_RGB16) ? 16 : 8;
    if (eval) { k->c.eval = true; k->c.sse = g_sse; k->c.hint_colours = mode == IDC_HINT_REVEAL ? g_cols : nullptr; }
    add_hints(*k, n);
    return k;
}

static unsigned long long fnv(unsigned long long h, const void* p, size_t n) {
    const unsigned char* b = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

struct Filled { BatchPlan p; std::vector<unsigned char> meta; };

static Filled run(BatchCall c, int filter) {
#ifndef RESAMPLE_PLAN_BASELINE
    c.ingest_filter = filter;
#else
    (void)filter;
#endif
    Filled f;
    std::string why;
    CHECK(plan_batch(c, H, W, NB, &f.p, &why) == IDC_OK);
    f.meta.assign(f.p.meta_bytes, 0);         // exactly sized: a write past the end is the sanitizer's to find
    fill_batch_meta(c, f.p, H, W, f.meta.data());
    return f;
}

static void print_off(const Call& k, const Filled& f) {
    const BatchPlan& p = f.p;
    unsigned long long hp = 14695981039346656037ull;
    for (const Piece& q : p.pieces) {
        const size_t v[4] = {q.in_at, q.in_bytes, q.out_at, q.out_bytes};
        hp = fnv(hp, v, sizeof(v));
    }
    printf("%s: want_rgb %d reveal %d dist %d score %d source_out %d n_hints %d kept %d in %zu rgb %zu table %zu hints %zu orig %zu meta %zu floor %zu "
           "cols %zu+%zu tiles %lld pixels %lld bpp %d/%d pieces %zu:%016llx block %016llx\n",
           k.name, (int)p.want_rgb, (int)p.reveal, (int)p.dist, (int)p.score, (int)p.source_out, p.n_hints, p.kept, p.in_bytes, p.rgb_bytes, p.table_at,
           p.hints_at, p.orig_at, p.meta_bytes, p.meta_floor, p.cols_at, p.cols_bytes, p.max_tiles, p.max_pixels, p.bpp_in, p.bpp_out, p.pieces.size(), hp,
           fnv(14695981039346656037ull, f.meta.data(), f.meta.size()));
}

#ifndef RESAMPLE_PLAN_BASELINE
static void check_on(const Call& k, const Filled& off, const Filled& on) {
    const BatchCall& c = k.c;
    const BatchPlan &p = on.p, &q = off.p;
    const int bpp = c.gray_bits ? c.gray_bits / 8 : 3, ch = c.gray_bits ? 1 : 3;
    const size_t net = (size_t)H * W * bpp;
    // which images are down-scaled: restated here
    std::vector<int> down;
    for (int i = 0; i < c.n; ++i) {
        const int h = c.ragged ? (c.gray_bits ? c.grays[i].h : c.images[i].h) : c.src_h, w = c.ragged ? (c.gray_bits ? c.grays[i].w : c.images[i].w) : c.src_w;
        if (h > H || w > W) down.push_back(i);
    }
    CHECK(p.naa == (int)down.size());
    // today's fields are untouched
    CHECK(p.want_rgb == q.want_rgb && p.reveal == q.reveal && p.source_out == q.source_out && p.n_hints == q.n_hints && p.kept == q.kept);
    CHECK(p.in_bytes == q.in_bytes && p.rgb_bytes == q.rgb_bytes && p.table_at == q.table_at && p.hints_at == q.hints_at && p.orig_at == q.orig_at);
    CHECK(p.meta_floor == q.meta_floor && p.cols_at == q.cols_at && p.cols_bytes == q.cols_bytes && p.max_tiles == q.max_tiles && p.max_pixels == q.max_pixels);
    CHECK(p.bpp_in == q.bpp_in && p.bpp_out == q.bpp_out && p.pieces.size() == q.pieces.size() && q.src_bytes == q.in_bytes && q.naa == 0);
    for (size_t i = 0; i < p.pieces.size(); ++i)
        CHECK(p.pieces[i].in_at == q.pieces[i].in_at && p.pieces[i].in_bytes == q.pieces[i].in_bytes && p.pieces[i].out_at == q.pieces[i].out_at &&
              p.pieces[i].out_bytes == q.pieces[i].out_bytes);
    CHECK(on.meta.size() >= off.meta.size() && memcmp(on.meta.data(), off.meta.data(), off.meta.size()) == 0);
    if (down.empty()) {                             // nothing to filter: the filter-off plan altogether
        CHECK(p.meta_bytes == q.meta_bytes && p.src_bytes == q.in_bytes && p.aa_at == 0 && p.view_at == 0 && p.jobs_at == 0 && p.aa_tiles == 0);
        return;
    }
    CHECK(p.aa_at >= p.in_bytes && p.aa_at % 48 == 0 && p.aa_at - p.in_bytes < 48 && p.src_bytes == p.aa_at + down.size() * net);
    CHECK(p.view_at >= q.meta_bytes && p.view_at % 16 == 0 && p.view_at - q.meta_bytes < 16);
    CHECK(p.jobs_at == (c.ragged ? p.view_at + ((size_t)(NB + 1) * sizeof(ImgDesc) + 15) / 16 * 16 : p.view_at) && p.jobs_at % 16 == 0);
    CHECK(p.meta_bytes == p.jobs_at + down.size() * sizeof(ResampleJob));
    const ResampleJob* jobs = (const ResampleJob*)(on.meta.data() + p.jobs_at);
    const ImgDesc* tab = (const ImgDesc*)(on.meta.data() + p.table_at);
    const ImgDesc* view = (const ImgDesc*)(on.meta.data() + p.view_at);
    int tiles = 0;
    for (size_t k2 = 0; k2 < down.size(); ++k2) {
        const int i = down[k2];
        const int h = c.ragged ? tab[i].h : c.src_h, w = c.ragged ? tab[i].w : c.src_w;
        const long long at = c.ragged ? tab[i].off : (long long)i * c.src_h * c.src_w * 3;
        CHECK(jobs[k2].src_off == at && jobs[k2].dst_off == (long long)(p.aa_at + k2 * net) && jobs[k2].h == h && jobs[k2].w == w);
        CHECK(jobs[k2].tw == resample_tile_width(w, W, ch) && jobs[k2].tiles == resample_tile_count(W, jobs[k2].tw) && jobs[k2].tiles >= 1);
        CHECK(jobs[k2].dst_off + (long long)net <= (long long)p.src_bytes && jobs[k2].src_off + (long long)h * w * bpp <= (long long)p.in_bytes);
        tiles = tiles > jobs[k2].tiles ? tiles : jobs[k2].tiles;
    }
    CHECK(p.aa_tiles == tiles);
    if (c.ragged) {
        size_t k2 = 0;
        for (int i = 0; i <= c.n; ++i) {
            const bool is_down = k2 < down.size() && down[k2] == i;
            if (!is_down) {
                CHECK(memcmp(&view[i], &tab[i], sizeof(ImgDesc)) == 0);
                continue;
            }
            CHECK(view[i].h == H && view[i].w == W && view[i].off == (long long)(p.aa_at + k2 * net) && view[i].first * bpp == view[i].off);
            ++k2;
        }
    }
}
#endif

int main() {
    const unsigned SRC = IDC_BATCH_OUT_SOURCE, R16 = IDC_BATCH_OUT_RGB16;
    std::vector<Call*> calls = {
        same_size("same 3 x 5x7", 3, 5, 7, 0, false),
        same_size("same 4 x 9x12 hints", 4, 9, 12, 0, true),
        same_size("same 2 x 40x50 source hints", 2, 40, 50, SRC, true),
        same_size("same 8 x 8x12", 8, 8, 12, SRC, false),
        ragged("ragged 8 net", 0, 8, 0, 0, IDC_HINT_AB, false),
        ragged("ragged 5 source rgb hints", 3, 5, 0, SRC, IDC_HINT_RGB, false),
        ragged("ragged 2 small", 0, 2, 0, SRC, IDC_HINT_AB, false),
        ragged("eval reveal 6", 2, 6, 0, 0, IDC_HINT_REVEAL, true),
        ragged("eval ab source 4", 5, 4, 0, SRC, IDC_HINT_AB, true),
        ragged("gray8 7 source", 1, 7, 8, SRC, IDC_HINT_AB, false),
        ragged("gray16 8 rgb16", 0, 8, 16, SRC | R16, IDC_HINT_AB, false),
        ragged("gray16 3 net", 5, 3, 16, 0, IDC_HINT_RGB, false),
    };
#ifndef RESAMPLE_PLAN_BASELINE
    int with_view = 0;
#endif
    for (Call* k : calls) {
        const Filled off = run(k->c, 0);
        print_off(*k, off);
#ifndef RESAMPLE_PLAN_BASELINE
        const Filled on = run(k->c, IDC_FILTER_ANTIALIAS);
        check_on(*k, off, on);
        with_view += on.p.naa > 0 && k->c.ragged;
        BatchCall bad = k->c;                       // a value that is no filter is the handle's to refuse: the plan treats it as off
        bad.ingest_filter = 7;
        BatchPlan pb;
        std::string why;
        CHECK(plan_batch(bad, H, W, NB, &pb, &why) == IDC_OK && pb.naa == 0 && pb.meta_bytes == off.p.meta_bytes);
#endif
        delete k;
    }
#ifndef RESAMPLE_PLAN_BASELINE
    CHECK(with_view >= 6);
#endif
    printf("resample_plan_selftest: ok (%zu calls)\n", calls.size());
    return 0;
}
