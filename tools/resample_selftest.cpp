// resample_selftest -- csrc/idc_resample.h without a device: the windows, spans, tile widths and chunks of the antialiased ingestion pre-pass
// (idc_resample.hip) for every source size the library accepts.  No HIP runtime call.  Checked (tests/test_resample_cpu.py runs this;
// `make resample_selftest SAN=1` builds it under ASan + UBSan), for every `in` in 1..16384, `out` in {1, 2, 3, 48, 64, 256} and a sample of
// other `out` up to 1024, one and three channels:
//   1. every window of a down-scaled axis lies inside [0, in), is not empty and holds at most ceil(2 s) + 1 taps; the two taps of an axis
//      that is not down-scaled lie inside [0, in) and ascend;
//   2. tw >= 1, tw <= kResampleMaxTW, tw * channels <= kResampleThreads (one lane per output sample of the horizontal pass);
//   3. the tiles cover 0 .. out-1 exactly once, in order;
//   4. a tile's span covers the taps of all its columns and lies inside [0, in);
//   5. a span fits one chunk of resample_chunk_cols unless tw == 1, and the staged elements of any chunk fit the LDS budget
//      (kResampleLdsBudget = 32 KiB), which resample_lds_bytes stays within;
//   6. resample_job carries the same tiling, and resample_applies is "larger on an axis".
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "idc_resample.h"

using namespace idc;

#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        if (!(cond)) {                                                                                           \
            fprintf(stderr, "%s:%d: CHECK failed: %s (in %d, out %d, channels %d)\n", __FILE__, __LINE__, #cond, \
                    g_in, g_out, g_ch);                                                                          \
            exit(1);                                                                                             \
        }                                                                                                        \
    } while (0)

static int g_in, g_out, g_ch;

static void check_axis(int in, int out, int ch, long long* windows, long long* chunked) {
    g_in = in; g_out = out; g_ch = ch;
    const int cols = resample_chunk_cols(ch);
    CHECK(cols >= 1 && cols * ch <= kResampleChunkElems);
    CHECK(resample_lds_bytes(ch) <= kResampleLdsBudget && kResampleLdsBudget == 32768);
    const int tw = resample_tile_width(in, out, ch);
    CHECK(tw >= 1 && tw <= kResampleMaxTW && tw <= (out > 1 ? out : 1) && tw * ch <= kResampleThreads);
    const int tiles = resample_tile_count(out, tw);
    CHECK(tiles >= 1 && (long long)(tiles - 1) * tw < out && (long long)tiles * tw >= out);
    const ResampleJob job = resample_job(7, 11, 5, in, out, ch);
    CHECK(job.tw == tw && job.tiles == tiles && job.src_off == 7 && job.dst_off == 11 && job.h == 5 && job.w == in);
    const double s = (double)in / (double)out;
    int next = 0;                                   // the first output index no tile has taken yet
    for (int t = 0; t < tiles; ++t) {
        const int i0 = t * tw, i1 = i0 + tw < out ? i0 + tw : out;
        CHECK(i0 == next && i1 > i0);
        next = i1;
        int c0, c1;
        resample_span(i0, i1, in, out, c0, c1);
        CHECK(c0 >= 0 && c1 <= in && c1 > c0);
        if (c1 - c0 > cols) {
            CHECK(tw == 1);
            ++*chunked;
        }
        const int chunks = (c1 - c0 + cols - 1) / cols;
        CHECK((long long)chunks * cols >= c1 - c0 && (chunks == 1 || tw == 1));
        for (int i = i0; i < i1; ++i) {
            if (in > out) {
                int lo, hi;
                resample_window(i, in, out, lo, hi);
                CHECK(lo >= 0 && hi <= in && hi > lo);
                CHECK(hi - lo <= (int)ceil(2.0 * s) + 1);
                CHECK(lo >= c0 && hi <= c1);
            } else {
                int t0, t1;
                double w;
                resample_taps2(i, in, out, t0, t1, w);
                CHECK(t0 >= 0 && t1 <= in - 1 && t0 <= t1 && t1 - t0 <= 1);
                CHECK(w >= 0.0 && w < 1.0);
                CHECK(t0 >= c0 && t1 < c1);
                if (in == out) CHECK(t0 == i && w == 0.0);          // the identity at the net size
            }
            ++*windows;
        }
    }
    CHECK(next == out);
}

// `resample_selftest in out channels [in out channels ...]`: checks 1..6 for each triple, then one line "tw tiles max_chunks" per triple -- the
// figures tests/resample_ref.py restates in Python and tests/test_resample_cpu.py holds equal to these.
static int print_tilings(int argc, char** argv) {
    if ((argc - 1) % 3 != 0) {
        fprintf(stderr, "usage: resample_selftest [in out channels]...\n");
        return 2;
    }
    for (int a = 1; a + 2 < argc; a += 3) {
        const int in = atoi(argv[a]), out = atoi(argv[a + 1]), ch = atoi(argv[a + 2]);
        if (in < 1 || in > 16384 || out < 1 || out > 16384 || (ch != 1 && ch != 3)) {
            fprintf(stderr, "resample_selftest: bad triple %s %s %s\n", argv[a], argv[a + 1], argv[a + 2]);
            return 2;
        }
        long long windows = 0, chunked = 0;
        check_axis(in, out, ch, &windows, &chunked);
        const int cols = resample_chunk_cols(ch), tw = resample_tile_width(in, out, ch), tiles = resample_tile_count(out, tw);
        int max_chunks = 0;
        for (int t = 0; t < tiles; ++t) {
            int c0, c1;
            resample_span(t * tw, (t + 1) * tw < out ? (t + 1) * tw : out, in, out, c0, c1);
            const int chunks = (c1 - c0 + cols - 1) / cols;
            max_chunks = chunks > max_chunks ? chunks : max_chunks;
        }
        printf("%d %d %d\n", tw, tiles, max_chunks);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) return print_tilings(argc, argv);
    g_in = g_out = g_ch = 0;
    CHECK(resample_applies(65, 64, 64, 64) && resample_applies(64, 65, 64, 64) && resample_applies(100, 40, 64, 64));
    CHECK(!resample_applies(64, 64, 64, 64) && !resample_applies(1, 1, 64, 64) && !resample_applies(30, 50, 64, 64));
    const int outs[] = {1, 2, 3, 48, 64, 256, 5, 17, 100, 513, 1000, 1024};
    long long windows = 0, chunked = 0;
    for (int in = 1; in <= 16384; ++in)
        for (int out : outs)
            for (int ch = 1; ch <= 3; ch += 2) check_axis(in, out, ch, &windows, &chunked);
    g_in = g_out = g_ch = 0;
    CHECK(chunked > 0);                             // 16384 -> 1 with three channels: one column's window is larger than a chunk
    // the example of the header's comment: 16384 -> 64 holds at most 513 taps
    int lo, hi, most = 0;
    for (int i = 0; i < 64; ++i) {
        resample_window(i, 16384, 64, lo, hi);
        most = most > hi - lo ? most : hi - lo;
    }
    CHECK(most == 512);
    printf("resample_selftest: ok (%lld windows, %lld tiles walk their span in chunks)\n", windows, chunked);
    return 0;
}
