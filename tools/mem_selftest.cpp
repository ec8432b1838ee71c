// mem_selftest -- the owners of csrc/idc_mem.h over counting fakes: no device, no HIP runtime call.
//
// FakeAlloc hands out malloc blocks, keeps the set of live ones, fails the k-th allocation on request and aborts with a message when a block is
// released twice or was never handed out.  Checked (tests/test_mem_cpu.py runs this; `make mem_selftest SAN=1` builds it under ASan + UBSan):
//   1. a sufficient capacity leaves pointer and size alone and allocates nothing;
//   2. a grow releases the old block exactly once, before it allocates, honours the floor and does not round a request above it
//      (the picker's 65536 bytes, the hint list's 256 entries and its 2 x n rule);
//   3. a five-buffer "ensure all" sequence shaped like ensure_post_buffers, its k-th allocation failing for k = 1..5: the failed member is empty,
//      the repeated sequence allocates exactly the members that were missing and all five hold their sizes;
//   4. move construction, move assignment onto a non-empty owner and reset() release exactly what they should;
//   5. nothing is live at exit -- and the same exactly-once checks for the stream / event owner over a fake create / destroy pair.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

#include "idc_mem.h"

using namespace idc;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

struct FakeAlloc {
    static std::set<void*> live;
    static std::vector<char> log;        // 'a' per allocation, 'r' per release, in order
    static int allocs, releases, fail_at;    // fail_at: the allocation (counted from 1, from when it is set) that fails; 0 = none
    static size_t last_bytes;
    static unsigned last_flags;
    static hipError_t alloc(void** p, size_t bytes, unsigned flags) {
        if (fail_at > 0 && --fail_at == 0) return hipErrorOutOfMemory;
        *p = malloc(bytes ? bytes : 1);
        live.insert(*p);
        ++allocs; last_bytes = bytes; last_flags = flags; log.push_back('a');
        return hipSuccess;
    }
    static void release(void* p) {
        if (!live.erase(p)) {
            fprintf(stderr, "FakeAlloc: %p released twice, or never handed out\n", p);
            abort();
        }
        free(p);
        ++releases; log.push_back('r');
    }
};
std::set<void*> FakeAlloc::live;
std::vector<char> FakeAlloc::log;
int FakeAlloc::allocs = 0, FakeAlloc::releases = 0, FakeAlloc::fail_at = 0;
size_t FakeAlloc::last_bytes = 0;
unsigned FakeAlloc::last_flags = 0;

template <class T> using FakeMem = Mem<T, FakeAlloc>;

struct FakeKind {
    using type = int*;
    static std::set<type> live;
    static int creates, destroys, fail_at;
    static unsigned last_flags;
    static hipError_t create(type* h, unsigned flags) {
        if (fail_at > 0 && --fail_at == 0) return hipErrorOutOfMemory;
        *h = new int(0);
        live.insert(*h);
        ++creates; last_flags = flags;
        return hipSuccess;
    }
    static void destroy(type h) {
        if (!live.erase(h)) {
            fprintf(stderr, "FakeKind: %p destroyed twice, or never created\n", (void*)h);
            abort();
        }
        delete h;
        ++destroys;
    }
};
std::set<int*> FakeKind::live;
int FakeKind::creates = 0, FakeKind::destroys = 0, FakeKind::fail_at = 0;
unsigned FakeKind::last_flags = 0;

using FakeHandle = Handle<FakeKind>;

static void test_sufficient_capacity() {
    FakeMem<float> m;
    CHECK(m.get() == nullptr && m.bytes() == 0);
    CHECK(m.ensure(0) == hipSuccess && m.get() == nullptr && FakeAlloc::allocs == 0);      // nothing asked, nothing allocated
    CHECK(m.ensure(1000) == hipSuccess && m.bytes() == 1000 && m.get() != nullptr);
    float* const p = m.get();
    const int a = FakeAlloc::allocs, r = FakeAlloc::releases;
    CHECK(m.ensure(1000) == hipSuccess && m.ensure(1) == hipSuccess && m.ensure(0) == hipSuccess && m.ensure(999, 1 << 20) == hipSuccess);
    CHECK(m.get() == p && m.bytes() == 1000 && FakeAlloc::allocs == a && FakeAlloc::releases == r);
}

static void test_grow_and_floor() {
    const size_t rect = 28;              // sizeof(HintRect): four ints, three floats
    {   // the picker: 65536 bytes to begin with, the exact size above that
        FakeMem<unsigned char> pick;
        CHECK(pick.ensure(100, 65536) == hipSuccess && pick.bytes() == 65536 && FakeAlloc::last_bytes == 65536);
        unsigned char* const p = pick.get();
        CHECK(pick.ensure(65536, 65536) == hipSuccess && pick.get() == p);
        FakeAlloc::log.clear();
        const int r = FakeAlloc::releases;
        CHECK(pick.ensure(65537, 65536) == hipSuccess && pick.bytes() == 65537 && FakeAlloc::last_bytes == 65537);      // not rounded
        CHECK(FakeAlloc::releases == r + 1);
        CHECK(FakeAlloc::log.size() == 2 && FakeAlloc::log[0] == 'r' && FakeAlloc::log[1] == 'a');                      // old block first
        CHECK(FakeAlloc::live.size() == 1);
    }
    {   // the hint list: 256 entries to begin with, 2 x n once it is longer (idc_set_hints)
        FakeMem<char> hints;
        auto cap = [&](size_t n) { return (n < 256 ? 256 : 2 * n) * rect; };
        CHECK(hints.ensure(1 * rect, cap(1)) == hipSuccess && hints.bytes() == 256 * rect);
        char* const p = hints.get();
        CHECK(hints.ensure(256 * rect, cap(256)) == hipSuccess && hints.get() == p && hints.bytes() == 256 * rect);
        const int a = FakeAlloc::allocs, r = FakeAlloc::releases;
        CHECK(hints.ensure(300 * rect, cap(300)) == hipSuccess && hints.bytes() == 600 * rect);
        CHECK(FakeAlloc::allocs == a + 1 && FakeAlloc::releases == r + 1);
        char* const q = hints.get();
        CHECK(hints.ensure(2 * rect, cap(2)) == hipSuccess && hints.ensure(600 * rect, cap(600)) == hipSuccess && hints.get() == q);
        CHECK(FakeAlloc::allocs == a + 1 && FakeAlloc::releases == r + 1);
    }
    CHECK(FakeAlloc::live.empty());
}

// five members ensured in a row, each call returning at the first failure: ensure_post_buffers
struct Five {
    FakeMem<unsigned char> d_rgb;
    FakeMem<double> d_labq;
    FakeMem<float> d_post_in;
    FakeMem<unsigned char> h_rgb;
    FakeMem<double> h_labq;
    static constexpr size_t px = 64 * 64 * 2;
    const size_t want[5] = {px * 3, px * 3 * 8, px * 3 * 4, px * 3, px * 3 * 8};
    hipError_t ensure_all() {
        hipError_t e;
        if ((e = d_rgb.ensure(want[0])) != hipSuccess) return e;
        if ((e = d_labq.ensure(want[1])) != hipSuccess) return e;
        if ((e = d_post_in.ensure(want[2])) != hipSuccess) return e;
        if ((e = h_rgb.ensure(want[3])) != hipSuccess) return e;
        return h_labq.ensure(want[4]);
    }
    size_t bytes(int i) const { return i == 0 ? d_rgb.bytes() : i == 1 ? d_labq.bytes() : i == 2 ? d_post_in.bytes() : i == 3 ? h_rgb.bytes() : h_labq.bytes(); }
    const void* ptr(int i) const {
        return i == 0 ? (const void*)d_rgb.get() : i == 1 ? (const void*)d_labq.get() : i == 2 ? (const void*)d_post_in.get() : i == 3 ? (const void*)h_rgb.get()
                                                                                                                                        : (const void*)h_labq.get();
    }
};

static void test_failure_and_retry() {
    for (int k = 1; k <= 5; ++k) {
        {
            Five f;
            const int a0 = FakeAlloc::allocs;
            FakeAlloc::fail_at = k;
            CHECK(f.ensure_all() == hipErrorOutOfMemory);
            CHECK(FakeAlloc::fail_at == 0 && FakeAlloc::allocs == a0 + k - 1);
            for (int i = 0; i < 5; ++i) {          // the members before the failure hold their blocks; the failed one and those after it are empty
                CHECK(f.bytes(i) == (i < k - 1 ? f.want[i] : 0));
                CHECK((f.ptr(i) != nullptr) == (i < k - 1));
            }
            const void* before[5];
            for (int i = 0; i < 5; ++i) before[i] = f.ptr(i);
            const int a1 = FakeAlloc::allocs, r1 = FakeAlloc::releases;
            CHECK(f.ensure_all() == hipSuccess);
            CHECK(FakeAlloc::allocs == a1 + (5 - (k - 1)) && FakeAlloc::releases == r1);       // only what was missing, nothing given back
            for (int i = 0; i < 5; ++i) {
                CHECK(f.bytes(i) == f.want[i] && f.ptr(i) != nullptr);
                if (i < k - 1) CHECK(f.ptr(i) == before[i]);
            }
            const int a2 = FakeAlloc::allocs;
            CHECK(f.ensure_all() == hipSuccess && FakeAlloc::allocs == a2);                    // and a third pass does nothing
            CHECK(FakeAlloc::live.size() == 5);
        }
        CHECK(FakeAlloc::live.empty());
    }
    {   // a failed grow leaves the owner empty (the old block is gone, once), and the next ensure allocates
        FakeMem<float> m;
        CHECK(m.ensure(64) == hipSuccess);
        const int r = FakeAlloc::releases;
        FakeAlloc::fail_at = 1;
        CHECK(m.ensure(128) == hipErrorOutOfMemory && m.get() == nullptr && m.bytes() == 0 && FakeAlloc::releases == r + 1);
        CHECK(m.ensure(16) == hipSuccess && m.bytes() == 16 && FakeAlloc::releases == r + 1);
    }
    CHECK(FakeAlloc::live.empty());
}

static void test_move_and_reset() {
    {
        FakeMem<int> a(7u);              // the policy's flags travel with the owner
        CHECK(a.ensure(40) == hipSuccess && FakeAlloc::last_flags == 7u);
        int* const pa = a.get();
        const int r = FakeAlloc::releases;
        FakeMem<int> b(std::move(a));                                                          // move construction: nothing released
        CHECK(a.get() == nullptr && a.bytes() == 0 && b.get() == pa && b.bytes() == 40 && FakeAlloc::releases == r);
        FakeMem<int> c;
        CHECK(c.ensure(80) == hipSuccess);
        int* const pc = c.get();
        c = std::move(b);                                                                      // onto a non-empty owner: its block goes, once
        CHECK(FakeAlloc::releases == r + 1 && !FakeAlloc::live.count(pc) && FakeAlloc::live.count(pa));
        CHECK(c.get() == pa && c.bytes() == 40 && b.get() == nullptr && b.bytes() == 0);
        CHECK(c.ensure(400) == hipSuccess && FakeAlloc::last_flags == 7u);
        FakeMem<int>& self = c;
        c = std::move(self);                                                                   // self-assignment keeps the block
        CHECK(c.bytes() == 400 && FakeAlloc::live.count(c.get()));
        const int r2 = FakeAlloc::releases;
        c.reset();
        CHECK(c.get() == nullptr && c.bytes() == 0 && FakeAlloc::releases == r2 + 1);
        c.reset();                                                                             // empty: nothing to release
        a.reset(); b.reset();
        CHECK(FakeAlloc::releases == r2 + 1 && FakeAlloc::live.empty());
    }
    {   // a vector of owners (the per-slot sources, the per-tensor allocations, the profiling events) grows by moves
        std::vector<FakeMem<char>> v(3);
        for (size_t i = 0; i < v.size(); ++i) CHECK(v[i].ensure(10 + i) == hipSuccess);
        const int r = FakeAlloc::releases;
        v.resize(100);
        CHECK(FakeAlloc::releases == r && FakeAlloc::live.size() == 3 && v[2].bytes() == 12);
        v[1] = FakeMem<char>();                                                                // drop_source
        CHECK(FakeAlloc::releases == r + 1 && v[1].get() == nullptr);
    }
    CHECK(FakeAlloc::live.empty());
}

static void test_handles() {
    {
        FakeHandle s;
        CHECK(s.get() == nullptr);
        FakeKind::fail_at = 1;
        CHECK(s.create(3u) == hipErrorOutOfMemory && s.get() == nullptr && FakeKind::creates == 0);
        CHECK(s.create(3u) == hipSuccess && s.get() != nullptr && FakeKind::creates == 1 && FakeKind::last_flags == 3u);
        int* const h = s.get();
        CHECK(s.create(3u) == hipSuccess && s.get() == h && FakeKind::creates == 1);           // once: the handle that is there stays
        FakeHandle t(std::move(s));
        CHECK(s.get() == nullptr && t.get() == h && FakeKind::destroys == 0);
        FakeHandle u;
        CHECK(u.create() == hipSuccess && FakeKind::last_flags == 0u);
        u = std::move(t);
        CHECK(FakeKind::destroys == 1 && u.get() == h && t.get() == nullptr);
        u.reset(); u.reset();
        CHECK(FakeKind::destroys == 2 && u.get() == nullptr);
        std::vector<FakeHandle> ring;
        ring.resize(8);
        for (auto& e : ring) CHECK(e.create() == hipSuccess);
        ring.resize(64);
        for (auto& e : ring) CHECK(e.create() == hipSuccess);
        CHECK(FakeKind::creates == 2 + 64 && FakeKind::live.size() == 64);
    }
    CHECK(FakeKind::live.empty() && FakeKind::creates == FakeKind::destroys);
}

int main() {
    test_sufficient_capacity();
    test_grow_and_floor();
    test_failure_and_retry();
    test_move_and_reset();
    test_handles();
    CHECK(FakeAlloc::live.empty() && FakeAlloc::allocs == FakeAlloc::releases);
    CHECK(FakeKind::live.empty());
    printf("mem_selftest: ok (%d blocks, %d handles)\n", FakeAlloc::allocs, FakeKind::creates);
    return 0;
}
