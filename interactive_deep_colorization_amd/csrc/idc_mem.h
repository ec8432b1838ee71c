// idc_mem.h -- who owns what the host code takes from the HIP runtime: device and pinned memory (Mem over an allocator policy), streams and
// events (Handle over a create / destroy pair).  Move-only; an empty owner releases nothing, so a handle that never touched the device
// (tools/plan_dump.cpp) destroys without a runtime call.  Host-only, nothing of the project's included: tools/mem_selftest.cpp instantiates
// both templates over counting fakes.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace idc {

struct DeviceAlloc {
    static hipError_t alloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
    static void release(void* p) { (void)hipFree(p); }
};
struct PinnedAlloc {
    static hipError_t alloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
    static void release(void* p) { (void)hipHostFree(p); }
};

template <class T, class Alloc>
class Mem {
  public:
    Mem() = default;
    explicit Mem(unsigned flags) : flags_(flags) {}      // allocation flags of the policy (pinned: hipHostMallocMapped for device-visible memory)
    Mem(Mem&& o) noexcept : p_(o.p_), bytes_(o.bytes_), flags_(o.flags_) { o.p_ = nullptr; o.bytes_ = 0; }
    Mem& operator=(Mem&& o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; flags_ = o.flags_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~Mem() { reset(); }
    T* get() const { return p_; }
    size_t bytes() const { return bytes_; }
    // At least `bytes` afterwards.  Enough already: nothing happens.  Otherwise the old block goes first, then max(bytes, floor) is allocated (the
    // contents are not carried over); on failure the owner is empty and a later ensure tries again.  Knows nothing about streams: whoever may
    // still have work in flight on the old block synchronises before calling.
    hipError_t ensure(size_t bytes, size_t floor = 0) {
        if (bytes_ >= bytes) return hipSuccess;
        reset();
        const size_t want = bytes < floor ? floor : bytes;
        void* p = nullptr;
        const hipError_t e = Alloc::alloc(&p, want, flags_);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p); bytes_ = want;
        return hipSuccess;
    }
    void reset() {
        if (p_) Alloc::release((void*)p_);
        p_ = nullptr; bytes_ = 0;
    }

  private:
    T* p_ = nullptr;
    size_t bytes_ = 0;
    unsigned flags_ = 0;
};
template <class T> using DevMem = Mem<T, DeviceAlloc>;
template <class T> using PinnedMem = Mem<T, PinnedAlloc>;

struct StreamKind {
    using type = hipStream_t;
    static hipError_t create(type* h, unsigned flags) { return hipStreamCreateWithFlags(h, flags); }
    static void destroy(type h) { (void)hipStreamDestroy(h); }
};
struct EventKind {
    using type = hipEvent_t;
    static hipError_t create(type* h, unsigned flags) { return hipEventCreateWithFlags(h, flags); }
    static void destroy(type h) { (void)hipEventDestroy(h); }
};

template <class Kind>
class Handle {
  public:
    using type = typename Kind::type;
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = type{}; }
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) { reset(); h_ = o.h_; o.h_ = type{}; }
        return *this;
    }
    ~Handle() { reset(); }
    type get() const { return h_; }
    hipError_t create(unsigned flags = 0) {              // once: a handle that is already there stays (0 = hipStreamDefault / hipEventDefault)
        if (h_) return hipSuccess;
        type h{};
        const hipError_t e = Kind::create(&h, flags);
        if (e == hipSuccess) h_ = h;
        return e;
    }
    void reset() {
        if (h_) Kind::destroy(h_);
        h_ = type{};
    }

  private:
    type h_{};
};
using Stream = Handle<StreamKind>;
using Event = Handle<EventKind>;

}  // namespace idc
