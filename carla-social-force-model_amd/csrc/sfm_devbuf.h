// sfm_devbuf.h -- what the host side of libsfm_hip.so owns on the device: arrays, pinned host blocks, events, a stream.
// Each wrapper owns one HIP object, is move-only, and releases it in its destructor; the destructor decides nothing about
// ordering -- whoever drops a buffer a kernel may still read synchronises first.  Needs the HIP runtime API and
// the standard library only (a plain host compiler will do).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>

namespace sfm {

struct DeviceMem {
    static hipError_t get(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t put(void* p) { return hipFree(p); }
};
struct PinnedMem {
    static hipError_t get(void** p, size_t bytes) { return hipHostMalloc(p, bytes, 0); }
    static hipError_t put(void* p) { return hipHostFree(p); }
};

// An array of T and its capacity in elements.  Converts to T*, so kernel argument structs fill as from a raw pointer.
template <typename T, typename Mem>
class OwnedBuf {
public:
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf&) = delete;
    OwnedBuf& operator=(const OwnedBuf&) = delete;
    OwnedBuf(OwnedBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {
        if (this != &o) { (void)reset(); swap(*this, o); }
        return *this;
    }
    ~OwnedBuf() { (void)reset(); }

    hipError_t reset() {
        T* p = p_;
        p_ = nullptr;
        cap_ = 0;
        return p ? Mem::put(p) : hipSuccess;
    }
    // frees, then allocates exactly n elements (n == 0: stays empty); empty with capacity 0 after a failure
    hipError_t alloc(size_t n) {
        hipError_t e = reset();
        if (e != hipSuccess || n == 0) return e;
        void* q = nullptr;
        e = Mem::get(&q, n * sizeof(T));
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(q);
        cap_ = n;
        return hipSuccess;
    }
    // grow-only, for buffers a host-in-the-loop caller refills every tick: hipMalloc / hipFree cost tens of microseconds
    // and synchronise the device
    hipError_t reserve(size_t n) {
        if (n <= cap_ && p_) return hipSuccess;
        return alloc(n + n / 2 + 16);
    }

    operator T*() const { return p_; }
    T* get() const { return p_; }
    size_t cap() const { return cap_; }
    friend void swap(OwnedBuf& a, OwnedBuf& b) noexcept { std::swap(a.p_, b.p_); std::swap(a.cap_, b.cap_); }

private:
    T* p_ = nullptr;
    size_t cap_ = 0;
};

template <typename T> using DevBuf = OwnedBuf<T, DeviceMem>;
template <typename T> using PinnedBuf = OwnedBuf<T, PinnedMem>;

// An event or a stream: created on demand, destroyed with its owner.  Converts to the raw handle.
template <typename H, hipError_t (*Destroy)(H)>
class OwnedHandle {
public:
    OwnedHandle() = default;
    OwnedHandle(const OwnedHandle&) = delete;
    OwnedHandle& operator=(const OwnedHandle&) = delete;
    OwnedHandle(OwnedHandle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    OwnedHandle& operator=(OwnedHandle&& o) noexcept {
        if (this != &o) { reset(); std::swap(h_, o.h_); }
        return *this;
    }
    ~OwnedHandle() { reset(); }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    operator H() const { return h_; }

protected:
    H h_ = nullptr;
};

struct Event : OwnedHandle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        const hipError_t e = hipEventCreateWithFlags(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
};

struct Stream : OwnedHandle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) {
        reset();
        const hipError_t e = hipStreamCreateWithFlags(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
};

}  // namespace sfm
