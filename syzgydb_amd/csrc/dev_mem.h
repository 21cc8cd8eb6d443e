// dev_mem.h -- who owns device memory: the owning buffers of the library and the ONE function every device allocation of
// theirs goes through.  Like column_str.h it is plain C++ given a backend -- allocate, free, set the device, the pinned
// forms, and how an error is reported -- so the library (HipBackend, below) and a host program over malloc
// (tests/cpp/test_dev_mem.cpp, under the sanitizers) run the same code.
//
//   BasicBuf<T, pinned>  a pointer and a capacity in elements, freed by the destructor.  Move-only.
//   BasicDevMem<T>       ... bound to a device ordinal: allocation and release make that device current.  What lives
//                        as long as a shard, a column or a mask is one of these.
//
// ensure(n) is the scratch rule: nothing while n elements fit, otherwise free FIRST (the old and the new block never
// exist side by side) and allocate max(n, 64) -- the contents are never carried over.  alloc_exact(n) releases and
// allocates exactly n (sizes the library reports -- a column's device_bytes, a heap's capacity -- are the sizes asked
// for).  Memory whose contents matter grows at the call site, in one shape:
//
//     DevMem<T> bigger(device);
//     if (int rc = bigger.alloc_exact(n, "what")) return rc;   // the holder is untouched
//     ... copy holder -> bigger ...
//     holder = std::move(bigger);                               // the old block goes here, on the holder's device
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace szgi {

enum DevErr {
    kDevRefused,  // the test hook's countdown refused the allocation on the host: out of memory, "(refused: test hook)"
    kDevNoMem,    // the backend's device allocation failed: out of memory
    kDevFailed,   // any other backend call failed
};

// Process-wide: the device blocks alive and their bytes (pinned memory is not counted), and the countdown of the test
// hook -- armed with n > 0, the n-th device allocation from now on is refused before the backend is asked, and the
// countdown disarms itself.
struct DevAllocState {
    std::atomic<uint64_t> blocks{0}, bytes{0};
    std::atomic<int64_t> refuse_in{0};
};
inline DevAllocState &dev_alloc_state()
{
    static DevAllocState s;
    return s;
}

// every device allocation of the buffers below; real_failure: what a failure of the backend itself counts as
template <class B>
int dev_block_alloc(void **p, size_t bytes, DevErr real_failure, const char *what)
{
    DevAllocState &st = dev_alloc_state();
    int64_t left = st.refuse_in.load();
    while (left > 0 && !st.refuse_in.compare_exchange_weak(left, left - 1)) {}
    if (left == 1) return B::error(kDevRefused, what, 0);
    *p = nullptr;
    if (const int e = B::dev_alloc(p, bytes)) return B::error(real_failure, what, e);
    st.blocks++;
    st.bytes += bytes;
    return 0;
}
template <class B>
int dev_block_free(void *p, size_t bytes)
{
    DevAllocState &st = dev_alloc_state();
    st.blocks--;
    st.bytes -= bytes;
    if (const int e = B::dev_free(p)) return B::error(kDevFailed, "free of device memory", e);
    return 0;
}

template <typename T, bool kPinned, class B>
class BasicBuf {
    T *p_ = nullptr;
    size_t cap_ = 0;

    int alloc(size_t n, DevErr real_failure, const char *what)  // (the buffer is empty)
    {
        void *p = nullptr;
        if (kPinned) {
            if (const int e = B::pinned_alloc(&p, n * sizeof(T))) return B::error(kDevFailed, what, e);
        } else if (const int rc = dev_block_alloc<B>(&p, n * sizeof(T), real_failure, what)) {
            return rc;
        }
        p_ = static_cast<T *>(p);
        cap_ = n;
        return 0;
    }

public:
    BasicBuf() = default;
    BasicBuf(BasicBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    BasicBuf &operator=(BasicBuf &&o) noexcept  // what this buffer held is released
    {
        if (this != &o) {
            (void)reset();
            p_ = o.p_, cap_ = o.cap_;
            o.p_ = nullptr, o.cap_ = 0;
        }
        return *this;
    }
    ~BasicBuf() { (void)reset(); }
    T *data() const { return p_; }
    operator T *() const { return p_; }
    size_t capacity() const { return cap_; }
    int reset()
    {
        if (!p_) return 0;
        T *p = p_;
        const size_t bytes = cap_ * sizeof(T);
        p_ = nullptr;
        cap_ = 0;
        if (!kPinned) return dev_block_free<B>(p, bytes);
        if (const int e = B::pinned_free(p)) return B::error(kDevFailed, "free of pinned memory", e);
        return 0;
    }
    int ensure(size_t need, const char *what = "scratch allocation")
    {
        if (cap_ >= need) return 0;
        if (const int rc = reset()) return rc;
        return alloc(need < 64 ? 64 : need, kDevFailed, what);
    }
    int alloc_exact(size_t n, const char *what)
    {
        if (const int rc = reset()) return rc;
        return n ? alloc(n, kDevNoMem, what) : 0;
    }
};

template <typename T, class B>
class BasicDevMem {
    int device_ = 0;
    BasicBuf<T, false, B> buf_;

    int make_current() const
    {
        if (const int e = B::set_device(device_)) return B::error(kDevFailed, "set device", e);
        return 0;
    }

public:
    explicit BasicDevMem(int device = 0) : device_(device) {}
    BasicDevMem(BasicDevMem &&) noexcept = default;
    BasicDevMem &operator=(BasicDevMem &&o) noexcept  // what this one held is released, on ITS device
    {
        if (this != &o) {
            (void)reset();
            device_ = o.device_;
            buf_ = std::move(o.buf_);
        }
        return *this;
    }
    ~BasicDevMem() { (void)reset(); }
    int device() const { return device_; }
    T *data() const { return buf_.data(); }
    operator T *() const { return buf_.data(); }
    size_t capacity() const { return buf_.capacity(); }
    int reset()
    {
        if (!buf_.data()) return 0;
        const int rc = make_current();
        const int rc2 = buf_.reset();
        return rc ? rc : rc2;
    }
    int ensure(size_t need, const char *what = "scratch allocation")  // (the device is current afterwards either way)
    {
        if (const int rc = make_current()) return rc;
        return buf_.ensure(need, what);
    }
    int alloc_exact(size_t n, const char *what)
    {
        if (const int rc = reset()) return rc;
        if (n == 0) return 0;
        if (const int rc = make_current()) return rc;
        return buf_.alloc_exact(n, what);
    }
};

}  // namespace szgi

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace szgi {

int dev_mem_error(DevErr kind, const char *what, hipError_t e);  // api_common.cpp: the error text and the SZG_E_* code

struct HipBackend {
    static int set_device(int device) { return (int)hipSetDevice(device); }
    static int dev_alloc(void **p, size_t bytes)
    {
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) (void)hipGetLastError();  // (not sticky: the caller may go on without the block)
        return (int)e;
    }
    static int dev_free(void *p) { return (int)hipFree(p); }
    static int pinned_alloc(void **p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static int pinned_free(void *p) { return (int)hipHostFree(p); }
    static int error(DevErr kind, const char *what, int e) { return dev_mem_error(kind, what, (hipError_t)e); }
};
template <typename T> using DevBuf = BasicBuf<T, false, HipBackend>;    // device memory of the device that is current
template <typename T> using PinnedBuf = BasicBuf<T, true, HipBackend>;  // pinned host memory
template <typename T> using DevMem = BasicDevMem<T, HipBackend>;        // device memory of its own device

}  // namespace szgi
#endif
