// vs_res.h -- move-only owners of the library's HIP resources: device buffers, pinned host buffers, streams, events.
//
// Creation returns the library's status (VS_OK, or VS_ERR_DEVICE after set_error, as HIPCHK does) and never throws; the
// destructor releases.  A handle converts to its raw HIP type, so that launch and copy code takes it as it took the raw
// pointer (.get() where a cast needs the pointer itself).  Releasing does not wait for queued work that still uses the
// resource: whoever frees a buffer that may be in use synchronises first.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <utility>

#include "../../include/vsearch.h"
#include "vs_host.h"

namespace vs {

inline int hip_status(hipError_t e, const char* call) {
    if (e == hipSuccess) return VS_OK;
    set_error(std::string(call) + ": " + hipGetErrorString(e));
    return VS_ERR_DEVICE;
}

// n elements of T in device memory (Pinned: page-locked host memory)
template <class T, bool Pinned>
class Buf {
  public:
    Buf() = default;
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            n_ = std::exchange(o.n_, 0);
        }
        return *this;
    }
    ~Buf() { reset(); }

    // releases what the buffer held, then allocates n elements (at least one)
    int alloc(size_t n) {
        reset();
        void* p = nullptr;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        const int rc = Pinned ? hip_status(hipHostMalloc(&p, bytes, hipHostMallocDefault), "hipHostMalloc")
                              : hip_status(hipMalloc(&p, bytes), "hipMalloc");
        if (rc) return rc;
        p_ = static_cast<T*>(p);
        n_ = n;
        return VS_OK;
    }
    // grow only: a buffer of fewer than n elements is freed and allocated anew (contents lost)
    int reserve(size_t n) { return p_ && n_ >= n ? VS_OK : alloc(n); }
    void reset() {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        n_ = 0;
    }

    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t size() const { return n_; }

  private:
    T* p_ = nullptr;
    size_t n_ = 0;
};
template <class T>
using DevBuf = Buf<T, false>;
template <class T>
using PinBuf = Buf<T, true>;

// one stream or event handle H, released by Destroy
template <class H, hipError_t (*Destroy)(H)>
class Handle {
  public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Handle() { reset(); }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    operator H() const { return h_; }

  protected:
    int adopt(hipError_t e, H h, const char* call) {
        reset();
        if (e == hipSuccess) h_ = h;
        return hip_status(e, call);
    }
    H h_ = nullptr;
};

class Stream : public Handle<hipStream_t, hipStreamDestroy> {
  public:
    int create() {  // non-blocking
        hipStream_t s = nullptr;
        return adopt(hipStreamCreateWithFlags(&s, hipStreamNonBlocking), s, "hipStreamCreateWithFlags");
    }
};

class Event : public Handle<hipEvent_t, hipEventDestroy> {
  public:
    int create(bool timing = false) {
        hipEvent_t e = nullptr;
        return timing ? adopt(hipEventCreate(&e), e, "hipEventCreate")
                      : adopt(hipEventCreateWithFlags(&e, hipEventDisableTiming), e, "hipEventCreateWithFlags");
    }
};

}  // namespace vs
