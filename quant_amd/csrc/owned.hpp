// owned.hpp -- move-only owners of the engine's device memory, pinned host memory, streams and
// events.  The buffer template knows nothing of HIP: where a block comes from and
// how it is freed is its policy M, so tests/cpp builds this part with a counting fake under the
// sanitizers.  The HIP policies and the stream / event handles follow, for hipcc only.
#pragma once
#include <cstddef>

namespace qvq {

// n elements of T from policy M:
//   M::error M::alloc(void **p, void **dev, size_t bytes)   (*dev: the block's device address, or null)
//   void M::free(void *p);   M::error, M::ok: alloc's result type and its success value
// A failed alloc or ensure leaves the buffer empty (null, size 0); it never dangles.
template <typename T, typename M>
class Owned {
    T *p_ = nullptr, *dev_ = nullptr;
    size_t n_ = 0;

public:
    Owned() = default;
    Owned(Owned &&o) noexcept : p_(o.p_), dev_(o.dev_), n_(o.n_) { o.p_ = o.dev_ = nullptr, o.n_ = 0; }
    Owned &operator=(Owned &&o) noexcept {
        if (this != &o) {
            reset();
            p_ = o.p_, dev_ = o.dev_, n_ = o.n_;
            o.p_ = o.dev_ = nullptr, o.n_ = 0;
        }
        return *this;
    }
    ~Owned() { reset(); }
    T *get() const { return p_; }
    operator T *() const { return p_; }
    T *dev() const { return dev_; }   // mapped host memory: the device's alias of get()
    size_t size() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }
    void reset() {
        if (p_) M::free(p_);
        p_ = dev_ = nullptr, n_ = 0;
    }
    T *release() {   // the block handed over: the caller frees it
        T *p = p_;
        p_ = dev_ = nullptr, n_ = 0;
        return p;
    }
    // Exactly n elements; the old block is freed first (peak memory: one block).
    typename M::error alloc(size_t n) {
        reset();
        void *p = nullptr, *d = nullptr;
        const auto e = M::alloc(&p, &d, n * sizeof(T));
        if (e == M::ok) p_ = static_cast<T *>(p), dev_ = static_cast<T *>(d), n_ = n;
        return e;
    }
    // Grow only: at least n elements; a block that is large enough stays where it is.
    typename M::error ensure(size_t n) { return n_ >= n ? M::ok : alloc(n); }
};

}  // namespace qvq

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace qvq {

struct DeviceMem {
    using error = hipError_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t alloc(void **p, void **dev, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        *dev = *p;
        return e;
    }
    static void free(void *p) { (void)hipFree(p); }
};
// Pinned host memory under hipHostMalloc's flags; mapped memory also gets its device alias.
template <unsigned Flags>
struct PinnedMem {
    using error = hipError_t;
    static constexpr hipError_t ok = hipSuccess;
    static hipError_t alloc(void **p, void **dev, size_t bytes) {
        hipError_t e = hipHostMalloc(p, bytes, Flags);
        if (e != hipSuccess || !(Flags & hipHostMallocMapped)) return e;
        if ((e = hipHostGetDevicePointer(dev, *p, 0)) != hipSuccess) free(*p), *p = nullptr;
        return e;
    }
    static void free(void *p) { (void)hipHostFree(p); }
};
template <typename T> using DevBuf = Owned<T, DeviceMem>;
template <typename T> using PinnedBuf = Owned<T, PinnedMem<hipHostMallocDefault>>;
template <typename T> using MappedBuf = Owned<T, PinnedMem<hipHostMallocMapped>>;
template <typename T> using CoherentBuf = Owned<T, PinnedMem<hipHostMallocMapped | hipHostMallocCoherent>>;

// A stream or an event: created through put() by whichever hip*Create* call fits (flags, a
// priority), destroyed with its owner.
template <typename H, hipError_t (*Destroy)(H)>
class Handle {
    H h_ = nullptr;

public:
    Handle() = default;
    Handle(Handle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Handle &operator=(Handle &&o) noexcept {
        if (this != &o) reset(), h_ = o.h_, o.h_ = nullptr;
        return *this;
    }
    ~Handle() { reset(); }
    operator H() const { return h_; }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    H *put() {
        reset();
        return &h_;
    }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

}  // namespace qvq
#endif
