// ffq_mem.h -- who owns device and pinned memory: one grow-only buffer type, a device + pinned pair of them.
//
// A Buf is a pointer and a capacity in ELEMENTS that free themselves.  grow() is the only way to get memory and it keeps
// what is there if that is enough; otherwise the old block is freed BEFORE the new one is asked for, and a request that
// fails leaves the buffer empty (p == nullptr, cap == 0), ready to be grown again.  Nothing else is decided here: the
// caller synchronises whatever may still use the old block before it grows, picks the size, binds its thread where the
// pinned pages should lie, and words the error (csrc/ffq_hip.hip, csrc/ffq_stream.h).
//
// An allocator policy is { using error; static constexpr error ok; static error alloc(void **, size_t bytes);
// static void release(void *); }.  The two of the library are at the end of this file; tests/membuf_host.cpp defines
// FFQ_MEM_NO_HIP and drives the templates with a counting malloc on a CPU.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ffq {

template <class T, class Alloc>
struct Buf {
    T *p = nullptr;
    int64_t cap = 0;             // elements

    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept
    {
        if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~Buf() { reset(); }

    void reset()
    {
        if (p) Alloc::release(p);
        p = nullptr; cap = 0;
    }

    typename Alloc::error grow(int64_t need)
    {
        if (need <= cap) return Alloc::ok;
        reset();
        void *q = nullptr;
        const typename Alloc::error e = Alloc::alloc(&q, (size_t)need * sizeof(T));
        if (e != Alloc::ok) return e;
        p = static_cast<T *>(q); cap = need;
        return Alloc::ok;
    }

    operator T *() const { return p; }
    T *operator->() const { return p; }
};

// a device buffer `d` and its pinned mirror `h`, grown together: both hold `need` elements, or both are empty
template <class T, class DevA, class PinA>
struct MirrorOf {
    Buf<T, DevA> d;
    Buf<T, PinA> h;

    typename DevA::error grow(int64_t need)
    {
        if (need <= d.cap && need <= h.cap) return DevA::ok;
        reset();
        typename DevA::error e = d.grow(need);
        if (e == DevA::ok) e = h.grow(need);
        if (e != DevA::ok) reset();
        return e;
    }
    void reset() { d.reset(); h.reset(); }
};

}  // namespace ffq

#ifndef FFQ_MEM_NO_HIP
#include <hip/hip_runtime_api.h>

namespace ffq {

struct DevAlloc {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void release(void *p) { (void)hipFree(p); }
};

template <unsigned Flags>
struct PinAlloc {
    using error = hipError_t;
    static constexpr error ok = hipSuccess;
    static error alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
    static void release(void *p) { (void)hipHostFree(p); }
};

template <class T> using DevBuf = Buf<T, DevAlloc>;
template <class T, unsigned Flags = hipHostMallocDefault> using PinBuf = Buf<T, PinAlloc<Flags>>;
template <class T> using Mirror = MirrorOf<T, DevAlloc, PinAlloc<hipHostMallocDefault>>;

}  // namespace ffq
#endif  // FFQ_MEM_NO_HIP
