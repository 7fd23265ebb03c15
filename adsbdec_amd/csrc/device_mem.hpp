// device_mem.hpp -- owners of the HIP resources the host side holds (internal, host-only): a buffer that only grows (alone, or paired with
// its pinned twin: Table, Totals), an event, a stream.  Each frees what it holds when it goes, so a handle is torn down by `delete` (adsb_destroy only has
// to quiesce the streams first) and a failed allocation half-way through a regrow leaks nothing.  Move-only; each
// converts to the raw pointer or handle it owns, so the HIP calls and the kernels' argument structs take them as they are.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#pragma GCC visibility push(hidden)

namespace adsb {

enum class Mem { Device, Pinned, PinnedCoherent }; // hipMalloc / hipHostMalloc Default / hipHostMalloc Coherent

// `cap` elements at `p`, never shrunk and never copied: reserve() beyond cap releases the old array first, so whoever may
// still be using it -- a kernel, a copy in flight -- is waited for by the caller BEFORE the call.
template <class T, Mem Kind = Mem::Device> struct Buf {
    T *p = nullptr;
    size_t cap = 0; // elements

    Buf() = default;
    Buf(Buf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    Buf &operator=(Buf &&o) noexcept // (the old array goes: "allocate new, copy, then replace")
    {
        if (this != &o) {
            (void)release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~Buf() { (void)release(); }

    hipError_t release()
    {
        hipError_t e = hipSuccess;
        if (p)
            e = Kind == Mem::Device ? hipFree(p) : hipHostFree(p);
        p = nullptr, cap = 0;
        return e;
    }
    // Room for `want` elements.  A failed allocation leaves {nullptr, 0}.
    hipError_t reserve(size_t want)
    {
        if (want <= cap)
            return hipSuccess;
        hipError_t e = release();
        if (e != hipSuccess)
            return e;
        void *q = nullptr;
        e = Kind == Mem::Device   ? hipMalloc(&q, want * sizeof(T))
            : Kind == Mem::Pinned ? hipHostMalloc(&q, want * sizeof(T), hipHostMallocDefault)
                                  : hipHostMalloc(&q, want * sizeof(T), hipHostMallocCoherent);
        if (e != hipSuccess)
            return e;
        p = static_cast<T *>(q), cap = want;
        return hipSuccess;
    }
    operator T *() const { return p; }
};

// A table a launch reads on the device and the pinned array the host fills it in: grown together, with headroom, in bytes.
struct Table {
    Buf<char, Mem::Device> dev;
    Buf<char, Mem::Pinned> host;
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= host.cap) // (allocated last: where it has room, both have)
            return hipSuccess;
        const size_t want = bytes + bytes / 4 + 4096;
        const hipError_t e = dev.reserve(want);
        return e != hipSuccess ? e : host.reserve(want);
    }
};

// Totals a kernel adds to on the device and the pinned array the host reads them from: `words` each, allocated together; zeroed
// and copied back by whoever launches (decoder_level.hip; decoder_level_batch.hip: kLevelWords per capture of a sub-batch).
template <class T> struct Totals {
    Buf<T, Mem::Device> dev;
    Buf<T, Mem::Pinned> host;
    hipError_t reserve(size_t words)
    {
        const hipError_t e = dev.reserve(words);
        return e != hipSuccess ? e : host.reserve(words);
    }
};

struct Event {
    hipEvent_t ev = nullptr;

    Event() = default;
    Event(Event &&o) noexcept : ev(o.ev) { o.ev = nullptr; }
    ~Event()
    {
        if (ev)
            (void)hipEventDestroy(ev);
    }
    hipError_t create(unsigned flags = hipEventDefault)
    {
        const hipError_t e = hipEventCreateWithFlags(&ev, flags);
        if (e != hipSuccess)
            ev = nullptr;
        return e;
    }
    operator hipEvent_t() const { return ev; }
};

// A stream of the library's own, or one the caller handed in (adsb_config.stream), which is used and never destroyed.
struct Stream {
    hipStream_t st = nullptr;
    bool owned = false;

    Stream() = default;
    Stream(Stream &&o) noexcept : st(o.st), owned(o.owned) { o.st = nullptr; }
    ~Stream()
    {
        if (st && owned)
            (void)hipStreamDestroy(st);
    }
    void adopt(hipStream_t theirs) { st = theirs, owned = false; }
    hipError_t create() { return created(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); }
    hipError_t create_with_priority(int priority) { return created(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, priority)); }
    operator hipStream_t() const { return st; }

private:
    hipError_t created(hipError_t e)
    {
        owned = e == hipSuccess;
        if (!owned)
            st = nullptr;
        return e;
    }
};

} // namespace adsb

#pragma GCC visibility pop
