// smpl_amd/csrc/device_mem.h -- who owns what the host holds on the device, on the construction side (grid_handle.h,
// field.hip and the headers in its tail) and on the search side (space.h and the headers of engine.hip): one owning
// pointer, the buffers that only ever grow, one work space, and the owners of a stream and of an event.  Every hipFree,
// hipHostFree, hipStreamDestroy and hipEventDestroy of the library is in this file.  No kernel includes this.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

// an owning device pointer: move-only, freed by its destructor; reads like the plain pointer wherever one is expected
template <class T>
struct DevPtr {
    T* p = nullptr;
    DevPtr() = default;
    DevPtr(DevPtr&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevPtr& operator=(DevPtr&& o) noexcept { if (this != &o) { reset(); p = o.p; o.p = nullptr; } return *this; }
    ~DevPtr() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; }
    // frees what it holds, then allocates n entries (one where n is 0: a list may be empty)
    hipError_t alloc(size_t n) { reset(); return hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)); }
    operator T*() const { return p; }
};

// a device buffer that only ever grows: a DevPtr (its `p` is the plain pointer) plus the entries it has room for.
// reserve(n) does nothing when n fits; else it frees the block, then allocates max(n, 64) entries.  After a failure the
// buffer is empty (p == nullptr, cap == 0).  The host engine calls it through reserve() of host_core.h, for an SMPLX code.
template <class T>
struct DevBuf : DevPtr<T> {
    size_t cap = 0;
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        cap = 0;
        const size_t want = n > 64 ? n : 64;
        if (const hipError_t e = this->alloc(want)) { this->p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
};

// its pinned host twin
template <class T>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    ~PinBuf() { reset(); }
    void reset() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
    hipError_t reserve(size_t n)
    {
        if (n <= cap) return hipSuccess;
        reset();
        const size_t want = n > 64 ? n : 64;
        if (const hipError_t e = hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault)) { p = nullptr; return e; }
        cap = want;
        return hipSuccess;
    }
};

// an owning stream or event: move-only, destroyed by its destructor; reads like the raw handle
template <class H, hipError_t (*Destroy)(H)>
struct DevHandle {
    H h = nullptr;
    DevHandle() = default;
    DevHandle(DevHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    DevHandle& operator=(DevHandle&& o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
    ~DevHandle() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    operator H() const { return h; }
};

struct DevStream : DevHandle<hipStream_t, hipStreamDestroy> {
    hipError_t create() { reset(); return hipStreamCreate(&h); }
};

struct DevEvent : DevHandle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { reset(); return hipEventCreateWithFlags(&h, flags); }
};

// the arrays of one call, carved out of one block that grows and never shrinks: a device allocation costs more than the
// kernels it serves (tools/voxelize_time.py).  A call that needs more frees the old block first; what an earlier call
// left in the block is gone either way, so calls on one owner take turns (they are not reentrant).
struct WorkSpace {
    DevPtr<char> base;
    size_t bytes = 0;
    // at[i] = offset of an array of sizes[i] bytes, each on a 256-byte boundary
    template <int N>
    hipError_t carve(const size_t (&sizes)[N], size_t (&at)[N])
    {
        size_t need = 0;
        for (int i = 0; i < N; ++i) { at[i] = need; need += (sizes[i] + 255) & ~(size_t)255; }
        if (need <= bytes) return hipSuccess;
        bytes = 0;
        const hipError_t e = base.alloc(need);
        if (e == hipSuccess) bytes = need;
        return e;
    }
};
