// smpl_amd/csrc/device_mem.h -- who owns device memory on the construction side (grid_handle.h, field.hip and the headers
// in its tail): one owning pointer and one work space.  No kernel includes this.
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
