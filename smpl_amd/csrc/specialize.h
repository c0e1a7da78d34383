// smpl_amd/csrc/specialize.h -- per-robot kernel specialisation.  The kinematic structure of a compiled model
// (joint kinds and origins, which link carries which sphere tree, the checked pairs) is turned into compile-time
// constants (model_compile.cpp model_const_header) and kernels.hip, with the headers it includes, is compiled against
// them with hiprtc when a planning space is created: the joint loop of the collision kernels becomes straight-line
// code.  Results are bit-identical to the generic kernels (same operations, same order).  Code objects are cached in the
// process and on disk ($SMPLX_CACHE_DIR, else $XDG_CACHE_HOME/smpl_amd, else $HOME/.cache/smpl_amd, else /tmp).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <tuple>
#include <utility>

#include "kernels.h"

namespace smplx {

#define X(id, kernel) K_##id,
enum KernelId { SMPLX_PER_ROBOT_KERNELS(X) K_COUNT };
#undef X

// a kernel to launch: the per-robot build (hipFunction_t from the hiprtc module) when present, else the generic
// kernel linked into the library
struct KernelRef {
    hipFunction_t fn = nullptr;
    const void* generic = nullptr;
};

struct KernelSet {
    KernelRef k[K_COUNT];
    bool specialized = false;
};

// generic kernels only
void generic_kernels(KernelSet& ks);

// fills ks with the per-robot kernels for `model` on the current device; on failure returns false with the reason
// in `why` and leaves ks generic.  Thread-safe.  closed_form: the build for spaces that plan with a closed-form
// heuristic instead of the BFS (lattice_steps.h closed_form_of), a code object of its own.
// what the closed-form build's constants header holds behind the model's (the one place that spells it)
static const char* const kClosedFormDefine = "#define CM_CLOSED_FORM 1\n";
bool specialized_kernels(const SmplxModelDev& model, bool closed_form, KernelSet& ks, std::string& why);

// Launch with the kernel's own parameter types: every argument is converted to the declared type first, then
// passed by address (hipModuleLaunchKernel / hipLaunchKernel take untyped argument arrays).
template <typename... P, typename... A, size_t... I>
inline hipError_t launch_impl(const KernelRef& k, dim3 grid, dim3 block, size_t lds, hipStream_t st, std::tuple<P...>& vals,
                              std::index_sequence<I...>)
{
    void* argv[sizeof...(P)] = {(void*)&std::get<I>(vals)...};
    if (k.fn) return hipModuleLaunchKernel(k.fn, grid.x, grid.y, grid.z, block.x, block.y, block.z, (unsigned)lds, st, argv, nullptr);
    return hipLaunchKernel(k.generic, grid, block, argv, lds, st);
}

template <typename... P, typename... A>
inline hipError_t launch(const KernelRef& k, void (*)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t st, A&&... a)
{
    static_assert(sizeof...(P) == sizeof...(A), "argument count does not match the kernel's prototype");
    std::tuple<P...> vals{static_cast<P>(std::forward<A>(a))...};
    return launch_impl<P...>(k, grid, block, lds, st, vals, std::index_sequence_for<P...>{});
}

}  // namespace smplx
