// smpl_amd/csrc/host_core.h -- what every part of the host engine (engine.hip and the headers it is made of) stands on:
// the thread's error text behind smplx_last_error(), the HIP_TRY / KLAUNCH early returns, the error code of a failed
// allocation (device_mem.h, which has the owners of everything the host holds on the device), the input guard of the
// entry points, and the two rounding helpers of every size computation.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>

#include "../../include/smpl_amd.h"
#include "device_mem.h"
#include "specialize.h"

namespace {

thread_local std::string g_error;

int set_error(int code, const std::string& msg)
{
    g_error = msg;
    return code;
}

int hip_status(hipError_t e, const char* what)
{
    return e == hipSuccess ? SMPLX_OK : set_error(SMPLX_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

// room for n entries in a DevBuf or a PinBuf (device_mem.h), as an SMPLX code
template <class Buf>
int reserve(Buf& b, size_t n) { return hip_status(b.reserve(n), "buffer allocation"); }

// input guard of the entry points that take joint values from the caller: a non-finite or absurd value would make the
// limit folding of KDLRobotModel::checkJointLimits (a -= 2*pi until in range) spin forever on the device
bool sane_values(const double* q, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!(q[i] > -1.0e6 && q[i] < 1.0e6)) return false;
    return true;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return set_error(SMPLX_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// launch of a model-dependent kernel: the per-robot build when the space has one (specialize.h)
#define KLAUNCH(space, ID, kern, grid, block, lds, stream, ...)                                                   \
    do {                                                                                                          \
        hipError_t le_ = smplx::launch((space)->ks.k[smplx::ID], kern, grid, block, lds, stream, __VA_ARGS__);   \
        if (le_ != hipSuccess) return set_error(SMPLX_E_HIP, std::string(#kern) + ": " + hipGetErrorString(le_)); \
    } while (0)

inline int blocks_for(long long n, int block) { return (int)((n + block - 1) / block); }

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

}  // namespace
