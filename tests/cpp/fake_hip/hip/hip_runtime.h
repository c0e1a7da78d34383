// tests/cpp/fake_hip/hip/hip_runtime.h -- a stand-in for the HIP runtime, for tests/cpp/device_mem_host_driver.cpp: just
// the calls smpl_amd/csrc/device_mem.h makes, on the host heap.  It keeps the set of live handles and an ordered log of
// what was created and destroyed, counts every release of a handle that is not live (a double free), and can be told to
// fail the k-th allocation from now.
#pragma once

#include <cstddef>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorOutOfMemory = 2 };
struct ihipStream_t { int unused; };
struct ihipEvent_t { int unused; };
typedef ihipStream_t* hipStream_t;
typedef ihipEvent_t* hipEvent_t;
enum { hipHostMallocDefault = 0, hipEventDefault = 0, hipEventDisableTiming = 2 };

namespace fake_hip {

struct LogEntry { std::string what; const void* handle; };

inline std::set<const void*>& live() { static std::set<const void*> s; return s; }
inline std::vector<LogEntry>& log() { static std::vector<LogEntry> l; return l; }
inline int& bad_releases() { static int n = 0; return n; }
inline int& fail_in() { static int k = 0; return k; }   // k > 0: the k-th allocation from now fails; 0: none does

inline hipError_t acquire(const char* what, size_t bytes, void** out)
{
    if (fail_in() > 0 && --fail_in() == 0) { log().push_back({std::string(what) + " FAILED", nullptr}); return hipErrorOutOfMemory; }
    *out = std::malloc(bytes ? bytes : 1);
    live().insert(*out);
    log().push_back({what, *out});
    return hipSuccess;
}

inline hipError_t release(const char* what, void* h)
{
    log().push_back({what, h});
    if (!live().erase(h)) { ++bad_releases(); return hipErrorInvalidValue; }
    std::free(h);
    return hipSuccess;
}

}  // namespace fake_hip

inline hipError_t hipMalloc(void** p, size_t bytes) { return fake_hip::acquire("hipMalloc", bytes, p); }
inline hipError_t hipFree(void* p) { return fake_hip::release("hipFree", p); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return fake_hip::acquire("hipHostMalloc", bytes, p); }
inline hipError_t hipHostFree(void* p) { return fake_hip::release("hipHostFree", p); }
inline hipError_t hipStreamCreate(hipStream_t* s) { return fake_hip::acquire("hipStreamCreate", sizeof(ihipStream_t), (void**)s); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return fake_hip::release("hipStreamDestroy", s); }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake_hip::acquire("hipEventCreate", sizeof(ihipEvent_t), (void**)e); }
inline hipError_t hipEventCreate(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDefault); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return fake_hip::release("hipEventDestroy", e); }
