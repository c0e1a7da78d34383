// tests/cpp/device_mem_host_driver.cpp -- the owners of smpl_amd/csrc/device_mem.h against a stand-in HIP runtime
// (tests/cpp/fake_hip) that keeps the live handles and an ordered log.  Built by tests/test_device_mem.py with the address
// and undefined-behaviour sanitizers and run as a program: exit status 0 and "ok" when every check holds.
#include "../../smpl_amd/csrc/device_mem.h"

#include <cstdio>
#include <type_traits>
#include <utility>

namespace {

int g_failed = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } } while (0)

size_t live() { return fake_hip::live().size(); }
size_t logged() { return fake_hip::log().size(); }
size_t count(const char* what)
{
    size_t n = 0;
    for (const fake_hip::LogEntry& e : fake_hip::log()) n += e.what == what;
    return n;
}

// what a space does: the stream first, buffers and events after it
struct StreamFirst {
    DevStream stream;
    DevPtr<int> a;
    DevBuf<double> b;
    PinBuf<int> pin;
    DevEvent done;
};

template <class Owner, class Raw>
void moves(Owner& a, Raw raw, const char* released)
{
    const size_t before = live();
    Owner b(std::move(a));                      // move construction: exactly one owner
    CHECK((Raw)a == nullptr && (Raw)b == raw && live() == before);
    Owner c;
    c = std::move(b);                           // move assignment into an empty owner
    CHECK((Raw)b == nullptr && (Raw)c == raw && live() == before);
    Owner& same = c;
    c = std::move(same);                        // self-move is harmless
    CHECK((Raw)c == raw && live() == before && count(released) == 0);
    a = std::move(c);
    CHECK((Raw)a == raw && (Raw)c == nullptr && live() == before && count(released) == 0);
}

}  // namespace

int main()
{
    {
        DevPtr<int> p;
        CHECK(p.alloc(10) == hipSuccess && p.p && live() == 1);
        moves(p, p.p, "hipFree");
        int* first = p.p;
        CHECK(p.alloc(20) == hipSuccess && live() == 1);             // alloc on a holder frees first
        CHECK(fake_hip::log()[logged() - 2].what == "hipFree" && fake_hip::log()[logged() - 2].handle == first);
        CHECK(fake_hip::log()[logged() - 1].what == "hipMalloc");
        DevPtr<int> q;
        CHECK(q.alloc(0) == hipSuccess && q.p && live() == 2);       // an empty list still has a block
        q = std::move(p);                                            // move assignment onto a holder frees what it held
        CHECK(live() == 1 && !p.p);
        DevStream s;
        CHECK(s.create() == hipSuccess);
        moves(s, s.h, "hipStreamDestroy");
        DevEvent e;
        CHECK(e.create(hipEventDisableTiming) == hipSuccess);
        moves(e, e.h, "hipEventDestroy");
        hipEvent_t old = e.h;
        CHECK(e.create() == hipSuccess && live() == 3 && !fake_hip::live().count(old));   // create on a holder destroys first
    }
    CHECK(live() == 0 && fake_hip::bad_releases() == 0);
    fake_hip::log().clear();
    {
        DevBuf<double> b;
        CHECK(b.reserve(10) == hipSuccess && b.p && b.cap == 64 && live() == 1);   // at least 64 entries
        double* first = b.p;
        size_t n = logged();
        CHECK(b.reserve(64) == hipSuccess && b.p == first && logged() == n);      // it fits: nothing happens
        CHECK(b.reserve(100) == hipSuccess && b.cap == 100 && live() == 1);        // it grows: the old block is freed, once
        CHECK(count("hipFree") == 1 && fake_hip::log()[n].what == "hipFree" && fake_hip::log()[n].handle == first);
        fake_hip::fail_in() = 1;
        CHECK(b.reserve(1000) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && live() == 0);   // a failed reserve leaves it empty
        CHECK(b.reserve(8) == hipSuccess && b.cap == 64 && live() == 1);          // ... and usable
        DevBuf<double> c(std::move(b));
        CHECK(!b.p && c.p && live() == 1);

        PinBuf<int> pin;
        CHECK(pin.reserve(1) == hipSuccess && pin.cap == 64 && live() == 2);
        int* pfirst = pin.p;
        n = logged();
        CHECK(pin.reserve(64) == hipSuccess && pin.p == pfirst && logged() == n);
        CHECK(pin.reserve(65) == hipSuccess && pin.cap == 65 && live() == 2 && count("hipHostFree") == 1);
        fake_hip::fail_in() = 1;
        CHECK(pin.reserve(1000) == hipErrorOutOfMemory && pin.p == nullptr && pin.cap == 0 && live() == 1);
        CHECK(pin.reserve(2) == hipSuccess);
        static_assert(!std::is_copy_constructible<PinBuf<int>>::value && !std::is_copy_constructible<DevBuf<int>>::value, "one owner");

        WorkSpace w;
        const size_t sizes[2] = {100, 300};
        size_t at[2];
        CHECK(w.carve(sizes, at) == hipSuccess && at[0] == 0 && at[1] == 256 && w.bytes == 768 && live() == 3);
        fake_hip::fail_in() = 1;
        const size_t more[1] = {4096};
        size_t at1[1];
        CHECK(w.carve(more, at1) == hipErrorOutOfMemory && w.bytes == 0 && live() == 2);
    }
    CHECK(live() == 0 && fake_hip::bad_releases() == 0);
    fake_hip::log().clear();
    {
        StreamFirst s;
        CHECK(s.stream.create() == hipSuccess && s.a.alloc(4) == hipSuccess && s.b.reserve(4) == hipSuccess && s.pin.reserve(4) == hipSuccess);
        CHECK(s.done.create(hipEventDisableTiming) == hipSuccess && live() == 5);
    }
    // members die in reverse order: the stream that was declared first is destroyed last
    CHECK(logged() == 10 && fake_hip::log().back().what == "hipStreamDestroy" && count("hipStreamDestroy") == 1);
    CHECK(fake_hip::log()[5].what == "hipEventDestroy" && count("hipFree") == 2 && count("hipHostFree") == 1);
    CHECK(live() == 0 && fake_hip::bad_releases() == 0);
    if (g_failed == 0) std::printf("ok\n");
    return g_failed ? 1 : 0;
}
