// tests/cpp/path_multi_host_driver.cpp -- the arithmetic of smplx_post_process_paths over the caller's offsets
// (smpl_amd/csrc/path_multi.h, the part in front of its HIP code) compiled by the host compiler: the offset validation, the
// output offsets with their 32-bit guard, the size bound and the block table of k_paths_valid.  Built by
// tests/test_post_process_multi_abi.py with the address and undefined-behaviour sanitizers; prints "ok".
#include <climits>
#include <cstdio>
#include <vector>

#define SMPLX_PATH_MULTI_ARITHMETIC_ONLY
#include "../../smpl_amd/csrc/path_multi.h"

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main()
{
    using namespace smplx_path_multi;
    long long total = -1;
    {   // well-formed offsets: empty paths, one path, the largest offset an int32 holds
        const int32_t a[] = {0, 0, 3, 3, 10};
        CHECK(check_offsets(a, 4, &total) && total == 10);
        const int32_t one[] = {0};
        CHECK(check_offsets(one, 0, &total) && total == 0);
        const int32_t big[] = {0, INT_MAX - 1, INT_MAX};
        CHECK(check_offsets(big, 2, &total) && total == INT_MAX);
        CHECK(check_offsets(a, 4, nullptr));
    }
    {   // malformed ones: decreasing, first[0] != 0, null, nq < 0; `total` keeps its value
        total = 77;
        const int32_t dec[] = {0, 5, 4, 9};
        CHECK(!check_offsets(dec, 3, &total));
        const int32_t neg[] = {0, -1, 4};
        CHECK(!check_offsets(neg, 2, &total));
        const int32_t off[] = {1, 2, 3};
        CHECK(!check_offsets(off, 2, &total));
        const int32_t wrap[] = {0, INT_MAX, INT_MIN, 5};      // what a sum past INT_MAX looks like in int32 offsets
        CHECK(!check_offsets(wrap, 3, &total));
        CHECK(!check_offsets(nullptr, 1, &total));
        CHECK(!check_offsets(dec, -1, &total));
        CHECK(total == 77);
    }
    {   // output offsets: sums up to INT_MAX fit, one more does not and nothing is written
        std::vector<int32_t> of(4, -7);
        const long long c[] = {4, 0, 9};
        CHECK(output_offsets(c, 3, of.data()) && of[0] == 0 && of[1] == 4 && of[2] == 4 && of[3] == 13);
        const long long edge[] = {INT_MAX - 5, 5, 0};
        CHECK(output_offsets(edge, 3, of.data()) && of[3] == INT_MAX);
        std::vector<int32_t> keep(4, -7);
        const long long over[] = {INT_MAX - 5, 5, 1};
        CHECK(!output_offsets(over, 3, keep.data()));
        const long long huge[] = {(long long)INT_MAX + 1, 0, 0};
        CHECK(!output_offsets(huge, 3, keep.data()));
        const long long sums[] = {INT_MAX, INT_MAX, INT_MAX};
        CHECK(!output_offsets(sums, 3, keep.data()));
        const long long minus[] = {3, -1, 2};
        CHECK(!output_offsets(minus, 3, keep.data()));
        for (int32_t v : keep) CHECK(v == -7);
    }
    {   // the size bound, in 64 bits
        CHECK(last_pass_bound(0, 0) == 0 && last_pass_bound(10, 3) == 23);
        CHECK(last_pass_bound(INT_MAX, INT_MAX) == 3ll * INT_MAX);
    }
    {   // the block table: a path's rows in blocks of their own, the last one short; no rows, no block
        std::vector<int32_t> b;
        append_blocks(b, 0, 0, 0, 128);
        CHECK(b.empty());
        append_blocks(b, 2, 10, 128, 128);
        CHECK(b.size() == 3 && b[0] == 2 && b[1] == 10 && b[2] == 128);
        append_blocks(b, 3, 138, 129, 128);
        CHECK(b.size() == 9 && b[3] == 3 && b[4] == 138 && b[5] == 128 && b[6] == 3 && b[7] == 266 && b[8] == 1);
        long long rows = 0;
        for (size_t i = 0; i < b.size(); i += 3) { CHECK(b[i + 2] >= 1 && b[i + 2] <= 128); rows += b[i + 2]; }
        CHECK(rows == 257);
    }
    std::printf("ok\n");
    return 0;
}
