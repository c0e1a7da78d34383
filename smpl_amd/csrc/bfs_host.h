// smpl_amd/csrc/bfs_host.h -- host driver of the BFS heuristic's distance field (BfsHost in space.h; kernels.hip
// k_bfs_brick_seed / k_bfs_brick_wave): from the goal cell, passes over the queued 8x8x8 bricks until none is queued,
// with launch sizes taken from the queue sizes of the previous goal's run.
#pragma once

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels.h"
#include "space.h"
#ifdef SMPLX_BFS_TRACE
extern __device__ long long g_bfs_trace[16];
#endif

namespace {

constexpr int kBfsHistory = 2048;   // passes whose queue sizes are kept behind the counters (d_counts)

// BFS_3D::run to completion on the device (bfs3d.cpp:156-201, 507-547): passes over the queued 8x8x8 bricks until none is
// queued (kernels.hip k_bfs_brick_wave)
int run_bfs(smplx_space* s, const double xyz[3])
{
    const smplx_grid* g = s->grid;
    int c[3];
    for (int a = 0; a < 3; ++a) c[a] = (int)(g->dev.inv_res * (xyz[a] - g->dev.origin_minus_res[a]) + 0.5) - 1;
    // BFS_3D::run's reset (bfs3d.cpp:162-166): the run's tag makes every other run's distances UNDISCOVERED; a pass over
    // the records only when the tags wrap (finish_goal chose the tag and uploaded it)
    if (s->bfs.reset_due) {
        hipLaunchKernelGGL(k_bfs_reset, dim3(2048), dim3(256), 0, s->stream, s->bfs.d_dist, (size_t)s->bfs.ints);
        HIP_TRY(hipGetLastError());
        s->bfs.reset_due = false;
    }
    const int tag_word = s->hs.bfs.tag_word, tag_mask = s->hs.bfs.tag_mask;
    s->bfs.levels = 0;
    const bool in_bounds = !(c[0] < 0 || c[1] < 0 || c[2] < 0 || c[0] >= g->n[0] || c[1] >= g->n[1] || c[2] >= g->n[2]);
    if (!in_bounds) {   // bfs3d.cpp:169-171: nothing is labelled
        HIP_TRY(hipStreamSynchronize(s->stream));
        return SMPLX_OK;
    }
    const int nbx = s->bfs.bricks[0], nby = s->bfs.bricks[1], nbz = s->bfs.bricks[2];
    const int nbricks = nbx * nby * nbz;
    // two brick lists alternate, each cut into 16 sub-lists of nbricks entries with their own counters on separate
    // lines: d_queue holds the lists, d_counts the 3 x 16 counters (in / next / zeroed for the pass after)
    const int kShards = 16;
    const size_t list_ints = (size_t)kShards * nbricks;
    int32_t* lists = s->bfs.d_queue;
    hipLaunchKernelGGL(k_bfs_brick_seed, dim3(1), dim3(64), 0, s->stream, s->bfs.d_dist, c[0], c[1], c[2], nbx, nby, nbz, lists, s->bfs.d_counts, tag_word);
    HIP_TRY(hipGetLastError());
    int pass = 0;
    std::vector<int32_t> cnt(3 * kShards * 32 + kBfsHistory);
    int32_t* queued[2] = {s->bfs.d_brick_queued, s->bfs.d_brick_queued + nbricks};
    int32_t* d_history = s->bfs.d_counts + 3 * kShards * 32;
    // Launch sizes.  Every block of a launch reads the counters even when it has no brick (16 384 mostly idle blocks cost
    // ~6 us, 2 048 ~2.4 us), and every look at the counters from the host costs ~40 us (copy, synchronise, the stream
    // running dry).  The passes of two goals in one grid are much alike, so the queue sizes of the last BFS (kept by
    // the kernel behind the counters) size this one: all its passes plus two are enqueued at once, each with twice
    // the blocks its neighbourhood of passes had bricks, and the one look at the end usually finds nothing queued.  A first BFS
    // -- or one that outlives the plan -- goes in chunks: 16 passes while the front is wide, 4 once fewer than 256 bricks
    // are queued (the tail is a narrow front: a chunk of 16 wasted eight passes on average).
    const std::vector<int32_t> plan = s->bfs.queue_sizes;
    int planned = 0;
    for (size_t k = 0; k < plan.size(); ++k) if (plan[k] > 0) planned = (int)k + 1;
    const int wave_grid_max = 16384;
    int wave_grid = planned > 0 ? 2048 : wave_grid_max;    // (past the plan: its tail)
    int chunk = planned > 0 ? planned + 2 : 16;
    const bool dbg = getenv("SMPLX_DEBUG_TIMING") != nullptr;
    if (dbg) chunk = 1;     // one look at the counters per pass: bricks and microseconds of every pass on stderr
    auto grid_of = [&](int p) {
        if (p >= planned) return wave_grid;
        int m = 0;
        for (int k = std::max(0, p - 1); k <= std::min(planned - 1, p + 1); ++k) m = std::max(m, plan[k]);
        return std::min(wave_grid_max, std::max(1024, 2 * m));
    };
    while (true) {
        const auto tp0 = std::chrono::steady_clock::now();
        for (int k = 0; k < chunk; ++k, ++pass) {
            const int in = pass & 1, out = (pass + 1) & 1;
            const int c_in = pass % 3, c_next = (pass + 1) % 3, c_after = (pass + 2) % 3;
            hipLaunchKernelGGL(k_bfs_brick_wave, dim3(std::min(nbricks, grid_of(pass))), dim3(64), 0, s->stream, s->bfs.d_dist, nbx, nby, nbz,
                               lists + in * list_ints, s->bfs.d_counts + c_in * kShards * 32, lists + out * list_ints,
                               s->bfs.d_counts + c_next * kShards * 32, s->bfs.d_counts + c_after * kShards * 32, nbricks,
                               queued[in], queued[out], pass < kBfsHistory ? d_history + pass : (int32_t*)nullptr, tag_word, tag_mask);
        }
        HIP_TRY(hipGetLastError());
        const size_t look = 3 * kShards * 32 + (size_t)std::min(pass, kBfsHistory);
        HIP_TRY(hipMemcpyAsync(cnt.data(), s->bfs.d_counts, sizeof(int32_t) * look, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        long pending = 0;
        const int set = pass % 3;   // the "in" counters of the pass that would come next
        for (int k = 0; k < kShards; ++k) pending += cnt[(size_t)set * kShards * 32 + 32 * k];
        if (dbg) {
            fprintf(stderr, "[smplx bfs] pass %d: %.1f us (launch + sync), %ld bricks queued for the next\n", pass - 1,
                    1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count(), pending);
#ifdef SMPLX_BFS_TRACE
            {
                long long tr[16], zero[16] = {0};
                if (hipMemcpyFromSymbol(tr, HIP_SYMBOL(g_bfs_trace), sizeof(tr)) == hipSuccess && tr[7] > 0) {
                    static const char* names[7] = {"", "list", "tile load", "sweeps", "stores", "requeue test", "claim"};
                    fprintf(stderr, "[smplx bfs]   %lld visits, longest / mean (us):", tr[7]);
                    for (int k = 1; k < 7; ++k) fprintf(stderr, " %s %.2f / %.2f%s", names[k], 0.01 * tr[k], 0.01 * tr[8 + k] / tr[7], k < 6 ? "," : "\n");
                }
                (void)hipMemcpyToSymbol(HIP_SYMBOL(g_bfs_trace), zero, sizeof(zero));
            }
#endif
        }
        if (pending == 0) break;
        if (!dbg) chunk = pending < 256 ? 4 : 16;
        wave_grid = pending < 256 ? std::min(wave_grid_max, 2048) : wave_grid_max;
        // (a label-correcting brick sweep can legitimately need on the order of nbricks passes on maze-like free space)
        if (pass > 4 * nbricks + 1024) return set_error(SMPLX_E_HIP, "BFS did not terminate");
    }
    s->bfs.queue_sizes.assign(cnt.begin() + 3 * kShards * 32, cnt.begin() + 3 * kShards * 32 + std::min(pass, kBfsHistory));
    s->bfs.levels = pass;
    return SMPLX_OK;
}

}  // namespace
