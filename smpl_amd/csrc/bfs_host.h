// smpl_amd/csrc/bfs_host.h -- host driver of the BFS heuristic's distance field (BfsHost in space.h; bfs_kernels.h
// k_bfs_brick_seed / k_bfs_brick_wave): from the goal cell, passes over the queued 8x8x8 bricks until none is queued,
// with launch sizes taken from the queue sizes of the previous goal's run.  run_bfs does it for one space, run_bfs_multi
// for the goals of several spaces in one shared sequence of launches (k_bfs_brick_seed_multi / k_bfs_brick_wave_multi).
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

// The most passes after which a run can still have a brick queued.  A cell d hops from the goal has its final value after
// pass d + 1: its neighbour at d - 1 hops got its own in some pass p <= d, by a visit that either held both cells (a visit
// relaxes its brick to a fixed point) or found that the cell's brick could improve and queued it for pass p + 1, which read
// the neighbour's final value.  Once every cell is final a visit improves nothing and queues nothing, so the bricks queued by
// pass dmax + 1 (dmax: the greatest hop count) are the last: nothing is queued after pass dmax + 2.  A path visits no cell
// twice, so dmax is below the number of cells of the grid.  The count cannot be tied to the bricks alone: a corridor one cell
// wide can cross the face between two bricks once for each of its rows, and a value crosses one face per visit -- a
// serpentine of 300 bricks needs over 2 500 passes.  Beyond the bound a run has failed to converge, which the sweep's monotone
// relaxation rules out; the guard turns a fault of that kind into an error instead of an endless loop.  It is a last resort:
// at 512^3 the bound is 1.3e8 passes, minutes of launches before the error.
inline long long bfs_pass_bound(const smplx_grid* g) { return (long long)g->n[0] * g->n[1] * g->n[2] + 2; }

// the cell of a goal position in the space's grid (BFS_3D::run's argument); false: outside the grid (bfs3d.cpp:169-171)
bool bfs_goal_cell(const smplx_space* s, const double xyz[3], int c[3])
{
    const smplx_grid* g = s->grid;
    for (int a = 0; a < 3; ++a) c[a] = (int)(g->dev.inv_res * (xyz[a] - g->dev.origin_minus_res[a]) + 0.5) - 1;
    return !(c[0] < 0 || c[1] < 0 || c[2] < 0 || c[0] >= g->n[0] || c[1] >= g->n[1] || c[2] >= g->n[2]);
}

// BFS_3D::run to completion on the device (bfs3d.cpp:156-201, 507-547): passes over the queued 8x8x8 bricks until none is
// queued (bfs_kernels.h k_bfs_brick_wave)
int run_bfs(smplx_space* s, const double xyz[3])
{
    int c[3];
    const bool in_bounds = bfs_goal_cell(s, xyz, c);
    // BFS_3D::run's reset (bfs3d.cpp:162-166): the run's tag makes every other run's distances UNDISCOVERED; a pass over
    // the records only when the tags wrap (finish_goal chose the tag and uploaded it)
    if (s->bfs.reset_due) {
        hipLaunchKernelGGL(k_bfs_reset, dim3(2048), dim3(256), 0, s->stream, s->bfs.d_dist, (size_t)s->bfs.ints);
        HIP_TRY(hipGetLastError());
        s->bfs.reset_due = false;
    }
    const int tag_word = s->hs.bfs.tag_word, tag_mask = s->hs.bfs.tag_mask;
    s->bfs.levels = 0;
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
        if ((long long)pass > bfs_pass_bound(s->grid)) return set_error(SMPLX_E_HIP, "BFS did not terminate");
    }
    s->bfs.queue_sizes.assign(cnt.begin() + 3 * kShards * 32, cnt.begin() + 3 * kShards * 32 + std::min(pass, kBfsHistory));
    s->bfs.levels = pass;
    return SMPLX_OK;
}

// run_bfs for the goals of nq spaces at once (smplx_set_goals_*_multi): one seed launch, then passes in which every goal's
// queued bricks are visited side by side (k_bfs_brick_wave_multi: blockIdx.y = goal), on the leading space's stream.  Each
// goal works on its own space's records, lists, counters and queued words under its own tag, so nothing here grows with
// nq x nbricks, and each goal's records reach the fixed point of the label-correcting sweep -- the exact hop counts --
// whatever passes the other goals need.  The caller has checked that the spaces live on one device and have the same
// bricks per axis, and has chosen and uploaded each space's tag.  The sequence ends when a pass found nothing queued for
// any goal; its length is every space's `levels`.
int run_bfs_multi(smplx_space* const* spaces, int nq)
{
    smplx_space* lead = spaces[0];
    hipStream_t stream = lead->stream;
    const int nbx = lead->bfs.bricks[0], nby = lead->bfs.bricks[1], nbz = lead->bfs.bricks[2];
    const int nbricks = nbx * nby * nbz;
    for (int q = 1; q < nq; ++q) HIP_TRY(hipStreamSynchronize(spaces[q]->stream));   // once: their work so far is behind us
    std::vector<SmplxBfsGoalDev> goals((size_t)nq);
    for (int q = 0; q < nq; ++q) {
        smplx_space* s = spaces[q];
        if (s->bfs.reset_due) {     // this space's tags wrapped (run_bfs)
            hipLaunchKernelGGL(k_bfs_reset, dim3(2048), dim3(256), 0, stream, s->bfs.d_dist, (size_t)s->bfs.ints);
            HIP_TRY(hipGetLastError());
            s->bfs.reset_due = false;
        }
        s->bfs.levels = 0;
        SmplxBfsGoalDev& G = goals[q];
        G.dist = s->bfs.d_dist; G.lists = s->bfs.d_queue; G.counts = s->bfs.d_counts; G.queued = s->bfs.d_brick_queued;
        G.tag_word = s->hs.bfs.tag_word; G.tag_mask = s->hs.bfs.tag_mask;
        int c[3];
        const bool in_bounds = bfs_goal_cell(s, s->goal.xyz, c);
        for (int a = 0; a < 3; ++a) G.cell[a] = in_bounds ? c[a] : -1;
        G.pad = 0;
    }
    // per pass {sum, largest} of the goals' queue sizes, and one more slot for a pass beyond the history
    const int n_stats = kBfsHistory + 1;
    if (int e = reserve(lead->bfs.b_goals, (size_t)nq)) return e;
    if (int e = reserve(lead->bfs.b_pass_stats, (size_t)2 * n_stats)) return e;
    const SmplxBfsGoalDev* d_goals = lead->bfs.b_goals.p;
    int32_t* d_stats = lead->bfs.b_pass_stats.p;
    HIP_TRY(hipMemcpyAsync(lead->bfs.b_goals.p, goals.data(), sizeof(SmplxBfsGoalDev) * nq, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_bfs_brick_seed_multi, dim3(nq), dim3(64), 0, stream, d_goals, nq, nbx, nby, nbz, d_stats, n_stats);
    HIP_TRY(hipGetLastError());
    // Launch sizes, as in run_bfs: the x width of a pass is sized by the LARGEST queue any goal had around that pass in the
    // spaces' last runs (the per-pass maxima over their queue_sizes); every block reads its goal's counters even when it has
    // no brick, and here there are nq rows of them, so the floor is lower than for one goal.  Without a plan, or past it:
    // chunks of 16 passes, 4 once fewer than 256 bricks are queued over all goals.
    std::vector<int32_t> plan;
    for (int q = 0; q < nq; ++q) {
        const std::vector<int32_t>& h = spaces[q]->bfs.queue_sizes;
        if (h.size() > plan.size()) plan.resize(h.size(), 0);
        for (size_t k = 0; k < h.size(); ++k) plan[k] = std::max(plan[k], h[k]);
    }
    int planned = 0;
    for (size_t k = 0; k < plan.size(); ++k) if (plan[k] > 0) planned = (int)k + 1;
    const int wave_grid_max = 16384, wave_grid_tail = 2048, wave_grid_min = 64;
    int chunk = planned > 0 ? planned + 2 : 16;
    const bool dbg = getenv("SMPLX_DEBUG_TIMING") != nullptr;
    if (dbg) chunk = 1;
    auto grid_of = [&](int p) {
        if (p >= planned) return wave_grid_tail;
        int m = 0;
        for (int k = std::max(0, p - 1); k <= std::min(planned - 1, p + 1); ++k) m = std::max(m, plan[k]);
        return std::min(wave_grid_max, std::max(wave_grid_min, 2 * m));
    };
    std::vector<int32_t> stats((size_t)2 * n_stats);
    long long pass_bound = 0;     // (the spaces have the same bricks per axis, not necessarily the same cells)
    for (int q = 0; q < nq; ++q) pass_bound = std::max(pass_bound, bfs_pass_bound(spaces[q]->grid));
    int pass = 0;
    while (true) {
        const auto tp0 = std::chrono::steady_clock::now();
        for (int k = 0; k < chunk; ++k, ++pass) {
            // a pass beyond the history keeps no queue sizes; the last of a chunk leaves its totals in the spare slot
            int32_t* slot = pass < kBfsHistory ? d_stats + 2 * pass : (k == chunk - 1 ? d_stats + 2 * kBfsHistory : (int32_t*)nullptr);
            if (pass >= kBfsHistory && slot) HIP_TRY(hipMemsetAsync(slot, 0, 2 * sizeof(int32_t), stream));
            hipLaunchKernelGGL(k_bfs_brick_wave_multi, dim3(std::min(nbricks, grid_of(pass)), nq), dim3(64), 0, stream, d_goals, nbx, nby, nbz, pass,
                               pass < kBfsHistory ? pass : -1, slot);
        }
        HIP_TRY(hipGetLastError());
        const int last = std::min(pass - 1, kBfsHistory);     // the slot of the last pass enqueued
        HIP_TRY(hipMemcpyAsync(stats.data(), d_stats, sizeof(int32_t) * 2 * ((size_t)last + 1), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const long visited = stats[(size_t)2 * last];     // bricks the last pass had queued, over all goals
        if (dbg)
            fprintf(stderr, "[smplx bfs multi] pass %d: %.1f us (launch + sync), %ld bricks queued over %d goals, at most %d for one\n", pass - 1,
                    1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count(), visited, nq, (int)stats[(size_t)2 * last + 1]);
        if (visited == 0) break;      // it queued nothing either: every goal's front has died out
        if (!dbg) chunk = visited < 256 ? 4 : 16;
        if ((long long)pass > pass_bound) return set_error(SMPLX_E_HIP, "BFS did not terminate");
    }
    // the launch-size hint of each space's next run, single or shared: the per-pass maxima of this one
    std::vector<int32_t> sizes((size_t)std::min(pass, kBfsHistory));
    for (size_t k = 0; k < sizes.size(); ++k) sizes[k] = stats[2 * k + 1];
    for (int q = 0; q < nq; ++q) { spaces[q]->bfs.queue_sizes = sizes; spaces[q]->bfs.levels = pass; }
    return SMPLX_OK;
}

}  // namespace
