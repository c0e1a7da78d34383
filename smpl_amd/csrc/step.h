// smpl_amd/csrc/step.h -- one expansion step on the GPU and what the host does around it.  The scratch layout
// (carve_work), the one rule for which kernels a launch takes (expand_path) and the launch itself (launch_expand);
// frontier batches -- the `inflight` states of one or many spaces packed, enqueued (issue_frontier) and ingested into
// the successor cache when they land (collect_batch, ingest_row); and GetSuccs on top of them (get_succs), which
// commits cached successors to state ids in the caller's sequential order.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <utility>
#include <vector>

#include "device_table.h"
#include "kernels.h"
#include "space.h"

namespace {

// per-block tallies: 4 uint64 per block of the (state x primitive) grid (step_kernels.h tally_block)
inline size_t counter_words(int B, int M) { return (size_t)blocks_for((long long)B * M, SMPLX_BLOCK) * SMPLX_TALLIES; }

// carve of the per-batch device scratch: the one statement of its layout (from a null base it only measures: .bytes)
struct ExpandWork {
    double* goal_dist;
    int32_t* state_lookups;
    unsigned char* state_bad;
    int32_t* edge_w;
    int32_t* edge_lookups;
    unsigned char* edge_bad;
    unsigned long long* succ_eval;   // successor role of k_pipe_configs: heuristic | table id << 32, per edge
    unsigned char* succ_goal;        // ... its goal bit
    int32_t* succ_coord;             // ... and its coordinates (out_coord is written by k_pipe_finish, for valid edges only)
    int32_t* work_count;        // NOT in the caller's scratch: the stream's counter set (StepLaunch::work_counters)
    unsigned long long* work;   // 64-bit items: edge | waypoint << 32 | waypoint count << 48
    int capacity;
    double* trig;               // per state: sines and cosines of its joint values, 4 N doubles (sphere_checks.h parent_trig)
    size_t bytes;               // of the whole scratch (smplx_expand_work_bytes)
};

ExpandWork carve_work(void* base, int B, int M, int N)
{
    unsigned char* w = (unsigned char*)base;
    const size_t b = (size_t)B, bm = (size_t)B * M;
    size_t o = 0;
    ExpandWork k;
    k.goal_dist = (double*)(w + o); o += align256(b * 8);
    k.state_lookups = (int32_t*)(w + o); o += align256(b * 4);
    k.state_bad = w + o; o += align256(b);
    k.edge_w = (int32_t*)(w + o); o += align256(bm * 4);
    k.edge_lookups = (int32_t*)(w + o); o += align256(bm * 4);
    k.edge_bad = w + o; o += align256(bm);
    k.succ_eval = (unsigned long long*)(w + o); o += align256(bm * 8);
    k.succ_goal = w + o; o += align256(bm);
    k.succ_coord = (int32_t*)(w + o); o += align256(bm * N * 4);
    k.work_count = nullptr; o += 2048;       // (where the counters used to live: the size callers allocate stays what it was)
    k.work = (unsigned long long*)(w + o); o += align256(bm * 16 * 8);
    k.capacity = (int)std::min<size_t>(bm * 16, (size_t)1 << 30) / 8 * 8;
    k.trig = (double*)(w + o); o += align256(b * 4 * N * 8);
    k.bytes = o;
    return k;
}

inline size_t expand_work_bytes(int B, int M, int N) { return carve_work(nullptr, B, M, N).bytes; }

// optional K5 outputs of an expansion launch
struct K5Out {
    int32_t* d_id = nullptr;                 // dense [B][M] ids (-1 = unknown)
    const SmplxCompactDev* cmp = nullptr;    // compact stream (device pointers), or null
    const int32_t* items = nullptr;          // states to insert at the head of the batch's first kernel: n_items x (N + 2)
    int n_items = 0;                         //   int32 (device memory, or pinned host memory for the zero-copy launch)
};

// The pending inserts of a batch travel in the same upload as its parents: they sit behind the B x N doubles of the
// pinned parent buffer.  Returns the doubles the items occupy; *items_at = their offset in doubles.
size_t stage_items(PinBuf<double>& p_q, size_t parent_doubles, const std::vector<int32_t>& items)
{
    if (items.empty()) return 0;
    std::memcpy((void*)(p_q.p + parent_doubles), items.data(), items.size() * sizeof(int32_t));
    return (items.size() + 1) / 2;
}

// pinned host buffers of a zero-copy small batch: the kernel reads the parents from, and also writes the results to, host
// memory (a few KB of PCIe traffic instead of DMA copies with their fixed latency)
struct ZeroCopy {
    const double* q = nullptr;
    unsigned char* flags = nullptr;
    int32_t* coord = nullptr;
    double* sq = nullptr;
    int32_t* h = nullptr;
    int32_t* id = nullptr;
};

// arguments of one expansion launch
struct ExpandArgs {
    const double* q = nullptr;                  // B x N parents (device)
    int B = 0;
    unsigned char* flags = nullptr;             // dense [B][M] outputs (device)
    int32_t* coord = nullptr;
    double* sq = nullptr;
    int32_t* h = nullptr;
    int32_t* cost = nullptr;
    int32_t* lookups = nullptr;
    void* work = nullptr;                       // expand_work_bytes(B, M, N)
    unsigned long long* counters = nullptr;     // per-block tallies, or null
    hipStream_t stream = nullptr;
    const SmplxSpaceDev* const* stab = nullptr; // cross-query batch: query table ...
    const unsigned short* state_q = nullptr;    // ... and per-row query index
    const ZeroCopy* zero_copy = nullptr;        // pinned host parents and outputs (the zero-copy single launch)
    const K5Out* k5 = nullptr;
    bool force_pipeline = false;                // no single launch with copies
};

enum class ExpandPath { SmallZeroCopy, Small, Fused, Pipeline, OneLaunch };

inline size_t small_lds_bytes(const smplx_space* s)
{
    return smplx_lds_bytes_n(s->blob_bytes, s->lds_nroot, s->model.dev.nslots, s->model.dev.nvars, s->model.dev.stack_bytes,
                             smplx_small_block(s->M));
}

// The one rule for how an expansion launch runs.  What differs between callers comes in explicitly: zero_copy_max, the
// largest batch whose parents and results may stay in pinned host memory (0: never), and force_pipeline, which rules out
// the single launch with copies.  Armed profile events rule out the zero-copy launch, an event triple left for this
// launch the single launch altogether; the fused mode takes precedence over the pipeline.
// A pipeline step runs as the one launch k_step_block (step_block.h) when the space runs per-robot kernels, neither
// pipeline test hook is set, no event triple is armed for this launch (the triple brackets k_pipe_configs) and its blocks
// are resident in one round (step_block_resident) with four blocks sharing a CU (three waves per SIMD: the geometry it was
// measured at -- arm7; dual14 keeps two blocks a CU, the mixed-kinds robot one, neither was timed and both stay on the
// pipeline); beyond one round the step is bound by throughput and the pipeline stays, as three_launch_blocks decides for
// its goal-distance wave.  The generic k_step_block has not been measured against the
// generic pipeline (its k_pipe_configs allows two waves per SIMD, so a batch of the benchmark's size is not resident).
// StepLaunch::one_launch (test hook): 0 never, 1 whenever the kernel can run at all, resident and per-robot or not.
ExpandPath expand_path(const smplx_space* s, int B, int zero_copy_max, bool force_pipeline)
{
    const bool small = !s->step.fused_mode && B <= s->small.batch_max && smplx_small_block(s->M) <= 512 &&
                       small_lds_bytes(s) <= 150 * 1024 && s->step.work_list_items == 0 && s->small.pipeline_left == 0 &&
                       s->step.prof_used + 3 > s->step.prof_events.size();
    if (small && B <= zero_copy_max && s->step.prof_events.empty()) return ExpandPath::SmallZeroCopy;
    if (small && !force_pipeline) return ExpandPath::Small;
    if (s->step.fused_mode) return ExpandPath::Fused;
    // (smplx_step_claim_fits: the packed claim words of k_step_block hold a shard's blocks and records; a grid beyond that --
    // a million blocks, never a resident one -- keeps the pipeline)
    const bool can_run = s->step.one_launch_blocks > 0 && !s->step.pipe_prep && s->step.work_list_items == 0 &&
                         s->step.prof_used + 3 > s->step.prof_events.size() &&
                         smplx_step_claim_fits(blocks_for((long long)B * s->M, SMPLX_BLOCK));
    const bool by_rule = s->ks.specialized && s->step.one_launch_per_cu >= 4 &&
                         blocks_for((long long)B * s->M, SMPLX_BLOCK) <= s->step.one_launch_blocks;
    if (can_run && s->step.one_launch != 0 && (s->step.one_launch == 1 || by_rule)) return ExpandPath::OneLaunch;
    return ExpandPath::Pipeline;
}

// Blocks of k_step_block that are resident at once: the occupancy of the kernel this space would launch, at its block
// size and dynamic LDS, times the CU count.  0: the kernel cannot run for this space (a block would hold the edges of more
// than SMPLX_STEP_STATES states, or does not fit a CU).  Asked once, when the space is created.
int step_block_resident(const smplx_space* s, size_t lds, int* blocks_per_cu)
{
    *blocks_per_cu = 0;
    if (smplx_step_states(s->M) > SMPLX_STEP_STATES) return 0;
    int per_cu = 0, cus = 0;
    const smplx::KernelRef& k = s->ks.k[smplx::K_STEP_BLOCK];
    const hipError_t e = k.fn ? hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, SMPLX_STEP_BLOCK, lds)
                              : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.generic, SMPLX_STEP_BLOCK, lds);
    if (e != hipSuccess) { (void)hipGetLastError(); return 0; }
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || cus <= 0) cus = 256;
    *blocks_per_cu = per_cu > 0 ? per_cu : 0;
    return per_cu > 0 ? per_cu * cus : 0;
}

// the step counters of `stream` (StepLaunch::WorkCounters): allocated and zeroed, once and synchronously, the first time the stream is seen
int work_counters_for(smplx_space* s, hipStream_t stream, StepLaunch::WorkCounters** out)
{
    for (StepLaunch::WorkCounters& w : s->step.work_counters)
        if (w.stream == stream) { *out = &w; return SMPLX_OK; }
    DevPtr<int32_t> p;
    HIP_TRY(p.alloc(SMPLX_WORK_COUNTER_BYTES / sizeof(int32_t)));
    hipError_t e = hipMemsetAsync(p, 0, SMPLX_WORK_COUNTER_BYTES, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (int c = hip_status(e, "work-list counters")) return c;
    s->step.work_counters.push_back({stream, std::move(p), false});
    *out = &s->step.work_counters.back();
    return SMPLX_OK;
}

int launch_expand(smplx_space* s, const ExpandArgs& a)
{
    const int B = a.B;
    ExpandWork k = carve_work(a.work, B, s->M, s->N);
    int32_t* d_id = a.k5 ? a.k5->d_id : nullptr;
    SmplxCompactDev cmp;
    std::memset(&cmp, 0, sizeof(cmp));
    if (a.k5 && a.k5->cmp) cmp = *a.k5->cmp;
    // (the compact stream is produced by k_pipe_finish or k_step_block: no single small launch when it is asked for)
    const ExpandPath path = expand_path(s, B, a.zero_copy ? B : 0, a.force_pipeline || cmp.rec_a);
    if (s->step.one_launch == 1 && path == ExpandPath::Pipeline)
        return set_error(SMPLX_E_ARG, "the one-launch step was asked for (smplx_test_set_one_launch) but cannot run: a pipeline test hook or a "
                                      "profile-event triple is set, a block of k_step_block does not fit this model, or the grid is beyond "
                                      "what its claim words count");
    const int32_t* ins_items = a.k5 && s->dt.d_table ? a.k5->items : nullptr;
    const int n_ins = ins_items ? a.k5->n_items : 0;
    if (s->step.work_list_items > 0) k.capacity = s->step.work_list_items;   // test hook: almost every edge overflows into the deferred pass
    DevEvent* ev = nullptr;
    if (s->step.prof_used + 3 <= s->step.prof_events.size()) { ev = &s->step.prof_events[s->step.prof_used]; s->step.prof_used += 3; }
    const int bs = blocks_for(B, SMPLX_BLOCK);
    const int be = blocks_for((long long)B * s->M, SMPLX_BLOCK);
    if (path == ExpandPath::SmallZeroCopy || path == ExpandPath::Small) {
        ++s->small.small_launches;
        // a handful of states: ONE launch, all FK chains side by side (small_batch.h k_small_batch)
        // zero_copy: parents are read from, and results also written to, that space's pinned host buffers
        const ZeroCopy* zc = path == ExpandPath::SmallZeroCopy ? a.zero_copy : nullptr;
        const int small_block = smplx_small_block(s->M);
        KLAUNCH(s, K_SMALL_BATCH, k_small_batch, dim3(B + blocks_for(n_ins, small_block)), dim3(small_block), small_lds_bytes(s), a.stream, s->d_space,
                           zc ? zc->q : a.q, B, k.goal_dist,
                           k.state_bad, k.state_lookups, a.flags, a.coord, a.sq, a.h, a.cost, a.lookups, a.stab, a.state_q,
                           zc ? zc->flags : (unsigned char*)nullptr, zc ? zc->coord : (int32_t*)nullptr,
                           zc ? zc->sq : (double*)nullptr, zc ? zc->h : (int32_t*)nullptr, d_id,
                           zc ? zc->id : (int32_t*)nullptr, ins_items, n_ins);
    } else if (path == ExpandPath::Fused) {
        // one thread walks a whole edge: exact reference early-exit order (and lookup tallies)
        if (d_id) HIP_TRY(hipMemsetAsync(d_id, 0xFF, sizeof(int32_t) * (size_t)B * s->M, a.stream));   // fused mode: no table lookups
        if (n_ins > 0) {
            hipLaunchKernelGGL(k_table_insert, dim3(blocks_for(n_ins, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), 0, a.stream, s->d_space, a.stab, ins_items, n_ins, s->N);
        }
        if (ev) (void)hipEventRecord(ev[0], a.stream);
        KLAUNCH(s, K_STATE_PREP, k_state_prep, dim3(bs), dim3(SMPLX_BLOCK), s->lds_bytes, a.stream, s->d_space, a.q, B,
                           k.goal_dist, k.state_bad, k.state_lookups, a.stab, a.state_q);
        if (ev) (void)hipEventRecord(ev[1], a.stream);
        KLAUNCH(s, K_EXPAND, k_expand, dim3(be), dim3(SMPLX_BLOCK), s->lds_bytes, a.stream, s->d_space, a.q, B,
                           k.goal_dist, k.state_bad, k.state_lookups, a.flags, a.coord, a.sq, a.h, a.cost, a.lookups,
                           a.counters, (const int*)nullptr, a.stab, a.state_q);
        if (ev) (void)hipEventRecord(ev[2], a.stream);
    } else if (path == ExpandPath::OneLaunch) {
        // the whole step in one launch (step_block.h): block b owns the edges block b of k_pipe_finish owns
        ++s->small.pipe_launches;
        StepLaunch::WorkCounters* wc = nullptr;
        if (int e = work_counters_for(s, a.stream, &wc)) return e;
        if (wc->dirty) HIP_TRY(hipMemsetAsync(wc->p, 0, SMPLX_WORK_COUNTER_BYTES, a.stream));
        wc->dirty = true;   // until the launch is in the stream: its last block leaves the set zeroed
        // K5 inserts: the table must be complete before the same launch probes it
        if (n_ins > 0) {
            hipLaunchKernelGGL(k_table_insert, dim3(blocks_for(n_ins, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), 0, a.stream, s->d_space, a.stab, ins_items, n_ins, s->N);
        }
        const unsigned char* blob = reinterpret_cast<const unsigned char*>(s->d_space.p) + offsetof(SmplxSpaceDev, model_blob);
        KLAUNCH(s, K_STEP_BLOCK, k_step_block, dim3(be), dim3(SMPLX_STEP_BLOCK), s->step.one_launch_lds, a.stream, s->d_space, a.q, B,
                           a.flags, a.coord, a.sq, a.h, a.cost, a.lookups, a.counters, a.stab, a.state_q, d_id, cmp, wc->p,
                           s->M, s->N, blob, (int)s->blob_bytes);
        wc->dirty = false;
        ++s->step.one_launch_steps;
    } else {
        const size_t lm = s->blob_bytes;
        ++s->small.pipe_launches;
        StepLaunch::WorkCounters* wc = nullptr;
        if (int e = work_counters_for(s, a.stream, &wc)) return e;
        if (wc->dirty) HIP_TRY(hipMemsetAsync(wc->p, 0, SMPLX_WORK_COUNTER_BYTES, a.stream));
        wc->dirty = true;   // until the whole sequence is in the stream: k_pipe_finish leaves the set zeroed
        k.work_count = wc->p;
        // Every kernel of the step takes nprims (s->M) and nvars (s->N) as arguments: a thread's state index is tid / nprims,
        // and with the divisor in the kernel's arguments its first indexed load does not wait for one from the space record
        // (a cross-query batch uses the lead space's actions for every row: one value per launch).
        // Three launches.  k_pipe_setup computes the goal distance of the states of each block itself and carries the K5
        // inserts in extra blocks.  With the test hook, k_pipe_prep does both in a launch of its own, as the step used to.
        // So it does for a batch whose setup blocks (3 waves each) no longer fit the chip at 4 waves per SIMD in one
        // round: there the step is bound by throughput, not by the length of the chain, and the goal-distance wave of
        // every block (one chain per state and block, 50 % more waves) costs more than the launch saves -- measured
        // at B = 16 384 and 65 536.
        if (s->step.three_launch_blocks == 0) {
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device) != hipSuccess || cus <= 0) cus = 256;
            s->step.three_launch_blocks = cus * 4 * 4 / (SMPLX_SETUP_BLOCK / 64);
        }
        const bool pipe_prep = s->step.pipe_prep || be > s->step.three_launch_blocks;
        if (pipe_prep)
            KLAUNCH(s, K_PIPE_PREP, k_pipe_prep, dim3(bs + blocks_for(n_ins, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), lm, a.stream, s->d_space, a.q, B,
                               k.goal_dist, k.work_count, a.stab, a.state_q, cmp.totals, ins_items, n_ins, k.trig);
        const int n_ins_setup = pipe_prep ? 0 : n_ins;
        KLAUNCH(s, K_PIPE_SETUP, k_pipe_setup, dim3(be + blocks_for(n_ins_setup, SMPLX_BLOCK)), dim3(pipe_prep ? SMPLX_BLOCK : SMPLX_SETUP_BLOCK), lm, a.stream, s->d_space, a.q, B,
                           k.goal_dist, a.flags, a.sq, k.edge_w, k.edge_lookups, k.edge_bad, k.state_lookups, k.state_bad,
                           k.work, k.work_count, k.capacity, a.stab, a.state_q, pipe_prep ? 1 : 0, cmp.totals, ins_items, n_ins_setup,
                           s->M, s->N, k.trig);
        if (ev) (void)hipEventRecord(ev[0], a.stream);
        // (a smaller grid was tried -- idle blocks cost next to nothing: 22.0 us at 3 configurations per edge, 21.7 at 1.35)
        // behind the bc collision blocks: one successor thread per edge (dense: it leaves at once where setup's flag is not 0)
        const int bc = blocks_for((long long)B + (long long)B * s->M * 3, SMPLX_BLOCK);
        // the model image (inside the space record) and its size go to the collision blocks as arguments: their copy of
        // it starts beside the shard counters, not behind a load of the header's size field
        const unsigned char* blob = reinterpret_cast<const unsigned char*>(s->d_space.p) + offsetof(SmplxSpaceDev, model_blob);
        KLAUNCH(s, K_PIPE_CONFIGS, k_pipe_configs, dim3(bc + be), dim3(SMPLX_BLOCK), s->lds_bytes_valid, a.stream, s->d_space, a.q, B,
                           a.sq, k.edge_w, k.edge_lookups, k.edge_bad, k.state_lookups, k.state_bad, k.work, k.work_count,
                           k.capacity, bc, a.flags, k.succ_coord, a.stab, a.state_q, d_id ? 1 : 0, k.succ_eval, k.succ_goal,
                           s->M, s->N, blob, (int)s->blob_bytes, k.trig);
        if (ev) (void)hipEventRecord(ev[1], a.stream);
        // edges whose waypoints did not fit the work list (normally none) are walked whole by their finish thread
        KLAUNCH(s, K_PIPE_FINISH, k_pipe_finish, dim3(be), dim3(SMPLX_BLOCK), s->lds_bytes, a.stream, s->d_space, a.q, B,
                           k.edge_w, k.edge_lookups, k.edge_bad, k.state_lookups, k.state_bad, a.flags, a.coord, a.sq, a.h,
                           a.cost, a.lookups, a.counters, k.goal_dist, a.stab, a.state_q, d_id, cmp, k.succ_eval, k.succ_goal, k.succ_coord,
                           k.work_count, s->M, s->N);
        wc->dirty = false;
        if (ev) (void)hipEventRecord(ev[2], a.stream);
    }
    HIP_TRY(hipGetLastError());
    return SMPLX_OK;
}

int reserve_expand(smplx_space* s, int B)
{
    const size_t BM = (size_t)B * s->M;
    int e;
    if ((e = reserve(s->batch.b_q, (size_t)B * s->N))) return e;
    if ((e = reserve(s->batch.b_work, expand_work_bytes(B, s->M, s->N)))) return e;
    if ((e = reserve(s->b_flags, BM))) return e;
    if ((e = reserve(s->b_coord, BM * s->N))) return e;
    if ((e = reserve(s->b_sq, BM * s->N))) return e;
    if ((e = reserve(s->b_h, BM))) return e;
    if ((e = reserve(s->batch.b_cost, BM))) return e;
    if ((e = reserve(s->batch.b_lookups, BM))) return e;
    if ((e = reserve(s->b_counters, counter_words(B, s->M)))) return e;
    return SMPLX_OK;
}

// plain-GetSuccs speculation pool (PlainSpeculation in space.h)
inline uint64_t pool_key(const smplx_space* s, int id)
{
    const int32_t h = s->lat.h_of_id[id];
    const double k = (double)s->lat.g_est[id] + s->spec.auto_w * (double)(h < 0 ? 0 : h);
    return k >= 1.8e19 ? ~0ull : (uint64_t)k;
}

inline void pool_push(smplx_space* s, int id)
{
    s->spec.pool.emplace_back(pool_key(s, id), id);
    std::push_heap(s->spec.pool.begin(), s->spec.pool.end(), std::greater<std::pair<uint64_t, int32_t>>());
}

// fill s->spec.hint with the best-ranked states that are neither evaluated nor committed
void auto_hint(smplx_space* s, int miss_id)
{
    s->spec.hint.clear();
    const auto cmp = std::greater<std::pair<uint64_t, int32_t>>();
    while (!s->spec.pool.empty() && (int)s->spec.hint.size() < s->spec.auto_spec) {
        std::pop_heap(s->spec.pool.begin(), s->spec.pool.end(), cmp);
        const std::pair<uint64_t, int32_t> top = s->spec.pool.back();
        s->spec.pool.pop_back();
        const int id = top.second;
        if (id == miss_id || s->lat.cache_off[id] != -1 || s->lat.done_off[id] >= 0) continue;   // evaluated meanwhile
        if (top.first != pool_key(s, id)) continue;                                        // a better-ranked copy exists
        s->spec.hint.push_back(id);
    }
}

// the states of the next frontier batch: `id` plus the hinted frontier states that are neither cached nor in flight
void select_batch(smplx_space* s, int id, int cap)
{
    std::vector<int32_t>& batch = s->inflight;
    batch.clear();
    batch.push_back(id);
    s->lat.cache_off[id] = -2;   // mark as "in this batch"
    for (int32_t hId : s->spec.hint) {
        if ((int)batch.size() >= cap) break;
        if (hId <= 0 || hId >= (int)s->lat.cache_off.size()) continue;
        if (s->lat.cache_off[hId] != -1 || s->lat.done_off[hId] >= 0) continue;
        s->lat.cache_off[hId] = -2;
        batch.push_back(hId);
    }
    s->spec.hint.clear();
}

// A frontier batch takes tens of microseconds; an interrupt-driven hipEventSynchronize adds about as much again to
// wake the thread up.  The search thread has nothing else to do, so it polls -- with a deadline: a batch that has not
// landed after SMPLX_BATCH_TIMEOUT_S seconds (default 30; a batch takes well under a millisecond) is a hung kernel,
// and the caller gets SMPLX_E_HIP instead of a thread that never returns (include/smpl_amd.h: every function returns).
double batch_timeout_seconds()
{
    static const double t = [] {
        const char* e = getenv("SMPLX_BATCH_TIMEOUT_S");
        const double v = e ? atof(e) : 0.0;
        return v > 0.0 ? v : 30.0;
    }();
    return t;
}

int wait_event_polling(hipEvent_t ev)
{
    std::chrono::steady_clock::time_point t0;
    bool timing = false;
    for (unsigned spins = 0;; ++spins) {
        const hipError_t st = hipEventQuery(ev);
        if (st == hipSuccess) return SMPLX_OK;
        if (st != hipErrorNotReady) return set_error(SMPLX_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(st));
        if ((spins & 0x3FFF) == 0x3FFF) {   // look at the clock every 16k polls (a few milliseconds)
            const auto now = std::chrono::steady_clock::now();
            if (!timing) { t0 = now; timing = true; }
            else if (std::chrono::duration<double>(now - t0).count() > batch_timeout_seconds())
                return set_error(SMPLX_E_HIP, "frontier batch did not complete within SMPLX_BATCH_TIMEOUT_S: kernel hung?");
        }
    }
}

// How a driver issues its frontier batches.  Each keeps the launch choice it was measured with (expand_path).
struct BatchMode {
    int zero_copy_max;      // largest batch that may take the zero-copy single launch (0: never)
    bool force_pipeline;    // no single launch with copies
    bool staged_parents;    // the parents' joint values wait in each space's inflight_q (staged by its worker), else in qs
};

// Enqueue one frontier batch on `stream` and return without waiting: the `inflight` states of spaces[q] for every q in
// slots[0..nslots), rows in that order.  q is also the space's slot in the query table `stab` of a cross-query batch
// (null: the batch of `lead` alone).  Parents and the spaces' pending K5 inserts go up in one upload (or stay in pinned
// memory for the zero-copy launch), the outputs come back into fb.pv, and fb.done is recorded behind them.
int issue_frontier(smplx_space* lead, FrontierBatch& fb, smplx_space* const* spaces, const int* slots, int nslots,
                   const SmplxSpaceDev* const* stab, hipStream_t stream, const BatchMode& mode)
{
    const int N = lead->N, M = lead->M;
    size_t total = 0;
    fb.ins_items.clear();
    for (int i = 0; i < nslots; ++i) {
        smplx_space* sq = spaces[slots[i]];
        total += sq->inflight.size();
        // K5: the states committed since the space's last batch join its device table at the head of this batch's first
        // kernel (a requesting space is not being touched by its search)
        if (int e = table_grow_if_needed(sq)) return e;
        table_take_pending(sq, slots[i], fb.ins_items);
    }
    const int B = (int)total;
    const size_t BM = total * M;
    const size_t staged = total * N + (fb.ins_items.size() + 1) / 2;   // doubles: the parents, then the inserts
    const size_t out_bytes = carve_out(nullptr, BM, N).bytes;
    int e;
    if ((e = reserve(fb.b_q, staged)) || (e = reserve(fb.p_q, staged)) || (e = reserve(fb.b_work, expand_work_bytes(B, M, (int)N))) ||
        (e = reserve(fb.b_cost, BM)) || (e = reserve(fb.b_lookups, BM)) || (e = reserve(fb.b_out, out_bytes)) ||
        (e = reserve(fb.p_out, out_bytes)))
        return e;
    if (stab && ((e = reserve(fb.b_stateq, total)) || (e = reserve(fb.p_stateq, total)))) return e;
    // a cross-query batch keeps no tallies: they would mix the queries
    if (!stab && (e = reserve(lead->b_counters, counter_words(B, M)))) return e;
    fb.dv = carve_out(fb.b_out.p, BM, N);
    fb.pv = carve_out(fb.p_out.p, BM, N);
    size_t row = 0;
    for (int i = 0; i < nslots; ++i) {
        const smplx_space* sq = spaces[slots[i]];
        const size_t nrows = sq->inflight.size();
        if (mode.staged_parents) std::memcpy(&fb.p_q.p[row * N], sq->inflight_q.data(), sizeof(double) * N * nrows);
        else
            for (size_t k = 0; k < nrows; ++k) std::memcpy(&fb.p_q.p[(row + k) * N], &sq->lat.qs[(size_t)sq->inflight[k] * N], sizeof(double) * N);
        if (stab) for (size_t k = 0; k < nrows; ++k) fb.p_stateq.p[row + k] = (unsigned short)slots[i];
        row += nrows;
    }
    const size_t item_doubles = stage_items(fb.p_q, total * N, fb.ins_items);
    fb.t_issue = std::chrono::steady_clock::now();
    fb.zero_copy = expand_path(lead, B, mode.zero_copy_max, mode.force_pipeline) == ExpandPath::SmallZeroCopy;
    K5Out k5;
    k5.d_id = fb.dv.id;
    k5.n_items = (int)(fb.ins_items.size() / ((size_t)N + 2));
    ExpandArgs a;
    a.q = fb.b_q.p; a.B = B;
    a.flags = fb.dv.flags; a.coord = fb.dv.coord; a.sq = fb.dv.sq; a.h = fb.dv.h; a.cost = fb.b_cost.p; a.lookups = fb.b_lookups.p;
    a.work = fb.b_work.p;
    a.counters = stab ? nullptr : lead->b_counters.p;
    a.stream = stream;
    a.stab = stab;
    a.k5 = &k5;
    a.force_pipeline = mode.force_pipeline;
    ZeroCopy zc;
    if (fb.zero_copy) {
        // one launch, no copies: parents, query indices, inserts and results live in pinned host memory
        zc.q = fb.p_q.p; zc.flags = fb.pv.flags; zc.coord = fb.pv.coord; zc.sq = fb.pv.sq; zc.h = fb.pv.h; zc.id = fb.pv.id;
        a.zero_copy = &zc;
        a.state_q = stab ? fb.p_stateq.p : nullptr;
        k5.items = (const int32_t*)(fb.p_q.p + total * N);
    } else {
        HIP_TRY(hipMemcpyAsync(fb.b_q.p, fb.p_q.p, sizeof(double) * (total * N + item_doubles), hipMemcpyHostToDevice, stream));
        if (stab) HIP_TRY(hipMemcpyAsync(fb.b_stateq.p, fb.p_stateq.p, sizeof(unsigned short) * total, hipMemcpyHostToDevice, stream));
        a.state_q = stab ? fb.b_stateq.p : nullptr;
        k5.items = (const int32_t*)(fb.b_q.p + total * N);
    }
    if ((e = launch_expand(lead, a))) return e;
    if (!fb.zero_copy)   // one copy for all five outputs
        HIP_TRY(hipMemcpyAsync(fb.p_out.p, fb.b_out.p, out_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(fb.done, stream));
    ++lead->gpu_batches;
    return SMPLX_OK;
}

// enqueue one frontier batch of the space's own (state `id` plus hinted frontier states) on its stream
int issue_batch(smplx_space* s, int id)
{
    select_batch(s, id, s->params.batch_states > 0 ? s->params.batch_states : 4096);
    if (s->small.pipeline_left > 0 && (int)s->inflight.size() <= s->small.batch_max) --s->small.pipeline_left;   // sitting out on the pipeline path (SmallBatchGovernor in space.h)
    const int self = 0;
    return issue_frontier(s, s->batch, &s, &self, 1, nullptr, s->stream, BatchMode{s->small.batch_max, false, false});
}

// one dense output row -> cached successor records (appended to recs); returns the record count
int ingest_row(smplx_space* s, const OutView& pv, size_t row, int* evals_out)
{
    const int N = s->N, M = s->M;
    // the flags first (25 bytes): how many records, then ONE growth of each array and plain copies into it
    int cnt = 0, evals = 0;
    const unsigned char* fl = &pv.flags[row * M];
    for (int p = 0; p < M; ++p) {
        evals += (fl[p] & SMPLX_F_INACTIVE) ? 0 : 1;
        cnt += (fl[p] & SMPLX_F_VALID) ? 1 : 0;
    }
    *evals_out = evals;
    if (cnt == 0) return 0;
    const size_t r0 = s->lat.recs.size();
    s->lat.recs.resize(r0 + cnt);
    s->lat.rec_coord.resize((r0 + cnt) * (size_t)N);
    s->lat.rec_q.resize((r0 + cnt) * (size_t)N);
    size_t r = r0;
    for (int p = 0; p < M; ++p) {
        const unsigned char f = fl[p];
        if (!(f & SMPLX_F_VALID)) continue;
        const size_t k = row * M + p;
        Lattice::Rec& rec = s->lat.recs[r];
        rec.cost = s->actions.dev.cost[p];
        rec.h = pv.h[k];
        rec.goal = (f & SMPLX_F_GOAL) ? 1 : 0;
        rec.known = s->dt.d_table ? pv.id[k] : -1;
        rec.prim = p;
        std::memcpy(&s->lat.rec_coord[r * N], &pv.coord[k * N], sizeof(int32_t) * N);
        std::memcpy(&s->lat.rec_q[r * N], &pv.sq[k * N], sizeof(double) * N);
        ++r;
    }
    return cnt;
}

// a frontier batch has landed: the space's rows of it, from row `first` on, become cached successor records
int collect_batch(smplx_space* s, const FrontierBatch& fb, size_t first)
{
    const std::vector<int32_t>& batch = s->inflight;
    const int B = (int)batch.size();
    if (&fb == &s->batch && fb.zero_copy && s->small.adaptive && B <= 16) {
        // issue-to-landing time of the single-launch path (the search thread has been polling since the issue); only the
        // handful-of-states batches are watched: a batch of hundreds of states legitimately takes longer
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - fb.t_issue).count();
        s->small.latency = s->small.seen == 0 ? dt : 0.8 * s->small.latency + 0.2 * dt;
        if (++s->small.seen >= 16 && s->small.latency > s->small.latency_limit) { s->small.pipeline_left = 2000; s->small.seen = 0; }
    }
    for (int i = 0; i < B; ++i) {
        const int sid = batch[i];
        s->lat.cache_off[sid] = (int64_t)s->lat.recs.size();
        int evals = 0;
        s->lat.cache_cnt[sid] = ingest_row(s, fb.pv, first + (size_t)i, &evals);
        s->lat.eval_count[sid] = evals;
        s->gpu_evals += evals;
    }
    s->inflight.clear();
    return SMPLX_OK;
}

int run_batch(smplx_space* s, int id)
{
    s->small.adaptive = true;   // synchronous: the landing time is the GPU's
    if (int e = issue_batch(s, id)) return e;
    if (int e = wait_event_polling(s->batch.done)) return e;
    return collect_batch(s, s->batch, 0);
}

// GetSuccs (manip_lattice.cpp:219-313): ids are assigned here, in the caller's sequential order
int get_succs(smplx_space* s, int id, const int32_t** succs, const int32_t** costs, int* n)
{
    if (id == 0) { *n = 0; *succs = nullptr; *costs = nullptr; return SMPLX_OK; }   // goal is absorbing (:231)
    if (id < 0 || id >= (int)s->lat.cache_off.size()) return set_error(SMPLX_E_STATE, "unknown state id");
    if (s->lat.done_off[id] < 0) {
        if (s->lat.cache_off[id] < 0) {
            ++s->cache_misses;   // plain GetSuccs callers (the unchanged ARA* of smpl): synchronous batch
            if (s->spec.plain_mode && s->spec.hint.empty() && s->spec.auto_spec > 0) auto_hint(s, id);
            if (int e = run_batch(s, id)) return e;
        } else {
            ++s->cache_hits;
        }
        const int64_t off = s->lat.cache_off[id];
        const int cnt = s->lat.cache_cnt[id];
        const int64_t dof = (int64_t)s->lat.done_succ.size();
        // With many queries per core the tables live in DRAM: a lookup is two dependent misses (slot, coordinate row).
        // The hashes of all records first, their slots prefetched together, then the rows the slots name: the ~14
        // lookups of an expansion overlap instead of queueing (commit is the host's largest share of an expansion).
        uint64_t hashes[SMPLX_MAX_PRIMS];
        const int npre = cnt <= SMPLX_MAX_PRIMS ? cnt : 0;
        for (int k = 0; k < npre; ++k) {
            hashes[k] = CoordTable::hash(&s->lat.rec_coord[(size_t)(off + k) * s->N], s->N);
            s->lat.table.prefetch_slot(hashes[k]);
        }
        for (int k = 0; k < npre; ++k) s->lat.table.prefetch_row(hashes[k], s->lat.coords);
        for (int k = 0; k < cnt; ++k) {
            const Lattice::Rec r = s->lat.recs[off + k];
            const int32_t* c = &s->lat.rec_coord[(size_t)(off + k) * s->N];
            // K5: the device table already named the state when the batch was evaluated (it only holds committed
            // states, so a hit is final); otherwise getOrCreateState on the host table
            int sid = r.known >= 0 ? r.known : (k < npre ? s->lat.table.find_hashed(c, hashes[k], s->lat.coords) : s->lat.table.find(c, s->lat.coords));
            if (sid < 0) {
                sid = new_state(s, c, &s->lat.rec_q[(size_t)(off + k) * s->N], r.h);
            }
            s->lat.done_succ.push_back(r.goal ? 0 : sid);
            s->lat.done_cost.push_back(r.cost);
            s->lat.done_prim.push_back(r.prim);
        }
        s->lat.done_off[id] = dof;
        s->lat.done_cnt[id] = cnt;
    }
    // every GetSuccs call of the reference runs the whole loop body again (a state re-expanded in a later ARA*
    // iteration is re-evaluated, manip_lattice.cpp:263-305); here the repeat is served from the committed list, but it
    // counts as the same number of successor evaluations, so that the figure compares with the CPU planner's
    s->committed_evals += s->lat.eval_count[id];
    if (s->spec.plain_mode) {
        // the caller is expanding `id` now: mirror its g-updates and (re)rank the successors not yet evaluated
        const uint32_t gp = s->lat.g_est[id];
        for (int k = 0; k < s->lat.done_cnt[id]; ++k) {
            const int sid = s->lat.done_succ[s->lat.done_off[id] + k];
            if (sid == 0 || gp >= 1000000000u) continue;
            const uint32_t g = gp + (uint32_t)s->lat.done_cost[s->lat.done_off[id] + k];
            if (g < s->lat.g_est[sid]) {
                s->lat.g_est[sid] = g;
                if (s->lat.cache_off[sid] == -1 && s->lat.done_off[sid] < 0) pool_push(s, sid);
            }
        }
    }
    *n = s->lat.done_cnt[id];
    *succs = s->lat.done_succ.data() + s->lat.done_off[id];
    *costs = s->lat.done_cost.data() + s->lat.done_off[id];
    return SMPLX_OK;
}

}  // namespace
