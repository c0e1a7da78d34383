// smpl_amd/csrc/multi_query.h -- the drivers of smplx_replan_multi: nq queries on the device-resident search
// (search_host.h) or on the host loop (ara_search.h), whose frontier batches go out per query, gathered by one thread
// into cross-query batches (run_group), or through worker threads and one submitter thread (run_pipelined).
#pragma once

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "ara_search.h"
#include "search_host.h"
#include "space.h"
#include "step.h"

namespace {

// Queries that share scene, robot and primitives, driven by the calling thread: every sweep runs each live query until
// it misses, gathers the misses into ONE cross-query frontier batch (per-state query index -> that query's goal and
// BFS grid), and hands the results back.
int run_group(smplx_space** spaces, Search* S, int nq, char* done, double* t_done, std::chrono::steady_clock::time_point t0)
{
    smplx_space* lead = spaces[0];
    int remaining = nq;
    for (int q = 0; q < nq; ++q) S[q].defer_issue = true;
    // hinted frontier states per query and sweep: enough to keep a query fed, small enough that the dense
    // download of a sweep stays in the hundreds of kilobytes
    const int cap_q = std::max(16, std::min(512, (lead->params.batch_states > 0 ? lead->params.batch_states : 4096) / std::max(1, nq / 4)));
    std::vector<int> reqs;
    const bool dbg = getenv("SMPLX_DEBUG_TIMING") != nullptr;
    double t_resume = 0, t_gpu = 0, t_collect = 0;
    long sweeps = 0, swept_states = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
    while (remaining > 0) {
        reqs.clear();
        const auto tr0 = now();
        for (int q = 0; q < nq; ++q) {
            if (done[q]) continue;
            const int r = S[q].resume();
            if (S[q].error) return S[q].error;
            if (r == Search::R_YIELD) { reqs.push_back(q); continue; }
            done[q] = 1;
            --remaining;
            t_done[q] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        }
        const auto tr1 = now();
        t_resume += secs(tr0, tr1);
        if (reqs.empty()) break;
        for (int q : reqs) { select_batch(spaces[q], S[q].miss_id, cap_q); swept_states += (long)spaces[q]->inflight.size(); }
        ++sweeps;
        if (int e = issue_frontier(lead, lead->batch, spaces, reqs.data(), (int)reqs.size(), lead->b_stab.p, lead->stream,
                                   BatchMode{0, false, false})) return e;
        HIP_TRY(hipStreamSynchronize(lead->stream));
        const auto tg1 = now();
        t_gpu += secs(tr1, tg1);
        size_t row = 0;
        for (int q : reqs) {
            const size_t nb = spaces[q]->inflight.size();
            if (int e = collect_batch(spaces[q], lead->batch, row)) return e;
            row += nb;
        }
        t_collect += secs(tg1, now());
    }
    if (dbg) fprintf(stderr, "[smplx timing] %d queries: %ld sweeps, %.1f states/sweep; search+commit %.3fs pack+gpu(issue..sync) %.3fs collect %.3fs\n",
                     nq, sweeps, sweeps ? (double)swept_states / sweeps : 0.0, t_resume, t_gpu, t_collect);
    return SMPLX_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// Asynchronous multi-query driver (host_threads > 1).  Measured on MI355X with the 128 queries of the config-4 shard:
// the sequential host work per expansion (heap, commit, hashing, record ingestion: about 4.7 us) outweighs the GPU time
// of a sweep 15:1 on one thread; several threads that each launch their own sweeps queue up behind each other in the
// runtime (8 threads: 800 us per sweep); and a round barrier between "all searches" and "one batch" makes every round
// as long as its slowest query.  So there are no rounds:
//   * T worker threads own the queries (static ownership: a query's heap and tables stay in one core's caches).  A worker
//     runs a query until it misses, leaves the request in the query's slot and turns to its next query; it makes no
//     HIP call at all.
//   * ONE submitter thread owns the GPU.  Whenever a buffer set is free it takes every request pending at that moment
//     into one cross-query frontier batch (per-state query index -> that query's goal and BFS grid), launches it and
//     moves on; up to kInFlight batches are in flight on their own streams, so the launch and copy overhead of one
//     hides behind the kernels of the other.  A landed batch is announced per query; the owner ingests it when it
//     comes round.
// Every query sees only its own successor records, in its own sequential order: results are those of a solo run.
// ---------------------------------------------------------------------------------------------------------------
struct RingSet : FrontierBatch {
    DevStream stream;
    std::atomic<int> uncollected{0};   // queries of the batch that landed in this set and have not been ingested yet
    std::vector<int> queries;          // the queries of the batch in flight
    bool in_flight = false;
};

enum { QS_RUNNABLE = 0, QS_REQUESTED = 1, QS_LANDED = 2, QS_IN_FLIGHT = 3 };

static inline void cpu_relax() { __builtin_ia32_pause(); }

int run_pipelined(smplx_space** spaces, Search* S, int nq, int nworkers, char* done, double* t_done,
                  std::chrono::steady_clock::time_point t0)
{
    enum { kSets = 8, kInFlight = 4 };
    const int small_zero_copy_max = 512;   // batches up to this size: one launch, results written straight to pinned host memory
    smplx_space* lead = spaces[0];
    const int N = lead->N;
    // one cache line per query state and per counter: the submitter polls them while the workers write them (with the
    // states packed 16 to a line, a scan of all queries cost the submitter 15-50 us per batch and slowed every worker store)
    struct alignas(64) PaddedInt { std::atomic<int> v{0}; };
    std::vector<PaddedInt> qstate_store(nq);
    auto qstate = [&](int q) -> std::atomic<int>& { return qstate_store[q].v; };
    PaddedInt pend_cnt[8], live_cnt[8];   // per issue group: requests waiting / queries not finished
    std::vector<long> row_of(nq, -1);
    std::vector<int> set_of(nq, -1);
    std::atomic<int> remaining{nq}, error{0};
    std::string error_msg;
    const int pause_after = 16;   // expansions without a miss before a query hands its worker to the next one (measured flat between 4 and 1000)
    for (int q = 0; q < nq; ++q) { qstate(q).store(QS_RUNNABLE); S[q].defer_issue = true; S[q].pause_after = pause_after; }
    const int cap_q = std::max(16, std::min(512, (lead->params.batch_states > 0 ? lead->params.batch_states : 4096) / std::max(1, nq / 8)));
    const bool dbg = getenv("SMPLX_DEBUG_TIMING") != nullptr;
    const int device = lead->device;
    const int issue_percent = 45;   // a batch is issued when this share of the live queries waits (1 %: 9.9e5 states/s, 45 %: 1.22e6, 70 %: 1.17e6)
    const int groups = 1;           // (forming batches within 2-3 independent groups of queries was measured: 1.37-1.39e6 against 1.42e6)
    for (int q = 0; q < nq; ++q) live_cnt[(q / nworkers) % groups].v.fetch_add(1, std::memory_order_relaxed);
    std::vector<RingSet> sets(kSets);

    auto fail = [&](int code, const std::string& msg) {
        int expect = 0;
        if (error.compare_exchange_strong(expect, code)) error_msg = msg;
    };

    // worker w owns the queries q with q % nworkers == w
    auto worker = [&](int w) {
        double t_work = 0, t_ingest = 0;
        long n_ingest = 0, n_resume = 0;
        const auto w_begin = std::chrono::steady_clock::now();
        while (remaining.load(std::memory_order_acquire) > 0 && error.load(std::memory_order_relaxed) == 0) {
            bool progressed = false;
            for (int q = w; q < nq; q += nworkers) {
                if (done[q]) continue;
                int st = qstate(q).load(std::memory_order_acquire);
                if (st == QS_REQUESTED || st == QS_IN_FLIGHT) continue;
                const auto a0 = std::chrono::steady_clock::now();
                if (st == QS_LANDED) {
                    RingSet& Bf = sets[set_of[q]];
                    if (int e = collect_batch(spaces[q], Bf, (size_t)row_of[q])) { fail(e, g_error); return; }
                    Bf.uncollected.fetch_sub(1, std::memory_order_acq_rel);
                    qstate(q).store(QS_RUNNABLE, std::memory_order_relaxed);
                    if (dbg) { t_ingest += std::chrono::duration<double>(std::chrono::steady_clock::now() - a0).count(); ++n_ingest; }
                }
                ++n_resume;
                const int r = S[q].resume();
                progressed = true;
                if (S[q].error) { fail(S[q].error, g_error); return; }
                if (r == Search::R_YIELD) {
                    if (S[q].miss_id >= 0) {
                        select_batch(spaces[q], S[q].miss_id, cap_q);
                        {   // stage the parents' joint values for the submitter
                            smplx_space* sq = spaces[q];
                            sq->inflight_q.resize(sq->inflight.size() * (size_t)N);
                            size_t r = 0;
                            for (int32_t id : sq->inflight) { std::memcpy(&sq->inflight_q[r * N], &sq->lat.qs[(size_t)id * N], sizeof(double) * N); ++r; }
                        }
                        qstate(q).store(QS_REQUESTED, std::memory_order_release);
                        pend_cnt[(q / nworkers) % groups].v.fetch_add(1, std::memory_order_release);
                    }
                } else {
                    done[q] = 1;
                    t_done[q] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                    live_cnt[(q / nworkers) % groups].v.fetch_sub(1, std::memory_order_acq_rel);
                    remaining.fetch_sub(1, std::memory_order_acq_rel);
                }
                t_work += std::chrono::duration<double>(std::chrono::steady_clock::now() - a0).count();
            }
            if (!progressed) cpu_relax();
        }
        if (dbg) {
            const double tot = std::chrono::duration<double>(std::chrono::steady_clock::now() - w_begin).count();
            fprintf(stderr, "[smplx timing] worker %d: search+commit+ingest %.3fs of %.3fs (ingest %.3fs in %ld landings; %ld resumes)\n", w, t_work, tot,
                    t_ingest, n_ingest, n_resume);
        }
    };

    auto submitter = [&]() -> int {
        HIP_TRY(hipSetDevice(device));
        for (RingSet& Bf : sets) {
            HIP_TRY(Bf.stream.create());
            HIP_TRY(Bf.done.create(hipEventDisableTiming));
        }
        long sweeps = 0, states = 0;
        double t_issue = 0;
        int in_flight = 0, next_set = 0, oldest = 0;
        // SMPLX_DEBUG_TIMING: how long the GPU had nothing of this shard, issue-to-landing time, depth at issue
        double t_gpu_idle = 0, lat_sum = 0;
        long depth_sum = 0;
        auto idle_since = std::chrono::steady_clock::now();
        std::chrono::steady_clock::time_point issued_at[kSets];
        unsigned poll_spins = 0;
        while (remaining.load(std::memory_order_acquire) > 0 && error.load(std::memory_order_relaxed) == 0) {
            bool did = false;
            // retire landed batches in issue order
            while (in_flight > 0) {
                RingSet& Bf = sets[oldest];
                const hipError_t st = hipEventQuery(Bf.done);
                if (st == hipErrorNotReady) {
                    // a batch takes well under a millisecond: one that has not landed after SMPLX_BATCH_TIMEOUT_S is a hung
                    // kernel; the workers leave through `error` and the call returns (include/smpl_amd.h: every function returns)
                    if ((++poll_spins & 0x3FFF) == 0 &&
                        std::chrono::duration<double>(std::chrono::steady_clock::now() - issued_at[oldest]).count() > batch_timeout_seconds())
                        return set_error(SMPLX_E_HIP, "frontier batch did not complete within SMPLX_BATCH_TIMEOUT_S: kernel hung?");
                    break;
                }
                if (st != hipSuccess) return set_error(SMPLX_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(st));
                Bf.uncollected.store((int)Bf.queries.size(), std::memory_order_relaxed);
                for (int q : Bf.queries) qstate(q).store(QS_LANDED, std::memory_order_release);
                Bf.in_flight = false;
                if (dbg) {
                    const auto nowt = std::chrono::steady_clock::now();
                    lat_sum += std::chrono::duration<double>(nowt - issued_at[oldest]).count();
                    if (in_flight == 1) idle_since = nowt;
                }
                oldest = (oldest + 1) % kSets;
                --in_flight;
                did = true;
            }
            // issue: every request pending right now, if a buffer set is free
            RingSet& Nf = sets[next_set];
            if (in_flight < kInFlight && !Nf.in_flight && Nf.uncollected.load(std::memory_order_acquire) == 0) {
                const auto i0 = std::chrono::steady_clock::now();
                // A batch has a fixed cost (issuing ~15 us, ~40 us on the GPU whatever its size).  Taking every request the
                // moment it appears gives many small batches and a query then waits for several batch times per miss, so a batch
                // is issued when issue_percent (45 %) of the live queries are waiting; the two counters are kept by the workers.
                int live_g[8], pend_g[8];
                for (int g = 0; g < groups; ++g) {
                    live_g[g] = live_cnt[g].v.load(std::memory_order_acquire);
                    pend_g[g] = pend_cnt[g].v.load(std::memory_order_acquire);
                }
                // the group closest to its threshold (one group: every live query)
                int pick = -1;
                for (int g = 0; g < groups; ++g) {
                    if (live_g[g] == 0 || pend_g[g] == 0) continue;
                    if (pend_g[g] < std::max(1, (live_g[g] * issue_percent + 99) / 100)) continue;
                    if (pick < 0 || (long)pend_g[g] * live_g[pick] > (long)pend_g[pick] * live_g[g]) pick = g;
                }
                Nf.queries.clear();
                size_t total = 0;
                if (pick >= 0) {
                    for (int q = 0; q < nq; ++q) {
                        if ((q / nworkers) % groups != pick) continue;
                        if (qstate(q).load(std::memory_order_acquire) != QS_REQUESTED) continue;
                        row_of[q] = (long)total;
                        set_of[q] = next_set;
                        total += spaces[q]->inflight.size();
                        Nf.queries.push_back(q);
                    }
                    pend_cnt[pick].v.fetch_sub((int)Nf.queries.size(), std::memory_order_acq_rel);
                }
                if (total > 0) {
                    for (int q : Nf.queries) qstate(q).store(QS_IN_FLIGHT, std::memory_order_relaxed);
                    // The parents' joint values were staged by each query's worker when it made the request (they were in
                    // its cache then; gathering 270 rows from 58 queries' state arrays here cost the submitter ~20 us of
                    // cache misses per batch).  Batches of up to 512 states: ONE launch, results written straight to
                    // pinned host memory.  Against the pipeline (two uploads, four kernels, one download: seven runtime
                    // calls) the submitter spends 34 instead of 48 us per batch and a batch lands after 78 instead of
                    // 113 us: shard +8..17 % (same box, A/B).  (Round 2 first measured the opposite -- 152 us per launch
                    // at ~100 states -- because the kernel then checked the snap-to-goal edge of every state ungated, see
                    // k_small_batch.)
                    if (int e = issue_frontier(lead, Nf, spaces, Nf.queries.data(), (int)Nf.queries.size(), lead->b_stab.p, Nf.stream,
                                               BatchMode{small_zero_copy_max, true, true})) return e;
                    issued_at[next_set] = i0;
                    if (dbg) {
                        depth_sum += in_flight;
                        if (in_flight == 0) t_gpu_idle += std::chrono::duration<double>(i0 - idle_since).count();
                    }
                    Nf.in_flight = true;
                    ++in_flight;
                    next_set = (next_set + 1) % kSets;
                    ++sweeps; states += (long)total;
                    did = true;
                    t_issue += std::chrono::duration<double>(std::chrono::steady_clock::now() - i0).count();
                }
            }
            if (!did) cpu_relax();
        }
        // drain what is still in flight (only on error paths: with no live query nothing is pending)
        for (RingSet& Bf : sets) if (Bf.stream) (void)hipStreamSynchronize(Bf.stream);
        if (dbg) fprintf(stderr, "[smplx timing] submitter: %ld batches, %.1f states/batch; issuing %.3fs (pack + enqueue); GPU without a batch %.3fs; "
                                 "issue-to-landing %.1f us on average; %.2f batches already in flight at issue\n",
                         sweeps, sweeps ? (double)states / sweeps : 0.0, t_issue, t_gpu_idle, sweeps ? 1e6 * lat_sum / sweeps : 0.0,
                         sweeps ? (double)depth_sum / sweeps : 0.0);
        return SMPLX_OK;
    };

    std::vector<std::thread> th;
    for (int w = 0; w < nworkers; ++w) th.emplace_back(worker, w);
    int rc = submitter();
    if (rc != SMPLX_OK) fail(rc, g_error);
    for (auto& x : th) x.join();
    for (RingSet& Bf : sets) if (Bf.stream) (void)hipStreamSynchronize(Bf.stream);   // before `sets` frees its buffers
    if (error.load() != 0) return set_error(error.load(), error_msg);
    return SMPLX_OK;
}

// two spaces that can share launches: the same scene (grid handle), model image, primitives and expansion mode
bool same_scene_and_robot(const smplx_space* a, const smplx_space* b)
{
    // (BFS or closed-form: a constant of the per-robot build, lattice_steps.h closed_form_of; Euclidean and joint distance may share)
    return a->grid == b->grid && a->blob_bytes == b->blob_bytes && std::memcmp(a->hs.model_blob, b->hs.model_blob, a->blob_bytes) == 0 &&
           std::memcmp(&a->hs.actions, &b->hs.actions, sizeof(SmplxActionsDev)) == 0 && a->step.fused_mode == b->step.fused_mode &&
           (a->params.heuristic == SMPLX_H_BFS) == (b->params.heuristic == SMPLX_H_BFS);
}

int read_counters(smplx_space* s, size_t cw, unsigned long long counters[4])
{
    std::vector<unsigned long long> part(cw);
    HIP_TRY(hipMemcpy(part.data(), s->b_counters.p, sizeof(unsigned long long) * cw, hipMemcpyDeviceToHost));
    for (int k = 0; k < 4; ++k) counters[k] = 0;
    for (size_t i = 0; i < cw; ++i) if (i % SMPLX_TALLIES < 4) counters[i % SMPLX_TALLIES] += part[i];
    return SMPLX_OK;
}

// ARAStar::replan(const TimeParameters&, ...) for nq queries (smplx_replan_multi); t_call: when the call began
int replan_multi(smplx_space** spaces, int nq, const smplx_time_params* p, int32_t* path_ids, int cap,
                        smplx_replan_stats* stats, double* wall_seconds, int host_threads, std::chrono::steady_clock::time_point t_call)
{
    for (int q = 0; q < nq; ++q) {
        smplx_space* s = spaces[q];
        if (!s) return set_error(SMPLX_E_ARG, "null space");
        if (!s->goal.set) return set_error(SMPLX_E_STATE, "goal not set");
        if (s->lat.start_id < 0) return set_error(SMPLX_E_STATE, "start not set");
        if (s->grid->epoch != s->goal.grid_epoch) return set_error(SMPLX_E_STATE, "the grid was edited after the goal was set: cached successors are stale, set the goal again");
        if (s->att.epoch != s->att.epoch_goal) return set_error(SMPLX_E_STATE, kBodiesChanged);
    }
    // ---- the device-resident search: one persistent workgroup per query, no host round trips.  Taken
    // whenever the kernel fits the robot (search_host.h); SMPLX_SEARCH=host selects the host-driven loop below, which is
    // also what serves an external SBPL planner through smplx_get_succs ----
    bool device = true;
    for (int q = 0; q < nq && device; ++q) device = search_on_device(spaces[q]);
    {
        const char* mode = getenv("SMPLX_SEARCH");
        if (mode && !std::strcmp(mode, "device")) {
            if (!device) return set_error(SMPLX_E_LIMIT, "SMPLX_SEARCH=device: the search kernel does not fit this robot / space");
        } else if (nq == 1) {
            // A lone query is a chain of dependent expansions: measured on MI355X (cfg 2) the host-driven loop with its
            // speculative frontier batches expands 1.1e5 states/s, the single workgroup 3.9e4; the device-resident search
            // wins where it has queries to run side by side (cfg 4: 4.5e6 against 1.5e6 states/s).
            device = false;
        }
    }
    // which queries continue the search their space holds (include/smpl_amd.h: same side, same start, no new goal, no
    // failed call since)
    const int side = device ? 1 : 2;
    std::vector<char> resume(nq, 0);
    for (int q = 0; q < nq; ++q) {
        const smplx_space* s = spaces[q];
        resume[q] = !p->from_scratch && s->search_side == side && s->search_start == s->lat.start_id && (device || s->host_search);
    }
    std::vector<Search> S(device ? 0 : nq);
    std::vector<size_t> cw(nq);
    struct Base { int64_t b, h, m, c, g; };
    std::vector<Base> base(nq);
    for (int q = 0; q < nq; ++q) {
        smplx_space* s = spaces[q];
        s->search_side = 0;                      // until this call has succeeded
        if (!resume[q]) {
            if (int e = pull_lattice(s)) return e;
            if (int e = pull_log(s)) return e;
            s->expansion_log.clear();
        }
        if (!device) {
            if (resume[q]) {
                S[q] = std::move(*s->host_search);
                set_call_params(S[q], p, t_call);
                S[q].continue_call();
            } else {
                fill_search(S[q], s, p, t_call);
            }
        }
        s->small.adaptive = nq == 1;
        if (nq > 1) s->small.pipeline_left = 0;
        const int capB = s->params.batch_states > 0 ? s->params.batch_states : 4096;
        cw[q] = counter_words(capB, s->M);
        if (int e = reserve(s->b_counters, cw[q])) return e;
        HIP_TRY(hipMemsetAsync(s->b_counters.p, 0, sizeof(unsigned long long) * cw[q], s->stream));
        base[q] = {s->gpu_batches, s->cache_hits, s->cache_misses, s->committed_evals, s->gpu_evals};
    }
    std::vector<char> done(nq, 0), waiting(nq, 0);
    std::vector<double> t_done(nq, 0.0);
    // Queries that share the scene (same grid handle), robot and primitives can share launches: their misses are
    // gathered into ONE cross-query frontier batch per sweep (per-state query index -> that query's goal and BFS
    // grid).  Otherwise each query issues its own batches on its own stream.
    bool grouped = nq > 1;
    for (int q = 1; q < nq && grouped; ++q) grouped = same_scene_and_robot(spaces[0], spaces[q]);
    const auto t0 = std::chrono::steady_clock::now();
    if (device) {
        if (grouped || nq == 1) {
            if (int e = search_run(spaces, nq, p, resume.data(), path_ids, cap, stats, t_done.data(), t0, t_call)) return e;
        } else {
            for (int q = 0; q < nq; ++q)
                if (int e = search_run(spaces + q, 1, p, resume.data() + q, path_ids ? path_ids + (size_t)q * cap : nullptr, cap, stats + q,
                                       t_done.data() + q, t0, t_call)) return e;
        }
        if (wall_seconds) *wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        for (int q = 0; q < nq; ++q) { spaces[q]->search_side = side; spaces[q]->search_start = spaces[q]->lat.start_id; }
        return SMPLX_OK;
    }
    // the host loop's cross-query batches check every row against the leading space's attached bodies: a query with
    // bodies of its own issues its own batches (the device search reads each query's bodies in its own workgroup)
    for (int q = 0; q < nq && grouped; ++q) grouped = spaces[q]->att.bodies.empty();
    if (grouped) {
        // the query table of the cross-query batches (per-row query index -> that query's goal and BFS grid), held by
        // the leading space
        HIP_TRY(hipSetDevice(spaces[0]->device));
        std::vector<const SmplxSpaceDev*> tab(nq);
        for (int q = 0; q < nq; ++q) tab[q] = spaces[q]->d_space;
        if (int e = reserve(spaces[0]->b_stab, nq)) return e;
        HIP_TRY(hipMemcpy(spaces[0]->b_stab.p, tab.data(), sizeof(void*) * nq, hipMemcpyHostToDevice));
        // one thread sweeps all queries (run_group), or host_threads worker threads own them and this thread is the only
        // GPU submitter (run_pipelined)
        const int nthreads = std::max(1, std::min(host_threads > 0 ? host_threads : 1, nq));
        const int e = nthreads == 1 || nq < 4 ? run_group(spaces, S.data(), nq, done.data(), t_done.data(), t0)
                                              : run_pipelined(spaces, S.data(), nq, nthreads, done.data(), t_done.data(), t0);
        if (e) return e;
    } else {
        // One host thread drives every query: a query runs until it misses, its frontier batch goes to its own
        // stream, and the thread moves on to the next query; a landed batch is collected when its turn comes again.
        double t_resume = 0, t_wait = 0, t_collect = 0;
        const bool dbg = getenv("SMPLX_DEBUG_TIMING") != nullptr;
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
        int remaining = nq;
        while (remaining > 0) {
            bool progressed = false;
            for (int q = 0; q < nq; ++q) {
                if (done[q]) continue;
                smplx_space* s = spaces[q];
                if (waiting[q]) {
                    const hipError_t st = hipEventQuery(s->batch.done);
                    if (st == hipErrorNotReady) continue;
                    if (st != hipSuccess) return set_error(SMPLX_E_HIP, std::string("hipEventQuery: ") + hipGetErrorString(st));
                    const auto c0 = now();
                    if (int e = collect_batch(s, s->batch, 0)) return e;
                    t_collect += secs(c0, now());
                    waiting[q] = 0;
                }
                const auto r0 = now();
                const int r = S[q].resume();
                t_resume += secs(r0, now());
                progressed = true;
                if (S[q].error) return S[q].error;
                if (r == Search::R_YIELD) { waiting[q] = 1; continue; }
                done[q] = 1;
                --remaining;
                t_done[q] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            }
            if (!progressed) {
                // every live query is waiting on the GPU: block on one of them instead of spinning
                const auto w0 = now();
                for (int q = 0; q < nq; ++q)
                    if (!done[q] && waiting[q]) { if (int e = wait_event_polling(spaces[q]->batch.done)) return e; break; }
                t_wait += secs(w0, now());
            }
        }
        if (dbg) fprintf(stderr, "[smplx timing] resume(search+issue) %.3fs wait %.3fs collect %.3fs; launches: single-kernel %lld pipeline %lld\n",
                         t_resume, t_wait, t_collect, (long long)spaces[0]->small.small_launches, (long long)spaces[0]->small.pipe_launches);
    }
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (wall_seconds) *wall_seconds = wall;
    for (int q = 0; q < nq; ++q) {
        smplx_space* s = spaces[q];
        unsigned long long counters[4] = {0, 0, 0, 0};
        if (!grouped) { if (int e = read_counters(s, cw[q], counters)) return e; }
        smplx_replan_stats& rs = stats[q];
        std::memset(&rs, 0, sizeof(rs));
        smplx_search_stats& st = rs.s;
        st.solved = S[q].solved;
        st.path_len = (int)S[q].solution.size();
        st.cost = S[q].cost;
        st.expansions = S[q].expand_count;
        st.expansions_init = S[q].expand_count_init;
        st.satisfied_eps = S[q].satisfied_eps;
        st.seconds = t_done[q];
        st.gpu_succ_evals = s->gpu_evals - base[q].g;
        st.grid_lookups = (int64_t)counters[2];
        st.committed_succ_evals = s->committed_evals - base[q].c;
        st.gpu_batches = s->gpu_batches - base[q].b;
        st.cache_misses = s->cache_misses - base[q].m;
        st.cache_hits = (s->cache_hits - base[q].h) - st.cache_misses;   // expansions served without waiting for the GPU
        if (path_ids)
            for (int i = 0; i < (int)S[q].solution.size() && i < cap; ++i) path_ids[(size_t)q * cap + i] = S[q].solution[i];
        rs.call_expansions = S[q].num;
        rs.resumed = resume[q];
        rs.result = S[q].err;
        if (S[q].solved && S[q].satisfied_eps == std::numeric_limits<double>::infinity()) rs.result = SMPLX_ARA_PARTIAL;
        else if (S[q].err == 0) rs.result = SMPLX_ARA_SUCCESS;
        // the search stays with its space for a later call
        if (!s->host_search) s->host_search = std::make_shared<Search>();
        *s->host_search = std::move(S[q]);
        s->search_side = side;
        s->search_start = s->lat.start_id;
    }
    return SMPLX_OK;
}

}  // namespace
