// smpl_amd/csrc/plan_entry.h -- the lattice and planning entry points of the C-ABI: the start state, GetSuccs and its
// lazy pair (lazy.h), the reads of the state table, smplx_plan / smplx_replan and their multi-query forms
// (multi_query.h), the expansion log, path post-processing (path_tools.h; a batch of paths: path_multi.h), and the counters and test hooks of the
// device-resident search (search_host.h, test_hooks.h).
#pragma once

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "heuristic_host.h"
#include "lazy.h"
#include "multi_query.h"
#include "path_tools.h"
#include "queries.h"
#include "search_host.h"
#include "test_hooks.h"

extern "C" {

int smplx_set_start(smplx_space* s, const double* q, int* id)
{
    if (!s || !q) return set_error(SMPLX_E_ARG, "null argument");
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "set the goal before the start (planner_interface.cpp:1469-1500 order)");
    if (!sane_values(q, s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (!host_check_limits(s->model.dev, q)) return set_error(SMPLX_E_INVALID, "start state violates joint limits");
    if (int e = pull_lattice(s)) return e;
    uint8_t ok = 0;
    if (int e = smplx_cc_state_valid_batch(s, q, 1, &ok, nullptr)) return e;
    if (!ok) return set_error(SMPLX_E_INVALID, "start state is in collision");
    std::vector<int32_t> c(s->N);
    state_to_coord(s->model.dev, q, c.data());
    int sid = s->lat.table.find(c.data(), s->lat.coords);
    int32_t h = 0;
    if (int e = run_heuristic(s, q, 1, &h, s->goal.start_xyz)) return e;   // also the start's planning-link position
    if (sid < 0) sid = new_state(s, c.data(), q, h);
    s->lat.start_id = sid;
    if (s->spec.plain_mode) { std::fill(s->lat.g_est.begin(), s->lat.g_est.end(), 1000000000u); s->lat.g_est[sid] = 0; s->spec.pool.clear(); }
    if (id) *id = sid;
    return SMPLX_OK;
}

int smplx_start_id(const smplx_space* s) { return s ? s->lat.start_id : -1; }
int smplx_goal_id(const smplx_space* s) { (void)s; return 0; }

int smplx_get_succs(smplx_space* s, int id, int32_t* succs, int32_t* costs, int cap, int* n)
{
    if (!s || !n) return set_error(SMPLX_E_ARG, "null argument");
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "goal not set");
    if (s->grid->epoch != s->goal.grid_epoch) return set_error(SMPLX_E_STATE, "the grid was edited after the goal was set: cached successors are stale, set the goal again");
    if (s->att.epoch != s->att.epoch_goal) return set_error(SMPLX_E_STATE, kBodiesChanged);
    if (int e = pull_lattice(s)) return e;
    if (!s->spec.plain_mode) {
        // first GetSuccs from outside: start mirroring the caller's g-values (the start has g = 0, arastar.cpp:172-176)
        s->spec.plain_mode = true;
        std::fill(s->lat.g_est.begin(), s->lat.g_est.end(), 1000000000u);
        if (s->lat.start_id > 0) s->lat.g_est[s->lat.start_id] = 0;
        s->spec.pool.clear();
    }
    const int32_t *ps, *pc;
    int cnt = 0;
    if (int e = get_succs(s, id, &ps, &pc, &cnt)) {
        // the SBPL-side caller (GetSuccs has no return value) sees an empty list; the error stays readable here
        if (s->status == SMPLX_OK) { s->status = e; s->status_msg = g_error; }
        return e;
    }
    *n = cnt;
    for (int i = 0; i < cnt && i < cap; ++i) {
        if (succs) succs[i] = ps[i];
        if (costs) costs[i] = pc[i];
    }
    return SMPLX_OK;
}

// ---- lazy successors: GetLazySuccs / GetTrueCost (include/smpl_amd.h; kernels: lazy_kernels.h, host: lazy.h) ----------

int smplx_get_lazy_succs(smplx_space* s, int id, int32_t* succs, int32_t* costs, int cap, int* n)
{
    if (n) *n = 0;
    if (!s || !n) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = lazy_guard(s)) return lazy_keep_status(s, e);
    const int32_t* ps = nullptr;
    int cnt = 0;
    if (int e = get_lazy_succs(s, id, &ps, &cnt)) return lazy_keep_status(s, e);
    *n = cnt;
    for (int i = 0; i < cnt && i < cap; ++i) {
        if (succs) succs[i] = ps[i];
        if (costs) costs[i] = SMPLX_LAZY_COST;
    }
    return SMPLX_OK;
}

int smplx_true_cost_batch(smplx_space* s, const int32_t* parent_ids, const int32_t* child_ids, int n, int32_t* costs, int32_t* prims,
                          int32_t* nmatch)
{
    if (!s || n < 0 || (n > 0 && (!parent_ids || !child_ids || !costs))) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (int e = lazy_guard(s)) return e;
    return true_cost_pairs(s, parent_ids, child_ids, n, costs, prims, nmatch, false);
}

int smplx_get_true_cost(smplx_space* s, int parent_id, int child_id, int32_t* cost)
{
    if (cost) *cost = -1;
    if (!s || !cost) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = lazy_guard(s)) return lazy_keep_status(s, e);
    const int32_t p = parent_id, c = child_id;
    return lazy_keep_status(s, true_cost_pairs(s, &p, &c, 1, cost, nullptr, nullptr, true));
}

int smplx_lazy_expand_batch(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* succ_q, int32_t* h,
                            int32_t* succ_id)
{
    if (!s || !q || B < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (B == 0) return SMPLX_OK;
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "set a goal first (the primitives are gated by goal distance)");
    if (!sane_values(q, (size_t)B * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    if (int e = pull_lattice(s)) return e;
    return lazy_rows(s, q, B, flags, coord, succ_q, h, succ_id, true);
}

int smplx_lazy_expand_batch_device(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_succ_q,
                                   int32_t* d_h, int32_t* d_succ_id, void* stream)
{
    if (!s || !d_q || !d_flags || B <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "set a goal first");
    if (int e = pull_lattice(s)) return e;
    return launch_lazy_succs(s, d_q, B, d_flags, d_coord, d_succ_q, d_h, d_succ_id, (hipStream_t)stream, true);
}

int smplx_true_cost_q_batch(smplx_space* s, const double* parent_q, const int32_t* child_coord, const uint8_t* goal_edge, int n,
                            int32_t* costs, int32_t* prims, int32_t* nmatch)
{
    if (!s || n < 0 || (n > 0 && (!parent_q || !child_coord || !costs))) return set_error(SMPLX_E_ARG, "bad argument");
    if (n == 0) return SMPLX_OK;
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "set a goal first (the primitives are gated by goal distance)");
    if (!sane_values(parent_q, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    return true_cost_items(s, parent_q, child_coord, goal_edge, n, costs, prims, nmatch);
}

size_t smplx_true_cost_work_doubles(const smplx_space* s, int n)
{
    return s && n > 0 ? (size_t)n * s->N * SMPLX_TRUE_COST_LANES : 0;
}

int smplx_true_cost_q_batch_device(smplx_space* s, const double* d_parent_q, const int32_t* d_child_coord, const uint8_t* d_goal_edge,
                                   int n, double* d_work_q, int32_t* d_costs, int32_t* d_prims, int32_t* d_nmatch, void* stream)
{
    if (!s || !d_parent_q || !d_child_coord || !d_goal_edge || !d_work_q || !d_costs || n <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "set a goal first");
    return launch_true_cost(s, d_parent_q, d_child_coord, d_goal_edge, n, d_work_q, d_costs, d_prims, d_nmatch, (hipStream_t)stream);
}

int smplx_lazy_counters(const smplx_space* s, int64_t out[6])
{
    if (!s || !out) return set_error(SMPLX_E_ARG, "null argument");
    for (int k = 0; k < 6; ++k) out[k] = s->lazy.counters[k];
    return SMPLX_OK;
}

int smplx_hint_frontier(smplx_space* s, const int32_t* ids, int n)
{
    if (!s || (!ids && n > 0)) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = pull_lattice(s)) return e;
    s->spec.hint.assign(ids, ids + n);
    return SMPLX_OK;
}

int smplx_get_goal_heuristic(smplx_space* s, int id, int32_t* h)
{
    if (!s || !h) return set_error(SMPLX_E_ARG, "null argument");
    if (int e = pull_lattice(s)) return e;
    if (id < 0 || id >= (int)s->lat.h_of_id.size()) return set_error(SMPLX_E_STATE, "unknown state id");
    *h = s->lat.h_of_id[id];
    return SMPLX_OK;
}

int smplx_num_states(const smplx_space* s)
{
    if (!s) return 0;
    if (s->ds.host_behind) return s->ds.h.nstates;     // the device-resident search created states the host has not fetched yet
    return (int)s->lat.h_of_id.size();
}

int smplx_space_counters(const smplx_space* s, int64_t out[6])
{
    if (!s || !out) return set_error(SMPLX_E_ARG, "null argument");
    out[0] = s->gpu_batches; out[1] = s->cache_hits; out[2] = s->cache_misses; out[3] = s->committed_evals;
    out[4] = s->gpu_evals; out[5] = (int64_t)smplx_num_states(s);
    return SMPLX_OK;
}

int smplx_get_state(const smplx_space* cs, int id, double* q, int32_t* coord)
{
    if (!cs) return set_error(SMPLX_E_ARG, "null argument");
    smplx_space* s = const_cast<smplx_space*>(cs);      // (fetching what the device created does not change the lattice)
    if (int e = pull_lattice(s)) return e;
    if (id < 0 || id >= (int)s->lat.h_of_id.size()) return set_error(SMPLX_E_STATE, "unknown state id");
    if (q) std::memcpy(q, &s->lat.qs[(size_t)id * s->N], sizeof(double) * s->N);
    if (coord) std::memcpy(coord, &s->lat.coords[(size_t)id * s->N], sizeof(int32_t) * s->N);
    return SMPLX_OK;
}

int smplx_replan_multi(smplx_space** spaces, int nq, const smplx_time_params* p, int32_t* path_ids, int cap,
                       smplx_replan_stats* stats, double* wall_seconds, int host_threads)
{
    const auto t_call = std::chrono::steady_clock::now();
    if (!spaces || nq <= 0 || !p || !stats) return set_error(SMPLX_E_ARG, "bad argument");
    if (path_ids && cap <= 0) return set_error(SMPLX_E_ARG, "path_ids needs cap > 0");
    if (p->type != SMPLX_TIME_EXPANSIONS && p->type != SMPLX_TIME_WALL) return set_error(SMPLX_E_ARG, "unknown timing type");
    if (!(p->max_seconds_init >= 0.0) || !(p->max_seconds >= 0.0)) return set_error(SMPLX_E_ARG, "time budgets must be >= 0");
    if (!(p->initial_eps >= 1.0) || !(p->final_eps >= 0.0) || !(p->delta_eps > 0.0) || !std::isfinite(p->initial_eps))
        return set_error(SMPLX_E_ARG, "epsilons: initial_eps >= 1 (finite), final_eps >= 0, delta_eps > 0");
    for (int q = 0; q < nq; ++q)
        for (int r = 0; r < q; ++r)
            if (spaces[q] && spaces[q] == spaces[r]) return set_error(SMPLX_E_ARG, "a space appears twice");
    const int e = replan_multi(spaces, nq, p, path_ids, cap, stats, wall_seconds, host_threads, t_call);
    if (e != SMPLX_OK)
        for (int q = 0; q < nq; ++q) if (spaces[q]) spaces[q]->search_side = 0;   // a failed call: the next one starts from scratch
    return e;
}

int smplx_replan(smplx_space* s, const smplx_time_params* p, int32_t* path_ids, int cap, smplx_replan_stats* st)
{
    if (!s) return set_error(SMPLX_E_ARG, "null argument");
    return smplx_replan_multi(&s, 1, p, path_ids, cap, st, nullptr, 1);
}

// ARAStar::replan from scratch under an expansion bound: smplx_replan_multi with from_scratch = 1
int smplx_plan_multi(smplx_space** spaces, int nq, const smplx_search_params* p, int32_t* path_ids, int cap,
                     smplx_search_stats* stats, double* wall_seconds, int host_threads)
{
    const auto t_call = std::chrono::steady_clock::now();
    if (!spaces || nq <= 0 || !p || !stats) return set_error(SMPLX_E_ARG, "bad argument");
    smplx_time_params tp;
    std::memset(&tp, 0, sizeof(tp));
    tp.initial_eps = p->initial_eps; tp.final_eps = p->final_eps; tp.delta_eps = p->delta_eps;
    tp.improve = p->improve; tp.bounded = p->bounded; tp.type = SMPLX_TIME_EXPANSIONS;
    tp.max_expansions_init = p->max_expansions_init; tp.max_expansions = p->max_expansions;
    tp.from_scratch = 1;
    std::vector<smplx_replan_stats> rs(nq);
    const int e = replan_multi(spaces, nq, &tp, path_ids, cap, rs.data(), wall_seconds, host_threads, t_call);
    if (e != SMPLX_OK) {
        for (int q = 0; q < nq; ++q) if (spaces[q]) spaces[q]->search_side = 0;
        return e;
    }
    for (int q = 0; q < nq; ++q) stats[q] = rs[q].s;
    return SMPLX_OK;
}

int smplx_plan(smplx_space* s, const smplx_search_params* p, int32_t* path_ids, int cap, smplx_search_stats* stats)
{
    if (!s) return set_error(SMPLX_E_ARG, "null argument");
    return smplx_plan_multi(&s, 1, p, path_ids, cap, stats, nullptr, 1);
}

int smplx_expansion_log_size(const smplx_space* s)
{
    if (!s) return 0;
    return s->ds.log_on_device ? s->ds.h.n_log : (int)s->expansion_log.size();
}

int smplx_expansion_log(const smplx_space* cs, int32_t* out)
{
    if (!cs || !out) return set_error(SMPLX_E_ARG, "null argument");
    smplx_space* s = const_cast<smplx_space*>(cs);
    if (int e = pull_log(s)) return e;
    std::copy(s->expansion_log.begin(), s->expansion_log.end(), out);
    return SMPLX_OK;
}

int smplx_post_process_path(smplx_space* s, const double* path, int n, int flags, double* out, int cap, int* nout,
                            int64_t* stats)
{
    if (!s || (!path && n > 0) || n < 0 || !nout) return set_error(SMPLX_E_ARG, "bad argument");
    if (n > 0 && !sane_values(path, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    PathTools T(s);
    std::vector<double> p(path, path + (size_t)n * s->N);
    const bool fork_test = !(flags & SMPLX_PP_UPSTREAM_LIMITS);
    bool done = false;
    // PlannerInterface::postProcessPath (planner_interface.cpp:2651-2697)
    if (flags & SMPLX_PP_SHORTCUT) {
        if (int e = interpolate_path(T, p, fork_test, &done)) return e;   // failure leaves the path as it was
        std::vector<double> in = p;
        if (int e = shortcut_path(T, in, p)) return e;
    }
    if (flags & SMPLX_PP_INTERPOLATE) {
        if (int e = interpolate_path(T, p, fork_test, &done)) return e;
    }
    const int np = (int)(p.size() / s->N);
    *nout = np;
    if (stats) { stats[0] = T.edge_batches; stats[1] = T.configs; }
    if (out) {
        if (np > cap) return set_error(SMPLX_E_LIMIT, "output path does not fit");
        std::memcpy(out, p.data(), sizeof(double) * p.size());
    }
    return SMPLX_OK;
}

int smplx_post_process_paths(smplx_space* const* spaces, int nq, const double* paths, const int32_t* first, int flags, double* out,
                             int cap, int32_t* out_first, int64_t* stats)
{
    if (nq < 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (nq == 0) {
        if (out_first) out_first[0] = 0;
        if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
        return SMPLX_OK;
    }
    if (!spaces || !first || !out_first || (out && cap < 0)) return set_error(SMPLX_E_ARG, "bad argument");
    long long total = 0;
    if (!smplx_path_multi::check_offsets(first, nq, &total)) return set_error(SMPLX_E_ARG, "first: nq + 1 offsets, first[0] == 0, non-decreasing");
    if (total > 0 && !paths) return set_error(SMPLX_E_ARG, "bad argument");
    for (int k = 0; k < nq; ++k) {
        if (!spaces[k]) return set_error(SMPLX_E_ARG, "null space");
        if (!same_grid_and_robot(spaces[0], spaces[k])) return set_error(SMPLX_E_ARG, "the spaces of one call share a grid, a robot model and a kernel build");
    }
    if (total > 0 && !sane_values(paths, (size_t)total * spaces[0]->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    return post_process_paths(spaces, nq, paths, first, flags, out, cap, out_first, stats);
}

int smplx_test_path_waypoints(smplx_space* s, const double* a, const double* b, int n, const int32_t* first, double* out, int32_t* counts)
{
    if (!s || !a || !b || !first || !out || !counts || n <= 0) return set_error(SMPLX_E_ARG, "bad argument");
    if (!smplx_path_multi::check_offsets(first, n, nullptr)) return set_error(SMPLX_E_ARG, "bad offsets");
    if (!sane_values(a, (size_t)n * s->N) || !sane_values(b, (size_t)n * s->N)) return set_error(SMPLX_E_ARG, "joint values must be finite (|q| < 1e6)");
    DevBuf<double> d_a, d_b, d_out;
    DevBuf<int32_t> d_first, d_counts;
    const size_t rows = (size_t)first[n];
    int e;
    if ((e = reserve(d_a, (size_t)n * s->N)) || (e = reserve(d_b, (size_t)n * s->N)) || (e = reserve(d_out, rows * s->N)) ||
        (e = reserve(d_first, (size_t)n + 1)) || (e = reserve(d_counts, (size_t)n))) return e;
    HIP_TRY(hipMemcpyAsync(d_a.p, a, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(d_b.p, b, sizeof(double) * n * s->N, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(d_first.p, first, sizeof(int32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(d_out.p, 0, sizeof(double) * (rows ? rows : 1) * s->N, s->stream));
    KLAUNCH(s, K_PATH_WAYPOINTS, k_path_waypoints, dim3((unsigned)n), dim3(SMPLX_BLOCK), s->lds_bytes, s->stream, s->d_space, d_a.p, d_b.p,
            d_first.p, d_out.p, d_counts.p);
    HIP_TRY(hipGetLastError());
    if (rows) HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(double) * rows * s->N, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(counts, d_counts.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

int smplx_search_counters(const smplx_space* s, int64_t out[16])
{
    if (!s || !out) return set_error(SMPLX_E_ARG, "null argument");
    for (int k = 0; k < 16; ++k) out[k] = 0;
    const DevSearch& D = s->ds;
    out[0] = D.searches; out[1] = D.grows; out[2] = D.dup_pushes;
    for (int k = 0; k < 7; ++k) out[3 + k] = D.ticks[k];
    out[10] = D.h.nstates;
    out[11] = search_heap_cache_entries(s, nullptr);
    out[12] = D.ticks[7] >> 32;            // evaluation rounds opened on a guess of the next pop
    out[13] = D.ticks[7] & 0xFFFFFFFFll;   // ... that the pop confirmed
    out[14] = D.table_allocs;              // empty state tables the search allocated and filled from the states' coordinates
    out[15] = s->dt.regrows;               // times the host loop's device table was outgrown and built again
    return SMPLX_OK;
}

int smplx_test_set_search_helper(smplx_space* s, int on)
{
    if (!s) return set_error(SMPLX_E_ARG, "null space");
    s->ds.test_no_helper = on == 0;
    return SMPLX_OK;
}

int smplx_test_set_search_capacity(smplx_space* s, int states)
{
    if (!s || states < 0) return set_error(SMPLX_E_ARG, "bad argument");
    s->ds.test_capacity = states;
    return SMPLX_OK;
}

int smplx_test_heap_ops(const int32_t* ops, int nops, int lds_entries, int32_t* top_after)
{
    if (!ops || !top_after || nops <= 0 || lds_entries < 1 || lds_entries > 4096) return set_error(SMPLX_E_ARG, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return set_error(SMPLX_E_HIP, "no HIP device");
    DevBuf<int32_t> d_ops, d_top;
    DevBuf<unsigned long long> d_heap;
    DevBuf<SmplxSState> d_st;
    int e;
    if ((e = reserve(d_ops, 2 * (size_t)nops))) return e;
    if ((e = reserve(d_top, (size_t)nops))) return e;
    if ((e = reserve(d_heap, (size_t)nops + 2))) return e;
    if ((e = reserve(d_st, (size_t)nops + 1))) return e;
    HIP_TRY(hipMemcpy(d_ops.p, ops, sizeof(int32_t) * 2 * (size_t)nops, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_st.p, 0, sizeof(SmplxSState) * ((size_t)nops + 1)));
    hipLaunchKernelGGL(k_heap_ops, dim3(1), dim3(64), (size_t)lds_entries * 8, 0, d_ops.p, nops, lds_entries, d_heap.p, d_st.p, d_top.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(top_after, d_top.p, sizeof(int32_t) * (size_t)nops, hipMemcpyDeviceToHost));
    return SMPLX_OK;
}

}  // extern "C"
