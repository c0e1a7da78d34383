// smpl_amd/csrc/lazy.h -- host side of the lazy successor pair: the launches of k_lazy_succs and k_true_cost
// (lazy_kernels.h), GetLazySuccs with its per-id lists (Lattice::lazy_*) and GetTrueCost with its cache
// (Lattice::true_cost).  Restates: manip_lattice.cpp:1012-1090, 1094-1167.
#pragma once

#include <algorithm>
#include <cstring>
#include <functional>
#include <utility>
#include <vector>

#include "device_table.h"
#include "kernels.h"
#include "search_host.h"
#include "space.h"

namespace {

// the refusals of smplx_get_succs: no goal, a field or a set of bodies newer than the goal; then the host's arrays catch
// up with a device search that ran on the space
int lazy_guard(smplx_space* s)
{
    if (!s->goal.set) return set_error(SMPLX_E_STATE, "goal not set");
    if (s->grid->epoch != s->goal.grid_epoch)
        return set_error(SMPLX_E_STATE, "the grid was edited after the goal was set: cached successors are stale, set the goal again");
    if (s->att.epoch != s->att.epoch_goal) return set_error(SMPLX_E_STATE, kBodiesChanged);
    return pull_lattice(s);
}

// GetLazySuccs and GetTrueCost have no way to report a failure to an SBPL caller: the first one stays on the space
int lazy_keep_status(smplx_space* s, int e)
{
    if (e != SMPLX_OK && s->status == SMPLX_OK) { s->status = e; s->status_msg = g_error; }
    return e;
}

// k_lazy_succs on device pointers (any output but d_flags may be null).  with_table: the states committed since the last
// upload are inserted in front of it, so that the ids it reads are those of every committed state.
int launch_lazy_succs(smplx_space* s, const double* d_q, int B, uint8_t* d_flags, int32_t* d_coord, double* d_sq, int32_t* d_h,
                      int32_t* d_id, hipStream_t stream, bool with_table)
{
    if (with_table) {
        if (int e = table_ensure(s)) return e;
        if (int e = table_flush(s, stream)) return e;
    } else if (s->dt.d_table) {
        if (int e = table_flush(s, stream)) return e;
    }
    KLAUNCH(s, K_LAZY_SUCCS, k_lazy_succs, dim3(blocks_for((long long)B * s->M, SMPLX_BLOCK)), dim3(SMPLX_BLOCK), s->blob_bytes, stream,
            s->d_space, d_q, B, d_flags, d_coord, d_sq, d_h, d_id);
    HIP_TRY(hipGetLastError());
    return SMPLX_OK;
}

int launch_true_cost(smplx_space* s, const double* d_pq, const int32_t* d_child, const uint8_t* d_goal, int n, double* d_work,
                     int32_t* d_cost, int32_t* d_prim, int32_t* d_nmatch, hipStream_t stream)
{
    KLAUNCH(s, K_TRUE_COST, k_true_cost, dim3(blocks_for((long long)n * SMPLX_TRUE_COST_LANES, SMPLX_BLOCK)), dim3(SMPLX_BLOCK),
            s->lds_bytes_valid, stream, s->d_space,
            d_pq, d_child, d_goal, n, d_work, d_cost, d_prim, d_nmatch);
    HIP_TRY(hipGetLastError());
    return SMPLX_OK;
}

// the dense rows of B parent states to host arrays (any may be null), synchronous.  Entries the kernel leaves alone --
// coordinate and joint values of an inactive primitive -- are zero.
int lazy_rows(smplx_space* s, const double* q, int B, uint8_t* flags, int32_t* coord, double* sq, int32_t* h, int32_t* id, bool with_table)
{
    LazyHost& Z = s->lazy;
    const size_t BM = (size_t)B * s->M, N = (size_t)s->N;
    int e;
    if ((e = reserve(Z.b_q, (size_t)B * N))) return e;
    if ((e = reserve(Z.b_sq, BM * N))) return e;
    if ((e = reserve(Z.b_coord, BM * N))) return e;
    if ((e = reserve(Z.b_h, BM))) return e;
    if ((e = reserve(Z.b_id, BM))) return e;
    if ((e = reserve(Z.b_flags, BM))) return e;
    HIP_TRY(hipMemsetAsync(Z.b_coord.p, 0, sizeof(int32_t) * BM * N, s->stream));
    HIP_TRY(hipMemsetAsync(Z.b_sq.p, 0, sizeof(double) * BM * N, s->stream));
    HIP_TRY(hipMemcpyAsync(Z.b_q.p, q, sizeof(double) * B * N, hipMemcpyHostToDevice, s->stream));
    if ((e = launch_lazy_succs(s, Z.b_q.p, B, Z.b_flags.p, Z.b_coord.p, Z.b_sq.p, Z.b_h.p, Z.b_id.p, s->stream, with_table))) return e;
    if (flags) HIP_TRY(hipMemcpyAsync(flags, Z.b_flags.p, BM, hipMemcpyDeviceToHost, s->stream));
    if (coord) HIP_TRY(hipMemcpyAsync(coord, Z.b_coord.p, sizeof(int32_t) * BM * N, hipMemcpyDeviceToHost, s->stream));
    if (sq) HIP_TRY(hipMemcpyAsync(sq, Z.b_sq.p, sizeof(double) * BM * N, hipMemcpyDeviceToHost, s->stream));
    if (h) HIP_TRY(hipMemcpyAsync(h, Z.b_h.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    if (id) HIP_TRY(hipMemcpyAsync(id, Z.b_id.p, sizeof(int32_t) * BM, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

// n items through k_true_cost, host arrays in and out (goal_edge, prims, nmatch may be null), synchronous
int true_cost_items(smplx_space* s, const double* parent_q, const int32_t* child_coord, const uint8_t* goal_edge, int n, int32_t* costs,
                    int32_t* prims, int32_t* nmatch)
{
    LazyHost& Z = s->lazy;
    const size_t N = (size_t)s->N;
    int e;
    if ((e = reserve(Z.b_q, (size_t)n * N))) return e;
    if ((e = reserve(Z.b_sq, (size_t)n * N * SMPLX_TRUE_COST_LANES))) return e;    // the kernel's work_q
    if ((e = reserve(Z.b_coord, (size_t)n * N))) return e;
    if ((e = reserve(Z.b_goal, n))) return e;
    if ((e = reserve(Z.b_out, (size_t)n * 3))) return e;
    HIP_TRY(hipMemcpyAsync(Z.b_q.p, parent_q, sizeof(double) * n * N, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(Z.b_coord.p, child_coord, sizeof(int32_t) * n * N, hipMemcpyHostToDevice, s->stream));
    if (goal_edge) HIP_TRY(hipMemcpyAsync(Z.b_goal.p, goal_edge, n, hipMemcpyHostToDevice, s->stream));
    else HIP_TRY(hipMemsetAsync(Z.b_goal.p, 0, n, s->stream));
    if ((e = launch_true_cost(s, Z.b_q.p, Z.b_coord.p, Z.b_goal.p, n, Z.b_sq.p, Z.b_out.p, Z.b_out.p + n, Z.b_out.p + 2 * (size_t)n, s->stream)))
        return e;
    HIP_TRY(hipMemcpyAsync(costs, Z.b_out.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
    if (prims) HIP_TRY(hipMemcpyAsync(prims, Z.b_out.p + n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
    if (nmatch) HIP_TRY(hipMemcpyAsync(nmatch, Z.b_out.p + 2 * (size_t)n, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return SMPLX_OK;
}

// k_lazy_succs for `id` and, in the same launch, for the hinted frontier states that have no row yet and then for the
// unevaluated states with the smallest heuristic (LazyHost::pool); the rows stay in the lattice.  A rider's row is only kept: ids are assigned when the caller's own call commits a state.
int lazy_evaluate(smplx_space* s, int id)
{
    Lattice& L = s->lat;
    const size_t M = (size_t)s->M, N = (size_t)s->N;
    std::vector<int32_t> batch(1, id);
    for (size_t k = 0; k < s->spec.hint.size() && (int)batch.size() <= s->lazy.riders; ++k) {
        const int r = s->spec.hint[k];
        if (r > 0 && r < L.size() && L.lazy_row[r] < 0 && L.lazy_off[r] < 0 && std::find(batch.begin(), batch.end(), r) == batch.end())
            batch.push_back(r);
    }
    s->spec.hint.clear();
    // no hints, or room left: the unevaluated states nearest the goal
    std::vector<std::pair<int32_t, int32_t>>& pool = s->lazy.pool;
    while (!pool.empty() && (int)batch.size() <= s->lazy.riders) {
        std::pop_heap(pool.begin(), pool.end(), std::greater<std::pair<int32_t, int32_t>>());
        const int r = pool.back().second;
        pool.pop_back();
        if (L.lazy_row[r] < 0 && L.lazy_off[r] < 0 && std::find(batch.begin(), batch.end(), r) == batch.end()) batch.push_back(r);
    }
    const size_t B = batch.size();
    std::vector<double> q(B * N);
    for (size_t i = 0; i < B; ++i) std::memcpy(&q[i * N], &L.qs[(size_t)batch[i] * N], sizeof(double) * N);
    const size_t row0 = L.lz_flags.size() / M;
    L.lz_flags.resize((row0 + B) * M);
    L.lz_coord.resize((row0 + B) * M * N);
    L.lz_q.resize((row0 + B) * M * N);
    L.lz_h.resize((row0 + B) * M);
    L.lz_known.resize((row0 + B) * M);
    const int e = lazy_rows(s, q.data(), (int)B, &L.lz_flags[row0 * M], &L.lz_coord[row0 * M * N], &L.lz_q[row0 * M * N], &L.lz_h[row0 * M],
                            &L.lz_known[row0 * M], false);
    if (e) {
        L.lz_flags.resize(row0 * M); L.lz_coord.resize(row0 * M * N); L.lz_q.resize(row0 * M * N); L.lz_h.resize(row0 * M);
        L.lz_known.resize(row0 * M);
        return e;
    }
    for (size_t i = 0; i < B; ++i) L.lazy_row[batch[i]] = (int64_t)(row0 + i);
    ++s->lazy.counters[0];
    return SMPLX_OK;
}

// GetLazySuccs (manip_lattice.cpp:1012-1090): every active action's state is created, in primitive order, with no
// limits or collision test in front; a goal successor is listed under the goal id
int get_lazy_succs(smplx_space* s, int id, const int32_t** succs, int* n)
{
    Lattice& L = s->lat;
    if (id == 0) { *n = 0; *succs = nullptr; return SMPLX_OK; }   // the goal is absorbing (:1022-1025)
    if (id < 0 || id >= L.size()) return set_error(SMPLX_E_STATE, "unknown state id");
    if (L.lazy_off[id] < 0) {
        if (L.lazy_row[id] < 0) {
            if (int e = lazy_evaluate(s, id)) return e;
        } else {
            ++s->lazy.counters[1];
        }
        const size_t M = (size_t)s->M, N = (size_t)s->N, row = (size_t)L.lazy_row[id];
        const int64_t off = (int64_t)L.lazy_succ.size();
        for (size_t pi = 0; pi < M; ++pi) {
            const size_t k = row * M + pi;
            const int f = L.lz_flags[k];
            if (f & SMPLX_F_INACTIVE) continue;
            const int32_t* c = &L.lz_coord[k * N];
            // the device table holds committed states only: a hit is final; a miss goes through the host's table
            int sid = L.lz_known[k] >= 0 ? L.lz_known[k] : L.table.find(c, L.coords);
            if (sid < 0) {
                sid = new_state(s, c, &L.lz_q[k * N], L.lz_h[k]);
                if (s->lazy.riders > 0 && !(f & SMPLX_F_GOAL)) {
                    s->lazy.pool.emplace_back(L.lz_h[k], sid);
                    std::push_heap(s->lazy.pool.begin(), s->lazy.pool.end(), std::greater<std::pair<int32_t, int32_t>>());
                }
            }
            const bool goal = (f & SMPLX_F_GOAL) != 0;
            L.lazy_succ.push_back(goal ? 0 : sid);
            L.lazy_goal.push_back(goal ? 1 : 0);
            L.lazy_prim.push_back((int32_t)pi);
        }
        L.lazy_off[id] = off;
        L.lazy_cnt[id] = (int32_t)((int64_t)L.lazy_succ.size() - off);
        s->lazy.recent.push_back(id);
    } else {
        ++s->lazy.counters[1];
    }
    *n = L.lazy_cnt[id];
    *succs = L.lazy_succ.data() + L.lazy_off[id];
    return SMPLX_OK;
}

inline uint64_t true_cost_key(int parent, int child) { return (uint64_t)(uint32_t)parent << 32 | (uint32_t)child; }

int true_cost_check_ids(const smplx_space* s, int parent, int child)
{
    if (parent == 0) return set_error(SMPLX_E_ARG, "the goal id has no coordinate: it is nobody's parent");
    if (parent < 0 || parent >= s->lat.size() || child < 0 || child >= s->lat.size()) return set_error(SMPLX_E_STATE, "unknown state id");
    return SMPLX_OK;
}

// GetTrueCost (manip_lattice.cpp:1094-1167) for n pairs: the pairs the cache does not hold go through k_true_cost in one
// launch -- with `ride`, the unevaluated edges of the parents' lazy lists and of the lists committed last beside them --
// and into the cache
int true_cost_pairs(smplx_space* s, const int32_t* parents, const int32_t* children, int n, int32_t* costs, int32_t* prims, int32_t* nmatch,
                    bool ride)
{
    Lattice& L = s->lat;
    const size_t N = (size_t)s->N;
    for (int i = 0; i < n; ++i)
        if (int e = true_cost_check_ids(s, parents[i], children[i])) return e;
    std::vector<uint64_t> keys;
    std::vector<double> pq;
    std::vector<int32_t> cc;
    std::vector<uint8_t> ge;
    const Lattice::TrueCost pending = {0, 0, -1};      // nmatch -1: queued in this call
    auto queue = [&](int parent, int child) {
        const uint64_t key = true_cost_key(parent, child);
        if (!L.true_cost.emplace(key, pending).second) return false;
        keys.push_back(key);
        pq.insert(pq.end(), &L.qs[(size_t)parent * N], &L.qs[(size_t)parent * N] + N);
        if (child == 0) cc.insert(cc.end(), N, 0);
        else cc.insert(cc.end(), &L.coords[(size_t)child * N], &L.coords[(size_t)child * N] + N);
        ge.push_back(child == 0 ? 1 : 0);
        return true;
    };
    for (int i = 0; i < n; ++i) {
        if (!queue(parents[i], children[i])) {
            if (L.true_cost[true_cost_key(parents[i], children[i])].nmatch >= 0) ++s->lazy.counters[4];
            continue;
        }
        ++s->lazy.counters[5];
        if (!ride) continue;
        auto ride_list = [&](int p) {
            if (L.lazy_off[p] >= 0)
                for (int k = 0; k < L.lazy_cnt[p]; ++k) queue(p, L.lazy_succ[L.lazy_off[p] + k]);
        };
        ride_list(parents[i]);
        const std::vector<int32_t>& recent = s->lazy.recent;
        for (size_t k = recent.size(); k > 0 && recent.size() - k < (size_t)s->lazy.ride_parents; --k) ride_list(recent[k - 1]);
    }
    if (!keys.empty()) {
        const int m = (int)keys.size();
        std::vector<int32_t> out((size_t)m * 3);
        if (int e = true_cost_items(s, pq.data(), cc.data(), ge.data(), m, &out[0], &out[m], &out[2 * (size_t)m])) {
            for (uint64_t k : keys) L.true_cost.erase(k);
            return e;
        }
        for (int k = 0; k < m; ++k) L.true_cost[keys[k]] = Lattice::TrueCost{out[k], out[m + k], out[2 * (size_t)m + k]};
        ++s->lazy.counters[2];
        s->lazy.counters[3] += m;
    }
    for (int i = 0; i < n; ++i) {
        const Lattice::TrueCost& r = L.true_cost[true_cost_key(parents[i], children[i])];
        costs[i] = r.cost;
        if (prims) prims[i] = r.prim;
        if (nmatch) nmatch[i] = r.nmatch;
    }
    return SMPLX_OK;
}

}  // namespace
