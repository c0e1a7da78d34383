// smpl_amd/csrc/small_batch.h -- one block per state: small frontier batches, and the pieces k_search is built from.
// Owns: ExpandLds, the lane functions (expand_config_lane, expand_book_*, expand_verdict), SMPLX_WAVE_SYNC,
// expand_state_block and k_small_batch.  search_kernel.h builds the rounds of k_search from the lane functions (round_prepare,
// search_book_table there).
// Restates: manip_lattice.cpp:254-305 (the GetSuccs loop body, in lane-sized pieces).
#pragma once

#include "config_checks.h"
#include "lattice_steps.h"

// ---------------------------------------------------------------------------------------------
// Small frontier batches (a search that misses on a handful of states) and the device-resident search (k_search): ONE
// block evaluates ONE state, because at this size the cost is launch + dependency latency, not throughput.
// Every WAVE of the block has one role, so that no wave runs two long code paths one after the other:
//   config waves   lanes 0 .. 7 M - 1: lane (p, k) checks waypoints k+1, k+8, ... of edge p (an edge with more than
//                  7 waypoints after the start wraps around its lanes); lane 7 M: the state itself (waypoint 0 of
//                  every edge).  One configuration per lane, one code path per wave.
//   last wave      lane p < M: the successor of primitive p -- joint values, limits, coordinates, planning-link FK,
//                  goal test, heuristic, and at the end the verdict; lane M: the state's metric goal distance (the gate
//                  of the primitives).
// The goal distance is computed first (one lane, while the successor joint values are formed): only the primitives it
// activates have their waypoints checked -- an ungated snap-to-goal primitive is an edge of a hundred waypoints, 15
// configurations in sequence on each of its 7 lanes (measured in round 2: 104 us per launch instead of 22).
// Results are identical to the pipeline.
// ---------------------------------------------------------------------------------------------
#define SMPLX_SMALL_LANES 7   // waypoint lanes per edge

// what one block-level expansion leaves in LDS (static shared memory of the calling kernel)
struct ExpandLds {
    double goal_dist;
    int state_bad, state_lookups;
    double parent[SMPLX_MAX_VARS];
    double sq[SMPLX_MAX_PRIMS][SMPLX_MAX_VARS];   // successor joint values of every primitive
    int coord[SMPLX_MAX_PRIMS][SMPLX_MAX_VARS];   // defined where flags has the valid bit
    int edge_bad[SMPLX_MAX_PRIMS], edge_lk[SMPLX_MAX_PRIMS];
    int h[SMPLX_MAX_PRIMS], lookups[SMPLX_MAX_PRIMS];
    int flags[SMPLX_MAX_PRIMS];
};

// ---- the GetSuccs loop body (manip_lattice.cpp:254-305) in lane-sized pieces; expand_state_block (k_small_batch) and
// k_search (search_kernel.h) put them together around their own barriers ----

// config lane c of the block: c < ncfg - 1: lane (p, slot) checks waypoints slot+1, slot+8, ... of edge p (an edge longer
// than 7 waypoints wraps around its lanes); c == ncfg - 1: the state itself (waypoint 0 of every edge)
template <bool RS = false>
__device__ __forceinline__ void expand_config_lane(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxActionsDev& A,
                                                   const SmplxGoalDev& G, const SmplxGridDev& grid, ExpandLds& X, int c, int ncfg)
{
    const double* parent = X.parent;
    if (c < ncfg - 1) {
        const int p = c / SMPLX_SMALL_LANES, slot = c % SMPLX_SMALL_LANES;
        if (prim_has_action(A, G, p) && mprim_active(A, X.goal_dist, A.type[p])) {
            const double* sq = X.sq[p];
            if (check_joint_limits(M, sq)) {
                const int Wc = edge_waypoint_count(M, parent, sq);
                int my_bad = 0, my_lk = 0;
                for (int wp = slot + 1; wp < Wc && !my_bad; wp += SMPLX_SMALL_LANES) {
                    EdgeRef e;
                    e.start = parent; e.finish = sq;
                    e.alpha = (double)wp * (1.0 / (double)(Wc - 1));
                    const bool ok = config_valid<RS>(M, L, grid, e, my_lk);
                    my_bad = ok ? 0 : 1;
                }
                if (my_bad) atomicOr(&X.edge_bad[p], 1);
                if (my_lk) atomicAdd(&X.edge_lk[p], my_lk);
            }
        }
    } else if (c == ncfg - 1) {
        EdgeRef e;
        e.start = parent; e.finish = parent; e.alpha = 0.0;
        int lk = 0;
        const bool ok = config_valid<RS>(M, L, grid, e, lk);
        if (!ok) atomicOr(&X.state_bad, 1);
        if (lk) atomicAdd(&X.state_lookups, lk);
    }
}

// bookkeeping lane of primitive p, behind successor_values, in two steps: (i) limits, waypoint count, coordinates (-> X.coord[p]);
// (ii) planning-link FK, goal test, heuristic.  (k_search starts the state-table probe of the coordinate between the two.)
struct BookLane { bool limits_ok; int W, h, is_goal; };
__device__ __forceinline__ void expand_book_coords(const ModelLds* __restrict__ M, ExpandLds& X, int p, BookLane& r)
{
    const int nv = MV_NVARS(M);
    r.W = 0; r.h = 0; r.is_goal = 0;
    const double* sq = X.sq[p];
    r.limits_ok = check_joint_limits(M, sq);
    if (r.limits_ok) {
        r.W = edge_waypoint_count(M, X.parent, sq);
        MV_UNROLL
        for (int v = 0; v < nv; ++v) X.coord[p][v] = var_to_coord(M, v, sq[v]);
    }
}
__device__ __forceinline__ void expand_book_goal(const ModelLds* __restrict__ M, const SmplxGridDev& grid, const SmplxBfsDev& bfs,
                                                 const SmplxGoalDev& G, const ExpandLds& X, int p, BookLane& r)
{
    if (!r.limits_ok) return;
    bool is_goal;
    r.h = successor_goal_h(M, G, bfs, grid, X.sq[p], X.coord[p], is_goal);
    r.is_goal = is_goal;
}
__device__ __forceinline__ BookLane expand_book_lane(const ModelLds* __restrict__ M, const SmplxGridDev& grid, const SmplxBfsDev& bfs,
                                                     const SmplxGoalDev& G, ExpandLds& X, int p)
{
    BookLane r;
    expand_book_coords(M, X, p, r);
    expand_book_goal(M, grid, bfs, G, X, p, r);
    return r;
}

// the verdict of edge p once the waypoint lanes have reported: SMPLX_F_* flags; lookups = the reference's tally for the edge
__device__ __forceinline__ int expand_verdict(const SmplxActionsDev& A, const ExpandLds& X, int p, bool have_action, const BookLane& b,
                                              int& lookups)
{
    lookups = 0;
    if (!have_action || !mprim_active(A, X.goal_dist, A.type[p])) return SMPLX_F_INACTIVE;
    if (!b.limits_ok) return SMPLX_F_LIMITS;
    lookups = X.edge_lk[p] + (b.W > 0 ? X.state_lookups : 0);
    const bool ok = (b.W == 0) || (X.state_bad == 0 && X.edge_bad[p] == 0);
    if (!ok) return SMPLX_F_COLLISION;
    return SMPLX_F_VALID | (b.is_goal ? SMPLX_F_GOAL : 0);
}

// lanes of ONE wave exchange data through LDS: no block barrier needed, only that neither the compiler nor the memory
// pipeline reorders the accesses (LDS operations of a wave execute in order)
#define SMPLX_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); \
                               __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

// The whole loop body for the state whose joint values are at parent_src (HBM or pinned host memory), by all threads of the
// block (blockDim.x = smplx_small_block(nprims)).  The bookkeeping wave loads the parent itself and starts at once; the
// other waves join at the first of three barriers.  Ends with a barrier: on return X.parent, X.flags, X.sq, X.coord, X.h,
// X.lookups, X.goal_dist, X.state_bad and X.state_lookups are final.
__device__ __forceinline__ void expand_state_block(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxSpaceDev* __restrict__ S,
                                                   const SmplxSpaceDev* __restrict__ Sq, const SmplxGridDev& grid, ExpandLds& X,
                                                   const double* __restrict__ parent_src)
{
    const SmplxActionsDev& A = S->actions;
    const SmplxBfsDev bfs = Sq->bfs;
    const int nprims = A.nprims, nv = MV_NVARS(M);
    const int t = threadIdx.x;
    const int ncfg = nprims * SMPLX_SMALL_LANES + 1;          // config lanes (the last one: the state itself)
    const int book0 = (ncfg + 63) / 64 * 64;                  // first lane of the bookkeeping wave
    if (t < nprims) { X.edge_bad[t] = 0; X.edge_lk[t] = 0; }
    if (t == 0) { X.state_bad = 0; X.state_lookups = 0; }
    const int bp = t - book0;                                 // primitive of a bookkeeping lane
    const bool book = bp >= 0 && bp < nprims;
    if (bp >= 0) {
        if (bp < nv) X.parent[bp] = parent_src[bp];
        SMPLX_WAVE_SYNC();
    }
    const bool have_action = book && successor_values(M, A, Sq->goal, bp, X.parent, X.sq[bp]);
    if (bp == nprims) X.goal_dist = metric_goal_distance(M, grid, bfs, X.parent);
    __syncthreads();   // every lane of every edge can read its successor's joint values and the gate from LDS
    BookLane b;
    b.limits_ok = false; b.W = 0; b.h = 0; b.is_goal = 0;
    if (t < book0) expand_config_lane(M, L, A, Sq->goal, grid, X, t, ncfg);
    else if (have_action) b = expand_book_lane(M, grid, bfs, Sq->goal, X, bp);
    __syncthreads();   // the waypoint verdicts and the state's own check have landed in LDS
    if (book) {
        int lookups;
        const int flags = expand_verdict(A, X, bp, have_action, b, lookups);
        X.flags[bp] = flags;
        X.h[bp] = (flags & SMPLX_F_VALID) ? b.h : 0;
        X.lookups[bp] = lookups;
    }
    __syncthreads();
}

extern "C" __global__ void __launch_bounds__(512)
k_small_batch(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int B,
              double* __restrict__ goal_dist_out, unsigned char* __restrict__ state_bad_out, int* __restrict__ state_lookups_out,
              unsigned char* __restrict__ out_flags, int* __restrict__ out_coord, double* __restrict__ out_q,
              int* __restrict__ out_h, int* __restrict__ out_cost, int* __restrict__ out_lookups,
              const SmplxSpaceDev* const* __restrict__ stab, const unsigned short* __restrict__ state_q,
              unsigned char* __restrict__ host_flags, int* __restrict__ host_coord, double* __restrict__ host_q,
              int* __restrict__ host_h, int* __restrict__ out_id, int* __restrict__ host_id,
              const int* __restrict__ ins_items, int n_ins)
{
    // host_*: optional pinned host buffers the results are ALSO written to (zero-copy: a small batch costs less
    // as a few KB of PCIe stores than as DMA copies); Q may itself be pinned host memory -- the parent's
    // joint values are staged into LDS once per block
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ ExpandLds X;
    if (n_ins > 0 && table_insert_block(S, stab, ins_items, n_ins, B)) return;   // K5: see k_pipe_prep
    ModelLds Mv;
    ThreadLds L = setup_lds(S, smem, &Mv, blockDim.x);
    const ModelLds* M = &Mv;
    const SmplxActionsDev& A = S->actions;
    const SmplxGridDev grid = S->grid;
    const long long si = blockIdx.x;
    const SmplxSpaceDev* Sq = stab ? stab[state_q[si]] : S;
    const int nprims = A.nprims, nv = MV_NVARS(M);
    const int t = threadIdx.x;
    expand_state_block(M, L, S, Sq, grid, X, Q + si * nv);
    if (t == 0) { goal_dist_out[si] = X.goal_dist; state_bad_out[si] = (unsigned char)X.state_bad; state_lookups_out[si] = X.state_lookups; }
    if (t < nprims) {
        const long long eid = si * nprims + t;
        const int flags = X.flags[t];
        out_flags[eid] = (unsigned char)flags;
        out_h[eid] = X.h[t];
        out_cost[eid] = (flags & SMPLX_F_VALID) ? A.cost[t] : 0;
        out_lookups[eid] = X.lookups[t];
        const bool active = !(flags & SMPLX_F_INACTIVE);
        if (active) {
            MV_UNROLL
            for (int v = 0; v < nv; ++v) out_q[eid * nv + v] = X.sq[t][v];
        }
        int sid = -1;
        if (flags & SMPLX_F_VALID) {
            MV_UNROLL
            for (int v = 0; v < nv; ++v) out_coord[eid * nv + v] = X.coord[t][v];
            if (out_id) sid = table_lookup<true>(Sq->table, X.coord[t], nv);   // K5: device copy of the state table (see k_pipe_finish)
        }
        if (out_id) out_id[eid] = sid;
        if (host_flags) {
            host_flags[eid] = (unsigned char)flags;
            if (host_id) host_id[eid] = sid;
            if (flags & SMPLX_F_VALID) {
                host_h[eid] = X.h[t];
                MV_UNROLL
                for (int v = 0; v < nv; ++v) { host_coord[eid * nv + v] = X.coord[t][v]; host_q[eid * nv + v] = X.sq[t][v]; }
            }
        }
    }
}
