// smpl_amd/csrc/lazy_kernels.h -- the lazy successor pair of ManipLattice.
// Owns: k_lazy_succs (GetLazySuccs, manip_lattice.cpp:1012-1090: everything of an expansion but the checks) and
// k_true_cost (GetTrueCost, manip_lattice.cpp:1094-1167: only the checks, for one (parent, child) pair an item).
// Both are built from the GetSuccs steps of lattice_steps.h and the edge check of config_checks.h; nothing is restated.
#pragma once

#include "config_checks.h"
#include "lattice_steps.h"

// One thread per (state, primitive); a block's 128 consecutive edges belong to at most 128 states, whose goal distances --
// planning-link FK and one BFS cell each -- are worked out once, by the block's first threads, and shared through LDS.
// Then per edge: gate, successor joint values, discretisation, goal test with the heuristic, table probe.  No limits test,
// no grid lookup for collision, no per-thread scratch: the dynamic LDS is the model image alone.
// The table is probed with plain loads: the inserts of the states committed so far ran in an earlier launch
// (k_table_insert).  Any output but out_flags may be null.
extern "C" __global__ void __launch_bounds__(BLOCK)
k_lazy_succs(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int B, unsigned char* __restrict__ out_flags,
             int* __restrict__ out_coord, double* __restrict__ out_q, int* __restrict__ out_h, int* __restrict__ out_id)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ double goal_dist[BLOCK];
    const ModelLds Mv = setup_model_only(S, smem);
    const ModelLds* M = &Mv;
    const SmplxActionsDev& A = S->actions;
    const SmplxGridDev grid = S->grid;
    const SmplxBfsDev bfs = S->bfs;
    const int nprims = A.nprims;
    const int nv = MV_NVARS(M);
    const long long total = (long long)B * nprims;
    const long long first = (long long)blockIdx.x * BLOCK;
    const long long tid = first + threadIdx.x;
    const long long last = (first + BLOCK < total ? first + BLOCK : total) - 1;   // the block's last edge (first <= last: the grid covers `total`)
    const int s0 = (int)(first / nprims), s1 = (int)(last / nprims);
    if (s0 + (int)threadIdx.x <= s1) goal_dist[threadIdx.x] = metric_goal_distance(M, grid, bfs, Q + (size_t)(s0 + threadIdx.x) * nv);
    __syncthreads();
    if (tid >= total) return;
    const int si = (int)(tid / nprims);
    const int pi = (int)(tid - (long long)si * nprims);
    const MprimGate gate = mprim_gate(A, A.type[pi]);
    double sq[SMPLX_MAX_VARS];
    int sc[SMPLX_MAX_VARS];
    bool have_action = false;
    if (mprim_active(gate, goal_dist[si - s0])) have_action = successor_values(M, A, S->goal, pi, Q + (size_t)si * nv, sq);
    int flags = SMPLX_F_INACTIVE, h = 0, id = -1;
    if (have_action) {
        MV_UNROLL
        for (int v = 0; v < nv; ++v) sc[v] = var_to_coord(M, v, sq[v]);
        const TableSlotWords probe = table_probe_issue(S->table, sc, nv);   // its loads fly under the FK of the goal test
        bool is_goal;
        h = successor_goal_h(M, S->goal, bfs, grid, sq, sc, is_goal);
        id = table_probe_resolve(S->table, sc, nv, probe);
        flags = SMPLX_F_UNCHECKED | (is_goal ? SMPLX_F_GOAL : 0);
        MV_UNROLL
        for (int v = 0; v < nv; ++v) {
            if (out_q) out_q[tid * nv + v] = sq[v];
            if (out_coord) out_coord[tid * nv + v] = sc[v];
        }
    }
    out_flags[tid] = (unsigned char)flags;
    if (out_h) out_h[tid] = h;
    if (out_id) out_id[tid] = id;
}

// SMPLX_TRUE_COST_LANES = 8 neighbouring lanes per item, 16 items a block.  item i: the parent's joint values Pq[i], and
// either the child's coordinate child_coord[i] or, with goal_edge[i] != 0, the mark "the child is the goal".
// The lanes of an item do the cheap part alike and share the dear one.  Alike: the parent's goal distance, and the parent's
// primitives re-applied in order with GetSuccs' gating, noting, one bit a primitive (SMPLX_MAX_PRIMS = 64), which actions
// match -- those whose coordinate equals the child's in every variable (goal edge: those for which isGoal holds).  Shared:
// the matches in ascending order, until one passes, go through checkAction (manip_lattice.cpp:1511-1580) -- joint limits,
// then the edge parent -> successor, attached bodies included, lane l taking waypoints l, l + 8, ... of the edge through
// config_valid (config_checks.h), each lane over its own LDS scratch as in k_edge_valid; three shuffles join the verdicts.
// An edge is valid iff every waypoint is (collision_space.cpp:561-577), so the verdict is edge_valid's.
// Why this shape and not one thread an item: a thread that walks an edge alone takes W
// configuration checks one after another, and GetTrueCost is asked for a handful of edges at a time, so that walk is the
// whole latency of a call; and with the check inside the primitive loop a wave whose 64 items matched 20 different
// primitives ran 20 edge checks one after another (4.6 times k_edge_valid on the edges of cfg 2, measured).
// out_cost 1000 or -1, out_prim the lowest matching primitive that passed or -1, out_nmatch the matching actions.
// work_q: SMPLX_TRUE_COST_LANES * n rows of nvars doubles, each lane's copy of the candidate successor (config_valid reads
// the edge's end point from memory).
extern "C" __global__ void __launch_bounds__(BLOCK, 2)   // >= 2 waves per SIMD: at most 256 VGPRs, whichever compiler builds it
k_true_cost(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Pq, const int* __restrict__ child_coord,
            const unsigned char* __restrict__ goal_edge, int n, double* __restrict__ work_q, int* __restrict__ out_cost,
            int* __restrict__ out_prim, int* __restrict__ out_nmatch)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ModelLds Mv;
#ifdef SMPLX_CONST_MODEL
    constexpr bool RS = true;      // as k_edge_valid
#else
    constexpr bool RS = false;
#endif
    ThreadLds L = setup_lds(S, smem, &Mv, BLOCK, !RS);
    const ModelLds* M = &Mv;
    static_assert(BLOCK % SMPLX_TRUE_COST_LANES == 0 && 64 % SMPLX_TRUE_COST_LANES == 0, "the lanes of an item lie in one wave");
    const long long t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const int i = (int)(t / SMPLX_TRUE_COST_LANES);
    const int lane = (int)threadIdx.x % SMPLX_TRUE_COST_LANES;
    if (i >= n) return;            // (all lanes of an item alike)
    const SmplxActionsDev& A = S->actions;
    const SmplxGridDev grid = S->grid;
    const SmplxBfsDev bfs = S->bfs;
    const int nprims = A.nprims;
    const int nv = MV_NVARS(M);
    const double* parent = Pq + (size_t)i * nv;
    double* sq = work_q + (size_t)t * nv;
    const bool to_goal = goal_edge[i] != 0;
    int child[SMPLX_MAX_VARS];
    MV_UNROLL
    for (int v = 0; v < nv; ++v) child[v] = to_goal ? 0 : child_coord[(size_t)i * nv + v];
    const double gd = metric_goal_distance(M, grid, bfs, parent);
    unsigned long long matches = 0;
    for (int pi = 0; pi < nprims; ++pi) {
        double cand[SMPLX_MAX_VARS];
        if (!mprim_active(A, gd, A.type[pi])) continue;
        if (!successor_values(M, A, S->goal, pi, parent, cand)) continue;
        int sc[SMPLX_MAX_VARS];
        int differ = 0;
        MV_UNROLL
        for (int v = 0; v < nv; ++v) { sc[v] = var_to_coord(M, v, cand[v]); differ |= sc[v] ^ child[v]; }
        bool match = differ == 0;
        if (to_goal) (void)successor_goal_h(M, S->goal, bfs, grid, cand, sc, match);
        if (match) matches |= 1ull << pi;
    }
    const int nmatch = __popcll(matches);
    int cost = -1, prim = -1;
    while (matches != 0 && cost < 0) {
        const int pi = __ffsll((long long)matches) - 1;
        matches &= matches - 1;
        (void)successor_values(M, A, S->goal, pi, parent, sq);
        if (!check_joint_limits(M, sq)) continue;
        // isStateToStateValid (collision_space.cpp:538-581) with the waypoints dealt out: W == 0, no motion, is valid
        const int W = edge_waypoint_count(M, parent, sq);
        int bad = 0, lk = 0;
        if (W > 0) {
            const double inv = 1.0 / (double)(W - 1);
            EdgeRef e;
            e.start = parent;
            e.finish = sq;
            for (int j = lane; j < W && !bad; j += SMPLX_TRUE_COST_LANES) {
                e.alpha = (double)j * inv;
                if (!config_valid<RS>(M, L, grid, e, lk)) bad = 1;
            }
        }
        // every lane of the item is here (matches and cost are the same in all of them): the verdicts joined
#pragma unroll
        for (int m = 1; m < SMPLX_TRUE_COST_LANES; m <<= 1) bad |= __shfl_xor(bad, m);
        if (bad) continue;
        cost = SMPLX_LAZY_COST;
        prim = pi;
    }
    if (lane != 0) return;
    out_cost[i] = cost;
    if (out_prim) out_prim[i] = prim;
    if (out_nmatch) out_nmatch[i] = nmatch;
}
