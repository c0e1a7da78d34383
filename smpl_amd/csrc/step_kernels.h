// smpl_amd/csrc/step_kernels.h -- the kernels of a frontier step.
// Owns: the fused pair k_state_prep + k_expand (one thread walks a whole edge: expand_edge) with tally_block, and the
// waypoint-parallel pipeline, which is the default: k_pipe_setup, k_pipe_configs, k_pipe_finish, with k_pipe_prep in
// front for the four-launch mode, and their helpers (pipe_edge_values, successor_coords, pipe_successor, pipe_successor_role).  The one-launch
// form of the pipeline for a batch that is resident in one round, k_step_block, is in step_block.h and built from the same
// helpers.
// Restates: manip_lattice.cpp:254-305, 1471-1535 (the GetSuccs loop body); manip_lattice_action_space.cpp:385-397;
// collision_space.cpp:561-577.
#pragma once

#include "config_checks.h"
#include "lattice_steps.h"

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(BLOCK, 2)   // >= 2 waves per SIMD: at most 256 VGPRs, whichever compiler builds it
k_state_prep(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int B,
             double* __restrict__ goal_dist, unsigned char* __restrict__ parent_valid, int* __restrict__ parent_lookups,
        const SmplxSpaceDev* const* __restrict__ stab, const unsigned short* __restrict__ state_q)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ModelLds Mv;
    ThreadLds L = setup_lds(S, smem, &Mv);
    const ModelLds* M = &Mv;
    const SmplxGridDev grid = S->grid;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= B) return;
    const SmplxBfsDev bfs = (stab ? stab[state_q[i]] : S)->bfs;   // per-query data in a cross-query batch
    const double* q = Q + (int64_t)i * MV_NVARS(M);
    goal_dist[i] = metric_goal_distance(M, grid, bfs, q);
    EdgeRef e;
    e.start = q; e.finish = q; e.alpha = 0.0;
    int lk = 0;
    const bool ok = config_valid(M, L, grid, e, lk);
    parent_valid[i] = ok ? 1 : 0;
    parent_lookups[i] = lk;
}

// per-block tallies without atomics: block b owns counters[4*b .. 4*b+3] (launches on one stream serialise,
// so a plain read-modify-write is safe); the host sums the blocks (smplx_counters_read).  WAVES: waves of the block.
template <int WAVES = BLOCK / 64>
__device__ __forceinline__ void tally_block(unsigned long long* __restrict__ counters, int ev, int va, int lk, int pf,
                                            int cfgs, int slk)
{
    __shared__ int t_acc[WAVES][SMPLX_TALLIES];
    const int wv = threadIdx.x >> 6;
    for (int off = 32; off > 0; off >>= 1) {
        lk += __shfl_down(lk, off); pf += __shfl_down(pf, off); cfgs += __shfl_down(cfgs, off); slk += __shfl_down(slk, off);
    }
    if ((threadIdx.x & 63) == 0) {
        t_acc[wv][0] = ev; t_acc[wv][1] = va; t_acc[wv][2] = lk; t_acc[wv][3] = pf; t_acc[wv][4] = cfgs; t_acc[wv][5] = slk;
    }
    __syncthreads();
    if (threadIdx.x < SMPLX_TALLIES) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < WAVES; ++k) v += t_acc[k][threadIdx.x];
        counters[(size_t)blockIdx.x * SMPLX_TALLIES + threadIdx.x] += (unsigned long long)v;
    }
}

// One (state, primitive) pair through the whole GetSuccs loop body in ONE thread (manip_lattice.cpp:1471-1535):
// gating, successor joint values, limits, the edge's waypoints in the reference's order, discretisation, goal test,
// heuristic.  parent_ok / parent_lk: result of the state's own check (waypoint 0 of every edge).
struct EdgeTally { int flags, lookups, performed, evaluated; };

__device__ __forceinline__ EdgeTally expand_edge(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxSpaceDev* __restrict__ S,
                                                 const SmplxSpaceDev* __restrict__ Sq, const SmplxGridDev& grid,
                                                 const double* __restrict__ Q, long long tid,
                                                 const double* __restrict__ goal_dist, bool parent_ok, int parent_lk,
                                                 unsigned char* __restrict__ out_flags, int* __restrict__ out_coord,
                                                 double* __restrict__ out_q, int* __restrict__ out_h, int* __restrict__ out_cost,
                                                 int* __restrict__ out_lookups)
{
    const SmplxActionsDev& A = S->actions;
    const int nprims = A.nprims;
    int flags = SMPLX_F_INACTIVE;
    int lookups = 0;
    int performed = 0;   // lookups this thread itself issued (waypoints >= 1)
    int evaluated = 0;
    {
        const int si = (int)(tid / nprims);
        const int pi = (int)(tid - (long long)si * nprims);
        const int nv = MV_NVARS(M);
        const double* parent = Q + (int64_t)si * nv;
        double* sq = out_q + tid * nv;
        int* sc = out_coord + tid * nv;
        const SmplxBfsDev bfs = Sq->bfs;
        int h = 0, cost = 0;
        bool have_action = false;
        if (mprim_active(A, goal_dist[si], A.type[pi])) have_action = successor_values(M, A, Sq->goal, pi, parent, sq);
        if (have_action) {
            evaluated = 1;
            flags = 0;
            if (!check_joint_limits(M, sq)) {
                flags = SMPLX_F_LIMITS;
            } else {
                int W = 0;
                int lk = 0;
                const bool ok = edge_valid(M, L, grid, parent, sq, true, parent_ok, lk, W);
                lookups = lk;
                performed = lk;
                if (W > 0) lookups += parent_lk;   // waypoint 0, done once per state
                if (!ok) {
                    flags = SMPLX_F_COLLISION;
                } else {
                    MV_UNROLL
                    for (int v = 0; v < nv; ++v) sc[v] = var_to_coord(M, v, sq[v]);
                    bool is_goal;
                    h = successor_goal_h(M, Sq->goal, bfs, grid, sq, sc, is_goal);
                    cost = A.cost[pi];
                    flags = SMPLX_F_VALID | (is_goal ? SMPLX_F_GOAL : 0);
                }
            }
        }
        out_flags[tid] = (unsigned char)flags;
        out_h[tid] = h;
        out_cost[tid] = cost;
        out_lookups[tid] = lookups;
    }
    EdgeTally t;
    t.flags = flags; t.lookups = lookups; t.performed = performed; t.evaluated = evaluated;
    return t;
}

extern "C" __global__ void __launch_bounds__(BLOCK, 2)   // >= 2 waves per SIMD: at most 256 VGPRs, whichever compiler builds it
k_expand(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int B,
         const double* __restrict__ goal_dist, const unsigned char* __restrict__ parent_valid,
         const int* __restrict__ parent_lookups,
         unsigned char* __restrict__ out_flags, int* __restrict__ out_coord, double* __restrict__ out_q,
         int* __restrict__ out_h, int* __restrict__ out_cost, int* __restrict__ out_lookups,
         unsigned long long* __restrict__ counters, const int* __restrict__ deferred_count,
        const SmplxSpaceDev* const* __restrict__ stab, const unsigned short* __restrict__ state_q)
{
    extern __shared__ __align__(16) unsigned char smem[];
    // second pass after the pipeline / the small-batch kernel (deferred_count != nullptr): nothing to do in the
    // common case.  deferred_count[0] < 0 means "no counter kept": the block looks at its own flags instead.
    const bool only_deferred = deferred_count != nullptr;
    if (only_deferred) {
        const int cnt = deferred_count[0];
        if (cnt == 0) return;
        if (cnt < 0) {
            const long long tid0 = (long long)blockIdx.x * BLOCK + threadIdx.x;
            const int mine = (tid0 < (long long)B * S->actions.nprims) ? (out_flags[tid0] & SMPLX_F_DEFERRED) : 0;
            if (!__syncthreads_or(mine)) return;
        }
    }
    ModelLds Mv;
    const SmplxActionsDev& A = S->actions;
    ThreadLds L = setup_lds(S, smem, &Mv);
    const ModelLds* M = &Mv;
    const SmplxGridDev grid = S->grid;
    const int nprims = A.nprims;
    const long long tid = (long long)blockIdx.x * BLOCK + threadIdx.x;
    bool in_range = tid < (long long)B * nprims;
    // second pass after the pipeline: only the edges it deferred (they did not fit the work list)
    if (only_deferred && in_range && !(out_flags[tid] & SMPLX_F_DEFERRED)) in_range = false;
    int flags = SMPLX_F_INACTIVE;
    int lookups = 0;
    int performed = 0;   // lookups this kernel itself issued (waypoints >= 1)
    int evaluated = 0;
    if (in_range) {
        const int si = (int)(tid / nprims);
        const SmplxSpaceDev* Sq = stab ? stab[state_q[si]] : S;   // per-query goal and BFS grid
        // fused mode: parent_valid holds 1 = valid (k_state_prep); deferred pass: the pipeline's state_bad (1 = bad)
        const bool pv = only_deferred ? parent_valid[si] == 0 : parent_valid[si] != 0;
        const EdgeTally t = expand_edge(M, L, S, Sq, grid, Q, tid, goal_dist, pv, parent_lookups[si], out_flags, out_coord,
                                        out_q, out_h, out_cost, out_lookups);
        flags = t.flags; lookups = t.lookups; performed = t.performed; evaluated = t.evaluated;
    }
    // per-wave tallies: ballots instead of one atomic per lane
    if (counters) {
        const unsigned long long m_eval = __ballot(evaluated);
        const unsigned long long m_valid = __ballot((flags & SMPLX_F_VALID) != 0);
        tally_block(counters, __popcll(m_eval), __popcll(m_valid), lookups, performed, 0, 0);
    }
}

// ---------------------------------------------------------------------------------------------
// Waypoint-parallel pipeline (default).  The fused k_expand above walks an edge's waypoints one
// after another inside one thread, which leaves the chip idle at B = 4096 (about 1.6 waves per
// SIMD, each a serial fp64 chain).  The pipeline spreads the same work over (edge, waypoint) items:
//   k_pipe_setup   per block: planning-link FK -> metric goal distance of the (at most BLOCK, 7 at M = 25) states its
//                  edges belong to, on a wave of its own behind the edge threads, shared through LDS;
//                  per (state, primitive): gating, successor joint values, limits, waypoint count;
//                  claims a range of the work list with one atomic per block (prefix count)
//   k_pipe_configs per work item: one configuration against the grid and the link pairs;
//                  items [0, B) are the states themselves (waypoint 0 of every edge).
//                  Behind those blocks, in blocks of their own, one thread per (state, primitive): the
//                  successor of an edge that passed the limits test -- discretisation, state-table id,
//                  planning-link FK, goal test, heuristic -- which needs no verdict and so runs beside
//                  the collision check instead of behind it (results, coordinates included, in the
//                  caller's work buffer: nothing a caller can see is written before the verdict)
//   k_pipe_finish  per (state, primitive): verdict from the configurations' results, joined with what
//                  the successor role left; cost, outputs, compact stream, tallies.  A colliding edge
//                  keeps nothing of its successor's evaluation.
//                  Stages the model only for a block that holds a deferred edge.
// Booleans, coordinates, heuristics and costs are identical to k_expand.  Without the serial
// early exit a colliding edge has all its waypoints examined, so the lookup tally of an INVALID
// edge can exceed the reference's; for valid edges it is identical.
// k_pipe_prep (per state: the goal distance, in a launch of its own in front of k_pipe_setup) is what the step began
// with until the distance moved into k_pipe_setup; it stays selectable (test_hooks.h smplx_test_set_pipe_prep) as the
// reference the three-launch step is compared against.
// The work-list counters belong to the engine, one set per stream, and are all-zero between steps: block 0 of
// k_pipe_finish clears them behind their last reader.
// Per-robot build: the step keeps each state's sines and cosines (sphere_checks.h parent_trig; ExpandWork::trig, 4 N doubles a
// state: raw, and of the normalised angles).  Written by whoever computes the state's goal distance, whose chain takes the
// normalised ones: the goal-distance wave of k_pipe_setup -- one (state, variable) pair a lane, handed by shuffles to the
// lanes that run the chain -- or, in the four-launch mode, the state threads of k_pipe_prep (lattice_steps.h
// trig_row_and_goal_distance); read a launch later by both roles of k_pipe_configs, in the same round of loads as the
// joint values: a collision thread evaluates smplx_sincos only for the variables its waypoint moves, a successor thread
// for those its primitive moves, in rounds of one variable per lane.  The generic build keeps computing from the values.
// What the host knows comes in as kernel arguments, so that no thread's first indexed load waits for a load from the
// space record: nprims (every thread's state index is tid / nprims; a cross-query batch uses the lead space's actions for
// every row, so one value per launch is right), nvars (generic build: row strides in front of the staged model) and, for
// the collision blocks of k_pipe_configs, the model image and its byte count (its copy starts beside the shard counters
// instead of behind the header's size field).  S->actions stays the source of the action table's contents.
// ---------------------------------------------------------------------------------------------

// work item (64 bits): edge index | waypoint << 32 | waypoint count << 48, so that a configuration thread needs no
// further load to know where it sits on its edge
#define SMPLX_WP_MAX 0xFFFF
#define SMPLX_WORK_BLANK 0xFFFFFFFFFFFFFFFFull
#define SMPLX_WORK_SHARDS 8
#define SMPLX_SHARD_STRIDE 32   // ints: one 128-byte line per shard counter

extern "C" __global__ void __launch_bounds__(BLOCK)
k_pipe_prep(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int B,
            double* __restrict__ goal_dist, int* __restrict__ work_count,
        const SmplxSpaceDev* const* __restrict__ stab, const unsigned short* __restrict__ state_q, int* __restrict__ cmp_totals,
            const int* __restrict__ ins_items, int n_ins, double* __restrict__ trig)
{
    extern __shared__ __align__(16) unsigned char smem[];
    // K5: the states the host committed since the last batch join the device table (createHashEntry) in extra blocks
    if (n_ins > 0 && table_insert_block(S, stab, ins_items, n_ins, (B + BLOCK - 1) / BLOCK)) return;
    const ModelLds Mv = setup_model_only(S, smem);
    const ModelLds* M = &Mv;
    const SmplxGridDev grid = S->grid;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i <= SMPLX_WORK_SHARDS) work_count[i * SMPLX_SHARD_STRIDE] = 0;   // shard counters + deferred count
    if (cmp_totals && blockIdx.x == 0)                                   // compaction counters of k_pipe_finish
        for (int k = threadIdx.x; k < SMPLX_CMP_TOTALS; k += BLOCK) cmp_totals[k] = 0;
    if (i >= B) return;
    const SmplxBfsDev bfs = (stab ? stab[state_q[i]] : S)->bfs;   // per-query data in a cross-query batch
#ifdef SMPLX_CONST_MODEL
    if constexpr (CM_PARENT_TRIG) {
        goal_dist[i] = trig_row_and_goal_distance(M, grid, bfs, Q + (int64_t)i * CM_NV, trig + (int64_t)i * SMPLX_TRIG_ROW, true);
        return;
    }
#endif
    goal_dist[i] = metric_goal_distance(M, grid, bfs, Q + (int64_t)i * MV_NVARS(M));
}

// The part of an edge that the gate does not decide (manip_lattice.cpp:1471-1490 for an active primitive): successor
// joint values into sq, limits, waypoint count.  Returns the edge's flags (SMPLX_F_INACTIVE: the primitive has no action
// for this goal type) and W.
__device__ __forceinline__ int pipe_edge_values(const ModelLds* __restrict__ M, const SmplxActionsDev& A,
                                                const SmplxSpaceDev* __restrict__ Sq, int pi,
                                                const double* __restrict__ parent, double* __restrict__ sq, int& W)
{
    W = 0;
    if (!successor_values(M, A, Sq->goal, pi, parent, sq)) return SMPLX_F_INACTIVE;
    if (!check_joint_limits(M, sq)) return SMPLX_F_LIMITS;
    W = edge_waypoint_count(M, parent, sq);
    return 0;
}

// A block of k_pipe_setup is BLOCK edge threads plus one more wave, which computes the goal distances beside them.
#ifdef SMPLX_CONST_MODEL
#define SMPLX_SETUP_SERIAL_DIST (!CM_PARENT_TRIG)   // one lane per state, the whole chain with its sincos
#else
#define SMPLX_SETUP_SERIAL_DIST true
#endif
extern "C" __global__ void __launch_bounds__(SMPLX_SETUP_BLOCK)
k_pipe_setup(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int B,
             double* __restrict__ goal_dist, unsigned char* __restrict__ out_flags, double* __restrict__ out_q,
             int* __restrict__ edge_w, int* __restrict__ edge_lookups, unsigned char* __restrict__ edge_bad,
             int* __restrict__ state_lookups, unsigned char* __restrict__ state_bad,
             unsigned long long* __restrict__ work, int* __restrict__ work_count, int capacity,
        const SmplxSpaceDev* const* __restrict__ stab, const unsigned short* __restrict__ state_q,
             int have_goal_dist, int* __restrict__ cmp_totals, const int* __restrict__ ins_items, int n_ins,
             int nprims, int nvars, double* __restrict__ trig)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const SmplxActionsDev& A = S->actions;
    const long long n_edges = (long long)B * nprims;
    // K5: the states the host committed since the last batch join the device table (createHashEntry) in extra blocks
    // behind the edge blocks; the table is first read one launch later (successor role of k_pipe_configs)
    if (n_ins > 0 && table_insert_block(S, stab, ins_items, n_ins, (int)((n_edges + BLOCK - 1) / BLOCK))) return;
    const ModelLds Mv = setup_model_only(S, smem, (int)blockDim.x);   // BLOCK threads when k_pipe_prep ran in front: no goal-distance wave
    const ModelLds* M = &Mv;
    const bool dist_wave = threadIdx.x >= BLOCK;   // the wave behind the edge threads
    const long long tid = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool in_range = !dist_wave && tid < n_edges;
    const int nv = ARG_NVARS(nvars);
    const int si = in_range ? (int)(tid / nprims) : 0;
    const int pi = in_range ? (int)(tid - (long long)si * nprims) : 0;
    const double* parent = Q + (int64_t)si * nv;
    const SmplxSpaceDev* Sq = stab ? stab[state_q[si]] : S;
    const int type = A.type[pi];
    int W = 0;
    int flags = SMPLX_F_INACTIVE;
#ifdef SMPLX_CONST_MODEL
    // per-robot build: what the gate does not decide is worked out in registers BEFORE the gate is known, beside the
    // goal-distance wave; an edge whose primitive turns out inactive stores none of it
    // (with k_pipe_prep in front the gate is known here already and, as ever, only an active primitive is worked out)
    double sqv[CM_NV];
    if (in_range && (!have_goal_dist || mprim_active(A, goal_dist[si], type)))
        flags = pipe_edge_values(M, A, Sq, pi, parent, sqv, W);
#endif
    // have_goal_dist: k_pipe_prep ran in front (test_hooks.h smplx_test_set_pipe_prep) and left goal_dist[] and zeroed
    // cmp_totals.  Otherwise the block computes the goal distance of the states its edges belong to -- s0 .. s1, at most
    // BLOCK of them (7 at M = 25) -- on the lanes of its last wave, with k_pipe_prep's own expression.  A state whose
    // edges straddle two blocks is computed by both: same inputs, same instructions, same bits.
    __shared__ double block_goal_dist[BLOCK];
    const long long e0 = (long long)blockIdx.x * BLOCK;
    const int s0 = (int)(e0 / nprims);
    if (!have_goal_dist) {
        if (dist_wave) {
            if (cmp_totals && blockIdx.x == 0)                               // compaction counters of k_pipe_finish
                for (int k = threadIdx.x - BLOCK; k < SMPLX_CMP_TOTALS; k += 64) cmp_totals[k] = 0;
            const long long e1 = e0 + BLOCK - 1 < n_edges ? e0 + BLOCK - 1 : n_edges - 1;   // (e0 < n_edges: this is an edge block)
            const int s1 = (int)(e1 / nprims);                                               // < B
#ifdef SMPLX_CONST_MODEL
            // Per-robot build: the chain's sincos are evaluated lane-parallel, one (state, variable) pair per lane, 64 / NV
            // states a round (one round at 7 states a block), and kept as the state's row of the table (sphere_checks.h
            // parent_trig); the normalised ones travel by shuffles to the lanes that then run the chain without a sincos in
            // it.  One writer per row: the block that holds the state's first edge, as for goal_dist.  (One lane per state
            // that evaluates and stores its whole row ahead of its chain, as k_pipe_prep does, made the step slower than
            // before the table: profiles/parent_trig_ab.txt section 5.)
            constexpr int PER = CM_PARENT_TRIG ? 64 / CM_NV : 0;
            const int l = (int)threadIdx.x - BLOCK;
            const int ls = l / CM_NV, lv = l - ls * CM_NV;
            for (int r0 = s0; PER > 0 && r0 <= s1; r0 += PER) {   // (uniform over the wave)
                const int sj = r0 + ls;
                double ns = 0.0, nc = 0.0;
                if (ls < PER && sj <= s1) {
                    const double x = Q[(int64_t)sj * CM_NV + lv];
                    double rs = 0.0, rc = 0.0;   // a variable no SMPLX_TK_REV_*_T joint turns on: nobody reads its pairs, zeros are stored
                    if ((CM_TRIG_ANY >> lv) & 1u) smplx_sincos(x, &rs, &rc);
                    ns = rs; nc = rc;
                    bool cont = false;
#pragma unroll
                    for (int u = 0; u < CM_NV; ++u) if (CM_VAR_TYPE[u] == SMPLX_JT_CONTINUOUS) cont = cont || lv == u;
                    if (cont && ((CM_TRIG_ANY >> lv) & 1u)) {
                        const double xn = smplx_normalize_angle(x);
                        if (__double_as_longlong(xn) != __double_as_longlong(x)) smplx_sincos(xn, &ns, &nc);
                    }
                    if ((long long)sj * nprims >= e0) {
                        trig_pair_t* row = reinterpret_cast<trig_pair_t*>(trig + (int64_t)sj * SMPLX_TRIG_ROW);
                        trig_pair_t raw, nrm;
                        raw.x = rs; raw.y = rc; nrm.x = ns; nrm.y = nc;
                        row[lv] = raw; row[CM_NV + lv] = nrm;
                    }
                }
                double sn[CM_NV], cs[CM_NV];
#pragma unroll
                for (int v = 0; v < CM_NV; ++v) {   // lane k < PER gathers the pairs of state r0 + k (every lane takes part)
                    const int from = (l * CM_NV + v) & 63;
                    sn[v] = __shfl(ns, from); cs[v] = __shfl(nc, from);
                }
                if (l < PER && r0 + l <= s1) {
                    const int sk = r0 + l;
                    const SmplxBfsDev bfs = (stab ? stab[state_q[sk]] : S)->bfs;
                    block_goal_dist[sk - s0] = metric_goal_distance_sc(M, S->grid, bfs, Q + (int64_t)sk * CM_NV, sn, cs);
                }
            }
#endif
            for (int sj = s0 + (int)threadIdx.x - BLOCK; SMPLX_SETUP_SERIAL_DIST && sj <= s1; sj += 64) {
                const SmplxBfsDev bfs = (stab ? stab[state_q[sj]] : S)->bfs;   // a copy: its loads travel in front of the FK chain
                block_goal_dist[sj - s0] = metric_goal_distance(M, S->grid, bfs, Q + (int64_t)sj * nv);
            }
        }
        __syncthreads();
    }
    int items = 0;
    if (in_range) {
        double* sq = out_q + tid * nv;
        const double gd = have_goal_dist ? goal_dist[si] : block_goal_dist[si - s0];
        if (pi == 0) {
            state_lookups[si] = 0; state_bad[si] = 0;
            if (!have_goal_dist) goal_dist[si] = gd;   // for the deferred pass of k_pipe_finish (expand_edge): one writer per state
        }
        if (!mprim_active(A, gd, type)) {
            flags = SMPLX_F_INACTIVE;
            W = 0;
        } else {
#ifdef SMPLX_CONST_MODEL
            if (flags != SMPLX_F_INACTIVE) {
#pragma unroll
                for (int v = 0; v < CM_NV; ++v) sq[v] = sqv[v];
            }
#else
            flags = pipe_edge_values(M, A, Sq, pi, parent, sq, W);
#endif
        }
        items = W > 0 ? W - 1 : 0;
        edge_lookups[tid] = 0;
        edge_bad[tid] = 0;
    }
    // claim a contiguous range of the work list.  Same-address atomics serialise at ~12 ns each on this
    // chip, so: wave prefix count (shuffles) -> block total through LDS -> ONE atomic per block, spread over
    // SMPLX_WORK_SHARDS counters that live on separate 128-byte lines.
    __shared__ int wave_sum[BLOCK / 64];
    __shared__ int block_base;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = items;
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off);
        if (lane >= off) incl += t;
    }
    if (lane == 63 && !dist_wave) wave_sum[wv] = incl;
    __syncthreads();
    const int shard = blockIdx.x % SMPLX_WORK_SHARDS;
    const int shard_cap = capacity / SMPLX_WORK_SHARDS;
    if (threadIdx.x == 0) {
        int tot = 0;
#pragma unroll
        for (int k = 0; k < BLOCK / 64; ++k) tot += wave_sum[k];
        block_base = tot > 0 ? atomicAdd(&work_count[shard * SMPLX_SHARD_STRIDE], tot) : 0;
    }
    __syncthreads();
    int first = block_base + incl - items;
    for (int k = 0; k < wv; ++k) first += wave_sum[k];
    if (in_range) {
        if (items > 0) {
            unsigned long long* wl = work + (size_t)shard * shard_cap;
            if (first + items <= shard_cap && W <= SMPLX_WP_MAX) {
                const unsigned long long base = (unsigned long long)tid | ((unsigned long long)W << 48);
                for (int k = 0; k < items; ++k) wl[first + k] = base | ((unsigned long long)(k + 1) << 32);
            } else {
                // does not fit: deferred to a fused pass (k_expand, SMPLX_F_DEFERRED); blank the part of the claim
                // that lies below the shard's capacity
                for (int k = first; k < first + items && k < shard_cap; ++k) wl[k] = SMPLX_WORK_BLANK;
                flags = SMPLX_F_DEFERRED;
                atomicAdd(&work_count[SMPLX_WORK_SHARDS * SMPLX_SHARD_STRIDE], 1);
            }
        }
        edge_w[tid] = W;
        out_flags[tid] = (unsigned char)flags;
    }
}

// ManipLattice::stateToCoord (manip_lattice.cpp:1263-1289) of the successor's joint values
__device__ __forceinline__ void successor_coords(const ModelLds* __restrict__ M, const double* __restrict__ sq, int* __restrict__ sc)
{
    const int nv = MV_NVARS(M);
    MV_UNROLL
    for (int v = 0; v < nv; ++v) sc[v] = var_to_coord(M, v, sq[v]);
}

// What the verdict of an edge does not decide: discretisation, state-table id, planning-link FK, goal test, heuristic
// (manip_lattice.cpp:1496-1535 for a successor that passed the limits test).  Needs the successor's joint values and
// the query's goal, BFS grid and table only, all final when k_pipe_setup ends.  sc: where the coordinates go.
// It is the composition of its pieces -- successor_coords, table_probe_issue, successor_goal_h (chain, goal test,
// heuristic), table_probe_resolve -- in this order, so that the home slot of the table travels during the chain.  The
// per-robot k_step_block (step_block.h) places the same pieces itself, the first two in front of its gate.
template <bool SC = false>
__device__ __forceinline__ void pipe_successor(const ModelLds* __restrict__ M, const SmplxSpaceDev* __restrict__ Sq,
                                               const SmplxGridDev& grid, const double* __restrict__ sq, int* __restrict__ sc,
                                               bool want_id, int& h, int& id, bool& is_goal, const double* sn = nullptr,
                                               const double* cs = nullptr)
{
    const int nv = MV_NVARS(M);
    const SmplxBfsDev bfs = Sq->bfs;
    successor_coords(M, sq, sc);
    const TableSlotWords home = want_id ? table_probe_issue(Sq->table, sc, nv) : table_probe_none();   // K5
    h = successor_goal_h<SC>(M, Sq->goal, bfs, grid, sq, sc, is_goal, sn, cs);
    id = want_id ? table_probe_resolve(Sq->table, sc, nv, home) : -1;
}

// Successor role of k_pipe_configs: the blocks behind the cfg_blocks collision blocks, one thread per edge.  An edge whose
// flag is 0 after k_pipe_setup (active, within limits, not deferred; W == 0 included) has its successor evaluated here,
// beside the collision check instead of behind it; k_pipe_finish joins the result with the verdict.  A whole wave has
// this one role, and it is shorter than a configuration wave (no sphere trees, one chain).
__device__ __forceinline__ void pipe_successor_role(const SmplxSpaceDev* __restrict__ S, int B, int cfg_blocks,
                                                    const unsigned char* __restrict__ out_flags, const double* __restrict__ out_q,
                                                    int* __restrict__ succ_coord, const SmplxSpaceDev* const* __restrict__ stab,
                                                    const unsigned short* __restrict__ state_q, bool want_id,
                                                    unsigned long long* __restrict__ succ_eval, unsigned char* __restrict__ succ_goal,
                                                    unsigned char* smem, int nprims, int nvars,
                                                    const double* __restrict__ Q, const double* __restrict__ trig)
{
    const long long tid = (long long)((int)blockIdx.x - cfg_blocks) * BLOCK + threadIdx.x;
    // as in the collision blocks: the flag (and, per-robot build, the joint values) are fetched BEFORE the model is staged
    const bool live = tid < (long long)B * nprims && out_flags[tid] == 0;
#ifdef SMPLX_CONST_MODEL
    double qv[CM_NV];
    if (live) {
#pragma unroll
        for (int v = 0; v < CM_NV; ++v) qv[v] = out_q[tid * CM_NV + v];
    }
    // ... and with them the parent's joint values and its row of normalised sines and cosines: a variable the primitive
    // leaves alone (d == 0: sq[v] has the parent's bits) takes the row's pair
    constexpr bool SC = CM_PARENT_TRIG && CM_TRIG_PLANNING != 0;
    double pq[CM_NV], prow[2 * CM_NV];
    if (SC && live) {
        const long long sp = tid / nprims;
#pragma unroll
        for (int v = 0; v < CM_NV; ++v) pq[v] = Q[sp * CM_NV + v];
        trig_row_load<true>(trig, sp, prow);
    }
#endif
    const ModelLds Mv = setup_model_only(S, smem);
    const ModelLds* M = &Mv;
    if (!live) return;
#ifndef ABL_NO_SUCC
    const int nv = ARG_NVARS(nvars);
    const int si = (int)(tid / nprims);
    const SmplxSpaceDev* Sq = stab ? stab[state_q[si]] : S;   // per-query goal, BFS grid and table in a cross-query batch
    const SmplxGridDev grid = S->grid;
#ifdef SMPLX_CONST_MODEL
    const double* sq = qv;
#else
    const double* sq = out_q + tid * nv;
#endif
    int h, id;
    bool is_goal;
#ifdef SMPLX_CONST_MODEL
    if constexpr (SC) {
        double sn[CM_NV], cs[CM_NV];
        parent_trig<CM_TRIG_PLANNING, true>(qv, pq, prow, sn, cs);
        pipe_successor<true>(M, Sq, grid, sq, succ_coord + tid * nv, want_id, h, id, is_goal, sn, cs);
    } else
#endif
    pipe_successor(M, Sq, grid, sq, succ_coord + tid * nv, want_id, h, id, is_goal);
    succ_eval[tid] = (unsigned long long)(unsigned int)h | ((unsigned long long)(unsigned int)id << 32);   // one 8-byte store
    succ_goal[tid] = is_goal ? 1 : 0;
#endif
}

extern "C" __global__ void __launch_bounds__(BLOCK, 2)   // >= 2 waves per SIMD: at most 256 VGPRs, whichever compiler builds it
k_pipe_configs(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int B,
               const double* __restrict__ out_q, const int* __restrict__ edge_w, int* __restrict__ edge_lookups,
               unsigned char* __restrict__ edge_bad, int* __restrict__ state_lookups, unsigned char* __restrict__ state_bad,
               const unsigned long long* __restrict__ work, const int* __restrict__ work_count, int capacity, int cfg_blocks,
               const unsigned char* __restrict__ out_flags, int* __restrict__ succ_coord,
               const SmplxSpaceDev* const* __restrict__ stab, const unsigned short* __restrict__ state_q, int want_id,
               unsigned long long* __restrict__ succ_eval, unsigned char* __restrict__ succ_goal, int nprims, int nvars,
               const unsigned char* __restrict__ blob, int blob_bytes, const double* __restrict__ trig)
{
    extern __shared__ __align__(16) unsigned char smem[];
    // the grid is cfg_blocks collision blocks, dispatched first (they hold the long waves), then one successor thread
    // per edge in blocks of their own
    if ((int)blockIdx.x >= cfg_blocks) {
        pipe_successor_role(S, B, cfg_blocks, out_flags, out_q, succ_coord, stab, state_q, want_id != 0, succ_eval, succ_goal, smem,
                            nprims, nvars, Q, trig);
        return;
    }
    // the model image is known from the arguments: its first pieces travel beside the shard counters
    const ModelFetch fetched = model_fetch(blob, blob_bytes);
#ifdef SMPLX_CONST_MODEL
    constexpr bool RS = true;      // saved link transforms in registers (as k_state_valid): LDS per block without the slots, which
                                   // is what several batches in flight, or one large one, share a CU by
#else
    constexpr bool RS = false;
#endif
    const int shard_cap = capacity / SMPLX_WORK_SHARDS;
    int pre[SMPLX_WORK_SHARDS + 1];   // prefix of the shard fill counts (claims beyond a shard's capacity were never written)
    pre[0] = 0;
#pragma unroll
    for (int k = 0; k < SMPLX_WORK_SHARDS; ++k) {
        int c = work_count[k * SMPLX_SHARD_STRIDE];
        if (c > shard_cap) c = shard_cap;
        pre[k + 1] = pre[k] + c;
    }
    const long long total = (long long)B + pre[SMPLX_WORK_SHARDS];
    if ((long long)blockIdx.x * BLOCK >= total) return;   // whole block idle: skip staging the model
#ifdef SMPLX_CONST_MODEL
    // Per-robot build: the launch covers every item (engine.hip sizes the grid for B + 3 B M items and k_pipe_setup never
    // lists more), one item per thread.  A block's life is a chain of dependent memory round trips of ~1 us each --
    // counts, model header, model bytes, work item, joint values -- in front of ~10 us of work: the item and the joint
    // values of its edge are fetched BEFORE the model is staged, so that they travel together with the model bytes
    // (5 round trips -> 3).
    if (total <= (long long)cfg_blocks * BLOCK) {
        constexpr int nv = CM_NV;
        const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
        unsigned long long it = SMPLX_WORK_BLANK;
        if (i >= B && i < total) {
            const int li = (int)(i - B);
            int sh = 0;
#pragma unroll
            for (int k = 1; k < SMPLX_WORK_SHARDS; ++k) sh += (li >= pre[k]) ? 1 : 0;
            it = work[(size_t)sh * shard_cap + (li - pre[sh])];
        }
        const bool is_state = i < B, is_item = it != SMPLX_WORK_BLANK;
        const long long edge = (long long)(it & 0xFFFFFFFFull);
        const int wp = (int)((it >> 32) & 0xFFFF);
        const int W = (int)(it >> 48);
        // ... and so is the parent's row of sines and cosines (sphere_checks.h parent_trig)
        constexpr bool SC = CM_PARENT_TRIG;
        double qs[CM_NV], qf[CM_NV], prow[2 * CM_NV];
        if (is_state || is_item) {
            const long long si = is_state ? i : edge / nprims;
            const double* ps = Q + si * nv;
            const double* pf = is_state ? ps : out_q + edge * nv;
#pragma unroll
            for (int v = 0; v < nv; ++v) { qs[v] = ps[v]; qf[v] = pf[v]; }
            if constexpr (SC) trig_row_load<false>(trig, si, prow);
        }
        ModelLds Mv;
        ThreadLds L = setup_lds(S, smem, &Mv, BLOCK, !RS, blob, blob_bytes, fetched);
        const ModelLds* M = &Mv;
        const SmplxGridDev grid = S->grid;
        if (!(is_state || is_item)) return;
        EdgeRef e;
        e.start = nullptr; e.finish = nullptr;   // config_valid_staged never dereferences them
        e.alpha = is_state ? 0.0 : (double)wp * (1.0 / (double)(W - 1));
        int lk = 0;
        double qc[CM_NV];
#ifndef ABL_NO_FK
#pragma unroll
        for (int v = 0; v < nv; ++v) {   // stage_config
            const double sv = qs[v];
            double q = sv;
            if (e.alpha != 0.0) q = sv + e.alpha * edge_diff(M, v, sv, qf[v]);
            lds_d(L, L.q_base + v) = q;
            qc[v] = q;
        }
#endif
        bool ok;
        if constexpr (SC) {
            // a state item changes nothing and evaluates nothing; a waypoint evaluates the one or two variables its
            // primitive moves (a snap: as many as it moves)
            double sn[CM_NV], cs[CM_NV];
            parent_trig<CM_TRIG_COLLISION, false>(qc, qs, prow, sn, cs);
            ok = config_valid_staged<RS, true>(M, L, grid, e, lk, sn, cs);
        } else {
            ok = config_valid_staged<RS>(M, L, grid, e, lk);
        }
        if (is_state) {
            state_lookups[i] = lk;
            if (!ok) state_bad[i] = 1;
        } else {
            atomicAdd(&edge_lookups[edge], lk);
            if (!ok) edge_bad[edge] = 1;
        }
        return;
    }
#endif
    ModelLds Mv;
    ThreadLds L = setup_lds(S, smem, &Mv, BLOCK, !RS, blob, blob_bytes, fetched);
    const ModelLds* M = &Mv;
    const SmplxGridDev grid = S->grid;
    const int nv = ARG_NVARS(nvars);
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < total; i += (long long)cfg_blocks * BLOCK) {
        EdgeRef e;
        int lk = 0;
        if (i < B) {   // the state itself: waypoint 0 of each of its edges
            e.start = Q + i * nv;
            e.finish = e.start;
            e.alpha = 0.0;
            const bool ok = config_valid<RS>(M, L, grid, e, lk);
            state_lookups[i] = lk;
            if (!ok) state_bad[i] = 1;
        } else {
            const int li = (int)(i - B);
            int sh = 0;
#pragma unroll
            for (int k = 1; k < SMPLX_WORK_SHARDS; ++k) sh += (li >= pre[k]) ? 1 : 0;
            const unsigned long long it = work[(size_t)sh * shard_cap + (li - pre[sh])];
            if (it == SMPLX_WORK_BLANK) continue;
            const long long edge = (long long)(it & 0xFFFFFFFFull);
            const int wp = (int)((it >> 32) & 0xFFFF);
            const int W = (int)(it >> 48);
            const int si = (int)(edge / nprims);
            e.start = Q + (int64_t)si * nv;
            e.finish = out_q + edge * nv;
            e.alpha = (double)wp * (1.0 / (double)(W - 1));
            const bool ok = config_valid<RS>(M, L, grid, e, lk);
            atomicAdd(&edge_lookups[edge], lk);
            if (!ok) edge_bad[edge] = 1;
        }
    }
}

extern "C" __global__ void __launch_bounds__(BLOCK, 2)   // holds the whole-edge walk for overflowed edges: keep it at 2 waves per SIMD
k_pipe_finish(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int B,
              const int* __restrict__ edge_w, const int* __restrict__ edge_lookups, const unsigned char* __restrict__ edge_bad,
              const int* __restrict__ state_lookups, const unsigned char* __restrict__ state_bad,
              unsigned char* __restrict__ out_flags, int* __restrict__ out_coord, double* __restrict__ out_q,
              int* __restrict__ out_h, int* __restrict__ out_cost, int* __restrict__ out_lookups,
              unsigned long long* __restrict__ counters, const double* __restrict__ goal_dist,
        const SmplxSpaceDev* const* __restrict__ stab, const unsigned short* __restrict__ state_q,
              int* __restrict__ out_id, SmplxCompactDev cmp, const unsigned long long* __restrict__ succ_eval,
              const unsigned char* __restrict__ succ_goal, const int* __restrict__ succ_coord, int* __restrict__ work_count,
              int nprims, int nvars)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const SmplxActionsDev& A = S->actions;
    // the stream's work-list counters (shards + deferred count) go back to zero for the next step's k_pipe_setup: their
    // last reader, k_pipe_configs, ended a launch ago
    if (blockIdx.x == 0 && threadIdx.x <= SMPLX_WORK_SHARDS) work_count[threadIdx.x * SMPLX_SHARD_STRIDE] = 0;
    const int nv = ARG_NVARS(nvars);   // (the model is not staged here)
    const long long tid = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const bool in_range = tid < (long long)B * nprims;
    int flags = SMPLX_F_INACTIVE, lookups = 0, performed = 0, evaluated = 0;
    int succ_id = -1, succ_h = 0;   // K5: id of the successor's coordinate in the device state table
    int ncfg = 0, slk = 0;   // configurations k_pipe_configs checked for this edge / lookups of the state's own check
    // everything the verdict needs, in ONE round of independent loads (rows that setup or the successor role did not
    // write are read and ignored)
    int si = 0, pi = 0, W = 0, e_lk = 0, e_bad = 0, s_lk = 0, s_bad = 0, s_goal = 0;
    unsigned long long se = 0;
#ifdef SMPLX_CONST_MODEL
    int s_coord[CM_NV];   // the successor's coordinates, fetched with the rest
#define PIPE_SUCC_COORD(v) s_coord[v]
#else
#define PIPE_SUCC_COORD(v) succ_coord[tid * nv + (v)]
#endif
    bool deferred = false;
    if (in_range) {
        si = (int)(tid / nprims);
        pi = (int)(tid - (long long)si * nprims);
        flags = out_flags[tid];
        W = edge_w[tid];
        e_lk = edge_lookups[tid];
        e_bad = edge_bad[tid];
        s_lk = state_lookups[si];
        s_bad = state_bad[si];
        se = succ_eval[tid];
        s_goal = succ_goal[tid];
#ifdef SMPLX_CONST_MODEL
#pragma unroll
        for (int v = 0; v < nv; ++v) s_coord[v] = succ_coord[tid * nv + v];
#endif
    }
    if (__syncthreads_or(flags & SMPLX_F_DEFERRED)) {
        // the model and the per-thread scratch are only needed by edges that overflowed the work list (normally none):
        // such an edge is walked whole by this thread
        ModelLds Mv;
        const ThreadLds L = setup_lds(S, smem, &Mv);
        if (flags & SMPLX_F_DEFERRED) {
            const SmplxSpaceDev* Sq = stab ? stab[state_q[si]] : S;
            const SmplxGridDev grid = S->grid;
            if (pi == 0) { slk = s_lk; ncfg = 1; }
            const EdgeTally t = expand_edge(&Mv, L, S, Sq, grid, Q, tid, goal_dist, s_bad == 0, s_lk,
                                            out_flags, out_coord, out_q, out_h, out_cost, out_lookups);
            flags = t.flags; lookups = t.lookups; performed = t.performed; evaluated = t.evaluated;
            succ_h = out_h[tid];
            // K5: getHashEntry on the device copy of the state table (manip_lattice.cpp:1302-1316).  The id is only a
            // hint to the host (it skips its own lookup); ids are still ASSIGNED on the host, in commit order.
            if (out_id) {
                if (flags & SMPLX_F_VALID) succ_id = table_lookup<false>(Sq->table, out_coord + tid * nv, nv);
                out_id[tid] = succ_id;
            }
            deferred = true;
        }
    }
    if (in_range && !deferred) {
        if (pi == 0) { slk = s_lk; ncfg = 1; }
        int h = 0, cost = 0;
        if (!(flags & SMPLX_F_INACTIVE)) evaluated = 1;
        if (flags == 0) {
            if (W > 0) ncfg += W - 1;
            performed = e_lk;
            const bool ok = (W == 0) || (s_bad == 0 && e_bad == 0);
            lookups = performed + (W > 0 ? s_lk : 0);
            if (!ok) {
                flags = SMPLX_F_COLLISION;
            } else {
                // the successor role of k_pipe_configs evaluated it beside the collision check; out_coord is written for a
                // valid edge only, as before (a colliding edge leaves the caller's row alone)
                MV_UNROLL
                for (int v = 0; v < nv; ++v) out_coord[tid * nv + v] = PIPE_SUCC_COORD(v);
                h = (int)(unsigned int)(se & 0xFFFFFFFFull);
                if (out_id) succ_id = (int)(unsigned int)(se >> 32);
                cost = A.cost[pi];
                flags = SMPLX_F_VALID | (s_goal ? SMPLX_F_GOAL : 0);
            }
        }
        out_flags[tid] = (unsigned char)flags;
        out_h[tid] = h;
        out_cost[tid] = cost;
        out_lookups[tid] = lookups;
        succ_h = h;
        if (out_id) out_id[tid] = succ_id;
    }
    // K5: validity compaction with wavefront ballots.  A valid successor leaves 8 bytes in region A; one whose
    // coordinate the table does not know (or a goal successor, whose own joint values extractPath reports) also a full
    // record in region B.  Ballot -> popcount of the lanes below -> wave totals in LDS -> ONE atomic per region and block.
    if (cmp.rec_a) {
        __shared__ int c_cnt[BLOCK / 64][2];
        __shared__ int c_base[2];
        const bool is_a = in_range && (flags & SMPLX_F_VALID) != 0;
        const bool is_b = is_a && (succ_id < 0 || (flags & SMPLX_F_GOAL) != 0);
        const unsigned long long m_a = __ballot(is_a), m_b = __ballot(is_b);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        if (lane == 0) { c_cnt[wv][0] = __popcll(m_a); c_cnt[wv][1] = __popcll(m_b); }
        __syncthreads();
        if (threadIdx.x == 0) {
            int ta = 0, tb = 0;
#pragma unroll
            for (int k = 0; k < BLOCK / 64; ++k) { ta += c_cnt[k][0]; tb += c_cnt[k][1]; }
            const int shard = blockIdx.x % SMPLX_CMP_SHARDS;
            const int sa = cmp.cap_a / SMPLX_CMP_SHARDS, sb = cmp.cap_b / SMPLX_CMP_SHARDS;
            int ba = ta > 0 ? atomicAdd(&cmp.totals[32 * shard], ta) : 0;
            int bb = tb > 0 ? atomicAdd(&cmp.totals[32 * shard + 1], tb) : 0;
            if (ba + ta > sa || bb + tb > sb) { cmp.totals[32 * SMPLX_CMP_SHARDS] = 1; ba = -1; }   // overflow: dense outputs stay valid
            else { ba += shard * sa; bb += shard * sb; }
            c_base[0] = ba; c_base[1] = bb;
            int* bt = cmp.block_tab + 4 * (size_t)blockIdx.x;
            bt[0] = ba; bt[1] = ta; bt[2] = bb; bt[3] = tb;
        }
        __syncthreads();
        if (c_base[0] >= 0 && is_a) {
            int ia = c_base[0] + __popcll(m_a & below), ib = c_base[1] + __popcll(m_b & below);
            for (int k = 0; k < wv; ++k) { ia += c_cnt[k][0]; ib += c_cnt[k][1]; }
            cmp.rec_a[2 * (size_t)ia] = succ_id;
            cmp.rec_a[2 * (size_t)ia + 1] = pi | ((flags & SMPLX_F_GOAL) ? 0x100 : 0) | (si << 9);
            if (is_b) {
                unsigned char* rb = cmp.rec_b + (size_t)ib * cmp.rec_b_bytes;
                int* ri = (int*)rb;
                double* rq = (double*)(rb + (size_t)((nv + 2) / 2 * 2) * 4);
                ri[0] = succ_h;
                MV_UNROLL
                for (int v = 0; v < nv; ++v) { ri[1 + v] = out_coord[tid * nv + v]; rq[v] = out_q[tid * nv + v]; }
            }
        }
    }
    if (counters) {
        const unsigned long long m_eval = __ballot(evaluated);
        const unsigned long long m_valid = __ballot((flags & SMPLX_F_VALID) != 0);
        tally_block(counters, __popcll(m_eval), __popcll(m_valid), lookups, performed, ncfg, slk);
    }
#undef PIPE_SUCC_COORD
}
