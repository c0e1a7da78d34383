// smpl_amd/csrc/search_kernel.h -- device-resident ARA* (SURVEY row N2), included at the end of kernels.hip.
// Owns: the search state's load / store (sstate_*), SearchRegs with search_regs_load / search_regs_store, BookRegs and
// BookOut with book_out_store / book_out_load, goal_distance_of_h, and the pieces of a step of k_search, each stated once:
// round_prepare (an evaluation round for a parent state), search_book_table with book_find_pairs (getOrCreateState's table
// side), open_improve_wave (the OPEN / INCONS operation of an improved successor); k_search itself.  OPEN is
// search_heap.h (the pop: heap_pop_wave, a new epsilon: heap_rekey_block), the state table search_table.h.
//
//   k_search      one persistent workgroup per query: pop -> expand on the lanes -> getOrCreateState -> push / decrease.
//                 Follows smpl/src/search/arastar.cpp:107-215 (replan), 486-527 (improvePath), 531-568 (expand),
//                 571-582 (reorderOpen, computeKey), 613-627 (reinitSearchState); OPEN is the reference's binary heap
//                 (smpl/include/smpl/detail/intrusive_heap.hpp:145-166 push / pop, 346-395 the sift rules: strict '<',
//                 the left child only if left < right), so ties pop in the reference's order and state ids -- assigned
//                 here, by the workgroup, in its own commit order (manip_lattice.cpp:1302-1354) -- are the reference's.
//
// Who does what inside the workgroup (blockDim.x = smplx_small_block(nprims)):
//   the LAST wave   ("search wave") runs the search: the replan state machine, pop, the successors' joint values, limits,
//                   coordinates, state-table probes, goal test and heuristic (lane p = primitive p), getOrCreateState, the
//                   relaxation in primitive order (the order decides ties in OPEN), INCONS.  It works as ONE unit: what a
//                   sequential program keeps in variables lives in its registers (uniform over the lanes), per-successor data
//                   in the lane of the primitive, and a value another lane holds is read with v_readlane -- a single lane
//                   walking LDS-resident structures costs a ~100-cycle round trip per step, which is what round 3 first
//                   measured (13 us of relaxation per expansion).  (The wave-parallel sifts of the heap: search_heap.h.)
//   the other waves check configurations: one waypoint of one edge per lane (expand_config_lane), between the two barriers
//                   of a step.
//
// A launch runs at most `max_steps` expansions and then stores its state in the query's SmplxSearchDev, so that the host
// sees progress, can stop a search, and can enlarge buffers (SMPLX_SS_GROW) between launches.
// A wall-clock budget (smplx_time_params, SMPLX_TIME_WALL) is checked by the search wave itself, once per step where the
// expansion bound is (ARAStar::timedOut, arastar.cpp:454-484): the first launch of a call records the call's start in the
// header, moved back by the host time the call spent before that launch (`pre_ticks`); later launches of the call keep it.
#pragma once

#include "small_batch.h"   // ExpandLds, expand_state_block's lane functions, SMPLX_WAVE_SYNC
#include "search_heap.h"
#include "search_table.h"

#define SMPLX_INFINITECOST 1000000000u     // SBPL INFINITECOST

enum { SA_EVAL = 0, SA_SKIP = 1, SA_REORDER = 2, SA_EXIT = 3 };

// ARAStar::reinitSearchState (arastar.cpp:613-627) on a copy of the state; h stays (GetGoalHeuristic of a state is fixed
// for a goal).  A state that was not touched in this call is not in OPEN: OPEN is emptied when a call starts.
__device__ __forceinline__ void sstate_reinit(SmplxSState& s, int call_number)
{
    s.g = SMPLX_INFINITECOST;
    s.f = SMPLX_INFINITECOST;
    s.eg = SMPLX_INFINITECOST;
    s.iteration_closed = 0;
    s.call_number = (unsigned short)call_number;
    s.bp = -1;
    s.heap_index = 0;
    s.flags = 0;
}

// the search state of a lane that has no successor (yet)
__device__ __forceinline__ SmplxSState sstate_blank()
{
    SmplxSState s;
    s.g = s.h = s.f = s.eg = 0; s.bp = -1; s.heap_index = 0; s.iteration_closed = 0; s.call_number = 0; s.flags = 0;
    return s;
}

typedef table_int4 sk_int4;   // (lattice_steps.h)

// write a state's fields back; heap_index only when the caller owns it (it is otherwise kept current by the sifts)
__device__ __forceinline__ void sstate_store(SMPLX_GLOBAL_AS SmplxSState* dst, const SmplxSState& s, bool with_heap_index)
{
    sk_int4 a;
    a.x = (int)s.g; a.y = (int)s.h; a.z = (int)s.f; a.w = (int)s.eg;
    *(SMPLX_GLOBAL_AS sk_int4*)dst = a;
    dst->bp = s.bp;
    if (with_heap_index) dst->heap_index = s.heap_index;
    *(SMPLX_GLOBAL_AS unsigned int*)&dst->iteration_closed = (unsigned int)s.iteration_closed | ((unsigned int)s.call_number << 16);
    dst->flags = s.flags;
}
__device__ __forceinline__ SmplxSState sstate_load(const SMPLX_GLOBAL_AS SmplxSState* src)
{
    const sk_int4 a = ((const SMPLX_GLOBAL_AS sk_int4*)src)[0], b = ((const SMPLX_GLOBAL_AS sk_int4*)src)[1];
    SmplxSState s;
    s.g = (unsigned int)a.x; s.h = (unsigned int)a.y; s.f = (unsigned int)a.z; s.eg = (unsigned int)a.w;
    s.bp = b.x; s.heap_index = b.y;
    s.iteration_closed = (unsigned short)((unsigned int)b.z & 0xFFFFu); s.call_number = (unsigned short)((unsigned int)b.z >> 16);
    s.flags = (unsigned int)b.w;
    return s;
}

// the search's variables: registers of the search wave, the same value in every lane
struct SearchRegs {
    double curr_eps, satisfied_eps;
    int heap_size, nstates, n_incons, n_log, n_succ;
    int iteration, call_number, phase, num, expand_count, expand_count_init, err;
    int dup_pushes, status, grow_what, steps_left;
    unsigned int goal_f;
    long long committed_evals, gpu_evals, lookups;
};
// ... as a launch finds them in the query's header, with `max_steps` expansions to go
__device__ __forceinline__ SearchRegs search_regs_load(const SmplxSearchDev* P, int max_steps)
{
    SearchRegs R;
    R.curr_eps = P->curr_eps; R.satisfied_eps = P->satisfied_eps;
    R.heap_size = P->heap_size; R.nstates = P->nstates; R.n_incons = P->n_incons; R.n_log = P->n_log; R.n_succ = P->n_succ;
    R.iteration = P->iteration; R.call_number = P->call_number; R.phase = P->phase; R.num = P->num;
    R.expand_count = P->expand_count; R.expand_count_init = P->expand_count_init; R.err = P->err;
    R.dup_pushes = P->dup_pushes; R.goal_f = P->goal_f;
    R.committed_evals = P->committed_evals; R.gpu_evals = P->gpu_evals; R.lookups = P->lookups;
    R.status = SMPLX_SS_RUNNING; R.grow_what = 0; R.steps_left = max_steps;
    return R;
}
// ... and as it leaves them there for the host and the next launch (one lane)
__device__ __forceinline__ void search_regs_store(SmplxSearchDev* Pd, const SearchRegs& R)
{
    Pd->curr_eps = R.curr_eps; Pd->satisfied_eps = R.satisfied_eps;
    Pd->heap_size = R.heap_size; Pd->nstates = R.nstates; Pd->n_incons = R.n_incons; Pd->n_log = R.n_log; Pd->n_succ = R.n_succ;
    Pd->iteration = R.iteration; Pd->call_number = R.call_number; Pd->phase = R.phase; Pd->num = R.num;
    Pd->expand_count = R.expand_count; Pd->expand_count_init = R.expand_count_init; Pd->err = R.err;
    Pd->dup_pushes = R.dup_pushes; Pd->goal_f = R.goal_f;
    Pd->status = R.status; Pd->grow_what = R.grow_what;
    Pd->committed_evals = R.committed_evals; Pd->gpu_evals = R.gpu_evals; Pd->lookups = R.lookups;
}

// getMetricGoalDistance recovered from a state's heuristic h = cost_per_cell * BFS distance (bfs_heuristic.cpp:129-138 /
// 355-366: both read the BFS cell of the same planning-link position); the caller knows that the product is invertible.
// The distance of an unreachable cell must stay the one metric_goal_distance (lattice_steps.h) gives.
__device__ __forceinline__ double goal_distance_of_h(int h, int cpc, const SmplxGridDev& grid)
{
    return h == 32767 ? (double)0x7FFFFFFF * grid.res : (double)(h / cpc) * grid.res;
}

// An evaluation round is got ready for a parent state in Y, by the whole search wave (lane v < nv brings the parent's joint
// value `parent_q`): the parent, the verdict words cleared, the goal distance -- from the state's heuristic `h` where
// `gd_from_h` says that it follows from it, else by lane 0 (metric_goal_distance) and a broadcast --, then per primitive
// whether it has an action here and the successor's joint values (manip_lattice.cpp:254-270).  Returns the lane's
// "primitive `lane` has a successor to evaluate", which Y.lookups tells the other waves.  No block barrier: opening the
// round (W.action / W.buf / W.seq and barrier A) is the caller's.
// In two halves, because the round of the popped state stages its parent ahead of the pop (the load of the joint values
// travels beside the sift-down) and does the rest behind it: round_stage, then round_gate; round_prepare is both.
// round_gate ends with the stores of Y.lookups and Y.goal_dist.  Where the popped state's round follows a wrong guess they
// now land ahead of the barrier that ends the guessed round (they used to follow it): Y is the buffer the guessed round
// does not use, and nobody reads it before barrier A of its own round, as for the top of OPEN's round further down.
__device__ __forceinline__ void round_stage(ExpandLds& Y, int lane, int nv, int nprims, double parent_q)
{
    if (lane < nv) Y.parent[lane] = parent_q;
    if (lane < nprims) { Y.edge_bad[lane] = 0; Y.edge_lk[lane] = 0; }
    if (lane == 0) { Y.state_bad = 0; Y.state_lookups = 0; }
}
__device__ __forceinline__ bool round_gate(const ModelLds* __restrict__ M, const SmplxActionsDev& A, const SmplxGoalDev& G,
                                              const SmplxGridDev& grid, const SmplxBfsDev& bfs, bool gd_from_h, ExpandLds& Y,
                                              int lane, int nprims, int h)
{
    SMPLX_WAVE_SYNC();                               // Y.parent is complete
    double gd;
    if (gd_from_h) gd = goal_distance_of_h(h, bfs.cost_per_cell, grid);
    else {
        double g1 = 0.0;
        if (lane == 0) g1 = metric_goal_distance(M, grid, bfs, Y.parent);
        gd = wave_rl_f64(g1, 0);
    }
    const bool in = lane < nprims;
    const bool act = in && mprim_active(A, gd, A.type[lane]) && successor_values(M, A, G, lane, Y.parent, Y.sq[lane]);
    if (in) Y.lookups[lane] = act ? 1 : 0;
    if (lane == 0) Y.goal_dist = gd;
    return act;
}
__device__ __forceinline__ bool round_prepare(const ModelLds* __restrict__ M, const SmplxActionsDev& A, const SmplxGoalDev& G,
                                              const SmplxGridDev& grid, const SmplxBfsDev& bfs, bool gd_from_h, ExpandLds& Y,
                                              int lane, int nv, int nprims, double parent_q, int h)
{
    round_stage(Y, lane, nv, nprims, parent_q);
    return round_gate(M, A, G, grid, bfs, gd_from_h, Y, lane, nprims, h);
}

// Pairs among the successors of one expansion for which `member` holds (successors whose coordinate the table does not
// know), by the whole wave: dup_of = the lowest earlier member with the lane's coordinate (that primitive creates the state),
// else -1; clash = an earlier member that is nobody's duplicate ended its probe at the lane's empty slot.
__device__ __forceinline__ void book_find_pairs(const ExpandLds& X, int lane, int nv, bool member, unsigned int hash,
                                                unsigned int free_slot, int& dup_of, bool& clash)
{
    dup_of = -1;
    clash = false;
    unsigned long long members = __ballot(member);
    while (members) {                                    // uniform
        const int j = __ffsll((long long)members) - 1;
        members &= members - 1;
        const unsigned int hj = wave_rlu(hash, j);
        if (j < lane && member && dup_of < 0 && hj == hash) {
            bool same = true;
            for (int v = 0; v < nv; ++v) same = same && X.coord[j][v] == X.coord[lane][v];
            if (same) dup_of = j;
        }
    }
    const bool mine = member && dup_of < 0;
    members = __ballot(mine);
    while (members) {
        const int j = __ffsll((long long)members) - 1;
        members &= members - 1;
        const unsigned int fj = wave_rlu(free_slot, j);
        if (j < lane && mine && fj == free_slot) clash = true;
    }
}

// getOrCreateState's table side (manip_lattice.cpp:1302-1354) for the successors of one expansion, by a whole wave (lane =
// primitive; every lane calls): hash and probe of each candidate's coordinate, the search state of a coordinate the table
// knows, and among the unknown ones the pairs that share a coordinate (the lower primitive creates the state) or whose
// probing ended at the same empty slot.  WithGoalFK: the planning-link FK / BFS cell / goal test of the successor is done
// here, between the probe's loads and their use (the search wave without a helper wave); otherwise b holds them already.
struct BookRegs { unsigned int hash; TableProbe pr; int dup_of; bool clash; };
template <bool WithGoalFK>
__device__ __forceinline__ void search_book_table(const ModelLds* __restrict__ M, const SmplxGridDev& grid, const SmplxBfsDev& bfs,
                                                  const SmplxGoalDev& G, const SmplxTableDev& table, SMPLX_GLOBAL_AS SmplxSState* st,
                                                  ExpandLds& X, int lane, int nv, bool act, BookLane& b, BookRegs& o, SmplxSState& ss)
{
    o.hash = 0; o.pr.id = -1; o.pr.free_slot = 0;
    if (act && b.limits_ok) {
        // getHashEntry (manip_lattice.cpp:1302-1316): the home slot's loads travel behind the planning-link FK; a coordinate the
        // table knows has its search state requested at once (it lands behind the waypoint lanes)
        o.hash = coord_hash_lds((const LDS_AS int*)X.coord[lane], nv);
        TableProbeLoads ld = table_probe_start(table, nv, o.hash);
        if constexpr (WithGoalFK) expand_book_goal(M, grid, bfs, G, X, lane, b);
        o.pr = table_probe_finish(table, ld, (const LDS_AS int*)X.coord[lane], nv);
        if (o.pr.id >= 0 && (!WithGoalFK || !b.is_goal)) ss = sstate_load(&st[o.pr.id]);   // (a goal successor takes the goal's state)
    }
    book_find_pairs(X, lane, nv, act && b.limits_ok && o.pr.id < 0, o.hash, o.pr.free_slot, o.dup_of, o.clash);
}

// what the helper wave leaves for the search wave at the end of a round: lane = primitive
struct BookOut {
    int limits_ok[64], wcount[64], h[64], is_goal[64];
    unsigned int hash[64], free_slot[64];
    int pr_id[64], dup_of[64], clash[64];
    int ss[8][64];                         // the successor's search state as stored (sstate_load's two 16-byte words)
};
__device__ __forceinline__ void book_out_store(BookOut& Bo, int p, const BookLane& b, const BookRegs& o, const SmplxSState& ss)
{
    Bo.limits_ok[p] = b.limits_ok ? 1 : 0; Bo.wcount[p] = b.W; Bo.h[p] = b.h; Bo.is_goal[p] = b.is_goal;
    Bo.hash[p] = o.hash; Bo.free_slot[p] = o.pr.free_slot; Bo.pr_id[p] = o.pr.id; Bo.dup_of[p] = o.dup_of; Bo.clash[p] = o.clash ? 1 : 0;
    Bo.ss[0][p] = (int)ss.g; Bo.ss[1][p] = (int)ss.h; Bo.ss[2][p] = (int)ss.f; Bo.ss[3][p] = (int)ss.eg;
    Bo.ss[4][p] = ss.bp; Bo.ss[5][p] = ss.heap_index;
    Bo.ss[6][p] = (int)((unsigned int)ss.iteration_closed | ((unsigned int)ss.call_number << 16)); Bo.ss[7][p] = (int)ss.flags;
}
__device__ __forceinline__ void book_out_load(const BookOut& Bo, int p, BookLane& b, BookRegs& o, SmplxSState& ss)
{
    b.limits_ok = Bo.limits_ok[p] != 0; b.W = Bo.wcount[p]; b.h = Bo.h[p]; b.is_goal = Bo.is_goal[p];
    o.hash = Bo.hash[p]; o.pr.free_slot = Bo.free_slot[p]; o.pr.id = Bo.pr_id[p];
    o.dup_of = Bo.dup_of[p]; o.clash = Bo.clash[p] != 0;
    ss.g = (unsigned int)Bo.ss[0][p]; ss.h = (unsigned int)Bo.ss[1][p]; ss.f = (unsigned int)Bo.ss[2][p];
    ss.eg = (unsigned int)Bo.ss[3][p]; ss.bp = Bo.ss[4][p]; ss.heap_index = Bo.ss[5][p];
    const unsigned int itc = (unsigned int)Bo.ss[6][p];
    ss.iteration_closed = (unsigned short)(itc & 0xFFFFu); ss.call_number = (unsigned short)(itc >> 16);
    ss.flags = (unsigned int)Bo.ss[7][p];
}

// The OPEN / INCONS operation of a successor whose g has just improved (arastar.cpp:555-566), by the whole wave with
// uniform arguments: state `id` with the new key f, its `flags`, whether it had been reached before in this call (only
// then can it be in OPEN) and whether it is closed in this iteration.  Not closed: its position is read where the sifts
// keep it current, behind a fence that lets earlier sifts' stores land; it sifts up from there (decrease), or it is pushed
// with the ancestor cache (`ac_complete`: the cache holds every HBM-resident ancestor the pushes read; the fence stands in
// where it does not).  Closed: appended to INCONS.
__device__ __forceinline__ void open_improve_wave(const HeapRef& H, SearchLds& W, SearchRegs& R, const SmplxSearchDev* P, int lane, int id,
                                                  unsigned int f, unsigned int flags, bool reached_before, bool closed_now, bool ac_complete)
{
    if (closed_now) {
        if (lane == 0) as_global(P->incons)[R.n_incons] = id;      // (never marked: arastar.cpp:563-565)
        ++R.n_incons;
        return;
    }
    if (id == 0) R.goal_f = f;
    // a state reached for the first time in this call is not in OPEN
    int hi = 0;
    if (reached_before || !ac_complete) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // earlier sifts' stores have landed
    if (reached_before) hi = as_global(P->st)[id].heap_index;
    const hent_t e = hent_make(f, id);
    if (hi != 0) {
        if (flags & 1u) heap_refresh_duplicates_wave(H, W, lane, R.heap_size, id, f);
        heap_sift_up_wave(H, W, lane, hi, e, false);
    } else {
        if ((flags & 1u) && R.dup_pushes > 0) heap_refresh_duplicates_wave(H, W, lane, R.heap_size, id, f);
        ++R.heap_size;
        heap_sift_up_wave(H, W, lane, R.heap_size, e, true);
    }
}

extern "C" __global__ void __launch_bounds__(512)
k_search(const SmplxSpaceDev* const* __restrict__ stab, int max_steps, int lh, int* __restrict__ status_out, long long pre_ticks)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ ExpandLds Xb[2];                  // two evaluations can be open: the one being committed and the next, speculative one
    __shared__ SearchLds W;
    __shared__ SmplxSearchDev Ph;                // the query's header as the launch found it: pointers, capacities, parameters
    __shared__ SmplxGoalDev Gh;                  // ... and the goal
    __shared__ BookOut Bo;                       // helper wave -> search wave, once per round
    __shared__ SmplxActionsDev Ah;               // the primitives: read by the search wave several times per expansion, each read a round trip to L2 otherwise
    static_assert(2 * sizeof(ExpandLds) + sizeof(SearchLds) + sizeof(SmplxSearchDev) + sizeof(SmplxActionsDev) + sizeof(SmplxGoalDev) + sizeof(BookOut) <= SMPLX_SEARCH_STATIC_LDS, "engine.hip budgets this much static LDS");
    const SmplxSpaceDev* Sq = stab[blockIdx.x];
    const SmplxSpaceDev* S = stab[0];            // scene, robot and primitives are shared by the queries of a launch
    SmplxSearchDev* const Pd = Sq->search;
    const int t = threadIdx.x;
    {
        const int st0 = Pd->status;
        if (st0 == SMPLX_SS_DONE || st0 == SMPLX_SS_ERROR) {   // uniform: this query needs nothing more
            if (t == 0 && status_out) status_out[blockIdx.x] = st0;
            return;
        }
    }
    for (int i = t; i < (int)(sizeof(SmplxSearchDev) / 4); i += blockDim.x) ((int*)&Ph)[i] = ((const int*)Pd)[i];
    for (int i = t; i < (int)(sizeof(SmplxActionsDev) / 4); i += blockDim.x) ((int*)&Ah)[i] = ((const int*)&S->actions)[i];
    for (int i = t; i < (int)(sizeof(SmplxGoalDev) / 4); i += blockDim.x) ((int*)&Gh)[i] = ((const int*)&Sq->goal)[i];
    if (t == 0) { W.action = SA_SKIP; W.buf = 0; W.seq = 0; W.go = 0; W.helper_gave_up = 0; W.ac_nlev = 0; }
    __syncthreads();
    const SmplxSearchDev* const P = &Ph;         // read-only view; what changes lives in the search wave and goes back to Pd at the end
    const SmplxActionsDev& A = Ah;
    const SmplxGoalDev& G = Gh;
    const int nprims = A.nprims;
    const int ncfg = nprims * SMPLX_SMALL_LANES + 1;          // config lanes (the last one: the state itself)
    const int book0 = (ncfg + 63) / 64 * 64;                  // first thread of the search wave
    ModelLds Mv;
#ifdef SMPLX_CONST_MODEL
    constexpr bool RS = true;        // the waypoint lanes keep the saved link transforms in registers (sphere_checks.h const_chain<.., true>)
#else
    constexpr bool RS = false;
#endif
    ThreadLds L = setup_lds(S, smem, &Mv, book0, !RS);        // per-thread scratch for the config waves only (nobody else walks a chain through LDS)
    Mv.bodies = Sq->bodies;                                   // attached bodies are the query's own
    const ModelLds* M = &Mv;
    const SmplxGridDev grid = S->grid;
    const SmplxBfsDev bfs = Sq->bfs;
    const SmplxTableDev table = Sq->table;
    const int nv = MV_NVARS(M);
    HeapRef H;
    {
        // the heap cache sits behind the model and the per-thread scratch of the expansion (setup_lds)
#ifdef SMPLX_CONST_MODEL
        const int nroot_lds = 0;
#else
        const int nroot_lds = Mv.nroot;
#endif
        const int* hdr = reinterpret_cast<const int*>(S->model_blob);
        unsigned int off = (unsigned int)hdr[SMPLX_BH_BYTES] +
                           (unsigned int)((3 * nroot_lds + 12 * (RS ? 0 : Mv.nslots) + Mv.nvars) * 8 + hdr[SMPLX_BH_STACK]) * (unsigned int)book0;
        off = (off + 15u) & ~15u;
        H.lds = (LDS_AS hent_t*)((LDS_AS unsigned char*)smem + off);
        H.hbm = (SMPLX_GLOBAL_AS hent_t*)as_global(P->heap);
        H.st = as_global(P->st);
        H.lh = lh;
    }
    {
        const int n = P->heap_size + 1 < lh ? P->heap_size + 1 : lh;
        for (int i = t; i < n; i += blockDim.x) H.lds[i] = H.hbm[i];
    }
    __syncthreads();

    // The wave behind the search wave, where the block has one (smplx_search_block): between the two barriers of a round it
    // does the bookkeeping of the round's successors that does not touch OPEN -- coordinates, heuristic (planning-link FK + BFS
    // cell), goal test, the state table's side of getOrCreateState -- and leaves it in Bo for the search wave, whose own
    // sequential work per expansion (pop, commit, relax) is what bounds the kernel.
    const int help0 = book0 + 64;
    const bool has_helper = (int)blockDim.x > help0;
    if (t < book0 || t >= help0) {
        // =============================== the config waves (and the helper wave) ===============================
        while (true) {
            __syncthreads();                                       // A: the step is published
            const int action = W.action;
            if (action == SA_EXIT) break;
            if (action == SA_EVAL) {
                ExpandLds& Xr = Xb[W.buf];
                if (t < book0) expand_config_lane<RS>(M, L, A, G, grid, Xr, t, ncfg);
                else {
                    // lane p = primitive p, as in the search wave.  First what needs no table: coordinate, planning-link FK, BFS
                    // cell, goal test.  Then -- once the search wave says the table holds everything committed before this round's
                    // state was popped (W.go) -- hash, probe, the known successor's search state, duplicates among the new ones.
                    const int p = t - help0;
                    const bool act = p < nprims && Xr.lookups[p] != 0;   // (lookups[p]: the search wave's "primitive p has an action here")
                    BookLane r;
                    r.limits_ok = false; r.W = 0; r.h = 0; r.is_goal = 0;
                    if (act) {
                        expand_book_coords(M, Xr, p, r);
                        expand_book_goal(M, grid, bfs, G, Xr, p, r);
                    }
                    const int my_round = W.seq;
                    // (bounded: ~a second; the search wave sets go before it joins the round's end on every path, so the bound is
                    // never met -- it is there so that no wave of this kernel can wait for ever)
                    for (int spins = 0; __atomic_load_n(&W.go, __ATOMIC_RELAXED) != my_round; ++spins) {
                        __builtin_amdgcn_s_sleep(2);
                        if (spins > (1 << 24)) { W.helper_gave_up = 1; break; }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    BookRegs o;
                    SmplxSState ss = sstate_blank();
                    search_book_table<false>(M, grid, bfs, G, table, as_global(P->st), Xr, p, nv, act, r, o, ss);
                    book_out_store(Bo, p, r, o, ss);
                }
            }
            if (action == SA_REORDER) {
                // heap_rekey_block (search_heap.h), which the search wave calls at the same moment with the same size, epsilon
                // and duplicates (it runs that function's barriers against the ones below), written out: called here,
                // the per-robot build of scenes.mixed_kinds_robot() needs 16 bytes of scratch and two VGPR spills more
                // (profiles/search_kernel_pieces_ab.txt).  The two must stay the same loop and the same barriers.
                const int size = W.reorder_size;
                const double eps = W.reorder_eps;
                for (int i = 1 + t; i <= size; i += blockDim.x) {     // f of every OPEN entry under the new epsilon (arastar.cpp:571-577)
                    const int eid = hent_id(hget(H, i));
                    SMPLX_GLOBAL_AS SmplxSState* ss = &as_global(P->st)[eid];
                    const unsigned int f = search_key(eps, ss->g, ss->h);
                    ss->f = f;
                    hput(H, i, hent_make(f, eid));
                }
                __syncthreads();
                heap_make_block(H, size, W.reorder_dups > 0);
            }
            __syncthreads();                                       // B: the waypoint verdicts have landed
        }
    } else {
        // =============================== the search wave ===============================
        const int lane = t - book0;
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        SearchRegs R = search_regs_load(P, max_steps);
        long long ticks[8];
        for (int k = 0; k < 8; ++k) ticks[k] = P->ticks[k];
        long long tick = (long long)wall_clock64();
        const long long t_start = P->t_start != 0 ? P->t_start : tick - pre_ticks;     // the call's start (wall-clock budget)
#define SK_TICK(k) do { const long long now_ = (long long)wall_clock64(); ticks[k] += now_ - tick; tick = now_; } while (0)

        if (R.phase == 0) {
            // ---- ARAStar::replan, from scratch (arastar.cpp:107-167): empty OPEN and INCONS, new call number, the start
            // state with g = 0 into OPEN ----
            R.heap_size = 0; R.n_incons = 0; R.n_log = 0;
            R.call_number = (R.call_number + 1) & 0xFFFF;
            if (R.call_number == 0) R.call_number = 1;
            SmplxSState ss = sstate_load(&as_global(P->st)[P->start_id]), gs = sstate_load(&as_global(P->st)[0]);
            sstate_reinit(ss, R.call_number);
            sstate_reinit(gs, R.call_number);
            R.iteration = 1;
            R.curr_eps = P->initial_eps;
            R.satisfied_eps = __builtin_inf();
            ss.g = 0;
            ss.f = search_key(R.curr_eps, ss.g, ss.h);
            R.goal_f = P->start_id == 0 ? ss.f : gs.f;
            R.heap_size = 1;
            if (lane == 0) {
                sstate_store(&as_global(P->st)[P->start_id], ss, true);
                if (P->start_id != 0) sstate_store(&as_global(P->st)[0], gs, true);
                hset(H, 1, hent_make(ss.f, P->start_id));
            }
            R.num = 0; R.err = 0; R.expand_count = 0; R.expand_count_init = 0; R.dup_pushes = 0;
            R.phase = 1;
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        }
        // the goal distance of a state follows from its heuristic when h = cost_per_cell * BFS distance is invertible
        // (bfs_heuristic.cpp:129-138 / 355-366: both read the BFS cell of the same planning-link position)
        const int cpc = bfs.cost_per_cell;
        // -- of the BFS kind only: a closed-form h says nothing of the gate's distance (lattice_steps.h closed_form_of), so
        // such a space takes the path beside it, metric_goal_distance: the FK (Euclidean) or the constant 0 (joint distance)
        const bool gd_from_h = closed_form_of(bfs) == nullptr && cpc > 0 && (32767 % cpc) != 0;
        // The next expansion, started early.  An evaluation round (barrier A .. barrier B) keeps the config waves busy for
        // ~14 us while this wave only fills in the bookkeeping, and committing and relaxing a step (~7 us) plus the next pop
        // (~4 us) kept THEM idle.  GetSuccs is a pure function of a state's joint values, so as soon as the verdicts of a
        // step are in, this wave guesses the state the next pop will return -- the best new successor, if it beats the top
        // of OPEN -- and opens the round for it in the other ExpandLds; the relaxation and the pop run beside it.  A right
        // guess is adopted (the round is already under way), a wrong one is waited out and dropped: results never depend
        // on it.  pend: the state whose round is open and not joined yet (-1: none), pbuf its buffer, p_act its lanes.
        int pend = -1, pbuf = 0;
        int round_seq = 0;               // number of the last round opened (W.seq)
        bool p_act = false;
        long long spec_issued = 0, spec_hits = 0;

        while (true) {
            // =========================== what happens next (ARAStar::replan / improvePath) ===========================
            int action = -1, m = 0;
            while (action < 0) {
                if (R.phase == 3) { action = SA_EXIT; break; }                          // finished; the path did not fit (below)
                if (R.phase == 1) {
                    // arastar.cpp:169-186
                    if (!(R.satisfied_eps > P->final_eps)) { R.phase = 3; action = SA_EXIT; break; }
                    if (R.curr_eps == R.satisfied_eps) {
                        if (!P->improve) { R.phase = 3; action = SA_EXIT; break; }
                        if (R.heap_size + R.n_incons > P->cap_heap) { R.status = SMPLX_SS_GROW; R.grow_what = 1; action = SA_EXIT; break; }
                        action = SA_REORDER;
                        break;
                    }
                    R.phase = 2;
                }
                // ---- one step of improvePath (arastar.cpp:486-527) ----
                int err = -1;
                hent_t top = 0;
                if (R.heap_size == 0) err = 5;                                          // EXHAUSTED_OPEN_LIST
                else {
                    top = hget(H, 1);
                    bool timed_out = false;
                    if (P->bounded) {
                        const bool init = R.satisfied_eps == __builtin_inf();
                        if (P->time_wall) timed_out = tick - t_start >= (init ? P->budget_init : P->budget_rep);   // (tick: end of the last step)
                        else timed_out = init ? R.num >= P->max_init : R.num >= P->max_rep;
                    }
                    if (hent_f(top) >= R.goal_f || hent_id(top) == 0) err = 0;          // SUCCESS
                    else if (timed_out) err = 4;                                        // TIMED_OUT
                }
                if (err >= 0) {
                    // back in replan (arastar.cpp:188-197)
                    if (R.curr_eps == P->initial_eps) R.expand_count_init += R.num;
                    R.phase = 1;
                    R.err = err;
                    if (err != 0) { R.phase = 3; action = SA_EXIT; break; }
                    R.satisfied_eps = R.curr_eps;
                    continue;
                }
                if (R.steps_left <= 0) { action = SA_EXIT; break; }                      // this launch has done its share
                // room for one more expansion?  (checked before anything is popped: the host enlarges and launches again)
                if (R.nstates + nprims > P->cap_states || R.heap_size + nprims > P->cap_heap || R.n_incons + nprims > P->cap_incons ||
                    R.n_log + 1 > P->cap_log || R.n_succ + nprims > P->cap_succ || (unsigned int)(2 * (R.nstates + nprims)) > table.mask + 1u) {
                    R.status = SMPLX_SS_GROW; R.grow_what = 2;
                    action = SA_EXIT;
                    break;
                }
                --R.steps_left;
                m = hent_id(top);
                action = SA_EVAL;
            }

            if (action != SA_EVAL && pend >= 0) {                                    // B of a round nobody will use
                if (lane == 0) __atomic_store_n(&W.go, round_seq, __ATOMIC_RELAXED);
                __syncthreads();
                pend = -1;
            }
            if (action == SA_EXIT) {
                if (lane == 0) W.action = SA_EXIT;
                __syncthreads();                                   // A
                break;
            }

            if (action == SA_REORDER) {
                // =========================== a new epsilon (arastar.cpp:174-186, 571-577) ===========================
                ++R.iteration;
                R.curr_eps -= P->delta_eps;
                R.curr_eps = R.curr_eps > P->final_eps ? R.curr_eps : P->final_eps;
                for (int i = 0; i < R.n_incons; ++i) {
                    const int sid = as_global(P->incons)[i];
                    const SmplxSState ss = sstate_load(&as_global(P->st)[sid]);
                    if (ss.heap_index != 0) {                       // already in OPEN: the same element twice from now on
                        if (lane == 0) as_global(P->st)[sid].flags = ss.flags | 1u;
                        ++R.dup_pushes;
                    }
                    ++R.heap_size;
                    heap_sift_up_wave(H, W, lane, R.heap_size, hent_make(ss.f, sid), false);
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");   // the next push reads what this one stored
                }
                R.n_incons = 0;
                if (lane == 0) { W.action = SA_REORDER; W.reorder_size = R.heap_size; W.reorder_eps = R.curr_eps; W.reorder_dups = R.dup_pushes; }
                __syncthreads();                                   // A
                heap_rekey_block(H, as_global(P->st), R.heap_size, R.curr_eps, R.dup_pushes > 0);
                __syncthreads();                                   // B
                R.goal_f = as_global(P->st)[0].f;      // (the goal state is re-initialised when a call starts: its f is this call's)
                R.phase = 2;
                SK_TICK(5);
                continue;
            }

            // =========================== expand state m (arastar.cpp:513-519, 531-568) ===========================
            // ---- pop (intrusive_heap.hpp:155-166).  The state popped is very often one the previous relaxation has just
            // stored (another lane of this wave did): those stores have landed before it is read ----
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            // ... and so has everything the previous step committed: the helper wave of an open round may read the table now
            if (pend >= 0 && lane == 0) __atomic_store_n(&W.go, round_seq, __ATOMIC_RELAXED);
            const SmplxSState sm = sstate_load(&as_global(P->st)[m]);           // g, h: in flight together with the loads below
            const hent_t last = hget(H, R.heap_size);
            const int off = as_global(P->done_off)[m];                          // >= 0: expanded before (a later ARA* iteration)
            const int dcnt = as_global(P->done_cnt)[m];
            const bool use_spec = pend == m && off < 0;                         // (only states never expanded are guessed)
            const int cur = use_spec ? pbuf : (pend >= 0 ? pbuf ^ 1 : 0);
            ExpandLds& X = Xb[cur];
            if (!use_spec) round_stage(X, lane, nv, nprims, lane < nv ? as_global(P->q)[(size_t)m * nv + lane] : 0.0);
            heap_pop_wave(H, lane, m, R.heap_size, last);
            // the new top of OPEN is what the NEXT pop returns unless this step puts something above it: its joint values and
            // heuristic are requested now and looked at when the guess is made (below), a whole evaluation later
            int top_id = -1, top_off = 0;
            unsigned int top_f = 0xFFFFFFFFu, top_h = 0;
            double top_q = 0.0;
            if (R.heap_size >= 1) {
                const hent_t tp = hget(H, 1);
                top_id = hent_id(tp);
                top_f = hent_f(tp);
                top_off = as_global(P->done_off)[top_id];
                top_h = as_global(P->st)[top_id].h;
                if (lane < nv) top_q = as_global(P->q)[(size_t)top_id * nv + lane];
            }
            const unsigned int eg = sm.g;
            if (lane == 0) {
                *(SMPLX_GLOBAL_AS unsigned int*)&as_global(P->st)[m].iteration_closed = ((unsigned int)R.iteration & 0xFFFFu) | ((unsigned int)sm.call_number << 16);
                as_global(P->st)[m].eg = eg;
                as_global(P->log)[R.n_log] = m;
            }
            ++R.n_log;
            SK_TICK(1);

            // per-lane data of this step: lane p < nprims = primitive p (evaluation), lane k < cnt = list entry k (cached)
            bool valid = false;
            bool ac_complete = true;     // the ancestor cache holds every HBM-resident ancestor the pushes will read
            int sid = -1, cost = 0, cnt = 0, evals = 0;
            SmplxSState ss = sstate_blank();                         // the successor's search state

            if (off < 0) {
                // ---- GetSuccs loop body (manip_lattice.cpp:254-305): successors' joint values, then the waypoint lanes ----
                const bool in = lane < nprims;
                bool act;
                if (use_spec) {
                    // the round for this state is open already: its successor values are in X, its lanes at work
                    act = p_act;
                    pend = -1;
                    ++spec_hits;
                } else {
                    act = round_gate(M, A, G, grid, bfs, gd_from_h, X, lane, nprims, (int)sm.h);
                    if (pend >= 0) { __syncthreads(); pend = -1; }   // B of the round that guessed wrong
                    ++round_seq;
                    if (lane == 0) { W.action = SA_EVAL; W.buf = cur; W.seq = round_seq; W.go = round_seq; }
                    __syncthreads();                                 // A
                }
                BookLane b;
                b.limits_ok = false; b.W = 0; b.h = 0; b.is_goal = 0;
                BookRegs bk;
                bk.hash = 0; bk.pr.id = -1; bk.pr.free_slot = 0; bk.dup_of = -1; bk.clash = false;
                if (!has_helper) {
                    // While the waypoint lanes work: everything of getOrCreateState that does not need their verdict
                    if (act) expand_book_coords(M, X, lane, b);
                    search_book_table<true>(M, grid, bfs, G, table, as_global(P->st), X, lane, nv, act, b, bk, ss);
                }
                const SmplxSState goal_ss = sstate_load(&as_global(P->st)[0]);   // (a goal successor relaxes the goal state)
                ac_complete = ancestor_cache_fill(H, W, lane, R.heap_size, __popcll(__ballot(act)));       // (an upper bound of the pushes to come)
                // ---- while the waypoint lanes finish: the round of the most likely next state, the top of OPEN, is got ready in
                // the other buffer (its successors' joint values), so that it can be opened the moment this round closes ----
                const int nxt = cur ^ 1;
                bool top_ready = false, top_act = false;
                if (top_id > 0 && top_off < 0 && top_f < R.goal_f && R.steps_left > 0) {
                    top_act = round_prepare(M, A, G, grid, bfs, gd_from_h, Xb[nxt], lane, nv, nprims, top_q, (int)top_h);
                    top_ready = true;
                }
                __syncthreads();                                     // B: the waypoint verdicts have landed
                SK_TICK(2);
                if (has_helper && W.helper_gave_up) R.steps_left = 0;      // leave at the next selection; the status says why (below)
                if (has_helper && in) book_out_load(Bo, lane, b, bk, ss);
                const bool cand = act && b.limits_ok;
                unsigned int hash = bk.hash;
                TableProbe pr = bk.pr;
                int dup_of = bk.dup_of;
                bool clash = bk.clash;
                {
                    // No edge that could create a state has a key below the top's (whatever the verdicts say): the next pop
                    // returns that top, and its round opens at once.  Otherwise the guess waits for the verdicts (below).
                    const bool maybe_new = cand && pr.id < 0 && !b.is_goal;
                    const unsigned int fj = maybe_new ? search_key(R.curr_eps, eg + (unsigned int)A.cost[lane], (unsigned int)b.h) : 0xFFFFFFFFu;
                    if (top_ready && __ballot(maybe_new && fj < top_f) == 0ull) {
                        ++round_seq;
                        if (lane == 0) { W.action = SA_EVAL; W.buf = nxt; W.seq = round_seq; }
                        __syncthreads();                             // A of the guessed round
                        pend = top_id;
                        pbuf = nxt;
                        p_act = top_act;
                        ++spec_issued;
                    }
                }
                int lookups = 0;
                const int flags = in ? expand_verdict(A, X, lane, act, b, lookups) : SMPLX_F_INACTIVE;
                valid = (flags & SMPLX_F_VALID) != 0;
                const bool goal_succ = valid && (flags & SMPLX_F_GOAL) != 0;
                int id = pr.id;
                // ---- getOrCreateState (manip_lattice.cpp:1318-1354) ----
                const bool unknown = valid && id < 0;
                if (!unknown) dup_of = -1;
                {
                    // a candidate that was to create the state for a later one turned out to collide (rare): the pairs again,
                    // among the valid successors only.  This is book_find_pairs(X, lane, nv, unknown, hash, pr.free_slot, dup_of,
                    // clash) written out: called here, the generic build needs 16 bytes of scratch and seven VGPR spills
                    // more (profiles/search_kernel_pieces_ab.txt).  The two must stay the same loops.
                    const bool root_valid = __shfl((int)valid, dup_of >= 0 ? dup_of : lane) != 0;
                    if (__ballot(unknown && dup_of >= 0 && !root_valid)) {
                        dup_of = -1;
                        unsigned long long members = __ballot(unknown);
                        while (members) {                            // uniform
                            const int j = __ffsll((long long)members) - 1;
                            members &= members - 1;
                            const unsigned int hj = wave_rlu(hash, j);
                            if (j < lane && unknown && dup_of < 0 && hj == hash) {
                                bool same = true;
                                for (int v = 0; v < nv; ++v) same = same && X.coord[j][v] == X.coord[lane][v];
                                if (same) dup_of = j;
                            }
                        }
                        const bool mine = unknown && dup_of < 0;
                        clash = false;
                        members = __ballot(mine);
                        while (members) {
                            const int j = __ffsll((long long)members) - 1;
                            members &= members - 1;
                            const unsigned int fj = wave_rlu(pr.free_slot, j);
                            if (j < lane && mine && fj == pr.free_slot) clash = true;
                        }
                    }
                }
                const bool is_new = unknown && dup_of < 0;
                if (!is_new) clash = false;
                const unsigned long long m_new = __ballot(is_new), m_valid = __ballot(valid), m_eval = __ballot(in && !(flags & SMPLX_F_INACTIVE));
                if (is_new) {
                    id = R.nstates + __popcll(m_new & below);
                    if (!clash) table_store_own(table, pr.free_slot, (const LDS_AS int*)X.coord[lane], nv, id);
                    for (int v = 0; v < nv; ++v) { as_global(P->coord)[(size_t)id * nv + v] = X.coord[lane][v]; as_global(P->q)[(size_t)id * nv + v] = X.sq[lane][v]; }
                    ss.h = (unsigned int)b.h;
                    sstate_reinit(ss, R.call_number);
                    sstate_store(&as_global(P->st)[id], ss, true);              // (what the relaxation changes is stored again behind it)
                    as_global(P->done_off)[id] = -1;
                }
                {
                    unsigned long long m_clash = __ballot(clash);
                    while (m_clash) {      // uniform loop: one clashing lane at a time probes behind what the others have stored
                        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                        const int j = __ffsll((long long)m_clash) - 1;
                        m_clash &= m_clash - 1;
                        if (lane == j) {
                            TableProbeLoads ld = table_probe_start(table, nv, hash);
                            const TableProbe p2 = table_probe_finish(table, ld, (const LDS_AS int*)X.coord[lane], nv);
                            table_store_own(table, p2.free_slot, (const LDS_AS int*)X.coord[lane], nv, id);
                        }
                    }
                }
                {
                    const int id_of_dup = __shfl(id, dup_of >= 0 ? dup_of : lane);
                    if (dup_of >= 0) id = id_of_dup;
                }
                cnt = __popcll(m_valid);
                evals = __popcll(m_eval);
                if (valid) {
                    sid = goal_succ ? 0 : id;      // a goal successor is reported as the goal id (manip_lattice.cpp:283-296)
                    cost = A.cost[lane];
                    if (goal_succ) ss = goal_ss;
                    // (id, cost | primitive << 24) as one 8-byte store
                    ((SMPLX_GLOBAL_AS unsigned long long*)as_global(P->succ))[R.n_succ + __popcll(m_valid & below)] =
                        (unsigned long long)(unsigned int)sid | ((unsigned long long)(unsigned int)(cost | (lane << 24)) << 32);
                }
                if (lane == 0) { as_global(P->done_off)[m] = R.n_succ; as_global(P->done_cnt)[m] = cnt | (evals << 8); }
                if (pend < 0) {
                    // ---- the guess (see above): the new successor with the least f if it beats the top of OPEN (a push does
                    // not pass an equal key: intrusive_heap.hpp:346-365), else that top ----
                    const bool cand = valid && is_new && !goal_succ;
                    const unsigned int fj = cand ? search_key(R.curr_eps, eg + (unsigned int)cost, ss.h) : 0xFFFFFFFFu;
                    unsigned long long key = ((unsigned long long)fj << 8) | (unsigned long long)lane;      // ties: the lower primitive
                    for (int o = 32; o > 0; o >>= 1) {
                        const unsigned long long other = __shfl_xor(key, o);
                        key = other < key ? other : key;
                    }
                    const unsigned int fbest = (unsigned int)(key >> 8);
                    const int jbest = (int)(key & 0xFFull);
                    const bool guess_succ = fbest != 0xFFFFFFFFu && fbest < top_f && fbest < R.goal_f;
                    const bool guess_top = !guess_succ && top_id > 0 && top_off < 0 && top_f < R.goal_f;
                    if ((guess_succ || guess_top) && R.steps_left > 0) {
                        double guess_q = top_q;
                        if (guess_succ && lane < nv) guess_q = X.sq[jbest][lane];
                        const int guess_h = guess_succ ? wave_rl((int)ss.h, jbest) : (int)top_h;
                        p_act = round_prepare(M, A, G, grid, bfs, gd_from_h, Xb[nxt], lane, nv, nprims, guess_q, guess_h);
                        ++round_seq;
                        if (lane == 0) { W.action = SA_EVAL; W.buf = nxt; W.seq = round_seq; }
                        __syncthreads();                             // A of the guessed round
                        pend = guess_succ ? wave_rl(sid, jbest) : top_id;
                        pbuf = nxt;
                        ++spec_issued;
                    }
                }
                R.n_succ += cnt;
                R.nstates += __popcll(m_new);
                R.gpu_evals += evals;
                {
                    int lk = in ? lookups : 0;       // grid lookups of this expansion, as the reference would count them
                    for (int o = 32; o > 0; o >>= 1) lk += __shfl_down(lk, o);
                    R.lookups += wave_rl(lk, 0);
                }
            } else {
                // ---- GetSuccs of a state expanded before: the committed list (no evaluation round) ----
                if (pend >= 0) { __syncthreads(); pend = -1; }       // B of the round that guessed wrong
                cnt = dcnt & 0xFF;
                evals = dcnt >> 8;
                valid = lane < cnt;
                if (valid) {
                    const unsigned long long sc = ((const SMPLX_GLOBAL_AS unsigned long long*)as_global(P->succ))[off + lane];
                    const int sc_cost_prim = (int)(unsigned int)(sc >> 32);
                    sid = (int)(unsigned int)sc;
                    cost = sc_cost_prim & 0xFFFFFF;
                    ss = sstate_load(&as_global(P->st)[sid]);
                }
                ac_complete = ancestor_cache_fill(H, W, lane, R.heap_size, cnt);
                SK_TICK(2);
            }

            // ---- which successors name the same state (two goal successors; a primitive that lands in an earlier one's
            // cell): the earliest lane keeps the state, the others refer to it ----
            const unsigned long long m_succ = __ballot(valid);
            int alias = -1;
            {
                unsigned long long rest = m_succ;
                while (rest) {
                    const int j = __ffsll((long long)rest) - 1;
                    rest &= rest - 1;
                    const int sj = wave_rl(sid, j);
                    if (valid && j < lane && alias < 0 && sj == sid) alias = j;
                }
            }
            // what earlier lanes of this wave stored (heap entries moved by the pop, the popped state's closing, new states'
            // rows) and others read below (a self-loop successor, the ancestor cache) has landed
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            SK_TICK(3);

            // ---- ARAStar::expand's loop over the successors, in primitive order (arastar.cpp:540-567): uniform control
            // flow, the state of successor j in the registers of lane j ----
            R.committed_evals += evals;
            bool dirty = false;
            if (__ballot(valid && alias >= 0) == 0ull) {
                // No two successors name the same state (nearly always): what expand's loop decides for a successor then depends
                // on that successor alone, so every lane works it out for its own -- reinitSearchState, the cost test, the key --
                // and the loop below only performs the OPEN / INCONS operations of the successors that improved, in
                // primitive order.  (The general loop further down costs ~0.37 us per successor, improved or not.)
                const bool fresh = valid && ss.call_number != (unsigned short)R.call_number;
                if (fresh) {
                    // reinitSearchState: not touched in this call (and so not in OPEN)
                    sstate_reinit(ss, R.call_number);
                    dirty = true;
                    as_global(P->st)[sid].heap_index = 0;
                }
                const unsigned int new_cost = eg + (unsigned int)cost;
                const bool improve = valid && new_cost < ss.g;
                const bool reached_before = ss.g != SMPLX_INFINITECOST;
                const bool closed_now = (unsigned int)ss.iteration_closed == ((unsigned int)R.iteration & 0xFFFFu);
                unsigned int f = 0;
                if (improve) {
                    ss.g = new_cost; ss.bp = m; dirty = true;
                    if (!closed_now) { f = search_key(R.curr_eps, new_cost, ss.h); ss.f = f; }
                }
                unsigned long long rest = __ballot(improve);
                while (rest) {
                    const int j = __ffsll((long long)rest) - 1;
                    rest &= rest - 1;
                    open_improve_wave(H, W, R, P, lane, wave_rl(sid, j), wave_rlu(f, j), wave_rlu(ss.flags, j),
                                      wave_rl((int)reached_before, j) != 0, wave_rl((int)closed_now, j) != 0, ac_complete);
                }
            } else {
                unsigned long long rest = m_succ;
                while (rest) {
                    const int j = __ffsll((long long)rest) - 1;
                    rest &= rest - 1;
                    const int aj = wave_rl(alias, j);
                    const int r = aj >= 0 ? aj : j;                  // the lane that keeps this successor's state
                    const int id = wave_rl(sid, j);
                    const int cj = wave_rl(cost, j);
                    unsigned int g_r = wave_rlu(ss.g, r);
                    const unsigned int h_r = wave_rlu(ss.h, r);
                    unsigned int itc_r = (unsigned int)wave_rl((int)ss.iteration_closed | ((int)ss.call_number << 16), r);
                    unsigned int flags_r = wave_rlu(ss.flags, r);
                    if ((itc_r >> 16) != (unsigned int)R.call_number) {
                        // reinitSearchState: not touched in this call (and so not in OPEN)
                        if (lane == r) { sstate_reinit(ss, R.call_number); dirty = true; }
                        if (lane == 0) as_global(P->st)[id].heap_index = 0;
                        g_r = SMPLX_INFINITECOST; itc_r = (unsigned int)R.call_number << 16; flags_r = 0;
                    }
                    const int new_cost = (int)(eg + (unsigned int)cj);
                    if (!((unsigned int)new_cost < g_r)) continue;
                    if (lane == r) { ss.g = (unsigned int)new_cost; ss.bp = m; dirty = true; }
                    const bool closed_now = (itc_r & 0xFFFFu) == ((unsigned int)R.iteration & 0xFFFFu);
                    unsigned int f = 0;
                    if (!closed_now) {
                        f = search_key(R.curr_eps, (unsigned int)new_cost, h_r);
                        if (lane == r) ss.f = f;
                    }
                    open_improve_wave(H, W, R, P, lane, id, f, flags_r, g_r != SMPLX_INFINITECOST, closed_now, ac_complete);
                }
            }
            if (dirty && valid && alias < 0) sstate_store(&as_global(P->st)[sid], ss, false);
            if (lane == 0) W.ac_nlev = 0;
            ++R.num;
            SK_TICK(4);
        }

        // ---- the launch ends: results, or the state the next launch picks up ----
        if (lane == 0) {
            int solved = Ph.solved, cost = Ph.cost, n_path = Ph.n_path;
            if (R.phase == 3) {
                // arastar.cpp:199-214: the goal's chain once there is a solution (also after a time-out while improving), else
                // with partial solutions allowed the chain of OPEN's minimum
                int from = -1;
                if (R.satisfied_eps != __builtin_inf()) from = 0;
                else if (Ph.allow_partial && R.heap_size > 0) from = hent_id(hget(H, 1));
                int n = 0;
                if (from >= 0) for (int sid = from; sid >= 0; sid = as_global(P->st)[sid].bp) ++n;
                if (n > P->cap_path) {
                    // the path does not fit: the host enlarges the buffer and launches again (phase 3 leaves at once)
                    R.status = SMPLX_SS_GROW; R.grow_what = 3;
                    n_path = n;
                } else {
                    R.expand_count += R.num;
                    R.status = SMPLX_SS_DONE;
                    if (from < 0) {
                        solved = 0; cost = 0; n_path = 0;
                    } else {
                        n = 0;
                        for (int sid = from; sid >= 0; sid = as_global(P->st)[sid].bp) as_global(P->path)[n++] = sid;
                        n_path = n;
                        cost = (int)as_global(P->st)[from].g;
                        solved = 1;
                    }
                    R.phase = 4;
                }
            }
            if (W.helper_gave_up) R.status = SMPLX_SS_ERROR;
            Pd->solved = solved; Pd->cost = cost; Pd->n_path = n_path;
            search_regs_store(Pd, R);
            Pd->t_start = t_start;
            SK_TICK(6);
            ticks[7] += (spec_issued << 32) + spec_hits;            // rounds opened on a guess | guesses the next pop confirmed
            for (int k = 0; k < 8; ++k) Pd->ticks[k] = ticks[k];
            if (status_out) status_out[blockIdx.x] = R.status;
            W.reorder_size = R.heap_size;                           // (for the write-back of the LDS part below)
        }
#undef SK_TICK
    }
    __syncthreads();
    {
        const int n = W.reorder_size + 1 < lh ? W.reorder_size + 1 : lh;
        for (int i = t; i < n; i += blockDim.x) H.hbm[i] = H.lds[i];
    }
}
