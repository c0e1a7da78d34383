// smpl_amd/csrc/step_block.h -- k_step_block: the waypoint-parallel frontier step (step_kernels.h) in ONE launch.
// Block b owns edges [128 b, 128 b + 128) of the (state, primitive) grid -- the edges block b of k_pipe_finish owns, so
// block_tab rows, compaction shards and per-block tallies keep their meaning -- and runs the pipeline's stages on them
// with everything between the stages in LDS instead of in HBM arrays and global atomics:
//   head       edge lanes load their parent's joint values and what their primitive's gate needs of the action record
//              (mprim_gate); the block stages the model image and the joint values of the (at most SMPLX_STEP_STATES, 7 at
//              M = 25) states its edges belong to
//   planning   the third wave is the goal-distance wave of k_pipe_setup (lane-parallel sincos -> the states' rows of sines
//              and cosines in LDS -> the chain); beside it the edge lanes run pipe_edge_values in registers and, per-robot
//              build, discretise an edge within limits
//   gate       one compare with the distance in LDS; successor joint values, waypoint counts and their prefix to LDS
//   successor  per-robot build, edge lanes only, behind the prefix's barrier: the rest of k_pipe_configs' successor role for
//              an edge that is active and within limits -- the loads of its home slot in the state table issued, chain, goal
//              test, heuristic, then the table id from the slot that has arrived meanwhile.  Only the verdict reads what it
//              leaves, so the goal-distance wave does not wait for it: that wave enters the collision phase at once
//   collision  n_states + sum(W - 1) items: the block's states at alpha 0, then (edge, waypoint) found by a search over the
//              prefix; one item is the fast path of k_pipe_configs.  Items are dealt in chunks of 64: chunk c goes to wave
//              NW - 1 - (c mod NW), NW = blockDim.x / 64, and a lane takes its lane's item of each of its wave's chunks.  The
//              goal-distance wave (wave NW - 1) is dealt first because it starts a successor evaluation ahead of the others:
//              at NW = 3 it owns chunks 0, 3, ..., so the ragged fourth chunk of a block of 193 .. 256 items runs beside the
//              edge waves' successor evaluation and first chunk, not behind them on a wave the other two wait for.  One static
//              rule: no claim counter, and no wave waits for another except at the barriers.  No list, hence no capacity, no
//              deferred edge and no whole-edge walk.  Every waypoint is examined, as on the pipeline: the lookup tally of a
//              colliding edge equals the pipeline's (integer adds: their order does not matter)
//   verdict    edge lanes: k_pipe_finish's verdict, outputs, ballot compaction, tally_block
// A state whose edges straddle two blocks has its distance and its own check computed by both (same inputs, same
// instructions, same bits); what is per state in the tallies is counted by the owner of its primitive 0.
// No block waits for another.  The one cross-block step is the claim of the compact stream: each compaction shard has one
// 64-bit word in the stream's counter set (all-zero between steps; kernels.h SMPLX_STEP_CTR_*) that holds the records
// claimed in region A, in region B and the blocks that have claimed, so ONE returning atomic per block claims both ranges
// and counts the block.  The block that claims last in the step's last shard copies the totals to the caller's -- which
// need not be zero beforehand -- and zeroes the set.  (One counter for all 800 blocks behind a fence each made the step
// 53 us; two claim atomics and a count, one after the other, were three round trips at the tail of every block.)
// The generic build keeps the successor's joint values in out_q (as its pipeline does) and evaluates the successor of a
// valid edge behind the verdict; the launch rule (step.h) takes this kernel for per-robot builds that keep four blocks a CU.
#pragma once

#include "step_kernels.h"

extern "C" __global__ void __launch_bounds__(SMPLX_STEP_BLOCK)
k_step_block(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int B,
             unsigned char* __restrict__ out_flags, int* out_coord, double* out_q,
             int* __restrict__ out_h, int* __restrict__ out_cost, int* __restrict__ out_lookups,
             unsigned long long* __restrict__ counters,
        const SmplxSpaceDev* const* __restrict__ stab, const unsigned short* __restrict__ state_q,
             int* __restrict__ out_id, SmplxCompactDev cmp, int* __restrict__ step_ctr, int nprims, int nvars,
             const unsigned char* __restrict__ blob, int blob_bytes)
{
    extern __shared__ __align__(16) unsigned char smem[];
    constexpr int NT = SMPLX_STEP_BLOCK;
#ifdef SMPLX_CONST_MODEL
    constexpr bool RS = true;   // saved link transforms in registers, as k_pipe_configs
#else
    constexpr bool RS = false;
#endif
    __shared__ double s_gd[SMPLX_STEP_STATES];                       // goal distance of the block's states
    __shared__ int s_slk[SMPLX_STEP_STATES], s_sbad[SMPLX_STEP_STATES];   // ... and the result of their own check
    __shared__ int s_W[BLOCK], s_pre[BLOCK], s_elk[BLOCK], s_ebad[BLOCK];    // per edge: waypoints, wave-wide inclusive item prefix, results
    __shared__ int s_wsum[BLOCK / 64];
#ifdef SMPLX_CONST_MODEL
    __shared__ double s_sq[CM_NV * BLOCK];                            // successor joint values, [v][edge]
    __shared__ double s_pq[SMPLX_STEP_STATES * CM_NV];                // joint values of the block's states
    __shared__ double s_trig[CM_PARENT_TRIG ? SMPLX_STEP_STATES * SMPLX_TRIG_ROW : 1];   // their rows (sphere_checks.h parent_trig)
#endif
    const int t = (int)threadIdx.x;
    const ModelFetch fetched = model_fetch(blob, blob_bytes, NT);
    const SmplxActionsDev& A = S->actions;
    const int nv = ARG_NVARS(nvars);
    const long long n_edges = (long long)B * nprims;
    const long long e0 = (long long)blockIdx.x * BLOCK;                                 // (e0 < n_edges: the grid is the edge blocks)
    const long long e1 = e0 + BLOCK - 1 < n_edges ? e0 + BLOCK - 1 : n_edges - 1;
    const int s0 = (int)(e0 / nprims), s1 = (int)(e1 / nprims);
    const int n_states = s1 - s0 + 1;                                                   // <= SMPLX_STEP_STATES: the launch rule sees to it
    const bool dist_wave = t >= BLOCK;
    const int l = t - BLOCK;                                                            // lane of the goal-distance wave
    const long long tid = e0 + t;
    const bool in_range = !dist_wave && tid < n_edges;
    const int si = in_range ? (int)(tid / nprims) : s0;
    const int pi = in_range ? (int)(tid - (long long)si * nprims) : 0;
    const int ks = si - s0;
    const SmplxSpaceDev* Sq = stab ? stab[state_q[si]] : S;
    const MprimGate gate = mprim_gate(A, A.type[pi]);   // constants of the launch: they travel with the model image and the parents
#if defined(SMPLX_CONST_MODEL) && !defined(ABL_NO_SUCC)
    SmplxTableDev table = {nullptr, 0u, 0, 0};
    if (out_id) table = Sq->table;
#endif
    if (t < BLOCK) { s_elk[t] = 0; s_ebad[t] = 0; }
    if (t < SMPLX_STEP_STATES) { s_slk[t] = 0; s_sbad[t] = 0; }
#ifdef SMPLX_CONST_MODEL
    double pqv[CM_NV], sqv[CM_NV];
#pragma unroll
    for (int v = 0; v < CM_NV; ++v) { pqv[v] = 0.0; sqv[v] = 0.0; }
    if (in_range) {
#pragma unroll
        for (int v = 0; v < CM_NV; ++v) pqv[v] = Q[(int64_t)si * CM_NV + v];
    }
    for (int i = t; i < n_states * CM_NV; i += NT) s_pq[i] = Q[(int64_t)s0 * CM_NV + i];
#endif
    ModelLds Mv;
    ThreadLds L = setup_lds(S, smem, &Mv, NT, !RS, blob, blob_bytes, fetched);
    const ModelLds* M = &Mv;
    const SmplxGridDev grid = S->grid;
    int W = 0;
    int flags = SMPLX_F_INACTIVE;
    int succ_h = 0, succ_id = -1;
    bool succ_goal = false;
#ifdef SMPLX_CONST_MODEL
    // per-robot build: joint values, limits and waypoint count are worked out in registers BEFORE the gate is known, beside
    // the goal-distance wave; an edge whose primitive turns out inactive keeps none of it
    int scv[CM_NV];
#pragma unroll
    for (int v = 0; v < CM_NV; ++v) scv[v] = 0;
    if (in_range) flags = pipe_edge_values(M, A, Sq, pi, pqv, sqv, W);
#ifndef ABL_NO_SUCC
    // ... and so are the coordinates of an edge within limits (pipe_successor's first piece): they need nothing of the
    // parent's sines and cosines.  (The home slot's loads issued here as well, beside the distance chain, measured no better
    // than behind the gate: 27.1 against 27.5 us a step, below three times the run-to-run spread.)
    if (in_range && flags == 0) {
        successor_coords(M, sqv, scv);
    }
#endif
    if (dist_wave) {
        if constexpr (CM_PARENT_TRIG) {
            // The goal-distance wave of k_pipe_setup as it stands: one (state, variable) pair a lane, 64 / NV states a round;
            // the rows go to LDS (first read behind the gate's barrier), the normalised pairs travel by shuffles to the lanes
            // that run the chain, so the wave needs no barrier of its own.
            constexpr int PER = 64 / CM_NV;
            const int ls = l / CM_NV, lv = l - ls * CM_NV;
            for (int r0 = 0; r0 < n_states; r0 += PER) {   // (uniform over the wave)
                const int k = r0 + ls;
                double ns = 0.0, nc = 0.0;
                if (ls < PER && k < n_states) {
                    const double x = s_pq[k * CM_NV + lv];
                    double rs = 0.0, rc = 0.0;   // a variable no SMPLX_TK_REV_*_T joint turns on: nobody reads its pairs
                    if ((CM_TRIG_ANY >> lv) & 1u) smplx_sincos(x, &rs, &rc);
                    ns = rs; nc = rc;
                    bool cont = false;
#pragma unroll
                    for (int u = 0; u < CM_NV; ++u) if (CM_VAR_TYPE[u] == SMPLX_JT_CONTINUOUS) cont = cont || lv == u;
                    if (cont && ((CM_TRIG_ANY >> lv) & 1u)) {
                        const double xn = smplx_normalize_angle(x);
                        if (__double_as_longlong(xn) != __double_as_longlong(x)) smplx_sincos(xn, &ns, &nc);
                    }
                    double* row = s_trig + k * SMPLX_TRIG_ROW;
                    row[2 * lv] = rs; row[2 * lv + 1] = rc;
                    row[2 * CM_NV + 2 * lv] = ns; row[2 * CM_NV + 2 * lv + 1] = nc;
                }
                double sn[CM_NV], cs[CM_NV];
#pragma unroll
                for (int v = 0; v < CM_NV; ++v) {   // lane j < PER gathers the pairs of state r0 + j (every lane takes part)
                    const int from = (l * CM_NV + v) & 63;
                    sn[v] = __shfl(ns, from); cs[v] = __shfl(nc, from);
                }
                if (l < PER && r0 + l < n_states) {
                    const int k2 = r0 + l;
                    const SmplxBfsDev bfs = (stab ? stab[state_q[s0 + k2]] : S)->bfs;
                    double qd[CM_NV];
#pragma unroll
                    for (int v = 0; v < CM_NV; ++v) qd[v] = s_pq[k2 * CM_NV + v];
                    s_gd[k2] = metric_goal_distance_sc(M, grid, bfs, qd, sn, cs);
                }
            }
        } else if (l < n_states) {
            // a robot without the table: one lane per state, the whole chain with its sincos
            const SmplxBfsDev bfs = (stab ? stab[state_q[s0 + l]] : S)->bfs;
            double qd[CM_NV];
#pragma unroll
            for (int v = 0; v < CM_NV; ++v) qd[v] = s_pq[l * CM_NV + v];
            s_gd[l] = metric_goal_distance(M, grid, bfs, qd);
        }
    }
#else
    // generic build: one lane per state, the whole chain with its sincos
    if (dist_wave && l < n_states) {
        const SmplxBfsDev bfs = (stab ? stab[state_q[s0 + l]] : S)->bfs;
        s_gd[l] = metric_goal_distance(M, grid, bfs, Q + (int64_t)(s0 + l) * nv);
    }
#endif
    __syncthreads();
    // the gate; successor joint values and waypoint counts where the collision phase finds them
    int items = 0;
    if (in_range) {
        if (!mprim_active(gate, s_gd[ks])) {
            flags = SMPLX_F_INACTIVE;
            W = 0;
        } else {
#ifdef SMPLX_CONST_MODEL
            if (flags != SMPLX_F_INACTIVE) {
#pragma unroll
                for (int v = 0; v < CM_NV; ++v) { s_sq[v * BLOCK + t] = sqv[v]; out_q[tid * CM_NV + v] = sqv[v]; }
            }
#else
            flags = pipe_edge_values(M, A, Sq, pi, Q + (int64_t)si * nv, out_q + tid * nv, W);
#endif
        }
        items = W > 0 ? W - 1 : 0;
    }
    const int lane = t & 63, wv = t >> 6;
    int incl = items;
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(incl, off);
        if (lane >= off) incl += u;
    }
    if (!dist_wave) {
        s_W[t] = W;
        s_pre[t] = incl;
        if (lane == 63) s_wsum[wv] = incl;
    }
    __syncthreads();
#if defined(SMPLX_CONST_MODEL) && !defined(ABL_NO_SUCC)
    // the rest of the successor role of k_pipe_configs, for an edge that is active and within limits: the home slot's
    // loads, which travel during the chain, planning-link FK, goal test, heuristic, table id.  It stands behind the item
    // prefix, not in front of it: no item reads what it leaves (the verdict does), and the goal-distance wave, which has no
    // edge, is a successor evaluation ahead of the edge waves in the item loop.
    // (With the chain in front of the gate too, beside the distance chain, every wave pays the seven sincos rounds of
    // its snap edges, active or not: 31.3 against 30.0 us a step.  Cutting the heuristic into a load here and its cost
    // in the verdict hid nothing: the compiler waits for the load where the edge lanes' branch rejoins.)
    if (in_range && flags == 0) {
        constexpr bool SC = CM_PARENT_TRIG && CM_TRIG_PLANNING != 0;
        const SmplxBfsDev sbfs = Sq->bfs;
        const TableSlotWords home = table_probe_issue(table, scv, CM_NV);
        if constexpr (SC) {
            double prow[2 * CM_NV], sn[CM_NV], cs[CM_NV];
#pragma unroll
            for (int j = 0; j < 2 * CM_NV; ++j) prow[j] = s_trig[ks * SMPLX_TRIG_ROW + 2 * CM_NV + j];
            parent_trig<CM_TRIG_PLANNING, true>(sqv, pqv, prow, sn, cs);
            succ_h = successor_goal_h<true>(M, Sq->goal, sbfs, grid, sqv, scv, succ_goal, sn, cs);
        } else {
            succ_h = successor_goal_h(M, Sq->goal, sbfs, grid, sqv, scv, succ_goal);
        }
        // the home slot arrived during the chain: the id costs one wait, and more only where the probe walks on
        succ_id = table_probe_resolve(table, scv, CM_NV, home);
    }
#endif
    // collision: items [0, n_states) are the block's states (waypoint 0 of every edge), the rest (edge, waypoint).  Chunk c
    // holds items [64 c, 64 c + 64) and goes to wave NW - 1 - (c mod NW): lane l of wave w takes items 64 (NW - 1 - w) + l,
    // + NT, ...  The goal-distance wave is wave NW - 1: it owns chunk 0 (the states, whose rows it wrote itself) and the
    // chunk behind every NW, so a block of NT + 1 .. NT + 64 items has its ragged last chunk on the wave that started first.
    {
        int wave_first[BLOCK / 64 + 1];
        wave_first[0] = 0;
#pragma unroll
        for (int k = 0; k < BLOCK / 64; ++k) wave_first[k + 1] = wave_first[k] + s_wsum[k];
#ifdef ABL_ONE_TURN
        const int total = min(n_states + wave_first[BLOCK / 64], NT);   // diagnostic: prices the turns behind the first
#else
        const int total = n_states + wave_first[BLOCK / 64];
#endif
        for (int i = 64 * (NT / 64 - 1 - wv) + lane; i < total; i += NT) {
            const bool is_state = i < n_states;
            int k = i, edge = 0, wp = 0, Wi = 0;
            if (!is_state) {
                int j = i - n_states;
                int w = 0;
#pragma unroll
                for (int u = 1; u < BLOCK / 64; ++u) w += (j >= wave_first[u]) ? 1 : 0;
                j -= wave_first[w];
                int lo = 0;   // the first edge of wave w whose inclusive prefix exceeds j
#pragma unroll
                for (int step = 32; step > 0; step >>= 1)
                    if (s_pre[w * 64 + lo + step - 1] <= j) lo += step;
                edge = w * 64 + lo;
                Wi = s_W[edge];
                wp = j - (s_pre[edge] - (Wi - 1)) + 1;
                k = (int)((e0 + edge) / nprims) - s0;
            }
            EdgeRef e;
            e.alpha = is_state ? 0.0 : (double)wp * (1.0 / (double)(Wi - 1));
            int lk = 0;
            bool ok;
#ifdef SMPLX_CONST_MODEL
            e.start = nullptr; e.finish = nullptr;   // config_valid_staged never dereferences them
            constexpr bool SC = CM_PARENT_TRIG;
            double qs[CM_NV], qc[CM_NV], prow[2 * CM_NV];
#pragma unroll
            for (int v = 0; v < CM_NV; ++v) { qs[v] = s_pq[k * CM_NV + v]; qc[v] = qs[v]; }
            if constexpr (SC) {
#pragma unroll
                for (int j = 0; j < 2 * CM_NV; ++j) prow[j] = s_trig[k * SMPLX_TRIG_ROW + j];
            }
#ifndef ABL_NO_FK
#pragma unroll
            for (int v = 0; v < CM_NV; ++v) {   // stage_config
                const double sv = qs[v];
                double q = sv;
                if (e.alpha != 0.0) q = sv + e.alpha * edge_diff(M, v, sv, s_sq[v * BLOCK + edge]);
                lds_d(L, L.q_base + v) = q;
                qc[v] = q;
            }
#endif
            if constexpr (SC) {
                double sn[CM_NV], cs[CM_NV];
                parent_trig<CM_TRIG_COLLISION, false>(qc, qs, prow, sn, cs);
                ok = config_valid_staged<RS, true>(M, L, grid, e, lk, sn, cs);
            } else {
                ok = config_valid_staged<RS>(M, L, grid, e, lk);
            }
#else
            e.start = Q + (int64_t)(s0 + k) * nv;
            e.finish = is_state ? e.start : out_q + (e0 + edge) * nv;
            ok = config_valid<RS>(M, L, grid, e, lk);
#endif
            if (is_state) {
                s_slk[k] = lk;
                if (!ok) s_sbad[k] = 1;
            } else {
                atomicAdd(&s_elk[edge], lk);
                if (!ok) s_ebad[edge] = 1;
            }
        }
    }
    __syncthreads();
    // verdict and outputs, as k_pipe_finish
    int lookups = 0, performed = 0, evaluated = 0, ncfg = 0, slk = 0;
    if (in_range) {
        const int s_lk = s_slk[ks];
        if (pi == 0) { slk = s_lk; ncfg = 1; }
        int h = 0, cost = 0;
        if (!(flags & SMPLX_F_INACTIVE)) evaluated = 1;
        if (flags == 0) {
            if (W > 0) ncfg += W - 1;
            performed = s_elk[t];
            const bool ok = (W == 0) || (s_sbad[ks] == 0 && s_ebad[t] == 0);
            lookups = performed + (W > 0 ? s_lk : 0);
            if (!ok) {
                flags = SMPLX_F_COLLISION;
                succ_id = -1;
            } else {
#ifdef SMPLX_CONST_MODEL
#pragma unroll
                for (int v = 0; v < CM_NV; ++v) out_coord[tid * CM_NV + v] = scv[v];
#else
                pipe_successor(M, Sq, grid, out_q + tid * nv, out_coord + tid * nv, out_id != nullptr, succ_h, succ_id, succ_goal);
#endif
                h = succ_h;
                cost = A.cost[pi];
                flags = SMPLX_F_VALID | (succ_goal ? SMPLX_F_GOAL : 0);
            }
        } else {
            succ_id = -1;
        }
        out_flags[tid] = (unsigned char)flags;
        out_h[tid] = h;
        out_cost[tid] = cost;
        out_lookups[tid] = lookups;
        succ_h = h;
        if (out_id) out_id[tid] = succ_id;
    }
    // K5: validity compaction, as k_pipe_finish, but the claim is on the stream's counter set (step_ctr), not on the caller's
    // totals, and it is one atomic: the shard's word holds records of region A in bits 0-23, of region B in bits 24-47 and
    // the blocks that have claimed in bits 48-63 (the launch rule keeps a shard's fields from running over: kernels.h
    // smplx_step_claim_fits).  Every block claims, also one without a record: the claim is what counts it.
    // Order: the last adder of a word sees every earlier add in that word's modification order; it adds to the count of
    // shards only after its own claim has returned, and the block whose add completes that count reads the words only
    // after that add has returned.  Device-scope atomics on this memory execute at one point of coherence, and only atomics
    // touch these words, so it reads every claim of the step; no block touches the set behind its own claim, so the set it
    // zeroes stays zero.  A sub-region has overflowed exactly when its final total exceeds its capacity (a block's claim
    // ends at the running total), so the flag is worked out from the totals and needs no word of its own.  If the order
    // broke, totals would be wrong and the set would stay non-zero: the tests read the set after back-to-back steps
    // (smplx_test_step_counters_zero).
    __shared__ int s_last;
    if (cmp.rec_a) {
        __shared__ int c_cnt[BLOCK / 64][2];
        __shared__ int c_base[2];
        const bool is_a = in_range && (flags & SMPLX_F_VALID) != 0;
        const bool is_b = is_a && (succ_id < 0 || (flags & SMPLX_F_GOAL) != 0);
        const unsigned long long m_a = __ballot(is_a), m_b = __ballot(is_b);
        const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
        if (lane == 0 && !dist_wave) { c_cnt[wv][0] = __popcll(m_a); c_cnt[wv][1] = __popcll(m_b); }
        __syncthreads();
        if (t == 0) {
            int ta = 0, tb = 0;
#pragma unroll
            for (int k = 0; k < BLOCK / 64; ++k) { ta += c_cnt[k][0]; tb += c_cnt[k][1]; }
            const int nb = (int)gridDim.x, shard = blockIdx.x % SMPLX_CMP_SHARDS;
            const int in_shard = (nb - shard + SMPLX_CMP_SHARDS - 1) / SMPLX_CMP_SHARDS;
            const int shards = nb < SMPLX_CMP_SHARDS ? nb : SMPLX_CMP_SHARDS;
            const int sa = cmp.cap_a / SMPLX_CMP_SHARDS, sb = cmp.cap_b / SMPLX_CMP_SHARDS;
            unsigned long long* word = reinterpret_cast<unsigned long long*>(step_ctr + SMPLX_STEP_CTR_BASE + 32 * shard);
            const unsigned long long mine = (unsigned long long)ta | ((unsigned long long)tb << 24) | (1ull << 48);
            const unsigned long long was = atomicAdd(word, mine);
            const int ba0 = ta > 0 ? (int)(was & 0xFFFFFFull) : 0, bb0 = tb > 0 ? (int)((was >> 24) & 0xFFFFFFull) : 0;
            int ba = ba0, bb = bb0;   // (a block without records of a region starts it at the sub-region's base, as ever)
            int last = 0;
            if ((int)(was >> 48) == in_shard - 1)
                last = atomicAdd(&step_ctr[SMPLX_STEP_CTR_DONE], 1) == shards - 1 ? 1 : 0;
            s_last = last;
            if (ba + ta > sa || bb + tb > sb) ba = -1;   // overflow: dense outputs stay valid
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
#ifdef SMPLX_CONST_MODEL
#pragma unroll
                for (int v = 0; v < CM_NV; ++v) { ri[1 + v] = scv[v]; rq[v] = s_sq[v * BLOCK + t]; }
#else
                for (int v = 0; v < nv; ++v) { ri[1 + v] = out_coord[tid * nv + v]; rq[v] = out_q[tid * nv + v]; }
#endif
            }
        }
    }
    if (counters) {
        const unsigned long long m_eval = __ballot(evaluated);
        const unsigned long long m_valid = __ballot((flags & SMPLX_F_VALID) != 0);
        tally_block<NT / 64>(counters, dist_wave ? 0 : __popcll(m_eval), dist_wave ? 0 : __popcll(m_valid), lookups, performed, ncfg, slk);
    }
    // The step's last claimer hands the totals to the caller (existing layout; whatever they held is overwritten) and leaves
    // the stream's set all-zero for the next step; every other block is done.  Every block of this grid owns a block_tab row
    // and has written it, so there is no unused row to zero.
    if (cmp.rec_a && s_last) {
        if (t < SMPLX_CMP_SHARDS) {
            unsigned long long* word = reinterpret_cast<unsigned long long*>(step_ctr + SMPLX_STEP_CTR_BASE + 32 * t);
            const unsigned long long tot = atomicExch(word, 0ull);
            const int na = (int)(tot & 0xFFFFFFull), nb = (int)((tot >> 24) & 0xFFFFFFull);
            cmp.totals[32 * t] = na;
            cmp.totals[32 * t + 1] = nb;
            const unsigned long long over = __ballot(na > cmp.cap_a / SMPLX_CMP_SHARDS || nb > cmp.cap_b / SMPLX_CMP_SHARDS);
            if (t == 0) {
                cmp.totals[32 * SMPLX_CMP_SHARDS] = over != 0ull ? 1 : 0;
                atomicExch(&step_ctr[SMPLX_STEP_CTR_DONE], 0);
            }
        }
    }
}
