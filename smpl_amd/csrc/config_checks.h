// smpl_amd/csrc/config_checks.h -- the validity of one configuration and of one edge.
// Owns: config_valid_staged and config_valid (CollisionSpace::isStateValid), edge_waypoint_count, edge_valid
// (CollisionSpace::isStateToStateValid), in the generic form and, under SMPLX_CONST_MODEL, over the per-robot chain.
// Restates: collision_space.cpp:532-581; self_collision_model.cpp:407-428; robot_motion_collision_model.cpp:371-407 and
// .h:173-181, 352-366.
#pragma once

#include "sphere_checks.h"
#include "attached_bodies.h"

// CollisionSpace::isStateValid for one configuration (collision_space.cpp:532-536 ->
// self_collision_model.cpp:407-428): group trees vs grid in chain order, then the checked
// link pairs sphere-vs-sphere.
// the configuration's joint values are already staged in the thread's LDS slots (stage_config or the caller itself)
// SC (per-robot build): sn[v], cs[v] = smplx_sincos of the staged value of every variable of CM_TRIG_COLLISION, which the
// caller has from the parent's row (sphere_checks.h parent_trig); every other caller leaves the chain to evaluate them
template <bool RS = false, bool SC = false>
__device__ __forceinline__ bool config_valid_staged(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                                    const EdgeRef& e, int& lookups, const double* sn = nullptr,
                                                    const double* cs = nullptr)
{
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.0;
    bool pair_hit = false, recheck_all = false;
    PendingPairs P;   // queued (earlier tree, later tree) pairs
    P.w0 = 0; P.w1 = 0; P.w2 = 0; P.n = 0;
#ifdef ABL_NO_FK
    lookups += (int)e.alpha; return true;
#endif
#ifdef SMPLX_CONST_MODEL
    {
        ChainState C;
#pragma unroll
        for (int i = 0; i < 12; ++i) C.T[i] = 0.0;
#pragma unroll
        for (int v = 0; v < CM_NV; ++v) C.q[v] = lds_d(L, L.q_base + v);
        if constexpr (SC) {
#pragma unroll
            for (int v = 0; v < CM_NV; ++v) { C.sn[v] = sn[v]; C.cs[v] = cs[v]; }
        }
        C.pair_hit = false; C.recheck_all = false; C.P = P;
        C.pd2 = 0;
        if (!const_chain<0, -1, RS, SC>(M, L, g, C, lookups)) return false;
        pair_hit = C.pair_hit; recheck_all = C.recheck_all;
        const PendingPairs filled = C.P;
        P = filled;
    }
    const int nj = 0;
#else
    const int nj = M->njoints;
#endif
    JointHead cur = load_joint_head(M, L, 0);
    for (int j = 0; j < nj; ++j) {
        // the next joint's record is requested from LDS now and consumed an iteration later, so its latency hides
        // behind this joint's sincos and products
        JointHead nxt = cur;
        if (j + 1 < nj) nxt = load_joint_head(M, L, j + 1);
        if (cur.src >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = lds_d(L, L.slot_base + 12 * cur.src + i);
        }
        if (cur.kind >= SMPLX_TK_FIXED_T) apply_joint_t(cur.kind, cur.tx, cur.ty, cur.tz, cur.q, T, cur.src == SMPLX_SRC_ROOT);
        else apply_joint(&M->joints[j], cur.q, T, cur.src == SMPLX_SRC_ROOT);
        if (cur.save_slot >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) lds_d(L, L.slot_base + 12 * cur.save_slot + i) = T[i];
        }
        const int jtree = cur.tree;
        cur = nxt;
        if (jtree >= 0) {
            const int t = jtree;
            double rp[3];
#ifdef ABL_NO_TREES
            rp[0] = T[3]; rp[1] = T[7]; rp[2] = T[11];
#else
            if (!check_tree(M, L, g, t, T, lookups, rp)) return false;   // voxel collision: the reference stops here too
#endif
            const int slot = M->tree_root_slot[t];
            if (slot >= 0) {
                lds_d(L, L.root_base + 3 * slot + 0) = rp[0];
                lds_d(L, L.root_base + 3 * slot + 1) = rp[1];
                lds_d(L, L.root_base + 3 * slot + 2) = rp[2];
            }
            // checked link pairs whose later tree is t: root-vs-root now (self_collision_model.cpp:1111-1123);
            // anything the roots do not settle is queued and resolved after the chain (the slow path reuses the
            // transform slots).  A hit does not stop the voxel pass: the reference runs ALL voxel checks before
            // the first pair (self_collision_model.cpp:418-421), so lookup tallies stay identical.
            const LDS_AS SmplxNode& B = L.nodes[M->tree_first[t + 1] - 1];
#ifdef ABL_NO_PAIRS
            for (int k = 0; k < 0; ++k) {
#else
            for (int k = M->pair_first[t]; k < M->pair_first[t + 1]; ++k) {
#endif
                const int ta = M->pair_other[k];
                const int sa = M->tree_root_slot[ta];
                const LDS_AS SmplxNode& A = L.nodes[M->tree_first[ta + 1] - 1];
                // pairs are stored (group-earlier, group-later); the subtraction order follows that
                const bool a_first = ta < t;
                const double ax = lds_d(L, L.root_base + 3 * sa + 0), ay = lds_d(L, L.root_base + 3 * sa + 1),
                             az = lds_d(L, L.root_base + 3 * sa + 2);
                const double dx = a_first ? rp[0] - ax : ax - rp[0];
                const double dy = a_first ? rp[1] - ay : ay - rp[1];
                const double dz = a_first ? rp[2] - az : az - rp[2];
                const double cd2 = (dx * dx + dy * dy) + dz * dz;
                const double rr = a_first ? A.r + B.r : B.r + A.r;
                if (cd2 > rr * rr) continue;
                if (A.left < 0 && B.left < 0) { pair_hit = true; continue; }
                // queue (ta, t): 8 bits each, up to 4 pairs in the 64-bit word; more -> recheck everything
                if (!pend_push(P, ta, t)) recheck_all = true;
            }
        }
    }
    // unresolved pairs (normally none): one call site for the slow path, so it can be inlined without
    // putting the model view into scratch memory
    const int total = recheck_all ? M->pair_first[M->ntrees] : P.n;
    int tcur = 0;
    for (int i = 0; i < total && !pair_hit; ++i) {
        int ta, t;
        if (recheck_all) {
            while (i >= M->pair_first[tcur + 1]) ++tcur;
            t = tcur;
            ta = M->pair_other[i];
        } else {
            const int code = pend_get(P, i);
            ta = code >> 8;
            t = code & 0xFF;
        }
        const int a = ta < t ? ta : t, b = ta < t ? t : ta;
        if (!check_pair_full<RS>(M, L, e, a, b)) pair_hit = true;
    }
    if (pair_hit) return false;
    if (M->bodies) return bodies_valid(M, L, g, lookups);    // uniform: the query has attached bodies
    return true;
}

template <bool RS = false>
__device__ __forceinline__ bool config_valid(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                             const EdgeRef& e, int& lookups)
{
#ifndef ABL_NO_FK
    stage_config(M, L, e);
#endif
    return config_valid_staged<RS>(M, L, g, e, lookups);
}

// waypoint count of the edge start -> finish (robot_motion_collision_model.cpp:371-407, .h:352-366, 173-181): 0 for an
// edge without motion.  The one definition for every path: edge_valid, the pipeline's setup, the block-per-state pieces.
__device__ __forceinline__ int edge_waypoint_count(const ModelLds* __restrict__ M, const double* __restrict__ start,
                                                   const double* __restrict__ finish)
{
    double motion = 0.0;
    const int nv = MV_NVARS(M);
    MV_UNROLL
    for (int v = 0; v < nv; ++v) {
        const int ty = MV_TYPE(M, v);
        const double sv = start[v], fv = finish[v];
        if (ty == SMPLX_JT_CONTINUOUS) motion += MV_K(M, v) * fabs(smplx_shortest_angle_diff(fv, sv));
        else if (ty == SMPLX_JT_REVOLUTE) motion += MV_K(M, v) * fabs(fv - sv);
        else if (ty == SMPLX_JT_PRISMATIC) motion += fabs(fv - sv);
    }
    int W = 0;
    if (motion != 0.0) {
        W = (int)ceil(motion / 0.05) + 1;
        if (W < 2) W = 2;
    }
    return W;
}

// CollisionSpace::isStateToStateValid (collision_space.cpp:538-581).  first_wp = 1 skips waypoint 0
// (the start configuration), whose result the caller already has.
template <bool RS = false>
__device__ __forceinline__ bool edge_valid(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                           const double* __restrict__ start, const double* __restrict__ finish,
                                           bool start_known, bool start_valid, int& lookups, int& waypoints)
{
    const int W = edge_waypoint_count(M, start, finish);
    waypoints = W;
    if (W == 0) return true;
    if (start_known && !start_valid) return false;
    const double inv = 1.0 / (double)(W - 1);
    EdgeRef e;
    e.start = start;
    e.finish = finish;
    if (W > 5) {
        for (int i = 0; i < 5; ++i) {
            for (int j = i; j < W; j += 5) {
                if (j == 0 && start_known) continue;
                e.alpha = (double)j * inv;
                if (!config_valid<RS>(M, L, g, e, lookups)) return false;
            }
        }
    } else {
        for (int j = start_known ? 1 : 0; j < W; ++j) {
            e.alpha = (double)j * inv;
            if (!config_valid<RS>(M, L, g, e, lookups)) return false;
        }
    }
    return true;
}
