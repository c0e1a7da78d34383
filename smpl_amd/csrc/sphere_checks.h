// smpl_amd/csrc/sphere_checks.h -- the pieces of a configuration's collision check.
// Owns: the voxel lookup (grid_d2), sphere tree against the grid (check_tree), the configuration on an edge staged into
// per-thread LDS (EdgeRef, stage_config), fk_two_links, the pending pairs, the whole per-robot chain (SMPLX_CONST_MODEL:
// ChainState, const_pairs, apply_joint_const, issue_root / resolve_root, const_chain, const_planning_chain,
// const_two_links) and sphere tree against sphere tree (check_pair_full).  config_checks.h puts them together.
// Restates: occupancy_grid.h:234 with distance_map.hpp:281-300, 520-536; collision_operations.h:105-164;
// robot_motion_collision_model.h:221-247, 297-320; self_collision_model.cpp:1093-1218.
#pragma once

#include "model_lds.h"

// voxel lookup: squared cell distance at a world point, 0 outside the grid
// (occupancy_grid.h:234 -> distance_map.hpp:281-300, 520-536)
__device__ __forceinline__ int grid_d2(const SmplxGridDev& g, const double p[3])
{
    const int x = (int)(g.inv_res * (p[0] - g.origin_minus_res[0]) + 0.5) - 1;
    const int y = (int)(g.inv_res * (p[1] - g.origin_minus_res[1]) + 0.5) - 1;
    const int z = (int)(g.inv_res * (p[2] - g.origin_minus_res[2]) + 0.5) - 1;
    // no branch around the load: a load inside a branch is waited for where the branches rejoin, which put the whole
    // round trip in front of whatever the caller meant to overlap with it.  Out of the grid: cell 0 is read and dropped.
    const bool outside = x < 0 || y < 0 || z < 0 || x >= g.n[0] || y >= g.n[1] || z >= g.n[2];
    const size_t brick = ((size_t)(x >> 2) * g.bricks[1] + (y >> 2)) * g.bricks[2] + (z >> 2);
    const size_t cell = brick * 64 + ((x & 3) << 4) + ((y & 3) << 2) + (z & 3);
    // the pointer comes out of a struct read from memory, so the compiler takes it for a FLAT address: a flat load counts
    // on the LDS counter as well, and every wait for an LDS read behind it (saved transforms, tree nodes) waited for the
    // grid gather too.  It is device memory: say so.
    const SMPLX_GLOBAL_AS unsigned short* d2 = (const SMPLX_GLOBAL_AS unsigned short*)g.d2;
    const int v = (int)d2[outside ? (size_t)0 : cell];
    return outside ? 0 : v;
}

// interpolated value of planning variable v on the edge start -> finish at parameter alpha
// (robot_motion_collision_model.h:221-247 diffs, 297-320 interpolate)
__device__ __forceinline__ double edge_diff(const ModelLds* __restrict__ M, int v, double sv, double fv)
{
    return (MV_TYPE(M, v) == SMPLX_JT_CONTINUOUS) ? smplx_shortest_angle_diff(fv, sv) : fv - sv;
}

// sphere tree vs voxel grid for the tree on the current link (collision_operations.h:105-164).
// Returns false at the first colliding leaf.  The root position comes back for the sphere-sphere tests.
__device__ __forceinline__ bool check_tree(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                           int t, const double T[12], int& lookups, double root_p[3])
{
    const int root = M->tree_first[t + 1] - 1;
    int sp = 0;
    int node = root;
    while (true) {
        const LDS_AS SmplxNode& nd = L.nodes[node];
        double c[3] = {nd.c[0], nd.c[1], nd.c[2]};
        double p[3];
        xform(T, c, p);
        if (node == root) { root_p[0] = p[0]; root_p[1] = p[1]; root_p[2] = p[2]; }
        ++lookups;
#ifdef ABL_NO_LOOKUP
        const int d2 = 60000 + (int)(p[0] * 0.0);
#else
        const int d2 = grid_d2(g, p);
#endif
        if (d2 < nd.thr) {              // CheckSphereCollision fails (collision_operations.h:67-77)
            if (nd.left < 0) return false;
            const double rl = L.nodes[nd.left].r, rr = L.nodes[nd.right].r;
            // larger child is examined first (:150-156): push the other one
            if (rl > rr) { lds_b(L, sp++) = (unsigned char)nd.right; node = nd.left; }
            else { lds_b(L, sp++) = (unsigned char)nd.left; node = nd.right; }
            continue;
        }
        if (sp == 0) break;
        node = lds_b(L, --sp);
    }
    return true;
}

// value source for the configuration being checked
struct EdgeRef {
    const double* __restrict__ start;    // N doubles
    const double* __restrict__ finish;   // N doubles
    double alpha;
};

// joint values of the configuration on the edge at parameter alpha
// (robot_motion_collision_model.h:221-247 diffs, 297-320 interpolate), staged into per-thread LDS once per
// configuration (the slow path of the sphere-sphere pass re-reads them)
__device__ __forceinline__ void stage_config(const ModelLds* __restrict__ M, const ThreadLds& L, const EdgeRef& e)
{
    const int nv = MV_NVARS(M);
    MV_UNROLL
    for (int v = 0; v < nv; ++v) {
        const double sv = e.start[v];
        double q = sv;
        if (e.alpha != 0.0) q = sv + e.alpha * edge_diff(M, v, sv, e.finish[v]);   // start + 0*diff == start exactly
        lds_d(L, L.q_base + v) = q;
    }
}

__device__ __forceinline__ double config_var(const ModelLds* __restrict__ M, const ThreadLds& L, int v)
{
    (void)M;
    return lds_d(L, L.q_base + v);
}

// link transforms of two trees' links for one configuration (slow path of the sphere-sphere pass)
__device__ __forceinline__ void fk_two_links(const ModelLds* __restrict__ M, const ThreadLds& L, const EdgeRef& e,
                                          int ja, int jb, double Ta[12], double Tb[12])
{
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.0;
    const int last = ja > jb ? ja : jb;
    for (int j = 0; j <= last; ++j) {
        JointPtr jt = &M->joints[j];
        const double q = jt->var >= 0 ? config_var(M, L, jt->var) : 0.0;
        if (jt->src >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = lds_d(L, L.slot_base + 12 * jt->src + i);
        }
        apply_joint(jt, q, T, jt->src == SMPLX_SRC_ROOT);
        if (jt->save_slot >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) lds_d(L, L.slot_base + 12 * jt->save_slot + i) = T[i];
        }
        if (j == ja) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Ta[i] = T[i];
        }
        if (j == jb) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Tb[i] = T[i];
        }
    }
}

// Checked link pairs whose root spheres overlap and are not both leaves wait here for the sphere-tree pass behind the
// chain: (earlier tree << 8 | later tree), 16 bits each, twelve of them in three words.  More than that -> every pair
// is rechecked.  (Four slots overflowed in most waves of random configurations, and a recheck of every pair pays a
// two-link FK per pair.)
#define SMPLX_PENDING_MAX 12
struct PendingPairs {
    unsigned long long w0, w1, w2;
    int n;
};
__device__ __forceinline__ bool pend_push(PendingPairs& P, int ta, int t)
{
    if (P.n >= SMPLX_PENDING_MAX) return false;
    const unsigned long long c = (unsigned long long)((ta << 8) | t) << (16 * (P.n & 3));
    const int k = P.n >> 2;
    if (k == 0) P.w0 |= c;
    else if (k == 1) P.w1 |= c;
    else P.w2 |= c;
    ++P.n;
    return true;
}
__device__ __forceinline__ int pend_get(const PendingPairs& P, int i)
{
    const int k = i >> 2;
    const unsigned long long w = k == 0 ? P.w0 : (k == 1 ? P.w1 : P.w2);
    return (int)((w >> (16 * (i & 3))) & 0xFFFF);
}

// the part of a joint record the chain step needs, in registers
struct JointHead {
    int kind, var, src, save_slot, tree;
    double tx, ty, tz, q;
};

__device__ __forceinline__ JointHead load_joint_head(const ModelLds* __restrict__ M, const ThreadLds& L, int j)
{
    JointPtr jt = &M->joints[j];
    JointHead h;
    h.kind = jt->kind; h.var = jt->var; h.src = jt->src; h.save_slot = jt->save_slot; h.tree = jt->tree;
    h.tx = jt->origin[3]; h.ty = jt->origin[7]; h.tz = jt->origin[11];
    h.q = h.var >= 0 ? lds_d(L, L.q_base + h.var) : 0.0;
    return h;
}

#ifdef SMPLX_CONST_MODEL
// ---------------------------------------------------------------------------------------------
// Per-robot specialisation: the chain structure (joint kinds, origins, which link carries which tree, the
// checked pairs) comes from compile-time constants (model_compile.cpp model_const_header), so the joint loop
// is straight-line code: no joint records read from LDS, no kind dispatch, root positions and joint values in
// registers.  Same operations in the same order as the generic path below: identical bits.
// ---------------------------------------------------------------------------------------------

struct ChainState {
    double T[12];
    double q[CM_NV];
    double sn[CM_NV], cs[CM_NV];   // const_chain<.., SC = true>: sine and cosine of q[v], handed in by the caller (parent_trig below)
    double roots[3 * (CM_NT > 0 ? CM_NT : 1)];   // only the slots that lead a pair are ever touched
    bool pair_hit, recheck_all;
    PendingPairs P;
    // the tree whose root lookup is in flight (software pipelining, see const_chain): its link transform and the
    // squared cell distance the lookup returns
    double Tp[12];
    int pd2;
    // RS (const_chain<.., true>): the saved link transforms here instead of in the thread's LDS slots -- 96 bytes of LDS per
    // thread and slot were what held the validity kernels at three waves per SIMD
    double S[SMPLX_MAX_SLOTS][12];
};

template <int T_, int K, int KEND>
__device__ __forceinline__ void const_pairs(const ThreadLds& L, ChainState& C, const double rp[3])
{
    if constexpr (K < KEND) {
        constexpr int ta = CM_PAIR_OTHER[K];
        constexpr int sa = CM_ROOT_SLOT[ta];
        constexpr bool a_first = ta < T_;
        const double ax = C.roots[3 * sa + 0], ay = C.roots[3 * sa + 1], az = C.roots[3 * sa + 2];
        const double dx = a_first ? rp[0] - ax : ax - rp[0];
        const double dy = a_first ? rp[1] - ay : ay - rp[1];
        const double dz = a_first ? rp[2] - az : az - rp[2];
        const double cd2 = (dx * dx + dy * dy) + dz * dz;
        constexpr double rr = a_first ? CM_ROOT_R[ta] + CM_ROOT_R[T_] : CM_ROOT_R[T_] + CM_ROOT_R[ta];
        if (!(cd2 > rr * rr)) {
            if constexpr (CM_ROOT_LEAF[ta] && CM_ROOT_LEAF[T_]) {
                C.pair_hit = true;
            } else {
                if (!pend_push(C.P, ta, T_)) C.recheck_all = true;
            }
        }
        const_pairs<T_, K + 1, KEND>(L, C, rp);
    }
}

// apply_joint_t with the origin's translation as literals: terms with an exactly-zero coefficient are dropped
// (x*0 is +-0 and adding it changes no non-zero value)
// SC: the sine and cosine of q come in as sv and cv (smplx_sincos(q) evaluated elsewhere: the same bits) -- the
// SMPLX_TK_REV_*_T kinds only; what follows the sincos is the same sequence of operations
template <int J, bool OnRoot, bool SC = false>
__device__ __forceinline__ void apply_joint_const(double q, double T[12], double sv = 0.0, double cv = 0.0)
{
    constexpr int kind = CM_KIND[J];
    constexpr double tx = CM_TX[J], ty = CM_TY[J], tz = CM_TZ[J];
    if constexpr (OnRoot && SC && kind != SMPLX_TK_FIXED_T) {
        // apply_joint_t on the root link, the sincos taken out
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = 0.0;
        T[0] = 1.0; T[5] = 1.0; T[10] = 1.0;
        T[3] = tx; T[7] = ty; T[11] = tz;
        const double s = sv, c = cv;
        if constexpr (kind == SMPLX_TK_REV_X_T) { T[5] = c; T[6] = 0.0 - s; T[9] = s; T[10] = c; }
        else if constexpr (kind == SMPLX_TK_REV_Y_T) { T[0] = c; T[2] = s; T[8] = 0.0 - s; T[10] = c; }
        else { T[0] = c; T[1] = 0.0 - s; T[4] = s; T[5] = c; }
    } else if constexpr (OnRoot) {
        apply_joint_t(kind, tx, ty, tz, q, T, true);
    } else {
        if constexpr (tx != 0.0 || ty != 0.0 || tz != 0.0) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                double acc = 0.0;
                bool have = false;
                if constexpr (tx != 0.0) { acc = T[4 * i + 0] * tx; have = true; }
                if constexpr (ty != 0.0) { acc = have ? acc + T[4 * i + 1] * ty : T[4 * i + 1] * ty; have = true; }
                if constexpr (tz != 0.0) { acc = have ? acc + T[4 * i + 2] * tz : T[4 * i + 2] * tz; have = true; }
                T[4 * i + 3] = acc + T[4 * i + 3];
            }
        }
        if constexpr (kind != SMPLX_TK_FIXED_T) {
            double s, c;
            if constexpr (SC) { s = sv; c = cv; }
            else smplx_sincos(q, &s, &c);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double a = T[4 * i + 0], b = T[4 * i + 1], d = T[4 * i + 2];
                if constexpr (kind == SMPLX_TK_REV_X_T) { T[4 * i + 1] = b * c + d * s; T[4 * i + 2] = d * c - b * s; }
                else if constexpr (kind == SMPLX_TK_REV_Y_T) { T[4 * i + 0] = a * c - d * s; T[4 * i + 2] = a * s + d * c; }
                else { T[4 * i + 0] = a * c + b * s; T[4 * i + 1] = b * c - a * s; }
            }
        }
    }
}

// check_tree with the root sphere as literals, cut in two so that the root's grid lookup can be IN FLIGHT while the next
// joint of the chain is computed (every tree used to cost one exposed L2/HBM round trip: the compare-and-branch sat
// right behind its load).  issue_root computes the root position and starts the lookup; resolve_root, called after the
// next joint's arithmetic, looks at the answer: in free space the root clears and nothing is read from LDS; a root that
// does not clear hands over to the generic traversal at its children (larger child first, as check_tree does), with
// the link transform kept in C.Tp.  The order of the lookups -- and so the tally, also of a colliding configuration --
// is unchanged: tree k is resolved before tree k+1 is issued.
template <int T_>
__device__ __forceinline__ void issue_root(const SmplxGridDev& g, ChainState& C, int& lookups, double root_p[3])
{
    constexpr double cx = CM_ROOT_CX[T_], cy = CM_ROOT_CY[T_], cz = CM_ROOT_CZ[T_];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        // ((a*x + b*y) + c*z) + t with exactly-zero coefficients dropped (see apply_joint_const)
        double acc = 0.0;
        bool have = false;
        if constexpr (cx != 0.0) { acc = C.T[4 * i + 0] * cx; have = true; }
        if constexpr (cy != 0.0) { acc = have ? acc + C.T[4 * i + 1] * cy : C.T[4 * i + 1] * cy; have = true; }
        if constexpr (cz != 0.0) { acc = have ? acc + C.T[4 * i + 2] * cz : C.T[4 * i + 2] * cz; have = true; }
        root_p[i] = have ? acc + C.T[4 * i + 3] : C.T[4 * i + 3];
    }
    ++lookups;
#ifdef ABL_NO_LOOKUP
    C.pd2 = 60000 + (int)(root_p[0] * 0.0);
#else
    C.pd2 = grid_d2(g, root_p);
#endif
    if constexpr (CM_ROOT_LEFT[T_] >= 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) C.Tp[i] = C.T[i];   // only a tree that can be descended into needs its transform later
    }
}

template <int T_>
__device__ __forceinline__ bool resolve_root(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                             const double* Tp, int pd2, int& lookups)
{
    (void)M;
    if (!(pd2 < CM_ROOT_THR[T_])) return true;
    if constexpr (CM_ROOT_LEFT[T_] < 0) {
        return false;
    } else {
        // descend: the same loop as check_tree, entered below the root
        int sp = 0;
        int node;
        {
            const double rl = L.nodes[CM_ROOT_LEFT[T_]].r, rr = L.nodes[CM_ROOT_RIGHT[T_]].r;
            if (rl > rr) { lds_b(L, sp++) = (unsigned char)CM_ROOT_RIGHT[T_]; node = CM_ROOT_LEFT[T_]; }
            else { lds_b(L, sp++) = (unsigned char)CM_ROOT_LEFT[T_]; node = CM_ROOT_RIGHT[T_]; }
        }
        while (true) {
            const LDS_AS SmplxNode& nd = L.nodes[node];
            double c[3] = {nd.c[0], nd.c[1], nd.c[2]};
            double p[3];
            xform(Tp, c, p);
            ++lookups;
#ifdef ABL_NO_LOOKUP
            const int dd = 60000 + (int)(p[0] * 0.0);
#else
            const int dd = grid_d2(g, p);
#endif
            if (dd < nd.thr) {
                if (nd.left < 0) return false;
                const double rl = L.nodes[nd.left].r, rr = L.nodes[nd.right].r;
                if (rl > rr) { lds_b(L, sp++) = (unsigned char)nd.right; node = nd.left; }
                else { lds_b(L, sp++) = (unsigned char)nd.left; node = nd.right; }
                continue;
            }
            if (sp == 0) break;
            node = lds_b(L, --sp);
        }
        return true;
    }
}

// PT = the tree whose root lookup was issued at an earlier joint and has not been looked at yet (-1: none)
// SC: the SMPLX_TK_REV_*_T joints take C.sn / C.cs instead of evaluating smplx_sincos(C.q[var])
template <int J, int PT, bool RS = false, bool SC = false>
__device__ __forceinline__ bool const_chain(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                            ChainState& C, int& lookups)
{
    if constexpr (J < CM_NJ) {
        constexpr int kind = CM_KIND[J], var = CM_VAR[J], src = CM_SRC[J], save = CM_SAVE[J], tree = CM_TREE[J];
        if constexpr (src >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) C.T[i] = RS ? C.S[src][i] : lds_d(L, L.slot_base + 12 * src + i);
        }
        double q = 0.0;
        if constexpr (var >= 0) q = C.q[var];
        if constexpr (SC && kind > SMPLX_TK_FIXED_T && var >= 0) apply_joint_const<J, src == SMPLX_SRC_ROOT, true>(q, C.T, C.sn[var], C.cs[var]);
        else if constexpr (kind >= SMPLX_TK_FIXED_T) apply_joint_const<J, src == SMPLX_SRC_ROOT>(q, C.T);
        else apply_joint(&M->joints[J], q, C.T, src == SMPLX_SRC_ROOT);
        if constexpr (save >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) { if constexpr (RS) C.S[save][i] = C.T[i]; else lds_d(L, L.slot_base + 12 * save + i) = C.T[i]; }
        }
        // the lookup issued at the previous tree has had this joint's sincos and products to land behind
        if constexpr (PT >= 0) {
#ifndef ABL_NO_TREES
            if (!resolve_root<PT>(M, L, g, C.Tp, C.pd2, lookups)) return false;
#endif
        }
        if constexpr (tree >= 0) {
            double rp[3];
#ifdef ABL_NO_TREES
            rp[0] = C.T[3]; rp[1] = C.T[7]; rp[2] = C.T[11];
#else
            issue_root<tree>(g, C, lookups, rp);
#endif
            constexpr int slot = CM_ROOT_SLOT[tree];
            if constexpr (slot >= 0) { C.roots[3 * slot] = rp[0]; C.roots[3 * slot + 1] = rp[1]; C.roots[3 * slot + 2] = rp[2]; }
#ifndef ABL_NO_PAIRS
            const_pairs<tree, CM_PAIR_FIRST[tree], CM_PAIR_FIRST[tree + 1]>(L, C, rp);
#endif
            return const_chain<J + 1, tree, RS, SC>(M, L, g, C, lookups);
        } else {
            return const_chain<J + 1, -1, RS, SC>(M, L, g, C, lookups);
        }
    } else {
        if constexpr (PT >= 0) {
#ifndef ABL_NO_TREES
            return resolve_root<PT>(M, L, g, C.Tp, C.pd2, lookups);
#else
            return true;
#endif
        } else {
            return true;
        }
    }
}

// planning-link chain (planning_fk below) over the on-chain joints
template <int J, bool First>
__device__ __forceinline__ void const_planning_chain(const ModelLds* __restrict__ M, const double* __restrict__ q, double T[12])
{
    if constexpr (J < CM_NJ) {
        if constexpr (CM_ON_CHAIN[J] != 0) {
            constexpr int kind = CM_KIND[J], var = CM_VAR[J];
            double qv = 0.0;
            if constexpr (var >= 0) {
                qv = q[var];
                if constexpr (CM_VAR_TYPE[var] == SMPLX_JT_CONTINUOUS) qv = smplx_normalize_angle(qv);
            }
            if constexpr (kind >= SMPLX_TK_FIXED_T) apply_joint_const<J, First>(qv, T);
            else apply_joint(&M->joints[J], qv, T, First);
            const_planning_chain<J + 1, false>(M, q, T);
        } else {
            const_planning_chain<J + 1, First>(M, q, T);
        }
    }
}

// ... with the sines and cosines handed in: sn[v], cs[v] = smplx_sincos of q[v], normalised first where v is continuous
// (what the chain above evaluates itself), for every variable of CM_TRIG_PLANNING.  q is still what the other kinds take.
template <int J, bool First>
__device__ __forceinline__ void const_planning_chain_sc(const ModelLds* __restrict__ M, const double* __restrict__ q,
                                                        const double* __restrict__ sn, const double* __restrict__ cs, double T[12])
{
    if constexpr (J < CM_NJ) {
        if constexpr (CM_ON_CHAIN[J] != 0) {
            constexpr int kind = CM_KIND[J], var = CM_VAR[J];
            if constexpr (kind > SMPLX_TK_FIXED_T && var >= 0) {
                apply_joint_const<J, First, true>(0.0, T, sn[var], cs[var]);
            } else {
                double qv = 0.0;
                if constexpr (var >= 0) {
                    qv = q[var];
                    if constexpr (CM_VAR_TYPE[var] == SMPLX_JT_CONTINUOUS) qv = smplx_normalize_angle(qv);
                }
                if constexpr (kind >= SMPLX_TK_FIXED_T) apply_joint_const<J, First>(qv, T);
                else apply_joint(&M->joints[J], qv, T, First);
            }
            const_planning_chain_sc<J + 1, false>(M, q, sn, cs, T);
        } else {
            const_planning_chain_sc<J + 1, First>(M, q, sn, cs, T);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The parent's sines and cosines ("a parent's sines and cosines").  A frontier step keeps, per
// state, smplx_sincos of every joint value in its scratch (ExpandWork::trig, step.h): row[si] is 4 * CM_NV doubles,
//   [0, 2 NV)     (sin, cos) of q[v]                          -- what the collision chain evaluates
//   [2 NV, 4 NV)  (sin, cos) of smplx_normalize_angle(q[v]) where v is continuous, of q[v] otherwise -- the planning-link chain
// each pair 16 bytes, each half a run of 16-byte pieces.  On an edge almost every variable keeps the parent's bits
// (start + alpha * 0 == start), and smplx_sincos is a function of its argument's bits: such a variable takes the row's pair,
// the others are evaluated, one per lane and round (a wave runs as many rounds as its worst lane has changed variables).
// ---------------------------------------------------------------------------------------------
typedef double __attribute__((ext_vector_type(2))) trig_pair_t;

constexpr unsigned cm_trig_vars(bool planning)
{
    unsigned m = 0;
    for (int j = 0; j < CM_NJ; ++j)
        if (CM_KIND[j] > SMPLX_TK_FIXED_T && CM_VAR[j] >= 0 && (!planning || CM_ON_CHAIN[j] != 0)) m |= 1u << CM_VAR[j];
    return m;
}
constexpr unsigned CM_TRIG_COLLISION = cm_trig_vars(false);   // variables a SMPLX_TK_REV_*_T joint of the whole chain turns on
constexpr unsigned CM_TRIG_PLANNING = cm_trig_vars(true);     // ... of the planning-link chain
constexpr int cm_popcount(unsigned m) { int n = 0; for (; m != 0; m &= m - 1) ++n; return n; }
// Whether the step keeps the table for this robot.  An edge evaluates the one or two variables it moves whatever else
// happens, so the table saves at most (variables of CM_TRIG_COLLISION) - 2 sincos a configuration and costs a row of loads and
// registers: a robot with fewer than four such variables (the mixed-kinds test robot has one) computes as it always did.
constexpr bool CM_PARENT_TRIG = cm_popcount(CM_TRIG_COLLISION) >= 4;
constexpr unsigned CM_TRIG_ANY = CM_TRIG_COLLISION | CM_TRIG_PLANNING;   // variables whose pairs some consumer reads
#define SMPLX_TRIG_ROW (4 * CM_NV)

// one half of a state's row (raw: Norm = false) into registers
template <bool Norm>
__device__ __forceinline__ void trig_row_load(const double* __restrict__ trig, long long si, double (&row)[2 * CM_NV])
{
    const trig_pair_t* p = reinterpret_cast<const trig_pair_t*>(trig + si * SMPLX_TRIG_ROW + (Norm ? 2 * CM_NV : 0));
#pragma unroll
    for (int v = 0; v < CM_NV; ++v) { const trig_pair_t t = p[v]; row[2 * v] = t.x; row[2 * v + 1] = t.y; }
}

// sn[v], cs[v] for the variables of Mask: the row's pair where x[v] has the bits of the parent's value ref[v] (compared as
// integers: -0.0 is not +0.0), smplx_sincos(x[v]) -- Norm: of the normalised angle of a continuous variable -- otherwise
template <unsigned Mask, bool Norm>
__device__ __forceinline__ void parent_trig(const double (&x)[CM_NV], const double (&ref)[CM_NV], const double (&row)[2 * CM_NV],
                                            double (&sn)[CM_NV], double (&cs)[CM_NV])
{
    unsigned todo = 0;
#pragma unroll
    for (int v = 0; v < CM_NV; ++v) {
        sn[v] = row[2 * v]; cs[v] = row[2 * v + 1];
        if ((Mask >> v) & 1u)
            if (__double_as_longlong(x[v]) != __double_as_longlong(ref[v])) todo |= 1u << v;
    }
    while (todo != 0) {
        const int v = __ffs((int)todo) - 1;
        todo &= todo - 1;
        double a = x[0];
#pragma unroll
        for (int u = 1; u < CM_NV; ++u) a = v == u ? x[u] : a;
        if (Norm) {
            bool cont = false;
#pragma unroll
            for (int u = 0; u < CM_NV; ++u) if (CM_VAR_TYPE[u] == SMPLX_JT_CONTINUOUS) cont = cont || v == u;
            if (cont) a = smplx_normalize_angle(a);
        }
        double s, c;
        smplx_sincos(a, &s, &c);
#pragma unroll
        for (int u = 0; u < CM_NV; ++u) { sn[u] = v == u ? s : sn[u]; cs[u] = v == u ? c : cs[u]; }
    }
}
#endif   // SMPLX_CONST_MODEL

#ifdef SMPLX_CONST_MODEL
// fk_two_links for the per-robot build: the transforms of the links at joints ja and jb, the chain walked as in
// const_chain (same operations in the same order: identical bits), stopping behind the later of the two
template <int J, bool RS = false>
__device__ __forceinline__ void const_two_links(const ModelLds* __restrict__ M, const ThreadLds& L, double T[12], const double* q,
                                                int ja, int jb, int last, double Ta[12], double Tb[12], double (&S)[SMPLX_MAX_SLOTS][12])
{
    if constexpr (J < CM_NJ) {
        if (J > last) return;
        constexpr int kind = CM_KIND[J], var = CM_VAR[J], src = CM_SRC[J], save = CM_SAVE[J];
        if constexpr (src >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = RS ? S[src][i] : lds_d(L, L.slot_base + 12 * src + i);
        }
        double qv = 0.0;
        if constexpr (var >= 0) qv = q[var];
        if constexpr (kind >= SMPLX_TK_FIXED_T) apply_joint_const<J, src == SMPLX_SRC_ROOT>(qv, T);
        else apply_joint(&M->joints[J], qv, T, src == SMPLX_SRC_ROOT);
        if constexpr (save >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) { if constexpr (RS) S[save][i] = T[i]; else lds_d(L, L.slot_base + 12 * save + i) = T[i]; }
        }
        if (J == ja) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Ta[i] = T[i];
        }
        if (J == jb) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Tb[i] = T[i];
        }
        const_two_links<J + 1, RS>(M, L, T, q, ja, jb, last, Ta, Tb, S);
    }
}
#endif

// sphere tree vs sphere tree (self_collision_model.cpp:1093-1218); false = collision
template <bool RS = false>
__device__ __forceinline__ bool check_pair_full(const ModelLds* __restrict__ M, const ThreadLds& L, const EdgeRef& e,
                                             int ta, int tb)
{
    double Ta[12], Tb[12];
#ifdef SMPLX_CONST_MODEL
    {
        // per-robot build: the chain as straight-line code (the generic loop reads every joint record from LDS and
        // dispatches on its kind: under random configurations, where root spheres of checked pairs overlap in most
        // waves, it was 78 % of the K2 micro-benchmark)
        double T[12], q[CM_NV];
#pragma unroll
        for (int i = 0; i < 12; ++i) { T[i] = 0.0; Ta[i] = 0.0; Tb[i] = 0.0; }
#pragma unroll
        for (int v = 0; v < CM_NV; ++v) q[v] = lds_d(L, L.q_base + v);
        const int ja = M->tree_joint[ta], jb = M->tree_joint[tb];
        double S[SMPLX_MAX_SLOTS][12];
        const_two_links<0, RS>(M, L, T, q, ja, jb, ja > jb ? ja : jb, Ta, Tb, S);
    }
#else
    fk_two_links(M, L, e, M->tree_joint[ta], M->tree_joint[tb], Ta, Tb);
#endif
    int sp = 0;
    int na = M->tree_first[ta + 1] - 1, nb = M->tree_first[tb + 1] - 1;
    while (true) {
        const LDS_AS SmplxNode& A = L.nodes[na];
        const LDS_AS SmplxNode& B = L.nodes[nb];
        double ca[3] = {A.c[0], A.c[1], A.c[2]}, cb[3] = {B.c[0], B.c[1], B.c[2]};
        double pa[3], pb[3];
        xform(Ta, ca, pa);
        xform(Tb, cb, pb);
        const double dx = pb[0] - pa[0], dy = pb[1] - pa[1], dz = pb[2] - pa[2];
        const double cd2 = (dx * dx + dy * dy) + dz * dz;
        const double rr = A.r + B.r;
        if (!(cd2 > rr * rr)) {
            const bool la = A.left < 0, lb = B.left < 0;
            if (la && lb) return false;   // leaf x leaf: the ACM lookup by sphere name never matches (:1136)
            bool split_a;
            if (la) split_a = false;
            else if (lb) split_a = true;
            else split_a = A.r > B.r;
            // both children are visited unless pruned; visiting order does not change the boolean
            if (split_a) {
                lds_b(L, sp++) = (unsigned char)A.right; lds_b(L, sp++) = (unsigned char)nb;
                na = A.left;
            } else {
                lds_b(L, sp++) = (unsigned char)na; lds_b(L, sp++) = (unsigned char)B.right;
                nb = B.left;
            }
            continue;
        }
        if (sp == 0) break;
        nb = lds_b(L, --sp);
        na = lds_b(L, --sp);
    }
    return true;
}
