// smpl_amd/csrc/clearance.h -- distance to collision of one configuration and of one edge.
// Owns: ClrMin (the running minima and their witnesses), clearance_lds (the per-thread LDS layout of the clearance kernels),
// world_term, config_clearance_staged -- the counterpart of config_valid_staged (config_checks.h) -- with its parts
// (robot_world_clearance, pair_clearance, bodies_clearance) and edge_clearance.
// The value is made of the reference's per-sphere terms (SphereCollisionDistance, collision_operations.h:81-89, over
// distance_map.hpp:143-146, 292-300; sphereDistance, self_collision_model.cpp:1644-1649) taken over every LEAF sphere and
// every leaf pair the validity check tests; the reference's own collisionDistance (self_collision_model.cpp:1386-1511) is
// unfinished and is not restated.
#pragma once

#include "config_checks.h"

// A bounding sphere encloses the spheres below it up to the rounding of its radius (model_compile.cpp TreeBuilder): a
// subtree is skipped only where its bound clears the running minimum by this much
#define SMPLX_CLR_SLACK 1e-9

// witness kinds (include/smpl_amd.h)
enum { SMPLX_CLR_NONE = -1, SMPLX_CLR_ROBOT_WORLD = 0, SMPLX_CLR_ROBOT_ROBOT = 1, SMPLX_CLR_BODY_WORLD = 2,
       SMPLX_CLR_BODY_ROBOT = 3, SMPLX_CLR_BODY_BODY = 4 };

// the two running minima, each with the term that attains it: {kind, a, b, waypoint}
struct ClrMin {
    double world, self;
    int wkind, wa, wwp;
    int skind, sa, sb, swp;
};

__device__ __forceinline__ void clr_init(ClrMin& C)
{
    C.world = __builtin_inf(); C.self = __builtin_inf();
    C.wkind = SMPLX_CLR_NONE; C.wa = -1; C.wwp = 0;
    C.skind = SMPLX_CLR_NONE; C.sa = -1; C.sb = -1; C.swp = 0;
}
__device__ __forceinline__ void clr_world(ClrMin& C, double v, int kind, int a, int wp)
{
    if (v < C.world) { C.world = v; C.wkind = kind; C.wa = a; C.wwp = wp; }
}
__device__ __forceinline__ void clr_self(ClrMin& C, double v, int kind, int a, int b, int wp)
{
    if (v < C.self) { C.self = v; C.skind = kind; C.sa = a; C.sb = b; C.swp = wp; }
}

// clearance = min(world, self) and the witness of the smaller one (the world term's where they tie)
__device__ __forceinline__ void clr_store(const ClrMin& C, int i, double* __restrict__ out, double* __restrict__ parts,
                                          int* __restrict__ witness)
{
    const bool w = C.world <= C.self;
    out[i] = w ? C.world : C.self;
    if (parts) { parts[2 * (size_t)i] = C.world; parts[2 * (size_t)i + 1] = C.self; }
    if (witness) {
        int* o = witness + 4 * (size_t)i;
        if (w && C.wkind >= 0) { o[0] = C.wkind; o[1] = C.wa; o[2] = -1; o[3] = C.wwp; }
        else if (C.skind >= 0) { o[0] = C.skind; o[1] = C.sa; o[2] = C.sb; o[3] = C.swp; }
        else { o[0] = SMPLX_CLR_NONE; o[1] = -1; o[2] = -1; o[3] = 0; }
    }
}

// The clearance kernels keep the root position of EVERY tree (three doubles each, by tree index) where the validity kernels
// keep those of the trees that lead a checked pair: behind the chain the bound of any pair is at hand without a link
// transform.  The saved link transforms are in LDS in both builds (kernels.h smplx_clearance_lds_bytes is the size).
__device__ __forceinline__ ThreadLds clearance_lds(const SmplxSpaceDev* __restrict__ S, unsigned char* smem, ModelLds* Mv)
{
    ThreadLds L = setup_lds(S, smem, Mv, BLOCK, true);
    L.root_base = 0;
    L.slot_base = 3 * Mv->ntrees;
    L.q_base = L.slot_base + 12 * Mv->nslots;
    L.stk = (LDS_AS unsigned char*)(L.d + (L.q_base + Mv->nvars) * BLOCK);
    return L;
}

// SphereCollisionDistance (collision_operations.h:81-89): m_sqrt_table[d2] = res * sqrt(d2) (distance_map.hpp:143-146)
// less the padded radius.  d2 is capped at dmax_sqrd and 0 outside the grid (grid_d2).
__device__ __forceinline__ double world_term(double res, int d2, double r, double padding)
{
    return res * sqrt((double)d2) - (r + padding);
}

// sphereDistance (self_collision_model.cpp:1644-1649) in the sum order of check_pair_full
__device__ __forceinline__ double pair_term(const double pa[3], double ra, const double pb[3], double rb)
{
    const double dx = pb[0] - pa[0], dy = pb[1] - pa[1], dz = pb[2] - pa[2];
    return sqrt((dx * dx + dy * dy) + dz * dz) - (ra + rb);
}

// The chain, once: every leaf of every tree against the grid, every tree's root position into its LDS slot.  The nodes of
// a tree are taken four at a time with their lookups issued back to back (independent gathers; an inner node's is read
// and dropped) and reduced afterwards.
__device__ __forceinline__ void robot_world_clearance(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                                      double padding, ClrMin& C, int wp)
{
    double T[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.0;
    const int nj = M->njoints;
    for (int j = 0; j < nj; ++j) {
        JointPtr jt = &M->joints[j];
        const int src = jt->src, var = jt->var, save = jt->save_slot, t = jt->tree;
        if (src >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = lds_d(L, L.slot_base + 12 * src + i);
        }
        apply_joint(jt, var >= 0 ? lds_d(L, L.q_base + var) : 0.0, T, src == SMPLX_SRC_ROOT);
        if (save >= 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) lds_d(L, L.slot_base + 12 * save + i) = T[i];
        }
        if (t < 0) continue;
        const int first = M->tree_first[t], end = M->tree_first[t + 1];
        for (int n0 = first; n0 < end; n0 += 4) {
            int d2[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int nd = n0 + k < end ? n0 + k : end - 1;
                const double c[3] = {L.nodes[nd].c[0], L.nodes[nd].c[1], L.nodes[nd].c[2]};
                double p[3];
                xform(T, c, p);
                d2[k] = grid_d2(g, p);
                if (nd == end - 1) {     // the root is stored last
                    lds_d(L, L.root_base + 3 * t + 0) = p[0];
                    lds_d(L, L.root_base + 3 * t + 1) = p[1];
                    lds_d(L, L.root_base + 3 * t + 2) = p[2];
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int nd = n0 + k;
                if (nd < end && L.nodes[nd].left < 0)
                    clr_world(C, world_term(g.res, d2[k], L.nodes[nd].r, padding), SMPLX_CLR_ROBOT_WORLD, nd, wp);
            }
        }
    }
}

// leaf x leaf of the checked pair (a, b), a the group-earlier tree: branch and bound over the stack layout of
// check_pair_full (two bytes per split).  A node pair's bound is the pair term of its two bounding spheres; it is left out
// iff bound - SMPLX_CLR_SLACK > the running self minimum, and of two children the nearer is visited first.
__device__ __forceinline__ void pair_clearance(const ModelLds* __restrict__ M, const ThreadLds& L, const EdgeRef& e, int a, int b,
                                               ClrMin& C, int wp)
{
    double Ta[12], Tb[12];
    fk_two_links(M, L, e, M->tree_joint[a], M->tree_joint[b], Ta, Tb);
    int sp = 0;
    int na = M->tree_first[a + 1] - 1, nb = M->tree_first[b + 1] - 1;
    while (true) {
        const LDS_AS SmplxNode& A = L.nodes[na];
        const LDS_AS SmplxNode& B = L.nodes[nb];
        const double ca[3] = {A.c[0], A.c[1], A.c[2]}, cb[3] = {B.c[0], B.c[1], B.c[2]};
        double pa[3], pb[3];
        xform(Ta, ca, pa);
        xform(Tb, cb, pb);
        const double bound = pair_term(pa, A.r, pb, B.r);
        if (!(bound - SMPLX_CLR_SLACK > C.self)) {
            const bool la = A.left < 0, lb = B.left < 0;
            if (la && lb) {
                clr_self(C, bound, SMPLX_CLR_ROBOT_ROBOT, na, nb, wp);
            } else {
                bool split_a;
                if (la) split_a = false;
                else if (lb) split_a = true;
                else split_a = A.r > B.r;
                const LDS_AS SmplxNode& P = split_a ? A : B;
                const int c0 = P.left, c1 = P.right;
                const double k0[3] = {L.nodes[c0].c[0], L.nodes[c0].c[1], L.nodes[c0].c[2]};
                const double k1[3] = {L.nodes[c1].c[0], L.nodes[c1].c[1], L.nodes[c1].c[2]};
                double p0[3], p1[3];
                xform(split_a ? Ta : Tb, k0, p0);
                xform(split_a ? Ta : Tb, k1, p1);
                const double* other = split_a ? pb : pa;
                const double ro = split_a ? B.r : A.r;
                const bool first0 = !(pair_term(p1, L.nodes[c1].r, other, ro) < pair_term(p0, L.nodes[c0].r, other, ro));
                const int near = first0 ? c0 : c1, far = first0 ? c1 : c0;
                if (split_a) {
                    lds_b(L, sp++) = (unsigned char)far; lds_b(L, sp++) = (unsigned char)nb;
                    na = near;
                } else {
                    lds_b(L, sp++) = (unsigned char)na; lds_b(L, sp++) = (unsigned char)far;
                    nb = near;
                }
                continue;
            }
        }
        if (sp == 0) break;
        nb = lds_b(L, --sp);
        na = lds_b(L, --sp);
    }
}

// the checked tree pairs (smplx_model_pairs), from the root positions the chain left: the pairs of two single-sphere trees
// first (their bound IS their term, so the minimum is low before any pair is descended into), then the others
__device__ __forceinline__ void pairs_clearance(const ModelLds* __restrict__ M, const ThreadLds& L, const EdgeRef& e, ClrMin& C, int wp)
{
    for (int sweep = 0; sweep < 2; ++sweep) {
        for (int t = 0; t < M->ntrees; ++t) {
            for (int k = M->pair_first[t]; k < M->pair_first[t + 1]; ++k) {
                const int ta = M->pair_other[k];
                const int a = ta < t ? ta : t, b = ta < t ? t : ta;     // group order (config_valid_staged)
                const int na = M->tree_first[a + 1] - 1, nb = M->tree_first[b + 1] - 1;
                const LDS_AS SmplxNode& A = L.nodes[na];
                const LDS_AS SmplxNode& B = L.nodes[nb];
                const bool leaves = A.left < 0 && B.left < 0;
                if (leaves != (sweep == 0)) continue;
                const double pa[3] = {lds_d(L, L.root_base + 3 * a), lds_d(L, L.root_base + 3 * a + 1), lds_d(L, L.root_base + 3 * a + 2)};
                const double pb[3] = {lds_d(L, L.root_base + 3 * b), lds_d(L, L.root_base + 3 * b + 1), lds_d(L, L.root_base + 3 * b + 2)};
                const double bound = pair_term(pa, A.r, pb, B.r);
                if (leaves) clr_self(C, bound, SMPLX_CLR_ROBOT_ROBOT, na, nb, wp);
                else if (!(bound - SMPLX_CLR_SLACK > C.self)) pair_clearance(M, L, e, a, b, C, wp);
            }
        }
    }
}

// one body leaf (world position p, radius r, node nb_) against the leaves of robot tree t at link transform Tt
__device__ __forceinline__ void sphere_tree_clearance(const ModelLds* __restrict__ M, const ThreadLds& L, int t, const double Tt[12],
                                                      const double p[3], double r, int nb_, ClrMin& C, int wp)
{
    int sp = 0;
    int node = M->tree_first[t + 1] - 1;
    while (true) {
        const LDS_AS SmplxNode& nd = L.nodes[node];
        const double c[3] = {nd.c[0], nd.c[1], nd.c[2]};
        double w[3];
        xform(Tt, c, w);
        const double bound = pair_term(p, r, w, nd.r);
        if (!(bound - SMPLX_CLR_SLACK > C.self)) {
            if (nd.left < 0) {
                clr_self(C, bound, SMPLX_CLR_BODY_ROBOT, nb_, node, wp);
            } else {
                lds_b(L, sp++) = (unsigned char)nd.right;    // one byte per level, as sphere_hits_tree
                node = nd.left;
                continue;
            }
        }
        if (sp == 0) return;
        node = lds_b(L, --sp);
    }
}

// ... against the leaves of a later body's tree [root, end) at transform T (pre-order, no stack)
__device__ __forceinline__ void sphere_body_clearance(BodyNodePtr nodes, int root, int end, const double T[12], const double p[3],
                                                      double r, int nb_, ClrMin& C, int wp)
{
    int n = root;
    while (n < end) {
        const SMPLX_GLOBAL_AS SmplxNode& nd = nodes[n];
        const double c[3] = {nd.c[0], nd.c[1], nd.c[2]};
        double w[3];
        xform(T, c, w);
        const double bound = pair_term(p, r, w, nd.r);
        if (bound - SMPLX_CLR_SLACK > C.self) { n = nd.pad; continue; }
        if (nd.left < 0) { clr_self(C, bound, SMPLX_CLR_BODY_BODY, nb_, n, wp); n = nd.pad; }
        else n = n + 1;
    }
}

// body tree [root, end) at Tb against robot tree t (t >= 0) or a later body's tree [o_root, o_end), at To: the body's
// subtrees whose bound against the partner's root sphere clears the minimum are skipped, every other body leaf goes down the
// partner's tree (body_hits with distances)
__device__ __forceinline__ void body_partner_clearance(const ModelLds* __restrict__ M, const ThreadLds& L, BodyNodePtr nodes, int root,
                                                       int end, const double Tb[12], int t, int o_root, int o_end,
                                                       const double To[12], ClrMin& C, int wp)
{
    double rp[3], rr;
    if (t >= 0) {
        const LDS_AS SmplxNode& R = L.nodes[M->tree_first[t + 1] - 1];
        const double c[3] = {R.c[0], R.c[1], R.c[2]};
        xform(To, c, rp);
        rr = R.r;
    } else {
        const SMPLX_GLOBAL_AS SmplxNode& R = nodes[o_root];
        const double c[3] = {R.c[0], R.c[1], R.c[2]};
        xform(To, c, rp);
        rr = R.r;
    }
    int n = root;
    while (n < end) {
        const SMPLX_GLOBAL_AS SmplxNode& nd = nodes[n];
        const double c[3] = {nd.c[0], nd.c[1], nd.c[2]};
        double p[3];
        xform(Tb, c, p);
        if (pair_term(p, nd.r, rp, rr) - SMPLX_CLR_SLACK > C.self) { n = nd.pad; continue; }
        if (nd.left >= 0) { n = n + 1; continue; }
        if (t >= 0) sphere_tree_clearance(M, L, t, To, p, nd.r, n, C, wp);
        else sphere_body_clearance(nodes, o_root, o_end, To, p, nd.r, n, C, wp);
        n = nd.pad;
    }
}

// the attached bodies: every leaf against the grid; every body against the robot trees and the later bodies that
// bodies_valid (attached_bodies.h) tests it against
__device__ __forceinline__ void bodies_clearance(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                                 double padding, ClrMin& C, int wp)
{
    const BodiesPtr B = as_global(M->bodies);
    const int nb = B->n;
    const BodyNodePtr nodes = B->nodes;
    double Tb[12], To[12];
    for (int b = 0; b < nb; ++b) {
        const int root = B->body[b].root, end = B->body[b].end;
        const uint32_t allow_t = B->body[b].allow_trees, allow_b = B->body[b].allow_bodies;
        body_link_transform(M, L, B, B->body[b].joint, Tb);
        for (int n = root; n < end; ++n) {
            const SMPLX_GLOBAL_AS SmplxNode& nd = nodes[n];
            if (nd.left >= 0) continue;
            const double c[3] = {nd.c[0], nd.c[1], nd.c[2]};
            double p[3];
            xform(Tb, c, p);
            clr_world(C, world_term(g.res, grid_d2(g, p), nd.r, padding), SMPLX_CLR_BODY_WORLD, n, wp);
        }
        for (int t = 0; t < M->ntrees; ++t) {
            if ((allow_t >> t) & 1u) continue;
            body_link_transform(M, L, B, M->tree_joint[t], To);
            body_partner_clearance(M, L, nodes, root, end, Tb, t, 0, 0, To, C, wp);
        }
        for (int o = b + 1; o < nb; ++o) {
            if ((allow_b >> o) & 1u) continue;
            body_link_transform(M, L, B, B->body[o].joint, To);
            body_partner_clearance(M, L, nodes, root, end, Tb, -1, B->body[o].root, B->body[o].end, To, C, wp);
        }
    }
}

// One configuration, its joint values staged in the thread's LDS (stage_config): its terms join the running minima of C
// under waypoint index wp.  The pruning only ever compares with the running SELF minimum, so C.self is the exact minimum
// of the pair terms on its own, whatever C.world is.
__device__ __forceinline__ void config_clearance_staged(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                                        const EdgeRef& e, double padding, ClrMin& C, int wp)
{
    robot_world_clearance(M, L, g, padding, C, wp);
    pairs_clearance(M, L, e, C, wp);
    if (M->bodies) bodies_clearance(M, L, g, padding, C, wp);    // uniform: the query has attached bodies
}

// The minimum over the configurations isStateToStateValid interpolates (edge_valid): waypoint j of W at alpha = j * (1 / (W - 1)).
// An edge without motion (W == 0), which the edge CHECK passes without visiting anything, answers with its start
// configuration as waypoint 0.  The minima run on from waypoint to waypoint, so later waypoints prune against earlier ones.
__device__ __forceinline__ void edge_clearance(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g,
                                               const double* __restrict__ start, const double* __restrict__ finish, double padding,
                                               ClrMin& C)
{
    const int W = edge_waypoint_count(M, start, finish);
    EdgeRef e;
    e.start = start;
    e.finish = finish;
    e.alpha = 0.0;
    if (W == 0) {
        stage_config(M, L, e);
        config_clearance_staged(M, L, g, e, padding, C, 0);
        return;
    }
    const double inv = 1.0 / (double)(W - 1);
    for (int j = 0; j < W; ++j) {
        e.alpha = (double)j * inv;
        stage_config(M, L, e);
        config_clearance_staged(M, L, g, e, padding, C, j);
    }
}
