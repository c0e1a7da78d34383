// smpl_amd/csrc/attached_bodies.h -- collision bodies attached to robot links (device_types.h SmplxBodiesDev).
// Owns: body_joint_step, the one out-of-line device function, and body_link_transform; body trees against the grid, the
// robot's trees and each other; bodies_valid, which config_valid_staged (config_checks.h) calls behind the robot's own
// checks.
// Restates: attached_bodies_collision_model.cpp; self_collision_model.cpp:407-428, 1093-1218, 1270-1345;
// collision_operations.h:105-164.
#pragma once

#include "model_lds.h"
#include "sphere_checks.h"   // grid_d2

// ---------------------------------------------------------------------------------------------
// Attached bodies (device_types.h SmplxBodiesDev).  Checked after the robot's own trees and pairs have passed, so a space
// without bodies pays one uniform branch on a null pointer.  The trees are walked in pre-order without a stack; the
// order of the walk differs from the reference's (larger child first), which leaves the verdicts unchanged, and the
// lookup tallies too where the configuration is valid (every node whose ancestors all fail the test is looked up).
// ---------------------------------------------------------------------------------------------
typedef const SMPLX_GLOBAL_AS SmplxBodiesDev* BodiesPtr;
typedef const SMPLX_GLOBAL_AS SmplxNode* BodyNodePtr;

// One joint of a body's link chain, out of line: inlined into the ancestor loop, the generic joint (every kind, chosen at run
// time) raised the collision kernels by up to 70 VGPRs and made k_expand spill, also where no body is attached; as a call
// it costs them nothing (a 208-byte stack frame, used only by the call).
struct BodyT { double t[12]; };
__device__ __attribute__((noinline)) BodyT body_joint_step(JointPtr jt, double q, BodyT T)
{
    apply_joint(jt, q, T.t, jt->src == SMPLX_SRC_ROOT);
    return T;
}

// transform of the child link of joint j (-1: the root link): the joints on its path from the root in depth-first
// order, the operations the chain pass performs on the same values (identical bits)
__device__ __forceinline__ void body_link_transform(const ModelLds* __restrict__ M, const ThreadLds& L, BodiesPtr B, int j,
                                                    double T[12])
{
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = 0.0;
    T[0] = 1.0; T[5] = 1.0; T[10] = 1.0;
    unsigned long long m = j >= 0 ? B->ancestors[j] : 0ull;
    while (m) {
        const int a = __ffsll((long long)m) - 1;
        m &= m - 1;
        JointPtr jt = &M->joints[a];
        const int var = jt->var;
        BodyT x;
#pragma unroll
        for (int i = 0; i < 12; ++i) x.t[i] = T[i];
        x = body_joint_step(jt, var >= 0 ? lds_d(L, L.q_base + var) : 0.0, x);
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = x.t[i];
    }
}

__device__ __forceinline__ bool spheres_overlap(const double a[3], double ra, const double b[3], double rb)
{
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    const double cd2 = (dx * dx + dy * dy) + dz * dz;
    const double rr = ra + rb;
    return !(cd2 > rr * rr);     // self_collision_model.cpp:1124-1130
}

// body tree vs the grid (collision_operations.h:105-164): false at the first colliding leaf
__device__ __forceinline__ bool body_vs_grid(BodyNodePtr nodes, int root, int end, const double T[12], const SmplxGridDev& g,
                                             int& lookups)
{
    int n = root;
    while (n < end) {
        const SMPLX_GLOBAL_AS SmplxNode& nd = nodes[n];
        const double c[3] = {nd.c[0], nd.c[1], nd.c[2]};
        double p[3];
        xform(T, c, p);
        ++lookups;
        if (grid_d2(g, p) < nd.thr) {
            if (nd.left < 0) return false;
            n = n + 1;                  // pre-order: the left child follows
        } else {
            n = nd.pad;                 // the sphere clears: skip its subtree
        }
    }
    return true;
}

// one world sphere against robot tree t at link transform Tt: true if a leaf of the tree overlaps it
__device__ __forceinline__ bool sphere_hits_tree(const ModelLds* __restrict__ M, const ThreadLds& L, int t, const double Tt[12],
                                                 const double p[3], double r)
{
    int sp = 0;
    int node = M->tree_first[t + 1] - 1;
    while (true) {
        const LDS_AS SmplxNode& nd = L.nodes[node];
        const double c[3] = {nd.c[0], nd.c[1], nd.c[2]};
        double w[3];
        xform(Tt, c, w);
        if (spheres_overlap(w, nd.r, p, r)) {
            if (nd.left < 0) return true;
            lds_b(L, sp++) = (unsigned char)nd.right;    // one byte per level, as check_tree (stack_bytes covers the depth)
            node = nd.left;
            continue;
        }
        if (sp == 0) return false;
        node = lds_b(L, --sp);
    }
}

// one world sphere against a body's tree at transform T: true if a leaf overlaps it
__device__ __forceinline__ bool sphere_hits_body(BodyNodePtr nodes, int root, int end, const double T[12], const double p[3], double r)
{
    int n = root;
    while (n < end) {
        const SMPLX_GLOBAL_AS SmplxNode& nd = nodes[n];
        const double c[3] = {nd.c[0], nd.c[1], nd.c[2]};
        double w[3];
        xform(T, c, w);
        if (spheres_overlap(w, nd.r, p, r)) {
            if (nd.left < 0) return true;
            n = n + 1;
        } else {
            n = nd.pad;
        }
    }
    return false;
}

// body tree vs robot tree t, or vs another body (other_body >= 0): true if a leaf of one overlaps a leaf of the other
// (self_collision_model.cpp:1093-1218: leaf x leaf is a collision).  The body's subtrees that miss the partner's root
// sphere are skipped; every body leaf that meets it is tested against the partner's whole tree.
__device__ __forceinline__ bool body_hits(const ModelLds* __restrict__ M, const ThreadLds& L, BodyNodePtr nodes, int root, int end,
                                          const double Tb[12], int t, int o_root, int o_end, const double To[12])
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
        if (!spheres_overlap(rp, rr, p, nd.r)) { n = nd.pad; continue; }
        if (nd.left >= 0) { n = n + 1; continue; }
        if (t >= 0 ? sphere_hits_tree(M, L, t, To, p, nd.r) : sphere_hits_body(nodes, o_root, o_end, To, p, nd.r)) return true;
        n = nd.pad;
    }
    return false;
}

// the attached bodies of a configuration whose robot checks passed (self_collision_model.cpp:407-428 with the bodies of
// attached_bodies_collision_model.cpp): every body vs the grid, then vs the robot's trees and the other bodies its
// allowed list does not name (self_collision_model.cpp:1270-1345)
__device__ __forceinline__ bool bodies_valid(const ModelLds* __restrict__ M, const ThreadLds& L, const SmplxGridDev& g, int& lookups)
{
    const BodiesPtr B = as_global(M->bodies);
    const int nb = B->n;
    const BodyNodePtr nodes = B->nodes;
    double Tb[12], To[12];
    for (int b = 0; b < nb; ++b) {
        body_link_transform(M, L, B, B->body[b].joint, Tb);
        if (!body_vs_grid(nodes, B->body[b].root, B->body[b].end, Tb, g, lookups)) return false;
    }
    for (int b = 0; b < nb; ++b) {
        const int root = B->body[b].root, end = B->body[b].end;
        const uint32_t allow_t = B->body[b].allow_trees, allow_b = B->body[b].allow_bodies;
        body_link_transform(M, L, B, B->body[b].joint, Tb);
        for (int t = 0; t < M->ntrees; ++t) {
            if ((allow_t >> t) & 1u) continue;
            body_link_transform(M, L, B, M->tree_joint[t], To);
            if (body_hits(M, L, nodes, root, end, Tb, t, 0, 0, To)) return false;
        }
        for (int o = b + 1; o < nb; ++o) {
            if ((allow_b >> o) & 1u) continue;
            body_link_transform(M, L, B, B->body[o].joint, To);
            if (body_hits(M, L, nodes, root, end, Tb, -1, B->body[o].root, B->body[o].end, To)) return false;
        }
    }
    return true;
}
