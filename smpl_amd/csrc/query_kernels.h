// smpl_amd/csrc/query_kernels.h -- the batch queries of the C-ABI, one thread per row.
// Owns: k_edge_valid, k_state_valid (CollisionChecker::isStateToStateValid, isStateValid), k_heuristic
// (BfsHeuristic::GetGoalHeuristic), k_heuristic_closed (GetGoalHeuristic of the two closed-form kinds), k_planning_pose
// (computePlanningLinkFK), k_bfs_metric (BfsHeuristic::getMetricGoalDistance, bfs_heuristic.cpp:129-138),
// k_sphere_positions and k_attached_positions (debug / parity).
#pragma once

#include "config_checks.h"
#include "lattice_steps.h"

extern "C" __global__ void __launch_bounds__(BLOCK, 2)   // >= 2 waves per SIMD: at most 256 VGPRs, whichever compiler builds it
k_edge_valid(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Aq, const double* __restrict__ Bq, int n,
             unsigned char* __restrict__ out, int* __restrict__ out_lookups, int* __restrict__ out_waypoints)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ModelLds Mv;
#ifdef SMPLX_CONST_MODEL
    constexpr bool RS = true;      // as k_state_valid below
#else
    constexpr bool RS = false;
#endif
    ThreadLds L = setup_lds(S, smem, &Mv, BLOCK, !RS);
    const ModelLds* M = &Mv;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    int lk = 0, W = 0;
    const SmplxGridDev grid = S->grid;
    const bool ok = edge_valid<RS>(M, L, grid, Aq + (size_t)i * MV_NVARS(M), Bq + (size_t)i * MV_NVARS(M), false, true, lk, W);
    out[i] = ok ? 1 : 0;
    if (out_lookups) out_lookups[i] = lk;
    if (out_waypoints) out_waypoints[i] = W;
}

extern "C" __global__ void __launch_bounds__(BLOCK, 2)   // >= 2 waves per SIMD: at most 256 VGPRs, whichever compiler builds it
k_state_valid(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int n, unsigned char* __restrict__ out,
              int* __restrict__ out_lookups)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ModelLds Mv;
#ifdef SMPLX_CONST_MODEL
    constexpr bool RS = true;      // saved link transforms in registers: engine.hip sizes this kernel's LDS without the slots
#else
    constexpr bool RS = false;
#endif
    ThreadLds L = setup_lds(S, smem, &Mv, BLOCK, !RS);
    const ModelLds* M = &Mv;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    EdgeRef e;
    e.start = Q + (size_t)i * MV_NVARS(M); e.finish = e.start; e.alpha = 0.0;
    int lk = 0;
    const SmplxGridDev grid = S->grid;
    const bool ok = config_valid<RS>(M, L, grid, e, lk);
    out[i] = ok ? 1 : 0;
    if (out_lookups) out_lookups[i] = lk;
}

extern "C" __global__ void __launch_bounds__(BLOCK)
k_heuristic(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int n, int* __restrict__ out_h,
            double* __restrict__ out_xyz)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const ModelLds Mv = setup_model_only(S, smem);
    const ModelLds* M = &Mv;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double p[3];
    planning_fk(M, Q + (size_t)i * MV_NVARS(M), p);
    int c[3];
    world_to_cell(S->grid, p, c);
    out_h[i] = bfs_cost_to_goal(S->bfs, c);
    if (out_xyz) { out_xyz[3 * i] = p[0]; out_xyz[3 * i + 1] = p[1]; out_xyz[3 * i + 2] = p[2]; }
}

// k_heuristic for a space of a closed-form kind (lattice_steps.h closed_form_of; the host picks the kernel, engine.hip
// run_heuristic): the same chain with its rotation, the h every expansion kernel gives the state.  A kernel of its own
// because the rotation and the goal record cost the per-robot k_heuristic 28 VGPRs and three occupancy steps when the
// two shared one body; k_heuristic is the text it was.
extern "C" __global__ void __launch_bounds__(BLOCK)
k_heuristic_closed(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int n, int* __restrict__ out_h,
                   double* __restrict__ out_xyz)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const ModelLds Mv = setup_model_only(S, smem);
    const ModelLds* M = &Mv;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const SMPLX_GLOBAL_AS SmplxHeurDev* H = closed_form_of(S->bfs);
    const double* q = Q + (size_t)i * MV_NVARS(M);
    double p[3], R[9];
    planning_fk(M, q, p, R);
    out_h[i] = H ? closed_form_h(M, H, p, R, q) : 0;      // (never launched for a BFS space)
    if (out_xyz) { out_xyz[3 * i] = p[0]; out_xyz[3 * i + 1] = p[1]; out_xyz[3 * i + 2] = p[2]; }
}

// planning-link transforms (computePlanningLinkFK) of a batch of states, row-major 3x4 each
extern "C" __global__ void __launch_bounds__(BLOCK)
k_planning_pose(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int n, double* __restrict__ out_T)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const ModelLds Mv = setup_model_only(S, smem);
    const ModelLds* M = &Mv;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    double p[3], R[9];
    planning_fk(M, Q + (size_t)i * MV_NVARS(M), p, R);
    double* T = out_T + (size_t)i * 12;
#pragma unroll
    for (int r = 0; r < 3; ++r) { T[4 * r] = R[3 * r]; T[4 * r + 1] = R[3 * r + 1]; T[4 * r + 2] = R[3 * r + 2]; T[4 * r + 3] = p[r]; }
}

// BfsHeuristic::getMetricGoalDistance (bfs_heuristic.cpp:129-138) for a batch of workspace points
extern "C" __global__ void __launch_bounds__(BLOCK)
k_bfs_metric(SmplxGridDev grid, SmplxBfsDev bfs, const double* __restrict__ xyz, int n, double* __restrict__ out)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double p[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    int c[3];
    world_to_cell(grid, p, c);
    out[i] = !bfs_in_bounds(bfs, c) ? (double)0x7FFFFFFF * grid.res : (double)bfs_dist(bfs, c) * grid.res;
}

// debug/parity: world positions of every tree node for one configuration per thread
extern "C" __global__ void __launch_bounds__(BLOCK)
k_sphere_positions(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int n, double* __restrict__ out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ModelLds Mv;
    ThreadLds L = setup_lds(S, smem, &Mv);
    const ModelLds* M = &Mv;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const double* q = Q + (size_t)i * MV_NVARS(M);
    double T[12];
    for (int k = 0; k < 12; ++k) T[k] = 0.0;
    for (int j = 0; j < M->njoints; ++j) {
        JointPtr jt = &M->joints[j];
        if (jt->src >= 0) for (int k = 0; k < 12; ++k) T[k] = lds_d(L, L.slot_base + 12 * jt->src + k);
        apply_joint(jt, jt->var >= 0 ? q[jt->var] : 0.0, T, jt->src == SMPLX_SRC_ROOT);
        if (jt->save_slot >= 0) for (int k = 0; k < 12; ++k) lds_d(L, L.slot_base + 12 * jt->save_slot + k) = T[k];
        if (jt->tree >= 0) {
            for (int nd = M->tree_first[jt->tree]; nd < M->tree_first[jt->tree + 1]; ++nd) {
                double c[3] = {L.nodes[nd].c[0], L.nodes[nd].c[1], L.nodes[nd].c[2]};
                double p[3];
                xform(T, c, p);
                double* o = out + ((size_t)i * M->nnodes + nd) * 3;
                o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
            }
        }
    }
}

// world positions of every attached-body node (SmplxBodiesDev order) for one configuration per thread
extern "C" __global__ void __launch_bounds__(BLOCK)
k_attached_positions(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int n, double* __restrict__ out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ModelLds Mv;
    ThreadLds L = setup_lds(S, smem, &Mv);
    const ModelLds* M = &Mv;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n || !M->bodies) return;
    EdgeRef e;
    e.start = Q + (size_t)i * MV_NVARS(M); e.finish = e.start; e.alpha = 0.0;
    stage_config(M, L, e);
    const BodiesPtr B = as_global(M->bodies);
    const int nn = B->nnodes;
    for (int b = 0; b < B->n; ++b) {
        double T[12];
        body_link_transform(M, L, B, B->body[b].joint, T);
        for (int nd = B->body[b].root; nd < B->body[b].end; ++nd) {
            const double c[3] = {B->nodes[nd].c[0], B->nodes[nd].c[1], B->nodes[nd].c[2]};
            double p[3];
            xform(T, c, p);
            double* o = out + ((size_t)i * nn + nd) * 3;
            o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
        }
    }
}
