// smpl_amd/csrc/clearance_kernels.h -- the clearance queries of the C-ABI, one thread per row.
// Owns: k_state_clearance (CollisionDistanceExtension::distanceToCollision(state), collision_checker.h:132-144) and
// k_edge_clearance (distanceToCollision(start, finish)).  Both use the generic chain in either build (clearance.h); the
// space's padding arrives as an argument (the device model holds it only folded into the nodes' thresholds).
// out_parts (n x 2: world, self) and out_witness (n x 4: kind, a, b, waypoint) may be null.
#pragma once

#include "clearance.h"

extern "C" __global__ void __launch_bounds__(BLOCK)
k_state_clearance(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Q, int n, double padding,
                  double* __restrict__ out, double* __restrict__ out_parts, int* __restrict__ out_witness)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ModelLds Mv;
    ThreadLds L = clearance_lds(S, smem, &Mv);
    const ModelLds* M = &Mv;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    EdgeRef e;
    e.start = Q + (size_t)i * MV_NVARS(M); e.finish = e.start; e.alpha = 0.0;
    const SmplxGridDev grid = S->grid;
    ClrMin C;
    clr_init(C);
    stage_config(M, L, e);
    config_clearance_staged(M, L, grid, e, padding, C, 0);
    clr_store(C, i, out, out_parts, out_witness);
}

extern "C" __global__ void __launch_bounds__(BLOCK)
k_edge_clearance(const SmplxSpaceDev* __restrict__ S, const double* __restrict__ Aq, const double* __restrict__ Bq, int n,
                 double padding, double* __restrict__ out, double* __restrict__ out_parts, int* __restrict__ out_witness)
{
    extern __shared__ __align__(16) unsigned char smem[];
    ModelLds Mv;
    ThreadLds L = clearance_lds(S, smem, &Mv);
    const ModelLds* M = &Mv;
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const SmplxGridDev grid = S->grid;
    ClrMin C;
    clr_init(C);
    edge_clearance(M, L, grid, Aq + (size_t)i * MV_NVARS(M), Bq + (size_t)i * MV_NVARS(M), padding, C);
    clr_store(C, i, out, out_parts, out_witness);
}
