// smpl_amd/csrc/bfs_record.h -- one cell of the BFS distance field read out of its brick-major records (device_types.h
// SmplxBfsDev): bfs_in_bounds and bfs_dist, for the heuristic (lattice_steps.h) and for k_bfs_export (bfs_kernels.h).
// Needs nothing from the model or collision headers.
// Restates: bfs3d.h:151-155, 213-220.
#pragma once

#include "kernels.h"   // SMPLX_GLOBAL_AS

// BFS_3D::inBounds / getNode (bfs3d.h:151-155, 213-220)
__device__ __forceinline__ bool bfs_in_bounds(const SmplxBfsDev& b, const int c[3])
{
    return !(c[0] < 0 || c[1] < 0 || c[2] < 0 || c[0] >= b.dim_x - 2 || c[1] >= b.dim_y - 2 || c[2] >= b.dim_z - 2);
}
__device__ __forceinline__ int bfs_dist(const SmplxBfsDev& b, const int c[3])
{
    const size_t brick = ((size_t)(c[2] >> 3) * b.nby + (c[1] >> 3)) * b.nbx + (c[0] >> 3);
    const SMPLX_GLOBAL_AS int* dist = (const SMPLX_GLOBAL_AS int*)b.dist;     // (device memory, not a flat address: see grid_d2)
    const int v = dist[brick * SMPLX_BFS_REC + ((c[2] & 7) << 6) + ((c[1] & 7) << 3) + (c[0] & 7)];
    if (v == 0x7FFFFFFF) return v;
    return ((v ^ b.tag_word) & b.tag_mask) != 0 ? -1 : (v & ~b.tag_mask);     // another run's value: UNDISCOVERED
}
