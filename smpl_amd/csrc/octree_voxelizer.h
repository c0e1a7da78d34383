// smpl_amd/csrc/octree_voxelizer.h -- the octree voxeliser of field.hip (SMPLX_SHAPE_OCTREE), over the arithmetic of
// octree_points.h.  Reference: sbpl_collision_checking/src/voxel_operations.cpp:405-436 (VoxelizeOcTree), then
// OccupancyGrid::worldToGrid (smpl/include/smpl/distance_map/detail/distance_map.hpp:520-527).
//
// Octrees are no meshes: a leaf is sampled at points, every point becomes a cell, and the list keeps them in generation
// order with duplicates.  Only the leaf rows (32 bytes each) cross to the device.  k_oct_trips gives every (leaf, axis)
// the trips of its loop; their products are scanned on the device (vox_common.h scan_exclusive, level by level);
// k_oct_points gives one thread one sample point and compacts the in-grid cells in order the way k_vox_compact does --
// chunk counts first, then, after the device scan of the counts, the write -- recomputing the point in the second pass
// instead of storing it.  The list is then added with occ_points.  The host reads back 32 bytes: the number of cells (to
// allocate the list) and the list's bounding range (for the edit window).
#pragma once

#include <climits>

#include "octree_points.h"
#include "vox_common.h"
#include "voxelize.h"

namespace {

// one thread per (leaf, axis): the trips of that loop, by the loop's own arithmetic.  The first six threads also empty
// the call's bounding range (x0 y0 z0 x1 y1 z1).
__global__ void __launch_bounds__(FIELD_BLOCK)
k_oct_trips(const double* __restrict__ leaves, int nleaves, double res, int* __restrict__ trips, int* __restrict__ box)
{
    const int i = blockIdx.x * FIELD_BLOCK + threadIdx.x;
    if (i < 6) box[i] = i < 3 ? INT_MAX : INT_MIN;
    if (i >= 3 * nleaves) return;
    const double* L = leaves + 4 * (size_t)(i / 3);
    trips[i] = oct_single(L[3], res) ? 1 : oct_axis_trips(L[i % 3], L[3], res);
}

// a chunk is one point a thread: the search for a point's leaf is a chain of dependent loads, so a thread that walks
// several points one after another (as k_vox_compact walks mask bytes) pays that latency several times over while a
// small octree leaves most of the device idle (profiles/octree_ab.txt)
#define OCT_CHUNK FIELD_BLOCK

struct OctGrid { double pose[12]; double origin_minus_res[3]; double inv_res, res; int n[3]; };

// one block per chunk of OCT_CHUNK sample points, one thread per point: the point's leaf by a search over the prefix, its
// (i, j, k) from the leaf's trips, the coordinates by the running sums, the pose, the cell.  The host launches a block
// for every chunk the BOUND on the points asks for (it never learns their number); a block past the last point has
// nothing to do.  Write == false: chunk_n[chunk] = points of the chunk whose cell lies inside the grid, entry gridDim.x is
// 0 (the scan turns it into the total), and box (x0 y0 z0 x1 y1 z1) grows to hold those cells.  Write == true: chunk_n
// holds the exclusive scan; the cells go to cells[chunk_n[chunk] + rank], in generation order (block_rank).
template <bool Write>
__global__ void __launch_bounds__(FIELD_BLOCK)
k_oct_points(const double* __restrict__ leaves, const int* __restrict__ trips, const long long* __restrict__ first, int nleaves, OctGrid G,
             long long* __restrict__ chunk_n, int* __restrict__ cells, int* __restrict__ box)
{
    __shared__ int wave_n[FIELD_BLOCK / 64];
    __shared__ int sbox[6];
    const long long total = first[nleaves];
    const long long begin = (long long)blockIdx.x * OCT_CHUNK;
    if (!Write && blockIdx.x == 0 && threadIdx.x == 0) chunk_n[gridDim.x] = 0;
    if (begin >= total) {                                  // the whole block alike
        if (!Write && threadIdx.x == 0) chunk_n[blockIdx.x] = 0;
        return;
    }
    if (!Write && threadIdx.x < 6) sbox[threadIdx.x] = threadIdx.x < 3 ? INT_MAX : INT_MIN;
    const long long p = begin + threadIdx.x;
    int c[3] = {-1, -1, -1};
    if (p < total) {
        int lo = 0, hi = nleaves;                          // first[lo] <= p < first[hi]; leaves without points are passed over
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= p) lo = mid; else hi = mid;
        }
        const double* L = leaves + 4 * (size_t)lo;
        const int* t = trips + 3 * (size_t)lo;
        const long long local = p - first[lo];
        const int k[3] = {(int)(local / ((long long)t[2] * t[1])), (int)(local / t[2] % t[1]), (int)(local % t[2])};
        const double v[3] = {oct_axis_value(L[0], L[3], G.res, k[0]), oct_axis_value(L[1], L[3], G.res, k[1]), oct_axis_value(L[2], L[3], G.res, k[2])};
        double w[3];
        vox_transform(G.pose, v, w);
        for (int a = 0; a < 3; ++a) c[a] = oct_world_to_cell(w[a], G.origin_minus_res[a], G.inv_res);
    }
    const bool on = c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[0] < G.n[0] && c[1] < G.n[1] && c[2] < G.n[2];
    const BlockRank r = block_rank(on, wave_n);
    if (Write) {
        if (on) {
            int* out = cells + 3 * (size_t)(chunk_n[blockIdx.x] + r.before + r.rank);
            out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
        }
        return;
    }
    if (on)
        for (int a = 0; a < 3; ++a) { atomicMin(&sbox[a], c[a]); atomicMax(&sbox[3 + a], c[a]); }
    __syncthreads();
    if (threadIdx.x == 0) chunk_n[blockIdx.x] = r.all;
    if (threadIdx.x < 6) {
        if (threadIdx.x < 3) atomicMin(&box[threadIdx.x], sbox[threadIdx.x]); else atomicMax(&box[threadIdx.x], sbox[threadIdx.x]);
    }
}

// the limits of octree_points.h over the octree shapes of one call, checked before anything is allocated or launched
int octree_limits(const std::vector<WorldShape>& shapes, double res)
{
    long long bound = 0, leaves = 0;
    for (const WorldShape& s : shapes) {
        if (s.type != SMPLX_SHAPE_OCTREE) continue;
        leaves += (long long)(s.vertices.size() / 4);
        if (leaves > OCT_MAX_LEAVES) return smplx_internal_set_error(SMPLX_E_LIMIT, "more than 2^28 octree leaves in one call");
        for (size_t k = 3; k < s.vertices.size(); k += 4) {
            if (!(s.vertices[k] / res <= OCT_MAX_RATIO)) return smplx_internal_set_error(SMPLX_E_LIMIT, "an octree leaf is wider than 1024 cells of the grid");
            const long long b = oct_axis_bound(s.vertices[k], res);
            bound += b * b * b;
            if (bound > OCT_MAX_POINTS) return smplx_internal_set_error(SMPLX_E_LIMIT, "the octree leaves may sample more than 2^31 / 3 points at this resolution");
        }
    }
    return SMPLX_OK;
}

// the cell list of one octree shape: the cells of its sample points that lie inside the grid, in generation order,
// duplicates kept; out is the list of that one shape.  The leaves' trips, the prefix of their point counts and the chunk
// counts of the compaction live in the grid's work space; the only allocation is the list.  One upload (the leaf rows)
// and one download (the number of cells and their bounding range, 32 bytes): the number of sample points stays on the
// device, the chunks being launched for their bound.  With edit the cells also become obstacles through occ_points (the
// caller updates the field).  Waits for the device.
int octree_run(const smplx_grid* g, const WorldShape& s, bool edit, VoxLists& out)
{
    out.first.assign(2, 0);
    out.box = {0, 0, 0, -1, -1, -1};
    const int nl = (int)(s.vertices.size() / 4);
    long long bound = 0;                               // octree_limits has held it to OCT_MAX_POINTS
    for (size_t k = 3; k < s.vertices.size(); k += 4) { const long long b = oct_axis_bound(s.vertices[k], g->res); bound += b * b * b; }
    const int nchunks = (int)((bound + OCT_CHUNK - 1) / OCT_CHUNK);
    struct Found { long long ncells; int box[6]; } found;      // as they lie behind the chunk counts
    const size_t bytes[5] = {sizeof(double) * 4 * (size_t)nl, sizeof(int) * 3 * (size_t)nl, sizeof(long long) * ((size_t)nl + 1),
                             sizeof(long long) * (size_t)nchunks + sizeof(Found), sizeof(long long) * scan_scratch((size_t)std::max(nl, nchunks) + 1)};
    size_t at[5];
    FIELD_TRY(g->vox.carve(bytes, at));
    char* const base = g->vox.base;
    double* const d_leaves = (double*)(base + at[0]);
    int* const d_trips = (int*)(base + at[1]);
    long long* const d_first = (long long*)(base + at[2]);
    long long* const d_chunk = (long long*)(base + at[3]);
    long long* const d_scratch = (long long*)(base + at[4]);
    int* const d_box = (int*)(d_chunk + nchunks + 1);
    OctGrid G;
    std::memcpy(G.pose, s.pose, sizeof(G.pose));
    for (int a = 0; a < 3; ++a) { G.origin_minus_res[a] = g->dev.origin_minus_res[a]; G.n[a] = g->n[a]; }
    G.inv_res = g->dev.inv_res; G.res = g->res;
    FIELD_TRY(hipMemcpy(d_leaves, s.vertices.data(), bytes[0], hipMemcpyHostToDevice));
    VoxTimer timer;
    // 1. every leaf's trips, the prefix of the leaves' points, the in-grid points of every chunk and their prefix
    FIELD_TRY(timer.begin());
    hipLaunchKernelGGL(k_oct_trips, dim3((3 * nl + FIELD_BLOCK - 1) / FIELD_BLOCK), dim3(FIELD_BLOCK), 0, 0, (const double*)d_leaves, nl, g->res, d_trips, d_box);
    scan_exclusive(d_first, nl + 1, d_scratch, d_trips);
    hipLaunchKernelGGL(k_oct_points<false>, dim3(nchunks), dim3(FIELD_BLOCK), 0, 0, (const double*)d_leaves, (const int*)d_trips, (const long long*)d_first, nl, G,
                       d_chunk, (int*)nullptr, d_box);
    scan_exclusive(d_chunk, nchunks + 1, d_scratch);
    FIELD_TRY(timer.end());
    FIELD_TRY(hipMemcpy(&found, d_chunk + nchunks, sizeof(found), hipMemcpyDeviceToHost));
    if (found.ncells <= 0) return SMPLX_OK;
    if (found.ncells > bound) return smplx_internal_set_error(SMPLX_E_HIP, "octree: more cells than the bound on the sample points");
    // 2. the list, and with edit its cells as obstacles
    FIELD_TRY(out.d_cells.alloc(3 * (size_t)found.ncells));
    FIELD_TRY(timer.begin());
    hipLaunchKernelGGL(k_oct_points<true>, dim3(nchunks), dim3(FIELD_BLOCK), 0, 0, (const double*)d_leaves, (const int*)d_trips, (const long long*)d_first, nl, G,
                       d_chunk, (int*)out.d_cells, (int*)nullptr);
    if (edit) occ_points(g, out.d_cells, (size_t)found.ncells, 1, true);
    FIELD_TRY(timer.end());
    FIELD_TRY(hipDeviceSynchronize());
    out.first[1] = (int)found.ncells;
    out.box.assign(found.box, found.box + 6);
    return SMPLX_OK;
}

}  // namespace
