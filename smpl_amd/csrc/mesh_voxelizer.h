// smpl_amd/csrc/mesh_voxelizer.h -- the triangle-mesh voxeliser of field.hip: three kernels over the arithmetic of
// voxelize.h, and the driver every lattice shares (the grid's own, world_objects.h; an attached object's,
// object_sphere_rows.h; a link model's HalfRes one, body_place.h).  Reference: smpl/src/geometry/voxelize.cpp:1008-1035
// (VoxelizeMesh over a grid), :962-986 (gridless), include/smpl/geometry/voxelize.hpp:115-176 (candidates and the test).
//
// Work distribution.  The host lists every triangle that has candidate voxels inside the grid (vertex indices and clipped
// range, 36 bytes) and takes the exclusive prefix sum of the clipped candidate-range volumes; k_vox_setup computes each
// listed triangle's constants on the device (the host computing and uploading 240 bytes a triangle cost more than all
// the kernels together).  k_vox_fill gives one thread one (triangle, voxel) pair:
// the block finds the triangle of its first pair by a search over the whole prefix (the same for all its threads), and
// since every listed triangle owns at least one pair, each thread's triangle lies within FIELD_BLOCK entries of it: eight
// more steps.  A filled voxel is a plain byte store of 1 into the shape's mask (all racing stores write the same value).
// The constants of a triangle are read straight from memory: a wavefront inside one large triangle reads one address,
// and small triangles are read once each, so staging them in LDS would move the same bytes.
// k_vox_compact turns the masks into ordered cell lists: chunks of VOX_CHUNK mask bytes, first counted, then -- after an
// exclusive scan of the chunk counts -- written, each wavefront ranking its cells by ballot (vox_common.h block_rank).
// The writing pass also applies the cells to the occupancy bytes (and reference counts) when the call is an edit.
// The call's arrays live in the caller's work space (device_mem.h), so a call allocates only the cell list it returns.
#pragma once

#include <climits>

#include "shape_meshes.h"
#include "vox_common.h"
#include "voxelize.h"

namespace {

#define VOX_ITEMS 8
#define VOX_CHUNK (FIELD_BLOCK * VOX_ITEMS)

// one thread per listed triangle: its constants, from the vertices the host transformed
__global__ void __launch_bounds__(FIELD_BLOCK)
k_vox_setup(const double* __restrict__ verts, const VoxItem* __restrict__ items, int ntri, double res, VoxTri* __restrict__ tris)
{
    const int i = blockIdx.x * FIELD_BLOCK + threadIdx.x;
    if (i >= ntri) return;
    const VoxItem it = items[i];
    VoxTri T;
    T.skip = vox_tri_setup(verts + 3 * (size_t)it.v[0], verts + 3 * (size_t)it.v[1], verts + 3 * (size_t)it.v[2], res, &T) ? 0 : 1;
    for (int a = 0; a < 3; ++a) T.lo[a] = it.lo[a];
    T.ny = it.ny; T.nz = it.nz; T.shape = it.shape;
    tris[i] = T;
}

__global__ void __launch_bounds__(FIELD_BLOCK)
k_vox_fill(const VoxTri* __restrict__ tris, const long long* __restrict__ first, int ntri, const VoxShape* __restrict__ shapes,
           unsigned char* __restrict__ mask, double ox, double oy, double oz, double res)
{
    const long long total = first[ntri];
    for (long long k0 = (long long)blockIdx.x * FIELD_BLOCK; k0 < total; k0 += (long long)gridDim.x * FIELD_BLOCK) {
        int lo = 0, hi = ntri;                         // first[lo] <= k0 < first[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (first[mid] <= k0) lo = mid; else hi = mid;
        }
        const long long k = k0 + threadIdx.x;
        if (k >= total) continue;
        int a = lo, b = lo + FIELD_BLOCK < ntri ? lo + FIELD_BLOCK : ntri;   // first[a] <= k < first[b]
        while (b - a > 1) {
            const int mid = (a + b) >> 1;
            if (first[mid] <= k) a = mid; else b = mid;
        }
        const VoxTri& T = tris[a];
        if (T.skip) continue;
        const long long local = k - first[a];
        const int cz = T.lo[2] + (int)(local % T.nz);
        const int cy = T.lo[1] + (int)(local / T.nz % T.ny);
        const int cx = T.lo[0] + (int)(local / ((long long)T.nz * T.ny));
        const double x[3] = {vox_continuize(cx, ox, res), vox_continuize(cy, oy, res), vox_continuize(cz, oz, res)};
        if (!vox_filled(T, x)) continue;
        const VoxShape& S = shapes[T.shape];
        mask[S.mask_first + ((long long)(cx - S.lo[0]) * S.dim[1] + (cy - S.lo[1])) * S.dim[2] + (cz - S.lo[2])] = 1;
    }
}

// one block per chunk of one shape's mask.  Write == false: chunk_n[chunk] = filled cells of the chunk.  Write == true:
// chunk_n holds the exclusive scan within the shape; the cells go to cells[S.list_first + chunk_n[chunk] + rank], in mask
// order, and -- with occ -- become obstacles (k_occ_points' rule: with counts every listing counts).
template <bool Write>
__global__ void __launch_bounds__(FIELD_BLOCK)
k_vox_compact(const unsigned char* __restrict__ mask, const VoxShape* __restrict__ shapes, int nshapes, int* __restrict__ chunk_n,
              int* __restrict__ cells, unsigned char* __restrict__ occ, int* __restrict__ counts, int ny, int nz)
{
    __shared__ int wave_n[FIELD_BLOCK / 64];
    const int chunk = blockIdx.x;
    int s = 0, hi = nshapes;                           // shapes[s].first_chunk <= chunk < shapes[hi].first_chunk
    while (hi - s > 1) {
        const int mid = (s + hi) >> 1;
        if (shapes[mid].first_chunk <= chunk) s = mid; else hi = mid;
    }
    const VoxShape& S = shapes[s];
    const long long size = (long long)S.dim[0] * S.dim[1] * S.dim[2];
    const long long begin = (long long)(chunk - S.first_chunk) * VOX_CHUNK;
    int base = Write ? chunk_n[chunk] : 0;
    for (int j = 0; j < VOX_ITEMS; ++j) {
        const long long i = begin + (long long)j * FIELD_BLOCK + threadIdx.x;
        const bool on = i < size && mask[S.mask_first + i] != 0;
        const BlockRank r = block_rank(on, wave_n);
        if (Write && on) {
            const int z = S.lo[2] + (int)(i % S.dim[2]);
            const int y = S.lo[1] + (int)(i / S.dim[2] % S.dim[1]);
            const int x = S.lo[0] + (int)(i / ((long long)S.dim[2] * S.dim[1]));
            int* c = cells + 3 * (S.list_first + base + r.before + r.rank);
            c[0] = x; c[1] = y; c[2] = z;
            if (occ) {
                const size_t g = ((size_t)x * ny + y) * nz + z;
                if (!counts) occ[g] = 1;
                else if (atomicAdd(&counts[g], 1) == 0) occ[g] = 1;
            }
        }
        base += r.all;
        __syncthreads();
    }
    if (!Write && threadIdx.x == 0) chunk_n[chunk] = base;
}

// the lattice a call voxelises on: voxel i along axis a is centred on offset[a] + i * res
struct VoxLattice {
    double offset[3];
    double res;
    bool half_res;     // indices by the HalfResDiscretizer (gridless voxel models, body_place.h), else by the
                       // PivotDiscretizer at `offset` (the occupancy grid's own lattice)
};

// voxelises meshes (vertices already in the lattice's frame) on a lattice.  clip: 6 ints per mesh, the inclusive index
// range {lo, hi} its candidates are clipped to.  work: the caller's work space.  With occ the cells also become obstacles
// of a grid whose y and z extents are ny, nz (an edit; the caller updates the field).  Waits for the device.
int voxelize_meshes(WorkSpace& work, const VoxLattice& L, const std::vector<Mesh>& meshes, const std::vector<int>& clip, unsigned char* occ,
                    int* counts, int ny, int nz, VoxLists& out)
{
    const int ns = (int)meshes.size();
    std::vector<VoxItem> items;
    std::vector<double> verts;                         // the call's vertices
    std::vector<long long> first(1, 0);
    std::vector<VoxShape> vs((size_t)ns + 1);
    out.first.assign((size_t)ns + 1, 0);
    out.box.assign((size_t)ns * 6, 0);
    long long mask_bytes = 0, chunks = 0;
    for (int s = 0; s < ns; ++s) {
        const Mesh& m = meshes[(size_t)s];
        const int* cl = &clip[6 * (size_t)s];
        const int v0 = (int)(verts.size() / 3);
        verts.insert(verts.end(), m.v.begin(), m.v.end());
        int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
        bool none = true;
        for (size_t k = 0; k + 2 < m.t.size(); k += 3) {
            const double* p[3] = {&m.v[3 * (size_t)m.t[k]], &m.v[3 * (size_t)m.t[k + 1]], &m.v[3 * (size_t)m.t[k + 2]]};
            // the candidates: worldToGrid of the vertices' minimum and maximum (voxelize.hpp:115-122), clipped
            // (a triangle the reference skips is listed too: k_vox_setup finds that out)
            int tl[3], th[3];
            bool any = true;
            for (int a = 0; a < 3; ++a) {
                const double mn = std::min(p[0][a], std::min(p[1][a], p[2][a])), mx = std::max(p[0][a], std::max(p[1][a], p[2][a]));
                if (L.half_res) {
                    tl[a] = std::max(cl[a], vox_half_discretize(mn, L.res));
                    th[a] = std::min(cl[3 + a], vox_half_discretize(mx, L.res));
                } else {
                    tl[a] = std::max(cl[a], vox_discretize_in(mn, L.offset[a], L.res, cl[a], cl[3 + a]));
                    th[a] = std::min(cl[3 + a], vox_discretize_in(mx, L.offset[a], L.res, cl[a], cl[3 + a]));
                }
                any = any && th[a] >= tl[a];
            }
            if (!any) continue;
            none = false;
            VoxItem it;
            for (int a = 0; a < 3; ++a) { it.v[a] = v0 + m.t[k + a]; it.lo[a] = tl[a]; lo[a] = std::min(lo[a], tl[a]); hi[a] = std::max(hi[a], th[a]); }
            it.ny = th[1] - tl[1] + 1; it.nz = th[2] - tl[2] + 1;
            it.shape = s;
            items.push_back(it);
            first.push_back(first.back() + (long long)(th[0] - tl[0] + 1) * it.ny * it.nz);
        }
        VoxShape& S = vs[(size_t)s];
        S.mask_first = mask_bytes; S.list_first = 0; S.first_chunk = (int)chunks; S.pad = 0;
        for (int a = 0; a < 3; ++a) { S.lo[a] = none ? 0 : lo[a]; S.dim[a] = none ? 0 : hi[a] - lo[a] + 1; }
        for (int a = 0; a < 3; ++a) { out.box[6 * (size_t)s + a] = none ? 0 : lo[a]; out.box[6 * (size_t)s + 3 + a] = none ? -1 : hi[a]; }
        const long long size = (long long)S.dim[0] * S.dim[1] * S.dim[2];
        mask_bytes += size;
        chunks += (size + VOX_CHUNK - 1) / VOX_CHUNK;
        if (chunks > INT_MAX / 2 || items.size() > (size_t)INT_MAX / 2 || verts.size() > (size_t)INT_MAX / 2)
            return smplx_internal_set_error(SMPLX_E_LIMIT, "too many voxels, triangles or vertices in one call");
    }
    vs[(size_t)ns].first_chunk = (int)chunks;          // sentinel of the chunk search
    if (items.empty() || chunks == 0) return SMPLX_OK;  // nothing inside the grid: empty lists
    const int ntri = (int)items.size(), nchunks = (int)chunks;

    const size_t bytes[7] = {sizeof(VoxTri) * items.size(), sizeof(long long) * first.size(), sizeof(VoxShape) * vs.size(),
                             sizeof(int) * (size_t)nchunks, (size_t)mask_bytes, sizeof(VoxItem) * items.size(), sizeof(double) * verts.size()};
    size_t at[7];
    FIELD_TRY(work.carve(bytes, at));
    char* const base = work.base;
    VoxTri* const d_tris = (VoxTri*)(base + at[0]);
    long long* const d_first = (long long*)(base + at[1]);
    VoxShape* const d_shapes = (VoxShape*)(base + at[2]);
    int* const d_chunk = (int*)(base + at[3]);
    unsigned char* const d_mask = (unsigned char*)(base + at[4]);
    VoxItem* const d_items = (VoxItem*)(base + at[5]);
    double* const d_verts = (double*)(base + at[6]);
    FIELD_TRY(hipMemcpy(d_items, items.data(), bytes[5], hipMemcpyHostToDevice));
    FIELD_TRY(hipMemcpy(d_verts, verts.data(), bytes[6], hipMemcpyHostToDevice));
    FIELD_TRY(hipMemcpy(d_first, first.data(), bytes[1], hipMemcpyHostToDevice));
    FIELD_TRY(hipMemcpy(d_shapes, vs.data(), bytes[2], hipMemcpyHostToDevice));
    FIELD_TRY(hipMemset(d_mask, 0, (size_t)mask_bytes));
    VoxTimer timer;
    FIELD_TRY(timer.begin());
    hipLaunchKernelGGL(k_vox_setup, dim3((ntri + FIELD_BLOCK - 1) / FIELD_BLOCK), dim3(FIELD_BLOCK), 0, 0, (const double*)d_verts, (const VoxItem*)d_items, ntri,
                       L.res, d_tris);
    hipLaunchKernelGGL(k_vox_fill, dim3(blocks_of((size_t)first.back())), dim3(FIELD_BLOCK), 0, 0, (const VoxTri*)d_tris, (const long long*)d_first, ntri,
                       (const VoxShape*)d_shapes, d_mask, L.offset[0], L.offset[1], L.offset[2], L.res);
    hipLaunchKernelGGL(k_vox_compact<false>, dim3(nchunks), dim3(FIELD_BLOCK), 0, 0, (const unsigned char*)d_mask, (const VoxShape*)d_shapes, ns, d_chunk,
                       (int*)nullptr, (unsigned char*)nullptr, (int*)nullptr, ny, nz);
    FIELD_TRY(timer.end());
    std::vector<int> chunk_n((size_t)nchunks);
    FIELD_TRY(hipMemcpy(chunk_n.data(), d_chunk, bytes[3], hipMemcpyDeviceToHost));
    // exclusive scan of the chunk counts within every shape; the shapes' lists lie back to back
    long long total = 0;
    for (int s = 0; s < ns; ++s) {
        vs[(size_t)s].list_first = total;
        long long run = 0;
        for (int c = vs[(size_t)s].first_chunk; c < vs[(size_t)s + 1].first_chunk; ++c) { const int n = chunk_n[(size_t)c]; chunk_n[(size_t)c] = (int)run; run += n; }
        total += run;
        if (total > INT_MAX / 3) return smplx_internal_set_error(SMPLX_E_LIMIT, "too many cells in one call");
        out.first[(size_t)s + 1] = (int)total;
    }
    if (total == 0) return SMPLX_OK;
    FIELD_TRY(hipMemcpy(d_chunk, chunk_n.data(), bytes[3], hipMemcpyHostToDevice));
    FIELD_TRY(hipMemcpy(d_shapes, vs.data(), bytes[2], hipMemcpyHostToDevice));
    FIELD_TRY(out.d_cells.alloc(3 * (size_t)total));
    FIELD_TRY(timer.begin());
    hipLaunchKernelGGL(k_vox_compact<true>, dim3(nchunks), dim3(FIELD_BLOCK), 0, 0, (const unsigned char*)d_mask, (const VoxShape*)d_shapes, ns, d_chunk,
                       (int*)out.d_cells, occ, counts, ny, nz);
    FIELD_TRY(timer.end());
    FIELD_TRY(hipDeviceSynchronize());
    return SMPLX_OK;
}

}  // namespace
