// smpl_amd/csrc/world_objects.h -- world objects on a grid (include/smpl_amd.h "world objects"), the tail of field.hip:
// shapes to meshes on the host, the voxeliser's three kernels, and the registry edits.  Reference:
// sbpl_collision_checking/src/world_collision_model.cpp:193-280, src/voxel_operations.cpp:319-402,
// smpl/src/geometry/mesh_utils.cpp:39-299, smpl/src/geometry/voxelize.cpp:608-615, 1008-1035.
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
// exclusive scan of the chunk counts -- written, each wavefront ranking its cells by ballot.  The writing pass also
// applies the cells to the occupancy bytes (and reference counts) when the call is an edit.
// The call's arrays live in one work space kept on the grid (smplx_grid::d_vox) that only grows: device allocations cost
// more than the kernels (tools/voxelize_time.py), so a call makes one only for the cell list an object keeps.
// k_vox_spheres turns a compacted list into the sphere rows of an attached object's model (object_spheres.h): one thread
// per cell; those calls use a work space kept on the space (AttachedBodies::d_vox) in the same way.
//
// Octrees (SMPLX_SHAPE_OCTREE; voxel_operations.cpp:405-436, arithmetic in octree_points.h) are no meshes: a leaf is
// sampled at points, every point becomes a cell, and the list keeps them in generation order with duplicates.  Only the
// leaf rows (32 bytes each) cross to the device.  k_oct_trips gives every (leaf, axis) the trips of its loop; their
// products are scanned on the device (k_scan_tiles / k_scan_add, level by level); k_oct_points gives one thread one
// sample point and compacts the in-grid cells in order the way k_vox_compact does -- chunk counts first, then, after the
// device scan of the counts, the write -- recomputing the point in the second pass instead of storing it.  The list is
// then added with k_occ_points.  The host reads back 32 bytes: the number of cells (to allocate the list) and the
// list's bounding range (for the edit window).
#pragma once

#include <climits>

#include "object_spheres.h"
#include "octree_points.h"
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = Write ? chunk_n[chunk] : 0;
    for (int j = 0; j < VOX_ITEMS; ++j) {
        const long long i = begin + (long long)j * FIELD_BLOCK + threadIdx.x;
        const bool on = i < size && mask[S.mask_first + i] != 0;
        const unsigned long long b = __ballot(on);
        if (lane == 0) wave_n[wave] = __popcll(b);
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < FIELD_BLOCK / 64; ++w) { before += w < wave ? wave_n[w] : 0; all += wave_n[w]; }
        if (Write && on) {
            const int z = S.lo[2] + (int)(i % S.dim[2]);
            const int y = S.lo[1] + (int)(i / S.dim[2] % S.dim[1]);
            const int x = S.lo[0] + (int)(i / ((long long)S.dim[2] * S.dim[1]));
            int* c = cells + 3 * (S.list_first + base + before + __popcll(b & ((1ull << lane) - 1ull)));
            c[0] = x; c[1] = y; c[2] = z;
            if (occ) {
                const size_t g = ((size_t)x * ny + y) * nz + z;
                if (!counts) occ[g] = 1;
                else if (atomicAdd(&counts[g], 1) == 0) occ[g] = 1;
            }
        }
        base += all;
        __syncthreads();
    }
    if (!Write && threadIdx.x == 0) chunk_n[chunk] = base;
}

// one thread per cell of a compacted list: the sphere an attached object's model has at that voxel (object_spheres.h),
// a 32-byte row {x, y, z, r}
__global__ void __launch_bounds__(FIELD_BLOCK)
k_vox_spheres(const int* __restrict__ cells, int n, double res, double radius, double* __restrict__ rows)
{
    const int i = blockIdx.x * FIELD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int c[3] = {cells[3 * (size_t)i], cells[3 * (size_t)i + 1], cells[3 * (size_t)i + 2]};
    double r[4];
    smplx_object_host::sphere_row(c, res, radius, r);
    double* out = rows + 4 * (size_t)i;
    out[0] = r[0]; out[1] = r[1]; out[2] = r[2]; out[3] = r[3];
}

// ---- octrees (octree_points.h): the sample points of the leaves, mapped to cells, in generation order, duplicates kept

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

// exclusive scan, in place, of every tile of FIELD_BLOCK entries of v; sums[tile] = the tile's total.  With trips the
// entries are not read but made: entry i < n - 1 is the points of leaf i, the product of its trips, and entry n - 1 is 0
// (the scan turns it into the total).
__global__ void __launch_bounds__(FIELD_BLOCK)
k_scan_tiles(long long* __restrict__ v, int n, long long* __restrict__ sums, const int* __restrict__ trips)
{
    __shared__ long long s[2][FIELD_BLOCK];
    const int i = blockIdx.x * FIELD_BLOCK + threadIdx.x;
    long long own = 0;
    if (trips) { if (i < n - 1) own = (long long)trips[3 * (size_t)i] * trips[3 * (size_t)i + 1] * trips[3 * (size_t)i + 2]; }
    else if (i < n) own = v[i];
    int cur = 0;
    s[0][threadIdx.x] = own;
    __syncthreads();
    for (int d = 1; d < FIELD_BLOCK; d <<= 1) {          // Hillis-Steele: after the step with d, s holds sums of 2d entries
        s[cur ^ 1][threadIdx.x] = s[cur][threadIdx.x] + ((int)threadIdx.x >= d ? s[cur][threadIdx.x - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    if (i < n) v[i] = s[cur][threadIdx.x] - own;
    if (threadIdx.x == FIELD_BLOCK - 1) sums[blockIdx.x] = s[cur][threadIdx.x];
}

// adds the scanned tile totals back: v[i] += sums[tile of i]
__global__ void __launch_bounds__(FIELD_BLOCK)
k_scan_add(long long* __restrict__ v, int n, const long long* __restrict__ sums)
{
    const int i = blockIdx.x * FIELD_BLOCK + threadIdx.x;
    if (i < n) v[i] += sums[blockIdx.x];
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
// holds the exclusive scan; the cells go to cells[chunk_n[chunk] + rank], in generation order (each wavefront ranks its
// cells by ballot).
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
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
    const unsigned long long b = __ballot(on);
    if (lane == 0) wave_n[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < FIELD_BLOCK / 64; ++w) { before += w < wave ? wave_n[w] : 0; all += wave_n[w]; }
    if (Write) {
        if (on) {
            int* out = cells + 3 * (size_t)(chunk_n[blockIdx.x] + before + __popcll(b & ((1ull << lane) - 1ull)));
            out[0] = c[0]; out[1] = c[1]; out[2] = c[2];
        }
        return;
    }
    if (on)
        for (int a = 0; a < 3; ++a) { atomicMin(&sbox[a], c[a]); atomicMax(&sbox[3 + a], c[a]); }
    __syncthreads();
    if (threadIdx.x == 0) chunk_n[blockIdx.x] = all;
    if (threadIdx.x < 6) {
        if (threadIdx.x < 3) atomicMin(&box[threadIdx.x], sbox[threadIdx.x]); else atomicMax(&box[threadIdx.x], sbox[threadIdx.x]);
    }
}

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1); }
};

struct Mesh { std::vector<double> v; std::vector<int> t; };

// CreateIndexedBoxMesh (mesh_utils.cpp:39-112)
void box_mesh(double length, double width, double height, Mesh& m)
{
    const double x = 0.5 * length, y = 0.5 * width, z = 0.5 * height;
    m.v = {-x, -y, -z, x, -y, -z, -x, y, -z, x, y, -z, -x, -y, z, x, -y, z, -x, y, z, x, y, z};
    m.t = {0, 2, 1, 1, 2, 3, 5, 1, 7, 1, 3, 7, 5, 7, 4, 4, 7, 6, 4, 6, 0, 0, 6, 2, 6, 7, 2, 7, 3, 2, 5, 0, 1, 4, 5, 0};
}

// CreateIndexedSphereMesh (mesh_utils.cpp:116-204)
void sphere_mesh(double radius, int lon, int lat, Mesh& m)
{
    m.v = {0.0, 0.0, radius};
    const double theta_inc = SMPLX_PI / (lat + 1), phi_inc = (2.0 * SMPLX_PI) / lon;
    for (int ti = 0; ti < lat; ++ti)
        for (int pi = 0; pi < lon; ++pi) {
            const double theta = (ti + 1) * theta_inc, phi = pi * phi_inc;
            m.v.push_back(radius * std::sin(theta) * std::cos(phi));
            m.v.push_back(radius * std::sin(theta) * std::sin(phi));
            m.v.push_back(radius * std::cos(theta));
        }
    m.v.insert(m.v.end(), {0.0, 0.0, -radius});
    const int nv = (int)(m.v.size() / 3);
    for (int i = 0; i < lon; ++i) m.t.insert(m.t.end(), {0, i + 1, i == lon - 1 ? 1 : i + 2});
    for (int i = 0; i < lat - 1; ++i)
        for (int j = 0; j < lon; ++j) {
            const int base = i * lon + j + 1, b = base + lon;
            int br = b + 1, r = base + 1;
            if ((br - 1) / lon != (b - 1) / lon) br -= lon;
            if ((r - 1) / lon != (base - 1) / lon) r -= lon;
            m.t.insert(m.t.end(), {base, b, br, base, br, r});
        }
    for (int i = 0; i < lon; ++i) m.t.insert(m.t.end(), {nv - 1, i == 0 ? nv - 1 - lon : nv - 1 - i, nv - 1 - (i + 1)});
}

// CreateIndexedCylinderMesh (mesh_utils.cpp:208-264)
void cylinder_mesh(double radius, double length, Mesh& m)
{
    const int rim = 16;
    for (int cap = 0; cap < 2; ++cap)
        for (int i = 0; i < rim; ++i) {
            const double theta = 2.0 * SMPLX_PI * (double)i / double(rim);
            m.v.insert(m.v.end(), {radius * std::cos(theta), radius * std::sin(theta), cap == 0 ? 0.5 * length : -0.5 * length});
        }
    m.v.insert(m.v.end(), {0.0, 0.0, 0.5 * length, 0.0, 0.0, -0.5 * length});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {i, (i + 1) % rim, i + rim, (i + 1) % rim, (i + 1) % rim + rim, i + rim});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {2 * rim, (i + 1) % rim, i});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {2 * rim + 1, (i + 1) % rim + rim, i + rim});
}

// CreateIndexedConeMesh (mesh_utils.cpp:268-299)
void cone_mesh(double radius, double height, Mesh& m)
{
    const int rim = 16;
    for (int i = 0; i < rim; ++i) {
        const double theta = 2.0 * SMPLX_PI * (double)i / (double)rim;
        m.v.insert(m.v.end(), {radius * std::cos(theta), radius * std::sin(theta), -0.5 * height});
    }
    m.v.insert(m.v.end(), {0.0, 0.0, 0.5 * height, 0.0, 0.0, -0.5 * height});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {i, (i + 1) % rim, rim});
    for (int i = 0; i < rim; ++i) m.t.insert(m.t.end(), {i, (i + 1) % rim, rim + 1});
}

void shape_mesh(const WorldShape& s, Mesh& m)
{
    m.v.clear(); m.t.clear();
    switch (s.type) {
    case SMPLX_SHAPE_BOX: box_mesh(s.dims[0], s.dims[1], s.dims[2], m); break;
    case SMPLX_SHAPE_SPHERE: sphere_mesh(s.dims[0], 7, 8, m); break;            // voxelize.cpp:741-756
    case SMPLX_SHAPE_CYLINDER: cylinder_mesh(s.dims[0], s.dims[1], m); break;
    case SMPLX_SHAPE_CONE: cone_mesh(s.dims[0], s.dims[1], m); break;
    default: m.v = s.vertices; m.t.assign(s.triangles.begin(), s.triangles.end()); break;
    }
    // TransformVertices (voxelize.cpp:608-615): R v + t
    for (size_t i = 0; i + 2 < m.v.size(); i += 3) {
        const double v[3] = {m.v[i], m.v[i + 1], m.v[i + 2]};
        vox_transform(s.pose, v, &m.v[i]);
    }
}

// checks the caller's shapes and copies them (mesh arrays included)
int take_shapes(const smplx_shape* shapes, int n, std::vector<WorldShape>& out)
{
    if (!shapes || n < 1) return smplx_internal_set_error(SMPLX_E_ARG, "an object needs at least one shape");
    out.resize((size_t)n);
    for (int i = 0; i < n; ++i) {
        const smplx_shape& s = shapes[i];
        WorldShape& w = out[(size_t)i];
        w.type = s.type;
        int nd = 0;
        switch (s.type) {
        case SMPLX_SHAPE_BOX: nd = 3; break;
        case SMPLX_SHAPE_SPHERE: nd = 1; break;
        case SMPLX_SHAPE_CYLINDER: case SMPLX_SHAPE_CONE: nd = 2; break;
        case SMPLX_SHAPE_MESH: case SMPLX_SHAPE_OCTREE: nd = 0; break;
        default: return smplx_internal_set_error(SMPLX_E_ARG, "unknown shape type (planes are not supported)");
        }
        for (int k = 0; k < 3; ++k) w.dims[k] = k < nd ? s.dims[k] : 0.0;
        if (!finite_coords(w.dims, 3) || !finite_coords(s.pose, 12)) return smplx_internal_set_error(SMPLX_E_ARG, "shape dimensions and pose must be finite (|x| < 1e6)");
        for (int k = 0; k < nd; ++k)
            if (!(w.dims[k] > 0.0)) return smplx_internal_set_error(SMPLX_E_ARG, "shape dimensions must be positive");
        std::memcpy(w.pose, s.pose, sizeof(w.pose));
        if (s.type == SMPLX_SHAPE_OCTREE) {
            if (!s.vertices || s.nvertices < 1 || s.triangles || s.ntriangles != 0)
                return smplx_internal_set_error(SMPLX_E_ARG, "an octree needs leaves (vertices: rows of cx cy cz size) and takes no triangles");
            if (!finite_coords(s.vertices, (size_t)s.nvertices * 4)) return smplx_internal_set_error(SMPLX_E_ARG, "octree leaves must be finite (|x| < 1e6)");
            for (size_t k = 0; k < (size_t)s.nvertices; ++k)
                if (!(s.vertices[4 * k + 3] > 0.0)) return smplx_internal_set_error(SMPLX_E_ARG, "the size of an octree leaf must be positive");
            w.vertices.assign(s.vertices, s.vertices + (size_t)s.nvertices * 4);
            continue;
        }
        if (s.type != SMPLX_SHAPE_MESH) continue;
        if (!s.vertices || !s.triangles || s.nvertices < 1 || s.ntriangles < 1) return smplx_internal_set_error(SMPLX_E_ARG, "a mesh needs vertices and triangles");
        if (!finite_coords(s.vertices, (size_t)s.nvertices * 3)) return smplx_internal_set_error(SMPLX_E_ARG, "mesh vertices must be finite (|x| < 1e6)");
        for (size_t k = 0; k < (size_t)s.ntriangles * 3; ++k)
            if (s.triangles[k] < 0 || s.triangles[k] >= s.nvertices) return smplx_internal_set_error(SMPLX_E_ARG, "triangle index outside the vertices");
        w.vertices.assign(s.vertices, s.vertices + (size_t)s.nvertices * 3);
        w.triangles.assign(s.triangles, s.triangles + (size_t)s.ntriangles * 3);
    }
    return SMPLX_OK;
}

bool good_id(const char* id) { return id && *id && !std::strchr(id, '\n'); }

int find_object(const smplx_grid* g, const char* id)
{
    for (size_t i = 0; i < g->objects.size(); ++i)
        if (g->objects[i].id == id) return (int)i;
    return -1;
}

// test hook (tools/voxelize_time.py): when on, voxelize_run brackets its launches with events
bool g_vox_timing = false;
double g_vox_kernel_ms = 0.0;

struct VoxLists {
    int32_t* d_cells = nullptr;       // owned by the caller after a successful run
    std::vector<int> first, box;      // as in WorldObject
};

// the lattice a call voxelises on: voxel i along axis a is centred on offset[a] + i * res
struct VoxLattice {
    double offset[3];
    double res;
    bool half_res;     // indices by the HalfResDiscretizer (gridless voxel models, body_place.h), else by the
                       // PivotDiscretizer at `offset` (the occupancy grid's own lattice)
};

// voxelises meshes (vertices already in the lattice's frame) on a lattice.  clip: 6 ints per mesh, the inclusive index
// range {lo, hi} its candidates are clipped to.  work / work_bytes: the caller's work space, grown on demand.  With occ
// the cells also become obstacles of a grid whose y and z extents are ny, nz (an edit; the caller updates the field).
// Waits for the device.
int voxelize_meshes(void** work, size_t* work_bytes, const VoxLattice& L, const std::vector<Mesh>& meshes, const std::vector<int>& clip,
                    unsigned char* occ, int* counts, int ny, int nz, VoxLists& out)
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

    // one work space on the grid for the call's seven arrays, each on a 256-byte boundary
    const size_t bytes[7] = {sizeof(VoxTri) * items.size(), sizeof(long long) * first.size(), sizeof(VoxShape) * vs.size(),
                             sizeof(int) * (size_t)nchunks, (size_t)mask_bytes, sizeof(VoxItem) * items.size(), sizeof(double) * verts.size()};
    size_t at[7], need = 0;
    for (int i = 0; i < 7; ++i) { at[i] = need; need += (bytes[i] + 255) & ~(size_t)255; }
    if (need > *work_bytes) {
        if (*work) (void)hipFree(*work);
        *work = nullptr; *work_bytes = 0;
        FIELD_TRY(hipMalloc(work, need));
        *work_bytes = need;
    }
    char* const base = (char*)*work;
    struct { void* p; } d_tris{base + at[0]}, d_first{base + at[1]}, d_shapes{base + at[2]}, d_chunk{base + at[3]}, d_mask{base + at[4]},
        d_items{base + at[5]}, d_verts{base + at[6]};
    FIELD_TRY(hipMemcpy(d_items.p, items.data(), bytes[5], hipMemcpyHostToDevice));
    FIELD_TRY(hipMemcpy(d_verts.p, verts.data(), bytes[6], hipMemcpyHostToDevice));
    FIELD_TRY(hipMemcpy(d_first.p, first.data(), bytes[1], hipMemcpyHostToDevice));
    FIELD_TRY(hipMemcpy(d_shapes.p, vs.data(), bytes[2], hipMemcpyHostToDevice));
    FIELD_TRY(hipMemset(d_mask.p, 0, (size_t)mask_bytes));
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    if (g_vox_timing) { for (hipEvent_t& e : ev) FIELD_TRY(hipEventCreate(&e)); FIELD_TRY(hipEventRecord(ev[0], 0)); }
    struct EvFree { hipEvent_t* e; ~EvFree() { for (int i = 0; i < 4; ++i) if (e[i]) (void)hipEventDestroy(e[i]); } } ev_free{ev};
    hipLaunchKernelGGL(k_vox_setup, dim3((ntri + FIELD_BLOCK - 1) / FIELD_BLOCK), dim3(FIELD_BLOCK), 0, 0, (const double*)d_verts.p, (const VoxItem*)d_items.p,
                       ntri, L.res, (VoxTri*)d_tris.p);
    hipLaunchKernelGGL(k_vox_fill, dim3(blocks_of((size_t)first.back())), dim3(FIELD_BLOCK), 0, 0, (const VoxTri*)d_tris.p, (const long long*)d_first.p,
                       ntri, (const VoxShape*)d_shapes.p, (unsigned char*)d_mask.p, L.offset[0], L.offset[1], L.offset[2], L.res);
    hipLaunchKernelGGL(k_vox_compact<false>, dim3(nchunks), dim3(FIELD_BLOCK), 0, 0, (const unsigned char*)d_mask.p, (const VoxShape*)d_shapes.p, ns,
                       (int*)d_chunk.p, (int*)nullptr, (unsigned char*)nullptr, (int*)nullptr, ny, nz);
    FIELD_TRY(hipGetLastError());
    if (g_vox_timing) FIELD_TRY(hipEventRecord(ev[1], 0));
    std::vector<int> chunk_n((size_t)nchunks);
    FIELD_TRY(hipMemcpy(chunk_n.data(), d_chunk.p, sizeof(int) * (size_t)nchunks, hipMemcpyDeviceToHost));
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
    FIELD_TRY(hipMemcpy(d_chunk.p, chunk_n.data(), sizeof(int) * (size_t)nchunks, hipMemcpyHostToDevice));
    FIELD_TRY(hipMemcpy(d_shapes.p, vs.data(), sizeof(VoxShape) * vs.size(), hipMemcpyHostToDevice));
    DevBuf d_cells;
    FIELD_TRY(d_cells.alloc(sizeof(int32_t) * 3 * (size_t)total));
    if (g_vox_timing) FIELD_TRY(hipEventRecord(ev[2], 0));
    hipLaunchKernelGGL(k_vox_compact<true>, dim3(nchunks), dim3(FIELD_BLOCK), 0, 0, (const unsigned char*)d_mask.p, (const VoxShape*)d_shapes.p, ns,
                       (int*)d_chunk.p, (int*)d_cells.p, occ, counts, ny, nz);
    FIELD_TRY(hipGetLastError());
    if (g_vox_timing) FIELD_TRY(hipEventRecord(ev[3], 0));
    FIELD_TRY(hipDeviceSynchronize());
    if (g_vox_timing) {
        float a = 0.f, b = 0.f;
        FIELD_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
        FIELD_TRY(hipEventElapsedTime(&b, ev[2], ev[3]));
        g_vox_kernel_ms += (double)a + (double)b;
    }
    out.d_cells = (int32_t*)d_cells.p;
    d_cells.p = nullptr;
    return SMPLX_OK;
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

// entries of scratch an exclusive scan of n entries needs: the tile totals of every level
size_t scan_scratch(size_t n)
{
    size_t total = 0;
    do { n = (n + FIELD_BLOCK - 1) / FIELD_BLOCK; total += n; } while (n > 1);
    return total;
}

// exclusive scan of v[0 .. n) in place on the device: tiles of FIELD_BLOCK, their totals scanned the same way, added back.
// With trips, v is first filled with the leaves' points (k_scan_tiles).
void scan_exclusive(long long* v, int n, long long* scratch, const int* trips = nullptr)
{
    const int tiles = (n + FIELD_BLOCK - 1) / FIELD_BLOCK;
    hipLaunchKernelGGL(k_scan_tiles, dim3(tiles), dim3(FIELD_BLOCK), 0, 0, v, n, scratch, trips);
    if (tiles == 1) return;
    scan_exclusive(scratch, tiles, scratch + tiles);
    hipLaunchKernelGGL(k_scan_add, dim3(tiles), dim3(FIELD_BLOCK), 0, 0, v, n, (const long long*)scratch);
}

// with the test hook on, the time between begin() and end() is added to g_vox_kernel_ms; end() also reports launch errors
struct VoxTimer {
    hipEvent_t a = nullptr, b = nullptr;
    ~VoxTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    hipError_t begin()
    {
        if (!g_vox_timing) return hipSuccess;
        if (!a) { if (hipError_t e = hipEventCreate(&a)) return e; if (hipError_t e = hipEventCreate(&b)) return e; }
        return hipEventRecord(a, 0);
    }
    hipError_t end()
    {
        if (hipError_t e = hipGetLastError()) return e;
        if (!g_vox_timing) return hipSuccess;
        if (hipError_t e = hipEventRecord(b, 0)) return e;
        if (hipError_t e = hipEventSynchronize(b)) return e;
        float ms = 0.f;
        if (hipError_t e = hipEventElapsedTime(&ms, a, b)) return e;
        g_vox_kernel_ms += (double)ms;
        return hipSuccess;
    }
};

struct OctList {
    int32_t* d_cells = nullptr;       // owned by the caller after a successful run
    int n = 0;
    int box[6] = {0, 0, 0, -1, -1, -1};
};

// the cell list of one octree shape (VoxelizeOcTree, voxel_operations.cpp:405-436, then worldToGrid): the cells of its
// sample points that lie inside the grid, in generation order, duplicates kept.  The leaves' trips, the prefix of their
// point counts and the chunk counts of the compaction live in the grid's work space; the only allocation is the list.
// One upload (the leaf rows) and one download (the number of cells and their bounding range, 32 bytes): the number of
// sample points stays on the device, the chunks being launched for their bound.  With occ the cells also become
// obstacles through k_occ_points (the caller updates the field).  Waits for the device.
int octree_run(const smplx_grid* g, const WorldShape& s, unsigned char* occ, int* counts, OctList& out)
{
    const int nl = (int)(s.vertices.size() / 4);
    long long bound = 0;                               // octree_limits has held it to OCT_MAX_POINTS
    for (size_t k = 3; k < s.vertices.size(); k += 4) { const long long b = oct_axis_bound(s.vertices[k], g->res); bound += b * b * b; }
    const int nchunks = (int)((bound + OCT_CHUNK - 1) / OCT_CHUNK);
    struct Found { long long ncells; int box[6]; } found;      // as they lie behind the chunk counts
    const size_t bytes[5] = {sizeof(double) * 4 * (size_t)nl, sizeof(int) * 3 * (size_t)nl, sizeof(long long) * ((size_t)nl + 1),
                             sizeof(long long) * (size_t)nchunks + sizeof(Found), sizeof(long long) * scan_scratch((size_t)std::max(nl, nchunks) + 1)};
    size_t at[5], need = 0;
    for (int i = 0; i < 5; ++i) { at[i] = need; need += (bytes[i] + 255) & ~(size_t)255; }
    if (need > g->vox_bytes) {
        if (g->d_vox) (void)hipFree(g->d_vox);
        g->d_vox = nullptr; g->vox_bytes = 0;
        FIELD_TRY(hipMalloc(&g->d_vox, need));
        g->vox_bytes = need;
    }
    char* const base = (char*)g->d_vox;
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
    // 2. the list, and with occ its cells as obstacles
    DevBuf d_cells;
    FIELD_TRY(d_cells.alloc(sizeof(int32_t) * 3 * (size_t)found.ncells));
    FIELD_TRY(timer.begin());
    hipLaunchKernelGGL(k_oct_points<true>, dim3(nchunks), dim3(FIELD_BLOCK), 0, 0, (const double*)d_leaves, (const int*)d_trips, (const long long*)d_first, nl, G,
                       d_chunk, (int*)d_cells.p, (int*)nullptr);
    if (occ)
        hipLaunchKernelGGL(k_occ_points, dim3((unsigned)((found.ncells + FIELD_BLOCK - 1) / FIELD_BLOCK)), dim3(FIELD_BLOCK), 0, 0, occ, counts, g->n[0], g->n[1],
                           g->n[2], (const int*)d_cells.p, (int)found.ncells, 1);
    FIELD_TRY(timer.end());
    FIELD_TRY(hipDeviceSynchronize());
    out.n = (int)found.ncells;
    std::copy(found.box, found.box + 6, out.box);
    out.d_cells = (int32_t*)d_cells.p;
    d_cells.p = nullptr;
    return SMPLX_OK;
}

// voxelises the shapes on the grid's lattice: the pivot is the grid's origin and the candidates are clipped to the grid.
// Meshes and the shapes that become meshes go through voxelize_meshes together, every octree through octree_run; with
// both kinds in one call the lists are then laid back to back in shape order.  With occ the cells also become obstacles
// (an edit; the caller updates the field).  Waits for the device.
int voxelize_run(const smplx_grid* g, const std::vector<WorldShape>& shapes, unsigned char* occ, int* counts, VoxLists& out)
{
    const size_t ns = shapes.size();
    std::vector<Mesh> meshes;
    std::vector<int> clip;
    for (size_t s = 0; s < ns; ++s) {
        if (shapes[s].type == SMPLX_SHAPE_OCTREE) continue;
        meshes.emplace_back();
        shape_mesh(shapes[s], meshes.back());
        clip.insert(clip.end(), {0, 0, 0, g->n[0] - 1, g->n[1] - 1, g->n[2] - 1});
    }
    const VoxLattice L{{g->origin[0], g->origin[1], g->origin[2]}, g->res, false};
    g_vox_kernel_ms = 0.0;
    if (meshes.size() == ns) return voxelize_meshes(&g->d_vox, &g->vox_bytes, L, meshes, clip, occ, counts, g->n[1], g->n[2], out);
    if (int e = octree_limits(shapes, g->res)) return e;
    VoxLists part;
    DevBuf mesh_cells;
    if (!meshes.empty()) {
        if (int e = voxelize_meshes(&g->d_vox, &g->vox_bytes, L, meshes, clip, occ, counts, g->n[1], g->n[2], part)) return e;
        mesh_cells.p = part.d_cells;
    }
    std::vector<OctList> octs(ns);
    std::vector<DevBuf> oct_cells(ns);
    out.first.assign(ns + 1, 0);
    out.box.assign(ns * 6, 0);
    long long total = 0;
    for (size_t s = 0, m = 0; s < ns; ++s) {
        int n = 0;
        if (shapes[s].type == SMPLX_SHAPE_OCTREE) {
            if (int e = octree_run(g, shapes[s], occ, counts, octs[s])) return e;
            oct_cells[s].p = octs[s].d_cells;
            n = octs[s].n;
            std::copy(octs[s].box, octs[s].box + 6, &out.box[6 * s]);
        } else {
            n = part.first[m + 1] - part.first[m];
            std::copy(&part.box[6 * m], &part.box[6 * m] + 6, &out.box[6 * s]);
            ++m;
        }
        total += n;
        if (total > INT_MAX / 3) return smplx_internal_set_error(SMPLX_E_LIMIT, "too many cells in one call");
        out.first[s + 1] = (int)total;
    }
    if (total == 0) return SMPLX_OK;
    if (ns == 1) {                                     // one octree: its list is the call's
        out.d_cells = octs[0].d_cells;
        oct_cells[0].p = nullptr;
        return SMPLX_OK;
    }
    DevBuf d_cells;
    FIELD_TRY(d_cells.alloc(sizeof(int32_t) * 3 * (size_t)total));
    for (size_t s = 0, m = 0; s < ns; ++s) {
        const bool oct = shapes[s].type == SMPLX_SHAPE_OCTREE;
        const int32_t* from = oct ? octs[s].d_cells : part.d_cells + 3 * (size_t)part.first[m];
        const int n = out.first[s + 1] - out.first[s];
        if (!oct) ++m;
        if (n > 0) FIELD_TRY(hipMemcpy((int32_t*)d_cells.p + 3 * (size_t)out.first[s], from, sizeof(int32_t) * 3 * (size_t)n, hipMemcpyDeviceToDevice));
    }
    out.d_cells = (int32_t*)d_cells.p;
    d_cells.p = nullptr;
    return SMPLX_OK;
}

// the sphere model of an attached object (generateSpheresModel, attached_bodies_collision_model.cpp:264-313): every
// shape's surface voxelised on the lattice of object_spheres.h -- pivot 0, resolution radius / sqrt(2), candidates clipped
// to the index range of the shape's own bounding box, negative indices kept -- and one row {x, y, z, radius} per filled
// voxel, the shapes' lists back to back (a voxel two shapes fill gives two rows).  work / work_bytes: the caller's work
// space; it holds the voxeliser's arrays and then the rows, which are copied back once.  Waits for the device.
int object_spheres_run(void** work, size_t* work_bytes, const std::vector<WorldShape>& shapes, double radius, std::vector<double>& rows,
                       std::vector<int32_t>& first)
{
    const double res = smplx_object_host::resolution(radius);
    std::vector<Mesh> meshes(shapes.size());
    std::vector<int> clip(6 * shapes.size());
    long long cells = 0;
    for (size_t s = 0; s < shapes.size(); ++s) {
        shape_mesh(shapes[s], meshes[s]);
        smplx_object_host::clip_range(meshes[s].v.data(), meshes[s].v.size() / 3, res, &clip[6 * s]);
        cells += smplx_object_host::range_cells(&clip[6 * s]);
        if (cells > smplx_object_host::kMaxRangeCells)
            return smplx_internal_set_error(SMPLX_E_LIMIT, "the shapes' bounding boxes hold more than 2^28 voxels at this radius");
    }
    const VoxLattice L{{0.0, 0.0, 0.0}, res, false};
    VoxLists lists;
    g_vox_kernel_ms = 0.0;
    if (int e = voxelize_meshes(work, work_bytes, L, meshes, clip, nullptr, nullptr, 0, 0, lists)) return e;
    DevBuf d_cells;
    d_cells.p = lists.d_cells;
    first.assign(lists.first.begin(), lists.first.end());
    const int total = lists.first.back();
    rows.assign(4 * (size_t)total, 0.0);
    if (total == 0) return SMPLX_OK;
    const size_t need = sizeof(double) * 4 * (size_t)total;
    if (need > *work_bytes) {          // the voxeliser's arrays are done with: the rows may take a new block
        if (*work) (void)hipFree(*work);
        *work = nullptr; *work_bytes = 0;
        FIELD_TRY(hipMalloc(work, need));
        *work_bytes = need;
    }
    hipLaunchKernelGGL(k_vox_spheres, dim3((total + FIELD_BLOCK - 1) / FIELD_BLOCK), dim3(FIELD_BLOCK), 0, 0, (const int*)d_cells.p, total, res, radius,
                       (double*)*work);
    FIELD_TRY(hipGetLastError());
    FIELD_TRY(hipMemcpy(rows.data(), *work, need, hipMemcpyDeviceToHost));
    return SMPLX_OK;
}

// takes the stored lists of an object out of the occupancy (removePointsFromField per shape, world_collision_model.cpp:
// 254-257) and grows `box` by the ranges they lie in; the caller updates the field
void remove_lists(smplx_grid* g, const WorldObject& o, Window& box)
{
    int* counts = g->ref_counted ? g->d_counts : nullptr;
    for (size_t s = 0; s + 1 < o.first.size(); ++s) {
        const int n = o.first[s + 1] - o.first[s];
        if (n <= 0) continue;
        // one thread per cell: an octree's list can hold more cells than blocks_of() gives threads
        hipLaunchKernelGGL(k_occ_points, dim3((unsigned)(((size_t)n + FIELD_BLOCK - 1) / FIELD_BLOCK)), dim3(FIELD_BLOCK), 0, 0, g->d_occ, counts, g->n[0], g->n[1],
                           g->n[2], (const int*)(o.d_cells + 3 * (size_t)o.first[s]), n, 0);
        const int* b = &o.box[6 * s];
        box.x0 = std::min(box.x0, b[0]); box.y0 = std::min(box.y0, b[1]); box.z0 = std::min(box.z0, b[2]);
        box.x1 = std::max(box.x1, b[3]); box.y1 = std::max(box.y1, b[4]); box.z1 = std::max(box.z1, b[5]);
    }
}

const char* const kNotEditable = "the grid was created from a finished field (smplx_grid_create), not on the GPU";

// insert (old < 0) or move: remove the old lists, voxelise and add the new ones, update the field once
int put_object(smplx_grid* g, const char* id, int old, std::vector<WorldShape>& shapes)
{
    if (int e = octree_limits(shapes, g->res)) return e;      // before the old lists go: a refused call changes nothing
    Window box{1 << 30, 1 << 30, 1 << 30, -1, -1, -1};
    if (old >= 0) remove_lists(g, g->objects[(size_t)old], box);
    VoxLists lists;
    const int rc = voxelize_run(g, shapes, g->d_occ, g->ref_counted ? g->d_counts : nullptr, lists);
    if (rc != SMPLX_OK) return rc;
    for (size_t s = 0; s + 1 < lists.first.size(); ++s) {
        if (lists.first[s + 1] == lists.first[s]) continue;
        const int* b = &lists.box[6 * s];
        box.x0 = std::min(box.x0, b[0]); box.y0 = std::min(box.y0, b[1]); box.z0 = std::min(box.z0, b[2]);
        box.x1 = std::max(box.x1, b[3]); box.y1 = std::max(box.y1, b[4]); box.z1 = std::max(box.z1, b[5]);
    }
    if (old < 0) { g->objects.emplace_back(); old = (int)g->objects.size() - 1; g->objects[(size_t)old].id = id; }
    WorldObject& o = g->objects[(size_t)old];
    if (o.d_cells) (void)hipFree(o.d_cells);
    o.d_cells = lists.d_cells;
    o.first.swap(lists.first);
    o.box.swap(lists.box);
    o.shapes.swap(shapes);
    if (box.x1 < 0) return SMPLX_OK;       // no cell inside the grid, before or after
    return field_update(g, edit_window(g, box));
}

}  // namespace

extern "C" {

// test hooks, not part of the ABI: time of the voxelisation launches of the last call (an octree's k_occ_points
// included), in milliseconds
void smplx_test_voxelize_timing(int on) { g_vox_timing = on != 0; }
double smplx_test_voxelize_kernel_ms(void) { return g_vox_kernel_ms; }

int smplx_world_insert_object(smplx_grid* g, const char* id, const smplx_shape* shapes, int n)
{
    if (!g || !good_id(id)) return smplx_internal_set_error(SMPLX_E_ARG, "null grid, or an id that is empty or holds a line break");
    std::vector<WorldShape> ws;
    if (int e = take_shapes(shapes, n, ws)) return e;
    if (!g->d_occ) return smplx_internal_set_error(SMPLX_E_STATE, kNotEditable);
    if (find_object(g, id) >= 0) return smplx_internal_set_error(SMPLX_E_ARG, (std::string("already have a world object with id ") + id).c_str());
    return put_object(g, id, -1, ws);
}

int smplx_world_move_object(smplx_grid* g, const char* id, const smplx_shape* shapes, int n)
{
    if (!g || !good_id(id)) return smplx_internal_set_error(SMPLX_E_ARG, "null grid, or an id that is empty or holds a line break");
    std::vector<WorldShape> ws;
    if (int e = take_shapes(shapes, n, ws)) return e;
    if (!g->d_occ) return smplx_internal_set_error(SMPLX_E_STATE, kNotEditable);
    const int old = find_object(g, id);
    if (old < 0) return smplx_internal_set_error(SMPLX_E_ARG, (std::string("no world object with id ") + id).c_str());
    return put_object(g, id, old, ws);
}

int smplx_world_remove_object(smplx_grid* g, const char* id)
{
    if (!g || !good_id(id)) return smplx_internal_set_error(SMPLX_E_ARG, "null grid, or an id that is empty or holds a line break");
    if (!g->d_occ) return smplx_internal_set_error(SMPLX_E_STATE, kNotEditable);
    const int at = find_object(g, id);
    if (at < 0) return smplx_internal_set_error(SMPLX_E_ARG, (std::string("no world object with id ") + id).c_str());
    Window box{1 << 30, 1 << 30, 1 << 30, -1, -1, -1};
    remove_lists(g, g->objects[(size_t)at], box);
    FIELD_TRY(hipGetLastError());
    FIELD_TRY(hipDeviceSynchronize());
    if (g->objects[(size_t)at].d_cells) (void)hipFree(g->objects[(size_t)at].d_cells);
    g->objects.erase(g->objects.begin() + at);
    if (box.x1 < 0) return SMPLX_OK;
    return field_update(g, edit_window(g, box));
}

int smplx_world_remove_all(smplx_grid* g)
{
    if (!g) return smplx_internal_set_error(SMPLX_E_ARG, "null grid");
    if (!g->d_occ) return smplx_internal_set_error(SMPLX_E_STATE, kNotEditable);
    Window box{1 << 30, 1 << 30, 1 << 30, -1, -1, -1};
    for (const WorldObject& o : g->objects) remove_lists(g, o, box);
    FIELD_TRY(hipGetLastError());
    FIELD_TRY(hipDeviceSynchronize());
    for (WorldObject& o : g->objects)
        if (o.d_cells) (void)hipFree(o.d_cells);
    g->objects.clear();
    if (box.x1 < 0) return SMPLX_OK;
    return field_update(g, edit_window(g, box));
}

int smplx_world_objects(const smplx_grid* g, char* names, int cap, int* n)
{
    if (n) *n = 0;
    if (!g || !n || cap < 0 || (cap > 0 && !names)) return smplx_internal_set_error(SMPLX_E_ARG, "bad argument");
    std::string text;
    for (const WorldObject& o : g->objects) text += o.id + "\n";
    if (cap > 0) { std::strncpy(names, text.c_str(), (size_t)cap - 1); names[cap - 1] = 0; }
    *n = (int)g->objects.size();
    return SMPLX_OK;
}

int smplx_world_object_cells(const smplx_grid* g, const char* id, int shape, int32_t* cells, int cap, int* n)
{
    if (n) *n = 0;
    if (!g || !good_id(id) || !n || cap < 0 || (cap > 0 && !cells)) return smplx_internal_set_error(SMPLX_E_ARG, "bad argument");
    const int at = find_object(g, id);
    if (at < 0) return smplx_internal_set_error(SMPLX_E_ARG, (std::string("no world object with id ") + id).c_str());
    const WorldObject& o = g->objects[(size_t)at];
    if (shape < 0 || shape + 1 >= (int)o.first.size()) return smplx_internal_set_error(SMPLX_E_ARG, "shape index outside the object");
    const int count = o.first[(size_t)shape + 1] - o.first[(size_t)shape];
    const int take = std::min(cap, count);
    if (take > 0) FIELD_TRY(hipMemcpy(cells, o.d_cells + 3 * (size_t)o.first[(size_t)shape], sizeof(int32_t) * 3 * (size_t)take, hipMemcpyDeviceToHost));
    *n = count;
    return SMPLX_OK;
}

int smplx_world_voxelize(const smplx_grid* g, const smplx_shape* shapes, int n, int32_t* cells, int cap, int32_t* first)
{
    if (!g || !first || cap < 0 || (cap > 0 && !cells)) return smplx_internal_set_error(SMPLX_E_ARG, "bad argument");
    std::vector<WorldShape> ws;
    if (int e = take_shapes(shapes, n, ws)) return e;
    VoxLists lists;
    const int rc = voxelize_run(g, ws, nullptr, nullptr, lists);
    hipError_t e = hipSuccess;
    if (rc == SMPLX_OK) {
        for (int s = 0; s <= n; ++s) first[s] = lists.first[(size_t)s];
        const int take = std::min(cap, lists.first[(size_t)n]);
        if (take > 0) e = hipMemcpy(cells, lists.d_cells, sizeof(int32_t) * 3 * (size_t)take, hipMemcpyDeviceToHost);
    }
    if (lists.d_cells) (void)hipFree(lists.d_cells);
    if (e != hipSuccess) return smplx_internal_set_error(SMPLX_E_HIP, (std::string("cell download: ") + hipGetErrorString(e)).c_str());
    return rc;
}

// for engine.hip (smplx_attach_object / smplx_object_spheres), not part of the ABI: checks the shapes and the radius and
// makes the sphere rows of the object; work / work_bytes is the voxeliser work space of the calling space
int smplx_internal_object_spheres(void** work, size_t* work_bytes, const smplx_shape* shapes, int n, double radius, std::vector<double>* rows,
                                  std::vector<int32_t>* first)
{
    std::vector<WorldShape> ws;
    if (int e = take_shapes(shapes, n, ws)) return e;
    for (const WorldShape& w : ws)
        if (w.type == SMPLX_SHAPE_OCTREE) return smplx_internal_set_error(SMPLX_E_ARG, "octrees cannot be attached: an attached object has no octree shapes");
    if (!(radius > 0.0 && radius < 1.0e6)) return smplx_internal_set_error(SMPLX_E_ARG, "the sphere radius must be positive and finite (< 1e6)");
    return object_spheres_run(work, work_bytes, ws, radius, *rows, *first);
}

}  // extern "C"
