// smpl_amd/csrc/object_sphere_rows.h -- the sphere rows of an object attached by shape, in field.hip: the mesh voxeliser
// on the lattice of object_spheres.h, then one row per filled voxel.  Reference:
// sbpl_collision_checking/src/attached_bodies_collision_model.cpp:264-313 (generateSpheresModel).
#pragma once

#include "mesh_voxelizer.h"
#include "object_spheres.h"

namespace {

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

// the sphere model of an attached object: every shape's surface voxelised on the lattice of object_spheres.h -- pivot 0,
// resolution radius / sqrt(2), candidates clipped to the index range of the shape's own bounding box, negative indices
// kept -- and one row {x, y, z, radius} per filled voxel, the shapes' lists back to back (a voxel two shapes fill gives
// two rows).  work: the calling space's work space; it holds the voxeliser's arrays and then the rows, which are copied
// back once.  Waits for the device.
int object_spheres_run(WorkSpace& work, const std::vector<WorldShape>& shapes, double radius, std::vector<double>& rows, std::vector<int32_t>& first)
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
    if (int e = voxelize_meshes(work, L, meshes, clip, nullptr, nullptr, 0, 0, lists)) return e;
    first.assign(lists.first.begin(), lists.first.end());
    const int total = lists.first.back();
    rows.assign(4 * (size_t)total, 0.0);
    if (total == 0) return SMPLX_OK;
    const size_t bytes[1] = {sizeof(double) * 4 * (size_t)total};
    size_t at[1];
    FIELD_TRY(work.carve(bytes, at));          // the voxeliser's arrays are done with: the rows may take a new block
    double* const d_rows = (double*)(work.base + at[0]);
    hipLaunchKernelGGL(k_vox_spheres, dim3((total + FIELD_BLOCK - 1) / FIELD_BLOCK), dim3(FIELD_BLOCK), 0, 0, (const int*)lists.d_cells, total, res, radius, d_rows);
    FIELD_TRY(hipGetLastError());
    FIELD_TRY(hipMemcpy(rows.data(), d_rows, bytes[0], hipMemcpyDeviceToHost));
    return SMPLX_OK;
}

}  // namespace
