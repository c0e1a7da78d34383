// smpl_amd/csrc/object_spheres.h -- the sphere model of an attached object (include/smpl_amd.h "attached collision
// bodies", smplx_attach_object): the lattice its shapes are voxelised on and the sphere a filled voxel becomes.  Nothing
// here makes a HIP call, so the host compiler builds it for tests/cpp/object_spheres_host_driver.cpp as it builds
// robot_body.h and voxelize.h for their drivers.
// What it stands behind: AttachedBodiesCollisionModel::generateSpheresModel
// (sbpl_collision_checking/src/attached_bodies_collision_model.cpp:264-313) over VoxelizeMesh(vertices, triangles, res,
// voxel_origin = 0, voxels, fill = false) (smpl/src/geometry/voxelize.cpp:1008-1035): a PivotVoxelGrid with pivot (0, 0, 0)
// laid over the mesh's own bounding box, whose index range VoxelGrid's constructor takes from `min` and `min + size`
// (smpl/include/smpl/geometry/voxel_grid.h:174-196), and one sphere at the centre of every filled voxel
// (PivotDiscretizer::continuize, discretize.h:40-61).  This is the voxeliser's third lattice: the occupancy grid's
// (world_objects.h voxelize_run) and the HalfRes one of a link's voxel model (body_place.h) are the other two.
#pragma once

#include <cstddef>

#include "voxelize.h"

namespace smplx_object_host {

// most cells the index ranges of one call's shapes may hold (one mask byte each on the device)
const long long kMaxRangeCells = 1ll << 28;

// object_enclosing_sphere_radius / std::sqrt(2)  (attached_bodies_collision_model.cpp:288): this quotient, not a product
inline double resolution(double radius) { return radius / sqrt(2.0); }

// PivotDiscretizer::discretize at pivot 0.  The index is clamped to +-2^30 in double before the cast: a tiny radius must
// not overflow an int (the caller refuses a range that large)
inline int pivot_index(double w, double res)
{
    double f = floor((w - 0.0) / res + 0.5);
    if (f < -1073741824.0) f = -1073741824.0;
    if (f > 1073741824.0) f = 1073741824.0;
    return (int)f;
}

// the inclusive index range {lo[3], hi[3]} of the grid VoxelizeMesh lays over nv vertices (already at the shape's pose):
// [discretize(min), discretize(min + (max - min))] along every axis, as VoxelGrid's constructor computes it
inline void clip_range(const double* v, size_t nv, double res, int clip[6])
{
    for (int a = 0; a < 3; ++a) {
        double mn = v[a], mx = v[a];
        for (size_t i = 1; i < nv; ++i) {
            const double x = v[3 * i + a];
            if (x < mn) mn = x;
            if (x > mx) mx = x;
        }
        const double size = mx - mn;
        clip[a] = pivot_index(mn, res);
        clip[3 + a] = pivot_index(mn + size, res);
    }
}

inline long long range_cells(const int clip[6])
{
    long long n = 1;
    for (int a = 0; a < 3; ++a) {
        const long long d = (long long)clip[3 + a] - clip[a] + 1;
        if (d <= 0) return 0;
        if (d > kMaxRangeCells) return kMaxRangeCells + 1;
        n *= d;
        if (n > kMaxRangeCells) return kMaxRangeCells + 1;
    }
    return n;
}

// the sphere of voxel (i, j, k): {0.0 + i * res, 0.0 + j * res, 0.0 + k * res, radius}
SMPLX_HD void sphere_row(const int* cell, double res, double radius, double* row)
{
    row[0] = vox_continuize(cell[0], 0.0, res);
    row[1] = vox_continuize(cell[1], 0.0, res);
    row[2] = vox_continuize(cell[2], 0.0, res);
    row[3] = radius;
}

}  // namespace smplx_object_host
