// smpl_amd/csrc/grid_handle.h -- the smplx_grid handle (include/smpl_amd.h), shared by engine.hip (lookup side) and
// field.hip (construction side)
#pragma once

#include <stdint.h>

#include <memory>
#include <string>
#include <vector>

#include "device_mem.h"
#include "device_types.h"

// a world object (sbpl::collision::Object: id, shapes, shape poses) with the cells its shapes were voxelised into
struct WorldShape {
    int type;
    double dims[3];
    double pose[12];
    std::vector<double> vertices;     // MESH only
    std::vector<int32_t> triangles;   // MESH only
};
struct WorldObject {
    std::string id;
    std::vector<WorldShape> shapes;   // as given
    DevPtr<int32_t> d_cells;          // the shapes' cell lists back to back, on the device (n x 3)
    std::vector<int> first;           // shapes + 1 entries: shape s owns cells [first[s], first[s + 1])
    std::vector<int> box;             // 6 per shape: the clipped cell range the list lies in (x0 y0 z0 x1 y1 z1)
};

// the robot body placed on a grid (body_place.h): the cell list of every outside voxels state, one cell per model point
struct GridBody {
    uint64_t serial = 0;              // which smplx_body it belongs to (the handle itself may be gone)
    std::vector<int> first;           // models + 1 entries: model m owns cells [first[m], first[m + 1]) of a half; a
                                      // model of a group link owns none
    std::vector<unsigned char> placed, half;   // per model: has a list; which half of d_cells holds it
    std::vector<int> box;             // 6 per model: the cell range its in-grid cells lie in (x1 < x0: none inside)
    DevPtr<int32_t> d_cells;          // two halves of first.back() cells each (n x 3): a put writes the other half
    DevPtr<double> d_points;          // the body's link-frame points (its own copy: the body may be destroyed)
    std::vector<int> point_first;     // models + 1: model m's points in d_points
    WorkSpace states;                 // of a put: transforms, prefixes and boxes of the states being placed
};

// Every device array of a grid is owned by the member that names it (DevPtr, WorkSpace, the body): deleting the grid frees
// them all, and nothing else does.
struct smplx_grid {
    SmplxGridDev dev;
    DevPtr<uint16_t> d_d2;           // brick-tiled squared cell distances (what the kernels read)
    DevPtr<unsigned char> d_occ;     // occupancy, x-major / z fastest (only grids built on the GPU: field.hip)
    DevPtr<uint16_t> d_tmp;          // two intermediate passes of the distance transform (kept: an edit recomputes a window of them)
    DevPtr<int32_t> d_counts;        // reference counts per cell (OccupancyGrid::m_counts), only while ref_counted
    bool ref_counted = false;
    uint64_t epoch = 0;              // bumped by every edit: spaces remember the epoch their caches belong to
    long long last_window_cells = 0; // cells the last edit recomputed (diagnostics)
    double origin[3];
    double res, max_dist;
    int n[3];
    int dmax_int, dmax_sqrd;
    std::vector<WorldObject> objects; // the world's objects in insertion order (world_objects.h)
    // work space of the voxelisers (mesh_voxelizer.h and octree_voxelizer.h carve it each in their own way and take turns);
    // mutable because smplx_world_voxelize works on a const grid; calls on one grid are not reentrant, like its edits
    mutable WorkSpace vox;
    std::unique_ptr<GridBody> body;   // at most one placed robot body (body_place.h)
};
