"""A plain restatement of the reference's octree voxeliser: the judge of the octree tests.

Restated lines, with Python floats (binary64, one rounding per operation, no fused multiply-add):
  - VoxelizeOcTree, sbpl_collision_checking/src/voxel_operations.cpp:405-436: a leaf {cx, cy, cz, size} with size <= res
    gives its centre (:415-418); any other gives ceil_val = ceil(size / res) * res (:420) and the three nested loops
    `for (v = centre - ceil_val; v < centre + ceil_val; v += res)`, x outermost, z innermost (:421-423).  The loop variable
    is a running sum, and the loops stop where that sum says so;
  - `pose * pt` (:417, :426) is Eigen's Affine3d * Vector3d: per row R[r,0] v0 + (R[r,1] v1 + R[r,2] v2), then + t[r], the
    form tests/voxelize_ref.py transform() uses for mesh vertices;
  - OccupancyGrid::worldToGrid, smpl/include/smpl/distance_map/detail/distance_map.hpp:520-527:
    (int)(inv_res * (w - (origin - res)) + 0.5) - 1, the C cast truncating towards zero.
The y loop does not depend on x nor the z loop on y, so each loop's values are computed once per leaf and the points are
their product in loop order: the same values the nested loops would compute again and again.
"""
import itertools
import math

import numpy as np


def axis_values(centre, size, res):
    """the values one loop of a leaf takes (:421-423); a leaf with size <= res has the one value `centre` (:415-416)"""
    if size <= res:
        return [centre]
    ceil_val = math.ceil(size / res) * res
    out = []
    v = centre - ceil_val
    while v < centre + ceil_val:
        out.append(v)
        v += res
    return out


def leaf_points(leaf, res):
    """the points of one leaf in the octree's frame, in generation order"""
    cx, cy, cz, size = (float(x) for x in leaf)
    return list(itertools.product(axis_values(cx, size, res), axis_values(cy, size, res), axis_values(cz, size, res)))


def transform(pose, p):
    P = [[float(x) for x in row] for row in np.asarray(pose, float).reshape(3, 4)]
    return tuple((P[r][0] * p[0] + (P[r][1] * p[1] + P[r][2] * p[2])) + P[r][3] for r in range(3))


def world_to_cell(w, origin, res):
    inv_res = 1.0 / res
    return int(inv_res * (w - (origin - res)) + 0.5) - 1


def points(leaves, pose, res):
    """(world-frame points of all leaves in generation order, points per leaf)"""
    out, per_leaf = [], []
    for leaf in np.asarray(leaves, float).reshape(-1, 4):
        pts = leaf_points(leaf, res)
        per_leaf.append(len(pts))
        out += [transform(pose, p) for p in pts]
    return out, per_leaf


def cells(leaves, pose, origin, res, dims=None):
    """the cell of every point, in generation order, duplicates kept (n x 3); with dims only those inside the grid"""
    pts, _ = points(leaves, pose, res)
    c = [tuple(world_to_cell(p[a], float(origin[a]), res) for a in range(3)) for p in pts]
    if dims is not None:
        c = [x for x in c if all(0 <= x[a] < dims[a] for a in range(3))]
    return np.asarray(c, dtype=np.int64).reshape(-1, 3)
