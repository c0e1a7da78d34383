"""Octree shapes and judged cell lists shared by the octree tests (tests/test_octree_model.py, tests/test_gpu_octree.py),
on the grid of tests/world_cases.py.  The model's answers (tests/octree_ref.py) are computed once per process and never
changed.  Every case is the smallest at which a distinct thing can break:
  small, equal    a leaf narrower than a cell and one exactly as wide: one point each;
  two_res, odd    leaves of 2 res and of 2.5 res (half-width 0.06) at centres where the running sum of a loop lands within
                  an ulp of its bound: some axes make 2 c / res trips, others one more (TRIPS; the model decided which);
  big             one leaf of 16 res, 32 or 33 trips an axis: many blocks of points, partly outside the grid;
  cloud           4097 leaves of four sizes from scenes.octree_leaves: the scan over the leaves crosses block boundaries;
  outside         a leaf wholly outside the grid."""
import functools

import numpy as np

import octree_ref as O
import world_cases as W
from smpl_amd import scenes

IDENTITY = W.pose()
POSES = {"identity": IDENTITY, "rotated": W.POSE}


def cloud_points(seed=3):
    """scattered points, a solid block aligned with the tree (merges twice, to leaves of 0.08) and one that is not (leaves
    of 0.04, 0.02 and 0.01 side by side), on an octree of resolution 0.01"""
    rng = np.random.default_rng(seed)
    scatter = rng.uniform((0.0, -0.1, 0.1), (0.5, 0.4, 0.5), (4400, 3))
    k = np.arange(16)
    aligned = np.stack(np.meshgrid(k + 16, k, k + 16, indexing="ij"), -1).reshape(-1, 3)
    k = np.arange(14)
    ragged = np.stack(np.meshgrid(k + 1, k + 21, k + 33, indexing="ij"), -1).reshape(-1, 3)
    return np.vstack([scatter, (aligned + 0.5) * 0.01, (ragged + 0.5) * 0.01])


@functools.lru_cache(maxsize=None)
def leaves(key):
    if key == "cloud":
        rows = scenes.octree_leaves(cloud_points(), 0.01, 10)
        assert len(rows) >= 4097
        rows = rows[:4097]
    else:
        rows = np.array(LEAVES[key], float)
    rows.setflags(write=False)
    return rows


LEAVES = {
    "small": [(0.05, 0.1, 0.2, 0.01)],
    "equal": [(0.05, 0.1, 0.2, 0.02)],
    "two_res": [(0.05, 0.15, 0.1, 0.04), (0.15, 0.05, 0.12, 0.04)],
    "odd": [(0.05, 0.13, 0.12, 0.05), (0.13, 0.12, 0.06, 0.05)],
    "big": [(0.3, 0.2, 0.2, 0.32)],
    "outside": [(5.0, 5.0, 5.0, 0.04)],
}
KEYS = ["small", "equal", "two_res", "odd", "big", "cloud", "outside"]
# trips per axis of every leaf of the two cases on the bound, as the model counts them: 2 c / res is 4 resp. 6
TRIPS = {"two_res": [(4, 5, 4), (5, 4, 5)], "odd": [(6, 7, 6), (7, 6, 6)]}


def shape(key, pose="rotated"):
    """what capi.octree returns for the case"""
    return dict(type=6, dims=(0.0, 0.0, 0.0), pose=POSES[pose], leaves=leaves(key))


@functools.lru_cache(maxsize=None)
def judged(key, pose="rotated"):
    """the model's cells inside the grid, in generation order, duplicates kept"""
    c = O.cells(leaves(key), POSES[pose], W.ORIGIN, W.RES, W.DIMS)
    c.setflags(write=False)
    return c


def multiplicities(cells):
    """how often each cell of the grid is listed"""
    m = np.zeros(W.DIMS, np.int32)
    np.add.at(m, tuple(np.asarray(cells).reshape(-1, 3).T), 1)
    return m


def unique_points(cells):
    """voxel centres of the distinct cells: what the point route hands to add_points"""
    return W.world_points(np.unique(np.asarray(cells).reshape(-1, 3), axis=0))
