"""The judge of the octree tests (tests/octree_ref.py) pinned by answers worked out by hand from the reference's lines
(voxel_operations.cpp:405-436), the octree's own source (smpl_amd/csrc/octree_points.h) compiled for the CPU -- with the
address and undefined-behaviour sanitizers, as a program -- against the judge, and scenes.octree_leaves on a hand-worked
cloud.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import octree_cases as T
import octree_ref as O
import world_cases as W
from smpl_amd import capi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_by_hand():
    """res = 1 (every sum below is exact): a leaf of size 1 or less is its centre; a leaf of size 2 at 0 has
    ceil_val = 2 and each loop runs -2, -1, 0, 1 (2 is not < 2): 64 points, twice the leaf's width, z fastest; a leaf of
    size 1.5 has ceil_val = ceil(1.5) = 2 as well"""
    assert O.leaf_points((0.25, 0.5, 0.75, 1.0), 1.0) == [(0.25, 0.5, 0.75)]
    assert O.leaf_points((0.25, 0.5, 0.75, 0.3), 1.0) == [(0.25, 0.5, 0.75)]
    p = O.leaf_points((0.0, 0.0, 0.0, 2.0), 1.0)
    assert len(p) == 64 and p[0] == (-2.0, -2.0, -2.0) and p[1] == (-2.0, -2.0, -1.0) and p[4] == (-2.0, -1.0, -2.0) and p[-1] == (1.0, 1.0, 1.0)
    assert O.axis_values(10.0, 1.5, 1.0) == [8.0, 9.0, 10.0, 11.0]
    # the running sum, not start + k * res: at res = 0.02 the two differ in the last bits
    v = O.axis_values(0.15, 0.04, 0.02)
    assert v[3] == ((0.15 - 0.04) + 0.02 + 0.02 + 0.02) and any(v[k] != (0.15 - 0.04) + k * 0.02 for k in range(len(v)))
    # the pose and worldToGrid
    assert O.transform(W.pose((1.0, 2.0, 3.0)), (0.5, 0.25, 0.125)) == (1.5, 2.25, 3.125)
    assert [O.world_to_cell(w, 0.0, 0.5) for w in (-0.26, -0.25, 0.0, 0.24, 0.25, 0.74, 0.75)] == [-1, 0, 0, 0, 1, 1, 2]
    c = O.cells([(0.0, 0.0, 0.0, 2.0)], W.pose(), (0.0, 0.0, 0.0), 1.0, (2, 2, 2))
    assert len(O.cells([(0.0, 0.0, 0.0, 2.0)], W.pose(), (0.0, 0.0, 0.0), 1.0)) == 64 and len(c) == 8 and c[0].tolist() == [0, 0, 0]


def test_both_trip_counts_occur():
    """the centres of the cases on the bound: the model itself says which axes make 2 c / res trips and which one more"""
    for key, nominal in (("two_res", 4), ("odd", 6)):
        got = [tuple(len(O.axis_values(leaf[a], leaf[3], W.RES)) for a in range(3)) for leaf in T.leaves(key)]
        assert got == T.TRIPS[key]
        flat = [n for t in got for n in t]
        assert nominal in flat and nominal + 1 in flat and set(flat) == {nominal, nominal + 1}
        assert nominal == 2 * math.ceil(T.leaves(key)[0][3] / W.RES)
    assert math.ceil(0.05 / W.RES) * W.RES == 0.06
    # the big leaf and the cloud: more points than a block, more leaves than a block, several sizes
    assert 32 ** 3 <= len(O.leaf_points(T.leaves("big")[0], W.RES)) <= 33 ** 3
    sizes = np.unique(T.leaves("cloud")[:, 3])
    assert len(T.leaves("cloud")) == 4097 and len(sizes) >= 4 and sizes.min() < W.RES < sizes.max()
    for key in T.KEYS:
        for pose in T.POSES:
            n = len(T.judged(key, pose))
            assert (n == 0) == (key == "outside"), (key, pose)
    _, per_leaf = O.points(T.leaves("big"), T.IDENTITY, W.RES)
    assert 0 < len(T.judged("big", "identity")) < per_leaf[0]        # partly outside the grid


def test_octree_leaves_by_hand():
    """res = 1, depth = 3 (keys -4 .. 3).  Eight points in the cells of the cube [0, 2)^3 merge into one leaf of size 2 at
    (1, 1, 1); seven of the cube [-2, 0)^3 do not.  Filling [-4, 0) x [0, 4) x [0, 4) (64 cells) merges twice, into one
    leaf of size 4 at (-2, 2, 2).  Depth-first order, children 0..7 with x in bit 0: at the top level the child with
    x < 0, y < 0, z < 0 comes first, then z >= 0 with x < 0, y >= 0, then x >= 0, y >= 0."""
    k = np.array([(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)], float)
    eight = k + 0.5
    seven = (k - 2.0 + 0.25)[:7]
    k4 = np.array([(x, y, z) for x in range(4) for y in range(4) for z in range(4)], float)
    block = k4 + np.array([-4.0, 0.0, 0.0]) + 0.5
    rows = scenes.octree_leaves(np.vstack([eight, seven, block]), 1.0, 3)
    want = [(-1.5, -1.5, -1.5, 1.0), (-0.5, -1.5, -1.5, 1.0), (-1.5, -0.5, -1.5, 1.0), (-0.5, -0.5, -1.5, 1.0),
            (-1.5, -1.5, -0.5, 1.0), (-0.5, -1.5, -0.5, 1.0), (-1.5, -0.5, -0.5, 1.0),
            (-2.0, 2.0, 2.0, 4.0), (1.0, 1.0, 1.0, 2.0)]
    assert rows.tolist() == [list(r) for r in want]
    # a point given twice is one leaf; a point outside the tree is refused
    assert scenes.octree_leaves([(0.1, 0.1, 0.1), (0.2, 0.3, 0.4)], 1.0, 3).tolist() == [[0.5, 0.5, 0.5, 1.0]]
    with pytest.raises(ValueError):
        scenes.octree_leaves([(4.5, 0.0, 0.0)], 1.0, 3)
    # capi.octree takes such rows and refuses anything that is not n x 4
    s = capi.octree(rows, W.POSE)
    assert s["type"] == capi.SHAPE_OCTREE == 6 and np.array_equal(s["leaves"], rows) and np.array_equal(s["pose"], W.POSE)
    for bad in ([], [(0.0, 0.0, 0.0)], [0.0, 0.0, 0.0, 1.0], np.zeros((2, 5))):
        with pytest.raises(capi.SmplxError) as e:
            capi.octree(bad)
        assert e.value.code == -1
    arr, n, keep = capi._shape_array([s])
    assert n == 1 and arr[0].type == 6 and arr[0].nvertices == 9 and arr[0].ntriangles == 0 and not arr[0].triangles
    assert [arr[0].vertices[i] for i in range(8)] == list(want[0]) + list(want[1])


@pytest.fixture(scope="module")
def host_octree(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("oct") / "octree_host_driver")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "octree_host_driver.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("pose", list(T.POSES))
@pytest.mark.parametrize("key", T.KEYS)
def test_the_kernels_source_on_the_cpu_equals_the_model(host_octree, key, pose):
    """smpl_amd/csrc/octree_points.h -- the trips of a (leaf, axis) and the value at a trip, as the kernels compile them --
    built by the host compiler and run point by point equals the model: points per leaf, every coordinate bit for bit,
    every cell"""
    L, P = T.leaves(key), T.POSES[pose]
    text = " ".join([float(x).hex() for x in W.ORIGIN] + [float(W.RES).hex()] + [float(x).hex() for x in np.asarray(P).ravel()] + [str(len(L))]
                    + [float(x).hex() for x in L.ravel()])
    out = subprocess.run([host_octree], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    want, per_leaf = O.points(L, P, W.RES)
    got_counts = [int(line.split()[1]) for line in out if line.startswith("leaf")]
    assert got_counts == per_leaf
    rows = [line.split() for line in out if not line.startswith("leaf")]
    assert len(rows) == len(want)
    assert [tuple(float.fromhex(x) for x in r[:3]) for r in rows] == want
    cells = np.array([[int(x) for x in r[3:]] for r in rows], np.int64).reshape(-1, 3)
    assert np.array_equal(cells, O.cells(L, P, W.ORIGIN, W.RES))
    assert np.array_equal(W.V.in_grid(cells, W.DIMS), T.judged(key, pose))
