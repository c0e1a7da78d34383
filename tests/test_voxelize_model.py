"""The judge of the world-object tests (tests/voxelize_ref.py) pinned by answers derived by hand from the reference's
lines, the identity of voxel indices and occupancy cells, and the voxeliser's own source (smpl_amd/csrc/voxelize.h)
compiled for the CPU against the judge.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import voxelize_ref as V
import world_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O0 = (0.0, 0.0, 0.0)


def cells_of(tris, origin=O0, res=1.0):
    v = np.array([p for t in tris for p in t], float)
    c, _ = V.voxelize_mesh(v, np.arange(len(v)).reshape(-1, 3), origin, res)
    return set(map(tuple, c))


def test_right_triangle_counted_by_hand():
    """p1 = (0,0,0), p2 = (4,0,0), p3 = (0,4,0) at res = 1, pivot 0: voxel centres are the integer points, rc^2 = 0.75,
    candidates x, y in 0..4 and z = 0 (voxelize.hpp:115-127), 25 voxels.
      vertex test (:145-147): only the three vertex voxels (every other centre is at least 1 away);
      edge tests (:152-154) on (p1,p3), (p2,p3), (p3,p1): the x = 0 column; the voxels on the hypotenuse x + y = 4; and the
        diagonals x + y = 3 and x + y = 5, whose centres are 1/sqrt(2) from it (dsq = 0.5 <= 0.75) and project inside it;
      plane and guards (:161-172): n = (0,0,1), t = rc * 0.5774 = 0.5, guards y > 0, x + y < 4, x > 0: of what is left only
        (1,1,0).  (1,0,0) and (2,0,0) lie ON edge p1-p2, which no edge test covers, and fail the guard y > 0: empty."""
    got = cells_of([[(0, 0, 0), (4, 0, 0), (0, 4, 0)]])
    vertex = {(0, 0, 0), (4, 0, 0), (0, 4, 0)}
    edge = {(0, 1, 0), (0, 2, 0), (0, 3, 0), (3, 1, 0), (2, 2, 0), (1, 3, 0), (1, 2, 0), (2, 1, 0), (3, 0, 0),
            (1, 4, 0), (2, 3, 0), (3, 2, 0), (4, 1, 0)}
    interior = {(1, 1, 0)}
    assert got == vertex | edge | interior and len(got) == 17
    assert (1, 0, 0) not in got and (2, 0, 0) not in got
    cells, filled, margin = V.voxelize_triangle((0, 0, 0), (4, 0, 0), (0, 4, 0), O0, 1.0)
    assert len(cells) == 25 and set(cells[:, 2]) == {0}
    # the guard y > 0 is an exact tie for the voxels on edge p1-p2: the model flags them
    tie = {tuple(c) for c, m in zip(cells, margin) if m < 1e-9}
    assert {(1, 0, 0), (2, 0, 0)} <= tie


def test_edge_p1_p2_is_never_tested_on_its_own():
    """The voxel (3,0,0) lies 0.4 outside edge (0,0.4,0)-(6,0.4,0) and far from the other two edges (1.7 and 3) and from
    every vertex: a capsule test of that edge would fill it (0.16 <= 0.75).  As p1-p2 it is not tested (voxelize.hpp:152-154)
    and the guard e1.x + d1 = -0.4 > 0 fails: empty.  The same triangle with its vertices rotated, so that the edge is
    (p2,p3), fills it."""
    a, b, c = (0, 0.4, 0), (6, 0.4, 0), (6, 3.4, 0)
    assert (3, 0, 0) not in cells_of([[a, b, c]])
    assert (3, 0, 0) in cells_of([[c, a, b]])
    assert (3, 0, 0) in cells_of([[b, c, a]])      # (p3,p1) is listed too


def test_collinear_triangle_is_skipped():
    assert cells_of([[(0, 0, 0), (1, 1, 1), (2, 2, 2)]]) == set()
    assert V.triangle_constants((0, 0, 0), (1, 1, 1), (2, 2, 2), 1.0) is None
    # ... while its vertices alone would fill voxels in a proper triangle
    assert (0, 0, 0) in cells_of([[(0, 0, 0), (1, 1, 1), (2, 0, 2)]])


def test_candidates_are_the_discretised_bounding_box_only():
    """The triangle of the first test lifted to z = 0.3: discretize(0.3) = floor(0.8) = 0, so z = 0 is the only layer.
    The voxel (0,0,1) has its centre 0.7 from p1 (0.49 <= rc^2 = 0.75) and still stays empty (voxelize.hpp:119-127)."""
    tri = [(0, 0, 0.3), (4, 0, 0.3), (0, 4, 0.3)]
    got = cells_of([tri])
    assert (0.0 - 0.0) ** 2 + (1.0 - 0.3) ** 2 <= 0.75
    assert (0, 0, 0) in got and (0, 0, 1) not in got and {c[2] for c in got} == {0}
    lo, hi = V.candidate_range(*tri, O0, 1.0)
    assert (lo, hi) == ([0, 0, 0], [4, 4, 0])
    # discretize / continuize (discretize.h:49-55): cell i is centred on pivot + i * res
    assert [V.discretize(x, 0.25, 0.5) for x in (-0.01, 0.0, 0.49, 0.5, 0.51, 1.0)] == [-1, 0, 0, 1, 1, 2]
    assert V.continuize(3, 0.25, 0.5) == 1.75


def test_mesh_generators():
    """vertex / triangle counts and first / last vertices (mesh_utils.cpp:91-98, 131-151, 217-238, 278-285)"""
    v, t = V.box_mesh(1.0, 2.0, 3.0)
    assert (len(v), len(t)) == (8, 12) and tuple(v[0]) == (-0.5, -1.0, -1.5) and tuple(v[-1]) == (0.5, 1.0, 1.5)
    assert t[0].tolist() == [0, 2, 1] and t[-1].tolist() == [4, 5, 0]
    v, t = V.sphere_mesh(2.0)
    assert (len(v), len(t)) == (58, 112) and tuple(v[0]) == (0.0, 0.0, 2.0) and tuple(v[-1]) == (0.0, 0.0, -2.0)
    assert np.allclose(np.linalg.norm(v, axis=1), 2.0) and t.min() == 0 and t.max() == 57
    assert t[0].tolist() == [0, 1, 2] and t[6].tolist() == [0, 7, 1] and t[-1].tolist() == [57, 51, 50]
    v, t = V.cylinder_mesh(1.5, 4.0)
    assert (len(v), len(t)) == (34, 64) and tuple(v[0]) == (1.5, 0.0, 2.0) and tuple(v[-1]) == (0.0, 0.0, -2.0)
    assert t[0].tolist() == [0, 1, 16] and t[-1].tolist() == [33, 16, 31]
    v, t = V.cone_mesh(1.5, 4.0)
    assert (len(v), len(t)) == (18, 32) and tuple(v[0]) == (1.5, 0.0, -2.0) and tuple(v[-1]) == (0.0, 0.0, -2.0)
    assert tuple(v[16]) == (0.0, 0.0, 2.0) and t[0].tolist() == [0, 1, 16] and t[-1].tolist() == [15, 0, 17]
    # every triangle of every generator is proper (none is skipped)
    for v, t in (V.box_mesh(1, 2, 3), V.sphere_mesh(2.0), V.cylinder_mesh(1.5, 4.0), V.cone_mesh(1.5, 4.0)):
        assert all(V.triangle_constants(v[a], v[b], v[c], 0.1) is not None for a, b, c in t)
    # TransformVertices: R v + t
    P = W.pose((1.0, 2.0, 3.0), W.ROT)
    assert np.allclose(V.transform(P, np.array([[0.3, -0.2, 0.5]])), W.ROT @ [0.3, -0.2, 0.5] + [1, 2, 3], atol=1e-15)


def _world_to_cell(w, origin, res):
    """smplx_grid_add_points' rule (smpl_amd/csrc/field.hip world_to_cell; OccupancyGrid::worldToGrid,
    distance_map.hpp:520-527), restated: the C cast truncates towards zero"""
    inv_res = 1.0 / res
    return int(inv_res * (w - (origin - res)) + 0.5) - 1


@pytest.mark.parametrize("origin,dims,res", [(W.ORIGIN, W.DIMS, W.RES), ((-0.78, -1.28, -0.48), (64, 64, 64), 0.04),
                                             ((-1.0, -2.5, 0.0), (256, 256, 256), 0.02), ((0.3, 0.0, -7.1), (100, 3, 17), 0.013)])
def test_voxel_index_is_the_occupancy_cell(origin, dims, res):
    """continuize(i) of the voxel grid whose pivot is the grid's origin lands in occupancy cell i, for every i of the
    grid and the border layer around it; and discretize inverts continuize"""
    for a in range(3):
        for i in range(-1, dims[a] + 1):
            w = V.continuize(i, origin[a], res)
            assert _world_to_cell(w, origin[a], res) == i, (a, i)
            assert V.discretize(w, origin[a], res) == i, (a, i)


def test_trial_cases_of_the_issue():
    """the cell counts of the trial restatement; no cell of the first four cases (and of the cone) is undecided, at 1e-9
    and even at 1e-6; the grid-aligned box sits on exact ties: its undecided cells stay below 15 % of its cells"""
    for key, n in W.TRIAL_CELLS.items():
        s, cells, und = W.judged(key)
        assert len(cells) == n, key
        if key != "aligned":
            assert len(und) == 0, key
            assert len(V.voxelize_shape(s, W.ORIGIN, W.RES, clip=W.DIMS, eps=1e-6)[1]) == 0, key
    assert len(W.judged("cone")[2]) == 0
    _, cells, und = W.judged("aligned")
    assert 0 < len(und) <= 0.15 * len(cells)
    # clipping changes nothing for shapes inside the grid, and cuts the straddling sphere
    for key in ("box", "soup"):
        assert np.array_equal(V.voxelize_shape(W.SHAPES[key], W.ORIGIN, W.RES)[0], W.judged(key)[1])
    whole = V.voxelize_shape(W.STRADDLE, W.ORIGIN, W.RES)[0]
    assert np.array_equal(V.in_grid(whole, W.DIMS), W.judged("straddle")[1]) and 0 < len(W.judged("straddle")[1]) < len(whole)
    assert len(W.judged("outside")[1]) == 0


@pytest.fixture(scope="module")
def host_voxeliser(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vox") / "voxelize_host_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "voxelize_host_driver.cpp"),
                           "-o", exe])
    return exe


@pytest.mark.parametrize("key", ["box", "sphere", "cylinder", "soup", "aligned", "cone", "straddle", "one_triangle", "big_and_small"])
def test_the_kernels_source_on_the_cpu_equals_the_model(host_voxeliser, key):
    """smpl_amd/csrc/voxelize.h -- the per-triangle constants and the per-voxel decision the kernels compile -- built by
    the host compiler and run over every clipped candidate voxel equals the model, in order, under the issue's rule"""
    s, want, und = W.judged(key)
    v, t = V.shape_mesh(s)
    text = " ".join([float(x).hex() for x in W.ORIGIN] + [float(W.RES).hex()] + [str(d) for d in W.DIMS] + [str(len(t))]
                    + [float(x).hex() for tri in t for i in tri for x in v[i]])
    out = subprocess.run([host_voxeliser], input=text, capture_output=True, text=True, check=True).stdout
    got = np.array(out.split(), int).reshape(-1, 3)
    W.compare(got, key)
    if key != "aligned" and key != "one_triangle":
        assert len(und) == 0 and np.array_equal(got, want)
