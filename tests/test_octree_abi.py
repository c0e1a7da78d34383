"""Octree shapes at the world-object entry points (include/smpl_amd.h "world objects") without a GPU: the header, the
binding and the C++ mirror name them, every bad octree is refused before any grid is touched, and a good one passes the
argument checks and gets as far as the check of the handle.  What needs a grid is in tests/test_gpu_octree.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from smpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_STATE = -1, -5
LEAVES = [(0.1, 0.2, 0.3, 0.04), (0.3, 0.2, 0.1, 0.01)]


def test_header_binding_and_mirror_name_the_octree():
    hdr = open(os.path.join(ROOT, "include", "smpl_amd.h")).read()
    assert re.search(r"SMPLX_SHAPE_OCTREE\s*=\s*6\b", hdr) and capi.SHAPE_OCTREE == 6 and callable(capi.octree)
    assert "voxel_operations.cpp:405-436" in hdr and "collision_space.cpp:154-156, 285-288" in hdr
    assert "octomaps are" not in hdr                    # no longer among what is refused
    # the struct keeps its layout
    assert C.sizeof(capi.ShapeStruct) == 8 + 24 + 96 + 16 + 16
    hpp = open(os.path.join(ROOT, "include", "smpl_amd", "plugin.hpp")).read()
    assert re.search(r"OCTREE\s*=\s*SMPLX_SHAPE_OCTREE", hpp) and "static Shape OcTree(" in hpp
    gpu = hpp[hpp.index("class GpuCollisionChecker"):]
    gpu = gpu[:gpu.index("\n};")]
    assert re.search(r"virtual\s+bool\s+processOctomapMsg\s*\(\s*const std::string&\s+\w+,\s*const std::vector<double>&\s+\w+,\s*const Pose&\s+\w+\s*\)", gpu)


def _calls():
    L = capi.lib()
    SP = C.POINTER(capi.ShapeStruct)
    ins, mov, vox = L.smplx_world_insert_object, L.smplx_world_move_object, L.smplx_world_voxelize
    ins.argtypes = mov.argtypes = [C.c_void_p, C.c_char_p, SP, C.c_int]
    vox.argtypes = [C.c_void_p, SP, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    return L, ins, mov, vox


def test_bad_octrees_are_refused():
    L, ins, mov, vox = _calls()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below fails on its shapes
    first = (C.c_int32 * 8)()
    cells = (C.c_int32 * 30)()
    nan, inf = float("nan"), float("inf")

    def refused(arr, n):
        for code in (ins(fake, b"a", arr, n), mov(fake, b"a", arr, n), vox(fake, arr, n, cells, 10, first)):
            assert code == E_ARG
            assert L.smplx_last_error().decode() != ""

    bad_rows = [
        [(0.1, 0.2, 0.3, 0.0)], [(0.1, 0.2, 0.3, -0.04)],                                  # size <= 0
        [(nan, 0.2, 0.3, 0.04)], [(0.1, inf, 0.3, 0.04)], [(0.1, 0.2, 0.3, nan)], [(0.1, 0.2, 0.3, inf)],
        [(0.1, 0.2, 1e6, 0.04)], [(-2e6, 0.2, 0.3, 0.04)], [(0.1, 0.2, 0.3, 1e6)],          # |x| >= 1e6
        LEAVES + [(0.1, 0.2, 0.3, 0.0)],                                                   # every leaf is checked
    ]
    for rows in bad_rows:
        arr, n, keep = capi._shape_array([capi.sphere(0.1), capi.octree(rows)])           # the bad one second
        refused(arr, 2)
    for pose in (capi.pose_at((nan, 0, 0)), capi.pose_at((0, 2e6, 0)), capi.pose_at(R=np.full((3, 3), inf))):
        arr, n, keep = capi._shape_array([capi.octree(LEAVES, pose)])
        refused(arr, 1)
    # no leaves: null vertices, nvertices < 1; triangles where none belong
    arr, n, keep = capi._shape_array([capi.octree(LEAVES)])
    arr[0].nvertices = 0
    refused(arr, 1)
    arr[0].nvertices = -3
    refused(arr, 1)
    arr[0].nvertices = 2
    arr[0].vertices = None
    refused(arr, 1)
    arr, n, keep = capi._shape_array([capi.octree(LEAVES)])
    tri = np.zeros(3, np.int32)
    arr[0].triangles = tri.ctypes.data_as(C.POINTER(C.c_int32))
    refused(arr, 1)                                       # a pointer with ntriangles == 0
    arr[0].ntriangles = 1
    refused(arr, 1)
    arr[0].triangles = None
    refused(arr, 1)                                       # ntriangles != 0 without a pointer
    # a box given type 6 has no leaves
    arr, n, keep = capi._shape_array([dict(capi.box((0.1, 0.2, 0.3)), type=6)])
    refused(arr, 1)
    assert "octree" in L.smplx_last_error().decode()
    # the rows never reach the library unless they are n x 4
    with pytest.raises(capi.SmplxError) as e:
        capi.octree([(0.1, 0.2, 0.3)])
    assert e.value.code == E_ARG


def test_a_good_octree_passes_the_argument_checks():
    """insert and move check the shapes first and the grid after them: on a handle that is all zero bytes -- a grid without
    an occupancy array, which is how the library tells a grid from a finished field -- a good octree, alone or beside a box
    (dims are ignored), gets as far as SMPLX_E_STATE, and a bad one is still SMPLX_E_ARG"""
    L, ins, mov, vox = _calls()
    blank = C.create_string_buffer(1 << 16)
    handle = C.cast(blank, C.c_void_p)
    for shapes in ([capi.octree(LEAVES)], [capi.box((0.1, 0.2, 0.3)), capi.octree(LEAVES, capi.pose_at((0.1, 0.0, 0.2)))],
                   [dict(capi.octree(LEAVES), dims=(-1.0, float("nan"), 0.0))]):
        arr, n, keep = capi._shape_array(shapes)
        for f in (ins, mov):
            assert f(handle, b"map", arr, n) == E_STATE
            assert "finished field" in L.smplx_last_error().decode()
    arr, n, keep = capi._shape_array([capi.octree([(0.1, 0.2, 0.3, -1.0)])])
    assert ins(handle, b"map", arr, 1) == E_ARG and mov(handle, b"map", arr, 1) == E_ARG
    assert blank.raw == bytes(1 << 16)                    # nothing was written
