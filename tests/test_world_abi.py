"""The world-object entry points (include/smpl_amd.h "world objects") without a GPU: the header
declares them, the library exports them, the Python binding and the C++ mirror name them, bad arguments are refused
before any grid is touched, and formats.env_objects turns a scene file into box objects.  What needs a grid -- duplicate
and unknown ids, a grid from a finished field -- is in tests/test_gpu_world_objects.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from smpl_amd import capi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NEW = ["smplx_world_insert_object", "smplx_world_remove_object", "smplx_world_move_object", "smplx_world_remove_all",
       "smplx_world_objects", "smplx_world_object_cells", "smplx_world_voxelize"]


def test_header_declares_and_library_exports_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "smpl_amd.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    for name, value in (("BOX", 1), ("SPHERE", 2), ("CYLINDER", 3), ("CONE", 4), ("MESH", 5)):
        assert re.search(r"SMPLX_SHAPE_%s\s*=\s*%d\b" % (name, value), hdr) and getattr(capi, "SHAPE_" + name) == value
    assert re.search(r"typedef\s+struct\s*\{[^}]*int32_t\s+type;[^}]*double\s+dims\[3\];[^}]*double\s+pose\[12\];[^}]*\}\s*smplx_shape;", hdr)
    for m in ("insert_object", "remove_object", "move_object", "remove_all_objects", "objects", "object_cells", "voxelize"):
        assert callable(getattr(capi.Grid, m)), m
    for f in ("box", "sphere", "cylinder", "cone", "mesh"):
        assert callable(getattr(capi, f)), f
    # the calls cite the reference lines they stand behind
    assert "collision_space.cpp:228-275" in hdr and "world_collision_model.cpp:193-280" in hdr and "voxelize.hpp:46-180" in hdr
    # the ctypes mirror of smplx_shape has the C layout: int32, 3 + 12 doubles, (pointer, int32) twice
    assert C.sizeof(capi.ShapeStruct) == 8 + 24 + 96 + 16 + 16
    assert capi.ShapeStruct.dims.offset == 8 and capi.ShapeStruct.vertices.offset == 128 and capi.ShapeStruct.ntriangles.offset == 152


def test_plugin_mirror_declares_the_virtuals():
    hpp = open(os.path.join(ROOT, "include", "smpl_amd", "plugin.hpp")).read()
    assert re.search(r"struct\s+CollisionObject\s*\{[^}]*std::string\s+id;[^}]*shapes;[^}]*shape_poses;", hpp)
    assert re.search(r"struct\s+Shape\s*\{", hpp)
    gpu = hpp[hpp.index("class GpuCollisionChecker"):]
    gpu = gpu[:gpu.index("\n};")]
    for name, arg in (("insertObject", "const CollisionObject&"), ("removeObject", "const CollisionObject&"),
                      ("removeObject", "const std::string&"), ("moveShapes", "const CollisionObject&"),
                      ("insertShapes", "const CollisionObject&"), ("removeShapes", "const CollisionObject&")):
        assert re.search(r"virtual\s+bool\s+%s\s*\(\s*%s\s+\w+\s*\)" % (name, re.escape(arg)), gpu), (name, arg)
    for call in ("smplx_world_insert_object(", "smplx_world_remove_object(", "smplx_world_move_object("):
        assert call in gpu, call
    assert "smplx_grid_create_empty(" in hpp[hpp.index("class GpuPlanningContext"):hpp.index("class GpuRobotModel")]


def _refused(code):
    assert code == E_ARG
    assert capi.lib().smplx_last_error().decode() != ""


def _shapes(*specs):
    arr, n, keep = capi._shape_array(specs)
    return arr, n, keep


def test_bad_arguments_are_refused():
    L = capi.lib()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below fails on its other arguments
    SP = C.POINTER(capi.ShapeStruct)
    ins, mov, rem, ra, obj, oc, vox = (L.smplx_world_insert_object, L.smplx_world_move_object, L.smplx_world_remove_object,
                                       L.smplx_world_remove_all, L.smplx_world_objects, L.smplx_world_object_cells, L.smplx_world_voxelize)
    ins.argtypes = mov.argtypes = [C.c_void_p, C.c_char_p, SP, C.c_int]
    rem.argtypes = [C.c_void_p, C.c_char_p]
    ra.argtypes = [C.c_void_p]
    obj.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p]
    oc.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    vox.argtypes = [C.c_void_p, SP, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    good, n, _ = _shapes(capi.box((0.1, 0.2, 0.3)))
    first = (C.c_int32 * 8)()
    cells = (C.c_int32 * 30)()
    cnt = C.c_int(7)
    buf = C.create_string_buffer(16)
    for f in (ins, mov):
        _refused(f(None, b"a", good, 1))
        _refused(f(fake, None, good, 1))
        _refused(f(fake, b"", good, 1))
        _refused(f(fake, b"two\nlines", good, 1))
        _refused(f(fake, b"a", None, 1))
        _refused(f(fake, b"a", good, 0))          # an empty shape list
        _refused(f(fake, b"a", good, -1))
    _refused(rem(None, b"a"))
    _refused(rem(fake, None))
    _refused(rem(fake, b""))
    _refused(ra(None))
    _refused(obj(None, buf, 16, C.byref(cnt)))
    assert cnt.value == 0
    _refused(obj(fake, buf, 16, None))
    _refused(obj(fake, None, 16, C.byref(cnt)))
    _refused(obj(fake, buf, -1, C.byref(cnt)))
    cnt.value = 7
    _refused(oc(None, b"a", 0, cells, 10, C.byref(cnt)))
    assert cnt.value == 0
    _refused(oc(fake, None, 0, cells, 10, C.byref(cnt)))
    _refused(oc(fake, b"a", 0, cells, 10, None))
    _refused(oc(fake, b"a", 0, None, 10, C.byref(cnt)))
    _refused(oc(fake, b"a", 0, cells, -1, C.byref(cnt)))
    _refused(vox(None, good, 1, cells, 10, first))
    _refused(vox(fake, None, 1, cells, 10, first))
    _refused(vox(fake, good, 0, cells, 10, first))
    _refused(vox(fake, good, 1, None, 10, first))
    _refused(vox(fake, good, 1, cells, -1, first))
    _refused(vox(fake, good, 1, cells, 10, None))
    # the shapes themselves: every entry point that takes them refuses them the same way
    nan, inf = float("nan"), float("inf")
    tri_v, tri_t = [(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 2)]
    bad = [
        dict(capi.box((0.1, 0.2, 0.3)), type=0),                      # unknown type
        dict(capi.box((0.1, 0.2, 0.3)), type=6),                      # a plane / octomap would be next: not supported
        capi.box((0.1, 0.0, 0.3)), capi.box((0.1, 0.2, -0.3)), capi.box((nan, 0.2, 0.3)), capi.box((inf, 0.2, 0.3)),
        capi.sphere(0.0), capi.sphere(-1.0), capi.sphere(nan),
        capi.cylinder(0.1, 0.0), capi.cylinder(0.0, 0.1), capi.cone(0.1, -0.2), capi.cone(inf, 0.2),
        capi.box((0.1, 0.2, 0.3), capi.pose_at((nan, 0, 0))), capi.sphere(0.1, capi.pose_at((0, 2e6, 0))),
        capi.sphere(0.1, capi.pose_at(R=np.full((3, 3), inf))),
        capi.mesh(tri_v, [(0, 1, 3)]), capi.mesh(tri_v, [(0, -1, 2)]), capi.mesh([(0, 0, 0), (nan, 0, 0), (0, 1, 0)], tri_t),
        capi.mesh([(0, 0, 0), (1e7, 0, 0), (0, 1, 0)], tri_t),
    ]
    for s in bad:
        arr, n, keep = _shapes(capi.sphere(0.1), s)        # the bad one second: all shapes are checked
        _refused(ins(fake, b"a", arr, 2))
        _refused(mov(fake, b"a", arr, 2))
        _refused(vox(fake, arr, 2, cells, 10, first))
    # a mesh without vertices or triangles
    arr, n, keep = _shapes(capi.mesh(tri_v, tri_t))
    arr[0].ntriangles = 0
    _refused(vox(fake, arr, 1, cells, 10, first))
    arr[0].ntriangles = 1
    arr[0].vertices = None
    _refused(ins(fake, b"a", arr, 1))
    # a triangle list whose length is no multiple of 3 never reaches the library
    with pytest.raises(capi.SmplxError) as e:
        capi.mesh(tri_v, [0, 1, 2, 0])
    assert e.value.code == E_ARG


def test_env_objects_of_the_tabletop_scene():
    text = open(os.path.join(ROOT, "tests", "golden", "tabletop.env")).read()
    objs = formats.env_objects(text)
    rows = formats.parse_env(text)
    assert [name for name, _ in objs] == [r[0] for r in rows] == ["tabletop"]
    for (name, shapes), (_, centre, size) in zip(objs, rows):
        assert len(shapes) == 1 and shapes[0]["type"] == capi.SHAPE_BOX and shapes[0]["dims"] == tuple(size)
        P = np.asarray(shapes[0]["pose"])
        assert np.array_equal(P[:, :3], np.eye(3)) and tuple(P[:, 3]) == tuple(centre)
    assert objs[0][1][0]["dims"] == (0.4, 1.5, 0.02) and tuple(objs[0][1][0]["pose"][:, 3]) == (0.55, 0.0, 0.6)
    # rows that share a name get distinct ids, in file order
    two = formats.env_objects("2\nbox 0 0 0 1 1 1\nbox 1 0 0 1 1 1\n")
    assert [n for n, _ in two] == ["box", "box#1"]
    # what it returns is what insert_object marshals
    arr, n, keep = capi._shape_array(objs[0][1])
    assert n == 1 and arr[0].type == 1 and list(arr[0].dims) == [0.4, 1.5, 0.02] and arr[0].pose[3] == 0.55
