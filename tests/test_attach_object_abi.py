"""Attaching objects by shape (smplx_attach_object / smplx_object_spheres, include/smpl_amd.h) without a GPU: the symbols
exist, the C++ mirror compiles warning-free, bad arguments are refused before anything touches a device, and the host
side of the sphere model's lattice (smpl_amd/csrc/object_spheres.h over voxelize.h, built by the host compiler into a
program of its own, with the address and undefined-behaviour sanitizers where the compiler has their runtime) gives the
judge's rows for every input of tests/object_cases.py, bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import object_cases as OC
import voxelize_ref as V
from smpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_symbols_exist():
    L = capi.lib()
    for name in ("smplx_attach_object", "smplx_object_spheres"):
        assert name in capi.SYMBOLS and hasattr(L, name)
    assert capi.ATTACHED_SPHERE_RADIUS == 0.025
    text = open(os.path.join(INC, "smpl_amd.h")).read()
    assert "#define SMPLX_ATTACHED_SPHERE_RADIUS 0.025" in text
    assert hasattr(capi.Space, "attach_object") and hasattr(capi.Space, "object_spheres")


def test_plugin_attach_object_compiles_warning_free(tmp_path):
    src = tmp_path / "attach_object.cpp"
    src.write_text('#include "smpl_amd/plugin.hpp"\n'
                   "using namespace smpl_amd;\n"
                   "bool f(GpuCollisionChecker& cc) {\n"
                   "    std::vector<Shape> shapes{Shape::Box(0.06, 0.04, 0.10)};\n"
                   "    std::vector<Pose> poses{PoseAt(0.25, 0.0, 0.0)};\n"
                   "    bool ok = cc.attachObject(\"box\", shapes, poses, \"gripper_palm_link\");\n"
                   "    ok = cc.attachObject(\"box2\", shapes, poses, \"gripper_palm_link\", {\"gripper_palm_link\"}) && ok;\n"
                   "    std::vector<std::array<double, 4>> sp{{0.1, 0.0, 0.0, 0.02}};\n"
                   "    ok = cc.attachObject(\"box3\", sp, \"gripper_palm_link\") && ok;      // the sphere overload stays\n"
                   "    AttachedCollisionObject ao;\n"
                   "    ao.object.id = \"held\"; ao.object.shapes = shapes; ao.object.shape_poses = poses;\n"
                   "    ao.link_name = \"gripper_palm_link\"; ao.touch_links = {\"gripper_palm_link\"};\n"
                   "    ao.operation = AttachedCollisionObject::ADD;\n"
                   "    ok = cc.processAttachedCollisionObject(ao) && ok;\n"
                   "    ao.operation = AttachedCollisionObject::MOVE;\n"
                   "    ok = !cc.processAttachedCollisionObject(ao) && ok;\n"
                   "    ao.operation = AttachedCollisionObject::REMOVE;\n"
                   "    return cc.processAttachedCollisionObject(ao) && cc.detachObject(\"box\") && ok;\n"
                   "}\n"
                   "static_assert(SMPLX_ATTACHED_SPHERE_RADIUS == 0.025, \"the reference's radius\");\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INC, str(src)])


def test_bad_arguments_are_refused():
    L = capi.lib()
    L.smplx_attach_object.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(capi.ShapeStruct), C.c_int, C.c_double,
                                      C.POINTER(C.c_char_p), C.c_int]
    L.smplx_object_spheres.argtypes = [C.c_void_p, C.POINTER(capi.ShapeStruct), C.c_int, C.c_double, C.POINTER(C.c_double),
                                       C.c_int, C.POINTER(C.c_int32)]
    arr, n, keep = capi._shape_array([capi.box((0.06, 0.04, 0.10), capi.pose_at((0.25, 0.0, 0.0)))])
    fake = C.c_void_p(1)    # never dereferenced: every call below fails its argument check first
    r = 0.025
    assert L.smplx_attach_object(None, b"box", b"link", arr, 1, r, None, 0) == -1
    assert L.smplx_attach_object(fake, None, b"link", arr, 1, r, None, 0) == -1
    assert L.smplx_attach_object(fake, b"box", None, arr, 1, r, None, 0) == -1
    assert L.smplx_attach_object(fake, b"box", b"link", None, 1, r, None, 0) == -1
    assert L.smplx_attach_object(fake, b"box", b"link", arr, 0, r, None, 0) == -1
    assert L.smplx_attach_object(fake, b"box", b"link", arr, 1, r, None, 2) == -1      # allowed names missing
    assert L.smplx_attach_object(fake, b"box", b"link", arr, 1, r, None, -1) == -1
    first = (C.c_int32 * 2)()
    rows = (C.c_double * 4)()
    assert L.smplx_object_spheres(None, arr, 1, r, None, 0, first) == -1
    assert L.smplx_object_spheres(fake, None, 1, r, None, 0, first) == -1
    assert L.smplx_object_spheres(fake, arr, 0, r, None, 0, first) == -1
    assert L.smplx_object_spheres(fake, arr, 1, r, None, 0, None) == -1
    assert L.smplx_object_spheres(fake, arr, 1, r, rows, -1, first) == -1
    assert L.smplx_object_spheres(fake, arr, 1, r, None, 1, first) == -1                # a capacity without a buffer
    assert b"bad argument" in L.smplx_last_error()


# ---- the judge on the sphere model's lattice: the figures of the issue ----------------------------------------------

@pytest.mark.parametrize("key", list(OC.CASES))
def test_judge_counts_and_inputs_are_decided(key):
    cells, rows, undecided = OC.judged(key)
    assert undecided == 0                      # a condition on the inputs: no cell is too close to a comparison to call
    assert len(cells) == OC.CASES[key][1]
    assert rows.shape == (len(cells), 4) and (rows[:, 3] == OC.RADIUS).all()
    if key in OC.RANGES:
        v, _ = V.shape_mesh(OC.shape(key))
        mn, mx = v.min(0), v.max(0)
        lo = tuple(V.discretize(mn[a], 0.0, OC.RES) for a in range(3))
        hi = tuple(V.discretize(mn[a] + (mx[a] - mn[a]), 0.0, OC.RES) for a in range(3))
        assert (lo, hi) == OC.RANGES[key]
        assert (cells.min(0) >= lo).all() and (cells.max(0) <= hi).all()
    if key in ("box", "cyl"):
        assert (cells < 0).any()               # negative indices are covered


def test_pair_shares_cells():
    rows, first = OC.judged_rows(["box", "cyl"])
    assert list(first) == [0, 122, 272]
    a = set(map(tuple, OC.judged("box")[0])) & set(map(tuple, OC.judged("cyl")[0]))
    assert len(a) > 0                          # a cell filled by both shapes: two rows


# ---- the host side, compiled on its own -----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host_driver(tmp_path_factory):
    """(program, built with sanitizers?)"""
    d = tmp_path_factory.mktemp("objsph")
    exe = str(d / "object_spheres_host_driver")
    src = os.path.join(ROOT, "tests", "cpp", "object_spheres_host_driver.cpp")
    base = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", src, "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = d / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    has_runtime = subprocess.run(["g++"] + san + [str(probe), "-o", str(d / "probe")], capture_output=True).returncode == 0
    subprocess.check_call(base + (san if has_runtime else []))
    return exe, has_runtime


def _driver_input(keys, radius=OC.RADIUS):
    words = [float(radius).hex(), str(len(keys))]
    for k in keys:
        v, t = V.shape_mesh(OC.shape(k) if isinstance(k, str) else k)
        words += [str(len(v)), str(len(t))] + [float(x).hex() for p in v for x in p] + [str(int(i)) for tri in t for i in tri]
    return " ".join(words)


def _run_driver(exe, text):
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    shapes, lines = [], out.stdout.splitlines()
    i = 0
    while i < len(lines):
        w = lines[i].split()
        assert w[0] == "shape" and int(w[1]) == len(shapes)
        n = int(w[2])
        rows = np.array([[float.fromhex(x) for x in l.split()] for l in lines[i + 1:i + 1 + n]]).reshape(-1, 4)
        shapes.append((rows, tuple(int(x) for x in w[3:6]), tuple(int(x) for x in w[6:9])))
        i += 1 + n
    return shapes


@pytest.mark.parametrize("key", list(OC.CASES))
def test_host_rows_equal_the_judge(host_driver, key):
    exe, _ = host_driver
    cells, want, undecided = OC.judged(key)
    assert undecided == 0
    (rows, lo, hi), = _run_driver(exe, _driver_input([key]))
    assert len(rows) == OC.CASES[key][1]
    assert OC.same_bits(rows, want)
    if key in OC.RANGES:
        assert (lo, hi) == OC.RANGES[key]


def test_host_pair_and_degenerate(host_driver):
    exe, _ = host_driver
    got = _run_driver(exe, _driver_input(["box", "cyl", OC.DEGENERATE]))
    want, first = OC.judged_rows(["box", "cyl"])
    assert [len(g[0]) for g in got] == [122, 150, 0]
    assert OC.same_bits(np.vstack([got[0][0], got[1][0]]), want)
