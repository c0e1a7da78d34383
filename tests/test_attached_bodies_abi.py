"""The attached-body entry points of the C-ABI (smplx_attach_body and its kin, include/smpl_amd.h) without a GPU: the C++
side (GpuCollisionChecker::attachObject / detachObject in include/smpl_amd/plugin.hpp) compiles warning-free, and bad
arguments are refused before anything touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np

from smpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def test_plugin_attach_compiles_warning_free(tmp_path):
    src = tmp_path / "attach.cpp"
    src.write_text('#include "smpl_amd/plugin.hpp"\n'
                   "using namespace smpl_amd;\n"
                   "bool f(GpuCollisionChecker& cc) {\n"
                   "    std::vector<std::array<double, 4>> sp{{0.1, 0.0, 0.0, 0.02}, {0.12, 0.0, 0.0, 0.02}};\n"
                   "    bool ok = cc.attachObject(\"box\", sp, \"gripper_palm_link\", {\"gripper_palm_link\"});\n"
                   "    ok = cc.attachObject(\"box2\", sp, \"gripper_palm_link\") && ok;\n"
                   "    return cc.detachObject(\"box\") && ok;\n"
                   "}\n")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", INC, str(src)])


def test_bad_arguments_are_refused():
    L = capi.lib()
    L.smplx_attach_body.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_int,
                                    C.POINTER(C.c_char_p), C.c_int]
    L.smplx_detach_body.argtypes = [C.c_void_p, C.c_char_p]
    L.smplx_attached_bodies.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
    L.smplx_attached_nodes.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.smplx_cc_attached_positions.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]
    sp = (C.c_double * 4)(0.1, 0.0, 0.0, 0.02)
    fake = C.c_void_p(1)    # never dereferenced: every call below fails its argument check first
    assert L.smplx_attach_body(None, b"box", b"link", sp, 1, None, 0) == -1
    assert L.smplx_attach_body(fake, None, b"link", sp, 1, None, 0) == -1
    assert L.smplx_attach_body(fake, b"box", None, sp, 1, None, 0) == -1
    assert L.smplx_attach_body(fake, b"box", b"link", None, 1, None, 0) == -1
    assert L.smplx_attach_body(fake, b"box", b"link", sp, 0, None, 0) == -1
    assert L.smplx_attach_body(fake, b"box", b"link", sp, 1, None, 2) == -1      # allowed names missing
    assert L.smplx_detach_body(None, b"box") == -1
    assert L.smplx_detach_body(fake, None) == -1
    assert L.smplx_attached_bodies(None, None, 0, None, None) == -1
    assert L.smplx_attached_nodes(None, None, None, None) == -1
    out = (C.c_double * 3)()
    assert L.smplx_cc_attached_positions(None, sp, 1, out) == -1
    assert L.smplx_cc_attached_positions(fake, None, 1, out) == -1
    assert L.smplx_cc_attached_positions(fake, sp, -1, out) == -1
    assert b"bad argument" in L.smplx_last_error()


def test_box_spheres():
    from smpl_amd import formats
    b = formats.box_spheres((0.2, 0.0, 0.0), (0.06, 0.06, 0.12), 0.0177, 0.025)
    assert b.shape == (200, 4) and (b[:, 3] == 0.025).all()
    assert np.allclose(b[:, :3].min(0), (0.17, -0.03, -0.06)) and np.allclose(b[:, :3].max(0), (0.23, 0.03, 0.06))
    flat = formats.box_spheres((0.0, 0.0, 0.1), (0.04, 0.04, 0.0), 0.02, 0.01)     # a plate: one layer
    assert flat.shape == (9, 4) and (flat[:, 2] == 0.1).all()
