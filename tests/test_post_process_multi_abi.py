"""smplx_post_process_paths without a GPU: the header declares the call and its launch bound, the library exports it, the
Python binding and the C++ mirror name it, bad arguments are refused before any space is touched, and the arithmetic over
the caller's offsets (smpl_amd/csrc/path_multi.h) holds as a program built with the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from smpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1


def test_header_declares_the_call_and_the_constant():
    hdr = open(os.path.join(ROOT, "include", "smpl_amd.h")).read()
    assert re.search(r"\bint\s+smplx_post_process_paths\s*\(\s*smplx_space\s*\*\s*const\s*\*\s*spaces\s*,\s*int\s+nq\s*,", hdr)
    m = re.search(r"#define\s+SMPLX_PP_MULTI_MAX_LAUNCHES\s+(\d+)", hdr)
    assert m and int(m.group(1)) == capi.PP_MULTI_MAX_LAUNCHES
    assert 1 <= capi.PP_MULTI_MAX_LAUNCHES <= 8          # a constant, and a small one: that is the point of the call
    hooks = open(os.path.join(ROOT, "smpl_amd", "csrc", "test_hooks.h")).read()
    assert re.search(r"\bint\s+smplx_test_path_waypoints\s*\(", hooks)


def test_library_exports_and_capi_binds_it():
    L = capi.lib()
    assert hasattr(L, "smplx_post_process_paths") and hasattr(L, "smplx_test_path_waypoints")
    assert "smplx_post_process_paths" in capi.SYMBOLS
    assert callable(capi.post_process_paths) and callable(capi.path_waypoints)


def test_plugin_mirror_declares_post_process_paths():
    hpp = open(os.path.join(ROOT, "include", "smpl_amd", "plugin.hpp")).read()
    assert re.search(r"inline\s+bool\s+PostProcessPaths\s*\(", hpp)
    assert "smplx_post_process_paths(" in hpp[hpp.index("PostProcessPaths"):]


def test_bad_arguments_are_refused_without_a_gpu():
    f = capi._post_process_paths_fn()
    L = capi.lib()
    fake = (C.c_void_p * 2)(0x1000, 0x1000)       # never dereferenced: every call below fails on its other arguments
    null_entry = (C.c_void_p * 2)(None, None)
    q = np.zeros((4, 7))
    first = np.array([0, 2, 4], np.int32)
    of = np.full(3, -7, np.int32)
    _dp, _ip = capi._dp, capi._ip
    pq, pf, po = q.ctypes.data_as(_dp), first.ctypes.data_as(_ip), of.ctypes.data_as(_ip)

    def refused(code):
        assert code == E_ARG
        assert L.smplx_last_error().decode() != ""
        assert (of == -7).all()
    refused(f(None, 2, pq, pf, 7, None, 0, po, None))
    refused(f(fake, -1, pq, pf, 7, None, 0, po, None))
    refused(f(fake, 2, pq, None, 7, None, 0, po, None))
    refused(f(fake, 2, pq, pf, 7, None, 0, None, None))
    refused(f(fake, 2, None, pf, 7, None, 0, po, None))
    refused(f(null_entry, 2, pq, pf, 7, None, 0, po, None))
    for bad in ([0, 3, 2], [1, 2, 4], [0, -1, 4], [0, 2 ** 31 - 1, -2 ** 31]):
        b = np.array(bad, np.int32)
        refused(f(fake, 2, pq, b.ctypes.data_as(_ip), 7, None, 0, po, None))
    # nq == 0 touches nothing and is fine with null arrays
    assert f(None, 0, None, None, 7, None, 0, None, None) == 0
    st = (C.c_int64 * 4)(9, 9, 9, 9)
    assert f(None, 0, None, None, 7, None, 0, po, st) == 0
    assert of[0] == 0 and list(st) == [0, 0, 0, 0]
    assert capi.post_process_paths([], [])[0] == []


def test_offset_arithmetic_as_a_sanitized_program(tmp_path):
    """tests/cpp/path_multi_host_driver.cpp: decreasing offsets, first[0] != 0, offsets that wrapped past INT_MAX, output
    sums at and beyond INT_MAX, the size bound in 64 bits, the block table"""
    exe = str(tmp_path / "path_multi_host_driver")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "tests", "cpp", "fake_hip"),
                           os.path.join(ROOT, "tests", "cpp", "path_multi_host_driver.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
