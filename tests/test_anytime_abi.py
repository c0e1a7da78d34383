"""The anytime ARA* entry points of the C-ABI (smplx_replan / smplx_replan_multi, include/smpl_amd.h) without a GPU: the
structs' layout as a C compiler sees it equals the ctypes layout of smpl_amd/capi.py, the C++ facade (GpuARAStar in
include/smpl_amd/plugin.hpp) compiles warning-free, and bad arguments are refused before anything touches a device."""
import ctypes as C
import os
import subprocess

import pytest

from smpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "smpl_amd.h"
#define F(T, f) printf(#T " " #f " %zu\n", offsetof(T, f))
int main(void) {
    printf("smplx_time_params size %zu\n", sizeof(smplx_time_params));
    printf("smplx_replan_stats size %zu\n", sizeof(smplx_replan_stats));
    F(smplx_time_params, initial_eps); F(smplx_time_params, final_eps); F(smplx_time_params, delta_eps);
    F(smplx_time_params, improve); F(smplx_time_params, bounded); F(smplx_time_params, type);
    F(smplx_time_params, max_expansions_init); F(smplx_time_params, max_expansions);
    F(smplx_time_params, max_seconds_init); F(smplx_time_params, max_seconds);
    F(smplx_time_params, allow_partial); F(smplx_time_params, from_scratch);
    F(smplx_replan_stats, s); F(smplx_replan_stats, result); F(smplx_replan_stats, call_expansions);
    F(smplx_replan_stats, resumed); F(smplx_replan_stats, pad);
    printf("enum %d %d %d %d %d %d\n", SMPLX_TIME_EXPANSIONS, SMPLX_TIME_WALL, SMPLX_ARA_SUCCESS, SMPLX_ARA_PARTIAL,
           SMPLX_ARA_TIMED_OUT, SMPLX_ARA_EXHAUSTED);
    return 0;
}
"""


def test_struct_layouts_match_ctypes(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    want = {"smplx_time_params": capi.TimeParams, "smplx_replan_stats": capi.ReplanStats}
    seen = 0
    for ln in lines:
        parts = ln.split()
        if parts[0] == "enum":
            assert [int(x) for x in parts[1:]] == [capi.TIME_EXPANSIONS, capi.TIME_WALL, capi.ARA_SUCCESS, capi.ARA_PARTIAL,
                                                    capi.ARA_TIMED_OUT, capi.ARA_EXHAUSTED]
            continue
        T, f, v = parts[0], parts[1], int(parts[2])
        if f == "size":
            assert C.sizeof(want[T]) == v, T
        else:
            assert getattr(want[T], f).offset == v, (T, f)
        seen += 1
    assert seen == 2 + 12 + 5


def test_plugin_facade_compiles_warning_free(tmp_path):
    src = tmp_path / "facade.cpp"
    src.write_text('#include "smpl_amd/plugin.hpp"\n'
                   'int use(smpl_amd::GpuPlanningContext* c) {\n'
                   '    smpl_amd::GpuARAStar s(c);\n'
                   '    s.setTargetEpsilon(1.0); s.setDeltaEpsilon(1.0); s.setImproveSolution(true); s.setBoundExpansions(true);\n'
                   '    s.allowPartialSolutions(true); s.setAllowedRepairTime(0.5); s.set_initialsolution_eps(5.0);\n'
                   '    s.set_search_mode(false); s.force_planning_from_scratch(); s.force_planning_from_scratch_and_free_memory();\n'
                   '    std::vector<int> path; int cost = 0;\n'
                   '    smpl_amd::GpuARAStar::TimeParameters tp; tp.type = smpl_amd::GpuARAStar::TimeParameters::EXPANSIONS;\n'
                   '    int r = s.replan(tp, &path, &cost) + s.replan(0.1, &path) + s.replan(0.1, &path, &cost);\n'
                   '    return r + s.get_n_expands() + s.get_n_expands_init_solution() + (int)s.get_solution_eps()\n'
                   '           + (int)s.get_initial_eps() + (int)s.get_final_epsilon();\n'
                   '}\n')
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", INC, str(src)])


def _replan(h, p, cap=16, stats=True):
    L = capi.lib()
    ids = (C.c_int32 * max(cap, 1))()
    st = capi.ReplanStats()
    return L.smplx_replan(h, C.byref(p) if p is not None else None, ids, cap, C.byref(st) if stats else None)


def _replan_multi(hs, nq, p, cap=16, stats=True):
    L = capi.lib()
    ids = (C.c_int32 * max(cap * max(nq, 1), 1))()
    st = (capi.ReplanStats * max(nq, 1))()
    wall = C.c_double()
    return L.smplx_replan_multi(hs, nq, C.byref(p) if p is not None else None, ids, cap, st if stats else None, C.byref(wall), 1)


def test_bad_arguments_are_refused():
    E_ARG = -1
    L = capi.lib()
    L.smplx_replan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    L.smplx_replan_multi.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    good = capi.time_params(5.0, 1.0, 1.0, True, True, 100, 100)
    assert _replan(None, good) == E_ARG
    fake = C.c_void_p(0x1000)      # never dereferenced: the parameters are checked first
    assert _replan(fake, None) == E_ARG
    assert _replan(fake, good, stats=False) == E_ARG
    assert _replan(fake, good, cap=0) == E_ARG
    for bad in [capi.time_params(5.0, 1.0, 1.0, wall=True, bounded=True, seconds_init=-1.0, seconds=1.0),
                capi.time_params(5.0, 1.0, 1.0, wall=True, bounded=True, seconds_init=float("nan"), seconds=1.0),
                capi.time_params(0.5, 1.0, 1.0), capi.time_params(5.0, 1.0, 0.0), capi.time_params(float("inf"), 1.0, 1.0)]:
        assert _replan(fake, bad) == E_ARG
    t = capi.time_params(5.0, 1.0, 1.0)
    t.type = 7
    assert _replan(fake, t) == E_ARG
    assert "timing type" in L.smplx_last_error().decode()
    hs = (C.c_void_p * 2)(fake.value, fake.value)
    assert _replan_multi(None, 1, good) == E_ARG
    assert _replan_multi(hs, 0, good) == E_ARG
    assert _replan_multi(hs, 1, None) == E_ARG
    assert _replan_multi(hs, 1, good, stats=False) == E_ARG
    assert _replan_multi(hs, 2, good) == E_ARG          # the same space twice
    assert "twice" in L.smplx_last_error().decode()
