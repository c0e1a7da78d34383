"""The lazy successor entry points (GetLazySuccs / GetTrueCost) without a GPU: the header declares
them, the library exports them, the Python binding and the C++ mirror name them, and bad arguments are refused before any
space is touched.  What needs a space -- no goal, the goal id as a parent, unknown ids, a grid edited after the goal -- is
in tests/test_gpu_lazy.py (a space cannot be created without a device)."""
import ctypes as C
import os
import re

from smpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NEW = ["smplx_get_lazy_succs", "smplx_get_true_cost", "smplx_true_cost_batch", "smplx_lazy_expand_batch",
       "smplx_lazy_expand_batch_device", "smplx_true_cost_q_batch", "smplx_true_cost_q_batch_device", "smplx_lazy_counters"]
SIZES = ["smplx_true_cost_work_doubles"]


def test_header_declares_and_library_exports_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "smpl_amd.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    for name in SIZES:
        assert re.search(r"\bsize_t\s+%s\s*\(" % name, hdr) and hasattr(L, name) and name in capi.SYMBOLS, name
    for m in ("get_lazy_succs", "get_true_cost", "true_cost_batch", "lazy_expand_batch", "lazy_expand_batch_device",
              "true_cost_q_batch", "true_cost_q_batch_device", "lazy_counters"):
        assert callable(getattr(capi.Space, m)), m
    # each call cites the reference lines it stands behind
    assert "manip_lattice.cpp:1012-1090" in hdr and "manip_lattice.cpp:1094-1167" in hdr and "robot_planning_space.h:124-130" in hdr


def test_plugin_mirror_declares_both_virtuals_and_their_overrides():
    hpp = open(os.path.join(ROOT, "include", "smpl_amd", "plugin.hpp")).read()
    base = hpp[hpp.index("class RobotPlanningSpace : public virtual Extension"):hpp.index("class GpuManipLattice")]
    assert re.search(r"virtual\s+void\s+GetLazySuccs\s*\(\s*int\s+\w+\s*,\s*std::vector<int>\*\s*\w+\s*,\s*std::vector<int>\*\s*\w+\s*,"
                     r"\s*std::vector<bool>\*\s*\w+\s*\)", base)
    assert re.search(r"virtual\s+int\s+GetTrueCost\s*\(\s*int\s+\w+\s*,\s*int\s+\w+\s*\)", base)
    # the defaults are GetSuccs with all-true costs (robot_planning_space.cpp:182-200)
    assert "true_costs->assign(succs->size(), true);" in base
    gpu = hpp[hpp.index("class GpuManipLattice"):]
    gpu = gpu[:gpu.index("\n};")]
    assert re.search(r"void\s+GetLazySuccs\s*\([^)]*\)\s*override", gpu) and "smplx_get_lazy_succs(" in gpu
    assert re.search(r"int\s+GetTrueCost\s*\([^)]*\)\s*override", gpu) and "smplx_get_true_cost(" in gpu
    assert "smplx_true_cost_batch(" in gpu


def _refused(code):
    assert code == E_ARG
    assert capi.lib().smplx_last_error().decode() != ""


def test_bad_arguments_are_refused():
    L = capi.lib()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below fails on its other arguments
    q = (C.c_double * 16)(*([0.1] * 16))
    ids = (C.c_int32 * 4)(1, 1, 1, 1)
    out = (C.c_int32 * 64)()
    fl = (C.c_uint8 * 64)()
    n = C.c_int(7)
    ls, tc, tb = L.smplx_get_lazy_succs, L.smplx_get_true_cost, L.smplx_true_cost_batch
    le, led, tq, tqd, ctr = (L.smplx_lazy_expand_batch, L.smplx_lazy_expand_batch_device, L.smplx_true_cost_q_batch,
                             L.smplx_true_cost_q_batch_device, L.smplx_lazy_counters)
    ls.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    tc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    tb.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    le.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    led.argtypes = [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
    tq.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    tqd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
    ctr.argtypes = [C.c_void_p, C.c_void_p]
    _refused(ls(None, 1, out, out, 4, C.byref(n)))
    _refused(ls(fake, 1, out, out, 4, None))
    _refused(tc(None, 1, 2, out))
    _refused(tc(fake, 1, 2, None))
    _refused(tb(None, ids, ids, 1, out, None, None))
    _refused(tb(fake, None, ids, 1, out, None, None))
    _refused(tb(fake, ids, None, 1, out, None, None))
    _refused(tb(fake, ids, ids, 1, None, None, None))
    _refused(tb(fake, ids, ids, -1, out, None, None))
    _refused(le(None, q, 1, fl, None, None, None, None))
    _refused(le(fake, None, 1, fl, None, None, None, None))
    _refused(le(fake, q, -1, fl, None, None, None, None))
    _refused(led(None, q, 1, fl, None, None, None, None, None))
    _refused(led(fake, None, 1, fl, None, None, None, None, None))
    _refused(led(fake, q, 1, None, None, None, None, None, None))
    _refused(led(fake, q, 0, fl, None, None, None, None, None))
    _refused(tq(None, q, ids, fl, 1, out, None, None))
    _refused(tq(fake, None, ids, fl, 1, out, None, None))
    _refused(tq(fake, q, None, fl, 1, out, None, None))
    _refused(tq(fake, q, ids, fl, 1, None, None, None))
    _refused(tq(fake, q, ids, fl, -1, out, None, None))
    _refused(tqd(None, q, ids, fl, 1, q, out, None, None, None))
    _refused(tqd(fake, q, ids, fl, 1, None, out, None, None, None))
    _refused(tqd(fake, q, ids, fl, 1, q, None, None, None, None))
    _refused(tqd(fake, q, ids, fl, 0, q, out, None, None, None))
    _refused(ctr(None, out))
    _refused(ctr(fake, None))
    # a refused GetLazySuccs leaves an empty list behind
    n.value = 7
    _refused(ls(None, 1, out, out, 4, C.byref(n)))
    assert n.value == 0
    cost = C.c_int32(5)
    _refused(tc(None, 1, 2, C.byref(cost)))
    assert cost.value == -1
    # n == 0 touches nothing, the space included
    assert tb(fake, None, None, 0, None, None, None) == 0
    assert le(fake, q, 0, None, None, None, None, None) == 0
    assert tq(fake, None, None, None, 0, None, None, None) == 0
