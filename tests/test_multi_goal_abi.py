"""smplx_set_goals_joint_multi / smplx_set_goals_xyz_multi without a GPU: the header declares them, the library exports
them, and bad arguments are refused before any space is touched."""
import ctypes as C
import os
import re

from smpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
_dp = C.POINTER(C.c_double)


def _lib():
    L = capi.lib()
    for name in ["smplx_set_goals_joint_multi", "smplx_set_goals_xyz_multi"]:
        getattr(L, name).argtypes = [C.c_void_p, C.c_int, _dp, _dp]
    return L


def test_header_declares_and_library_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "smpl_amd.h")).read()
    for name, rows in [("smplx_set_goals_joint_multi", "angles"), ("smplx_set_goals_xyz_multi", "xyz")]:
        assert re.search(r"\bint\s+%s\s*\(\s*smplx_space\*\*\s*spaces,\s*int\s+nq,\s*const\s+double\*\s*%s" % (name, rows), hdr), name
        assert hasattr(capi.lib(), name)
        assert name in capi.SYMBOLS
    assert callable(capi.Space.set_goals_joint_multi) and callable(capi.Space.set_goals_xyz_multi)
    # the contract is written down where a C caller reads it
    assert "SHARED sequence" in hdr and "twice" in hdr


def test_bad_arguments_are_refused():
    L = _lib()
    fake = [0x1000, 0x2000]      # never dereferenced: these arguments are checked on the handles alone
    two = (C.c_void_p * 2)(*fake)
    same = (C.c_void_p * 2)(fake[0], fake[0])
    hole = (C.c_void_p * 2)(fake[0], None)
    v = (C.c_double * 32)(*([0.25] * 32))
    for fn in [L.smplx_set_goals_joint_multi, L.smplx_set_goals_xyz_multi]:
        assert fn(None, 1, v, v) == E_ARG               # no array of spaces
        assert fn(two, 0, v, v) == E_ARG                # nq < 1
        assert fn(two, -3, v, v) == E_ARG
        assert fn(hole, 2, v, v) == E_ARG               # a null handle in the array
        assert "null" in L.smplx_last_error().decode()
        assert fn(same, 2, v, v) == E_ARG               # the same space twice
        assert "twice" in L.smplx_last_error().decode()
        assert fn(two, 2, None, v) == E_ARG             # no goals
        assert fn(two, 2, v, None) == E_ARG             # no tolerances
    # a goal position that is not finite: refused before the spaces are looked at (a joint goal's row length is the
    # spaces' number of variables, so its values are checked with the spaces: tests/test_gpu_multi_goal.py)
    for bad in [float("nan"), float("inf"), -float("inf")]:
        for k in range(6):
            xyz = (C.c_double * 6)(0.1, 0.2, 0.3, 0.4, 0.5, 0.6)
            xyz[k] = bad
            assert L.smplx_set_goals_xyz_multi(two, 2, xyz, v) == E_ARG
            assert "finite" in L.smplx_last_error().decode()
