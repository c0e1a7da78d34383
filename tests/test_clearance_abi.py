"""The clearance entry points (distance to collision) without a GPU: the header declares them, the
library exports them, the Python binding and the C++ mirror name them, and bad arguments are refused before any space is
touched."""
import ctypes as C
import os
import re

from smpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NEW = ["smplx_cc_state_clearance_batch", "smplx_cc_state_clearance_batch_device", "smplx_cc_edge_clearance_batch"]


def test_header_declares_and_library_exports_the_three_symbols():
    hdr = open(os.path.join(ROOT, "include", "smpl_amd.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    for m in ("state_clearance_batch", "state_clearance_batch_device", "edge_clearance_batch"):
        assert callable(getattr(capi.Space, m)), m


def test_plugin_mirror_declares_the_extension():
    hpp = open(os.path.join(ROOT, "include", "smpl_amd", "plugin.hpp")).read()
    assert re.search(r"class\s+CollisionDistanceExtension\s*:\s*public\s+virtual\s+Extension", hpp)
    ext = hpp[hpp.index("class CollisionDistanceExtension"):]
    ext = ext[:ext.index("};")]
    assert re.search(r"virtual\s+double\s+distanceToCollision\s*\(\s*const\s+RobotState&\s*\w*\s*\)\s*=\s*0", ext)
    assert re.search(r"virtual\s+double\s+distanceToCollision\s*\(\s*const\s+RobotState&\s*\w*\s*,\s*const\s+RobotState&\s*\w*\s*\)\s*=\s*0", ext)
    gpu = hpp[hpp.index("class GpuCollisionChecker"):]
    gpu = gpu[:gpu.index("\n};")]
    assert "public CollisionDistanceExtension" in gpu.splitlines()[0]
    assert len(re.findall(r"double\s+distanceToCollision\s*\([^)]*\)\s*override", gpu)) == 2
    assert len(re.findall(r"bool\s+distancesToCollision\s*\(", gpu)) == 2
    assert "GetClassCode<CollisionDistanceExtension>()" in gpu
    # isStateValid(state, dist) answers what it always did
    assert "distToObst = std::numeric_limits<double>::max();" in gpu


def _refused(code):
    assert code == E_ARG
    assert capi.lib().smplx_last_error().decode() != ""


def test_bad_arguments_are_refused():
    L = capi.lib()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below fails on its other arguments
    q = (C.c_double * 16)(*([0.1] * 16))
    out = (C.c_double * 4)()
    st, dv, ed = L.smplx_cc_state_clearance_batch, L.smplx_cc_state_clearance_batch_device, L.smplx_cc_edge_clearance_batch
    st.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    dv.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    ed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    _refused(st(None, q, 1, out, None, None))
    _refused(st(fake, None, 1, out, None, None))
    _refused(st(fake, q, 1, None, None, None))
    _refused(st(fake, q, -1, out, None, None))
    _refused(dv(None, q, 1, out, None, None, None))
    _refused(dv(fake, None, 1, out, None, None, None))
    _refused(dv(fake, q, 1, None, None, None, None))
    _refused(dv(fake, q, -1, out, None, None, None))
    _refused(ed(None, q, q, 1, out, None, None))
    _refused(ed(fake, None, q, 1, out, None, None))
    _refused(ed(fake, q, None, 1, out, None, None))
    _refused(ed(fake, q, q, 1, None, None, None))
    _refused(ed(fake, q, q, -1, out, None, None))
    # n == 0 touches nothing, the space included
    assert st(fake, q, 0, out, None, None) == 0
    assert dv(fake, q, 0, out, None, None, None) == 0
    assert ed(fake, q, q, 0, out, None, None) == 0
