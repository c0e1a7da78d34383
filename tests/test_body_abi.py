"""The robot-body entry points without a GPU: the header declares them, the library exports them, capi binds them, every
text-level refusal is SMPLX_E_ARG with its line number before any GPU is touched, and formats.urdf_to_body_text writes
the body text from a URDF and the collision-model YAML."""
import ctypes as C
import os
import re

import pytest

from smpl_amd import capi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["smplx_body_create", "smplx_body_counts", "smplx_body_set_joint", "smplx_body_joint", "smplx_body_link_transforms",
       "smplx_body_model_link", "smplx_body_model_points", "smplx_body_dirty", "smplx_grid_put_body", "smplx_grid_take_body",
       "smplx_grid_body_cells"]


def test_header_declares_and_library_exports_the_symbols():
    hdr = open(os.path.join(ROOT, "include", "smpl_amd.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    assert re.search(r"\bvoid\s+smplx_body_destroy\s*\(", hdr) and hasattr(L, "smplx_body_destroy") and "smplx_body_destroy" in capi.SYMBOLS
    for name in ("LINKS", "MODEL_POINTS", "POINTS", "LATTICE"):
        assert re.search(r"#define\s+SMPLX_BODY_MAX_%s\s+\d+" % name, hdr), name
    for m in ("set_joint", "joint", "link_transforms", "model_link", "model_points", "dirty"):
        assert callable(getattr(capi.Body, m)), m
    for m in ("put_body", "take_body", "body_cells"):
        assert callable(getattr(capi.Grid, m)), m
    # each piece cites the reference lines it stands behind
    for cite in ("self_collision_model.cpp:616-760", "robot_collision_model.cpp:959-1073", "voxelize.cpp:962-986", "discretize.h:94-113",
                 "robot_collision_state.h:473-497", "robot_collision_state.cpp:62-96", "robot_collision_state.cpp:264-266"):
        assert cite in hdr, cite


def test_plugin_mirror_declares_the_body_calls():
    hpp = open(os.path.join(ROOT, "include", "smpl_amd", "plugin.hpp")).read()
    gpu = hpp[hpp.index("class GpuCollisionChecker"):]
    for sig in (r"bool\s+attachRobotBody\s*\(\s*const\s+std::string&\s+body_text\s*\)", r"bool\s+detachRobotBody\s*\(\s*\)",
                r"bool\s+setJointPosition\s*\(\s*const\s+std::string&\s+name,\s*double\s+position\s*\)"):
        assert re.search(sig, gpu), sig


def create(text):
    h = C.c_void_p()
    L = capi.lib()
    L.smplx_body_create.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    rc = L.smplx_body_create(text.encode() if text is not None else None, C.byref(h))
    return rc, L.smplx_last_error().decode(), h


def test_text_refusals_come_with_their_line_before_any_gpu_is_touched():
    from test_body_model import MALFORMED
    for text, line in MALFORMED:
        rc, msg, h = create(text)
        assert rc == capi.E_ARG and msg.startswith("line %d: " % line) and not h.value, (text, rc, msg)
    rc, msg, h = create("")
    assert rc == capi.E_ARG and not h.value
    assert create(None)[0] == capi.E_ARG
    L = capi.lib()
    assert L.smplx_body_create(b"link a\n", None) == capi.E_ARG
    rc, msg, h = create("".join("link l%d\n" % i for i in range(4097)))
    assert rc == -3 and msg.startswith("line 4097: ")
    # null handles
    L.smplx_body_set_joint.argtypes = [C.c_void_p, C.c_char_p, C.c_double]
    assert L.smplx_body_set_joint(None, b"j", 0.0) == capi.E_ARG
    L.smplx_grid_put_body.argtypes = [C.c_void_p, C.c_void_p]
    assert L.smplx_grid_put_body(None, None) == capi.E_ARG
    L.smplx_grid_take_body.argtypes = [C.c_void_p]
    assert L.smplx_grid_take_body(None) == capi.E_ARG
    n = C.c_int(7)
    L.smplx_grid_body_cells.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    assert L.smplx_grid_body_cells(None, 0, None, 0, C.byref(n)) == capi.E_ARG and n.value == 0


URDF = """<robot name="five">
  <link name="base"><collision><origin xyz="0.1 0.2 0.3" rpy="0.01 0.02 0.03"/><geometry><box size="0.4 0.5 0.6"/></geometry></collision>
    <collision><geometry><sphere radius="0.07"/></geometry></collision></link>
  <link name="torso"><collision><origin xyz="0 0 0.2"/><geometry><cylinder radius="0.11" length="0.7"/></geometry></collision></link>
  <link name="head"><collision><origin xyz="0 0 0.05"/><geometry><mesh filename="package://five/head.stl" scale="2 2 2"/></geometry></collision></link>
  <link name="upper"><collision><geometry><box size="0.3 0.05 0.05"/></geometry></collision></link>
  <link name="fore"/>
  <joint name="lift" type="prismatic"><parent link="base"/><child link="torso"/><origin xyz="0 0 0.4"/><axis xyz="0 0 1"/><limit lower="0" upper="0.3"/></joint>
  <joint name="pan" type="continuous"><parent link="torso"/><child link="head"/><origin xyz="0 0 0.5" rpy="0 0 0.1"/><axis xyz="0 0 1"/></joint>
  <joint name="shoulder" type="revolute"><parent link="torso"/><child link="upper"/><origin xyz="0 -0.2 0.3"/><axis xyz="0 1 0"/><limit lower="-1" upper="1"/></joint>
  <joint name="elbow" type="revolute"><parent link="upper"/><child link="fore"/><origin xyz="0.3 0 0"/><axis xyz="0 1 0"/><limit lower="-2" upper="2"/></joint>
</robot>"""
YAML = """robot_collision_model:
  voxels_models:
    - { link_name: base, res: 0.01 }
    - { link_name: head, res: 0.02 }
    - { link_name: torso, res: 0.01 }
    - { link_name: upper, res: 0.01 }
  collision_groups:
    - name: arm
      chains:
        - { base: upper, tip: fore }
"""
HEAD = {"package://five/head.stl": ([(0, 0, 0), (0.05, 0, 0), (0, 0.05, 0), (0, 0, 0.05)], [(0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)])}


def test_urdf_to_body_text():
    text = formats.urdf_to_body_text(URDF, YAML, "arm", meshes=HEAD, values={"lift": 0.1137, "pan": -0.4321})
    rows = [r.split() for r in text.splitlines()]
    assert [r[1] for r in rows if r[0] == "link"] == ["base", "torso", "head", "upper", "fore"]
    assert [(r[1], r[2], r[3], r[4]) for r in rows if r[0] == "joint"] == [("lift", "prismatic", "base", "torso"), ("pan", "continuous", "torso", "head"),
                                                                         ("shoulder", "revolute", "torso", "upper"), ("elbow", "revolute", "upper", "fore")]
    assert [float(x) for x in [r for r in rows if r[0] == "joint"][1][5:16]] == [0, 0, 0.5, 0, 0, 0.1, 0, 0, 1, 0, 0]
    geoms = [r for r in rows if r[0] == "geom"]
    assert [(g[1], g[2]) for g in geoms] == [("base", "box"), ("base", "sphere"), ("torso", "cylinder"), ("head", "mesh"), ("upper", "box")]
    assert [float(x) for x in geoms[0][3:]] == [0.4, 0.5, 0.6, 0.1, 0.2, 0.3, 0.01, 0.02, 0.03]
    assert [float(x) for x in geoms[1][3:]] == [0.07, 0, 0, 0, 0, 0, 0]
    assert [float(x) for x in geoms[2][3:]] == [0.11, 0.7, 0, 0, 0.2, 0, 0, 0]
    assert geoms[3][3:5] == ["4", "4"] and [float(x) for x in geoms[3][5:]] == [0, 0, 0.05, 0, 0, 0]
    assert [[float(x) for x in r[1:]] for r in rows if r[0] == "v"] == [[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1]]   # scaled
    assert [[int(x) for x in r[1:]] for r in rows if r[0] == "t"] == [list(t) for t in HEAD["package://five/head.stl"][1]]
    assert [(r[1], float(r[2])) for r in rows if r[0] == "voxels"] == [("base", 0.01), ("head", 0.02), ("torso", 0.01), ("upper", 0.01)]   # the YAML's list
    assert [r for r in rows if r[0] == "group"] == [["group", "arm", "upper", "fore"]]
    assert [(r[1], float(r[2])) for r in rows if r[0] == "value"] == [("lift", 0.1137), ("pan", -0.4321)]
    with pytest.raises(ValueError, match="head.stl"):
        formats.urdf_to_body_text(URDF, YAML, "arm")
    with pytest.raises(ValueError, match="planar"):
        formats.urdf_to_body_text(URDF.replace('type="prismatic"', 'type="planar"'), YAML, "arm", meshes=HEAD)
    # the text is one the parser takes: the model reads it and the library gets past the text (it then needs a GPU)
    import body_ref
    b = body_ref.Body(text)
    assert b.outside == [True, True, True, False] and b.q["lift"] == 0.1137
    rc, msg, h = create(text)
    assert rc in (0, -4) and not msg.startswith("line "), msg
    if rc == 0:
        capi.lib().smplx_body_destroy.argtypes = [C.c_void_p]
        capi.lib().smplx_body_destroy.restype = None
        capi.lib().smplx_body_destroy(h)
