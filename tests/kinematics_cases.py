"""The robots, state sets and shared reference positions of tests/test_kinematics_ref.py (CPU, the oracle) and
tests/test_gpu_kinematics.py (GPU, both kernel builds): every robot's reference is worked out once per process by
tests/kinematics_ref.py and handed out read-only.

The robots are the smallest set that takes every joint kind, rotated origins, an axis that is none of X / Y / Z, a
branching tree, leaves on fixed joints and both ends of the variable-count range."""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

import kinematics_ref as kr
import width_cases
from smpl_amd import scenes

ROBOTS = ["small_cfg", "cfg3_pr2", "mixed", "dual_arm", "nv1", "nv4", "nv7", "nv12", "nv16"]


def config(name, request):
    """the Config of an entry of ROBOTS (the two data-file robots are the session fixtures of conftest.py)"""
    if name in ("small_cfg", "cfg3_pr2"):
        return request.getfixturevalue(name)
    if name == "mixed":
        return scenes.config_mixed(n=16, nboxes=0)
    if name == "dual_arm":
        return scenes.config5(n=64, nboxes=12, res=0.08)
    return width_cases.case_config(name)


class Reference:
    """states Q, the nodes of the compiled model with their links, and the reference's sphere and planning-link values"""

    def __init__(self, robot_text, start, goal):
        from smpl_amd import capi
        self.robot = kr.Robot(robot_text)
        self.Q = kr.state_set(self.robot, start, goal)
        self.nodes = kr.model_nodes(self.robot, capi.Model(robot_text).arrays())
        self.spheres = self.robot.positions(self.Q, self.nodes)         # (hi, lo) [n][nodes][3]
        self.pose = self.robot.planning_poses(self.Q)                   # (hi, lo) [n][3][4]
        for a in (self.Q,) + self.spheres + self.pose:
            a.setflags(write=False)

    @property
    def xyz(self):
        return self.pose[0][:, :, 3], self.pose[1][:, :, 3]


_REFERENCES = {}


def reference(name, cfg):
    if name not in _REFERENCES:
        _REFERENCES[name] = Reference(cfg.robot_text, cfg.start, cfg.goal)
    return _REFERENCES[name]


def worst(got, ref):
    """the largest error of got against a (hi, lo) reference, in units of 2^-52"""
    return float(kr.error(got, ref).max()) / kr.U52


# ----------------------------------------------------------------------------------------------------------------------
# smplx_sincos: the host function, and a robot that hands its value out untouched
# ----------------------------------------------------------------------------------------------------------------------

def host_sincos(x):
    """(sin, cos) of every double of x by the host build of smplx_sincos (oracle/liboracle.so, orc_sincos)"""
    from oracle_binding import ORACLE_DIR, build_oracle
    build_oracle()
    L = C.CDLL(os.path.join(ORACLE_DIR, "liboracle.so"))
    L.orc_sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    x = np.asarray(x, np.float64).reshape(-1)
    s, c = np.zeros(len(x)), np.zeros(len(x))
    a, b = C.c_double(), C.c_double()
    for i, v in enumerate(x):
        L.orc_sincos(float(v), C.byref(a), C.byref(b))
        s[i], c[i] = a.value, b.value
    return s, c


PROBE_ROBOT = """robot sincos_probe
link base_link
link arm_link
link tool_link
joint spin continuous base_link arm_link  0 0 0  0 0 0  0 0 1  0.0 0.0
joint tool fixed arm_link tool_link  1 0 0  0 0 0  0 0 1  0.0 0.0
sphere arm_link s0 1 0 0 0.05 1
group arm arm_link
planning_joints spin
planning_link tool_link
"""


def probe_config():
    """One continuous joint about Z with an identity origin, the planning link fixed at (1, 0, 0) and one sphere at
    (1, 0, 0): both are at (cos q, sin q, 0), and every product on the way is by an exact 0 or 1, so the positions are
    the bits smplx_sincos returns.  Grid, parameters and primitives of the one-variable width case."""
    return dataclasses.replace(width_cases.width_case(1), name="sincos_probe", robot_text=PROBE_ROBOT)


_SINCOS = {}


def sincos_sets():
    """{name: (x, host sin, host cos, truth of sin, truth of cos)} over kinematics_ref.sincos_inputs(), once per process"""
    if not _SINCOS:
        for name, x in kr.sincos_inputs().items():
            s, c = host_sincos(x)
            ts, tc = kr.sincos_truth(x)
            for a in (x, s, c) + ts + tc:
                a.setflags(write=False)
            _SINCOS[name] = (x, s, c, ts, tc)
    return _SINCOS


def probe_angles():
    """(angles within [-pi, pi], angles beyond): the input sets split as the probe tests use them.  Within: the random set
    of [-pi, pi], k pi/2 and its neighbours for |k| <= 2, the tiny arguments and the two zeros; beyond: the set of
    [-1e5, 1e5] and every other k pi/2."""
    sets = kr.sincos_inputs()
    allx = np.concatenate([sets[k] for k in ("[-pi, pi]", "k pi/2", "tiny", "zero", "[-1e5, 1e5]")])
    inside = np.abs(allx) <= np.pi
    return np.ascontiguousarray(allx[inside]), np.ascontiguousarray(allx[~inside])


def normalized(x):
    return np.array([kr.normalize_angle(float(v)) for v in np.asarray(x).reshape(-1)])
