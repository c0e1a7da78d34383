"""The pose-goal (XYZ_RPY_GOAL) entry points without a GPU: the header declares them, the library exports them, bad
arguments are refused before any space is touched, and smplx_rpy_angle is the reference's orientation distance
(manip_lattice.cpp:1652-1665)."""
import ctypes as C
import math
import os
import re

import numpy as np

import pose_goal_ref as ref
from smpl_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -1
NEW = ["smplx_set_goal_pose", "smplx_set_goals_pose_multi", "smplx_goal_orientation", "smplx_planning_pose_batch", "smplx_rpy_angle"]
# 2 acos(d) near d = 1 turns an error of 1e-16 in d into about 1.5e-8 in the angle
ANGLE_TOL = 1e-6


def _arr(*v):
    return (C.c_double * len(v))(*v)


def test_header_declares_and_library_exports_the_five_symbols():
    hdr = open(os.path.join(ROOT, "include", "smpl_amd.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
    for m in ("set_goal_pose", "set_goals_pose_multi", "goal_orientation", "planning_pose_batch", "rpy_angle"):
        assert callable(getattr(capi.Space, m)), m
    assert callable(capi.rpy_angle)


def test_single_goal_bad_arguments_are_refused():
    L = capi.lib()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below fails on its other arguments
    v = _arr(0.1, 0.2, 0.3)
    assert L.smplx_set_goal_pose(None, v, v, v, 0.2) == E_ARG
    assert "null" in L.smplx_last_error().decode()
    assert L.smplx_set_goal_pose(fake, None, v, v, 0.2) == E_ARG
    assert L.smplx_set_goal_pose(fake, v, None, v, 0.2) == E_ARG
    assert L.smplx_set_goal_pose(fake, v, v, None, 0.2) == E_ARG
    for bad in [float("nan"), float("inf"), -float("inf"), 1.0e6, -1.0e6]:
        for k in range(3):
            x = _arr(0.1, 0.2, 0.3)
            x[k] = bad
            assert L.smplx_set_goal_pose(fake, x, v, v, 0.2) == E_ARG, (bad, k)      # position: finite, |xyz| < 1e6
            assert "finite" in L.smplx_last_error().decode()
            # orientation: finite, |rpy| < 1e6 (the sine and cosine of the goal rotation reduce their argument through an int)
            assert L.smplx_set_goal_pose(fake, v, x, v, 0.2) == E_ARG, (bad, k)
            assert "finite" in L.smplx_last_error().decode()
    assert L.smplx_set_goal_pose(fake, v, _arr(0.0, 1.0e12, 0.0), v, 0.2) == E_ARG
    for k in range(3):
        t = _arr(0.1, 0.2, 0.3)
        t[k] = float("nan")
        assert L.smplx_set_goal_pose(fake, v, v, t, 0.2) == E_ARG                    # a NaN tolerance
    assert L.smplx_set_goal_pose(fake, v, v, v, float("nan")) == E_ARG
    # the accessors and the FK batch
    out = _arr(0.0, 0.0, 0.0)
    tol = C.c_double(0.0)
    assert L.smplx_goal_orientation(None, out, C.byref(tol)) == E_ARG
    assert L.smplx_goal_orientation(fake, None, C.byref(tol)) == E_ARG
    assert L.smplx_goal_orientation(fake, out, None) == E_ARG
    T = (C.c_double * 12)()
    assert L.smplx_planning_pose_batch(None, v, 1, T) == E_ARG
    assert L.smplx_planning_pose_batch(fake, None, 1, T) == E_ARG
    assert L.smplx_planning_pose_batch(fake, v, 1, None) == E_ARG
    assert L.smplx_planning_pose_batch(fake, v, -1, T) == E_ARG
    th = C.c_double(0.0)
    assert L.smplx_rpy_angle(None, v, C.byref(th)) == E_ARG
    assert L.smplx_rpy_angle(v, None, C.byref(th)) == E_ARG
    assert L.smplx_rpy_angle(v, v, None) == E_ARG
    assert L.smplx_rpy_angle(_arr(0.0, float("nan"), 0.0), v, C.byref(th)) == E_ARG


def test_multi_goal_bad_arguments_are_refused():
    L = capi.lib()
    fake = [0x1000, 0x2000]      # never dereferenced: these arguments are checked on the handles alone
    two = (C.c_void_p * 2)(*fake)
    same = (C.c_void_p * 2)(fake[0], fake[0])
    hole = (C.c_void_p * 2)(fake[0], None)
    v = (C.c_double * 6)(*([0.25] * 6))
    fn = L.smplx_set_goals_pose_multi
    assert fn(None, 1, v, v, v, v) == E_ARG              # no array of spaces
    assert fn(two, 0, v, v, v, v) == E_ARG               # nq < 1
    assert fn(two, -3, v, v, v, v) == E_ARG
    assert fn(hole, 2, v, v, v, v) == E_ARG              # a null handle in the array
    assert "null" in L.smplx_last_error().decode()
    assert fn(same, 2, v, v, v, v) == E_ARG              # the same space twice
    assert "twice" in L.smplx_last_error().decode()
    for k in range(4):                                   # a null array
        a = [v, v, v, v]
        a[k] = None
        assert fn(two, 2, *a) == E_ARG
    for k in range(4):                                   # a NaN anywhere, in the second goal too
        a = [(C.c_double * 6)(*([0.25] * 6)) for _ in range(4)]
        a[k][1 if k == 3 else 4] = float("nan")
        assert fn(two, 2, *a) == E_ARG, k
        assert "finite" in L.smplx_last_error().decode()
    x = (C.c_double * 6)(0.1, 0.2, 0.3, 0.4, float("inf"), 0.6)
    assert fn(two, 2, x, v, v, v) == E_ARG
    for bad in (1.0e6, -1.0e12):                         # |xyz|, |rpy| < 1e6, in the second goal too
        x = (C.c_double * 6)(0.1, 0.2, 0.3, 0.4, bad, 0.6)
        assert fn(two, 2, x, v, v, v) == E_ARG and fn(two, 2, v, x, v, v) == E_ARG


def _angle(a, b):
    return capi.rpy_angle(a, b)


def test_rpy_angle_is_the_references_formula():
    rng = np.random.default_rng(20260)
    A = rng.uniform(-math.pi, math.pi, size=(1000, 3))
    B = rng.uniform(-math.pi, math.pi, size=(1000, 3))
    A[:, 1] *= 0.5
    B[:, 1] *= 0.5                                       # pitch in [-pi/2, pi/2]
    worst = 0.0
    for a, b in zip(A, B):
        got, exp = _angle(a, b), ref.rpy_angle(a, b)
        assert 0.0 <= got <= math.pi
        worst = max(worst, abs(got - exp))
        # the same angle from the rotations the two triples recompose to (semantics 2 of the pose goal)
        assert abs(got - ref.rotation_angle(ref.rpy_matrix(a), ref.rpy_matrix(b))) <= ANGLE_TOL
    print("rpy_angle against the numpy restatement, 1000 pairs: worst", worst)
    assert worst <= ANGLE_TOL


def test_rpy_angle_special_classes():
    rng = np.random.default_rng(7)
    for a in rng.uniform(-3.0, 3.0, size=(50, 3)):
        # identical: 0 up to the conditioning of acos at 1
        t = _angle(a, a)
        assert 0.0 <= t <= ANGLE_TOL
        # the antipodal quaternion: the same rotation reached by another turn of one angle, or by the other Euler triple
        for k in range(3):
            b = a.copy(); b[k] += 2.0 * math.pi
            t = _angle(a, b)
            assert 0.0 <= t <= ANGLE_TOL, (a, k, t)
            assert np.dot(ref.rpy_quat(a), ref.rpy_quat(b)) < 0.0            # ... and it is the sign-flip branch
        b = np.array([a[0] + math.pi, math.pi - a[1], a[2] + math.pi])
        assert 0.0 <= _angle(a, b) <= ANGLE_TOL
    # half a turn apart: pi, never beyond
    for a in rng.uniform(-3.0, 3.0, size=(50, 3)):
        b = a.copy(); b[0] += math.pi                                         # Rx(pi) behind the same rotation
        t = _angle(a, b)
        assert abs(t - math.pi) <= ANGLE_TOL and t <= math.pi
    # gimbal lock, pitch = +-pi/2: only roll -+ yaw counts
    for sign in (1.0, -1.0):
        p = sign * 0.5 * math.pi
        for r, y, d in rng.uniform(-1.0, 1.0, size=(50, 3)):
            a = np.array([r, p, y])
            b = np.array([r + d, p, y + sign * d])                            # the same rotation
            assert 0.0 <= _angle(a, b) <= ANGLE_TOL
            c = np.array([r + d, p, y])                                       # a turn of d about the locked axis
            got = _angle(a, c)
            assert abs(got - abs(d)) <= ANGLE_TOL and abs(got - ref.rpy_angle(a, c)) <= ANGLE_TOL
