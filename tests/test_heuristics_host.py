"""The closed-form heuristics (smplx_params.heuristic: SMPLX_H_EUCLID, SMPLX_H_JOINT_DIST) without a GPU: the accuracy of
smplx_acos (det_math.h), the two host-arithmetic calls smplx_pose_distance and smplx_joint_distance -- the functions of
smpl_amd/csrc/heuristics.h that the kernels compile too -- against plain references, the layout of smplx_params, and the
argument and state errors that are found before a device is touched.  tests/test_gpu_heuristic_kinds.py holds the kernels
to these host functions bit for bit."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

import kinematics_ref as kr
import pose_goal_ref as ref
from heuristic_cases import WEIGHTS, np_joint_distance, np_pose_distance
from smpl_amd import capi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
E_ARG, E_STATE = -1, -5
NEW = ["smplx_set_euclid_weights", "smplx_metric_goal_distance", "smplx_pose_distance", "smplx_joint_distance", "smplx_space_heuristic"]

# smplx_acos over [0, 1]: the measured maximum, as the comment in det_math.h states it, and the bound the test holds it
# to -- twice that.  Measured by test_acos_accuracy (worst, in ulp of the true value):
#     uniform in [0, 1]                  40000    0.748
#     uniform in [0.5 - 1e-3, 0.5 + 1e-3] 5000    0.764     (where the two branches meet; stated as 0.77)
#     1 - k ulp, k = 0 .. 4000            4001    0.500     (exact at 1)
#     log-uniform in [1e-300, 0.5]        5000    0.595
ACOS_MEASURED_ULPS = 0.77
ACOS_BOUND_ULPS = 2 * ACOS_MEASURED_ULPS

# |1000 dist (host) - 1000 dist (numpy)| over the 2 robots x 2000 states x 3 weight sets of
# test_pose_distance_against_numpy: the largest difference measured is 8.8e-10 (a state 1e-3 rad from the goal rotation
# would give more: acos is ill-conditioned at 1; none of the seeded states is that near).  The tolerance is ten times that.
POSE_MEASURED = 8.8e-10
POSE_TOL = 10 * POSE_MEASURED


def _arr(*v):
    return (C.c_double * len(v))(*v)


def _acos_sets():
    rng = np.random.default_rng(27182)
    one = np.float64(1.0)
    below = [one]
    for _ in range(4000):
        below.append(np.nextafter(below[-1], 0.0))
    return {
        "[0, 1]": rng.uniform(0.0, 1.0, 40000),
        "around 1/2": rng.uniform(0.5 - 1e-3, 0.5 + 1e-3, 5000),
        "1 - k ulp": np.array(below),
        "tiny": np.exp(rng.uniform(math.log(1e-300), math.log(0.5), 5000)),
    }


def _acos_truth(x):
    out = np.zeros((2, len(x)))
    for i, v in enumerate(x):
        out[0, i], out[1, i] = kr.split(kr.MP.acos(kr.mpf(float(v))))
    return out[0], out[1]


def test_acos_accuracy():
    """smplx_acos (the host build, through the test hook) against the 192-bit reference, in ulp of the true value."""
    worst = 0.0
    for name, x in _acos_sets().items():
        got = capi.host_acos(x)
        truth = _acos_truth(x)
        err = kr.error(got, truth)
        ulps = np.where(truth[0] == 0.0, np.where(err == 0.0, 0.0, np.inf), err / kr.ulp_of(truth))
        print(f"smplx_acos on {name}: n {len(x)}, worst {ulps.max():.3f} ulp at x = {float(x[int(ulps.argmax())])!r}")
        assert (got >= 0.0).all() and (got <= math.pi / 2).all()
        assert ulps.max() <= ACOS_BOUND_ULPS, name
        worst = max(worst, float(ulps.max()))
    print("smplx_acos: worst of all sets", worst, "ulp; stated", ACOS_MEASURED_ULPS)
    # the statement in det_math.h is the measurement, not a guess: it may not understate what is measured here
    assert worst <= ACOS_MEASURED_ULPS + 0.005
    assert "at most %.2f ulp" % ACOS_MEASURED_ULPS in open(os.path.join(ROOT, "smpl_amd", "csrc", "det_math.h")).read()


def test_acos_endpoints_and_neighbours_of_one():
    got = capi.host_acos([0.0, 1.0, 0.5])
    assert got[0] == math.pi / 2 and got[1] == 0.0
    assert abs(got[2] - math.pi / 3) <= 2.0 ** -52
    x = [1.0]
    for _ in range(8):
        x.append(float(np.nextafter(x[-1], 0.0)))
    got = capi.host_acos(x)
    assert (np.diff(got) > 0.0).all()                      # strictly larger angles a few ulp below 1
    for v, g in zip(x[1:], got[1:]):
        t = kr.MP.acos(kr.mpf(v))
        assert abs(kr.mpf(float(g)) - t) <= ACOS_BOUND_ULPS * 2.0 ** -52 * float(t)


def test_pose_distance_against_numpy(small_cfg, cfg3_pr2):
    worst = 0.0
    for cfg in (small_cfg, cfg3_pr2):
        chain = ref.Chain(cfg.robot_text)
        T, Tg = chain.transforms(scenes.random_states(scenes.ARM7_LIMITS, 2000, 4242)), chain.transform(np.array(cfg.goal))
        for w in WEIGHTS:
            got = np.array([capi.pose_distance(t[:3], Tg[:3], w) for t in T])
            exp = np.array([np_pose_distance(t, Tg, w) for t in T])
            diff = np.abs(1000.0 * got - 1000.0 * exp).max()
            print(f"{cfg.name} w {w}: 1000 dist against numpy, worst difference {diff:.3g}; smallest dist {got.min():.4f}")
            assert (got >= 0.0).all() and diff <= POSE_TOL, (cfg.name, w)
            worst = max(worst, diff)
    print("pose distance: worst of all", worst, "; stated", POSE_MEASURED)
    # special values: the same pose is at distance 0 whatever the weights; a pure translation has no rotation term
    assert capi.pose_distance(Tg[:3], Tg[:3], WEIGHTS[1]) <= 1e-7 * math.sqrt(WEIGHTS[1][3])
    Tm = Tg.copy(); Tm[:3, 3] += [0.3, -0.4, 0.0]
    assert abs(capi.pose_distance(Tg[:3], Tm[:3], (1, 1, 1, 0)) - 0.5) <= 1e-15
    Th = Tg.copy(); Th[:3, :3] = Tg[:3, :3] @ ref.rot_x(math.pi)          # half a turn: theta = pi, never beyond
    assert abs(capi.pose_distance(Tg[:3], Th[:3], (0, 0, 0, 1)) - math.pi) <= 1e-7


def test_joint_distance_is_the_loop_in_variable_order():
    rng = np.random.default_rng(99)
    for n in (1, 7, 15, 16):
        for _ in range(200):
            a, b = rng.uniform(-7.0, 7.0, n), rng.uniform(-7.0, 7.0, n)      # beyond +-2 pi: no wrapping
            assert capi.joint_distance(a, b) == np_joint_distance(a, b), n
        a = rng.uniform(-1.0, 1.0, n)
        assert capi.joint_distance(a, a) == 0.0
    # the order matters in the last bit somewhere: the sum is the sequential one, not a pairwise or a sorted one
    a, b = np.array([1e8, 1.0, -1e8, 1.0] * 4), np.zeros(16)
    assert capi.joint_distance(a, b) == np_joint_distance(a, b)


_PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include <string.h>
#include "smpl_amd.h"
int main(void) {
    smplx_params p;
    memset(&p, 0, sizeof p);
    printf("%zu %zu %zu %d %d %d %d\n", sizeof(smplx_params), offsetof(smplx_params, flags), offsetof(smplx_params, heuristic),
           SMPLX_H_BFS, SMPLX_H_EUCLID, SMPLX_H_JOINT_DIST, p.heuristic == SMPLX_H_BFS);
    return 0;
}
"""


def test_params_layout_and_symbols(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text(_PROBE)
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, str(src), "-o", str(exe)])
    size, off_flags, off_h, bfs, euclid, joint, zero_is_bfs = (int(x) for x in subprocess.check_output([str(exe)]).split())
    assert size == C.sizeof(capi.Params) and off_flags == capi.Params.flags.offset and off_h == capi.Params.heuristic.offset
    assert off_h == off_flags + 4                              # appended: every earlier field stays where it was
    assert (bfs, euclid, joint) == (capi.H_BFS, capi.H_EUCLID, capi.H_JOINT_DIST) == (0, 1, 2) and zero_is_bfs == 1
    hdr = open(os.path.join(INC, "smpl_amd.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert hasattr(L, name) and name in capi.SYMBOLS, name
    assert hasattr(L, "smplx_test_acos") and "smplx_test_acos" not in hdr       # a test hook, not part of the boundary


def test_bad_arguments_are_refused_before_a_device_is_touched():
    L = capi.lib()
    fake = C.c_void_p(0x1000)      # never dereferenced: every call below fails on its other arguments
    # smplx_space_create: an unknown kind
    out = C.c_void_p()
    for bad in (3, -1, 1 << 20):
        P = capi.Params()
        P.heuristic = bad
        assert L.smplx_space_create(fake, fake, b"", C.byref(P), C.byref(out)) == E_ARG, bad
        assert "heuristic" in L.smplx_last_error().decode()
    w = _arr(1.0, 1.0, 1.0, 1.0)
    # smplx_set_euclid_weights
    assert L.smplx_set_euclid_weights(None, w) == E_ARG
    assert L.smplx_set_euclid_weights(fake, None) == E_ARG
    for bad in (-1.0, -1e-300, float("nan"), float("inf")):
        for k in range(4):
            x = _arr(1.0, 1.0, 1.0, 1.0)
            x[k] = bad
            assert L.smplx_set_euclid_weights(fake, x) == E_ARG, (bad, k)
            assert "weights" in L.smplx_last_error().decode()
    # smplx_metric_goal_distance
    v = _arr(0.1, 0.2, 0.3)
    assert L.smplx_metric_goal_distance(None, v, 1, v) == E_ARG
    assert L.smplx_metric_goal_distance(fake, None, 1, v) == E_ARG
    assert L.smplx_metric_goal_distance(fake, v, 1, None) == E_ARG
    assert L.smplx_metric_goal_distance(fake, v, -1, v) == E_ARG
    # smplx_pose_distance
    T = (C.c_double * 12)(1, 0, 0, 0.1, 0, 1, 0, 0.2, 0, 0, 1, 0.3)
    d = C.c_double(-1.0)
    assert L.smplx_pose_distance(T, T, w, C.byref(d)) == 0 and d.value == 0.0
    assert L.smplx_pose_distance(None, T, w, C.byref(d)) == E_ARG
    assert L.smplx_pose_distance(T, None, w, C.byref(d)) == E_ARG
    assert L.smplx_pose_distance(T, T, None, C.byref(d)) == E_ARG
    assert L.smplx_pose_distance(T, T, w, None) == E_ARG
    for bad in (float("nan"), float("inf")):
        X = (C.c_double * 12)(*list(T))
        X[5] = bad
        assert L.smplx_pose_distance(X, T, w, C.byref(d)) == E_ARG and L.smplx_pose_distance(T, X, w, C.byref(d)) == E_ARG
    assert L.smplx_pose_distance(T, T, _arr(1.0, -1.0, 1.0, 1.0), C.byref(d)) == E_ARG
    assert L.smplx_pose_distance(T, T, _arr(1.0, 1.0, 1.0, float("nan")), C.byref(d)) == E_ARG
    # smplx_joint_distance
    a = (C.c_double * 17)(*([0.5] * 17))
    assert L.smplx_joint_distance(a, a, 16, C.byref(d)) == 0 and d.value == 0.0
    assert L.smplx_joint_distance(a, a, 0, C.byref(d)) == 0 and d.value == 0.0
    assert L.smplx_joint_distance(None, a, 3, C.byref(d)) == E_ARG
    assert L.smplx_joint_distance(a, None, 3, C.byref(d)) == E_ARG
    assert L.smplx_joint_distance(a, a, 3, None) == E_ARG
    assert L.smplx_joint_distance(a, a, -1, C.byref(d)) == E_ARG
    assert L.smplx_joint_distance(a, a, 17, C.byref(d)) == E_ARG
    b = (C.c_double * 3)(0.0, float("nan"), 0.0)
    assert L.smplx_joint_distance(b, a, 3, C.byref(d)) == E_ARG and L.smplx_joint_distance(a, b, 3, C.byref(d)) == E_ARG
    assert L.smplx_joint_distance(b, a, 1, C.byref(d)) == 0          # the NaN lies beyond n
