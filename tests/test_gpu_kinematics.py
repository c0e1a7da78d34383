"""Every world-frame position the kernels hand out against tests/kinematics_ref.py, the 192-bit forward kinematics written
from the robot text alone: k_sphere_positions, k_planning_pose, the xyz of k_heuristic and k_attached_positions, in the
per-robot build and in the kernels linked into the library.  The states, the robots and the bound (2^-46 m in every
component, 2^-46 in every rotation entry) are those tests/test_kinematics_ref.py holds the oracle to; the reference of a
robot is worked out once and shared between the builds.

The device copy of smplx_sincos is probed directly: a one-joint robot whose sphere and planning link sit at
(cos q, sin q, 0) hands out the function's bits, which are compared with the host build's over the argument sets of
kinematics_ref.sincos_inputs()."""
import numpy as np
import pytest

import kinematics_cases as cases
import kinematics_ref as kr

pytestmark = pytest.mark.gpu

BUILDS = ["specialized", "generic"]


def _space(cfg, kind):
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    s = capi.Space.from_config(cfg, generic_kernels=(kind == "generic"))
    assert s.specialized()[0] == (kind == "specialized"), s.specialized()[1]
    return s


@pytest.mark.parametrize("kind", BUILDS)
@pytest.mark.parametrize("robot", cases.ROBOTS)
def test_sphere_positions(robot, kind, request):
    """all tree nodes of the robot at every state of the set.  Worst error in units of 2^-52 m (bound: 64), specialized /
    generic: small_cfg 1.71 / 1.71, cfg3_pr2 1.50 / 1.50, mixed 1.30 / 1.30, dual_arm 1.66 / 1.66, nv1 0.62 / 0.62,
    nv4 0.96 / 0.96, nv7 2.31 / 2.31, nv12 2.75 / 2.75, nv16 2.49 / 2.49"""
    cfg = cases.config(robot, request)
    ref = cases.reference(robot, cfg)
    s = _space(cfg, kind)
    P = s.sphere_positions(ref.Q)
    assert P.shape == ref.spheres[0].shape
    e = cases.worst(P, ref.spheres)
    print(f"{robot} {kind}: sphere nodes against the reference: {e:.2f} * 2^-52 m over {len(ref.Q)} states, {P.shape[1]} nodes")
    assert e * kr.U52 <= kr.BOUND
    s.close()


@pytest.mark.parametrize("kind", BUILDS)
@pytest.mark.parametrize("robot", cases.ROBOTS)
def test_planning_link(robot, kind, request):
    """planning_pose_batch's translation column and rotation, and heuristic_batch's xyz, against the reference's planning
    link.  Worst error in units of 2^-52 (bound: 64), translation / rotation / xyz, the same in both builds:
    small_cfg 1.09 / 1.24 / 1.09, cfg3_pr2 0.75 / 1.35 / 0.75, mixed 0.96 / 1.64 / 0.96, dual_arm 1.09 / 1.25 / 1.09,
    nv1 0.73 / 0.55 / 0.73, nv4 1.30 / 1.59 / 1.30, nv7 2.40 / 1.48 / 2.40, nv12 2.01 / 2.60 / 2.01,
    nv16 1.97 / 3.82 / 1.97"""
    cfg = cases.config(robot, request)
    ref = cases.reference(robot, cfg)
    s = _space(cfg, kind)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    T = s.planning_pose_batch(ref.Q)
    _, xyz = s.heuristic_batch(ref.Q)
    assert T.shape == ref.pose[0].shape and xyz.shape == (len(ref.Q), 3)
    et = cases.worst(T[:, :, 3], ref.xyz)
    er = cases.worst(T[:, :, :3], (ref.pose[0][:, :, :3], ref.pose[1][:, :, :3]))
    ex = cases.worst(xyz, ref.xyz)
    print(f"{robot} {kind}: planning link against the reference, in 2^-52: translation {et:.2f}, rotation {er:.2f}, "
          f"heuristic xyz {ex:.2f}")
    assert et * kr.U52 <= kr.BOUND
    assert er * kr.U52 <= kr.BOUND
    assert ex * kr.U52 <= kr.BOUND
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# attached bodies
# ----------------------------------------------------------------------------------------------------------------------

HELD = [(0.20, 0.0, 0.0, 0.02), (0.24, 0.02, 0.0, 0.02), (0.24, -0.02, 0.01, 0.015), (0.28, 0.0, 0.02, 0.02),
        (0.22, 0.005, -0.03, 0.025)]
PAD = [(0.03, -0.01, 0.02, 0.015)]
BODY_LINKS = {"small_cfg": ("gripper_palm_link", "l_finger_tip_link"), "mixed": ("wrist", "pad")}
_BODY_REFERENCES = {}


def _body_reference(key, ref, bodies, xyzr):
    """the reference positions of the attached nodes, once per robot and set of bodies (the node centres are the same in
    both builds: the tree builder is host code)"""
    key = (key, xyzr.tobytes())
    if key not in _BODY_REFERENCES:
        _BODY_REFERENCES[key] = ref.robot.positions(ref.Q, kr.body_nodes(bodies, xyzr))
    return _BODY_REFERENCES[key]


@pytest.mark.parametrize("kind", BUILDS)
@pytest.mark.parametrize("robot", ["small_cfg", "mixed"])
def test_attached_positions(robot, kind, request):
    """a body of five spheres (a tree with inner nodes) on the wrist and a one-sphere body on a link that hangs on a fixed
    joint (the mixed robot's pad: a rotated fixed origin); after the first is detached the second still matches.
    Worst error in units of 2^-52 m (bound: 64), both bodies / the second alone, the same in both builds:
    small_cfg 1.48 / 1.48, mixed 1.31 / 1.22"""
    cfg = cases.config(robot, request)
    ref = cases.reference(robot, cfg)
    wrist, finger = BODY_LINKS[robot]
    fixed = ref.robot.joint_of[finger]
    assert fixed["type"] == "fixed" and (robot != "mixed" or any(fixed["rpy"]))
    s = _space(cfg, kind)
    s.attach_body("held", wrist, HELD, allowed=ref.robot.links)
    s.attach_body("pad", finger, PAD, allowed=ref.robot.links)
    bodies = s.attached_bodies()
    xyzr, left, _ = s.attached_nodes()
    assert [(b["id"], b["link"], b["count"]) for b in bodies] == [("held", wrist, 9), ("pad", finger, 1)]
    assert (left >= 0).sum() == 4                       # the first body's tree has inner nodes
    B = s.attached_positions(ref.Q)
    assert B.shape == (len(ref.Q), 10, 3)
    e2 = cases.worst(B, _body_reference(robot, ref, bodies, xyzr))
    s.detach_body("held")
    bodies = s.attached_bodies()
    xyzr, left, _ = s.attached_nodes()
    assert [(b["id"], b["link"], b["first"], b["count"]) for b in bodies] == [("pad", finger, 0, 1)]
    B = s.attached_positions(ref.Q)
    assert B.shape == (len(ref.Q), 1, 3)
    e1 = cases.worst(B, _body_reference(robot, ref, bodies, xyzr))
    print(f"{robot} {kind}: attached nodes against the reference, in 2^-52 m: both bodies {e2:.2f}, the second alone {e1:.2f}")
    assert e2 * kr.U52 <= kr.BOUND and e1 * kr.U52 <= kr.BOUND
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# the device smplx_sincos
# ----------------------------------------------------------------------------------------------------------------------

_PROBE = {}


def _probe_expected():
    """(angles, rows within [-pi, pi], host sin and cos of every angle, of every normalised angle, and for the rows beyond
    pi the truth of both), once"""
    if not _PROBE:
        inside, beyond = cases.probe_angles()
        x = np.concatenate([inside, beyond])
        xn = cases.normalized(x)
        assert np.array_equal(xn[:len(inside)], inside) and (np.abs(xn) <= np.pi).all()
        _PROBE["x"], _PROBE["n_inside"] = x, len(inside)
        _PROBE["raw"], _PROBE["norm"] = cases.host_sincos(x), cases.host_sincos(xn)
        _PROBE["truth_raw"], _PROBE["truth_norm"] = kr.sincos_truth(beyond), kr.sincos_truth(xn[len(inside):])
    return _PROBE


@pytest.mark.parametrize("kind", BUILDS)
def test_device_sincos_holds_the_host_bits(kind):
    """The probe robot (kinematics_cases.probe_config) at every angle of the input sets, one launch per entry point.
    Within [-pi, pi] -- 20 000 random angles, k pi/2 and both neighbours for |k| <= 2, 3000 tiny arguments, +0 and -0 --
    sphere_positions, planning_pose_batch (translation, rotation entries [0,0] and [1,0]) and heuristic_batch's xyz hold
    exactly the host function's values.  Beyond (20 000 angles up to 1e5, k pi/2 for |k| <= 63 000) the sphere takes the
    angle as it is and the planning link the normalised one: each still holds the host's value at that argument, and
    is within max(2.5 ulp, 2^-70) of mpmath's there."""
    p = _probe_expected()
    x, ni = p["x"], p["n_inside"]
    assert ni > 23000 and len(x) - ni > 40000
    s = _space(cases.probe_config(), kind)
    s.set_goal_xyz([-0.3, 0.06, 1.2], [0.02, 0.02, 0.02])
    S = s.sphere_positions(x)[:, 0, :]
    T = s.planning_pose_batch(x)
    _, xyz = s.heuristic_batch(x)
    (rs, rc), (ns, nc) = p["raw"], p["norm"]
    zero = np.zeros(len(x))
    # values, not bit patterns: equal for every nonzero double, and either zero passes for a zero
    assert np.array_equal(S, np.stack([rc, rs, zero], 1))
    assert np.array_equal(T[:, :, 3], np.stack([nc, ns, zero], 1))
    assert np.array_equal(T[:, 0, 0], nc) and np.array_equal(T[:, 1, 0], ns)
    assert np.array_equal(xyz, np.stack([nc, ns, zero], 1))
    assert np.array_equal(rs[:ni], ns[:ni]) and np.array_equal(rc[:ni], nc[:ni])
    (ts, tc), (tsn, tcn) = p["truth_raw"], p["truth_norm"]
    assert kr.sincos_within_bound(S[ni:, 1], ts).all() and kr.sincos_within_bound(S[ni:, 0], tc).all()
    for got in (T[ni:, :, 3], xyz[ni:]):
        assert kr.sincos_within_bound(got[:, 1], tsn).all() and kr.sincos_within_bound(got[:, 0], tcn).all()
    assert kr.sincos_within_bound(T[ni:, 1, 0], tsn).all() and kr.sincos_within_bound(T[ni:, 0, 0], tcn).all()
    s.close()
