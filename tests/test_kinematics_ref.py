"""The oracle's world-frame positions and the host smplx_sincos against tests/kinematics_ref.py, a 192-bit forward
kinematics written from the robot text alone.  Everything else the suite says about a position is bit equality between
the engine and the oracle, which share their conventions (origin order, axis, the prismatic rule) and their sine and
cosine: these tests are where a mistake common to both would show.  tests/test_gpu_kinematics.py holds the kernels to the
same reference, the same states and the same bound.

The bound on a position, BOUND = 2^-46 m in every component: the oracle's error measured at 7 joints and 1.2 m of reach
is 1.9 * 2^-52 m; a factor of 32 over that leaves room for 16-joint chains and longer arms, and is ten orders of
magnitude below what a wrong convention produces (1e-4 m at the least; see test_prismatic_axis_is_ignored for one)."""
import math

import numpy as np
import pytest

import kinematics_cases as cases
import kinematics_ref as kr
import width_cases
from oracle_binding import Oracle
from smpl_amd import scenes


def _oracle_positions(cfg, ref):
    o = Oracle(cfg)
    nn = len(ref.nodes)
    S = np.stack([o.sphere_positions(q, nn) for q in ref.Q])
    P = np.stack([o.planning_fk(q) for q in ref.Q])
    return S, P


@pytest.mark.parametrize("robot", cases.ROBOTS)
def test_oracle_positions_against_reference(robot, request):
    """Every tree node and the planning link at 64 seeded states, the start, the goal, every variable at each limit and
    continuous variables beyond +-2 pi.  Worst error of the oracle, in units of 2^-52 m (the bound is 64 of them):

        robot       states  nodes  sphere nodes  planning link
        small_cfg     86      38       1.71          1.09
        cfg3_pr2      86      38       1.50          0.75
        mixed         80      14       1.30          0.96
        dual_arm     104      76       1.66          1.09
        nv1           68       3       0.62          0.73
        nv4           78       8       0.96          1.30
        nv7           84      15       2.31          2.40
        nv12          96      24       2.75          2.01
        nv16         106      32       2.49          1.97

    All are under 2^-49 m (8 units), the level at which a robot would have been looked into before any bound moved."""
    cfg = cases.config(robot, request)
    ref = cases.reference(robot, cfg)
    S, P = _oracle_positions(cfg, ref)
    es, ep = cases.worst(S, ref.spheres), cases.worst(P, ref.xyz)
    print(f"{robot}: {len(ref.Q)} states, {len(ref.nodes)} nodes; oracle against the reference, in 2^-52 m: "
          f"sphere nodes {es:.2f}, planning link {ep:.2f}")
    assert len(ref.Q) >= 64 + 2 + 2 * ref.robot.nvars
    assert es * kr.U52 <= kr.BOUND and ep * kr.U52 <= kr.BOUND


def test_state_sets_take_the_normalisation_path(request):
    """the state set of a robot with continuous variables holds values beyond +-2 pi and the values -pi and pi, and the
    normalised angle is the same angle: a whole number of turns away, to the 2.5e-16 rad per turn that subtracting the double
    nearest to 2 pi costs"""
    ref = cases.reference("small_cfg", cases.config("small_cfg", request))
    cont = np.array(ref.robot.continuous())
    assert cont.sum() == 2
    q = ref.Q[:, cont]
    assert (np.abs(q) > 2 * math.pi).sum() >= 4 and (q == math.pi).any() and (q == -math.pi).any()
    for a in q[np.abs(q) > math.pi]:
        n = kr.normalize_angle(float(a))
        turns = (kr.mpf(float(a)) - kr.mpf(n)) / (2 * kr.MP.pi)
        assert abs(n) <= math.pi and abs(turns - round(turns)) <= 8 * 2.5e-16 / (2 * math.pi)


# ----------------------------------------------------------------------------------------------------------------------
# smplx_sincos on the host
# ----------------------------------------------------------------------------------------------------------------------

def test_host_sincos_against_mpmath():
    """orc_sincos (the host build of smplx_sincos) against mpmath: error <= max(2.5 ulp of the true value, 2^-70).
    2.5 ulp is the worst error on the two random sets, 2.18, rounded up to the next half; 2^-70 is a thousand times the
    absolute error next to a multiple of pi/2, where the relative error is unbounded.  Measured (sin / cos):

        set                                         n      worst, ulp       worst absolute
        uniform in [-pi, pi]                      20000    1.01 / 1.35      2^-53.0
        uniform in [-1e5, 1e5]                    20000    2.01 / 2.18      2^-52.6
        k pi/2 and both neighbours, |k| <= 63000  21003    25533 / 25533    2^-87.1 where over 2.5 ulp
        log-uniform in [1e-300, 0.1]               3000    0.48 / 0.49      2^-54.0
        +0, -0                                        2    exact
    """
    worst_random = 0.0
    for name, (x, s, c, ts, tc) in cases.sincos_sets().items():
        (es, us), (ec, uc) = kr.sincos_errors(s, ts), kr.sincos_errors(c, tc)
        over = np.concatenate([es[us > kr.SINCOS_ULPS], ec[uc > kr.SINCOS_ULPS], [0.0]]).max()
        print(f"{name}: n {len(x)}; worst ulp sin {us.max():.2f} cos {uc.max():.2f}; worst absolute "
              f"{max(es.max(), ec.max()):.3g}; worst absolute where over {kr.SINCOS_ULPS} ulp {over:.3g}")
        assert kr.sincos_within_bound(s, ts).all() and kr.sincos_within_bound(c, tc).all(), name
        if name in ("[-pi, pi]", "[-1e5, 1e5]"):
            worst_random = max(worst_random, us.max(), uc.max())
            assert max(us.max(), uc.max()) <= kr.SINCOS_ULPS           # no help from the absolute term on the random sets
    # E is the measured maximum rounded up to the next half ulp, and a tighter function would get a tighter E
    assert kr.SINCOS_ULPS == math.ceil(2 * worst_random) / 2
    x, s, c, _, _ = cases.sincos_sets()["zero"]
    assert list(s) == [0.0, 0.0] and list(c) == [1.0, 1.0]
    assert not np.signbit(x[0]) and np.signbit(x[1])      # (the sine of -0 may be either zero: the reduction gives +0)


def test_sincos_reference_is_sound():
    """the judge itself: known values, and the ulp of a true value just under a power of two"""
    (sh, sl), (ch, cl) = kr.sincos_truth([math.pi / 6, 1.0])
    assert abs(sh[0] - 0.5) <= 2 ** -53 and abs((ch[1] + cl[1]) ** 2 + (sh[1] + sl[1]) ** 2 - 1.0) <= 2 ** -52
    assert sl[0] != 0.0                                   # the double nearest to pi / 6 is not pi / 6
    hi, lo = np.array([0.5, 0.5, 0.75]), np.array([-1e-20, 1e-20, 0.0])
    assert list(kr.ulp_of((hi, lo))) == [2.0 ** -54, 2.0 ** -53, 2.0 ** -53]


# ----------------------------------------------------------------------------------------------------------------------
# the probe robot of the device test, on the oracle
# ----------------------------------------------------------------------------------------------------------------------

def test_probe_robot_hands_out_sincos_on_the_oracle():
    """On the oracle the probe robot's sphere and planning link are at (cos q, sin q, 0) with the host function's bits for
    |q| <= pi.  Beyond, the sphere takes q as it is and the planning link the normalised angle: both hold the bits of
    smplx_sincos at that argument, and the bound of test_host_sincos_against_mpmath against mpmath there."""
    cfg = cases.probe_config()
    o = Oracle(cfg)
    inside, beyond = cases.probe_angles()
    assert len(inside) > 23000 and len(beyond) > 40000
    for x, n in ((inside, len(inside)), (beyond, 4000)):
        x = x[np.random.default_rng(5).permutation(len(x))[:n]] if n < len(x) else x
        S = np.stack([o.sphere_positions([q], 1)[0] for q in x])
        P = np.stack([o.planning_fk([q]) for q in x])
        xn = cases.normalized(x)
        s, c = cases.host_sincos(x)
        sn, cn = cases.host_sincos(xn)
        assert np.array_equal(S, np.stack([c, s, np.zeros(len(x))], 1))
        assert np.array_equal(P, np.stack([cn, sn, np.zeros(len(x))], 1))
        if x is inside:
            assert np.array_equal(xn, x)
        else:
            (ts, tc), (tsn, tcn) = kr.sincos_truth(x), kr.sincos_truth(xn)
            assert kr.sincos_within_bound(S[:, 1], ts).all() and kr.sincos_within_bound(S[:, 0], tc).all()
            assert kr.sincos_within_bound(P[:, 1], tsn).all() and kr.sincos_within_bound(P[:, 0], tcn).all()


# ----------------------------------------------------------------------------------------------------------------------
# the prismatic rule, pinned on purpose; the case generator's own kinematics
# ----------------------------------------------------------------------------------------------------------------------

def test_prismatic_axis_is_ignored(request):
    """transform_functions.h:218-226 moves a prismatic joint along the joint frame's Z whatever its axis says.  The mixed
    robot with the lift joint's axis changed from 1 0 0 to 0 1 0 gives bit-identical oracle positions, and moving lift
    displaces the mast's spheres along the joint frame's Z (0.1 m along it, 0.14 m from where the X axis would put them)."""
    cfg = cases.config("mixed", request)
    ref = cases.reference("mixed", cfg)
    line = [l for l in cfg.robot_text.splitlines() if l.startswith("joint lift prismatic")]
    assert len(line) == 1 and line[0].split()[11:14] == ["1", "0", "0"]
    w = line[0].split()
    w[11:14] = ["0", "1", "0"]
    import dataclasses
    other = dataclasses.replace(cfg, robot_text=cfg.robot_text.replace(line[0], " ".join(w)))
    assert other.robot_text != cfg.robot_text
    S, P = _oracle_positions(cfg, ref)
    S2, P2 = _oracle_positions(other, ref)
    assert np.array_equal(S, S2) and np.array_equal(P, P2)
    mast = [k for k, (l, _) in enumerate(ref.nodes) if l == "mast"]
    assert len(mast) == 3                                           # two leaves and their parent
    d = 0.1
    q0 = np.array(cfg.start); q1 = q0.copy(); q1[1] += d
    o = Oracle(cfg)
    move = o.sphere_positions(q1, len(ref.nodes))[mast] - o.sphere_positions(q0, len(ref.nodes))[mast]
    R, _ = ref.robot.frames(q0, ["mast"])["mast"]                   # a prismatic joint leaves the rotation alone
    z = np.array([float(R[i][2]) for i in range(3)]) * d
    x = np.array([float(R[i][0]) for i in range(3)]) * d
    assert np.abs(move - z).max() <= 2 * kr.BOUND
    assert np.abs(move - x).max() > 0.05
    hi0, _ = ref.robot.positions([q0], [ref.nodes[k] for k in mast])
    hi1, _ = ref.robot.positions([q1], [ref.nodes[k] for k in mast])
    assert np.abs((hi1 - hi0)[0] - z).max() <= 2 * kr.BOUND


@pytest.mark.parametrize("nv", width_cases.WIDTHS)
def test_chain_sphere_centres_agree_with_the_reference(nv):
    """width_cases.chain_sphere_centres, the numpy kinematics that places the boxes of the width cases, within 1e-12 m of
    the reference at the start and the goal of every case (the project's tolerance for a double-precision numpy chain)"""
    cfg = width_cases.width_case(nv)
    robot = kr.Robot(cfg.robot_text)
    nodes = [(f"l{v}", c[:3]) for v in range(nv) for c in robot.spheres[f"l{v}"]]
    for q in (cfg.start, cfg.goal):
        got = width_cases.chain_sphere_centres(nv, q)
        flat = np.array([c for v in range(nv) for c, _ in got[v]])
        radii = [r for v in range(nv) for _, r in got[v]]
        assert radii == [c[3] for v in range(nv) for c in robot.spheres[f"l{v}"]]
        err = kr.error(flat, tuple(a[0] for a in robot.positions([q], nodes))).max()
        assert err <= 1e-12, (nv, err)
