"""One GetSuccs loop body for every expansion kernel: the four shared steps (successor joint values, metric goal distance,
goal test plus heuristic in csrc/lattice_steps.h; waypoint count in csrc/config_checks.h) are reached through six launch paths, and every path
must leave the oracle's bits for the same rows.

Inputs: 37 states of the 7-DOF arm on the small scene -- the start, the goal, the goal with each joint moved by 4 degrees
either way (within the short-primitive and the snap thresholds), one state on a joint limit, random states.  37 x 25
edges are 8 pipeline blocks of 128 threads, the last one ragged, with states straddling every block boundary.  Each path
runs once with a joint goal and once with an XYZ goal (the planning-link position of the same goal state).  Everything
is integer or fp64 work in one order: the tolerance is zero.
"""
import numpy as np
import pytest

from smpl_amd import scenes

pytestmark = pytest.mark.gpu

B = 37
XYZ_TOL = [0.04] * 3
TINY_WORK_LIST_ITEMS = 8 * 16     # what capi.Space(tiny_work_list=True) leaves of the work list
# (name, Space.from_config arguments, k_pipe_prep in a launch of its own)
PATHS = [("fused", dict(fused=True), False),
         ("pipeline", dict(no_small_kernel=True), False),
         ("pipeline, k_pipe_prep in front", dict(no_small_kernel=True), True),
         ("pipeline, edges deferred", dict(no_small_kernel=True, tiny_work_list=True), False),
         ("small batch", dict(), False),
         ("generic kernels", dict(no_small_kernel=True, generic_kernels=True), False)]


def _states(cfg):
    g = np.array(cfg.goal)
    Q = [np.array(cfg.start), g]
    for k in range(7):
        for sign in (1.0, -1.0):
            q = g.copy(); q[k] += sign * 4 * scenes.DEG; Q.append(q)
    q = np.array(cfg.start); q[3] = scenes.ARM7_LIMITS[3][1]; Q.append(q)     # on a limit: a primitive steps over it
    Q = np.vstack([np.array(Q), scenes.random_states(scenes.ARM7_LIMITS, B - len(Q), 1)])
    assert Q.shape == (B, 7)
    return np.ascontiguousarray(Q)


def _set_goal(x, o, cfg, goal_kind):
    if goal_kind == "joint":
        x.set_goal_joint(cfg.goal, cfg.goal_tol)
    else:
        x.set_goal_xyz(o.planning_fk(cfg.goal), XYZ_TOL)


@pytest.fixture(scope="module", params=["joint", "xyz"])
def rows(small_cfg, request):
    """(goal kind, oracle, Q, the oracle's GetSuccs loop body for every row, waypoint count per checked edge, validity of
    the states themselves)."""
    from oracle_binding import Oracle
    o = Oracle(small_cfg)
    o.set_order(chain=True)
    _set_goal(o, o, small_cfg, request.param)
    Q = _states(small_cfg)
    per_state = [o.eval_state(q) for q in Q]
    exp = {k: np.stack([r[k] for r in per_state]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}
    checked = (exp["flags"] & 0x30) == 0          # evaluated and within the limits: the edges that have waypoints
    W = np.zeros(checked.shape, np.int64)
    for i, p in zip(*np.nonzero(checked)):
        W[i, p] = o.waypoint_count(Q[i], exp["q"][i, p])
    state_ok = np.array([o.state_valid(q)[0] for q in Q])
    return request.param, o, Q, exp, W, state_ok


def test_rows_reach_every_branch(rows):
    """Conditions on the input, on the oracle's output alone: every verdict occurs, an edge has no waypoints, and the work
    list of the deferring path cannot hold the batch."""
    goal_kind, o, Q, exp, W, state_ok = rows
    f = exp["flags"]
    assert f.shape == (B, 25)
    checked = (f & 0x30) == 0
    for bit in (0x10, 0x20, 0x40, 1, 2):          # inactive, limits, collision, valid, goal
        assert ((f & bit) != 0).any(), hex(bit)
    coll = (f & 0x40) != 0                        # both ways to collide: on a waypoint of its own, on the state itself
    assert coll[state_ok].any() and coll[~state_ok].any()
    if goal_kind == "joint":
        assert (checked & (W == 0) & ((f & 2) != 0)).any()    # the goal's own snap: no motion, a goal successor
    else:
        # under an XYZ goal the snap has no action, and no other primitive leaves a state where it is
        assert not (checked & (W == 0)).any()
    assert np.maximum(W - 1, 0).sum() > TINY_WORK_LIST_ITEMS


def _assert_oracle(got, exp, name):
    f = exp["flags"]
    assert np.array_equal(got["flags"], f), name
    valid, evaluated, coll = (f & 1) != 0, (f & 0x10) == 0, (f & 0x40) != 0
    assert np.array_equal(got["coord"][valid], exp["coord"][valid]), name
    assert np.array_equal(got["q"][evaluated], exp["q"][evaluated]), name
    assert np.array_equal(got["h"][valid], exp["h"][valid]) and not got["h"][~valid].any(), name
    assert np.array_equal(got["cost"][valid], exp["cost"][valid]) and not got["cost"][~valid].any(), name
    assert np.array_equal(got["lookups"][~coll], exp["lookups"][~coll]), name


def test_six_launch_paths_leave_the_same_rows(small_cfg, rows):
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    goal_kind, o, Q, exp = rows[:4]
    f = exp["flags"]
    valid, evaluated, coll = (f & 1) != 0, (f & 0x10) == 0, (f & 0x40) != 0
    first = None
    for name, kw, prep in PATHS:
        s = capi.Space.from_config(small_cfg, **kw)
        assert s.specialized()[0] == (not kw.get("generic_kernels", False)), name
        _set_goal(s, o, small_cfg, goal_kind)
        if prep:
            s.set_pipe_prep(True)
        got = s.expand_batch(Q)
        s.close()
        _assert_oracle(got, exp, name)
        if kw.get("fused"):
            # one thread walks an edge in the reference's order with its early exit: the tally of a colliding edge is the
            # oracle's too, which no waypoint-parallel path promises -- this run did take k_expand
            assert np.array_equal(got["lookups"], exp["lookups"]), name
        if first is None:
            first = got
            continue
        for k in ("flags", "h", "cost"):
            assert np.array_equal(got[k], first[k]), (name, k)
        assert np.array_equal(got["coord"][valid], first["coord"][valid]), name
        assert np.array_equal(got["q"][evaluated], first["q"][evaluated]), name
        assert np.array_equal(got["lookups"][~coll], first["lookups"][~coll]), name
