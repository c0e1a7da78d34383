"""A frontier step keeps each state's sines and cosines in its scratch (csrc/sphere_checks.h parent_trig): the collision
blocks and the successor role of k_pipe_configs take the pair of a variable whose value has the parent's bits from
there and evaluate smplx_sincos only for the variables an edge moves; k_pipe_setup (three launches) or k_pipe_prep
(four) writes the rows.  smplx_sincos is a function of its argument's bits, so nothing a caller sees may change.

Fixtures, shapes and helpers are those of tests/test_gpu_three_launch_step.py (used as they are): valid states among
scenes.benchmark_states(ARM7_LIMITS, 1200, 777) on the small scene, a pipeline-only space whose device table knows the
states of a 40-expansion search.  References: the oracle's eval_state rows, the four-launch step of the same space, and
the generic build (which keeps no table) of the same space.  Everything compared is integer or fp64 work in an
unchanged order: the tolerance is zero.
"""
import math

import numpy as np
import pytest

from smpl_amd import scenes
from test_gpu_step_round_trips import _assert_region_b_fields
from test_gpu_three_launch_step import (B_MAIN, GOAL_ROW, SIZES, START_ROW, _assert_oracle, _assert_same, _host_ids, _need_gpu,  # noqa: F401
                                        _run, _space, _work, batch, hip)

pytestmark = pytest.mark.gpu

INACTIVE, LIMITS, VALID = 0x10, 0x20, 0x01
DEG = math.pi / 180.0
SNAP = 2                                 # the snap primitive's slot among the three adaptive ones in front of the .mprim rows
NEAR_CELLS = [2, -1, 1, -2, 0, 1, 0]     # goal of the many-variable case: this many cells from row 0, five joints moved


def _oracle_rows(cfg, Q, goal):
    from oracle_binding import Oracle
    o = Oracle(cfg)
    o.set_order(chain=True)
    o.set_goal_joint(goal, cfg.goal_tol)
    rows = [o.eval_state(q) for q in Q]
    return o, {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}


def _space_for(cfg, goal, start, **kw):
    """_space() takes its goal and start from rows GOAL_ROW and START_ROW of what it is given."""
    rows = np.zeros((max(GOAL_ROW, START_ROW) + 1, len(goal)))
    rows[GOAL_ROW], rows[START_ROW] = goal, start
    return _space(cfg, rows, **kw)


def _changed(parent, sq):
    """Variables whose successor value does not have the parent's bits (-0.0 is not +0.0)."""
    return int((np.ascontiguousarray(sq).view(np.int64) != np.ascontiguousarray(parent).view(np.int64)).sum())


def _three_four_generic(hip, cfg, Q, exp, goal, start, sizes):
    """Each batch Q[:B]: three launches against the oracle, against four launches, and against the generic build."""
    s = _space_for(cfg, goal, start)
    g = _space_for(cfg, goal, start, generic_kernels=True)
    assert s.specialized()[0] and not g.specialized()[0]
    host = _host_ids(s)
    assert host == _host_ids(g)
    for B in sizes:
        three, = _run(hip, s, Q, [B])
        four, = _run(hip, s, Q, [B], prep=[True])
        gen, = _run(hip, g, Q, [B])
        _assert_oracle(three, exp, host, s.N)
        for other in (four, gen):
            _assert_same(three, other)
            _assert_region_b_fields(three, other, s.N, s.M)
    return s, host


def test_fixture_shapes(small_cfg, batch, hip):
    """B = 1, 6 (a state straddles two blocks at M = 25) and 300: dense outputs, lookups where the edge does not collide,
    the compact stream and region B field by field."""
    _need_gpu()
    Q, exp = batch
    _three_four_generic(hip, small_cfg, Q, exp, Q[GOAL_ROW], Q[START_ROW], SIZES)


def _crafted(cfg):
    st = np.array(cfg.start, dtype=np.float64)
    rows = [st.copy() for _ in range(5)]
    rows[0][4] += 2.0 * math.pi              # continuous: the normalised angle is not the raw one
    rows[1][4], rows[1][6] = 3.5, -7.0       # beyond pi, beyond -2 pi
    rows[2][4], rows[2][6] = -3.3, 9.5
    rows[3][2], rows[3][4] = -0.0, 0.0       # signed zero: -0.0 + alpha * 0.0 is +0.0, which counts as changed
    return np.array(rows)                    # (row 4: the start itself)


@pytest.mark.parametrize("goal_is", ["start", "crafted0"])
def test_crafted_parents(small_cfg, batch, hip, goal_is):
    """Parents whose continuous variables lie outside (-pi, pi] and a parent with -0.0, appended to the B = 6 batch; then
    the same step on a scratch full of 0xFF bytes, in three launches and in four, and on a zeroed one (the rows of the table
    are all written before they are read)."""
    _need_gpu()
    cfg = small_cfg
    Qb, _ = batch
    C = _crafted(cfg)
    Q = np.ascontiguousarray(np.vstack([Qb[:6], C]))
    goal = np.array(cfg.start) if goal_is == "start" else C[0]
    o, exp = _oracle_rows(cfg, Q, goal)
    crafted = exp["flags"][6:]
    assert all(o.state_valid(q)[0] for q in C)
    assert (((crafted & VALID) != 0).sum(axis=1) >= 14).all() and not (crafted & 0x40).any()
    assert np.signbit(C[3][2]) and _changed(C[0], np.array(cfg.start)) == 1
    s, host = _three_four_generic(hip, cfg, Q, exp, goal, cfg.start, [len(Q)])
    dirty, = _run(hip, s, Q, [len(Q)], work=_work(hip, s, 0xFF))
    clean, = _run(hip, s, Q, [len(Q)], work=_work(hip, s, 0))
    dirty4, = _run(hip, s, Q, [len(Q)], prep=[True], work=_work(hip, s, 0xFF))   # k_pipe_prep writes the rows
    _assert_oracle(dirty, exp, host, s.N)
    _assert_same(dirty, clean)
    _assert_same(dirty4, clean)


def test_edges_that_move_many_variables_share_a_wave_with_the_rest(small_cfg, batch, hip):
    """The goal lies a few cells from row 0 on five joints, so that row 0 has a valid snap edge.  On the oracle alone: the
    B = 6 batch holds a valid snap edge with at least 3 changed variables, an edge with exactly one and an edge with
    exactly two (an xy-rotated primitive), and the first wave of the first collision block -- items 0..63: the six
    states, then the waypoints 1..W-1 of block 0's edges in edge order -- mixes state items, waypoints of one-variable
    edges and waypoints of the snap edge."""
    _need_gpu()
    cfg = small_cfg
    Qb, _ = batch
    Q = np.ascontiguousarray(Qb[:6])
    goal = Q[0] + np.array(NEAR_CELLS) * DEG
    o, exp = _oracle_rows(cfg, Q, goal)
    M = exp["flags"].shape[1]
    assert M == 25
    items = [("state", 0)] * 6
    nchanged = {}
    for i in range(6):
        for p in range(M):
            if exp["flags"][i, p] & (INACTIVE | LIMITS):
                continue
            nchanged[i, p] = _changed(Q[i], exp["q"][i, p])
            W = o.waypoint_count(Q[i], exp["q"][i, p])
            if i * M + p < 128:   # an edge of setup's block 0, whose claim is the head of shard 0
                items += [("snap" if p == SNAP else "edge", nchanged[i, p])] * max(W - 1, 0)
    assert exp["flags"][0, SNAP] & VALID and nchanged[0, SNAP] >= 3
    assert 1 in nchanged.values() and 2 in nchanged.values()
    wave0 = set(items[:64])
    assert ("state", 0) in wave0 and ("edge", 1) in wave0 and ("snap", nchanged[0, SNAP]) in wave0
    assert o.waypoint_count(Q[0], exp["q"][0, SNAP]) > 2
    _three_four_generic(hip, cfg, Q, exp, goal, Q[START_ROW], [6])


@pytest.mark.parametrize("robot", ["dual14", "mixed"])
def test_other_robots(robot):
    """One pipeline step of the 14-variable dual arm and of the mixed-kinds robot (prismatic and general-axis joints, which
    keep taking the joint value) at their small test shapes, against the oracle's rows."""
    _need_gpu()
    from oracle_binding import Oracle
    from smpl_amd import capi
    from test_gpu_parity import _compare_expand
    if robot == "dual14":
        cfg = scenes.config5(n=64, nboxes=12, res=0.08)
        Q = np.vstack([np.array(cfg.start), scenes.random_states(scenes.ARM7_LIMITS + scenes.ARM7_LIMITS, 60, 32)])
    else:
        cfg = scenes.config_mixed()
        R = np.vstack([np.array(cfg.start), np.array(cfg.goal), scenes.random_states(scenes.MIXED_LIMITS, 120, 9)])
        Q = None
    o = Oracle(cfg)
    o.set_order(chain=True)
    s = capi.Space.from_config(cfg, no_small_kernel=True)
    assert s.specialized()[0]
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    if Q is None:
        Q = R[np.array([o.state_valid(q)[0] for q in R])][:48]
    got = _compare_expand(o, s, Q)
    assert (got["flags"] & VALID).sum() > 50
