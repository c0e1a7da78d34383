"""Shared by the tests of the closed-form heuristic kinds (tests/test_heuristics_host.py, tests/test_arastar_loop.py,
tests/test_gpu_heuristic_kinds.py): the weight sets, the numpy forms of the two distances, and the start from which the
searches are run, with the check -- by the plain ARA* loop over the ORACLE's successors and a numpy heuristic, no engine
involved -- that the first iteration of a bounded search reaches the joint goal from it."""
import math

import numpy as np

import pose_goal_ref as ref
from smpl_amd import scenes

WEIGHTS = [(1.0, 1.0, 1.0, 1.0), (2.0, 0.5, 3.0, 0.25), (1.0, 0.0, 1.0, 40.0)]      # the last: a zero in one place

# eps 10 -> 1 in steps of 3, bounded: 3000 expansions for the first iteration, 600 for each later one
SEARCH = (10.0, 1.0, 3.0, True, True, 3000, 600)
# A closed-form heuristic knows nothing of the obstacles or of how the arm folds: from small_cfg's own start the bounded
# first iteration does not reach the joint goal under either kind.  NEAR is a start a few long primitives from the goal
# configuration, from which it does (first_iteration_on_the_oracle: 12 expansions under the Euclidean h, 27 under joint
# distance, against the budget of 3000).
NEAR = np.array([12.0, -8.0, 10.0, -10.0, 14.0, -10.0, 16.0]) * scenes.DEG


def start_of(cfg, near=True):
    return np.array(cfg.goal) + NEAR if near else np.array(cfg.start)


def np_pose_distance(Ta, Tb, w):
    """EuclidDistHeuristic::computeDistance in numpy; the angle by atan2 (pose_goal_ref.rotation_angle), not acos"""
    d = Tb[:3, 3] - Ta[:3, 3]
    th = ref.rotation_angle(Ta[:3, :3], Tb[:3, :3])
    return math.sqrt(w[0] * d[0] ** 2 + w[1] * d[1] ** 2 + w[2] * d[2] ** 2 + w[3] * th ** 2)


def np_joint_distance(a, b):
    d = 0.0
    for x, y in zip(a, b):
        dj = float(x) - float(y)
        d += dj * dj
    return math.sqrt(d)


def first_iteration_on_the_oracle(cfg, kind, start, eps0=SEARCH[0], budget=SEARCH[5]):
    """The plain ARA* loop (arastar_loop.py) over the oracle's GetSuccs with the numpy heuristic of `kind` ("euclid" or
    "joint_distance"), one iteration at eps0 within `budget` expansions.  The oracle gates its primitives by the BFS, so
    this is the engine's search only in outline; it serves to choose a start and a budget, not as a reference."""
    from arastar_loop import AraStarLoop
    from oracle_binding import Oracle
    o = Oracle(cfg)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    sid = o.set_start(start)
    if kind == "euclid":
        chain = ref.Chain(cfg.robot_text)
        Tg = chain.transform(np.array(cfg.goal))
        h = lambda i: 0 if i == 0 else int(1000.0 * np_pose_distance(chain.transform(o.get_state(i)[0]), Tg, WEIGHTS[0]))
    else:
        h = lambda i: 0 if i == 0 else int(1000.0 * np_joint_distance(o.get_state(i)[0], cfg.goal))
    return AraStarLoop(o.get_succs, h).replan(sid, 0, eps0, eps0, 1.0, budget, budget)
