"""The plain model of the lazy successor pair (tests/lazy_ref.py) held to the oracle proper, without a GPU.

For every state of every case of tests/test_gpu_lazy.py: the model's lazy successors that its own GetTrueCost accepts are, as
a set of (coordinate, goal mark), exactly the oracle's eager GetSuccs rows with the valid bit -- lazy generation followed
by the true cost is the eager expansion.  The census of the cases is pinned as well: it is what makes the GPU tests
meaningful (every verdict occurs, some items have several matching actions, a goal edge among them)."""
import numpy as np
import pytest

import lazy_ref
import width_cases as wc
from smpl_amd import scenes

WIDTH_CASES = ["nv1", "nv4", "nv15", "nv16", "M5", "M63"]
# (active edges, valid, refused by limits, refused by collision, goal successors among the valid) of the 300 states of a case
CENSUS = {
    "nv1": (603, 603, 0, 0, 1),
    "nv4": (2878, 2651, 227, 0, 8),
    "nv15": (3433, 2375, 1054, 4, 1),
    "nv16": (3623, 2536, 1022, 65, 1),
    "M5": (601, 601, 0, 0, 1),
    "M63": (8629, 5595, 2855, 179, 2),
    "small_cfg": (2712, 1756, 119, 837, 0),
}
# states with two active primitives that land in one cell
SHARED_CELLS = {"nv16": 5, "M63": 8}


def case(name, small_cfg):
    """(cfg, the 300 states, joint goal) of a case"""
    if name == "small_cfg":
        cfg = small_cfg
        return cfg, scenes.random_states(scenes.ARM7_LIMITS, 300, 21), lazy_ref.Goal.joint(cfg.goal, cfg.goal_tol)
    cfg = wc.case_config(name)
    return cfg, wc.batch_states(cfg), lazy_ref.Goal.joint(cfg.goal, cfg.goal_tol)


_TOTALS = {}


@pytest.mark.parametrize("name", WIDTH_CASES + ["small_cfg"])
def test_lazy_then_true_cost_is_the_eager_expansion(name, small_cfg):
    from oracle_binding import Oracle
    cfg, Q, goal = case(name, small_cfg)
    o = Oracle(cfg)
    o.set_order(chain=True)
    m = lazy_ref.LazyModel(o, cfg, goal)
    active = valid = limits = collided = goals = shared = multi_goal = 0
    multi_match = multi_goal_edge = 0
    for q in Q:
        acts = m.actions(q)
        active += len(acts)
        cells = [c for _, _, c, _ in acts]
        shared += len(cells) != len(set(cells))
        lazy_kept = set()
        for p, a, c, g in acts:
            v = m.verdict(q, a)
            valid += v == "ok"; limits += v == "limits"; collided += v == "collision"
            cost, prim, nmatch = m.true_cost_q(q, c)
            multi_match += nmatch >= 2
            assert nmatch >= 1 and (cost == lazy_ref.COST) == any(m.verdict(q, b) == "ok" for _, b, d, _ in acts if d == c)
            if g:
                gc, gp, gn = m.true_cost_q(q, None)
                if gc >= 0:
                    lazy_kept.add((c, True))       # (some action into the goal passes; this one may not be it)
            if cost >= 0 and not g:
                lazy_kept.add((c, False))
        ngoal = sum(1 for _, _, _, g in acts if g)
        multi_goal += ngoal >= 2
        multi_goal_edge += m.true_cost_q(q, None)[2] >= 2
        r = o.eval_state(q)
        ok = (r["flags"] & lazy_ref.F_VALID) != 0
        goals += int(((r["flags"] & lazy_ref.F_GOAL) != 0).sum())
        eager = {(tuple(int(x) for x in r["coord"][p]), bool(r["flags"][p] & lazy_ref.F_GOAL)) for p in np.nonzero(ok)[0]}
        # the model's kept set, action by action: an action is kept when IT passes (the set view of the eager rows)
        kept = {(c, g) for _, a, c, g in acts if m.verdict(q, a) == "ok"}
        assert kept == eager
        # ... and GetTrueCost, which answers per cell, keeps exactly the cells some passing action lands in
        assert {c for c, g in lazy_kept if not g} == {c for c, g in eager if not g}
        assert any(g for _, g in lazy_kept) == any(g for _, g in eager)
    print(f"{name}: active {active} valid {valid} limits {limits} collided {collided} goal {goals}; states with a shared cell {shared}, "
          f"with two goal successors {multi_goal}; items with >= 2 matches {multi_match}, goal edges with >= 2 {multi_goal_edge}")
    assert (active, valid, limits, collided, goals) == CENSUS[name]
    if name in SHARED_CELLS:
        assert shared == SHARED_CELLS[name]
    if name == "M63":
        assert multi_goal == 1
    _TOTALS[name] = (valid, limits, collided, multi_match, multi_goal_edge)


def test_every_verdict_occurs_often_enough():
    """over the cases together: each verdict at least 50 times, an item and a goal edge with two or more matching actions"""
    if len(_TOTALS) < len(CENSUS):
        pytest.fail("runs behind test_lazy_then_true_cost_is_the_eager_expansion of every case")
    t = np.array(list(_TOTALS.values())).sum(axis=0)
    assert t[0] >= 50 and t[1] >= 50 and t[2] >= 50
    assert t[3] >= 1 and t[4] >= 1
