"""tests/arastar_loop.py, the plain Python ARA* loop, without a GPU: over the oracle's successors and heuristic its expansion
log, path, cost and satisfied eps are the oracle's own search's, id for id -- so the loop may serve as the outside reference of
the engine's searches under the heuristic kinds the oracle does not have (tests/test_gpu_heuristic_kinds.py) -- and from the
NEAR start of heuristic_cases.py the first iteration of a bounded search reaches the joint goal under both closed forms."""
import numpy as np
import pytest

import heuristic_cases as hc
from arastar_loop import AraStarLoop
from oracle_binding import Oracle


@pytest.mark.parametrize("search", [(5.0, 1.0, 1.0, 1500, 1500), (2.0, 1.0, 1.0, 2500, 2500), (5.0, 3.0, 1.0, 0, 0)],
                         ids=["eps5-bounded", "eps2-bounded", "eps5-to-3-unbounded"])
def test_loop_is_the_oracles_search(small_cfg, search):
    cfg = small_cfg
    eps0, fin, delta, mi, mr = search
    o = Oracle(cfg)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    o.set_start(cfg.start)
    o.search_params(eps0, fin, delta, True, mi > 0, mi, mr)
    e = o.plan()
    p = Oracle(cfg)
    p.set_goal_joint(cfg.goal, cfg.goal_tol)
    sid = p.set_start(cfg.start)
    r = AraStarLoop(p.get_succs, lambda i: 0 if i == 0 else p.heuristic_q(p.get_state(i)[0])).replan(sid, 0, eps0, fin, delta, mi, mr)
    assert e["expansions"] > 500                       # several iterations, with reorderings of OPEN between them
    assert r["solved"] == e["ok"] and r["expansions"] == e["expansions"]
    assert np.array_equal(r["log"], e["expansion_log"])
    assert r["cost"] == e["cost"] and np.array_equal(r["path"], e["path"]) and r["satisfied_eps"] == e["eps"]
    assert p.num_states() == o.num_states()


def _unreachable(nv):
    import width_cases as wc
    cfg = wc.width_case(nv)
    o = Oracle(cfg)
    o.set_goal_joint(wc.unreachable_goal(nv), cfg.goal_tol)
    return cfg, o, o.set_start(cfg.start)


@pytest.mark.parametrize("eps0", [5.0, 1.0])
@pytest.mark.parametrize("nv", [1, 2])
def test_loop_exhausts_open_as_the_oracle_does(nv, eps0):
    """A goal no lattice state satisfies (width_cases.unreachable_goal): the oracle's search and the loop over the oracle's
    successors pop every reachable state once, in the same order, and end with an empty OPEN -- EXHAUSTED_OPEN_LIST, no
    solution, with or without partial solutions allowed.  tests/test_gpu_search_endings.py takes the result codes it expects
    of the engine from this loop."""
    cfg, o, _ = _unreachable(nv)
    o.search_params(eps0, 1.0, 1.0, True, False, 0, 0)
    e = o.plan()
    cfg, p, sid = _unreachable(nv)
    loop = AraStarLoop(p.get_succs, lambda i: 0 if i == 0 else p.heuristic_q(p.get_state(i)[0]))
    r = loop.replan(sid, 0, eps0, 1.0, 1.0)
    print(f"chain{nv} eps {eps0}: {len(r['log'])} pops, {p.num_states()} states")
    assert r["result"] == 5 and r["solved"] == 0 and r["path"] == [] and r["cost"] == 0 and r["satisfied_eps"] == np.inf
    assert e["ok"] == 0 and len(e["path"]) == 0 and e["eps"] == np.inf
    assert r["expansions"] == r["call_expansions"] == e["expansions"] == len(r["log"])
    assert np.array_equal(r["log"], e["expansion_log"])
    # every state but the goal's entry was popped once: the log is the whole reachable lattice
    assert p.num_states() == o.num_states() and len(r["log"]) == p.num_states() - 1
    assert sorted(r["log"]) == list(range(1, p.num_states()))
    # OPEN is empty: nothing to return as a partial solution, and a further call has nothing to pop
    a = loop.replan(sid, 0, eps0, 1.0, 1.0, resume=True, allow_partial=True)
    assert a["result"] == 5 and a["solved"] == 0 and a["path"] == [] and a["call_expansions"] == 0 and a["log"] == r["log"]
    a = loop.replan(sid, 0, eps0, 1.0, 1.0, allow_partial=True)
    assert a["result"] == 5 and a["solved"] == 0 and a["path"] == [] and a["log"] == r["log"]


def test_loop_in_chunks_and_with_partial_solutions():
    """The two switches the GPU tests lean on, against the oracle: a search continued in chunks of 997 pops is the
    uninterrupted search (every chunk but the last TIMED_OUT at its budget, the last EXHAUSTED_OPEN_LIST), and the partial
    solution after k pops is the bp chain of the state the oracle's k + 1-bounded search pops last."""
    cfg, o, _ = _unreachable(2)
    o.search_params(5.0, 1.0, 1.0, True, False, 0, 0)
    e = o.plan()
    cfg, p, sid = _unreachable(2)
    loop = AraStarLoop(p.get_succs, lambda i: 0 if i == 0 else p.heuristic_q(p.get_state(i)[0]))
    calls = [loop.replan(sid, 0, 5.0, 1.0, 1.0, 997, 997)]
    while calls[-1]["result"] == 4:
        calls.append(loop.replan(sid, 0, 5.0, 1.0, 1.0, 997, 997, resume=True))
        assert len(calls) < 100
    assert [c["result"] for c in calls] == [4] * (len(calls) - 1) + [5] and len(calls) >= 3
    assert all(c["call_expansions"] == 997 for c in calls[:-1])
    assert sum(c["call_expansions"] for c in calls) == calls[-1]["expansions"] == e["expansions"]
    assert np.array_equal(calls[-1]["log"], e["expansion_log"])

    import width_cases as wc
    cfg = wc.width_case(1)
    k = 300
    o = Oracle(cfg)
    o.set_goal_joint(cfg.goal, cfg.goal_tol); sid = o.set_start(cfg.start)
    o.search_params(5.0, 1.0, 1.0, True, True, k + 1, k + 1)
    nxt = o.plan()["expansion_log"]
    p = Oracle(cfg)
    p.set_goal_joint(cfg.goal, cfg.goal_tol); p.set_start(cfg.start)
    r = AraStarLoop(p.get_succs, lambda i: 0 if i == 0 else p.heuristic_q(p.get_state(i)[0])).replan(
        sid, 0, 5.0, 1.0, 1.0, k, k, allow_partial=True)
    assert r["result"] == 4 and r["solved"] == 1 and r["satisfied_eps"] == np.inf and r["call_expansions"] == k
    assert len(nxt) == k + 1 and np.array_equal(r["log"], nxt[:k])
    assert r["path"][0] == sid and r["path"][-1] == int(nxt[-1])
    total = 0
    for a, b in zip(r["path"], r["path"][1:]):
        succ, cost = p.get_succs(a)
        total += min(int(c) for s, c in zip(succ, cost) if int(s) == b)
    assert total == r["cost"]


@pytest.mark.parametrize("kind", ["euclid", "joint_distance"])
def test_near_start_reaches_the_goal_in_the_first_iteration(small_cfg, kind):
    """the choice of heuristic_cases.NEAR and of the budget, by the loop on the oracle's successors"""
    r = hc.first_iteration_on_the_oracle(small_cfg, kind, hc.start_of(small_cfg, True))
    print(kind, "from NEAR on the oracle's successors:", r["expansions"], "expansions, cost", r["cost"])
    assert r["solved"] == 1 and r["path"][-1] == 0 and 5 <= r["expansions"] <= hc.SEARCH[5] // 10
