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


@pytest.mark.parametrize("kind", ["euclid", "joint_distance"])
def test_near_start_reaches_the_goal_in_the_first_iteration(small_cfg, kind):
    """the choice of heuristic_cases.NEAR and of the budget, by the loop on the oracle's successors"""
    r = hc.first_iteration_on_the_oracle(small_cfg, kind, hc.start_of(small_cfg, True))
    print(kind, "from NEAR on the oracle's successors:", r["expansions"], "expansions, cost", r["cost"])
    assert r["solved"] == 1 and r["path"][-1] == 0 and 5 <= r["expansions"] <= hc.SEARCH[5] // 10
