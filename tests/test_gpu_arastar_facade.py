"""smpl_amd::GpuARAStar (include/smpl_amd/plugin.hpp), the mirror of smpl's ARAStar over the engine's own anytime search,
driven from C++ (tests/cpp/arastar_facade_driver.cpp) and compared line by line with the C-ABI and the oracle: chunks
bounded by expansions that continue one search, replan(0.0) with and without partial solutions, and
force_planning_from_scratch + replan(allowed_time) to completion; and a goal no state satisfies, where replan returns 0 with
an empty OPEN and leaves the caller's solution alone."""
import os
import subprocess

import pytest

from smpl_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("side", ["device", "host"])
def test_gpu_arastar_facade_matches_the_c_abi_and_the_oracle(small_cfg, tmp_path, side, monkeypatch):
    from oracle_binding import Oracle
    from smpl_amd.plugin_tools import build_driver, write_query
    cfg = small_cfg
    chunk = 1000
    exe = build_driver("arastar_facade_driver", tmp_path)
    write_query(cfg, tmp_path, [chunk])
    env = dict(os.environ, SMPLX_SEARCH=side)
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=env)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()

    o = Oracle(cfg)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    sid = o.set_start(cfg.start)
    o.search_params(5.0, 3.0, 1.0, True, False, 0, 0)
    eo = o.plan()
    path = " ".join(str(int(x)) for x in eo["path"])

    calls = [ln.split() for ln in lines if ln.startswith("call ")]
    assert len(calls) == (eo["expansions"] + chunk - 1) // chunk
    for k, c in enumerate(calls[:-1]):
        # (replan returns 1 once the search has a solution, time-outs while improving included: arastar.cpp:199-214)
        assert c[2] in ("0", "1") and c[3:] == [str(capi.ARA_TIMED_OUT), str(chunk), str(int(k > 0))], k
    assert calls[-1][2:4] == ["1", str(capi.ARA_SUCCESS)] and calls[-1][5] == str(int(len(calls) > 1))
    final = next(ln for ln in lines if ln.startswith("final ")).split()
    assert final[1:4] == ["1", str(eo["cost"]), str(eo["expansions"])]
    assert float(final[5]) == eo["eps"] and float(final[6]) == 5.0 and float(final[7]) == 3.0
    assert " ".join(final[8:]) == path

    # the same chunks through the C-ABI on a fresh space
    s = capi.Space.from_config(cfg, batch_states=256)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    assert s.set_start(cfg.start) == sid
    monkeypatch.setenv("SMPLX_SEARCH", side)
    r = [s.replan(5.0, 3.0, 1.0, True, True, chunk, chunk) for _ in calls][-1]
    assert r["result"] == capi.ARA_SUCCESS and r["expansions_init"] == int(final[4]) and r["cost"] == eo["cost"]

    assert next(ln for ln in lines if ln.startswith("zero ")) == f"zero 0 {capi.ARA_TIMED_OUT} 0 0"
    assert next(ln for ln in lines if ln.startswith("zero_partial ")) == f"zero_partial 1 {capi.ARA_PARTIAL} 0 0 {sid}"
    timed = next(ln for ln in lines if ln.startswith("timed ")).split()
    assert timed[1:5] == ["1", str(capi.ARA_SUCCESS), str(eo["cost"]), str(eo["expansions"])]
    assert float(timed[5]) == eo["eps"] and " ".join(timed[6:]) == path
    assert lines[-1] == "done"


@pytest.mark.parametrize("side", ["device", "host"])
def test_gpu_arastar_facade_on_an_exhausted_open_list(tmp_path, side):
    """GpuARAStar::replan for a goal that no state of the one-joint chain satisfies (width_cases.unreachable_goal): the
    search pops every reachable state and ends with an empty OPEN, so replan returns 0 (arastar.cpp:204-210) and touches
    neither the solution vector nor the cost; get_n_expands() is the oracle's count.  The same planner then plans to the
    reachable goal on the same space.  The result code expected of the engine is the plain loop's (arastar_loop.py)."""
    import dataclasses

    import numpy as np

    import width_cases as wc
    from arastar_loop import AraStarLoop
    from oracle_binding import Oracle
    from smpl_amd.plugin_tools import build_driver, write_query
    cfg = wc.width_case(1)
    bad = wc.unreachable_goal(1)
    exe = build_driver("arastar_facade_driver", tmp_path)
    write_query(dataclasses.replace(cfg, goal=bad), tmp_path, [0, 1, *[float(x) for x in cfg.goal]])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120,
                         env=dict(os.environ, SMPLX_SEARCH=side))
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    print("\n".join(ln[:200] for ln in lines))

    o = Oracle(cfg)
    o.set_goal_joint(bad, cfg.goal_tol)
    sid = o.set_start(cfg.start)
    o.search_params(5.0, 1.0, 1.0, True, False, 0, 0)
    eo = o.plan()
    p = Oracle(cfg)
    p.set_goal_joint(bad, cfg.goal_tol); p.set_start(cfg.start)
    want = AraStarLoop(p.get_succs, lambda i: 0 if i == 0 else p.heuristic_q(p.get_state(i)[0])).replan(sid, 0, 5.0, 1.0, 1.0)
    assert want["result"] == capi.ARA_EXHAUSTED and want["solved"] == 0 and np.array_equal(want["log"], eo["expansion_log"])
    n = eo["expansions"]
    # ret, result, call_expansions, get_n_expands, solved, path_len, the caller's cost, get_solution_eps, the caller's vector
    assert next(ln for ln in lines if ln.startswith("exhausted ")).split() == \
        ["exhausted", "0", str(want["result"]), str(n), str(n), "0", "0", "-3", "inf", "-7", "-7"]

    r = Oracle(cfg)
    r.set_goal_joint(cfg.goal, cfg.goal_tol); r.set_start(cfg.start)
    r.search_params(5.0, 1.0, 1.0, True, False, 0, 0)
    er = r.plan()
    assert er["ok"] == 1
    second = next(ln for ln in lines if ln.startswith("second ")).split()
    # ret, result, resumed, cost, get_n_expands, get_solution_eps, then the path: ids of this space, whose lattice started
    # over with the new goal -- held to its length, its ends and, through the cost, its edges
    assert second[1:6] == ["1", str(capi.ARA_SUCCESS), "0", str(er["cost"]), str(er["expansions"])] and float(second[6]) == er["eps"]
    assert len(second[7:]) == len(er["path"]) and second[7] == str(sid) and second[-1] == "0"
    assert lines[-1] == "done"
