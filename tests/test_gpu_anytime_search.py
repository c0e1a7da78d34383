"""Anytime ARA* (smplx_replan / smplx_replan_multi, include/smpl_amd.h): expansion and wall-clock budgets, searches that
continue between calls, partial solutions -- on the device-resident search and on the host-driven loop.  The oracle always
plans from scratch, so the checks rest on two facts: a search run in chunks pops what one uninterrupted search pops, and a
search stopped after k expansions has the oracle's k-bounded log as its log."""
import time

import numpy as np
import pytest

from smpl_amd import capi, scenes

pytestmark = pytest.mark.gpu
SIDES = ["device", "host"]
TO, PARTIAL, SUCCESS = capi.ARA_TIMED_OUT, capi.ARA_PARTIAL, capi.ARA_SUCCESS


def _need_gpu():
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _pair(cfg):
    from oracle_binding import Oracle
    o = Oracle(cfg)
    s = capi.Space.from_config(cfg, batch_states=256)
    o.set_goal_joint(cfg.goal, cfg.goal_tol); s.set_goal_joint(cfg.goal, cfg.goal_tol)
    assert o.set_start(cfg.start) == s.set_start(cfg.start)
    return o, s


def _start(s):
    return capi.lib().smplx_start_id(s.h)


def _oracle(o, eps0, final, improve=True, k=None):
    o.search_params(eps0, final, 1.0, improve, k is not None, k or 0, k or 0)
    return o.plan()


def _chunked(s, eps0, final, chunk, improve=True):
    calls = []
    while True:
        r = s.replan(eps0, final, 1.0, improve, True, chunk, chunk)
        calls.append(r)
        if r["result"] != TO:
            return calls
        assert len(calls) < 100000


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("chunk", [97, 1000])
def test_chunked_resume_equals_one_search(small_cfg, monkeypatch, side, chunk):
    monkeypatch.setenv("SMPLX_SEARCH", side)
    _need_gpu()
    o, s = _pair(small_cfg)
    eo = _oracle(o, 5.0, 3.0)
    calls = _chunked(s, 5.0, 3.0, chunk)
    last = calls[-1]
    for i, r in enumerate(calls[:-1]):
        assert r["result"] == TO and r["call_expansions"] == chunk, i
        assert r["resumed"] == (i > 0), i
    assert last["resumed"] == 1 and last["result"] == SUCCESS and last["call_expansions"] <= chunk
    assert sum(r["call_expansions"] for r in calls) == eo["expansions"] == last["expansions"]
    assert np.array_equal(last["expansion_log"], eo["expansion_log"])
    assert last["cost"] == eo["cost"] and np.array_equal(last["path"], eo["path"])
    assert last["satisfied_eps"] == eo["eps"] <= 3.0
    assert s.num_states() == o.num_states()
    assert sum(r["committed_succ_evals"] for r in calls) == eo["succ_evals"]
    n = s.num_states()
    for i in list(range(1, 200)) + list(range(200, n, 997)) + [n - 1]:
        assert np.array_equal(o.get_state(i)[0], s.get_state(i)[0]), i


@pytest.mark.parametrize("side", SIDES)
def test_lowering_final_eps_on_resume(small_cfg, monkeypatch, side):
    monkeypatch.setenv("SMPLX_SEARCH", side)
    _need_gpu()
    o, s = _pair(small_cfg)
    a = s.replan(5.0, 4.0, 1.0, True, False)
    assert a["result"] == SUCCESS and a["satisfied_eps"] == 4.0 and a["resumed"] == 0
    b = s.replan(5.0, 3.0, 1.0, True, False)
    assert b["resumed"] == 1 and b["result"] == SUCCESS
    eo = _oracle(o, 5.0, 3.0)
    assert np.array_equal(b["expansion_log"], eo["expansion_log"]) and b["expansions"] == eo["expansions"]
    assert b["cost"] == eo["cost"] and np.array_equal(b["path"], eo["path"]) and b["satisfied_eps"] == eo["eps"]
    assert a["call_expansions"] + b["call_expansions"] == eo["expansions"]


@pytest.mark.parametrize("side", SIDES)
def test_zero_wall_budget(small_cfg, monkeypatch, side):
    monkeypatch.setenv("SMPLX_SEARCH", side)
    _need_gpu()
    _, s = _pair(small_cfg)
    r = s.replan(5.0, 1.0, 1.0, True, True, wall=True, seconds_init=0.0, seconds=0.0, from_scratch=True)
    assert r["result"] == TO and r["call_expansions"] == 0 and r["solved"] == 0 and r["path_len"] == 0
    r = s.replan(5.0, 1.0, 1.0, True, True, wall=True, seconds_init=0.0, seconds=0.0, allow_partial=True, from_scratch=True)
    assert r["result"] == PARTIAL and r["solved"] == 1 and r["cost"] == 0 and r["call_expansions"] == 0
    assert r["path"].tolist() == [_start(s)]


@pytest.mark.parametrize("side", SIDES)
def test_partial_solution_after_k_expansions(small_cfg, monkeypatch, side):
    monkeypatch.setenv("SMPLX_SEARCH", side)
    _need_gpu()
    o, s = _pair(small_cfg)
    k = 300
    r = s.replan(5.0, 1.0, 1.0, True, True, k, k, allow_partial=True)
    assert r["result"] == PARTIAL and r["solved"] == 1 and r["call_expansions"] == k
    nxt = _oracle(o, 5.0, 1.0, k=k + 1)["expansion_log"]
    assert len(nxt) == k + 1
    assert np.array_equal(r["expansion_log"], nxt[:k])
    path = [int(x) for x in r["path"]]
    assert path[0] == _start(s) and path[-1] == int(nxt[-1]) and len(path) >= 2
    total = 0
    for a, b in zip(path, path[1:]):
        succ, cost = s.get_succs(a)
        c = [int(cc) for ss, cc in zip(succ, cost) if int(ss) == b]
        assert c, (a, b)
        total += min(c)
    assert total == r["cost"]


@pytest.mark.parametrize("side", SIDES)
def test_wall_budget_on_config2(monkeypatch, side):
    from oracle_binding import Oracle
    monkeypatch.setenv("SMPLX_SEARCH", side)
    _need_gpu()
    cfg = scenes.config2()
    s = capi.Space.from_config(cfg, batch_states=4096)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_start(cfg.start)
    eps0 = cfg.params.eps0
    t = time.perf_counter()
    a = s.replan(eps0, 1.0, 1.0, False, True, wall=True, seconds_init=0.05, seconds=0.05)
    dt = time.perf_counter() - t
    assert a["result"] == TO and a["call_expansions"] > 0 and dt < 0.5
    print(f"[anytime] {side}: 50 ms budget -> {dt * 1e3:.1f} ms in the call ({a['call_expansions']} expansions)")
    o = Oracle(cfg)
    o.set_goal_joint(cfg.goal, cfg.goal_tol); o.set_start(cfg.start)
    ko = _oracle(o, eps0, 1.0, improve=False, k=a["call_expansions"])
    assert np.array_equal(a["expansion_log"], ko["expansion_log"])
    b = s.replan(eps0, 1.0, 1.0, False, True, wall=True, seconds_init=120.0, seconds=120.0)
    assert b["resumed"] == 1 and b["result"] == SUCCESS
    f = capi.Space.from_config(cfg, batch_states=4096)
    f.set_goal_joint(cfg.goal, cfg.goal_tol); f.set_start(cfg.start)
    u = f.plan(eps0, 1.0, 1.0, False, False)
    assert b["cost"] == u["cost"] and np.array_equal(b["path"], u["path"]) and b["expansions"] == u["expansions"]
    assert np.array_equal(b["expansion_log"], u["expansion_log"]) and s.num_states() == f.num_states()


def _shard(cfg):
    DEG = np.pi / 180.0
    rng = np.random.default_rng(3)
    cells = rng.integers(-6, 7, size=(16, 7)) * np.array([7, 7, 7, 7, 4, 4, 4])
    goals = [[cfg.start[i] + c * DEG for i, c in enumerate(cs)] for cs in cells]
    grid = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    model = capi.Model(cfg.robot_text)
    probe = capi.Space(model, grid, cfg.mprim, cfg.params, 256)
    ok = probe.state_valid_batch(np.array(goals))[0].astype(bool)
    goals = [g for g, k in zip(goals, ok) if k]
    assert len(goals) >= 8

    def make():
        out = []
        for g in goals:
            sp = capi.Space(model, grid, cfg.mprim, cfg.params, 512)
            sp.set_goal_joint(g, cfg.goal_tol); sp.set_start(cfg.start)
            out.append(sp)
        return out
    return make


@pytest.mark.parametrize("side,threads", [("device", 1), ("host", 1), ("host", 4)])
def test_multi_query_budgets(small_cfg, monkeypatch, side, threads):
    monkeypatch.setenv("SMPLX_SEARCH", side)
    _need_gpu()
    make = _shard(small_cfg)
    # (some of the goals need far more expansions than a test can wait for: every search is bounded, 31 chunks of 97)
    chunk, nchunks = 97, 31
    solo = [sp.plan(5.0, 5.0, 1.0, False, True, chunk * nchunks, chunk * nchunks) for sp in make()]
    sp = make()
    for k in range(nchunks):
        rs, _ = capi.Space.replan_multi(sp, 5.0, 5.0, 1.0, False, True, chunk, chunk, host_threads=threads)
        assert all(r["resumed"] == (k > 0) for r in rs)
        assert all(r["result"] != TO or r["call_expansions"] == chunk for r in rs)
    assert any(r["result"] == SUCCESS for r in rs)
    for a, r in zip(solo, rs):
        assert a["solved"] == r["solved"] and a["cost"] == r["cost"] and np.array_equal(a["path"], r["path"])
        assert np.array_equal(a["expansion_log"], r["expansion_log"]) and a["expansions"] == r["expansions"]
    rs, _ = capi.Space.replan_multi(make(), 5.0, 5.0, 1.0, False, True, wall=True, seconds_init=0.0, seconds=0.0,
                                    host_threads=threads)
    assert all(r["result"] == TO and r["call_expansions"] == 0 for r in rs)
    rs, wall = capi.Space.replan_multi(make(), 5.0, 5.0, 1.0, False, True, wall=True, seconds_init=0.02, seconds=0.02,
                                       host_threads=threads)
    print(f"[anytime] {side} x{threads}: 16 queries, 20 ms budget -> {wall * 1e3:.1f} ms in the call")
    for a, r in zip(solo, rs):
        n = len(r["expansion_log"])
        assert n == r["call_expansions"] and np.array_equal(r["expansion_log"], a["expansion_log"][:n])


@pytest.mark.parametrize("side", SIDES)
def test_when_a_call_resumes_or_starts_over(small_cfg, monkeypatch, side):
    monkeypatch.setenv("SMPLX_SEARCH", side)
    _need_gpu()
    DEG = np.pi / 180.0

    def fresh(start=None):
        f = capi.Space.from_config(small_cfg, batch_states=256)
        f.set_goal_joint(small_cfg.goal, small_cfg.goal_tol)
        f.set_start(small_cfg.start if start is None else start)
        return f.replan(5.0, 4.0, 1.0, True, True, 1500, 1500)

    def same(a, b):
        assert a["result"] == b["result"] and a["cost"] == b["cost"] and np.array_equal(a["path"], b["path"])
        assert np.array_equal(a["expansion_log"], b["expansion_log"]) and a["expansions"] == b["expansions"]

    _, s = _pair(small_cfg)
    want = fresh()
    a = s.replan(5.0, 4.0, 1.0, True, True, 1500, 1500)
    assert a["resumed"] == 0
    same(a, want)
    b = s.replan(5.0, 4.0, 1.0, True, True, 1500, 1500, from_scratch=True)
    assert b["resumed"] == 0
    same(b, want)
    if a["satisfied_eps"] <= 4.0:
        c = s.replan(5.0, 4.0, 1.0, True, True, 1500, 1500)
        assert c["resumed"] == 1 and c["call_expansions"] == 0 and c["cost"] == a["cost"] and np.array_equal(c["path"], a["path"])
    other = np.array(small_cfg.start) + np.array([7, 0, 7, 0, 0, 0, 4]) * DEG
    s.set_start(other)
    d = s.replan(5.0, 4.0, 1.0, True, True, 1500, 1500)
    assert d["resumed"] == 0
    # (the lattice is shared with the first search: compare what does not depend on state ids)
    fo = fresh(other)
    assert d["result"] == fo["result"] and d["cost"] == fo["cost"]
    s.set_goal_joint(small_cfg.goal, small_cfg.goal_tol)
    s.set_start(small_cfg.start)
    e = s.replan(5.0, 4.0, 1.0, True, True, 1500, 1500)
    assert e["resumed"] == 0
    same(e, want)
