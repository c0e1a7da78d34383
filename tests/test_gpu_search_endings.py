"""Every way a search ends (smplx_replan / smplx_replan_multi / smplx_plan, include/smpl_amd.h), on the device-resident search
and on the host-driven loop: an OPEN list that runs empty (SMPLX_ARA_EXHAUSTED), alone, with partial solutions allowed, in
chunks, while the buffers and the state table are outgrown, and followed by another goal on the same space; a solution
longer than the device search's path buffer; and shards whose queries end differently.

The scenes are the one- and two-joint chains of width_cases.py.  width_cases.unreachable_goal(nv) is a goal that no state
inside the joint limits satisfies: the search for it pops every reachable state exactly once -- 573 states at nv = 1 and 7 500
at nv = 2 when this was written; nothing here depends on the numbers -- so its expansion log is the whole reachable lattice
in the oracle's order, and a slip at the joint limits, in the collision gate or in the state table shows in it.

What is expected comes from the oracle (logs, paths, costs, states) and from the plain loop of arastar_loop.py over the
oracle's successors (result codes, partial solutions, the calls of a search run in chunks); tests/test_arastar_loop.py
holds the two to each other.  Nothing expected comes from the engine, except where a test says that two runs of the engine
must agree.  Every comparison is of integers, or of doubles that both sides copy from the same lattice."""
import functools

import numpy as np
import pytest

import width_cases as wc
from arastar_loop import AraStarLoop
from smpl_amd import capi

pytestmark = pytest.mark.gpu
TO, PARTIAL, SUCCESS, EXHAUSTED = capi.ARA_TIMED_OUT, capi.ARA_PARTIAL, capi.ARA_SUCCESS, capi.ARA_EXHAUSTED
EPS = (5.0, 1.0, 1.0)
# (side, nv, generic kernels): both chains on the per-robot kernels, the one-joint chain on the kernels linked into the library
BUILDS = [(side, nv, generic) for nv, generic in ((1, False), (2, False), (1, True)) for side in ("device", "host")]
BUILD_IDS = [f"{side}-nv{nv}{'-generic' if generic else ''}" for side, nv, generic in BUILDS]
CHUNK = {1: 97, 2: 997}         # pops per call of the searches run in chunks
SHARD_BUDGET = 3000             # pops per call of the shards
PARTIAL_K = 300                 # pops before the partial solution of the one-joint chain


def _need_gpu():
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


@pytest.fixture(scope="module", autouse=True)
def kernels_built():
    """the first space of a robot compiles its per-robot kernels: here, not in a test's own time"""
    _need_gpu()
    for nv in (1, 2):
        capi.Space.from_config(wc.width_case(nv), batch_states=16).close()


def _goal(nv, reachable):
    return list(wc.width_case(nv).goal) if reachable else wc.unreachable_goal(nv)


def _oracle(nv, reachable):
    from oracle_binding import Oracle
    cfg = wc.width_case(nv)
    o = Oracle(cfg)
    o.set_goal_joint(_goal(nv, reachable), cfg.goal_tol)
    return o, o.set_start(cfg.start)


def _loop(nv, reachable):
    o, sid = _oracle(nv, reachable)
    return sid, AraStarLoop(o.get_succs, lambda i: 0 if i == 0 else o.heuristic_q(o.get_state(i)[0]))


@functools.lru_cache(maxsize=None)
def _truth(nv, reachable):
    """the unbounded search eps 5 -> 1 by the oracle, every state of its lattice, and the plain loop's result of the same search"""
    o, sid = _oracle(nv, reachable)
    o.search_params(*EPS, True, False, 0, 0)
    eo = o.plan()
    states = [o.get_state(i) for i in range(o.num_states())]
    lsid, loop = _loop(nv, reachable)
    lr = loop.replan(lsid, 0, *EPS)
    assert lsid == sid and np.array_equal(lr["log"], eo["expansion_log"]) and lr["solved"] == eo["ok"]
    if reachable:
        assert lr["result"] == SUCCESS and eo["ok"] == 1 and np.array_equal(lr["path"], eo["path"]) and lr["cost"] == eo["cost"]
    else:
        assert lr["result"] == EXHAUSTED and eo["ok"] == 0 and len(eo["expansion_log"]) == len(states) - 1
    return dict(sid=sid, eo=eo, states=states, loop=lr)


@functools.lru_cache(maxsize=None)
def _loop_calls(nv, reachable, budget, ncalls=None):
    """the plain loop's calls of a search bounded by `budget` pops per call and continued until it no longer times out (or
    for ncalls calls): [(result, call_expansions, solved)]"""
    sid, loop = _loop(nv, reachable)
    calls = [loop.replan(sid, 0, *EPS, budget, budget)]
    while (calls[-1]["result"] == TO) if ncalls is None else (len(calls) < ncalls):
        calls.append(loop.replan(sid, 0, *EPS, budget, budget, resume=True))
        assert len(calls) < 1000
    return [(c["result"], c["call_expansions"], c["solved"]) for c in calls]


def _space(nv, reachable=False, generic=False, **kw):
    cfg = wc.width_case(nv)
    s = capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic, **kw)
    assert s.specialized()[0] == (not generic), s.specialized()[1]
    s.set_goal_joint(_goal(nv, reachable), cfg.goal_tol)
    assert s.set_start(cfg.start) == _truth(nv, reachable)["sid"]
    return s


def _assert_exhausted(r, t, calls=None):
    """r: the call after which OPEN was empty; t: _truth of the unreachable goal"""
    eo, want = t["eo"], t["loop"]
    print(f"result {r['result']} solved {r['solved']} path_len {r['path_len']} cost {r['cost']} eps {r['satisfied_eps']} "
          f"expansions {r['expansions']} (oracle {eo['expansions']}) log {len(r['expansion_log'])}")
    assert want["result"] == EXHAUSTED and want["solved"] == 0
    assert r["result"] == want["result"] and r["solved"] == want["solved"]
    assert r["path_len"] == 0 and len(r["path"]) == 0 and r["cost"] == 0 and r["satisfied_eps"] == np.inf == eo["eps"]
    assert r["expansions"] == eo["expansions"] == len(eo["expansion_log"])
    assert np.array_equal(r["expansion_log"], eo["expansion_log"])
    if calls is None:
        assert r["call_expansions"] == eo["expansions"]


def _assert_lattice(s, t):
    assert s.num_states() == len(t["states"])
    for i in range(1, len(t["states"])):
        q, c = s.get_state(i)
        assert np.array_equal(c, t["states"][i][1]) and np.array_equal(q, t["states"][i][0]), i


# ----------------------------------------------------------------------------------------------------------------------
# an OPEN list that runs empty
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side,nv,generic", BUILDS, ids=BUILD_IDS)
def test_exhausted_from_scratch(monkeypatch, side, nv, generic):
    """One unbounded replan: SMPLX_ARA_EXHAUSTED, no solution, the oracle's log element for element and the oracle's whole
    lattice state for state; smplx_plan on a fresh space pops the same."""
    monkeypatch.setenv("SMPLX_SEARCH", side)
    t = _truth(nv, False)
    s = _space(nv, generic=generic)
    r = s.replan(*EPS, improve=True, bounded=False)
    assert r["resumed"] == 0
    _assert_exhausted(r, t)
    _assert_lattice(s, t)
    f = _space(nv, generic=generic)
    p = f.plan(*EPS, True, False)
    assert p["solved"] == 0 and p["path_len"] == 0 and p["cost"] == 0 and p["satisfied_eps"] == np.inf
    assert p["expansions"] == t["eo"]["expansions"] and np.array_equal(p["expansion_log"], t["eo"]["expansion_log"])
    assert f.num_states() == len(t["states"])
    # a search at eps 1 alone pops the same set: every reachable state, once
    one = _space(nv, generic=generic).replan(1.0, 1.0, 1.0, improve=True, bounded=False)
    assert one["result"] == EXHAUSTED and one["solved"] == 0 and one["expansions"] == t["eo"]["expansions"]
    assert sorted(one["expansion_log"].tolist()) == list(range(1, len(t["states"])))


@pytest.mark.parametrize("side,nv,generic", BUILDS, ids=BUILD_IDS)
def test_exhausted_with_partial_solutions_allowed(monkeypatch, side, nv, generic):
    """OPEN is empty, so there is no minimum whose chain could be returned (arastar.cpp:204-210): no solution, from scratch
    and on a call that continues the exhausted search -- no chain from a heap slot that is no longer part of OPEN."""
    monkeypatch.setenv("SMPLX_SEARCH", side)
    t = _truth(nv, False)
    sid, loop = _loop(nv, False)
    want = [loop.replan(sid, 0, *EPS, allow_partial=True), loop.replan(sid, 0, *EPS, allow_partial=True, resume=True)]
    assert [(w["result"], w["solved"], len(w["path"])) for w in want] == [(EXHAUSTED, 0, 0)] * 2
    s = _space(nv, generic=generic)
    r = s.replan(*EPS, improve=True, bounded=False, allow_partial=True)
    assert r["resumed"] == 0
    _assert_exhausted(r, t)
    again = s.replan(*EPS, improve=True, bounded=False, allow_partial=True)
    assert again["resumed"] == 1 and again["call_expansions"] == want[1]["call_expansions"] == 0
    _assert_exhausted(again, t, calls=2)


@pytest.mark.parametrize("side,nv,generic", [b for b in BUILDS if b[1] == 2 or b[2]], ids=[i for i, b in zip(BUILD_IDS, BUILDS) if b[1] == 2 or b[2]])
def test_chunks_to_the_end(monkeypatch, side, nv, generic):
    """Calls bounded by 997 pops (97 on the one-joint chain) that continue one search until OPEN is empty: every call but
    the last times out at its budget, the last is exhausted, together they are the uninterrupted search; one more call has
    nothing to pop; from_scratch pops everything again."""
    monkeypatch.setenv("SMPLX_SEARCH", side)
    t = _truth(nv, False)
    k = CHUNK[nv]
    want = _loop_calls(nv, False, k)
    assert len(want) >= 3 and [w[0] for w in want] == [TO] * (len(want) - 1) + [EXHAUSTED]
    s = _space(nv, generic=generic)
    calls = []
    for i, w in enumerate(want):
        r = s.replan(*EPS, True, True, k, k)
        calls.append(r)
        assert (r["result"], r["call_expansions"], r["solved"]) == w, i
        assert r["resumed"] == (i > 0) and r["path_len"] == 0, i
    for r in calls[:-1]:
        assert r["result"] == TO and r["call_expansions"] == k
    assert sum(r["call_expansions"] for r in calls) == t["eo"]["expansions"]
    _assert_exhausted(calls[-1], t, calls=len(calls))
    more = s.replan(*EPS, True, True, k, k)
    assert more["resumed"] == 1 and more["call_expansions"] == 0
    _assert_exhausted(more, t, calls=len(calls) + 1)
    _assert_lattice(s, t)
    whole = s.replan(*EPS, True, False, from_scratch=True)
    assert whole["resumed"] == 0
    _assert_exhausted(whole, t)


@pytest.mark.parametrize("nv,generic,capacity", [(2, False, 500), (1, True, 100)], ids=["nv2", "nv1-generic"])
def test_growing_while_exhausting(monkeypatch, nv, generic, capacity):
    """The device search with a first capacity of a few hundred states (test hooks): buffers and state table are outgrown
    many times on the way to an empty OPEN; same log, same lattice, same ending."""
    monkeypatch.setenv("SMPLX_SEARCH", "device")
    t = _truth(nv, False)
    cfg = wc.width_case(nv)
    s = capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic)
    s.set_search_capacity(capacity)
    s.set_table_slots(64)
    s.set_goal_joint(_goal(nv, False), cfg.goal_tol)
    assert s.set_start(cfg.start) == t["sid"]
    r = s.replan(*EPS, improve=True, bounded=False)
    sc = s.search_counters()
    print(f"grows {sc['grows']} table_allocs {sc['table_allocs']} launches {r['gpu_batches']}")
    _assert_exhausted(r, t)
    _assert_lattice(s, t)
    assert sc["grows"] >= 3 and sc["table_allocs"] >= 3 and r["gpu_batches"] >= 3
    assert r["cache_misses"] == 0                      # (the device search served every expansion)


@pytest.mark.parametrize("side,nv,generic", BUILDS, ids=BUILD_IDS)
def test_the_same_space_afterwards(monkeypatch, side, nv, generic):
    """After an exhausted search the space gets the reachable goal: the search for it is a fresh oracle's -- expansion log
    and path compared as lattice coordinates (a new goal numbers the states anew), cost and expansion count as they are."""
    monkeypatch.setenv("SMPLX_SEARCH", side)
    t, tr = _truth(nv, False), _truth(nv, True)
    cfg = wc.width_case(nv)
    s = _space(nv, generic=generic)
    _assert_exhausted(s.replan(*EPS, improve=True, bounded=False), t)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_start(cfg.start)
    r = s.replan(*EPS, improve=True, bounded=False)
    eo = tr["eo"]
    assert tr["loop"]["result"] == SUCCESS
    assert r["resumed"] == 0 and r["result"] == tr["loop"]["result"] and r["solved"] == 1 and r["satisfied_eps"] == eo["eps"] == 1.0
    assert r["cost"] == eo["cost"] and r["expansions"] == eo["expansions"] and s.num_states() == len(tr["states"])

    def coords(ids, get):
        return [None if int(i) == 0 else tuple(int(x) for x in get(int(i))) for i in ids]      # (0: the goal's entry)
    assert coords(r["expansion_log"], lambda i: s.get_state(i)[1]) == coords(eo["expansion_log"], lambda i: tr["states"][i][1])
    assert coords(r["path"], lambda i: s.get_state(i)[1]) == coords(eo["path"], lambda i: tr["states"][i][1])
    assert r["path"][-1] == 0 and len(r["path"]) == r["path_len"] == len(eo["path"])


# ----------------------------------------------------------------------------------------------------------------------
# a solution longer than the device search's path buffer
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])
def test_a_path_longer_than_its_buffer(monkeypatch, generic):
    """smplx_test_set_search_capacity(4096) gives the device search a path buffer of 64 ids and leaves every other buffer
    room for the whole search of the one-joint chain, whose solution has a few hundred states: the workgroup finds that the
    path does not fit (grow_what = 3), the host doubles the buffer until it does and launches again for the path alone.
    Path, cost and log are the oracle's; the one visible sign of the extra launch is gpu_batches, compared with the same
    search without the hook.  The same for a partial solution after 300 pops."""
    monkeypatch.setenv("SMPLX_SEARCH", "device")
    tr = _truth(1, True)
    eo = tr["eo"]
    assert len(eo["path"]) > 2 * 64
    cfg = wc.width_case(1)

    def run(hook, **search):
        s = capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic)
        s.set_search_capacity(hook)
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        assert s.set_start(cfg.start) == tr["sid"]
        return s.replan(*EPS, **search), s.search_counters()

    plain, pc = run(0, improve=True, bounded=False)
    small, sc = run(4096, improve=True, bounded=False)
    print(f"solution of {len(eo['path'])} states: gpu_batches {plain['gpu_batches']} -> {small['gpu_batches']}, grows {pc['grows']} -> {sc['grows']}")
    for r in (plain, small):
        assert r["result"] == tr["loop"]["result"] == SUCCESS and r["solved"] == 1 and r["satisfied_eps"] == eo["eps"]
        assert r["cost"] == eo["cost"] and np.array_equal(r["path"], eo["path"]) and r["path_len"] == len(eo["path"])
        assert r["expansions"] == r["call_expansions"] == eo["expansions"] and np.array_equal(r["expansion_log"], eo["expansion_log"])
    assert small["gpu_batches"] > plain["gpu_batches"]

    sid, loop = _loop(1, True)
    want = loop.replan(sid, 0, *EPS, PARTIAL_K, PARTIAL_K, allow_partial=True)
    assert want["result"] == TO and want["solved"] == 1 and want["satisfied_eps"] == np.inf and len(want["path"]) > 64
    search = dict(improve=True, bounded=True, max_init=PARTIAL_K, max_rep=PARTIAL_K, allow_partial=True)
    plain, pc = run(0, **search)
    small, sc = run(4096, **search)
    print(f"partial solution of {len(want['path'])} states: gpu_batches {plain['gpu_batches']} -> {small['gpu_batches']}, grows {pc['grows']} -> {sc['grows']}")
    for r in (plain, small):
        assert r["result"] == PARTIAL and r["solved"] == 1 and r["satisfied_eps"] == np.inf
        assert r["call_expansions"] == r["expansions"] == want["call_expansions"] == PARTIAL_K
        assert r["cost"] == want["cost"] and r["path"].tolist() == want["path"] and r["expansion_log"].tolist() == want["log"]
    assert small["gpu_batches"] > plain["gpu_batches"]


# ----------------------------------------------------------------------------------------------------------------------
# shards whose queries end differently
# ----------------------------------------------------------------------------------------------------------------------

def _shard(reachable, capacity=0):
    """spaces of the two-joint chain on one model and one grid, one per entry of `reachable`"""
    cfg = wc.width_case(2)
    grid = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    model = capi.Model(cfg.robot_text)
    out = []
    for ok in reachable:
        sp = capi.Space(model, grid, cfg.mprim, cfg.params, 512)
        if capacity:
            sp.set_search_capacity(capacity)
        sp.set_goal_joint(_goal(2, ok), cfg.goal_tol)
        assert sp.set_start(cfg.start) == _truth(2, ok)["sid"]
        out.append(sp)
    return out


def _assert_final(r, t):
    """the last call of a query against the oracle's unbounded search"""
    eo = t["eo"]
    assert r["solved"] == eo["ok"] and r["cost"] == eo["cost"] and np.array_equal(r["path"], eo["path"])
    assert r["expansions"] == eo["expansions"] and np.array_equal(r["expansion_log"], eo["expansion_log"])
    assert r["satisfied_eps"] == eo["eps"]


MIXED = [True, False, True, False, True, False]


@pytest.mark.parametrize("side,threads,capacity", [("device", 1, 0), ("device", 1, 500), ("host", 1, 0), ("host", 4, 0)],
                         ids=["device", "device-growing", "host-1-thread", "host-4-threads"])
def test_one_shard_three_endings(monkeypatch, side, threads, capacity):
    """Six queries of one shard, goals reachable and unreachable in turn, 3 000 pops per call: after the first call the
    reachable ones have succeeded and the others timed out at exactly their budget; further calls end the others with an
    empty OPEN while the finished ones return at once.  Call by call every query is the plain loop's and the same query
    run alone through smplx_replan; at the end it is the oracle's unbounded search.  device-growing: with a first capacity of
    500 states the unreachable queries stop for room again and again, so that a launch finds the workgroups of the
    reachable ones already done."""
    monkeypatch.setenv("SMPLX_SEARCH", side)
    want = {ok: _loop_calls(2, ok, SHARD_BUDGET, ncalls=len(_loop_calls(2, False, SHARD_BUDGET))) for ok in (True, False)}
    ncalls = len(want[False])
    assert ncalls >= 3 and want[True][0][0] == SUCCESS and all(w == (SUCCESS, 0, 1) for w in want[True][1:])
    assert want[False][0] == (TO, SHARD_BUDGET, 0) and want[False][-1][0] == EXHAUSTED and want[False][-1][2] == 0
    bounded = (*EPS, True, True, SHARD_BUDGET, SHARD_BUDGET)

    solo = {}
    for ok in (True, False):
        sp = _shard([ok], capacity)[0]
        solo[ok] = [sp.replan(*bounded) for _ in range(ncalls)]
        assert [(r["result"], r["call_expansions"], r["solved"]) for r in solo[ok]] == want[ok]

    spaces = _shard(MIXED, capacity)
    for k in range(ncalls):
        rs, _ = capi.Space.replan_multi(spaces, *bounded, host_threads=threads)
        print(f"call {k}: " + " ".join(f"{r['result']}/{r['call_expansions']}" for r in rs) + f" launches {rs[0]['gpu_batches']}")
        for q, (ok, r) in enumerate(zip(MIXED, rs)):
            a = solo[ok][k]
            assert (r["result"], r["call_expansions"], r["solved"]) == want[ok][k], (k, q)
            assert r["resumed"] == (k > 0), (k, q)
            assert r["cost"] == a["cost"] and np.array_equal(r["path"], a["path"]) and r["expansions"] == a["expansions"], (k, q)
            assert np.array_equal(r["expansion_log"], a["expansion_log"]) and r["satisfied_eps"] == a["satisfied_eps"], (k, q)
        if side == "device" and capacity and k == 0:
            # a shard's launches are counted for all its queries alike: the reachable queries, which alone need fewer, were
            # done when the later ones came
            print(f"launches of the first call alone: reachable {solo[True][0]['gpu_batches']}, unreachable {solo[False][0]['gpu_batches']}")
            assert solo[True][0]["gpu_batches"] < solo[False][0]["gpu_batches"] <= rs[0]["gpu_batches"]
    for ok, r in zip(MIXED, rs):
        _assert_final(r, _truth(2, ok))
    for sp, ok in zip(spaces, MIXED):
        assert sp.num_states() == len(_truth(2, ok)["states"])


@pytest.mark.parametrize("side,threads,capacity", [("device", 1, 0), ("device", 1, 500), ("host", 1, 0), ("host", 4, 0)],
                         ids=["device", "device-growing", "host-1-thread", "host-4-threads"])
def test_mixed_shard_unbounded(monkeypatch, side, threads, capacity):
    """smplx_plan_multi without a budget on the same six queries: each is the oracle's search, solved or exhausted"""
    monkeypatch.setenv("SMPLX_SEARCH", side)
    spaces = _shard(MIXED, capacity)
    rs, _ = capi.Space.plan_multi(spaces, *EPS, True, False, host_threads=threads)
    for ok, r in zip(MIXED, rs):
        assert r["path_len"] == len(_truth(2, ok)["eo"]["path"])
        _assert_final(r, _truth(2, ok))


@pytest.mark.parametrize("side", ["device", "host"])
def test_a_shard_of_one_unreachable_query(monkeypatch, side):
    monkeypatch.setenv("SMPLX_SEARCH", side)
    want = _loop_calls(2, False, SHARD_BUDGET)
    assert want[-1][0] == EXHAUSTED
    spaces = _shard([False])
    for k, w in enumerate(want):
        rs, _ = capi.Space.replan_multi(spaces, *EPS, True, True, SHARD_BUDGET, SHARD_BUDGET)
        assert (rs[0]["result"], rs[0]["call_expansions"], rs[0]["solved"]) == w and rs[0]["resumed"] == (k > 0), k
    _assert_exhausted(rs[0], _truth(2, False), calls=len(want))
    rs, _ = capi.Space.plan_multi(_shard([False]), *EPS, True, False)
    _assert_final(rs[0], _truth(2, False))
