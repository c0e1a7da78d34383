"""Every expansion path at every variable count and primitive count (width_cases.py): the batched step in each of its
launch shapes against the oracle's GetSuccs loop body, the K5 ids and records against a plain dict of the host's states,
the device-resident search against the oracle and the host loop -- with buffers and a state table that are outgrown on
the way -- and a shard of 16-variable queries in one launch.  tests/test_width_references.py shows on the CPU that the
cases are not vacuous: every variable, the last one in particular, tells states apart in the joint-goal search of every
case (the XYZ-goal searches are held to their length only).

Everything is integer or fp64 work in an unchanged order: every comparison is exact.

The search cases see a fault of the table probe (table_slot_match) only by chance: a state's home slot comes from a hash of
all its coordinates, so a probe that ignored one coordinate takes state B for its sibling A only when A's slot lies in B's
probe run.  test_table_probe_compares_every_coordinate is what pins the probe: the probe functions themselves on a table
of 64 slots, once with every state's probe starting at the same slot, for every variable of every width."""
import numpy as np
import pytest

import width_cases as wc
from test_gpu_device_search import _check_against_oracle
from test_gpu_three_launch_step import _assert_oracle, _assert_same, _Hip, _need_gpu, _Out, _work, hip  # noqa: F401

pytestmark = pytest.mark.gpu

NAMES = [c[0] for c in wc.ALL_CASES]
WIDTH_NAMES = [f"nv{nv}" for nv in wc.WIDTHS]
PRIM_NAMES = [c[0] for c in wc.PRIM_CASES]
SEARCH = (5.0, 1.0, 1.0, True, True, 3000, 3000)
N_EXPANDED, B_K5 = 150, 280
# An XYZ goal of a whole cell either way is reached within a few dozen expansions at some widths; with 0.3 of a cell the oracle's
# search takes 438 (nv = 1) to 3 000 expansions at every case.
XYZ_TOL_CELLS = 0.3


_BUILT = set()


@pytest.fixture()
def kernels_built(request):
    """The first space of a robot compiles its per-robot kernels (up to a minute for a 16-variable chain, then cached in the
    process and on disk): done here, in the set-up of the first test that names the robot (its `name` parameter), so that no
    test's own time holds a compiler run.  Returns the function from a case's name to its Config."""
    from smpl_amd import capi
    _need_gpu()
    cfg = wc.case_config(request.node.callspec.params["name"])
    if cfg.robot_text not in _BUILT:
        capi.Space.from_config(cfg, batch_states=16).close()
        _BUILT.add(cfg.robot_text)
    return wc.case_config


@pytest.mark.parametrize("one_home", [False, True], ids=["hashed", "one-home-slot"])
@pytest.mark.parametrize("nv", wc.WIDTHS)
def test_table_probe_compares_every_coordinate(nv, one_home):
    """table_probe_start / table_probe_finish / table_store_own of the device search, through a hook kernel, on a table of 64
    slots: a base coordinate and, for every variable in turn (the last included), two states that differ from it in that
    variable alone go in; then every one of them and, for every variable, two absent siblings that differ from the base in
    that variable alone are looked up, against the plain dict.  hashed: home slots by the search's own hash (the table is
    half full at nv = 16).  one-home-slot: every probe starts at slot 0, so each lookup walks over every state inserted
    before its own, and an absent sibling over all of them: a probe that skipped any coordinate of any word would take one
    for another."""
    from smpl_amd import capi
    _need_gpu()
    rng = np.random.default_rng(100 + nv)
    base = rng.integers(3, 60, size=nv)
    inserted, absent = [base.copy()], []
    for v in range(nv):
        for d, there in ((1, True), (2, True), (-1, False), (3, False)):
            c = base.copy()
            c[v] += d
            (inserted if there else absent).append(c)
    assert len(inserted) == 1 + 2 * nv < 64 and len(absent) == 2 * nv
    table = {tuple(int(x) for x in c): i for i, c in enumerate(inserted)}
    assert len(table) == len(inserted)
    queries = inserted + absent
    found, ids = capi.table_probe(nv, 64, one_home, np.array(inserted), np.array(queries))
    assert (found == -1).all()                      # no new coordinate was taken for one already there
    want = [table.get(tuple(int(x) for x in q), -1) for q in queries]
    assert ids.tolist() == want
    # every coordinate twice (128 slots: the hook wants fewer rows than slots): the second time each is found under its id
    found, ids2 = capi.table_probe(nv, 128, one_home, np.array(inserted + inserted), np.array(queries))
    assert found.tolist() == [-1] * len(inserted) + list(range(len(inserted))) and ids2.tolist() == want


def _M(name):
    for n, nv, rows in wc.ALL_CASES:
        if n == name:
            return wc.prim_count(wc.default_rows(nv) if rows is None else rows)
    raise KeyError(name)


def _rows(o, Q):
    rows = [o.eval_state(q) for q in Q]
    return {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}


@pytest.fixture(scope="module")
def batches():
    """(cfg, Q, oracle rows) per case: 300 states on whole cells around the start, the start and a state in the goal's
    cell among them, through the oracle's GetSuccs loop body with the case's joint goal"""
    from oracle_binding import Oracle
    cache = {}

    def get(name):
        if name not in cache:
            cfg = wc.case_config(name)
            o = Oracle(cfg)
            o.set_order(chain=True)
            o.set_goal_joint(cfg.goal, cfg.goal_tol)
            Q = wc.batch_states(cfg)
            exp = _rows(o, Q)
            f = exp["flags"]
            census = dict(valid=int(((f & 1) != 0).sum()), goal=int(((f & 2) != 0).sum()), inactive=int(((f & 0x10) != 0).sum()),
                          limits=int(((f & 0x20) != 0).sum()), collided=int(((f & 0x40) != 0).sum()))
            print(f"{name}: flag census of the batch {census}")
            assert census["valid"] >= 300 and census["goal"] >= 1 and census["inactive"] >= 300
            cache[name] = cfg, Q, exp
        return cache[name]
    return get


@pytest.fixture(scope="module")
def plans():
    """(oracle, plan, every state's (joint values, coordinate)) per (case, goal kind): the bounded search from the start"""
    from oracle_binding import Oracle
    cache = {}

    def get(name, goal_kind):
        if (name, goal_kind) not in cache:
            cfg = wc.case_config(name)
            o = Oracle(cfg)
            _set_goal(o, o, cfg, goal_kind)
            assert o.set_start(cfg.start) == 1
            o.search_params(*SEARCH)
            eo = o.plan()
            assert eo["expansions"] >= 200
            cache[(name, goal_kind)] = o, eo, [o.get_state(i) for i in range(o.num_states())]
        return cache[(name, goal_kind)]
    return get


def _set_goal(x, o, cfg, goal_kind):
    if goal_kind == "joint":
        x.set_goal_joint(cfg.goal, cfg.goal_tol)
    else:
        x.set_goal_xyz(o.planning_fk(cfg.goal), [XYZ_TOL_CELLS * cfg.grid.res] * 3)


def _compare_rows(exp, got, what):
    """a dense batch against the oracle's rows.  A colliding edge's lookup tally depends on where the walk stops, which the
    waypoint-parallel paths do not share with the reference: it is compared where the edge does not collide."""
    assert np.array_equal(exp["flags"], got["flags"]), what
    f = exp["flags"]
    v, ev, coll = (f & 1) != 0, (f & 0x10) == 0, (f & 0x40) != 0
    assert np.array_equal(exp["coord"][v], got["coord"][v]), what
    assert np.array_equal(exp["q"][ev], got["q"][ev]), what
    assert np.array_equal(exp["h"][v], got["h"][v]) and np.array_equal(exp["cost"][v], got["cost"][v]), what
    assert np.array_equal(exp["lookups"][~coll], got["lookups"][~coll]), what


# (name, space arguments, hook)
SHAPES = [("small-kernel", {}, None),
          ("four-launch", dict(no_small_kernel=True), "prep"),
          ("one-launch", dict(no_small_kernel=True), "one"),
          ("fused", dict(fused=True), None),
          ("tiny-work-list", dict(tiny_work_list=True), None),
          ("pipeline", dict(no_small_kernel=True), None),
          ("generic", dict(generic_kernels=True), None),
          ("generic-pipeline", dict(generic_kernels=True, no_small_kernel=True), None)]


@pytest.mark.parametrize("name", NAMES)
def test_batched_step_in_every_launch_shape(name, batches, kernels_built):
    """expand_batch of the same 300 states by a space of each shape: the single launch k_small_batch (a batch of up to 512
    states takes it), the pipeline in four launches, k_step_block, the fused pair, the pipeline with a work list that
    nearly every edge overflows, the pipeline by the rule, and the kernels linked into the library on both routes.  Each
    equals the oracle row by row, so all agree.  Where a block of k_step_block would hold the edges of more than 16 states
    (M < 9) the forced one-launch step fails with an error and the rule never takes the kernel."""
    from smpl_amd import capi
    _need_gpu()
    kernels_built(name)
    cfg, Q, exp = batches(name)
    M = _M(name)
    for shape, kw, hook in SHAPES:
        s = capi.Space.from_config(cfg, batch_states=512, **kw)
        assert s.N == len(cfg.start) and s.M == M
        assert s.specialized()[0] == ("generic_kernels" not in kw), s.specialized()[1]
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        if hook == "prep":
            s.set_pipe_prep(1)
        if hook == "one":
            s.set_one_launch(1)
            if not wc.step_allowed(M):
                with pytest.raises(capi.SmplxError):
                    s.expand_batch(Q)
                assert s.one_launch_steps() == 0
                s.close()
                continue
        got = s.expand_batch(Q)
        _compare_rows(exp, got, f"{name} {shape}")
        if hook == "one":
            assert s.one_launch_steps() == 1
        elif not wc.step_allowed(M) or "generic_kernels" in kw or hook == "prep" or "tiny_work_list" in kw or "fused" in kw:
            assert s.one_launch_steps() == 0
        s.close()


def _small_k5(hip, s, Q, work):
    """smplx_expand_batch_k5_device without the compact stream: a batch of up to 512 states is one launch of k_small_batch,
    which looks the ids up itself"""
    B, M, N = Q.shape[0], s.M, s.N
    d_q = hip.upload(Q)
    flags, coord, sq = hip.alloc(B * M), hip.alloc(4 * B * M * N), hip.alloc(8 * B * M * N)
    h, cost, lk, sid = (hip.alloc(4 * B * M) for _ in range(4))
    s.expand_batch_k5_device(d_q, B, flags, coord, sq, h, cost, lk, sid, None, 0, None, 0, None, None, work, None, None)
    hip.sync()
    d = hip.download
    return dict(flags=d(flags, B * M, np.uint8).reshape(B, M), coord=d(coord, B * M * N, np.int32).reshape(B, M, N),
                q=d(sq, B * M * N, np.float64).reshape(B, M, N), h=d(h, B * M, np.int32).reshape(B, M),
                cost=d(cost, B * M, np.int32).reshape(B, M), lookups=d(lk, B * M, np.int32).reshape(B, M),
                succ_id=d(sid, B * M, np.int32).reshape(B, M))


@pytest.mark.parametrize("grown", [False, True], ids=["first-table", "grown-table"])
@pytest.mark.parametrize("name", WIDTH_NAMES)
def test_k5_ids_and_records_equal_the_plain_dict(name, grown, hip, kernels_built, monkeypatch):
    """GetSuccs on the first 150 states in id order through the host loop, then the K5 step on the joint values of those
    states and of the up to 130 states after them, which have not been expanded, so that many of their successors are
    unknown: every valid successor gets the id the plain dict of the host's states holds for its coordinate, -1 where it
    holds none;
    the rec_a / rec_b records decode to the same ids, coordinates and joint values (the doubles of rec_b sit behind
    (nv + 2) / 2 * 2 ints: another layout at odd and at even nv).  Through the pipeline, through k_step_block, and without
    the stream through k_small_batch.

    grown-table: a device search of two expansions with a first capacity of 64 states leaves the space a table of a few
    hundred slots (smplx_test_set_search_capacity); the 150 expansions then commit more states than half of it, so the
    table the ids are read from has been outgrown, allocated again at four times the size and filled with every state."""
    from oracle_binding import Oracle
    from smpl_amd import capi
    _need_gpu()
    cfg = kernels_built(name)
    o = Oracle(cfg)
    o.set_order(chain=True)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    s = capi.Space.from_config(cfg, batch_states=512)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    if grown:
        monkeypatch.setenv("SMPLX_SEARCH", "device")
        s.set_search_capacity(64)
    assert s.set_start(cfg.start) == 1
    if grown:
        r = s.plan(5.0, 1.0, 1.0, True, True, 2, 2)
        assert r["expansions"] == 2 and r["cache_misses"] == 0 and s.search_counters()["searches"] == 1
    for i in range(1, N_EXPANDED + 1):
        assert i < s.num_states()
        s.get_succs(i)
    n = s.num_states()
    B = min(n - 1, B_K5)
    if grown:
        assert n - 1 > wc.first_table_slots(s.M, 64) // 2
    Q = np.stack([s.get_state(i)[0] for i in range(1, B + 1)])
    s.table_sync()
    sc = s.search_counters()
    assert sc["table_regrows"] >= 1 if grown else sc["table_regrows"] == 0      # the table was outgrown and built again
    table = wc.plain_table(s)
    assert len(table) == n
    host = {c: i for c, i in table.items() if i > 0}
    exp = _rows(o, Q)
    d_q, work = hip.upload(Q), _work(hip, s)
    runs = {}
    for mode in (0, 1):
        out = _Out(hip, s)
        before = s.one_launch_steps()
        s.set_one_launch(mode)
        out.issue(s, d_q, B, work, None)
        hip.sync()
        s.set_one_launch(-1)
        assert s.one_launch_steps() - before == mode
        runs[mode] = out.read(s)
        _assert_oracle(runs[mode], exp, host, s.N)
    _assert_same(runs[0], runs[1])
    valid = (exp["flags"] & 1) != 0
    known = runs[0]["succ_id"][valid] >= 0
    print(f"{name}: {B} states, {int(known.sum())} successors the table knows, {int((~known).sum())} it does not")
    assert known.sum() >= 100 and (~known).sum() >= (100 if s.N > 2 else 1)     # (a lattice of one or two dimensions has a short frontier)
    small = _small_k5(hip, s, Q, work)
    _compare_rows(exp, small, f"{name} small")
    assert np.array_equal(small["succ_id"], runs[0]["succ_id"])
    assert s.compact_rec_b_bytes() == wc.rec_b_bytes(s.N)
    s.close()


def _device_space(cfg, o, goal_kind, **kw):
    from smpl_amd import capi
    s = capi.Space.from_config(cfg, batch_states=256, **kw)
    _set_goal(s, o, cfg, goal_kind)
    assert s.set_start(cfg.start) == 1
    return s


def _assert_states(s, states):
    """every state the search created: the oracle's joint values and coordinate under the same id; the plain dict of the
    space's states has one key per id -- no two ids share a coordinate"""
    n = s.num_states()
    assert n == len(states)
    for i in range(1, n):
        gq, gc = s.get_state(i)
        assert np.array_equal(gc, states[i][1]) and np.array_equal(gq, states[i][0]), i
    assert len(wc.plain_table(s)) == n


@pytest.mark.parametrize("goal_kind", ["joint", "xyz"])
@pytest.mark.parametrize("name", NAMES)
def test_device_search_equals_the_oracle(name, goal_kind, plans, kernels_built, monkeypatch):
    """The device-resident search (SMPLX_SEARCH=device: a case that the engine would hand to the host loop fails) against the
    oracle: expansion log, ids, cost, path, epsilon, state count, evaluation count, and every state."""
    _need_gpu()
    monkeypatch.setenv("SMPLX_SEARCH", "device")
    cfg = kernels_built(name)
    o, eo, states = plans(name, goal_kind)
    s = _device_space(cfg, o, goal_kind)
    go = s.plan(*SEARCH)
    print(f"{name} {goal_kind}: oracle {eo['expansions']} expansions, {o.num_states()} states; device {go['expansions']} expansions, "
          f"{s.num_states()} states")
    _check_against_oracle(o, s, eo, go)
    assert go["cache_misses"] == 0 and s.search_counters()["searches"] == 1
    _assert_states(s, states)
    s.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_search_outgrows_buffers_and_table(name, plans, monkeypatch):
    """The same search from a first capacity of a sixth of the states it will create: the workgroup stops for room several
    times, and each time the state table has become too small as well it is allocated again and filled from the states'
    coordinates (k_search_table_fill) before the search probes it again."""
    _need_gpu()
    monkeypatch.setenv("SMPLX_SEARCH", "device")
    cfg = wc.case_config(name)
    o, eo, states = plans(name, "joint")
    s = _device_space(cfg, o, "joint")
    s.set_search_capacity(max(64, len(states) // 6))
    go = s.plan(*SEARCH)
    _check_against_oracle(o, s, eo, go)
    sc = s.search_counters()
    grows, fills = sc["grows"], sc["table_allocs"]
    print(f"{name}: {len(states)} states from a first capacity of {max(64, len(states) // 6)}: {grows} allocations, {fills} tables")
    assert grows >= 3          # the first allocation and at least two enlargements
    assert fills >= 3          # the first table and at least two larger ones, each filled again by k_search_table_fill
    _assert_states(s, states)
    s.close()


@pytest.mark.parametrize("name", NAMES)
def test_host_loop_search_equals_the_oracle(name, plans, monkeypatch):
    """SMPLX_SEARCH=host on the same case: the host loop's own table_lookup compares all nv coordinates; same log and path."""
    _need_gpu()
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    cfg = wc.case_config(name)
    o, eo, states = plans(name, "joint")
    s = _device_space(cfg, o, "joint")
    go = s.plan(*SEARCH)
    _check_against_oracle(o, s, eo, go)
    assert go["cache_misses"] > 0
    _assert_states(s, states)
    s.close()


def test_device_search_at_53_primitives_without_the_helper_wave(plans, monkeypatch):
    """M = 53 is the largest count whose k_search block has room for the helper wave; the default run above has it, this one
    is the same search with the search wave doing the bookkeeping inline, as from M = 55 on."""
    _need_gpu()
    monkeypatch.setenv("SMPLX_SEARCH", "device")
    assert wc.search_has_helper(53) and not wc.search_has_helper(55)
    cfg = wc.case_config("M53")
    o, eo, states = plans("M53", "joint")
    s = _device_space(cfg, o, "joint")
    s.set_search_helper(False)
    go = s.plan(*SEARCH)
    _check_against_oracle(o, s, eo, go)
    assert go["cache_misses"] == 0
    _assert_states(s, states)
    s.close()


@pytest.mark.parametrize("name", ["M5", "M63"])
def test_get_succs_on_single_states(name):
    """GetSuccs state by state through the host loop (a batch of one: k_small_batch with 5 and with 63 primitive lanes),
    ids and costs against the oracle's, 60 states in id order."""
    from oracle_binding import Oracle
    from smpl_amd import capi
    _need_gpu()
    cfg = wc.case_config(name)
    o = Oracle(cfg)
    s = capi.Space.from_config(cfg, batch_states=256)
    o.set_goal_joint(cfg.goal, cfg.goal_tol); s.set_goal_joint(cfg.goal, cfg.goal_tol)
    assert o.set_start(cfg.start) == s.set_start(cfg.start)
    total = 0
    for i in range(1, 61):
        es, ec = o.get_succs(i)
        gs, gc = s.get_succs(i)
        assert np.array_equal(es, gs) and np.array_equal(ec, gc), i
        total += len(es)
    assert total >= 100 and o.num_states() == s.num_states()
    for i in range(1, s.num_states()):
        assert np.array_equal(o.get_state(i)[1], s.get_state(i)[1]), i
    s.close()


def test_shard_of_16_variable_queries_in_one_launch(monkeypatch):
    """Eight 16-variable queries that share grid, robot and primitives: one workgroup each in one launch of k_search.  Every
    query equals its solo device run and the host-driven loop."""
    from smpl_amd import capi
    _need_gpu()
    cfg = wc.case_config("nv16")
    res = np.asarray(cfg.params.resolutions)
    rng = np.random.default_rng(16)
    cells = rng.integers(-4, 5, size=(40, 16))
    goals = [list(np.asarray(cfg.start) + c * res) for c in cells]
    grid = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    model = capi.Model(cfg.robot_text)
    probe = capi.Space(model, grid, cfg.mprim, cfg.params, 256)
    ok = probe.state_valid_batch(np.array(goals))[0].astype(bool) & probe.check_joint_limits(np.array(goals)).astype(bool)
    goals = [g for g, k in zip(goals, ok) if k][:8]
    assert len(goals) == 8
    bounds = (5.0, 1.0, 1.0, True, True, 1500, 1000)

    def make():
        out = []
        for g in goals:
            sp = capi.Space(model, grid, cfg.mprim, cfg.params, 512)
            sp.set_goal_joint(g, cfg.goal_tol); sp.set_start(cfg.start)
            out.append(sp)
        return out
    monkeypatch.setenv("SMPLX_SEARCH", "device")
    multi_spaces = make()
    multi, wall = capi.Space.plan_multi(multi_spaces, *bounds)
    solo_spaces = make()
    solo = [sp.plan(*bounds) for sp in solo_spaces]
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    host, _ = capi.Space.plan_multi(make(), *bounds, host_threads=3)
    assert sum(a["expansions"] for a in solo) >= 2000 and sum(a["solved"] for a in solo) >= 4
    for a, b, c in zip(solo, multi, host):
        for x in (b, c):
            assert a["solved"] == x["solved"] and a["cost"] == x["cost"] and np.array_equal(a["expansion_log"], x["expansion_log"])
            assert np.array_equal(a["path"], x["path"]) and a["committed_succ_evals"] == x["committed_succ_evals"]
    assert all(m["cache_misses"] == 0 for m in multi) and any(h["cache_misses"] > 0 for h in host)
    for a, b in zip(solo_spaces, multi_spaces):
        assert a.num_states() == b.num_states() and len(wc.plain_table(b)) == b.num_states()
    assert len({tuple(m["expansion_log"][:50]) for m in multi}) >= 4       # different searches
