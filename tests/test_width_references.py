"""The cases of width_cases.py on the CPU, with the oracle alone: every width and every primitive count builds, searches
and meets the conditions it is there for, so that tests/test_gpu_widths.py cannot pass vacuously; the plain dict names
every state as the oracle's own table does; and the Python restatement of the layout formulas equals the engine's headers
(compiled into a small host program) and has its edges where the cases sit."""
import os
import subprocess

import numpy as np
import pytest

import width_cases as wc
from oracle_binding import Oracle

NAMES = [c[0] for c in wc.ALL_CASES]
SEARCH = (5.0, 1.0, 1.0, True, True, 3000, 3000)
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def _case(name):
    for n, nv, rows in wc.ALL_CASES:
        if n == name:
            return nv, wc.default_rows(nv) if rows is None else rows
    raise KeyError(name)


@pytest.fixture(scope="module")
def searched():
    """(oracle, plan, ids expanded) per case: a joint goal, the bounded search from the start, then GetSuccs on the first
    200 states of the expansion log once more, as a later caller would (it creates nothing new)"""
    cache = {}

    def get(name):
        if name not in cache:
            cfg = wc.case_config(name)
            o = Oracle(cfg)
            assert o.set_goal_joint(cfg.goal, cfg.goal_tol)
            sid = o.set_start(cfg.start)
            assert sid == 1
            o.search_params(*SEARCH)
            cache[name] = (o, o.plan(), sid)
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_case_builds_and_every_oracle_entry_works(name):
    nv, rows = _case(name)
    cfg = wc.case_config(name)
    assert len(cfg.start) == nv and len(set(cfg.grid.dims)) == 3 and max(cfg.grid.dims) <= 64
    assert len(cfg.boxes) >= 5
    o = Oracle(cfg)
    assert o.N == nv and o.M == wc.prim_count(rows) <= 63
    ok, lookups = o.state_valid(cfg.start)
    assert ok and lookups >= 1 and o.state_valid(cfg.goal)[0]
    assert o.check_joint_limits(cfg.start) and o.check_joint_limits(cfg.goal)
    cells = np.rint((np.asarray(cfg.goal) - np.asarray(cfg.start)) / np.asarray(cfg.params.resolutions)).astype(int)
    moved = np.abs(cells[cells != 0])
    assert moved.size >= min(nv, 2) and (moved >= 6).all()
    if nv > 2:
        assert (moved <= 10).all()
    # XYZ goal, then the joint goal: the heuristic, a start, its successors and a state
    assert o.set_goal_xyz(o.planning_fk(cfg.goal), [cfg.grid.res] * 3)
    assert o.heuristic_q(cfg.start) > 0
    assert o.set_goal_joint(cfg.goal, cfg.goal_tol)
    assert o.heuristic_q(cfg.start) > 0 and o.heuristic_q(cfg.goal) == 0
    sid = o.set_start(cfg.start)
    succs, costs = o.get_succs(sid)
    assert len(succs) >= 2 and len(costs) == len(succs) and o.num_states() == 2 + len(set(succs.tolist()))
    q, c = o.get_state(sid)
    assert np.array_equal(q, np.asarray(cfg.start)) and np.array_equal(c, o.state_to_coord(cfg.start)) and c.shape == (nv,)
    # the batch of the GPU tests: states on whole cells, some beyond a limit, the goal's cell among them
    Q = wc.batch_states(cfg)
    inside = np.array([o.check_joint_limits(x) for x in Q])
    assert inside[:2].all() and np.array_equal(o.state_to_coord(Q[1]), o.state_to_coord(cfg.goal))
    if any(wc.KINDS[v % 5] in ("rev_z", "prismatic") for v in range(nv)):
        assert (~inside).sum() >= 10 and inside.sum() >= 10


@pytest.mark.parametrize("name", NAMES)
def test_search_shows_every_variable(name, searched):
    """What makes a dropped or misplaced coordinate visible: the search is long enough, for every variable (the last one in
    particular) the state set holds pairs of states that differ in that variable alone -- a table that ignored it would
    take each pair for one state -- and, where the rows have the all-variables one, some state differs from its parent in
    every variable."""
    nv, rows = _case(name)
    o, plan, sid = searched(name)
    print(f"{name}: nv {nv} M {o.M} expansions {plan['expansions']} solved {plan['ok']} cost {plan['cost']} eps {plan['eps']} "
          f"states {o.num_states()}")
    assert plan["expansions"] >= 200 and plan["expansions"] <= 3000
    assert len(set(plan["expansion_log"].tolist())) >= 200 or nv == 1
    coords = [o.get_state(i)[1] for i in range(1, o.num_states())]
    pairs = wc.pairs_differing_in_one_variable(coords)
    print(f"{name}: pairs of states that differ in one variable alone, by variable: {pairs}")
    assert len(pairs) == nv and min(pairs) >= 5 and pairs[nv - 1] >= 5
    if rows[2] or nv == 1:
        found = 0
        for i in plan["expansion_log"][:50]:
            _, pc = o.get_state(int(i))
            succs, _ = o.get_succs(int(i))
            found += sum(1 for s in succs if s != 0 and (o.get_state(int(s))[1] != pc).all())
        assert found >= 1


@pytest.mark.parametrize("name", NAMES)
def test_plain_dict_names_states_as_the_oracle_does(name, searched):
    """The dict over the oracle's states against its own getOrCreateState: the ids GetSuccs returns for the first 200
    expanded states are the dict's ids of the successors' coordinates (0, the goal id, for a goal successor)."""
    nv, _ = _case(name)
    o, plan, sid = searched(name)
    log = [int(i) for i in plan["expansion_log"][:200]]
    got = [o.get_succs(i)[0] for i in log]
    table = wc.plain_table(o)
    assert len(table) == o.num_states()           # no two ids share a coordinate (id 0, the goal's entry, has its own)
    checked = 0
    for i, ids in zip(log, got):
        rows = o.eval_state(o.get_state(i)[0])
        valid = (rows["flags"] & 1) != 0
        goal = (rows["flags"] & 2) != 0
        want = [0 if g else table[tuple(int(x) for x in c)] for c, g in zip(rows["coord"][valid], goal[valid])]
        assert ids.tolist() == want, i
        checked += len(want)
    assert checked >= 400


def _header_values(tmp_path_factory):
    d = tmp_path_factory.mktemp("layout")
    exe = os.path.join(str(d), "layout_formulas")
    # the ROCm the library is built against (smpl_amd/build.py links with -L<root>/lib): its headers
    from smpl_amd import build
    roots = [os.path.dirname(f[2:].rstrip("/")) for f in build.LINK if f.startswith("-L")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__"] + [f"-I{os.path.join(d, 'include')}" for d in roots] +
                          [os.path.join(CSRC, "layout_formulas_driver.cpp"), "-o", exe])
    out = {"nv": {}, "M": {}}
    for line in subprocess.check_output([exe]).decode().splitlines():
        w = line.split()
        if w[0] == "limits":
            out["limits"] = [int(x) for x in w[1:]]
        else:
            out[w[0]][int(w[1])] = [int(x) for x in w[2:]]
    return out


def test_layout_formulas_equal_the_headers_and_have_their_edges_at_the_cases(tmp_path_factory):
    hv = _header_values(tmp_path_factory)
    assert hv["limits"] == [wc.MAX_VARS, wc.MAX_PRIMS, 16, 128]
    for nv in range(1, wc.MAX_VARS + 1):
        assert hv["nv"][nv] == [wc.table_stride(nv), wc.rec_b_bytes(nv)], nv
    for M in range(4, wc.MAX_PRIMS + 1):
        assert hv["M"][M] == [wc.small_block(M), wc.search_block(M), wc.step_states(M)], M
    # the state-table slot: every change of the word count and of the stride has a width on either side
    assert [wc.slot_words(nv) for nv in wc.WIDTHS] == [1, 1, 1, 2, 2, 3, 3, 4, 4, 5]
    assert [wc.table_stride(nv) for nv in wc.WIDTHS] == [8, 8, 8, 8, 8, 16, 16, 16, 16, 24]
    edges = [nv for nv in range(1, wc.MAX_VARS) if wc.slot_words(nv) != wc.slot_words(nv + 1) or wc.table_stride(nv) != wc.table_stride(nv + 1)]
    assert edges == [3, 7, 11, 15] and all(nv in wc.WIDTHS and nv + 1 in wc.WIDTHS for nv in edges)
    assert wc.WIDTHS[0] == 1 and wc.WIDTHS[-1] == wc.MAX_VARS
    assert all(wc.slot_words(nv) * 4 <= wc.table_stride(nv) for nv in range(1, wc.MAX_VARS + 1))     # the loads stay inside the slot
    # rec_b: the doubles start on 8 bytes, behind h and the coordinate; odd and even widths differ by the padding int
    for nv in wc.WIDTHS:
        assert wc.rec_b_ints(nv) >= nv + 1 and wc.rec_b_ints(nv) % 2 == 0 and wc.rec_b_ints(nv) - (nv + 1) == (nv + 1) % 2
    assert sum(nv % 2 for nv in wc.WIDTHS) == 5
    # the default rows
    for nv in wc.WIDTHS:
        M = wc.prim_count(wc.default_rows(nv))
        assert M == 3 + 2 * (min(nv, 4) + nv + 1) <= 63
    # the primitive-count cases sit on their edges
    assert [wc.prim_count(rows) for _, _, rows in wc.PRIM_CASES] == [5, 7, 9, 53, 55, 63]
    for name, nv, rows in wc.PRIM_CASES:
        M = wc.prim_count(rows)
        assert (M, wc.step_allowed(M), wc.search_has_helper(M)) == wc.PRIM_EXPECT[name], name
        assert wc.small_block(M) <= 512 and M + 1 <= 64
    assert not wc.step_allowed(7) and wc.step_allowed(9) and wc.step_states(9) == 16 and wc.step_states(7) == 20
    assert wc.search_block(53) == 512 and wc.small_block(53) == 448 and wc.search_block(55) == wc.small_block(55) == 512
    assert wc.small_block(63) == 512 and wc.small_block(64) > 512
    long_rows, short_rows, all_row = wc.PRIM_CASES[-1][2]
    assert len(long_rows) == 14 and len(short_rows) == 16 and not all_row
