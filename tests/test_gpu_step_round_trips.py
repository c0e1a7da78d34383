"""The three step kernels take what the host knows -- nprims, nvars, the model image and its byte count -- as kernel
arguments instead of loading it from the space record in front of their first indexed load.  Nothing a caller sees may
change: every dense output, the compact stream, and region B field by field (h, coordinates, joint values), on the
ordinary path, through the deferred pass, in cross-query batches, on a non-cubic grid, in both builds.

Fixtures and shapes are those of tests/test_gpu_three_launch_step.py (whose helpers are used as they are): valid states
among scenes.benchmark_states(ARM7_LIMITS, 1200, 777) on the small scene, goal = row 3, a pipeline-only space whose
device table knows the states of a 40-expansion search.  References: the four-launch step of the same space
(set_pipe_prep), the oracle's eval_state rows, and each query's own single-space run.  Everything compared is integer
or fp64 work in an unchanged order: the tolerance is zero.
"""
import struct

import numpy as np
import pytest

import noncubic_cases as nc
from test_gpu_three_launch_step import (B_MAIN, GOAL_ROW, SIZES, _assert_oracle, _assert_same, _host_ids, _need_gpu, _run,  # noqa: F401
                                        _space, _stream, batch, hip)

pytestmark = pytest.mark.gpu

VALID, GOAL, COLLISION = 0x01, 0x02, 0x40
BUILDS = pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])


def _records(got, N):
    """The compact stream in block order, region B taken apart: [(succ_id, meta, None | (h, coord[N], q[N]))]."""
    ints = (N + 2) // 2 * 2
    seq_a, seq_b = _stream(got)
    out, ib = [], 0
    for rid, meta in seq_a:
        full = None
        if rid < 0 or meta & 0x100:
            vals = struct.unpack(f"<{ints}i{N}d", seq_b[ib]); ib += 1
            full = (vals[0], tuple(vals[1:1 + N]), tuple(vals[ints:]))
        out.append((rid, meta, full))
    assert ib == len(seq_b)
    return out


def _assert_region_b_fields(got, ref, N, M):
    """Region B field by field against another run of the same batch, and against the run's own dense outputs: a record's
    h, coordinates and joint values are those of its edge's rows."""
    a, b = _records(got, N), _records(ref, N)
    assert len(a) == len(b)
    for (rid, meta, full), (rid2, meta2, full2) in zip(a, b):
        assert (rid, meta) == (rid2, meta2)
        assert (full is None) == (full2 is None)
        if full is None:
            continue
        i, p = meta >> 9, meta & 0xFF
        assert full[0] == full2[0] == got["h"][i, p], (i, p)
        assert full[1] == full2[1] == tuple(int(v) for v in got["coord"][i, p]), (i, p)
        assert full[2] == full2[2] == tuple(float(v) for v in got["q"][i, p]), (i, p)


def _assert_both_kinds_of_record(got, N):
    """The batch writes both kinds of region-B record: for a valid successor the table does not know, and for a goal
    successor (with goal = row 3 the B = 300 batch of the fixture has both)."""
    valid = (got["flags"] & VALID) != 0
    assert (valid & (got["succ_id"] < 0)).any()
    assert (valid & ((got["flags"] & GOAL) != 0)).any()
    assert (valid & (got["succ_id"] >= 0) & ((got["flags"] & GOAL) == 0)).any()   # and edges that leave no record in B
    recs = _records(got, N)
    assert any(full is not None and rid < 0 for rid, meta, full in recs)
    assert any(full is not None and meta & 0x100 for rid, meta, full in recs)


@BUILDS
def test_three_launches_equal_four_and_the_oracle(small_cfg, batch, hip, generic):
    """B = 1, 6 (the smallest batch with a state that straddles two blocks at M = 25) and 300 (59 blocks, the last one
    partial): every dense output, the compact stream block by block, region B field by field."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q, generic_kernels=generic)
    assert s.specialized()[0] == (not generic)
    host = _host_ids(s)
    for B in SIZES:
        three, = _run(hip, s, Q, [B])
        four, = _run(hip, s, Q, [B], prep=[True])
        if B == B_MAIN:
            _assert_both_kinds_of_record(three, s.N)
        _assert_oracle(three, exp, host, s.N)
        _assert_same(three, four)
        _assert_region_b_fields(three, four, s.N, s.M)


def _set_work_list_items(s, items):
    import ctypes as C
    from smpl_amd import capi
    f = capi.lib().smplx_test_set_work_list_items
    f.argtypes = [C.c_void_p, C.c_int]
    assert f(s.h, items) == 0


@BUILDS
def test_deferred_pass_and_the_counters_it_leaves(small_cfg, batch, hip, generic):
    """The B = 300 step with the work list shrunk to 128 items, so that most edges are walked whole by their finish
    thread (a deferred edge's record holds what expand_edge wrote to the caller's rows).  lookups is
    compared on valid edges (a deferred colliding edge stops at its first collision, one on the list does not).  Then
    the hook is restored and a normal step on the same stream still matches: the work-list counters were left zeroed."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q, generic_kernels=generic)
    side = hip.stream()
    full, = _run(hip, s, Q, [B_MAIN], stream=side)
    _assert_both_kinds_of_record(full, s.N)
    _set_work_list_items(s, 8 * 16)
    try:
        tiny, = _run(hip, s, Q, [B_MAIN], stream=side)
    finally:
        _set_work_list_items(s, 0)
    valid = (full["flags"] & VALID) != 0
    assert np.array_equal(tiny["flags"], full["flags"])
    assert np.array_equal(tiny["coord"][valid], full["coord"][valid])
    evaluated = (full["flags"] & 0x10) == 0
    assert np.array_equal(tiny["q"][evaluated], full["q"][evaluated])
    assert np.array_equal(tiny["h"], full["h"]) and np.array_equal(tiny["cost"], full["cost"])
    assert np.array_equal(tiny["succ_id"], full["succ_id"])
    assert np.array_equal(tiny["lookups"][valid], full["lookups"][valid])
    assert [int(x) for x in tiny["totals"]] == [int(x) for x in full["totals"]]
    assert _stream(tiny) == _stream(full)
    _assert_region_b_fields(tiny, full, s.N, s.M)
    # edges were in fact deferred: the early exit shows in the tally of colliding edges, and nowhere else
    d = tiny["lookups"] != full["lookups"]
    assert d.any() and not d[(full["flags"] & COLLISION) == 0].any()
    again, = _run(hip, s, Q, [B_MAIN], stream=side)
    _assert_same(again, full)
    _assert_region_b_fields(again, full, s.N, s.M)


@BUILDS
def test_cross_query_batches_equal_each_querys_own_run(small_cfg, monkeypatch, generic):
    """Two queries with different goals on one scene through smplx_plan_multi's host-driven loop, at most 6 states of
    each per sweep, so that every frontier batch is a cross-query one whose rows alternate between the two spaces (the
    kernels take nprims from the launch and the goal, BFS grid and table from each row's own space).  Every query
    equals its solo run: cost, path, the order of its expansions, the successor evaluations it committed."""
    from smpl_amd import capi
    _need_gpu()
    cfg = small_cfg
    DEG = np.pi / 180.0
    cells = [[-49, 7, 21, -14, -8, -12, 16], [-21, 7, 14, -7, 8, -4, 12]]
    goals = [[cfg.start[i] + c * DEG for i, c in enumerate(cs)] for cs in cells]
    grid = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    model = capi.Model(cfg.robot_text)

    def make():
        out = []
        for g in goals:
            sp = capi.Space(model, grid, cfg.mprim, cfg.params, 6, no_small_kernel=True, generic_kernels=generic)
            sp.set_goal_joint(g, cfg.goal_tol); sp.set_start(cfg.start)
            out.append(sp)
        return out
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    solo = [sp.plan(5.0, 1.0, 1.0, True, True, 400, 400) for sp in make()]
    multi, _ = capi.Space.plan_multi(make(), 5.0, 1.0, 1.0, True, True, 400, 400, host_threads=1)
    assert len({tuple(a["expansion_log"]) for a in solo}) == 2       # the two queries do differ
    for a, b in zip(solo, multi):
        assert len(a["expansion_log"]) > 6
        assert a["solved"] == b["solved"] and a["cost"] == b["cost"] and np.array_equal(a["expansion_log"], b["expansion_log"])
        assert np.array_equal(a["path"], b["path"]) and a["committed_succ_evals"] == b["committed_succ_evals"]


@pytest.fixture(scope="module")
def noncubic_batch():
    """(cfg, Q, oracle rows of Q[:6]) on a planning grid whose three extents differ (61 x 46 x 35 cells)."""
    from oracle_binding import Oracle
    cfg = nc.planning_case(0)
    assert len(set(cfg.grid.dims)) == 3
    o = Oracle(cfg)
    o.set_order(chain=True)
    Qall = nc.bench_states()
    ok = np.array([o.state_valid(q)[0] for q in Qall[:40]])
    Q = np.ascontiguousarray(Qall[:40][ok][:6])
    assert Q.shape[0] == 6
    o.set_goal_joint(Q[GOAL_ROW], cfg.goal_tol)
    rows = [o.eval_state(q) for q in Q]
    return cfg, Q, {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}


@BUILDS
def test_non_cubic_grid(noncubic_batch, hip, generic):
    """The B = 6 comparison on a grid with three different extents: the collision role, whose prologue changed, indexes it."""
    _need_gpu()
    cfg, Q, exp = noncubic_batch
    s = _space(cfg, Q, generic_kernels=generic)
    assert s.specialized()[0] == (not generic)
    three, = _run(hip, s, Q, [6])
    four, = _run(hip, s, Q, [6], prep=[True])
    assert ((exp["flags"] & VALID) != 0).any() and (exp["lookups"] > 0).any()   # the grid was in fact looked up
    _assert_oracle(three, exp, _host_ids(s), s.N)
    _assert_same(three, four)
    _assert_region_b_fields(three, four, s.N, s.M)
