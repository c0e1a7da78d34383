"""The frontier step in one launch (csrc/step_block.h k_step_block): each block owns 128 edges and keeps everything between
its phases in LDS; the claim counters of the compact stream belong to the engine, one set per stream, all-zero between
steps.  The three-launch step of the same space (set_one_launch(0)) is the reference in the same build; the oracle is the
other one.

Inputs, fixtures and helpers are those of test_gpu_three_launch_step.py: valid states among
scenes.benchmark_states(ARM7_LIMITS, 1200, 777) on the small scene, goal = row 3, start = row 5, a short search for table
contents.  Everything is integer or fp64 work in an unchanged order: the tolerance is zero everywhere.
"""
import copy

import numpy as np
import pytest

from smpl_amd import scenes
from test_gpu_three_launch_step import (B_MAIN, GOAL_ROW, SIZES, START_ROW, _assert_oracle, _assert_same, _host_ids, _Hip,  # noqa: F401
                                        _need_gpu, _Out, _space, _stream, _work, batch, hip)

pytestmark = pytest.mark.gpu

VALID, LIMITS, INACTIVE, COLLISION = 1, 0x20, 0x10, 0x40
ONE, THREE = 1, 0
# the per-robot build and the generic kernels: the rule never picks the generic k_step_block, set_one_launch(1) runs it
BUILDS = pytest.mark.parametrize("generic", [False, True], ids=["specialized", "generic"])


def _run(hip, s, Q, sizes, modes, stream=None, work=None, poison=False):
    """The batches Q[:B] for B in sizes, back to back on one stream without a synchronise between them; modes: per step,
    set_one_launch's argument.  poison: the caller's totals and block_tab hold 0xFF bytes beforehand.  A step asked to run
    as one launch (mode 1) that cannot raises (smplx_test_set_one_launch), and the space's count of one-launch steps is
    checked against the modes.  Returns one result per step."""
    d_q = hip.upload(Q)
    work = work if work is not None else _work(hip, s)
    outs = [_Out(hip, s) for _ in sizes]
    if poison:
        for o in outs:
            assert hip.rt.hipMemset(hip.C.c_void_p(o.tot), 0xFF, hip.C.c_size_t(4 * o.ntot)) == 0
            assert hip.rt.hipMemset(hip.C.c_void_p(o.btab), 0xFF, hip.C.c_size_t(4 * o.nbt)) == 0
    hip.sync()
    before = s.one_launch_steps()
    try:
        for B, o, m in zip(sizes, outs, modes):
            s.set_one_launch(m)
            o.issue(s, d_q, B, work, stream)
        hip.sync()
    finally:
        s.set_one_launch(-1)
    if -1 not in modes:
        assert s.one_launch_steps() - before == sum(1 for m in modes if m == ONE)
    return [o.read(s) for o in outs]


@BUILDS
def test_smallest_shapes_against_the_oracle_and_the_three_launch_step(small_cfg, batch, hip, generic):
    """Case 1: B = 1, 6 (row 5 straddles blocks 0 and 1) and 300 (59 blocks, the last one partial), each in a step of
    its own.  By the rule the per-robot build takes the kernel at B = 300, the generic build never."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q, generic_kernels=generic)
    assert s.specialized()[0] == (not generic)
    host = _host_ids(s)
    for B in SIZES:
        one, = _run(hip, s, Q, [B], [ONE])
        three, = _run(hip, s, Q, [B], [THREE])
        _assert_oracle(one, exp, host, s.N)
        _assert_same(one, three)
    before = s.one_launch_steps()
    by_rule, = _run(hip, s, Q, [300], [-1])
    assert s.one_launch_steps() == before + (0 if generic else 1)   # per-robot kernels, 59 blocks: resident in one round
    _assert_same(by_rule, three)


def test_a_forced_one_launch_step_that_cannot_run_fails_loudly(small_cfg, batch, hip):
    """Case 1, the assertion's other half: with a pipeline test hook set the kernel is ruled out, and mode 1 raises."""
    _need_gpu()
    from smpl_amd import capi
    Q, exp = batch
    s = _space(small_cfg, Q)
    s.set_pipe_prep(True)
    with pytest.raises(capi.SmplxError):
        _run(hip, s, Q, [6], [ONE])
    s.set_pipe_prep(False)
    one, = _run(hip, s, Q, [6], [ONE])
    _assert_oracle(one, exp, _host_ids(s), s.N)


@BUILDS
def test_every_waypoint_of_a_colliding_edge_is_examined(small_cfg, batch, hip, generic):
    """Case 2: no early exit across the items of an edge -- the lookup tally of a colliding edge equals the pipeline's."""
    _need_gpu()
    from oracle_binding import Oracle
    Q, exp = batch
    o = Oracle(small_cfg)
    coll = (exp["flags"] & COLLISION) != 0
    long_coll = np.zeros(coll.shape, bool)
    for i, p in zip(*np.nonzero(coll)):
        long_coll[i, p] = o.waypoint_count(Q[i], exp["q"][i, p]) >= 3
    assert long_coll.sum() >= 20
    s = _space(small_cfg, Q, generic_kernels=generic)
    one, = _run(hip, s, Q, [B_MAIN], [ONE])
    three, = _run(hip, s, Q, [B_MAIN], [THREE])
    assert np.array_equal(one["lookups"][long_coll], three["lookups"][long_coll])
    assert (one["lookups"][long_coll] > exp["lookups"][long_coll]).any()   # the reference does stop early on some of them
    _assert_same(one, three)


@BUILDS
def test_a_block_with_more_items_than_threads(small_cfg, hip, generic):
    """Case 3: primitives of 25 and 40 cells give edges of up to ~35 waypoints, so that a 128-edge block holds more
    configurations than a block of 192 or of 256 threads: its threads loop over the items."""
    _need_gpu()
    from oracle_binding import Oracle
    cfg = copy.copy(small_cfg)
    cfg.mprim = scenes.mprim_text(7, [0, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6], long_cells=40, short_cells=25)
    o = Oracle(cfg)
    o.set_order(chain=True)
    Qall = scenes.benchmark_states(scenes.ARM7_LIMITS, 300, 777)
    Q = np.ascontiguousarray(Qall[np.array([o.state_valid(q)[0] for q in Qall])][:24])
    assert Q.shape[0] == 24
    o.set_goal_joint(Q[GOAL_ROW], cfg.goal_tol)
    rows = [o.eval_state(q) for q in Q]
    exp = {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}
    M = exp["flags"].shape[1]
    walked = (exp["flags"] & (INACTIVE | LIMITS)) == 0
    items = np.zeros(walked.shape, int)
    for i, p in zip(*np.nonzero(walked)):
        items[i, p] = max(o.waypoint_count(Q[i], exp["q"][i, p]) - 1, 0)
    flat = items.reshape(-1)
    per_block = []
    for b in range((24 * M + 127) // 128):
        e0, e1 = 128 * b, min(128 * b + 127, 24 * M - 1)
        per_block.append((e1 // M - e0 // M + 1) + int(flat[e0:e1 + 1].sum()))
    assert max(per_block) > 256 and sum(n > 192 for n in per_block) >= 2
    s = _space(cfg, Q, generic_kernels=generic)
    one, = _run(hip, s, Q, [24], [ONE])
    three, = _run(hip, s, Q, [24], [THREE])
    _assert_oracle(one, exp, _host_ids(s), s.N)
    _assert_same(one, three)


def test_the_callers_buffers_carry_nothing(small_cfg, batch, hip):
    """Case 4: the caller's scratch, totals and block_tab full of 0xFF bytes beforehand: same results as on zeroed ones."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q)
    host = _host_ids(s)
    for B in (6, 300):
        dirty, = _run(hip, s, Q, [B], [ONE], work=_work(hip, s, 0xFF), poison=True)
        clean, = _run(hip, s, Q, [B], [ONE], work=_work(hip, s, 0))
        _assert_oracle(dirty, exp, host, s.N)
        _assert_same(dirty, clean)


def test_counters_are_reused_on_one_stream(small_cfg, batch, hip):
    """Case 5: steps of sizes 300, 6, 300, 1, 300 back to back on one non-blocking stream, no synchronise between them,
    one-launch and pipeline steps alternating; the stream's counter set is all-zero afterwards."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q)
    single = {B: _run(hip, s, Q, [B], [THREE])[0] for B in SIZES}
    seq = [300, 6, 300, 1, 300]
    side = hip.stream()
    for modes in ([ONE] * 5, [ONE, THREE, ONE, THREE, ONE], [THREE, ONE, THREE, ONE, THREE]):
        for got, B in zip(_run(hip, s, Q, seq, modes, stream=side), seq):
            _assert_same(got, single[B])
        assert s.step_counters_zero(side)


def test_four_streams_share_one_space(small_cfg, batch, hip):
    """Case 6: one space, four streams, four work buffers, sixteen one-launch steps round-robin, one synchronise."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q)
    single, = _run(hip, s, Q, [300], [THREE])
    d_q = hip.upload(Q)
    streams = [hip.stream() for _ in range(4)]
    works = [_work(hip, s) for _ in range(4)]
    outs = [_Out(hip, s) for _ in range(16)]
    hip.sync()
    before = s.one_launch_steps()
    s.set_one_launch(ONE)
    for i, o in enumerate(outs):
        o.issue(s, d_q, 300, works[i % 4], streams[i % 4])
    hip.sync()
    s.set_one_launch(-1)
    assert s.one_launch_steps() == before + 16
    for o in outs:
        _assert_same(o.read(s), single)
    assert all(s.step_counters_zero(st) for st in streams)


def test_pending_inserts_go_in_front_of_the_launch(small_cfg, batch):
    """Case 7: a one-launch step issued while committed states wait for the device table knows them all -- the ids equal
    those of the same step after table_sync()."""
    _need_gpu()
    from smpl_amd import capi
    Q, exp = batch
    s = capi.Space.from_config(small_cfg, batch_states=256, no_small_kernel=True)
    s.set_goal_joint(Q[GOAL_ROW], small_cfg.goal_tol)
    s.table_sync()                               # the device table exists: states created from here on wait for the next batch
    s.set_start(Q[START_ROW])
    s.plan(5.0, 1.0, 1.0, True, True, 40, 40)    # commits states; those of its last expansions are still pending
    host = _host_ids(s)
    s.set_one_launch(ONE)
    before = s.one_launch_steps()
    pending = s.expand_batch_k5(Q)
    s.table_sync()
    synced = s.expand_batch_k5(Q)
    assert s.one_launch_steps() == before + 2
    assert np.array_equal(pending["succ_id"], synced["succ_id"])
    assert np.array_equal(pending["flags"], synced["flags"]) and np.array_equal(pending["h"], synced["h"])
    assert _stream(pending) == _stream(synced)
    valid = (exp["flags"] & VALID) != 0
    want = np.full(valid.shape, -1, np.int32)
    for i, p in zip(*np.nonzero(valid)):
        want[i, p] = host.get(tuple(pending["coord"][i, p]), -1)
    assert np.array_equal(pending["succ_id"], want)
    assert (want[START_ROW][valid[START_ROW]] >= 0).all() and (want >= 0).sum() >= 1


def test_cross_query_batches_equal_each_querys_own_run(small_cfg, monkeypatch):
    """Case 8: two queries with different goals through smplx_plan_multi's host-driven loop, at most 6 states of each per
    sweep: every frontier batch is a cross-query one-launch step (per-row goal, BFS grid and table; the lead space's
    actions).  Every query equals its own three-launch run."""
    from smpl_amd import capi
    _need_gpu()
    cfg = small_cfg
    DEG = np.pi / 180.0
    cells = [[-49, 7, 21, -14, -8, -12, 16], [-21, 7, 14, -7, 8, -4, 12]]
    goals = [[cfg.start[i] + c * DEG for i, c in enumerate(cs)] for cs in cells]
    grid = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    model = capi.Model(cfg.robot_text)

    def make(mode):
        out = []
        for g in goals:
            sp = capi.Space(model, grid, cfg.mprim, cfg.params, 6, no_small_kernel=True)
            sp.set_goal_joint(g, cfg.goal_tol); sp.set_start(cfg.start)
            sp.set_one_launch(mode)
            out.append(sp)
        return out
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    solo = [sp.plan(5.0, 1.0, 1.0, True, True, 400, 400) for sp in make(THREE)]
    spaces = make(ONE)
    multi, _ = capi.Space.plan_multi(spaces, 5.0, 1.0, 1.0, True, True, 400, 400, host_threads=1)
    assert spaces[0].one_launch_steps() > 6
    assert len({tuple(a["expansion_log"]) for a in solo}) == 2       # the two queries do differ
    for a, b in zip(solo, multi):
        assert len(a["expansion_log"]) > 6
        assert a["solved"] == b["solved"] and a["cost"] == b["cost"] and np.array_equal(a["expansion_log"], b["expansion_log"])
        assert np.array_equal(a["path"], b["path"]) and a["committed_succ_evals"] == b["committed_succ_evals"]


def _other_case(name):
    """(cfg, candidate states) of the robots and grids beside the 7-variable arm on its cubic grid."""
    if name == "dual14":
        cfg = scenes.config5(n=64, nboxes=12, res=0.08)
        return cfg, np.vstack([np.array(cfg.start), scenes.random_states(scenes.ARM7_LIMITS + scenes.ARM7_LIMITS, 60, 32)])
    if name == "mixed":
        cfg = scenes.config_mixed()
        return cfg, np.vstack([np.array(cfg.start), np.array(cfg.goal), scenes.random_states(scenes.MIXED_LIMITS, 120, 9)])
    import noncubic_cases as nc
    cfg = nc.planning_case(0)
    assert len(set(cfg.grid.dims)) == 3
    return cfg, nc.bench_states()[:40]


@pytest.mark.parametrize("name", ["dual14", "mixed", "noncubic"])
def test_other_robots_and_a_non_cubic_grid(name, hip):
    """Case 9: the 14-variable dual arm (a block holds the edges of at most 4 states, rows of 56 doubles), the mixed-kinds
    robot (no table of sines and cosines: serial distance lanes) and a grid whose three extents differ: one launch equals
    three launches, and the oracle where it is compared, on at most 64 states."""
    _need_gpu()
    from oracle_binding import Oracle
    cfg, R = _other_case(name)
    o = Oracle(cfg)
    o.set_order(chain=True)
    Q = np.ascontiguousarray(R[np.array([o.state_valid(q)[0] for q in R])][:48])
    assert 6 <= Q.shape[0] <= 64
    B = Q.shape[0]
    o.set_goal_joint(Q[GOAL_ROW], cfg.goal_tol)
    rows = [o.eval_state(q) for q in Q]
    exp = {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}
    assert ((exp["flags"] & VALID) != 0).sum() > 20
    s = _space(cfg, Q)
    assert s.specialized()[0]
    one, = _run(hip, s, Q, [B], [ONE])
    three, = _run(hip, s, Q, [B], [THREE])
    _assert_oracle(one, exp, _host_ids(s), s.N)
    _assert_same(one, three)


def test_without_the_k5_outputs(small_cfg, batch, hip):
    """Case 10: expand_batch_device -- no ids, no compact stream: the dense outputs are equal, the counter set stays zero."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q)
    d_q, work = hip.upload(Q), _work(hip, s)
    got = {}
    for mode in (ONE, THREE):
        o = _Out(hip, s)
        s.set_one_launch(mode)
        before = s.one_launch_steps()
        s.expand_batch_device(d_q, B_MAIN, o.flags, o.coord, o.sq, o.h, o.cost, o.lk, work, None, None)
        hip.sync()
        s.set_one_launch(-1)
        assert s.one_launch_steps() - before == (1 if mode == ONE else 0)
        o.B = B_MAIN
        got[mode] = o.read(s)
    a, b = got[ONE], got[THREE]
    valid = (exp["flags"] & VALID) != 0
    evaluated = (exp["flags"] & INACTIVE) == 0
    assert np.array_equal(a["flags"], exp["flags"]) and np.array_equal(a["flags"], b["flags"])
    assert np.array_equal(a["coord"][valid], b["coord"][valid]) and np.array_equal(a["coord"][valid], exp["coord"][valid])
    assert np.array_equal(a["q"][evaluated], b["q"][evaluated]) and not a["q"][~evaluated].any()
    assert np.array_equal(a["h"], b["h"]) and np.array_equal(a["cost"], b["cost"]) and np.array_equal(a["lookups"], b["lookups"])
    assert s.step_counters_zero(None)
