"""The dependent memory round trips k_step_block no longer makes (csrc/step_block.h): the gate's constants are loaded at the
head of the kernel (lattice_steps.h mprim_gate), the state-table probe reads a whole slot in one round of 16-byte loads and
is cut into issue and resolve (table_probe_issue / table_probe_resolve -- table_lookup<false> of every kernel is the two
together; k_step_block issues the home slot behind its gate, ahead of the planning-link chain), and one packed 64-bit atomic
per block claims both regions of the compact stream and counts the block.

What these tests add to the one-launch and three-launch suites is inputs that take the paths those suites reach only by
chance: probe chains that go beyond the home slot (a table dense enough for it: smplx_test_set_table_slots), every branch of
the gate (the action-space switches of the planning parameters), and the claim of a block without records, of a region that
overflows and of steps back to back.  Inputs, fixtures and helpers are those of test_gpu_three_launch_step.py and
test_gpu_one_launch_step.py.  Everything is integer or fp64 work in an unchanged order: the tolerance is zero everywhere.
"""
import copy
import dataclasses

import numpy as np
import pytest

from smpl_amd import scenes
from test_gpu_one_launch_step import BUILDS, ONE, THREE, _run
from test_gpu_three_launch_step import (B_MAIN, GOAL_ROW, SIZES, START_ROW, _assert_oracle, _assert_same, _host_ids, _Hip,  # noqa: F401
                                        _need_gpu, _Out, _space, _work, batch, hip)

pytestmark = pytest.mark.gpu

VALID, INACTIVE = 1, 0x10
EXPANSIONS = 64       # of the search that fills the dense table
FRINGE = 32           # states it created last and did not expand, beside the expanded ones: the batch is at most 96 states


def _coord_hash(c):
    """smplx_coord_hash (csrc/device_types.h) of every row of c."""
    c = np.ascontiguousarray(c, np.int32).reshape(-1, c.shape[-1])
    m = np.uint64(0xFFFFFFFF)
    h = np.full(c.shape[0], 2166136261, np.uint64)
    for v in range(c.shape[1]):
        h = ((h ^ c[:, v].astype(np.uint32).astype(np.uint64)) * np.uint64(16777619)) & m
    h ^= h >> np.uint64(15); h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


def _oracle_rows(cfg, Q, goal, items=False):
    """The oracle's rows of the batch; items: also, per edge, the work items of the pipeline (waypoints behind the first)."""
    from oracle_binding import Oracle
    o = Oracle(cfg)
    o.set_order(chain=True)
    o.set_goal_joint(goal, cfg.goal_tol)
    rows = [o.eval_state(q) for q in Q]
    exp = {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}
    if items:
        walked = (exp["flags"] & (INACTIVE | 0x20)) == 0
        exp["items"] = np.zeros(walked.shape, int)
        for i, p in zip(*np.nonzero(walked)):
            exp["items"][i, p] = max(o.waypoint_count(Q[i], exp["q"][i, p]) - 1, 0)
    return exp


def _dense_space(cfg, Q, generic):
    """_space, but with a device table that starts at 64 slots and grows by the ordinary rule."""
    from smpl_amd import capi
    s = capi.Space.from_config(cfg, batch_states=256, no_small_kernel=True, generic_kernels=generic)
    s.set_table_slots(64)
    s.set_goal_joint(Q[GOAL_ROW], cfg.goal_tol)
    s.set_start(Q[START_ROW])
    log = s.plan(5.0, 1.0, 1.0, True, True, EXPANSIONS, EXPANSIONS)["expansion_log"]
    assert s.table_slots() == 0          # the host-driven search keeps no device table: the first one is table_sync's
    s.table_sync()
    return s, [int(i) for i in log]


_dense_exp = {}


@BUILDS
def test_probe_chains_beyond_the_home_slot(small_cfg, batch, hip, generic):
    """Case 1: a table between one eighth and one half full after a search of 64 expansions, and a batch of the states that
    search expanded (every committed coordinate but the start's is a successor of one of them) and of the 32 it created
    last without expanding them (their successors are mostly unknown): at most 96 states, 19 blocks, the last one partial,
    a state straddling nearly every block boundary.  (The first 64 states of a search of 40 expansions gave 4 shared home
    slots among 162 committed states on 1024 slots: a longer search and a longer batch, the floors as they were.)
    The floors are checked first: successors the host does not know whose home slot some committed coordinate occupies
    (a miss that has to walk on), and home slots that several committed coordinates share, all of them successors of this
    batch (a hit beyond the home slot, whatever order the inserts landed in)."""
    _need_gpu()
    Q, _ = batch
    s, log = _dense_space(small_cfg, Q, generic)
    assert s.specialized()[0] == (not generic)
    slots, committed = s.table_slots(), s.num_states() - 1
    assert slots >= 64 and slots & (slots - 1) == 0
    assert slots // 8 <= committed <= slots // 2
    expanded = [i for i in dict.fromkeys(log) if i != 0]
    fringe = [i for i in range(committed, 0, -1) if i not in set(expanded)][:FRINGE]
    assert len(expanded) >= 32 and len(fringe) == FRINGE
    Qd = np.ascontiguousarray(np.stack([s.get_state(i)[0] for i in expanded + fringe]))
    DENSE_B = Qd.shape[0]
    assert DENSE_B * s.M % 128 != 0 and DENSE_B <= B_MAIN
    key = Qd.tobytes()
    if key not in _dense_exp:            # the search is the oracle's, id for id: both builds expand the same states
        _dense_exp.clear()
        _dense_exp[key] = _oracle_rows(small_cfg, Qd, Q[GOAL_ROW])
    exp = _dense_exp[key]
    host = _host_ids(s)
    # ---- coverage floors
    known = np.array(list(host.keys()), np.int32)
    home_of = {c: int(h) for c, h in zip(host.keys(), _coord_hash(known) & np.uint64(slots - 1))}
    occupied = {}
    for c, h in home_of.items():
        occupied.setdefault(h, []).append(c)
    valid = (exp["flags"] & VALID) != 0
    succ = {tuple(int(x) for x in c) for c in exp["coord"][valid]}
    unknown = np.array([c for c in succ if c not in host], np.int32)
    walked_miss = sum(int(h) in occupied for h in _coord_hash(unknown) & np.uint64(slots - 1))
    shared = sum(len(cs) >= 2 and all(c in succ for c in cs) for cs in occupied.values())
    print(f"slots {slots}, committed {committed}, successors {len(succ)}, unknown {len(unknown)}, "
          f"misses beyond the home slot {walked_miss}, shared home slots {shared}")
    assert walked_miss >= 8
    assert shared >= 8
    # ---- the step
    one, = _run(hip, s, Qd, [DENSE_B], [ONE])
    three, = _run(hip, s, Qd, [DENSE_B], [THREE])
    _assert_oracle(one, exp, host, s.N)
    _assert_oracle(three, exp, host, s.N)     # table_lookup<false> of the pipeline is the same two functions
    _assert_same(one, three)
    assert (one["succ_id"] >= 0).sum() >= 8 and ((one["succ_id"] < 0) & valid).sum() >= 8


GATES = {
    "short_on": dict(),
    "long_and_short": dict(use_long_and_short=True),
    "short_off": dict(use_short=False),
    "short_off_long_and_short": dict(use_short=False, use_long_and_short=True),
    "snap_off": dict(use_xyzrpy_snap=False),
}
_gate_exp = {}


@BUILDS
@pytest.mark.parametrize("gate", list(GATES))
def test_every_branch_of_the_gate(small_cfg, batch, hip, generic, gate):
    """Case 2: the six-state batch (states beyond the short-distance threshold, one within it, the goal itself) under every
    setting of the action space's switches that the gate reads.
    The three-launch step keeps the (edge, waypoint) items of this batch in two shards of its work list, 300 items each at
    B = 6 (step.h carve_work: 16 B M items in 8 shards, block b in shard b % 8).  Where the oracle's waypoint counts say
    that a block's items cannot fit its shard, the pipeline defers edges to its whole-edge walk, which stops at the first
    collision: the lookup tally of a colliding edge is then not the waypoint-parallel one (with long primitives active
    beside the short ones near the goal: 37 against the 73 of k_step_block, which has no list and defers nothing, for one
    edge; the step before this change gives the same two figures).  There, and only there, the comparison takes
    _assert_same's mode for a work list that overflows; everything else stays compared exactly."""
    _need_gpu()
    Q, exp0 = batch
    B = SIZES[1]
    cfg = copy.copy(small_cfg)
    cfg.params = dataclasses.replace(small_cfg.params, **GATES[gate])
    if gate not in _gate_exp:
        _gate_exp[gate] = _oracle_rows(cfg, Q[:B], Q[GOAL_ROW], items=True)
    exp = _gate_exp[gate]
    flat = exp["items"].reshape(-1)
    shard_items = B * exp["flags"].shape[1] * 16 // 8 * 8 // 8
    fits = all(flat[e0:e0 + 128].sum() <= shard_items for e0 in range(0, flat.size, 128))
    if gate == "short_on":
        assert fits                      # the default setting stays compared exactly, whatever becomes of the shard arithmetic above
    print(f"{gate}: items per block {[int(flat[e0:e0 + 128].sum()) for e0 in range(0, flat.size, 128)]}, shard {shard_items}")
    if gate != "short_on":               # the switch does change which primitives are active in this batch
        assert not np.array_equal(exp["flags"] & INACTIVE, exp0["flags"][:B] & INACTIVE)
    s = _space(cfg, Q, generic_kernels=generic)
    host = _host_ids(s)
    one, = _run(hip, s, Q, [B], [ONE])
    three, = _run(hip, s, Q, [B], [THREE])
    _assert_oracle(one, exp, host, s.N)
    _assert_same(one, three, exact_tallies=fits)


def _dense_equal(a, b):
    """The dense outputs of two runs of one batch (the compact stream aside)."""
    assert np.array_equal(a["flags"], b["flags"])
    valid = (a["flags"] & VALID) != 0
    evaluated = (a["flags"] & INACTIVE) == 0
    assert np.array_equal(a["coord"][valid], b["coord"][valid])
    assert np.array_equal(a["q"][evaluated], b["q"][evaluated])
    assert np.array_equal(a["h"], b["h"]) and np.array_equal(a["cost"], b["cost"])
    assert np.array_equal(a["lookups"], b["lookups"]) and np.array_equal(a["succ_id"], b["succ_id"])


def test_a_block_without_records_still_claims(small_cfg, batch, hip):
    """Case 3a: six copies of a state in collision -- 150 edges in two blocks, no valid successor in either: each block's
    claim adds no record and still counts the block, so the step ends, the totals are zero and the set is zero again."""
    _need_gpu()
    from oracle_binding import Oracle
    Q, _ = batch
    o = Oracle(small_cfg)
    o.set_order(chain=True)
    Qall = scenes.benchmark_states(scenes.ARM7_LIMITS, 1200, 777)
    bad = next(q for q in Qall if not o.state_valid(q)[0])
    Qbad = np.ascontiguousarray(np.tile(bad, (6, 1)))
    s = _space(small_cfg, Q)
    one, = _run(hip, s, Qbad, [6], [ONE], poison=True)
    three, = _run(hip, s, Qbad, [6], [THREE])
    assert not (one["flags"] & VALID).any()
    assert [int(x) for x in one["totals"]] == [0, 0, 0]
    assert one["block_tab"].shape == (2, 4) and not one["block_tab"][:, 1].any() and not one["block_tab"][:, 3].any()
    assert np.array_equal(one["block_tab"], three["block_tab"])
    assert s.step_counters_zero(None)
    _assert_same(one, three)


def test_an_overflowing_region(small_cfg, batch, hip):
    """Case 3b: B_MAIN states into regions of 16 records (one per shard): the overflow word is 1, the dense outputs are
    those of the three-launch step, the set is zero afterwards and the next step on the stream, at full capacity, is right
    in every output."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q)
    host = _host_ids(s)
    d_q, work = hip.upload(Q), _work(hip, s)
    got = {}
    for mode in (ONE, THREE):
        o = _Out(hip, s)
        o.cap = 16
        hip.sync()
        before = s.one_launch_steps()
        s.set_one_launch(mode)
        try:
            o.issue(s, d_q, B_MAIN, work, None)
            hip.sync()
        finally:
            s.set_one_launch(-1)
        assert s.one_launch_steps() - before == (1 if mode == ONE else 0)
        raw = hip.download(o.tot, o.ntot, np.int32)
        assert raw[-1] == 1
        got[mode] = o.read(s)
        assert s.step_counters_zero(None)
    _dense_equal(got[ONE], got[THREE])
    assert np.array_equal(got[ONE]["flags"], exp["flags"])
    after, = _run(hip, s, Q, [B_MAIN], [ONE])
    _assert_oracle(after, exp, host, s.N)
    assert s.step_counters_zero(None)


def test_two_steps_back_to_back(small_cfg, batch, hip):
    """Case 3c: two one-launch steps on one non-blocking stream without a synchronise between them: the second's totals
    (and everything else of both) equal a step's of its own, and the set is zero afterwards."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q)
    single = {B: _run(hip, s, Q, [B], [THREE])[0] for B in (B_MAIN, 6)}
    side = hip.stream()
    for seq in ([B_MAIN, 6], [6, B_MAIN], [B_MAIN, B_MAIN]):
        for got, B in zip(_run(hip, s, Q, seq, [ONE, ONE], stream=side, poison=True), seq):
            _assert_same(got, single[B])
        assert s.step_counters_zero(side)
