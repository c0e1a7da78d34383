"""k_step_block's collision items dealt in chunks of 64, the goal-distance wave first (csrc/step_block.h): chunk c of a
block's items goes to wave NW - 1 - (c mod NW), and in the per-robot build the successor evaluation of the edge lanes runs
between the item prefix and the item loop, beside the distance wave's first chunk.  Every item is the same call as before
and the per-edge tallies are integer adds, so every output is bit-identical: the three-launch step of the same space
(set_one_launch(0)) and the oracle are the references, and the tolerance is zero.

Inputs are those of test_gpu_one_launch_step.py's case 3 with shorter primitives: the first 24 valid rows of
scenes.benchmark_states(ARM7_LIMITS, 300, 777) on the small scene, goal = row 3, primitives of L and S cells.  At B = 24
and M = 25 there are five blocks; the three (L, S) rows give blocks of 3 to 8 chunks (CASES below).  B = 6 keeps block 0
and adds a partial second block.  The item totals are recomputed with the oracle and the properties the cases are there for
are asserted on them.

The pipeline's work list holds B * M * 16 items in 8 shards, so at B = 6 a block of more than 300 edge items (block 0 of the
16 / 10 row) overflows its shard: the pipeline walks the edges that did not fit with the reference's early exit, and its
tally of a colliding one of them is the reference's, not the waypoint-parallel one.  The tallies of a B = 6 step are
therefore compared, all of them and exactly, with rows 0 .. 5 of the three-launch step at B = 24, whose list holds every
edge (a tally does not depend on the batch an edge is in); everything else is compared with the three-launch step at B = 6.
"""
import copy

import numpy as np
import pytest

from smpl_amd import scenes
from test_gpu_one_launch_step import (BUILDS, COLLISION, INACTIVE, LIMITS, ONE, THREE, _run)
from test_gpu_three_launch_step import (GOAL_ROW, _assert_oracle, _assert_same, _host_ids, _need_gpu, _Out, _space, _work,  # noqa: F401
                                        hip)

pytestmark = pytest.mark.gpu

# (long_cells, short_cells): items per block at B = 24 as the oracle counts them
#   7, 4    197, 244, 221, 194, 130   four chunks with a ragged fourth beside a three-chunk block
#   10, 6   268, 327, 309, 273, 180   five and six chunks: the fifth goes to an edge wave, the sixth is the distance wave's second
#   16, 10  384, 481, 444, 417, 254   six full chunks and no ragged one, seven and eight chunks, a fourth chunk of 62 items
CASES = [(7, 4), (10, 6), (16, 10)]
B_FULL, B_PART = 24, 6
_cache = {}


def _case(small_cfg, L, S):
    """(cfg, Q, oracle rows, items per (state, primitive), colliding edges of three or more waypoints), computed once."""
    if (L, S) not in _cache:
        from oracle_binding import Oracle
        cfg = copy.copy(small_cfg)
        cfg.mprim = scenes.mprim_text(7, [0, 1, 2, 3], [0, 1, 2, 3, 4, 5, 6], long_cells=L, short_cells=S)
        o = Oracle(cfg)
        o.set_order(chain=True)
        Qall = scenes.benchmark_states(scenes.ARM7_LIMITS, 300, 777)
        Q = np.ascontiguousarray(Qall[np.array([o.state_valid(q)[0] for q in Qall])][:B_FULL])
        assert Q.shape[0] == B_FULL
        o.set_goal_joint(Q[GOAL_ROW], cfg.goal_tol)
        rows = [o.eval_state(q) for q in Q]
        exp = {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}
        walked = (exp["flags"] & (INACTIVE | LIMITS)) == 0
        W = np.zeros(walked.shape, int)
        for i, p in zip(*np.nonzero(walked)):
            W[i, p] = o.waypoint_count(Q[i], exp["q"][i, p])
        long_coll = ((exp["flags"] & COLLISION) != 0) & walked & (W >= 3)
        _cache[(L, S)] = (cfg, Q, exp, np.maximum(W - 1, 0), long_coll)
    return _cache[(L, S)]


def _totals(items, B):
    """Items of each 128-edge block of the batch items[:B]: its states, then waypoints 1 .. W - 1 of its walked edges."""
    M = items.shape[1]
    flat = items[:B].reshape(-1)
    out = []
    for b in range((B * M + 127) // 128):
        e0, e1 = 128 * b, min(128 * b + 127, B * M - 1)
        out.append((e1 // M - e0 // M + 1) + int(flat[e0:e1 + 1].sum()))
    return out


def _preconditions(small_cfg):
    """What the three rows are there for, asserted on the oracle's counts (a failure here is a failure, not a skip)."""
    full = {c: _totals(_case(small_cfg, *c)[3], B_FULL) for c in CASES}
    part = {c: _totals(_case(small_cfg, *c)[3], B_PART) for c in CASES}
    every = [n for c in CASES for n in full[c]]
    assert any(any(192 < n <= 256 for n in v) and any(n <= 192 for n in v) for v in full.values())   # ... in the same launch
    assert any(n % 64 == 0 for n in every)                  # no ragged chunk
    assert any(0 < n % 64 <= 2 for n in every)              # a last chunk of one or two items
    assert any((n + 63) // 64 > 6 for n in every)           # a third chunk for some wave
    assert len({(n + 63) // 64 for n in every}) >= 5
    for c in CASES:
        assert _case(small_cfg, *c)[4].sum() >= 10          # colliding edges of three or more waypoints among the walked
        assert len(part[c]) == 2 and part[c][0] == full[c][0] and part[c][0] > 192 and part[c][1] < 192
    return full, part


def _assert_step(one, three, full, B):
    """A one-launch step of Q[:B] against the three-launch step of Q[:B] and, for the tallies, of Q[:B_FULL] (module
    docstring): every tally is compared exactly either way."""
    _assert_same(one, three, exact_tallies=(B == B_FULL))
    assert np.array_equal(one["lookups"], full["lookups"][:B])


@BUILDS
@pytest.mark.parametrize("B", [B_FULL, B_PART])
@pytest.mark.parametrize("L,S", CASES)
def test_every_chunk_count_against_the_three_launch_step_and_the_oracle(small_cfg, hip, generic, L, S, B):
    """Blocks of three to eight chunks, with and without a ragged last chunk, and a partial block: one launch equals
    three launches and the oracle on every output and on the compact stream; the lookup tallies of colliding edges, whose
    items now land on other waves, equal the pipeline's."""
    _need_gpu()
    _preconditions(small_cfg)
    cfg, Q, exp, items, long_coll = _case(small_cfg, L, S)
    s = _space(cfg, Q, generic_kernels=generic)
    assert s.specialized()[0] == (not generic)
    one, = _run(hip, s, Q, [B], [ONE])
    three, = _run(hip, s, Q, [B], [THREE])
    full = three if B == B_FULL else _run(hip, s, Q, [B_FULL], [THREE])[0]
    _assert_oracle(one, exp, _host_ids(s), s.N)
    _assert_step(one, three, full, B)
    coll = long_coll[:B]
    assert np.array_equal(one["lookups"][coll], full["lookups"][:B][coll])
    if B == B_FULL:
        assert coll.sum() >= 10


@BUILDS
def test_the_rows_back_to_back_on_one_stream(small_cfg, hip, generic):
    """Steps of the three rows at B = 24 and B = 6 back to back on one non-blocking stream, no synchronise between them:
    each equals its own three-launch step, and every space's counter set on that stream is all-zero afterwards."""
    _need_gpu()
    _preconditions(small_cfg)
    side = hip.stream()
    spaces, singles, outs = [], [], []
    for L, S in CASES:
        cfg, Q, exp, items, long_coll = _case(small_cfg, L, S)
        s = _space(cfg, Q, generic_kernels=generic)
        singles.append([_run(hip, s, Q, [B], [THREE])[0] for B in (B_FULL, B_PART)])
        spaces.append((s, hip.upload(Q), _work(hip, s)))
        outs.append([_Out(hip, s), _Out(hip, s)])
    hip.sync()
    before = [s.one_launch_steps() for s, _, _ in spaces]
    try:
        for _ in range(2):   # the second round overwrites the first round's outputs with the same values
            for (s, d_q, work), pair in zip(spaces, outs):
                s.set_one_launch(ONE)
                for B, o in zip((B_FULL, B_PART), pair):
                    o.issue(s, d_q, B, work, side)
        hip.sync()
    finally:
        for s, _, _ in spaces:
            s.set_one_launch(-1)
    for (s, _, _), pair, want, n0 in zip(spaces, outs, singles, before):
        assert s.one_launch_steps() == n0 + 4
        for o, w, B in zip(pair, want, (B_FULL, B_PART)):
            _assert_step(o.read(s), w, want[0], B)
        assert s.step_counters_zero(side)
