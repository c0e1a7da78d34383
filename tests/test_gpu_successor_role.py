"""The successor role of k_pipe_configs: successors are evaluated beside the collision check and k_pipe_finish only joins
them with the verdict.  What that move could break and the older tests do not pin down: work done for an edge that then
collides must leave no trace, ids come from a lookup made one kernel earlier, deferred edges and successor-role edges
share blocks, and the role's blocks sit behind a grid whose size depends on B.

Inputs: valid states among scenes.benchmark_states(ARM7_LIMITS, 1200, 777) on the small scene; the goal is one of them,
so that its own snap primitive is a goal successor of zero motion (W == 0).  Everything is integer or fp64 work in an
unchanged order: the tolerance is zero.
"""
import struct

import numpy as np
import pytest

from smpl_amd import scenes

pytestmark = pytest.mark.gpu

B_MAIN = 300          # 300 x 25 edges: not a multiple of the 128-thread block
GOAL_ROW, START_ROW = 3, 5


def _need_gpu():
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


@pytest.fixture(scope="module")
def batch(small_cfg):
    """(Q, oracle rows): the oracle's GetSuccs loop body for every state of the batch."""
    from oracle_binding import Oracle
    o = Oracle(small_cfg)
    o.set_order(chain=True)
    Qall = scenes.benchmark_states(scenes.ARM7_LIMITS, 1200, 777)
    ok = np.array([o.state_valid(q)[0] for q in Qall])
    Q = np.ascontiguousarray(Qall[ok][:B_MAIN])
    assert Q.shape[0] == B_MAIN
    o.set_goal_joint(Q[GOAL_ROW], small_cfg.goal_tol)
    rows = [o.eval_state(q) for q in Q]
    exp = {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost")}
    return Q, exp


def _space(cfg, Q, **kw):
    """A space whose device table knows the states of a short search from one of the batch's own states: the successors
    of that state are known to the table, most others are not."""
    from smpl_amd import capi
    s = capi.Space.from_config(cfg, batch_states=256, **kw)
    s.set_goal_joint(Q[GOAL_ROW], cfg.goal_tol)
    s.set_start(Q[START_ROW])
    s.plan(5.0, 1.0, 1.0, True, True, 40, 40)
    s.table_sync()
    return s


def _stream(got):
    """The compact stream in block order: region A records and region B records."""
    seq_a, seq_b = [], []
    for ba, ca, bb, cb in got["block_tab"]:
        seq_a += [tuple(int(v) for v in x) for x in got["rec_a"][ba:ba + ca]]
        seq_b += [bytes(x) for x in got["rec_b"][bb:bb + cb]]
    return seq_a, seq_b


def _assert_same(a, b):
    """Two runs of the same batch: everything a caller may look at is equal."""
    assert np.array_equal(a["flags"], b["flags"])
    valid = (a["flags"] & 1) != 0
    evaluated = (a["flags"] & 0x10) == 0
    assert np.array_equal(a["coord"][valid], b["coord"][valid])
    assert np.array_equal(a["q"][evaluated], b["q"][evaluated])
    assert np.array_equal(a["h"], b["h"])
    assert np.array_equal(a["succ_id"], b["succ_id"])
    assert [int(x) for x in a["totals"]] == [int(x) for x in b["totals"]]
    assert _stream(a) == _stream(b)


def test_batch_holds_every_kind_of_edge(batch):
    """Not vacuous: collisions, limits, inactive primitives, goal successors and an edge of zero motion are all there."""
    Q, exp = batch
    f = exp["flags"]
    evaluated = (f & 0x10) == 0
    w0 = evaluated & np.all(exp["q"] == Q[:, None, :], axis=2)
    assert ((f & 0x40) != 0).sum() >= 20 and ((f & 0x20) != 0).sum() >= 20 and (~evaluated).sum() >= 20
    assert ((f & 2) != 0).sum() >= 2 and ((f & 1) != 0).sum() >= 1000
    assert (w0 & ((f & 1) != 0)).sum() >= 1


def test_verdict_joins_the_successor_and_a_rejected_edge_leaves_no_trace(small_cfg, batch):
    """(a) and (b): dense outputs against the oracle, ids against a host lookup, the stream against both."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q)
    n = s.num_states()
    host = {tuple(s.get_state(i)[1]): i for i in range(1, n)}
    B, M, N = Q.shape[0], s.M, s.N
    got = s.expand_batch_k5(Q)
    dense = s.expand_batch(Q)          # the same pipeline, with the cost column the K5 host call does not return
    assert np.array_equal(got["flags"], exp["flags"]) and np.array_equal(dense["flags"], exp["flags"])
    valid = (exp["flags"] & 1) != 0
    goal = (exp["flags"] & 2) != 0
    for g in (got, dense):
        assert np.array_equal(g["coord"][valid], exp["coord"][valid])
        assert np.array_equal(g["h"][valid], exp["h"][valid])
        assert not g["h"][~valid].any()
    assert np.array_equal(dense["cost"][valid], exp["cost"][valid]) and not dense["cost"][~valid].any()
    want_id = np.full((B, M), -1, np.int32)
    for i, p in zip(*np.nonzero(valid)):
        want_id[i, p] = host.get(tuple(got["coord"][i, p]), -1)
    assert np.array_equal(got["succ_id"], want_id)
    # known and unknown successors: the search expanded its start, a row of the batch, so every valid successor of that
    # row is a committed state; the other rows are random states far from it
    assert valid[START_ROW].sum() >= 1 and (want_id[START_ROW][valid[START_ROW]] >= 0).all()
    assert (want_id[valid] < 0).sum() >= 1000
    # the stream lists the valid edges and nothing else, in (state, primitive) order
    tot = got["totals"]
    need_b = valid & ((want_id < 0) | goal)
    assert tot[2] == 0 and tot[0] == valid.sum() and tot[1] == need_b.sum()
    seq_a, seq_b = _stream(got)
    assert len(seq_a) == valid.sum() and len(seq_b) == need_b.sum()
    ints = (N + 2) // 2 * 2
    ib = 0
    for (i, p), (rid, meta) in zip(zip(*np.nonzero(valid)), seq_a):
        assert rid == want_id[i, p]
        assert meta == (p | (0x100 if goal[i, p] else 0) | (i << 9))
        if need_b[i, p]:
            vals = struct.unpack(f"<{ints}i{N}d", seq_b[ib]); ib += 1
            assert vals[0] == exp["h"][i, p]
            assert list(vals[1:1 + N]) == list(exp["coord"][i, p])
            assert list(vals[ints:]) == list(exp["q"][i, p])
    assert ib == len(seq_b)


def test_deferred_edges_and_successor_role_edges_in_one_block(small_cfg, batch):
    """(c): with the work list shrunk most edges are walked whole by their finish thread, the few that fit and the edges
    without waypoints still come from the successor role."""
    _need_gpu()
    Q, exp = batch
    full = _space(small_cfg, Q).expand_batch_k5(Q)
    tiny = _space(small_cfg, Q, tiny_work_list=True).expand_batch_k5(Q)
    assert not (tiny["flags"] & 0x80).any()
    _assert_same(full, tiny)


def test_generic_and_per_robot_builds_agree(small_cfg, batch):
    """(d)"""
    _need_gpu()
    Q, exp = batch
    spec = _space(small_cfg, Q)
    gen = _space(small_cfg, Q, generic_kernels=True)
    assert spec.specialized()[0] and not gen.specialized()[0]
    _assert_same(spec.expand_batch_k5(Q), gen.expand_batch_k5(Q))


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("rows", [1, 37, 129])
def test_ragged_batches_on_the_pipeline(small_cfg, batch, rows, generic):
    """(e): B = 1 and batches that end inside a block; the K5 call always takes the pipeline."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q, generic_kernels=generic)
    first = GOAL_ROW if rows == 1 else 0          # B = 1: the state whose snap is the goal successor of zero motion
    got = s.expand_batch_k5(Q[first:first + rows])
    e = {k: v[first:first + rows] for k, v in exp.items()}
    assert np.array_equal(got["flags"], e["flags"])
    valid = (e["flags"] & 1) != 0
    assert np.array_equal(got["coord"][valid], e["coord"][valid]) and np.array_equal(got["h"][valid], e["h"][valid])
    assert not got["h"][~valid].any() and (got["succ_id"][~valid] == -1).all()
    assert got["totals"][0] == valid.sum() and len(_stream(got)[0]) == valid.sum()
    if rows == 1:
        assert (e["flags"] & 2).any()
