"""The frontier step in three launches: k_pipe_setup computes the goal distance of its block's states itself, carries the
K5 inserts and zeroes the compaction totals; the work-list counters belong to the engine, one set per stream, and are
all-zero between steps.  The four-launch step (k_pipe_prep in front, smplx_test_set_pipe_prep) is the reference in the
same build; the oracle is the other one.

Inputs: valid states among scenes.benchmark_states(ARM7_LIMITS, 1200, 777) on the small scene; the goal is row 3, so
that rows 0..5 -- one block at M = 25, with row 5 straddling into the next -- hold states beyond the short-distance
threshold, one within it and the goal itself.  Everything is integer or fp64 work in an unchanged order: the tolerance
is zero.
"""
import struct

import numpy as np
import pytest

from smpl_amd import scenes

pytestmark = pytest.mark.gpu

B_MAIN = 300          # 300 x 25 edges: 59 blocks of 128 threads, the last one partial
GOAL_ROW, START_ROW = 3, 5
SIZES = (1, 6, 300)   # one block and one state / the smallest batch with a state whose gate two blocks compute / many blocks


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
    exp = {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}
    return Q, exp


def _space(cfg, Q, **kw):
    """A pipeline-only space whose device table knows the states of a short search from one of the batch's own states."""
    from smpl_amd import capi
    s = capi.Space.from_config(cfg, batch_states=256, no_small_kernel=True, **kw)
    s.set_goal_joint(Q[GOAL_ROW], cfg.goal_tol)
    s.set_start(Q[START_ROW])
    s.plan(5.0, 1.0, 1.0, True, True, 40, 40)
    s.table_sync()
    return s


class _Hip:
    """The few HIP runtime calls the tests need for buffers and streams of their own (the runtime the library uses)."""

    def __init__(self):
        import ctypes as C
        import os
        from smpl_amd import build
        # by the path the library is linked against: a bare name could resolve to another copy of the runtime that some
        # other module brought into the process, and a second runtime sees no device
        paths = [os.path.join(f[2:], "libamdhip64.so") for f in build.LINK if f.startswith("-L")]
        path = next((q for q in paths if os.path.exists(q)), "libamdhip64.so")
        self.C, self.rt = C, C.CDLL(path)
        self.bufs, self.streams = [], []

    def alloc(self, nbytes, fill=0):
        p = self.C.c_void_p()
        assert self.rt.hipMalloc(self.C.byref(p), self.C.c_size_t(max(nbytes, 1))) == 0
        self.bufs.append(p)
        assert self.rt.hipMemset(p, fill, self.C.c_size_t(max(nbytes, 1))) == 0
        return p.value

    def upload(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        assert self.rt.hipMemcpy(self.C.c_void_p(p), a.ctypes.data_as(self.C.c_void_p), self.C.c_size_t(a.nbytes), 1) == 0
        return p

    def download(self, p, n, dtype):
        a = np.zeros(n, dtype)
        assert self.rt.hipMemcpy(a.ctypes.data_as(self.C.c_void_p), self.C.c_void_p(p), self.C.c_size_t(a.nbytes), 2) == 0
        return a

    def stream(self):
        st = self.C.c_void_p()
        assert self.rt.hipStreamCreateWithFlags(self.C.byref(st), 1) == 0   # non-blocking: no implicit order with the null stream
        self.streams.append(st)
        return st.value

    def sync(self):
        assert self.rt.hipDeviceSynchronize() == 0

    def close(self):
        self.rt.hipDeviceSynchronize()
        for st in self.streams:
            self.rt.hipStreamDestroy(st)
        for p in self.bufs:
            self.rt.hipFree(p)
        self.bufs, self.streams = [], []


@pytest.fixture()
def hip():
    h = _Hip()
    yield h
    h.close()


class _Out:
    """Device buffers for the outputs of one step of up to B_MAIN states (zeroed: rows a step leaves alone stay zero)."""

    def __init__(self, hip, s):
        from smpl_amd import capi
        self.hip = hip
        BM, N = B_MAIN * s.M, s.N
        self.rb = s.compact_rec_b_bytes()
        self.cap = capi.lib().smplx_compact_capacity(s.h, B_MAIN)
        self.nbt = s.compact_blocks(B_MAIN) * 4
        self.ntot = capi.lib().smplx_compact_totals_len()
        self.flags, self.coord, self.sq = hip.alloc(BM), hip.alloc(4 * BM * N), hip.alloc(8 * BM * N)
        self.h, self.cost, self.lk, self.id = (hip.alloc(4 * BM) for _ in range(4))
        self.rec_a, self.rec_b = hip.alloc(8 * self.cap), hip.alloc(self.cap * self.rb)
        self.btab, self.tot = hip.alloc(4 * self.nbt), hip.alloc(4 * self.ntot)
        self.B = 0

    def issue(self, s, d_q, B, d_work, stream):
        """Enqueue one step on `stream` (None: the null stream); does not synchronise."""
        self.B = B
        s.expand_batch_k5_device(d_q, B, self.flags, self.coord, self.sq, self.h, self.cost, self.lk, self.id,
                                 self.rec_a, self.cap, self.rec_b, self.cap, self.btab, self.tot, d_work, None, stream)

    def read(self, s):
        B, M, N = self.B, s.M, s.N
        d = self.hip.download
        raw = d(self.tot, self.ntot, np.int32)
        return dict(flags=d(self.flags, B * M, np.uint8).reshape(B, M), coord=d(self.coord, B * M * N, np.int32).reshape(B, M, N),
                    q=d(self.sq, B * M * N, np.float64).reshape(B, M, N), h=d(self.h, B * M, np.int32).reshape(B, M),
                    cost=d(self.cost, B * M, np.int32).reshape(B, M), lookups=d(self.lk, B * M, np.int32).reshape(B, M),
                    succ_id=d(self.id, B * M, np.int32).reshape(B, M), rec_a=d(self.rec_a, 2 * self.cap, np.int32).reshape(-1, 2),
                    rec_b=d(self.rec_b, self.cap * self.rb, np.uint8).reshape(-1, self.rb),
                    block_tab=d(self.btab, self.nbt, np.int32).reshape(-1, 4)[:s.compact_blocks(B)],
                    totals=np.array([raw[0:-1:32].sum(), raw[1:-1:32].sum(), raw[-1]]))


def _work(hip, s, fill=0):
    return hip.alloc(s.expand_work_bytes(B_MAIN), fill)


def _run(hip, s, Q, sizes, stream=None, prep=None, work=None):
    """The batches Q[:B] for B in sizes, back to back on one stream without a synchronise between them (prep: per step,
    whether k_pipe_prep runs in a launch of its own).  Returns one result per step."""
    d_q = hip.upload(Q)
    work = work if work is not None else _work(hip, s)
    outs = [_Out(hip, s) for _ in sizes]
    hip.sync()
    for i, (B, o) in enumerate(zip(sizes, outs)):
        if prep is not None:
            s.set_pipe_prep(prep[i])
        o.issue(s, d_q, B, work, stream)
    hip.sync()
    s.set_pipe_prep(False)
    return [o.read(s) for o in outs]


def _stream(got):
    """The compact stream in block order: region A records and region B records."""
    seq_a, seq_b = [], []
    for ba, ca, bb, cb in got["block_tab"]:
        seq_a += [tuple(int(v) for v in x) for x in got["rec_a"][ba:ba + ca]]
        seq_b += [bytes(x) for x in got["rec_b"][bb:bb + cb]]
    return seq_a, seq_b


def _assert_same(a, b, exact_tallies=True):
    """Two runs of the same batch by the same kind of space: everything a caller may look at is equal.  exact_tallies =
    False for a shrunk work list: which edges fit it is up to the order of the blocks' claims, a deferred edge is walked
    with the reference's early exit and one on the list without, so the lookup tally of a colliding edge (and of no other)
    may differ from run to run."""
    assert np.array_equal(a["flags"], b["flags"])
    valid = (a["flags"] & 1) != 0
    evaluated = (a["flags"] & 0x10) == 0
    assert np.array_equal(a["coord"][valid], b["coord"][valid])
    assert np.array_equal(a["q"][evaluated], b["q"][evaluated])
    assert np.array_equal(a["h"], b["h"]) and np.array_equal(a["cost"], b["cost"])
    tallied = np.ones(valid.shape, bool) if exact_tallies else (a["flags"] & 0x40) == 0
    assert np.array_equal(a["lookups"][tallied], b["lookups"][tallied])
    assert np.array_equal(a["succ_id"], b["succ_id"])
    assert [int(x) for x in a["totals"]] == [int(x) for x in b["totals"]]
    assert _stream(a) == _stream(b)


def _host_ids(s):
    return {tuple(s.get_state(i)[1]): i for i in range(1, s.num_states())}


def _assert_oracle(got, exp, host, N):
    """One step against the oracle rows of its states; ids against the host's table; the stream against both.
    The lookup tally of a colliding edge has no early exit on the waypoint-parallel path (csrc/step_kernels.h, the comment above
    the pipeline): it is compared where the edge does not collide."""
    B = got["flags"].shape[0]
    e = {k: v[:B] for k, v in exp.items()}
    assert np.array_equal(got["flags"], e["flags"])
    valid = (e["flags"] & 1) != 0
    goal = (e["flags"] & 2) != 0
    evaluated = (e["flags"] & 0x10) == 0
    coll = (e["flags"] & 0x40) != 0
    assert np.array_equal(got["coord"][valid], e["coord"][valid])
    assert np.array_equal(got["q"][evaluated], e["q"][evaluated]) and not got["q"][~evaluated].any()
    assert np.array_equal(got["h"][valid], e["h"][valid]) and not got["h"][~valid].any()
    assert np.array_equal(got["cost"][valid], e["cost"][valid]) and not got["cost"][~valid].any()
    assert np.array_equal(got["lookups"][~coll], e["lookups"][~coll])
    want_id = np.full(valid.shape, -1, np.int32)
    for i, p in zip(*np.nonzero(valid)):
        want_id[i, p] = host.get(tuple(got["coord"][i, p]), -1)
    assert np.array_equal(got["succ_id"], want_id)
    need_b = valid & ((want_id < 0) | goal)
    tot = got["totals"]
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
            assert vals[0] == e["h"][i, p]
            assert list(vals[1:1 + N]) == list(e["coord"][i, p])
            assert list(vals[ints:]) == list(e["q"][i, p])
    assert ib == len(seq_b)


def test_the_gate_is_not_vacuous(batch):
    """Case 1, on the oracle: in the B = 6 and the B = 300 batch a state has active and inactive primitives, and block 0
    (rows 0..5 at M = 25) holds states on both sides of the short-distance threshold; so does a later block of B = 300."""
    Q, exp = batch
    M = exp["flags"].shape[1]
    assert M == 25
    inactive = (exp["flags"] & 0x10) != 0
    for B in (6, 300):
        ina = inactive[:B]
        assert (ina.any(axis=1) & ~ina.all(axis=1)).all()         # every state: some primitives gated off, some not
        assert len({tuple(r) for r in ina[:6]}) >= 2                # block 0: different gates, i.e. different sides of a threshold
    assert not np.array_equal(inactive[5], inactive[GOAL_ROW])      # the straddling state is gated differently from the goal row
    blocks = [set(range(128 * b // M, min(299, (128 * b + 127) // M) + 1)) for b in range(1, 59)]
    assert sum(len({tuple(inactive[i]) for i in rows}) >= 2 for rows in blocks) >= 10


@pytest.mark.parametrize("generic", [False, True])
def test_smallest_shapes_against_the_oracle_and_the_four_launch_step(small_cfg, batch, hip, generic):
    """Case 1: B = 1, 6, 300, each in a step of its own, three launches and four."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q, generic_kernels=generic)
    assert s.specialized()[0] == (not generic)
    host = _host_ids(s)
    for B in SIZES:
        three, = _run(hip, s, Q, [B])
        four, = _run(hip, s, Q, [B], prep=[True])
        _assert_oracle(three, exp, host, s.N)
        _assert_same(three, four)


def test_the_callers_scratch_carries_nothing(small_cfg, batch, hip):
    """Case 2: the same step on a work buffer full of 0xFF bytes, then on another, zero-filled one."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q)
    host = _host_ids(s)
    for B in (6, 300):
        dirty, = _run(hip, s, Q, [B], work=_work(hip, s, 0xFF))
        clean, = _run(hip, s, Q, [B], work=_work(hip, s, 0))
        _assert_oracle(dirty, exp, host, s.N)
        _assert_same(dirty, clean)


@pytest.mark.parametrize("tiny", [False, True])
def test_counters_are_reused_on_one_stream(small_cfg, batch, hip, tiny):
    """Cases 3 and 6: steps of different sizes back to back on one stream, no synchronise between them; with the work list
    shrunk (shard counts beyond capacity, edges deferred to k_pipe_finish, which reads goal_dist); with the prep switch
    flipped between steps."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q, tiny_work_list=tiny)
    host = _host_ids(s)
    single = {B: _run(hip, s, Q, [B])[0] for B in SIZES}
    for B in SIZES:
        assert not (single[B]["flags"] & 0x80).any()
        _assert_oracle(single[B], exp, host, s.N)
    if tiny:
        # some edge was in fact deferred: a deferred edge is walked with the reference's early exit, so the lookup tally of
        # colliding edges differs from the waypoint-parallel one -- and of no other edge
        full = _run(hip, _space(small_cfg, Q), Q, [300])[0]
        d = single[300]["lookups"] != full["lookups"]
        assert d.any() and not d[(exp["flags"] & 0x40) == 0].any()
    seq = [300, 6, 300, 1, 300]
    side = hip.stream()
    for prep in (None, [False, True, True, False, True]):
        for got, B in zip(_run(hip, s, Q, seq, stream=side, prep=prep), seq):
            _assert_same(got, single[B], exact_tallies=not tiny)


def test_four_streams_share_one_space(small_cfg, batch, hip):
    """Case 4: one space, four streams, four work buffers, sixteen steps round-robin, one synchronise at the end."""
    _need_gpu()
    Q, exp = batch
    s = _space(small_cfg, Q)
    single, = _run(hip, s, Q, [300])
    _assert_oracle(single, exp, _host_ids(s), s.N)
    d_q = hip.upload(Q)
    streams = [hip.stream() for _ in range(4)]
    works = [_work(hip, s) for _ in range(4)]
    outs = [_Out(hip, s) for _ in range(16)]
    hip.sync()
    for i, o in enumerate(outs):
        o.issue(s, d_q, 300, works[i % 4], streams[i % 4])
    hip.sync()
    for o in outs:
        _assert_same(o.read(s), single)


def test_inserts_ride_with_the_first_kernel(small_cfg, batch):
    """Case 5: a step issued while committed states wait for the device table knows them all -- the ids equal those of the
    same step after table_sync()."""
    _need_gpu()
    from smpl_amd import capi
    Q, exp = batch
    s = capi.Space.from_config(small_cfg, batch_states=256, no_small_kernel=True)
    s.set_goal_joint(Q[GOAL_ROW], small_cfg.goal_tol)
    s.table_sync()                               # the device table exists: states created from here on wait for the next batch
    s.set_start(Q[START_ROW])
    s.plan(5.0, 1.0, 1.0, True, True, 40, 40)    # commits states; those of its last expansions are still pending
    host = _host_ids(s)
    pending = s.expand_batch_k5(Q)
    s.table_sync()
    synced = s.expand_batch_k5(Q)
    assert np.array_equal(pending["succ_id"], synced["succ_id"])
    assert np.array_equal(pending["flags"], synced["flags"]) and np.array_equal(pending["h"], synced["h"])
    assert _stream(pending) == _stream(synced)       # (where a block's records land is up to the atomics: block order)
    valid = (exp["flags"] & 1) != 0
    want = np.full(valid.shape, -1, np.int32)
    for i, p in zip(*np.nonzero(valid)):
        want[i, p] = host.get(tuple(pending["coord"][i, p]), -1)
    assert np.array_equal(pending["succ_id"], want)
    assert (want[START_ROW][valid[START_ROW]] >= 0).all() and (want >= 0).sum() >= 1
