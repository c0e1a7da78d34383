"""Every kernel that walks sphere trees, on robots that drive the walks' fixed-size scratch to its edge
(tests/tree_cases.py): the 64-byte traversal stack and a 40-byte one, the queue of twelve pending pairs filled exactly,
overflowed by one and by many, pairs the kernels meet in the opposite order from the one they are stored in.
tests/test_tree_references.py shows on the CPU that the inputs used here reach those edges; here the engine's answers are
held to the oracle (validity, edges, expansion rows, searches), to the brute-force leaf minimum of tests/clearance_ref.py
(clearance) and to the lazy model of tests/lazy_ref.py (GetTrueCost).  A stack or an LDS size that is a few bytes short does
not fault, it reads back a wrong node: so every comparison is exact, and every launch shape that sizes its own LDS (128
threads, the step block's 192, the small-batch and the search block) is gone through.
"""
import ctypes as C

import numpy as np
import pytest

import clearance_ref as ref
import tree_cases as tc

pytestmark = pytest.mark.gpu

ROBOTS = ["deep", "deep40", "crowd", "order"]
BUILDS = ["specialized", "generic"]
SEARCH = (5.0, 1.0, 1.0, True, True, 250, 250)        # eps0, eps_final, eps_delta, improve, bounded, max_init, max_rep
F_VALID, F_INACTIVE, F_LIMITS, F_COLLISION = 1, 0x10, 0x20, 0x40


def _need_gpu():
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


_BUILT = set()


@pytest.fixture()
def kernels_built(request):
    """The first space of a robot compiles its per-robot kernels (then cached in the process and on disk): done here, in
    the set-up of the first test that names the robot, so that no test's own time holds a compiler run."""
    from smpl_amd import capi
    _need_gpu()
    name = request.node.callspec.params["name"]
    if name not in _BUILT:
        capi.Space.from_config(tc.case(name), batch_states=16).close()
        _BUILT.add(name)


def _space(name, build, **kw):
    from smpl_amd import capi
    s = capi.Space.from_config(tc.case(name), generic_kernels=(build == "generic"), **kw)
    assert s.specialized()[0] == (build == "specialized"), s.specialized()[1]
    return s


@pytest.fixture(scope="module")
def judged():
    """per robot: the state set with the oracle's verdicts, tallies and sphere positions (chain order), computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            o, probe = tc.oracle_and_probe(name)
            Q, S = tc.state_set(name)
            exp = [o.state_valid(q) for q in Q]
            ok, lk = np.array([e[0] for e in exp]), np.array([e[1] for e in exp], np.int32)
            P = np.stack([o.sphere_positions(q, probe.nn) for q in Q])
            for a in (ok, lk, P):
                a.setflags(write=False)
            cache[name] = (Q, S, ok, lk, P)
        return cache[name]
    return get


def _device_state_valid(s, Q):
    """smplx_cc_state_valid_batch_device: buffers from the HIP runtime, null stream"""
    hip = C.CDLL("libamdhip64.so")
    n = Q.shape[0]
    Q = np.ascontiguousarray(Q)
    ptrs = [C.c_void_p() for _ in range(3)]
    for pp, nb in zip(ptrs, (Q.nbytes, n, 4 * n)):
        assert hip.hipMalloc(C.byref(pp), C.c_size_t(nb)) == 0
    try:
        assert hip.hipMemcpy(ptrs[0], Q.ctypes.data_as(C.c_void_p), C.c_size_t(Q.nbytes), 1) == 0
        s.state_valid_batch_device(ptrs[0].value, n, ptrs[1].value, ptrs[2].value, None)
        assert hip.hipDeviceSynchronize() == 0
        v = np.zeros(n, np.uint8); lk = np.zeros(n, np.int32)
        assert hip.hipMemcpy(v.ctypes.data_as(C.c_void_p), ptrs[1], C.c_size_t(n), 2) == 0
        assert hip.hipMemcpy(lk.ctypes.data_as(C.c_void_p), ptrs[2], C.c_size_t(4 * n), 2) == 0
    finally:
        for pp in ptrs:
            hip.hipFree(pp)
    return v, lk


def _differ(got, want, Q):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return f"{bad.size} rows differ, the first {bad[:6].tolist()}: got {np.asarray(got)[bad[:6]].tolist()}, want {np.asarray(want)[bad[:6]].tolist()}"


# ----------------------------------------------------------------------------------------------------------------------
# 1. states and edges
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ROBOTS)
def test_state_verdicts_and_tallies_equal_the_oracle(name, build, judged, kernels_built):
    Q, S, ok, lk, P = judged(name)
    s = _space(name, build)
    assert np.array_equal(s.sphere_positions(Q), P)
    got_ok, got_lk = s.state_valid_batch(Q)
    assert np.array_equal(got_ok.astype(bool), ok), _differ(got_ok.astype(bool), ok, Q)
    assert np.array_equal(got_lk, lk), _differ(got_lk, lk, Q)
    dev_ok, dev_lk = _device_state_valid(s, Q)
    assert np.array_equal(dev_ok.astype(bool), ok), _differ(dev_ok.astype(bool), ok, Q)
    assert np.array_equal(dev_lk, lk)
    # a set that is no multiple of a wave, and one state alone: the last threads of a block own the last stack bytes
    for sl in (slice(0, 131), slice(len(Q) - 1, len(Q))):
        a, b = s.state_valid_batch(Q[sl])
        assert np.array_equal(a.astype(bool), ok[sl]) and np.array_equal(b, lk[sl])
    assert ok.any() and not ok.all()
    s.close()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ROBOTS)
def test_edge_verdicts_tallies_and_waypoints_equal_the_oracle(name, build, kernels_built):
    """state to state across the set, primitive-sized steps, through the fold of the deep robots; among them edges between
    two valid states that only an inner waypoint refuses: the probe finds that waypoint on interpolate's points"""
    o, probe = tc.oracle_and_probe(name)
    A, B, ok, lk, inner, show = tc.edges(name)
    s = _space(name, build)
    got_ok, got_lk, W = s.edge_valid_batch(A, B)
    assert np.array_equal(W, np.array([o.waypoint_count(a, b) for a, b in zip(A, B)]))
    assert np.array_equal(got_ok, ok), _differ(got_ok, ok, A)
    assert np.array_equal(got_lk, lk), _differ(got_lk, lk, A)
    assert (W <= 5).sum() >= 50 and (W > 5).sum() >= 50 and 20 <= ok.sum() <= len(ok) - 20
    assert len(inner) >= 20
    at_the_edge = 0
    assert len(show) >= 6
    for i in show:
        pts, n = s.interpolate(A[i], B[i])
        assert n == W[i] and np.array_equal(pts, tc.waypoints(A[i], B[i], n))
        states = [probe.state(q) for q in pts]
        bad = [k for k, st in enumerate(states) if not st["valid"]]
        assert bad and 0 < bad[0] and bad[-1] < n - 1, (i, bad, n)
        at_the_edge += any(tc.reaches_the_edge(name, st) for st in states)
    print(f"{name} {build}: {len(A)} edges, {int(ok.sum())} valid, {len(inner)} refused by inner waypoints alone; of {len(show)} looked "
          f"at, {at_the_edge} with a waypoint at the edge of the walks' scratch")
    assert at_the_edge == len(show)     # (a waypoint that holds the whole stack, overflows the queue, is decided by a swapped pair)
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 2. expansion rows through every launch shape
# ----------------------------------------------------------------------------------------------------------------------

SHAPES = {"one-launch": dict(no_small_kernel=True), "pipeline": dict(no_small_kernel=True),
          "tiny-work-list": dict(no_small_kernel=True, tiny_work_list=True), "small-batch": {}, "fused": dict(fused=True)}


def _compare_rows(exp, got, fused):
    """the masks of test_gpu_parity._compare_expand"""
    for i in range(exp["flags"].shape[0]):
        assert np.array_equal(exp["flags"][i], got["flags"][i]), f"flags of parent {i}: {exp['flags'][i].tolist()} {got['flags'][i].tolist()}"
        f = exp["flags"][i]
        v, ev, coll = (f & F_VALID) != 0, (f & F_INACTIVE) == 0, (f & F_COLLISION) != 0
        assert np.array_equal(exp["coord"][i][v], got["coord"][i][v]), i
        assert np.array_equal(exp["q"][i][ev], got["q"][i][ev]), i
        assert np.array_equal(exp["h"][i][v], got["h"][i][v]) and np.array_equal(exp["cost"][i][v], got["cost"][i][v]), i
        if fused:       # one thread per edge, the reference's waypoint order and early exit: tallies identical everywhere
            assert np.array_equal(exp["lookups"][i], got["lookups"][i]), i
        else:           # waypoint-parallel: a colliding edge has all its waypoints examined, its tally can only be larger
            assert np.array_equal(exp["lookups"][i][~coll], got["lookups"][i][~coll]), i
            assert (got["lookups"][i][coll] >= exp["lookups"][i][coll]).all(), i


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ROBOTS)
def test_expansion_rows_equal_eval_state(name, shape, build, kernels_built):
    """The parents' rows against the oracle's GetSuccs loop body through k_step_block, the three-launch pipeline, the
    pipeline's deferred pass (a work list of 128 items), k_small_batch and the fused k_expand.  The probe has looked at the
    oracle's successor configurations: some of them hold the whole stack, overflow the queue, are decided by a swapped pair."""
    cfg = tc.case(name)
    goal, P = tc.parents(name)
    exp, at_the_edge = tc.expansion_rows(name)
    assert at_the_edge >= 5
    f = exp["flags"]
    assert ((f & F_VALID) != 0).sum() >= 300 and ((f & F_COLLISION) != 0).sum() >= 20
    s = _space(name, build, **SHAPES[shape])
    s.set_goal_joint(goal, cfg.goal_tol)
    if shape in ("one-launch", "pipeline"):
        s.set_one_launch(1 if shape == "one-launch" else 0)
    before = s.one_launch_steps()
    got = s.expand_batch(P)
    assert s.one_launch_steps() - before == (1 if shape == "one-launch" else 0)
    _compare_rows(exp, got, shape == "fused")
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 3. searches
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_plans():
    from oracle_binding import Oracle
    cache = {}

    def get(name):
        if name not in cache:
            cfg = tc.case(name)
            goal, P = tc.parents(name)
            o = Oracle(cfg)
            o.set_goal_joint(goal, cfg.goal_tol)
            sid = o.set_start(P[0])
            o.search_params(*SEARCH)
            cache[name] = (o.plan(), o.num_states(), sid)
        return cache[name]
    return get


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("name", ROBOTS)
def test_bounded_search_equals_the_oracle(name, mode, build, oracle_plans, monkeypatch, kernels_built):
    """250 expansions from the first parent (the deep robots: a step away from the fold; crowd: overflowed) towards another
    state of the set.  The device-resident search runs where a k_search block with this robot's scratch fits a CU's LDS
    (search_heap_cache_entries: the count is in smplx_search_counters); where it does not, the host loop answers."""
    monkeypatch.setenv("SMPLX_SEARCH", mode)
    cfg = tc.case(name)
    goal, P = tc.parents(name)
    eo, n_states, sid = oracle_plans(name)
    assert eo["expansions"] >= 100
    s = _space(name, build, batch_states=256)
    s.set_goal_joint(goal, cfg.goal_tol)
    assert s.set_start(P[0]) == sid
    fits = s.search_counters()["heap_cache_entries"] > 0
    go = s.plan(*SEARCH)
    assert eo["ok"] == go["solved"] and eo["expansions"] == go["expansions"]
    assert np.array_equal(eo["expansion_log"], go["expansion_log"])
    assert eo["cost"] == go["cost"] and np.array_equal(eo["path"], go["path"])
    assert eo["eps"] == go["satisfied_eps"] and eo["succ_evals"] == go["committed_succ_evals"]
    assert n_states == s.num_states()
    on_device = s.search_counters()["searches"] > 0
    print(f"{name} {build} {mode}: heap cache entries {s.search_counters()['heap_cache_entries']}, searched on the device: {on_device}")
    assert on_device == (mode == "device" and fits)
    assert (go["cache_misses"] == 0) == on_device
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 4. clearance
# ----------------------------------------------------------------------------------------------------------------------

def _clearance_model(name, s, allowed=None):
    from smpl_amd import capi
    cfg = tc.case(name)
    bodies = s.attached_bodies()
    return ref.ClearanceModel(cfg.robot_text, capi.Model(cfg.robot_text).arrays(), s.grid.d2(), cfg.grid.origin, cfg.grid.res, 0.0,
                              bodies, s.attached_nodes() if bodies else None, allowed)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ROBOTS)
def test_state_clearance_equals_brute_force(name, build, judged, kernels_built):
    """the rule of test_gpu_clearance.test_states_equal_brute_force: both parts, the minimum and the witness's own term bit
    for bit against the leaf minimum; pair_clearance walks the deep pair with the same two bytes per split"""
    Q, S, ok, lk, P = judged(name)
    s = _space(name, build, no_small_kernel=True)
    c, p, w = s.state_clearance_batch(Q)
    assert np.array_equal(s.sphere_positions(Q), P)
    ref.check_against_model(_clearance_model(name, s), P, None, c, p, w)
    assert (w[:, 3] == 0).all() and set(w[:, 0].tolist()) <= {0, 1}
    assert 20 <= (c < 0).sum() <= len(c) - 20
    assert ((w[:, 0] == 1).sum() >= 20) and ((w[:, 0] == 0).sum() >= 20)
    assert ok[c > 1e-9].all()
    s.close()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ROBOTS)
def test_edge_clearance_equals_the_brute_force_minimum_over_the_waypoints(name, build, kernels_built):
    A, B, _, _, inner, _ = tc.edges(name)
    pick = np.concatenate([inner[:40], np.arange(0, len(A), 7)])
    A, B = A[pick], B[pick]
    s = _space(name, build, no_small_kernel=True)
    c, p, w = s.edge_clearance_batch(A, B)
    pts, off = [], [0]
    for a, b in zip(A, B):
        x, n = s.interpolate(a, b)
        pts.append(x if n else a[None])
        off.append(off[-1] + len(pts[-1]))
    off = np.array(off)
    Pw = s.sphere_positions(np.vstack(pts))
    m = _clearance_model(name, s)
    ec, ep = m.evaluate(Pw)
    want_c = np.minimum.reduceat(ec, off[:-1])
    want_p = np.stack([np.minimum.reduceat(ep[:, 0], off[:-1]), np.minimum.reduceat(ep[:, 1], off[:-1])], 1)
    assert np.array_equal(ref.bits(p), ref.bits(want_p))
    assert np.array_equal(ref.bits(c), ref.bits(want_c))
    assert (w[:, 3] >= 0).all() and (w[:, 3] < np.diff(off)).all()
    at = off[:-1] + w[:, 3]
    wt = m.witness_term(Pw[at], None, w)
    assert np.array_equal(ref.bits(wt), ref.bits(c))
    assert 5 <= (c < 0).sum() <= len(c) - 5
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 5. GetTrueCost
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def true_cost_items():
    import lazy_ref
    from oracle_binding import Oracle
    cache = {}

    def get(name):
        if name not in cache:
            cfg = tc.case(name)
            goal, P = tc.parents(name)
            o = Oracle(cfg)
            o.set_order(chain=True)
            m = lazy_ref.LazyModel(o, cfg, lazy_ref.Goal.joint(goal, cfg.goal_tol))
            pq, cc, ge, want = [], [], [], []
            for q in P[:40]:
                for _, _, coord, _ in m.actions(q):
                    pq.append(q); cc.append(list(coord)); ge.append(0); want.append(m.true_cost_q(q, coord))
                pq.append(q); cc.append([0] * m.N); ge.append(1); want.append(m.true_cost_q(q, None))
            cache[name] = (np.array(pq), np.array(cc, np.int32), np.array(ge, np.uint8), np.array(want, np.int32))
        return cache[name]
    return get


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["deep", "crowd"])
def test_true_cost_equals_the_lazy_model(name, build, true_cost_items, kernels_built):
    """k_true_cost over every action of 40 parents and their goal edges: cost, primitive and match count"""
    cfg = tc.case(name)
    goal, _ = tc.parents(name)
    pq, cc, ge, want = true_cost_items(name)
    assert len(pq) <= 512
    s = _space(name, build, batch_states=256)
    s.set_goal_joint(goal, cfg.goal_tol)
    cost, prim, nm = s.true_cost_q_batch(pq, cc, ge)
    got = np.stack([cost, prim, nm], axis=1)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], want[bad[:10]])
    succ = ge == 0
    print(f"{name} {build}: {len(pq)} items, {int((want[succ, 0] > 0).sum())} pass, {int((want[succ, 0] < 0).sum())} refused")
    assert (want[succ, 0] > 0).sum() >= 50 and (want[succ, 0] < 0).sum() >= 10
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 6. an attached body against a depth-16 robot tree
# ----------------------------------------------------------------------------------------------------------------------

BODY = np.array([[0.0, 0.035, 0.0, 0.01], [0.0, -0.035, 0.0, 0.01], [0.02, 0.0, 0.03, 0.008], [-0.03, 0.0, 0.0, 0.012]])
BODY_ALLOWED = ["c", "mid"]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["deep"])
def test_attached_body_against_the_deep_tree(name, build, judged, kernels_built):
    """Four spheres on `c`, around the dense end of its row, allowed to touch `c` and `mid` but not `a`: sphere_hits_tree
    and sphere_tree_clearance walk a's depth-16 tree.  Validity against the oracle of the robot with the body as a
    pseudo-link (the judge of test_gpu_attached_bodies.py), clearance against the brute-force model with bodies."""
    import test_gpu_attached_bodies as ab
    Q, S, ok0, lk0, P = judged(name)
    cfg = tc.case(name)
    o = ab._oracle_with_body(cfg, "c", BODY, BODY_ALLOWED)
    s = _space(name, build, no_small_kernel=True)
    s.attach_body("held", "c", BODY, allowed=BODY_ALLOWED)
    ok, lk = s.state_valid_batch(Q)
    eok, elk, _ = o.state_valid_batch_timed(Q)
    ok, eok = ok.astype(bool), eok.astype(bool)
    assert np.array_equal(ok, eok), _differ(ok, eok, Q)
    assert np.array_equal(lk[ok], elk[ok])
    turned = int((ok0 & ~ok).sum())
    print(f"{name} {build}: the body turns {turned} verdicts")
    assert turned >= 10 and ok.sum() >= 20
    c, p, w = s.state_clearance_batch(Q)
    ref.check_against_model(_clearance_model(name, s, allowed=[BODY_ALLOWED]), s.sphere_positions(Q), s.attached_positions(Q), c, p, w)
    assert (w[:, 0] == 3).sum() >= 10
    A, B, _, _, inner, _ = tc.edges(name)
    eok2, elk2 = o.edge_valid_batch(A[inner[:60]], B[inner[:60]])
    gok2, glk2, _ = s.edge_valid_batch(A[inner[:60]], B[inner[:60]])
    assert np.array_equal(gok2, eok2)
    s.close()
