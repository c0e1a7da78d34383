"""GetLazySuccs and GetTrueCost on the GPU (k_lazy_succs, k_true_cost) against the plain model of
tests/lazy_ref.py, which tests/test_lazy_ref.py holds to the oracle.  Every comparison is exact: integers, and the bit
patterns of doubles.

Cases: one variable (nv1), both sides of the four-word slot boundary of the state table (nv15, nv16), the most variables
(nv16, M63), a nearly empty wave of primitives (M5) and a full one (M63), and the 7-DOF arm of small_cfg.  Joint goals on
every case, XYZ goals on nv4 and nv16, a pose goal on small_cfg; each on the per-robot build and on the generic kernels."""
import numpy as np
import pytest

import lazy_ref
import width_cases as wc
from lazy_ref import F_GOAL, F_INACTIVE, F_UNCHECKED
from smpl_amd import scenes

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -1, -5
CASES = [("nv1", "joint"), ("nv4", "joint"), ("nv4", "xyz"), ("nv15", "joint"), ("nv16", "joint"), ("nv16", "xyz"), ("M5", "joint"),
         ("M63", "joint"), ("small_cfg", "joint"), ("small_cfg", "pose")]
IDS = [f"{n}-{g}" for n, g in CASES]
BUILDS = ["per-robot", "generic"]
XYZ_TOL_CELLS = 1.0       # an XYZ goal box of one cell either way around the planning link's position at the goal configuration
POSE_XYZ_TOL, POSE_RPY_TOL = [0.03] * 3, 0.2


def _need_gpu():
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _cfg(name):
    return scenes.config_small() if name == "small_cfg" else wc.case_config(name)


_BUILT = set()


@pytest.fixture()
def kernels_built(request):
    """The first space of a robot compiles its per-robot kernels (up to a minute for a 16-variable chain, then cached in the
    process and on disk): done here, in the set-up of the first test that names the robot (its `name` parameter), so that no
    test's own time holds a compiler run."""
    from smpl_amd import capi
    _need_gpu()
    cfg = _cfg(request.node.callspec.params["name"])
    if cfg.robot_text not in _BUILT:
        capi.Space.from_config(cfg, batch_states=16).close()
        _BUILT.add(cfg.robot_text)
    return _cfg


def _space(cfg, build, **kw):
    from smpl_amd import capi
    s = capi.Space.from_config(cfg, batch_states=256, generic_kernels=(build == "generic"), **kw)
    assert s.specialized()[0] == (build != "generic"), s.specialized()[1]
    return s


class Ref:
    """Everything the model says about a (case, goal kind), computed once: the states, the dense rows, the true-cost items
    with their answers."""

    def __init__(self, name, goal_kind, oracle=None):
        from oracle_binding import Oracle
        self.cfg = cfg = _cfg(name)
        o = oracle or Oracle(cfg)
        o.set_order(chain=True)
        if name == "small_cfg":
            Q = scenes.random_states(scenes.ARM7_LIMITS, 300, 21)
        else:
            Q = wc.batch_states(cfg)
        if goal_kind == "joint":
            goal = lazy_ref.Goal.joint(cfg.goal, cfg.goal_tol)
        elif goal_kind == "xyz":
            goal = lazy_ref.Goal.xyz(o.planning_fk(cfg.goal), [XYZ_TOL_CELLS * cfg.grid.res] * 3)
        else:
            # parents whose successors land on the goal pose, and the same with the wrist rolled out of the tolerance
            from test_gpu_pose_goal import _goal_pose, _small_parents
            xyz, rpy, _ = _goal_pose(cfg)
            goal = lazy_ref.Goal.pose(xyz, rpy, POSE_XYZ_TOL, POSE_RPY_TOL)
            Q = np.vstack([_small_parents(cfg)[0][:60], Q[:120]])
        self.goal = goal
        self.m = m = lazy_ref.LazyModel(o, cfg, goal)
        if goal_kind == "pose":
            # a state one of whose goal tests falls within the margin of the tolerance is judged by rounding alone: left out
            keep = []
            for q in Q:
                before = m.unsure
                m.actions(q)
                keep.append(m.unsure == before)
            Q = Q[np.array(keep)]
            assert len(Q) >= 150
        self.Q = Q = np.ascontiguousarray(Q)
        rows = [m.lazy_row(q) for q in Q]
        self.rows = {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h")}
        self._items()

    def _items(self):
        """the items of true_cost_q_batch and the model's answers"""
        m, N = self.m, self.m.N
        pq, cc, ge, want, kind = [], [], [], [], []

        def add(q, coord, what):
            pq.append(q); cc.append([0] * N if coord is None else list(coord)); ge.append(coord is None)
            want.append(m.true_cost_q(q, coord)); kind.append(what)
        for q in self.Q:
            acts = m.actions(q)
            for _, _, c, _ in acts:
                add(q, c, "succ")
            add(q, None, "goal")
            add(q, tuple(int(x) for x in m.o.state_to_coord(q)), "own")
            if acts:
                for v in range(N):
                    c = list(acts[(v * 7) % len(acts)][2])
                    c[v] += 1 if v % 2 == 0 else -1
                    add(q, tuple(c), "off")
        self.pq, self.cc, self.ge = np.array(pq), np.array(cc, np.int32), np.array(ge, np.uint8)
        self.want, self.kind = np.array(want, np.int32), np.array(kind)


_REFS = {}


def _ref(name, goal_kind):
    if (name, goal_kind) not in _REFS:
        _REFS[(name, goal_kind)] = Ref(name, goal_kind)
    return _REFS[(name, goal_kind)]


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name,goal_kind", CASES, ids=IDS)
def test_lazy_rows_equal_the_model(name, goal_kind, build, kernels_built):
    """lazy_expand_batch of every state of the case: flags everywhere; coordinate, joint values (bit for bit) and heuristic
    of every active primitive; zeros where a primitive is inactive.  No state exists yet: every id is -1.  Then, with the
    start and its lazy successors committed, the ids are those of the plain dict of the space's states."""
    r = _ref(name, goal_kind)
    s = _space(r.cfg, build)
    r.goal.set_on(s)
    got = s.lazy_expand_batch(r.Q)
    exp = r.rows
    act = (exp["flags"] & F_INACTIVE) == 0
    print(f"{name} {goal_kind} {build}: {len(r.Q)} states, {int(act.sum())} active edges, {int(((exp['flags'] & F_GOAL) != 0).sum())} goal successors")
    assert np.array_equal(got["flags"], exp["flags"])
    assert set(np.unique(exp["flags"])) <= {F_INACTIVE, F_UNCHECKED, F_UNCHECKED | F_GOAL}
    assert np.array_equal(got["coord"], exp["coord"]) and np.array_equal(_bits(got["q"]), _bits(exp["q"]))
    assert np.array_equal(got["h"], exp["h"])
    assert (got["succ_id"] == -1).all()
    if goal_kind in ("xyz", "pose") or name == "small_cfg":
        assert ((exp["flags"] & F_GOAL) != 0).sum() >= (1 if goal_kind != "joint" else 0)
    # ids: the start, its lazy successors and theirs are committed; the dense ids follow the plain dict
    sid = s.set_start(r.cfg.start)
    for i in list(s.get_lazy_succs(sid)[0])[:4]:
        s.get_lazy_succs(int(i))
    table = wc.plain_table(s)
    table = {c: i for c, i in table.items() if i > 0}
    Q2 = np.vstack([np.asarray(r.cfg.start)[None, :], r.Q[:40]])
    got = s.lazy_expand_batch(Q2)
    known = 0
    for i in range(Q2.shape[0]):
        for p in range(s.M):
            if got["flags"][i, p] & F_INACTIVE:
                assert got["succ_id"][i, p] == -1
            else:
                want = table.get(tuple(int(x) for x in got["coord"][i, p]), -1)
                assert got["succ_id"][i, p] == want
                known += want >= 0
    assert known >= len(s.get_lazy_succs(sid)[0]) >= 1
    assert s.num_states() == len(table) + 1           # the dense call created nothing
    s.close()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name,goal_kind", CASES, ids=IDS)
def test_true_cost_items_equal_the_model(name, goal_kind, build, kernels_built):
    """true_cost_q_batch over, per state: every active successor's coordinate; the goal edge; the parent's own cell, which
    no action reaches; for every variable v an active successor's coordinate moved by one cell in v alone, which matches only
    where another action lands there (a comparison that skipped a variable would match).  Cost, primitive and match count
    against the model.  Also a batch of one item and one of 131, no multiple of a wave or a block."""
    r = _ref(name, goal_kind)
    s = _space(r.cfg, build)
    r.goal.set_on(s)
    cost, prim, nm = s.true_cost_q_batch(r.pq, r.cc, r.ge)
    got = np.stack([cost, prim, nm], axis=1)
    w = r.want
    by = {k: r.kind == k for k in ("succ", "goal", "own", "off")}
    print(f"{name} {goal_kind} {build}: {len(w)} items; successors: {int((w[by['succ'], 0] > 0).sum())} pass, {int((w[by['succ'], 0] < 0).sum())} refused, "
          f"{int((w[by['succ'], 2] >= 2).sum())} with two or more matches; goal edges: {int((w[by['goal'], 2] >= 1).sum())} with a match, "
          f"{int((w[by['goal'], 2] >= 2).sum())} with two or more; own cell matched {int((w[by['own'], 2] > 0).sum())}; off-by-one matched {int((w[by['off'], 2] > 0).sum())}")
    bad = np.nonzero((got != w).any(axis=1))[0]
    assert bad.size == 0, (bad[:10], got[bad[:10]], w[bad[:10]], r.kind[bad[:10]])
    assert set(np.unique(cost)) <= {-1, lazy_ref.COST}
    assert (w[by["succ"], 2] >= 1).all() and (w[by["own"], 2] == 0).sum() >= 0.8 * by["own"].sum()
    assert (w[by["off"], 2] == 0).sum() >= 0.5 * by["off"].sum()
    for sl in (slice(3, 4), slice(5, 136)):
        c1, p1, n1 = s.true_cost_q_batch(r.pq[sl], r.cc[sl], r.ge[sl])
        assert np.array_equal(np.stack([c1, p1, n1], axis=1), w[sl])
    s.close()


def test_true_cost_with_an_attached_body(small_cfg):
    """small_cfg with a box held in the gripper: the edge check of k_true_cost sees the body.  The judge is the model over the
    oracle of the robot with the body as a pseudo-link (tests/test_gpu_attached_bodies.py); some verdicts of the bodyless
    model turn."""
    from test_gpu_attached_bodies import _held_box, _oracle_with_body, _touch, _wrist
    _need_gpu()
    cfg = small_cfg
    link, sp = _wrist(cfg), _held_box()
    bare = _ref("small_cfg", "joint")
    held = Ref("small_cfg", "joint", oracle=_oracle_with_body(cfg, link, sp, _touch(cfg)))
    assert np.array_equal(held.cc, bare.cc) and np.array_equal(held.pq, bare.pq)      # the same items
    turned = int((held.want[:, 0] != bare.want[:, 0]).sum())
    print("items whose cost the body turns:", turned, "of", len(held.want))
    assert turned >= 20
    for build in BUILDS:
        s = _space(cfg, build)
        s.attach_body("box", link, sp, allowed=_touch(cfg))
        held.goal.set_on(s)
        cost, prim, nm = s.true_cost_q_batch(held.pq, held.cc, held.ge)
        assert np.array_equal(np.stack([cost, prim, nm], axis=1), held.want), build
        # the dense rows do no check: they are the bodyless ones
        assert np.array_equal(s.lazy_expand_batch(held.Q[:50])["flags"], bare.rows["flags"][:50])
        s.close()


def _same_lattice(s, m):
    assert s.num_states() == m.num_states()
    for i in range(1, m.num_states()):
        gq, gc = s.get_state(i)
        mq, mc = m.get_state(i)
        assert np.array_equal(gc, mc) and np.array_equal(_bits(gq), _bits(mq)), i
        assert s.goal_heuristic(i) == m.goal_heuristic(i), i


@pytest.mark.parametrize("name", ["small_cfg", "nv16"])
def test_ids_follow_the_callers_sequence(name, kernels_built):
    """start; get_lazy_succs(start); get_lazy_succs of three of its successors; get_succs of a fourth; get_lazy_succs(start)
    again -- lists, state count and every state against the model after every step.  The repeated call creates nothing.
    get_true_cost and true_cost_batch agree with each other and with the model on every listed edge; bad ids and a grid edited
    after the goal are refused."""
    from oracle_binding import Oracle
    from smpl_amd import capi
    cfg = _cfg(name)
    o = Oracle(cfg)
    o.set_order(chain=True)
    goal = lazy_ref.Goal.joint(cfg.goal, cfg.goal_tol)
    m = lazy_ref.LazyModel(o, cfg, goal)
    s = _space(cfg, "per-robot")
    # no goal yet
    for call in (lambda: s.get_lazy_succs(1), lambda: s.get_true_cost(1, 2), lambda: s.true_cost_batch([1], [2]),
                 lambda: s.lazy_expand_batch(cfg.start), lambda: s.true_cost_q_batch(cfg.start, [0] * s.N)):
        with pytest.raises(capi.SmplxError) as e:
            call()
        assert e.value.code == E_STATE
    capi.lib().smplx_space_clear_status(s.h)
    goal.set_on(s)
    start = s.set_start(cfg.start)
    assert start == m.set_start(cfg.start) == 1
    edges = []

    def lazy(i):
        gs, gc = s.get_lazy_succs(i)
        ms, mc = m.get_lazy_succs(i)
        assert gs.tolist() == ms and gc.tolist() == mc, i
        edges.extend((i, int(t)) for t in ms)
        _same_lattice(s, m)
        return ms
    first = lazy(start)
    assert len(first) >= 5 and s.get_lazy_succs(0)[0].size == 0
    picks = [t for t in dict.fromkeys(first) if t > 0]
    for t in picks[:3]:
        lazy(t)
    gs, gc = s.get_succs(picks[3])
    ms, mc = m.get_succs(picks[3])
    assert gs.tolist() == ms and gc.tolist() == mc
    _same_lattice(s, m)
    n = s.num_states()
    assert lazy(start) == first and s.num_states() == n
    c = s.lazy_counters()
    assert c["lazy_launches"] + c["lazy_served"] == 5 and 1 <= c["lazy_launches"] <= 4 and c["lazy_served"] >= 1
    # true costs of every listed edge: one by one for the start's, then all in one batch
    want = [m.get_true_cost(a, b) for a, b in edges]
    one = [s.get_true_cost(a, b) for a, b in edges[:len(first)]]
    assert one == want[:len(first)]
    c = s.lazy_counters()
    assert c["true_cost_launches"] == 1 and c["cache_misses"] == 1 and c["cache_hits"] == len(first) - 1    # the others rode along
    cost, prim, nm = s.true_cost_batch([a for a, _ in edges], [b for _, b in edges])
    assert cost.tolist() == want and (nm >= 1).all() and ((prim >= 0) == (cost > 0)).all()
    print(f"{name}: {len(edges)} listed edges, {want.count(lazy_ref.COST)} pass, {want.count(-1)} refused; {s.num_states()} states")
    assert s.num_states() == n                                                   # GetTrueCost creates nothing
    # an edge nobody listed: the start is not its own successor
    assert s.get_true_cost(start, start) == m.get_true_cost(start, start) == -1
    # illegal ids
    for a, b, code in ((0, 1, E_ARG), (n, 1, E_STATE), (1, n, E_STATE), (-1, 1, E_STATE)):
        with pytest.raises(capi.SmplxError) as e:
            s.get_true_cost(a, b)
        assert e.value.code == code
    with pytest.raises(capi.SmplxError) as e:
        s.get_lazy_succs(n)
    assert e.value.code == E_STATE
    capi.lib().smplx_space_clear_status(s.h)
    s.close()
    # a grid edited after the goal (a field built on the GPU can be edited): refused until the goal is set again, which
    # starts the lattice over
    g = capi.Grid.from_boxes(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.boxes)
    s = capi.Space(capi.Model(cfg.robot_text), g, cfg.mprim, cfg.params)
    goal.set_on(s)
    assert s.set_start(cfg.start) == 1
    first = s.get_lazy_succs(1)[0].tolist()
    assert len(first) >= 5 and s.get_true_cost(1, first[0]) in (-1, lazy_ref.COST)
    s.grid.add_boxes([((0.6, 0.0, 0.9), (0.1, 0.1, 0.1))])
    for call in (lambda: s.get_lazy_succs(1), lambda: s.get_true_cost(1, first[0]), lambda: s.true_cost_batch([1], [first[0]])):
        with pytest.raises(capi.SmplxError) as e:
            call()
        assert e.value.code == E_STATE
    assert s.status()[0] == E_STATE
    goal.set_on(s)
    assert s.num_states() == 1 and s.lazy_counters()["lazy_launches"] == 0
    s.close()


@pytest.mark.parametrize("name", ["small_cfg"])
def test_riders_never_change_ids(name, monkeypatch):
    """States ride along in a GetLazySuccs launch: those of hint_frontier, and without hints the unevaluated states nearest the
    goal.  Lists and ids are those of the run without riders (SMPLX_LAZY_RIDERS=0: one launch a call), and riders are then
    served without a launch."""
    _need_gpu()
    cfg = _cfg(name)
    goal = lazy_ref.Goal.joint(cfg.goal, cfg.goal_tol)
    runs = {}
    for mode in ("none", "hinted", "auto"):
        if mode == "none":
            monkeypatch.setenv("SMPLX_LAZY_RIDERS", "0")
        else:
            monkeypatch.delenv("SMPLX_LAZY_RIDERS", raising=False)
        s = _space(cfg, "per-robot")
        goal.set_on(s)
        start = s.set_start(cfg.start)
        first = np.array([t for t in dict.fromkeys(s.get_lazy_succs(start)[0].tolist()) if t > 0], np.int32)
        if mode == "hinted":
            s.hint_frontier(first)
        lists = [s.get_lazy_succs(int(t))[0].tolist() for t in first]
        second = [t for l in lists for t in l if t > 0][:40]
        lists += [s.get_lazy_succs(int(t))[0].tolist() for t in second]
        runs[mode] = (lists, s.num_states(), [s.get_state(i)[1].tolist() for i in range(1, s.num_states())], s.lazy_counters())
        s.close()
    assert runs["none"][:3] == runs["hinted"][:3] == runs["auto"][:3]
    calls = 1 + len(runs["none"][0])
    launches = {m: r[3]["lazy_launches"] for m, r in runs.items()}
    print("GetLazySuccs calls:", calls, "launches:", launches)
    assert all(r[3]["lazy_launches"] + r[3]["lazy_served"] == calls for r in runs.values())
    assert launches["none"] == len({1, *first.tolist(), *second}) and launches["hinted"] < launches["none"] and launches["auto"] < launches["none"]
