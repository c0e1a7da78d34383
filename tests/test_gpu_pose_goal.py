"""XYZ_RPY pose goals (ManipLattice::isGoal, manip_lattice.cpp:1614-1671) on every expansion path.

The oracle has no pose goal.  The references are the oracle's XYZ-goal results -- a pose goal is the XYZ goal plus one
predicate on the planning link's rotation -- and a plain numpy chain FK (pose_goal_ref.py) for that rotation, whose
position is first checked against the oracle's.  The reference goal bit is `XYZ goal bit of the oracle AND numpy
theta < rpy_tol`; rows whose theta lies within MARGIN of the tolerance are left out of the goal-bit comparison (the
engine tests 1 + trace > 4 cos^2(tol / 2) where the reference tests 2 acos(q . qg) < tol: the same predicate in other
arithmetic), and the tests bound how many rows that may be."""
import numpy as np
import pytest

import pose_goal_ref as ref
from smpl_amd import scenes

pytestmark = pytest.mark.gpu

XYZ_TOL = [0.03] * 3
RPY_TOL = 0.2
MARGIN = 1e-6
ROLL_CELLS = [12, -12, 17, -25, 40, -60, 90]      # class (b): whole cells of the wrist roll, all beyond RPY_TOL = 11.46 cells
# eps 10 -> 1 in steps of 3, bounded.  A weighted A* at eps 10 over the oracle's successors and the numpy predicate reaches the
# goal region of small_cfg after about 1500 expansions (at eps 5 not within 30000: the heuristic knows nothing of the
# orientation), so the first iteration has 13 times what it needs; the later iterations may run out and keep that solution
SEARCH = (10.0, 1.0, 3.0, True, True, 20000, 1500)


def _need_gpu():
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _goal_pose(cfg):
    """numpy pose of the configuration cfg.goal: position, roll/pitch/yaw, rotation"""
    T = ref.Chain(cfg.robot_text).transform(np.array(cfg.goal))
    return T[:3, 3].copy(), ref.matrix_rpy(T[:3, :3]), T[:3, :3].copy()


class Rows:
    """Parents, the oracle's XYZ-goal loop body for them, and the numpy orientation distance of every box-passing row."""

    def __init__(self, cfg, Q, xyz, rpy, xyz_tol, rpy_tol):
        from oracle_binding import Oracle
        self.o = o = Oracle(cfg)
        o.set_order(chain=True)
        o.set_goal_xyz(xyz, xyz_tol)
        self.Q = Q = np.ascontiguousarray(Q)
        per_state = [o.eval_state(q) for q in Q]
        self.xyz_exp = {k: np.stack([r[k] for r in per_state]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}
        f = self.xyz_exp["flags"]
        self.box = (f & 2) != 0
        chain, Rg = ref.Chain(cfg.robot_text), ref.rpy_matrix(rpy)
        self.theta = np.full(f.shape, np.nan)
        self.fk_err = 0.0      # the numpy chain's position against the oracle's, on the very states whose rotation it judges
        for i, p in zip(*np.nonzero(self.box)):
            T = chain.transform(self.xyz_exp["q"][i, p])
            self.fk_err = max(self.fk_err, np.abs(T[:3, 3] - o.planning_fk(self.xyz_exp["q"][i, p])).max())
            self.theta[i, p] = ref.rotation_angle(Rg, T[:3, :3])
        with np.errstate(invalid="ignore"):
            self.unsure = self.box & (np.abs(self.theta - rpy_tol) < MARGIN)
            self.goal = self.box & (self.theta < rpy_tol)
        self.exp = dict(self.xyz_exp)
        self.exp["flags"] = np.where(self.box & ~self.goal, f & ~np.uint8(2), f)


def _small_parents(cfg):
    """(a) the goal configuration minus each active primitive's motion: the successor lands on the goal; (b) the rows of
    (a) with the wrist roll moved by whole cells: the position stays, the orientation leaves the tolerance; (c) 200 seeded
    states elsewhere.  The first six rows alternate (a) and (b)."""
    from oracle_binding import Oracle
    o = Oracle(cfg)
    xyz, rpy, _ = _goal_pose(cfg)
    o.set_goal_xyz(xyz, XYZ_TOL)
    g = np.array(cfg.goal)
    at_goal = o.eval_state(g)
    evaluated = (at_goal["flags"] & 0x10) == 0
    A = np.array([g - (at_goal["q"][p] - g) for p in np.nonzero(evaluated)[0]])
    Bc = A.copy()
    Bc[:, 6] += np.array([ROLL_CELLS[i % len(ROLL_CELLS)] for i in range(len(A))]) * scenes.DEG
    Cc = scenes.random_states(scenes.ARM7_LIMITS, 200, 31)
    head = np.empty((6, 7))
    head[0::2], head[1::2] = A[:3], Bc[:3]
    Q = np.vstack([head, A[3:], Bc[3:], Cc])
    cls = np.array(["a", "b"] * 3 + ["a"] * (len(A) - 3) + ["b"] * (len(Bc) - 3) + ["c"] * len(Cc))
    return Q, cls


@pytest.fixture(scope="module")
def small_rows(small_cfg):
    xyz, rpy, _ = _goal_pose(small_cfg)
    Q, cls = _small_parents(small_cfg)
    r = Rows(small_cfg, Q, xyz, rpy, XYZ_TOL, RPY_TOL)
    r.cls, r.xyz, r.rpy = cls, xyz, rpy
    return r


def _pose_states(limits):
    """the states of test_planning_pose_batch"""
    return scenes.random_states(limits, 256, 77)


def test_numpy_chain_matches_the_oracles_position(small_cfg, cfg3_pr2, small_rows):
    """The numpy FK is a reference only if it is right: its position against orc_planning_fk, 1e-12, on the states it
    serves as reference for -- the 256 states of test_planning_pose_batch for each of the three robots, the goal
    configuration whose pose is the goal, and the box-passing successors of the goal-bit rows (the cfg 3 rows and the
    successors of the tight-tolerance search make the same check where they are built).  No GPU work."""
    from oracle_binding import Oracle
    for cfg, limits in [(small_cfg, scenes.ARM7_LIMITS), (cfg3_pr2, scenes.ARM7_LIMITS),
                        (scenes.config_mixed(n=16, nboxes=0), scenes.MIXED_LIMITS)]:
        o = Oracle(cfg)
        chain = ref.Chain(cfg.robot_text)
        Q = np.vstack([np.array(cfg.start), np.array(cfg.goal), _pose_states(limits)])
        worst = max(np.abs(chain.transform(q)[:3, 3] - o.planning_fk(q)).max() for q in Q)
        print(cfg.name, "numpy chain against the oracle's position: worst", worst)
        assert worst <= 1e-12, cfg.name
    print("box-passing successors of the goal-bit rows:", int(small_rows.box.sum()), "worst", small_rows.fk_err)
    assert small_rows.box.sum() > 0 and small_rows.fk_err <= 1e-12


def test_rows_reach_both_verdicts(small_rows):
    """Conditions on the input, by the oracle and numpy alone (no GPU work): (a) holds goal rows, (b) holds rows inside the
    position box that the orientation test rejects, and few rows lie within the margin of the tolerance."""
    r = small_rows
    a, b = r.cls == "a", r.cls == "b"
    goal_a = (r.goal & ~r.unsure)[a].sum()
    rejected_b = (r.box & ~r.goal & ~r.unsure)[b].sum()
    print("goal rows of (a):", goal_a, " box-passing rows of (b) the orientation rejects:", rejected_b,
          " box-passing rows:", r.box.sum(), " within the margin:", r.unsure.sum())
    assert goal_a >= 10 and rejected_b >= 10
    assert r.unsure.sum() <= 0.01 * r.box.sum()
    assert a.sum() >= 10 and a.sum() == b.sum() and (r.cls == "c").sum() == 200


@pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])
@pytest.mark.parametrize("robot", ["small", "cfg3_pr2", "mixed"])
def test_planning_pose_batch(small_cfg, cfg3_pr2, robot, generic):
    """256 seeded states: the position bit-equal to heuristic_batch's, the rotation within 1e-12 of the numpy chain and
    orthonormal within 1e-12."""
    from smpl_amd import capi
    _need_gpu()
    cfg, limits = {"small": (small_cfg, scenes.ARM7_LIMITS), "cfg3_pr2": (cfg3_pr2, scenes.ARM7_LIMITS),
                   "mixed": (scenes.config_mixed(n=16, nboxes=0), scenes.MIXED_LIMITS)}[robot]
    s = capi.Space.from_config(cfg, generic_kernels=generic)
    assert s.specialized()[0] == (not generic)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    Q = _pose_states(limits)
    T = s.planning_pose_batch(Q)
    _, xyz = s.heuristic_batch(Q)
    assert T.shape == (256, 3, 4)
    assert np.array_equal(T[:, :, 3], xyz)
    want = ref.Chain(cfg.robot_text).transforms(Q)
    err_r = np.abs(T[:, :, :3] - want[:, :3, :3]).max()
    err_o = np.abs(np.einsum("nji,njk->nik", T[:, :, :3], T[:, :, :3]) - np.eye(3)).max()
    print(robot, "rotation against numpy:", err_r, " R^T R - I:", err_o)
    assert err_r <= 1e-12 and err_o <= 1e-12
    assert len(s.planning_pose_batch(Q[:0])) == 0
    s.close()


def _assert_rows(got, r, n, name, dense=True):
    """got (the first n parents) against the reference: the goal bit outside the margin, everything else exactly"""
    f = r.exp["flags"][:n]
    skip = np.where(r.unsure[:n], np.uint8(2), np.uint8(0))
    assert np.array_equal(got["flags"] | skip, f | skip), name
    valid, evaluated, coll = (f & 1) != 0, (f & 0x10) == 0, (f & 0x40) != 0
    assert np.array_equal(got["coord"][valid], r.exp["coord"][:n][valid]), name
    assert np.array_equal(got["q"][evaluated], r.exp["q"][:n][evaluated]), name
    assert np.array_equal(got["h"][valid], r.exp["h"][:n][valid]) and not got["h"][~valid].any(), name
    if dense:
        assert np.array_equal(got["cost"][valid], r.exp["cost"][:n][valid]) and not got["cost"][~valid].any(), name
        assert np.array_equal(got["lookups"][~coll], r.exp["lookups"][:n][~coll]), name


LAUNCH_PATHS = [("fused", dict(fused=True), False),
                ("pipeline", dict(no_small_kernel=True), False),
                ("pipeline, k_pipe_prep in front", dict(no_small_kernel=True), True),
                ("pipeline, edges deferred", dict(no_small_kernel=True, tiny_work_list=True), False),
                ("small batch", dict(), False),
                ("k5", dict(no_small_kernel=True), False)]


@pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])
@pytest.mark.parametrize("path", LAUNCH_PATHS, ids=[p[0] for p in LAUNCH_PATHS])
def test_goal_bit_on_every_launch_path(small_cfg, small_rows, path, generic):
    from smpl_amd import capi
    _need_gpu()
    r = small_rows
    name, kw, prep = path
    s = capi.Space.from_config(small_cfg, generic_kernels=generic, **kw)
    assert s.specialized()[0] == (not generic)
    s.set_goal_pose(r.xyz, r.rpy, XYZ_TOL, RPY_TOL)
    assert np.array_equal(s.goal_pose(), r.xyz)
    if prep:
        s.set_pipe_prep(True)
    for n in (1, 6, len(r.Q)):
        if name == "k5":
            got = s.expand_batch_k5(r.Q[:n])
            _assert_rows(got, r, n, (name, n), dense=False)
            assert got["totals"][2] == 0
            valid = (got["flags"] & 1) != 0
            seq = [tuple(x) for ba, ca, _, _ in got["block_tab"] for x in got["rec_a"][ba:ba + ca]]
            assert len(seq) == valid.sum()
            for (i, p), (_, meta) in zip(zip(*np.nonzero(valid)), seq):      # the compacted stream carries the same goal bit
                assert meta & 0xFF == p and meta >> 9 == i
                if not r.unsure[i, p]:
                    assert bool(meta & 0x100) == bool(r.goal[i, p]), (i, p)
        else:
            got = s.expand_batch(r.Q[:n])
            _assert_rows(got, r, n, (name, n))
            if kw.get("fused"):
                assert np.array_equal(got["lookups"], r.exp["lookups"][:n]), name      # this run did take k_expand
    s.close()


def _same_plan(a, b):
    assert a["solved"] == b["solved"] and a["expansions"] == b["expansions"]
    assert np.array_equal(a["expansion_log"], b["expansion_log"])
    assert a["cost"] == b["cost"] and np.array_equal(a["path"], b["path"])


@pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])
def test_wide_tolerance_is_the_xyz_goal(small_cfg, generic, monkeypatch):
    """rpy_tol > pi admits every orientation: plan, on the host loop, on the device and through plan_multi, is the XYZ
    goal's and the oracle's."""
    from oracle_binding import Oracle
    from smpl_amd import capi
    _need_gpu()
    cfg = small_cfg
    xyz, rpy, _ = _goal_pose(cfg)
    o = Oracle(cfg)
    o.set_goal_xyz(xyz, [0.04] * 3)
    sid = o.set_start(cfg.start)
    o.search_params(5.0, 1.0, 1.0, True, True, 6000, 3000)
    eo = o.plan()
    assert eo["ok"]
    for mode in ("host", "device"):
        monkeypatch.setenv("SMPLX_SEARCH", mode)
        plans = []
        for pose in (False, True):
            s = capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic)
            assert s.specialized()[0] == (not generic)
            if pose:
                s.set_goal_pose(xyz, rpy, [0.04] * 3, 4.0)
            else:
                s.set_goal_xyz(xyz, [0.04] * 3)
            assert s.set_start(cfg.start) == sid
            plans.append(s.plan(5.0, 1.0, 1.0, True, True, 6000, 3000))
            assert s.num_states() == o.num_states()
            if mode == "device":
                assert s.search_counters()["searches"] == 1
            s.close()
        _same_plan(plans[0], plans[1])
        go = plans[1]
        assert go["solved"] == eo["ok"] and np.array_equal(go["expansion_log"], eo["expansion_log"])
        assert go["cost"] == eo["cost"] and np.array_equal(go["path"], eo["path"])
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    S = [capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic) for _ in range(3)]
    for s in S:
        s.set_goal_pose(xyz, rpy, [0.04] * 3, 4.0)
        assert s.set_start(cfg.start) == sid
    res, _ = capi.Space.plan_multi(S, 5.0, 1.0, 1.0, True, True, 6000, 3000)
    for g in res:
        assert g["solved"] == eo["ok"] and g["cost"] == eo["cost"]
        assert np.array_equal(g["expansion_log"], eo["expansion_log"]) and np.array_equal(g["path"], eo["path"])
    for s in S:
        s.close()


def _predicate(cfg, o, q, xyz, rpy, rpy_tol):
    """(valid successors in primitive order: goal by the reference rule, within the margin) of the state q; o is an
    oracle with the XYZ goal set"""
    e = o.eval_state(q)
    chain, Rg = ref.Chain(cfg.robot_text), ref.rpy_matrix(rpy)
    goal, unsure = [], []
    for p in np.nonzero(e["flags"] & 1)[0]:
        if not e["flags"][p] & 2:
            goal.append(False); unsure.append(False)
            continue
        T = chain.transform(e["q"][p])
        assert np.abs(T[:3, 3] - o.planning_fk(e["q"][p])).max() <= 1e-12      # the numpy chain on the state it judges
        th = ref.rotation_angle(Rg, T[:3, :3])
        goal.append(th < rpy_tol); unsure.append(abs(th - rpy_tol) < MARGIN)
    return np.array(goal, bool), np.array(unsure, bool)


@pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])
def test_tight_tolerance_host_and_device_agree(small_cfg, generic, monkeypatch):
    """rpy_tol = 0.2: the host loop and the device search give the same log, path and cost; the device search did run; the
    path ends in a state the numpy predicate accepts; GetSuccs names the goal id exactly where the predicate holds."""
    from oracle_binding import Oracle
    from smpl_amd import capi
    _need_gpu()
    cfg = small_cfg
    xyz, rpy, _ = _goal_pose(cfg)
    o = Oracle(cfg)
    o.set_order(chain=True)
    o.set_goal_xyz(xyz, XYZ_TOL)
    plans = {}
    for mode in ("host", "device"):
        monkeypatch.setenv("SMPLX_SEARCH", mode)
        s = capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic)
        assert s.specialized()[0] == (not generic)
        s.set_goal_pose(xyz, rpy, XYZ_TOL, RPY_TOL)
        assert np.array_equal(s.goal_orientation()[0], rpy) and s.goal_orientation()[1] == RPY_TOL
        s.set_start(cfg.start)
        before = s.search_counters()["searches"]
        g = plans[mode] = s.plan(*SEARCH)
        print(mode, "solved", g["solved"], "expansions", g["expansions"], "cost", g["cost"], "eps", g["satisfied_eps"])
        assert s.search_counters()["searches"] == before + (1 if mode == "device" else 0)
        assert g["solved"] == 1 and g["path"][-1] == 0
        qs = s.extract_path(g["path"])
        # the goal id's own joint values pass the reference rule, and they are a successor of the state before it
        T = ref.Chain(cfg.robot_text).transform(qs[-1])
        assert (np.abs(T[:3, 3] - xyz) <= np.array(XYZ_TOL) + 1e-12).all()
        assert ref.rotation_angle(ref.rpy_matrix(rpy), T[:3, :3]) < RPY_TOL + MARGIN
        goal, unsure = _predicate(cfg, o, qs[-2], xyz, rpy, RPY_TOL)
        assert (goal | unsure).any()
        s.close()
    _same_plan(plans["host"], plans["device"])
    # GetSuccs on a fresh space, in expansion order (every state is created by an earlier expansion) up to the first
    # expansion of the state before the goal on the path: id 0 exactly where the reference rule holds, checked for the first
    # 200 expanded states and for that last one, which does have a goal successor
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    s = capi.Space.from_config(cfg, generic_kernels=generic)
    assert s.specialized()[0] == (not generic)
    s.set_goal_pose(xyz, rpy, XYZ_TOL, RPY_TOL)
    s.set_start(cfg.start)
    log = plans["host"]["expansion_log"]
    last = int(np.nonzero(log == plans["host"]["path"][-2])[0][0])
    ngoal = nskip = 0
    for k, i in enumerate(log[:last + 1]):
        succ, _ = s.get_succs(int(i))
        if k >= 200 and k != last:
            continue
        goal, unsure = _predicate(cfg, o, s.get_state(int(i))[0], xyz, rpy, RPY_TOL)
        assert len(succ) == len(goal)
        assert np.array_equal((succ == 0)[~unsure], goal[~unsure]), i
        ngoal += int((goal & ~unsure).sum()); nskip += int(unsure.sum())
    print("GetSuccs replayed up to expansion", last, ": goal successors by the reference rule", ngoal, ", within the margin", nskip)
    assert ngoal > 0 and nskip <= 2
    s.close()


@pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])
@pytest.mark.parametrize("mode", ["host", "device"])
def test_zero_tolerance_has_no_goal(small_cfg, mode, generic, monkeypatch):
    """rpy_tol = 0: theta < 0 never holds.  500 expansions report no goal and the call returns unsolved, not an error."""
    from smpl_amd import capi
    _need_gpu()
    monkeypatch.setenv("SMPLX_SEARCH", mode)
    cfg = small_cfg
    xyz, rpy, _ = _goal_pose(cfg)
    s = capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic)
    assert s.specialized()[0] == (not generic)
    s.set_goal_pose(xyz, rpy, [0.2] * 3, 0.0)
    s.set_start(cfg.start)
    g = s.plan(10.0, 1.0, 3.0, True, True, 500, 500)
    assert g["solved"] == 0 and g["expansions"] >= 500 and len(g["path"]) == 0
    got = s.expand_batch(np.array([cfg.goal]))
    assert not (got["flags"] & 2).any()
    s.set_goal_pose(xyz, rpy, [0.2] * 3, -1.0)
    assert not (s.expand_batch(np.array([cfg.goal]))["flags"] & 2).any()
    s.close()


@pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])
def test_set_goals_pose_multi_equals_the_single_calls(small_cfg, generic, monkeypatch):
    from smpl_amd import capi
    _need_gpu()
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    cfg = small_cfg
    chain = ref.Chain(cfg.robot_text)
    g = np.array(cfg.goal)
    confs = [g, g + np.array([10, -5, 8, 6, 20, -10, 30]) * scenes.DEG, np.array(cfg.start) + np.array([-20, 10, 0, -10, 0, 0, 45]) * scenes.DEG]
    T = [chain.transform(q) for q in confs]
    xyz = np.array([t[:3, 3] for t in T]); rpy = np.array([ref.matrix_rpy(t[:3, :3]) for t in T])
    xyz_tol = np.array([[0.03] * 3, [0.04, 0.03, 0.05], [0.05] * 3]); rpy_tol = np.array([0.2, 0.5, 4.0])
    single = [capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic) for _ in range(3)]
    multi = [capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic) for _ in range(3)]
    for k, s in enumerate(single):
        s.set_goal_pose(xyz[k], rpy[k], xyz_tol[k], rpy_tol[k])
    capi.Space.set_goals_pose_multi(multi, xyz, rpy, xyz_tol, rpy_tol)
    one = capi.Space.from_config(cfg, batch_states=256, generic_kernels=generic)
    for s in single + multi + [one]:
        assert s.specialized()[0] == (not generic)
    capi.Space.set_goals_pose_multi([one], xyz[1], rpy[1], xyz_tol[1], rpy_tol[1:2])
    grids = [s.bfs_grid() for s in single]
    assert not np.array_equal(grids[0], grids[2])
    for a, b in list(zip(single, multi)) + [(single[1], one)]:
        assert np.array_equal(a.bfs_grid(), b.bfs_grid())
        assert np.array_equal(a.goal_pose(), b.goal_pose())
        (ra, ta), (rb, tb) = a.goal_orientation(), b.goal_orientation()
        assert np.array_equal(ra, rb) and ta == tb
    for k, (a, b) in enumerate(zip(single, multi)):
        assert np.array_equal(a.goal_orientation()[0], rpy[k]) and a.goal_orientation()[1] == rpy_tol[k]
        assert a.set_start(cfg.start) == b.set_start(cfg.start)
        _same_plan(a.plan(5.0, 1.0, 1.0, True, True, 1500, 1500), b.plan(5.0, 1.0, 1.0, True, True, 1500, 1500))
    # any other goal is no pose goal
    single[0].set_goal_xyz(xyz[0], xyz_tol[0])
    with pytest.raises(capi.SmplxError) as e:
        single[0].goal_orientation()
    assert e.value.code == -5
    for s in single + multi + [one]:
        s.close()


@pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])
def test_cfg3_with_the_references_own_request(cfg3_pr2, generic):
    """smpl_test/experiments/pr2_goal.yaml asks for x 0.4, y -0.2, z 0.36, roll = pitch = yaw = 0; the tolerances are what
    call_planner.cpp:92-96 packs into the request -- a box of 0.015 per axis and 0.05 rad about every axis -- and
    planner_interface.cpp:2300-2302, 2329-2331 and 1300-1305 carry into xyz_tolerance and rpy_tolerance, of which isGoal
    reads rpy_tolerance[0].  Whether a plan is found within a test-sized budget is not known and not asserted."""
    from smpl_amd import capi
    _need_gpu()
    cfg = cfg3_pr2
    xyz, rpy, xyz_tol, rpy_tol = [0.4, -0.2, 0.36], [0.0, 0.0, 0.0], [0.015] * 3, 0.05
    Q = np.vstack([np.array(cfg.start), scenes.random_states(scenes.ARM7_LIMITS, 64, 3)])
    r = Rows(cfg, Q, xyz, rpy, xyz_tol, rpy_tol)
    assert not r.unsure.any() and r.fk_err <= 1e-12
    s = capi.Space.from_config(cfg, generic_kernels=generic)
    assert s.specialized()[0] == (not generic)
    s.set_goal_pose(xyz, rpy, xyz_tol, rpy_tol)
    _assert_rows(s.expand_batch(Q), r, len(Q), "cfg3")
    bfs = s.bfs_grid()
    s.set_goal_xyz(xyz, xyz_tol)
    assert np.array_equal(bfs, s.bfs_grid())
    assert np.array_equal(bfs, r.o.bfs_grid())
    s.close()
