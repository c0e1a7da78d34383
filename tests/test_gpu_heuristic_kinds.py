"""The closed-form heuristic kinds (smplx_params.heuristic: SMPLX_H_EUCLID, SMPLX_H_JOINT_DIST) on the GPU.

h of every kernel is held bit for bit to the host functions smplx_pose_distance / smplx_joint_distance
(smpl_amd/csrc/heuristics.h, which the kernels compile too) and, independently of the engine, to numpy; the gate of the
primitives to each heuristic's own metric goal distance; the host loop, the device search, smplx_plan_multi and
smplx_replan to one another; and a closed-form space is shown to hold and run no BFS.  Every test here needs
smplx_params.heuristic, which the code before this feature does not have."""
import dataclasses
import math

import numpy as np
import pytest

import pose_goal_ref as ref
import width_cases
from arastar_loop import AraStarLoop
from heuristic_cases import SEARCH, WEIGHTS, first_iteration_on_the_oracle, np_pose_distance, start_of
from smpl_amd import capi, scenes
from smpl_amd.plugin_tools import build_driver, write_query

pytestmark = pytest.mark.gpu

EUCLID, JOINT = capi.H_EUCLID, capi.H_JOINT_DIST
KINDS = [("euclid", EUCLID), ("joint_distance", JOINT)]
XYZ_TOL = [0.03] * 3
BUILDS = pytest.mark.parametrize("generic", [False, True], ids=["per-robot", "generic"])
INT_MARGIN = 1e-6          # a numpy 1000 * dist this close to an integer may truncate to the other side


def _need_gpu():
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _space(cfg, kind, generic=False, **kw):
    s = capi.Space.from_config(cfg, generic_kernels=generic, heuristic=kind, **kw)
    assert s.specialized()[0] == (not generic), s.specialized()
    return s


def _robot(name, small_cfg, cfg3_pr2):
    return {"small": (small_cfg, scenes.ARM7_LIMITS), "cfg3_pr2": (cfg3_pr2, scenes.ARM7_LIMITS),
            "mixed": (scenes.config_mixed(n=16, nboxes=0), scenes.MIXED_LIMITS)}[name]


def _goal_T(cfg):
    return ref.Chain(cfg.robot_text).transform(np.array(cfg.goal))


def _set_goal(s, cfg, goal):
    """joint, xyz or pose goal at the configuration cfg.goal; returns the goal transform the Euclidean heuristic measures
    against, as the ENGINE holds it (3x4): its own FK of the goal angles, the identity rotation, or the rotation it built
    from rpy (read back through the test hook smplx_test_goal_rotation)"""
    Tn = _goal_T(cfg)
    if goal == "joint":
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        return s.planning_pose_batch(np.array([cfg.goal]))[0]
    T = np.zeros((3, 4))
    T[:, 3] = Tn[:3, 3]
    if goal == "xyz":
        s.set_goal_xyz(Tn[:3, 3], XYZ_TOL)
        T[:, :3] = np.eye(3)
    else:
        rpy = ref.matrix_rpy(Tn[:3, :3])
        s.set_goal_pose(Tn[:3, 3], rpy, XYZ_TOL, 0.2)
        T[:, :3] = s.goal_rotation()                      # the rotation the host built from rpy with smplx_sincos
        assert np.abs(T[:, :3] - ref.rpy_matrix(rpy)).max() <= 1e-15
    assert np.array_equal(s.goal_pose(), Tn[:3, 3])
    return T


# ----------------------------------------------------------------------------------------------------------------------
# 5. batch h
# ----------------------------------------------------------------------------------------------------------------------

@BUILDS
@pytest.mark.parametrize("goal", ["joint", "xyz", "pose"])
@pytest.mark.parametrize("robot", ["small", "cfg3_pr2", "mixed"])
def test_euclid_batch_h_is_the_host_function(small_cfg, cfg3_pr2, robot, goal, generic):
    """smplx_heuristic_batch on 256 seeded states == (int)(1000 smplx_pose_distance(row of smplx_planning_pose_batch, goal
    transform, w)), row for row and bit for bit, for joint, xyz and pose goals, with the default weights and after
    smplx_set_euclid_weights.  The goal transform is the one the engine holds (_set_goal)."""
    _need_gpu()
    cfg, limits = _robot(robot, small_cfg, cfg3_pr2)
    Q = scenes.random_states(limits, 256, 77)
    s = _space(cfg, EUCLID, generic)
    for w in WEIGHTS:
        if w != WEIGHTS[0]:
            s.set_euclid_weights(w)
            with pytest.raises(capi.SmplxError) as e:       # the goal must be set again: no stale h
                s.expand_batch(Q[:1])
            assert e.value.code == capi.E_STATE
        Tg = _set_goal(s, cfg, goal)
        h, xyz = s.heuristic_batch(Q)
        T = s.planning_pose_batch(Q)
        assert np.array_equal(T[:, :, 3], xyz)
        d = np.array([1000.0 * capi.pose_distance(t, Tg, w) for t in T])
        assert np.array_equal(h, d.astype(np.int64)), (robot, goal, w)
        if goal == "joint":
            assert np.array_equal(s.goal_rotation(), Tg[:, :3])
        assert (h >= 0).all() and h.max() > 100
        # the metric goal distance of the kind: the plain distance to the goal position
        md = s.heuristic_metric_goal_distance(xyz)
        assert np.allclose(md, np.linalg.norm(xyz - Tg[:, 3], axis=1), rtol=0, atol=1e-12)
    s.close()


@BUILDS
@pytest.mark.parametrize("robot", ["small", "cfg3_pr2", "mixed"])
def test_euclid_batch_h_against_numpy(small_cfg, cfg3_pr2, robot, generic):
    """Independence from the engine: the same rows against the numpy chain FK and numpy's distance, under a joint goal.
    Equal wherever numpy's 1000 dist is farther than 1e-6 from an integer, within 1 elsewhere; at most 1 % of the rows may
    be that close (a condition on the seeds, checked on the numpy side alone)."""
    _need_gpu()
    cfg, limits = _robot(robot, small_cfg, cfg3_pr2)
    Q = scenes.random_states(limits, 256, 77)
    chain = ref.Chain(cfg.robot_text)
    Tg = chain.transform(np.array(cfg.goal))
    s = _space(cfg, EUCLID, generic)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    h, _ = s.heuristic_batch(Q)
    d = np.array([1000.0 * np_pose_distance(t, Tg, WEIGHTS[0]) for t in chain.transforms(Q)])
    sure = np.abs(d - np.rint(d)) > INT_MARGIN
    print(robot, "rows within", INT_MARGIN, "of an integer:", int((~sure).sum()), "of", len(d))
    assert (~sure).sum() <= 0.01 * len(d)
    assert np.array_equal(h[sure], d[sure].astype(np.int64)) and (np.abs(h - d.astype(np.int64)) <= 1).all()
    s.close()


@BUILDS
@pytest.mark.parametrize("nv", [1, 15, 16])
def test_joint_distance_batch_h_is_the_host_function(nv, generic):
    """chain robots of 1, 15 and 16 variables (16: the last variable lies in a fifth word of a table slot): h equals
    (int)(1000 smplx_joint_distance(state, goal angles)) and the plain Python loop; 0 for every state under a pose goal
    and an xyz goal; the metric goal distance is 0 everywhere."""
    _need_gpu()
    cfg = width_cases.width_case(nv)
    Q = width_cases.batch_states(cfg, n=256, seed=9)
    s = _space(cfg, JOINT, generic)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    h, xyz = s.heuristic_batch(Q)
    want = np.array([int(1000.0 * capi.joint_distance(q, cfg.goal)) for q in Q])
    loop = np.array([int(1000.0 * math.sqrt(sum((float(a) - float(b)) ** 2 for a, b in zip(q, cfg.goal)))) for q in Q])
    assert np.array_equal(h, want) and np.array_equal(h, loop) and h.max() > 0
    assert not s.heuristic_metric_goal_distance(xyz).any()
    T = s.planning_pose_batch(np.array([cfg.goal]))[0]
    s.set_goal_xyz(T[:, 3], XYZ_TOL)
    assert not s.heuristic_batch(Q)[0].any()
    s.set_goal_pose(T[:, 3], [0.1, 0.2, 0.3], XYZ_TOL, 0.2)
    assert not s.heuristic_batch(Q)[0].any()
    s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 6. every launch path
# ----------------------------------------------------------------------------------------------------------------------

LAUNCH_PATHS = [("fused", dict(fused=True), False, False),
                ("pipeline", dict(no_small_kernel=True), False, False),
                ("pipeline, k_pipe_prep in front", dict(no_small_kernel=True), True, False),
                ("pipeline, edges deferred", dict(no_small_kernel=True, tiny_work_list=True), False, False),
                ("small batch", dict(), False, False),
                ("k5", dict(no_small_kernel=True), False, False),
                ("lazy", dict(), False, True)]


def _parents(cfg):
    """the goal configuration, the start and 200 seeded states"""
    return np.vstack([np.array(cfg.goal), np.array(cfg.start), scenes.random_states(scenes.ARM7_LIMITS, 200, 31)])


@BUILDS
@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("path", LAUNCH_PATHS, ids=[p[0] for p in LAUNCH_PATHS])
def test_successor_h_on_every_launch_path(small_cfg, path, kind, generic):
    """each successor's h equals the batch h of that successor's joint values; the rows of every path are the rows of
    the fused pair"""
    _need_gpu()
    name, kw, prep, lazy = path
    cfg = small_cfg
    Q = _parents(cfg)
    s = _space(cfg, kind[1], generic, **kw)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    if prep:
        s.set_pipe_prep(True)
    base = _space(cfg, kind[1], generic, fused=True)
    base.set_goal_joint(cfg.goal, cfg.goal_tol)
    want = base.expand_batch(Q)
    for n in (1, 6, len(Q)):
        got = s.lazy_expand_batch(Q[:n]) if lazy else (s.expand_batch_k5(Q[:n]) if name == "k5" else s.expand_batch(Q[:n]))
        f = got["flags"]
        have = (f & 4) != 0 if lazy else (f & 1) != 0
        assert have.sum() > 0
        hb, _ = s.heuristic_batch(got["q"][have])
        assert np.array_equal(got["h"][have], hb), (name, n)
        if not lazy:
            assert np.array_equal(f, want["flags"][:n]) and np.array_equal(got["h"], want["h"][:n]), (name, n)
            assert np.array_equal(got["coord"][have], want["coord"][:n][have])
        else:
            assert np.array_equal((f & 0x10) != 0, (want["flags"][:n] & 0x10) != 0)
    assert got["h"][have].max() > 0
    s.close(); base.close()


# ----------------------------------------------------------------------------------------------------------------------
# 7. the gate
# ----------------------------------------------------------------------------------------------------------------------

def _all_prims_cfg(cfg):
    """cfg with use_long_and_short and thresholds larger than the grid: every primitive is evaluated for every parent"""
    return dataclasses.replace(cfg, params=dataclasses.replace(cfg.params, use_long_and_short=True, short_thresh=1e9, xyzrpy_thresh=1e9))


def _prim_classes(cfg):
    """(long, short, snap) masks over the primitives, from the oracle's own gate under the BFS: at the goal configuration
    (distance 0) short and snap are active; at a state between the two thresholds short alone"""
    from oracle_binding import Oracle
    o = Oracle(cfg)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    at_goal = (o.eval_state(np.array(cfg.goal))["flags"] & 0x10) == 0
    for q in scenes.random_states(scenes.ARM7_LIMITS, 400, 5):
        d = o.metric_goal_distance(*o.planning_fk(q))
        if cfg.params.xyzrpy_thresh + 0.04 < d <= cfg.params.short_thresh - 0.04:
            mid = (o.eval_state(q)["flags"] & 0x10) == 0
            return ~at_goal, at_goal & mid, at_goal & ~mid
    raise AssertionError("no state between the thresholds")


def _gate_parents(cfg, all_rows_at_goal):
    g = np.array(cfg.goal)
    near = np.array([g - (all_rows_at_goal["q"][p] - g) for p in range(all_rows_at_goal["q"].shape[0])])
    return np.vstack([near, scenes.random_states(scenes.ARM7_LIMITS, 200, 31)])


@BUILDS
def test_euclid_gate_is_the_euclidean_distance(small_cfg, generic):
    """The engine's rows under the Euclidean kind (real thresholds) are the oracle's rows with every primitive evaluated,
    masked by the numpy gate: the Euclidean distance of the numpy FK to the goal position against each threshold.  Flags,
    coordinates, joint values and cost are the oracle's; h is the batch h (test 5).  A parent within 1e-9 of a threshold is
    left out; at most two may be."""
    from oracle_binding import Oracle
    _need_gpu()
    cfg = small_cfg
    assert not cfg.params.use_long_and_short and cfg.params.use_short and cfg.params.use_xyzrpy_snap
    long_, short, snap = _prim_classes(cfg)
    assert long_.sum() > 0 and short.sum() > 0 and snap.sum() == 1
    o = Oracle(_all_prims_cfg(cfg))
    o.set_order(chain=True)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    Q = _gate_parents(cfg, o.eval_state(np.array(cfg.goal)))
    chain = ref.Chain(cfg.robot_text)
    gxyz = chain.transform(np.array(cfg.goal))[:3, 3]
    dist = np.array([np.linalg.norm(chain.transform(q)[:3, 3] - gxyz) for q in Q])
    ts, tn = cfg.params.short_thresh, cfg.params.xyzrpy_thresh
    keep = (np.abs(dist - ts) > 1e-9) & (np.abs(dist - tn) > 1e-9)
    assert (~keep).sum() <= 2
    assert (dist[keep] <= ts).sum() >= short.sum() and (dist[keep] > ts).sum() >= 20      # both sides of the gate are met
    s = _space(cfg, EUCLID, generic)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    got = s.expand_batch(Q)
    checked = 0
    for i in np.nonzero(keep)[0]:
        exp = o.eval_state(Q[i])
        near_s, near_n = dist[i] <= ts, dist[i] <= tn
        active = np.where(long_, not near_s, np.where(short, near_s, near_n))      # manip_lattice_action_space.cpp:662-691
        f = np.where(active, exp["flags"], np.uint8(0x10))
        assert np.array_equal(got["flags"][i], f), i
        ev = active & ((exp["flags"] & 0x10) == 0)
        v = ev & ((exp["flags"] & 1) != 0)
        assert np.array_equal(got["q"][i][ev], exp["q"][ev]) and np.array_equal(got["coord"][i][v], exp["coord"][v])
        assert np.array_equal(got["cost"][i][v], exp["cost"][v])
        checked += int(v.sum())
    assert checked > 500
    valid = (got["flags"] & 1) != 0
    hb, _ = s.heuristic_batch(got["q"][valid])
    assert np.array_equal(got["h"][valid], hb)
    s.close()


@BUILDS
def test_joint_distance_gate_sees_every_state_at_the_goal(small_cfg, generic):
    """getMetricGoalDistance is 0.0: short primitives and the joint-goal snap are active for every parent, the long ones for
    none; with use_long_and_short all are.  The rows are the oracle's with every primitive evaluated."""
    from oracle_binding import Oracle
    _need_gpu()
    cfg = small_cfg
    long_, short, snap = _prim_classes(cfg)
    o = Oracle(_all_prims_cfg(cfg))
    o.set_order(chain=True)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    Q = _gate_parents(cfg, o.eval_state(np.array(cfg.goal)))[::3]
    both = dataclasses.replace(cfg, params=dataclasses.replace(cfg.params, use_long_and_short=True))
    for c, active in ((cfg, short | snap), (both, np.ones(len(long_), bool))):
        s = _space(c, JOINT, generic)
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        got = s.expand_batch(Q)
        for i, q in enumerate(Q):
            exp = o.eval_state(q)
            assert np.array_equal(got["flags"][i], np.where(active, exp["flags"], np.uint8(0x10))), i
            v = active & ((exp["flags"] & 1) != 0)
            assert np.array_equal(got["coord"][i][v], exp["coord"][v]) and np.array_equal(got["cost"][i][v], exp["cost"][v])
        s.close()


# ----------------------------------------------------------------------------------------------------------------------
# 8. the searches agree with one another
# ----------------------------------------------------------------------------------------------------------------------

def _same_plan(a, b):
    assert a["solved"] == b["solved"] and a["expansions"] == b["expansions"]
    assert np.array_equal(a["expansion_log"], b["expansion_log"])
    assert a["cost"] == b["cost"] and np.array_equal(a["path"], b["path"]) and a["satisfied_eps"] == b["satisfied_eps"]


def _search_cfg(cfg, kind, snap=True):
    """Under joint distance the gate sees every state at the goal.  Without use_long_and_short only the short primitives
    and the snap ever move the arm, so a search across the workspace needs the long ones switched on beside them; and the
    snap is active at EVERY state, so a search ends with its first expansion wherever the straight edge to the goal
    configuration is free (from both starts of small_cfg it is) -- snap=False takes the snap away to get a search of
    more than one step (it then runs out of its budget: the logs of 3000 expansions are what is compared)."""
    if kind != JOINT:
        return cfg
    return dataclasses.replace(cfg, params=dataclasses.replace(cfg.params, use_long_and_short=True, use_xyzrpy_snap=snap))


def _plan(cfg, kind, generic, mode, monkeypatch, goal="joint", search=SEARCH, near=True, snap=True):
    monkeypatch.setenv("SMPLX_SEARCH", mode)
    s = _space(_search_cfg(cfg, kind, snap), kind, generic, batch_states=256)
    _set_goal(s, cfg, goal)
    s.set_start(start_of(cfg, near))
    before = s.search_counters()["searches"]
    g = s.plan(*search)
    assert s.search_counters()["searches"] == before + (1 if mode == "device" else 0)      # the device search did run
    s.close()
    return g


@BUILDS
@pytest.mark.parametrize("near", [True, False], ids=["near", "far"])
@pytest.mark.parametrize("case", [("euclid", EUCLID, "joint", True), ("euclid", EUCLID, "pose", True),
                                  ("joint_distance", JOINT, "joint", True), ("joint_distance", JOINT, "joint", False)],
                         ids=["euclid-joint", "euclid-pose", "joint_distance-joint", "joint_distance-joint-no-snap"])
def test_host_loop_and_device_search_agree(small_cfg, case, near, generic, monkeypatch):
    """the same expansion log, path, cost and satisfied eps from the host loop and the device search, which did run; from
    the near start a joint goal is reached"""
    _need_gpu()
    _, kind, goal, snap = case
    plans = {m: _plan(small_cfg, kind, generic, m, monkeypatch, goal, near=near, snap=snap) for m in ("host", "device")}
    g = plans["host"]
    print(case[0], goal, "snap" if snap else "no snap", "near" if near else "far", "solved", g["solved"], "expansions", g["expansions"], "cost", g["cost"],
          "eps", g["satisfied_eps"])
    _same_plan(plans["host"], plans["device"])
    assert g["expansions"] > 0
    if goal == "joint" and near and snap:
        assert g["solved"] == 1 and g["path"][-1] == 0


@BUILDS
def test_plan_multi_mixes_the_kinds(small_cfg, generic, monkeypatch):
    """four queries whose spaces are of all three kinds in one smplx_plan_multi: each record equals its single run.  With
    per-robot kernels BFS and closed-form spaces cannot share a grouped launch (the kind is a constant of that build, DESIGN.md
    section 21), so this call runs its queries ungrouped; with the generic kernels, which read the kind per space, the four
    share their launches."""
    _need_gpu()
    cfg = small_cfg
    kinds = [capi.H_BFS, EUCLID, JOINT, EUCLID]
    for mode in ("host", "device"):
        single = [_plan(cfg, k, generic, mode, monkeypatch) for k in kinds]
        monkeypatch.setenv("SMPLX_SEARCH", mode)
        S = [_space(_search_cfg(cfg, k), k, generic, batch_states=256) for k in kinds]
        capi.Space.set_goals_joint_multi(S, [cfg.goal] * 4, [cfg.goal_tol] * 4)
        for s in S:
            s.set_start(start_of(cfg, True))
        res, _ = capi.Space.plan_multi(S, *SEARCH)
        for a, b in zip(single, res):
            _same_plan(a, b)
        for s in S:
            s.close()
    assert len({tuple(g["expansion_log"][:50]) for g in single}) == 3      # the kinds do search differently


@BUILDS
@pytest.mark.parametrize("kind", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("mode", ["host", "device"])
def test_replan_in_two_budgets_equals_one_run(small_cfg, kind, mode, generic, monkeypatch):
    """smplx_replan with a budget of 7 expansions, then with the rest of 150, continues where it stopped: the log, result,
    path and cost of one run of 150 (which may or may not reach the goal: the Euclidean kind does, in fewer)"""
    _need_gpu()
    monkeypatch.setenv("SMPLX_SEARCH", mode)
    cfg = small_cfg
    one = _space(_search_cfg(cfg, kind[1], snap=False), kind[1], generic, batch_states=256)
    two = _space(_search_cfg(cfg, kind[1], snap=False), kind[1], generic, batch_states=256)
    for s in (one, two):
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        s.set_start(start_of(cfg, True))
    K = 150
    a = one.replan(10.0, 10.0, 1.0, True, True, K, K)
    assert a["expansions"] > 7 and a["resumed"] == 0
    first = two.replan(10.0, 10.0, 1.0, True, True, 7, 7)
    assert first["result"] == capi.ARA_TIMED_OUT and first["call_expansions"] == 7 and first["resumed"] == 0
    b = two.replan(10.0, 10.0, 1.0, True, True, K - 7, K - 7)
    assert b["resumed"] == 1 and b["result"] == a["result"] and b["solved"] == a["solved"] and b["expansions"] == a["expansions"]
    assert np.array_equal(a["expansion_log"], b["expansion_log"]) and a["cost"] == b["cost"] and np.array_equal(a["path"], b["path"])
    assert a["satisfied_eps"] == b["satisfied_eps"]
    one.close(); two.close()


def _loop_plan(s, start_id, search):
    """the plain ARA* loop (arastar_loop.py) over smplx_get_succs and smplx_get_goal_heuristic of the space"""
    eps0, fin, delta, _, bounded, mi, mr = search
    return AraStarLoop(s.get_succs, s.goal_heuristic).replan(start_id, 0, eps0, fin, delta, mi if bounded else 0, mr)


def _same_as_loop(g, r):
    assert g["solved"] == r["solved"] and g["expansions"] == r["expansions"]
    assert np.array_equal(g["expansion_log"], r["log"])
    if r["solved"]:
        assert g["cost"] == r["cost"] and np.array_equal(g["path"], r["path"]) and g["satisfied_eps"] == r["satisfied_eps"]


@BUILDS
def test_loop_is_pinned_to_the_oracle_under_the_bfs_kind(small_cfg, generic):
    """First the judge: under the BFS kind the loop's expansion log over smplx_get_succs / smplx_get_goal_heuristic on
    small_cfg equals the oracle's, id for id (tests/test_arastar_loop.py pins it on the oracle's own successors too)."""
    from oracle_binding import Oracle
    _need_gpu()
    cfg = small_cfg
    o = Oracle(cfg)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    o.set_start(cfg.start)
    o.search_params(5.0, 1.0, 1.0, True, True, 1500, 1500)
    e = o.plan()
    s = _space(cfg, capi.H_BFS, generic, batch_states=256)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    r = _loop_plan(s, s.set_start(cfg.start), (5.0, 1.0, 1.0, True, True, 1500, 1500))
    assert r["solved"] == e["ok"] and r["expansions"] == e["expansions"] == 1500
    assert np.array_equal(r["log"], e["expansion_log"]) and r["cost"] == e["cost"] and np.array_equal(r["path"], e["path"])
    assert r["satisfied_eps"] == e["eps"]
    s.close()


LOOP_CASES = [("euclid", EUCLID, "joint", True), ("euclid", EUCLID, "pose", True), ("joint_distance", JOINT, "joint", True),
              ("joint_distance", JOINT, "joint", False)]


@BUILDS
@pytest.mark.parametrize("case", LOOP_CASES, ids=["euclid-joint", "euclid-pose", "joint_distance-joint", "joint_distance-joint-no-snap"])
def test_loop_host_search_and_device_search_agree(small_cfg, case, generic, monkeypatch):
    """For each new kind the loop, the host search and the device search (which did run) give the same expansion log, path,
    cost and satisfied eps, from the NEAR start -- chosen by the loop on the oracle's successors so that the first iteration
    reaches the joint goal (tests/test_arastar_loop.py; checked here for the engine's own successors too).  The Euclidean
    kind also plans to a pose goal with rpy_tol = 0.2.  Under joint distance with the snap the search is one expansion long
    (the snap is active everywhere); the no-snap case gives the order something to decide."""
    _need_gpu()
    name, kind, goal, snap = case
    cfg = small_cfg
    s = _space(_search_cfg(cfg, kind, snap), kind, generic, batch_states=256)
    _set_goal(s, cfg, goal)
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    r = _loop_plan(s, s.set_start(start_of(cfg, True)), SEARCH)
    s.close()
    print(name, goal, "snap" if snap else "no snap", "loop: solved", r["solved"], "expansions", r["expansions"], "cost", r["cost"])
    for mode in ("host", "device"):
        _same_as_loop(_plan(cfg, kind, generic, mode, monkeypatch, goal, near=True, snap=snap), r)
    if goal == "joint" and snap:
        assert r["solved"] == 1 and r["path"][-1] == 0
        assert first_iteration_on_the_oracle(cfg, name, start_of(cfg, True))["solved"] == 1


# ----------------------------------------------------------------------------------------------------------------------
# 10. the plugin mirror
# ----------------------------------------------------------------------------------------------------------------------

@BUILDS
@pytest.mark.parametrize("kind", [("bfs", capi.H_BFS)] + KINDS, ids=["bfs", "euclid", "joint_distance"])
def test_plugin_mirror_plans_with_each_kind(small_cfg, kind, generic, tmp_path, monkeypatch):
    """tests/cpp/heuristic_kinds_driver.cpp wires GpuBfsHeuristic, GpuEuclidDistHeuristic or GpuJointDistHeuristic by a
    command-line word and runs an SBPL-shaped ARA* that knows GetSuccs and GetGoalHeuristic alone: its log, path, cost and
    satisfied eps are the Python loop's and the host search's.  The driver itself fails unless the heuristic classes of the
    other kinds refuse their init and an XYZ_GOAL with an rpy is refused on a Euclidean space (and only there).
    GetFromToHeuristic between two states equals the host call; to the goal it is GetGoalHeuristic."""
    import subprocess
    _need_gpu()
    name, k = kind
    cfg = _search_cfg(small_cfg, k, snap=False)
    near = dataclasses.replace(cfg, start=[float(x) for x in start_of(small_cfg, True)])
    exe = build_driver("heuristic_kinds_driver", tmp_path)
    write_query(near, tmp_path, [SEARCH[0], SEARCH[1], SEARCH[2], SEARCH[5], SEARCH[6]])
    monkeypatch.setenv("SMPLX_SPECIALIZE", "0" if generic else "2")
    out = subprocess.run([exe, str(tmp_path), name], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = {l.split(" ", 1)[0]: l.split(" ", 1)[1] if " " in l else "" for l in out.stdout.decode().splitlines()}
    assert "done" in lines
    assert [int(x) for x in lines["refusals"].split()] == [int(k == j) for j in range(3)]
    monkeypatch.delenv("SMPLX_SPECIALIZE")
    s = _space(cfg, k, generic, batch_states=256)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    r = _loop_plan(s, s.set_start(near.start), SEARCH)
    s.close()
    solved, cost, nexp, plen, secs, eps = lines["result"].split()
    assert int(solved) == r["solved"] and int(nexp) == r["expansions"]
    assert np.array_equal(np.array(lines["log"].split(), dtype=np.int64), r["log"])
    if r["solved"]:
        assert int(cost) == r["cost"] and float(eps) == r["satisfied_eps"]
        assert np.array_equal(np.array(lines["path"].split(), dtype=np.int64), r["path"])
    _same_as_loop(_plan(small_cfg, k, generic, "host", monkeypatch, "joint", near=True, snap=False), r)
    ab, host, a_goal, h_a, start_b = (int(x) for x in lines["fromto"].split())
    assert a_goal == h_a
    if k != capi.H_BFS:
        assert ab == host and ab > 0
    assert start_b == (0 if k != JOINT else start_b) and (k != JOINT or start_b > 0)
    mg, ms = (float(x) for x in lines["metric"].split())
    assert mg == 0.0 and (k == capi.H_BFS or ms == 0.0)


# ----------------------------------------------------------------------------------------------------------------------
# 9. a closed-form space holds and runs no BFS
# ----------------------------------------------------------------------------------------------------------------------

@BUILDS
def test_closed_form_space_has_no_bfs(small_cfg, generic):
    _need_gpu()
    cfg = small_cfg
    for _, kind in KINDS:
        s = _space(cfg, kind, generic)
        assert s.bfs_size() == 0 and s.bfs_levels() == 0
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        assert s.bfs_size() == 0 and s.bfs_levels() == 0
        for call in (lambda: s.bfs_grid(), lambda: s.metric_goal_distance([[0.1, 0.2, 0.3]]), lambda: s.metric_start_distance([[0.1, 0.2, 0.3]])):
            with pytest.raises(capi.SmplxError) as e:
                call()
            assert e.value.code == capi.E_STATE and "closed-form" in str(e.value)
        if kind != EUCLID:
            with pytest.raises(capi.SmplxError) as e:
                s.set_euclid_weights([1, 1, 1, 1])
            assert e.value.code == capi.E_STATE
        s.close()
    b = _space(cfg, capi.H_BFS, generic)
    with pytest.raises(capi.SmplxError) as e:
        b.set_euclid_weights([1, 1, 1, 1])
    assert e.value.code == capi.E_STATE
    b.set_goal_joint(cfg.goal, cfg.goal_tol)
    assert b.bfs_size() == 66 ** 3 and b.bfs_levels() > 0
    xyz = np.array([[0.3, 0.1, 0.4], [0.5, -0.2, 0.6]])
    assert np.array_equal(b.heuristic_metric_goal_distance(xyz), b.metric_goal_distance(xyz))
    b.close()


@BUILDS
def test_set_goals_multi_over_a_mixed_set(small_cfg, generic):
    """smplx_set_goals_joint_multi over spaces of all three kinds: every space ends as its single call leaves it (goal pose,
    h of the start, h of seeded states), and the BFS grids of the BFS spaces are those of a call without the others"""
    _need_gpu()
    cfg = small_cfg
    g = np.array(cfg.goal)
    goals = [g, g + np.array([10, -5, 8, 6, 20, -10, 30]) * scenes.DEG, g, g + np.array([-6, 4, 0, 5, -15, 8, 0]) * scenes.DEG, g]
    kinds = [EUCLID, capi.H_BFS, JOINT, capi.H_BFS, EUCLID]
    Q = scenes.random_states(scenes.ARM7_LIMITS, 64, 3)
    single = [_space(cfg, k, generic) for k in kinds]
    multi = [_space(cfg, k, generic) for k in kinds]
    only_bfs = [_space(cfg, capi.H_BFS, generic) for k in kinds if k == capi.H_BFS]
    for s, a in zip(single, goals):
        s.set_goal_joint(a, cfg.goal_tol)
    capi.Space.set_goals_joint_multi(multi, goals, [cfg.goal_tol] * len(kinds))
    capi.Space.set_goals_joint_multi(only_bfs, [a for a, k in zip(goals, kinds) if k == capi.H_BFS], [cfg.goal_tol] * len(only_bfs))
    for a, b, k in zip(single, multi, kinds):
        assert np.array_equal(a.goal_pose(), b.goal_pose())
        assert np.array_equal(a.heuristic_batch(Q)[0], b.heuristic_batch(Q)[0])
        ia, ib = a.set_start(cfg.start), b.set_start(cfg.start)
        assert ia == ib and a.goal_heuristic(ia) == b.goal_heuristic(ib) and a.goal_heuristic(0) == b.goal_heuristic(0) == 0
        assert a.bfs_size() == b.bfs_size() == (66 ** 3 if k == capi.H_BFS else 0)
    bfs_multi = [s for s, k in zip(multi, kinds) if k == capi.H_BFS]
    for a, b, c in zip([s for s, k in zip(single, kinds) if k == capi.H_BFS], bfs_multi, only_bfs):
        assert np.array_equal(a.bfs_grid(), b.bfs_grid()) and np.array_equal(b.bfs_grid(), c.bfs_grid())
    for s in single + multi + only_bfs:
        s.close()
