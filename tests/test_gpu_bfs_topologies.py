"""The BFS brick sweep (csrc/bfs_kernels.h) and its host drivers (csrc/bfs_host.h) on the fields of tests/bfs_cases.py:
chains that join bricks through one corner slot or one edge copy, plates pierced by one hole, two routes of which the
longer labels a tail first, serpentine corridors that re-enter their bricks dozens of times -- one for more passes than the
drivers' history holds -- and random tangles.  tests/test_bfs_cases.py asserts on the CPU that each field does what it is
named for and that the plain floods used here agree with each other and with the oracle.

The expected value is always noncubic_cases.PlainBfs on the whole padded grid; every comparison is exact.
"""
import time

import numpy as np
import pytest

import bfs_cases as bc
import noncubic_cases as nc
from smpl_amd import scenes

pytestmark = pytest.mark.gpu

XYZ_TOL = [0.04] * 3


def _need_gpu():
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


class Scene:
    """one grid handle of a case's field and the probe robot's model, and spaces on them"""

    def __init__(self, case):
        from smpl_amd import capi
        self.case, self.cfg = case, case.cfg
        g = self.cfg.grid
        self.grid = capi.Grid(g.origin, g.dims, g.res, g.max_dist, g.d2)
        self.model = capi.Model(self.cfg.robot_text)

    def space(self):
        from smpl_amd import capi
        return capi.Space(self.model, self.grid, self.cfg.mprim, self.cfg.params)


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {bad.shape[0]} cells differ, the first [z y x] {bad[:6].tolist()}: "
                           f"got {[int(got[tuple(b)]) for b in bad[:6]]}, want {[int(want[tuple(b)]) for b in bad[:6]]}")


def _bfs_both(s, plain, cfg, goal, what, flood=nc.level_flood):
    xyz = bc.goal_xyz(cfg, goal)
    s.set_goal_xyz(list(xyz), XYZ_TOL)
    want = plain.run(xyz, flood)
    _same(s.bfs_grid(), want, what)
    return want


# ----------------------------------------------------------------------------------------------------------------------
# 1. small fields: the grid, the metric distance and the heuristic at every cell
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", bc.SMALL_NAMES)
def test_small_field_grid_metric_distance_and_heuristic(name):
    """Every goal of the case in order on ONE space.  The heuristic kernel reads the same records through bfs_dist: the probe
    robot is put at the centre of every cell, and the oracle gives the expected value."""
    from oracle_binding import Oracle
    _need_gpu()
    case = bc.small_case(name)
    cfg, g = case.cfg, case.cfg.grid
    s = Scene(case).space()
    plain = bc.plain_bfs(cfg)
    o = Oracle(cfg)
    cells = np.argwhere(np.ones(g.dims, bool))
    Q = nc.cell_centre(g, cells)
    P = nc.metric_points(g, 900)
    for k, goal in enumerate(case.goals):
        want = _bfs_both(s, plain, cfg, goal, f"{name}, goal {k} {goal}")
        assert bc.labelled(want).sum() >= 1
        assert np.array_equal(s.metric_goal_distance(P), nc.plain_metric_goal(g, want, P)), (name, k)
        o.set_goal_xyz(list(bc.goal_xyz(cfg, goal)), XYZ_TOL)
        h, xyz = s.heuristic_batch(Q)
        assert np.array_equal(scenes.world_to_grid(g.origin, g.res, xyz), cells), (name, k)       # the probe is where q says
        want_h = np.array([o.heuristic_q(q) for q in Q], dtype=np.int32)
        bad = np.nonzero(h != want_h)[0]
        assert bad.size == 0, f"{name}, goal {k}: the heuristic differs at {bad.size} cells, the first {cells[bad[:6]].tolist()}"
        assert len(np.unique(h)) >= 3


# ----------------------------------------------------------------------------------------------------------------------
# 2. goal sequences on one space: the host driver's plan
# ----------------------------------------------------------------------------------------------------------------------

def test_goal_sequence_swings_the_plan_between_one_brick_and_hundreds():
    """Serpentine end (more than a hundred passes of a brick or two), hall centre (a few wide passes under a plan of one-brick
    passes), serpentine middle (outlives the short plan: the chunks past it), hall corner, outside the grid, the hall
    again, and on until the tag has wrapped.  A single-goal launch is never narrower than 1024 blocks or the grid's 432
    bricks, so no block takes a second brick here: that is test_hall_goals_planned_by_serpentine_runs_stride_over_bricks."""
    _need_gpu()
    case = bc.hall_case()
    cfg = case.cfg
    s = Scene(case).space()
    plain = bc.plain_bfs(cfg)
    assert len(case.goals) >= 9
    levels, farthest = [], []
    for k, goal in enumerate(case.goals):
        want = _bfs_both(s, plain, cfg, goal, f"goal {k} {goal}")
        levels.append(s.bfs_levels())
        farthest.append(int(want.max(where=bc.labelled(want), initial=0)))
        if goal is bc.OUTSIDE:
            assert not bc.labelled(want).any() and levels[-1] == 0
    print(f"serpentine beside a hall: passes per goal {levels}")
    crossings = bc.brick_crossings(case.path)
    assert levels[0] >= crossings - bc.brick_layer_changes(case.path)   # a value crosses one brick face per visit
    # (on a space with a plan bfs_levels() counts the passes enqueued, the plan's and two more at the least, not the passes
    # that found a brick: that the hall's runs need a dozen passes and the serpentine's over a hundred is asserted from the
    # pass model in tests/test_bfs_cases.py)
    assert all(n > 0 for n, goal in zip(levels, case.goals) if goal is not bc.OUTSIDE)
    # The serpentine-middle run outlived the plan the hall-centre run left it.  A run has nothing queued after pass D + 2, D
    # its greatest hop count (csrc/bfs_host.h bfs_pass_bound), so that plan has at most D + 2 passes and the first chunk at
    # most D + 4: more passes than that were enqueued because a look at the counters found bricks queued past the plan.
    assert levels[2] > farthest[1] + 4
    assert levels[9] > farthest[8] + 4                                  # and again after the pocket's run of one brick


# ----------------------------------------------------------------------------------------------------------------------
# 3. the same field through set_goals_xyz_multi
# ----------------------------------------------------------------------------------------------------------------------

def test_mixed_goals_in_shared_launches_equal_single_calls_and_the_plain_flood():
    """Five spaces on one grid with 0, 1, 3, 6 and 7 earlier goals (tags 1..7, a reset of the records at the wrap); one call
    with a goal in the serpentine, the hall, a pocket, on a wall cell and outside the grid, then a second with the roles
    rotated.  Each space equals its own PlainBfs and a twin that took the same history through single calls."""
    from smpl_amd import capi
    _need_gpu()
    case = bc.hall_case()
    cfg = case.cfg
    sc = Scene(case)
    earlier = [0, 1, 3, 6, 7]
    n = len(earlier)
    spaces, twins = [sc.space() for _ in range(n)], [sc.space() for _ in range(n)]
    plains = [bc.plain_bfs(cfg) for _ in range(n)]
    centre, corner = case.note["centre"], case.note["corner"]
    pre = [centre, case.path[-1], corner, (bc.HALL_X0, 0, 0), case.path[0], (bc.HALL_X0 + 5, 30, 60), case.path[len(case.path) // 2]]
    for s, t, p, cnt in zip(spaces, twins, plains, earlier):
        for k in range(cnt):
            xyz = bc.goal_xyz(cfg, pre[k])
            s.set_goal_xyz(list(xyz), XYZ_TOL)
            t.set_goal_xyz(list(xyz), XYZ_TOL)
            p.run(xyz, nc.level_flood)
    roles = [case.path[len(case.path) // 4], centre, case.note["pocket"], case.note["wall"], bc.OUTSIDE]
    for call in range(2):
        goals = roles[2 * call:] + roles[:2 * call]
        pts = np.array([bc.goal_xyz(cfg, c) for c in goals])
        capi.Space.set_goals_xyz_multi(spaces, pts, np.tile(XYZ_TOL, (n, 1)))
        levels = {s.bfs_levels() for s in spaces}
        # one shared sequence, as long as the serpentine's run: from a quarter of the corridor, three quarters of it are ahead
        assert len(levels) == 1 and levels.pop() > (bc.brick_crossings(case.path) - bc.brick_layer_changes(case.path)) // 2
        for k in range(n):
            twins[k].set_goal_xyz(list(pts[k]), XYZ_TOL)
            want = plains[k].run(pts[k], nc.level_flood)
            got = spaces[k].bfs_grid()
            _same(got, want, f"call {call}, space {k}, goal {goals[k]}")
            _same(twins[k].bfs_grid(), got, f"call {call}, twin of space {k}")
            if goals[k] is bc.OUTSIDE:
                assert not bc.labelled(got).any()
            else:
                assert got[goals[k][2] + 1, goals[k][1] + 1, goals[k][0] + 1] == 0
    wall = case.note["wall"]
    assert all(not p.walls[wall[2] + 1, wall[1] + 1, wall[0] + 1] for p in (plains[3], plains[1]))     # opened where it was a goal
    assert plains[0].walls[wall[2] + 1, wall[1] + 1, wall[0] + 1]


def test_hall_goals_planned_by_serpentine_runs_stride_over_bricks():
    """The stride loop of bfs_wave_pass: every space's last run was a serpentine goal, so the shared call's plan is a brick
    or two per pass and each goal's row of a launch is 64 blocks wide; the hall goals' fronts reach 100 to 200 bricks
    (asserted from the pass model and the width rule in tests/test_bfs_cases.py), so blocks take a second, third and
    fourth brick.  A second call with the goals rotated is planned by the first one's wide passes."""
    from smpl_amd import capi
    _need_gpu()
    case = bc.hall_case()
    cfg = case.cfg
    sc = Scene(case)
    earlier, goals = bc.stride_earlier(case), bc.stride_goals(case)
    n = len(goals)
    spaces = [sc.space() for _ in range(n)]
    plains = [bc.plain_bfs(cfg) for _ in range(n)]
    for s, p, c in zip(spaces, plains, earlier):
        _bfs_both(s, p, cfg, c, f"earlier goal {c}")
    for call in range(2):
        order = goals[call:] + goals[:call]
        pts = np.array([bc.goal_xyz(cfg, c) for c in order])
        capi.Space.set_goals_xyz_multi(spaces, pts, np.tile(XYZ_TOL, (n, 1)))
        assert len({s.bfs_levels() for s in spaces}) == 1
        for k in range(n):
            _same(spaces[k].bfs_grid(), plains[k].run(pts[k], nc.level_flood), f"call {call}, space {k}, goal {order[k]}")


# ----------------------------------------------------------------------------------------------------------------------
# 4. the long serpentine: more passes than the history holds
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def long_reference():
    """the deque floods of the long serpentine's two goals, computed once and left unchanged"""
    case = bc.long_serpentine_case()
    grids = [bc.plain_bfs(case.cfg).run_cell(goal) for goal in case.goals]
    for g in grids:
        g.setflags(write=False)
    return case, grids


def test_long_serpentine_single_goal_runs_past_the_history(long_reference):
    """40 799 cells in one corridor through 300 bricks: the first run has no plan and goes in chunks of 4 passes; the second,
    on the same space, is planned by a full history and still has passes to go when the plan ends."""
    _need_gpu()
    case, wants = long_reference
    cfg = case.cfg
    s = Scene(case).space()
    crossings, layer_changes = bc.brick_crossings(case.path), bc.brick_layer_changes(case.path)
    levels, seconds = [], []
    for k, goal in enumerate(case.goals):
        t0 = time.perf_counter()
        s.set_goal_xyz(list(bc.goal_xyz(cfg, goal)), XYZ_TOL)
        seconds.append(time.perf_counter() - t0)
        levels.append(s.bfs_levels())
        _same(s.bfs_grid(), wants[k], f"goal {k} {goal}")
    print(f"long serpentine: {crossings} crossings ({layer_changes} between layers of bricks), passes {levels}, "
          f"set_goal_xyz {['%.3f s' % t for t in seconds]}")
    assert levels[0] > bc.HISTORY and levels[1] > bc.HISTORY
    assert levels[0] >= crossings - layer_changes


def test_long_serpentine_in_shared_launches(long_reference):
    """both goals in one call on two fresh spaces, then exchanged: the second call is planned by two full histories"""
    from smpl_amd import capi
    _need_gpu()
    case, wants = long_reference
    cfg = case.cfg
    sc = Scene(case)
    spaces = [sc.space(), sc.space()]
    pts = np.array([bc.goal_xyz(cfg, c) for c in case.goals])
    for call in range(2):
        order = [0, 1] if call == 0 else [1, 0]
        t0 = time.perf_counter()
        capi.Space.set_goals_xyz_multi(spaces, pts[order], np.tile(XYZ_TOL, (2, 1)))
        dt = time.perf_counter() - t0
        levels = [s.bfs_levels() for s in spaces]
        print(f"long serpentine, two goals in one call ({call}): passes {levels}, {dt:.3f} s")
        assert levels[0] == levels[1] > bc.HISTORY
        for k in range(2):
            _same(spaces[k].bfs_grid(), wants[order[k]], f"call {call}, space {k}")
