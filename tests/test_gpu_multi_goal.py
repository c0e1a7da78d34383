"""smplx_set_goals_joint_multi / smplx_set_goals_xyz_multi: the goals of many spaces in one call, their BFS runs in one
shared sequence of launches.  The reference is always a fresh space given the same goal through smplx_set_goal_*, and
where stated the oracle or the plain flood of tests/noncubic_cases.py as well.  Every comparison is exact.
"""
import numpy as np
import pytest

import noncubic_cases as nc
from smpl_amd import scenes

pytestmark = pytest.mark.gpu

XYZ_TOL = [0.04] * 3
E_ARG = -1


def _need_gpu():
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


class Scene:
    """one grid handle and one model, and spaces on them"""

    def __init__(self, cfg):
        from smpl_amd import capi
        self.cfg = cfg
        self.grid = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
        self.model = capi.Model(cfg.robot_text)

    def space(self, batch_states=0):
        from smpl_amd import capi
        return capi.Space(self.model, self.grid, self.cfg.mprim, self.cfg.params, batch_states)

    def spaces(self, n, batch_states=0):
        return [self.space(batch_states) for _ in range(n)]


@pytest.fixture(scope="module")
def small(small_cfg):
    _need_gpu()
    return Scene(small_cfg)


def _labelled(grid):
    return int(((grid >= 0) & (grid < nc.WALL)).sum())


def _joint_goals(cfg, n, seed):
    """goals drawn as in test_bfs_grid_over_ten_goals_in_one_space"""
    rng = np.random.default_rng(seed)
    return np.array([np.array(cfg.goal) + rng.uniform(-0.4, 0.4, size=len(cfg.goal)) for _ in range(n)])


def _tols(cfg, n):
    return np.tile(np.asarray(cfg.goal_tol, dtype=np.float64), (n, 1))


def _free_cell(cfg, cell):
    """not a wall of the BFS (bfs_heuristic.cpp:331-353)"""
    g = cfg.grid
    return g.res * np.sqrt(float(g.d2[cell[0], cell[1], cell[2]])) > cfg.params.bfs_radius


# ----------------------------------------------------------------------------------------------------------------------
# 1. twelve joint goals on one grid and model
# ----------------------------------------------------------------------------------------------------------------------

def test_twelve_joint_goals_equal_the_single_calls_and_the_oracle(small):
    from oracle_binding import Oracle
    from smpl_amd import capi
    cfg = small.cfg
    n = 12
    goals = _joint_goals(cfg, n, 17)
    spaces = small.spaces(n)
    capi.Space.set_goals_joint_multi(spaces, goals, _tols(cfg, n))
    Q = scenes.random_states(scenes.ARM7_LIMITS, 200, 4242)
    P = nc.metric_points(cfg.grid, 31, n=96)
    assert P.shape[0] >= 200
    levels = {s.bfs_levels() for s in spaces}
    assert len(levels) == 1 and levels.pop() > 0      # the passes of the shared sequence, the same for every space
    o = Oracle(cfg)
    for k, s in enumerate(spaces):
        ref = small.space()
        ref.set_goal_joint(list(goals[k]), cfg.goal_tol)
        want = ref.bfs_grid()
        assert _labelled(want) > 1000, "the reference flood is not empty"
        assert np.array_equal(s.bfs_grid(), want), k
        assert np.array_equal(s.goal_pose(), ref.goal_pose()), k
        hs, xs = s.heuristic_batch(Q)
        hr, xr = ref.heuristic_batch(Q)
        assert np.array_equal(hs, hr) and np.array_equal(xs, xr), k
        assert np.array_equal(s.metric_goal_distance(P), ref.metric_goal_distance(P)), k
        assert s.goal_heuristic(0) == ref.goal_heuristic(0) == 0, k
        if k % 3 == 0:
            o.set_goal_joint(list(goals[k]), cfg.goal_tol)
            assert np.array_equal(s.bfs_grid(), o.bfs_grid()), f"oracle, goal {k}"


# ----------------------------------------------------------------------------------------------------------------------
# 2. goal placement
# ----------------------------------------------------------------------------------------------------------------------

def test_goal_placement_same_cell_outside_the_grid_and_brick_corners(small):
    from smpl_amd import capi
    cfg = small.cfg
    g = cfg.grid
    corner_cells = [c for c in [(8, 8, 8), (7, 7, 7), (16, 24, 8), (15, 24, 7)] if _free_cell(cfg, c)]
    assert len(corner_cells) >= 3
    fk = small.space()
    fk.set_goal_joint(cfg.goal, cfg.goal_tol)
    home = fk.goal_pose()                                   # an ordinary free place: the config goal's pose
    reach = np.argwhere((fk.bfs_grid() >= 0) & (fk.bfs_grid() < nc.WALL))      # padded [z][y][x] cells the flood reaches
    assert reach.shape[0] > 1000
    near = [nc.cell_centre(g, reach[j][::-1] - 1) for j in (reach.shape[0] // 3, 2 * reach.shape[0] // 3)]
    far = np.array([50.0, 50.0, 50.0])
    pts = [home, home.copy(),                               # two spaces with the same goal cell
           near[0], far, near[1]]                           # one goal outside the grid between two ordinary ones
    pts += [nc.cell_centre(g, c) for c in corner_cells]     # on and beside brick corners
    rng = np.random.default_rng(5)
    while len(pts) < 12:
        pts.append(home + rng.uniform(-0.15, 0.15, size=3))
    pts = np.array(pts)
    spaces = small.spaces(12)
    capi.Space.set_goals_xyz_multi(spaces, pts, np.tile(XYZ_TOL, (12, 1)))
    grids = [s.bfs_grid() for s in spaces]
    for k, s in enumerate(spaces):
        ref = small.space()
        ref.set_goal_xyz(list(pts[k]), XYZ_TOL)
        assert np.array_equal(grids[k], ref.bfs_grid()), k
        assert np.array_equal(s.goal_pose(), pts[k]), k
        assert s.goal_heuristic(0) == ref.goal_heuristic(0), k
    assert np.array_equal(grids[0], grids[1])
    assert _labelled(grids[3]) == 0 and spaces[3].goal_heuristic(0) == 32767      # outside: nothing is labelled
    assert _labelled(grids[2]) > 1000 and _labelled(grids[4]) > 1000              # its neighbours are untouched by it
    for j, c in enumerate(corner_cells):
        assert np.array_equal(grids[5 + j], nc.PlainBfs(g, cfg.params.bfs_radius).run_cell(c, nc.level_flood)), c
        assert grids[5 + j][c[2] + 1, c[1] + 1, c[0] + 1] == 0


# ----------------------------------------------------------------------------------------------------------------------
# 3. tags
# ----------------------------------------------------------------------------------------------------------------------

def test_tags_differ_per_space_and_wrap_inside_multi_calls(small):
    """Every space counts its own BFS runs (tag 1..7, a reset of the records at the wrap): spaces with 0, 1, 3, 6 and 7
    earlier goals share the calls, one is due its reset in the first call, others wrap in the calls that follow."""
    from smpl_amd import capi
    cfg = small.cfg
    earlier = [0, 1, 3, 6, 7]
    n = len(earlier)
    spaces = small.spaces(n)
    refs = small.spaces(n)          # the same history through single calls only
    pre = _joint_goals(cfg, 8, 23)
    for s, r, cnt in zip(spaces, refs, earlier):
        for k in range(cnt):
            s.set_goal_joint(list(pre[k]), cfg.goal_tol)
            r.set_goal_joint(list(pre[k]), cfg.goal_tol)
    for call in range(3):
        goals = _joint_goals(cfg, n, 100 + call)
        capi.Space.set_goals_joint_multi(spaces, goals, _tols(cfg, n))
        for k in range(n):
            refs[k].set_goal_joint(list(goals[k]), cfg.goal_tol)
            fresh = small.space()
            fresh.set_goal_joint(list(goals[k]), cfg.goal_tol)
            want = fresh.bfs_grid()
            assert _labelled(want) > 1000
            assert np.array_equal(spaces[k].bfs_grid(), want), (call, k)
            assert np.array_equal(refs[k].bfs_grid(), want), (call, k)
    # multi -> single on two of the spaces
    last = _joint_goals(cfg, 2, 321)
    for k, j in enumerate([1, 3]):
        spaces[j].set_goal_joint(list(last[k]), cfg.goal_tol)
        fresh = small.space()
        fresh.set_goal_joint(list(last[k]), cfg.goal_tol)
        assert np.array_equal(spaces[j].bfs_grid(), fresh.bfs_grid()), j
        assert np.array_equal(spaces[j].goal_pose(), fresh.goal_pose()), j


# ----------------------------------------------------------------------------------------------------------------------
# 4. different walls on one grid handle
# ----------------------------------------------------------------------------------------------------------------------

def test_spaces_keep_the_walls_they_were_created_with(small_cfg):
    from smpl_amd import capi
    _need_gpu()
    cfg = small_cfg
    g = cfg.grid
    grid = capi.Grid.from_boxes(g.origin, g.dims, g.res, g.max_dist, cfg.boxes)
    model = capi.Model(cfg.robot_text)
    field_a = scenes.Grid(g.origin, g.dims, g.res, g.max_dist, grid.d2())
    a = capi.Space(model, grid, cfg.mprim, cfg.params)
    probe = capi.Space(model, grid, cfg.mprim, cfg.params)
    probe.set_goal_joint(cfg.goal, cfg.goal_tol)
    goal = probe.goal_pose()
    # a slab through the free space beside the goal: the flood has to go round it
    grid.add_boxes([((float(goal[0]) + 0.25, float(goal[1]), float(goal[2])), (0.08, 0.9, 0.9))])
    field_b = scenes.Grid(g.origin, g.dims, g.res, g.max_dist, grid.d2())
    assert not np.array_equal(field_a.d2, field_b.d2)
    b = capi.Space(model, grid, cfg.mprim, cfg.params)
    capi.Space.set_goals_xyz_multi([a, b], np.array([goal, goal]), np.tile(XYZ_TOL, (2, 1)))
    ga, gb = a.bfs_grid(), b.bfs_grid()
    want_a = nc.PlainBfs(field_a, cfg.params.bfs_radius).run(goal, nc.level_flood)
    want_b = nc.PlainBfs(field_b, cfg.params.bfs_radius).run(goal, nc.level_flood)
    assert _labelled(want_a) > 1000 and _labelled(want_b) > 1000
    assert np.array_equal(ga, want_a), "the old walls"
    assert np.array_equal(gb, want_b), "the new walls"
    assert not np.array_equal(ga, gb)


# ----------------------------------------------------------------------------------------------------------------------
# 5. non-cubic and thin grids
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", range(len(nc.PLANNING_GRIDS)))
def test_noncubic_planning_grids(i):
    from smpl_amd import capi
    _need_gpu()
    cfg = nc.planning_case(i)
    g = cfg.grid
    sc = Scene(cfg)
    probe = sc.space()
    probe.set_goal_joint(cfg.goal, cfg.goal_tol)
    corners = nc.last_brick_corner_cells(g.dims)
    # the high corner of the last brick of all three axes, a corner of a last brick along one axis, and the config goal
    cells = [corners[7], corners[8], corners[-1]]
    pts = np.array([nc.cell_centre(g, c) for c in cells] + [probe.goal_pose()])
    spaces = sc.spaces(4)
    capi.Space.set_goals_xyz_multi(spaces, pts, np.tile(XYZ_TOL, (4, 1)))
    spread = 0
    for k, s in enumerate(spaces):
        want = nc.PlainBfs(g, cfg.params.bfs_radius).run(pts[k], nc.level_flood)
        got = s.bfs_grid()
        assert got.shape == (g.dims[2] + 2, g.dims[1] + 2, g.dims[0] + 2)
        assert np.array_equal(got, want), (i, k)
        spread += _labelled(want)
    assert spread > 1000


@pytest.mark.parametrize("i", range(len(nc.THIN_GRIDS)))
def test_thin_grids(i):
    """axes shorter than one brick, one grid of a single layer: two free cells and a wall cell as goals"""
    from smpl_amd import capi
    _need_gpu()
    cfg = nc.thin_case(i)
    g = cfg.grid
    sc = Scene(cfg)
    walls = nc.PlainBfs(g, cfg.params.bfs_radius).walls[1:-1, 1:-1, 1:-1].transpose(2, 1, 0)
    free, wall = np.argwhere(~walls), np.argwhere(walls)
    assert free.shape[0] >= 3 and wall.shape[0] >= 1
    cells = [tuple(free[0]), tuple(free[-1]), tuple(wall[0])]
    pts = np.array([nc.cell_centre(g, c) for c in cells])
    spaces = sc.spaces(3)
    capi.Space.set_goals_xyz_multi(spaces, pts, np.tile(XYZ_TOL, (3, 1)))
    for k, s in enumerate(spaces):
        want = nc.PlainBfs(g, cfg.params.bfs_radius).run_cell(cells[k], nc.level_flood)
        assert np.array_equal(s.bfs_grid(), want), (i, k)
        assert _labelled(want) >= 2


# ----------------------------------------------------------------------------------------------------------------------
# 6. one goal, and more goals than a launch width is tuned for
# ----------------------------------------------------------------------------------------------------------------------

def test_one_goal_equals_the_single_call(small):
    from smpl_amd import capi
    cfg = small.cfg
    s, ref = small.space(), small.space()
    capi.Space.set_goals_joint_multi([s], np.array([cfg.goal]), _tols(cfg, 1))
    ref.set_goal_joint(cfg.goal, cfg.goal_tol)
    assert _labelled(ref.bfs_grid()) > 1000
    assert np.array_equal(s.bfs_grid(), ref.bfs_grid())
    assert np.array_equal(s.goal_pose(), ref.goal_pose())
    assert s.goal_heuristic(0) == ref.goal_heuristic(0)
    assert s.set_start(cfg.start) == ref.set_start(cfg.start)
    a, b = s.plan(5.0, 1.0, 1.0, True, True, 200, 200), ref.plan(5.0, 1.0, 1.0, True, True, 200, 200)
    assert a["cost"] == b["cost"] and np.array_equal(a["expansion_log"], b["expansion_log"])


def test_forty_goals_in_one_call(small):
    from smpl_amd import capi
    cfg = small.cfg
    n = 40
    goals = _joint_goals(cfg, n, 77)
    spaces = small.spaces(n)
    capi.Space.set_goals_joint_multi(spaces, goals, _tols(cfg, n))
    for k in range(0, n, 5):
        ref = small.space()
        ref.set_goal_joint(list(goals[k]), cfg.goal_tol)
        want = ref.bfs_grid()
        assert _labelled(want) > 1000
        assert np.array_equal(spaces[k].bfs_grid(), want), k
        assert np.array_equal(spaces[k].goal_pose(), ref.goal_pose()), k
    # a second call on the same spaces is sized by the first one's queue sizes: the same grids again
    capi.Space.set_goals_joint_multi(spaces, goals[::-1].copy(), _tols(cfg, n))
    for k in range(0, n, 5):
        ref = small.space()
        ref.set_goal_joint(list(goals[k]), cfg.goal_tol)
        assert np.array_equal(spaces[n - 1 - k].bfs_grid(), ref.bfs_grid()), k


# ----------------------------------------------------------------------------------------------------------------------
# 7. refusals that need real spaces
# ----------------------------------------------------------------------------------------------------------------------

def test_mismatched_spaces_and_bad_goals_are_refused_and_nothing_is_touched(small):
    from smpl_amd import capi
    cfg = small.cfg
    other = Scene(nc.planning_case(0))
    a, b = small.space(), other.space()
    ga = np.array(cfg.goal) + 0.1
    a.set_goal_joint(list(ga), cfg.goal_tol)
    b.set_goal_joint(other.cfg.goal, other.cfg.goal_tol)
    before = [a.bfs_grid(), b.bfs_grid(), a.goal_pose(), b.goal_pose()]
    new = _joint_goals(cfg, 2, 9)
    with pytest.raises(capi.SmplxError) as e:
        capi.Space.set_goals_joint_multi([a, b], new, _tols(cfg, 2))
    assert e.value.code == E_ARG and "bricks" in str(e.value)
    with pytest.raises(capi.SmplxError) as e:
        capi.Space.set_goals_xyz_multi([a, b], np.array([before[2], before[3]]) + 0.04, np.tile(XYZ_TOL, (2, 1)))
    assert e.value.code == E_ARG
    # a joint goal that is not finite, in the second row: the first space is not touched either
    c = small.space()
    c.set_goal_joint(cfg.goal, cfg.goal_tol)
    gc = c.bfs_grid()
    bad = new.copy()
    bad[1, 3] = float("nan")
    with pytest.raises(capi.SmplxError) as e:
        capi.Space.set_goals_joint_multi([a, c], bad, _tols(cfg, 2))
    assert e.value.code == E_ARG and "finite" in str(e.value)
    with pytest.raises(capi.SmplxError) as e:
        capi.Space.set_goals_joint_multi([a, a], new, _tols(cfg, 2))
    assert e.value.code == E_ARG and "twice" in str(e.value)
    # both spaces still answer with the goals they had before
    assert np.array_equal(a.bfs_grid(), before[0]) and np.array_equal(b.bfs_grid(), before[1])
    assert np.array_equal(a.goal_pose(), before[2]) and np.array_equal(b.goal_pose(), before[3])
    assert np.array_equal(c.bfs_grid(), gc)
    Q = scenes.random_states(scenes.ARM7_LIMITS, 50, 3)
    ref = small.space()
    ref.set_goal_joint(list(ga), cfg.goal_tol)
    assert np.array_equal(a.heuristic_batch(Q)[0], ref.heuristic_batch(Q)[0])
    assert a.set_start(cfg.start) == ref.set_start(cfg.start)
    ra, rr = a.plan(5.0, 1.0, 1.0, True, True, 100, 100), ref.plan(5.0, 1.0, 1.0, True, True, 100, 100)
    assert np.array_equal(ra["expansion_log"], rr["expansion_log"])


# ----------------------------------------------------------------------------------------------------------------------
# 8. search after it
# ----------------------------------------------------------------------------------------------------------------------

def _eight_queries(small):
    """8 queries of the config-4 list if its first candidates are valid in the small scene, else 8 pairs drawn there"""
    probe = small.space()
    cs, cg = scenes.config4_candidates()
    ok = (probe.state_valid_batch(cs)[0] != 0) & (probe.state_valid_batch(cg)[0] != 0)
    if int(ok.sum()) >= 8:
        idx = np.nonzero(ok)[0][:8]
        return cs[idx], cg[idx]
    Q = scenes.random_states(scenes.ARM7_LIMITS, 400, 2024)
    Q = Q[probe.state_valid_batch(Q)[0] != 0]
    assert Q.shape[0] >= 16
    return Q[:8], Q[8:16]


def test_plan_multi_after_multi_goals_equals_plan_multi_after_single_goals(small):
    from smpl_amd import capi
    cfg = small.cfg
    S, G = _eight_queries(small)
    nb = 300

    def run(multi):
        spaces = small.spaces(8, 1024)
        if multi:
            capi.Space.set_goals_joint_multi(spaces, G, _tols(cfg, 8))
        else:
            for sp, b in zip(spaces, G):
                sp.set_goal_joint(list(b), cfg.goal_tol)
        ids = [sp.set_start(list(a)) for sp, a in zip(spaces, S)]
        out, _ = capi.Space.plan_multi(spaces, 5.0, 1.0, 1.0, True, True, nb, nb)
        return ids, out

    ids_m, got = run(True)
    ids_s, want = run(False)
    assert ids_m == ids_s
    for q in range(8):
        for f in ["solved", "cost", "expansions"]:
            assert got[q][f] == want[q][f], (q, f)
        assert np.array_equal(got[q]["expansion_log"], want[q]["expansion_log"]), q
        assert np.array_equal(got[q]["path"], want[q]["path"]), q
    assert sum(r["expansions"] for r in want) > 8
