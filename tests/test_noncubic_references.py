"""The cases of noncubic_cases.py on the CPU: they meet the conditions they are there for, the oracle equals the plain
numpy references on every one of them (so either may serve as the expected value of tests/test_gpu_noncubic_grids.py),
and they tell the axes apart: the same operations carried out with two extents exchanged give something else.

That last check is what stands in for mutating the kernels' indices; a kernel with wrong indexing is never run."""
import itertools

import numpy as np
import pytest

import noncubic_cases as nc
from oracle_binding import Oracle
from smpl_amd import scenes

PLANNING = range(len(nc.PLANNING_GRIDS))
THIN = range(len(nc.THIN_GRIDS))
ALL = [("planning", i) for i in PLANNING] + [("thin", i) for i in THIN]


def _case(kind, i):
    return nc.planning_case(i) if kind == "planning" else nc.thin_case(i)


@pytest.fixture(scope="module")
def oracles():
    cache = {}

    def get(kind, i):
        if (kind, i) not in cache:
            cache[(kind, i)] = Oracle(_case(kind, i))
        return cache[(kind, i)]
    return get


def _free_goal(cfg):
    """centre of a free cell in the middle of the list of free cells"""
    free = np.argwhere(~nc.plain_walls(cfg.grid, cfg.params.bfs_radius)[1:-1, 1:-1, 1:-1].transpose(2, 1, 0))
    assert free.shape[0] >= 3
    return nc.cell_centre(cfg.grid, free[free.shape[0] // 2])


@pytest.mark.parametrize("i", PLANNING)
def test_planning_grids_meet_their_conditions(i, oracles):
    cfg = nc.planning_case(i)
    n = cfg.grid.dims
    b4, b8 = nc.brick_counts(n)
    assert len(set(n)) == 3 and len(set(b4)) == 3 and len(set(b8)) == 3
    assert all(v % 8 for v in n) and any(v % 4 for v in n)
    o = oracles("planning", i)
    assert o.state_valid(cfg.start)[0] and o.state_valid(cfg.goal)[0]
    valid = sum(o.state_valid(q)[0] for q in nc.bench_states())
    print(f"{cfg.name}: dims {n}, 4-cell bricks {b4}, 8-cell bricks {b8}, valid states {valid} of 1200")
    assert valid >= 500
    # the cell of the field test's single added point is free, and its window has three different extents
    c = nc.corner_edit_cell(n)
    assert cfg.grid.d2[c] > 0
    ext = [min(a + cfg.grid.dmax_int, m - 1) - max(a - cfg.grid.dmax_int, 0) + 1 for a, m in zip(c, n)]
    assert len(set(ext)) == 3 and all(e < 2 * cfg.grid.dmax_int + 1 for e in ext)


@pytest.mark.parametrize("i", THIN)
def test_thin_grids_have_obstacles_free_cells_and_a_short_axis(i):
    cfg = nc.thin_case(i)
    d2 = cfg.grid.d2
    assert (d2 == 0).any() and (d2 > 0).sum() >= 3 and min(cfg.grid.dims) < 4


@pytest.mark.parametrize("kind,i", ALL)
def test_oracle_lookup_equals_plain_lookup(kind, i, oracles):
    cfg = _case(kind, i)
    o = oracles(kind, i)
    P = nc.lookup_points(cfg.grid, 100 + i)
    assert P.shape[0] >= 20000
    c, inside = nc.cells_of(cfg.grid, P)
    n = np.asarray(cfg.grid.dims)
    for a in range(3):       # both sides of both faces of every axis
        assert (c[:, a] == -1).any() and (c[:, a] == 0).any() and (c[:, a] == n[a] - 1).any() and (c[:, a] == n[a]).any()
    assert inside.sum() >= 500 and (~inside).sum() >= 500
    got = np.array([o.grid_sqdist(*p) for p in P])
    assert np.array_equal(got, nc.plain_lookup(cfg.grid, P))
    assert np.array_equal(np.array([o.world_to_grid(*p) for p in P[:2000]]), c[:2000])


@pytest.mark.parametrize("kind,i", ALL)
def test_oracle_bfs_and_metric_distances_equal_the_plain_ones(kind, i, oracles):
    """The config goal (planning grids) or a free cell (thin grids), then a goal on a wall cell, a goal outside the grid and
    the first goal again, on ONE oracle and one PlainBfs: the deque flood, the level flood and the oracle agree."""
    cfg = _case(kind, i)
    o = oracles(kind, i)
    g = cfg.grid
    tol = [0.04] * 3
    first = o.planning_fk(cfg.goal) if kind == "planning" else _free_goal(cfg)
    walls = nc.plain_walls(g, cfg.params.bfs_radius)
    wall_cells = np.argwhere(walls[1:-1, 1:-1, 1:-1].transpose(2, 1, 0))
    on_wall = nc.cell_centre(g, wall_cells[wall_cells.shape[0] // 2])
    a, b = nc.PlainBfs(g, cfg.params.bfs_radius), nc.PlainBfs(g, cfg.params.bfs_radius)
    P = nc.metric_points(g, 200 + i)
    for k, xyz in enumerate([first, on_wall, [50.0, 50.0, 50.0], first]):
        o.set_goal_xyz(list(xyz), tol)
        want = a.run(xyz)
        assert np.array_equal(want, b.run(xyz, nc.level_flood)), k
        got = o.bfs_grid()
        assert got.shape == (g.dims[2] + 2, g.dims[1] + 2, g.dims[0] + 2)
        assert np.array_equal(got, want), k
        assert np.array_equal(np.array([o.metric_goal_distance(*p) for p in P]), nc.plain_metric_goal(g, want, P)), k
        reached = ((want >= 0) & (want < nc.WALL)).sum()
        if k == 2:
            assert reached == 0
        else:
            assert reached >= (1 if k == 1 else 2), k      # (a goal inside a wall may be shut in)
        if k == 1:
            assert (want == 0).sum() == 1 and not a.walls[tuple(np.argwhere(want == 0)[0])]
    if kind == "planning":
        # the oracle has no getMetricStartDistance of its own: its forward kinematics and its worldToGrid, put together as
        # bfs_heuristic.cpp:103-127 does, against the plain formula
        sxyz = o.planning_fk(cfg.start)
        sc = o.world_to_grid(*sxyz).astype(np.int64)
        got = np.array([g.res * float(np.abs(o.world_to_grid(*p).astype(np.int64) - sc).sum()) for p in P])
        assert np.array_equal(got, nc.plain_metric_start(g, sxyz, P))
        assert len(np.unique(got)) > 20


def _exchanged(d2, a, b):
    return np.ascontiguousarray(np.swapaxes(d2, a, b))


@pytest.mark.parametrize("i", PLANNING)
@pytest.mark.parametrize("a,b", list(itertools.combinations(range(3), 2)))
def test_cases_tell_the_axes_apart(i, a, b):
    """What an implementation that exchanged axes a and b in its indexing would compute, without running one: the field
    transposed and the two extents exchanged, the queries left as they are.  The lookup table over every cell and the layer
    outside, and the BFS grid of the config goal (transposed back to the true shape), both differ from the true ones; so do
    the synthetic field of the lookup probe and the brick counts."""
    cfg = nc.planning_case(i)
    g = cfg.grid
    cells = nc.padded_cells(g.dims)
    P = nc.cell_centre(g, cells)
    true_table = nc.plain_lookup(g, P)
    gx = scenes.Grid(g.origin, _exchanged(g.d2, a, b).shape, g.res, g.max_dist, _exchanged(g.d2, a, b))
    assert gx.dims != g.dims
    assert not np.array_equal(nc.plain_lookup(gx, P), true_table)
    goal_xyz = Oracle(cfg).planning_fk(cfg.goal)
    true_bfs = nc.PlainBfs(g, cfg.params.bfs_radius).run(goal_xyz, nc.level_flood)
    other = nc.PlainBfs(gx, cfg.params.bfs_radius).run(goal_xyz, nc.level_flood)
    back = np.swapaxes(other, 2 - a, 2 - b)                   # [z][y][x]: axis a of the grid is axis 2 - a here
    assert back.shape == true_bfs.shape and not np.array_equal(back, true_bfs)
    # the probe's field, as bits per cell
    bits = nc.hash_bits(cells).reshape([n + 2 for n in g.dims])
    sw = cells.copy()
    sw[:, [a, b]] = sw[:, [b, a]]
    assert 0.3 < bits.mean() < 0.7
    assert (nc.hash_bits(sw).reshape(bits.shape) != bits).mean() > 0.2
    b4, b8 = nc.brick_counts(g.dims)
    assert b4[a] != b4[b] and b8[a] != b8[b]


@pytest.mark.parametrize("kind,i", ALL)
def test_probe_robot_sits_where_its_joint_values_say(kind, i):
    """The lookup probe's robot through the oracle: at q = the centre of a cell the sphere is in that cell, and the state is
    valid exactly where the synthetic field's bit is set; outside the grid it never is."""
    base = _case(kind, i).grid
    cfg = nc.probe_case(base.dims, base.origin, base.res, base.max_dist)
    o = Oracle(cfg)
    cells = nc.padded_cells(base.dims)
    rng = np.random.default_rng(5)
    pick = cells[rng.choice(cells.shape[0], size=min(3000, cells.shape[0]), replace=False)]
    Q = nc.cell_centre(cfg.grid, pick)
    inside = np.all((pick >= 0) & (pick < np.asarray(base.dims)), axis=1)
    want = np.where(inside, nc.hash_bits(pick), 0).astype(bool)
    for q, c, w in zip(Q, pick, want):
        pos = o.sphere_positions(q, 1)[0]
        assert np.array_equal(scenes.world_to_grid(base.origin, base.res, pos), c)
        ok, lookups = o.state_valid(q)
        assert ok == w and lookups == 1
    assert want.any() and (~want[inside]).any() and (~inside).any()
