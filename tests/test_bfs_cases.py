"""The fields of bfs_cases.py on the CPU: the plain floods agree with each other and with the oracle on every one of them
(so either may serve as the expected value of tests/test_gpu_bfs_topologies.py), and every field does what it is named for
-- the certificates are asserted here, so that a case cannot quietly stop exercising its part of the brick sweep."""
import numpy as np
import pytest

import bfs_cases as bc
import noncubic_cases as nc
from oracle_binding import Oracle

TOL = [0.04] * 3


def _floods_agree(case, oracle=True):
    """every goal of the case in order on ONE PlainBfs per flood and one oracle; returns the grids"""
    cfg = case.cfg
    a, b = bc.plain_bfs(cfg), bc.plain_bfs(cfg)
    o = Oracle(cfg) if oracle else None
    out = []
    for k, goal in enumerate(case.goals):
        xyz = bc.goal_xyz(cfg, goal)
        want = a.run(xyz)
        assert np.array_equal(want, b.run(xyz, nc.level_flood)), (case.name, k)
        if goal is not bc.OUTSIDE:
            assert want[goal[2] + 1, goal[1] + 1, goal[0] + 1] == 0, (case.name, k)       # the centre of a cell is in that cell
        if o is not None:
            o.set_goal_xyz(list(xyz), TOL)
            assert np.array_equal(o.bfs_grid(), want), (case.name, k)
        out.append(want)
    return out


def _model_equals_flood(case, goal):
    grid, passes, lowered, visits, _ = bc.pass_model(case.free, goal)
    assert np.array_equal(grid, bc.cell_grid(case.free, goal)), (case.name, goal)
    return passes, lowered, visits


@pytest.mark.parametrize("name", bc.SMALL_NAMES)
def test_small_fields_floods_oracle_and_pass_model_agree(name):
    case = bc.small_case(name)
    grids = _floods_agree(case)
    assert all(bc.labelled(g).sum() >= 1 for g in grids)
    for goal in case.goals[:2]:
        _model_equals_flood(case, goal)


def test_corner_chains_join_bricks_through_one_corner_slot_each_way():
    """Every brick the chain leaves, it leaves across a corner (all three brick indices change), nothing else is free, and
    the two goals of the four chains send values through all eight corner directions."""
    directions = set()
    for case in bc.corner_chains():
        assert case.dims == bc.SMALL_DIMS and all(n % 8 == 3 for n in case.dims)
        assert len(case.path) == bc.CHAIN_CELLS and case.free.sum() == bc.CHAIN_CELLS
        steps = bc.brick_steps(case.path)
        assert len(steps) >= 2 and all(abs(s[0]) == abs(s[1]) == abs(s[2]) == 1 for _, s in steps)
        for _, s in steps:
            directions.add(bc.corner_direction(s))                              # goal at the chain's first cell
            directions.add(bc.corner_direction(tuple(-v for v in s)))           # goal at its last cell
        for goal, far in ((case.path[0], case.path[-1]), (case.path[-1], case.path[0])):
            g = bc.cell_grid(case.free, goal)
            assert g[far[2] + 1, far[1] + 1, far[0] + 1] == bc.CHAIN_CELLS - 1 and bc.labelled(g).sum() == bc.CHAIN_CELLS
    assert directions == set(range(8))
    # a chain on the main diagonal starts exactly at a grid corner; the others as near one as the brick phase allows
    assert bc.corner_chains()[0].path[0] == (0, 0, 0)


def test_edge_chains_join_bricks_through_one_edge_each_way():
    """Two brick indices change on every brick change, the third coordinate stays where it was put: inside a brick (3) or on
    either boundary layer of a brick face (7, 8).  All twelve edge directions are crossed, each at all three places."""
    seen = set()
    for case in bc.edge_chains():
        d, fixed = case.note["d"], case.note["fixed"]
        still = d.index(0)
        assert len(case.path) == bc.CHAIN_CELLS and case.free.sum() == bc.CHAIN_CELLS
        assert all(c[still] == fixed for c in case.path)
        steps = bc.brick_steps(case.path)
        assert len(steps) >= 2
        for _, s in steps:
            assert s[still] == 0 and sorted(abs(v) for v in s) == [0, 1, 1]
            seen.add((s, fixed))
            seen.add((tuple(-v for v in s), fixed))
        g = bc.cell_grid(case.free, case.path[0])
        far = case.path[-1]
        assert g[far[2] + 1, far[1] + 1, far[0] + 1] == bc.CHAIN_CELLS - 1
    assert len(seen) == 12 * len(bc.EDGE_THIRD)
    assert {f % 8 for f in bc.EDGE_THIRD} == {3, 7, 0}


def test_pierced_plates_have_one_hole_and_both_sides_flooded_through_it():
    cases = bc.plate_cases()
    assert len(cases) == 3 * 8
    for case in cases:
        axis, hole = case.note["axis"], case.note["hole"]
        plane = np.take(case.free, bc.BRICK, axis=axis)
        assert plane.sum() == 1 and case.free[hole] and hole[axis] == bc.BRICK
        assert case.free.sum() == case.free.size - plane.size + 1
        low, high = case.goals
        assert low[axis] < bc.BRICK < high[axis]
        g = bc.cell_grid(case.free, low)
        assert bc.labelled(g).sum() == case.free.sum()                  # the far side is reached, through the hole alone
        h = g[hole[2] + 1, hole[1] + 1, hole[0] + 1]
        assert g[high[2] + 1, high[1] + 1, high[0] + 1] > h > 0
    # the holes sit in a brick's interior, on the faces, edges and corners of bricks, and in the last, partial bricks
    for axis in range(3):
        holes = bc.plate_holes(bc.SMALL_DIMS, axis)
        assert {(0, 0), (7, 7), (7, 8), (8, 8), (3, 4)} <= set(holes)
        nu, nv = [bc.SMALL_DIMS[a] for a in range(3) if a != axis]
        assert (nu - 1, nv - 1) in holes and (nu - 1, 0) in holes and (0, nv - 1) in holes


def test_two_routes_produce_label_correction():
    case = bc.two_routes_case()
    assert case.dims == bc.TWO_ROUTES_DIMS
    slow, fast, tail = case.note["slow"], case.note["fast"], case.note["tail"]
    junction = slow[-1]
    assert all(bc.brick_of(a)[0] != bc.brick_of(b)[0] for a, b in zip(slow, slow[1:]))     # every hop of S crosses x = 7|8
    assert len({bc.brick_of(c)[0] for c in fast}) == 1                                      # F stays in one brick column
    assert len(tail) == bc.TWO_ROUTES_TAIL and len({bc.brick_of(c)[0] for c in tail}) == 3
    only_fast = case.free.copy()
    for c in slow[1:-1]:
        only_fast[c] = False
    via_slow = bc.cell_grid(case.free, slow[0])[junction[2] + 1, junction[1] + 1, junction[0] + 1]
    via_fast = bc.cell_grid(only_fast, slow[0])[junction[2] + 1, junction[1] + 1, junction[0] + 1]
    assert via_slow == len(slow) - 1 and via_slow < via_fast < nc.WALL
    passes, lowered, visits = _model_equals_flood(case, slow[0])
    print(f"two routes: S {via_slow} hops, F {via_fast} hops, {passes} passes, {lowered} cells lowered after their first label")
    assert lowered > 0
    assert max(visits.values()) > 10
    _model_equals_flood(case, tail[-1])


def test_short_serpentine_reenters_its_bricks():
    case = bc.short_serpentine_case()
    assert case.dims == bc.SHORT_SERPENTINE_DIMS and case.free.sum() == len(case.path) == len(set(case.path))
    crossings = bc.brick_crossings(case.path)
    passes, lowered, visits = _model_equals_flood(case, case.goals[0])
    print(f"short serpentine: {len(case.path)} cells, {crossings} crossings, {passes} passes, most visits of a brick {max(visits.values())}")
    assert max(visits.values()) > 10
    assert passes >= crossings                                          # a value crosses one brick face per visit
    g = bc.cell_grid(case.free, case.goals[0])
    assert bc.labelled(g).sum() == len(case.path)
    for goal in case.goals[1:]:
        _model_equals_flood(case, goal)


def test_long_serpentine_outlasts_the_history_and_the_old_guard():
    """Too long for the pass model: the crossing count stands for the passes.  A brick visit writes only its own cells, so a
    value crosses one brick face per visit and the corridor needs a pass per crossing; the crossings on which the corridor
    changes its layer of bricks along z are left out, for the passes in which both bricks of a pair are queued."""
    case = bc.long_serpentine_case()
    nx, ny, nz = case.dims
    assert case.dims == bc.LONG_SERPENTINE_DIMS
    layers, rows = nz // 2, ny // 2
    assert len(case.path) == len(set(case.path)) == case.free.sum() == layers * (rows * nx + rows - 1) + layers - 1
    crossings, layer_changes, nbricks = bc.brick_crossings(case.path), bc.brick_layer_changes(case.path), bc.n_bricks(case.dims)
    print(f"long serpentine: {len(case.path)} cells, {nbricks} bricks, {crossings} crossings, {layer_changes} of them between layers of bricks")
    assert crossings == layers * rows + nz // 8 - 1 and layer_changes == nz // 8 - 1
    assert crossings - layer_changes > bc.HISTORY
    assert crossings - layer_changes > 4 * nbricks + 1024               # the bound the host driver had: a legitimate field beat it
    for goal in case.goals:
        g = bc.plain_bfs(case.cfg).run_cell(goal)                       # deque flood
        assert bc.labelled(g).sum() == len(case.path)
        # every turn between two rows is cut by one diagonal step on either side of the joining cell
        assert g.max(where=bc.labelled(g), initial=0) == len(case.path) - 1 - 2 * (layers * rows - 1)


def test_serpentine_beside_a_hall_is_sealed_and_its_goals_are_what_they_say():
    case = bc.hall_case()
    assert case.dims == bc.HALL_DIMS and len(case.goals) >= 9
    grids = _floods_agree(case, oracle=False)
    n_path, n_hall = len(case.path), int(case.free[bc.HALL_X0:].sum())
    assert n_hall == (bc.HALL_DIMS[0] - bc.HALL_X0) * bc.HALL_DIMS[1] * bc.HALL_DIMS[2]
    assert case.free[16:bc.HALL_X0].sum() == 1                          # only the pocket: the regions are sealed
    pocket, wall = case.note["pocket"], case.note["wall"]
    assert case.free[pocket] and not case.free[wall]
    sizes = [int(bc.labelled(g).sum()) for g in grids]
    hall_goals = sum(1 for s in sizes if s >= n_hall)
    for goal, s in zip(case.goals, sizes):
        if goal is bc.OUTSIDE:
            assert s == 0
        elif goal == pocket:
            assert s == 1
        elif goal in case.path:
            assert s == n_path
        else:
            assert s in (n_hall, n_hall + 1)                            # (+ the wall cell, once it has been a goal)
    assert hall_goals >= 4 and sizes.count(n_path) >= 4
    assert case.goals[0] == case.path[-1] and case.goals[1] == case.note["centre"] and case.goals[2] == case.path[len(case.path) // 2]
    assert case.goals[3] == case.note["corner"] and case.goals[4] is bc.OUTSIDE and sizes[5] == n_hall
    # the plan swings: the serpentine's runs take more than a hundred passes of a brick or two, the hall's a dozen wide ones
    crossings = bc.brick_crossings(case.path)
    _, serpentine_passes, _, visits, _ = bc.pass_model(case.free, case.goals[0])
    _, hall_passes, _, hall_visits, _ = bc.pass_model(case.free, case.goals[1])
    _, middle_passes, _, _, _ = bc.pass_model(case.free, case.goals[2])
    print(f"serpentine beside a hall: {crossings} crossings, {serpentine_passes} passes from the serpentine's end, {middle_passes} from "
          f"its middle, {hall_passes} from the hall's centre over {len(hall_visits)} bricks")
    assert serpentine_passes >= crossings > 100
    assert hall_passes + 2 < middle_passes < serpentine_passes         # the middle's run outlives the plan the hall's run leaves
    assert hall_passes < 20 and len(hall_visits) > 200


@pytest.mark.parametrize("fraction", bc.SPARSE_FRACTIONS)
def test_sparse_random_goals_meet_their_conditions(fraction):
    case = bc.sparse_case(fraction)
    assert case.dims == bc.SPARSE_DIMS
    first, pocket, wall, again = case.goals
    assert again == first and case.free[first] and case.free[pocket] and not case.free[wall]
    n_free = int(case.free.sum())
    assert abs(n_free / case.free.size - fraction) < 0.01
    a = bc.plain_bfs(case.cfg)
    grids = [a.run_cell(g, nc.level_flood) for g in case.goals]
    reach = [int(bc.labelled(g).sum()) for g in grids]
    print(f"{case.name}: {n_free} free cells, the goals reach {reach}")
    assert 2 * reach[0] >= n_free                                       # reaches at least half the free cells
    assert 1 <= reach[1] <= 3                                           # a component of at most 3 cells
    assert not a.walls[wall[2] + 1, wall[1] + 1, wall[0] + 1]           # the former wall stays free ...
    assert reach[3] >= reach[0] + 1 and grids[3][wall[2] + 1, wall[1] + 1, wall[0] + 1] > 0      # ... and the first flood now enters it
    if fraction == 0.14:
        assert (reach[0], n_free) == (5723, 6522)                       # the tangle of diagonal contacts of seed 5
        _, lowered, _ = _model_equals_flood(case, first)
        assert lowered > 0


def test_a_hall_goal_planned_by_serpentine_runs_has_more_bricks_queued_than_blocks():
    """The certificate of the stride loop (bfs_wave_pass: `for (it = block; it < n; it += nblocks)`).  When the last run of
    every space of a shared call was a serpentine goal, the plan is a brick or two per pass and a goal's row of a launch is
    64 blocks wide; a hall goal in that call has passes in which more bricks IMPROVE than that -- and a brick that improves
    was queued -- so blocks take a second brick.  The plan is bounded from above by the model's queue sizes, which hold all
    26 neighbours of a changed brick where the kernel queues only those that can improve."""
    case = bc.hall_case()
    nbricks = bc.n_bricks(case.dims)
    earlier, goals = bc.stride_earlier(case), bc.stride_goals(case)
    assert len(earlier) == len(goals) and all(c in case.path for c in earlier)
    traces = [bc.pass_model(case.free, c)[4] for c in earlier]
    plan = [max(t[p][0] if p < len(t) else 0 for t in traces) for p in range(max(len(t) for t in traces))]
    assert 2 * max(plan) <= bc.MULTI_WIDTH_FLOOR < nbricks and len(plan) > 100
    for goal in goals[:2]:
        sizes = bc.pass_model(case.free, goal)[4]
        assert len(sizes) < len(plan)                                   # the whole hall run lies inside the plan
        width = [bc.multi_launch_width(plan, p, nbricks) for p in range(len(sizes))]
        assert set(width) == {bc.MULTI_WIDTH_FLOOR}
        over = [improved for (_, improved), w in zip(sizes, width) if improved > w]
        print(f"hall goal {goal}: bricks improved per pass {[i for _, i in sizes]}, {width[0]} blocks: {len(over)} passes stride")
        assert len(over) >= 2
