"""Every grid-indexed kernel on grids whose three extents differ (tests/noncubic_cases.py), against plain numpy references
and the oracle.  On the cubes of the other GPU tests an exchange of two per-axis extents anywhere in grid_d2, the BFS
bricks (z-major, the opposite order from the distance bricks), the export, the packer or the edit window goes unseen;
tests/test_noncubic_references.py shows that on these grids it does not.  Everything is integer or fp64 work in a fixed
order: every comparison is exact.
"""
import numpy as np
import pytest

import noncubic_cases as nc
from smpl_amd import scenes

pytestmark = pytest.mark.gpu

PLANNING = range(len(nc.PLANNING_GRIDS))
THIN = range(len(nc.THIN_GRIDS))
ALL = [("planning", i) for i in PLANNING] + [("thin", i) for i in THIN]
B_MAIN, GOAL_ROW, START_ROW = 300, 3, 5
SEARCH = (5.0, 1.0, 1.0, True, True, 3000, 3000)      # eps0, eps_final, eps_delta, improve, bounded, max_init, max_rep
XYZ_TOL = [0.04] * 3


def _need_gpu():
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")


def _case(kind, i):
    return nc.planning_case(i) if kind == "planning" else nc.thin_case(i)


@pytest.fixture(scope="module")
def oracles():
    """one oracle per planning grid (chain order: the kernels walk the sphere trees link by link)"""
    from oracle_binding import Oracle
    cache = {}

    def get(i):
        if i not in cache:
            cache[i] = Oracle(nc.planning_case(i))
            cache[i].set_order(chain=True)
        return cache[i]
    return get


# ----------------------------------------------------------------------------------------------------------------------
# 1. lookup: grid_d2 at every cell
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,i", ALL)
def test_lookup_probe_reads_every_cell(kind, i):
    """A sphere on three prismatic joints along x, y, z is put at the centre of every cell and of the layer outside every
    face of a field whose values are an asymmetric hash of (x, y, z): its validity is the hash bit, 0 outside.  Nothing
    here goes through the exporter, so a packer and an exporter that are wrong in the same way cannot hide each other;
    Grid.d2() is then held to the input as well."""
    from smpl_amd import capi
    _need_gpu()
    base = _case(kind, i).grid
    cfg = nc.probe_case(base.dims, base.origin, base.res, base.max_dist)
    grid = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    s = capi.Space(capi.Model(cfg.robot_text), grid, cfg.mprim, cfg.params)
    cells = nc.padded_cells(base.dims)
    Q = nc.cell_centre(cfg.grid, cells)
    pos = s.sphere_positions(Q)
    assert pos.shape == (Q.shape[0], 1, 3)
    assert np.array_equal(scenes.world_to_grid(base.origin, base.res, pos[:, 0, :]), cells)     # the probe is where q says
    inside = np.all((cells >= 0) & (cells < np.asarray(base.dims)), axis=1)
    want = np.where(inside, nc.hash_bits(cells), 0).astype(np.uint8)
    ok, lookups = s.state_valid_batch(Q)
    bad = np.nonzero(ok != want)[0]
    assert bad.size == 0, f"{bad.size} cells differ, the first at {cells[bad[:8]].tolist()}"
    assert (lookups == 1).all()
    assert want.any() and not want[~inside].any() and (~inside).sum() == cells.shape[0] - int(np.prod(base.dims))
    assert np.array_equal(grid.d2(), cfg.grid.d2)
    # and with the real field of the case: valid wherever the cell's distance reaches the probe's radius
    real = _case(kind, i)
    g2 = capi.Grid(real.grid.origin, real.grid.dims, real.grid.res, real.grid.max_dist, real.grid.d2)
    s2 = capi.Space(capi.Model(cfg.robot_text), g2, cfg.mprim, cfg.params)
    ok2, _ = s2.state_valid_batch(Q)
    assert np.array_equal(ok2.astype(bool), nc.plain_lookup(real.grid, Q) >= nc.PROBE_RADIUS * nc.PROBE_RADIUS)
    assert np.array_equal(g2.d2(), real.grid.d2)


# ----------------------------------------------------------------------------------------------------------------------
# 2. BFS
# ----------------------------------------------------------------------------------------------------------------------

def _bfs_both(s, plain, xyz, what):
    s.set_goal_xyz(list(xyz), XYZ_TOL)
    want = plain.run(xyz, nc.level_flood)
    got = s.bfs_grid()
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {bad.shape[0]} cells differ, the first [z y x] {bad[:6].tolist()}"
    return want


@pytest.mark.parametrize("i", PLANNING)
def test_bfs_grid_equals_the_plain_flood(i, oracles):
    """The config goal (deque flood), ten goals in a row, goal cells at the corners of the last, partial 8-cell brick of
    each axis (walls among them: the goal cell overwrites a wall) and a goal outside the grid, on ONE space."""
    from smpl_amd import capi
    _need_gpu()
    cfg = nc.planning_case(i)
    g = cfg.grid
    o = oracles(i)
    s = capi.Space.from_config(cfg)
    plain = nc.PlainBfs(g, cfg.params.bfs_radius)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    assert np.array_equal(s.goal_pose(), o.planning_fk(cfg.goal))
    want = plain.run(s.goal_pose())
    assert np.array_equal(s.bfs_grid(), want)
    assert ((want >= 0) & (want < nc.WALL)).sum() > 1000
    rng = np.random.default_rng(17 + i)
    for k in range(10):
        q = np.array(cfg.goal) + rng.uniform(-0.4, 0.4, size=len(cfg.goal))
        want = _bfs_both(s, plain, o.planning_fk(q), f"goal {k}")
        if k == 4:
            out = _bfs_both(s, plain, [50.0, 50.0, 50.0], "goal outside the grid")
            assert not ((out >= 0) & (out < nc.WALL)).any()
    corners = nc.last_brick_corner_cells(g.dims)
    assert len(corners) >= 24
    spread = 0
    for c in corners:
        want = _bfs_both(s, plain, nc.cell_centre(g, c), f"goal cell {c}")
        assert want[c[2] + 1, c[1] + 1, c[0] + 1] == 0
        spread += ((want > 0) & (want < nc.WALL)).sum() > 1000
    assert spread >= 8


@pytest.mark.parametrize("i", THIN)
def test_bfs_grid_on_thin_grids(i):
    """Axes shorter than one 8-cell brick, one grid of a single layer: every free cell and two wall cells as goals."""
    from smpl_amd import capi
    _need_gpu()
    cfg = nc.thin_case(i)
    g = cfg.grid
    s = capi.Space.from_config(cfg)
    plain = nc.PlainBfs(g, cfg.params.bfs_radius)
    walls = plain.walls[1:-1, 1:-1, 1:-1].transpose(2, 1, 0).copy()
    free, wall = np.argwhere(~walls), np.argwhere(walls)
    assert free.shape[0] >= 3 and wall.shape[0] >= 1
    goals = [tuple(c) for c in free[::max(1, free.shape[0] // 12)]] + [tuple(wall[0]), tuple(wall[-1])]
    reached = 0
    for c in goals:
        want = _bfs_both(s, plain, nc.cell_centre(g, c), f"goal cell {c}")
        reached = max(reached, int(((want > 0) & (want < nc.WALL)).sum()))
    assert reached >= 2
    out = _bfs_both(s, plain, [50.0, 50.0, 50.0], "goal outside the grid")
    assert not ((out >= 0) & (out < nc.WALL)).any()
    P = nc.metric_points(g, 300 + i)
    want = _bfs_both(s, plain, nc.cell_centre(g, goals[0]), "first goal again")
    assert np.array_equal(s.metric_goal_distance(P), nc.plain_metric_goal(g, want, P))


@pytest.mark.parametrize("i", PLANNING)
def test_metric_goal_and_start_distances(i, oracles):
    """getMetricGoalDistance / getMetricStartDistance at points inside, on the faces and outside."""
    from smpl_amd import capi
    _need_gpu()
    cfg = nc.planning_case(i)
    g = cfg.grid
    o = oracles(i)
    s = capi.Space.from_config(cfg)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_start(cfg.start)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    want = nc.PlainBfs(g, cfg.params.bfs_radius).run(o.planning_fk(cfg.goal))
    P = nc.metric_points(g, 200 + i)
    _, inside = nc.cells_of(g, P)
    assert inside.sum() > 100 and (~inside).sum() > 100
    mg = s.metric_goal_distance(P)
    assert np.array_equal(mg, nc.plain_metric_goal(g, want, P))
    assert np.array_equal(mg, np.array([o.metric_goal_distance(*p) for p in P]))
    ms = s.metric_start_distance(P)
    assert np.array_equal(ms, nc.plain_metric_start(g, o.planning_fk(cfg.start), P))
    assert len(np.unique(mg)) > 20 and len(np.unique(ms)) > 20


# ----------------------------------------------------------------------------------------------------------------------
# 3. collision
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", ["specialized", "generic"])
@pytest.mark.parametrize("i", PLANNING)
def test_collision_checks_equal_the_oracle_and_respect_the_plain_lookup(i, build, oracles):
    from smpl_amd import capi
    _need_gpu()
    cfg = nc.planning_case(i)
    o = oracles(i)
    s = capi.Space.from_config(cfg, generic_kernels=(build == "generic"))
    Q = nc.bench_states()
    nn = s.model.nnodes
    pos = s.sphere_positions(Q)
    assert np.array_equal(pos, np.stack([o.sphere_positions(q, nn) for q in Q]))
    ok, lk = s.state_valid_batch(Q)
    exp = [o.state_valid(q) for q in Q]
    assert np.array_equal(ok.astype(bool), np.array([e[0] for e in exp]))
    assert np.array_equal(lk, np.array([e[1] for e in exp]))
    assert ok.sum() >= 500
    # edges: primitive-sized moves, long edges, wrap-around of a continuous joint, zero motion
    rng = np.random.default_rng(3)
    A = Q
    B = A.copy()
    j = rng.integers(0, 7, size=A.shape[0])
    B[np.arange(A.shape[0]), j] += rng.choice([-7, -4, 4, 7], size=A.shape[0]) * scenes.DEG
    B[800:] = scenes.random_states(scenes.ARM7_LIMITS, 400, 4)
    B[1100:, 4] += 2.5 * np.pi
    B[1150:] = A[1150:]
    eok, elk, w = s.edge_valid_batch(A, B)
    ook, olk = o.edge_valid_batch(A, B)
    assert np.array_equal(w, np.array([o.waypoint_count(a, b) for a, b in zip(A, B)]))
    assert np.array_equal(eok, ook) and np.array_equal(elk, olk)
    assert w.max() > 5 and (w == 0).sum() == 50 and 20 < eok.sum() < 1180
    # without the oracle: every leaf clears the plain lookup and every checked pair of leaves is apart => valid
    m = s.model.arrays()
    leaves = np.nonzero(m["left"] < 0)[0]
    r = m["xyzr"][:, 3]
    tree_of = np.zeros(nn, int)
    for t in range(len(m["tree_first"]) - 1):
        tree_of[m["tree_first"][t]:m["tree_first"][t + 1]] = t
    look = nc.plain_lookup(cfg.grid, pos[:, leaves, :].reshape(-1, 3)).reshape(Q.shape[0], -1)
    clear = np.all(look >= (r[leaves] * r[leaves])[None, :], axis=1)
    pairs = {tuple(p) for p in m["pairs"].tolist()}
    I, J = [], []
    for a in leaves:
        for b in leaves:
            if (tree_of[a], tree_of[b]) in pairs:
                I.append(a); J.append(b)
    d = pos[:, J, :] - pos[:, I, :]
    rr = r[I] + r[J]
    apart = np.all((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2] > (rr * rr)[None, :], axis=1)
    brute = clear & apart
    assert brute.sum() >= 300
    assert ok[brute].all()                                  # no false collisions


# ----------------------------------------------------------------------------------------------------------------------
# 4. expansion
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def batches(oracles):
    """(Q, oracle rows) per planning grid: the first 300 valid benchmark states, the goal one of them"""
    cache = {}

    def get(i):
        if i not in cache:
            cfg, o = nc.planning_case(i), oracles(i)
            Qall = nc.bench_states()
            ok = np.array([o.state_valid(q)[0] for q in Qall])
            Q = np.ascontiguousarray(Qall[ok][:B_MAIN])
            assert Q.shape[0] == B_MAIN
            o.set_goal_joint(Q[GOAL_ROW], cfg.goal_tol)
            rows = [o.eval_state(q) for q in Q]
            cache[i] = Q, {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}
        return cache[i]
    return get


def _compare_rows(exp, got, rows):
    """the masks of test_gpu_configs._compare_batch"""
    for n, i in enumerate(rows):
        assert np.array_equal(exp["flags"][i], got["flags"][n]), f"flags of state {i}"
        f = exp["flags"][i]
        v = (f & 1) != 0
        ev = (f & 0x10) == 0
        assert np.array_equal(exp["coord"][i][v], got["coord"][n][v]), i
        assert np.array_equal(exp["q"][i][ev], got["q"][n][ev]), i
        assert np.array_equal(exp["h"][i][v], got["h"][n][v]) and np.array_equal(exp["cost"][i][v], got["cost"][n][v]), i
        coll = (f & 0x40) != 0
        assert np.array_equal(exp["lookups"][i][~coll], got["lookups"][n][~coll]), i


def _table_space(cfg, Q, **kw):
    """a space whose device table knows the states of a short search from one of the batch's own states"""
    from smpl_amd import capi
    s = capi.Space.from_config(cfg, batch_states=256, **kw)
    s.set_goal_joint(Q[GOAL_ROW], cfg.goal_tol)
    s.set_start(Q[START_ROW])
    s.plan(5.0, 1.0, 1.0, True, True, 40, 40)
    s.table_sync()
    return s


@pytest.mark.parametrize("i", PLANNING)
def test_expansion_batch_has_every_kind_of_edge(i, batches):
    Q, exp = batches(i)
    f = exp["flags"]
    census = dict(valid=int(((f & 1) != 0).sum()), goal=int(((f & 2) != 0).sum()), inactive=int(((f & 0x10) != 0).sum()),
                  limits=int(((f & 0x20) != 0).sum()), collided=int(((f & 0x40) != 0).sum()))
    print(f"{nc.planning_case(i).name}: flag census of the {B_MAIN}-state batch {census}")
    assert census["collided"] >= 20 and census["limits"] >= 20 and census["inactive"] >= 20 and census["goal"] >= 1
    assert census["valid"] >= 1000


@pytest.mark.parametrize("kernels", ["single-launch", "pipeline", "generic", "tiny-work-list"])
@pytest.mark.parametrize("i", PLANNING)
def test_expansion_rows_equal_eval_state(i, kernels, batches):
    """Every row of the batch against the oracle's GetSuccs loop body, through the single-launch kernel (batches of at
    most 256 states), the pipeline, the kernels linked into the library and the pipeline with a shrunken work list; on the
    pipeline the K5 call as well: ids against a host lookup."""
    _need_gpu()
    cfg = nc.planning_case(i)
    Q, exp = batches(i)
    kw = {"single-launch": {}, "pipeline": dict(no_small_kernel=True), "generic": dict(no_small_kernel=True, generic_kernels=True),
          "tiny-work-list": dict(no_small_kernel=True, tiny_work_list=True)}[kernels]
    s = _table_space(cfg, Q, **kw)
    assert s.specialized()[0] == (kernels != "generic")
    if kernels == "single-launch":
        for first in (0, 150):
            _compare_rows(exp, s.expand_batch(Q[first:first + 150]), range(first, first + 150))
        return
    got = s.expand_batch(Q)
    _compare_rows(exp, got, range(B_MAIN))
    assert not (got["flags"] & 0x80).any()
    k5 = s.expand_batch_k5(Q)
    valid = (exp["flags"] & 1) != 0
    assert np.array_equal(k5["flags"], exp["flags"])
    assert np.array_equal(k5["coord"][valid], exp["coord"][valid]) and np.array_equal(k5["h"][valid], exp["h"][valid])
    host = {tuple(s.get_state(n)[1]): n for n in range(1, s.num_states())}
    want_id = np.full(valid.shape, -1, np.int32)
    for a, p in zip(*np.nonzero(valid)):
        want_id[a, p] = host.get(tuple(exp["coord"][a, p]), -1)
    assert np.array_equal(k5["succ_id"], want_id)
    assert (want_id[START_ROW][valid[START_ROW]] >= 0).all() and valid[START_ROW].any() and (want_id[valid] < 0).sum() >= 1000
    goal = (exp["flags"] & 2) != 0
    assert k5["totals"][2] == 0 and k5["totals"][0] == valid.sum() and k5["totals"][1] == (valid & ((want_id < 0) | goal)).sum()


# ----------------------------------------------------------------------------------------------------------------------
# 5. search
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_plans():
    """the oracle's bounded 3000/3000 eps 5 -> 1 search per (planning grid, goal kind), fork semantics"""
    from oracle_binding import Oracle
    cache = {}

    def get(i, goal_kind):
        if (i, goal_kind) not in cache:
            cfg = nc.planning_case(i)
            o = Oracle(cfg)
            _set_goal(o, o, cfg, goal_kind)
            sid = o.set_start(cfg.start)
            o.search_params(*SEARCH)
            cache[(i, goal_kind)] = (o.plan(), o.num_states(), sid)
        return cache[(i, goal_kind)]
    return get


def _set_goal(x, o, cfg, goal_kind):
    if goal_kind == "joint":
        x.set_goal_joint(cfg.goal, cfg.goal_tol)
    else:
        x.set_goal_xyz(o.planning_fk(cfg.goal), XYZ_TOL)


def _same_plan(eo, n_states, go, s=None):
    assert eo["ok"] == go["solved"] and eo["expansions"] == go["expansions"]
    assert np.array_equal(eo["expansion_log"], go["expansion_log"])
    assert eo["cost"] == go["cost"] and np.array_equal(eo["path"], go["path"])
    assert eo["eps"] == go["satisfied_eps"]
    assert eo["succ_evals"] == go["committed_succ_evals"]
    if s is not None:
        assert n_states == s.num_states()


@pytest.mark.parametrize("goal_kind", ["joint", "xyz"])
@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("i", PLANNING)
def test_search_equals_the_oracle(i, mode, goal_kind, oracles, oracle_plans, monkeypatch):
    from smpl_amd import capi
    _need_gpu()
    monkeypatch.setenv("SMPLX_SEARCH", mode)
    cfg = nc.planning_case(i)
    eo, n_states, sid = oracle_plans(i, goal_kind)
    assert eo["expansions"] >= 1000
    s = capi.Space.from_config(cfg, batch_states=256)
    _set_goal(s, oracles(i), cfg, goal_kind)
    assert s.set_start(cfg.start) == sid
    go = s.plan(*SEARCH)
    _same_plan(eo, n_states, go, s)
    assert (go["cache_misses"] == 0) == (mode == "device")


@pytest.mark.parametrize("mode", ["host", "device"])
def test_plan_multi_over_three_different_grids(mode, oracles, oracle_plans, monkeypatch):
    """smplx_plan_multi with one space per planning grid in ONE call: the search kernel's per-query space table holds three
    grids of different shapes.  Each query equals its solo run and the oracle."""
    from smpl_amd import capi
    _need_gpu()
    monkeypatch.setenv("SMPLX_SEARCH", mode)

    def make():
        out = []
        for i in PLANNING:
            cfg = nc.planning_case(i)
            sp = capi.Space.from_config(cfg, batch_states=256)
            sp.set_goal_joint(cfg.goal, cfg.goal_tol)
            sp.set_start(cfg.start)
            out.append(sp)
        return out
    spaces = make()
    multi, wall = capi.Space.plan_multi(spaces, *SEARCH, host_threads=3 if mode == "host" else 1)
    assert len(multi) == 3 and wall > 0
    for i, (sp, solo_sp, m) in enumerate(zip(spaces, make(), multi)):
        eo, n_states, _ = oracle_plans(i, "joint")
        _same_plan(eo, n_states, m, sp)
        solo = solo_sp.plan(*SEARCH)
        _same_plan(eo, n_states, solo, solo_sp)
        assert (m["cache_misses"] == 0) == (mode == "device")
    assert len({tuple(m["expansion_log"][:200]) for m in multi}) == 3       # three different searches


# ----------------------------------------------------------------------------------------------------------------------
# 6. field
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", PLANNING)
def test_field_on_planning_grids(i):
    """Grid.from_boxes against the host builder; the window of one added point near a corner is the product of three
    different clipped extents; add / update / remove equals a fresh build."""
    from smpl_amd import capi
    _need_gpu()
    cfg = nc.planning_case(i)
    gr = cfg.grid
    dims, dmax = gr.dims, gr.dmax_int
    g = capi.Grid.from_boxes(gr.origin, dims, gr.res, gr.max_dist, cfg.boxes)
    assert np.array_equal(g.d2(), gr.d2)
    c = nc.corner_edit_cell(dims)
    assert gr.d2[c] > 0
    g.add_points(nc.cell_centre(gr, [c]))
    want = nc.edit_window_cells(dims, c, dmax)
    assert g.last_edit_cells() == want and want < (2 * dmax + 1) ** 3
    rng = np.random.default_rng(3 + i)
    free = np.argwhere(gr.d2 > 0)
    free = free[~np.all(free == np.asarray(c), axis=1)]
    pick = free[rng.choice(free.shape[0], size=290, replace=False)]
    cloud_a, cloud_b = pick[:200], np.vstack([pick[:120], pick[200:]])
    g.add_points(nc.cell_centre(gr, cloud_a))
    g.update_points(nc.cell_centre(gr, cloud_a), nc.cell_centre(gr, cloud_b))
    g.remove_points(nc.cell_centre(gr, [c]))
    fresh = capi.Grid.from_boxes(gr.origin, dims, gr.res, gr.max_dist, cfg.boxes)
    fresh.add_points(nc.cell_centre(gr, cloud_b))
    got = g.d2()
    assert np.array_equal(got, fresh.d2())
    host = scenes.build_grid(gr.origin, dims, gr.res, gr.max_dist,
                             list(cfg.boxes) + [(tuple(p), (gr.res * 0.5,) * 3) for p in nc.cell_centre(gr, cloud_b)])
    assert np.array_equal(got, host.d2)


@pytest.mark.parametrize("i", THIN)
def test_field_on_thin_grids(i):
    from smpl_amd import capi
    _need_gpu()
    cfg = nc.thin_case(i)
    gr = cfg.grid
    dmax = gr.dmax_int
    g = capi.Grid.empty(gr.origin, gr.dims, gr.res, gr.max_dist)
    assert np.array_equal(g.d2(), nc.brute_force(np.zeros(gr.dims, bool), dmax))
    g.add_boxes(cfg.boxes)
    assert np.array_equal(g.d2(), gr.d2)
    occ = nc.box_occupancy(gr.origin, gr.res, gr.dims, cfg.boxes)
    free = np.argwhere(~occ)
    add = free[::max(1, free.shape[0] // 5)]
    g.add_points(nc.cell_centre(gr, add))
    occ[add[:, 0], add[:, 1], add[:, 2]] = True
    assert np.array_equal(g.d2(), nc.brute_force(occ, dmax))
    g.remove_points(nc.cell_centre(gr, add[:2]))
    occ[add[:2, 0], add[:2, 1], add[:2, 2]] = False
    assert np.array_equal(g.d2(), nc.brute_force(occ, dmax))


# ----------------------------------------------------------------------------------------------------------------------
# 7. attached body
# ----------------------------------------------------------------------------------------------------------------------

def test_attached_body_states_equal_oracle_pseudo_link():
    """test_gpu_attached_bodies.test_states_equal_oracle_pseudo_link on the first planning grid"""
    import test_gpu_attached_bodies as ab
    ab.test_states_equal_oracle_pseudo_link(nc.planning_case(0), "specialized")
