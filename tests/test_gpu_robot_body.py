"""The robot body on the GPU (include/smpl_amd.h "robot body") against the plain model
(tests/body_ref.py) on the shared body of tests/body_cases.py: voxel models point for point, link transforms against
independent kinematics, placed cells against the point rule, the field against fresh grids that got the same cells
through add_points, the bookkeeping of a put, and a planning query that has to avoid a body link."""
import copy

import numpy as np
import pytest

import body_cases as C
import body_ref as B
import kinematics_ref as K
from smpl_amd import capi, scenes

pytestmark = pytest.mark.gpu

NM = len(C.MODELS)
DMAX = int(np.ceil(C.MAX_DIST / C.RES))


def _grid(counted=False):
    g = capi.Grid.empty(C.ORIGIN, C.DIMS, C.RES, C.MAX_DIST)
    if counted:
        g.set_ref_counted(True)
    return g


def _refused(code, call):
    with pytest.raises(capi.SmplxError) as e:
        call()
    assert e.value.code == code


def _centres(cells, origin=C.ORIGIN, res=C.RES):
    """world points that land in the given cells (rows of -1 left out)"""
    c = np.asarray(cells, int).reshape(-1, 3)
    c = c[c[:, 0] >= 0]
    return np.asarray(origin) + c * res


def _fresh_from(occ, counts, counted):
    """a new grid that got, through add_points, every occupied cell (with counts: as often as it counts)"""
    g = _grid(counted)
    cells = np.argwhere(occ)
    if counted:
        cells = np.repeat(cells, counts[occ].astype(int), axis=0)
    if len(cells):
        g.add_points(_centres(cells))
    return g


def _same(g, want, counted):
    assert np.array_equal(g.d2(), want.d2())
    if counted:
        assert np.array_equal(g.counts(), want.counts())


def _window(cell_lists):
    c = np.vstack([np.asarray(x).reshape(-1, 3) for x in cell_lists])
    c = c[c[:, 0] >= 0]
    lo = np.maximum(c.min(0) - DMAX, 0)
    hi = np.minimum(c.max(0) + DMAX, np.asarray(C.DIMS) - 1)
    n, whole = int(np.prod(hi - lo + 1)), int(np.prod(C.DIMS))
    return whole if 2 * n > whole else n


def _expected_cells(body):
    """the point rule on the engine's own transforms and points, per model"""
    T = body.link_transforms()
    out = []
    for m in range(NM):
        cells, margin = B.place(T[body.model_link(m)], body.model_points(m), C.ORIGIN, C.RES, C.DIMS)
        assert len(margin) == 0 or margin.min() > 1e-9, C.MODELS[m]     # no exemption
        out.append(cells)
    return out


# ---- 1. models -------------------------------------------------------------------------------------------------------
def test_models_equal_the_reference_model_point_for_point():
    body = capi.Body(C.body_text())
    assert (body.nlinks, body.njoints, body.nmodels, body.noutside) == (8, 7, NM, NM - 1)
    total = 0
    for m in range(NM):
        want, near, missing = C.model_points(m)
        got = body.model_points(m)
        total += len(got)
        print(f"{C.MODELS[m]}: {len(got)} points, the model {len(want)}, undecided {int(near.sum()) + len(missing)}")
        if m != C.GROUP_MODEL:
            assert near.sum() == 0 and len(missing) == 0
            assert np.array_equal(got, want), C.MODELS[m]
        else:       # the axis-aligned box: undecided voxels (at most 15 %) left out, the decided ones equal and in order
            und = set(map(tuple, want[near])) | set(map(tuple, missing))
            assert 0 < len(und) <= 0.15 * len(want)
            keep = lambda p: np.array([r for r in p if tuple(r) not in und]).reshape(-1, 3)
            assert np.array_equal(keep(got), keep(want))
        assert body.model_link(m) == C.model().links.index(C.MODELS[m])
    assert body.npoints == total
    _refused(-1, lambda: body.model_points(NM))
    # a link without geom rows has an empty model; a finer model of the same link is a different lattice
    b2 = capi.Body("link a\nlink b\njoint j fixed a b 0 0 0 0 0 0 0 0 1 0 0\ngeom b sphere 0.03 0.0013 0.0027 0.0031 0.1 0.2 0.3\n"
                   "voxels a 0.01\nvoxels b 0.005\n")
    assert len(b2.model_points(0)) == 0
    want = B.Body("link b\ngeom b sphere 0.03 0.0013 0.0027 0.0031 0.1 0.2 0.3\nvoxels b 0.005\n").model_points(0)
    assert want[1].sum() == 0 and np.array_equal(b2.model_points(1), want[0])
    g = _grid()
    g.put_body(b2)
    assert len(g.body_cells(0)) == 0 and len(g.body_cells(1)) == len(want[0])


# ---- 2. transforms ---------------------------------------------------------------------------------------------------
def test_link_transforms_against_independent_kinematics():
    body = capi.Body(C.body_text())
    M = B.Body(C.body_text())
    for step in [None, C.SECOND_Q, ("j1", -1.2137), ("js", 2.5137), ("jf", 0.3137)]:
        if step:
            body.set_joint(*step)
            M.set_joint(*step)
            assert body.joint(step[0]) == step[1]
        T, F = body.link_transforms(), M.frames()
        worst = max(K.error(T[i], F[l]).max() for i, l in enumerate(M.links))
        print(f"after {step}: worst error {worst / K.U52:.2f} x 2^-52")
        assert worst <= K.BOUND
    _refused(-1, lambda: body.set_joint("nosuch", 0.1))
    _refused(-1, lambda: body.set_joint("jt", 0.1))           # fixed
    _refused(-1, lambda: body.set_joint("j1", float("nan")))
    _refused(-1, lambda: body.joint("nosuch"))
    assert body.joint("j1") == -1.2137


# ---- 3. and 4. placing and the field ---------------------------------------------------------------------------------
@pytest.mark.parametrize("counted", [False, True])
def test_put_places_the_states_and_updates_the_field_once(counted):
    body = capi.Body(C.body_text())
    M = B.Body(C.body_text())
    g = _grid(counted)
    assert body.dirty().all() and all(len(g.body_cells(m)) == 0 for m in range(NM))
    g.put_body(body)
    first = _expected_cells(body)
    for m in range(NM):
        got = g.body_cells(m)
        if m == C.GROUP_MODEL:
            assert len(got) == 0                            # a group link's model has no list
            continue
        assert np.array_equal(got, first[m]), C.MODELS[m]
    far, edge = C.MODELS.index("far"), C.MODELS.index("edge")
    assert (first[far] == -1).all() and 0 < (first[edge][:, 0] >= 0).sum() < len(first[edge])
    placed = M.put()
    assert placed == [m for m in range(NM) if m != C.GROUP_MODEL]
    assert np.array_equal(body.dirty(), M.dirty) and body.dirty().tolist() == [m == C.GROUP_MODEL for m in range(NM)]
    steps = [([], first[m]) for m in placed]
    occ, counts = B.occupancy_after(steps, C.DIMS, counted)
    _same(g, _fresh_from(occ, counts, counted), counted)
    if counted:
        assert counts.max() >= 2                            # several 0.01 m points in one 0.02 m cell count several times
    assert g.last_edit_cells() == _window([first[m] for m in placed])

    # the middle joint: only its link and the descendants are placed again
    body.set_joint(*C.SECOND_Q)
    M.set_joint(*C.SECOND_Q)
    assert np.array_equal(body.dirty(), M.dirty)
    moved = M.put()
    assert moved == [C.MODELS.index("l2")]
    g.put_body(body)
    second = _expected_cells(body)
    for m in range(NM):
        got = g.body_cells(m)
        if m == C.GROUP_MODEL:
            assert len(got) == 0
        elif m in moved:
            assert np.array_equal(got, second[m]) and not np.array_equal(got, first[m])
        else:
            assert np.array_equal(got, first[m]) and np.array_equal(second[m], first[m])
    assert not body.dirty()[moved[0]]
    steps += [(first[m], second[m]) for m in moved]
    occ, counts = B.occupancy_after(steps, C.DIMS, counted)
    _same(g, _fresh_from(occ, counts, counted), counted)
    if counted:     # with counts the grid is that of the new points alone
        occ2, counts2 = B.occupancy_after([([], second[m]) for m in placed], C.DIMS, True)
        assert np.array_equal(counts, counts2)
    one = _window([first[m] for m in moved] + [second[m] for m in moved])
    assert g.last_edit_cells() == one < int(np.prod(C.DIMS))

    # take: everything out again
    g.take_body()
    assert all(len(g.body_cells(m)) == 0 for m in range(NM))
    if counted:
        _same(g, _grid(True), True)
    else:
        assert np.array_equal(g.d2(), _grid().d2())
    _refused(-5, lambda: g.take_body())


def _rooted_text():
    """the body of body_cases under one more link: the joint jr on the new root moves every link at once"""
    return (C.body_text().replace("link base", "link world\nlink base", 1)
            + "joint jr revolute world base  0 0 0  0 0 0  0 0 1  -3 3\nvoxels world 0.01\nvalue jr 0.0\n")


def test_the_work_space_of_a_put_across_puts():
    """A put carves the transforms, prefixes and boxes of the states it places out of a work space kept with the grid's
    record of the body, which only grows (device_mem.h): one state takes three 256-byte pieces, all seven take six.  A
    grid's first put of a body places every state, whatever moved, so the small put cannot come before it; from there the
    order is a put that places one state (a leaf joint moved) inside the larger block, a put that places all states (the
    root joint moved), then take_body -- the record and its work space go -- and a put of the body again.  The cells of
    every model are the point rule's on the engine's own transforms, and counts and field those of a fresh grid that got
    the replayed lists, at each step."""
    text = _rooted_text()
    body, M = capi.Body(text), B.Body(text)
    nm = body.nmodels
    assert nm == NM + 1 and len(body.model_points(nm - 1)) == 0            # the new root's model is empty
    outside = [m for m in range(nm) if M.outside[m] and len(body.model_points(m)) > 0]
    assert len(outside) == 7

    def expected():
        T = body.link_transforms()
        out = []
        for m in range(nm):
            cells, margin = B.place(T[body.model_link(m)], body.model_points(m), C.ORIGIN, C.RES, C.DIMS)
            assert len(margin) == 0 or margin.min() > 1e-9, m
            out.append(cells)
        return out

    g = _grid(True)
    steps, now = [], {m: [] for m in outside}

    def put_and_check(moved, tag):
        g.put_body(body)
        want = expected()
        for m in outside:
            assert np.array_equal(g.body_cells(m), want[m]), (tag, m)
            assert (m in moved) or np.array_equal(want[m], now[m]), (tag, m)
        for m in moved:
            steps.append((now[m], want[m]))
            now[m] = want[m]
        occ, counts = B.occupancy_after(steps, C.DIMS, True)
        _same(g, _fresh_from(occ, counts, True), True)

    put_and_check(outside, "first put")
    l2 = [m for m in outside if body.model_link(m) == M.links.index("l2")]
    body.set_joint(*C.SECOND_Q)
    assert [m for m in outside if body.dirty()[m]] == l2 and len(l2) == 1
    put_and_check(l2, "one state")
    body.set_joint("jr", 0.0137)
    assert [m for m in outside if body.dirty()[m]] == outside
    put_and_check(outside, "all states")
    g.take_body()
    _same(g, _grid(True), True)
    steps, now = [], {m: [] for m in outside}
    put_and_check(outside, "after take")


@pytest.mark.parametrize("counted", [False, True])
def test_a_world_object_that_overlaps_the_body(counted):
    body = capi.Body(C.body_text())
    g = _grid(counted)
    crate = capi.box((0.1, 0.1, 0.1), capi.pose_at((0.2137, 0.0137, 0.1537)))    # around the base link's box
    g.insert_object("crate", [crate])
    obj = g.object_cells("crate", 0)
    g.put_body(body)
    cells = [g.body_cells(m) for m in range(NM)]
    inside = np.vstack([c[c[:, 0] >= 0] for c in cells])
    shared = set(map(tuple, obj)) & set(map(tuple, inside))
    assert len(shared) > 20
    g.take_body()
    want = _grid(counted)
    want.add_points(_centres(obj))
    if counted:     # the object survives with its cells intact
        _same(g, want, True)
    else:           # it loses the shared cells, as remove_object would take them
        want.remove_points(_centres(inside))
        _same(g, want, False)
        only = _grid()
        only.add_points(_centres(obj))
        assert not np.array_equal(g.d2(), only.d2())


# ---- 5. no-op, staleness, ownership ----------------------------------------------------------------------------------
def _bar_text(at, q=0.0):
    return ("robot bar\nlink world\nlink bar\njoint swing revolute world bar  %r %r %r  0 0 0  0 0 1  -3 3\n"
            "geom bar box 0.1 0.1 0.1  0.0013 0.0021 0.0017  0 0 0\nvoxels bar 0.01\nvalue swing %r\n"
            % (float(at[0]), float(at[1]), float(at[2]), float(q)))


def _small_space(cfg, kind):
    gr = cfg.grid
    g = capi.Grid.from_boxes(gr.origin, gr.dims, gr.res, gr.max_dist, cfg.boxes)
    s = capi.Space(capi.Model(cfg.robot_text), g, cfg.mprim, cfg.params, 128, generic_kernels=(kind == "generic"))
    assert s.specialized()[0] == (kind == "specialized"), s.specialized()[1]
    return g, s


@pytest.mark.parametrize("kind", ["specialized", "generic"])
def test_no_op_put_staleness_and_ownership(small_cfg, kind):
    cfg = small_cfg
    g, s = _small_space(cfg, kind)
    g.set_ref_counted(True)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    start = s.set_start(cfg.start)
    n_succs = len(s.get_succs(start)[0])
    at = np.asarray(cfg.grid.origin) + 0.3137
    body = capi.Body(_bar_text(at, 0.4321))
    g.put_body(body)                                        # changes cells: an edit
    _refused(-5, lambda: s.get_succs(start))
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    start = s.set_start(cfg.start)
    assert len(s.get_succs(start)[0]) == n_succs
    d2, counts, edit = g.d2(), g.counts(), g.last_edit_cells()
    g.put_body(body)                                        # nothing dirty: not an edit
    body.set_joint("swing", 0.4321)                         # the same value dirties nothing
    assert not body.dirty().any()
    g.put_body(body)
    assert np.array_equal(g.d2(), d2) and np.array_equal(g.counts(), counts) and g.last_edit_cells() == edit
    assert len(s.get_succs(start)[0]) == n_succs            # the space still answers
    body.set_joint("swing", 0.9137)
    g.put_body(body)
    _refused(-5, lambda: s.get_succs(start))
    assert not np.array_equal(g.d2(), d2)
    # a second body is refused and changes nothing
    other = capi.Body(_bar_text(at + 0.2))
    d2, cells = g.d2(), g.body_cells(0)
    _refused(-5, lambda: g.put_body(other))
    assert np.array_equal(g.d2(), d2) and np.array_equal(g.body_cells(0), cells) and other.dirty().all()
    # take, then put is fine; the handle may be destroyed while placed and take still works
    g.take_body()
    g.put_body(other)
    assert len(g.body_cells(0)) == other.npoints and not other.dirty().any()
    other.close()
    assert len(g.body_cells(0)) > 0
    g.take_body()
    fresh = capi.Grid.from_boxes(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.boxes)
    fresh.set_ref_counted(True)
    assert np.array_equal(g.d2(), fresh.d2()) and np.array_equal(g.counts(), fresh.counts())
    # a body the grid has not seen is placed whole, whatever its flags say
    g.put_body(body)
    assert len(g.body_cells(0)) == body.npoints
    # a grid from a finished field refuses, as it refuses objects
    fixed = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    _refused(-5, lambda: fixed.put_body(body))
    _refused(-5, lambda: fixed.take_body())


# ---- 6. it matters ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["specialized", "generic"])
def test_a_body_link_across_the_path_is_avoided(small_cfg, kind):
    from oracle_binding import Oracle
    cfg, gr = small_cfg, small_cfg.grid
    g, s = _small_space(cfg, kind)
    a, b = np.asarray(cfg.start), np.asarray(cfg.goal)
    Q = np.array([a + t * (b - a) for t in np.linspace(0.0, 1.0, 9)])
    before_s = s.state_valid_batch(Q)[0]
    before_e = s.edge_valid_batch(Q[:-1], Q[1:])[0]
    assert before_s.all()
    # a box of 0.1 m beside the arm's far end half way along the straight path: the path's fourth state runs into it, and a
    # detour exists (the oracle finds one that costs two steps more than the free path's 19500)
    centre = s.sphere_positions(Q[4:5])[0, -1] + np.array([0.0, 0.1, 0.0])
    body = capi.Body(_bar_text(centre, 0.4321))
    g.put_body(body)
    # the oracle on a grid given the same points through add_points
    T = body.link_transforms()[body.model_link(0)]
    cells, margin = B.place(T, body.model_points(0), gr.origin, gr.res, gr.dims)
    assert margin.min() > 1e-9 and np.array_equal(g.body_cells(0), cells)
    g2 = capi.Grid.from_boxes(gr.origin, gr.dims, gr.res, gr.max_dist, cfg.boxes)
    g2.add_points(_centres(cells, gr.origin, gr.res))
    cfg2 = copy.copy(cfg)
    cfg2.grid = scenes.Grid(gr.origin, gr.dims, gr.res, gr.max_dist, g2.d2())
    assert np.array_equal(g.d2(), cfg2.grid.d2)
    o = Oracle(cfg2)
    after_s = s.state_valid_batch(Q)[0]
    after_e = s.edge_valid_batch(Q[:-1], Q[1:])[0]
    assert np.array_equal(after_s, [int(o.state_valid(q)[0]) for q in Q])
    assert np.array_equal(after_e, o.edge_valid_batch(Q[:-1], Q[1:])[0])
    assert after_s[3] == 0 and after_s[0] == 1 and after_s[-1] == 1 and (after_e < before_e).any() and (after_e <= before_e).all()
    # the old space is stale until the goal is set again, and then plans (with the BFS walls of the field it was created
    # on: EDITS AND SPACES in include/smpl_amd.h)
    _refused(-5, lambda: s.plan(5.0, 1.0, 1.0, True, True, 1500, 1500))
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_start(cfg.start)
    s.plan(5.0, 1.0, 1.0, True, True, 200, 200)
    # a space created on the grid as it is now has the new walls too: its plan equals the oracle's on the grid that got the
    # same points through add_points -- ids, order, cost
    s2 = capi.Space(capi.Model(cfg.robot_text), g, cfg.mprim, cfg.params, 128, generic_kernels=(kind == "generic"))
    s2.set_goal_joint(cfg.goal, cfg.goal_tol)
    o.set_order(chain=False)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    assert o.set_start(cfg.start) == s2.set_start(cfg.start)
    o.search_params(5.0, 1.0, 1.0, True, True, 4000, 4000)
    ro = o.plan()
    rg = s2.plan(5.0, 1.0, 1.0, True, True, 4000, 4000)
    print(f"plan with the body in the way: cost {rg['cost']}, {rg['expansions']} expansions, path of {len(rg['path'])}")
    assert ro["cost"] == rg["cost"] and np.array_equal(ro["expansion_log"], rg["expansion_log"]) and np.array_equal(ro["path"], rg["path"])
    assert rg["cost"] > 19500 and len(rg["path"]) > 0      # solved, around the body
