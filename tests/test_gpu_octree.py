"""Octree shapes on the GPU (include/smpl_amd.h "world objects"): the device's cell lists against the model of the
reference (tests/octree_ref.py; cases in tests/octree_cases.py) -- same length, order and duplicates -- and insert / remove
/ move against fresh grids that got the model's cells through add_points.  The implementation is never compared with
itself."""
import numpy as np
import pytest

import octree_cases as T
import octree_ref as O
import world_cases as W
from smpl_amd import capi

pytestmark = pytest.mark.gpu

E_ARG, E_LIMIT = -1, -3


def _grid(counted=False):
    g = capi.Grid.empty(W.ORIGIN, W.DIMS, W.RES, W.MAX_DIST)
    if counted:
        g.set_ref_counted(True)
    return g


@pytest.fixture(scope="module")
def empty():
    g = _grid(True)
    return g.d2(), g.counts()


def _refused(code, call, word=None):
    with pytest.raises(capi.SmplxError) as e:
        call()
    assert e.value.code == code
    if word:
        assert word in str(e.value)


@pytest.mark.parametrize("pose", list(T.POSES))
@pytest.mark.parametrize("key", T.KEYS)
def test_lists_counts_and_field_equal_the_model(empty, key, pose):
    want = T.judged(key, pose)
    s = capi.octree(T.leaves(key), T.POSES[pose])
    if key in T.TRIPS:      # both trip counts occur in this case: the model's own loops say so
        trips = [tuple(len(O.axis_values(leaf[a], leaf[3], W.RES)) for a in range(3)) for leaf in T.leaves(key)]
        flat = {n for t in trips for n in t}
        assert trips == T.TRIPS[key] and flat == {min(flat), min(flat) + 1} and min(flat) == 2 * np.ceil(T.leaves(key)[0][3] / W.RES)
    g = _grid(counted=True)
    (got,) = g.voxelize([s])
    print(f"{key}/{pose}: {len(T.leaves(key))} leaves, {len(got)} cells, the model {len(want)}, distinct {len(np.unique(want, axis=0))}")
    assert got.shape == want.shape and np.array_equal(got, want)
    assert g.objects() == [] and np.array_equal(g.counts(), empty[1])          # voxelize changes nothing
    g.insert_object("map", [s])
    assert g.objects() == ["map"]
    stored = g.object_cells("map", 0)
    assert stored.shape == want.shape and np.array_equal(stored, want)
    assert np.array_equal(g.counts(), T.multiplicities(want))
    if len(want):
        assert (key in ("small", "equal")) == (len(want) == 1)
        f = _grid()
        f.add_points(T.unique_points(want))
        assert np.array_equal(g.d2(), f.d2())
    else:
        assert np.array_equal(g.d2(), empty[0])                                 # a valid edit with 0 cells
    g.remove_object("map")
    assert g.objects() == [] and np.array_equal(g.counts(), empty[1]) and np.array_equal(g.d2(), empty[0])


def test_duplicates_are_kept_and_counted():
    """the reference samples twice the leaf's width at the grid's own resolution: cells are hit more than once"""
    want = T.judged("two_res", "rotated")
    assert len(np.unique(want, axis=0)) < len(want)
    g = _grid(counted=True)
    g.insert_object("a", [capi.octree(T.leaves("two_res"), W.POSE)])
    assert g.counts().max() >= 2 and g.counts().sum() == len(want)
    # a second object over the same cells; removing one leaves the other whole
    g.insert_object("b", [capi.octree(T.leaves("two_res"), W.POSE)])
    assert np.array_equal(g.counts(), 2 * T.multiplicities(want))
    g.remove_object("a")
    assert np.array_equal(g.counts(), T.multiplicities(want))


def test_without_counts_remove_frees_shared_cells_and_move_is_remove_then_insert():
    a_s = capi.octree(T.leaves("odd"), T.IDENTITY)
    b_s = capi.octree(T.leaves("big"), T.IDENTITY)
    a_c, b_c = T.judged("odd", "identity"), T.judged("big", "identity")
    assert set(map(tuple, a_c)) & set(map(tuple, b_c))            # the objects overlap
    g = _grid()
    g.insert_object("a", [a_s])
    g.insert_object("b", [b_s])
    g.remove_object("a")
    f = _grid()
    f.add_points(T.unique_points(a_c))
    f.add_points(T.unique_points(b_c))
    f.remove_points(T.unique_points(a_c))
    assert np.array_equal(g.d2(), f.d2())
    only_b = _grid()
    only_b.add_points(T.unique_points(b_c))
    assert not np.array_equal(g.d2(), only_b.d2())                # as the reference: the shared cells went with `a`
    # move: one edit that equals remove followed by insert, with and without counts
    for counted in (False, True):
        m, r = _grid(counted), _grid(counted)
        for h in (m, r):
            h.insert_object("other", [W.judged("cone")[0]])
            h.insert_object("map", [capi.octree(T.leaves("two_res"), W.POSE)])
        moved = capi.octree(T.leaves("odd"), W.POSE)
        m.move_object("map", [moved])
        r.remove_object("map")
        r.insert_object("map", [moved])
        assert np.array_equal(m.d2(), r.d2()) and np.array_equal(m.object_cells("map", 0), T.judged("odd", "rotated"))
        assert m.objects() == ["other", "map"]
        if counted:
            assert np.array_equal(m.counts(), r.counts())
            assert np.array_equal(m.counts(), T.multiplicities(T.judged("odd", "rotated")) + T.multiplicities(W.judged("cone")[1]))


def test_an_object_mixing_shapes_keeps_per_shape_lists_in_order():
    box, box_cells, und = W.judged("box")
    assert len(und) == 0
    oct_s, oct_c = capi.octree(T.leaves("odd"), W.POSE), T.judged("odd", "rotated")
    far = capi.octree(T.leaves("outside"), W.POSE)
    big_s, big_c = capi.octree(T.leaves("big"), T.IDENTITY), T.judged("big", "identity")
    g = _grid(counted=True)
    shapes = [oct_s, box, far, big_s, W.judged("cone")[0]]
    lists = g.voxelize(shapes)
    want = [oct_c, box_cells, np.zeros((0, 3), int), big_c, W.judged("cone")[1]]
    assert [len(c) for c in lists] == [len(c) for c in want]
    for got, w in zip(lists, want):
        assert np.array_equal(got, w)
    g.insert_object("mixed", shapes)
    for i, w in enumerate(want):
        assert np.array_equal(g.object_cells("mixed", i), w), i
    assert np.array_equal(g.counts(), sum(T.multiplicities(w) for w in want if len(w)))
    f = _grid()
    for w in want:
        if len(w):
            f.add_points(T.unique_points(w))
    assert np.array_equal(g.d2(), f.d2())
    g.move_object("mixed", [box, oct_s])
    assert np.array_equal(g.object_cells("mixed", 0), box_cells) and np.array_equal(g.object_cells("mixed", 1), oct_c)
    assert np.array_equal(g.counts(), T.multiplicities(box_cells) + T.multiplicities(oct_c))
    g.remove_all_objects()
    assert g.counts().max() == 0


def test_limits_are_refused_before_anything_changes():
    g = _grid(counted=True)
    ok = capi.octree(T.leaves("two_res"), W.POSE)
    g.insert_object("map", [ok])
    before_counts, before_d2 = g.counts(), g.d2()
    wide = capi.octree([(0.1, 0.1, 0.1, 1025 * W.RES)])                       # size / res > 1024
    many = capi.octree(np.tile([(0.1, 0.1, 0.1, 300 * W.RES)], (4, 1)))        # 4 * 601^3 > 2^31 / 3 sample points; 3 would fit
    for bad in (wide, many):
        _refused(E_LIMIT, lambda: g.voxelize([bad]))
        _refused(E_LIMIT, lambda: g.insert_object("big", [ok, bad]))
        _refused(E_LIMIT, lambda: g.move_object("map", [bad]))
    assert g.objects() == ["map"] and np.array_equal(g.object_cells("map", 0), T.judged("two_res", "rotated"))
    assert np.array_equal(g.counts(), before_counts) and np.array_equal(g.d2(), before_d2)
    _refused(E_ARG, lambda: g.insert_object("map", [ok]))                      # the id is taken (checkInsertOctomap)


def test_a_space_sees_the_octree_and_attachment_refuses_it(small_cfg):
    """EDITS AND SPACES: the collision checker reads the new field at once -- a state whose sphere centre lies inside an
    inserted leaf turns invalid; an octree cannot be attached to the robot"""
    cfg, gr = small_cfg, small_cfg.grid
    g = capi.Grid.empty(gr.origin, gr.dims, gr.res, gr.max_dist)
    s = capi.Space(capi.Model(cfg.robot_text), g, cfg.mprim, cfg.params, 16)
    q = np.asarray([cfg.start])
    assert s.state_valid_batch(q)[0][0] == 1
    centre = s.sphere_positions(q)[0, -1]
    leaf = capi.octree([tuple(centre) + (gr.res,)])
    g.insert_object("map", [leaf])
    cell = tuple(O.world_to_cell(float(centre[a]), float(gr.origin[a]), gr.res) for a in range(3))
    assert g.object_cells("map", 0).tolist() == [list(cell)]
    assert s.state_valid_batch(q)[0][0] == 0
    g.remove_object("map")
    assert s.state_valid_batch(q)[0][0] == 1
    link = "r_gripper_palm_link" if "link r_gripper_palm_link" in cfg.robot_text else "gripper_palm_link"
    _refused(E_ARG, lambda: s.object_spheres([leaf]), "octree")
    _refused(E_ARG, lambda: s.object_spheres([capi.box((0.05, 0.05, 0.05)), leaf]), "octree")
    _refused(E_ARG, lambda: s.attach_object("held", link, [leaf]), "octree")
    assert s.attached_bodies() == []
