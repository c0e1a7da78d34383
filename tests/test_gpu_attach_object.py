"""Objects attached by shape (smplx_attach_object; CollisionSpace::attachObject(id, shapes, transforms, link),
collision_space.cpp:297-304): the sphere model AttachedBodiesCollisionModel::generateSpheresModel makes
(attached_bodies_collision_model.cpp:264-313), voxelised on the GPU.

The judge is tests/voxelize_ref.py on that model's lattice (tests/object_cases.py).  Every comparison is exact -- doubles
bit for bit -- and every test first asserts that no cell of its input is too close to one of the voxeliser's comparisons
to call.  What the rows then do as a body is checked against smplx_attach_body with the judge's rows on a second space:
the same nodes, verdicts, lookup tallies and searches (smplx_attach_body itself: tests/test_gpu_attached_bodies.py)."""
import numpy as np
import pytest

import object_cases as OC
from test_gpu_attached_bodies import SEARCH, _edges, _space, _states, _touch, _wrist

pytestmark = pytest.mark.gpu


def _shapes(keys):
    return [OC.shape(k) for k in keys]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the sphere rows
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def probe(small_cfg):
    return _space(small_cfg, "small")


@pytest.mark.parametrize("keys", [[k] for k in OC.SINGLE] + [["box", "cyl"]], ids=lambda k: "+".join(k))
def test_sphere_rows_equal_the_judge(probe, keys):
    want, first = OC.judged_rows(keys)            # asserts that nothing is undecided
    got, gfirst = probe.object_spheres(_shapes(keys))
    assert list(gfirst) == list(first)
    assert len(got) == sum(OC.CASES[k][1] for k in keys)
    assert OC.same_bits(got, want)
    assert probe.attached_bodies() == []          # the call changes nothing


def test_sphere_rows_cap_and_radius(probe):
    """a buffer smaller than the list gets its first rows; another radius moves the lattice with it"""
    import ctypes as C
    from smpl_amd import capi
    L = capi.lib()
    want, first = OC.judged_rows(["box", "cyl"])
    arr, n, keep = capi._shape_array(_shapes(["box", "cyl"]))
    L.smplx_object_spheres.argtypes = [C.c_void_p, C.POINTER(capi.ShapeStruct), C.c_int, C.c_double, capi._dp, C.c_int, capi._ip]
    f = np.zeros(3, np.int32)
    few = np.zeros((130, 4))
    assert L.smplx_object_spheres(probe.h, arr, n, OC.RADIUS, capi._p(few, capi._dp), 130, capi._p(f, capi._ip)) == 0
    assert list(f) == list(first) and OC.same_bits(few, want[:130])
    assert L.smplx_object_spheres(probe.h, arr, n, OC.RADIUS, None, 0, capi._p(f, capi._ip)) == 0 and list(f) == list(first)
    import voxelize_ref as V
    r = 0.02
    cells, und = V.voxelize_shape(OC.shape("box"), (0.0, 0.0, 0.0), r / np.sqrt(2.0), None, eps=1e-6)
    assert len(und) == 0
    got, _ = probe.object_spheres(_shapes(["box"]), radius=r)
    assert OC.same_bits(got, OC.rows_of(cells, r))


def test_the_rows_work_space_across_radii(small_cfg):
    """A space keeps one work space for these calls: the voxeliser's arrays first, then the sphere rows, and the block only
    grows (object_sphere_rows.h).  A flat triangle on a new space at a large radius, at a small one and at the large one
    again: at the small radius the rows (32 bytes a filled voxel) outgrow the voxeliser's seven arrays -- one triangle,
    one chunk and a mask of one byte per voxel of the vertices' index range, each rounded up to 256 bytes -- so the middle
    call replaces the block between its two uses, and the last call runs inside a block larger than it needs.  Each
    result equals the judge's, bit for bit."""
    import voxelize_ref as V
    s = OC._shape(V.MESH, (), vertices=np.array([(0.2013, 0.0007, 0.0013), (0.2613, 0.0007, 0.0013), (0.2013, 0.0507, 0.0013)]),
                  triangles=np.array([(0, 1, 2)]))
    want = {}
    for r in (0.025, 0.004):
        res = r / np.sqrt(2.0)
        cells, und = V.voxelize_shape(s, (0.0, 0.0, 0.0), res, None, eps=1e-6)
        assert len(und) == 0 and len(cells) > 0
        want[r] = OC.rows_of(cells, r)
        v = np.asarray(s["vertices"])
        mask = int(np.prod(np.floor(v.max(0) / res) - np.floor(v.min(0) / res) + 3))     # a bound: two voxels to spare an axis
        assert mask <= 8 * 256                                                           # one chunk
        voxeliser = 6 * 256 + (mask + 255) // 256 * 256
        print(f"radius {r}: {len(cells)} rows = {32 * len(cells)} bytes, the voxeliser's arrays at most {voxeliser}")
        assert (32 * len(cells) > voxeliser) == (r == 0.004)
    probe = _space(small_cfg, "small")
    for r in (0.025, 0.004, 0.025):
        got, first = probe.object_spheres([s], radius=r)
        assert list(first) == [0, len(want[r])] and OC.same_bits(got, want[r]), r


# ---------------------------------------------------------------------------------------------------------------------
# 2. the body's nodes
# ---------------------------------------------------------------------------------------------------------------------

def _pair_of_spaces(cfg, kind, shapes, rows):
    """one space holding the object attached by shape, one holding the judge's rows attached as spheres"""
    link, touch = _wrist(cfg), _touch(cfg)
    a, b = _space(cfg, kind), _space(cfg, kind)
    a.attach_object("held", link, shapes, allowed=touch)
    b.attach_body("held", link, rows, allowed=touch)
    return a, b


def _same_nodes(a, b):
    assert a.attached_bodies() == b.attached_bodies()
    (xa, la, ra), (xb, lb, rb) = a.attached_nodes(), b.attached_nodes()
    assert OC.same_bits(xa, xb) and np.array_equal(la, lb) and np.array_equal(ra, rb)


def test_body_nodes_equal_attach_body(small_cfg):
    rows, _ = OC.judged_rows(["box", "cyl"])
    a, b = _pair_of_spaces(small_cfg, "small", _shapes(["box", "cyl"]), rows)
    _same_nodes(a, b)
    assert a.attached_bodies() == [dict(id="held", link=_wrist(small_cfg), first=0, count=2 * 272 - 1)]
    Q = _states(small_cfg, 64, 17)
    assert OC.same_bits(a.attached_positions(Q), b.attached_positions(Q))


# ---------------------------------------------------------------------------------------------------------------------
# 3. verdicts and lookup tallies
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["specialized", "generic"])
@pytest.mark.parametrize("cfg_name", ["small_cfg", "cfg3_pr2"])
def test_verdicts_equal_attach_body(request, cfg_name, kind):
    cfg = request.getfixturevalue(cfg_name)
    Q = _states(cfg, 4096, 4321)
    A, Bq = _edges(cfg, 1024, 77)
    # the object as placed, or shifted along x until the share of valid states lies inside (0.02, 0.98): a condition on
    # the input, like the judge's undecided set being empty
    for dx in (0.0, 0.05, 0.1, 0.15, 0.2, 0.3, -0.05, -0.1):
        shapes = [OC.shifted(s, dx) for s in _shapes(["box", "cyl"])]
        try:
            rows = np.vstack([OC.judged_shape_rows(s) for s in shapes])
        except AssertionError:
            continue
        a, b = _pair_of_spaces(cfg, kind, shapes, rows)
        ok, lk = a.state_valid_batch(Q)
        if 0.02 < ok.astype(bool).mean() < 0.98:
            break
    else:
        pytest.fail("no placement of the object leaves between 2 % and 98 % of the states valid")
    _same_nodes(a, b)
    ok2, lk2 = b.state_valid_batch(Q)
    assert np.array_equal(ok, ok2) and np.array_equal(lk, lk2)
    e, elk, ew = a.edge_valid_batch(A, Bq)
    e2, elk2, ew2 = b.edge_valid_batch(A, Bq)
    assert np.array_equal(e, e2) and np.array_equal(elk, elk2) and np.array_equal(ew, ew2)
    # the object changes verdicts: states the robot alone passes now fail
    ok0 = _space(cfg, kind).state_valid_batch(Q)[0].astype(bool)
    assert (ok0 & ~ok.astype(bool)).sum() > 20


# ---------------------------------------------------------------------------------------------------------------------
# 4. search
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", ["device", "host"])
def test_search_equals_attach_body(small_cfg, mode, monkeypatch):
    cfg = small_cfg
    rows, _ = OC.judged_rows(["rod"])
    monkeypatch.setenv("SMPLX_SEARCH", mode)
    a, b = _pair_of_spaces(cfg, "small", _shapes(["rod"]), rows)
    res = []
    for s in (a, b):
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        s.set_start(cfg.start)
        res.append(s.plan(*SEARCH))
    ra, rb = res
    assert ra["solved"] == rb["solved"]
    assert list(ra["path"]) == list(rb["path"]) and ra["cost"] == rb["cost"]
    assert np.array_equal(ra["expansion_log"], rb["expansion_log"]) and len(ra["expansion_log"]) > 0
    # the rod takes part in the checks: states the robot alone passes fail with it
    Q = _states(cfg, 2048, 9)
    ok0 = _space(cfg, "small").state_valid_batch(Q)[0].astype(bool)
    assert (ok0 & ~a.state_valid_batch(Q)[0].astype(bool)).sum() > 20


# ---------------------------------------------------------------------------------------------------------------------
# 5. the limit
# ---------------------------------------------------------------------------------------------------------------------

def test_an_object_over_the_limit_changes_nothing(small_cfg, monkeypatch):
    from smpl_amd import capi
    cfg = small_cfg
    assert OC.judged("big")[2] == 0
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    s = _space(cfg, "small")
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    sid = s.set_start(cfg.start)
    before = s.get_succs(sid)
    with pytest.raises(capi.SmplxError) as e:
        s.attach_object("big", _wrist(cfg), _shapes(["big"]), allowed=_touch(cfg))
    assert e.value.code == -3 and "1172" in str(e.value)
    assert s.attached_bodies() == [] and s.attached_nodes()[0].shape == (0, 4)
    after = s.get_succs(sid)                  # no SMPLX_E_STATE: the goal need not be set again
    assert len(before) == len(after)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    # what it would have attached can still be asked for
    got, first = s.object_spheres(_shapes(["big"]))
    assert list(first) == [0, 1172] and OC.same_bits(got, OC.judged("big")[1])
    # eight bodies: the ninth is refused with the count of its spheres in the text
    for k in range(8):
        s.attach_object(f"b{k}", _wrist(cfg), _shapes(["one_tri"]), allowed=_touch(cfg))
    with pytest.raises(capi.SmplxError) as e:
        s.attach_object("b8", _wrist(cfg), _shapes(["one_tri"]))
    assert e.value.code == -3 and "13 spheres" in str(e.value)
    assert len(s.attached_bodies()) == 8


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals, detach and attach again
# ---------------------------------------------------------------------------------------------------------------------

def test_refusals_and_reattach(small_cfg):
    import voxelize_ref as V
    from smpl_amd import capi
    cfg = small_cfg
    link, touch = _wrist(cfg), _touch(cfg)
    rows, _ = OC.judged_rows(["box"])
    s, ref = _pair_of_spaces(cfg, "small", _shapes(["box"]), rows)
    box = OC.shape("box")
    unknown = dict(box, type=9)
    bad_index = dict(OC.shape("tet"), triangles=np.array([(0, 1, 4)]))
    non_finite = dict(box, dims=(0.06, float("nan"), 0.1))
    flat = dict(box, dims=(0.06, 0.0, 0.1))
    cases = {
        "a duplicate id": lambda: s.attach_object("held", link, [box], allowed=touch),
        "an unknown link": lambda: s.attach_object("x", "no_such_link", [box]),
        "a link outside the group": lambda: s.attach_object("x", "base_link", [box]),
        "radius 0": lambda: s.attach_object("x", link, [box], radius=0.0),
        "radius nan": lambda: s.attach_object("x", link, [box], radius=float("nan")),
        "a negative radius": lambda: s.attach_object("x", link, [box], radius=-0.025),
        "an unknown shape type": lambda: s.attach_object("x", link, [unknown]),
        "a mesh index out of range": lambda: s.attach_object("x", link, [bad_index]),
        "a non-finite dimension": lambda: s.attach_object("x", link, [non_finite]),
        "a dimension of 0": lambda: s.attach_object("x", link, [flat]),
        "no shape": lambda: s.attach_object("x", link, []),
        "a degenerate mesh that makes no sphere": lambda: s.attach_object("x", link, [OC.DEGENERATE]),
        "radius 0 for the rows alone": lambda: s.object_spheres([box], radius=0.0),
    }
    assert len(V.voxelize_shape(OC.DEGENERATE, (0.0, 0.0, 0.0), OC.RES, None)[0]) == 0
    for what, call in cases.items():
        with pytest.raises(capi.SmplxError) as e:
            call()
        assert e.value.code == -1, what
        _same_nodes(s, ref)                    # a refused call changes nothing
    # the rows of a shape that makes no sphere: an empty list, not an error
    got, first = s.object_spheres([OC.DEGENERATE, box])
    assert list(first) == [0, 0, 122] and OC.same_bits(got, rows)
    # detach serves an object attached by shape; the id is free again
    s.detach_body("held")
    assert s.attached_bodies() == []
    with pytest.raises(capi.SmplxError) as e:
        s.detach_body("held")
    assert e.value.code == -1
    s.attach_object("held", link, [box], allowed=touch)
    _same_nodes(s, ref)
    Q = _states(cfg, 512, 5)
    for x, y in zip(s.state_valid_batch(Q), ref.state_valid_batch(Q)):
        assert np.array_equal(x, y)
