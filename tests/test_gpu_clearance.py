"""Clearance queries on the GPU (smplx_cc_state_clearance_batch, _device, smplx_cc_edge_clearance_batch; DESIGN.md
section 16): distance to collision of states and edges with its two parts and a witness.

The reference's collisionDistance is unfinished, so the judge is the plain numpy model of tests/clearance_ref.py: brute
force over the engine's own sphere positions, the arithmetic in the specified order.  Every value is compared bit for bit
(float64 viewed as int64), never with a tolerance.  Edges are compared with the state query over the waypoints
smplx_cc_interpolate returns.
"""
import numpy as np
import pytest

import clearance_ref as ref
from smpl_amd import scenes

pytestmark = pytest.mark.gpu

BUILDS = ["specialized", "generic"]
N_STATES, N_EDGES, SEED = 3000, 300, 99
SLACK = 1e-9


def _capi():
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return capi


def _space(cfg, kind, padding=0.0):
    return _capi().Space.from_config(cfg, no_small_kernel=True, generic_kernels=(kind == "generic"), padding=padding)


def _model(cfg, s, padding=0.0, allowed=None, grid=None):
    capi = _capi()
    g = grid or cfg.grid
    bodies = s.attached_bodies()
    return ref.ClearanceModel(cfg.robot_text, capi.Model(cfg.robot_text).arrays(), s.grid.d2(), g.origin, g.res, padding,
                              bodies, s.attached_nodes() if bodies else None, allowed)


def _states(n=N_STATES, seed=SEED):
    return scenes.random_states(scenes.ARM7_LIMITS, n, seed)


def _wrist(cfg):
    return "r_gripper_palm_link" if "link r_gripper_palm_link" in cfg.robot_text else "gripper_palm_link"


def _touch(cfg):
    w = _wrist(cfg)
    return [w] + [l.split()[1] for l in cfg.robot_text.splitlines() if l.startswith("link ") and "finger" in l]


def _box(center, size, pitch, r):
    axes = [np.arange(-s / 2 + pitch / 2, s / 2, pitch) + c for c, s in zip(center, size)]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    return np.hstack([g, np.full((len(g), 1), r)])


@pytest.fixture(params=["small_cfg", "cfg3_pr2"])
def cfg(request):
    return request.getfixturevalue(request.param)


# the brute-force answer for the body-free robot of a configuration, worked out once per scene and shared
_EXPECTED = {}


def _expected(cfg, s, Q):
    if cfg.name not in _EXPECTED:
        P = s.sphere_positions(Q)
        c, p = _model(cfg, s).evaluate(P)
        for a in (P, c, p):
            a.setflags(write=False)
        _EXPECTED[cfg.name] = (P, c, p)
    return _EXPECTED[cfg.name]


# ---------------------------------------------------------------------------------------------------------------------
# 1. states against brute force; 2. the two builds agree; 3. validity, one direction
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BUILDS)
def test_states_equal_brute_force(cfg, kind):
    s = _space(cfg, kind)
    assert s.specialized()[0] == (kind == "specialized"), s.specialized()[1]
    Q = _states()
    c, p, w = s.state_clearance_batch(Q)
    P, exp_c, exp_p = _expected(cfg, s, Q)
    assert np.array_equal(s.sphere_positions(Q), P)
    share = float((c < 0).mean())
    print(f"{cfg.name} {kind}: clearance < 0 in {share:.3f} of the rows; min {c.min():.6f} max {c.max():.6f}; "
          f"witness kinds {sorted(set(w[:, 0].tolist()))}")
    got_c, got_p = ref.check_against_model(_model(cfg, s), P, None, c, p, w)
    assert np.array_equal(ref.bits(got_c), ref.bits(exp_c)) and np.array_equal(ref.bits(got_p), ref.bits(exp_p))
    assert (w[:, 3] == 0).all()                     # a state has waypoint 0
    assert 0.02 < share < 0.98                      # neither side is empty: the comparison is not vacuous
    assert set(w[:, 0].tolist()) <= {0, 1}          # no bodies: robot leaf against the world or against a robot leaf


def test_builds_agree_bit_for_bit(cfg):
    Q = _states()
    A, B = _edges(cfg, 60, 7)
    outs = []
    for kind in BUILDS:
        s = _space(cfg, kind)
        outs.append(s.state_clearance_batch(Q)[:2] + s.edge_clearance_batch(A, B)[:2])
    for x, y in zip(*outs):
        assert np.array_equal(ref.bits(x), ref.bits(y))


def test_clearance_implies_valid(cfg):
    s = _space(cfg, "specialized")
    Q = _states()
    c = s.state_clearance_batch(Q)[0]
    ok = s.state_valid_batch(Q)[0].astype(bool)
    clear = c > SLACK
    assert ok[clear].all()
    assert clear.sum() >= 20 and (~clear).sum() >= 20
    A, B = _edges(cfg, N_EDGES, 11)
    ce = s.edge_clearance_batch(A, B)[0]
    oke = s.edge_valid_batch(A, B)[0].astype(bool)
    print("edges with clearance above the slack:", int((ce > SLACK).sum()), "of", len(ce))
    assert oke[ce > SLACK].all() and (ce > SLACK).any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. padding; 5. the cap and the outside of the grid
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BUILDS)
def test_padding_moves_the_world_part_only(small_cfg, kind):
    cfg = small_cfg
    s, s0 = _space(cfg, kind, padding=0.03), _space(cfg, kind)
    Q = _states()
    c, p, w = s.state_clearance_batch(Q)
    P = s.sphere_positions(Q)
    ref.check_against_model(_model(cfg, s, padding=0.03), P, None, c, p, w)
    p0 = s0.state_clearance_batch(Q)[1]
    assert np.array_equal(ref.bits(p[:, 1]), ref.bits(p0[:, 1]))       # self pairs are not padded
    assert (p[:, 0] < p0[:, 0]).all()


def _space_on_grid(cfg, grid_spec, padding, kind="specialized"):
    capi = _capi()
    origin, dims, res, max_dist = grid_spec
    g = capi.Grid.empty(origin, dims, res, max_dist)
    s = capi.Space(capi.Model(cfg.robot_text), g, cfg.mprim, cfg.params, no_small_kernel=True,
                   generic_kernels=(kind == "generic"), padding=padding)
    return s, scenes.Grid(origin, dims, res, max_dist, None)


def test_outside_the_grid_and_at_the_cap(small_cfg):
    cfg = small_cfg
    Q = _states()
    pad = 0.01
    # (a) a 16^3 grid of 4 cm cells around the shoulder: most of the arm is outside it
    s, g = _space_on_grid(cfg, ((-0.1, -0.5, 0.6), (16, 16, 16), 0.04, 0.2), pad)
    m = _model(cfg, s, padding=pad, grid=g)
    c, p, w = s.state_clearance_batch(Q)
    P = s.sphere_positions(Q)
    ref.check_against_model(m, P, None, c, p, w)
    cells = scenes.world_to_grid(np.array(g.origin), g.res, P)
    outside = ~np.all((cells >= 0) & (cells < 16), axis=-1)
    leaf = m.left < 0
    assert outside[:, leaf].any() and (~outside[:, leaf]).any()
    # a row whose witness sphere is outside has exactly -(r + pad)
    rows = np.arange(len(Q))[w[:, 0] == 0]
    wout = rows[outside[rows, w[rows, 1]]]
    assert len(wout) > 100
    assert np.array_equal(ref.bits(c[wout]), ref.bits(-(m.xyzr[w[wout, 1], 3] + pad)))
    # (b) an empty 64^3 grid whose field stops at 0.2 m: spheres in the interior sit at the cap
    s, g = _space_on_grid(cfg, ((0.3 - 1.28, -0.188 - 1.28, 0.8 - 1.28), (64, 64, 64), 0.04, 0.2), pad)
    m = _model(cfg, s, padding=pad, grid=g)
    c, p, w = s.state_clearance_batch(Q)
    P = s.sphere_positions(Q)
    ref.check_against_model(m, P, None, c, p, w)
    dmax_sqrd = int(m.d2.max())
    cap = g.res * np.sqrt(np.float64(dmax_sqrd)) - (m.xyzr[leaf, 3].max() + pad)     # the largest leaf at the cap
    at_cap = ref.bits(p[:, 0]) == ref.bits(np.full(len(Q), cap))
    print("rows whose world part is the cap value:", int(at_cap.sum()))
    assert at_cap.sum() > 100 and (p[:, 0] <= cap).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. attached bodies
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BUILDS)
def test_attached_bodies(small_cfg, kind):
    cfg = small_cfg
    link, touch = _wrist(cfg), _touch(cfg)
    Q = _states()
    held = _box((0.25, 0.0, 0.0), (0.06, 0.06, 0.06), 0.02, 0.015)
    second = _box((0.27, 0.0, 0.02), (0.04, 0.04, 0.04), 0.02, 0.015)
    near = _box((0.05, 0.0, 0.0), (0.04, 0.04, 0.04), 0.02, 0.02)
    s = _space(cfg, kind)
    free = s.state_clearance_batch(Q)
    kinds = set()
    scenes_ = [
        [("a", held, touch)],                                       # the held box with its touch links
        [("a", held, touch), ("b", second, touch)],                 # a second body overlapping it: the pair is checked
        [("a", held, touch), ("b", second, touch + ["a"])],         # ... unless one lists the other
        [("near", near, [])],                                       # no allowed links: checked against its own link too
        [("a", held, touch), ("near", near, []), ("far", _box((0.45, 0.0, 0.0), (0.04, 0.04, 0.04), 0.02, 0.015), touch)],
    ]
    for bodies in scenes_:
        for bid, sp, allowed in bodies:
            s.attach_body(bid, link, sp, allowed=allowed)
        m = _model(cfg, s, allowed=[b[2] for b in bodies])
        c, p, w = s.state_clearance_batch(Q)
        P, B = s.sphere_positions(Q), s.attached_positions(Q)
        ref.check_against_model(m, P, B, c, p, w)
        seen = set(w[:, 0].tolist())
        print([b[0] for b in bodies], "witness kinds", sorted(seen))
        kinds |= seen
        assert (c <= free[0]).all()
        if len(bodies) == 2:
            assert (4 in seen) == ("a" not in bodies[1][2])
        for bid, _, _ in bodies:
            s.detach_body(bid)
    assert {2, 3, 4} <= kinds
    for x, y in zip(s.state_clearance_batch(Q), free):                # detached: the body-free values again
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------------------------------------
# 7. edges
# ---------------------------------------------------------------------------------------------------------------------

def _edges(cfg, n, seed):
    """short edges (few waypoints), longer ones, start -> goal, state -> state across the whole range, and a == b"""
    rng = np.random.default_rng(seed + 1)
    A = _states(n, seed)
    scale = np.where(np.arange(n) % 2 == 0, 0.02, 0.15)[:, None]
    B = A + rng.uniform(-1.0, 1.0, A.shape) * scale
    k = min(8, n // 6)
    B[:k] = _states(k, seed + 2)                     # long: anywhere to anywhere
    A[k], B[k] = cfg.start, cfg.goal
    B[k + 1:2 * k + 1] = A[k + 1:2 * k + 1]           # no motion
    return A, B


@pytest.mark.parametrize("kind", BUILDS)
def test_edges_equal_the_minimum_over_their_waypoints(cfg, kind):
    s = _space(cfg, kind)
    A, B = _edges(cfg, N_EDGES, 5)
    c, p, w = s.edge_clearance_batch(A, B)
    pts, off, W = [], [0], []
    for a, b in zip(A, B):
        x, n = s.interpolate(a, b)
        assert n <= 4096
        W.append(n)
        pts.append(x if n else a[None])               # an edge without motion: its start configuration alone
        off.append(off[-1] + len(pts[-1]))
    W, off = np.array(W), np.array(off)
    print("waypoint counts: none", int((W == 0).sum()), "up to 5:", int(((W > 0) & (W <= 5)).sum()), "more:", int((W > 5).sum()),
          "largest", int(W.max()))
    assert (W == 0).sum() >= 5 and ((W > 0) & (W <= 5)).sum() >= 20 and (W > 5).sum() >= 20
    assert np.array_equal(W, s.edge_valid_batch(A, B)[2])
    cs, ps, ws = s.state_clearance_batch(np.vstack(pts))
    exp_c = np.minimum.reduceat(cs, off[:-1])
    exp_p = np.stack([np.minimum.reduceat(ps[:, 0], off[:-1]), np.minimum.reduceat(ps[:, 1], off[:-1])], 1)
    assert np.array_equal(ref.bits(c), ref.bits(exp_c))
    assert np.array_equal(ref.bits(p), ref.bits(exp_p))
    assert np.array_equal(ref.bits(c), ref.bits(np.minimum(p[:, 0], p[:, 1])))
    # the witness: its waypoint is one of the edge's, and that waypoint's own part of the witness's kind is the clearance
    assert (w[:, 3] >= 0).all() and (w[:, 3] < np.maximum(W, 1)).all()
    at = off[:-1] + w[:, 3]
    part = np.where(np.isin(w[:, 0], (0, 2)), ps[at, 0], ps[at, 1])
    assert np.array_equal(ref.bits(part), ref.bits(c))
    assert np.array_equal(ref.bits(cs[at]), ref.bits(c))
    # a == b: the state query of a, waypoint 0
    still = W == 0
    c0, p0, w0 = s.state_clearance_batch(A[still])
    assert np.array_equal(ref.bits(c[still]), ref.bits(c0)) and np.array_equal(ref.bits(p[still]), ref.bits(p0))
    assert np.array_equal(w[still], w0)
    assert 0 < (c < 0).sum() < len(c)


# ---------------------------------------------------------------------------------------------------------------------
# 8. device pointers; 9. every joint kind; the call contract
# ---------------------------------------------------------------------------------------------------------------------

def test_device_pointer_form(small_cfg):
    import ctypes as C
    s = _space(small_cfg, "specialized")
    Q = np.ascontiguousarray(_states())
    n = Q.shape[0]
    c, p, w = s.state_clearance_batch(Q)
    hip = C.CDLL("libamdhip64.so")
    ptrs = [C.c_void_p() for _ in range(5)]          # q, clearance, parts, witness, clearance of the second call
    sizes = (Q.nbytes, 8 * n, 16 * n, 16 * n, 8 * n)
    for pp, nb in zip(ptrs, sizes):
        assert hip.hipMalloc(C.byref(pp), C.c_size_t(nb)) == 0
    try:
        assert hip.hipMemcpy(ptrs[0], Q.ctypes.data_as(C.c_void_p), C.c_size_t(Q.nbytes), 1) == 0
        s.state_clearance_batch_device(ptrs[0].value, n, ptrs[1].value, ptrs[2].value, ptrs[3].value, None)
        s.state_clearance_batch_device(ptrs[0].value, n, ptrs[4].value, None, None, None)     # parts and witness left out
        assert hip.hipDeviceSynchronize() == 0
        dc, dp, dw, dc2 = np.zeros(n), np.zeros((n, 2)), np.zeros((n, 4), np.int32), np.zeros(n)
        for host, dev, nb in zip((dc, dp, dw, dc2), ptrs[1:], sizes[1:]):
            assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), dev, C.c_size_t(nb), 2) == 0
    finally:
        for pp in ptrs:
            hip.hipFree(pp)
    assert np.array_equal(ref.bits(dc), ref.bits(c)) and np.array_equal(ref.bits(dp), ref.bits(p))
    assert np.array_equal(dw, w) and np.array_equal(ref.bits(dc2), ref.bits(c))


@pytest.mark.parametrize("kind", BUILDS)
def test_mixed_joint_kinds(kind):
    cfg = scenes.config_mixed()
    s = _space(cfg, kind)
    Q = scenes.random_states(scenes.MIXED_LIMITS, 1000, 17)
    c, p, w = s.state_clearance_batch(Q)
    ref.check_against_model(_model(cfg, s), s.sphere_positions(Q), None, c, p, w)
    assert 0 < (c < 0).sum() < len(c)
    A = Q[:100]
    B = A + np.random.default_rng(3).uniform(-0.2, 0.2, A.shape) * np.array([1, 0.2, 1, 1, 1])
    ce, pe, we = s.edge_clearance_batch(A, B)
    for i in range(len(A)):
        pts, n = s.interpolate(A[i], B[i])
        cs = s.state_clearance_batch(pts)[0]
        assert ref.bits(ce[i:i + 1])[0] == ref.bits(cs.min(keepdims=True))[0], i
        assert ref.bits(cs[we[i, 3]:we[i, 3] + 1])[0] == ref.bits(ce[i:i + 1])[0]


def test_call_contract(small_cfg):
    capi = _capi()
    s = _space(small_cfg, "specialized")
    c, p, w = s.state_clearance_batch(np.zeros((0, 7)))
    assert c.shape == (0,) and p.shape == (0, 2) and w.shape == (0, 4)
    assert s.edge_clearance_batch(np.zeros((0, 7)), np.zeros((0, 7)))[0].shape == (0,)
    bad = np.array(small_cfg.start, float)
    for v in (np.nan, np.inf, 1e6):
        x = bad.copy(); x[3] = v
        for call in (lambda: s.state_clearance_batch(x), lambda: s.edge_clearance_batch(bad, x),
                     lambda: s.edge_clearance_batch(x, bad)):
            with pytest.raises(capi.SmplxError) as e:
                call()
            assert e.value.code == -1 and "finite" in str(e.value)
    # no goal, a grid edit and an attach later: still answered (a field built on the GPU can be edited)
    cfg = small_cfg
    g = capi.Grid.from_boxes(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.boxes)
    s = capi.Space(capi.Model(cfg.robot_text), g, cfg.mprim, cfg.params, no_small_kernel=True)
    before = s.state_clearance_batch(_states(200))[0]
    s.grid.add_boxes([((0.6, 0.0, 0.9), (0.1, 0.1, 0.1))])
    assert (s.state_clearance_batch(_states(200))[0] < before).any()
    s.attach_body("box", _wrist(small_cfg), _box((0.25, 0.0, 0.0), (0.06, 0.06, 0.06), 0.02, 0.015), allowed=_touch(small_cfg))
    c, p, w = s.state_clearance_batch(_states(200))
    ref.check_against_model(_model(small_cfg, s, allowed=[_touch(small_cfg)]), s.sphere_positions(_states(200)),
                            s.attached_positions(_states(200)), c, p, w)


# ---------------------------------------------------------------------------------------------------------------------
# 10. a search that is resumed across a clearance call
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", ["device", "host"])
def test_searches_undisturbed(small_cfg, side, monkeypatch):
    monkeypatch.setenv("SMPLX_SEARCH", side)
    capi = _capi()
    cfg = small_cfg
    Q = _states()
    runs = []
    for with_query in (False, True):
        s = capi.Space.from_config(cfg, batch_states=256)
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        s.set_start(cfg.start)
        a = s.replan(5.0, 1.0, 1.0, False, True, 150, 150)
        if with_query:
            c = s.state_clearance_batch(Q)[0]
            assert np.isfinite(c).all()
            s.edge_clearance_batch(Q[:50], Q[50:100])
        b = s.replan(5.0, 1.0, 1.0, False, True, 6000, 6000)
        runs.append((a, b))
    (a0, b0), (a1, b1) = runs
    assert a0["result"] == capi.ARA_TIMED_OUT and a0["call_expansions"] == 150
    assert b0["resumed"] == 1 and b1["resumed"] == 1 and b0["solved"] == 1
    for x, y in ((a0, a1), (b0, b1)):
        assert x["result"] == y["result"] and x["cost"] == y["cost"] and x["expansions"] == y["expansions"]
        assert list(x["path"]) == list(y["path"])
        assert np.array_equal(x["expansion_log"], y["expansion_log"])
