"""Collision bodies attached to robot links (smplx_attach_body; CollisionSpace::attachObject, collision_space.cpp:297-345).

The oracle has no attach call; a body on link L with L allowed is the same thing as a fixed pseudo-link under L that
carries the spheres, belongs to the group and has `acm` rows for the allowed links, so the unchanged oracle checks that
case.  What the pseudo-link cannot express (a body that may not touch its own link, body x body pairs, padding) is checked
against numpy brute force over the engine's own sphere positions: the grid rule of collision_operations.h:105-164 (a node
is looked at only when every ancestor fails, so "any leaf fails" would be wrong: the cell distance at a parent's centre
does not bound the cell distances at its leaves') and any-leaf overlap for the sphere pairs.  Expansion (pipeline,
fused, small-batch, generic kernels), both searches, detach, the call contract and the C++ boundary follow.
"""
import copy

import numpy as np
import pytest

from smpl_amd import scenes

pytestmark = pytest.mark.gpu

KINDS = ["pipeline", "fused", "small", "generic"]   # which expansion kernels serve the space (test_gpu_parity.py)
BUILDS = ["specialized", "generic"]                 # what the collision-only entry points (K2, edges) can differ in
F_VALID, F_INACTIVE, F_LIMITS = 1, 0x10, 0x20
SEARCH = (5.0, 1.0, 1.0, False, True, 6000, 6000)   # eps0, eps_final, eps_delta, improve, bounded, max_init, max_rep


def _space(cfg, kind, padding=0.0):
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    s = capi.Space.from_config(cfg, fused=(kind == "fused"), no_small_kernel=(kind in ("pipeline", "generic", "specialized")),
                               generic_kernels=(kind == "generic"), padding=padding)
    s.fused = kind == "fused"
    return s


def _wrist(cfg):
    return "r_gripper_palm_link" if "link r_gripper_palm_link" in cfg.robot_text else "gripper_palm_link"


def _touch(cfg):
    """the held object's touch links: the wrist link and the fingers"""
    w = _wrist(cfg)
    return [w] + [l.split()[1] for l in cfg.robot_text.splitlines() if l.startswith("link ") and "finger" in l]


def _box(center, size, pitch, r):
    """spheres on a regular grid filling a box (test data; not the reference's mesh voxeliser)"""
    axes = [np.arange(-s / 2 + pitch / 2, s / 2, pitch) + c for c, s in zip(center, size)]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    return np.hstack([g, np.full((len(g), 1), r)])


def _held_box():
    # in front of the fingers, 6 x 6 x 6 cm at 2 cm pitch
    return _box((0.25, 0.0, 0.0), (0.06, 0.06, 0.06), 0.02, 0.015)


def _oracle_text(robot_text, link, spheres, allowed):
    """the pseudo-link stand-in for the oracle: fixed joint at `link`, the spheres on a new link in the group"""
    out = []
    for line in robot_text.splitlines():
        if line.split()[:1] == ["group"]:
            line = line + " attached_body_link"
        out.append(line)
    out.append("link attached_body_link")
    out.append(f"joint attached_body_joint fixed {link} attached_body_link  0 0 0  0 0 0  0 0 1  0.0 0.0")
    for i, (x, y, z, r) in enumerate(spheres):
        out.append(f"sphere attached_body_link b{i} {float(x)!r} {float(y)!r} {float(z)!r} {float(r)!r} 0")
    for a in allowed:
        out.append(f"acm attached_body_link {a}")
    return "\n".join(out) + "\n"


def _oracle_with_body(cfg, link, spheres, allowed):
    from oracle_binding import Oracle
    c = copy.copy(cfg)
    c.robot_text = _oracle_text(cfg.robot_text, link, spheres, allowed)
    o = Oracle(c)
    o.set_order(chain=True)
    return o


def _states(cfg, n, seed):
    lim = scenes.ARM7_LIMITS
    return scenes.random_states(lim, n, seed)


@pytest.fixture(params=["small_cfg", "cfg3_pr2"])
def cfg(request):
    return request.getfixturevalue(request.param)


# ---------------------------------------------------------------------------------------------------------------------
# 1. oracle equivalence for states
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BUILDS)
def test_states_equal_oracle_pseudo_link(cfg, kind):
    link = _wrist(cfg)
    sp = _held_box()
    o = _oracle_with_body(cfg, link, sp, _touch(cfg))
    s = _space(cfg, kind)
    s.attach_body("box", link, sp, allowed=_touch(cfg))
    Q = _states(cfg, 1 << 14, 1234)
    ok, lk = s.state_valid_batch(Q)
    eok, elk, _ = o.state_valid_batch_timed(Q)
    ok, eok = ok.astype(bool), eok.astype(bool)
    assert np.array_equal(ok, eok)
    assert np.array_equal(lk[ok], elk[ok])
    assert 0.02 < ok.mean() < 0.98
    # the body changes verdicts: some states the robot alone passes now fail
    s2 = _space(cfg, kind)
    ok0, lk0 = s2.state_valid_batch(Q)
    assert (ok0.astype(bool) & ~ok).sum() > 20
    assert (lk[ok] > lk0[ok]).all()       # every valid state looked the body up
    _check_device_path(s, Q, eok, elk)


def _check_device_path(s, Q, eok, elk):
    """smplx_cc_state_valid_batch_device (the K2 form): HBM buffers from the HIP runtime, null stream"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    n = Q.shape[0]
    Q = np.ascontiguousarray(Q)
    ptrs = [C.c_void_p() for _ in range(3)]
    for pp, nb in zip(ptrs, (Q.nbytes, n, 4 * n)):
        assert hip.hipMalloc(C.byref(pp), C.c_size_t(nb)) == 0
    try:
        assert hip.hipMemcpy(ptrs[0], Q.ctypes.data_as(C.c_void_p), C.c_size_t(Q.nbytes), 1) == 0
        s.state_valid_batch_device(ptrs[0].value, n, ptrs[1].value, ptrs[2].value, None)
        assert hip.hipDeviceSynchronize() == 0
        v = np.zeros(n, np.uint8); lk = np.zeros(n, np.int32)
        assert hip.hipMemcpy(v.ctypes.data_as(C.c_void_p), ptrs[1], C.c_size_t(n), 2) == 0
        assert hip.hipMemcpy(lk.ctypes.data_as(C.c_void_p), ptrs[2], C.c_size_t(4 * n), 2) == 0
    finally:
        for pp in ptrs:
            hip.hipFree(pp)
    assert np.array_equal(v.astype(bool), eok)
    assert np.array_equal(lk[eok], elk[eok])



# ---------------------------------------------------------------------------------------------------------------------
# brute force over the engine's positions
# ---------------------------------------------------------------------------------------------------------------------

class Brute:
    """the bodies' part of a verdict; the robot's own part comes from a space without bodies (oracle-checked elsewhere)"""

    def __init__(self, cfg, s, padding=0.0):
        from smpl_amd import capi
        a = capi.Model(cfg.robot_text).arrays()
        self.rleft, self.rxyzr, self.first = a["left"], a["xyzr"], a["tree_first"]
        g = cfg.grid
        self.d2 = (g.res * np.sqrt(np.asarray(g.d2, np.float64))) ** 2      # sphere_threshold's (res sqrt(i))^2
        self.org, self.res, self.dims = np.array(g.origin, float), g.res, np.array(g.dims)
        self.s, self.pad = s, padding
        self.bodies = s.attached_bodies()
        self.bxyzr, self.bleft, bright = s.attached_nodes()
        self.bparent = -np.ones(len(self.bleft), int)
        for i in range(len(self.bleft)):
            if self.bleft[i] >= 0:
                self.bparent[self.bleft[i]] = i
                self.bparent[bright[i]] = i

    def _grid_sq(self, p):
        c = scenes.world_to_grid(self.org, self.res, p)       # distance_map.hpp:520-536; outside the grid reads 0
        inside = np.all((c >= 0) & (c < self.dims), axis=-1)
        cc = np.clip(c, 0, self.dims - 1)
        return np.where(inside, self.d2[cc[..., 0], cc[..., 1], cc[..., 2]], 0.0)

    def valid(self, Q, tree_allowed, body_allowed):
        """tree_allowed[b]: robot tree indices body b may touch; body_allowed: allowed (b, c) pairs.  Returns the verdict
        of the bodies and a mask of states with a sphere pair within 1e-9 of touching (rounding decides those)"""
        Q = np.asarray(Q, np.float64).reshape(-1, self.s.N)
        P = self.s.sphere_positions(Q)
        B = self.s.attached_positions(Q)
        n = Q.shape[0]
        ok = np.ones(n, bool)
        amb = np.zeros(n, bool)
        fail = self._grid_sq(B) < (self.bxyzr[:, 3] + self.pad) ** 2
        reached = np.ones_like(fail)
        for i in range(len(self.bleft)):
            j = self.bparent[i]
            while j >= 0:
                reached[:, i] &= fail[:, j]
                j = self.bparent[j]
        ok &= ~(fail & reached)[:, self.bleft < 0].any(1)

        def pair(pa, ra, pb, rb):
            dd = ((pa[:, :, None] - pb[:, None]) ** 2).sum(-1) - (ra[:, None] + rb[None]) ** 2
            return (dd <= 0).any((1, 2)), (np.abs(dd) < 1e-9).any((1, 2))
        leaves = []
        for k, bd in enumerate(self.bodies):
            idx = [i for i in range(bd["first"], bd["first"] + bd["count"]) if self.bleft[i] < 0]
            leaves.append(idx)
            for t in range(len(self.first) - 1):
                if t in tree_allowed[k]:
                    continue
                lt = [i for i in range(self.first[t], self.first[t + 1]) if self.rleft[i] < 0]
                hit, a = pair(B[:, idx], self.bxyzr[idx, 3], P[:, lt], self.rxyzr[lt, 3])
                ok &= ~hit
                amb |= a
        for k in range(len(self.bodies)):
            for c in range(k + 1, len(self.bodies)):
                if (k, c) in body_allowed or (c, k) in body_allowed:
                    continue
                hit, a = pair(B[:, leaves[k]], self.bxyzr[leaves[k], 3], B[:, leaves[c]], self.bxyzr[leaves[c], 3])
                ok &= ~hit
                amb |= a
        return ok, amb


def _tree_links(cfg):
    """the link of each sphere tree, in tree order (group order of the links with spheres)"""
    from smpl_amd import capi
    a = capi.Model(cfg.robot_text).arrays()
    group = [l for l in cfg.robot_text.splitlines() if l.startswith("group")][0].split()[2:]
    with_spheres = {l.split()[1] for l in cfg.robot_text.splitlines() if l.startswith("sphere")}
    links = [g for g in group if g in with_spheres]
    assert len(links) == len(a["tree_first"]) - 1
    return links


def _touch_trees(cfg):
    links = _tree_links(cfg)
    return {links.index(x) for x in _touch(cfg) if x in links}


# ---------------------------------------------------------------------------------------------------------------------
# 2. brute force for what the oracle cannot express
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", BUILDS)
def test_bodies_against_brute_force(cfg, kind):
    link = _wrist(cfg)
    links = _tree_links(cfg)
    Q = _states(cfg, 3000, 99)
    robot_ok = _space(cfg, kind).state_valid_batch(Q)[0].astype(bool)
    # (a) no allowed links: the body is checked against its own link too
    near = _box((0.05, 0.0, 0.0), (0.04, 0.04, 0.04), 0.02, 0.02)
    s = _space(cfg, kind)
    s.attach_body("near", link, near)
    ok = s.state_valid_batch(Q)[0].astype(bool)
    exp, amb = Brute(cfg, s).valid(Q, [set()], set())
    exp &= robot_ok
    assert np.array_equal(ok[~amb], exp[~amb])
    s.detach_body("near")
    s.attach_body("near", link, near, allowed=links)
    ok_all = s.state_valid_batch(Q)[0].astype(bool)
    exp2, amb2 = Brute(cfg, s).valid(Q, [set(range(len(links)))], set())
    exp2 &= robot_ok
    assert np.array_equal(ok_all[~amb2], exp2[~amb2])
    assert (ok_all & ~ok).any(), "the body's own link makes a difference"
    # (b) two bodies that overlap each other: checked unless one lists the other
    for acm in (False, True):
        s = _space(cfg, kind)
        s.attach_body("a", link, _held_box(), allowed=_touch(cfg))
        s.attach_body("b", link, _box((0.27, 0.0, 0.02), (0.04, 0.04, 0.04), 0.02, 0.015), allowed=_touch(cfg) + (["a"] if acm else []))
        ok = s.state_valid_batch(Q)[0].astype(bool)
        tt = _touch_trees(cfg)
        exp, amb = Brute(cfg, s).valid(Q, [tt, tt], {(0, 1)} if acm else set())
        exp &= robot_ok
        assert np.array_equal(ok[~amb], exp[~amb]), acm
        assert ok.any() == acm
    # (c) padding > 0: the grid checks grow by it (self pairs are not padded, self_collision_model.cpp:1124-1130)
    s = _space(cfg, kind, padding=0.03)
    s.attach_body("box", link, _held_box(), allowed=_touch(cfg))
    ok = s.state_valid_batch(Q)[0].astype(bool)
    exp, amb = Brute(cfg, s, padding=0.03).valid(Q, [_touch_trees(cfg)], set())
    exp &= _space(cfg, kind, padding=0.03).state_valid_batch(Q)[0].astype(bool)
    assert np.array_equal(ok[~amb], exp[~amb])
    assert 0.01 < ok.mean() < 0.99


# ---------------------------------------------------------------------------------------------------------------------
# 3. edges
# ---------------------------------------------------------------------------------------------------------------------

def _edges(cfg, n, seed):
    A = _states(cfg, n, seed)
    return A, A + np.random.default_rng(seed + 1).uniform(-0.15, 0.15, A.shape)


@pytest.mark.parametrize("kind", BUILDS)
def test_edges_with_body(cfg, kind):
    link = _wrist(cfg)
    s, s0 = _space(cfg, kind), _space(cfg, kind)
    A, Bq = _edges(cfg, 300, 5)
    w0 = [s0.interpolate(a, b)[1] for a, b in zip(A[:50], Bq[:50])]
    s.attach_body("box", link, _held_box(), allowed=_touch(cfg))
    w1 = [s.interpolate(a, b)[1] for a, b in zip(A[:50], Bq[:50])]
    assert w0 == w1
    ok, _, W = s.edge_valid_batch(A, Bq)
    ok0, _, W0 = s0.edge_valid_batch(A, Bq)
    assert np.array_equal(W, W0)
    b = Brute(cfg, s)
    checked = 0
    for i in range(A.shape[0]):
        pts, n = s.interpolate(A[i], Bq[i])
        if n == 0:
            continue
        exp, amb = b.valid(pts, [_touch_trees(cfg)], set())
        if amb.any():
            continue
        exp &= s0.state_valid_batch(pts)[0].astype(bool)
        assert bool(ok[i]) == bool(exp.all()), i
        checked += 1
    assert checked > 200 and 0 < ok.sum() < len(ok)
    assert (ok0.astype(bool) & ~ok.astype(bool)).any()


# ---------------------------------------------------------------------------------------------------------------------
# expansion: every kernel variant sees the body
# ---------------------------------------------------------------------------------------------------------------------

def test_expansion_kernels_with_body(small_cfg):
    cfg = small_cfg
    link = _wrist(cfg)
    Q = _states(cfg, 4000, 8)
    probe = _space(cfg, "generic")
    probe.attach_body("box", link, _held_box(), allowed=_touch(cfg))
    parents = Q[probe.state_valid_batch(Q)[0].astype(bool)][:300]     # 300: the pipeline; small batches below
    outs = {}
    for kind in KINDS:
        s = _space(cfg, kind)
        s.attach_body("box", link, _held_box(), allowed=_touch(cfg))
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        outs[kind] = [s.expand_batch(parents), s.expand_batch(parents[:40])]
    ref = outs["generic"][0]
    for kind in KINDS:
        for big, small in ((outs[kind][0], None), (outs[kind][1], 40)):
            want = ref if small is None else {k: v[:small] for k, v in ref.items()}
            assert np.array_equal(big["flags"], want["flags"]), kind
            v = big["flags"] & F_VALID != 0
            assert np.array_equal(big["coord"][v], want["coord"][v]) and np.array_equal(big["cost"][v], want["cost"][v]), kind
    # the verdicts are the edge checks' (k_edge_valid, checked against brute force above)
    f, sq = ref["flags"], ref["q"]
    act = (f & (F_INACTIVE | F_LIMITS)) == 0
    pi, mi = np.nonzero(act)
    ev, _, _ = probe.edge_valid_batch(parents[pi], sq[pi, mi])
    assert np.array_equal(ev.astype(bool), (f[pi, mi] & F_VALID) != 0)
    s0 = _space(cfg, "generic")
    s0.set_goal_joint(cfg.goal, cfg.goal_tol)
    f0 = s0.expand_batch(parents)["flags"]
    assert ((f0 & F_VALID != 0) & (f & F_VALID == 0)).sum() > 5      # the body removes successors


# ---------------------------------------------------------------------------------------------------------------------
# 4. detach
# ---------------------------------------------------------------------------------------------------------------------

def test_detach_restores_everything(small_cfg):
    cfg = small_cfg
    link = _wrist(cfg)
    s, s0 = _space(cfg, "small"), _space(cfg, "small")
    s.attach_body("box", link, _held_box(), allowed=_touch(cfg))
    s.attach_body("box2", link, _box((0.0, 0.1, 0.0), (0.04, 0.04, 0.04), 0.02, 0.015))
    s.detach_body("box")
    assert [b["id"] for b in s.attached_bodies()] == ["box2"]
    s.detach_body("box2")
    assert s.attached_bodies() == []
    Q = _states(cfg, 4000, 3)
    for x, y in zip(s.state_valid_batch(Q), s0.state_valid_batch(Q)):
        assert np.array_equal(x, y)
    ids = []
    for sp in (s, s0):
        sp.set_goal_joint(cfg.goal, cfg.goal_tol)
        ids.append(sp.set_start(cfg.start))
    a, b = s.get_succs(ids[0]), s0.get_succs(ids[1])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    r, r0 = s.plan(*SEARCH), s0.plan(*SEARCH)
    assert r["solved"] and list(r["path"]) == list(r0["path"]) and r["cost"] == r0["cost"]
    assert np.array_equal(r["expansion_log"], r0["expansion_log"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. planning
# ---------------------------------------------------------------------------------------------------------------------

def _plan_on(s, cfg, device, monkeypatch):
    monkeypatch.setenv("SMPLX_SEARCH", "device" if device else "host")
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_start(cfg.start)
    return s.plan(*SEARCH)


@pytest.mark.parametrize("device", [True, False])
def test_inert_body_plans_like_the_oracle(small_cfg, device, monkeypatch):
    from oracle_binding import Oracle
    from smpl_amd import capi
    cfg = small_cfg
    link = _wrist(cfg)
    links = _tree_links(cfg)
    a = capi.Model(cfg.robot_text).arrays()
    t = links.index(link)
    leaf = [i for i in range(a["tree_first"][t], a["tree_first"][t + 1]) if a["left"][i] < 0][0]
    c = a["xyzr"][leaf]
    # tiny spheres at the centre of one of the palm's own leaves, allowed to touch every link
    sp = np.array([[c[0], c[1], c[2], 1e-4], [c[0] + 1e-4, c[1], c[2], 1e-4]])
    s = _space(cfg, "small")
    s.attach_body("inert", link, sp, allowed=links)
    r = _plan_on(s, cfg, device, monkeypatch)
    o = Oracle(cfg)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    o.set_start(cfg.start)
    o.search_params(*SEARCH)
    e = o.plan()
    assert r["solved"] == 1 and e["ok"]
    assert list(r["path"]) == list(e["path"]) and r["cost"] == e["cost"]
    assert np.array_equal(r["expansion_log"], e["expansion_log"])


def test_blocking_body_changes_the_plan(small_cfg, monkeypatch):
    cfg = small_cfg
    link = _wrist(cfg)
    s0 = _space(cfg, "small")
    r0 = _plan_on(s0, cfg, False, monkeypatch)
    assert r0["solved"]
    P0 = s0.extract_path(r0["path"])
    # a large object held well in front of the gripper: it hits the scene along the no-body path, not at start or goal
    rod = np.array([[0.7, 0.2, 0.0, 0.12]])
    t = _space(cfg, "small")
    t.attach_body("rod", link, rod, allowed=_touch(cfg))
    assert t.state_valid_batch(np.asarray([cfg.start, cfg.goal]))[0].all()
    assert not t.edge_valid_batch(P0[:-1], P0[1:])[0].all()
    res = []
    for device in (True, False):
        s = _space(cfg, "small")
        s.attach_body("rod", link, rod, allowed=_touch(cfg))
        res.append((s, _plan_on(s, cfg, device, monkeypatch)))
    (sd, rd), (sh, rh) = res
    assert rd["solved"] == rh["solved"]
    assert list(rd["path"]) == list(rh["path"]) and rd["cost"] == rh["cost"]
    assert np.array_equal(rd["expansion_log"], rh["expansion_log"])
    if rh["solved"]:
        P = sh.extract_path(rh["path"])
        assert sh.edge_valid_batch(P[:-1], P[1:])[0].all()
        b = Brute(cfg, sh)
        for i in range(len(P) - 1):
            pts, n = sh.interpolate(P[i], P[i + 1])
            exp, amb = b.valid(pts, [_touch_trees(cfg)], set())
            assert exp[~amb].all() and s0.state_valid_batch(pts)[0].all()
        assert list(rh["path"]) != list(r0["path"])


# ---------------------------------------------------------------------------------------------------------------------
# 6. contract
# ---------------------------------------------------------------------------------------------------------------------

def test_epoch_errors_and_limits(small_cfg, monkeypatch):
    from smpl_amd import capi
    cfg = small_cfg
    link = _wrist(cfg)
    monkeypatch.setenv("SMPLX_SEARCH", "host")
    s = _space(cfg, "small")
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    sid = s.set_start(cfg.start)
    r = s.replan(*SEARCH)
    assert r["solved"]
    s.attach_body("box", link, _held_box(), allowed=_touch(cfg))
    for call in (lambda: s.get_succs(sid), lambda: s.plan(*SEARCH), lambda: s.replan(*SEARCH)):
        with pytest.raises(capi.SmplxError) as e:
            call()
        assert e.value.code == -5
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_start(cfg.start)
    r = s.replan(*SEARCH)
    assert r["solved"] and not r["resumed"]
    for args in (("x", "no_such_link", _held_box()), ("x", "base_link", _held_box()), ("box", link, _held_box())):
        with pytest.raises(capi.SmplxError) as e:
            s.attach_body(*args)
        assert e.value.code == -1, args
    with pytest.raises(capi.SmplxError) as e:
        s.detach_body("nope")
    assert e.value.code == -1
    for k in range(7):
        s.attach_body(f"b{k}", link, _held_box()[:2], allowed=_touch(cfg))
    with pytest.raises(capi.SmplxError) as e:
        s.attach_body("b9", link, _held_box()[:2])
    assert e.value.code == -3
    s2 = _space(cfg, "small")
    big = _box((0.3, 0.0, 0.0), (0.16, 0.16, 0.16), 0.02, 0.01)    # 512 spheres = 1023 nodes
    s2.attach_body("big", link, big, allowed=_touch(cfg))
    with pytest.raises(capi.SmplxError) as e:
        s2.attach_body("two", link, _held_box()[:2])      # 3 more nodes: 1026
    assert e.value.code == -3
    assert [b["count"] for b in s2.attached_bodies()] == [2 * len(big) - 1]


@pytest.mark.parametrize("mode", ["device", "host"])
def test_plan_multi_mixed_bodies(small_cfg, mode, monkeypatch):
    from smpl_amd import capi
    cfg = small_cfg
    link = _wrist(cfg)
    rng = np.random.default_rng(4)
    goals = [list(np.array(cfg.goal) + rng.uniform(-0.1, 0.1, 7)) for _ in range(4)]
    rod = _box((0.28, 0.0, 0.0), (0.2, 0.02, 0.02), 0.02, 0.02)
    monkeypatch.setenv("SMPLX_SEARCH", mode)

    def mk(q):
        s = _space(cfg, "small")
        if q % 2:
            s.attach_body("rod", link, rod, allowed=_touch(cfg))
        s.set_goal_joint(goals[q], cfg.goal_tol)
        s.set_start(cfg.start)
        return s
    singles = [mk(q).plan(*SEARCH) for q in range(4)]
    out, _ = capi.Space.plan_multi([mk(q) for q in range(4)], *SEARCH)
    for q in range(4):
        assert out[q]["solved"] == singles[q]["solved"], q
        assert list(out[q]["path"]) == list(singles[q]["path"]) and out[q]["cost"] == singles[q]["cost"], q
        assert np.array_equal(out[q]["expansion_log"], singles[q]["expansion_log"]), q


# ---------------------------------------------------------------------------------------------------------------------
# 7. C++: GpuCollisionChecker::attachObject / detachObject with GpuARAStar
# ---------------------------------------------------------------------------------------------------------------------

def test_cpp_attach_plan_detach(small_cfg, tmp_path, monkeypatch):
    import subprocess
    from oracle_binding import Oracle
    from smpl_amd.plugin_tools import build_driver, write_query
    cfg = small_cfg
    link = _wrist(cfg)
    rod = _box((0.28, 0.0, 0.0), (0.2, 0.02, 0.02), 0.02, 0.02)
    exe = build_driver("attached_body_driver", tmp_path)
    write_query(cfg, tmp_path, [])
    with open(tmp_path / "body.txt", "w") as f:
        f.write(f"rod {link} {len(_touch(cfg))} {' '.join(_touch(cfg))}\n")
        for x, y, z, r in rod:
            f.write(f"{float(x)!r} {float(y)!r} {float(z)!r} {float(r)!r}\n")
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in out.stdout.decode().splitlines() if " " in l}
    s = _space(cfg, "small")
    s.attach_body("rod", link, rod, allowed=_touch(cfg))
    assert lines["valid"] == f"1 {int(s.state_valid_batch(np.asarray([cfg.start]))[0][0])}"
    # with the body: what the C-ABI plans on a space holding the same body
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_start(cfg.start)
    r = s.replan(*SEARCH)
    w = lines["with"].split()
    assert int(w[1]) == r["cost"] and [int(x) for x in w[3:]] == list(r["path"])
    # after the detach: the oracle without a body
    o = Oracle(cfg)
    o.set_goal_joint(cfg.goal, cfg.goal_tol)
    o.set_start(cfg.start)
    o.search_params(*SEARCH)
    e = o.plan()
    wo = lines["without"].split()
    assert int(wo[1]) == e["cost"] and [int(x) for x in wo[3:]] == list(e["path"])
