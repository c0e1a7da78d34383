"""smplx_post_process_paths on the GPU: a batch of paths in one call against two judges, the single-path call
(Space.post_process_path, path by path, on the path's own space) and the CPU oracle (Oracle.post_process).  Equal always
means the same shape and np.array_equal: the outputs are byte-identical or the test fails.

The oracle takes a third of a second for a 30-point path, so the 300-path case asks it about every tenth path; every
path of every case is held to the single-path call.
"""
import ctypes as C
import math

import numpy as np
import pytest

from smpl_amd import scenes

import post_process_cases as cases

pytestmark = pytest.mark.gpu

MODES = [(True, True, False), (True, True, True), (True, False, True), (False, True, True), (False, True, False)]
UP = (True, True, True)          # shortcut, interpolate, upstream's limits test: every stage runs
BLOCK = 128                      # smpl_amd/csrc/kernels.h SMPLX_BLOCK: the lanes of a k_shortcut block, all of them checking


def _capi():
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return capi


def _oracle(cfg):
    from oracle_binding import Oracle
    o = Oracle(cfg)
    o.set_order(chain=True)
    return o


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _check(spaces, paths, mode, oracles=None, oracle_every=1):
    """one batched call; every output against the single call on its own space and, where given, the oracle"""
    capi = _capi()
    outs, st = capi.post_process_paths(spaces, paths, *mode)
    assert len(outs) == len(paths)
    for k, (s, P) in enumerate(zip(spaces, paths)):
        want = s.post_process_path(P, *mode)[0]
        assert _same(outs[k], want), f"path {k} mode {mode}: {outs[k].shape} against the single call's {want.shape}"
        if oracles is not None and oracles[k] is not None and k % oracle_every == 0:
            ref = oracles[k].post_process(np.asarray(P, float).reshape(-1, s.N), *mode)[0]
            assert _same(outs[k], ref), f"path {k} mode {mode}: {outs[k].shape} against the oracle's {ref.shape}"
    assert 0 <= st["launches"] <= capi.PP_MULTI_MAX_LAUNCHES and 0 <= st["waits"] <= capi.PP_MULTI_MAX_LAUNCHES
    assert st["paths"] == len(paths)
    return outs, st


@pytest.fixture(scope="module", params=["per-robot", "generic"])
def ctx(small_cfg, request):
    capi = _capi()
    s = capi.Space.from_config(small_cfg, generic_kernels=(request.param == "generic"))
    assert s.specialized()[0] == (request.param == "per-robot"), s.specialized()[1]
    return small_cfg, _oracle(small_cfg), s


@pytest.fixture(scope="module")
def planned_path(small_cfg):
    capi = _capi()
    cfg = small_cfg
    s = capi.Space.from_config(cfg, batch_states=256)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_start(cfg.start)
    go = s.plan(5.0, 1.0, 1.0, True, True, 6000, 3000)
    assert go["solved"]
    return s.extract_path(go["path"])


@pytest.fixture(scope="module")
def valid_states(small_cfg):
    """valid random states of the small scene, seed 77 first (the zig-zag of tests/test_gpu_parity.py), then more"""
    capi = _capi()
    s = capi.Space.from_config(small_cfg, generic_kernels=True)
    Q = np.vstack([scenes.random_states(scenes.ARM7_LIMITS, 400, 77), scenes.random_states(scenes.ARM7_LIMITS, 3200, 78)])
    ok = s.state_valid_batch(Q)[0].astype(bool)
    return Q[ok]


def _five(planned_path, valid_states):
    return [planned_path, valid_states[:30], planned_path[:1], planned_path[:2], planned_path[:0]]


# 1 and 7 -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
def test_the_five_paths_in_one_call(ctx, planned_path, valid_states, mode):
    cfg, o, s = ctx
    paths = _five(planned_path, valid_states)
    outs, st = _check([s] * 5, paths, mode, [o] * 5)
    if mode == (False, True, False):       # the fork's limits test leaves an in-limits path un-interpolated
        for got, P in zip(outs, paths):
            assert _same(got, P)
    if mode[0]:                            # (under the fork's test only the shortcut stage launches)
        assert st["launches"] == (3 if mode == UP else 2 if mode[2] else 1) and st["configs"] > 0


# 2 and 9 -------------------------------------------------------------------------------------------------------------

def test_more_paths_than_compute_units_and_the_launch_bound(ctx, valid_states):
    cfg, o, s = ctx
    capi = _capi()
    assert valid_states.shape[0] >= 1800
    paths = [valid_states[6 * k:6 * k + 6] for k in range(300)]
    outs, st = _check([s] * 300, paths, UP, [o] * 300, oracle_every=10)
    assert st["launches"] == 3 and st["waits"] == 3 and st["paths"] == 300
    # the size bound of path_multi.h last_pass_bound, path by path: the last pass writes at most twice the waypoints the
    # first pass checks (the counts of the input path's edges, through smplx_cc_interpolate) plus P.  The first pass's
    # OUTPUT is no bound: an edge in collision leaves one point there and a free shortcut across it is interpolated whole
    for k in range(300):
        rows = sum(s.interpolate(paths[k][i], paths[k][i + 1], cap=1)[1] for i in range(5))
        assert outs[k].shape[0] <= 2 * rows + 6
    for nq in (1, 64):
        _, st = capi.post_process_paths([s] * nq, paths[:nq], *UP)
        assert st["launches"] <= capi.PP_MULTI_MAX_LAUNCHES and st["waits"] <= capi.PP_MULTI_MAX_LAUNCHES and st["paths"] == nq


# 3 -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def slider():
    """the slider robot (post_process_cases.py) on the generic kernels: the dealing of waypoints to lanes is the same
    text in both builds, and a robot of its own would cost the suite a per-robot compilation"""
    capi = _capi()
    cfg = cases.slider_cfg()
    return cfg, _oracle(cfg), capi.Space.from_config(cfg, generic_kernels=True)


def _slide_for(s, ja0, ja1, target):
    """the prismatic travel that gives the edge (ja0, 0) -> (ja1, d) exactly `target` waypoints"""
    base = s.interpolate([ja0, 0.0], [ja1, 0.0], cap=1)[1]
    d = max(0.0, (target - base - 3) * 0.05)
    while d < 40.0:
        n = s.interpolate([ja0, 0.0], [ja1, d], cap=1)[1]
        if n == target:
            return d
        assert n < target, (n, target)
        d += 0.004
    raise AssertionError("no travel gives %d waypoints" % target)


@pytest.mark.parametrize("target", [BLOCK, BLOCK + 1, 5 * BLOCK + 60])
def test_waypoint_counts_at_and_beyond_the_lane_count(slider, target):
    cfg, o, s = slider
    # the first angle at which the arm collides, on a raster finer than any waypoint spacing used below
    ang = np.linspace(0.5, 1.0, 5001)
    ok = s.state_valid_batch(np.stack([ang, np.zeros_like(ang)], 1))[0].astype(bool)
    assert ok[0] and not ok[-1]
    hit = float(ang[np.argmin(ok)])
    paths = []
    for ja1, all_valid in ((0.45, True), (hit, False)):
        d = _slide_for(s, 0.0, ja1, target)
        a, b = np.array([0.0, 0.0]), np.array([ja1, d])
        wp, n = s.interpolate(a, b, cap=8192)
        assert n == target and wp.shape[0] == target          # the count, through smplx_cc_interpolate
        v = s.state_valid_batch(wp)[0].astype(bool)
        if all_valid:
            assert v.all()
        else:
            # only the waypoint dealt last -- the edge's end, lane (target - 1) % BLOCK in its last round -- collides
            assert v[:-1].all() and not v[-1]
        paths += [np.stack([a, b]), np.stack([a, b, np.array([0.2, min(40.0, d + 1.5)])])]
    for mode in (UP, (True, False, True)):
        _check([s] * len(paths), paths, mode, [o] * len(paths))


# 4 -------------------------------------------------------------------------------------------------------------------

def test_edges_without_motion(ctx, valid_states):
    cfg, o, s = ctx
    V = valid_states[40:44]
    paths = [np.stack([V[0], V[0], V[1], V[2]]), np.stack([V[0], V[1], V[1], V[2]]), np.stack([V[0], V[1], V[2], V[2]]),
             np.stack([V[3]] * 8)]
    for mode in (UP, (True, False, True), (True, True, False)):
        _check([s] * len(paths), paths, mode, [o] * len(paths))


def test_a_full_turn_of_a_continuous_joint_is_no_motion():
    """the robot of every joint kind (scenes.config_mixed, what mixed_ctx of tests/test_gpu_parity.py builds)"""
    capi = _capi()
    cfg = scenes.config_mixed()
    o, s = _oracle(cfg), capi.Space.from_config(cfg, generic_kernels=True)   # (no per-robot compilation for one small case)
    q = np.array(cfg.start)
    turn = q.copy()
    turn[3] += 2 * math.pi
    assert s.interpolate(q, turn, cap=1)[1] == 0
    paths = [np.stack([q, turn]), np.stack([q, turn, np.array(cfg.goal)]), np.stack([q, np.array(cfg.goal), turn])]
    for mode in (UP, (True, False, True), (True, True, False)):
        _check([s] * len(paths), paths, mode, [o] * len(paths))


# 5 -------------------------------------------------------------------------------------------------------------------

def test_nothing_to_shortcut_and_everything_to_shortcut(ctx, valid_states):
    cfg, o, s = ctx
    # valid states every two of which are joined by an edge that crosses an obstacle
    V = valid_states[:80]
    keep = [0]
    for j in range(1, V.shape[0]):
        if len(keep) == 5:
            break
        A = np.stack([V[i] for i in keep])
        if not s.edge_valid_batch(A, np.repeat(V[j][None], len(keep), 0))[0].any():
            keep.append(j)
    assert len(keep) == 5
    blocked = np.stack([V[i] for i in keep])
    # a straight free line of 40 points; the steps are powers of two, so the direct cost equals the summed one exactly
    start = np.array(cfg.start)
    line = None
    for sgn in (1.0, -1.0):
        end = start.copy()
        end[0] += sgn * 39 / 64
        if s.edge_valid_batch(start, end)[0][0]:
            line = np.stack([start + np.eye(7)[0] * sgn * k / 64 for k in range(40)])
            break
    assert line is not None
    outs, _ = _check([s, s], [blocked, line], (True, False, True), [o, o])
    assert _same(outs[0], blocked)                       # the first pass keeps the end points, no shortcut is accepted
    assert _same(outs[1], line[[0, 39]])                 # collapses to 2
    _check([s, s], [blocked, line], UP, [o, o])


# 6 and 7 -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("build", ["per-robot", "generic"])
def test_spaces_that_differ_in_their_attached_bodies(small_cfg, valid_states, build):
    capi = _capi()
    cfg = small_cfg
    g = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    A = capi.Space.from_config(cfg, generic_kernels=(build == "generic"), grid=g)
    B = capi.Space.from_config(cfg, generic_kernels=(build == "generic"), grid=g)
    # the held object of tests/test_gpu_attached_bodies.py: spheres of 1.5 cm on a 2 cm raster filling a 6 cm box in front of
    # the fingers.  The oracle has no attached bodies, and its pseudo-link stand-in is no judge of a path: spheres on a link
    # raise the joints' motion weights (the motion spheres, robot_motion_collision_model.cpp:41-275), so its edges have more waypoints than
    # the engine's, whose attached bodies leave the weights alone as the reference's attachObject does.  Space B is held to
    # its own single call, as the issue sets; space A to the oracle as well.
    body, touch = cases.held_box(), cases.touch_links(cfg.robot_text)
    B.attach_body("held", "gripper_palm_link", body, allowed=touch)
    oa = _oracle(cfg)
    P = valid_states[:30]
    for mode in (UP, (True, False, True)):
        wa, wb = A.post_process_path(P, *mode)[0], B.post_process_path(P, *mode)[0]
        assert not _same(wa, wb)                         # the input discriminates
        outs, _ = _check([A, B, A], [P, P, P], mode, [oa, None, oa])
        assert _same(outs[0], outs[2]) and not _same(outs[0], outs[1])
        assert _same(outs[0], wa) and _same(outs[1], wb)


# 8 -------------------------------------------------------------------------------------------------------------------

def test_protocol(ctx, planned_path, valid_states):
    cfg, o, s = ctx
    capi = _capi()
    from smpl_amd.capi import _dp, _ip, _p
    f = capi._post_process_paths_fn()
    paths = _five(planned_path, valid_states)
    N = s.N
    first = np.zeros(6, np.int32)
    first[1:] = np.cumsum([p.shape[0] for p in paths])
    flat = np.ascontiguousarray(np.vstack(paths))
    H = (C.c_void_p * 5)(*[s.h] * 5)
    want = [s.post_process_path(p, *UP)[0] for p in paths]
    total = sum(w.shape[0] for w in want)
    # the size query
    of = np.full(6, -7, np.int32)
    st = (C.c_int64 * 4)()
    assert f(H, 5, _p(flat, _dp), _p(first, _ip), 7, None, 0, _p(of, _ip), st) == 0
    assert of.tolist() == np.concatenate([[0], np.cumsum([w.shape[0] for w in want])]).tolist()
    # one point short: SMPLX_E_LIMIT, out_first filled, out untouched
    out = np.full((total, N), 123.25)
    of2 = np.full(6, -7, np.int32)
    assert f(H, 5, _p(flat, _dp), _p(first, _ip), 7, _p(out, _dp), total - 1, _p(of2, _ip), st) == -3
    assert np.array_equal(of2, of) and (out == 123.25).all()
    assert f(H, 5, _p(flat, _dp), _p(first, _ip), 7, _p(out, _dp), total, _p(of2, _ip), st) == 0
    assert np.array_equal(out, np.vstack(want))
    # a NaN in path 3 of 5: SMPLX_E_ARG, nothing written
    bad = flat.copy()
    bad[first[3], 2] = np.nan
    out[:] = 123.25
    of2[:] = -7
    assert f(H, 5, _p(bad, _dp), _p(first, _ip), 7, _p(out, _dp), total, _p(of2, _ip), st) == capi.E_ARG
    assert (of2 == -7).all() and (out == 123.25).all()
    # bad offsets
    dec = first.copy()
    dec[2] = dec[1] - 1
    assert f(H, 5, _p(flat, _dp), _p(dec, _ip), 7, None, 0, _p(of2, _ip), st) == capi.E_ARG
    # spaces on different grids
    other = capi.Space.from_config(cfg, generic_kernels=not s.specialized()[0])    # (its own grid handle; the same build)
    H2 = (C.c_void_p * 5)(s.h, s.h, other.h, s.h, s.h)
    assert f(H2, 5, _p(flat, _dp), _p(first, _ip), 7, None, 0, _p(of2, _ip), st) == capi.E_ARG
    assert (of2 == -7).all()


# 10 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("side", ["host", "device"])
def test_the_call_leaves_a_resumable_search_alone(small_cfg, valid_states, monkeypatch, side):
    monkeypatch.setenv("SMPLX_SEARCH", side)
    capi = _capi()
    cfg = small_cfg
    P = [valid_states[:12], valid_states[12:20]]

    def run(between):
        s = capi.Space.from_config(cfg, batch_states=256)
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        s.set_start(cfg.start)
        # (eps 5 -> 4 takes 426 expansions on this scene; down to 1 it takes more than any budget a test should spend)
        a = s.replan(5.0, 4.0, 1.0, True, True, 200, 200)
        assert a["result"] == capi.ARA_TIMED_OUT
        outs = between(s)
        b = s.replan(5.0, 4.0, 1.0, True, True, 100000, 100000)
        assert b["resumed"] == 1 and b["result"] == capi.ARA_SUCCESS
        return b, outs

    def call_twice(s):
        x = capi.post_process_paths([s, s], P, *UP)[0]
        y = capi.post_process_paths([s, s], P, *UP)[0]
        assert all(_same(p, q) and p.tobytes() == q.tobytes() for p, q in zip(x, y))
        return x

    b0, _ = run(lambda s: None)
    b1, _ = run(call_twice)
    assert np.array_equal(b0["expansion_log"], b1["expansion_log"]) and b0["cost"] == b1["cost"]
    assert np.array_equal(b0["path"], b1["path"]) and b0["expansions"] == b1["expansions"]


# 11 ------------------------------------------------------------------------------------------------------------------

def test_the_waypoints_the_kernel_checks_are_the_hosts(ctx):
    cfg, o, s = ctx
    capi = _capi()
    Q = scenes.random_states(scenes.ARM7_LIMITS, 400, 5)
    A, B = Q[:200].copy(), Q[200:].copy()
    B[0] = A[0]                                  # an edge without motion
    B[1] = A[1] + np.eye(7)[4] * 2 * math.pi     # ... and one whose only motion is a full turn
    rows, counts = capi.path_waypoints(s, A, B)
    for i in range(200):
        want, n = s.interpolate(A[i], B[i], cap=4096)
        assert counts[i] == n and n == want.shape[0]
        assert _same(rows[i], want), f"edge {i}"
    assert counts[0] == 0 and max(counts) > BLOCK      # an edge with a second round of dealing
