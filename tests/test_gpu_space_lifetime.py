"""A space owns everything it holds on the device (smpl_amd/csrc/space.h, device_mem.h): one space touches every resource
that is created on first use, is destroyed, and the next one starts from nothing -- forty times in one process, with the
same plan at the end as at the beginning.  A create that fails leaves nothing behind that a later create trips over.
Free device memory is not looked at: the card is shared and the figure is device-wide."""
import ctypes as C

import numpy as np
import pytest

from smpl_amd import scenes
from test_gpu_three_launch_step import _Hip

pytestmark = pytest.mark.gpu

ROUNDS = 40
E_ARG, E_PARSE = -1, -2


@pytest.fixture(scope="module")
def scene(small_cfg):
    """the model and the grid every round shares, and the per-robot kernels built before any round is timed"""
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    g = small_cfg.grid
    grid, model = capi.Grid(g.origin, g.dims, g.res, g.max_dist, g.d2), capi.Model(small_cfg.robot_text)
    capi.Space(model, grid, small_cfg.mprim, small_cfg.params, batch_states=256).close()
    return capi, small_cfg, model, grid


def _round(capi, cfg, model, grid, hip, Q):
    """every call raises unless it returns SMPLX_OK"""
    s = capi.Space(model, grid, cfg.mprim, cfg.params, batch_states=256)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    s.set_start(cfg.start)
    plan = s.plan(5.0, 1.0, 1.0, True, True, 6000, 3000)             # the device-resident search: arena, header, table
    assert s.search_counters()["searches"] == 1
    s.table_sync()
    s.attach_body("held", "gripper_palm_link", [[0.1, 0.0, 0.0, 0.03], [0.15, 0.0, 0.0, 0.03]])
    s.detach_body("held")
    s.profile_begin(2)                                               # ... and no profile_end: the events die with the space
    B, BM, N = Q.shape[0], Q.shape[0] * s.M, s.N
    d_q, st = hip.upload(Q), hip.stream()                            # a caller's stream: a second set of step counters
    out = [hip.alloc(n) for n in (BM, 4 * BM * N, 8 * BM * N, 4 * BM, 4 * BM, 4 * BM, s.expand_work_bytes(B))]
    s.expand_batch(Q)                                                # (the first set, on the space's own stream)
    s.expand_batch_device(d_q, B, *out, None, st)
    assert s.step_counters_zero(st)
    flags = hip.download(out[0], BM, np.uint8)
    s.state_clearance_batch(Q)
    s.lazy_expand_batch(Q)
    s.close()
    hip.close()
    return plan, flags


def test_forty_spaces_one_after_the_other(scene, monkeypatch):
    capi, cfg, model, grid = scene
    monkeypatch.setenv("SMPLX_SEARCH", "device")      # a lone query takes the host loop otherwise; fail if the kernel does not fit
    Q = scenes.random_states(scenes.ARM7_LIMITS, 24, 5)
    hip = _Hip()
    first = last = None
    for r in range(ROUNDS):
        last = _round(capi, cfg, model, grid, hip, Q)
        first = first or last
    (p0, f0), (p1, f1) = first, last
    assert p0["solved"] and p0["path_len"] > 1
    assert np.array_equal(p0["path"], p1["path"]) and p0["cost"] == p1["cost"] and p0["solved"] == p1["solved"]
    assert np.array_equal(p0["expansion_log"], p1["expansion_log"]) and np.array_equal(f0, f1)


def test_a_failed_create_then_a_good_one(scene):
    """the refusals of smplx_space_create keep their codes and texts: a bad primitive file (the space exists by then, its
    stream does not), a bad heuristic kind (nothing exists yet); each is followed by a create that succeeds and plans"""
    capi, cfg, model, grid = scene
    for kw, mprim, code, text in (({}, "not a primitive file", E_PARSE, "mprim: first token must be 'Motion_Primitives(degrees):'"),
                                  ({}, "Motion_Primitives(degrees): 2 3 0\n1 0 0\n", E_PARSE, "mprim: column count does not match the planning variables"),
                                  ({"heuristic": 7}, cfg.mprim, E_ARG, "smplx_params.heuristic: SMPLX_H_BFS, SMPLX_H_EUCLID or SMPLX_H_JOINT_DIST")):
        for _ in range(3):
            with pytest.raises(capi.SmplxError) as e:
                capi.Space(model, grid, mprim, cfg.params, batch_states=256, **kw)
            assert e.value.code == code and capi.lib().smplx_last_error().decode() == text
        s = capi.Space(model, grid, cfg.mprim, cfg.params, batch_states=256)
        s.set_goal_joint(cfg.goal, cfg.goal_tol)
        s.set_start(cfg.start)
        assert s.plan(5.0, 1.0, 1.0, True, True, 6000, 3000)["solved"]
        s.close()
    capi.lib().smplx_space_destroy(None)                             # a null handle is nothing to destroy
