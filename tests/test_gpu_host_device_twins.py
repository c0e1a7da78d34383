"""The host form of a collision query stages its rows and calls its _device twin (smpl_amd/csrc/queries.h): both forms give
the same bytes -- validity with its lookups, clearance with its parts and its witness -- on either side of a block of 64
states, and each keeps its own refusals."""
import numpy as np
import pytest

from smpl_amd import scenes
from test_gpu_three_launch_step import _Hip

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65]
E_ARG = -1


@pytest.fixture(scope="module")
def space(small_cfg):
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    return capi.Space.from_config(small_cfg, batch_states=256)


@pytest.fixture()
def hip():
    h = _Hip()
    yield h
    h.close()


def _states():
    return np.ascontiguousarray(scenes.random_states(scenes.ARM7_LIMITS, max(SIZES), 99))    # the clearance tests' states


def test_the_states_are_on_both_sides(space):
    ok = space.state_valid_batch(_states())[0]
    assert 0 < ok.sum() < len(ok)


@pytest.mark.parametrize("n", SIZES)
def test_state_valid(space, hip, n):
    Q = _states()[:n]
    valid, lookups = space.state_valid_batch(Q)
    d_q = hip.upload(Q)
    for stream in (None, hip.stream()):
        d_valid, d_lookups = hip.alloc(n, 0xEE), hip.alloc(4 * n, 0xEE)      # fresh for each stream: nothing left of the other
        space.state_valid_batch_device(d_q, n, d_valid, d_lookups, stream)
        hip.sync()
        assert hip.download(d_valid, n, np.uint8).tobytes() == valid.tobytes()
        assert hip.download(d_lookups, n, np.int32).tobytes() == lookups.tobytes()
    assert set(valid.tolist()) <= {0, 1}


@pytest.mark.parametrize("n", SIZES)
def test_state_clearance(space, hip, n):
    Q = _states()[:n]
    c, p, w = space.state_clearance_batch(Q)
    d_q = hip.upload(Q)
    for stream in (None, hip.stream()):
        d_c, d_p, d_w = hip.alloc(8 * n, 0xEE), hip.alloc(16 * n, 0xEE), hip.alloc(16 * n, 0xEE)     # fresh for each stream
        space.state_clearance_batch_device(d_q, n, d_c, d_p, d_w, stream)
        hip.sync()
        assert hip.download(d_c, n, np.float64).tobytes() == c.tobytes()
        assert hip.download(d_p, 2 * n, np.float64).tobytes() == p.tobytes()
        assert hip.download(d_w, 4 * n, np.int32).tobytes() == w.tobytes()


def test_refusals(space, hip):
    """n == 0: the host forms and the clearance _device form return SMPLX_OK and touch nothing, the validity _device form
    refuses it; n < 0: every form refuses"""
    from smpl_amd import capi
    Q = _states()[:1]
    d_q, d_out = hip.upload(Q), hip.alloc(64, 0xEE)
    none = np.zeros((0, space.N))
    assert all(len(a) == 0 for a in space.state_valid_batch(none) + space.state_clearance_batch(none))
    space.state_clearance_batch_device(d_q, 0, d_out, None, None, None)
    bad = [lambda: space.state_valid_batch_device(d_q, 0, d_out, d_out, None),
           lambda: space.state_valid_batch_device(d_q, -1, d_out, d_out, None),
           lambda: space.state_clearance_batch_device(d_q, -1, d_out, None, None, None)]
    L = capi.lib()
    v, lk, c = np.full(1, 0xEE, np.uint8), np.zeros(1, np.int32), np.zeros(1)
    dp, up, ip = capi._dp, capi._up, capi._ip
    bad.append(lambda: capi._chk(L.smplx_cc_state_valid_batch(space.h, capi._p(Q, dp), -1, capi._p(v, up), capi._p(lk, ip))))
    bad.append(lambda: capi._chk(L.smplx_cc_state_clearance_batch(space.h, capi._p(Q, dp), -1, capi._p(c, dp), None, None)))
    for call in bad:
        with pytest.raises(capi.SmplxError) as e:
            call()
        assert e.value.code == E_ARG and L.smplx_last_error().decode() == "bad argument"
    hip.sync()
    assert (hip.download(d_out, 64, np.uint8) == 0xEE).all() and v[0] == 0xEE
