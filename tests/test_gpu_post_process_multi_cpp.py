"""smpl_amd::PostProcessPaths through the C++ plugin mirror (include/smpl_amd/plugin.hpp), on the GPU: three paths in one
call (tests/cpp/post_process_multi_driver.cpp) come out as three PostProcessPath calls give them, double for double, with
the sizes the C-ABI reports and within the launch bound."""
import subprocess

import numpy as np
import pytest

from smpl_amd import scenes
from smpl_amd.plugin_tools import build_driver, write_query

pytestmark = pytest.mark.gpu


def test_three_paths_through_the_plugin_mirror(small_cfg, tmp_path):
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    cfg = small_cfg
    s = capi.Space.from_config(cfg)
    Q = scenes.random_states(scenes.ARM7_LIMITS, 60, 31)
    V = Q[s.state_valid_batch(Q)[0].astype(bool)][:17]
    assert V.shape[0] == 17
    exe = build_driver("post_process_multi_driver", tmp_path)
    write_query(cfg, tmp_path, [len(V), *[float(v) for v in V.ravel()]])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = [l.split() for l in out.stdout.decode().splitlines()]
    assert [l for l in lines if l[0] == "equal"] == [["equal", str(k), "1"] for k in range(3)]
    paths = [V[:12], V[12:14], V[14:]]
    want = [s.post_process_path(p, True, True, True)[0].shape[0] for p in paths]
    assert [int(l[2]) for l in lines if l[0] == "size"] == want
    st = [int(x) for x in next(l for l in lines if l[0] == "stats")[1:]]
    bound = int(next(l for l in lines if l[0] == "bound")[1])
    assert bound == capi.PP_MULTI_MAX_LAUNCHES and 1 <= st[0] <= bound and 1 <= st[1] <= bound and st[2] > 0 and st[3] == 3
    assert ["mismatch", "0"] in lines and ["empty", "1"] in lines and ["done"] in lines
