"""Distance to collision through the C++ plugin mirror (include/smpl_amd/plugin.hpp), on the GPU: a caller that holds a
CollisionChecker asks it for its CollisionDistanceExtension (tests/cpp/clearance_driver.cpp) and gets, bit for bit, what the
C-ABI answers; isStateValid(state, dist) still returns what it did."""
import subprocess

import numpy as np
import pytest

from smpl_amd import scenes
from smpl_amd.plugin_tools import build_driver, write_query

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def test_distance_extension_through_the_plugin_mirror(small_cfg, tmp_path):
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    cfg = small_cfg
    Q = scenes.random_states(scenes.ARM7_LIMITS, 6, 21)
    exe = build_driver("clearance_driver", tmp_path)
    write_query(cfg, tmp_path, [len(Q), *[float(v) for v in Q.ravel()]])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = {l.split(" ", 1)[0]: l.split(" ", 1)[1] if " " in l else "" for l in out.stdout.decode().splitlines()}
    assert lines["extension"] == "1 1"
    s = capi.Space.from_config(cfg)
    start, goal = np.array(cfg.start, float), np.array(cfg.goal, float)

    def num(key):
        return np.array(lines[key].split(), dtype=np.float64)
    assert np.array_equal(_bits(num("state")), _bits(s.state_clearance_batch(start)[0]))
    assert np.array_equal(_bits(num("edge")), _bits(s.edge_clearance_batch(start, goal)[0]))
    assert np.array_equal(_bits(num("still")), _bits(num("state")))            # an edge without motion: its start
    assert np.array_equal(_bits(num("states")), _bits(s.state_clearance_batch(Q)[0]))
    assert np.array_equal(_bits(num("edges")), _bits(s.edge_clearance_batch(Q[:-1], Q[1:])[0]))
    assert num("edge")[0] <= num("state")[0]
    # the validity, and the largest double in the distance argument, as before
    assert lines["valid"] == f"{int(s.state_valid_batch(start)[0][0])} 1"
    assert lines["short"] == "1"                                               # NaN for a state of the wrong length
    assert "done" in lines
