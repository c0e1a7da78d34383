"""A lazy planner through the C++ plugin mirror (include/smpl_amd/plugin.hpp), on the GPU: tests/cpp/lazy_loop_driver.cpp
is a small lazy weighted A* that calls only GpuManipLattice::GetLazySuccs, GetTrueCost and GetGoalHeuristic.  The same loop
in Python (lazy_ref.lazy_search) over the plain model of tests/lazy_ref.py must print the same expansion order, the same
evaluated edges with the same costs, the same path and cost: ids, lists, heuristics and true costs all have to agree for
that, in the order a lazy search asks for them."""
import subprocess

import pytest

import lazy_ref
import width_cases as wc
from smpl_amd import scenes
from smpl_amd.plugin_tools import build_driver, write_query

pytestmark = pytest.mark.gpu

EPS, MAX_EXPANSIONS = 5.0, 1500


@pytest.mark.parametrize("name", ["small_cfg", "M63"])
def test_lazy_loop_equals_the_model(name, tmp_path):
    from oracle_binding import Oracle
    from smpl_amd import capi
    if capi.lib().smplx_device_count() == 0:
        pytest.fail("no GPU visible: the gpu-marked tests must run on the MI355X box")
    cfg = scenes.config_small() if name == "small_cfg" else wc.case_config(name)
    o = Oracle(cfg)
    o.set_order(chain=True)
    m = lazy_ref.LazyModel(o, cfg, lazy_ref.Goal.joint(cfg.goal, cfg.goal_tol))
    want = lazy_ref.lazy_search(m, m.set_start(cfg.start), EPS, MAX_EXPANSIONS)
    exe = build_driver("lazy_loop_driver", tmp_path)
    write_query(cfg, tmp_path, [EPS, MAX_EXPANSIONS])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = out.stdout.decode().splitlines()
    print(name, ":", len(want[0].split()) - 1, "expansions,", len(want[1].split()) - 1, "edges evaluated,", want[3], ",",
          sum(e.endswith(":-1") for e in want[1].split()[1:]), "refused ;", got[4])
    assert len(want[0].split()) - 1 >= 20 and len(want[1].split()) - 1 >= 20      # the search does something
    assert [l.rstrip() for l in got[:4]] == [l.rstrip() for l in want]
    assert got[4].startswith("stats ") and got[5] == "done"
