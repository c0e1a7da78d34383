"""An XYZ_RPY_GOAL through the C++ plugin mirror (include/smpl_amd/plugin.hpp), on the GPU: GpuManipLattice::setGoal
takes the goal type the reference's front end emits (planner_interface.cpp:1282), refuses a target offset it would
otherwise ignore, and a search that knows only GetSuccs / GetGoalHeuristic reaches the goal id (pose_goal_driver.cpp)."""
import subprocess

import numpy as np
import pytest

import pose_goal_ref as ref
from smpl_amd.plugin_tools import build_driver, write_query

pytestmark = pytest.mark.gpu

XYZ_TOL, RPY_TOL = 0.03, 0.2


def test_pose_goal_through_the_plugin_mirror(small_cfg, tmp_path):
    cfg = small_cfg
    chain = ref.Chain(cfg.robot_text)
    T = chain.transform(np.array(cfg.goal))
    xyz, rpy = T[:3, 3], ref.matrix_rpy(T[:3, :3])
    exe = build_driver("pose_goal_driver", tmp_path)
    write_query(cfg, tmp_path, [*[float(v) for v in xyz], *[float(v) for v in rpy], XYZ_TOL, RPY_TOL, 10.0, 20000])
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = {l.split(" ", 1)[0]: l.split(" ", 1)[1] if " " in l else "" for l in out.stdout.decode().splitlines()}
    assert lines["offset"] == "0"          # a non-zero xyz_offset: refused
    assert lines["short"] == "0"           # a pose without an orientation: refused
    assert lines["pose"] == "1"
    fk = np.array(lines["fk"].split(), dtype=np.float64).reshape(3, 4)
    assert np.abs(fk - chain.transform(np.array(cfg.start))[:3]).max() <= 1e-12
    reached, _, nexp, _, cost = lines["reached"].split()
    print("reached", reached, "after", nexp, "expansions, cost", cost)
    assert reached == "1" and int(cost) > 0
    last = np.array(lines["last"].split(), dtype=np.float64)      # the goal id's own joint values: inside the goal region
    Tl = chain.transform(last)
    assert (np.abs(Tl[:3, 3] - xyz) <= XYZ_TOL + 1e-12).all()
    assert ref.rotation_angle(T[:3, :3], Tl[:3, :3]) < RPY_TOL + 1e-6
    assert "done" in lines
