"""Octomaps through the C++ mirror: tests/cpp/octree_driver.cpp runs processOctomapMsg, a duplicate id, moveShapes and
removeObject through smpl_amd::GpuCollisionChecker (include/smpl_amd/plugin.hpp) on a context with an editable grid; the
bool returns are those of CollisionSpace::processOctomapMsg (collision_space.cpp:285-288, checkInsertOctomap,
world_collision_model.cpp:553-572) and isStateValid flips with the leaf."""
import subprocess

import numpy as np
import pytest

from smpl_amd import capi

pytestmark = pytest.mark.gpu


def test_cpp_octomap_insert_move_remove(small_cfg, tmp_path):
    from smpl_amd.plugin_tools import build_driver, write_query
    cfg, gr = small_cfg, small_cfg.grid
    exe = build_driver("octree_driver", tmp_path)
    write_query(cfg, tmp_path, [])
    # a point inside the arm at the start state: the centre of the model's last sphere, on an EMPTY grid of the scene's size
    g = capi.Grid.empty(gr.origin, gr.dims, gr.res, gr.max_dist)
    s = capi.Space(capi.Model(cfg.robot_text), g, cfg.mprim, cfg.params, 16)
    q = np.asarray([cfg.start])
    assert s.state_valid_batch(q)[0][0] == 1
    centre = s.sphere_positions(q)[0, -1]
    with open(tmp_path / "object.txt", "w") as f:
        f.write(" ".join(repr(float(x)) for x in centre) + f" {gr.res!r}\n")
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()
    assert lines == [
        "empty 1",
        "octomap 1 0",              # inserted; the start is now in collision
        "octomap_again 0",          # checkInsertOctomap: the id is taken
        "octomap_no_leaves 0",
        "octomap_ragged 0",         # leaf rows come in fours
        "move 1 1",                 # moved into a corner: free again
        "move_back 1 0",            # two leaves, one at the arm
        "remove 1 1",
        "remove_again 0",
        "insert_mixed 1 0",         # a box in the corner and a leaf at the arm in one object
        "octomap_beside 1 0",
        "remove_mixed 1 1",
        "done",
    ], lines
