"""World objects through the C++ mirror: tests/cpp/world_objects_driver.cpp inserts, moves and removes an object through
smpl_amd::GpuCollisionChecker (include/smpl_amd/plugin.hpp) on a context with an editable grid; the bool returns are
those of CollisionSpace (collision_space.cpp:228-275) and isStateValid flips with the object."""
import subprocess

import numpy as np
import pytest

from smpl_amd import capi

pytestmark = pytest.mark.gpu


def test_cpp_insert_move_remove(small_cfg, tmp_path):
    from smpl_amd.plugin_tools import build_driver, write_query
    cfg, gr = small_cfg, small_cfg.grid
    exe = build_driver("world_objects_driver", tmp_path)
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
        "insert 1 0",               # inserted; the start is now in collision
        "insert_again 0",           # checkObjectInsert: the id is taken
        "insert_mismatched 0",      # shapes and poses of different lengths
        "move 1 1",                 # moved into a corner: free again
        "insert_shapes 1 0",        # a second shape, at the arm
        "remove_shapes 1 1",        # back to the one in the corner
        "move_unknown 0",
        "remove 1 1",
        "remove_again 0",           # checkObjectRemove
        "reinsert 1 0",
        "remove_by_object 1 1",
        "done",
    ], lines
    # the same flip through the C-ABI
    g.insert_object("crate", [capi.box((gr.res,) * 3, capi.pose_at(centre))])
    assert s.state_valid_batch(q)[0][0] == 0
