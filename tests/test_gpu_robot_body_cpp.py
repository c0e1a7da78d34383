"""The robot body through the C++ mirror: tests/cpp/robot_body_driver.cpp attaches a body, moves its joint and detaches it
through smpl_amd::GpuCollisionChecker (include/smpl_amd/plugin.hpp) alone; every line it prints is compared with the same
sequence through the C ABI."""
import subprocess

import numpy as np
import pytest

from smpl_amd import capi

pytestmark = pytest.mark.gpu

VALUES = [1.5708, 1.5708, 0.0137, 3.1, -0.0137]


def test_cpp_attach_set_joint_detach(small_cfg, tmp_path):
    from smpl_amd.plugin_tools import build_driver, write_query
    cfg, gr = small_cfg, small_cfg.grid
    exe = build_driver("robot_body_driver", tmp_path)
    write_query(cfg, tmp_path, [])
    g = capi.Grid.empty(gr.origin, gr.dims, gr.res, gr.max_dist)
    s = capi.Space(capi.Model(cfg.robot_text), g, cfg.mprim, cfg.params, 16)
    q = np.asarray([cfg.start])
    valid = lambda: int(s.state_valid_batch(q)[0][0])
    # a box on an arm of 0.25 m that swings about a vertical axis: at swing = 0 it sits on the centre of the model's last sphere
    centre = s.sphere_positions(q)[0, -1]
    text = ("robot bar\nlink world\nlink bar\njoint swing revolute world bar  %r %r %r  0 0 0  0 0 1  -4 4\n"
            "geom bar box 0.1 0.1 0.1  0.25 0.0013 0.0017  0 0 0\nvoxels bar 0.01\n" % (float(centre[0]) - 0.25, float(centre[1]), float(centre[2])))
    (tmp_path / "body.txt").write_text(text)
    (tmp_path / "values.txt").write_text(" ".join(repr(v) for v in VALUES) + "\n")
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    lines = out.stdout.decode().splitlines()

    # the same sequence through the C ABI
    want = ["empty %d" % valid(), "set_without_body 0", "detach_without_body 0", "attach_malformed 0"]
    with pytest.raises(capi.SmplxError):
        capi.Body("link a\nvoxels nosuch 0.01\n")
    body = capi.Body(text)
    g.put_body(body)
    want += ["attach 1 %d" % valid(), "attach_again 0"]
    for v in VALUES:
        body.set_joint("swing", v)
        g.put_body(body)
        want.append("set 1 %d" % valid())
    with pytest.raises(capi.SmplxError):
        body.set_joint("nosuch", 0.5)
    want.append("set_unknown 0")
    g.take_body()
    want += ["detach 1 %d" % valid(), "detach_again 0"]
    body = capi.Body(text)
    g.put_body(body)
    want += ["reattach 1 %d" % valid(), "done"]
    assert lines == want, lines
    # and the body matters: in the way at swing = 0, out of it a quarter turn on
    assert want[0] == "empty 1" and want[4] == "attach 1 0" and want[6] == "set 1 1" and want[8] == "set 1 0" and want[-2] == "reattach 1 0"
