"""Inputs of tests/test_gpu_post_process_multi.py that need a robot of their own.

`slider`: an arm of one revolute joint with a sphere at its tip, and a second planning variable, a prismatic joint of
40 m that moves a link without spheres.  The prismatic variable adds motion -- 20 waypoints a metre
(robot_motion_collision_model.h:352-366) -- and nothing to the collision check, so an edge can be given any waypoint count
up to 800 while its validity is the arm's alone: the counts at and beyond the lane count of k_shortcut
(smpl_amd/csrc/path_kernels.h), which the 7-DOF arm's limits cannot reach (its longest edge has 487 waypoints).
The scene is one box in the sweep of the arm's tip: the arm is free from ja = 0 up to an angle near 1 rad and in
collision from there on.
"""
from __future__ import annotations

import functools

from smpl_amd import scenes

DEG = scenes.DEG
RES, CAP = 0.04, 0.4
DIMS = (48, 40, 32)
ORIGIN = (-0.96, -0.8, 0.0)
ARM = 0.40
SLIDER_LIMITS = [(-0.5, 2.0), (0.0, 40.0)]
SLIDER_BOX = ((ARM * 0.5403, ARM * 0.8415, 0.62), (0.12, 0.12, 0.2))     # at the tip's place for ja = 1 rad

_J = "joint {n} {t} {pa} {ch}  {o[0]} {o[1]} {o[2]}  {r[0]} {r[1]} {r[2]}  {a[0]} {a[1]} {a[2]}  {lo} {hi}"


def slider_robot() -> str:
    L = ["robot slider"] + [f"link {l}" for l in ("base_link", "mount", "a", "rail", "tool_link")]

    def joint(n, t, pa, ch, o=(0, 0, 0), r=(0, 0, 0), a=(0, 0, 1), lo=0.0, hi=0.0):
        L.append(_J.format(n=n, t=t, pa=pa, ch=ch, o=o, r=r, a=a, lo=lo, hi=hi))

    joint("mount_fix", "fixed", "base_link", "mount", o=(0.0, 0.0, 0.62))
    joint("ja", "revolute", "mount", "a", a=(0, 0, 1), lo=SLIDER_LIMITS[0][0], hi=SLIDER_LIMITS[0][1])
    joint("slide", "prismatic", "a", "rail", a=(0, 0, 1), lo=SLIDER_LIMITS[1][0], hi=SLIDER_LIMITS[1][1])
    joint("tool", "fixed", "a", "tool_link", o=(ARM, 0.0, 0.0))
    L.append(f"sphere a a0 {ARM!r} 0.0 0.0 0.05 1")
    L.append(f"sphere a a1 {0.5 * ARM!r} 0.0 0.0 0.04 1")
    t = "\n".join(L) + "\n"
    t += "group g a\n"
    t += "planning_joints ja slide\n"
    t += "planning_link tool_link\n"
    return t


def held_box():
    """spheres (x, y, z, r) in the wrist's frame: 3 x 3 x 3 of radius 1.5 cm at 2 cm pitch around (0.25, 0, 0)"""
    import numpy as np
    axes = [np.arange(-0.03 + 0.01, 0.03, 0.02) + c for c in (0.25, 0.0, 0.0)]
    g = np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    return np.hstack([g, np.full((len(g), 1), 0.015)])


def touch_links(robot_text: str, wrist: str = "gripper_palm_link"):
    return [wrist] + [l.split()[1] for l in robot_text.splitlines() if l.startswith("link ") and "finger" in l]


@functools.lru_cache(maxsize=None)
def slider_cfg():
    grid = scenes.build_grid(ORIGIN, DIMS, RES, CAP, [SLIDER_BOX])
    p = scenes.PlanningParams([2 * DEG, 0.02], eps0=5.0, bfs_radius=0.04, cost_per_cell=500)
    start = [0.0, 0.0]
    return scenes.Config("slider", slider_robot(), scenes.mprim_text(2, range(2), range(2), long_cells=4, short_cells=1), grid, p,
                         start, list(start), [3 * DEG, 0.03], [SLIDER_BOX])
