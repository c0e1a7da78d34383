"""The measurements of the robot body (profiles/robot_body_ab.txt records them), one JSON line, in
one process on one GPU.  Grid: 256^3 cells of 0.02 m, max_dist 0.2 m (an edit window reaches 10 cells).

The body has the size of the reference's PR2 list (tests/golden/collision_model_pr2.yaml, voxels_models): 46 links with a
voxel model at res 0.01 m -- generated boxes and cylinders of PR2-like dimensions (a base, four casters with two wheels
each, a torso on a lift joint, two laser links, eight head and sensor links, a left arm of fourteen links, a right arm of
eight) -- of which the left arm's last five are the planning group's, so 41 models are placed.
Medians over --reps repetitions after a warm-up, the legs alternating inside each repetition:
         create_ms         smplx_body_create: parse, meshes, the voxeliser's launches for all models, download, upload
         first_put_ms      smplx_grid_put_body of a new body: every outside state placed, one field update
         root_put_ms       smplx_body_set_joint on the torso lift (moves most of the placed states) + put
         leaf_put_ms       smplx_body_set_joint on the head tilt joint (moves the head's links) + put
         take_ms           smplx_grid_take_body
and beside each put the parent commit's only route for the same cells: the points transformed on the host (numpy, timed)
and sent through smplx_grid_remove_points (the states' old points; not for the first put) + smplx_grid_add_points (uploads
and both field edits included).  The host voxelisation that route needs first is EXCLUDED (the parent has none on the
GPU; tests/body_ref.py takes seconds).
Host clock around synchronous calls (each ends in a device synchronise).

    python tools/robot_body_time.py [--reps R]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smpl_amd import capi  # noqa: E402

ORIGIN, DIMS, RES, MAX_DIST = (-2.0, -2.5, -0.2), (256, 256, 256), 0.02, 0.2


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
            "calls": int(ms.size)}


def pr2_like_body():
    links, joints, geoms = ["base_link"], [], ["geom base_link box 0.65 0.65 0.3  0.0013 0.0027 0.1531  0 0 0.0137"]

    def add(name, parent, jtype, xyz, axis, geom, lim=(-3.0, 3.0)):
        links.append(name)
        joints.append("joint %s_joint %s %s %s  %r %r %r  0.0 0.0 0.0137  %r %r %r  %r %r" % ((name, jtype, parent, name) + tuple(xyz) + tuple(axis) + lim))
        geoms.append("geom %s %s  0.0011 0.0023 0.0017  0.0137 0.0213 0.0" % (name, geom))

    for c, (x, y) in zip(("fl", "fr", "bl", "br"), ((0.2246, 0.2246), (0.2246, -0.2246), (-0.2246, 0.2246), (-0.2246, -0.2246))):
        add(c + "_caster_rotation_link", "base_link", "continuous", (x, y, 0.0793), (0, 0, 1), "box 0.19 0.08 0.1")
        for w, dy in (("l", 0.049), ("r", -0.049)):
            add("%s_caster_%s_wheel_link" % (c, w), c + "_caster_rotation_link", "continuous", (0.0, dy, 0.0), (0, 1, 0), "cylinder 0.074 0.034")
    add("torso_lift_link", "base_link", "prismatic", (-0.05, 0.0, 0.7397), (0, 0, 1), "box 0.3 0.36 0.8", (0.0, 0.31))
    add("laser_tilt_mount_link", "torso_lift_link", "revolute", (0.0981, 0.0, 0.2273), (0, 1, 0), "box 0.06 0.1 0.08")
    add("base_laser_link", "base_link", "fixed", (0.275, 0.0, 0.252), (0, 0, 1), "cylinder 0.03 0.06")
    add("head_pan_link", "torso_lift_link", "revolute", (-0.0171, 0.0, 0.3815), (0, 0, 1), "box 0.16 0.28 0.1")
    add("head_tilt_link", "head_pan_link", "revolute", (0.068, 0.0, 0.0), (0, 1, 0), "box 0.13 0.29 0.12")
    add("head_plate_frame", "head_tilt_link", "fixed", (0.0232, 0.0, 0.0645), (0, 0, 1), "box 0.1 0.26 0.03")
    add("sensor_mount_link", "head_plate_frame", "fixed", (0.0, 0.0, 0.03), (0, 0, 1), "box 0.08 0.2 0.05")
    add("double_stereo_link", "sensor_mount_link", "fixed", (0.0, 0.0, 0.04), (0, 0, 1), "box 0.05 0.24 0.05")
    add("head_mount_kinect_link", "head_plate_frame", "fixed", (-0.05, 0.0, 0.12), (0, 0, 1), "box 0.07 0.28 0.06")
    add("imu_link", "torso_lift_link", "fixed", (-0.02977, -0.1497, 0.164), (0, 0, 1), "box 0.04 0.04 0.03")
    add("projector_link", "head_plate_frame", "fixed", (0.0, 0.11, 0.05), (0, 0, 1), "cylinder 0.02 0.05")
    arm = [("l_shoulder_pan_link", "torso_lift_link", (0.0, 0.188, 0.0), (0, 0, 1), "cylinder 0.14 0.3"),
           ("l_shoulder_lift_link", "l_shoulder_pan_link", (0.1, 0.0, 0.0), (0, 1, 0), "box 0.18 0.16 0.18"),
           ("l_upper_arm_roll_link", "l_shoulder_lift_link", (0.0, 0.0, 0.0), (1, 0, 0), "cylinder 0.07 0.12"),
           ("l_upper_arm_link", "l_upper_arm_roll_link", (0.2, 0.0, 0.0), (0, 1, 0), "box 0.36 0.14 0.14"),
           ("l_elbow_flex_link", "l_upper_arm_link", (0.2, 0.0, 0.0), (0, 1, 0), "cylinder 0.07 0.13"),
           ("l_forearm_roll_link", "l_elbow_flex_link", (0.0, 0.0, 0.0), (1, 0, 0), "cylinder 0.06 0.1"),
           ("l_forearm_link", "l_forearm_roll_link", (0.16, 0.0, 0.0), (0, 1, 0), "box 0.3 0.1 0.1"),
           ("l_wrist_flex_link", "l_forearm_link", (0.161, 0.0, 0.0), (0, 1, 0), "cylinder 0.045 0.08"),
           ("l_wrist_roll_link", "l_wrist_flex_link", (0.0, 0.0, 0.0), (1, 0, 0), "cylinder 0.04 0.06"),
           ("l_gripper_palm_link", "l_wrist_roll_link", (0.05, 0.0, 0.0), (0, 0, 1), "box 0.1 0.1 0.05"),
           ("l_gripper_l_finger_link", "l_gripper_palm_link", (0.0769, 0.01, 0.0), (0, 0, 1), "box 0.09 0.03 0.03"),
           ("l_gripper_r_finger_link", "l_gripper_palm_link", (0.0769, -0.01, 0.0), (0, 0, 1), "box 0.09 0.03 0.03"),
           ("l_gripper_l_finger_tip_link", "l_gripper_l_finger_link", (0.0916, 0.005, 0.0), (0, 0, 1), "box 0.04 0.02 0.02"),
           ("l_gripper_r_finger_tip_link", "l_gripper_r_finger_link", (0.0916, -0.005, 0.0), (0, 0, 1), "box 0.04 0.02 0.02")]
    for name, parent, xyz, axis, geom in arm:
        add(name, parent, "revolute", xyz, axis, geom)
    for name, parent, xyz, axis, geom in arm[:8]:          # the right arm down to the wrist, mirrored
        add("r" + name[1:], parent if parent == "torso_lift_link" else "r" + parent[1:], "revolute", (xyz[0], -xyz[1], xyz[2]), axis, geom)
    group = [a[0] for a in arm[-5:]]
    assert len(links) == 46
    text = ["robot pr2_like"] + ["link " + l for l in links] + joints + geoms + ["voxels %s 0.01" % l for l in links]
    text += ["group left_gripper " + " ".join(group), "value torso_lift_link_joint 0.0137", "value head_pan_link_joint 0.1137"]
    return "\n".join(text) + "\n", links, group


def world_points(body, models):
    """the parent's host side: every model's points under its link's transform (numpy)"""
    T = body.link_transforms()
    out = []
    for m in models:
        A = T[body.model_link(m)]
        out.append(body.model_points(m) @ A[:, :3].T + A[:, 3])
    return np.vstack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    text, links, group = pr2_like_body()
    g = capi.Grid.empty(ORIGIN, DIMS, RES, MAX_DIST)
    g2 = capi.Grid.empty(ORIGIN, DIMS, RES, MAX_DIST)
    probe = capi.Body(text)
    outside = [m for m in range(probe.nmodels) if links[probe.model_link(m)] not in group]
    pts = {m: probe.model_points(m) for m in range(probe.nmodels)}      # what the parent would have to voxelise on the host
    probe.model_points = lambda m: pts[m]
    kids = {l: [] for l in links}
    for row in text.splitlines():
        w = row.split()
        if w and w[0] == "joint":
            kids[w[3]].append(w[4])

    def below(link):
        out = [link]
        for k in kids[link]:
            out += below(k)
        return out
    moved = {j: [m for m in outside if links[probe.model_link(m)] in below(j[:-len("_joint")])] for j in ("torso_lift_link_joint", "head_tilt_link_joint")}
    legs = {k: [] for k in ("create", "first_put", "first_put_parent", "root_put", "root_put_parent", "leaf_put", "leaf_put_parent", "take")}
    cells = {}

    def clock(name, f, keep):
        t = time.perf_counter()
        r = f()
        if keep:
            legs[name].append((time.perf_counter() - t) * 1e3)
        return r

    for rep in range(a.warmup + a.reps):
        keep = rep >= a.warmup
        body = clock("create", lambda: capi.Body(text), keep)
        clock("first_put", lambda: g.put_body(body), keep)
        cells["first_put"] = g.last_edit_cells()
        probe.set_joint("torso_lift_link_joint", 0.0137); probe.set_joint("head_tilt_link_joint", 0.0)
        clock("first_put_parent", lambda: g2.add_points(world_points(probe, outside)), keep)
        for leg, joint, q in (("root_put", "torso_lift_link_joint", 0.2137), ("leaf_put", "head_tilt_link_joint", 0.4321)):
            def ours():
                body.set_joint(joint, q)
                g.put_body(body)

            def parents():
                old = world_points(probe, moved[joint])
                probe.set_joint(joint, q)
                g2.remove_points(old)
                g2.add_points(world_points(probe, moved[joint]))
            clock(leg, ours, keep)
            cells[leg] = g.last_edit_cells()
            clock(leg + "_parent", parents, keep)
        if rep == 0:    # without counts a removal frees shared cells, and the two routes remove in a different order
            cells["fields_differ_in"] = int((g.d2() != g2.d2()).sum())
        clock("take", lambda: g.take_body(), keep)
        g2.remove_points(world_points(probe, outside))
        body.close()
    out = {"links": len(links), "models": probe.nmodels, "outside_models": len(outside), "points": probe.npoints,
           "outside_points": int(sum(len(pts[m]) for m in outside)), "moved_states": {k: len(v) for k, v in moved.items()},
           "edit_cells": cells, "grid": list(DIMS), "res": RES, "reps": a.reps}
    out.update({k: stats(v) for k, v in legs.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
