"""The measurement of attaching an object by shape (profiles/attach_object_ab.txt records it), one
JSON line, in one process on one GPU.  Space: the cfg-3 PR2 right arm; object: the box and the cylinder of the tests
(tests/object_cases.py: 6 x 4 x 10 cm and r 3 cm x 12 cm, 122 + 150 = 272 spheres of radius 0.025) on r_gripper_palm_link
with the gripper's links as touch links.

Medians over --reps attach / detach pairs after 3 warm-ups, host clock, hipDeviceSynchronize on both sides of each call:
    attach_object_ms    smplx_attach_object: meshes, triangle list, uploads, the voxeliser's launches, k_vox_spheres, the
                        rows' download, then what attach_body does
    attach_body_ms      smplx_attach_body of the same 272 rows: the host tree build, the image upload
    object_spheres_ms   smplx_object_spheres alone: the first part of attach_object
    detach_ms           smplx_detach_body
    vox_kernels_ms      k_vox_setup + k_vox_fill + both k_vox_compact launches of one such call, HIP events inside the
                        library (smplx_test_voxelize_timing)
A library without smplx_attach_object (the parent commit) gets the rows from --rows (an .npy file) and reports
attach_body_ms and detach_ms alone.

    python tools/attach_object_time.py [--reps R] [--rows FILE] [--save-rows FILE]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smpl_amd import capi, scenes  # noqa: E402


def cfg3():
    g = os.path.join(ROOT, "tests", "golden")
    acm = json.load(open(os.path.join(g, "pr2_right_arm_acm.json")))["allowed_pairs"]
    return scenes.config3_pr2(open(os.path.join(g, "collision_model_pr2.yaml")).read(),
                              open(os.path.join(g, "pr2_right_arm.urdf")).read(), acm)


def pose(rpy, t):
    """3x4 [Rz(yaw) Ry(pitch) Rx(roll) | t]"""
    (sr, cr), (sp, cp), (sy, cy) = ((math.sin(a), math.cos(a)) for a in rpy)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, t[0]],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, t[1]],
                     [-sp, cp * sr, cp * cr, t[2]]])


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
            "calls": int(ms.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rows", default="")
    ap.add_argument("--save-rows", default="")
    a = ap.parse_args()
    L = capi.lib()
    if L.smplx_device_count() == 0:
        sys.exit("no GPU: nothing is measured without one")
    hip = C.CDLL("libamdhip64.so")
    by_shape = hasattr(L, "smplx_attach_object")
    cfg = cfg3()
    link = "r_gripper_palm_link"
    touch = [l.split()[1] for l in cfg.robot_text.splitlines() if l.startswith("link r_gripper_")]
    s = capi.Space.from_config(cfg)
    shapes = None
    if by_shape:
        shapes = [capi.box((0.06, 0.04, 0.10), pose((0.3, -0.2, 0.5), (0.25, 0.01, -0.02))),
                  capi.cylinder(0.03, 0.12, pose((0.1, 1.3, -0.4), (0.24, -0.01, 0.02)))]
        rows, first = s.object_spheres(shapes)
        if a.save_rows:
            np.save(a.save_rows, rows)
    else:
        rows = np.load(a.rows)

    def clock(f):
        assert hip.hipDeviceSynchronize() == 0
        t0 = time.perf_counter()
        f()
        assert hip.hipDeviceSynchronize() == 0
        return 1e3 * (time.perf_counter() - t0)

    T = {k: [] for k in ("attach_object_ms", "attach_body_ms", "object_spheres_ms", "detach_ms", "vox_kernels_ms")}
    for r in range(a.reps + 3):
        t = {}
        if by_shape:
            L.smplx_test_voxelize_kernel_ms.restype = C.c_double
            L.smplx_test_voxelize_timing(1)
            s.object_spheres(shapes)
            t["vox_kernels_ms"] = float(L.smplx_test_voxelize_kernel_ms())
            L.smplx_test_voxelize_timing(0)
            t["object_spheres_ms"] = clock(lambda: s.object_spheres(shapes))
            t["attach_object_ms"] = clock(lambda: s.attach_object("held", link, shapes, allowed=touch))
            s.detach_body("held")
        t["attach_body_ms"] = clock(lambda: s.attach_body("held", link, rows, allowed=touch))
        t["detach_ms"] = clock(lambda: s.detach_body("held"))
        if r >= 3:
            for k, v in t.items():
                T[k].append(v)
    res = {"measure": "attach_object", "config": "cfg3 PR2 right arm", "spheres": int(len(rows)), "nodes": int(2 * len(rows) - 1),
           "by_shape": bool(by_shape), "specialized": bool(s.specialized()[0])}
    res.update({k: stats(v) for k, v in T.items() if v})
    if by_shape:
        res["attach_object_over_attach_body"] = round(res["attach_object_ms"]["median_ms"] / res["attach_body_ms"]["median_ms"], 2)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
