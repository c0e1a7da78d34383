"""K2 checks/s (2^20 random states through k_state_valid) on the cfg-3 PR2 right arm with no attached body and with a
~200-leaf box held between the fingers of r_gripper_palm_link, which with the finger links are its touch links
(6 x 6 x 12 cm at the reference's 1.77 cm voxel pitch, radius 0.025 m:
attached_bodies_collision_model.cpp:264-313; spheres filled by formats.box_spheres, not the reference's mesh
voxeliser).  Prints one JSON line.

    python tools/attached_time.py [--states N] [--reps R]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smpl_amd import capi, formats, scenes  # noqa: E402


def cfg3():
    g = os.path.join(ROOT, "tests", "golden")
    acm = json.load(open(os.path.join(g, "pr2_right_arm_acm.json")))["allowed_pairs"]
    return scenes.config3_pr2(open(os.path.join(g, "collision_model_pr2.yaml")).read(),
                              open(os.path.join(g, "pr2_right_arm.urdf")).read(), acm)


def time_k2(space, Q, reps):
    n = Q.shape[0]
    dq = torch.from_numpy(Q).cuda()
    dv = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dl = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream()
    for _ in range(2):
        space.state_valid_batch_device(dq.data_ptr(), n, dv.data_ptr(), dl.data_ptr(), st.cuda_stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    for _ in range(reps):
        space.state_valid_batch_device(dq.data_ptr(), n, dv.data_ptr(), dl.data_ptr(), st.cuda_stream)
    e1.record(st)
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    return {"ms": round(ms, 4), "checks_per_s": round(n / (ms * 1e-3), 1), "valid": int(dv.sum().item()),
            "lookups": int(dl.sum(dtype=torch.int64).item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    cfg = cfg3()
    Q = scenes.benchmark_states(scenes.ARM7_LIMITS, a.states, 12345)
    link = "r_gripper_palm_link"
    box = formats.box_spheres((0.20, 0.0, 0.0), (0.06, 0.06, 0.12), 0.0177, 0.025)
    touch = [l.split()[1] for l in cfg.robot_text.splitlines() if l.startswith("link r_gripper_")]
    out = {"config": "cfg3 PR2 right arm, K2 (k_state_valid)", "states": a.states, "body_leaves": len(box), "touch_links": touch}
    s = capi.Space.from_config(cfg)
    out["specialized"] = s.specialized()[0]
    out["no_body"] = time_k2(s, Q, a.reps)
    s.attach_body("box", link, box, allowed=touch)
    out["body"] = time_k2(s, Q, a.reps)
    s.detach_body("box")
    out["after_detach"] = time_k2(s, Q, a.reps)
    out["body_over_no_body"] = round(out["body"]["ms"] / out["no_body"]["ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
