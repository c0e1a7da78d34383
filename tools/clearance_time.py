"""Time per launch of k_state_clearance beside k_state_valid on the same 2^20 random states of the cfg-3 PR2 right arm, in
one process: HIP events on the launch stream around each launch, warm-up first, median and range.  Prints one JSON line
(profiles/clearance_ab.txt records it).

    python tools/clearance_time.py [--states N] [--reps R] [--generic]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smpl_amd import capi, scenes  # noqa: E402


def cfg3():
    g = os.path.join(ROOT, "tests", "golden")
    acm = json.load(open(os.path.join(g, "pr2_right_arm_acm.json")))["allowed_pairs"]
    return scenes.config3_pr2(open(os.path.join(g, "collision_model_pr2.yaml")).read(),
                              open(os.path.join(g, "pr2_right_arm.urdf")).read(), acm)


def time_launches(launch, reps, warmup=3):
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        launch(st.cuda_stream)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record(st)
        launch(st.cuda_stream)
        e1.record(st)
    torch.cuda.synchronize()
    ms = np.array([e0.elapsed_time(e1) for e0, e1 in ev])
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
            "launches": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--generic", action="store_true")
    a = ap.parse_args()
    cfg = cfg3()
    n = a.states
    Q = scenes.benchmark_states(scenes.ARM7_LIMITS, n, 12345)
    s = capi.Space.from_config(cfg, generic_kernels=a.generic)
    dq = torch.from_numpy(Q).cuda()
    dv = torch.zeros(n, dtype=torch.uint8, device="cuda")
    dl = torch.zeros(n, dtype=torch.int32, device="cuda")
    dc = torch.zeros(n, dtype=torch.float64, device="cuda")
    dp = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
    dw = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    out = {"config": "cfg3 PR2 right arm", "states": n, "specialized": s.specialized()[0]}
    out["k_state_valid"] = time_launches(lambda st: s.state_valid_batch_device(dq.data_ptr(), n, dv.data_ptr(), dl.data_ptr(), st), a.reps)
    out["k_state_clearance"] = time_launches(
        lambda st: s.state_clearance_batch_device(dq.data_ptr(), n, dc.data_ptr(), dp.data_ptr(), dw.data_ptr(), st), a.reps)
    out["clearance_over_valid"] = round(out["k_state_clearance"]["median_ms"] / out["k_state_valid"]["median_ms"], 2)
    out["valid_share"] = round(float(dv.float().mean().item()), 4)
    out["clear_share"] = round(float((dc > 1e-9).double().mean().item()), 4)
    out["witness_kinds"] = sorted(set(dw[:, 0].cpu().numpy().tolist()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
