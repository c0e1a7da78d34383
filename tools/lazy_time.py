"""The three measurements of the lazy successor pair (profiles/lazy_ab.txt records them), one JSON
line each, in one process on one GPU:

  true_cost   k_true_cost against k_edge_valid on the same 4096 (state, primitive) edges of cfg 2: both through their
              synchronous host entry points (smplx_true_cost_q_batch, smplx_cc_edge_valid_batch: upload, one launch, download),
              alternating, host clock around each call; and k_true_cost alone through its device form, HIP events
  lazy_succs  k_lazy_succs against the engine's frontier step (smplx_expand_batch_device, the one-launch k_step_block where
              the batch is resident) on the same B = 4096 states of cfg 2, device forms, HIP events, alternating
  loops       tests/cpp/lazy_loop_driver.cpp against tests/cpp/sbpl_loop_driver.cpp on small_cfg, each to its first solution
              at eps 5: wall time inside the loop, expansions, edge checks, cache hit rate of GetTrueCost

    python tools/lazy_time.py [--reps R] [--generic] [--only true_cost|lazy_succs|loops]

Kernel times proper come from a rocprofv3 --kernel-trace --stats run of this script (--only true_cost / lazy_succs)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch   # before the engine's library: one HIP runtime in the process, the one torch brings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smpl_amd import capi, scenes  # noqa: E402
from smpl_amd.plugin_tools import build_driver, write_query  # noqa: E402

F_INACTIVE = 0x10
N_ITEMS = 4096


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
            "calls": int(ms.size)}


def event_times(launches, reps, warmup=3):
    """launches: {name: f(stream)}; alternates them, HIP events around each launch"""
    st = torch.cuda.current_stream()
    for _ in range(warmup):
        for f in launches.values():
            f(st.cuda_stream)
    torch.cuda.synchronize()
    ev = {k: [] for k in launches}
    for _ in range(reps):
        for k, f in launches.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            f(st.cuda_stream)
            e1.record(st)
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def space2(generic):
    cfg = scenes.config2()
    s = capi.Space.from_config(cfg, generic_kernels=generic)
    s.set_goal_joint(cfg.goal, cfg.goal_tol)
    return cfg, s


def true_cost(a):
    cfg, s = space2(a.generic)
    Q = scenes.random_states(scenes.ARM7_LIMITS, N_ITEMS, 4242)
    rows = s.lazy_expand_batch(Q)
    si, pi = np.nonzero((rows["flags"] & F_INACTIVE) == 0)
    si, pi = si[:N_ITEMS], pi[:N_ITEMS]
    assert si.size == N_ITEMS
    pq = np.ascontiguousarray(Q[si]); sq = np.ascontiguousarray(rows["q"][si, pi]); cc = np.ascontiguousarray(rows["coord"][si, pi])
    ge = np.zeros(N_ITEMS, np.uint8)
    host = {"k_true_cost": [], "k_edge_valid": []}
    for r in range(a.reps + 3):
        t0 = time.perf_counter(); cost, prim, nm = s.true_cost_q_batch(pq, cc, ge); t1 = time.perf_counter()
        ok, lk, w = s.edge_valid_batch(pq, sq); t2 = time.perf_counter()
        if r >= 3:
            host["k_true_cost"].append(1e3 * (t1 - t0)); host["k_edge_valid"].append(1e3 * (t2 - t1))
    lim = s.check_joint_limits(sq).astype(bool)
    # the two agree where they answer the same question: an edge within limits passes GetTrueCost iff the edge check passes
    # (items that share their cell with another action aside)
    single = nm == 1
    assert np.array_equal((cost > 0)[single], (ok.astype(bool) & lim)[single])
    d = [torch.from_numpy(x).cuda() for x in (pq, cc, ge)]
    work = torch.zeros(s.true_cost_work_doubles(N_ITEMS), dtype=torch.float64, device="cuda"); out = torch.zeros((3, N_ITEMS), dtype=torch.int32, device="cuda")
    dev = event_times({"k_true_cost": lambda st: s.true_cost_q_batch_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), N_ITEMS,
                                                                           work.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                                           out[2].data_ptr(), st)}, a.reps)
    res = {"measure": "true_cost", "config": "cfg2", "items": N_ITEMS, "prims": s.M, "specialized": s.specialized()[0],
           "host_call": {k: stats(v) for k, v in host.items()}, "device_launch": dev,
           "pass_share": round(float((cost > 0).mean()), 4), "limits_share": round(float((~lim).mean()), 4),
           "collision_share": round(float((lim & ~ok.astype(bool)).mean()), 4), "mean_waypoints": round(float(w.mean()), 2)}
    res["host_ratio"] = round(res["host_call"]["k_true_cost"]["median_ms"] / res["host_call"]["k_edge_valid"]["median_ms"], 2)
    print(json.dumps(res))


def lazy_succs(a):
    cfg, s = space2(a.generic)
    B, M, N = N_ITEMS, s.M, s.N
    Q = scenes.random_states(scenes.ARM7_LIMITS, B, 4242)
    dq = torch.from_numpy(Q).cuda()
    flags = torch.zeros(B * M, dtype=torch.uint8, device="cuda")
    coord = torch.zeros(B * M * N, dtype=torch.int32, device="cuda"); sq = torch.zeros(B * M * N, dtype=torch.float64, device="cuda")
    h, cost, lk, sid = (torch.zeros(B * M, dtype=torch.int32, device="cuda") for _ in range(4))
    work = torch.zeros(s.expand_work_bytes(B), dtype=torch.uint8, device="cuda")
    before = s.one_launch_steps()
    t = event_times({
        "k_lazy_succs": lambda st: s.lazy_expand_batch_device(dq.data_ptr(), B, flags.data_ptr(), coord.data_ptr(), sq.data_ptr(),
                                                              h.data_ptr(), sid.data_ptr(), st),
        "frontier_step": lambda st: s.expand_batch_device(dq.data_ptr(), B, flags.data_ptr(), coord.data_ptr(), sq.data_ptr(), h.data_ptr(),
                                                          cost.data_ptr(), lk.data_ptr(), work.data_ptr(), None, st)}, a.reps)
    res = {"measure": "lazy_succs", "config": "cfg2", "B": B, "prims": M, "specialized": s.specialized()[0], "device_launch": t,
           "one_launch_steps": s.one_launch_steps() - before,
           "step_over_lazy": round(t["frontier_step"]["median_ms"] / t["k_lazy_succs"]["median_ms"], 2)}
    print(json.dumps(res))


def loops(a):
    cfg = scenes.config_small()
    tmp = tempfile.mkdtemp()
    out = {"measure": "loops", "config": "small_cfg", "eps": 5.0}
    for name, tail in (("lazy_loop_driver", [5.0, 1500]), ("sbpl_loop_driver", [5.0, 5.0, 1.0, 0, 0])):
        exe = build_driver(name, tmp)
        write_query(cfg, tmp, tail)
        runs = []
        for _ in range(3):
            t0 = time.perf_counter()
            p = subprocess.run([exe, tmp], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
            wall = time.perf_counter() - t0
            assert p.returncode == 0, p.stderr.decode()[-1000:]
            lines = {l.split(" ", 1)[0]: l.split(" ", 1)[1] if " " in l else "" for l in p.stdout.decode().splitlines()}
            kv = dict(x.split("=") for x in lines["stats"].split())
            if name == "lazy_loop_driver":
                runs.append(dict(loop_seconds=float(kv["seconds"]), process_seconds=round(wall, 3), expansions=int(kv["expansions"]),
                                 edge_checks=int(kv["edges_evaluated"]), true_cost_calls=int(kv["evaluated"]),
                                 cache_hit_rate=round(int(kv["cache_hits"]) / max(1, int(kv["cache_hits"]) + int(kv["cache_misses"])), 3),
                                 launches=int(kv["lazy_launches"]) + int(kv["true_cost_launches"]), states=int(kv["states"]),
                                 cost=int(lines["cost"])))
            else:
                r = lines["result"].split()
                runs.append(dict(loop_seconds=float(r[4]), process_seconds=round(wall, 3), expansions=int(r[2]),
                                 edge_checks=int(kv["committed_succ_evals"]), gpu_evals=int(kv["gpu_succ_evals_total"]),
                                 launches=int(kv["gpu_batches"]), states=int(kv["states"]), cost=int(r[1])))
        best = min(runs, key=lambda r: r["loop_seconds"])
        best["loop_seconds_all"] = [r["loop_seconds"] for r in runs]
        out[name] = best
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--generic", action="store_true")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    if capi.lib().smplx_device_count() == 0:
        sys.exit("no GPU: nothing is measured without one")
    for name, f in (("true_cost", true_cost), ("lazy_succs", lazy_succs), ("loops", loops)):
        if not a.only or a.only == name:
            f(a)


if __name__ == "__main__":
    main()
