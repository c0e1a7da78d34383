"""Goal setup of a 128-query shard: 128 x smplx_set_goal_joint against one smplx_set_goals_joint_multi.

The cfg-2 grid (256^3) and the 128 goals of shard 0 of config 4.  One warm-up pass of each method, then `--pairs`
pairs in one process, alternating the two methods; a host clock around calls that end in a stream synchronise.  Per
method: every run's time, the median and the spread (max - min); the launches of each method (FK + seed + passes, counted
from smplx_bfs_levels) and the pass count of the shared sequence.  A check that both methods leave the same grids runs
once, outside the timed region.

    python tools/goal_setup_time.py [--pairs 5] [--goals 128] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smpl_amd import capi, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--goals", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = scenes.config2()
    grid = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    model = capi.Model(cfg.robot_text)
    probe = capi.Space(model, grid, cfg.mprim, cfg.params, 256)
    cs, cg = scenes.config4_candidates()
    _, G = scenes.config4_queries(cs, cg, probe.state_valid_batch(cs)[0], probe.state_valid_batch(cg)[0])
    first, last = scenes.shard_range(0, 8)
    G = np.ascontiguousarray(G[first:last][:a.goals])
    n = G.shape[0]
    tols = np.tile(np.asarray(cfg.goal_tol, dtype=np.float64), (n, 1))
    loop_spaces = [capi.Space(model, grid, cfg.mprim, cfg.params, 1024) for _ in range(n)]
    multi_spaces = [capi.Space(model, grid, cfg.mprim, cfg.params, 1024) for _ in range(n)]

    def loop():
        t0 = time.perf_counter()
        for sp, g in zip(loop_spaces, G):
            sp.set_goal_joint(g, cfg.goal_tol)
        return time.perf_counter() - t0

    def multi():
        t0 = time.perf_counter()
        capi.Space.set_goals_joint_multi(multi_spaces, G, tols)
        return time.perf_counter() - t0

    lines = [f"goal setup, {n} goals of config-4 shard 0 on the cfg-2 grid {cfg.grid.dims}, {a.pairs} alternating pairs after one warm-up of each"]
    w_loop, w_multi = loop(), multi()
    lines.append(f"warm-up (first run, launches not yet sized by a previous run): loop {w_loop:.6f} s, multi {w_multi:.6f} s")
    same = all(np.array_equal(loop_spaces[k].bfs_grid(), multi_spaces[k].bfs_grid()) for k in range(0, n, max(1, n // 8)))
    lines.append(f"grids of every {max(1, n // 8)}th space equal between the methods: {same}")
    t_loop, t_multi = [], []
    for _ in range(a.pairs):
        t_loop.append(loop())
        t_multi.append(multi())
    loop_levels = [sp.bfs_levels() for sp in loop_spaces]
    shared = multi_spaces[0].bfs_levels()
    for name, t in [("loop  (128 x set_goal_joint)", t_loop), ("multi (one set_goals_joint_multi)", t_multi)]:
        lines.append(f"{name}: runs " + " ".join(f"{x:.6f}" for x in t) + f" s; median {statistics.median(t):.6f} s; "
                     f"spread (max - min) {max(t) - min(t):.6f} s")
    lines.append(f"launches per run: loop {n} FK + {n} seed + {sum(loop_levels)} passes = {2 * n + sum(loop_levels)} "
                 f"(passes per goal {min(loop_levels)}..{max(loop_levels)}); multi 1 FK + 1 seed + {shared} passes = {2 + shared}")
    lines.append(f"passes of the shared sequence: {shared}")
    lines.append(f"ratio of medians loop / multi: {statistics.median(t_loop) / statistics.median(t_multi):.2f}")
    lines.append(f"slowest multi run {max(t_multi):.6f} s {'<' if max(t_multi) < min(t_loop) else '>='} fastest loop run {min(t_loop):.6f} s")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
