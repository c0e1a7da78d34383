"""Post-processing of a shard's paths: a loop of smplx_post_process_path against one smplx_post_process_paths call.

The cfg-2 grid (256^3) and the queries of shard 0 of config 4, planned with smplx_plan_multi (eps 5 -> 1, the benchmark's
expansion bound); the input is the extracted paths of the solved ones.  Mode (shortcut, interpolate, upstream limits).
  A   for every path one smplx_post_process_path.  With --parent-lib it runs in a libsmpl_amd.so built from the parent
      commit, loaded beside this build's, on a space of its own over a copy of the grid (the paths' spaces carry no
      bodies, so one space answers for all); without it, in this build, whose single call is the parent's text.
  B   one smplx_post_process_paths call over the paths' own spaces.
One warm-up of each, then `--pairs` alternating pairs in one process; a host clock around calls that end in a stream
synchronise.  Per method and batch size (--sizes, default 1 16 all): every run's time, the median, the spread, and the
counters each reports.  That A and B return the same bytes is checked once per size, outside the timed region.

    python tools/post_process_multi_time.py [--pairs 7] [--queries 128] [--parent-lib FILE] [--out FILE]
"""
import argparse
import ctypes as C
import os
import socket
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from smpl_amd import capi, scenes  # noqa: E402

_dp, _ip = capi._dp, capi._ip


class ParentSpace:
    """one space in another build of the library: grid, model and space made and used through that library alone"""

    def __init__(self, path, cfg):
        L = C.CDLL(path)
        L.smplx_last_error.restype = C.c_char_p
        self.L = L
        o = np.ascontiguousarray(cfg.grid.origin, np.float64)
        d2 = np.ascontiguousarray(cfg.grid.d2, np.int32)
        self.g, self.m, self.h = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.smplx_grid_create.argtypes = [_dp, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _ip, C.POINTER(C.c_void_p)]
        L.smplx_model_create.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.smplx_space_create.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(capi.Params), C.POINTER(C.c_void_p)]
        L.smplx_post_process_path.argtypes = [C.c_void_p, _dp, C.c_int, C.c_int, _dp, C.c_int, _ip, C.POINTER(C.c_int64)]
        self._chk(L.smplx_grid_create(o.ctypes.data_as(_dp), *cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, d2.ctypes.data_as(_ip), C.byref(self.g)))
        self._chk(L.smplx_model_create(cfg.robot_text.encode(), C.byref(self.m)))
        p, P = cfg.params, capi.Params()
        for i, r in enumerate(p.resolutions):
            P.resolutions[i] = r
        P.bfs_inflation_radius, P.cost_per_cell = p.bfs_radius, p.cost_per_cell
        P.use_short_dist_mprims, P.short_dist_mprims_thresh = int(p.use_short), p.short_thresh
        P.use_xyzrpy_snap_mprim, P.xyzrpy_snap_dist_thresh = int(p.use_xyzrpy_snap), p.xyzrpy_thresh
        P.xy_rotate_by_var3, P.use_long_and_short = int(p.xy_rotate_by_var3), int(p.use_long_and_short)
        P.batch_states = 1024
        self._chk(L.smplx_space_create(self.m, self.g, cfg.mprim.encode(), C.byref(P), C.byref(self.h)))
        self.N = L.smplx_space_num_vars(self.h)

    def _chk(self, code):
        if code != 0:
            raise RuntimeError(f"parent library: error {code}: {self.L.smplx_last_error().decode()}")

    def post_process_path(self, path, shortcut=True, interpolate=True, upstream_limits=False):
        path = np.ascontiguousarray(path, np.float64).reshape(-1, self.N)
        flags = (1 if shortcut else 0) | (2 if interpolate else 0) | (4 if upstream_limits else 0)
        n = C.c_int()
        st = (C.c_int64 * 2)()
        f = self.L.smplx_post_process_path
        self._chk(f(self.h, path.ctypes.data_as(_dp), path.shape[0], flags, None, 0, C.byref(n), st))
        out = np.zeros((max(n.value, 1), self.N))
        self._chk(f(self.h, path.ctypes.data_as(_dp), path.shape[0], flags, out.ctypes.data_as(_dp), out.shape[0], C.byref(n), st))
        return out[:n.value], dict(edge_batches=st[0], configs=st[1])


def device_name():
    try:
        import torch
        return torch.cuda.get_device_name(0)
    except Exception:
        pass
    try:
        import subprocess
        out = subprocess.run(["/opt/rocm/bin/rocminfo"], capture_output=True, text=True, timeout=60).stdout
        names = [l.split(":", 1)[1].strip() for l in out.splitlines() if "Marketing Name" in l]
        gpus = [n for n in names if "Instinct" in n or "MI3" in n]
        return (gpus or names or ["device name not available"])[0]
    except Exception:
        return "device name not available"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--queries", type=int, default=128, help="queries of shard 0 to plan: a prefix when the visit is short")
    ap.add_argument("--expansions", type=int, default=20000)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1, 16, 0], help="batch sizes, 0 = every path")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    mode = (True, True, True)
    cfg = scenes.config2()
    grid = capi.Grid(cfg.grid.origin, cfg.grid.dims, cfg.grid.res, cfg.grid.max_dist, cfg.grid.d2)
    model = capi.Model(cfg.robot_text)
    probe = capi.Space(model, grid, cfg.mprim, cfg.params, 256)
    cs, cg = scenes.config4_candidates()
    S, G = scenes.config4_queries(cs, cg, probe.state_valid_batch(cs)[0], probe.state_valid_batch(cg)[0])
    first, last = scenes.shard_range(0, 8)
    S, G = S[first:last][:a.queries], np.ascontiguousarray(G[first:last][:a.queries])
    n = G.shape[0]
    spaces = [capi.Space(model, grid, cfg.mprim, cfg.params, 1024) for _ in range(n)]
    capi.Space.set_goals_joint_multi(spaces, G, np.tile(np.asarray(cfg.goal_tol, dtype=np.float64), (n, 1)))
    for sp, s in zip(spaces, S):
        sp.set_start(s)
    p = cfg.params
    res, wall = capi.Space.plan_multi(spaces, p.eps0, p.eps_final, p.eps_delta, True, True, a.expansions, a.expansions)
    solved = [k for k in range(n) if res[k]["solved"]]
    paths = [spaces[k].extract_path(res[k]["path"]) for k in solved]
    sp_of = [spaces[k] for k in solved]
    single = ParentSpace(a.parent_lib, cfg) if a.parent_lib else probe

    lines = [f"post-processing of the planned paths of config-4 shard 0 on the cfg-2 grid {cfg.grid.dims}: queries [0, {n}) of the shard "
             f"planned with smplx_plan_multi (eps {p.eps0} -> {p.eps_final}, bound {a.expansions}) in {wall:.3f} s, {len(solved)} solved",
             f"box {socket.gethostname()}, {device_name()}; mode (shortcut, interpolate, upstream limits); "
             f"{a.pairs} alternating pairs after one warm-up of each",
             "A = a loop of smplx_post_process_path, " + (f"in the parent commit's build ({os.path.basename(a.parent_lib)} loaded beside this one)"
                                                           if a.parent_lib else "in THIS build (no --parent-lib given)"),
             "B = one smplx_post_process_paths call",
             f"path lengths: {min(len(q) for q in paths)}..{max(len(q) for q in paths)} points, {sum(len(q) for q in paths)} in all"]
    ok = True
    for size in a.sizes:
        nq = len(paths) if size <= 0 else min(size, len(paths))
        P, SP = paths[:nq], sp_of[:nq]

        def run_a():
            t0 = time.perf_counter()
            outs = [single.post_process_path(q, *mode) for q in P]
            return time.perf_counter() - t0, outs

        def run_b():
            t0 = time.perf_counter()
            outs, st = capi.post_process_paths(SP, P, *mode)
            return time.perf_counter() - t0, (outs, st)

        (wa, oa), (wb, (ob, stb)) = run_a(), run_b()
        same = all(x[0].shape == y.shape and np.array_equal(x[0], y) for x, y in zip(oa, ob))
        ok = ok and same
        ta, tb = [], []
        for _ in range(a.pairs):
            ta.append(run_a()[0])
            tb.append(run_b()[0])
        batches = sum(x[1]["edge_batches"] for x in oa)
        configs = sum(x[1]["configs"] for x in oa)
        lines.append(f"--- nq = {nq}: outputs of A and B equal, byte for byte: {same}; {sum(len(y) for y in ob)} output points")
        lines.append(f"warm-up: A {wa:.6f} s, B {wb:.6f} s")
        for name, t in (("A", ta), ("B", tb)):
            lines.append(f"{name}: runs " + " ".join(f"{x:.6f}" for x in t) + f" s; median {statistics.median(t):.6f} s; "
                         f"spread (max - min) {max(t) - min(t):.6f} s")
        lines.append(f"A stats: {batches} edge batches (each a launch, a copy back and a wait) + the passes' batches, {configs} configurations checked "
                     f"(size query and output call together); B stats of one call: launches {stb['launches']}, host waits {stb['waits']}, "
                     f"configurations {stb['configs']}, paths {stb['paths']} (the wrapper calls twice: size query, then output)")
        lines.append(f"ratio of medians A / B: {statistics.median(ta) / statistics.median(tb):.2f}")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    sys.stdout.flush()
    # the parent library's handles are left to the process's end: this build's destructors must not see them
    os._exit(0 if ok else 1)


if __name__ == "__main__":
    sys.exit(main())
