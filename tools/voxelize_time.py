"""The measurements of the world objects (profiles/world_objects_ab.txt records them), one JSON line
per case, in one process on one GPU.  Grid: 256^3 cells of 0.02 m, max_dist 0.2 m (an edit window reaches 10 cells).

Cases:   sphere     one sphere of radius 0.3 m (112 triangles)
         tabletop   the objects of tests/golden/tabletop.env through formats.env_objects (one box, 12 triangles)
         mesh       a height field of 224 x 224 quads: 100 352 triangles of about one voxel each
Per case, medians over --reps repetitions after a warm-up, alternating the legs inside each repetition:
         kernels_ms        k_vox_setup + k_vox_fill + both k_vox_compact launches of a smplx_world_voxelize call, HIP events
                           inside the library (the chunk-count round trip between them is not in it)
         voxelize_call_ms  the whole smplx_world_voxelize call without a cell download: host meshes and triangle list, uploads,
                           the launches, the chunk-count round trip
         insert_ms         smplx_world_insert_object: the above with the occupancy change, plus the field update
         remove_ms         smplx_world_remove_object
         add_points_ms     the parent's route for the same cells: the cell list handed to smplx_grid_add_points as world
                           points.  The host voxelisation that route needs first is EXCLUDED (the parent has none on the
                           GPU; tests/voxelize_ref.py takes seconds): this is the field edit alone
         move_ms           smplx_world_move_object to a pose 0.1 m away, against
         remove_insert_ms  smplx_world_remove_object followed by smplx_world_insert_object at that pose
Host clock around synchronous calls (each ends in a device synchronise).

    python tools/voxelize_time.py [--reps R] [--only sphere|tabletop|mesh]

Kernel times proper come from a rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from smpl_amd import capi, formats  # noqa: E402

ORIGIN, DIMS, RES, MAX_DIST = (-1.0, -2.5, 0.0), (256, 256, 256), 0.02, 0.2


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4), "max_ms": round(float(ms.max()), 4),
            "calls": int(ms.size)}


def height_field(n=224):
    xs, ys = np.linspace(0.0, 3.0, n + 1), np.linspace(-2.0, 1.5, n + 1)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    v = np.stack([X, Y, 2.0 + 0.3 * np.sin(3.0 * X) * np.cos(2.0 * Y)], axis=-1).reshape(-1, 3)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).ravel()
    t = np.concatenate([np.stack([a, a + n + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + 1], 1)])
    return v, t


def shifted(objects, d):
    out = []
    for name, shapes in objects:
        moved = []
        for s in shapes:
            P = np.array(s["pose"], float)
            P[:, 3] += d
            moved.append(dict(s, pose=P))
        out.append((name, moved))
    return out


def clock(f):
    t0 = time.perf_counter()
    f()
    return 1e3 * (time.perf_counter() - t0)


def case(name, objects, reps):
    L = capi.lib()
    L.smplx_test_voxelize_kernel_ms.restype = C.c_double
    g = capi.Grid.empty(ORIGIN, DIMS, RES, MAX_DIST)
    there = shifted(objects, np.array([0.1, 0.1, 0.1]))
    all_shapes = [s for _, shapes in objects for s in shapes]
    arr, n, keep = capi._shape_array(all_shapes)
    first = np.zeros(n + 1, np.int32)
    cells = np.vstack(g.voxelize(all_shapes))
    points = np.asarray(ORIGIN) + cells.astype(float) * RES
    ntri = sum(12 if s["type"] == capi.SHAPE_BOX else 112 if s["type"] == capi.SHAPE_SPHERE else len(s["triangles"]) for s in all_shapes)
    T = {k: [] for k in ("kernels_ms", "voxelize_call_ms", "insert_ms", "remove_ms", "add_points_ms", "move_ms", "remove_insert_ms")}
    window = 0
    for r in range(reps + 3):
        t = {}
        L.smplx_test_voxelize_timing(1)
        capi._chk(L.smplx_world_voxelize(g.h, arr, n, None, 0, capi._p(first, capi._ip)))
        t["kernels_ms"] = float(L.smplx_test_voxelize_kernel_ms())
        L.smplx_test_voxelize_timing(0)
        t["voxelize_call_ms"] = clock(lambda: capi._chk(L.smplx_world_voxelize(g.h, arr, n, None, 0, capi._p(first, capi._ip))))
        t["insert_ms"] = clock(lambda: [g.insert_object(k, s) for k, s in objects])
        window = g.last_edit_cells()
        t["move_ms"] = clock(lambda: [g.move_object(k, s) for k, s in there])
        t["remove_ms"] = clock(lambda: [g.remove_object(k) for k, _ in there])
        t["add_points_ms"] = clock(lambda: g.add_points(points))
        g.remove_points(points)
        for k, s in objects:
            g.insert_object(k, s)
        t["remove_insert_ms"] = clock(lambda: [(g.remove_object(k), g.insert_object(k, s)) for k, s in there])
        g.remove_all_objects()
        if r >= 3:
            for k, v in t.items():
                T[k].append(v)
    res = {"measure": "world_objects", "case": name, "grid": list(DIMS), "res": RES, "dmax_cells": int(np.ceil(MAX_DIST / RES)),
           "objects": len(objects), "shapes": n, "triangles": int(ntri), "cells": int(cells.shape[0]), "insert_window_cells": int(window)}
    res.update({k: stats(v) for k, v in T.items()})
    res["insert_over_add_points"] = round(res["insert_ms"]["median_ms"] / res["add_points_ms"]["median_ms"], 2)
    res["move_over_remove_insert"] = round(res["move_ms"]["median_ms"] / res["remove_insert_ms"]["median_ms"], 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    if capi.lib().smplx_device_count() == 0:
        sys.exit("no GPU: nothing is measured without one")
    text = open(os.path.join(ROOT, "tests", "golden", "tabletop.env")).read()
    v, t = height_field()
    cases = {"sphere": [("ball", [capi.sphere(0.3, capi.pose_at((1.0, 0.0, 1.5)))])],
             "tabletop": formats.env_objects(text),
             "mesh": [("terrain", [capi.mesh(v, t)])]}
    for name, objects in cases.items():
        if not a.only or a.only == name:
            case(name, objects, a.reps)


if __name__ == "__main__":
    main()
