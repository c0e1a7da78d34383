"""The measurement of octree world objects (profiles/octree_ab.txt records it): builds tools/octree_time.cpp against the
library and runs it on the 4097-leaf octree of the tests (tests/octree_cases.py "cloud", under the rotated pose) on a grid
of 256^3 cells of 0.02 m.  The program compares smplx_world_insert_object with the route the engine offered before -- the
reference's loops run on the host, in C++, and the points handed to smplx_grid_add_points -- and prints one JSON line; see
its head for the legs.

    python tools/octree_time.py [--reps R]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import octree_cases as T  # noqa: E402
from smpl_amd import build, capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    if capi.lib().smplx_device_count() == 0:
        sys.exit("no GPU: nothing is measured without one")
    lib = build.build()
    with tempfile.TemporaryDirectory() as d:
        exe, rows = os.path.join(d, "octree_time"), os.path.join(d, "leaves.bin")
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "octree_time.cpp"),
                               "-o", exe, lib, f"-Wl,-rpath,{os.path.dirname(lib)}", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"])
        np.ascontiguousarray(T.leaves("cloud"), np.float64).tofile(rows)
        pose = [repr(float(x)) for x in np.asarray(T.POSES["rotated"]).ravel()]
        subprocess.check_call([exe, rows] + pose + [str(a.reps)])


if __name__ == "__main__":
    main()
