"""The body, the grid and the poses the robot-body tests share (tests/test_body_model.py asserts the conditions on the
model alone, on the CPU; tests/test_gpu_robot_body.py runs the engine against it).  Nothing is grid-aligned: origins and
joint values carry digits such as 0.0137 and 0.4321 rad."""
import functools
import math

import numpy as np

import body_ref as B

DIMS = (64, 48, 40)                      # non-cubic
RES = 0.02
MAX_DIST = 0.2
ORIGIN = (-0.3137, -0.4421, -0.1263)     # the grid spans x to 0.9663, y to 0.5179, z to 0.6737


def strip_mesh():
    """a bumpy strip of 5 x 4 quads: 30 vertices, 40 triangles"""
    v, t = [], []
    for i in range(6):
        for j in range(5):
            v.append((0.024 * i - 0.0571, 0.026 * j - 0.0493, 0.017 * math.sin(1.3 * i + 0.7 * j) + 0.0113))
    for i in range(5):
        for j in range(4):
            a, b, c, d = i * 5 + j, (i + 1) * 5 + j, (i + 1) * 5 + j + 1, i * 5 + j + 1
            t += [(a, b, c), (a, c, d)]
    return v, t


def body_text():
    v, t = strip_mesh()
    rows = [
        "robot testbody",
        "link base", "link l1", "link l2", "link s1", "link g1", "link tiny", "link edge", "link far",
        "joint j1 revolute base l1  0.3137 0.0237 0.2137  0.1 0.05 0.2  0 0 1  -3 3",
        "joint j2 revolute l1 l2  0.1 0.0137 0.1  0.03 -0.02 0.01  0 1 0  -3 3",
        "joint js continuous base s1  -0.0637 0.2137 0.3337  0.2 0.1 -0.3  0.6 0 0.8  0 0",
        "joint j3 revolute l2 g1  0.05 0.02 0.03  0 0 0  1 0 0  -3 3",
        "joint jt fixed s1 tiny  0.0437 0.0137 0.0237  0 0 0  0 0 1  0 0",
        "joint je fixed base edge  0.9537 0.5037 0.3037  0 0 0  0 0 1  0 0",
        "joint jf prismatic base far  2.0137 0.0137 0.2137  0 0 0  0 0 1  -1 1",
        "geom base box 0.13 0.21 0.07  0.2137 0.0137 0.1537  0.3 -0.2 0.4321",
        "geom l1 cylinder 0.04 0.15  0.0137 0.0037 0.05  0.2 0.1 0.0",
        "geom l1 sphere 0.035  0.02 0.03 0.14  0.0 0.0 0.0",
        "geom l2 mesh %d %d  0.0137 0.0237 0.0337  0.1 0.2 0.3" % (len(v), len(t)),
    ]
    rows += ["v %r %r %r" % p for p in v] + ["t %d %d %d" % q for q in t]
    rows += [
        "geom s1 box 0.09 0.05 0.11  0.0137 0.0237 0.0337  0.4 0.5 0.6",
        "geom g1 box 0.1 0.08 0.06  0 0 0  0 0 0",             # axis-aligned: faces on lattice boundaries
        "geom tiny sphere 0.002  0.0051 0.0049 0.0052  0 0 0",   # inside one voxel of the lattice
        "geom edge box 0.1 0.1 0.1  0.0 0.0 0.0  0.1 0.2 0.3",   # across the grid's high x and high y faces
        "geom far sphere 0.03  0.0013 0.0027 0.0031  0.1 0.2 0.3",                   # wholly outside
        "voxels base 0.01", "voxels l1 0.01", "voxels l2 0.01", "voxels s1 0.01", "voxels g1 0.01", "voxels tiny 0.01",
        "voxels edge 0.01", "voxels far 0.01",
        "group arm g1",
        "value j1 0.4321", "value j2 -0.2137", "value js 0.3137", "value jf 0.0137",
    ]
    return "\n".join(rows) + "\n"


MODELS = ["base", "l1", "l2", "s1", "g1", "tiny", "edge", "far"]
GROUP_MODEL = 4          # g1: in the group, never placed; its axis-aligned box is the one judged under the 15 % rule
SECOND_Q = ("j2", 0.5137)   # the middle joint: moves l2 (and g1, which is never placed)


@functools.lru_cache(maxsize=None)
def model():
    return B.Body(body_text())


@functools.lru_cache(maxsize=None)
def model_points(m):
    return model().model_points(m)
