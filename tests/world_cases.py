"""Shapes, grid and judged cell lists shared by the world-object tests (tests/test_voxelize_model.py,
tests/test_gpu_world_objects.py).  The model's answers are computed once per process and never changed."""
import functools
import math

import numpy as np

import voxelize_ref as V

ORIGIN = (-0.1, -0.2, 0.05)
DIMS = (40, 40, 32)
RES = 0.02
MAX_DIST = 0.2
EPS = 1e-9


def _rx(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def _ry(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def _rz(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def pose(xyz=(0.0, 0.0, 0.0), R=None):
    P = np.zeros((3, 4))
    P[:, :3] = np.eye(3) if R is None else R
    P[:, 3] = xyz
    return P


ROT = _rz(0.5) @ _ry(-0.4) @ _rx(0.3)
POSE = pose((0.21, 0.13, 0.37), ROT)


def shape(ty, dims=(), at=None, **more):
    d = tuple(float(x) for x in dims) + (0.0,) * (3 - len(dims))
    return dict(type=ty, dims=d, pose=POSE if at is None else at, **more)


def soup():
    rng = np.random.default_rng(7)
    v = rng.uniform(-0.15, 0.15, (30, 3))
    t = rng.integers(0, 30, (40, 3))
    return shape(V.MESH, vertices=v, triangles=t)


def subdivided_box(ntri=4097, seed=11):
    """the box's 12 triangles, a seeded pick split at the midpoint of its longest edge until there are ntri"""
    v, t = V.box_mesh(0.3, 0.26, 0.22)
    v, t = [tuple(x) for x in v], [tuple(x) for x in t]
    rng = np.random.default_rng(seed)
    while len(t) < ntri:
        k = int(rng.integers(len(t)))
        a, b, c = t[k]
        for _ in range(3):      # rotate until (a, b) is the longest edge
            lab, lbc, lca = (sum((v[i][d] - v[j][d]) ** 2 for d in range(3)) for i, j in ((a, b), (b, c), (c, a)))
            if lab >= lbc and lab >= lca:
                break
            a, b, c = b, c, a
        v.append(tuple(0.5 * (v[a][d] + v[b][d]) for d in range(3)))
        m = len(v) - 1
        t[k] = (a, m, c)
        t.append((m, b, c))
    return shape(V.MESH, vertices=np.array(v), triangles=np.array(t))


def one_triangle():
    return shape(V.MESH, at=pose(), vertices=[(0.053, 0.004, 0.207), (0.431, 0.113, 0.312), (0.204, 0.377, 0.523)], triangles=[(0, 1, 2)])


def big_and_small(nsmall=300, seed=5):
    """one triangle spanning the whole grid (its vertices lie far outside) with many of about one voxel"""
    rng = np.random.default_rng(seed)
    v = [(-0.5, -0.5, 0.1), (1.5, -0.3, 0.6), (0.2, 1.5, 0.4)]
    t = [(0, 1, 2)]
    for _ in range(nsmall):
        c = rng.uniform((0.0, -0.1, 0.1), (0.6, 0.5, 0.6))
        k = len(v)
        v += [tuple(c + rng.uniform(-0.003, 0.003, 3)) for _ in range(3)]
        t.append((k, k + 1, k + 2))
    return shape(V.MESH, at=pose(), vertices=np.array(v), triangles=np.array(t))


# the five trial cases of the issue and a cone; "aligned" sits on exact ties
SHAPES = {
    "box": shape(V.BOX, (0.13, 0.21, 0.07)),
    "sphere": shape(V.SPHERE, (0.11,)),
    "cylinder": shape(V.CYLINDER, (0.06, 0.23)),
    "soup": soup(),
    "aligned": shape(V.BOX, (0.4, 0.5, 0.02), at=pose((0.3, 0.1, 0.35))),
    "cone": shape(V.CONE, (0.07, 0.15)),
}
TRIAL_CELLS = {"box": 409, "sphere": 572, "cylinder": 436, "soup": 1156, "aligned": 1182}
# a sphere across the low x and low y faces of the grid, and one wholly outside
STRADDLE = shape(V.SPHERE, (0.11,), at=pose((ORIGIN[0] + 0.03, ORIGIN[1] + 0.05, 0.3), ROT))
OUTSIDE = shape(V.SPHERE, (0.11,), at=pose((5.0, 5.0, 5.0)))


@functools.lru_cache(maxsize=None)
def _judged(key):
    s = EXTRA[key]() if key in EXTRA else SHAPES[key]
    cells, und = V.voxelize_shape(s, ORIGIN, RES, clip=DIMS, eps=EPS)
    cells.setflags(write=False)
    und.setflags(write=False)
    return s, cells, und


EXTRA = {"subdivided": subdivided_box, "one_triangle": one_triangle, "big_and_small": big_and_small,
         "straddle": lambda: STRADDLE, "outside": lambda: OUTSIDE}


def judged(key):
    """(shape, the model's cells inside the grid in ExtractVoxels order, the cells undecided at EPS)"""
    return _judged(key)


def world_points(cells):
    """voxel centres of cells: what the parent's route hands to add_points"""
    c = np.asarray(cells, float).reshape(-1, 3)
    return np.asarray(ORIGIN) + c * RES


def compare(got, key):
    """the rule of the issue: undecided cells are left out; everything else equal as sets and in order"""
    _, want, und = judged(key)
    u = set(map(tuple, und))
    g = [c for c in map(tuple, np.asarray(got).reshape(-1, 3)) if c not in u]
    w = [c for c in map(tuple, want) if c not in u]
    assert len(set(g)) == len(g), key + ": a cell listed twice"
    assert set(g) == set(w), "%s: %d cells only here, %d only in the model" % (key, len(set(g) - set(w)), len(set(w) - set(g)))
    assert g == w, key + ": order"
    return len(want), len(und)
