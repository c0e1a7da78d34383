"""Shapes and judged sphere rows shared by the attach-by-shape tests (tests/test_attach_object_abi.py,
tests/test_gpu_attach_object.py, tests/test_gpu_attach_object_cpp.py).  The judge is tests/voxelize_ref.py on the lattice
of AttachedBodiesCollisionModel::generateSpheresModel (attached_bodies_collision_model.cpp:264-313): pivot (0, 0, 0),
res = radius / sqrt(2), no clip; a filled voxel (i, j, k) is the sphere {0.0 + i * res, 0.0 + j * res, 0.0 + k * res, radius}.
The answers are computed once per process and never changed.  Every comparison made with them is exact."""
import functools
import math

import numpy as np

import voxelize_ref as V

RADIUS = 0.025
RES = RADIUS / math.sqrt(2.0)


def pose(rpy=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0)):
    """3x4 [Rz(yaw) Ry(pitch) Rx(roll) | t], in scalar arithmetic"""
    sr, cr = math.sin(rpy[0]), math.cos(rpy[0])
    sp, cp = math.sin(rpy[1]), math.cos(rpy[1])
    sy, cy = math.sin(rpy[2]), math.cos(rpy[2])
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr, t[0]],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr, t[1]],
                     [-sp, cp * sr, cp * cr, t[2]]])


def _shape(ty, dims, rpy=(0.0, 0.0, 0.0), t=(0.0, 0.0, 0.0), **more):
    d = tuple(float(x) for x in dims) + (0.0,) * (3 - len(dims))
    return dict(type=ty, dims=d, pose=pose(rpy, t), **more)


# key -> (shape, spheres the judge makes)
CASES = {
    "box": (_shape(V.BOX, (0.06, 0.04, 0.10), (0.3, -0.2, 0.5), (0.25, 0.01, -0.02)), 122),
    "cyl": (_shape(V.CYLINDER, (0.03, 0.12), (0.1, 1.3, -0.4), (0.24, -0.01, 0.02)), 150),
    "sph": (_shape(V.SPHERE, (0.04,), (0.2, 0.1, 0.7), (0.26, 0.003, 0.001)), 95),
    "cone": (_shape(V.CONE, (0.04, 0.08), (-0.5, 0.2, 0.9), (0.25, 0.02, 0.01)), 82),
    "tet": (_shape(V.MESH, (), vertices=np.array([(0.20, 0, 0), (0.29, 0.01, 0), (0.22, 0.08, 0.01), (0.24, 0.03, 0.09)]),
                   triangles=np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)])), 82),
    "one_tri": (_shape(V.MESH, (), (0.1, 0.2, 0.3), (0.2, 0.0, 0.0), vertices=np.array([(0, 0, 0), (0.05, 0, 0), (0, 0.03, 0.01)]),
                       triangles=np.array([(0, 1, 2)])), 13),
    "rod": (_shape(V.BOX, (0.3, 0.02, 0.02), (0.05, -0.1, 0.2), (0.3, 0.0, 0.0)), 118),
    "big": (_shape(V.BOX, (0.2, 0.2, 0.2), (0.3, -0.2, 0.5), (0.3, 0.0, 0.0)), 1172),
}
SINGLE = ["box", "cyl", "sph", "cone", "tet", "one_tri", "rod"]     # every single-shape row but `big`
RANGES = {"box": ((12, -2, -4), (16, 3, 2)), "cyl": ((10, -4, -1), (17, 3, 4))}
# three collinear points: the reference skips the triangle (voxelize.hpp:57-60), so the shape makes no sphere
DEGENERATE = _shape(V.MESH, (), vertices=np.array([(0.2, 0.0, 0.0), (0.25, 0.0, 0.0), (0.3, 0.0, 0.0)]), triangles=np.array([(0, 1, 2)]))


def shape(key):
    return CASES[key][0]


def shifted(s, dx):
    """the shape moved by dx along the link's x axis"""
    out = dict(s)
    out["pose"] = np.array(s["pose"], float)
    out["pose"][0, 3] += dx
    return out


def rows_of(cells, radius=RADIUS):
    res = radius / math.sqrt(2.0)
    c = np.asarray(cells, int).reshape(-1, 3)
    out = np.empty((len(c), 4))
    for a in range(3):
        out[:, a] = 0.0 + c[:, a] * res
    out[:, 3] = radius
    return out


@functools.lru_cache(maxsize=None)
def _judged(key):
    cells, und = V.voxelize_shape(shape(key), (0.0, 0.0, 0.0), RES, None, eps=1e-9)
    _, und6 = V.voxelize_shape(shape(key), (0.0, 0.0, 0.0), RES, None, eps=1e-6)
    rows = rows_of(cells)
    for a in (cells, rows):
        a.setflags(write=False)
    return cells, rows, len(und) + len(und6)


def judged(key):
    """(the judge's cells in ExtractVoxels order, their sphere rows, the number of undecided cells at 1e-9 plus at 1e-6).
    The caller asserts the last is 0 before it compares anything: a condition on the inputs."""
    return _judged(key)


def judged_rows(keys):
    """rows of the shapes laid back to back, and `first`"""
    first, rows = [0], []
    for k in keys:
        cells, r, und = judged(k)
        assert und == 0, k
        rows.append(r)
        first.append(first[-1] + len(r))
    return np.vstack(rows), np.array(first, np.int32)


def judged_shape_rows(s):
    """the same for a shape that is not a row of the table (a shifted one)"""
    cells, und = V.voxelize_shape(s, (0.0, 0.0, 0.0), RES, None, eps=1e-6)
    assert len(und) == 0
    return rows_of(cells)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
