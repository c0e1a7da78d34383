"""A plain restatement of the reference's surface voxeliser: the judge of the world-object tests.

Restated lines (binary64, the reference's operation order; numpy is used only for elementwise +,-,*,/ over the candidate
voxels of one triangle, which rounds like the scalar operations):
  - shapes to meshes: smpl/src/geometry/mesh_utils.cpp:39-112 (box), :116-204 (sphere, 7 x 8), :208-264 (cylinder),
    :268-299 (cone); TransformVertices, smpl/src/geometry/voxelize.cpp:608-615 (R v + t);
  - the voxel grid: PivotDiscretizer, smpl/include/smpl/geometry/discretize.h:40-61, with the pivot and resolution of
    VoxelizeMesh(..., res, voxel_origin, ...), voxelize.cpp:1008-1035;
  - VoxelizeTriangle, smpl/include/smpl/geometry/detail/voxelize.hpp:46-180, and Distance, voxelize.cpp:626-649;
  - ExtractVoxels order (x-major, z fastest), voxelize.cpp:207-222.
Three-term sums are Eigen's unrolled reduction a0*b0 + (a1*b1 + a2*b2).

For every (triangle, voxel) the model also gives the smallest normalised distance from equality of the comparisons the
reference reaches for that pair: squared lengths over rc^2, plane and guard values over res, projections onto an edge
over |pq| * res.  A cell is UNDECIDED at eps if any triangle that has it as a candidate comes within eps.
"""
import math

import numpy as np

BOX, SPHERE, CYLINDER, CONE, MESH = 1, 2, 3, 4, 5


# ---- meshes ---------------------------------------------------------------------------------------------------------
def box_mesh(length, width, height):
    x, y, z = 0.5 * length, 0.5 * width, 0.5 * height
    v = [(-x, -y, -z), (x, -y, -z), (-x, y, -z), (x, y, -z), (-x, -y, z), (x, -y, z), (-x, y, z), (x, y, z)]
    t = [0, 2, 1, 1, 2, 3, 5, 1, 7, 1, 3, 7, 5, 7, 4, 4, 7, 6, 4, 6, 0, 0, 6, 2, 6, 7, 2, 7, 3, 2, 5, 0, 1, 4, 5, 0]
    return np.array(v, float), np.array(t, int).reshape(-1, 3)


def sphere_mesh(radius, lon=7, lat=8):
    v = [(0.0, 0.0, radius)]
    theta_inc = math.pi / (lat + 1)
    phi_inc = (2.0 * math.pi) / lon
    for ti in range(lat):
        for pi in range(lon):
            theta, phi = (ti + 1) * theta_inc, pi * phi_inc
            v.append((radius * math.sin(theta) * math.cos(phi), radius * math.sin(theta) * math.sin(phi), radius * math.cos(theta)))
    v.append((0.0, 0.0, -radius))
    nv = len(v)
    t = []
    for i in range(lon):
        t += [0, i + 1, 1 if i == lon - 1 else i + 2]
    for i in range(lat - 1):
        for j in range(lon):
            base = i * lon + j + 1
            b = base + lon
            br, r = b + 1, base + 1
            if (br - 1) // lon != (b - 1) // lon:
                br -= lon
            if (r - 1) // lon != (base - 1) // lon:
                r -= lon
            t += [base, b, br, base, br, r]
    for i in range(lon):
        t += [nv - 1, nv - 1 - lon if i == 0 else nv - 1 - i, nv - 1 - (i + 1)]
    return np.array(v, float), np.array(t, int).reshape(-1, 3)


def cylinder_mesh(radius, length, rim=16):
    v = []
    for zc in (0.5 * length, -0.5 * length):
        for i in range(rim):
            theta = 2.0 * math.pi * float(i) / float(rim)
            v.append((radius * math.cos(theta), radius * math.sin(theta), zc))
    v += [(0.0, 0.0, 0.5 * length), (0.0, 0.0, -0.5 * length)]
    t = []
    for i in range(rim):
        t += [i, (i + 1) % rim, i + rim, (i + 1) % rim, (i + 1) % rim + rim, i + rim]
    for i in range(rim):
        t += [2 * rim, (i + 1) % rim, i]
    for i in range(rim):
        t += [2 * rim + 1, (i + 1) % rim + rim, i + rim]
    return np.array(v, float), np.array(t, int).reshape(-1, 3)


def cone_mesh(radius, height, rim=16):
    v = []
    for i in range(rim):
        theta = 2.0 * math.pi * float(i) / float(rim)
        v.append((radius * math.cos(theta), radius * math.sin(theta), -0.5 * height))
    v += [(0.0, 0.0, 0.5 * height), (0.0, 0.0, -0.5 * height)]
    t = []
    for i in range(rim):
        t += [i, (i + 1) % rim, rim]
    for i in range(rim):
        t += [i, (i + 1) % rim, rim + 1]
    return np.array(v, float), np.array(t, int).reshape(-1, 3)


def transform(pose, v):
    """TransformVertices: R v + t with pose the 3x4 [R | t]."""
    P = np.asarray(pose, float).reshape(3, 4)
    out = np.empty_like(v)
    for r in range(3):
        out[:, r] = (P[r, 0] * v[:, 0] + (P[r, 1] * v[:, 1] + P[r, 2] * v[:, 2])) + P[r, 3]
    return out


def shape_mesh(shape):
    """shape: dict(type, dims, pose[, vertices, triangles]) -> world-frame vertices, triangles."""
    ty, d = shape["type"], shape.get("dims", (0, 0, 0))
    if ty == BOX:
        v, t = box_mesh(d[0], d[1], d[2])
    elif ty == SPHERE:
        v, t = sphere_mesh(d[0], 7, 8)
    elif ty == CYLINDER:
        v, t = cylinder_mesh(d[0], d[1])
    elif ty == CONE:
        v, t = cone_mesh(d[0], d[1])
    elif ty == MESH:
        v = np.asarray(shape["vertices"], float).reshape(-1, 3)
        t = np.asarray(shape["triangles"], int).reshape(-1, 3)
    else:
        raise ValueError("unknown shape type")
    return transform(shape["pose"], v), t


# ---- the voxel grid -------------------------------------------------------------------------------------------------
def discretize(d, pivot, res):
    return int(math.floor((d - pivot) / res + 0.5))


def continuize(i, pivot, res):
    return pivot + i * res


# ---- one triangle ---------------------------------------------------------------------------------------------------
def _dot(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _normalized(v):
    z = _dot(v, v)
    if z > 0.0:
        s = math.sqrt(z)
        return (v[0] / s, v[1] / s, v[2] / s)
    return v


def _edge_normal(edge, n):
    c = _cross(edge, n)
    return _normalized((-c[0], -c[1], -c[2]))


def triangle_constants(p1, p2, p3, res):
    """voxelize.hpp:52-113; None for a triangle the reference skips (:57-60)."""
    p1, p2, p3 = (tuple(float(x) for x in p) for p in (p1, p2, p3))
    c = _cross(_sub(p2, p1), _sub(p3, p1))
    if math.sqrt(_dot(c, c)) == 0.0:
        return None
    rc = math.sqrt(3.0) * 0.5 * res
    u, v, w = _sub(p2, p1), _sub(p3, p2), _sub(p1, p3)
    n = _normalized(_cross(u, v))
    ca = max(_dot((sx * 0.5774, sy * 0.5774, sz * 0.5774), n) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1))
    e1, e2, e3 = _edge_normal(u, n), _edge_normal(v, n), _edge_normal(w, n)
    return dict(p1=p1, p2=p2, p3=p3, rc2=rc * rc, n=n, t=rc * ca, d=-_dot(n, p1), e1=e1, e2=e2, e3=e3,
                d1=-_dot(e1, p1), d2=-_dot(e2, p2), d3=-_dot(e3, p3))


def candidate_range(p1, p2, p3, origin, res):
    lo = [discretize(min(p1[a], p2[a], p3[a]), origin[a], res) for a in range(3)]
    hi = [discretize(max(p1[a], p2[a], p3[a]), origin[a], res) for a in range(3)]
    return lo, hi


def voxelize_triangle(p1, p2, p3, origin, res, clip=None):
    """-> (cells[k,3] candidates, filled[k] bool, margin[k]) of one triangle; clip = grid dims keeps the candidates
    inside the occupancy grid (the engine's deliberate difference)."""
    K = triangle_constants(p1, p2, p3, res)
    if K is None:
        return np.zeros((0, 3), int), np.zeros(0, bool), np.zeros(0)
    lo, hi = candidate_range(K["p1"], K["p2"], K["p3"], origin, res)
    if clip is not None:
        lo = [max(0, lo[a]) for a in range(3)]
        hi = [min(clip[a] - 1, hi[a]) for a in range(3)]
    if any(hi[a] < lo[a] for a in range(3)):
        return np.zeros((0, 3), int), np.zeros(0, bool), np.zeros(0)
    gx, gy, gz = np.meshgrid(*[np.arange(lo[a], hi[a] + 1) for a in range(3)], indexing="ij")
    cells = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1)
    X = [origin[a] + cells[:, a] * res for a in range(3)]        # continuize
    k = cells.shape[0]
    filled = np.zeros(k, bool)
    alive = np.ones(k, bool)                   # pairs whose control flow is still running
    margin = np.full(k, np.inf)
    rc2 = K["rc2"]

    def reach(values, where):
        margin[where] = np.minimum(margin[where], values[where])

    def dotv(c, V):
        return c[0] * V[0] + (c[1] * V[1] + c[2] * V[2])

    def sqn(V):
        return V[0] * V[0] + (V[1] * V[1] + V[2] * V[2])

    # vertex tests (:145-147), short-circuit ||
    for p in (K["p1"], K["p2"], K["p3"]):
        s = sqn([X[a] - p[a] for a in range(3)])
        reach(np.abs(s - rc2) / rc2, alive)
        hit = alive & (s <= rc2)
        filled |= hit
        alive &= ~hit
    # edge tests (:152-154) on (p1,p3), (p2,p3), (p3,p1) as written
    for p, q in ((K["p1"], K["p3"]), (K["p2"], K["p3"]), (K["p3"], K["p1"])):
        pq = _sub(q, p)
        px = [X[a] - p[a] for a in range(3)]
        d = px[0] * pq[0] + (px[1] * pq[1] + px[2] * pq[2])
        len2 = _dot(pq, pq)
        scale = math.sqrt(len2) * res
        reach(np.abs(d) / scale, alive)
        in1 = alive & ~(d < 0.0)
        reach(np.abs(d - len2) / scale, in1)
        in2 = in1 & ~(d > len2)
        dsq = sqn(px) - (d * d) / len2
        reach(np.abs(dsq - rc2) / rc2, in2)
        hit = in2 & ~(dsq > rc2) & (dsq != -1.0)
        filled |= hit
        alive &= ~hit
    # plane and guards (:161-172)
    nx = dotv(K["n"], X)
    a_, b_ = nx + (K["d"] + K["t"]), nx + (K["d"] - K["t"])
    reach(np.minimum(np.abs(a_), np.abs(b_)) / res, alive)
    alive &= np.sign(a_) != np.sign(b_)
    for e, dd in ((K["e1"], K["d1"]), (K["e2"], K["d2"]), (K["e3"], K["d3"])):
        g = dotv(e, X) + dd
        reach(np.abs(g) / res, alive)
        alive &= g > 0.0
    filled |= alive
    return cells, filled, margin


# ---- a mesh, a shape ------------------------------------------------------------------------------------------------
def voxelize_mesh(vertices, triangles, origin, res, clip=None, eps=1e-9):
    """-> (cells[n,3] in ExtractVoxels order, undecided[m,3]); each filled cell once."""
    filled, near = set(), set()
    for t in np.asarray(triangles, int).reshape(-1, 3):
        cells, f, m = voxelize_triangle(vertices[t[0]], vertices[t[1]], vertices[t[2]], origin, res, clip)
        filled.update(map(tuple, cells[f]))
        near.update(map(tuple, cells[m < eps]))
    out = np.array(sorted(filled), int).reshape(-1, 3)       # x-major, z fastest
    und = np.array(sorted(near), int).reshape(-1, 3)
    return out, und


def voxelize_shape(shape, origin, res, clip=None, eps=1e-9):
    v, t = shape_mesh(shape)
    return voxelize_mesh(v, t, origin, res, clip, eps)


def in_grid(cells, dims):
    c = np.asarray(cells, int).reshape(-1, 3)
    ok = np.all((c >= 0) & (c < np.asarray(dims)), axis=1)
    return c[ok]
