"""Non-cubic grids: the cases and the plain numpy references of tests/test_noncubic_references.py (CPU) and
tests/test_gpu_noncubic_grids.py (GPU).

Every scene of scenes.py is a cube, and on a cube an engine that exchanged two per-axis extents (nbx/nby/nbz of the 8x8x8
BFS bricks, bricks[1]/bricks[2] of the 4x4x4 distance bricks, nx/ny of the padded BFS export) computes the same thing.
The grids here have three different extents, three different counts of 4-cell bricks and three different counts of
8-cell bricks, no extent is a multiple of 8 and at least one is not a multiple of 4; the thin grids have an axis shorter
than a brick, one of them a single layer.

The references below are written for reading, not for speed, and share no code with the oracle or with
scenes.build_grid; cells come from scenes.world_to_grid (distance_map.hpp:520-527).  Everything is integer or fp64 work
in a fixed order: callers compare with np.array_equal.
"""
from __future__ import annotations

import dataclasses
import functools
import math
from collections import deque

import numpy as np

from smpl_amd import scenes

WALL = 0x7FFFFFFF
UNREACHED = -1

RES, CAP = 0.04, 0.4
# dims, origin: the small scene's boxes cropped to three boxes of cells around the arm
PLANNING_GRIDS = [((61, 46, 35), (-0.78, -1.08, 0.10)),
                  ((45, 58, 27), (-0.5, -1.2, 0.3)),
                  ((70, 37, 50), (-0.9, -1.0, 0.0))]
# lookup, BFS and field only (no arm fits): shorter than a 4-cell brick and/or an 8-cell brick on some axis; one layer
THIN_GRIDS = [(9, 5, 3), (3, 17, 11), (33, 7, 1)]
THIN_ORIGIN, THIN_RES, THIN_CAP = (-0.3, 0.1, 0.0), 0.05, 0.2
THIN_BFS_RADIUS = 0.02          # below one cell: only occupied cells are walls, so that a flood has somewhere to go


def brick_counts(dims):
    """(4-cell bricks per axis, 8-cell bricks per axis)"""
    return tuple((n + 3) // 4 for n in dims), tuple((n + 7) // 8 for n in dims)


def brute_force(occ, dmax):
    """Squared distance of every interior cell to the nearest occupied or border cell, capped (O(cells x obstacles))."""
    nx, ny, nz = occ.shape
    pad = np.ones((nx + 2, ny + 2, nz + 2), bool)
    pad[1:-1, 1:-1, 1:-1] = occ
    # the narrowest integers that hold 3 n^2, the largest squared distance there is (n: the longest extent): the work
    # is cells x obstacles element operations, and numpy does them four times as fast on 2 bytes as on 8
    bound = 3 * max(occ.shape) ** 2
    dt = np.int16 if bound < 2 ** 15 else np.int32 if bound < 2 ** 31 else np.int64
    obs = (np.argwhere(pad) - 1).astype(dt)              # interior coordinates; the border layer sits at -1 and n
    out = np.zeros(occ.shape, np.int64)
    cells = np.argwhere(np.ones(occ.shape, bool)).astype(dt)
    for k in range(0, cells.shape[0], 256):              # (256 cells x obstacles at a time stays in cache)
        c = cells[k:k + 256]
        d = sum((c[:, None, a] - obs[None, :, a]) ** 2 for a in range(3)).min(axis=1)
        assert d.dtype == dt
        out[c[:, 0], c[:, 1], c[:, 2]] = d
    return np.minimum(out, dmax * dmax).astype(np.int32)


def box_occupancy(origin, res, dims, boxes):
    """Cells between the cells of a box's two corners, clipped to the grid (what addBox voxelises to at cell centres)."""
    occ = np.zeros(dims, bool)
    for c, s in boxes:
        lo = scenes.world_to_grid(origin, res, np.asarray(c) - 0.5 * np.asarray(s))
        hi = scenes.world_to_grid(origin, res, np.asarray(c) + 0.5 * np.asarray(s))
        lo = np.maximum(lo, 0)
        hi = np.minimum(hi, np.asarray(dims) - 1)
        if np.all(hi >= lo):
            occ[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    return occ


@functools.lru_cache(maxsize=None)
def planning_case(i: int):
    """config_small's robot, primitives, parameters and boxes on planning grid i"""
    cfg = scenes.config_small()
    dims, origin = PLANNING_GRIDS[i]
    return dataclasses.replace(cfg, name=f"noncubic{i}", grid=scenes.build_grid(origin, dims, RES, CAP, cfg.boxes))


def thin_boxes(dims):
    """two boxes of a cell or two, placed by the grid's own extents"""
    o, n = np.asarray(THIN_ORIGIN), np.asarray(dims)
    out = []
    for frac, cells in ((0.3, 1.2), (0.75, 0.4)):
        c = o + THIN_RES * np.floor(frac * n)
        out.append((tuple(float(v) for v in c), (cells * THIN_RES,) * 3))
    return out


@functools.lru_cache(maxsize=None)
def thin_case(i: int):
    """A thin grid whose field is the brute-force transform of two small boxes; the arm's model only fills the slot a
    space needs (no state of it fits): lookups, the BFS and the field are what these cases are for."""
    cfg = scenes.config_small()
    dims = THIN_GRIDS[i]
    boxes = thin_boxes(dims)
    occ = box_occupancy(THIN_ORIGIN, THIN_RES, dims, boxes)
    dmax = int(math.ceil(THIN_CAP * (1.0 / THIN_RES)))
    grid = scenes.Grid(THIN_ORIGIN, dims, THIN_RES, THIN_CAP, brute_force(occ, dmax))
    return dataclasses.replace(cfg, name=f"thin{i}", grid=grid, boxes=boxes,
                               params=dataclasses.replace(cfg.params, bfs_radius=THIN_BFS_RADIUS))


def cell_centre(grid, cells):
    """gridToWorld (distance_map.hpp:506-518): origin + res * cell"""
    return np.asarray(grid.origin) + np.asarray(cells, dtype=np.float64) * grid.res


def cells_of(grid, pts):
    c = scenes.world_to_grid(grid.origin, grid.res, np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    inside = np.all((c >= 0) & (c < np.asarray(grid.dims)), axis=1)
    return c, inside


# ----------------------------------------------------------------------------------------------------------------------
# lookup
# ----------------------------------------------------------------------------------------------------------------------

def plain_lookup(grid, pts):
    """getSquaredDist: d = res * sqrt(d2[cell]) and d * d (the product of the rounded metric distance with itself, which
    is what a lookup returns; not res^2 * d2, which rounds differently); 0 outside the grid."""
    c, inside = cells_of(grid, pts)
    out = np.zeros(c.shape[0], np.float64)
    ci = c[inside]
    d = grid.res * np.sqrt(grid.d2[ci[:, 0], ci[:, 1], ci[:, 2]].astype(np.float64))
    out[inside] = d * d
    return out


def lookup_points(grid, seed, bulk=12000, per_face=1500):
    """bulk + 6 * per_face points: uniform over the grid grown by three cells, and within 1.5 cells of each face"""
    rng = np.random.default_rng(seed)
    o, n, r = np.asarray(grid.origin), np.asarray(grid.dims), grid.res
    lo, hi = o - 3.5 * r, o + (n + 2.5) * r          # cell c covers [o + (c - 0.5) r, o + (c + 0.5) r)
    P = [lo + rng.uniform(size=(bulk, 3)) * (hi - lo)]
    for a in range(3):
        for face in (o[a] - 0.5 * r, o[a] + (n[a] - 0.5) * r):
            p = lo + rng.uniform(size=(per_face, 3)) * (hi - lo)
            p[:, a] = face + rng.uniform(-1.5, 1.5, size=per_face) * r
            P.append(p)
    return np.vstack(P)


def padded_cells(dims):
    """every cell of the grid and the layer outside each face: [(nx+2)(ny+2)(nz+2), 3], x-major"""
    ax = [np.arange(-1, n + 1) for n in dims]
    return np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)


def hash_bits(cells):
    """An occupancy bit per cell that no exchange of two axes leaves alone (tests/test_noncubic_references.py)."""
    c = np.asarray(cells, dtype=np.int64)
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    h = x * 73856093 + y * 19349669 + z * 83492791 + x * y * 7 + y * z * 13 + (x ^ (z << 1)) * 5
    return ((h >> 2) ^ (h >> 5) ^ (h >> 9)) & 1


def synthetic_field(dims, dmax):
    """d2 in {0, dmax^2}: 0 where hash_bits is 0.  Not a distance transform; a lookup does not care."""
    cells = np.stack(np.meshgrid(*[np.arange(n) for n in dims], indexing="ij"), -1)
    return (hash_bits(cells) * (dmax * dmax)).astype(np.int32)


PROBE_RADIUS = 0.01


def probe_robot() -> str:
    """Three prismatic joints along world x, y, z and one sphere: joint values ARE the sphere's world position.  A
    prismatic joint moves along its local z, so each origin turns local z onto the next world axis:
    Ry(90) z = x;  Ry(90) Rx(-90) z = y;  Ry(90) Rx(-90) Ry(-90) z = z."""
    h = repr(0.5 * math.pi)
    return "\n".join([
        "robot probe3", "link base_link", "link sx", "link sy", "link sz", "link tool_link",
        f"joint jx prismatic base_link sx  0 0 0  0 {h} 0  0 0 1  -100.0 100.0",
        f"joint jy prismatic sx sy  0 0 0  -{h} 0 0  0 0 1  -100.0 100.0",
        f"joint jz prismatic sy sz  0 0 0  0 -{h} 0  0 0 1  -100.0 100.0",
        "joint tool fixed sz tool_link  0 0 0  0 0 0  0 0 1  0.0 0.0",
        f"sphere sz s0 0.0 0.0 0.0 {PROBE_RADIUS} 1",
        "group probe sz", "planning_joints jx jy jz", "planning_link tool_link"]) + "\n"


def probe_case(dims, origin, res, cap):
    """the probe robot on a synthetic field over the given grid"""
    dmax = int(math.ceil(cap * (1.0 / res)))
    grid = scenes.Grid(tuple(origin), tuple(dims), res, cap, synthetic_field(dims, dmax))
    p = scenes.PlanningParams([0.01] * 3, bfs_radius=0.5 * res)
    c = cell_centre(grid, [0, 0, 0])
    return scenes.Config("probe", probe_robot(), scenes.mprim_text(3, range(3), range(3)), grid, p, list(c), list(c),
                         [0.01] * 3, [])


# ----------------------------------------------------------------------------------------------------------------------
# BFS
# ----------------------------------------------------------------------------------------------------------------------

def plain_walls(grid, bfs_radius):
    """bool [z][y][x] over the padded grid: the border layer, and every cell whose metric distance is within the radius
    (bfs_heuristic.cpp:331-353)"""
    nx, ny, nz = grid.dims
    w = np.ones((nz + 2, ny + 2, nx + 2), bool)
    near = grid.res * np.sqrt(grid.d2.astype(np.float64)) <= bfs_radius
    w[1:-1, 1:-1, 1:-1] = near.transpose(2, 1, 0)
    return w


def _offsets(shape):
    dxy, dx = shape[1] * shape[2], shape[2]
    return [a * dxy + b * dx + c for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]


neighbour_offsets = _offsets       # for the other case files


def deque_flood(dist, start):
    """26-connected flood of the UNREACHED cells of the padded array from flat index `start` (its value is 0 already)"""
    d = dist.reshape(-1).tolist()
    offs = _offsets(dist.shape)
    todo = deque([start])
    while todo:
        cur = todo.popleft()
        cost = d[cur] + 1
        for o in offs:
            if d[cur + o] < 0:
                d[cur + o] = cost
                todo.append(cur + o)
    return np.asarray(d, dtype=np.int32).reshape(dist.shape)


def level_flood(dist, start):
    """The same distances level by level with array operations (a breadth-first distance does not depend on the order
    within a level); test_noncubic_references.py holds it to deque_flood on every case.  For sweeps of many goals."""
    flat = dist.copy().reshape(-1)
    offs = np.asarray(_offsets(dist.shape), dtype=np.int64)
    front = np.asarray([start], dtype=np.int64)
    level = 0
    while front.size:
        level += 1
        cand = (front[:, None] + offs[None, :]).reshape(-1)
        cand = np.unique(cand[flat[cand] == UNREACHED])
        flat[cand] = level
        front = cand
    return flat.reshape(dist.shape)


class PlainBfs:
    """BFS_3D + BfsHeuristic of one space: walls once, then one flood per goal.  As in the reference (bfs3d.cpp:162-178) a
    goal on a wall cell overwrites the wall, and the cell stays free for the goals that follow."""

    def __init__(self, grid, bfs_radius):
        self.grid = grid
        self.walls = plain_walls(grid, bfs_radius)

    def run_cell(self, cell, flood=deque_flood):
        dist = np.where(self.walls, WALL, UNREACHED).astype(np.int32)
        c = np.asarray(cell)
        if np.all((c >= 0) & (c < np.asarray(self.grid.dims))):
            z, y, x = int(c[2]) + 1, int(c[1]) + 1, int(c[0]) + 1
            self.walls[z, y, x] = False
            dist[z, y, x] = 0
            dist = flood(dist, (z * dist.shape[1] + y) * dist.shape[2] + x)
        return dist

    def run(self, xyz, flood=deque_flood):
        return self.run_cell(scenes.world_to_grid(self.grid.origin, self.grid.res, np.asarray(xyz, dtype=np.float64)), flood)


def plain_metric_goal(grid, dist, pts):
    """BFS value x res; WALL x res outside the grid (bfs_heuristic.cpp:129-138)"""
    c, inside = cells_of(grid, pts)
    out = np.full(c.shape[0], float(WALL) * grid.res)
    ci = c[inside]
    out[inside] = dist[ci[:, 2] + 1, ci[:, 1] + 1, ci[:, 0] + 1].astype(np.float64) * grid.res
    return out


def plain_metric_start(grid, start_xyz, pts):
    """Manhattan cells to the cell of the start's planning link x res (bfs_heuristic.cpp:103-127)"""
    sc = scenes.world_to_grid(grid.origin, grid.res, np.asarray(start_xyz, dtype=np.float64))
    c = scenes.world_to_grid(grid.origin, grid.res, np.asarray(pts, dtype=np.float64).reshape(-1, 3))
    return grid.res * np.abs(c - sc[None, :]).sum(axis=1).astype(np.float64)


def last_brick_corner_cells(dims, brick=8):
    """For each axis, a brick that is the last (partial) one along that axis and a middle one along the others, and the
    brick that is last along all three: the eight corner cells of each (the high corner clipped to the grid)."""
    n = np.asarray(dims)
    nb = (n + brick - 1) // brick
    bricks = [tuple(nb - 1)]
    for a in range(3):
        b = nb // 2
        b[a] = nb[a] - 1
        bricks.append(tuple(b))
    out = []
    for b in bricks:
        lo = np.asarray(b) * brick
        hi = np.minimum(lo + brick - 1, n - 1)
        for k in range(8):
            c = tuple(int(hi[a] if (k >> a) & 1 else lo[a]) for a in range(3))
            if c not in out:
                out.append(c)
    return out


def metric_points(grid, seed, n=600):
    """points inside, on the faces (cell boundaries at a face) and outside"""
    P = lookup_points(grid, seed, bulk=n, per_face=n // 6)
    o, d, r = np.asarray(grid.origin), np.asarray(grid.dims), grid.res
    faces = []
    for a in range(3):
        for f in (o[a] - 0.5 * r, o[a] + (d[a] - 0.5) * r):
            p = o + 0.5 * d * r
            p[a] = f
            faces.append(p)
    return np.vstack([P, np.asarray(faces), cell_centre(grid, [[0, 0, 0], d - 1, [-1, 0, 0], d])])


# ----------------------------------------------------------------------------------------------------------------------
# states
# ----------------------------------------------------------------------------------------------------------------------

def bench_states():
    return scenes.benchmark_states(scenes.ARM7_LIMITS, 1200, 777)


def corner_edit_cell(dims):
    """a cell near the low-x / high-y / high-z corner: the window of an edit there (the cell grown by dmax cells, clipped)
    has three different extents"""
    return (3, dims[1] - 6, dims[2] - 8)


def edit_window_cells(dims, cell, dmax):
    return int(np.prod([min(c + dmax, n - 1) - max(c - dmax, 0) + 1 for c, n in zip(cell, dims)]))
