"""Fields on which the BFS brick sweep has to do everything it can do: the cases of tests/test_bfs_cases.py (CPU) and
tests/test_gpu_bfs_topologies.py (GPU), and a certificate for each that it exercises what it is named for.

The sweep (csrc/bfs_kernels.h) relaxes one 8x8x8 brick at a time against a halo of six face copies, twelve edge copies
and eight corner slots, and re-queues the neighbour bricks that can still improve.  On the open scenes of the other BFS
tests the front moves outward once: no brick is entered twice, no cell is lowered after it was labelled, no brick hangs on
its neighbour by an edge or a corner alone, and a run ends in a few dozen passes.  Here:

  corner chains, edge chains   consecutive bricks are joined through ONE corner slot / one edge copy only
  pierced plates               the whole flood passes a single hole in a wall on a brick face, edge or corner
  two routes                   a route that is longer in hops but crosses fewer bricks labels a tail first; it is lowered later
  serpentines                  one corridor that crosses a brick face once per row: as many passes as crossings, more than
                               the 2048 passes of the host driver's history on the long one
  serpentine beside a hall     a run of over a hundred one-brick passes and a run of a few wide ones on one space
  sparse random                tangles of diagonal contacts, pockets, a goal on a wall cell

Every field is a boolean array free[x, y, z]; its distance field is d2 = dmax^2 where free and 0 elsewhere, and the BFS
radius is half a cell, so that the walls of the BFS are exactly the cells that are not free, and the border
(noncubic_cases.probe_case does the same for its synthetic field).  The robot is noncubic_cases.probe_robot, which fits
any grid.  The plain references are those of noncubic_cases (PlainBfs, deque_flood, level_flood).

The certificates are plain Python: brick_steps / brick_crossings walk a corridor, pass_model is the sweep with everything
taken out but its schedule -- every queued brick relaxes its own cells to a fixed point against a snapshot of the grid
taken when the pass began, and a brick that changed queues its 26 neighbours.
"""
from __future__ import annotations

import dataclasses
import functools
import itertools
from collections import Counter, deque

import numpy as np

import noncubic_cases as nc
from smpl_amd import scenes

RES, CAP, ORIGIN = 0.05, 0.2, (-0.3, 0.1, 0.0)
BRICK = 8
SMALL_DIMS = (27, 19, 35)           # = 3 (mod 8) on every axis: 4 x 3 x 5 bricks, the last of every axis partial
TWO_ROUTES_DIMS = (19, 88, 5)
SHORT_SERPENTINE_DIMS = (16, 8, 32)
LONG_SERPENTINE_DIMS = (16, 8, 1200)
HALL_DIMS = (61, 43, 67)
SPARSE_DIMS = (37, 29, 43)
SPARSE_SEED = 5
SPARSE_FRACTIONS = (0.5, 0.2, 0.14)
CHAIN_CELLS = 19
HISTORY = 2048                      # kBfsHistory of csrc/bfs_host.h: the passes whose queue sizes the driver keeps
OUTSIDE = None                      # a goal outside the grid
OUTSIDE_XYZ = (50.0, 50.0, 50.0)


@dataclasses.dataclass
class Case:
    name: str
    free: np.ndarray                # bool [x, y, z]
    goals: list                     # cells (or OUTSIDE), run in this order on ONE space
    path: list = None               # the corridor, in order, where the field is one
    note: dict = dataclasses.field(default_factory=dict)

    @property
    def dims(self):
        return self.free.shape

    @functools.cached_property
    def cfg(self):
        return field_config(self.name, self.free)


def field_config(name, free):
    """the probe robot on the field of a free-cell array: d2 = dmax^2 where free, 0 elsewhere; BFS radius half a cell"""
    dims = tuple(int(n) for n in free.shape)
    base = nc.probe_case(dims, ORIGIN, RES, CAP)
    dmax = base.grid.dmax_int
    d2 = np.where(free, dmax * dmax, 0).astype(np.int32)
    return dataclasses.replace(base, name=name, grid=scenes.Grid(ORIGIN, dims, RES, CAP, d2))


def goal_xyz(cfg, goal):
    return np.asarray(OUTSIDE_XYZ) if goal is OUTSIDE else nc.cell_centre(cfg.grid, goal)


def plain_bfs(cfg):
    return nc.PlainBfs(cfg.grid, cfg.params.bfs_radius)


def n_bricks(dims):
    return int(np.prod([(n + BRICK - 1) // BRICK for n in dims]))


def brick_of(cell):
    return tuple(int(c) // BRICK for c in cell)


def labelled(grid):
    return (grid >= 0) & (grid < nc.WALL)


def cell_grid(free, goal, flood=nc.level_flood):
    """the plain flood of one goal on a fresh copy of the field (no earlier goal has opened a wall)"""
    return plain_bfs(field_config("tmp", free)).run_cell(goal, flood)


# ----------------------------------------------------------------------------------------------------------------------
# certificates
# ----------------------------------------------------------------------------------------------------------------------

def brick_steps(path):
    """for every step of a corridor that leaves a brick: (step index, the brick index's change per axis)"""
    out = []
    for k in range(len(path) - 1):
        a, b = brick_of(path[k]), brick_of(path[k + 1])
        if a != b:
            out.append((k, tuple(b[i] - a[i] for i in range(3))))
    return out


def brick_crossings(path):
    """brick-face crossings along a single corridor: a step into another brick counts one per axis it changes"""
    return sum(sum(abs(d) for d in step) for _, step in brick_steps(path))


def brick_layer_changes(path, axis=2):
    """the steps of a corridor on which the brick index along `axis` changes"""
    return sum(1 for _, step in brick_steps(path) if step[axis] != 0)


def _box_min(a):
    """3x3x3 minimum of the interior of a, as three 3-wide minima"""
    a = np.minimum(np.minimum(a[:-2], a[1:-1]), a[2:])
    a = np.minimum(np.minimum(a[:, :-2], a[:, 1:-1]), a[:, 2:])
    return np.minimum(np.minimum(a[:, :, :-2], a[:, :, 1:-1]), a[:, :, 2:])


def pass_model(free, goal):
    """The brick sweep's schedule without its machinery.  Returns (padded grid [z][y][x] as PlainBfs gives it, passes,
    cells that were lowered after they had a label, visits per brick, per pass (bricks queued, bricks that improved))."""
    dims = free.shape
    nb = [(n + BRICK - 1) // BRICK for n in dims]
    inf = 1 << 40
    shape = tuple(b * BRICK + 2 for b in nb)            # whole bricks and a one-cell rim: [x + 1, y + 1, z + 1]
    wall = np.ones(shape, bool)
    wall[1:dims[0] + 1, 1:dims[1] + 1, 1:dims[2] + 1] = ~free
    dist = np.full(shape, inf, np.int64)
    gx, gy, gz = (int(c) + 1 for c in goal)
    wall[gx, gy, gz] = False                            # the goal cell overwrites a wall
    dist[gx, gy, gz] = 0
    lowered = np.zeros(shape, bool)
    visits = Counter()
    queue = {brick_of(goal)}
    passes = 0
    sizes = []
    while queue:
        snap = dist.copy()
        nxt = set()
        improved = 0
        for b in sorted(queue):
            visits[b] += 1
            lo = [BRICK * v for v in b]
            tile_of = tuple(slice(l, l + BRICK + 2) for l in lo)
            own = tuple(slice(l + 1, l + BRICK + 1) for l in lo)
            tile = snap[tile_of].copy()
            w = wall[own]
            inner = (slice(1, -1),) * 3
            while True:
                new = np.where(w, tile[inner], np.minimum(tile[inner], _box_min(tile) + 1))
                if np.array_equal(new, tile[inner]):
                    break
                tile[inner] = new
            better = new < snap[own]
            if better.any():
                improved += 1
                lowered[own] |= better & (snap[own] < inf)
                dist[own] = new
                for d in itertools.product((-1, 0, 1), repeat=3):
                    q = tuple(b[a] + d[a] for a in range(3))
                    if d != (0, 0, 0) and all(0 <= q[a] < nb[a] for a in range(3)):
                        nxt.add(q)
        sizes.append((len(queue), improved))
        queue = nxt
        passes += 1
    inner = dist[1:dims[0] + 1, 1:dims[1] + 1, 1:dims[2] + 1]
    w = wall[1:dims[0] + 1, 1:dims[1] + 1, 1:dims[2] + 1]
    cells = np.where(w, nc.WALL, np.where(inner >= inf, nc.UNREACHED, inner)).astype(np.int32)
    out = np.full((dims[2] + 2, dims[1] + 2, dims[0] + 2), nc.WALL, np.int32)
    out[1:-1, 1:-1, 1:-1] = cells.transpose(2, 1, 0)
    return out, passes, int(lowered.sum()), visits, sizes


def components(free):
    """26-connected components of the free cells: (label per cell, -1 where not free; size per label)"""
    pad = np.full(tuple(n + 2 for n in free.shape), -2, np.int64)
    pad[1:-1, 1:-1, 1:-1] = np.where(free, -1, -2)
    flat = pad.reshape(-1).tolist()
    offs = nc.neighbour_offsets(pad.shape)
    sizes = []
    for start in np.flatnonzero(pad.reshape(-1) == -1).tolist():
        if flat[start] != -1:
            continue
        lab = len(sizes)
        flat[start] = lab
        todo, n = deque([start]), 1
        while todo:
            cur = todo.popleft()
            for o in offs:
                if flat[cur + o] == -1:
                    flat[cur + o] = lab
                    todo.append(cur + o)
                    n += 1
        sizes.append(n)
    lab = np.asarray(flat, np.int64).reshape(pad.shape)[1:-1, 1:-1, 1:-1]
    return np.where(lab < 0, -1, lab), np.asarray(sizes)


# ----------------------------------------------------------------------------------------------------------------------
# chains
# ----------------------------------------------------------------------------------------------------------------------

def _crossing_steps(start, d, n, length):
    """steps k (k -> k + 1) at which start + k d enters another brick; None if the chain leaves [0, n)"""
    cells = [start + k * d for k in range(length)]
    if min(cells) < 0 or max(cells) >= n:
        return None
    return frozenset(k for k in range(length - 1) if cells[k] // BRICK != cells[k + 1] // BRICK)


def aligned_chain(dims, d, fixed=0, length=CHAIN_CELLS):
    """A straight chain of `length` cells along the diagonal d (components 0, +1, -1; a 0 axis stays at `fixed`) whose
    moving axes all cross their brick boundaries IN THE SAME STEPS, so that consecutive bricks of the chain touch only
    through a corner (three moving axes) or an edge (two).  Of the possible starts the one nearest a grid corner.

    With extents = 3 (mod 8) an axis walked upward from cell 0 crosses after 8 and 16 cells, one walked downward from the
    last cell, n - 1 = 2 (mod 8), after 3 and 11: a chain that is to start exactly at a grid corner on every moving axis
    exists only where all of them run the same way.  Elsewhere the start on some axis is a few cells in from the face."""
    best = {}
    moving = [a for a in range(3) if d[a] != 0]
    for a in moving:
        for s in range(dims[a]):
            steps = _crossing_steps(s, d[a], dims[a], length)
            if steps:
                off = min(s, dims[a] - 1 - s)
                if (a, steps) not in best or off < best[(a, steps)][0]:
                    best[(a, steps)] = (off, s)
    keys = set.intersection(*[{st for (a, st) in best if a == m} for m in moving])
    assert keys, (dims, d)
    steps = min(keys, key=lambda st: (sum(best[(m, st)][0] for m in moving), sorted(st)))
    start = [best[(a, steps)][1] if d[a] else fixed for a in range(3)]
    return [tuple(start[a] + k * d[a] for a in range(3)) for k in range(length)]


def chain_case(name, dims, d, fixed=0):
    path = aligned_chain(dims, d, fixed)
    free = np.zeros(dims, bool)
    for c in path:
        free[c] = True
    return Case(name, free, [path[0], path[-1]], path, {"d": tuple(d), "fixed": fixed})


BODY_DIAGONALS = [(1, 1, 1), (1, 1, -1), (1, -1, 1), (1, -1, -1)]
PLANE_DIAGONALS = [(1, 1, 0), (1, -1, 0), (1, 0, 1), (1, 0, -1), (0, 1, 1), (0, 1, -1)]
EDGE_THIRD = (3, 7, 8)              # inside a brick, and the two boundary layers of a brick face


def corner_chains():
    return [chain_case("corner_chain_%+d%+d%+d" % d, SMALL_DIMS, d) for d in BODY_DIAGONALS]


def edge_chains():
    return [chain_case("edge_chain_%+d%+d%+d_at%d" % (d + (t,)), SMALL_DIMS, d, t) for d in PLANE_DIAGONALS for t in EDGE_THIRD]


def corner_direction(step):
    """the corner-slot index (x | y << 1 | z << 2, 1 = the high side) through which a value leaves a brick on `step`"""
    return (step[0] > 0) | ((step[1] > 0) << 1) | ((step[2] > 0) << 2)


# ----------------------------------------------------------------------------------------------------------------------
# pierced plates
# ----------------------------------------------------------------------------------------------------------------------

def plate_holes(dims, axis):
    """hole positions in the plane's own two coordinates (the axes other than `axis`, in order)"""
    nu, nv = [dims[a] for a in range(3) if a != axis]
    return [(0, 0), (7, 7), (7, 8), (8, 8), (3, 4), (nu - 1, 0), (0, nv - 1), (nu - 1, nv - 1)]


def plate_cases():
    out = []
    for axis in range(3):
        others = [a for a in range(3) if a != axis]
        for hole in plate_holes(SMALL_DIMS, axis):
            free = np.ones(SMALL_DIMS, bool)
            idx = [slice(None)] * 3
            idx[axis] = BRICK
            free[tuple(idx)] = False
            h = [0, 0, 0]
            h[axis], h[others[0]], h[others[1]] = BRICK, hole[0], hole[1]
            free[tuple(h)] = True
            lo = [n // 2 for n in SMALL_DIMS]
            hi = list(lo)
            lo[axis], hi[axis] = 3, SMALL_DIMS[axis] - 4
            out.append(Case("plate_%s8_hole_%d_%d" % ("xyz"[axis], hole[0], hole[1]), free, [tuple(lo), tuple(hi)],
                            note={"axis": axis, "hole": tuple(h)}))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# two routes
# ----------------------------------------------------------------------------------------------------------------------

TWO_ROUTES_JUNCTION_Y = 48
TWO_ROUTES_TAIL = 40


def two_routes_case():
    """Route S zig-zags across the x = 7|8 brick face: every hop enters the other brick, so it advances about one hop per
    pass.  Route F goes out to x = 2, along y and back in at the junction: more hops, but inside one column of bricks, a
    whole brick per pass.  The tail beyond the junction is labelled by F first and lowered when S arrives."""
    free = np.zeros(TWO_ROUTES_DIMS, bool)
    J = TWO_ROUTES_JUNCTION_Y
    slow = [(7 if y % 2 == 0 else 8, y, 0) for y in range(J + 1)]
    fast = [(x, 0, 0) for x in range(6, 1, -1)] + [(2, y, 0) for y in range(1, J)] + [(x, J, 0) for x in range(2, 7)]
    y_turn = J + 1 + TWO_ROUTES_TAIL - (TWO_ROUTES_DIMS[0] - 8)
    tail = [(7, y, 0) for y in range(J + 1, y_turn)] + [(x, y_turn, 0) for x in range(8, TWO_ROUTES_DIMS[0])]
    assert len(tail) == TWO_ROUTES_TAIL
    for c in slow + fast + tail:
        free[c] = True
    return Case("two_routes", free, [slow[0], tail[-1]], note={"slow": slow, "fast": fast, "tail": tail})


# ----------------------------------------------------------------------------------------------------------------------
# serpentines
# ----------------------------------------------------------------------------------------------------------------------

def serpentine_path(nx, ny, nz):
    """One corridor through a box of nx x ny x nz cells: rows along x at even (y, z), joined alternately at the ends by one
    cell at the odd y between them, the layers joined by one cell at the odd z between them.  One cell wide under
    26-connectivity: rows and layers are two cells apart."""
    path = []
    forward, up = True, True
    for z in range(0, nz, 2):
        ys = list(range(0, ny, 2))
        ys = ys if up else ys[::-1]
        for j, y in enumerate(ys):
            xs = range(nx) if forward else range(nx - 1, -1, -1)
            path += [(x, y, z) for x in xs]
            forward = not forward
            if j + 1 < len(ys):
                path.append((path[-1][0], (y + ys[j + 1]) // 2, z))
        up = not up
        if z + 2 < nz:
            path.append((path[-1][0], path[-1][1], z + 1))
    return path


def serpentine_case(name, dims, goals_at):
    path = serpentine_path(*dims)
    free = np.zeros(dims, bool)
    for c in path:
        free[c] = True
    return Case(name, free, [path[int(f * (len(path) - 1))] for f in goals_at], path)


def short_serpentine_case():
    return serpentine_case("short_serpentine", SHORT_SERPENTINE_DIMS, (0.0, 0.5, 1.0))


@functools.lru_cache(maxsize=None)
def long_serpentine_case():
    return serpentine_case("long_serpentine", LONG_SERPENTINE_DIMS, (0.0, 1.0))


HALL_X0 = 20
HALL_SERPENTINE = (16, 8, 64)


@functools.lru_cache(maxsize=None)
def hall_case():
    """the serpentine in x 0..15, y 0..7, z 0..63 and a free hall at x >= 20, sealed from each other; the goals of the
    sequence test: the host driver's plan goes from more than a hundred one-brick passes to a few wide ones and back"""
    path = serpentine_path(*HALL_SERPENTINE)
    free = np.zeros(HALL_DIMS, bool)
    for c in path:
        free[c] = True
    free[HALL_X0:, :, :] = True
    nx, ny, nz = HALL_DIMS
    centre = ((HALL_X0 + nx) // 2, ny // 2, nz // 2)
    corner = (nx - 1, ny - 1, nz - 1)
    pocket = (17, 30, 10)                               # a free cell shut in by the wall between the two regions
    wall = (HALL_X0 - 1, 20, 20)                        # a wall cell on the hall's face: once a goal, part of the hall
    free[pocket] = True
    goals = [path[-1], centre, path[len(path) // 2], corner, OUTSIDE, (HALL_X0, 0, 0), path[0], wall, pocket,
             path[len(path) // 3], centre]
    return Case("serpentine_beside_hall", free, goals, path, {"centre": centre, "corner": corner, "pocket": pocket, "wall": wall})


MULTI_WIDTH_FLOOR, WIDTH_MAX, WIDTH_PAST_PLAN = 64, 16384, 2048      # run_bfs_multi's grid_of (csrc/bfs_host.h)


def multi_launch_width(plan, p, nbricks):
    """blocks per goal of pass p of a shared run whose plan -- the per-pass maxima of the spaces' last queue sizes -- is
    `plan`: run_bfs_multi's rule, restated"""
    planned = max([k + 1 for k, v in enumerate(plan) if v > 0], default=0)
    if p >= planned:
        return min(nbricks, WIDTH_PAST_PLAN)
    m = max(plan[max(0, p - 1):min(planned - 1, p + 1) + 1])
    return min(nbricks, WIDTH_MAX, max(MULTI_WIDTH_FLOOR, 2 * m))


def stride_earlier(case):
    """the last goal of every space before the shared call of the stride test: all in the serpentine"""
    return [case.path[-1], case.path[0], case.path[len(case.path) // 2]]


def stride_goals(case):
    """the goals of that call: two in the hall, whose fronts are wider than a row of the launch, and one in the serpentine"""
    return [case.note["centre"], case.note["corner"], case.path[-1]]


# ----------------------------------------------------------------------------------------------------------------------
# sparse random
# ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def sparse_case(fraction):
    """Free cells drawn with the given probability.  The cell at the high corner is made a pocket of its own (free, its
    seven neighbours walls), so that every fraction has a component of at most 3 cells.  Goals: a cell of the largest
    component, the pocket, a wall cell next to the largest component, the first again."""
    rng = np.random.default_rng(SPARSE_SEED)
    free = rng.random(SPARSE_DIMS) < fraction
    nx, ny, nz = SPARSE_DIMS
    free[nx - 2:, ny - 2:, nz - 2:] = False
    pocket = (nx - 1, ny - 1, nz - 1)
    free[pocket] = True
    lab, sizes = components(free)
    big = int(np.argmax(sizes))
    cells = np.argwhere(lab == big)
    first = tuple(int(v) for v in cells[cells.shape[0] // 2])
    wall = None
    for c in cells[::-1]:                               # a wall cell with a neighbour in the largest component
        for d in itertools.product((-1, 0, 1), repeat=3):
            q = tuple(int(c[a]) + d[a] for a in range(3))
            if all(0 <= q[a] < SPARSE_DIMS[a] for a in range(3)) and not free[q]:
                wall = q
                break
        if wall:
            break
    return Case("sparse_random_%g" % fraction, free, [first, pocket, wall, first],
                note={"pocket": pocket, "wall": wall, "largest": int(sizes[big]), "free": int(free.sum())})


def sparse_cases():
    return [sparse_case(f) for f in SPARSE_FRACTIONS]


# ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def small_cases():
    """every field small enough for the oracle, the pass model and a look at every cell"""
    return tuple(corner_chains() + edge_chains() + plate_cases() + [two_routes_case(), short_serpentine_case()] + sparse_cases())


def small_case(name):
    return next(c for c in small_cases() if c.name == name)


SMALL_NAMES = [c.name for c in small_cases()]
