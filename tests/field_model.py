"""A plain model of the reference's occupancy edits, for tests/test_field_model.py (CPU) and
tests/test_gpu_field_edits.py (GPU, against smpl_amd/csrc/field.hip).

The reference keeps TWO states per cell: the obstacle flag inside the distance map (a cell is an obstacle when it is its
own nearest obstacle, `c.obs == &c` / `dist_new == 0`) and, beside it, OccupancyGrid::m_counts.  They go out of step by
design: updatePointsInField edits the flag and leaves the counts alone (occupancy_grid.cpp:416-422, "TODO: ref
counting"), a counted add forwards a point to the map only when the count was 0 (:370-374) and a counted remove only when
the count returns to 0 (:398-403).  `counts > 0` is therefore NOT the occupancy.  FieldModel keeps both arrays and restates
the loops; everything is integer work in a fixed order, callers compare with np.array_equal.

The model takes nothing from the engine but the cell of a point, scenes.world_to_grid (distance_map.hpp:520-527), and its
transform is noncubic_cases.brute_force.  Below it: the seeded operation sequences both test files run, and the edits near
the arm of the small scene (whose 64^3 field comes from the host builder scenes.build_grid, not from brute force).
"""
from __future__ import annotations

import numpy as np

from noncubic_cases import box_occupancy, brute_force
from smpl_amd import scenes


class FieldModel:
    """occ: bool [nx, ny, nz], the obstacle flags of the distance map; counts: int64 [nx, ny, nz], OccupancyGrid::m_counts,
    or None while the grid is not reference counted."""

    def __init__(self, origin, dims, res):
        self.origin, self.dims, self.res = tuple(origin), tuple(int(n) for n in dims), float(res)
        self.occ = np.zeros(self.dims, bool)
        self.counts = None

    def cells(self, pts):
        """worldToGrid of every point, [n, 3]"""
        return scenes.world_to_grid(self.origin, self.res, np.asarray(pts, dtype=np.float64).reshape(-1, 3))

    def in_bounds(self, c):
        """isInBounds (occupancy_grid.cpp:367, :395) / isCellValid (distance_map.hpp:312, :340)"""
        return all(0 <= int(c[a]) < self.dims[a] for a in range(3))

    def add_points(self, pts):
        """OccupancyGrid::addPointsToField (occupancy_grid.cpp:357-382) over DistanceMap::addPointsToMap
        (distance_map.hpp:306-328).  Point by point, in order: a cell listed twice in one call is counted twice."""
        for c in self.cells(pts):
            if not self.in_bounds(c):                    # :367 / hpp:312-314
                continue
            c = tuple(int(v) for v in c)
            if self.counts is None:                      # :379-381: every point goes to the map
                self.occ[c] = True                       # hpp:319-323 (a cell that is an obstacle already stays one)
                continue
            if self.counts[c] == 0:                      # :370-372: forwarded only when the count was 0 ...
                self.occ[c] = True                       # ... hpp:319-323
            self.counts[c] += 1                          # :374

    def remove_points(self, pts):
        """OccupancyGrid::removePointsFromField (occupancy_grid.cpp:385-411) over DistanceMap::removePointsFromMap
        (distance_map.hpp:334-361)."""
        for c in self.cells(pts):
            if not self.in_bounds(c):                    # :395 / hpp:340-342
                continue
            c = tuple(int(v) for v in c)
            if self.counts is None:                      # :408-410
                self.occ[c] = False                      # hpp:348-357 (a free cell stays free)
                continue
            if self.counts[c] > 0:                       # :398
                self.counts[c] -= 1                      # :399
                if self.counts[c] == 0:                  # :400-402: forwarded only when the count returns to 0 ...
                    self.occ[c] = False                  # ... hpp:348-357

    def update_points(self, old_pts, new_pts):
        """OccupancyGrid::updatePointsInField (occupancy_grid.cpp:416-422) passes both clouds to
        DistanceMap::updatePointsInMap (distance_map.hpp:367-435) and does not touch the counts."""
        old = {tuple(int(v) for v in c) for c in self.cells(old_pts) if self.in_bounds(c)}      # hpp:371-379
        new = {tuple(int(v) for v in c) for c in self.cells(new_pts) if self.in_bounds(c)}      # hpp:381-389
        for c in sorted(old - new):                      # hpp:393-398, 408-418
            self.occ[c] = False
        for c in sorted(new - old):                      # hpp:400-405, 423-432
            self.occ[c] = True

    def set_ref_counted(self, on):
        """OccupancyGrid::initRefCounts (occupancy_grid.cpp:424-441): 1 where the cell is an obstacle, else 0; cleared
        when counting is off (:426-428)."""
        self.counts = np.where(self.occ, 1, 0).astype(np.int64) if on else None

    def box_range(self, center, size):
        """The engine's rule for a box (field.hip smplx_grid_add_boxes, scenes.py box_cells): the cells from the cell of
        its low corner to the cell of its high corner, clipped to the grid; None when nothing is left."""
        lo = self.cells(np.asarray(center, dtype=np.float64) - 0.5 * np.asarray(size, dtype=np.float64))[0]
        hi = self.cells(np.asarray(center, dtype=np.float64) + 0.5 * np.asarray(size, dtype=np.float64))[0]
        lo = [max(int(lo[a]), 0) for a in range(3)]
        hi = [min(int(hi[a]), self.dims[a] - 1) for a in range(3)]
        if any(hi[a] < lo[a] for a in range(3)):
            return None
        return lo, hi

    def add_boxes(self, boxes):
        """Every cell of a box becomes an obstacle; with counts, each box adds one count to every cell it covers.  (The
        flag is set whatever the count was: the engine's rule)"""
        for center, size in boxes:
            r = self.box_range(center, size)
            if r is None:
                continue
            (x0, y0, z0), (x1, y1, z1) = r
            self.occ[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] = True
            if self.counts is not None:
                self.counts[x0:x1 + 1, y0:y1 + 1, z0:z1 + 1] += 1

    def d2(self, dmax):
        return brute_force(self.occ, dmax)


def dmax_of(res, max_dist):
    """distance_map.hpp:126, as the engine computes it"""
    return int(np.ceil(max_dist * (1.0 / res)))


def edit_window_cells(dims, dmax, lo, hi):
    """field.hip edit_window: the cells an edit recomputes.  lo, hi: the inclusive bounding box of the listed cells that
    lie inside the grid (for boxes: of their clipped cell ranges).  The box grown by dmax along every axis and clipped
    to the grid; the whole grid when that is more than half of it."""
    n = 1
    for a in range(3):
        n *= min(dims[a] - 1, hi[a] + dmax) - max(0, lo[a] - dmax) + 1
    whole = dims[0] * dims[1] * dims[2]
    return whole if 2 * n > whole else n


def bounding_box(model, pts):
    """(lo, hi) over the cells of pts that lie inside the grid; None when none does"""
    c = [c for c in model.cells(pts) if model.in_bounds(c)]
    if not c:
        return None
    c = np.asarray(c)
    return [int(v) for v in c.min(axis=0)], [int(v) for v in c.max(axis=0)]


# ----------------------------------------------------------------------------------------------------------------------
# seeded operation sequences
# ----------------------------------------------------------------------------------------------------------------------

# how often each kind is planned at least (the rest of a sequence is drawn uniformly)
OP_KINDS = {"add": 12, "remove": 10, "update": 9, "ref_on": 4, "ref_off": 2,
            "box_overlap": 3, "box_clipped": 3, "box_outside": 2, "box_thin": 3, "box_on_points": 3}


def apply(target, kind, payload):
    """one operation on a FieldModel or on anything with the same methods (capi.Grid)"""
    if kind == "add":
        target.add_points(payload)
    elif kind == "remove":
        target.remove_points(payload)
    elif kind == "update":
        target.update_points(payload[0], payload[1])
    elif kind in ("ref_on", "ref_off"):
        target.set_ref_counted(kind == "ref_on")
    else:
        assert kind.startswith("box_"), kind
        target.add_boxes(payload)


def random_ops(seed, origin, dims, res, n=72):
    """n + 1 operations [(kind, payload)]: every kind of OP_KINDS at least as often as its number there, shuffled, with
    counting switched on early so that most of the sequence runs counted.

    Points lie anywhere inside their cells (not only at the centres); every add / remove / update carries duplicates and
    points outside the grid; adds also name cells that earlier operations named, removes also cells that were never
    added; the two clouds of an update share points.  While counting is on, an update frees obstacles whose count is
    positive and a later add names such cells: where the reference's flag and count part."""
    rng = np.random.default_rng(seed)
    o, d = np.asarray(origin, dtype=np.float64), np.asarray(dims)
    kinds = [k for k, w in OP_KINDS.items() for _ in range(w)]
    kinds += [str(k) for k in rng.choice(list(OP_KINDS), size=max(0, n - len(kinds)))]
    rng.shuffle(kinds)
    kinds.insert(2, "ref_on")
    pool = np.zeros((0, 3), np.int64)                   # cells some operation has named so far
    track = FieldModel(origin, dims, res)               # the state so far: the sequence aims at the cells where flag and count part

    def world(cells):
        cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
        return o + (cells + rng.uniform(-0.4, 0.4, size=cells.shape)) * res

    def cluster(k):
        """k cells around a random centre: one cell, a few cells wide, or all over the grid (and past its faces)"""
        spread = int(rng.choice([0, 1, 2, int(d.max())]))
        return rng.integers(0, d) + rng.integers(-spread, spread + 1, size=(k, 3))

    def outside():
        far = np.array([[9.0, 9.0, 9.0], [-5.0, 0.0, 0.0]])
        return np.vstack([world([[-1, 0, 0], d, [0, d[1], 0], [d[0] - 1, d[1] - 1, -1]]), far])

    def from_pool(k):
        return pool[rng.integers(0, pool.shape[0], size=k)] if pool.shape[0] else cluster(k)

    def some(mask, k):
        """up to k of the cells of a mask"""
        c = np.argwhere(mask)
        return c[rng.permutation(c.shape[0])[:k]]

    def cell_box(lo, hi):
        """a box whose corners lie 0.3 cells outside the centres of cells lo and hi"""
        lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
        return tuple(o + 0.5 * (lo + hi) * res), tuple((hi - lo + 0.6) * res)

    ops = []
    for kind in kinds:
        if kind == "add":
            c = np.vstack([cluster(int(rng.integers(1, 9))), from_pool(3)])     # new cells, and cells with a history
            if track.counts is not None:                # cells an update freed while their count stayed positive
                c = np.vstack([c, some((track.counts > 0) & ~track.occ, 2)])
            pts = np.vstack([world(c), world(c[:(len(c) + 1) // 2]), world(c[:1]), outside()])
            pool = np.vstack([pool, c])
            ops.append((kind, pts))
        elif kind == "remove":
            c = np.vstack([from_pool(int(rng.integers(1, 9))), cluster(3)])
            ops.append((kind, np.vstack([world(c), world(c[:2]), outside()])))
        elif kind == "update":
            old = np.vstack([from_pool(int(rng.integers(2, 8))), cluster(2)])
            new = np.vstack([old[:len(old) // 2], cluster(int(rng.integers(1, 6))), old[:1]])
            if track.counts is not None:                # free two counted obstacles, occupy a cell whose count is 0
                old = np.vstack([old, some((track.counts > 0) & track.occ, 2)])
                new = np.vstack([new, some((track.counts == 0) & ~track.occ, 1)])
            pool = np.vstack([pool, new])
            ops.append((kind, (np.vstack([world(old), outside()]), np.vstack([world(new), outside()]))))
        elif kind in ("ref_on", "ref_off"):
            ops.append((kind, None))
        elif kind == "box_overlap":
            lo = rng.integers(0, d)
            hi = np.minimum(lo + rng.integers(0, 4, size=3), d - 1)
            lo2 = lo + rng.integers(0, hi - lo + 1)                     # a corner inside the first box
            boxes = [cell_box(lo, hi), cell_box(lo2, lo2 + rng.integers(0, 4, size=3))]
            if rng.integers(0, 2):
                boxes.append(cell_box(lo, hi))                          # the same box twice: two counts
            ops.append((kind, boxes))
        elif kind == "box_clipped":
            lo = rng.integers(0, d)
            hi = lo + rng.integers(0, 3, size=3)
            a, how = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            if how == 0:
                lo[a], hi[a] = -2, 1                                    # through the low face
            elif how == 1:
                lo[a], hi[a] = d[a] - 2, d[a] + 1                       # through the high face
            else:
                lo[a], hi[a] = -1, d[a]                                 # through both
            ops.append((kind, [cell_box(lo, hi)]))
        elif kind == "box_outside":
            lo = rng.integers(0, d)
            hi = lo + rng.integers(0, 3, size=3)
            a = int(rng.integers(0, 3))
            if rng.integers(0, 2):
                lo[a], hi[a] = d[a] + 1, d[a] + 3
            else:
                lo[a], hi[a] = -4, -2
            ops.append((kind, [cell_box(lo, hi), ((50.0, 0.0, -50.0), (0.1, 0.1, 0.1))]))
        elif kind == "box_thin":
            c = rng.integers(0, d)
            size = np.where(rng.integers(0, 2, size=3) == 1, 0.3, 1.4)
            size[int(rng.integers(0, 3))] = 0.3                         # thinner than a cell along one axis at least
            centre = o + (c + rng.uniform(-0.45, 0.45, size=3)) * res   # within one cell, or across a cell boundary
            ops.append((kind, [(tuple(centre), tuple(size * res))]))
        elif kind == "box_on_points":
            c = from_pool(1)[0]
            ops.append((kind, [cell_box(c - 1, c + 1)]))
        else:
            raise AssertionError(kind)
        apply(track, *ops[-1])
    return ops


# ----------------------------------------------------------------------------------------------------------------------
# edits near the arm of the small scene, for the check of the field the collision kernels read
# ----------------------------------------------------------------------------------------------------------------------

ARM_STATES, ARM_STATES_SEED = 512, 2024
ARM_FIRST_NODE = 8              # scenes.arm7_robot: the sphere-tree nodes of forearm_link and of the links after it


def arm_edits(cfg, sphere_positions):
    """(states, [(kind, payload)]) on the small scene: the sphere centres of six seeded states become obstacle points
    (an add), half of them are removed again, and an update moves the rest onto the spheres of six other states.
    sphere_positions(q) -> [nnodes, 3] of one state.  Only the spheres from the forearm on: an obstacle on the shoulder
    would end every state alike."""
    states = scenes.random_states(scenes.ARM7_LIMITS, ARM_STATES, ARM_STATES_SEED)
    poses = scenes.random_states(scenes.ARM7_LIMITS, 12, 41)
    clouds = [np.asarray(sphere_positions(q), dtype=np.float64).reshape(-1, 3)[ARM_FIRST_NODE:] for q in poses]
    first = np.vstack(clouds[:6])
    kept = np.vstack([first[1::2], clouds[0][:4]])
    moved = np.vstack([kept[:len(kept) // 2]] + clouds[6:])
    return states, [("add", first), ("remove", first[::2]), ("update", (kept, moved))]


def arm_edited_grid(cfg, edits):
    """The small scene's grid after the edits, as a finished field.  Brute force over 64^3 cells and ~30 000 obstacle and
    border cells is 10^10 distance evaluations, so the transform here is the host builder's, which
    tests/test_field_model.py holds to brute force: the model's occupancy goes in as one box per
    run of occupied cells along z (a remove may free cells of the scene's own boxes, so those are not passed on as they
    were), and is checked to come out of that box list unchanged."""
    gr = cfg.grid
    m = FieldModel(gr.origin, gr.dims, gr.res)
    m.add_boxes(cfg.boxes)
    for kind, payload in edits:
        apply(m, kind, payload)
    o, boxes = np.asarray(gr.origin), []
    for x, y in np.argwhere(m.occ.any(axis=2)):
        col = np.concatenate([[False], m.occ[x, y], [False]])
        for z0, z1 in zip(np.flatnonzero(col[1:] & ~col[:-1]), np.flatnonzero(col[:-1] & ~col[1:]) - 1):   # z0..z1 occupied
            boxes.append((tuple(o + np.array([x, y, 0.5 * (z0 + z1)]) * gr.res), (0.5 * gr.res, 0.5 * gr.res, (z1 - z0 + 0.5) * gr.res)))
    assert np.array_equal(box_occupancy(gr.origin, gr.res, gr.dims, boxes), m.occ)
    return scenes.build_grid(gr.origin, gr.dims, gr.res, gr.max_dist, boxes)
