"""The reference the GPU field-edit tests lean on (tests/field_model.py), held to two independent witnesses on the CPU:
a literal dict of cell -> (flag, count) driven one point at a time through the reference's loops, and, for box-only
scenes, the host builder's transform (scenes.build_grid, a scipy feature transform).  No GPU."""
import itertools

import numpy as np
import pytest

import field_model as fm
from smpl_amd import scenes

GRIDS = [((13, 10, 7), 0.05, 0.2), ((1, 9, 6), 0.05, 0.2), ((2, 3, 17), 0.05, 0.2), ((21, 18, 15), 0.02, 0.08)]
ORIGIN = (-0.3, 0.1, 0.0)


class DictField:
    """cell -> [flag, count], one point at a time.  Slow, and obviously the reference's loops:
    occupancy_grid.cpp:357-441 over distance_map.hpp:306-435."""

    def __init__(self, origin, dims, res):
        self.origin, self.dims, self.res = origin, dims, res
        self.cell = {c: [False, 0] for c in itertools.product(*[range(n) for n in dims])}
        self.counted = False

    def _cell(self, p):
        c = tuple(int(v) for v in scenes.world_to_grid(self.origin, self.res, np.asarray(p, dtype=np.float64)))
        return c if c in self.cell else None             # isInBounds / isCellValid

    def add_points(self, pts):
        forwarded = []
        for p in np.asarray(pts).reshape(-1, 3):
            c = self._cell(p)
            if c is None:
                continue
            if not self.counted:
                forwarded.append(c)
                continue
            if self.cell[c][1] == 0:
                forwarded.append(c)
            self.cell[c][1] += 1
        for c in forwarded:                              # addPointsToMap, after the loop as in the reference
            self.cell[c][0] = True

    def remove_points(self, pts):
        forwarded = []
        for p in np.asarray(pts).reshape(-1, 3):
            c = self._cell(p)
            if c is None:
                continue
            if not self.counted:
                forwarded.append(c)
                continue
            if self.cell[c][1] > 0:
                self.cell[c][1] -= 1
                if self.cell[c][1] == 0:
                    forwarded.append(c)
        for c in forwarded:                              # removePointsFromMap
            self.cell[c][0] = False

    def update_points(self, old_pts, new_pts):
        old, new = set(), set()
        for p in np.asarray(old_pts).reshape(-1, 3):
            if self._cell(p) is not None:
                old.add(self._cell(p))
        for p in np.asarray(new_pts).reshape(-1, 3):
            if self._cell(p) is not None:
                new.add(self._cell(p))
        for c in old:
            if c not in new:
                self.cell[c][0] = False
        for c in new:
            if c not in old:
                self.cell[c][0] = True

    def set_ref_counted(self, on):
        self.counted = bool(on)
        for c, v in self.cell.items():
            v[1] = (1 if v[0] else 0) if on else 0

    def add_boxes(self, boxes):
        for center, size in boxes:
            lo = scenes.world_to_grid(self.origin, self.res, np.asarray(center) - 0.5 * np.asarray(size))
            hi = scenes.world_to_grid(self.origin, self.res, np.asarray(center) + 0.5 * np.asarray(size))
            for c, v in self.cell.items():               # cell by cell: inside the box or not
                if all(lo[a] <= c[a] <= hi[a] for a in range(3)):
                    v[0] = True
                    if self.counted:
                        v[1] += 1

    def arrays(self):
        occ = np.zeros(self.dims, bool)
        counts = np.zeros(self.dims, np.int64)
        for c, (flag, count) in self.cell.items():
            occ[c], counts[c] = flag, count
        return occ, (counts if self.counted else None)


@pytest.mark.parametrize("dims,res,max_dist", GRIDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_model_equals_the_dict_restatement(dims, res, max_dist):
    model, ref = fm.FieldModel(ORIGIN, dims, res), DictField(ORIGIN, dims, res)
    seen, out_of_step = set(), False
    for step, (kind, payload) in enumerate(fm.random_ops(17, ORIGIN, dims, res, n=300)):
        fm.apply(model, kind, payload)
        fm.apply(ref, kind, payload)
        occ, counts = ref.arrays()
        assert np.array_equal(model.occ, occ), (step, kind)
        assert (model.counts is None) == (counts is None), (step, kind)
        if counts is not None:
            assert np.array_equal(model.counts, counts), (step, kind)
            out_of_step = out_of_step or not np.array_equal(model.occ, model.counts > 0)
        seen.add(kind)
    assert seen == set(fm.OP_KINDS)
    assert out_of_step               # flag and counts did part: `counts > 0` would not have been a model of this sequence


def test_every_box_case_is_what_its_name_says():
    """the sequences hold boxes that are clipped, dropped, thinner than a cell, overlapping, and over earlier points"""
    dims, res = (13, 10, 7), 0.05
    m = fm.FieldModel(ORIGIN, dims, res)
    raw = {k: 0 for k in fm.OP_KINDS if k.startswith("box_")}
    for kind, payload in fm.random_ops(17, ORIGIN, dims, res, n=300):
        if kind == "box_outside":
            assert all(m.box_range(c, s) is None for c, s in payload)
            raw[kind] += 1
        elif kind == "box_clipped":
            for c, s in payload:
                lo = m.cells(np.asarray(c) - 0.5 * np.asarray(s))[0]
                hi = m.cells(np.asarray(c) + 0.5 * np.asarray(s))[0]
                assert m.box_range(c, s) is not None and (np.any(lo < 0) or np.any(hi >= np.asarray(dims)))
            raw[kind] += 1
        elif kind == "box_thin":
            assert all(min(s) < res for c, s in payload)
            raw[kind] += 1
        elif kind == "box_overlap":
            (a0, a1), (b0, b1) = m.box_range(*payload[0]), m.box_range(*payload[1])
            assert all(max(a0[a], b0[a]) <= min(a1[a], b1[a]) for a in range(3))
            raw[kind] += 1
        elif kind == "box_on_points":
            raw[kind] += 1
        fm.apply(m, kind, payload)
    assert all(v >= 2 for v in raw.values()), raw


@pytest.mark.parametrize("dims,res,max_dist", GRIDS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_model_field_equals_the_host_builder_on_boxes(dims, res, max_dist):
    """brute force (the model's d2) against the scipy transform of scenes.build_grid, on the boxes of a sequence"""
    boxes = [b for kind, payload in fm.random_ops(23, ORIGIN, dims, res) if kind.startswith("box_") for b in payload]
    assert len(boxes) > 12
    for k in (0, 3, len(boxes)):
        m = fm.FieldModel(ORIGIN, dims, res)
        m.add_boxes(boxes[:k])
        host = scenes.build_grid(ORIGIN, dims, res, max_dist, boxes[:k])
        assert np.array_equal(m.d2(fm.dmax_of(res, max_dist)), host.d2), k
    assert m.occ.any() and not m.occ.all()


def test_window_rule():
    """edit_window_cells restates field.hip's edit_window; the figures the existing 128^3 test asserts follow from it"""
    d = (128, 128, 128)
    assert fm.edit_window_cells(d, 20, [64, 64, 64], [64, 64, 64]) == 41 ** 3
    assert fm.edit_window_cells(d, 20, [2, 120, 64], [2, 120, 64]) == 23 * 28 * 41
    assert fm.edit_window_cells((21, 18, 15), 4, [4, 9, 4], [16, 9, 10]) == 21 * 9 * 15 == 5670 // 2      # exactly half: a window
    assert fm.edit_window_cells((21, 18, 15), 4, [4, 9, 4], [16, 10, 10]) == 5670                          # over half: the grid


def test_arm_edits_flip_verdicts_of_the_reference(small_cfg):
    """The edits of tests/test_gpu_field_edits.py's check of the tiled field, judged by the CPU oracle alone: at least
    5 % of the 512 states change their verdict between the scene's field and the field after each edit."""
    import dataclasses
    from oracle_binding import Oracle
    from smpl_amd import capi
    cfg, gr = small_cfg, small_cfg.grid
    nnodes = capi.Model(cfg.robot_text).nnodes
    before = Oracle(cfg)
    states, edits = fm.arm_edits(cfg, lambda q: before.sphere_positions(q, nnodes))
    v0 = np.array([before.state_valid(q)[0] for q in states])
    for k in range(1, len(edits) + 1):
        after = Oracle(dataclasses.replace(cfg, grid=fm.arm_edited_grid(cfg, edits[:k])))
        v1 = np.array([after.state_valid(q)[0] for q in states])
        assert (v0 != v1).mean() >= 0.05, (k, (v0 != v1).mean())
        assert v1.any() and not v1.all()
    # and every edit moved something: each intermediate occupancy differs from the one before
    m = fm.FieldModel(gr.origin, gr.dims, gr.res)
    m.add_boxes(cfg.boxes)
    for kind, payload in edits:
        occ = m.occ.copy()
        fm.apply(m, kind, payload)
        assert not np.array_equal(occ, m.occ), kind
