"""Edit semantics of the distance field on the GPU (smpl_amd/csrc/field.hip) against tests/field_model.py, the plain
model of the reference's edit loops that tests/test_field_model.py guards on the CPU: mixed counted and uncounted
operations, boxes with counts, the window an edit recomputes, the 16-bit limit, and the brick-tiled field the collision
kernels read."""
import dataclasses

import numpy as np
import pytest

import field_model as fm
from noncubic_cases import brute_force

pytestmark = pytest.mark.gpu

ORIGIN = (-0.3, 0.1, 0.0)
# dims, res, max_dist, dmax
SEQUENCE_GRIDS = [((13, 10, 7), 0.05, 0.2, 4),
                  ((1, 9, 6), 0.05, 0.2, 4),
                  ((2, 3, 17), 0.05, 0.2, 4),
                  ((6, 6, 6), 0.05, 0.05, 1),            # dmax 1: every scan loop of the three passes is empty
                  ((7, 5, 9), 0.05, 0.5, 10),            # dmax beyond every extent
                  ((21, 18, 15), 0.02, 0.08, 4)]         # small windows inside a grid that is no multiple of the brick


@pytest.mark.parametrize("dims,res,max_dist,dmax", SEQUENCE_GRIDS, ids=["x".join(map(str, g[0])) for g in SEQUENCE_GRIDS])
def test_random_edit_sequences_equal_the_model(dims, res, max_dist, dmax):
    """After every operation of a seeded sequence the field equals the brute-force transform of the model's flags, and the
    counts equal the model's.  The sequence is first run on the model alone: it must hold every kind of operation, reach
    a state where the flags are not `counts > 0` (the gap an occupancy model of counts alone cannot see), and hold a
    counted add on a cell that an update freed while its count stayed positive."""
    from smpl_amd import capi
    assert fm.dmax_of(res, max_dist) == dmax
    ops = fm.random_ops(101, ORIGIN, dims, res, n=60)
    assert len(ops) >= 60
    assert {k for k, _ in ops} == set(fm.OP_KINDS)
    m = fm.FieldModel(ORIGIN, dims, res)
    out_of_step = add_on_freed = 0
    for kind, payload in ops:
        if kind == "add" and m.counts is not None:       # a counted add on a cell that is free with a positive count: it stays free
            add_on_freed += any(m.counts[tuple(c)] > 0 and not m.occ[tuple(c)] for c in m.cells(payload) if m.in_bounds(c))
        fm.apply(m, kind, payload)
        out_of_step += m.counts is not None and not np.array_equal(m.occ, m.counts > 0)
    assert out_of_step > 0 and add_on_freed > 0

    g = capi.Grid.empty(ORIGIN, dims, res, max_dist)
    m = fm.FieldModel(ORIGIN, dims, res)
    occ, want = m.occ.copy(), m.d2(dmax)
    assert np.array_equal(g.d2(), want)
    for step, (kind, payload) in enumerate(ops):
        fm.apply(g, kind, payload)
        fm.apply(m, kind, payload)
        if not np.array_equal(m.occ, occ):               # (the transform is a function of the flags alone)
            occ, want = m.occ.copy(), m.d2(dmax)
        assert np.array_equal(g.d2(), want), (step, kind)
        if m.counts is not None:
            assert np.array_equal(g.counts(), m.counts), (step, kind)
        else:
            with pytest.raises(capi.SmplxError) as err:
                g.counts()
            assert err.value.code == -5, (step, kind)
    assert m.occ.any()


def test_edit_windows_on_a_grid_that_is_no_multiple_of_the_brick():
    """(21, 18, 15) with a cap of 4 cells: last_edit_cells() is what edit_window's rule gives -- the bounding box of the
    listed cells inside the grid, grown by 4, clipped; the whole grid when that is MORE than half of it -- and the field
    equals the model after every edit."""
    from smpl_amd import capi
    dims, res, max_dist, dmax = (21, 18, 15), 0.02, 0.08, 4
    whole = 21 * 18 * 15
    assert fm.dmax_of(res, max_dist) == dmax
    g = capi.Grid.empty(ORIGIN, dims, res, max_dist)
    m = fm.FieldModel(ORIGIN, dims, res)
    assert g.last_edit_cells() == whole                  # the empty field was built over the whole grid

    def world(cells):
        return np.asarray(ORIGIN) + np.asarray(cells, dtype=np.float64).reshape(-1, 3) * res

    def window(pts):
        lo, hi = fm.bounding_box(m, pts)
        return fm.edit_window_cells(dims, dmax, lo, hi)

    def check(kind, payload, cells, tag):
        fm.apply(g, kind, payload)
        fm.apply(m, kind, payload)
        assert g.last_edit_cells() == cells, tag
        assert np.array_equal(g.d2(), m.d2(dmax)), tag

    outside = np.array([[9.0, 9.0, 9.0], [-5.0, 0.0, 0.0]])
    for cell, cells in (((0, 0, 0), 5 * 5 * 5),          # a corner
                        ((0, 17, 7), 5 * 5 * 9),         # an edge
                        ((10, 9, 7), 9 * 9 * 9)):        # the middle: the window's low corner (6, 5, 3) is on no brick boundary
        pts = np.vstack([world([cell]), outside])
        assert window(pts) == cells
        check("add", pts, cells, cell)
    check("remove", world([(10, 9, 7)]), 9 * 9 * 9, "remove")
    # x 4..16 and z 4..10 grow to the whole of their axes, y 9 to 5..13: 21 * 9 * 15 cells, exactly half of the grid
    half = world([(4, 9, 4), (16, 9, 10), (9, 9, 7)])
    assert window(half) == 21 * 9 * 15 == whole // 2 and whole % 2 == 0
    check("add", half, whole // 2, "half")
    # one more layer of y (3150 cells, more than half): everything
    over = world([(4, 9, 4), (16, 10, 10)])
    assert window(over) == whole
    check("add", over, whole, "over half")
    # clipped on both sides of x: x 2..18 grows to -2..22
    both = world([(2, 9, 7), (18, 9, 7)])
    assert window(both) == 21 * 9 * 9
    check("add", both, 21 * 9 * 9, "clipped on both sides")
    # a call with nothing inside the grid: the field and the window stay as they were
    before = g.d2()
    for kind in ("add", "remove"):
        fm.apply(g, kind, outside)
        assert g.last_edit_cells() == 21 * 9 * 9 and np.array_equal(g.d2(), before), kind
    g.add_boxes([((50.0, 0.0, 0.0), (0.1, 0.1, 0.1))])
    g.update_points(outside, outside[::-1])
    assert g.last_edit_cells() == 21 * 9 * 9 and np.array_equal(g.d2(), before)
    # an update is two edits, old \ new removed, then new \ old added: the window left behind is the second one's
    old, new = both, world([(2, 9, 7), (12, 3, 11)])
    check("update", (old, new), window(world([(12, 3, 11)])), "update")
    assert g.last_edit_cells() == 9 * 8 * 8              # x 8..16, y 0..7, z 7..14
    # when nothing is added, the first one's
    check("update", (world([(12, 3, 11), (0, 0, 0)]), world([(0, 0, 0)])), 9 * 8 * 8, "update, removal only")
    # a box through the high face of y: its window comes from its clipped cells, x 5..6, y 16..17, z 2
    box = ((ORIGIN[0] + 5.5 * res, ORIGIN[1] + 17.5 * res, ORIGIN[2] + 2 * res), (1.6 * res, 3.6 * res, 0.3 * res))
    assert m.box_range(*box) == ([5, 16, 2], [6, 17, 2])
    check("box_clipped", [box], 10 * 6 * 7, "box")
    # with counts a remove that frees nothing still recomputes the window of the cells it names
    g.set_ref_counted(True)
    m.set_ref_counted(True)
    check("add", world([(2, 9, 7)]), 7 * 9 * 9, "counted add on an occupied cell")
    check("remove", world([(2, 9, 7)]), 7 * 9 * 9, "counted remove, count 2 -> 1")
    assert m.occ[2, 9, 7] and m.counts[2, 9, 7] == 1 and np.array_equal(g.counts(), m.counts)


def test_the_16_bit_limit_is_255_cells():
    """Squared distances are 16-bit: a cap of 255 cells (65 025) is served, 256 cells (65 536) is refused with
    SMPLX_E_LIMIT, and the refusal leaves the library usable."""
    from smpl_amd import capi
    origin, dims, res = (0.0, 0.0, 0.0), (2, 2, 2), 0.01
    max_dist = 2.55
    if fm.dmax_of(res, max_dist) == 256:                 # (2.55 * 100.0 rounds to just under 255.0 in fp64; in case it does not)
        max_dist = np.nextafter(max_dist, 0.0)
    assert fm.dmax_of(res, max_dist) == 255
    g = capi.Grid.empty(origin, dims, res, max_dist)
    occ = np.zeros(dims, bool)
    assert np.array_equal(g.d2(), brute_force(occ, 255))
    g.add_points(np.array([[0.01, 0.0, 0.01]]))
    occ[1, 0, 1] = True
    assert np.array_equal(g.d2(), brute_force(occ, 255))
    assert fm.dmax_of(res, 2.56) == 256
    with pytest.raises(capi.SmplxError) as err:
        capi.Grid.empty(origin, dims, res, 2.56)
    assert err.value.code == -3                          # SMPLX_E_LIMIT, include/smpl_amd.h
    g3 = capi.Grid.empty(origin, dims, res, 0.05)
    assert np.array_equal(g3.d2(), brute_force(np.zeros(dims, bool), 5))
    assert np.array_equal(g.d2(), brute_force(occ, 255))  # and the earlier grid is as it was


def test_one_edit_of_more_than_2_to_the_24_points_edits_every_point():
    """k_occ_points handles one cell a thread, so its launch must cover every listed cell (field.hip occ_points): a grid
    capped at 65 536 blocks of 256 threads stops after 2^24 points.  One add_points call on a reference-counted 32^3 grid
    carries 2^24 + 512 points: the first 2^24 cycle through the 4 096 cells of the slab x < 4 (each listed 4 096 times),
    the last 512 fall into 512 distinct cells with x >= 16.  Counts equal the bincount of the cells and the field the
    model's on that occupancy; one remove_points call with the same array leaves zero counts and the empty grid's field."""
    from smpl_amd import capi
    dims, res, max_dist, dmax = (32, 32, 32), 0.05, 0.2, 4
    assert fm.dmax_of(res, max_dist) == dmax
    m = fm.FieldModel(ORIGIN, dims, res)
    slab = np.argwhere(np.ones((4, 32, 32), bool))                                # 4 096 cells, x < 4
    tail = np.argwhere(np.ones((8, 8, 8), bool)) + (16, 3, 5)                      # 512 cells, x 16..23
    unique = np.vstack([slab, tail])
    world = np.asarray(ORIGIN) + unique.astype(np.float64) * res                   # cell centres
    assert np.array_equal(m.cells(world), unique)
    n = 2 ** 24 + 512
    pts = np.empty((n, 3), np.float64)
    pts[:2 ** 24].reshape(4096, 4096, 3)[:] = world[:4096]                         # tiled, not looped
    pts[2 ** 24:] = world[4096:]
    flat = np.empty(n, np.int64)
    flat[:2 ** 24].reshape(4096, 4096)[:] = np.ravel_multi_index(slab.T, dims)
    flat[2 ** 24:] = np.ravel_multi_index(tail.T, dims)
    want = np.bincount(flat, minlength=32 ** 3).reshape(dims)
    assert want[:4].min() == want.max() == 4096 and (want == 1).sum() == 512 and want.sum() == n

    g = capi.Grid.empty(ORIGIN, dims, res, max_dist)
    empty = g.d2()
    g.set_ref_counted(True)
    g.add_points(pts)
    got = g.counts()
    print(f"counted points: {int(got.sum())} of {n}; cells of the last 512 that are occupied: {int((got[16:] > 0).sum())}")
    assert np.array_equal(got, want)
    m.occ = want > 0
    assert np.array_equal(g.d2(), m.d2(dmax))
    g.remove_points(pts)
    assert not g.counts().any()
    assert np.array_equal(g.d2(), empty)
    assert np.array_equal(empty, capi.Grid.empty(ORIGIN, dims, res, max_dist).d2())


def test_collision_kernels_read_the_edited_field_as_a_host_tiled_upload_of_the_model(small_cfg):
    """The tiled field k_edt_axis<true> writes, judged by the kernels that read it and not by k_untile: after each of a
    windowed add, a remove and an update near the arm, 512 states get the same verdicts and the same lookup tallies from
    a space on the edited grid as from a space on the model's field uploaded as a finished one (tiled on the host, an
    independent path), and the verdicts are the CPU oracle's on that field.  At least 5 % of the verdicts differ from
    those before the edits (tests/test_field_model.py holds that for the oracle alone)."""
    from oracle_binding import Oracle
    from smpl_amd import capi
    cfg, gr = small_cfg, small_cfg.grid
    model = capi.Model(cfg.robot_text)
    oracle = Oracle(cfg)
    states, edits = fm.arm_edits(cfg, lambda q: oracle.sphere_positions(q, model.nnodes))
    g = capi.Grid.from_boxes(gr.origin, gr.dims, gr.res, gr.max_dist, cfg.boxes)
    s = capi.Space(model, g, cfg.mprim, cfg.params, 256)
    v0, _ = s.state_valid_batch(states)
    v0 = v0.copy()
    whole = gr.dims[0] * gr.dims[1] * gr.dims[2]
    for k, (kind, payload) in enumerate(edits):
        fm.apply(g, kind, payload)
        assert g.last_edit_cells() < whole, kind         # a window, not a rebuild
        want = fm.arm_edited_grid(cfg, edits[:k + 1])
        fixed = capi.Grid(gr.origin, gr.dims, gr.res, gr.max_dist, want.d2)
        t = capi.Space(model, fixed, cfg.mprim, cfg.params, 256)
        v, lk = s.state_valid_batch(states)
        vt, lkt = t.state_valid_batch(states)
        print(f"{kind}: {int(v.sum())} of {len(v)} valid, {float((v != v0).mean()):.3f} of the verdicts changed")
        assert np.array_equal(v, vt), kind
        assert np.array_equal(lk, lkt), kind
        after = Oracle(dataclasses.replace(cfg, grid=want))
        assert np.array_equal(v != 0, np.array([after.state_valid(q)[0] for q in states])), kind
        assert (v != v0).mean() >= 0.05, kind
        assert np.array_equal(g.d2(), want.d2), kind
