"""Robots of every width: the cases of tests/test_width_references.py (CPU) and tests/test_gpu_widths.py (GPU).

The engine takes up to SMPLX_MAX_VARS = 16 planning variables and SMPLX_MAX_PRIMS = 64 motion primitives, and much of
the device code is shaped by the two numbers:

  * a slot of the state table is a tag and nv coordinates in smplx_table_stride(nv) = ceil((nv + 1) / 8) * 8 ints, and the
    device search reads it as ceil((nv + 1) / 4) words of 16 bytes.  The word count changes at nv = 3 -> 4, 7 -> 8,
    11 -> 12 and 15 -> 16, the stride at 7 -> 8 and 15 -> 16.  WIDTHS holds both sides of every one of these edges and
    the two extremes, 1 and 16;
  * a rec_b record of the compact successor stream puts its doubles behind (nv + 2) / 2 * 2 ints, so odd and even nv
    have different layouts; WIDTHS has five of each;
  * the primitive count M = 3 + 2 * rows decides tid / nprims in every step kernel, whether k_step_block may run
    (smplx_step_states(M) <= 16: first true at M = 9), whether k_search has its helper wave (up to M = 53, not from
    M = 55) and the lane layout of k_small_batch; PRIM_CASES sits on each of these edges and on M = 63, the largest
    count the parser can produce.

chain_robot(nv) is a serial chain whose joint kinds cycle, so every branch of the coordinate discretisation and of the
joint-limit check is taken at low and at high variable indices; the formulas of kernels.h / device_types.h are restated
below in Python, and tests/test_width_references.py holds every case to the edge it is there for.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from smpl_amd import scenes

MAX_VARS, MAX_PRIMS = 16, 64            # SMPLX_MAX_VARS, SMPLX_MAX_PRIMS (device_types.h)
WIDTHS = [1, 2, 3, 4, 7, 8, 11, 12, 15, 16]

DEG = scenes.DEG
ANGLE_RES, SLIDE_RES = 2 * DEG, 0.01    # radians per cell of a rotating variable, metres per cell of a prismatic one
KINDS = ["rev_x", "rev_y", "rev_z", "continuous", "prismatic"]      # variable v is of kind KINDS[v % 5]
LINK = 0.075                            # metres from one joint to the next, along the link's x
LEADS = 3                               # links whose spheres are checked against later links (see chain_robot)


# ----------------------------------------------------------------------------------------------------------------------
# the layout formulas, restated (device_types.h, kernels.h, search_kernel.h, search_table.h, search_host.h)
# ----------------------------------------------------------------------------------------------------------------------

def table_stride(nv):
    """smplx_table_stride: int32 per slot of the state table"""
    return (nv + 1 + 7) // 8 * 8


def slot_words(nv):
    """16-byte words of a slot that hold the tag and the coordinate (table_slot_load)"""
    return (nv + 1 + 3) // 4


def rec_b_ints(nv):
    """ints in front of a rec_b record's doubles: h and the coordinate, padded to an even count"""
    return (nv + 2) // 2 * 2


def rec_b_bytes(nv):
    """smplx_rec_b_bytes"""
    return rec_b_ints(nv) * 4 + nv * 8


def small_block(M):
    """smplx_small_block: threads of a k_small_batch block"""
    return (M * 7 + 1 + 63) // 64 * 64 + 64


def search_block(M):
    """smplx_search_block: threads of a k_search block"""
    b = small_block(M)
    return b + 64 if b + 64 <= 512 else b


def search_has_helper(M):
    return search_block(M) > small_block(M)


def step_states(M):
    """smplx_step_states: most states that 128 consecutive edges belong to"""
    return (128 - 2 + M) // M + 1


def step_allowed(M):
    """whether k_step_block can run at all (SMPLX_STEP_STATES = 16)"""
    return step_states(M) <= 16


def first_table_slots(M, capacity):
    """slots of the state table a device search allocates under smplx_test_set_search_capacity(capacity) on a space that
    holds the goal's entry and the start: the smallest power of two, from 64, that holds its first capacity half full
    (search_run, search_reserve)"""
    states = max(capacity, 2 + 2 * M + 64)
    slots = 64
    while slots < 2 * states:
        slots *= 2
    return slots


# ----------------------------------------------------------------------------------------------------------------------
# the robot
# ----------------------------------------------------------------------------------------------------------------------

def _rpy_matrix(r, p, y):
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def _axis_matrix(axis, q):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(q) * K + (1 - math.cos(q)) * (K @ K)


def _joint_spec(v):
    """(type, axis, origin rpy, lo, hi, start) of the joint of variable v.  Every third origin is rotated; the revolute Z
    joints and the prismatic ones have a limit five cells from the start, the others are wide."""
    kind = KINDS[v % 5]
    rpy = (0.0, 0.2, -0.3) if v % 3 == 1 else (0.0, 0.0, 0.0)
    sign = -1.0 if (v // 5) % 2 else 1.0
    if kind == "rev_x":
        return "revolute", (1, 0, 0), rpy, -2.0, 1.5, 0.3 * sign
    if kind == "rev_y":
        return "revolute", (0, 1, 0), rpy, -1.4, 1.2, -0.2 * sign
    if kind == "rev_z":
        start = 0.25 * sign
        return "revolute", (0, 0, 1), rpy, start - 40 * ANGLE_RES, start + 5 * ANGLE_RES, start
    if kind == "continuous":          # about x, and every other one about an axis that is none of X / Y / Z
        return "continuous", (1, 0, 0) if (v // 5) % 2 == 0 else (0.6, 0.0, 0.8), rpy, 0.0, 0.0, 0.4 * sign
    return "prismatic", (0, 0, 1), rpy, 0.0, 0.25, 5 * SLIDE_RES


def chain_limits(nv):
    """(lo, hi) of every variable; continuous ones as [-pi, pi]"""
    out = []
    for v in range(nv):
        t, _, _, lo, hi, _ = _joint_spec(v)
        out.append((-math.pi, math.pi) if t == "continuous" else (lo, hi))
    return out


def chain_start(nv):
    return [_joint_spec(v)[5] for v in range(nv)]


def chain_resolutions(nv):
    """cell sizes; the single variable of the one-joint robot has cells of a quarter of a degree, so that its lattice, a
    line, has a few hundred cells between the limits"""
    if nv == 1:
        return [ANGLE_RES / 8]
    return [SLIDE_RES if KINDS[v % 5] == "prismatic" else ANGLE_RES for v in range(nv)]


MOUNT_XYZ, MOUNT_RPY = (-0.45, 0.05, 1.0), (0.0, 0.0, 0.2)
TOOL_XYZ = (LINK, 0.12, 0.08)           # off every joint axis: the planning link moves with every variable, the first included


def _spheres(v, nv):
    """one or two spheres on moving link v: (name, x, y, z, r); every fourth link carries a fat one that reaches back
    over its neighbour"""
    out = [(f"s{v}a", 0.5 * LINK, 0.0, 0.0, 0.034)]
    if v % 2 == 0:
        out.append((f"s{v}b", 0.85 * LINK, 0.0, 0.012, 0.03))
    if v % 4 == 3:
        out[0] = (f"s{v}a", 0.3 * LINK, 0.0, 0.0, 0.06)
    return out


def chain_sphere_centres(nv, q):
    """{link index: [(centre in the world, radius)]} at joint values q, by a plain forward kinematics of the chain (the
    conventions of scenes.mixed_kinds_robot: origin = translation * Rz(yaw) Ry(pitch) Rx(roll), a revolute joint turns
    about its axis behind the origin, a prismatic one moves along its local z)"""
    R, t = _rpy_matrix(*MOUNT_RPY), np.asarray(MOUNT_XYZ, dtype=np.float64)
    out = {}
    for v in range(nv):
        typ, axis, rpy, _, _, _ = _joint_spec(v)
        o = np.array([0.0 if v == 0 else LINK, 0.0, 0.04 if v == 0 else 0.0])
        t = t + R @ o
        R = R @ _rpy_matrix(*rpy)
        if typ == "prismatic":
            t = t + R @ np.array([0.0, 0.0, q[v]])
        else:
            R = R @ _axis_matrix(axis, q[v])
        out[v] = [(t + R @ np.array([x, y, z]), r) for (_, x, y, z, r) in _spheres(v, nv)]
    return out


@functools.lru_cache(maxsize=None)
def chain_robot(nv: int) -> str:
    """A serial chain of nv moving joints on a fixed mount, in the format of scenes.mixed_kinds_robot.  Joint kinds cycle
    through revolute about X, Y and Z, continuous and prismatic; every third origin is rotated, so is the mount; every moving
    link carries one or two spheres, and a tool link sits on the last joint.

    Allowed pairs: every pair of links whose spheres touch at the start pose, and every pair whose earlier link is not one
    of the first LEADS links.  The second rule is what keeps the wide robots on the device search: in the kernels
    linked into the library a link that is checked against a later one keeps its root position in per-thread LDS (3 doubles
    for each thread of a k_search block), and with every non-adjacent pair checked a 16-variable chain would need more LDS
    than a CU has (search_heap_cache_entries).
    Every sphere is checked against the grid whatever this list says."""
    assert 1 <= nv <= MAX_VARS
    L = [f"robot chain{nv}", "link base_link", "link mount_link"] + [f"link l{v}" for v in range(nv)] + ["link tool_link"]
    J = "joint {n} {t} {pa} {ch}  {o[0]} {o[1]} {o[2]}  {r[0]} {r[1]} {r[2]}  {a[0]} {a[1]} {a[2]}  {lo} {hi}"
    L.append(J.format(n="mount", t="fixed", pa="base_link", ch="mount_link", o=MOUNT_XYZ, r=MOUNT_RPY, a=(0, 0, 1), lo=0.0, hi=0.0))
    for v in range(nv):
        typ, axis, rpy, lo, hi, _ = _joint_spec(v)
        L.append(J.format(n=f"j{v}", t=typ, pa="mount_link" if v == 0 else f"l{v - 1}", ch=f"l{v}",
                          o=(0.0 if v == 0 else LINK, 0.0, 0.04 if v == 0 else 0.0), r=rpy, a=axis, lo=repr(lo), hi=repr(hi)))
    L.append(J.format(n="tool", t="fixed", pa=f"l{nv - 1}", ch="tool_link", o=TOOL_XYZ, r=(0.0, 0.0, 0.0), a=(0, 0, 1),
                      lo=0.0, hi=0.0))
    for v in range(nv):
        for (name, x, y, z, r) in _spheres(v, nv):
            L.append(f"sphere l{v} {name} {x} {y} {z} {r} 1")
    L.append("group chain " + " ".join(f"l{v}" for v in range(nv)))
    at_start = chain_sphere_centres(nv, chain_start(nv))
    for a in range(nv):
        for b in range(a + 2, nv):          # (adjacent links are never checked)
            touch = any(np.linalg.norm(ca - cb) <= ra + rb + 0.01 for ca, ra in at_start[a] for cb, rb in at_start[b])
            if touch or a >= LEADS:
                L.append(f"acm l{a} l{b}")
    L.append("planning_joints " + " ".join(f"j{v}" for v in range(nv)))
    L.append("planning_link tool_link")
    return "\n".join(L) + "\n"


# ----------------------------------------------------------------------------------------------------------------------
# primitives
# ----------------------------------------------------------------------------------------------------------------------

def default_rows(nv):
    """(variables with a long row, variables with a short row, whether a short row moves every variable at once): a long
    row for each of the first min(nv, 4) variables and a short row for every variable"""
    return tuple(range(min(nv, 4))), tuple(range(nv)), True


def prim_count(rows):
    long_vars, short_vars, all_row = rows
    return 3 + 2 * (len(long_vars) + len(short_vars) + (1 if all_row else 0))


def rows_text(nv, rows, long_cells=3, short_cells=1):
    """the .mprim text (scenes.mprim_text's layout).  The all-variables row moves variable v by +1 or -1 cell, the sign
    alternating with v."""
    long_vars, short_vars, all_row = rows
    table = []
    for v in long_vars:
        r = [0] * nv
        r[v] = long_cells
        table.append(r)
    for v in short_vars:
        r = [0] * nv
        r[v] = short_cells
        table.append(r)
    if all_row:
        table.append([short_cells if v % 2 == 0 else -short_cells for v in range(nv)])
    nshort = len(short_vars) + (1 if all_row else 0)
    out = [f"Motion_Primitives(degrees): {len(table)} {nv} {nshort}"] + [" ".join(str(x) for x in r) for r in table]
    return "\n".join(out) + "\n"


# (name, width, rows): M = 5, 7 and 9 (k_step_block is allowed from 9 on), 53 and 55 (the k_search helper wave fits up to
# 53), 63 (the most the parser produces: 14 long rows and 16 short ones, which leaves no room for an all-variables row)
PRIM_CASES = [
    ("M5", 1, ((), (0,), False)),
    ("M7", 2, ((), (1,), True)),
    ("M9", 2, ((), (0, 1), True)),
    ("M53", 16, (tuple(range(8)), tuple(range(16)), True)),
    ("M55", 16, (tuple(range(9)), tuple(range(16)), True)),
    ("M63", 16, (tuple(range(14)), tuple(range(16)), False)),
]
# what each case is there for: (M, k_step_block allowed, k_search has its helper wave)
PRIM_EXPECT = {"M5": (5, False, True), "M7": (7, False, True), "M9": (9, True, True), "M53": (53, True, True),
               "M55": (55, True, False), "M63": (63, True, False)}
ALL_CASES = [(f"nv{nv}", nv, None) for nv in WIDTHS] + PRIM_CASES


# ----------------------------------------------------------------------------------------------------------------------
# scenes
# ----------------------------------------------------------------------------------------------------------------------

GRID_DIMS, GRID_CAP = (61, 46, 53), 0.4
# (cell size, origin, table): a chain of up to four joints reaches a quarter of a metre, and a joint goal a few cells off
# moves its planning link by centimetres -- the narrow robots get cells of 2 cm around the mount, the wide ones 4 cm
NARROW = (0.02, (-0.9, -0.4, 0.5), ((-0.3, 0.05, 0.62), (0.9, 0.7, 0.04)))
WIDE = (0.04, (-1.1, -0.9, 0.0), ((0.0, 0.0, 0.3), (1.6, 1.2, 0.04)))
# seed of each case's goal and boxes, chosen with the oracle (tests/test_width_references.py holds every case to what the
# choice is for: a start and a goal that are free, a search of at least 200 expansions, a state set that shows every variable)
CASE_SEED = {(2, 7): 1, (2, 9): 1, (2, 13): 1, (3, 17): 5, (4, 21): 3, (7, 27): 5, (8, 29): 2, (11, 35): 5, (12, 37): 1, (15, 43): 3, (16, 45): 3,
             (16, 53): 1, (16, 55): 1, (16, 63): 1}


def _goal_cells(nv, rng, far):
    """goal - start in cells: 6 to 10 cells in about two variables of three (in every one up to nv = 3), towards the far
    limit where a limit is five cells off; a lattice of one or two dimensions gets a goal `far` times as far, or the
    search would be over at once"""
    mag = rng.integers(6, 11, size=nv)
    sign = np.where(rng.random(nv) < 0.5, -1, 1)
    moved = (rng.random(nv) < 0.67) | (nv <= 3)
    c = [int(m * s) if k else 0 for m, s, k in zip(mag, sign, moved)]
    for v in range(nv):
        if KINDS[v % 5] == "rev_z":
            c[v] = -abs(c[v])
        if KINDS[v % 5] == "prismatic":
            c[v] = abs(c[v])
    if nv <= 2:
        c = [-far * abs(x) for x in c]
    return c


@functools.lru_cache(maxsize=None)
def width_case(nv: int, rows=None, seed=None) -> scenes.Config:
    """chain_robot(nv) over a table and five seeded boxes on a 61 x 46 x 53 grid, with the default rows of the width or the
    given ones.  The boxes keep clear of the chain's spheres at the start and at the goal; the joint goal lies 6 to 10 cells
    from the start in several variables.  Short primitives are active within short_thresh of the goal, long ones beyond:
    the threshold is set so that a search from the start sees both."""
    rows = default_rows(nv) if rows is None else rows
    seed = CASE_SEED.get((nv, prim_count(rows)), 0) if seed is None else seed
    goal_rng, box_rng = (np.random.default_rng(1000 + 17 * nv + seed) for _ in range(2))     # (independent of each other's draws)
    res = chain_resolutions(nv)
    start = chain_start(nv)
    far = 40 if nv == 1 else 4 if rows[0] else 2
    goal = [s + c * r for s, c, r in zip(start, _goal_cells(nv, goal_rng, far), res)]
    clear = [c for q in (start, goal) for sp in chain_sphere_centres(nv, q).values() for c, _ in sp]
    clear.append(np.asarray(MOUNT_XYZ))
    cell, origin, table = NARROW if nv <= 4 else WIDE
    boxes = [table] + scenes.random_boxes(box_rng, 5, origin, GRID_DIMS, cell, clear, 5.5 * cell, edge=(2 * cell, 7 * cell))
    grid = scenes.build_grid(origin, GRID_DIMS, cell, GRID_CAP, boxes)
    # short primitives within three cells of the goal, long ones beyond; the snap to the goal from inside the goal's cell
    # (rows without a long one: the short ones everywhere)
    p = scenes.PlanningParams(res, eps0=5.0, bfs_radius=cell, cost_per_cell=500, short_thresh=3 * cell if rows[0] else 100.0,
                              xyzrpy_thresh=0.0)
    return scenes.Config(f"chain{nv}_M{prim_count(rows)}", chain_robot(nv), rows_text(nv, rows), grid, p, start, goal,
                         [1.5 * r for r in res], boxes)


def unreachable_goal(nv):
    """width_case(nv)'s joint goal with variable 0 five cells below its lower limit: no state inside the limits satisfies it
    (the tolerance is a cell and a half), and the lattice inside the limits is finite, so a search for it pops every
    reachable state once and ends with an empty OPEN (tests/test_arastar_loop.py, tests/test_gpu_search_endings.py)"""
    cfg = width_case(nv)
    return [chain_limits(nv)[0][0] - 5 * cfg.params.resolutions[0]] + list(cfg.goal[1:])


def case_config(name):
    """the Config of an entry of ALL_CASES"""
    for n, nv, rows in ALL_CASES:
        if n == name:
            return width_case(nv, rows)
    raise KeyError(name)


def batch_states(cfg, n=300, seed=5, spread=6):
    """n states on whole cells within `spread` cells of the start in every variable; row 0 is the start, row 1 a state in
    the goal's cell"""
    nv = len(cfg.start)
    rng = np.random.default_rng(seed + nv)
    res = np.asarray(cfg.params.resolutions)
    Q = np.asarray(cfg.start)[None, :] + rng.integers(-spread, spread + 1, size=(n, nv)) * res[None, :]
    Q[0] = cfg.start
    Q[1] = cfg.goal
    return np.ascontiguousarray(Q)


def plain_table(space):
    """{coordinate tuple: state id} over get_state(i) of every id of a space or an oracle: the state table as a dict"""
    return {tuple(int(x) for x in space.get_state(i)[1]): i for i in range(space.num_states())}


def pairs_differing_in_one_variable(coords):
    """count, per variable v, of the unordered pairs of distinct coordinates that differ in v alone"""
    coords = [tuple(c) for c in coords]
    nv = len(coords[0])
    out = [0] * nv
    for v in range(nv):
        groups = {}
        for c in coords:
            k = c[:v] + c[v + 1:]
            groups[k] = groups.get(k, 0) + 1
        out[v] = sum(g * (g - 1) // 2 for g in groups.values())
    return out
