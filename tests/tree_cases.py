"""Sphere-tree walks at their edges: the robots, scenes, state sets and the probe of tests/test_tree_references.py (CPU)
and tests/test_gpu_tree_walks.py (GPU).

The walks of smpl_amd/csrc/sphere_checks.h, config_checks.h, clearance.h and attached_bodies.h rest on three fixed-size
pieces of scratch: the per-thread byte stack in LDS (model_compile.cpp sizes it: 16 .. 64 bytes), the queue of twelve
pending pairs (SMPLX_PENDING_MAX; beyond it every checked pair is walked again) and the pair bookkeeping that re-derives a
pair's orientation from tree indices.  The robots here sit on those edges:

    deep     two 17-leaf trees of depth 16 that form a checked pair: stack need 2 * (16 + 16) = 64 = SMPLX_STACK_MAX
    deep40   the same chain with 12 + 10 leaves: need 2 * (11 + 9) = 40 = stack_bytes (no multiple of 16)
    crowd    nine short links in a row, every tree an inner root over two leaves set wide apart: 28 checked pairs whose
             roots overlap at most poses while leaves rarely touch -- the queue runs from 0 to far beyond 12
    order    two levels of branching (both save slots), group links listed in an order that is not depth-first order,
             single-leaf and inner trees mixed, a tree that leads no pair

The probe restates the walks recursively in plain Python: no explicit stack, no queue, no regrouping.  It works from
Oracle.model(), Oracle.sphere_positions and Oracle.grid_sqdist, and adds to the oracle's verdict what no engine reports: how
much stack a pair walk holds, which stack bytes it reads back, how long the queue gets, which pair decides.
"""
from __future__ import annotations

import functools
import math

import numpy as np

from smpl_amd import scenes

DEG = scenes.DEG
RES, CAP = 0.04, 0.4
DIMS = (48, 40, 32)
ORIGIN = (-0.96, -0.8, 0.0)
PENDING_MAX = 12            # sphere_checks.h SMPLX_PENDING_MAX
STACK_MIN, STACK_MAX = 16, 64

_J = "joint {n} {t} {pa} {ch}  {o[0]} {o[1]} {o[2]}  {r[0]} {r[1]} {r[2]}  {a[0]} {a[1]} {a[2]}  {lo} {hi}"


class _Text:
    """lines of a robot in the text format of scenes.mixed_kinds_robot"""

    def __init__(self, name, links):
        self.L = [f"robot {name}"] + [f"link {l}" for l in links]

    def joint(self, n, t, pa, ch, o=(0, 0, 0), r=(0, 0, 0), a=(0, 0, 1), lo=0.0, hi=0.0):
        self.L.append(_J.format(n=n, t=t, pa=pa, ch=ch, o=o, r=r, a=a, lo=lo, hi=hi))

    def sphere(self, link, name, x, y, z, r, pr=1):
        self.L.append(f"sphere {link} {name} {float(x)!r} {float(y)!r} {float(z)!r} {float(r)!r} {pr}")

    def text(self, group, planning_joints, planning_link, acm=()):
        t = "\n".join(self.L) + "\n"
        t += "group g " + " ".join(group) + "\n"
        t += "".join(f"acm {a} {b}\n" for a, b in acm)
        t += "planning_joints " + " ".join(planning_joints) + "\n"
        t += f"planning_link {planning_link}\n"
        return t


# ----------------------------------------------------------------------------------------------------------------------
# robots
# ----------------------------------------------------------------------------------------------------------------------

def row_x(k):
    """The tree builder splits a link's spheres at the mean along the axis of largest extent
    (model_compile.cpp TreeBuilder::build): of 0.25 * 20^-k, k = j .. n-1, only the first lies above the mean, so every
    level peels one sphere off to the right and the tree of n spheres has depth n - 1."""
    return 0.25 * 20.0 ** -k


def row_radius(k, n):
    """Leaf radii of a row of n.  From k = 3 on the spheres of a row sit within 0.04 mm of the link origin, and the
    bounding sphere of such a sub-row is its largest leaf: the last leaf small, the one before it large and so on in turn,
    so that an inner node overlaps where the first leaf pair the walk reaches (the left children: the last leaves) does
    not, and the walk has to come back up for the pair that decides."""
    if k < 3:
        return (0.05, 0.02, 0.012)[k]
    return 0.012 if (n - 1 - k) % 2 else 0.005


DEEP_ARM = 0.30
DEEP_LIMITS = [(-1.5, 1.5), (-1.2, 1.2), (-2.8, 2.8)]


def deep_robot(na: int = 17, nc: int = 17, name: str = "deep") -> str:
    """mount - a - mid - c in a plane tilted against the grid.  `mid` is as long as `a` and its joint's origin is turned by
    pi: at jm = 0 it lies back along `a` and puts the origin of `c` -- the dense end of its row -- onto the origin of `a`."""
    T = _Text(name, ["base_link", "mount", "a", "mid", "c", "tool_link"])
    T.joint("mount_fix", "fixed", "base_link", "mount", o=(0.0, -0.05, 0.62), r=(0.15, -0.1, 0.4))
    T.joint("ja", "revolute", "mount", "a", o=(0.0, 0.0, 0.05), a=(0, 0, 1), lo=DEEP_LIMITS[0][0], hi=DEEP_LIMITS[0][1])
    T.joint("jm", "revolute", "a", "mid", o=(DEEP_ARM, 0.0, 0.0), r=(0.0, 0.0, repr(math.pi)), a=(0, 0, 1),
            lo=DEEP_LIMITS[1][0], hi=DEEP_LIMITS[1][1])
    T.joint("jc", "revolute", "mid", "c", o=(DEEP_ARM, 0.0, 0.0), a=(0, 0, 1), lo=DEEP_LIMITS[2][0], hi=DEEP_LIMITS[2][1])
    T.joint("tool", "fixed", "c", "tool_link", o=(0.27, 0.0, 0.0))
    for link, n in (("a", na), ("c", nc)):
        for k in range(n):
            T.sphere(link, f"{link}{k}", row_x(k), 0.0, 0.0, row_radius(k, n))
    T.sphere("mid", "m0", 0.5 * DEEP_ARM, 0.0, 0.0, 0.03)
    return T.text(["a", "mid", "c"], ["ja", "jm", "jc"], "tool_link")


CROWD_LINKS = 9
CROWD_STEP = 0.05
CROWD_LIMITS = [(-2.8, 2.8)] * 4


def crowd_robot() -> str:
    """Nine links 5 cm apart; every second joint turns about z, the others are fixed.  Each link carries two small leaves
    +-w along z (the joints' axis: two links' leaves are as far apart as their roots are), so a root is an inner sphere of
    radius w + r: with the chain stretched no two non-adjacent roots overlap, curled up most of the 28 pairs do."""
    names = [f"k{i}" for i in range(CROWD_LINKS)]
    T = _Text("crowd", ["base_link", "mount"] + names + ["tool_link"])
    T.joint("mount_fix", "fixed", "base_link", "mount", o=(-0.1, 0.05, 0.6), r=(-0.2, 0.1, -0.3))
    prev = "mount"
    var = 0
    pj = []
    for i, n in enumerate(names):
        if i % 2 == 1:
            T.joint(f"t{i}", "revolute", prev, n, o=(CROWD_STEP, 0.0, 0.0), a=(0, 0, 1), lo=CROWD_LIMITS[var][0],
                    hi=CROWD_LIMITS[var][1])
            pj.append(f"t{i}")
            var += 1
        else:
            T.joint(f"f{i}", "fixed", prev, n, o=(CROWD_STEP, 0.0, 0.0), r=(0.0, 0.0, 0.05 * i))
        w = 0.024 + 0.002 * (i % 4)
        r = 0.010 + 0.001 * (i % 3)
        T.sphere(n, f"{n}u", 0.0, 0.0, w, r)
        T.sphere(n, f"{n}d", 0.0, 0.0, -w, r)
        prev = n
    T.joint("tool", "fixed", prev, "tool_link", o=(0.03, 0.0, 0.0))
    return T.text(names, pj, "tool_link")


ORDER_LIMITS = [(-2.0, 2.0), (-2.4, 2.4), (-2.0, 2.0), (-2.4, 2.4)]
ORDER_GROUP = ["r2", "l2", "fb", "l1", "r1", "fa"]          # depth-first order is l1 l2 r1 r2 fa fb


def order_robot() -> str:
    """mount carries two arms (the first save slot), the right arm's second link two fingers (the second).  The group lists
    the links in an order that is neither depth-first order nor its reverse; l2 and fb are single leaves, the others inner
    trees of unequal radii.  fb comes last in depth-first order: it leads no pair."""
    T = _Text("order", ["base_link", "mount", "l1", "l2", "r1", "r2", "fa", "fb", "tool_link"])
    T.joint("mount_fix", "fixed", "base_link", "mount", o=(0.05, 0.0, 0.6), r=(0.1, 0.2, -0.2))
    T.joint("jl1", "revolute", "mount", "l1", o=(0.0, 0.09, 0.0), a=(0, 0, 1), lo=ORDER_LIMITS[0][0], hi=ORDER_LIMITS[0][1])
    T.joint("jl2", "revolute", "l1", "l2", o=(0.16, 0.0, 0.0), a=(0, 0, 1), lo=ORDER_LIMITS[1][0], hi=ORDER_LIMITS[1][1])
    T.joint("jr1", "revolute", "mount", "r1", o=(0.0, -0.09, 0.0), a=(0, 0, 1), lo=ORDER_LIMITS[2][0], hi=ORDER_LIMITS[2][1])
    T.joint("jr2", "revolute", "r1", "r2", o=(0.16, 0.0, 0.0), a=(0, 0, 1), lo=ORDER_LIMITS[3][0], hi=ORDER_LIMITS[3][1])
    T.joint("ffa", "fixed", "r2", "fa", o=(0.14, 0.03, 0.0), r=(0.0, 0.0, 0.3))
    T.joint("ffb", "fixed", "r2", "fb", o=(0.14, -0.03, 0.0), r=(0.0, 0.0, -0.3))
    T.joint("tool", "fixed", "fa", "tool_link", o=(0.06, 0.0, 0.0))
    T.sphere("l1", "l1a", 0.04, 0.0, 0.0, 0.035)
    T.sphere("l1", "l1b", 0.12, 0.0, 0.0, 0.025)
    T.sphere("l2", "l2a", 0.10, 0.0, 0.0, 0.045)
    T.sphere("r1", "r1a", 0.03, 0.0, 0.0, 0.03)
    T.sphere("r1", "r1b", 0.09, 0.0, 0.0, 0.02)
    T.sphere("r1", "r1c", 0.13, 0.0, 0.02, 0.015)
    T.sphere("r2", "r2a", 0.04, 0.0, 0.0, 0.03)
    T.sphere("r2", "r2b", 0.10, 0.0, 0.0, 0.022)
    T.sphere("fa", "fa0", 0.02, 0.0, 0.0, 0.014)
    T.sphere("fa", "fa1", 0.05, 0.0, 0.0, 0.011)
    T.sphere("fb", "fb0", 0.03, 0.0, 0.0, 0.02)
    return T.text(ORDER_GROUP, ["jl1", "jl2", "jr1", "jr2"], "tool_link")


def limit_robot(leaves, npairs, name="limits") -> str:
    """A serial chain of len(leaves) links, link i with leaves[i] spheres in a row: len(leaves) trees, 2 * sum(leaves) -
    len(leaves) nodes.  Of the pairs of non-adjacent links the first `npairs` in group order stay checked; `acm` rows allow
    the others."""
    names = [f"n{i}" for i in range(len(leaves))]
    T = _Text(name, ["base_link"] + names + ["tool_link"])
    prev = "base_link"
    for i, n in enumerate(names):
        T.joint(f"j{i}", "revolute" if i < 3 else "fixed", prev, n, o=(0.04, 0.0, 0.02), r=(0.0, 0.0, 0.1) if i >= 3 else (0, 0, 0),
                a=(0, 0, 1), lo=-1.0 if i < 3 else 0.0, hi=1.0 if i < 3 else 0.0)
        for k in range(leaves[i]):
            T.sphere(n, f"{n}_{k}", 0.01 * k, 0.0, 0.0, 0.01)
        prev = n
    T.joint("tool", "fixed", prev, "tool_link", o=(0.02, 0.0, 0.0))
    pairs = [(a, b) for a in range(len(names)) for b in range(a + 2, len(names))]
    assert npairs <= len(pairs)
    return T.text(names, ["j0", "j1", "j2"], "tool_link", acm=[(names[a], names[b]) for a, b in pairs[npairs:]])


def three_branchings_robot() -> str:
    """a link with two children below a link with two children below a link with two children: a third saved transform"""
    T = _Text("branchy", ["base_link", "m", "a1", "a2", "b1", "b2", "c1", "c2", "tool_link"])
    T.joint("jm", "fixed", "base_link", "m", o=(0.0, 0.0, 0.5))
    for parent, kids in (("m", ("a1", "a2")), ("a1", ("b1", "b2")), ("b1", ("c1", "c2"))):
        for i, k in enumerate(kids):
            T.joint(f"j{k}", "revolute", parent, k, o=(0.1, 0.05 * (1 - 2 * i), 0.0), a=(0, 0, 1), lo=-1.0, hi=1.0)
    T.joint("tool", "fixed", "c1", "tool_link", o=(0.05, 0.0, 0.0))
    for k in ("a1", "a2", "b1", "b2", "c1", "c2"):
        T.sphere(k, f"{k}s", 0.05, 0.0, 0.0, 0.02)
    return T.text(["a1", "a2", "b1", "b2", "c1", "c2"], ["ja1", "jb1", "jc1"], "tool_link")


ROBOTS = {"deep": deep_robot, "deep40": lambda: deep_robot(12, 10, "deep40"), "crowd": crowd_robot, "order": order_robot}
LIMITS = {"deep": DEEP_LIMITS, "deep40": DEEP_LIMITS, "crowd": CROWD_LIMITS, "order": ORDER_LIMITS}
BOXES = {
    "deep": [((0.42, 0.10, 0.70), (0.12, 0.40, 0.30)), ((-0.30, -0.35, 0.55), (0.30, 0.12, 0.50)), ((0.0, 0.0, 0.30), (0.6, 0.6, 0.04))],
    "crowd": [((0.10, 0.10, 0.66), (0.10, 0.10, 0.10)), ((-0.32, 0.02, 0.55), (0.10, 0.30, 0.20)), ((0.0, 0.0, 0.36), (0.5, 0.5, 0.04))],
    "order": [((0.36, 0.0, 0.64), (0.08, 0.5, 0.3)), ((0.0, 0.42, 0.6), (0.4, 0.08, 0.3)), ((0.0, 0.0, 0.36), (0.5, 0.5, 0.04))],
}
BOXES["deep40"] = BOXES["deep"]
# bytes of traversal stack each robot's walks need (model_compile.cpp:503-513 rounds them up to a multiple of 8, at least 16)
STACK_NEED = {"deep": 64, "deep40": 40, "crowd": 4, "order": 6}


@functools.lru_cache(maxsize=None)
def case(name: str):
    """the robot `name` in a 48 x 40 x 32 grid of 4 cm cells with three boxes"""
    n = len(LIMITS[name])
    grid = scenes.build_grid(ORIGIN, DIMS, RES, CAP, BOXES[name])
    p = scenes.PlanningParams([2 * DEG] * n, eps0=5.0, bfs_radius=0.04, cost_per_cell=500)
    start = [0.5 * (lo + hi) for lo, hi in LIMITS[name]]
    if name in ("deep", "deep40"):
        start = [0.0, 0.8, 0.0]
    if name == "order":
        start = [0.8, 0.5, -0.8, -0.5]
    return scenes.Config(name, ROBOTS[name](), scenes.mprim_text(n, range(n), range(n), long_cells=4, short_cells=1), grid, p,
                         start, list(start), [3 * DEG] * n, BOXES[name])


# ----------------------------------------------------------------------------------------------------------------------
# the robot text, read once more (the probe's own reading: which link carries which tree, in which order the chain
# reaches them)
# ----------------------------------------------------------------------------------------------------------------------

def chain_order(robot_text):
    """(names of the links with spheres in group order = tree order, tree indices in depth-first order of the joints)"""
    links, children, group, with_spheres = [], {}, [], set()
    for line in robot_text.splitlines():
        w = line.split()
        if not w:
            continue
        if w[0] == "link":
            links.append(w[1])
        elif w[0] == "joint":
            children.setdefault(w[3], []).append(w[4])
        elif w[0] == "sphere":
            with_spheres.add(w[1])
        elif w[0] == "group":
            group = w[2:]
    trees = [g for g in group if g in with_spheres]
    order = []

    def visit(link):
        if link in trees:
            order.append(trees.index(link))
        for c in children.get(link, []):
            visit(c)
    visit(links[0])
    assert sorted(order) == list(range(len(trees)))
    return trees, order


# ----------------------------------------------------------------------------------------------------------------------
# the probe
# ----------------------------------------------------------------------------------------------------------------------

class PairWalk:
    """what one tree-against-tree walk held and read back"""
    __slots__ = ("hit", "stack", "popped", "hit_after_pop", "splits_at_hit")

    def __init__(self):
        self.hit = None             # (node a, node b) of the colliding leaves, or None
        self.stack = 0              # most bytes held at once: 2 x splits on the path
        self.popped = -1            # highest stack byte read back before the walk ended
        self.hit_after_pop = -1     # highest stack byte read back before the colliding leaf pair was reached
        self.splits_at_hit = 0


class Probe:
    """per-state instrumentation on top of an Oracle of the same configuration"""

    def __init__(self, cfg, oracle):
        self.o = oracle
        m = oracle.model()
        self.xyzr, self.first = m["xyzr"], m["tree_first"].tolist()
        self.nt = len(self.first) - 1
        self.left, self.right = m["left"].tolist(), m["right"].tolist()      # child indices within the tree: made global here
        for t in range(self.nt):
            for n in range(self.first[t], self.first[t + 1]):
                if self.left[n] >= 0:
                    self.left[n] += self.first[t]
                    self.right[n] += self.first[t]
        self.r = self.xyzr[:, 3].tolist()
        self.pairs = [tuple(int(v) for v in p) for p in m["pairs"]]
        self.nn = len(self.left)
        self.roots = [self.first[t + 1] - 1 for t in range(self.nt)]
        self.tree_links, self.chain = chain_order(cfg.robot_text)
        self.chain_pos = {t: i for i, t in enumerate(self.chain)}
        assert len(self.tree_links) == self.nt

    def depth(self, n):
        return 0 if self.left[n] < 0 else 1 + max(self.depth(self.left[n]), self.depth(self.right[n]))

    def stack_need(self):
        """model_compile.cpp:503-513 from the oracle's trees: one byte per level of a tree, two per split of a checked pair"""
        d = [self.depth(r) for r in self.roots]
        return max(d + [2 * (d[a] + d[b]) for a, b in self.pairs])

    # ---- sphere tree against the grid (collision_operations.h:105-164) ------------------------------------------------
    def _tree_clear(self, n, P, tally):
        tally[0] += 1
        r = self.r[n]
        if self.o.grid_sqdist(*P[n]) >= r * r:
            return True
        if self.left[n] < 0:
            return False
        a, b = self.left[n], self.right[n]
        if not self.r[a] > self.r[b]:       # the larger child first
            a, b = b, a
        return self._tree_clear(a, P, tally) and self._tree_clear(b, P, tally)

    # ---- sphere tree against sphere tree (self_collision_model.cpp:1093-1218) -----------------------------------------
    def _overlap(self, a, b, P):
        dx, dy, dz = P[b][0] - P[a][0], P[b][1] - P[a][1], P[b][2] - P[a][2]
        rr = self.r[a] + self.r[b]
        return not ((dx * dx + dy * dy) + dz * dz > rr * rr)

    def _pair(self, a, b, P, splits, w):
        """True: a leaf pair below (a, b) collides.  The first branch is walked at once, the second is what an explicit
        stack would hold at bytes 2 * splits and 2 * splits + 1 and read back afterwards."""
        if not self._overlap(a, b, P):
            return False
        la, lb = self.left[a] < 0, self.left[b] < 0
        if la and lb:
            w.hit = (a, b)
            w.hit_after_pop = w.popped
            w.splits_at_hit = splits
            return True
        split_a = (not la) and (lb or self.r[a] > self.r[b])
        w.stack = max(w.stack, 2 * (splits + 1))
        first, second = ((self.left[a], b), (self.right[a], b)) if split_a else ((a, self.left[b]), (a, self.right[b]))
        if self._pair(first[0], first[1], P, splits + 1, w):
            return True
        w.popped = max(w.popped, 2 * splits + 1)
        return self._pair(second[0], second[1], P, splits + 1, w)

    def walk_pair(self, ta, tb, P):
        w = PairWalk()
        self._pair(self.roots[ta], self.roots[tb], P, 0, w)
        return w

    def state(self, q):
        """dict of: valid, lookups (both as Oracle.state_valid in chain order gives them), voxel_clear, walks (one PairWalk
        per checked pair, group order), stack (largest over the pairs), queue (pairs whose roots overlap and are not both
        leaves), leaf_roots (pairs decided by their roots alone: both leaves, overlapping), first_pair (index of the first
        colliding pair in group order, or -1)"""
        P = self.o.sphere_positions(q, self.nn).tolist()
        tally = [0]
        clear = True
        for t in self.chain:
            if not self._tree_clear(self.roots[t], P, tally):
                clear = False
                break
        out = dict(valid=False, lookups=tally[0], voxel_clear=clear, walks=[], stack=0, queue=0, leaf_roots=0, first_pair=-1, P=P)
        if not clear:
            return out
        for k, (a, b) in enumerate(self.pairs):
            ra, rb = self.roots[a], self.roots[b]
            if self._overlap(ra, rb, P):
                if self.left[ra] < 0 and self.left[rb] < 0:
                    out["leaf_roots"] += 1
                else:
                    out["queue"] += 1
            w = self.walk_pair(a, b, P)
            out["walks"].append(w)
            out["stack"] = max(out["stack"], w.stack)
            if w.hit is not None and out["first_pair"] < 0:
                out["first_pair"] = k
        out["valid"] = out["first_pair"] < 0
        hits = [k for k, w in enumerate(out["walks"]) if w.hit is not None]
        # every colliding pair is one of two single-leaf trees: nothing but the root test of the chain can decide
        out["decided_by_leaf_roots"] = bool(hits) and all(self.left[self.roots[t]] < 0 for k in hits for t in self.pairs[k])
        out["first_pair_swapped"] = bool(hits) and self.pair_is_swapped(hits[0])
        out["early_pairs"] = self.kernel_pair_order()[:3]
        return out

    def pair_is_swapped(self, k):
        """the pair's group-earlier tree comes later in depth-first order: the kernels meet it with a_first == false"""
        a, b = self.pairs[k]
        return self.chain_pos[a] > self.chain_pos[b]

    def kernel_pair_order(self):
        """the pairs in the order of the kernels' pair_other table (model_compile.cpp:483-501): by the tree that comes
        later in depth-first order, trees in index order, each tree's partners in group order"""
        later = {t: [] for t in range(self.nt)}
        for k, (a, b) in enumerate(self.pairs):
            later[b if self.chain_pos[a] < self.chain_pos[b] else a].append(k)
        return [k for t in range(self.nt) for k in later[t]]


# ----------------------------------------------------------------------------------------------------------------------
# state sets: at most 512 states per robot, found by a seeded search
# ----------------------------------------------------------------------------------------------------------------------

SET_SIZE = 512


@functools.lru_cache(maxsize=None)
def oracle_and_probe(name):
    from oracle_binding import Oracle
    cfg = case(name)
    o = Oracle(cfg)
    o.set_order(chain=True)
    return o, Probe(cfg, o)


def stack_level(name):
    """the stack a full-depth walk holds: the need, or the last multiple of 2 at or below it"""
    return STACK_NEED[name] // 2 * 2


def _candidates(name, rng, n):
    lo = np.array([l for l, h in LIMITS[name]])
    hi = np.array([h for l, h in LIMITS[name]])
    Q = lo + rng.uniform(size=(n, len(lo))) * (hi - lo)
    if name in ("deep", "deep40"):
        # two thirds folded: jm within a few degrees of 0 puts the two dense ends within a few centimetres
        k = 2 * n // 3
        Q[:k, 1] = rng.uniform(-0.12, 0.12, size=k)
    return Q


def _classes(name, s):
    """the classes of section 3 a state belongs to (keys of QUOTA[name])"""
    out = []
    if name in ("deep", "deep40"):
        full = s["voxel_clear"] and s["stack"] == stack_level(name)
        if full:
            w = s["walks"][[i for i, x in enumerate(s["walks"]) if x.stack == s["stack"]][0]]
            out.append("full")
            if w.popped >= stack_level(name) - 1:
                out.append("full_top_read_back")
            if w.hit is not None and w.hit_after_pop >= stack_level(name) // 2:
                out.append("full_hit_after_upper_pop")
        elif s["voxel_clear"]:
            out.append("valid" if s["valid"] else "invalid")
        else:
            out.append("voxel")
    elif name == "crowd":
        if not s["voxel_clear"]:
            return ["voxel"]
        n = s["queue"]
        out.append("q0" if n == 0 else "q1_11" if n < PENDING_MAX else "q12" if n == PENDING_MAX else "q13" if n == 13 else "q14up")
        if n >= 13:
            out.append("over_valid" if s["valid"] else "over_invalid")
            if s["first_pair"] in s["early_pairs"]:
                out.append("over_invalid_early")
    else:
        if not s["voxel_clear"]:
            return ["voxel"]
        out.append("valid" if s["valid"] else "invalid")
        if s["decided_by_leaf_roots"]:
            out.append("leaf_roots_decide")
        if s["first_pair"] >= 0 and s["first_pair_swapped"]:
            out.append("swapped_pair_decides")
    return out


QUOTA = {
    "deep": dict(full=120, full_top_read_back=60, full_hit_after_upper_pop=60, valid=120, invalid=60, voxel=60),
    "crowd": dict(q0=50, q1_11=80, q12=50, q13=60, q14up=120, over_valid=60, over_invalid=80, over_invalid_early=30, voxel=40),
    "order": dict(valid=180, invalid=180, leaf_roots_decide=40, swapped_pair_decides=60, voxel=50),
}
QUOTA["deep40"] = QUOTA["deep"]


@functools.lru_cache(maxsize=None)
def state_set(name):
    """(Q [n <= 512][vars], the probe's dict per state): candidates in a seeded order, each kept while one of its classes
    is short of its quota"""
    o, probe = oracle_and_probe(name)
    rng = np.random.default_rng({"deep": 41, "deep40": 42, "crowd": 43, "order": 44}[name])
    have = {k: 0 for k in QUOTA[name]}
    Q, S = [], []
    for _ in range(40):
        for q in _candidates(name, rng, 1000):
            s = probe.state(q)
            cl = _classes(name, s)
            if any(have[c] < QUOTA[name][c] for c in cl):
                for c in cl:
                    have[c] += 1
                del s["P"]
                Q.append(q)
                S.append(s)
                if len(Q) == SET_SIZE:
                    break
        if len(Q) == SET_SIZE or all(have[c] >= QUOTA[name][c] for c in have):
            break
    Q = np.ascontiguousarray(np.array(Q))
    Q.setflags(write=False)
    return Q, S


def census(name):
    """class sizes of the state set, for the logs"""
    Q, S = state_set(name)
    out = {}
    for s in S:
        for c in _classes(name, s):
            out[c] = out.get(c, 0) + 1
    return out


# ----------------------------------------------------------------------------------------------------------------------
# expansion parents, goals, edges
# ----------------------------------------------------------------------------------------------------------------------

N_PARENTS = 96


def reaches_the_edge(name, s):
    """a configuration that drives the walks to the edge its robot is there for"""
    if not s["voxel_clear"]:
        return False
    if name in ("deep", "deep40"):
        return s["stack"] == stack_level(name)
    if name == "crowd":
        return s["queue"] > PENDING_MAX
    return s["decided_by_leaf_roots"] or (s["first_pair"] >= 0 and s["first_pair_swapped"])


@functools.lru_cache(maxsize=None)
def parents(name):
    """(goal, parents [N_PARENTS][vars]): valid states of the set; for the deep robots those whose walk goes deepest first (a
    step of jm away from a full-depth configuration), for crowd the overflowed ones first"""
    Q, S = state_set(name)
    valid = [i for i, s in enumerate(S) if s["valid"]]
    key = {"deep": lambda i: -S[i]["stack"], "deep40": lambda i: -S[i]["stack"], "crowd": lambda i: -S[i]["queue"],
           "order": lambda i: 0}[name]
    if name == "order":
        # ... for order those with the most colliding neighbours a long primitive (four cells of one joint) away
        o, probe = oracle_and_probe(name)
        near = {}
        for i in valid:
            n = 0
            for v in range(Q.shape[1]):
                for d in (-8 * DEG, 8 * DEG):
                    q = np.array(Q[i])
                    q[v] += d
                    n += reaches_the_edge(name, probe.state(q))
            near[i] = n
        key = lambda i: -near[i]
    valid.sort(key=key)                       # (stable: ties stay in the set's order)
    assert len(valid) > N_PARENTS
    return np.array(Q[valid[-1]]), np.ascontiguousarray(Q[valid[:N_PARENTS]])


@functools.lru_cache(maxsize=None)
def expansion_rows(name):
    """the oracle's GetSuccs loop body for every parent, and how many successor configurations reach the edge"""
    o, probe = oracle_and_probe(name)
    cfg = case(name)
    goal, P = parents(name)
    o.set_goal_joint(goal, cfg.goal_tol)
    rows = [o.eval_state(q) for q in P]
    exp = {k: np.stack([r[k] for r in rows]) for k in ("flags", "coord", "q", "h", "cost", "lookups")}
    edge = 0
    for r in rows:
        for p in range(o.M):
            if (r["flags"][p] & 0x30) == 0:          # an action within the joint limits
                edge += reaches_the_edge(name, probe.state(r["q"][p]))
    for a in exp.values():
        a.setflags(write=False)
    return exp, edge


@functools.lru_cache(maxsize=None)
def edges(name):
    """(A, B, oracle verdicts, oracle tallies, indices of the edges between two valid states that the oracle refuses, up to
    twelve of those with a waypoint that reaches the edge of the walks' scratch): state to state across the set, a valid
    state to another valid state, primitive-sized steps, and for the deep robots a valid state to its mirror image in jm --
    through the fold"""
    o, probe = oracle_and_probe(name)
    Q, S = state_set(name)
    valid = np.array([i for i, s in enumerate(S) if s["valid"]])
    rng = np.random.default_rng(7)
    step = rng.choice([-2, -1, 1, 2], size=(100, Q.shape[1])) * 2 * DEG
    step[50:] *= np.arange(Q.shape[1])[None, :] == (np.arange(50) % Q.shape[1])[:, None]          # the second half: one joint alone
    n = min(150, len(valid))
    A = [Q[:100], Q[valid[:n]], Q[valid[:100]]]
    B = [Q[100:200], Q[valid[(np.arange(n) * 7 + 3) % len(valid)]], Q[valid[:100]] + step]
    if name in ("deep", "deep40"):
        m = Q[valid[:100]].copy()
        m[:, 1] = -m[:, 1]
        A.append(Q[valid[:100]])
        B.append(m)
    A, B = np.ascontiguousarray(np.vstack(A)), np.ascontiguousarray(np.vstack(B))
    assert len(A) == len(B) <= SET_SIZE
    ok, lk = o.edge_valid_batch(A, B)
    ends_valid = np.array([o.state_valid(a)[0] and o.state_valid(b)[0] for a, b in zip(A, B)])
    inner = np.nonzero(ends_valid & (ok == 0))[0]
    show = []
    for i in inner:
        if any(reaches_the_edge(name, probe.state(q)) for q in waypoints(A[i], B[i], o.waypoint_count(A[i], B[i]))):
            show.append(int(i))
            if len(show) == 12:
                break
    for a in (A, B, ok, lk):
        a.setflags(write=False)
    return A, B, ok, lk, inner, np.array(show)


def waypoints(a, b, W):
    """the configurations an edge of revolute joints is checked at (robot_motion_collision_model.h:297-320): start +
    alpha * (finish - start), alpha = j * (1 / (W - 1))"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if W == 0:
        return a[None].copy()
    inv = 1.0 / float(W - 1)
    return np.stack([a if j == 0 else a + (float(j) * inv) * (b - a) for j in range(W)])
