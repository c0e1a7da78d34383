"""Plain numpy model of the clearance queries (smplx_cc_state_clearance_batch; include/smpl_amd.h).

Brute force over sphere positions the caller supplies (the engine's own, from sphere_positions / attached_positions, or the
oracle's): every leaf against the grid, every leaf pair of every checked tree pair, every body leaf against the leaves of
the robot trees and of the later bodies it is checked against.  No pruning, no tree traversal.  The arithmetic is written in
the order the specification states, one rounding per operation, so the engine's answers must equal these bit for bit:

    world term   res * sqrt((double)d2) - (r + pad)          d2: the cell of the position, 0 outside the grid
    pair term    sqrt((dx*dx + dy*dy) + dz*dz) - (ra + rb)    d = pb - pa

Kinds of a witness {kind, a, b, waypoint}: 0 robot leaf / world, 1 robot leaf / robot leaf, 2 body leaf / world, 3 body
leaf / robot leaf, 4 body leaf / body leaf, -1 no term.
"""
import numpy as np

from smpl_amd import scenes

INF = np.inf


def bits(x):
    """float64 array as int64: equality of these is equality of every bit, infinities included"""
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def tree_links(robot_text, ntrees):
    """the link of each sphere tree, in tree order (group order of the links with spheres)"""
    group = [l for l in robot_text.splitlines() if l.startswith("group")][0].split()[2:]
    with_spheres = {l.split()[1] for l in robot_text.splitlines() if l.startswith("sphere")}
    links = [g for g in group if g in with_spheres]
    assert len(links) == ntrees
    return links


class ClearanceModel:
    """arrays: capi.Model(robot_text).arrays(); d2, origin, res: the grid (Grid.d2(), its origin and resolution);
    bodies / body_nodes: Space.attached_bodies() / Space.attached_nodes() (None without bodies); body_allowed_links[k]:
    the names body k was attached with (links and body ids)"""

    def __init__(self, robot_text, arrays, d2, origin, res, padding=0.0, bodies=None, body_nodes=None, body_allowed=None):
        self.xyzr, self.left, self.first = arrays["xyzr"], arrays["left"], arrays["tree_first"]
        self.pairs = [tuple(int(v) for v in p) for p in arrays["pairs"]]
        self.ntrees = len(self.first) - 1
        self.tree_of = np.zeros(len(self.left), int)
        for t in range(self.ntrees):
            self.tree_of[self.first[t]:self.first[t + 1]] = t
        self.leaves = [np.array([i for i in range(self.first[t], self.first[t + 1]) if self.left[i] < 0], int)
                       for t in range(self.ntrees)]
        self.d2 = np.asarray(d2)
        self.org, self.res, self.dims, self.pad = np.array(origin, float), float(res), np.array(self.d2.shape), float(padding)
        self.bodies = bodies or []
        if self.bodies:
            self.bxyzr, self.bleft, _ = body_nodes
            self.body_of = np.zeros(len(self.bleft), int)
            self.bleaves = []
            for k, bd in enumerate(self.bodies):
                self.body_of[bd["first"]:bd["first"] + bd["count"]] = k
                self.bleaves.append(np.array([i for i in range(bd["first"], bd["first"] + bd["count"]) if self.bleft[i] < 0], int))
            links = tree_links(robot_text, self.ntrees)
            ids = [bd["id"] for bd in self.bodies]
            self.allow_trees = [{links.index(x) for x in body_allowed[k] if x in links} for k in range(len(ids))]
            self.allow_bodies = set()
            for k in range(len(ids)):
                for x in body_allowed[k]:
                    if x in ids and ids.index(x) != k:
                        self.allow_bodies |= {(k, ids.index(x)), (ids.index(x), k)}

    # ---- the two terms -----------------------------------------------------------------------------------------------
    def world_term(self, p, r):
        c = scenes.world_to_grid(self.org, self.res, p)                 # distance_map.hpp:520-527
        inside = np.all((c >= 0) & (c < self.dims), axis=-1)
        cc = np.clip(c, 0, self.dims - 1)
        d2 = np.where(inside, self.d2[cc[..., 0], cc[..., 1], cc[..., 2]], 0)
        return self.res * np.sqrt(d2.astype(np.float64)) - (r + self.pad)

    @staticmethod
    def pair_term(pa, ra, pb, rb):
        d = pb - pa
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz) - (ra + rb)

    # ---- all terms of n configurations ----------------------------------------------------------------------------------
    def evaluate(self, P, B=None):
        """P: [n][robot nodes][3]; B: [n][body nodes][3].  Returns (clearance[n], parts[n, 2])."""
        n = P.shape[0]
        world = np.full(n, INF)
        selfd = np.full(n, INF)
        for t in range(self.ntrees):
            lt = self.leaves[t]
            world = np.minimum(world, self.world_term(P[:, lt], self.xyzr[lt, 3]).min(1))
        for a, b in self.pairs:
            la, lb = self.leaves[a], self.leaves[b]
            v = self.pair_term(P[:, la, None], self.xyzr[la, 3][:, None], P[:, None, lb], self.xyzr[lb, 3][None, :])
            selfd = np.minimum(selfd, v.min((1, 2)))
        for k in range(len(self.bodies)):
            lk = self.bleaves[k]
            world = np.minimum(world, self.world_term(B[:, lk], self.bxyzr[lk, 3]).min(1))
            for t in range(self.ntrees):
                if t in self.allow_trees[k]:
                    continue
                lt = self.leaves[t]
                v = self.pair_term(B[:, lk, None], self.bxyzr[lk, 3][:, None], P[:, None, lt], self.xyzr[lt, 3][None, :])
                selfd = np.minimum(selfd, v.min((1, 2)))
            for o in range(k + 1, len(self.bodies)):
                if (k, o) in self.allow_bodies:
                    continue
                lo = self.bleaves[o]
                v = self.pair_term(B[:, lk, None], self.bxyzr[lk, 3][:, None], B[:, None, lo], self.bxyzr[lo, 3][None, :])
                selfd = np.minimum(selfd, v.min((1, 2)))
        return np.minimum(world, selfd), np.stack([world, selfd], 1)

    # ---- the term a witness names ---------------------------------------------------------------------------------------
    def witness_term(self, P, B, witness):
        """the value of the term each row's witness names, recomputed from the positions; asserts that the witness names
        a term that exists (leaves, a checked pair in its order, a body against something it is checked against)"""
        out = np.full(P.shape[0], INF)
        kind, a, b = witness[:, 0], witness[:, 1], witness[:, 2]
        assert ((kind >= -1) & (kind <= 4)).all()
        rows = np.arange(P.shape[0])
        for k in range(5):
            r = rows[kind == k]
            if len(r) == 0:
                continue
            ia, ib = a[r], b[r]
            if k in (0, 1):
                assert (self.left[ia] < 0).all()
            if k in (2, 3, 4):
                assert (self.bleft[ia] < 0).all()
            if k in (0, 2):
                assert (ib == -1).all()
                src, rad = (P, self.xyzr) if k == 0 else (B, self.bxyzr)
                out[r] = self.world_term(src[r, ia], rad[ia, 3])
                continue
            if k == 1:
                assert (self.left[ib] < 0).all()
                assert all((int(x), int(y)) in self.pairs for x, y in zip(self.tree_of[ia], self.tree_of[ib]))
                out[r] = self.pair_term(P[r, ia], self.xyzr[ia, 3], P[r, ib], self.xyzr[ib, 3])
            elif k == 3:
                assert (self.left[ib] < 0).all()
                assert all(int(t) not in self.allow_trees[int(bd)] for bd, t in zip(self.body_of[ia], self.tree_of[ib]))
                out[r] = self.pair_term(B[r, ia], self.bxyzr[ia, 3], P[r, ib], self.xyzr[ib, 3])
            else:
                assert (self.bleft[ib] < 0).all()
                assert all(int(x) < int(y) and (int(x), int(y)) not in self.allow_bodies
                           for x, y in zip(self.body_of[ia], self.body_of[ib]))
                out[r] = self.pair_term(B[r, ia], self.bxyzr[ia, 3], B[r, ib], self.bxyzr[ib, 3])
        return out


def check_against_model(model, P, B, clearance, parts, witness):
    """the assertions of the brute-force tests: values, the minimum, the witness"""
    exp_c, exp_p = model.evaluate(P, B)
    assert np.array_equal(bits(parts[:, 0]), bits(exp_p[:, 0])), "world part"
    assert np.array_equal(bits(parts[:, 1]), bits(exp_p[:, 1])), "self part"
    assert np.array_equal(bits(clearance), bits(exp_c))
    assert np.array_equal(bits(clearance), bits(np.minimum(parts[:, 0], parts[:, 1])))
    wt = model.witness_term(P, B, witness)
    assert np.array_equal(bits(wt), bits(clearance)), "the witness's own term is the clearance"
    kind = witness[:, 0]
    world_smaller, self_smaller = parts[:, 0] < parts[:, 1], parts[:, 1] < parts[:, 0]
    assert np.isin(kind[world_smaller], (0, 2)).all() and np.isin(kind[self_smaller], (1, 3, 4)).all()
    assert ((kind == -1) == np.isinf(clearance)).all()
    return exp_c, exp_p
