"""A plain Python model of ManipLattice's lazy successor pair -- GetLazySuccs (manip_lattice.cpp:1012-1090) and
GetTrueCost (manip_lattice.cpp:1094-1167) -- composed from element functions of the CPU oracle (oracle_binding.Oracle):

  eval_state          the action set of a state: the joint values of every primitive's action and which primitives have
                      none there (the inactive bit);
  state_to_coord      stateToCoord;
  check_joint_limits, edge_valid    the two halves of checkAction (manip_lattice.cpp:1511-1580) for a one-waypoint action;
  planning_fk         the planning link's position, for the XYZ goal test;
  heuristic_q         the BFS cost of the planning link's cell.

The orientation test of a pose goal comes from pose_goal_ref.py.  The model keeps its own dictionary coordinate -> id and
calls nothing of the engine.  Test infrastructure: the judge of tests/test_gpu_lazy.py and tests/test_gpu_lazy_cpp.py, held
to the oracle proper by tests/test_lazy_ref.py.

Flags of a dense row, as smplx_lazy_expand_batch gives them: 0x10 where the primitive has no action at the state, else 4
("generated, unchecked"), plus 2 where isGoal holds for the action."""
from __future__ import annotations

import numpy as np

import pose_goal_ref

F_VALID, F_GOAL, F_UNCHECKED, F_INACTIVE, F_LIMITS, F_COLLISION = 1, 2, 4, 0x10, 0x20, 0x40
COST = 1000            # the three-argument cost() (manip_lattice.cpp:1388-1412) and int(1000 * 1) (:1156)
POSE_MARGIN = 1e-6     # as tests/test_gpu_pose_goal.py: theta this close to the tolerance is judged by rounding alone


class Goal:
    """kind 'joint' (angles, tol), 'xyz' (xyz, tol) or 'pose' (xyz, rpy, xyz_tol, rpy_tol); set_on hands it to an Oracle or
    a capi.Space (for the oracle a pose goal is its XYZ goal: gating and heuristic are the XYZ goal's)"""

    def __init__(self, kind, **kw):
        self.kind = kind
        self.__dict__.update(kw)

    @classmethod
    def joint(cls, angles, tol):
        return cls("joint", angles=list(angles), tol=list(tol))

    @classmethod
    def xyz(cls, xyz, tol):
        return cls("xyz", xyz=np.asarray(xyz, float), tol=np.asarray(tol, float))

    @classmethod
    def pose(cls, xyz, rpy, xyz_tol, rpy_tol):
        return cls("pose", xyz=np.asarray(xyz, float), rpy=np.asarray(rpy, float), tol=np.asarray(xyz_tol, float), rpy_tol=float(rpy_tol))

    def set_on(self, x, oracle=False):
        if self.kind == "joint":
            x.set_goal_joint(self.angles, self.tol)
        elif self.kind == "xyz" or oracle:
            x.set_goal_xyz(self.xyz, self.tol)
        else:
            x.set_goal_pose(self.xyz, self.rpy, self.tol, self.rpy_tol)


class LazyModel:
    """o: an Oracle of the case (the goal is set on it here); goal: a Goal"""

    def __init__(self, o, cfg, goal):
        self.o, self.cfg, self.goal = o, cfg, goal
        self.N, self.M = o.N, o.M
        goal.set_on(o, oracle=True)
        if goal.kind == "joint":
            self.goal_coord = o.state_to_coord(goal.angles)
        if goal.kind == "pose":
            self.chain, self.Rg = pose_goal_ref.Chain(cfg.robot_text), pose_goal_ref.rpy_matrix(goal.rpy)
        self.unsure = 0            # goal tests that fell within POSE_MARGIN of the orientation tolerance
        self._actions, self._checks = {}, {}
        # the lattice: id 0 is the goal (manip_lattice.cpp:122), which has no coordinate
        self.table, self.coords, self.qs, self.hs = {}, [None], [None], [None]
        # the goal id's heuristic: the BFS cost at the goal pose's cell, the seed of the BFS
        self.hs[0] = int(o.heuristic_q(goal.angles)) if goal.kind == "joint" else 0
        self.lazy_lists, self.eager_lists = {}, {}

    # ---- elements -------------------------------------------------------------------------------------------------
    def is_goal(self, q, coord):
        g = self.goal
        if g.kind == "joint":          # :1596-1606, on coordinates
            return all(abs(int(coord[v]) - int(self.goal_coord[v])) <= g.tol[v] for v in range(self.N))
        p = self.o.planning_fk(q)      # :1632-1637, :1682-1684
        if not all(abs(p[a] - g.xyz[a]) <= g.tol[a] for a in range(3)):
            return False
        if g.kind == "xyz":
            return True
        theta = pose_goal_ref.rotation_angle(self.Rg, self.chain.transform(q)[:3, :3])     # :1652-1667
        if abs(theta - g.rpy_tol) < POSE_MARGIN:
            self.unsure += 1
        return theta < g.rpy_tol

    def actions(self, q):
        """[(primitive, joint values, coordinate, isGoal)] of the actions at q, in primitive order (the action set GetSuccs sees)"""
        key = np.ascontiguousarray(q, np.float64).tobytes()
        if key not in self._actions:
            r = self.o.eval_state(q)
            out = []
            for p in range(self.M):
                if r["flags"][p] & F_INACTIVE:
                    continue
                sq = r["q"][p].copy()
                c = self.o.state_to_coord(sq)
                out.append((p, sq, tuple(int(x) for x in c), bool(self.is_goal(sq, c))))
            self._actions[key] = out
        return self._actions[key]

    def verdict(self, q, sq):
        """checkAction of the one-waypoint action q -> sq: 'ok', 'limits' or 'collision'"""
        key = np.ascontiguousarray(q, np.float64).tobytes() + np.ascontiguousarray(sq, np.float64).tobytes()
        if key not in self._checks:
            if not self.o.check_joint_limits(sq):
                self._checks[key] = "limits"
            else:
                self._checks[key] = "ok" if self.o.edge_valid(q, sq)[0] else "collision"
        return self._checks[key]

    # ---- the two calls on joint values -------------------------------------------------------------------------------
    def lazy_row(self, q):
        """dense row of GetLazySuccs' loop body: flags[M], coord[M, N], q[M, N], h[M]"""
        flags = np.full(self.M, F_INACTIVE, np.uint8)
        coord = np.zeros((self.M, self.N), np.int32); sq = np.zeros((self.M, self.N)); h = np.zeros(self.M, np.int32)
        for p, a, c, g in self.actions(q):
            flags[p] = F_UNCHECKED | (F_GOAL if g else 0)
            coord[p] = c; sq[p] = a; h[p] = self.o.heuristic_q(a)
        return dict(flags=flags, coord=coord, q=sq, h=h)

    def true_cost_q(self, q, coord=None):
        """GetTrueCost of the parent q and the child's coordinate (None: the goal edge): (cost, lowest matching primitive that
        passed or -1, matching actions)"""
        want = None if coord is None else tuple(int(x) for x in coord)
        cost, prim, nmatch = -1, -1, 0
        for p, a, c, g in self.actions(q):
            if (g if want is None else c == want):
                nmatch += 1
                if cost < 0 and self.verdict(q, a) == "ok":
                    cost, prim = COST, p
        return cost, prim, nmatch

    # ---- the lattice: ids in the caller's call order -------------------------------------------------------------------
    def num_states(self):
        return len(self.coords)

    def get_state(self, i):
        return self.qs[i], np.array(self.coords[i], np.int32)

    def _get_or_create(self, coord, q):
        if coord not in self.table:
            self.table[coord] = len(self.coords)
            self.coords.append(coord); self.qs.append(np.array(q, float)); self.hs.append(int(self.o.heuristic_q(q)))
        return self.table[coord]

    def set_start(self, q):
        return self._get_or_create(tuple(int(x) for x in self.o.state_to_coord(q)), q)

    def goal_heuristic(self, i):
        return self.hs[i]

    def get_lazy_succs(self, i):
        """(ids, costs): a state for every action, no test in front (:1054-1077)"""
        if i == 0:
            return [], []
        if i not in self.lazy_lists:
            self.lazy_lists[i] = [0 if g else sid for sid, g in
                                  [(self._get_or_create(c, a), g) for _, a, c, g in self.actions(self.qs[i])]]
        return list(self.lazy_lists[i]), [COST] * len(self.lazy_lists[i])

    def get_true_cost(self, parent, child):
        assert 0 < parent < len(self.coords) and 0 <= child < len(self.coords)
        return self.true_cost_q(self.qs[parent], None if child == 0 else self.coords[child])[0]

    def get_succs(self, i):
        """eager GetSuccs on the same lattice (manip_lattice.cpp:219-313): states only for the actions that pass"""
        if i == 0:
            return [], []
        if i not in self.eager_lists:
            r = self.o.eval_state(self.qs[i])
            ids, costs = [], []
            for p in range(self.M):
                if r["flags"][p] & F_VALID:
                    sid = self._get_or_create(tuple(int(x) for x in r["coord"][p]), r["q"][p])
                    ids.append(0 if r["flags"][p] & F_GOAL else sid); costs.append(int(r["cost"][p]))
            self.eager_lists[i] = (ids, costs)
        return list(self.eager_lists[i][0]), list(self.eager_lists[i][1])


def lazy_search(space, start_id, eps, max_expansions=1500):
    """The lazy weighted A* of tests/cpp/lazy_loop_driver.cpp, line for line, over anything with get_lazy_succs,
    get_true_cost and goal_heuristic.  OPEN is keyed by (f, insertion number).  A state is pushed once per (parent, cost)
    candidate; a popped candidate whose edge is unevaluated gets its true cost and goes back with it, or is dropped.
    Returns the lines the driver prints."""
    import heapq
    open_, counter = [], 0
    g, bp, closed, h = {start_id: 0}, {start_id: -1}, set(), {}

    def heur(i):
        if i not in h:
            h[i] = space.goal_heuristic(i)
        return h[i]
    heapq.heappush(open_, (int(eps * heur(start_id)), counter, start_id, -1, 0, True))
    expanded, evaluated, found = [], [], False
    while open_ and len(expanded) < max_expansions:
        f, _, sid, parent, gval, true_cost = heapq.heappop(open_)
        if sid in closed:
            continue
        if not true_cost:
            c = space.get_true_cost(parent, sid)
            evaluated.append((parent, sid, c))
            if c < 0:
                continue
            counter += 1
            gnew = g[parent] + c           # (the parent was closed when it generated this candidate)
            heapq.heappush(open_, (gnew + int(eps * heur(sid)), counter, sid, parent, gnew, True))
            continue
        closed.add(sid); g[sid] = gval; bp[sid] = parent
        if sid == 0:
            found = True
            break
        expanded.append(sid)
        ids, costs = space.get_lazy_succs(sid)
        for t, c in zip(ids, costs):
            if t in closed:
                continue
            counter += 1
            heapq.heappush(open_, (gval + c + int(eps * heur(t)), counter, t, sid, gval + c, False))
    lines = ["expanded " + " ".join(str(x) for x in expanded),
             "evaluated " + " ".join(f"{a}>{b}:{c}" for a, b, c in evaluated)]
    if found:
        path, s = [], 0
        while s >= 0:
            path.append(s); s = bp[s]
        lines.append("path " + " ".join(str(x) for x in reversed(path)))
        lines.append(f"cost {g[0]}")
    else:
        lines.append("path")
        lines.append("cost -1")
    return lines
