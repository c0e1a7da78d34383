"""A plain Python restatement of the ARA* loop (smpl/src/search/arastar.cpp:107-214, 486-568) with the reference's heap sift
rules (smpl/include/smpl/detail/intrusive_heap.hpp:346-395).  It knows two things of its environment, handed in as
callables: get_succs(id) -> (successor ids, costs) and goal_heuristic(id) -> h -- smplx_get_succs and
smplx_get_goal_heuristic of a space, or the oracle's successors with a heuristic worked out in numpy.  Nothing here calls
the engine's own searches: it is what they are compared with (tests/test_gpu_heuristic_kinds.py)."""
import math

INF = 1000000000      # SBPL INFINITECOST


class _Node:
    __slots__ = ("g", "h", "f", "eg", "closed", "call", "bp", "heap_index", "incons")

    def __init__(self):
        self.g = INF; self.h = 0; self.f = INF; self.eg = INF
        self.closed = 0; self.call = 0; self.bp = -1; self.heap_index = 0; self.incons = False


class AraStarLoop:
    def __init__(self, get_succs, goal_heuristic):
        self.get_succs, self.goal_heuristic = get_succs, goal_heuristic
        self.n = {}
        self.heap = [0]          # entry 0 unused, as in the reference's heap
        self.incons = []
        self.log = []
        self.call = 0

    # ---- intrusive_heap.hpp: percolate down / up with a hole, strict comparisons
    def _less(self, a, b):
        return self.n[a].f < self.n[b].f

    def _down(self, pivot):
        heap, n = self.heap, self.n
        if pivot >= len(heap):
            return
        left, right = pivot << 1, (pivot << 1) + 1
        tmp = heap[pivot]
        while left < len(heap):
            c = right
            if right >= len(heap) or self._less(heap[left], heap[right]):
                c = left
            if not self._less(heap[c], tmp):
                break
            heap[pivot] = heap[c]
            n[heap[pivot]].heap_index = pivot
            pivot = c
            left, right = pivot << 1, (pivot << 1) + 1
        heap[pivot] = tmp
        n[tmp].heap_index = pivot

    def _up(self, pivot):
        heap, n = self.heap, self.n
        tmp = heap[pivot]
        while pivot != 1:
            p = pivot >> 1
            if self._less(heap[p], tmp):
                break
            heap[pivot] = heap[p]
            n[heap[pivot]].heap_index = pivot
            pivot = p
        heap[pivot] = tmp
        n[tmp].heap_index = pivot

    def _push(self, e):
        self.n[e].heap_index = len(self.heap)
        self.heap.append(e)
        self._up(len(self.heap) - 1)

    def _pop(self):
        heap = self.heap
        self.n[heap[1]].heap_index = 0
        last = heap.pop()
        if len(heap) > 1:
            heap[1] = last
            self._down(1)

    def _key(self, s):
        return s.g + int(self.eps * s.h)

    def _reinit(self, i):
        s = self.n.get(i)
        if s is None:
            s = self.n[i] = _Node()
        if s.call != self.call:
            s.g = INF
            s.h = int(self.goal_heuristic(i))        # the only heuristic access
            s.f = INF; s.eg = INF; s.closed = 0; s.call = self.call; s.bp = -1; s.incons = False
        return s

    def replan(self, start, goal, eps0, eps_final, eps_delta, max_init=0, max_rep=0, allow_partial=False, resume=False):
        """dict(solved, cost, expansions, satisfied_eps, path, log, result, call_expansions): a bounded search when
        max_init > 0 (expansion budgets of the first and of the later iterations, TimeParameters::EXPANSIONS).  result is the
        ReplanResultCode the call's last improvePath ended with (0 SUCCESS, 4 TIMED_OUT, 5 EXHAUSTED_OPEN_LIST; 0 when the
        call had nothing to improve).  allow_partial: a search without a solution returns the bp chain of OPEN's minimum,
        where OPEN has one (arastar.cpp:204-209), with solved = 1 and satisfied_eps = inf.  resume: the call continues the
        search of the call before it (the same start: arastar.cpp:128 is not taken) -- OPEN, INCONS, epsilons and log stay,
        the call's own expansion count starts at 0 and `expansions` goes on counting"""
        if not resume:
            for i in self.heap[1:]:              # intrusive_heap.hpp clear(): what an earlier call left in OPEN is out of it
                self.n[i].heap_index = 0
            self.heap = [0]; self.incons = []; self.log = []
            self.call += 1
            self.eps = eps0
            self._reinit(start); self._reinit(goal)
            s = self.n[start]
            s.g = 0
            s.f = self._key(s)
            self._push(start)
            self.iteration, self.satisfied, self.total = 1, math.inf, 0
        iteration, num, satisfied = self.iteration, 0, self.satisfied
        fin = max(eps_final, 1.0)
        err = 0
        while satisfied > fin:
            if self.eps == satisfied:
                iteration += 1
                self.eps = max(self.eps - eps_delta, fin)
                for i in self.incons:
                    self.n[i].incons = False
                    self._push(i)
                for i in self.heap[1:]:
                    self.n[i].f = self._key(self.n[i])
                for i in range((len(self.heap) - 1) >> 1, 0, -1):
                    self._down(i)
                self.incons = []
            err, num = self._improve(goal, iteration, num, satisfied, max_init, max_rep)
            if err:
                break
            satisfied = self.eps
        self.iteration, self.satisfied = iteration, satisfied
        self.total += num
        out = dict(solved=int(satisfied != math.inf), cost=0, expansions=self.total, satisfied_eps=satisfied, path=[],
                   log=list(self.log), result=err, call_expansions=num)
        last = goal if out["solved"] else self.heap[1] if allow_partial and len(self.heap) > 1 else -1
        if last >= 0:
            i = last
            while i >= 0:
                out["path"].insert(0, i)
                i = self.n[i].bp
            out["cost"] = self.n[last].g
            out["solved"] = 1
        return out

    def _improve(self, goal, iteration, elapsed, satisfied, max_init, max_rep):
        n = self.n
        while len(self.heap) > 1:
            m = self.heap[1]
            if n[m].f >= n[goal].f or m == goal:
                return 0, elapsed
            if max_init > 0 and elapsed >= (max_init if satisfied == math.inf else max_rep):
                return 4, elapsed
            self._pop()
            n[m].closed = iteration
            n[m].eg = n[m].g
            self.log.append(m)
            succs, costs = self.get_succs(m)             # the only successor access
            eg = n[m].eg
            for nid, c in zip(succs, costs):
                nid = int(nid)
                t = self._reinit(nid)
                new_cost = eg + int(c)
                if new_cost < t.g:
                    t.g = new_cost
                    t.bp = m
                    if t.closed != iteration:
                        t.f = self._key(t)
                        if t.heap_index != 0:
                            self._up(t.heap_index)
                        else:
                            self._push(nid)
                    elif not t.incons:
                        # arastar.cpp:563-564 never raises the flag it tests: INCONS holds a state once per improvement,
                        # and such a state enters OPEN as often at the next reordering.  Restated as it is
                        self.incons.append(nid)
            elapsed += 1
        return 5, elapsed
