"""Which rare branches of the device search (smpl_amd/csrc/search_kernel.h) a search takes, counted on the CPU from the
oracle alone: its expansion log, the successor lists of the expanded states and the coordinates of its states.

  * two successors of one expansion that name one state: k_search then leaves the per-lane relaxation for the general
    one, which walks the successors in primitive order.  By kind: both are goal successors (id 0); the state was created
    by this very expansion (on the device: a same-coordinate pair among the new states, the lower primitive creates);
    the state is older (two probes that find the same slot);
  * two new states of one expansion whose probes of the state table end at the same empty slot: the later one probes
    again, alone, behind what the others have stored.  This needs a model of the table: open addressing with linear
    probing from smplx_coord_hash & (slots - 1), filled in id order (the goal's entry, id 0, has no coordinate and no
    slot).  Which slots are occupied does not depend on the order of insertion, so the model holds for as long as the
    device keeps the table it allocated first.

Only the first expansion of a state counts: a later ARA* iteration takes its successors from the committed list.
Ids are handed out in creation order, so the states an expansion created are the ids from the first unused one on."""
from __future__ import annotations

import numpy as np

MAX_STATES = 20000


def coord_hash(c):
    """smplx_coord_hash (csrc/device_types.h) of every row of c"""
    c = np.ascontiguousarray(c, np.int32)
    c = c.reshape(-1, c.shape[-1])
    m = np.uint64(0xFFFFFFFF)
    h = np.full(c.shape[0], 2166136261, np.uint64)
    for v in range(c.shape[1]):
        h = ((h ^ c[:, v].astype(np.uint32).astype(np.uint64)) * np.uint64(16777619)) & m
    h ^= h >> np.uint64(15); h = (h * np.uint64(0x85EBCA6B)) & m
    h ^= h >> np.uint64(13); h = (h * np.uint64(0xC2B2AE35)) & m
    h ^= h >> np.uint64(16)
    return h


class TableModel:
    """the occupied slots of a state table of `slots` slots (a power of two)"""

    def __init__(self, slots):
        assert slots >= 64 and slots & (slots - 1) == 0
        self.mask = slots - 1
        self.used = np.zeros(slots, bool)
        self.count = 0

    def probe_end(self, h):
        """the empty slot at which the probe for a coordinate of hash h, which the table does not hold, ends"""
        k = int(h) & self.mask
        while self.used[k]:
            k = (k + 1) & self.mask
        return k

    def insert(self, h):
        assert 2 * (self.count + 1) <= self.mask + 1, "the device would have enlarged this table"
        self.used[self.probe_end(h)] = True
        self.count += 1


def count_pairs(keys):
    """unordered pairs of equal entries"""
    _, n = np.unique(np.asarray(keys), return_counts=True)
    return int((n * (n - 1) // 2).sum())


def branch_events(log, succs_of, coords, first_new_id, table_slots=0):
    """log: the expansion log; succs_of(id): the successor ids of a state, in primitive order; coords: the coordinate of
    every state, a row per id; first_new_id: the number of states before the search began (the goal's entry, the start).
    table_slots: slots of the table model, 0 for none.  Returns the number of first expansions
      two_goal   whose list holds id 0 at least twice,
      alias_new  whose list holds twice a state the expansion created,
      alias_old  whose list holds twice an older state (not id 0),
      clash      that created two states whose probes end at the same empty slot
    and `clash_pairs`, `expansions` (first ones), `states` (after the last one), `states_before_last` and `unlisted`: the
    states no list names.  A goal successor is listed as id 0 whatever state its coordinate has, so the state made for it
    shows in no list; which of two neighbouring expansions with goal successors made it is then a guess (the earlier one),
    and a caller that relies on the table model asserts that `unlisted` is 0."""
    coords = np.asarray(coords)
    assert len(coords) <= MAX_STATES
    out = dict(two_goal=0, alias_new=0, alias_old=0, clash=0, clash_pairs=0, expansions=0, states=first_new_id,
               states_before_last=first_new_id, unlisted=0)
    table = None
    if table_slots:
        table = TableModel(table_slots)
        for h in coord_hash(coords[1:first_new_id]):
            table.insert(h)
    firsts, seen = [], {0}
    for sid in (int(x) for x in log):
        if sid not in seen:
            seen.add(sid)
            firsts.append((sid, np.asarray(succs_of(sid), np.int64)))
    listed = np.zeros(len(coords) + 1, bool)
    for _, ids in firsts:
        listed[ids] = True
    known = first_new_id
    for sid, ids in firsts:
        out["expansions"] += 1
        out["states_before_last"] = known
        uniq, n = np.unique(ids, return_counts=True)
        twice = uniq[n >= 2]
        out["two_goal"] += int(np.any(twice == 0))
        out["alias_new"] += int(np.any(twice >= known))
        out["alias_old"] += int(np.any((twice > 0) & (twice < known)))
        # the states this expansion created: the listed ids from `known` on and, where it has a goal successor, the
        # unlisted ids between and behind them
        goal_succ = bool(np.any(uniq == 0))
        hi = known
        while hi < len(coords) and (hi in uniq or (goal_succ and not listed[hi])):
            hi += 1
        assert np.all(uniq < hi)
        out["unlisted"] += int(np.sum(~listed[known:hi]))
        if table is not None and hi > known:
            hs = coord_hash(coords[known:hi])
            pairs = count_pairs([table.probe_end(h) for h in hs])
            out["clash_pairs"] += pairs
            out["clash"] += int(pairs > 0)
            for h in hs:
                table.insert(h)
        known = hi
    out["states"] = known
    return out


def oracle_events(o, eo, first_new_id, table_slots=0):
    """branch_events of a search the oracle `o` has just run (eo = o.plan())"""
    n = o.num_states()
    assert n <= MAX_STATES
    coords = np.zeros((n, o.N), np.int32)
    for i in range(1, n):
        coords[i] = o.get_state(i)[1]
    ev = branch_events(eo["expansion_log"], lambda i: o.get_succs(i)[0], coords, first_new_id, table_slots)
    assert o.num_states() == n == ev["states"]        # (asking for the successors of an expanded state creates nothing)
    return ev


# ----------------------------------------------------------------------------------------------------------------------
# the searches of tests/test_gpu_device_search.py that are there for one of these branches: what the oracle makes of each
# ----------------------------------------------------------------------------------------------------------------------

# config_small with a joint goal whose tolerance is 30 cells in five variables and the whole circle in the two whose
# coordinates wrap between start and goal (the goal test compares cells, not angles): states with several primitives
# inside the goal before the search is over, and epsilon steps down to 1
GOAL_PAIR_TOL = [30.5, 30.5, 30.5, 30.5, 400.0, 30.5, 400.0]
GOAL_PAIR_BOUNDS = (6000, 3000)
# the two-joint chain of width_cases.py with the short row of variable 1 listed twice: both copies of a primitive land in
# one cell, of a new state or of a known one
TWIN_ROWS = ((), (0, 1, 1), True)
TWIN_BOUNDS = (300, 300)
# config_small stopped after 110 expansions: about a thousand states, which a table of 2048 slots holds half full
CLASH_BOUNDS = (110, 110)
EPS = (5.0, 1.0, 1.0)


def case_config(name):
    from smpl_amd import scenes
    import width_cases as wc
    return wc.width_case(2, TWIN_ROWS) if name == "twin_rows" else scenes.config_small()


def case_goal_tol(name, cfg):
    return GOAL_PAIR_TOL if name == "goal_pair" else cfg.goal_tol


def case_bounds(name):
    return {"goal_pair": GOAL_PAIR_BOUNDS, "twin_rows": TWIN_BOUNDS, "clash": CLASH_BOUNDS}[name]


def clash_capacity(ev, nprims):
    """the least first capacity (smplx_test_set_search_capacity) with which the device search of ev never stops for room:
    k_search asks for room for one more expansion before each pop, and the log holds max(64, capacity / 8) expansions"""
    cap = ev["states_before_last"] + nprims
    assert ev["expansions"] + 1 <= max(64, cap // 8)
    return cap


_cache = {}


def case_truth(name):
    """(oracle, its set_start id, its plan(), branch events) of a case, computed once; the clash case with the table model
    of the size width_cases.first_table_slots gives for clash_capacity"""
    if name not in _cache:
        from oracle_binding import Oracle
        import width_cases as wc
        cfg = case_config(name)
        o = Oracle(cfg)
        o.set_goal_joint(cfg.goal, case_goal_tol(name, cfg))
        sid = o.set_start(cfg.start)
        first = o.num_states()
        o.search_params(*EPS, True, True, *case_bounds(name))
        eo = o.plan()
        ev = oracle_events(o, eo, first)
        if name == "clash":
            slots = wc.first_table_slots(o.M, clash_capacity(ev, o.M))
            ev = dict(oracle_events(o, eo, first, slots), table_slots=slots)
        _cache[name] = (o, sid, eo, ev)
    return _cache[name]
