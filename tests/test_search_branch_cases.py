"""tests/search_branch_cases.py, without a GPU: the counting on logs written by hand, the table model against a plain
dict-free restatement, and that each search tests/test_gpu_device_search.py runs for a rare branch of k_search takes that
branch in the oracle."""
import numpy as np
import pytest

import search_branch_cases as sb
import width_cases as wc


def test_coord_hash_is_the_c_hash():
    """smplx_coord_hash restated with Python integers"""
    def plain(c):
        h = 2166136261
        for x in c:
            h = ((h ^ (x & 0xFFFFFFFF)) * 16777619) & 0xFFFFFFFF
        h ^= h >> 15; h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13; h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        return h ^ (h >> 16)
    rng = np.random.default_rng(1)
    for nv in (1, 2, 7, 16):
        c = rng.integers(-400, 400, size=(50, nv)).astype(np.int32)
        assert sb.coord_hash(c).tolist() == [plain([int(x) for x in row]) for row in c]


def test_table_model_probes_linearly_and_wraps():
    t = sb.TableModel(64)
    for h in (5, 5 + 64, 6, 63, 63 + 128):
        t.insert(h)
    assert np.nonzero(t.used)[0].tolist() == [0, 5, 6, 7, 63]      # 5, 5 -> 6, 6 -> 7, 63, 63 -> 0
    assert t.probe_end(5) == 8 and t.probe_end(62) == 62 and t.probe_end(63 + 64) == 1 and t.count == 5
    # the occupied slots do not depend on the order of insertion
    u = sb.TableModel(64)
    for h in (63 + 128, 6, 5 + 64, 63, 5):
        u.insert(h)
    assert np.array_equal(t.used, u.used)
    for h in range(27):
        t.insert(1000 + h)
    with pytest.raises(AssertionError):
        t.insert(7)                       # the 33rd state of a table of 64 slots


def _coords_with_ends(table_slots, ends, nv=2, seed=0):
    """distinct coordinates whose home slots in an empty table of table_slots slots are `ends`"""
    rng = np.random.default_rng(seed)
    out, used = [], set()
    for e in ends:
        while True:
            c = tuple(int(x) for x in rng.integers(0, 1000, size=nv))
            if c not in used and int(sb.coord_hash(np.array([c]))[0]) & (table_slots - 1) == e:
                used.add(c); out.append(c)
                break
    return out


def test_branch_events_on_a_log_written_by_hand():
    """ids 0 (goal) and 1 (start) exist; four first expansions and one repeated one"""
    succ = {1: [2, 3, 3, 4],          # creates 2 3 4; 3 twice: a pair among the new states
            2: [1, 5, 1, 0],          # creates 5 and 6 (6: the goal successor's state, listed as 0); 1 twice: an older state
            3: [0, 7, 0],             # creates 7; two goal successors, of known states
            5: [8, 9]}                # creates 8 9, whose home slot is the same
    coords = np.zeros((10, 2), np.int32)
    coords[1:8] = _coords_with_ends(64, [1, 10, 20, 30, 40, 41, 50])
    coords[8:10] = _coords_with_ends(64, [40, 40], seed=1)        # both probes walk 40 -> 41 -> 42
    ev = sb.branch_events([1, 2, 3, 5, 2], succ.__getitem__, coords, 2, table_slots=64)
    assert ev == dict(two_goal=1, alias_new=1, alias_old=1, clash=1, clash_pairs=1, expansions=4, states=10,
                      states_before_last=8, unlisted=1)
    # without the last expansion nothing clashes; without a table nothing is probed
    assert sb.branch_events([1, 2, 3], succ.__getitem__, coords[:8], 2, table_slots=64)["clash"] == 0
    assert sb.branch_events([1, 2, 3, 5], succ.__getitem__, coords, 2)["clash_pairs"] == 0


def test_each_case_takes_its_branch_in_the_oracle():
    """what the GPU cases assert before they compare the device search with the oracle's, here for the oracle alone"""
    _, _, eo, ev = sb.case_truth("goal_pair")
    print("goal_pair", eo["expansions"], eo["eps"], ev)
    assert ev["two_goal"] >= 1 and eo["ok"] == 1 and eo["eps"] == 1.0
    _, _, eo, ev = sb.case_truth("twin_rows")
    print("twin_rows", eo["expansions"], ev)
    assert ev["alias_new"] >= 1 and ev["alias_old"] >= 1 and eo["expansions"] == sb.TWIN_BOUNDS[0]
    o, _, eo, ev = sb.case_truth("clash")
    print("clash", eo["expansions"], ev)
    assert ev["clash"] >= 1 and ev["unlisted"] == 0 and eo["expansions"] == sb.CLASH_BOUNDS[0]
    assert ev["two_goal"] == ev["alias_new"] == ev["alias_old"] == 0
    # the table is the smallest the device search can have: half as many slots would be more than half full
    assert ev["table_slots"] == wc.first_table_slots(o.M, sb.clash_capacity(ev, o.M)) and ev["states"] > ev["table_slots"] // 4
