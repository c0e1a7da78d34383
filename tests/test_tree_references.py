"""The cases of tree_cases.py on the CPU: the robots have the shape they are there for, the probe equals the oracle on
every state used (so the oracle stays the judge of tests/test_gpu_tree_walks.py and the probe only says what a state
exercises), the state sets reach the edges of the walks' scratch, and the model compiler accepts a model at each of its
limits and refuses one just past it.

No kernel with a short stack or a short queue is ever run: that the last stack byte is written AND read back, that the
queue holds exactly twelve, thirteen and more pairs, is shown here, on the inputs.

One condition cannot be met by any robot, and the tests say why (test_full_depth_walks_cannot_end_valid): a pair walk that
holds the whole stack has split the deepest inner node of a tree, and under the tree builder's split at the mean the two
leaves below the deepest node of a depth-16 tree lie within 1e-13 of the link's extent of each other; that node IS its
larger leaf, so the pair that made the walk split it collides.  Full-depth walks are therefore all invalid; what the valid
ones were wanted for -- every byte read back before the verdict -- is asserted on invalid states instead: the walk reads
the top stack bytes back and only then reaches the leaf pair that decides.
"""
import ctypes as C
import re

import numpy as np
import pytest

import tree_cases as tc

NAMES = ["deep", "deep40", "crowd", "order"]


def _header(model):
    from smpl_amd import capi
    L = capi.lib()
    L.smplx_test_const_header.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int]
    n = L.smplx_test_const_header(model.h, 0, None, 0)
    buf = C.create_string_buffer(n)
    L.smplx_test_const_header(model.h, 0, buf, n)
    return buf.value.decode()


def _ints(header, name):
    m = re.search(name + r"\[[^\]]*\]\s*=\s*\{([^}]*)\}", header)
    assert m, name
    return [int(v) for v in m.group(1).replace(",", " ").split()]


@pytest.fixture(scope="module")
def models():
    from smpl_amd import capi
    return {n: capi.Model(tc.case(n).robot_text) for n in NAMES}


# ----------------------------------------------------------------------------------------------------------------------
# the robots
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_engine_and_oracle_compile_the_same_trees_and_pairs(name, models):
    m = models[name]
    a = m.arrays()
    o, probe = tc.oracle_and_probe(name)
    om = o.model()
    assert np.array_equal(a["xyzr"], om["xyzr"]) and np.array_equal(a["tree_first"], om["tree_first"])
    assert np.array_equal(a["left"], np.array(probe.left)) and np.array_equal(a["right"], np.array(probe.right))
    assert np.array_equal(a["pairs"], om["pairs"])
    assert m.nvars <= 4
    print(f"{name}: {m.njoints} joints, {m.ntrees} trees, {m.nnodes} nodes, {m.npairs} pairs, {m.nslots} save slots")


@pytest.mark.parametrize("name", NAMES)
def test_stack_bytes_is_the_probes_need_rounded_up(name, models):
    _, probe = tc.oracle_and_probe(name)
    need = probe.stack_need()
    assert need == tc.STACK_NEED[name]
    h = _header(models[name])
    got = int(re.search(r"#define CM_STACK_BYTES (\d+)", h).group(1))
    assert got == max(tc.STACK_MIN, (need + 7) // 8 * 8)
    print(f"{name}: stack need {need}, CM_STACK_BYTES {got}")


def test_deep_trees_peel_one_sphere_per_level():
    for name, (da, dc) in (("deep", (16, 16)), ("deep40", (11, 9))):
        _, probe = tc.oracle_and_probe(name)
        d = [probe.depth(r) for r in probe.roots]
        assert d == [da, 0, dc] and probe.pairs == [(0, 2)]
        for t in (0, 2):         # the left child carries the rest of the row, the right child is the peeled leaf
            n = probe.roots[t]
            while probe.left[n] >= 0:
                assert probe.left[probe.right[n]] < 0
                n = probe.left[n]
    _, probe = tc.oracle_and_probe("deep")
    assert tc.STACK_NEED["deep"] == tc.STACK_MAX
    assert 24 < tc.STACK_NEED["deep40"] < 64 and ((tc.STACK_NEED["deep40"] + 7) // 8 * 8) % 16 != 0


def test_order_robot_is_out_of_order(models):
    m = models["order"]
    _, probe = tc.oracle_and_probe("order")
    assert m.nslots == 2
    assert probe.chain != sorted(probe.chain) and probe.chain != sorted(probe.chain, reverse=True)
    swapped = [probe.pair_is_swapped(k) for k in range(len(probe.pairs))]
    assert any(swapped) and not all(swapped)
    h = _header(m)
    slots = _ints(h, "CM_ROOT_SLOT")
    assert -1 in slots and slots[probe.chain[-1]] == -1          # the tree the chain reaches last leads no pair
    leaf = [probe.left[r] < 0 for r in probe.roots]
    assert any(leaf) and not all(leaf)
    assert any(leaf[a] and leaf[b] for a, b in probe.pairs)
    inner_r = [probe.r[r] for r, l in zip(probe.roots, leaf) if not l]
    assert len(set(inner_r)) == len(inner_r)
    # the kernels' pair table, restated: same pairs, grouped by the partner that comes later in depth-first order
    other, first = _ints(h, "CM_PAIR_OTHER"), _ints(h, "CM_PAIR_FIRST")
    want = []
    for t in range(m.ntrees):
        assert first[t] == len(want)
        for k in probe.kernel_pair_order():
            a, b = probe.pairs[k]
            late, early = (b, a) if probe.chain_pos[a] < probe.chain_pos[b] else (a, b)
            if late == t:
                want.append(early)
    assert other == want and first[m.ntrees] == len(want) == m.npairs


def test_crowd_robot_pairs(models):
    m = models["crowd"]
    _, probe = tc.oracle_and_probe("crowd")
    assert m.ntrees >= 8 and (0, m.ntrees - 1) in probe.pairs
    assert m.npairs == (m.ntrees - 1) * (m.ntrees - 2) // 2 > 2 * tc.PENDING_MAX
    assert all(probe.left[r] >= 0 for r in probe.roots)          # every root is inner: an overlap of roots is queued


# ----------------------------------------------------------------------------------------------------------------------
# the probe against the oracle, and the conditions on the state sets
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_probe_equals_the_oracle_on_every_state(name, models):
    o, probe = tc.oracle_and_probe(name)
    Q, S = tc.state_set(name)
    assert 0 < len(Q) <= tc.SET_SIZE and len(S) == len(Q)
    lim = np.array(tc.LIMITS[name])
    assert (Q >= lim[:, 0]).all() and (Q <= lim[:, 1]).all()
    for q, s in zip(Q, S):
        ok, lookups = o.state_valid(q)
        assert ok == s["valid"] and lookups == s["lookups"]
        assert s["stack"] <= tc.STACK_NEED[name]
    print(f"{name}: {len(Q)} states, classes {tc.census(name)}")
    cfg = tc.case(name)
    assert o.state_valid(cfg.start)[0]


@pytest.mark.parametrize("name", ["deep", "deep40"])
def test_deep_sets_reach_the_last_stack_byte(name):
    Q, S = tc.state_set(name)
    level = tc.stack_level(name)
    assert level == tc.STACK_NEED[name] and level > {"deep": 56, "deep40": 32}[name]      # within the last 8 bytes of stack_bytes
    full = [s for s in S if s["voxel_clear"] and s["stack"] == level]
    walks = [s["walks"][0] for s in full]
    assert len(full) >= 32
    # the walk misses the first leaf pair below the deepest node, reads the top two bytes back, and is decided by a
    # leaf pair it reaches only after popping from the upper half of the stack
    top = [w for w in walks if w.popped >= level - 1]
    upper = [w for w in walks if w.hit is not None and w.hit_after_pop >= level // 2]
    both = [w for w in walks if w.hit is not None and w.hit_after_pop >= level - 1]
    print(f"{name}: full depth {len(full)}, top bytes read back {len(top)}, decided after a pop from the upper half {len(upper)}, "
          f"decided after the top pop {len(both)}")
    assert len(top) >= 8 and len(upper) >= 8 and len(both) >= 8
    # both verdicts in the set, and valid states whose walk goes as deep as a valid walk can
    rest = [s for s in S if s["voxel_clear"] and s["stack"] < level]
    assert sum(s["valid"] for s in rest) >= 8 and sum(not s["valid"] for s in rest) >= 8
    assert max(s["stack"] for s in rest if s["valid"]) >= 8
    assert sum(not s["voxel_clear"] for s in S) >= 8


@pytest.mark.parametrize("name", ["deep", "deep40"])
def test_full_depth_walks_cannot_end_valid(name):
    """Valid states among the full-depth ones would show a walk that holds the whole stack and pops every byte again.
    There are none, whatever the radii: the deepest inner node of each row is, to the last bit of a world position, its
    larger leaf, so whatever overlaps it collides (measured: deep 120 full-depth states of 360, deep40 120 of 360, all
    invalid; 79 and 85 of them read the top two bytes back before the leaf pair that decides)."""
    _, probe = tc.oracle_and_probe(name)
    Q, S = tc.state_set(name)
    for t in (0, 2):
        n = probe.roots[t]
        while probe.left[probe.left[n]] >= 0:
            n = probe.left[n]
        kids = (probe.left[n], probe.right[n])
        big = max(kids, key=lambda k: probe.r[k])
        assert probe.r[n] == probe.r[big]
        assert np.abs(probe.xyzr[n, :3] - probe.xyzr[big, :3]).max() < 1e-18
    full = [s for s in S if s["voxel_clear"] and s["stack"] == tc.stack_level(name)]
    assert full and not any(s["valid"] for s in full)


def test_crowd_set_fills_and_overflows_the_queue():
    _, probe = tc.oracle_and_probe("crowd")
    Q, S = tc.state_set("crowd")
    clear = [s for s in S if s["voxel_clear"]]
    n = np.array([s["queue"] for s in clear])
    sizes = {"0": int((n == 0).sum()), "1..11": int(((n >= 1) & (n <= 11)).sum()), "12": int((n == 12).sum()),
             "13": int((n == 13).sum()), ">13": int((n > 13).sum())}
    over = [s for s in clear if s["queue"] >= 13]
    valid, invalid = [s for s in over if s["valid"]], [s for s in over if not s["valid"]]
    first = sorted({s["first_pair"] for s in invalid})
    print(f"crowd: queue classes {sizes}, largest {n.max()}; overflowed and valid {len(valid)}, invalid {len(invalid)}, "
          f"first colliding pairs {[probe.pairs[k] for k in first]}")
    assert min(sizes.values()) >= 20
    assert len(valid) >= 20 and len(invalid) >= 20
    assert len(first) >= 6
    last = probe.nt - 1
    assert any(last in probe.pairs[k] for k in first)
    assert set(first) & set(probe.kernel_pair_order()[:3])
    assert all(s["leaf_roots"] == 0 for s in clear)


def test_order_set_is_decided_by_swapped_pairs_and_by_leaf_roots():
    _, probe = tc.oracle_and_probe("order")
    Q, S = tc.state_set("order")
    clear = [s for s in S if s["voxel_clear"]]
    assert sum(s["valid"] for s in clear) >= 20 and sum(not s["valid"] for s in clear) >= 20
    swapped = [s for s in clear if s["first_pair"] >= 0 and probe.pair_is_swapped(s["first_pair"])]
    leaf = [s for s in clear if s["decided_by_leaf_roots"]]
    only_swapped = [s for s in clear if not s["valid"] and
                    all(probe.pair_is_swapped(k) for k, w in enumerate(s["walks"]) if w.hit is not None)]
    print(f"order: decided by a swapped pair {len(swapped)} (no other pair collides in {len(only_swapped)}), "
          f"by leaf roots alone {len(leaf)}")
    assert len(swapped) >= 20 and len(only_swapped) >= 20 and len(leaf) >= 20
    assert all(s["leaf_roots"] > 0 for s in leaf)


# ----------------------------------------------------------------------------------------------------------------------
# the model's limits
# ----------------------------------------------------------------------------------------------------------------------

def _create(text):
    from smpl_amd import capi
    L = capi.lib()
    h = C.c_void_p()
    code = L.smplx_model_create(text.encode(), C.byref(h))
    L.smplx_last_error.restype = C.c_char_p
    msg = L.smplx_last_error().decode() if code != 0 else ""
    if code == 0:
        c = [C.c_int() for _ in range(6)]
        L.smplx_model_counts(h, *[C.byref(x) for x in c])
        L.smplx_model_destroy(h)
        return 0, "", [x.value for x in c]
    return code, msg, h.value


def _leaves(ntrees, nnodes):
    """leaves per tree of a model of ntrees trees and nnodes nodes (a tree of n leaves has 2 n - 1 nodes)"""
    total = (nnodes + ntrees) // 2
    assert 2 * total - ntrees == nnodes
    out = [total // ntrees] * ntrees
    for i in range(total - sum(out)):
        out[i] += 1
    return out


def test_models_at_the_limits_are_accepted():
    # 24 trees, 128 nodes and 160 checked pairs at once
    code, msg, counts = _create(tc.limit_robot(_leaves(24, 128), 160))
    assert code == 0, msg
    assert counts[2:5] == [24, 128, 160]
    # stack need 64
    code, msg, counts = _create(tc.deep_robot(17, 17))
    assert code == 0, msg
    # two levels of branching
    code, msg, counts = _create(tc.order_robot())
    assert code == 0 and counts[5] == 2


@pytest.mark.parametrize("what,text,message", [
    ("129 nodes", lambda: tc.limit_robot(_leaves(23, 129), 100), "too many sphere-tree nodes"),
    ("25 trees", lambda: tc.limit_robot([1] * 25, 100), "too many sphere trees"),
    ("161 pairs", lambda: tc.limit_robot(_leaves(24, 128), 161), "too many checked link pairs"),
    ("three levels of branching", tc.three_branchings_robot, "branches too deeply"),
    ("stack need 68", lambda: tc.deep_robot(18, 18), "too deep for the traversal stack"),
])
def test_models_past_a_limit_are_refused(what, text, message):
    code, msg, handle = _create(text())
    assert code != 0 and handle is None, what
    assert message in msg, msg
    others = {"too many sphere-tree nodes", "too many sphere trees", "too many checked link pairs", "branches too deeply",
              "too deep for the traversal stack"} - {message}
    assert not any(o in msg for o in others)


def test_one_step_inside_each_limit_is_what_the_refusals_exceed():
    """the refused models differ from accepted ones by the one count: 127 nodes in 23 trees, 24 single-leaf trees, 18
    spheres on one link only (need 2 * (17 + 15) = 64)"""
    assert _create(tc.limit_robot(_leaves(23, 127), 100))[0] == 0
    assert _create(tc.limit_robot([1] * 24, 100))[0] == 0
    assert _create(tc.deep_robot(18, 16))[0] == 0


@pytest.mark.parametrize("name", NAMES)
def test_edge_sets_hold_edges_refused_by_an_inner_waypoint_alone(name):
    """edges between two valid states that the oracle refuses; on some of them a waypoint reaches the edge of the walks'
    scratch (the probe on the waypoints of tree_cases.waypoints, which the GPU module holds to the engine's own)"""
    o, probe = tc.oracle_and_probe(name)
    A, B, ok, lk, inner, show = tc.edges(name)
    assert len(A) <= tc.SET_SIZE and len(inner) >= 20 and len(show) >= 6
    W = np.array([o.waypoint_count(a, b) for a, b in zip(A, B)])
    assert (W <= 5).sum() >= 50 and (W > 5).sum() >= 50 and 20 <= ok.sum() <= len(ok) - 20
    for i in show[:3]:
        states = [probe.state(q) for q in tc.waypoints(A[i], B[i], W[i])]
        bad = [k for k, st in enumerate(states) if not st["valid"]]
        assert bad and 0 < bad[0] and bad[-1] < W[i] - 1
    print(f"{name}: {len(A)} edges, {int(ok.sum())} valid, {len(inner)} refused by inner waypoints alone, waypoints up to {W.max()}")
