"""The oracle's IntrusiveHeap against golden vectors produced by the REFERENCE's own header
(smpl/include/smpl/intrusive_heap.h compiled in place: oracle/_ref/heap_ref, tests/golden/make_heap_golden.py).
This is the one piece of the path the reference's code pins directly."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from oracle_binding import ORACLE_DIR, Oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden", "heap_ref.json")
GOLD_LIVE = os.path.join(os.path.dirname(__file__), "golden", "heap_ref_live.json")


@pytest.fixture(scope="module")
def oracle(small_cfg):
    return Oracle(small_cfg)


def test_heap_matches_reference_golden(oracle):
    cases = json.load(open(GOLD))["cases"]
    assert len(cases) >= 6
    for c in cases:
        got = oracle.heap_run(np.array(c["ops"], np.int32))
        assert got.tolist() == c["top_after_each_op"], f"case seed={c['seed']}"


def test_survey_tie_order(oracle):
    # priorities {5,3,3,9,1} pop in element order 4,1,2,0,3 (ties: the newer element sifts above)
    ops = [(0, 5), (0, 3), (0, 3), (0, 9), (0, 1)] + [(1, 0)] * 5
    got = oracle.heap_run(np.array(ops, np.int32)).tolist()
    assert got[4:] == [4, 1, 2, 0, 3, -1]


def live_ops():
    """The seeded sequence of the live test (tests/golden/make_live_golden.py stores the reference's answers to it)."""
    rng = np.random.default_rng(77)
    ops = []
    n = 0
    for _ in range(1500):
        r = rng.random()
        if r < 0.5 or n == 0:
            ops.append((0, int(rng.integers(0, 6)))); n += 1
        elif r < 0.85:
            ops.append((1, 0))
        else:
            ops.append((3, int(rng.integers(0, n))))
    return ops, f"{len(ops)}\n" + "\n".join(f"{c} {k}" for c, k in ops) + "\n"


def test_live_reference_binary_agrees_when_present(oracle):
    """The reference heap on a seeded sequence of its own: its answers are stored in tests/golden/heap_ref_live.json, and
    where oracle/_ref/heap_ref is built (the reference's header compiled in place) it is driven live as well."""
    ops, text = live_ops()
    with open(GOLD_LIVE) as f:
        stored = json.load(f)
    assert stored["input_sha256"] == hashlib.sha256(text.encode()).hexdigest(), "the seeded sequence is not the stored one"
    ref = stored["top_after_each_op"]
    binp = os.path.join(ORACLE_DIR, "_ref", "heap_ref")
    if os.path.exists(binp):
        live = subprocess.run([binp], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.split()
        assert [int(x) for x in live] == ref
    assert oracle.heap_run(np.array(ops, np.int32)).tolist() == ref
