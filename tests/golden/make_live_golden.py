"""Generates tests/golden/heap_ref_live.json and tests/golden/shortcut_ref_live.json: the answers of the REFERENCE's
heap and shortcutting loop (compiled in place into oracle/_ref/ by oracle/Makefile) to the seeded inputs of the two
live tests (test_heap_golden.live_ops, test_shortcut_golden.live_cases), so that those tests also run where the
reference is absent.  Run where the reference exists:

    make -C oracle ref && python tests/golden/make_live_golden.py

Each fixture holds the SHA-256 of the exact input text and the reference's outputs; the tests regenerate the inputs
from their seeds and check the digest first."""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_heap_golden import live_ops          # noqa: E402
from test_shortcut_golden import live_cases    # noqa: E402


def run(name, text):
    exe = os.path.join(ROOT, "oracle", "_ref", name)
    return [int(x) for x in subprocess.run([exe], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.split()]


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def main():
    _, text = live_ops()
    with open(os.path.join(ROOT, "tests", "golden", "heap_ref_live.json"), "w") as f:
        json.dump({"source": "smpl/include/smpl/intrusive_heap.h via oracle/_ref/heap_ref", "input_sha256": sha(text),
                   "top_after_each_op": run("heap_ref", text)}, f)
    cases = []
    for P, _, _, text in live_cases():
        out = run("shortcut_ref", text)
        assert out[0] == 1
        cases.append({"P": P, "input_sha256": sha(text), "out": out[2:]})
    with open(os.path.join(ROOT, "tests", "golden", "shortcut_ref_live.json"), "w") as f:
        json.dump({"source": "smpl/include/smpl/geometry/detail/shortcut.hpp:110-286 compiled in place (oracle/_ref/shortcut_ref)",
                   "cases": cases}, f)
    print("heap: 1 sequence; shortcut:", len(cases), "cases")


if __name__ == "__main__":
    main()
