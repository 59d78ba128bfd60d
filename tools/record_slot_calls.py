#!/usr/bin/env python3
"""Record what the slot loop (``Denoiser.open_slots`` -> ``SlotLoop``) of a PARENT checkout does on the cases of tests/slot_cases.py.

    python tools/record_slot_calls.py --tree PARENT_CHECKOUT [--commit SHA] [--out tests/golden/slot_calls_v1.json]

Imports ``ns2vc_amd`` from PARENT_CHECKOUT, puts the recording engine of tests/recording_engine.py in place of its ``pipeline.Engine`` and writes,
per case and step, the engine calls (method and a hash of the arguments; tensors enter as dtype, shape and SHA-256), the exception's type and text
of a refusal, the host state of every open loop afterwards and every field of each ``Suspended`` that came out.  Run it on the parent of a change
to the slot loop, never on the changed tree: a record taken from the code under test proves nothing.  tests/test_slot_calls_cpu.py holds the tree
to the record.  CPU only."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="a checkout of the parent commit")
    ap.add_argument("--commit", default=None, help="the parent commit (default: git rev-parse HEAD in --tree)")
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "slot_calls_v1.json"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if tree == HERE:
        sys.exit("--tree names this checkout: the record comes from the parent commit, not from the tree it will judge")
    commit = a.commit or subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, tree)
    import pytest
    from ns2vc_amd import pipeline
    assert os.path.abspath(pipeline.__file__).startswith(tree + os.sep), pipeline.__file__
    import slot_cases
    cases = {}
    for c in slot_cases.CASES:
        with pytest.MonkeyPatch.context() as mp:
            cases[c] = slot_cases.run_case(mp, c)
        print(f"{c}: {len(cases[c])} steps, {sum(len(s.get('calls', '').split()) for s in cases[c])} engine calls, "
              f"{sum('error' in s for s in cases[c])} refusals and failures", flush=True)
    with open(a.out, "w") as f:      # one line per step
        f.write('{"parent_commit": %s, "cases": {\n' % json.dumps(commit))
        f.write(",\n".join("%s: [\n%s\n]" % (json.dumps(c), ",\n".join(json.dumps(s, separators=(",", ":"), sort_keys=True) for s in steps))
                           for c, steps in cases.items()))
        f.write("\n}}\n")
    print(f"{len(cases)} cases of {commit[:12]} -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
