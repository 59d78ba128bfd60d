#!/usr/bin/env python3
"""Record what the three host loops of a PARENT checkout's ``ns2vc_amd/schedule.py`` compute on the cases of tests/host_loop_cases.py.

    python tools/record_host_loops.py --tree PARENT_CHECKOUT [--commit SHA] [--out tests/golden/host_loops_v1.json]

Imports ``ns2vc_amd`` from PARENT_CHECKOUT and writes, per case, the digests of the result, of every trace entry, of the arguments of every
``x0_fn`` and ``noise_fn`` call, or the text of the refusal.  Run it on the parent of a change to the loops, never on the changed tree: a
record taken from the code under test proves nothing.  tests/test_host_loops_cpu.py holds the tree to the record.  CPU only."""
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
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "host_loops_v1.json"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if tree == HERE:
        sys.exit("--tree names this checkout: the record comes from the parent commit, not from the tree it will judge")
    commit = a.commit or subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, tree)
    from ns2vc_amd import schedule
    assert os.path.abspath(schedule.__file__).startswith(tree + os.sep), schedule.__file__
    import host_loop_cases
    cases = {c: host_loop_cases.run_case(c) for c in host_loop_cases.CASES}
    for c, r in cases.items():
        print(f"{c}: " + (f"refused: {r['error']}" if "error" in r else f"{len(r['trace'])} steps, {len(r['x0_calls'])} x0_fn and "
                                                                       f"{len(r['noise_calls'])} noise_fn calls"), flush=True)
    with open(a.out, "w") as f:      # one line per case
        f.write('{"parent_commit": %s, "cases": {\n' % json.dumps(commit))
        f.write(",\n".join(f"{json.dumps(c)}: {json.dumps(r, separators=(',', ':'), sort_keys=True)}" for c, r in cases.items()))
        f.write("\n}}\n")
    print(f"{len(cases)} cases ({sum('error' in r for r in cases.values())} refusals) of {commit[:12]} -> {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
