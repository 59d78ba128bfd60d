#!/usr/bin/env python3
"""Record what the solver-update and quantile kernels of a PARENT checkout compute on the cases of tests/solver_cases.py.

    python tools/record_solver_bits.py --tree PARENT_CHECKOUT [--commit SHA] [--out tests/golden/solver_bits_v2.json]

Loads PARENT_CHECKOUT/ns2vc_amd/lib/libns2vc_hip.so through that tree's own binding (as tools/item_schedules_bench.py --tree does), building it
with the tree's Makefile first when it is not there, runs every case and writes per case and array the shape, the dtype and the SHA-256 of the
bytes, with the parent's commit and the compiler's version line.  Run it on the parent of a change to these kernels, never on the changed tree: a
record taken from the code under test proves nothing.  tests/test_solver_bits_gpu.py holds the built library to the record.  Needs the GPU."""
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
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "solver_bits_v2.json"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if tree == HERE:
        sys.exit("--tree names this checkout: the record comes from the parent commit, not from the tree it will judge")
    if not os.path.exists(os.path.join(tree, "ns2vc_amd", "lib", "libns2vc_hip.so")):
        subprocess.run(["make", "-C", os.path.join(tree, "ns2vc_amd", "csrc"), "-j", "8"], check=True)
    commit = a.commit or subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    hipcc = subprocess.run(["hipcc", "--version"], check=True, capture_output=True, text=True).stdout.splitlines()[0].strip()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, tree)
    from ns2vc_amd import _lib
    assert os.path.abspath(_lib.__file__).startswith(tree + os.sep), _lib.__file__
    import solver_cases
    lib = _lib.load()
    cases = {}
    for c in solver_cases.CASES:
        cases[c] = solver_cases.digest(solver_cases.run_case(lib, c))
        print(c, " ".join(f"{k}:{v['sha256'][:8]}" for k, v in cases[c].items()), flush=True)
    with open(a.out, "w") as f:
        json.dump({"parent_commit": commit, "hipcc": hipcc, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(cases)} cases of {commit[:12]} -> {a.out}")


if __name__ == "__main__":
    main()
