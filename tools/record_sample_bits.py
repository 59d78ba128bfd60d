#!/usr/bin/env python3
"""Record the latents ``Denoiser.sample`` / ``sample_long`` of a PARENT checkout return on the call sequence of tests/sample_cases.py (BIT_CALLS).

    python tools/record_sample_bits.py --tree PARENT_CHECKOUT [--commit SHA] [--out tests/golden/sample_bits_v1.json]

Imports ``ns2vc_amd`` from PARENT_CHECKOUT (its library must be built), runs the sequence on one ``Denoiser("fp16")`` and one ``Denoiser("fp32")``
with ``procedural_state_dict(seed=0)`` and writes, per precision and call, the SHA-256 of the returned latent and ``graph_captures()`` of the head
and the tail engine after the call.  Run it on the parent of a change to ns2vc_amd/pipeline.py, never on the changed tree.
tests/test_sample_bits_gpu.py holds the tree to the record.  Needs the GPU."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="a checkout of the parent commit, built")
    ap.add_argument("--commit", default=None, help="the parent commit (default: git rev-parse HEAD in --tree)")
    ap.add_argument("--out", default=os.path.join(HERE, "tests", "golden", "sample_bits_v1.json"))
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    if tree == HERE:
        sys.exit("--tree names this checkout: the record comes from the parent commit, not from the tree it will judge")
    commit = a.commit or subprocess.run(["git", "-C", tree, "rev-parse", "HEAD"], check=True, capture_output=True, text=True).stdout.strip()
    sys.path.insert(0, os.path.join(HERE, "tests"))
    sys.path.insert(0, tree)
    from ns2vc_amd import pipeline
    assert os.path.abspath(pipeline.__file__).startswith(tree + os.sep), pipeline.__file__
    from ns2vc_amd.weights import procedural_state_dict
    import sample_cases
    W = procedural_state_dict(seed=0)
    record = {}
    for prec in ("fp16", "fp32"):
        record[prec] = sample_cases.run_bits(pipeline.Denoiser(W, precision=prec))
        for label, r in record[prec].items():
            print(prec, label, r["sha256"][:12], r["head_captures"], r["tail_captures"], flush=True)
    with open(a.out, "w") as f:
        json.dump({"parent_commit": commit, "calls": record}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{sum(len(v) for v in record.values())} calls of {commit[:12]} -> {a.out}")


if __name__ == "__main__":
    main()
