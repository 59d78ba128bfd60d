"""Cost of the per-item x0 correction's two kernels at the bench shape (fp16 state, B = 32, T = 938, Lp = 469, UniPC 20 steps through the per-item
form: Engine.load_samplers with 32 equal schedules, so every leg runs the items path and differs in the step's last one or two launches only):
  p0      no correction                      solver_update_items_kernel<.., TH 0>
  p1      loop-wide dynamic thresholding     abs_quantile_items_kernel + solver_update_items_kernel<.., TH 1>
  p2      loop-wide clamp                    solver_update_items_kernel<.., TH 2>
  m0      the table on, every record off     solver_update_mixed_kernel (no quantile launch)
  m1_32   the table, 32 records dynamic      abs_quantile_mixed_kernel + solver_update_mixed_kernel
  m1_8    ... 8 dynamic, 24 off
  m1_1    ... 1 dynamic, 31 off
  m2      the table, 32 records clamp        solver_update_mixed_kernel (no quantile launch)
One process, ONE engine, the legs alternating (p0, p1, ..., m2, p0, ...) for `--rounds` rounds; per leg and round the median of `--reps` timed
captured loops after a warm-up loop that captures (HIP events around the whole loop, condition set outside), divided by the 20 steps.  Reported
per leg: ms per step per round, median, spread (max - min); and the differences mixed - loop-wide in us per step: m0 - p0, m1_32 - p1, m2 - p2,
and m1_8 / m1_1 against p1.  The p legs run the parent's kernels, so their spread across rounds is the yardstick for the differences.
Usage: python tools/item_corrections_bench.py [--reps 5] [--rounds 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from ns2vc_amd.engine import Engine
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    T, Lp, NB, STEPS = 938, 469, 32, 20
    RATIO, MAXV = 0.995, 1.0
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("icb.c", (NB, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("icb.p", (NB, Lp, 256))).to(dev)
    xT = torch.from_numpy(hash_normal("icb.x", (NB, 100, T))).to(dev)
    e = Engine(precision="fp16")
    e.load_state_dict(procedural_state_dict(seed=0))
    e.prepare(NB, T, Lp)
    e.load_samplers([dict(solver="unipc", steps=STEPS)] * NB)
    e.set_condition(c, p, None)
    x = xT.clone()

    def table(n_dyn, rest):
        return lambda: e.set_x0_correction_items(["dynamic_thresholding"] * n_dyn + [rest] * (NB - n_dyn), [RATIO] * NB, [MAXV] * NB)

    legs = {"p0": lambda: None, "p1": lambda: e.set_x0_correction("dynamic_thresholding", RATIO, MAXV), "p2": lambda: e.set_x0_correction("clamp", RATIO, MAXV),
            "m0": table(0, None), "m1_32": table(32, None), "m1_8": table(8, None), "m1_1": table(1, None), "m2": table(0, "clamp")}

    def loop():
        x.copy_(xT)
        e.sample(x, use_graph=True)

    def leg(setup):
        e.set_x0_correction_items(None)
        e.set_x0_correction(None)
        setup()
        loop()                       # (captures)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            loop()
            s1.record()
            torch.cuda.synchronize()
            ts.append(s0.elapsed_time(s1) / STEPS)
        return float(np.median(ts))

    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, setup in legs.items():
            ms[k].append(leg(setup))
    e.close()
    r = {"precision": "fp16", "B": NB, "T": T, "Lp": Lp, "steps": STEPS, "reps": a.reps, "rounds": a.rounds, "ratio": RATIO, "max_val": MAXV}
    for k, v in ms.items():
        r[k + "_ms_per_step"] = {"rounds": [round(t, 4) for t in v], "median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4)}
    med = {k: float(np.median(v)) for k, v in ms.items()}
    r["mixed_minus_loop_wide_us_per_step"] = {f"{m}-{q}": round((med[m] - med[q]) * 1e3, 1)
                                              for m, q in (("m0", "p0"), ("m1_32", "p1"), ("m2", "p2"), ("m1_8", "p1"), ("m1_1", "p1"))}
    r["loop_wide_cost_us_per_step"] = {"p1-p0": round((med["p1"] - med["p0"]) * 1e3, 1), "p2-p0": round((med["p2"] - med["p0"]) * 1e3, 1)}
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
