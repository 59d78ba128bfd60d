"""Cost and gain of per-item sampler schedules in the captured loop (fp16, T = 938, Lp = 469), four legs:
  (a) the shared-table loop, UniPC-20 at B = 32 (the bench shape) -- the feature off;
  (b) the same job through the per-item form: Engine.load_samplers with 32 EQUAL schedules (Denoiser.sample would route them to (a); the engine
      call forces the items update, the items time embedding and the records) -- the price of the per-item launches;
  (c) ONE batch of 32 with eight items each at 10 / 20 / 30 / 50 UniPC steps: one loop of 50 steps;
  (d) the same work as four B = 8 shared-table loops of 10, 20, 30 and 50 steps, one after the other (one engine per loop, prepared outside).
One process, the legs alternating (a, b, c, d, a, ...) for `--rounds` rounds; per leg and round the median of `--reps` timed loops after a
warm-up loop (HIP events around the whole loop, condition set outside).  Reported: (a), (b) in ms per step, (c), (d) in total ms, per round,
with median and spread (max - min); (b) - (a); (d) / (c).  `--tree DIR` imports the package (and its library) from another checkout: a tree
without Engine.load_samplers runs (a) and (d) only, so the same script measures leg (a) on the parent commit.
Usage: python tools/item_schedules_bench.py [--reps 5] [--rounds 3] [--legs abcd] [--tree DIR] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from ns2vc_amd.engine import Engine
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    T, Lp, NB = 938, 469, 32
    MIX = (10, 20, 30, 50)
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("isb.c", (NB, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("isb.p", (NB, Lp, 256))).to(dev)
    xT = torch.from_numpy(hash_normal("isb.x", (NB, 100, T))).to(dev)
    W = procedural_state_dict(seed=0)
    has_items = hasattr(Engine, "load_samplers")
    engines = {}

    def engine(key, B, load):
        if key not in engines:
            e = Engine(precision="fp16")
            e.load_state_dict(W)
            e.prepare(B, T, Lp)
            load(e)
            engines[key] = e
        return engines[key]

    def timed(fn):
        ts = []
        for _ in range(a.reps):
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            fn()
            s1.record()
            torch.cuda.synchronize()
            ts.append(s0.elapsed_time(s1))
        return float(np.median(ts))

    def captured(jobs):
        """jobs = [(engine, x_T)]: capture + warm-up, then the timed loops, one after the other"""
        xs = [x0.clone() for _, x0 in jobs]
        for (e, _), x in zip(jobs, xs):
            e.sample(x, use_graph=True)
        torch.cuda.synchronize()

        def loop():
            for (e, x0), x in zip(jobs, xs):
                x.copy_(x0)
                e.sample(x, use_graph=True)
        return timed(loop)

    def leg_a():
        e = engine("a", NB, lambda e: e.load_sampler("unipc", 20))
        e.set_condition(c, p, None)
        return captured([(e, xT)]) / 20

    def leg_b():
        e = engine("b", NB, lambda e: e.load_samplers([dict(solver="unipc", steps=20)] * NB))
        e.set_condition(c, p, None)
        return captured([(e, xT)]) / 20

    def leg_c():
        e = engine("c", NB, lambda e: e.load_samplers([dict(solver="unipc", steps=MIX[b // 8]) for b in range(NB)]))
        e.set_condition(c, p, None)
        return captured([(e, xT)])

    def leg_d():
        jobs = []
        for g, n in enumerate(MIX):
            e = engine(f"d{g}", 8, lambda e, n=n: e.load_sampler("unipc", n))
            e.set_condition(c[8 * g:8 * g + 8].contiguous(), p[8 * g:8 * g + 8].contiguous(), None)
            jobs.append((e, xT[8 * g:8 * g + 8].contiguous()))
        return captured(jobs)

    legs = {"a_shared_b32_ms_per_step": leg_a, "d_four_b8_loops_total_ms": leg_d}
    if has_items:
        legs.update({"b_items_equal_b32_ms_per_step": leg_b, "c_one_mixed_b32_loop_total_ms": leg_c})
    legs = {k: v for k, v in sorted(legs.items()) if k[0] in a.legs}
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            ms[k].append(fn())
    r = {"precision": "fp16", "T": T, "Lp": Lp, "reps": a.reps, "rounds": a.rounds, "mix_steps": list(MIX), "items_in_library": has_items,
         "tree": os.path.basename(os.path.abspath(a.tree))}
    for k, v in ms.items():
        r[k] = {"rounds": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4)}
    ka, kb, kc, kd = "a_shared_b32_ms_per_step", "b_items_equal_b32_ms_per_step", "c_one_mixed_b32_loop_total_ms", "d_four_b8_loops_total_ms"
    if ka in ms and kb in ms:
        r["b_minus_a_ms_per_step"] = round(r[kb]["median"] - r[ka]["median"], 4)
    if kc in ms and kd in ms:
        r["d_over_c"] = round(r[kd]["median"] / r[kc]["median"], 3)
    for e in engines.values():
        e.close()
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
