"""Cost of classifier-free guidance in the captured loop (UniPC-20, fp16, T = 938, Lp = 469, unconditional prompt of 469 rows), four legs:
  (a) the unguided loop at B = 32 (the bench shape);
  (b) the guided loop for n = 16 items: a 32-item engine, ns2vc_sampler_set_guidance, per-item scales;
  (c) the guided loop for n = 32 items: a 64-item engine;
  (d) what a caller without guidance in the loop must do for n = 16: per step two eager evaluations at B = 16 (one engine per condition, so
      no condition is set inside the loop) and the combination in torch.  The solver update itself is left out of (d): it only gets cheaper.
One process, the legs alternating (a, b, c, d, a, b, ...) for `--rounds` rounds; per leg and round the median of `--reps` timed loops after
a warm-up loop (HIP events around the whole loop, condition set outside).  Reported: per leg the ms per step of every round, their median
and spread (max - min); (b) - (a) against (a)'s spread; (d) / (b).  A library without ns2vc_sampler_set_guidance runs (a) and (d) only, so
the same script measures leg (a) on the parent commit.
Usage: python tools/guidance_bench.py [--reps 5] [--rounds 3] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from ns2vc_amd.engine import Engine
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--legs", default="abcd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T, Lp, NB = 938, 469, 32
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("gdb.c", (NB, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("gdb.p", (NB, Lp, 256))).to(dev)
    u = torch.from_numpy(hash_normal("gdb.u", (1, Lp, 256))).to(dev).expand(NB, -1, -1).contiguous()
    xT = torch.from_numpy(hash_normal("gdb.x", (NB, 100, T))).to(dev)
    W = procedural_state_dict(seed=0)
    has_guidance = hasattr(Engine, "set_guidance")
    engines = {}

    def engine(key, B):
        if key not in engines:
            e = Engine(precision="fp16")
            e.load_state_dict(W)
            e.prepare(B, T, Lp)
            e.load_sampler("unipc", a.steps)
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
        return float(np.median(ts)) / a.steps

    def captured(e, x0):
        x = x0.clone()
        e.sample(x, use_graph=True)            # capture (first round) + warm-up
        torch.cuda.synchronize()

        def loop():
            x.copy_(x0)
            e.sample(x, use_graph=True)
        return timed(loop)

    def leg_a():
        e = engine("a", NB)
        e.set_condition(c, p, None)
        return captured(e, xT)

    def guided(key, n):
        e = engine(key, 2 * n)
        e.set_guidance(np.linspace(1.5, 3.0, n).astype(np.float32))
        e.set_condition(torch.cat([c[:n], c[:n]]).contiguous(), torch.cat([u[:n], p[:n]]).contiguous(), None)
        return captured(e, xT[:n].contiguous())

    def leg_d():
        n = 16
        eu, ec = engine("du", n), engine("dc", n)
        eu.set_condition(c[:n].contiguous(), u[:n].contiguous(), None)
        ec.set_condition(c[:n].contiguous(), p[:n].contiguous(), None)
        x = xT[:n].contiguous().clone()
        ou, oc = torch.empty_like(x), torch.empty_like(x)
        sc = torch.linspace(1.5, 3.0, n, device=dev).view(n, 1, 1)
        ts = [torch.full((n,), float(t), device=dev) for t in eu.table.t_model]

        def loop():
            for t in ts:
                eu.forward(x, t, ou)
                ec.forward(x, t, oc)
                torch.where(sc == 1.0, oc, ou + sc * (oc - ou))
        loop()
        torch.cuda.synchronize()
        return timed(loop)

    legs = {"a_unguided_b32": leg_a, "d_two_eager_calls_n16": leg_d}
    if has_guidance:
        legs.update({"b_guided_n16": lambda: guided("b", 16), "c_guided_n32": lambda: guided("c", 32)})
    legs = {k: v for k, v in sorted(legs.items()) if k[0] in a.legs}
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            ms[k].append(fn())
    r = {"solver": f"unipc-{a.steps}", "precision": "fp16", "T": T, "Lp": Lp, "reps": a.reps, "rounds": a.rounds, "guidance_in_library": has_guidance}
    for k, v in ms.items():
        r[k] = {"ms_per_step_rounds": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4)}
    if "b_guided_n16" in ms and "a_unguided_b32" in ms:
        r["b_minus_a_ms"] = round(r["b_guided_n16"]["median"] - r["a_unguided_b32"]["median"], 4)
    if "b_guided_n16" in ms and "d_two_eager_calls_n16" in ms:
        r["d_over_b"] = round(r["d_two_eager_calls_n16"]["median"] / r["b_guided_n16"]["median"], 3)
    for e in engines.values():
        e.close()
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
