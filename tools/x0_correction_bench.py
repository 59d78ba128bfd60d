"""Cost of the x0 correction in the captured loop (dynamic thresholding / clamp), two parts in one process.

Kernel part, T = 938, ld = 128, nc = 100, fp16 state, at n = 32 and n = 1 items (one workgroup per item: n = 1 is the worst occupancy), each
the median of `--reps` timings of `--inner` back-to-back launches between two HIP events, the legs alternating for `--rounds` rounds:
  plain      ns2vc_k_solver_update                                  (the 24.6 us update of DESIGN 4.8)
  clamp      ns2vc_k_solver_update_corrected mode 2                 (the corrected update alone)
  quantile   ns2vc_k_abs_quantile on ready values                   (the radix select alone: 3 sweeps of one operand)
  dynamic    ns2vc_k_solver_update_corrected mode 1                 (the quantile launch on x0 + xe, then the update by thr)
  torch      torch.quantile(|m|.reshape(n, -1), p, dim=1), maximum, clamp, divide on an (n, 100, 938) tensor: what a caller outside the loop runs
Loop part (UniPC-20, fp16, B = 32, T = 938, Lp = 469, as tools/guidance_bench.py): ms per step of the captured loop with the correction off,
with the clamp and with dynamic thresholding, alternating.  A library without ns2vc_sampler_set_x0_correction runs `plain`, `torch` and the
loop with the correction off only, so the same script measures the parent commit.
Usage: python tools/x0_correction_bench.py [--reps 5] [--rounds 3] [--inner 20] [--skip-loop] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from ns2vc_amd import _lib
    from ns2vc_amd import schedule as S
    from ns2vc_amd.engine import DevBuf, Engine
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-loop", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = _lib.load()
    has = hasattr(Engine, "set_x0_correction")
    T, LD, NC, Lp, NB = 938, 128, 100, 469, 32
    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)

    def timed(fn, per):
        ts = []
        for _ in range(a.reps):
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            fn()
            s1.record()
            torch.cuda.synchronize()
            ts.append(s0.elapsed_time(s1))
        return float(np.median(ts)) / per

    table = S.build_table("unipc", 10, order=2)
    coef, step = DevBuf.from_numpy(np.ascontiguousarray(table.coef, np.float32)), DevBuf.from_numpy(np.array([4, 0, 0, 0], np.int32))
    r = {"T": T, "ld": LD, "nc": NC, "reps": a.reps, "rounds": a.rounds, "inner": a.inner, "correction_in_library": has, "kernels_us": {}}
    for n in (NB, 1):
        rows = n * T
        rng = np.random.default_rng(n)
        st = {k: DevBuf.from_numpy(rng.standard_normal((rows, LD)).astype(np.float32)) for k in ("x0", "xe", "xbar", "d1", "mprev")}
        op, thr = DevBuf(rows * 2 * LD * 2), DevBuf(((n + 3) // 4) * 16)
        m_t = torch.randn((n, NC, T), device=dev)

        def upd(mode):
            def go():
                for _ in range(a.inner):
                    if mode == 0:
                        lib.ns2vc_k_solver_update(coef.ptr, step.ptr, st["x0"].ptr, st["xe"].ptr, op.ptr, 2, st["xbar"].ptr, st["d1"].ptr, st["mprev"].ptr, None,
                                                  rows * LD, LD, None)
                    else:
                        lib.ns2vc_k_solver_update_corrected(coef.ptr, step.ptr, st["x0"].ptr, st["xe"].ptr, op.ptr, 2, st["xbar"].ptr, st["d1"].ptr,
                                                            st["mprev"].ptr, None, rows * LD, LD, T, None, None, NC, mode, 0.995, 1.0, thr.ptr, None)
            return go

        def quant():
            for _ in range(a.inner):
                lib.ns2vc_k_abs_quantile(st["x0"].ptr, n, T, LD, NC, None, 0.995, thr.ptr, None)

        def torch_way():
            for _ in range(a.inner):
                s = torch.quantile(m_t.abs().reshape(n, -1), 0.995, dim=1)
                s = torch.maximum(s, torch.ones_like(s)).reshape(n, 1, 1)
                torch.clamp(m_t, -s, s) / s
        legs = {"plain": upd(0), "torch": torch_way}
        if has:
            legs.update({"clamp": upd(2), "quantile": quant, "dynamic": upd(1)})
        us = {k: [] for k in legs}
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in legs.items():
                us[k].append(1000.0 * timed(fn, a.inner))
        r["kernels_us"][f"n{n}"] = {k: {"rounds": [round(x, 2) for x in v], "median": round(float(np.median(v)), 2)} for k, v in us.items()}
    if not a.skip_loop:
        c = torch.from_numpy(hash_normal("gdb.c", (NB, 256, T))).to(dev)
        p = torch.from_numpy(hash_normal("gdb.p", (NB, Lp, 256))).to(dev)
        xT = torch.from_numpy(hash_normal("gdb.x", (NB, 100, T))).to(dev)
        e = Engine(precision="fp16")
        e.load_state_dict(procedural_state_dict(seed=0))
        e.prepare(NB, T, Lp)
        e.load_sampler("unipc", a.steps)
        e.set_condition(c, p, None)
        x = xT.clone()

        def loop_leg(corr):
            if has:
                e.set_x0_correction(*corr)
            x.copy_(xT)
            e.sample(x, use_graph=True)          # capture + warm-up
            torch.cuda.synchronize()

            def loop():
                x.copy_(xT)
                e.sample(x, use_graph=True)
            return timed(loop, a.steps)
        legs = {"off": (None,)}
        if has:
            legs.update({"clamp": ("clamp", 0.995, 1.0), "dynamic": ("dynamic_thresholding", 0.995, 1.0)})
        ms = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, corr in legs.items():
                ms[k].append(loop_leg(corr))
        r["loop_ms_per_step"] = {k: {"rounds": [round(v, 4) for v in vs], "median": round(float(np.median(vs)), 4), "spread": round(max(vs) - min(vs), 4)}
                                 for k, vs in ms.items()}
        e.close()
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
