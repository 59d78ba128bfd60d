"""Order-3 multistep solvers at the bench shape (10 s x batch 32, Lp 469, procedural weights, fp16, captured): speed and precision.

  speed      ms/step of UniPC-2, UniPC-3, DPM-Solver++(2M) and DPM-Solver++(3M) at 20 steps, alternated in one process (--rounds rounds)
  precision  each fp16 loop with tail = 0, 1, 2, 3 fp32 evaluations against the fp32 engine on the same x_T: rel-L2, worst item,
             worst frame / channel (tests/util.py local_errors) -- what sets pipeline.DEFAULT_TAIL_FP32_ORDER3
  order      for information only: the fp32 loop at NFE 5 / 8 / 10 / 15 / 20 against a 200-step fp32 UniPC-3 loop (logSNR and
             time_uniform).  Procedural weights are not a trained model: this shows the solvers' order, not audio quality.

python tools/solver_bench.py [--rounds 3] [--skip-precision] [--skip-order]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ns2vc_amd.engine import Engine, Event  # noqa: E402
from ns2vc_amd.weights import hash_normal, procedural_state_dict  # noqa: E402
from util import local_errors, rel_l2  # noqa: E402

CASES = [("UniPC-2", "unipc", 2), ("UniPC-3", "unipc", 3), ("DPM++-2M", "dpmsolver++", 2), ("DPM++-3M", "dpmsolver++", 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--skip-precision", action="store_true")
    ap.add_argument("--skip-order", action="store_true")
    ap.add_argument("--tails", default="0,1,2,3", help="fp32 tail lengths of the precision table")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, Lp = 32, 938, 469
    W = procedural_state_dict(seed=0)
    c = torch.from_numpy(hash_normal("sob.c", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("sob.p", (B, Lp, 256))).to(dev)
    mask = torch.ones((B, Lp), dtype=torch.uint8, device=dev)
    x_T = torch.from_numpy(hash_normal("sob.x", (B, 100, T))).to(dev)
    N = a.steps

    def engine(prec):
        e = Engine(precision=prec)
        e.load_state_dict(W)
        e.prepare(B, T, Lp)
        e.set_condition(c, p, mask)
        return e

    def timed(e, tail=None, k=0):
        x = x_T.clone()
        t0, t1 = Event(), Event()
        t0.record(None)
        e.sample(x, tail=tail, tail_steps=k)
        t1.record(None)
        return t0.elapsed_ms(t1), x

    # ---- speed: one engine per case (each keeps its captured graph), alternated
    engs = {}
    for name, solver, order in CASES:
        engs[name] = engine("fp16")
        engs[name].load_sampler(solver, N, order=order)
        timed(engs[name])                                  # capture + warm-up
    ms = {name: [] for name, _, _ in CASES}
    for _ in range(a.rounds):
        for name, _, _ in CASES:
            ms[name].append(timed(engs[name])[0] / N)
    for name, _, _ in CASES:
        print(f"speed {name}-{N} fp16 captured: {np.median(ms[name]):.3f} ms/step (rounds {' '.join(f'{v:.3f}' for v in ms[name])})", flush=True)
    base = {"unipc": np.median(ms["UniPC-2"]), "dpmsolver++": np.median(ms["DPM++-2M"])}
    for name, solver, order in CASES:
        if order == 3:
            print(f"speed {name} / order 2: {np.median(ms[name]) / base[solver]:.4f}", flush=True)

    if not a.skip_precision:
        e32, et = engine("fp32"), engine("fp32")
        for name, solver, order in CASES:
            e32.load_sampler(solver, N, order=order)
            et.load_sampler(solver, N, order=order)
            y32 = timed(e32)[1].cpu().numpy()
            e16 = engs[name]
            for tail in (int(v) for v in a.tails.split(",")):
                timed(e16, et if tail else None, tail)
                t, y = timed(e16, et if tail else None, tail)
                y = y.cpu().numpy()
                loc = local_errors(y, y32)
                print(f"precision {name}-{N} fp16 tail {tail}: rel-L2 {rel_l2(y, y32):.3e}, worst item {loc['item']:.3e}, "
                      f"worst frame {loc['frame']:.3e}, worst channel {loc['chan']:.3e}; loop {t:.1f} ms", flush=True)
        del e32, et
    del engs

    if not a.skip_order:
        # the order figure needs no batch of 32: 4 items
        Bo = 4
        eo = Engine(precision="fp32")
        eo.load_state_dict(W)
        eo.prepare(Bo, T, Lp)
        eo.set_condition(c[:Bo].contiguous(), p[:Bo].contiguous(), mask[:Bo].contiguous())

        def run(solver, steps, order, skip):
            eo.load_sampler(solver, steps, order=order, skip_type=skip)
            x = x_T[:Bo].clone()
            eo.sample(x)
            torch.cuda.synchronize()
            return x.cpu().numpy()
        for skip in ("logSNR", "time_uniform"):
            ref = run("unipc", 200, 3, skip)
            for name, solver, order in CASES:
                errs = [rel_l2(run(solver, n, order, skip), ref) for n in (5, 8, 10, 15, 20)]
                print(f"order {skip} {name}: NFE 5/8/10/15/20 vs 200-step fp32 UniPC-3: " + " ".join(f"{v:.2e}" for v in errs), flush=True)


if __name__ == "__main__":
    main()
