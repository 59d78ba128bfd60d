"""Stochastic samplers at the bench shape (10 s x batch 32, Lp 469, procedural weights): speed and precision.

  speed      ms/step of the captured fp16 loop for DDPM-1000, DDIM-100 (eta 0 and 1) and UniPC-20 (same box, same process), and the
             reference's path for DDPM: the drop-in module called eagerly per step with the isnan check, the posterior update and a
             torch.randn_like per step (model.py p_sample), timed over --eager-steps steps
  precision  the fp16 loop with tail = 0, 1, 2 fp32 evaluations against the fp32 engine on the same x_T and seeds: rel-L2, worst item,
             worst frame / channel (tests/util.py local_errors)

python tools/stochastic_bench.py [--skip-precision] [--eager-steps 50]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ns2vc_amd import schedule as S  # noqa: E402
from ns2vc_amd.engine import Engine, Event  # noqa: E402
from ns2vc_amd.weights import hash_normal, procedural_state_dict  # noqa: E402
from util import local_errors, rel_l2  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-precision", action="store_true")
    ap.add_argument("--eager-steps", type=int, default=50)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    B, T, Lp = 32, 938, 469
    W = procedural_state_dict(seed=0)
    c = torch.from_numpy(hash_normal("stb.c", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("stb.p", (B, Lp, 256))).to(dev)
    mask = torch.ones((B, Lp), dtype=torch.uint8, device=dev)
    x_T = torch.from_numpy(hash_normal("stb.x", (B, 100, T))).to(dev)
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(1000)
    b64 = S.linear_betas(1000, np.float64)
    cases = [("ddpm", 1000, 0.0), ("ddim", 100, 0.0), ("ddim", 100, 1.0), ("unipc", 20, 0.0)]

    def engine(prec):
        e = Engine(precision=prec)
        e.load_state_dict(W)
        e.prepare(B, T, Lp)
        e.set_condition(c, p, mask)
        return e

    def load(e, solver, steps, eta):
        if solver in S.DISCRETE_SOLVERS:
            e.load_sampler(solver, steps, b64, eta=eta)
        else:
            e.load_sampler(solver, steps)
        e.set_seeds(seeds)

    # ---- speed
    e16 = engine("fp16")
    for solver, steps, eta in cases:
        load(e16, solver, steps, eta)
        x = x_T.clone()
        e16.sample(x)                      # capture + warm-up
        ts = []
        for _ in range(3):
            x = x_T.clone()
            t0, t1 = Event(), Event()
            t0.record(None)
            e16.sample(x)
            t1.record(None)
            ts.append(t0.elapsed_ms(t1) / steps)
        print(f"speed {solver}{steps} eta {eta:g} fp16 captured: {np.median(ts):.3f} ms/step (runs {' '.join(f'{v:.3f}' for v in ts)})", flush=True)
    del e16

    # the reference's DDPM path: drop-in module, eager, per-step isnan + randn_like
    from unet1d import UNet1DConditionModel
    m = UNet1DConditionModel(in_channels=356, out_channels=100, block_out_channels=(128, 256, 384, 512), norm_num_groups=8, cross_attention_dim=256,
                             attention_head_dim=8, addition_embed_type="text", resnet_time_scale_shift="scale_shift", engine_precision="fp16")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in W.items()}, strict=True)
    m = m.to(dev).eval()
    bf = S._discrete_buffers(b64)
    c1, c2 = torch.from_numpy(bf["posterior_mean_coef1"]).to(dev), torch.from_numpy(bf["posterior_mean_coef2"]).to(dev)
    lv = torch.from_numpy(bf["posterior_log_variance_clipped"]).to(dev)
    bm = mask.bool()

    def eager(n):
        x = x_T.clone()
        with torch.no_grad():
            for k in range(n):
                t = 999 - k
                assert not torch.isnan(x).any()
                x0 = m(torch.cat([x, c], dim=1), torch.full((B,), t, device=dev, dtype=torch.long), p, encoder_attention_mask=bm).sample
                x = c1[t] * x0 + c2[t] * x + (0.5 * lv[t]).exp() * torch.randn_like(x)
        return x
    eager(3)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eager(a.eager_steps)
    torch.cuda.synchronize()
    print(f"speed ddpm reference path (drop-in module eager, isnan + randn_like per step): {(time.perf_counter() - t0) / a.eager_steps * 1e3:.3f} ms/step "
          f"over {a.eager_steps} steps", flush=True)
    del m

    if a.skip_precision:
        return
    # ---- precision: fp16 with tail 0, 1, 2 against the fp32 engine
    e32, e16, et = engine("fp32"), engine("fp16"), engine("fp32")
    for solver, steps, eta in cases[:2]:
        load(e32, solver, steps, eta)
        y32 = x_T.clone()
        e32.sample(y32)
        y32 = x_T.clone()
        t0, t1 = Event(), Event()
        t0.record(None)
        e32.sample(y32)
        t1.record(None)
        print(f"speed {solver}{steps} fp32 captured: {t0.elapsed_ms(t1) / steps:.3f} ms/step", flush=True)
        y32 = y32.cpu().numpy()
        for tail in (0, 1, 2):
            load(e16, solver, steps, eta)
            load(et, solver, steps, eta)
            x = x_T.clone()
            e16.sample(x, tail=et if tail else None, tail_steps=tail)      # (captures the graphs)
            x = x_T.clone()
            t0, t1 = Event(), Event()
            t0.record(None)
            e16.sample(x, tail=et if tail else None, tail_steps=tail)
            t1.record(None)
            ms = t0.elapsed_ms(t1)
            y = x.cpu().numpy()
            per_item = [rel_l2(y[b], y32[b]) for b in range(B)]
            loc = local_errors(y, y32)
            print(f"precision {solver}{steps} fp16 tail {tail}: rel-L2 {rel_l2(y, y32):.3e}, worst item {max(per_item):.3e}, "
                  f"worst frame {loc['frame']:.3e}, worst channel {loc['chan']:.3e}; loop {ms:.1f} ms", flush=True)


if __name__ == "__main__":
    main()
