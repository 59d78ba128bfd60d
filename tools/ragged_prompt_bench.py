"""Cost of a conversion job whose segments use reference clips of different lengths (32 segments at T = 938, eight clips with prompt
lengths spread over 235..469, four segments per clip; UniPC-20, fp16, captured loop), three ways:
  (a) one B = 32 batch, prompts padded to 469 rows with per-item prompt lengths (ns2vc_unet_set_prompt_lengths), option masked_attn off
      (attn2 reads the bias row);
  (b) the same with masked_attn on (attn2 takes the table as k_lens: the key tiles past an item's prompt are skipped);
  (c) what an engine without prompt lengths must do with the same segments: one batch per prompt length, here eight B = 4 batches.
Per leg: ms per solver step (sum of the legs' loops / steps; median of `--reps` timed loops after a warm-up loop, condition set outside the
timing) and the time of set_condition (median of `--reps`, HIP events).  A library without ns2vc_unet_set_prompt_lengths runs leg (c) only.
Usage: python tools/ragged_prompt_bench.py [--reps 5] [--out FILE]"""
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
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B, T, Lp, per_clip = 32, 938, 469, 4
    clip_lens = [int(v) for v in np.linspace(235, 469, B // per_clip).round()]
    plens = [clip_lens[b // per_clip] for b in range(B)]
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("rpb.c", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("rpb.p", (B, Lp, 256))).to(dev)
    for b, P in enumerate(plens):
        p[b, P:] = 0.0
    xT = torch.from_numpy(hash_normal("rpb.x", (B, 100, T))).to(dev)
    e = Engine(precision="fp16")
    e.load_state_dict(procedural_state_dict(seed=0))
    has_plens = hasattr(e, "set_prompt_lengths")

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

    def leg(sl, lp, lengths):
        """(loop ms, set_condition ms) of the items `sl` with prompts of `lp` rows"""
        cb, pb, x0 = c[sl].contiguous(), p[sl, :lp].contiguous(), xT[sl].contiguous()
        if e.shape != (cb.shape[0], T, lp):
            e.prepare(cb.shape[0], T, lp)
            e.load_sampler("unipc", a.steps)
        if has_plens:
            e.set_prompt_lengths(lengths)
        e.set_condition(cb, pb, None)
        x = x0.clone()
        e.sample(x, use_graph=True)            # capture + warm-up
        torch.cuda.synchronize()

        def loop():
            x.copy_(x0)
            e.sample(x, use_graph=True)
        return timed(loop), timed(lambda: e.set_condition(cb, pb, None))

    r = {"segments": B, "T": T, "prompt_lengths": clip_lens, "solver": f"unipc-{a.steps}", "precision": "fp16"}
    if has_plens:
        for name, attn in (("a_bias", False), ("b_klens", True)):
            e.set_option("masked_attn", attn)
            ms, cond = leg(slice(None), Lp, plens)
            r[name] = {"ms_per_step": round(ms / a.steps, 4), "set_condition_ms": round(cond, 3), "launches": e.launches()[0]}
        e.set_option("masked_attn", False)
    ms = cond = 0.0
    for k, P in enumerate(clip_lens):
        m, s = leg(slice(k * per_clip, (k + 1) * per_clip), P, None)
        ms, cond = ms + m, cond + s
    r["c_per_prompt_length"] = {"ms_per_step": round(ms / a.steps, 4), "set_condition_ms": round(cond, 3), "batches": len(clip_lens)}
    e.close()
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
