"""What the option masked_attn_resident gives a serving loop (fp16, UniPC order 2, all five other masked_* options on):
  (s) a slot loop of 32 slots (Denoiser.open_slots, T = 938, Lp = 469) at full occupancy -- every request `--frames` frames (default 938: the length
      tables mask nothing) -- timed as ms per loop step (HIP events around `--steps` captured steps, median of `--reps`), the option off and on in turn
      for `--rounds` rounds in one process;
  (p) after each leg of the last round, ns2vc_unet_profile_forward of the same plan: the per-launch time of every `.sdpa` launch, by name, and their sum.
--frames-lo L spreads the requests' lengths evenly over L .. `--frames` instead (the ragged case).
Usage: python tools/masked_attn_resident_bench.py [--reps 5] [--rounds 3] [--steps 10] [--frames 938] [--frames-lo L] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10, help="loop steps per timed run")
    ap.add_argument("--frames", type=int, default=938)
    ap.add_argument("--frames-lo", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from ns2vc_amd import _lib
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    lib = _lib.load()
    T, Lp, NB = 938, 469, 32
    lens = [a.frames] * NB if a.frames_lo is None else [int(v) for v in np.linspace(a.frames_lo, a.frames, NB).round()]
    total = 4 + a.steps * a.reps                   # warm-up (capture) + the timed runs: every request stays active throughout
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("marb.c", (NB, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("marb.p", (NB, Lp, 256))).to(dev)
    xT = torch.from_numpy(hash_normal("marb.x", (NB, 100, T))).to(dev)
    den = Denoiser(procedural_state_dict(seed=0), precision="fp16", precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None,
                   **{k: True for k in ("masked_fuse", "masked_attn", "masked_rows", "masked_ffn", "masked_geglu")})

    def leg(on, profile):
        den.set_option("masked_attn_resident", on)
        n0 = lib.ns2vc_debug_attn_resident_lens_launches()
        loop = den.open_slots(NB, T, Lp)
        loop.admit_group(list(range(NB)), [c[b] for b in range(NB)], [p[b] for b in range(NB)], [xT[b] for b in range(NB)], lengths=lens,
                         schedules=[dict(solver="unipc", steps=total, order=2)] * NB)
        loop.run(4)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            loop.run(a.steps)
            s1.record()
            torch.cuda.synchronize()
            ts.append(s0.elapsed_time(s1) / a.steps)
        made = lib.ns2vc_debug_attn_resident_lens_launches() - n0
        loop.close()
        torch.cuda.synchronize()
        prof = None
        if profile:                                # (the plan and the length tables of the loop are still the engine's)
            ms = den.engine.profile_forward(reps=20)
            prof = {name: round(float(ms[i]) * 1e3, 2) for i, (name, *_) in enumerate(den.engine.op_info(0)) if name.endswith(".sdpa")}
            print(json.dumps({"leg": "on" if on else "off", "ms_per_loop_step": ts, "sdpa_us": prof}), flush=True)      # (kept if a later leg fails)
        return float(np.median(ts)), made, den.engine.launches()[0], prof

    r = {"precision": "fp16", "slots": NB, "T": T, "Lp": Lp, "lengths": [min(lens), max(lens)], "steps_per_run": a.steps, "reps": a.reps,
         "rounds": a.rounds, "ms_per_loop_step": {"off": [], "on": []}}
    for i in range(a.rounds):
        for on in ((False, True) if i % 2 == 0 else (True, False)):      # the order alternates
            ms, made, launches, prof = leg(on, i == a.rounds - 1)
            k = "on" if on else "off"
            r["ms_per_loop_step"][k].append(round(ms, 4))
            r.setdefault("launches_on_the_masked_resident_kernel", {})[k] = made
            r.setdefault("launches_per_step", {})[k] = launches
            if prof is not None:
                r.setdefault("sdpa_us", {})[k] = prof
                r.setdefault("sdpa_sum_us", {})[k] = round(sum(prof.values()), 1)
    med = {k: float(np.median(v)) for k, v in r["ms_per_loop_step"].items()}
    r["median_ms_per_loop_step"] = {k: round(v, 4) for k, v in med.items()}
    r["spread_ms"] = {k: round(max(v) - min(v), 4) for k, v in r["ms_per_loop_step"].items()}
    r["on_minus_off_ms"] = round(med["on"] - med["off"], 4)
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
