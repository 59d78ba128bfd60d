"""Cost of known frames in the captured loop, two measurements on one box in one process:
  (a) the bench shape -- B = 32, T = 938, Lp = 469, UniPC-20, fp16 engine -- with no hold against 64 held frames per item
      (ns2vc_sampler_set_known; the first 64 frames, as a chunk of sample_long holds them): ms per step and launches per step;
  (b) eight 30 s items (T = 2813): Denoiser.sample_long(chunk_frames=938, overlap_frames=64) -- four chained batches of 938 / 938 / 938 / 191
      frames -- against ONE sample call at T = 2813, total ms per job, with the launches per step of every shape.
The legs alternate (off, on, off, on, ...) for `--rounds` rounds; per leg and round the median of `--reps` timed loops after a warm-up loop (HIP
events around the whole loop, condition set outside for (a)).  Reported: per leg the figures of every round, their median and spread (max - min),
and on - off beside off's spread.  The comparison is always the same build with the hold off.
"Launches per step" are COMPUTED, not counted from the captured graph: the launches of the per-step plan (ns2vc_unet_num_launches) plus one for
the solver update, plus one for the hold launch where a hold is set (`launches_per_step_how` in the output says so).
Usage: python tools/known_frames_bench.py [--reps 5] [--rounds 3] [--legs ab] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from ns2vc_amd.engine import Engine
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--held", type=int, default=64)
    ap.add_argument("--legs", default="ab")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    W = procedural_state_dict(seed=0)
    r = {"solver": f"unipc-{a.steps}", "precision": "fp16", "reps": a.reps, "rounds": a.rounds, "held_frames_per_item": a.held,
         "launches_per_step_how": "computed: per-step plan launches + 1 (solver update) + 1 under a hold; not counted from the captured graph"}

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

    def summary(v):
        return {"rounds": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4)}

    if "a" in a.legs:
        T, Lp, NB = 938, 469, 32
        c = torch.from_numpy(hash_normal("kfb.c", (NB, 256, T))).to(dev)
        p = torch.from_numpy(hash_normal("kfb.p", (NB, Lp, 256))).to(dev)
        xT = torch.from_numpy(hash_normal("kfb.x", (NB, 100, T))).to(dev)
        k = torch.from_numpy(hash_normal("kfb.k", (NB, 100, T))).to(dev)
        mask = np.zeros((NB, T), dtype=bool)
        mask[:, :a.held] = True
        e = Engine(precision="fp16")
        e.load_state_dict(W)
        e.prepare(NB, T, Lp)
        e.load_sampler("unipc", a.steps)
        e.set_condition(c, p, None)
        x = xT.clone()

        def loop():
            x.copy_(xT)
            e.sample(x, use_graph=True)

        ms = {"off": [], "on": []}
        for _ in range(a.rounds):
            for leg in ("off", "on"):
                if leg == "on":
                    e.set_known(k, mask)
                else:
                    e.set_known(None, None)
                loop()                              # capture + warm-up
                torch.cuda.synchronize()
                ms[leg].append(timed(loop, a.steps))
        r["a_bench_shape"] = {"B": NB, "T": T, "Lp": Lp, "ms_per_step_off": summary(ms["off"]), "ms_per_step_on": summary(ms["on"]),
                              "on_minus_off_us": round(1e3 * (float(np.median(ms["on"])) - float(np.median(ms["off"]))), 2),
                              "launches_per_step_off": e.launches()[0] + 1, "launches_per_step_on": e.launches()[0] + 2,
                              "graph_captures": e.graph_captures()}
        e.close()
        del c, p, xT, k, x

    if "b" in a.legs:
        T, Lp, NB, chunk, V = 2813, 469, 8, 938, 64
        c = torch.from_numpy(hash_normal("kfb.lc", (NB, 256, T))).to(dev)
        p = torch.from_numpy(hash_normal("kfb.lp", (NB, Lp, 256))).to(dev)
        xT = torch.from_numpy(hash_normal("kfb.lx", (NB, 100, T))).to(dev)
        den = Denoiser(W, precision="fp16")
        kw = dict(solver="unipc", steps=a.steps)
        launches = {}

        def one():
            den.sample(c, p, None, xT, **kw)
            launches[f"T={den._shape[1]}"] = den.engine.launches()[0] + 1

        def long():
            den.sample_long(c, p, None, xT, chunk_frames=chunk, overlap_frames=V, **kw)
            launches[f"T={den._shape[1]} (last chunk, held)"] = den.engine.launches()[0] + 2

        ms = {"one_call": [], "sample_long": []}
        for _ in range(a.rounds):
            for leg, fn in (("one_call", one), ("sample_long", long)):
                fn()                                # warm-up (the first also runs the once-per-weights checks)
                torch.cuda.synchronize()
                ms[leg].append(timed(fn, 1))
        from ns2vc_amd.schedule import plan_chunks
        r["b_long_utterances"] = {"B": NB, "T": T, "Lp": Lp, "chunk_frames": chunk, "overlap_frames": V, "chunks": plan_chunks(T, chunk, V),
                                  "ms_per_job_one_call": summary(ms["one_call"]), "ms_per_job_sample_long": summary(ms["sample_long"]),
                                  "sample_long_over_one_call": round(float(np.median(ms["sample_long"])) / float(np.median(ms["one_call"])), 3),
                                  "launches_per_step": launches}
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
