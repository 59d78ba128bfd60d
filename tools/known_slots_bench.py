"""Cost and use of known frames in the slot loop, on one box in one process, fp16 engine with the masked_* options on:
  (a) the slot loop's step at full occupancy -- 32 slots x 938 frames, Lp = 469, every slot busy with a UniPC-20 request -- in three forms: the
      known-frame form off (ns2vc_sampler_open), on with nothing held, on with `--held` held frames per slot: ms per step;
  (b) a chained job -- eight utterances of 2813 frames with 24 of 938, UniPC-20, overlap 64 -- as closed batches (Denoiser.sample_long on the eight
      plus one Denoiser.sample on the 24) against ONE slot loop of 32 x 938 driven by schedule.plan_chains: ms per job, loop steps, and the
      slot-step utilisation (busy slot-steps / (slots x loop steps)).
The legs alternate for `--rounds` rounds; per leg and round the median of `--reps` timed runs after a warm-up run (HIP events around the run).
Reported per leg: the figures of every round, their median and spread (max - min).  (c), the comparison of bench.py against the parent commit,
is two checkouts and a shell loop, not part of this tool (profiles/known_slots.txt says how it was run).
Usage: python tools/known_slots_bench.py [--reps 5] [--rounds 3] [--legs ab] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from ns2vc_amd.pipeline import MASKED_OPTIONS, Denoiser
    from ns2vc_amd.schedule import plan_chains, plan_chunks
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
    NB, T, Lp, V = 32, 938, 469, a.held
    spec = dict(solver="unipc", steps=a.steps, order=2)
    den = Denoiser(W, precision="fp16", precision_check=None, ln_guard=None, attn_fallback_limit=None, **{k: True for k in MASKED_OPTIONS})
    r = {"solver": f"unipc-{a.steps}", "precision": "fp16", "reps": a.reps, "rounds": a.rounds, "held_frames": V, "options": list(MASKED_OPTIONS)}

    def tensor(tag, shape):
        return torch.from_numpy(hash_normal(tag, shape)).to(dev)

    def timed(fn, per=1.0):
        """median over --reps of fn() -> (start event, stop event), in ms / per"""
        ts = []
        for _ in range(a.reps):
            s0, s1 = fn()
            torch.cuda.synchronize()
            ts.append(s0.elapsed_time(s1))
        return float(np.median(ts)) / per

    def events():
        return torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def summary(v):
        return {"rounds": [round(x, 4) for x in v], "median": round(float(np.median(v)), 4), "spread": round(max(v) - min(v), 4)}

    if "a" in a.legs:
        c, p, x, k = tensor("ksb.c", (NB, 256, T)), tensor("ksb.p", (NB, Lp, 256)), tensor("ksb.x", (NB, 100, T)), tensor("ksb.k", (NB, 100, T))
        mask = np.zeros((T,), dtype=bool)
        mask[:V] = True
        ms = {"off": [], "on_none": [], "on_held": []}
        for _ in range(a.rounds):
            for leg in ms:
                loop = den.open_slots(NB, T, Lp, **(dict(known_frames=True) if leg != "off" else {}))

                def full_loop():
                    hold = dict(knowns=[k[b] for b in range(NB)], known_masks=[mask] * NB) if leg == "on_held" else {}
                    loop.admit_group(list(range(NB)), [c[b] for b in range(NB)], [p[b] for b in range(NB)], [x[b] for b in range(NB)],
                                     schedules=[spec] * NB, **hold)
                    s0, s1 = events()
                    s0.record()
                    loop.run(a.steps)
                    s1.record()
                    loop.take(list(range(NB)))
                    return s0, s1
                full_loop()                         # capture + warm-up
                torch.cuda.synchronize()
                ms[leg].append(timed(full_loop, a.steps))
                loop.close()
        med = {leg: float(np.median(v)) for leg, v in ms.items()}
        r["a_step_at_full_occupancy"] = {"slots": NB, "T": T, "Lp": Lp, **{f"ms_per_step_{leg}": summary(v) for leg, v in ms.items()},
                                         "on_none_minus_off_us": round(1e3 * (med["on_none"] - med["off"]), 2),
                                         "on_held_minus_off_us": round(1e3 * (med["on_held"] - med["off"]), 2)}
        del c, p, x, k

    if "b" in a.legs:
        NL, NS, TL = 8, 24, 2813
        cl, pl, xl = tensor("ksb.lc", (NL, 256, TL)), tensor("ksb.lp", (NL, Lp, 256)), tensor("ksb.lx", (NL, 100, TL))
        cs, ps, xs = tensor("ksb.sc", (NS, 256, T)), tensor("ksb.sp", (NS, Lp, 256)), tensor("ksb.sx", (NS, 100, T))
        kw = dict(solver="unipc", steps=a.steps)
        chunks = plan_chunks(TL, T, V)
        chains = [[a.steps] * len(chunks)] * NL + [[a.steps]] * NS
        plan = plan_chains(chains, NB)
        loop_steps = plan[-1][0]
        util = sum(sum(ch) for ch in chains) / (NB * loop_steps)

        def closed():
            s0, s1 = events()
            s0.record()
            den.sample_long(cl, pl, None, xl, chunk_frames=T, overlap_frames=V, **kw)
            den.sample(cs, ps, None, xs, **kw)
            s1.record()
            return s0, s1

        def slots():
            s0, s1 = events()
            s0.record()
            loop = den.open_slots(NB, T, Lp, known_frames=True)
            out = torch.zeros((NL, 100, TL), device=dev)
            tails = {}
            for step, take, admit in plan:
                if step > loop.step:
                    loop.run(step - loop.step)
                if take:
                    lat = loop.take([b for b, _ in take])
                    for i, (_, (u, j)) in enumerate(take):
                        if u >= NL:
                            continue
                        start, stop = chunks[j]
                        keep = V if j > 0 else 0
                        out[u, :, start + keep:stop] = lat[i, :, keep:stop - start]
                        tails[u] = lat[i, :, stop - start - V:stop - start]
                if admit:
                    cc, pp, xx, kn, km = [], [], [], [], []
                    for _, (u, j) in admit:
                        if u >= NL:
                            cc.append(cs[u - NL])
                            pp.append(ps[u - NL])
                            xx.append(xs[u - NL])
                            kn.append(None)
                            km.append(None)
                            continue
                        start, stop = chunks[j]
                        cc.append(cl[u, :, start:stop])
                        pp.append(pl[u])
                        xx.append(xl[u, :, start:stop])
                        if j == 0:
                            kn.append(None)
                            km.append(None)
                        else:
                            kj = torch.zeros((100, stop - start), device=dev)
                            kj[:, :V] = tails.pop(u)
                            mj = np.zeros((stop - start,), dtype=bool)
                            mj[:V] = True
                            kn.append(kj)
                            km.append(mj)
                    held = any(v is not None for v in kn)
                    loop.admit_group([b for b, _ in admit], cc, pp, xx, schedules=[spec] * len(admit), knowns=kn if held else None,
                                     known_masks=km if held else None)
            loop.close()
            s1.record()
            return s0, s1

        ms = {"closed_batches": [], "slot_loop": []}
        for _ in range(a.rounds):
            for leg, fn in (("closed_batches", closed), ("slot_loop", slots)):
                fn()                                # warm-up (prepare, capture)
                torch.cuda.synchronize()
                ms[leg].append(timed(fn))
        r["b_chained_job"] = {"long": [NL, TL], "short": [NS, T], "Lp": Lp, "chunk_frames": T, "overlap_frames": V, "chunks": chunks, "slots": NB,
                              "ms_per_job_closed_batches": summary(ms["closed_batches"]), "ms_per_job_slot_loop": summary(ms["slot_loop"]),
                              "slot_loop_over_closed": round(float(np.median(ms["slot_loop"])) / float(np.median(ms["closed_batches"])), 3),
                              "loop_steps": loop_steps, "slot_step_utilisation": round(util, 4), "events": len(plan)}
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
