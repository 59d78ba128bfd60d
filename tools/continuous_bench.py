"""Continuous batching against closed batches (fp16, T = 938, Lp = 469, UniPC order 2): 96 requests, 24 each at 10 / 20 / 30 / 50 steps.
  (g) closed batches, the best the per-item loop can do: three batches of 32 sorted by steps (Denoiser.sample(schedules=), one captured loop of
      20, 30 and 50 steps: 100 loop steps), condition set per batch;
  (s) one slot loop of 32 slots (Denoiser.open_slots) driven by schedule.plan_slots, longest request first: 90 loop steps; every admission sets
      the condition of its slots and admits them, every retirement takes them.
Both legs run on the same Denoiser (same plan options: lengths and prompt lengths on) from ready content / prompt tensors -- the front end and the
vocoder are outside, as in tools/item_schedules_bench.py.  One process, the legs alternating for `--rounds` rounds; per leg and round the median of
`--reps` timed runs after a warm-up run (HIP events around the whole job).  Reported: total ms and slot-step utilisation of both, (g) / (s);
the arrival-to-latent time when the same requests arrive one per loop step (from the two plans in loop steps, times each leg's measured step
time); the admission cost split into condition rebuild, admit and take (ms per call, one slot, HIP events around 20 calls); and the step time of a
full slot loop against the closed per-item loop at B = 32.
The arrival-to-latent figures are COMPUTED, not timed: loop steps from the two plans times each leg's average ms per loop step (admissions
included in the slot leg's average, the front end in neither).
Usage: python tools/continuous_bench.py [--reps 5] [--rounds 3] [--masked] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--masked", action="store_true", help="the Denoiser's masked_fuse / masked_attn / masked_rows / masked_ffn / masked_geglu options on (both legs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.schedule import plan_slots
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    T, Lp, NB = 938, 469, 32
    STEPS = [50] * 24 + [30] * 24 + [20] * 24 + [10] * 24          # the queue, longest first
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("cbb.c", (NB, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("cbb.p", (NB, Lp, 256))).to(dev)
    xT = torch.from_numpy(hash_normal("cbb.x", (NB, 100, T))).to(dev)
    den = Denoiser(procedural_state_dict(seed=0), precision="fp16", precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None,
                   **({k: True for k in ("masked_fuse", "masked_attn", "masked_rows", "masked_ffn", "masked_geglu")} if a.masked else {}))
    spec = lambda n: dict(solver="unipc", steps=n, order=2)      # noqa: E731
    lens, plens = [T] * NB, [Lp] * NB

    def timed(fn, reps):
        ts = []
        for _ in range(reps):
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            fn()
            s1.record()
            torch.cuda.synchronize()
            ts.append(s0.elapsed_time(s1))
        return float(np.median(ts))

    batches = [sorted(STEPS)[k:k + NB] for k in range(0, len(STEPS), NB)]      # sorted by steps: (10 x 24 + 20 x 8), (20 x 16 + 30 x 16), (30 x 8 + 50 x 24)
    closed_steps = sum(max(b) for b in batches)

    def leg_closed():
        for b in batches:
            den.sample(c, p, None, xT, schedules=[spec(n) for n in b], lengths=lens, prompt_lengths=plens)

    events = plan_slots(STEPS, NB)
    slot_steps = events[-1][0]

    def leg_slots():
        loop = den.open_slots(NB, T, Lp)
        for r, take, admit in events:
            if r > loop.step:
                loop.run(r - loop.step)
            if take:
                loop.take([b for b, _ in take])
            if admit:
                k = [b for b, _ in admit]
                loop.admit_group(k, [c[b] for b in k], [p[b] for b in k], [xT[b] for b in k], schedules=[spec(STEPS[i]) for _, i in admit])

    legs = {"g_closed_batches_total_ms": leg_closed, "s_slot_loop_total_ms": leg_slots}
    ms = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            fn()
            torch.cuda.synchronize()
            ms[k].append(timed(fn, a.reps))
    work = sum(STEPS)
    r = {"precision": "fp16", "masked_options": bool(a.masked), "T": T, "Lp": Lp, "slots": NB, "requests": len(STEPS), "reps": a.reps, "rounds": a.rounds,
         "closed_loop_steps": closed_steps, "slot_loop_steps": slot_steps,
         "closed_utilisation": round(work / (closed_steps * NB), 4), "slot_utilisation": round(work / (slot_steps * NB), 4)}
    for k, v in ms.items():
        r[k] = {"rounds": [round(x, 3) for x in v], "median": round(float(np.median(v)), 3), "spread": round(max(v) - min(v), 3)}
    g, s = r["g_closed_batches_total_ms"]["median"], r["s_slot_loop_total_ms"]["median"]
    r["g_over_s"] = round(g / s, 3)
    # latency: request i (the same queue) arrives at loop step i.  Closed batches: batch k starts when its last request has arrived and the
    # batch before it is done, and delivers everything at its end; slots: plan_slots with the arrivals.
    arr = list(range(len(STEPS)))
    done_closed, t_free = [], 0
    for k in range(0, len(STEPS), NB):
        start = max(t_free, arr[min(k + NB, len(STEPS)) - 1])
        t_free = start + max(STEPS[k:k + NB])
        done_closed += [t_free] * len(STEPS[k:k + NB])
    done_slots = {}
    for rr, take, _ in plan_slots(STEPS, NB, arr):
        for _, i in take:
            done_slots[i] = rr
    lat_c = np.array([d - t for d, t in zip(done_closed, arr)], float) * (g / closed_steps)
    lat_s = np.array([done_slots[i] - arr[i] for i in range(len(STEPS))], float) * (s / slot_steps)
    r["latency_ms"] = {"closed_mean": round(float(lat_c.mean()), 1), "closed_worst": round(float(lat_c.max()), 1),
                       "slots_mean": round(float(lat_s.mean()), 1), "slots_worst": round(float(lat_s.max()), 1)}
    # admission cost, one slot at a time, and the step time at full occupancy
    loop = den.open_slots(NB, T, Lp)
    loop.admit_group(list(range(1, NB)), [c[b] for b in range(1, NB)], [p[b] for b in range(1, NB)], [xT[b] for b in range(1, NB)],
                     schedules=[spec(50)] * (NB - 1))
    eng = den.engine
    s_ = torch.cuda.current_stream(dev)
    c1, p1, x1, out1 = c[:1].contiguous(), p[:1].contiguous(), xT[:1].contiguous(), torch.empty_like(xT[:1])
    n_calls = 20
    r["condition_rebuild_ms"] = round(timed(lambda: [eng.set_condition_items([0], c1, p1, None, stream=s_) for _ in range(n_calls)], a.reps) / n_calls, 4)
    tab2 = loop.check_request(spec(2))[1]
    row0 = loop.pool.acquire("bench", tab2.coef)[0]
    eng.write_sampler_rows(row0, tab2.coef, stream=s_)

    def admit_take():
        for _ in range(n_calls):
            eng.admit([0], x1, [[row0, 2, loop.step, 0]], stream=s_)
            eng.sample_steps(2, stream=s_)
            loop.step += 2
            eng.take([0], out1, stream=s_)

    def two_steps():
        for _ in range(n_calls):
            eng.sample_steps(2, stream=s_)
            loop.step += 2
    loop.items = [None] * NB          # (this tool drives the engine itself from here on: 31 slots stay busy for 50 steps, then held)
    both, steps_only = timed(admit_take, a.reps), timed(two_steps, a.reps)
    r["admit_plus_take_ms"] = round((both - steps_only) / n_calls, 4)
    r["slot_loop_step_ms"] = round(steps_only / (2 * n_calls), 4)
    eng.take(list(range(1, NB)), torch.empty_like(xT[1:]), stream=s_)      # (their 50 steps are long behind the loop step)
    torch.cuda.synchronize()
    x = xT.clone()
    den.sample(c, p, None, x, schedules=[spec(20 + (b % 2)) for b in range(NB)], lengths=lens, prompt_lengths=plens)
    r["closed_items_loop_step_ms"] = round(timed(lambda: den.engine.sample(x, use_graph=True), a.reps) / 21, 4)
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
