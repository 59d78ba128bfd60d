"""Preemption in a slot loop (fp32 Denoiser, T = 938, Lp = 469): 32 slots of ddim-100 renders (priority 0, all queued at loop step 0)
and `--previews` 10-step UniPC previews (priority 1) arriving every `--every` loop steps from loop step 5 on.
  (p) preempt off: schedule.plan_slots_preemptive with every priority 0 (= schedule.plan_slots): a preview waits for the first render to finish;
  (q) preempt on: the same planner with the priorities: a preview suspends a render (SlotLoop.suspend), runs, and the render resumes.
Both legs drive one SlotLoop step by step with a HIP event after every loop step, so a request's latency is read in loop steps from the plan and
in ms from the events of the run itself (arrival step -> the step its take happens at).  Reported per leg: loop steps and total ms, preview latency
(mean / worst, loop steps and ms), the renders' end (mean / worst loop step) and their delay against leg (p); the same latencies COMPUTED from the
two plans alone (loop steps times the leg's mean ms per loop step).  And the cost of one SlotLoop.suspend + SlotLoop.resume of one slot at this
shape in a loop opened with history 2 (5 planes = 2.4 MB; the condition rebuild included), HIP events around `--calls` pairs.
Usage: python tools/preempt_bench.py [--previews 8] [--every 12] [--reps 2] [--calls 10] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--previews", type=int, default=8)
    ap.add_argument("--every", type=int, default=12)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.schedule import plan_slots_preemptive
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    T, Lp, NB = 938, 469, 32
    dev = torch.device("cuda", 0)
    n = NB + a.previews
    c = torch.from_numpy(hash_normal("pb.c", (NB, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("pb.p", (NB, Lp, 256))).to(dev)
    xT = torch.from_numpy(hash_normal("pb.x", (NB, 100, T))).to(dev)
    den = Denoiser(procedural_state_dict(seed=0), precision="fp32", precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None)
    render, preview = dict(solver="ddim", steps=100, eta=0.0), dict(solver="unipc", steps=10, order=2)
    specs = [render] * NB + [preview] * a.previews
    steps = [s["steps"] for s in specs]
    arrivals = [0] * NB + [5 + a.every * k for k in range(a.previews)]
    priorities = [0] * NB + [1] * a.previews
    plans = {"p_preempt_off": plan_slots_preemptive(steps, NB, arrivals), "q_preempt_on": plan_slots_preemptive(steps, NB, arrivals, priorities)}

    def ends(plan):
        return {i: r for r, take, _, _ in plan for _, i in take}

    def leg(plan):
        """one run of the plan -> ms since loop step 0 at every loop step"""
        loop = den.open_slots(NB, T, Lp)
        marks = [torch.cuda.Event(enable_timing=True)]
        marks[0].record()
        held = {}
        try:
            for r, take, suspend, admit in plan:
                while loop.step < r:
                    loop.run(1)
                    marks.append(torch.cuda.Event(enable_timing=True))
                    marks[-1].record()
                if take:
                    loop.take([b for b, _ in take])
                if suspend:
                    for (_, i, _), q in zip(suspend, loop.suspend([b for b, _, _ in suspend])):
                        held[i] = q
                back = [(b, i) for b, i, d in admit if d > 0]
                if back:
                    loop.resume([b for b, _ in back], [held.pop(i) for _, i in back])
                new = [(b, i) for b, i, d in admit if d == 0]
                if new:
                    loop.admit_group([b for b, _ in new], [c[i % NB] for _, i in new], [p[i % NB] for _, i in new], [xT[i % NB] for _, i in new],
                                     schedules=[specs[i] for _, i in new])
            torch.cuda.synchronize()
        finally:
            loop.close()
        return [marks[0].elapsed_time(m) for m in marks]

    r = {"precision": "fp32", "T": T, "Lp": Lp, "slots": NB, "renders": "32 x ddim-100", "previews": f"{a.previews} x unipc-10 from loop step 5 every {a.every}",
         "reps": a.reps}
    base_end = ends(plans["p_preempt_off"])
    for name, plan in plans.items():
        leg(plan)                                        # warm-up: the graph, the tables
        runs = [leg(plan) for _ in range(a.reps)]
        t = np.median(np.array(runs), axis=0)
        end = ends(plan)
        L = plan[-1][0]
        per_step = float(t[L] / L)
        pv = list(range(NB, n))
        lat_steps = np.array([end[i] - arrivals[i] for i in pv], float)
        lat_ms = np.array([t[end[i]] - t[arrivals[i]] for i in pv], float)
        rend = np.array([end[i] for i in range(NB)], float)
        delay = np.array([end[i] - base_end[i] for i in range(NB)], float)
        r[name] = {"loop_steps": L, "total_ms": [round(float(x[L]), 1) for x in runs], "ms_per_loop_step": round(per_step, 3),
                   "suspensions": sum(len(s) for _, _, s, _ in plan),
                   "preview_latency_steps": {"mean": round(float(lat_steps.mean()), 2), "worst": float(lat_steps.max())},
                   "preview_latency_ms": {"mean": round(float(lat_ms.mean()), 1), "worst": round(float(lat_ms.max()), 1)},
                   "preview_latency_ms_from_plan": {"mean": round(float(lat_steps.mean()) * per_step, 1), "worst": round(float(lat_steps.max()) * per_step, 1)},
                   "render_end_step": {"mean": round(float(rend.mean()), 2), "worst": float(rend.max())},
                   "render_delay_steps_vs_p": {"mean": round(float(delay.mean()), 2), "worst": float(delay.max()), "delayed": int((delay > 0).sum())},
                   "render_delay_ms_from_plan": {"mean": round(float(delay.mean()) * per_step, 1), "worst": round(float(delay.max()) * per_step, 1)}}
    # one suspend + resume of one slot in a full loop with history 2 (5 planes), the condition rebuild of the resume included
    loop = den.open_slots(NB, T, Lp, order3=True)
    try:
        loop.admit_group(list(range(NB)), [c[b] for b in range(NB)], [p[b] for b in range(NB)], [xT[b] for b in range(NB)], schedules=[render] * NB)
        loop.run(2)
        planes = den.engine.state_shape()

        def pair():
            for _ in range(a.calls):
                (q,) = loop.suspend([0])
                loop.resume([0], [q])
        pair()
        torch.cuda.synchronize()
        ts = []
        for _ in range(3):
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            pair()
            s1.record()
            torch.cuda.synchronize()
            ts.append(s0.elapsed_time(s1) / a.calls)
        r["suspend_plus_resume_ms"] = {"state_shape": list(planes), "state_bytes": int(np.prod(planes)) * 4, "runs": [round(x, 4) for x in ts],
                                       "median": round(float(np.median(ts)), 4)}
    finally:
        loop.close()
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
