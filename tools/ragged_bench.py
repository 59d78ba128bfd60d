"""Throughput of a mixed-length conversion job (32 segments, lengths spread over 470..938 frames, UniPC-20, fp16, captured loop), three ways:
  (a) dense     -- one B = 32 batch, every segment 938 frames (the benchmark's best case);
  (b) ragged    -- one B = 32 batch padded to 938 with per-item lengths (ns2vc_unet_set_lengths);
  (c) per-shape -- equal-shape grouping without padding, which for 32 distinct lengths is 32 batch-1 loops.
--masked-fuse adds (b') -- leg (b) with the engine option masked_fuse on -- in the same process, `--alternate` times in turn with (a) and (b), the order rotating;
--masked-attn (with --masked-fuse) adds (b'') -- leg (b') with the engine option masked_attn on as well -- to that rotation;
--masked-rows (with --masked-fuse --masked-attn) adds (b3) -- leg (b'') with the engine option masked_rows on as well -- to that rotation;
--masked-ffn (with --masked-fuse --masked-attn --masked-rows) adds (b4) -- leg (b3) with the engine option masked_ffn on as well -- to that rotation;
--masked-geglu (with --masked-fuse --masked-attn --masked-rows --masked-ffn) adds (b5) -- leg (b4) with the engine option masked_geglu on as well -- to that rotation;
--masked-attn-resident (with the five above) adds (b6) -- leg (b5) with the engine option masked_attn_resident on as well -- to that rotation;
--skip-per-shape leaves (c) out.
Each figure is the median of `--reps` timed sampling loops (hipGraph replays, condition set outside the timing) after a warm-up loop.
Usage: python tools/ragged_bench.py [--reps 5] [--out FILE]"""
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
    ap.add_argument("--masked-fuse", action="store_true", help="also run leg (b) with the option masked_fuse on")
    ap.add_argument("--masked-attn", action="store_true", help="with --masked-fuse: also run leg (b') with the option masked_attn on")
    ap.add_argument("--masked-rows", action="store_true", help="with --masked-fuse --masked-attn: also run leg (b'') with the option masked_rows on")
    ap.add_argument("--masked-ffn", action="store_true", help="with --masked-fuse --masked-attn --masked-rows: also run leg (b3) with the option masked_ffn on")
    ap.add_argument("--masked-geglu", action="store_true", help="with --masked-fuse --masked-attn --masked-rows --masked-ffn: also run leg (b4) with the option masked_geglu on")
    ap.add_argument("--masked-attn-resident", action="store_true",
                    help="with --masked-fuse --masked-attn --masked-rows --masked-ffn --masked-geglu: also run leg (b5) with the option masked_attn_resident on")
    ap.add_argument("--alternate", type=int, default=3, help="repetitions of (a), (b), (b') in turn (with --masked-fuse)")
    ap.add_argument("--skip-per-shape", action="store_true")
    a = ap.parse_args()
    B, T, Lp = 32, 938, 469
    lens = [int(v) for v in np.linspace(470, 938, B).round()]
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("rb.c", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("rb.p", (1, Lp, 256))).expand(B, -1, -1).contiguous().to(dev)
    xT = torch.from_numpy(hash_normal("rb.x", (B, 100, T))).to(dev)
    e = Engine(precision="fp16")
    e.load_state_dict(procedural_state_dict(seed=0))
    fused_now = attn_now = rows_now = ffn_now = geglu_now = False      # the engine's masked_fuse / masked_attn / masked_rows / masked_ffn / masked_geglu options as last set
    ares_now = False                                                   # ... and masked_attn_resident

    def loop_ms(bsz, tl, lengths=None, sl=slice(None), fuse=False, attn=False, rows=False, ffn=False, geglu=False, ares=False):
        nonlocal fused_now, attn_now, rows_now, ffn_now, geglu_now, ares_now
        if fused_now != fuse:
            e.set_option("masked_fuse", fuse)        # (drops the plan: prepared again below)
            fused_now = fuse
        if attn_now != attn:
            e.set_option("masked_attn", attn)
            attn_now = attn
        if rows_now != rows:
            e.set_option("masked_rows", rows)
            rows_now = rows
        if ffn_now != ffn:
            e.set_option("masked_ffn", ffn)
            ffn_now = ffn
        if geglu_now != geglu:
            e.set_option("masked_geglu", geglu)
            geglu_now = geglu
        if ares_now != ares:
            e.set_option("masked_attn_resident", ares)
            ares_now = ares
        if e.shape != (bsz, tl, Lp):
            e.prepare(bsz, tl, Lp)
            e.load_sampler("unipc", a.steps)
        e.set_lengths(lengths)
        e.set_condition(c[sl, :, :tl].contiguous(), p[sl].contiguous(), None)
        x0 = xT[sl, :, :tl].contiguous()
        x = x0.clone()
        e.sample(x, use_graph=True)            # capture + warm-up
        ts = []
        for _ in range(a.reps):
            x.copy_(x0)
            s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s0.record()
            e.sample(x, use_graph=True)
            s1.record()
            torch.cuda.synchronize()
            ts.append(s0.elapsed_time(s1))
        return float(np.median(ts))

    dense = loop_ms(B, T)
    ragged = loop_ms(B, T, lens)
    alt = []
    if a.masked_fuse:
        legs = {"a": lambda: loop_ms(B, T), "b": lambda: loop_ms(B, T, lens), "b_fused": lambda: loop_ms(B, T, lens, fuse=True)}
        order = ["a", "b", "b_fused"]
        if a.masked_attn:
            legs["b_fused_attn"] = lambda: loop_ms(B, T, lens, fuse=True, attn=True)
            order.append("b_fused_attn")
            if a.masked_rows:
                legs["b_fused_attn_rows"] = lambda: loop_ms(B, T, lens, fuse=True, attn=True, rows=True)
                order.append("b_fused_attn_rows")
                if a.masked_ffn:
                    legs["b_fused_attn_rows_ffn"] = lambda: loop_ms(B, T, lens, fuse=True, attn=True, rows=True, ffn=True)
                    order.append("b_fused_attn_rows_ffn")
                    if a.masked_geglu:
                        legs["b_fused_attn_rows_ffn_geglu"] = lambda: loop_ms(B, T, lens, fuse=True, attn=True, rows=True, ffn=True, geglu=True)
                        order.append("b_fused_attn_rows_ffn_geglu")
                        if a.masked_attn_resident:
                            legs["b_all_attn_resident"] = lambda: loop_ms(B, T, lens, fuse=True, attn=True, rows=True, ffn=True, geglu=True, ares=True)
                            order.append("b_all_attn_resident")
        for i in range(a.alternate):             # the order rotates, so that a drift of the clocks does not favour one leg
            k0 = i % len(order)
            rot = order[k0:] + order[:k0]
            rep = {k: round(legs[k](), 3) for k in rot}
            rep["order"] = rot
            alt.append(rep)
        loop_ms(B, T)                            # (option off again for leg (c))
    per = 0.0 if a.skip_per_shape else sum(loop_ms(1, L, None, slice(i, i + 1)) for i, L in enumerate(lens))
    e.close()
    r = {"segments": B, "lengths": [min(lens), max(lens)], "solver": f"unipc-{a.steps}", "precision": "fp16",
         "a_dense_ms": round(dense, 3), "b_ragged_ms": round(ragged, 3), "c_per_shape_ms": round(per, 3),
         "b_over_a": round(ragged / dense, 3), "c_over_b": round(per / ragged, 2),
         "ms_per_step": {"a": round(dense / a.steps, 3), "b": round(ragged / a.steps, 3), "c": round(per / a.steps, 3)}}
    if alt:
        med = {k: float(np.median([x[k] for x in alt])) for k in alt[0] if k != "order"}
        r["alternating_ms"] = alt
        r["fused"] = {"b_fused_ms": round(med["b_fused"], 3), "b_fused_over_a": round(med["b_fused"] / med["a"], 3), "b_fused_over_b": round(med["b_fused"] / med["b"], 3),
                      "ms_per_step": {k: round(v / a.steps, 3) for k, v in med.items()}}
        if "b_fused_attn" in med:
            r["fused"].update({"b_fused_attn_ms": round(med["b_fused_attn"], 3), "b_fused_attn_over_a": round(med["b_fused_attn"] / med["a"], 3),
                               "b_fused_attn_over_b_fused": round(med["b_fused_attn"] / med["b_fused"], 3)})
        if "b_fused_attn_rows" in med:
            r["fused"].update({"b_fused_attn_rows_ms": round(med["b_fused_attn_rows"], 3),
                               "b_fused_attn_rows_over_a": round(med["b_fused_attn_rows"] / med["a"], 3),
                               "b_fused_attn_rows_over_b_fused_attn": round(med["b_fused_attn_rows"] / med["b_fused_attn"], 3)})
        if "b_fused_attn_rows_ffn" in med:
            r["fused"].update({"b_fused_attn_rows_ffn_ms": round(med["b_fused_attn_rows_ffn"], 3),
                               "b_fused_attn_rows_ffn_over_a": round(med["b_fused_attn_rows_ffn"] / med["a"], 3),
                               "b_fused_attn_rows_ffn_over_b_fused_attn_rows": round(med["b_fused_attn_rows_ffn"] / med["b_fused_attn_rows"], 3)})
        if "b_fused_attn_rows_ffn_geglu" in med:
            r["fused"].update({"b_fused_attn_rows_ffn_geglu_ms": round(med["b_fused_attn_rows_ffn_geglu"], 3),
                               "b_fused_attn_rows_ffn_geglu_over_a": round(med["b_fused_attn_rows_ffn_geglu"] / med["a"], 3),
                               "b_fused_attn_rows_ffn_geglu_over_b_fused_attn_rows_ffn": round(med["b_fused_attn_rows_ffn_geglu"] / med["b_fused_attn_rows_ffn"], 3)})
        if "b_all_attn_resident" in med:
            r["fused"].update({"b_all_attn_resident_ms": round(med["b_all_attn_resident"], 3),
                               "b_all_attn_resident_over_a": round(med["b_all_attn_resident"] / med["a"], 3),
                               "b_all_attn_resident_over_b_fused_attn_rows_ffn_geglu": round(med["b_all_attn_resident"] / med["b_fused_attn_rows_ffn_geglu"], 3)})
    line = json.dumps(r)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
