#!/usr/bin/env python3
"""Condense rocprofv3 counter_collection CSVs into the small JSON summaries kept under profiles/ (see pmc_profile.sh).
usage: pmc_summarize.py TAG fetch.csv write.csv mfma.csv OUTDIR"""
import csv, json, os, re, subprocess, sys
from collections import defaultdict

tag, f_fetch, f_write, f_mfma, outdir = sys.argv[1:6]
STEPS_EQUIV = None


def short(name):
    m = re.search(r"ns2vc::(\w+)(<[^(]*>)?\(", name)
    if not m:
        return name.split("(")[0][:60]
    return m.group(1) + (m.group(2) or "").replace("ns2vc::", "")


def family(k):
    if k.startswith(("gemm", "conv3ts", "ffn", "geglu", "rowchain", "splitk")):      # the kind-1 launches of the engine plan (bench.py family table)
        return "implicit_gemm"
    if k.startswith("attn"):
        return "attention"
    if k.startswith(("gn_", "ln_apply_op")):
        return "norm_stats"
    return "other"


def load(path):
    per = defaultdict(lambda: defaultdict(list))       # kernel -> counter -> values
    dur = defaultdict(list)
    seen = set()
    with open(path) as f:
        for r in csv.DictReader(f):
            k = short(r["Kernel_Name"])
            per[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
            if r["Dispatch_Id"] not in seen:
                seen.add(r["Dispatch_Id"])
                dur[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return per, dur


def commit():
    try:
        return subprocess.check_output(["git", "-C", os.path.dirname(os.path.abspath(__file__)), "rev-parse", "--short=12", "HEAD"], text=True).strip()
    except Exception:
        return os.environ.get("NS2VC_COMMIT", "unknown (GPU box has no .git; see the commit that added this file)")


fetch, _ = load(f_fetch)
write, _ = load(f_write)
kern, fam = {}, defaultdict(lambda: {"launches_counted": 0, "fetch": 0.0, "write": 0.0})
for k in sorted(set(fetch) | set(write)):
    fv, wv = fetch.get(k, {}).get("FETCH_SIZE", []), write.get(k, {}).get("WRITE_SIZE", [])
    n = max(len(fv), len(wv), 1)
    fmb, wmb = 2.0 * sum(fv) / 1024.0 / max(len(fv), 1), sum(wv) / 1024.0 / max(len(wv), 1)     # KB -> MB; FETCH_SIZE x2 (gfx950)
    if not k.startswith(("__amd", "at::", "void at::")) and "at::native" not in k:
        kern[k] = {"launches_counted": n, "fetch_mb_per_launch_x2_corrected": round(fmb, 3), "write_mb_per_launch": round(wmb, 3)}
    f = fam[family(k)]
    f["launches_counted"] += n; f["fetch"] += fmb * n; f["write"] += wmb * n
families = {k: {"launches_counted": v["launches_counted"], "fetch_mb_per_launch_x2_corrected": round(v["fetch"] / v["launches_counted"], 3),
                "write_mb_per_launch": round(v["write"] / v["launches_counted"], 3),
                "hbm_mb_per_launch": round((v["fetch"] + v["write"]) / v["launches_counted"], 3)} for k, v in fam.items()}
# launches per step of the engine plan = ffn(10) is the anchor: count of ffn launches / 10 = forward-equivalents in the trace
n_fwd = sum(v["launches_counted"] for k, v in kern.items() if k.startswith("ffn")) / 10.0 or 1.0
total_mb = sum((v["fetch_mb_per_launch_x2_corrected"] + v["write_mb_per_launch"]) * v["launches_counted"] for v in kern.values())
out = {"source": "rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) --kernel-trace -- python bench.py --full --skip-cpu --skip-fp32 --skip-others --skip-strong --steps 4 --warmup 4 --reps 1; "
                 "FETCH_SIZE doubled per MI355X_MICROARCH.md (gfx950 counts 128-B requests as 64 B); KB -> MB /1024",
       "workload": "10 s x batch 32, fp16, unipc", "precision": "fp16", "shape": [32, 938, 469], "commit": commit(),
       "forward_equivalents_in_trace": n_fwd, "hbm_gb_per_step": round(total_mb / n_fwd / 1e3, 3), "families": families, "kernels": kern}
json.dump(out, open(os.path.join(outdir, f"{tag}_pmc_hbm_traffic.json"), "w"), indent=1)

per, dur = load(f_mfma)
mk = {}
for k, c in per.items():
    if "at::" in k or k.startswith("__amd"):
        continue
    n = len(dur[k])
    us = sum(dur[k]) / max(n, 1)
    busy, insts = sum(c.get("SQ_VALU_MFMA_BUSY_CYCLES", [0])), sum(c.get("SQ_INSTS_MFMA", [0]))
    wave, valu = sum(c.get("SQ_WAVE_CYCLES", [0])), sum(c.get("SQ_ACTIVE_INST_VALU", [0]))
    mk[k] = {"launches": n, "avg_us_under_counters": round(us, 2), "SQ_VALU_MFMA_BUSY_CYCLES": busy, "SQ_INSTS_MFMA": insts,
             "mfma_pipe_busy_fraction": round(busy / max(sum(dur[k]) * 1e-6 * 2.4e9 * 1024, 1), 4),
             "valu_active_over_wave_cycles": round(valu / max(wave, 1), 4)}
json.dump({"source": "rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_INSTS_MFMA SQ_ACTIVE_INST_VALU --kernel-trace -- "
                     "python bench.py --full --skip-cpu --skip-fp32 --skip-others --skip-strong --steps 4 --warmup 4 --reps 1",
           "note": "mfma_pipe_busy_fraction = SQ_VALU_MFMA_BUSY_CYCLES (= 32 x MFMA instructions, summed over the chip) / (kernel duration x 2.4 GHz x 1024 SIMDs); "
                   "durations are those measured WITH counters enabled (slower than the plain run)",
           "commit": commit(), "kernels": dict(sorted(mk.items(), key=lambda kv: -kv[1]["launches"] * kv[1]["avg_us_under_counters"]))},
          open(os.path.join(outdir, f"{tag}_pmc_mfma_util.json"), "w"), indent=1)
print("wrote", tag, "summaries; HBM GB/step", out["hbm_gb_per_step"])
