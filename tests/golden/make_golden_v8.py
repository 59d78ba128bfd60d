"""Golden vectors of the reference's own x0 correction (``correcting_x0_fn="dynamic_thresholding"``) -> golden_v8.npz.

BUILD CONTAINER ONLY (reads the reference checkout).  ``sampler.uni_pc.UniPC`` and ``sampler.dpm_solver.DPM_Solver(algorithm_type=
"dpmsolver++")`` are CONSTRUCTED with ``correcting_x0_fn="dynamic_thresholding", thresholding_max_val=..., dynamic_thresholding_ratio=...``
(uni_pc.py:236-294, dpm_solver.py:338-442) and run multistep in float32, one B = 1 call per item, each item at its own length:

  g17.*  the synthetic x0 model of v5 through ``model_wrapper(model_type="x_start")``
  g18.*  the guided synthetic noise model of v7 through ``model_wrapper(model_type="noise", guidance_type="classifier-free", ...)``

Items are (1, C, L_b) with C = 5 and L = (8, 7, 5), so n_b = 40, 35, 25 elements: ratio * (n_b - 1) is fractional for the first two at both
ratios of the grid and the integer 18 for the third at ratio 0.75 (and n_b - 1 itself at ratio 1).  ``max_val`` comes from the model's own |x0|
quantiles along the UNCORRECTED loop (UniPC order 2, time_uniform; recorded here as <prefix>.maxval.q75_plain / .q90_plain / .absmax_plain).
The reference runs one item per call, so max_val is per item, <prefix>.maxval of shape (legs, items): leg
  a  half the smallest 0.75-quantile: the threshold is the quantile on every step, 1 - ratio of the elements are clamped every time;
  b  per item, halfway between its 0.9-quantile and its maximum of |x0| at the FIRST evaluation (the same in every case: x_T and t_T are
     shared): max_val is the threshold there and clamps the item's largest elements at the first step.  This model's |x0| does not decay
     along the loop (its maximum hovers around 0.9), so a max_val that bites early and then stops for good does not exist for it; where leg
     b bites after the first step is recorded per case (``.clamped``), and the report counts the evaluations;
  c  1.5 x the largest |x0| anywhere: nothing is ever clamped, only the division by max_val acts.
Every case records, per item and evaluation, the share of elements beyond the threshold (``.clamped``), so that a test can tell that legs a
and b do clamp.  What is committed is data only: x_T, the conditions, max_val per leg, model times, clamped shares and final latents.  The
report also holds the relative L2 of ``schedule.run_table_numpy(correct_x0=...)`` against every case, the figures the CPU test's bound cites.

Run: python tests/golden/make_golden_v8.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden_v6 import REF, save_npz_deterministic  # noqa: E402
sys.path.insert(0, REF)
from ns2vc_amd import schedule as S  # noqa: E402

C, LENS, STEPS = 5, (8, 7, 5), 8
LEGS = ("a", "b", "c")
# (solver, order, skip_type, ratio, leg, extra options)
CASES17 = [(sv, o, "time_uniform", r, leg, {}) for sv in ("unipc", "dpmsolver++") for o in (1, 2, 3) for r in (0.9, 0.75) for leg in LEGS]
CASES17 += [(sv, 3, "logSNR", 0.9, "a", {"denoise_to_zero": True}) for sv in ("unipc", "dpmsolver++")]
CASES17 += [(sv, 2, "logSNR", r, "a", {}) for sv in ("unipc", "dpmsolver++") for r in (0.995, 1.0)]
# (solver, order, skip_type, ratio, leg, scale)
CASES18 = [(sv, o, "logSNR", 0.9, leg, 2.5) for sv in ("unipc", "dpmsolver++") for o in (1, 2, 3) for leg in ("a", "b")]
CASES18 += [(sv, 2, "logSNR", 0.75, "a", 7.0) for sv in ("unipc", "dpmsolver++")]


def tag17(solver, order, skip, ratio, leg, extra):
    return (f"{'unipc' if solver == 'unipc' else 'dpmpp'}{order}_{skip}_r{ratio:g}_{leg}" + "".join(f"_{k}" for k in sorted(extra))).replace(".", "p")


def tag18(solver, order, skip, ratio, leg, scale):
    return f"{'unipc' if solver == 'unipc' else 'dpmpp'}{order}_{skip}_r{ratio:g}_{leg}_s{scale:g}".replace(".", "p")


def synthetic_x0(x, t, cond=None):
    """the stand-in denoiser of v4 / v5 (cond None) and v7: x (1, C, L), t (1,), cond (1, C, 1) -> x0"""
    tt = t.to(x.dtype).reshape(-1, 1, 1)
    return 0.9 * torch.tanh(x if cond is None else x + cond) + 0.05 * torch.cos(0.01 * tt)


def run_reference(M, betas, solver, order, skip, ratio, max_val, x_T, extra=None, guide=None, spy_ratio=1.0):
    """one B = 1 loop of the reference -> (latent, model times in call order, and per evaluation: the share of elements beyond the threshold, the
    |x0| quantile, the |x0| maximum).  ratio None: the uncorrected loop (quantile at spy_ratio).  guide = (cond, uncond, scale): the guided noise model."""
    extra = extra or {}
    times, seen = [], []
    ns = M.NoiseScheduleVP(schedule="discrete", betas=betas)
    corr = {} if ratio is None else dict(correcting_x0_fn="dynamic_thresholding", thresholding_max_val=max_val, dynamic_thresholding_ratio=ratio)
    if guide is None:
        def x0_model(x, t):
            times.append(float(t.reshape(-1)[0]))
            return synthetic_x0(x, t)
        model_fn = M.model_wrapper(x0_model, ns, model_type="x_start")
    else:
        cond, uncond, scale = guide

        def eps_model(x, t_input, c):      # model_type="noise": t_input = (t_continuous - 1/N) * N  (uni_pc.py:170-179)
            times.append(float(t_input.reshape(-1)[0]))
            t_cont = t_input / ns.total_N + 1.0 / ns.total_N
            alpha = ns.marginal_alpha(t_cont).reshape(-1, 1, 1)
            sigma = ns.marginal_std(t_cont).reshape(-1, 1, 1)
            return (x - alpha * synthetic_x0(x, t_input, c)) / sigma
        model_fn = M.model_wrapper(eps_model, ns, model_type="noise", guidance_type="classifier-free", condition=cond, unconditional_condition=uncond,
                                   guidance_scale=scale)
    kw = dict(steps=STEPS, order=order, skip_type=skip, method="multistep", lower_order_final=True, denoise_to_zero=bool(extra.get("denoise_to_zero", False)))
    if solver == "unipc":
        s = M.UniPC(model_fn, ns, variant="bh2", **corr)
    else:
        s = M.DPM_Solver(model_fn, ns, algorithm_type="dpmsolver++", **corr)
        kw["solver_type"] = "dpmsolver"
    # the x0 the solver is about to correct, read where it is formed (noise_prediction_fn feeds data_prediction_fn in both classes)
    inner = s.noise_prediction_fn

    def spy(x, t):
        noise = inner(x, t)
        a = ((x - ns.marginal_std(t) * noise) / ns.marginal_alpha(t)).abs().reshape(-1)
        q = float(torch.quantile(a, spy_ratio if ratio is None else ratio))
        thr = q if ratio is None else max(q, max_val)
        seen.append((float((a > thr).float().mean()), q, float(a.max())))
        return noise
    s.noise_prediction_fn = spy
    with torch.no_grad():
        y = s.sample(x_T.clone(), **kw)
    arr = np.array(seen, dtype=np.float32)
    return y.numpy(), np.array(times, dtype=np.float32), arr[:, 0], arr[:, 1], arr[:, 2]


def host_loop(solver, order, skip, ratio, max_val, x_T, extra, guide=None):
    f = np.float32
    t = S.build_table(solver, STEPS, order=order, skip_type=skip, **extra)

    def syn(x, tm, cond=None):
        tt = np.asarray(tm, f).reshape(-1, 1, 1)
        xx = x.astype(f) if cond is None else (x.astype(f) + cond.astype(f)).astype(f)
        return (f(0.9) * np.tanh(xx) + f(0.05) * np.cos(f(0.01) * tt)).astype(f)
    if guide is None:
        fn = syn
    else:
        cond, uncond, scale = guide
        fn = lambda x, tm: S.guided_x0(syn(x, tm, uncond.numpy()), syn(x, tm, cond.numpy()), f(scale))      # noqa: E731
    return t, S.run_table_numpy(t, fn, x_T, correct_x0=dict(mode="dynamic_thresholding", ratio=ratio, max_val=max_val))


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def main():
    torch.set_default_dtype(torch.float32)
    torch.set_num_threads(4)
    from sampler import dpm_solver, uni_pc  # type: ignore
    mods = {"unipc": uni_pc, "dpmsolver++": dpm_solver}
    betas = torch.from_numpy(S.linear_betas())
    rng = np.random.default_rng(17)
    x_T = [torch.from_numpy(rng.standard_normal((1, C, L)).astype(np.float32)) for L in LENS]
    cond = torch.from_numpy((0.8 * rng.standard_normal((1, C, 1))).astype(np.float32))
    uncond = torch.from_numpy((0.8 * rng.standard_normal((1, C, 1))).astype(np.float32))
    out = {f"x_T{b}": x.numpy() for b, x in enumerate(x_T)}
    out.update(cond=cond.numpy(), uncond=uncond.numpy(), lens=np.array(LENS, np.int32))
    report = {}

    def legs_of(guide):
        """max_val per leg and item, (3, items), from the uncorrected loops (UniPC order 2, time_uniform) of the three items: their |x0| quantiles at
        the grid's ratios 0.75 and 0.9 and the |x0| maximum, each (items, evaluations)"""
        runs = [[run_reference(uni_pc, betas, "unipc", 2, "time_uniform", None, None, x, guide=guide, spy_ratio=r) for x in x_T] for r in (0.75, 0.9)]
        q75, q90, mx = np.array([r[3] for r in runs[0]]), np.array([r[3] for r in runs[1]]), np.array([r[4] for r in runs[0]])
        n = len(x_T)
        legs = np.stack([np.full(n, 0.5 * q75.min()), 0.5 * (q90[:, 0] + mx[:, 0]), np.full(n, 1.5 * mx.max())]).astype(np.float32)
        assert (legs[1] > q90[:, 0]).all() and (legs[1] < mx[:, 0]).all()
        return legs, q75, q90, mx

    for prefix, cases, guided in (("g17", CASES17, False), ("g18", CASES18, True)):
        for case in cases:
            solver, order, skip, ratio, leg = case[:5]
            guide = (cond, uncond, case[5]) if guided else None
            extra = {} if guided else case[5]
            key = prefix + ".maxval" + (("_s" + f"{case[5]:g}".replace(".", "p")) if guided else "")
            if key not in out:
                legs, q75, q90, mx = legs_of(guide)
                out[key] = legs
                out[key + ".q75_plain"], out[key + ".q90_plain"], out[key + ".absmax_plain"] = q75.astype(np.float32), q90.astype(np.float32), mx.astype(np.float32)
                report[key] = {k: [float(v) for v in legs[i]] for i, k in enumerate(LEGS)}
            max_vals = [float(v) for v in out[key][LEGS.index(leg)]]
            tag = (tag18 if guided else tag17)(*case)
            errs, shares = [], []
            for b, x in enumerate(x_T):
                max_val = max_vals[b]
                y, times, clamped, q, _ = run_reference(mods[solver], betas, solver, order, skip, ratio, max_val, x, extra, guide)
                out[f"{prefix}.{tag}.y{b}"], out[f"{prefix}.{tag}.clamped{b}"] = y, clamped
                if b == 0:
                    out[f"{prefix}.{tag}.times"] = times
                t, yh = host_loop(solver, order, skip, ratio, max_val, x.numpy(), extra, guide)
                assert t.steps == len(times)
                errs.append(rel_l2(yh, y))
                shares.append([float(v) for v in clamped])
            report[f"{prefix}.{tag}"] = {"max_val": max_vals, "ratio": ratio, "evals": int(len(times)), "host_rel_l2": errs,
                                         "evals_clamping": [int(sum(v > 0 for v in s_)) for s_ in shares], "clamped_first_last": [[s_[0], s_[-1]] for s_ in shares]}
    for prefix in ("g17", "g18"):
        report[f"{prefix}.worst_host_rel_l2"] = max(max(v["host_rel_l2"]) for k, v in report.items() if k.startswith(prefix + ".") and "host_rel_l2" in v)
    save_npz_deterministic(os.path.join(HERE, "golden_v8.npz"), out)
    with open(os.path.join(HERE, "golden_v8_report.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(f"{len(CASES17) + len(CASES18)} cases, {os.path.getsize(os.path.join(HERE, 'golden_v8.npz'))} bytes; worst host rel L2: "
          f"g17 {report['g17.worst_host_rel_l2']:.3e}, g18 {report['g18.worst_host_rel_l2']:.3e}")


if __name__ == "__main__":
    main()
