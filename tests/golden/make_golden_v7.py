"""Golden vectors of the reference's own classifier-free guidance -> golden_v7.npz.

BUILD CONTAINER ONLY (reads the reference checkout).  The reference's ``model_wrapper(..., guidance_type="classifier-free", condition=c,
unconditional_condition=u, guidance_scale=s)`` runs under ``sampler.uni_pc.UniPC.sample`` and ``sampler.dpm_solver.DPM_Solver.sample``
(``algorithm_type="dpmsolver++"``, multistep), float32, one B = 1 call per case, on ``NoiseScheduleVP("discrete", betas=<model.py's float32
buffer, model.py:426-433>)``.

The model is ``model_type="noise"``: it returns ``eps = (x - alpha x0(x, t, cond)) / sigma`` of the closed-form ``synthetic_x0`` below.  The
reference's x_start wrapper cannot run a guided batch -- its ``alpha_t`` of shape (2,) does not broadcast against (2, C, T)
(uni_pc.py:190-191) -- while the noise wrapper has no such problem and defines the same mathematics: the reference combines
``eps_u + s (eps_c - eps_u)``, which for one x, alpha, sigma is the eps of ``x0_u + s (x0_c - x0_u)``.

What is committed is data only: x_T, the two conditions (the model's parameters), model times in call order and final latents.

  g16.<tag>.y / .times   tag = <solver><order>_<skip_type>_<steps>[_bh1]_s<scale>
  grid: both solvers x order {1, 2, 3} x steps {5, 8} x scale {0, 0.5, 1, 2.5, 7} at logSNR (UniPC: bh2 and bh1), plus the three
  skip_types at scale 2.5 (order 2, 8 steps).

Run: python tests/golden/make_golden_v7.py
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

C, T = 4, 8
SCALES = (0.0, 0.5, 1.0, 2.5, 7.0)
SKIPS = ("logSNR", "time_uniform", "time_quadratic")
# (solver, steps, order, skip_type, variant, scale)
CASES = [(sv, n, o, "logSNR", v, s) for sv, vs in (("unipc", ("bh2", "bh1")), ("dpmsolver++", (None,))) for v in vs for o in (1, 2, 3)
         for n in (5, 8) for s in SCALES]
CASES += [(sv, 8, 2, k, v, 2.5) for sv, v in (("unipc", "bh2"), ("dpmsolver++", None)) for k in SKIPS[1:]]


def case_tag(solver, steps, order, skip, variant, scale):
    return (f"{'unipc' if solver == 'unipc' else 'dpmpp'}{order}_{skip}_{steps}" + ("_bh1" if variant == "bh1" else "") + f"_s{scale:g}").replace(".", "p")


def synthetic_x0(x, t, cond):
    """the stand-in denoiser of v4 / v5 with a condition: x (B, C, T), t (B,), cond (B, C, 1) -> x0"""
    tt = t.to(x.dtype).reshape(-1, 1, 1)
    return 0.9 * torch.tanh(x + cond) + 0.05 * torch.cos(0.01 * tt)


def run_reference(M, betas, solver, steps, order, skip, variant, scale, x_T, cond, uncond):
    times = []
    ns = M.NoiseScheduleVP(schedule="discrete", betas=betas)

    def eps_model(x, t_input, c):      # model_type="noise": t_input = (t_continuous - 1/N) * N  (uni_pc.py:170-179)
        times.append(float(t_input.reshape(-1)[0]))
        t_cont = t_input / ns.total_N + 1.0 / ns.total_N
        alpha = ns.marginal_alpha(t_cont).reshape(-1, 1, 1)
        sigma = ns.marginal_std(t_cont).reshape(-1, 1, 1)
        return (x - alpha * synthetic_x0(x, t_input, c)) / sigma

    model_fn = M.model_wrapper(eps_model, ns, model_type="noise", guidance_type="classifier-free", condition=cond,
                               unconditional_condition=uncond, guidance_scale=scale)
    kw = dict(steps=steps, order=order, skip_type=skip, method="multistep", lower_order_final=True)
    if solver == "unipc":
        s = M.UniPC(model_fn, ns, variant=variant)
    else:
        s = M.DPM_Solver(model_fn, ns, algorithm_type="dpmsolver++")
        kw["solver_type"] = "dpmsolver"
    with torch.no_grad():
        y = s.sample(x_T.clone(), **kw)
    return y.numpy(), np.array(times, dtype=np.float32)


def main():
    torch.set_default_dtype(torch.float32)
    torch.set_num_threads(4)
    from sampler import dpm_solver, uni_pc  # type: ignore
    betas = torch.from_numpy(S.linear_betas())
    assert betas.dtype == torch.float32
    rng = np.random.default_rng(16)
    x_T = torch.from_numpy(rng.standard_normal((1, C, T)).astype(np.float32))
    cond = torch.from_numpy((0.8 * rng.standard_normal((1, C, 1))).astype(np.float32))
    uncond = torch.from_numpy((0.8 * rng.standard_normal((1, C, 1))).astype(np.float32))
    out = {"g16.x_T": x_T.numpy(), "g16.cond": cond.numpy(), "g16.uncond": uncond.numpy()}
    report = {}
    for case in CASES:
        y, times = run_reference(uni_pc if case[0] == "unipc" else dpm_solver, betas, *case, x_T, cond, uncond)
        tag = case_tag(*case)
        out[f"g16.{tag}.y"], out[f"g16.{tag}.times"] = y, times
        report[f"g16.{tag}"] = {"evals": len(times), "y_rms": float(np.sqrt((y.astype(np.float64) ** 2).mean()))}
    save_npz_deterministic(os.path.join(HERE, "golden_v7.npz"), out)
    with open(os.path.join(HERE, "golden_v7_report.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(f"{len(report)} cases, {os.path.getsize(os.path.join(HERE, 'golden_v7.npz'))} bytes")


if __name__ == "__main__":
    main()
