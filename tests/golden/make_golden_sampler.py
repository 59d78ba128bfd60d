#!/usr/bin/env python3
"""Golden data of the top-level ``sampler`` package (tests/test_sampler_pkg_cpu.py, tests/test_sampler_pkg_gpu.py).

BUILD CONTAINER ONLY (reads the reference checkout).  The reference's two modules are loaded from their files under private names, because
``import sampler`` now finds THIS repository's package wherever the repository is on the path.

What is committed is data only -- names, settings, model times and results; no program text:

  sampler_signatures.json   parameter names and defaults (``repr``; "<required>" where there is none) of NoiseScheduleVP and model_wrapper of
                            both modules, of the two solver constructors and of their ``sample`` methods
  golden_v9.npz             the reference's own loops (float32, one B = 1 call per item) from ``g14.x_T`` of golden_v5.npz on the closed-form denoiser of
                            tests/util.synthetic_x0 re-expressed as a ``model_type="noise"`` model, eps = (x - alpha x0) / sigma, and as a
                            ``model_type="v"`` model, v = alpha eps - sigma x0:
                              g17.<noise|v>.<tag>.y / .times      tag as tests/test_solvers_cpu.case_tag; CASES below
"""
from __future__ import annotations

import importlib.util
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden_v6 import REF, save_npz_deterministic  # noqa: E402
from ns2vc_amd import schedule as S  # noqa: E402
from test_solvers_cpu import case_tag  # noqa: E402

# (solver, steps, order, skip_type, lower_order_final, extra): one UniPC order-2 and one DPM-Solver++ order-3 case per model type
CASES = [("unipc", 8, 2, "time_uniform", True, {}), ("dpmsolver++", 10, 3, "logSNR", True, {})]
KINDS = ("noise", "v")


def load_reference(name):
    spec = importlib.util.spec_from_file_location(f"reference_{name}", os.path.join(REF, "sampler", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def signature_of(fn):
    return [[p.name, "<required>" if p.default is inspect.Parameter.empty else repr(p.default)] for p in inspect.signature(fn).parameters.values()
            if p.name != "self"]


def synthetic_x0(x, t):
    tt = t.to(x.dtype).reshape(-1, 1, 1)
    return 0.9 * torch.tanh(x) + 0.05 * torch.cos(0.01 * tt)


def run_reference(M, kind, betas, solver, steps, order, skip, lof, extra, x_T):
    times = []
    ns = M.NoiseScheduleVP(schedule="discrete", betas=betas)

    def model(x, t_input):
        times.append(float(t_input.reshape(-1)[0]))
        t_cont = t_input / ns.total_N + 1.0 / ns.total_N
        alpha = ns.marginal_alpha(t_cont).reshape(-1, 1, 1)
        sigma = ns.marginal_std(t_cont).reshape(-1, 1, 1)
        x0 = synthetic_x0(x, t_input)
        eps = (x - alpha * x0) / sigma
        return eps if kind == "noise" else alpha * eps - sigma * x0

    model_fn = M.model_wrapper(model, ns, model_type=kind)
    kw = dict(steps=steps, order=order, skip_type=skip, method="multistep", lower_order_final=lof)
    if solver == "unipc":
        s = M.UniPC(model_fn, ns, variant=extra.get("variant", "bh2"))
    else:
        s = M.DPM_Solver(model_fn, ns, algorithm_type="dpmsolver++")
    # one B = 1 call per item: the uni_pc wrapper's alpha_t of shape (B,) does not broadcast against (B, C, T) for "v" (uni_pc.py:190-194);
    # nothing in the loop couples the items
    with torch.no_grad():
        y = torch.cat([s.sample(x_T[b:b + 1].clone(), **kw) for b in range(x_T.shape[0])])
    return y.numpy(), np.array(times[:len(times) // x_T.shape[0]], dtype=np.float32)


def main():
    torch.set_default_dtype(torch.float32)
    torch.set_num_threads(4)
    dpm_solver, uni_pc = load_reference("dpm_solver"), load_reference("uni_pc")
    sig = {}
    for name, mod, cls in (("dpm_solver", dpm_solver, "DPM_Solver"), ("uni_pc", uni_pc, "UniPC")):
        sig[f"{name}.NoiseScheduleVP"] = signature_of(mod.NoiseScheduleVP.__init__)
        sig[f"{name}.model_wrapper"] = signature_of(mod.model_wrapper)
        sig[f"{name}.{cls}"] = signature_of(getattr(mod, cls).__init__)
        sig[f"{name}.{cls}.sample"] = signature_of(getattr(mod, cls).sample)
    with open(os.path.join(HERE, "sampler_signatures.json"), "w") as f:
        json.dump(sig, f, indent=1, sort_keys=True)
        f.write("\n")
    betas = torch.from_numpy(S.linear_betas())
    x_T = torch.from_numpy(np.load(os.path.join(HERE, "golden_v5.npz"))["g14.x_T"])
    out = {}
    for kind in KINDS:
        for case in CASES:
            y, times = run_reference(uni_pc if case[0] == "unipc" else dpm_solver, kind, betas, *case, x_T)
            out[f"g17.{kind}.{case_tag(*case)}.y"], out[f"g17.{kind}.{case_tag(*case)}.times"] = y, times
    save_npz_deterministic(os.path.join(HERE, "golden_v9.npz"), out)
    print(f"{len(sig)} signatures, {len(out) // 2} cases, {os.path.getsize(os.path.join(HERE, 'golden_v9.npz'))} bytes")


if __name__ == "__main__":
    main()
