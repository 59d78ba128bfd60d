"""CPU tests of the top-level ``sampler`` package (sampler/dpm_solver.py, sampler/uni_pc.py): the reference's signatures
(tests/golden/sampler_signatures.json), its own loops as recorded in the goldens (g14 of golden_v5.npz, g16 of golden_v7.npz, g17 of
golden_v9.npz: make_golden_sampler.py) through the package's classes on CPU tensors -- the ``host`` path --, the schedule's methods, the
refusals, what ``import sampler`` loads, and the export and register audit of ``ns2vc_k_solver_step_flat``."""
import inspect
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from ns2vc_amd import schedule as S
from test_solvers_cpu import SYN_CASES, SYN_TOL, case_tag, rel_l2
from test_guidance_cpu import CASES as GUIDED_CASES, GUIDED_TOL, case_tag as guided_tag
from util import synthetic_x0

from sampler import dpm_solver, uni_pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
# the g17 grid of make_golden_sampler.py
KIND_CASES = [("unipc", 8, 2, "time_uniform", True, {}), ("dpmsolver++", 10, 3, "logSNR", True, {})]


@pytest.fixture(scope="module")
def gold():
    return {"v1": np.load(os.path.join(GOLDEN, "golden_v1.npz")), "v5": np.load(os.path.join(GOLDEN, "golden_v5.npz")),
            "v7": np.load(os.path.join(GOLDEN, "golden_v7.npz")), "v9": np.load(os.path.join(GOLDEN, "golden_v9.npz"))}


def schedule_of(module=uni_pc):
    return module.NoiseScheduleVP(schedule="discrete", betas=torch.from_numpy(S.linear_betas()))


def run_case(case, model, model_type, x_T, **wrapper):
    """one golden case through the package's own classes on CPU tensors -> (solver, result, the model's time inputs)"""
    solver, steps, order, skip, lof, extra = case
    extra = dict(extra)
    module = uni_pc if solver == "unipc" else dpm_solver
    ns = schedule_of(module)
    times = []

    def recording(x, t, *a, **kw):
        times.append(float(t.reshape(-1)[0]))
        return model(ns, x, t, *a, **kw)

    fn = module.model_wrapper(recording, ns, model_type=model_type, **wrapper)
    if solver == "unipc":
        s = module.UniPC(fn, ns, variant=extra.pop("variant", "bh2"))
    else:
        s = module.DPM_Solver(fn, ns, algorithm_type="dpmsolver++")
    y = s.sample(torch.from_numpy(x_T), steps=steps, order=order, skip_type=skip, method="multistep", lower_order_final=lof, **extra)
    return s, y.numpy(), np.array(times, dtype=np.float32)


def x0_model(ns, x, t, cond=None):
    return torch.from_numpy(synthetic_x0(x.numpy(), t.numpy(), None if cond is None else cond.numpy()))


def eps_model(ns, x, t_input, cond=None):
    """the closed-form denoiser as a noise model: eps = (x - alpha x0) / sigma at the continuous time of t_input"""
    t_cont = t_input / ns.total_N + 1.0 / ns.total_N
    alpha, sigma = ns.marginal_alpha(t_cont).reshape(-1, 1, 1), ns.marginal_std(t_cont).reshape(-1, 1, 1)
    return (x - alpha * x0_model(ns, x, t_input, cond)) / sigma


def v_model(ns, x, t_input):
    t_cont = t_input / ns.total_N + 1.0 / ns.total_N
    alpha, sigma = ns.marginal_alpha(t_cont).reshape(-1, 1, 1), ns.marginal_std(t_cont).reshape(-1, 1, 1)
    x0 = x0_model(ns, x, t_input)
    return alpha * ((x - alpha * x0) / sigma) - sigma * x0


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------
def signature_of(fn):
    return [[p.name, "<required>" if p.default is inspect.Parameter.empty else repr(p.default)] for p in inspect.signature(fn).parameters.values()
            if p.name != "self"]


def test_signatures_equal_the_reference():
    """parameter names, order and defaults -- also where they differ from this project's own (UniPC's variant defaults to bh1)"""
    with open(os.path.join(GOLDEN, "sampler_signatures.json")) as f:
        want = json.load(f)
    assert len(want) == 8
    for name, mod, cls in (("dpm_solver", dpm_solver, "DPM_Solver"), ("uni_pc", uni_pc, "UniPC")):
        assert sorted(mod.__all__) == sorted(["NoiseScheduleVP", "model_wrapper", cls])
        assert signature_of(mod.NoiseScheduleVP.__init__) == want[f"{name}.NoiseScheduleVP"]
        assert signature_of(mod.model_wrapper) == want[f"{name}.model_wrapper"]
        assert signature_of(getattr(mod, cls).__init__) == want[f"{name}.{cls}"]
        assert signature_of(getattr(mod, cls).sample) == want[f"{name}.{cls}.sample"]
    assert S.TABLE_OPTIONS["variant"] == "bh2" and dict(want["uni_pc.UniPC"])["variant"] == "'bh1'"


def test_import_loads_neither_the_oracle_nor_the_library():
    code = ("import sys, sampler, sampler.dpm_solver, sampler.uni_pc\n"
            "from ns2vc_amd import _lib\n"
            "assert 'oracle' not in sys.modules and not [m for m in sys.modules if m.startswith('oracle.')]\n"
            "assert _lib._lib is None\n"
            "assert 'libns2vc_hip' not in open('/proc/self/maps').read()\n"
            "assert sampler.capture is True\n")
    env = {k: v for k, v in os.environ.items() if k != "NS2VC_SAMPLER_CAPTURE"}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-c", "import sampler; assert sampler.capture is False"], cwd=ROOT, env=dict(env, NS2VC_SAMPLER_CAPTURE="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


# ---- 2. the reference's loops ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SYN_CASES, ids=[case_tag(*c) for c in SYN_CASES])
def test_g14_through_the_classes(case, gold):
    """every g14 case: the x_start model behind model_wrapper, the package's class, CPU tensors.  Model times under the assert_allclose
    of tests/test_solvers_cpu.py, the result within its SYN_TOL."""
    tag = case_tag(*case)
    s, y, times = run_case(case, x0_model, "x_start", gold["v5"]["g14.x_T"])
    assert s.last_path == "host"
    np.testing.assert_allclose(times, gold["v5"][f"g14.{tag}.times"], rtol=1e-6, atol=2e-4)
    e = rel_l2(y, gold["v5"][f"g14.{tag}.y"])
    print(f"{tag}: {e:.3e}")
    assert e <= SYN_TOL, e


@pytest.mark.parametrize("kind", ["noise", "v"])
@pytest.mark.parametrize("case", KIND_CASES, ids=[case_tag(*c) for c in KIND_CASES])
def test_noise_and_v_models(case, kind, gold):
    tag = case_tag(*case)
    s, y, times = run_case(case, eps_model if kind == "noise" else v_model, kind, gold["v5"]["g14.x_T"])
    assert s.last_path == "host"
    np.testing.assert_allclose(times, gold["v9"][f"g17.{kind}.{tag}.times"], rtol=1e-6, atol=2e-4)
    e = rel_l2(y, gold["v9"][f"g17.{kind}.{tag}.y"])
    print(f"{kind} {tag}: {e:.3e}")
    assert e <= SYN_TOL, e


def test_a_bare_callable_is_a_noise_function(gold):
    case = ("unipc", 8, 2, "time_uniform", True, {})
    ns = schedule_of()
    fn = uni_pc.model_wrapper(lambda x, t: eps_model(ns, x, t), ns, model_type="noise")
    s = uni_pc.UniPC(lambda x, t: fn(x, t), ns, variant="bh2")
    y = s.sample(torch.from_numpy(gold["v5"]["g14.x_T"]), steps=8, order=2)
    assert s.last_path == "host" and rel_l2(y.numpy(), gold["v9"][f"g17.noise.{case_tag(*case)}.y"]) <= SYN_TOL


@pytest.mark.parametrize("case", GUIDED_CASES, ids=[guided_tag(*c) for c in GUIDED_CASES])
def test_classifier_free_guidance_against_reference(case, gold):
    """the reference-recorded guided cases of tests/test_guidance_cpu.py through model_wrapper(guidance_type="classifier-free"), at its gates"""
    solver, steps, order, skip, variant, scale = case
    g = gold["v7"]
    tag = guided_tag(*case)
    s, y, times = run_case((solver, steps, order, skip, True, {"variant": variant} if variant else {}), eps_model, "noise", g["g16.x_T"],
                           guidance_type="classifier-free", condition=torch.from_numpy(g["g16.cond"]),
                           unconditional_condition=torch.from_numpy(g["g16.uncond"]), guidance_scale=scale)
    assert s.last_path == "host"
    np.testing.assert_allclose(times, g[f"g16.{tag}.times"], rtol=1e-6, atol=2e-4)
    e = rel_l2(y, g[f"g16.{tag}.y"])
    print(f"{tag}: {e:.3e}")
    assert e <= GUIDED_TOL[scale], e


def test_dtype_and_shape_of_x(gold):
    """x of another floating dtype and of another rank: float32 arithmetic, the result in x.dtype"""
    ns = schedule_of()
    fn = uni_pc.model_wrapper(lambda x, t: 0.9 * torch.tanh(x), ns, model_type="x_start")
    x = torch.from_numpy(gold["v5"]["g14.x_T"])
    y32 = uni_pc.UniPC(fn, ns).sample(x, steps=5)
    y64 = uni_pc.UniPC(fn, ns).sample(x.double(), steps=5)
    y2d = uni_pc.UniPC(fn, ns).sample(x.reshape(2, -1), steps=5)
    assert y64.dtype == torch.float64 and y32.dtype == torch.float32 and y2d.shape == (2, 32)
    # (the model itself ran in float64 on the float64 x: its values differ from the float32 run's by float32 rounding, the state's precision)
    assert rel_l2(y64.numpy(), y32.numpy()) <= SYN_TOL and torch.equal(y2d.reshape(x.shape), y32)


# ---- 3. the schedule ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 6, 20, 30, 40, 50])
@pytest.mark.parametrize("module", [dpm_solver, uni_pc], ids=["dpm_solver", "uni_pc"])
def test_noise_schedule_methods_match_the_g4_scalars(module, steps, gold):
    """tolerances of tests/test_cpu.py test_schedule_scalars_match_reference"""
    g = gold["v1"]
    ns = schedule_of(module)
    assert (ns.T, ns.total_N, ns.schedule) == (1.0, 1000, "discrete")
    t = torch.from_numpy(g[f"g4.s{steps}.t"])
    lam = ns.marginal_lambda(t)
    assert lam.dtype == torch.float32 and lam.shape == t.shape
    assert np.allclose(lam.numpy(), g[f"g4.s{steps}.lambda"], rtol=2e-5, atol=2e-6)
    assert np.allclose(ns.marginal_alpha(t).numpy(), g[f"g4.s{steps}.alpha"], rtol=2e-5, atol=1e-7)
    assert np.allclose(ns.marginal_std(t).numpy(), g[f"g4.s{steps}.sigma"], rtol=2e-5, atol=1e-7)
    assert np.allclose(torch.exp(ns.marginal_log_mean_coeff(t)).numpy(), g[f"g4.s{steps}.alpha"], rtol=2e-5, atol=1e-7)
    assert np.allclose(ns.model_time(t).numpy(), g[f"g4.s{steps}.t_model"], rtol=0, atol=1e-3)
    assert np.allclose(ns.inverse_lambda(torch.from_numpy(g[f"g4.s{steps}.lambda"])).numpy(), g[f"g4.s{steps}.t"], rtol=1e-5, atol=1e-7)


def test_alphas_cumprod_gives_the_same_schedule():
    b = S.linear_betas(dtype=np.float64)
    a = uni_pc.NoiseScheduleVP("discrete", alphas_cumprod=torch.from_numpy(np.cumprod(1.0 - b)))
    n = schedule_of()
    t = torch.linspace(1e-3, 1.0, 37)
    assert np.allclose(a.marginal_lambda(t).numpy(), n.marginal_lambda(t).numpy(), rtol=2e-5, atol=2e-6)
    assert a.marginal_alpha(t.double()).dtype == torch.float32 and a.betas is None


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def _solver(module, **kw):
    ns = schedule_of(module)
    fn = module.model_wrapper(lambda x, t: x, ns, model_type="x_start")
    return (module.UniPC if module is uni_pc else module.DPM_Solver)(fn, ns, **kw)


@pytest.mark.parametrize("module", [dpm_solver, uni_pc], ids=["dpm_solver", "uni_pc"])
def test_refusals_name_the_keyword(module):
    x = torch.zeros(1, 2, 4)
    for method in ("singlestep", "singlestep_fixed", "adaptive"):
        with pytest.raises(ValueError, match=r"method must be 'multistep' \(.*\), got '" + method + "'"):
            _solver(module).sample(x, steps=5, method=method)
    with pytest.raises(ValueError, match=r"return_intermediate must be False \(.*\), got True"):
        _solver(module).sample(x, steps=5, return_intermediate=True)
    with pytest.raises(ValueError, match=r"correcting_xt_fn must be None \(.*\), got"):
        _solver(module, correcting_xt_fn=lambda x, t, step: x)
    bad = "dpmsolver" if module is dpm_solver else "noise_prediction"
    with pytest.raises(ValueError, match=r"algorithm_type must be '.*' \(.*\), got '" + bad + "'"):
        _solver(module, algorithm_type=bad)
    for schedule in ("linear", "cosine"):
        with pytest.raises(ValueError, match=r"schedule must be 'discrete' \(.*\), got '" + schedule + "'"):
            module.NoiseScheduleVP(schedule=schedule)
    with pytest.raises(ValueError, match="correcting_x0_fn"):
        _solver(module, correcting_x0_fn="clamp_everything")
    with pytest.raises(ValueError, match="order"):
        _solver(module).sample(x, steps=5, order=4)
    with pytest.raises(ValueError, match="skip_type"):
        _solver(module).sample(x, steps=5, skip_type="uniform")
    with pytest.raises(ValueError, match="model_type"):
        module.model_wrapper(lambda x, t: x, schedule_of(module), model_type="eps")
    assert _solver(module).sample(x, steps=5, atol=1.0, rtol=1.0).shape == x.shape      # accepted and unused


def test_out_of_scope_methods_and_variants():
    with pytest.raises(ValueError, match="inverse"):
        _solver(dpm_solver).inverse(torch.zeros(1, 2, 4))
    with pytest.raises(ValueError, match="add_noise"):
        _solver(dpm_solver).add_noise(torch.zeros(1, 2, 4), torch.ones(1))
    with pytest.raises(ValueError, match="variant"):
        _solver(uni_pc, variant="vary_coeff").sample(torch.zeros(1, 2, 4), steps=5)
    with pytest.raises(ValueError, match="solver_type"):
        _solver(dpm_solver).sample(torch.zeros(1, 2, 4), steps=5, solver_type="midpoint")


# ---- 5. corrections on the host path ----------------------------------------------------------------------------------------------
def test_host_corrections(gold):
    """dynamic thresholding is run_table_numpy's, bit for bit; a callable that clamps is its "clamp" mode within float32 rounding of the
    second round trip the corrected m takes"""
    x_T = 3.0 * gold["v5"]["g14.x_T"]
    ns = schedule_of()
    fn = uni_pc.model_wrapper(lambda x, t: x0_model(ns, x, t), ns, model_type="x_start")
    table = S.build_table("unipc", 6, order=2)
    y = uni_pc.UniPC(fn, ns, variant="bh2", correcting_x0_fn="dynamic_thresholding", thresholding_max_val=0.5,
                     dynamic_thresholding_ratio=0.9).sample(torch.from_numpy(x_T), steps=6)
    want = S.run_table_numpy(table, synthetic_x0, x_T, correct_x0=dict(mode="dynamic_thresholding", ratio=0.9, max_val=0.5))
    assert np.array_equal(y.numpy(), want)
    plain = uni_pc.UniPC(fn, ns, variant="bh2").sample(torch.from_numpy(x_T), steps=6)
    assert rel_l2(plain.numpy(), want) > 1e-2      # (the correction matters here)
    seen = []

    def clamp(x0, t):
        seen.append(tuple(t.shape))
        return x0.clamp(-0.5, 0.5)

    y = uni_pc.UniPC(fn, ns, variant="bh2", correcting_x0_fn=clamp).sample(torch.from_numpy(x_T), steps=6)
    want = S.run_table_numpy(table, synthetic_x0, x_T, correct_x0=dict(mode="clamp", max_val=0.5))
    assert seen == [(2,)] * 6 and rel_l2(y.numpy(), want) <= SYN_TOL


# ---- 6. the new export and its registers ------------------------------------------------------------------------------------------
def test_flat_step_is_declared_bound_exported_and_refuses():
    import ctypes as C
    from ns2vc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    assert "#define NS2VC_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7
    assert re.search(r"\bint ns2vc_k_solver_step_flat\(", header) and "ns2vc_k_solver_step_flat" in _lib.PROTOTYPES
    blocks = int(re.search(r"#define NS2VC_FLAT_MAX_BLOCKS (\d+)", header).group(1))
    assert _lib.FLAT_TRIP == blocks * 256 * 4 and _lib.FLAT_KINDS == {"x_start": 0, "noise": 1, "v": 2, "score": 3, "data": 4}
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    step = lambda coef=p, rows=2, row=0, kind=0, out=p, xe=p, xbar=p, d1=p, mprev=p, mprev2=None, m_out=None, n=4: \
        lib.ns2vc_k_solver_step_flat(coef, rows, row, kind, out, xe, xbar, d1, mprev, mprev2, m_out, n, None)      # noqa: E731
    # every refusal returns in front of the launch (no device is touched)
    for kw, what in ((dict(coef=None), "null"), (dict(out=None), "null"), (dict(xe=None), "null"), (dict(xbar=None), "null"), (dict(d1=None), "null"),
                     (dict(mprev=None), "null"), (dict(n=0), "n must be"), (dict(kind=5), "kind"), (dict(kind=-1), "kind"), (dict(row=2), "row"),
                     (dict(row=-1), "row"), (dict(rows=0), "row"), (dict(xe=p + 2), "aligned"), (dict(m_out=p + 1), "aligned")):
        assert step(**kw) != 0, kw
        assert what in lib.ns2vc_last_error().decode(), (kw, lib.ns2vc_last_error())


def test_flat_step_kernels_use_no_lds_no_scratch_and_spill_nothing():
    """the compiler's kernel-resource-usage remarks on misc.hip: 15 instantiations of solver_step_flat_kernel (five kinds x history 1, history 2,
    FORM) -- no LDS, no scratch, no spilled register, full occupancy; the counts of the kernels in front of them stand"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I../../include", "-Rpass-analysis=kernel-resource-usage", "-c", "misc.hip",
                        "-o", os.devnull], cwd=os.path.join(ROOT, "ns2vc_amd", "csrc"), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out, fn = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill|LDS Size \[bytes/block\]|VGPRs|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and fn:
            out.setdefault(fn, {})[m.group(1)] = int(m.group(2))
    new = {n: v for n, v in out.items() if "solver_step_flat_kernel" in n}
    assert len(new) == 15, sorted(new)
    for n, v in sorted(new.items()):
        print(n, v)
        assert (v["ScratchSize [bytes/lane]"], v["VGPRs Spill"], v["SGPRs Spill"], v["LDS Size [bytes/block]"]) == (0, 0, 0, 0), (n, v)
        assert v["VGPRs"] <= 64 and v["Occupancy [waves/SIMD]"] == 8, (n, v)
    count = lambda s: len([n for n in out if s in n])      # noqa: E731
    assert (count("solver_update_kernel"), count("solver_update_items_kernel"), count("sampler_suspend_kernel"), count("sampler_resume_kernel")) == (12, 18, 1, 3)
