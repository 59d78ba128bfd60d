"""CPU checks of the x0 correction (dynamic thresholding / clamp): ``schedule.abs_quantile`` against ``torch.quantile`` bit for bit,
``run_table_numpy(correct_x0=...)`` against the reference's own corrected loops (tests/golden/golden_v8.npz, make_golden_v8.py), the keyword
checks and the routing of ``Denoiser.sample``, the exports."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from ns2vc_amd import schedule as S
from recording_engine import denoiser as _denoiser      # the real Denoiser constructor on the recording engine -> (denoiser, recording)
from util import synthetic_x0

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "golden_v8.npz")
REPORT = os.path.join(HERE, "golden", "golden_v8_report.json")

STEPS, LENS, LEGS = 8, (8, 7, 5), ("a", "b", "c")
# the grids of make_golden_v8.py.  g17: (solver, order, skip_type, ratio, leg, extra options); g18: (solver, order, skip_type, ratio, leg, scale)
CASES17 = [(sv, o, "time_uniform", r, leg, {}) for sv in ("unipc", "dpmsolver++") for o in (1, 2, 3) for r in (0.9, 0.75) for leg in LEGS]
CASES17 += [(sv, 3, "logSNR", 0.9, "a", {"denoise_to_zero": True}) for sv in ("unipc", "dpmsolver++")]
CASES17 += [(sv, 2, "logSNR", r, "a", {}) for sv in ("unipc", "dpmsolver++") for r in (0.995, 1.0)]
CASES18 = [(sv, o, "logSNR", 0.9, leg, 2.5) for sv in ("unipc", "dpmsolver++") for o in (1, 2, 3) for leg in ("a", "b")]
CASES18 += [(sv, 2, "logSNR", 0.75, "a", 7.0) for sv in ("unipc", "dpmsolver++")]
# Relative L2 of run_table_numpy (float32) against the reference's float32 loop.  The expectation is the bound of the uncorrected loops of golden_v5
# (tests/test_solvers_cpu.py: 3.8e-6).  golden_v8_report.json records what the corrected loops give: worst 6.8e-7 over g17 and 1.1e-6 over g18
# (guided, scales 2.5 and 7) -- the clamp is 1-Lipschitz and the division by s >= max_val does not amplify beyond the latent's own scale, so the
# correction adds nothing that would need a wider bound.  It stays at v5's.
V8_TOL = 3.8e-6


def tag17(solver, order, skip, ratio, leg, extra):
    return (f"{'unipc' if solver == 'unipc' else 'dpmpp'}{order}_{skip}_r{ratio:g}_{leg}" + "".join(f"_{k}" for k in sorted(extra))).replace(".", "p")


def tag18(solver, order, skip, ratio, leg, scale):
    return f"{'unipc' if solver == 'unipc' else 'dpmpp'}{order}_{skip}_r{ratio:g}_{leg}_s{scale:g}".replace(".", "p")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---- the quantile --------------------------------------------------------------------------------
def _torch_q(a, p):
    return torch.quantile(torch.from_numpy(np.abs(np.asarray(a, np.float32)).reshape(-1)), float(p)).numpy()


@pytest.mark.parametrize("p", [0.0, 0.5, 0.995, 1.0])
@pytest.mark.parametrize("n", [1, 2, 12, 444, 6600])
def test_abs_quantile_equals_torch_quantile_bitwise_random(n, p):
    rng = np.random.default_rng(n)
    for rep in range(8):
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4)).astype(np.float32)
        assert S.abs_quantile(a, p).tobytes() == _torch_q(a, p).tobytes(), (n, p, rep)
    assert S.abs_quantile(a.reshape(-1, 1) if n % 2 else a.reshape(2, -1), p).tobytes() == _torch_q(a, p).tobytes()      # any shape: flattened


@pytest.mark.parametrize("p", [0.0, 0.5, 0.995, 1.0])
def test_abs_quantile_equal_and_tied_arrays(p):
    f = np.float32
    for n in (1, 2, 12, 444):
        a = np.full(n, -0.37, f)                                   # all equal
        assert S.abs_quantile(a, p).tobytes() == _torch_q(a, p).tobytes() == f(0.37).tobytes()
    rng = np.random.default_rng(3)
    for n in (12, 444, 6600):                                      # ties exactly at ranks lo and hi, distinct values around them
        a = np.sort(np.abs(rng.standard_normal(n).astype(f)))
        pos = f(p) * f(n - 1)
        lo, hi = int(np.floor(pos)), int(np.ceil(pos))
        a[hi] = a[lo]
        if lo > 0:
            a[lo - 1] = a[lo]
        a = rng.permutation(a) * np.where(rng.random(n) < 0.5, f(-1), f(1))
        assert S.abs_quantile(a, p).tobytes() == _torch_q(a, p).tobytes(), (n, p)


def test_abs_quantile_rejects_bad_arguments():
    for p in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError):
            S.abs_quantile(np.ones(4, np.float32), p)
    with pytest.raises(ValueError):
        S.abs_quantile(np.ones(0, np.float32), 0.5)


def test_correct_x0_is_the_reference_formula_per_item():
    """against torch's statement of dynamic_thresholding_fn, item by item at its own length; clamp; mode 0 returns m"""
    f = np.float32
    rng = np.random.default_rng(7)
    m = (2.0 * rng.standard_normal((3, 5, 8))).astype(f)
    lens = [8, 7, 5]
    y = S.correct_x0(m, "dynamic_thresholding", 0.75, 1.2, lengths=lens)
    for b, L in enumerate(lens):
        x0 = torch.from_numpy(m[b:b + 1, :, :L])
        s = torch.quantile(x0.abs().reshape(1, -1), 0.75, dim=1)
        s = torch.maximum(s, 1.2 * torch.ones_like(s)).reshape(1, 1, 1)
        assert np.array_equal(y[b, :, :L], (torch.clamp(x0, -s, s) / s).numpy()[0])
    assert np.array_equal(S.correct_x0(m, "clamp", max_val=0.5), np.clip(m, f(-0.5), f(0.5)))
    assert S.correct_x0(m, None) is not None and np.array_equal(S.correct_x0(m, None), m) and np.array_equal(S.correct_x0(m, 0), m)
    assert np.array_equal(S.correct_x0(m, 1, 0.75, 1.2, lengths=lens), y) and np.array_equal(S.correct_x0(m, 2, max_val=0.5), S.correct_x0(m, "clamp", max_val=0.5))


# ---- the goldens ---------------------------------------------------------------------------------
def test_golden_grid_is_the_one_asked_for(gold):
    """both solvers, orders 1-3, three legs of max_val, denoise_to_zero, two fractional positions and an integer one, guided"""
    want = {f"g17.{tag17(*c)}" for c in CASES17} | {f"g18.{tag18(*c)}" for c in CASES18}
    have = {k[:-3] for k in gold.files if k.endswith(".y0")}
    assert have == want and len(want) == len(CASES17) + len(CASES18) == 56
    assert os.path.getsize(GOLD) <= 400 * 1024
    assert tuple(gold["lens"]) == LENS and [gold[f"x_T{b}"].shape for b in range(3)] == [(1, 5, L) for L in LENS]
    f = np.float32
    pos = {(r, L): float(f(r) * f(5 * L - 1)) for r in (0.9, 0.75) for L in LENS}
    assert pos[(0.75, 5)] == 18.0                                                        # an integer position
    assert sum(1 for (r, L), v in pos.items() if v != np.floor(v)) >= 4                  # at least two lengths with a fractional one
    assert {c[1] for c in CASES17} == {1, 2, 3} and any(c[5].get("denoise_to_zero") for c in CASES17)


def test_legs_a_and_b_clamp_in_the_goldens(gold):
    """leg a (max_val below every quantile) and leg b (max_val between the item's 0.9-quantile and its largest |x0| at the first evaluation) clamp more than 0.1 % of the
    elements on some step in EVERY case and item (ratio 1 aside: the quantile is the maximum there, nothing lies beyond it); leg c never does"""
    for prefix, cases, tag in (("g17", CASES17, tag17), ("g18", CASES18, tag18)):
        for c in cases:
            for b in range(3):
                share = gold[f"{prefix}.{tag(*c)}.clamped{b}"]
                if c[4] == "c" or c[3] == 1.0:
                    assert float(share.max()) == 0.0, (c, b)
                else:
                    assert float(share.max()) > 1e-3, (c, b, share)
                if c[4] == "b":
                    assert float(share[0]) > 1e-3, (c, b)                                   # the first evaluation, by construction
    mv = gold["g17.maxval"]                                                                 # (legs, items)
    assert mv.shape == (3, 3) and (mv[0] < gold["g17.maxval.q75_plain"].min()).all() and (mv[2] > gold["g17.maxval.absmax_plain"].max()).all()
    assert (gold["g17.maxval.q90_plain"][:, 0] < mv[1]).all() and (mv[1] < gold["g17.maxval.absmax_plain"][:, 0]).all()


def _host(gold, solver, order, skip, ratio, max_val, b, extra, guide=None):
    t = S.build_table(solver, STEPS, order=order, skip_type=skip, **extra)
    if guide is None:
        fn = synthetic_x0
    else:
        fn = lambda x, tm: S.guided_x0(synthetic_x0(x, tm, gold["uncond"]), synthetic_x0(x, tm, gold["cond"]), np.float32(guide))      # noqa: E731
    return t, S.run_table_numpy(t, fn, gold[f"x_T{b}"], correct_x0=dict(mode="dynamic_thresholding", ratio=ratio, max_val=max_val))


@pytest.mark.parametrize("case", CASES17, ids=[tag17(*c) for c in CASES17])
def test_run_table_numpy_corrected_against_reference(case, gold):
    """``run_table_numpy(correct_x0=...)`` reproduces the reference's UniPC / DPM-Solver++ constructed with correcting_x0_fn="dynamic_thresholding",
    every item alone at its own length.  Recorded worst case 6.8e-7; gated at v5's 3.8e-6 (V8_TOL)."""
    solver, order, skip, ratio, leg, extra = case
    tag = tag17(*case)
    for b in range(3):
        t, y = _host(gold, solver, order, skip, ratio, float(gold["g17.maxval"][LEGS.index(leg), b]), b, extra)
        times = gold[f"g17.{tag}.times"]
        assert t.steps == len(times) == STEPS + int(bool(extra.get("denoise_to_zero")))
        np.testing.assert_allclose(t.t_model, times, rtol=1e-6, atol=2e-4)
        e = rel_l2(y, gold[f"g17.{tag}.y{b}"])
        print(f"{tag} item {b}: {e:.3e}")
        assert e <= V8_TOL, (b, e)


@pytest.mark.parametrize("case", CASES18, ids=[tag18(*c) for c in CASES18])
def test_run_table_numpy_corrected_guided_against_reference(case, gold):
    """the same through the reference's classifier-free guidance (the noise model of golden_v7): the threshold is the quantile of the GUIDED x0.
    Recorded worst case 1.1e-6 (scales 2.5 and 7); gated at 3.8e-6."""
    solver, order, skip, ratio, leg, scale = case
    tag = tag18(*case)
    for b in range(3):
        max_val = float(gold["g18.maxval_s" + f"{scale:g}".replace(".", "p")][LEGS.index(leg), b])
        t, y = _host(gold, solver, order, skip, ratio, max_val, b, {}, guide=scale)
        assert t.steps == len(gold[f"g18.{tag}.times"])
        e = rel_l2(y, gold[f"g18.{tag}.y{b}"])
        print(f"{tag} item {b}: {e:.3e}")
        assert e <= V8_TOL, (b, e)


def test_report_records_the_measured_errors():
    r = json.load(open(REPORT))
    assert r["g17.worst_host_rel_l2"] <= V8_TOL and r["g18.worst_host_rel_l2"] <= V8_TOL
    assert all(max(v["host_rel_l2"]) <= V8_TOL for v in r.values() if isinstance(v, dict) and "host_rel_l2" in v)


def test_the_correction_matters_and_defaults_to_off(gold):
    """off by default (the existing behaviour and its tests are untouched); leg a moves the latent, and the legs differ"""
    t = S.build_table("unipc", STEPS, order=2)
    x = gold["x_T0"]
    plain = S.run_table_numpy(t, synthetic_x0, x)
    assert np.array_equal(plain, S.run_table_numpy(t, synthetic_x0, x, correct_x0=None))
    assert np.array_equal(plain, S.run_table_numpy(t, synthetic_x0, x, correct_x0=dict(mode=None, ratio=0.5, max_val=0.1)))
    ys = [gold[f"g17.{tag17('unipc', 2, 'time_uniform', 0.9, leg, {})}.y0"] for leg in LEGS]
    assert rel_l2(ys[0], plain) > 1e-2 and rel_l2(ys[0], ys[1]) > 1e-2 and rel_l2(ys[1], ys[2]) > 1e-2
    # ragged: item b of a padded batch == the item alone at its own length (the quantile runs over its own frames)
    L = 5
    xb = np.zeros((2, 5, 8), np.float32)
    xb[0], xb[1, :, :L] = gold["x_T0"][0], gold["x_T2"][0]
    k = dict(mode="dynamic_thresholding", ratio=0.75, max_val=float(gold["g17.maxval"][0, 0]))
    yb = S.run_table_numpy(t, synthetic_x0, xb, correct_x0=dict(k, lengths=[8, L]))
    alone = S.run_table_numpy(t, synthetic_x0, gold["x_T2"], correct_x0=k)
    assert np.array_equal(yb[1, :, :L], alone[0])
    with pytest.raises(ValueError, match="stochastic"):
        S.run_table_numpy(S.build_table("ddim", 4, S.linear_betas(1000, np.float64), eta=1.0), synthetic_x0, x, noise_fn=lambda i: np.zeros_like(x), correct_x0=k)


# ---- keyword validation --------------------------------------------------------------------------
BAD = [
    (dict(correcting_x0_fn=lambda x0, t: x0), "callable"),
    (dict(correcting_x0_fn="dynamic"), "correcting_x0_fn"),
    (dict(correcting_x0_fn=3), "correcting_x0_fn"),
    (dict(correcting_x0_fn=1), "correcting_x0_fn"),                                         # the engine's mode numbers are not names
    (dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=1.5), "ratio"),
    (dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=-0.1), "ratio"),
    (dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=float("nan")), "ratio"),
    (dict(correcting_x0_fn="clamp", thresholding_max_val=0.0), "max_val"),
    (dict(correcting_x0_fn="clamp", thresholding_max_val=float("inf")), "max_val"),
    (dict(correcting_x0_fn=None, thresholding_max_val=-1.0), "max_val"),                   # out of range even while off
]


@pytest.mark.parametrize("kw,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_correction_keywords_raise_before_any_engine_call(kw, match, monkeypatch):
    """the checks run in front of everything: no engine call is recorded"""
    d, rec = _denoiser(monkeypatch)
    c, p = torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256))
    with pytest.raises(ValueError, match=match):
        d.sample(c, p, solver="unipc", steps=5, **kw)
    assert rec.calls == []
    with pytest.raises(ValueError, match=match):
        S.check_x0_correction(kw.get("correcting_x0_fn"), kw.get("dynamic_thresholding_ratio", 0.995), kw.get("thresholding_max_val", 1.0), names_only=True)


@pytest.mark.parametrize("solver", ["ddim", "ddpm"])
def test_correction_is_refused_for_the_discrete_samplers(solver, monkeypatch):
    d, rec = _denoiser(monkeypatch)
    c, p = torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256))
    with pytest.raises(ValueError, match="unipc / dpmsolver"):
        d.sample(c, p, solver=solver, steps=None if solver == "ddpm" else 5, correcting_x0_fn="clamp")
    assert rec.calls == []
    from ns2vc_amd.pipeline import OverlappedPipeline                                       # noqa: F401  (needs a device to construct)
    from ns2vc_amd.service import GroupedConverter
    with pytest.raises(ValueError, match="unipc / dpmsolver"):
        GroupedConverter(None, None, solver=solver, steps=5, correcting_x0_fn="clamp")


def test_corrected_tail_min_is_the_stated_rule():
    """ceil(log3(g e1 / bar)), g = 2 x the guidance gain; a floor under the default tail, for 16-bit loops under a correction only"""
    from ns2vc_amd.pipeline import EVALUATION_ERROR, PARITY_BAR, corrected_tail_min
    assert [corrected_tail_min(p) for p in ("fp16", "bf16", "fp32")] == [1, 3, 0]
    assert corrected_tail_min("fp16", [0.5, 1.0]) == 1 and corrected_tail_min("fp16", [2.5, 0.5]) == 2 and corrected_tail_min("bf16", [7.0]) == 5
    for p, e1 in EVALUATION_ERROR.items():
        n = corrected_tail_min(p)
        assert 2 * e1 / 3 ** n <= PARITY_BAR < 2 * e1 / 3 ** (n - 1)


def test_denoiser_raises_the_default_tail_under_a_correction(monkeypatch):
    """fp16 UniPC order 2: no default tail; 1 under a correction; tail_fp32= still overrides; DPM-Solver++(3M)'s 4 stay 4"""
    d, rec = _denoiser(monkeypatch, "fp16")
    c, p, x = torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256)), torch.zeros(2, 100, 16)
    on = dict(correcting_x0_fn="dynamic_thresholding")
    d.sample(c, p, noise=x, solver="unipc", steps=6)
    d.sample(c, p, noise=x, solver="unipc", steps=6, **on)
    d.sample(c, p, noise=x, solver="unipc", steps=6, tail_fp32=0, **on)
    d.sample(c, p, noise=x, solver="dpmsolver++", steps=6, order=3, **on)
    d, rec16 = _denoiser(monkeypatch, "bf16")
    d.sample(c, p, noise=x, solver="unipc", steps=6, correcting_x0_fn="clamp")
    assert [a["tail_steps"] for a in rec.of("sample") + rec16.of("sample")] == [0, 1, 0, 4, 3]
    assert [a["tail"] for a in rec.of("sample") + rec16.of("sample")] == [None, "tail", None, "tail", "tail"]


def test_engine_set_x0_correction_validates_on_the_host():
    from ns2vc_amd.engine import Engine
    e = Engine.__new__(Engine)       # (no device: only the argument checks in front of the C call)
    e.x0_correction = None
    for a in (("thresholding",), (lambda x: x,), ("clamp", 2.0), ("clamp", 0.5, 0.0), ("dynamic_thresholding", 0.5, float("nan"))):
        with pytest.raises(ValueError):
            e.set_x0_correction(*a)


def test_denoiser_routes_the_keywords_to_the_engine(monkeypatch):
    """on: set before the loop with the three values; the defaults reach nothing; a later call without the keywords turns it off again"""
    d, rec = _denoiser(monkeypatch)
    c, p, x = torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256)), torch.zeros(2, 100, 16)
    d.sample(c, p, noise=x, solver="unipc", steps=5)
    d.sample(c, p, noise=x, solver="unipc", steps=5, thresholding_max_val=2.0, dynamic_thresholding_ratio=0.5)      # off: the values go nowhere
    assert not rec.of("set_x0_correction")
    d.sample(c, p, noise=x, solver="dpmsolver++", steps=5, order=3, correcting_x0_fn="dynamic_thresholding", thresholding_max_val=2.0,
             dynamic_thresholding_ratio=0.9)
    assert rec.of("set_x0_correction") == [dict(mode="dynamic_thresholding", ratio=0.9, max_val=2.0)]
    names = rec.names()
    assert names.index("set_x0_correction") < len(names) - 1 and names[-1] == "sample" and "sample" not in names[names.index("set_x0_correction"):-1]
    assert rec.engines[0].x0_correction == (1, float(np.float32(0.9)), 2.0)
    d.sample(c, p, noise=x, solver="unipc", steps=5, correcting_x0_fn="clamp")
    assert rec.engines[0].x0_correction == (2, float(np.float32(0.995)), 1.0)
    d.sample(c, p, noise=x, solver="unipc", steps=5)
    assert rec.of("set_x0_correction")[-1] == dict(mode=None, ratio=0.995, max_val=1.0) and rec.engines[0].x0_correction is None
    assert "sample" not in rec.names()[len(rec.names()) - 1 - rec.names()[::-1].index("set_x0_correction"):-1]      # (off before the last loop ran)


def test_grouped_converter_and_sharded_pass_the_keywords_through():
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import GroupedConverter
    from ns2vc_amd.spec import UNetConfig
    g = GroupedConverter(None, None, correcting_x0_fn="dynamic_thresholding", thresholding_max_val=1.5, dynamic_thresholding_ratio=0.9)
    assert g.kw["correcting_x0_fn"] == "dynamic_thresholding" and g.kw["thresholding_max_val"] == 1.5 and g.kw["dynamic_thresholding_ratio"] == 0.9
    assert "correcting_x0_fn" not in GroupedConverter(None, None).kw
    d = Denoiser.__new__(Denoiser)
    d.cfg = UNetConfig()
    seen = {}

    def fake_sample(content, prompt, prompt_mask=None, noise=None, **kw):
        seen.update(kw)
        return noise
    d.sample = fake_sample
    c, p, x = torch.zeros((3, 256, 8)), torch.zeros((3, 4, 256)), torch.zeros(3, 100, 8)
    d.sample_sharded(c, p, None, x, solver="unipc", steps=4, correcting_x0_fn="clamp", thresholding_max_val=0.7)
    assert seen["correcting_x0_fn"] == "clamp" and seen["thresholding_max_val"] == 0.7


# ---- the library ---------------------------------------------------------------------------------
def test_library_exports_the_three_symbols_abi_still_7():
    from ns2vc_amd import _lib
    lib = _lib.load()
    assert lib.ns2vc_abi_version() == 7
    hdr = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    raw = C.CDLL(lib._name)
    for sym in ("ns2vc_sampler_set_x0_correction", "ns2vc_k_abs_quantile", "ns2vc_k_solver_update_corrected"):
        assert hasattr(raw, sym), sym
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
    assert lib.ns2vc_sampler_set_x0_correction(None, 1, 0.9, 1.0) != 0      # a null handle is an error, not a crash
    assert b"null engine handle" in lib.ns2vc_last_error()
