"""Per-item sampler schedules, host side: run_tables_numpy against run_table_numpy one item at a time, build_tables, the argument checks and
routing of Denoiser.sample(schedules=), the new exports and the register audit of the new kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from ns2vc_amd import noise as N
from ns2vc_amd import schedule as S
from recording_engine import denoiser as _denoiser      # the real Denoiser constructor on the recording engine -> (denoiser, recording)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B64 = S.linear_betas(1000, np.float64)
# the four schedules of the issue: UniPC-2 6 steps, DPM-Solver++(3M) 5 steps logSNR, UniPC-3 bh1 4 steps + denoise_to_zero, DDIM eta 1 5 steps
SPECS = [dict(solver="unipc", steps=6, order=2),
         dict(solver="dpmsolver++", steps=5, order=3, skip_type="logSNR"),
         dict(solver="unipc", steps=4, order=3, variant="bh1", denoise_to_zero=True),
         dict(solver="ddim", steps=5, eta=1.0)]
SHAPE = (4, 6, 10)
SEEDS = np.array([3, 5, 7, 11], np.uint64)


def _table(spec):
    kw = {k: v for k, v in spec.items() if k not in ("solver", "steps", "order", "eta")}
    return S.build_table(spec["solver"], spec["steps"], B64 if spec["solver"] in S.DISCRETE_SOLVERS else None, spec.get("order", 2),
                         spec.get("eta", 0.0), **kw)


def _x0(x, t):
    """per-item-independent synthetic model: depends on the item's own x and model time only"""
    t = np.asarray(t, np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    return (np.tanh(x * np.float32(0.7)) * np.float32(0.9) + np.float32(0.05) * np.sin(t * np.float32(0.01) + x)).astype(np.float32)


def _x0_cond(x, t, shift):
    return (_x0(x, t) + np.float32(shift) * np.cos(x)).astype(np.float32)


def _gauss(b, j):
    return N.gauss(int(SEEDS[b]), j, SHAPE[1], SHAPE[2])[0]


def test_run_tables_numpy_equals_each_item_alone():
    x_T = np.random.default_rng(0).standard_normal(SHAPE).astype(np.float32)
    tabs = S.build_tables(SPECS, None, B64)
    assert tabs.steps == 6 and tabs.start.tolist() == [0, 1, 1, 1]
    trace = []
    y = S.run_tables_numpy(tabs, _x0, x_T, trace=trace, noise_fn=_gauss)
    assert len(trace) == 6
    for b, spec in enumerate(SPECS):
        alone = S.run_table_numpy(_table(spec), _x0, x_T[b:b + 1], noise_fn=lambda i, b=b: _gauss(b, i)[None])
        assert np.array_equal(y[b:b + 1], alone), spec
    # a held item keeps x_T until its start
    assert np.array_equal(trace[0][1:], x_T[1:]) and not np.array_equal(trace[0][0], x_T[0])


@pytest.mark.parametrize("mode", [None, "clamp", "dynamic_thresholding"])
def test_run_tables_numpy_guided_and_corrected_subset(mode):
    """guidance (and a correction) on the non-stochastic subset: every item what run_table_numpy gives it alone"""
    specs, scales = SPECS[:3], np.array([2.5, 1.0, 0.5], np.float32)
    x_T = np.random.default_rng(1).standard_normal((3,) + SHAPE[1:]).astype(np.float32)
    corr = None if mode is None else dict(mode=mode, ratio=0.9, max_val=0.6)

    def both(x, t):      # cat([unconditional, conditional])
        n = x.shape[0] // 2
        return np.concatenate([_x0_cond(x[:n], t[:n], 0.0), _x0_cond(x[n:], t[n:], 0.3)], axis=0)

    y = S.run_tables_numpy(S.build_tables(specs), both, x_T, guided_x0=scales, correct_x0=corr)
    for b, spec in enumerate(specs):
        fn = lambda x, t, b=b: S.guided_x0(_x0_cond(x, t, 0.0), _x0_cond(x, t, 0.3), scales[b:b + 1])      # noqa: E731
        alone = S.run_table_numpy(_table(spec), fn, x_T[b:b + 1], correct_x0=corr)
        assert np.array_equal(y[b:b + 1], alone), (spec, mode)
    with pytest.raises(ValueError, match="stochastic"):
        S.run_tables_numpy(S.build_tables(SPECS, None, B64), _x0, np.zeros(SHAPE, np.float32), noise_fn=_gauss, correct_x0=dict(mode="clamp"))


def test_build_tables_dedupes_right_aligns_and_keeps_rows():
    specs = [SPECS[0], SPECS[1], dict(SPECS[0]), dict(solver="unipc", steps=6), SPECS[2]]      # (order 2 is the default: the same schedule)
    tabs = S.build_tables(specs)
    assert len(tabs.tables) == 3 and tabs.index.tolist() == [0, 1, 0, 0, 2]
    assert tabs.rows.tolist() == [6, 5, 5] and tabs.steps == 6 and tabs.start.tolist() == [0, 1, 0, 0, 1]
    off = np.concatenate([[0], np.cumsum(tabs.rows)])
    for k, spec in enumerate([SPECS[0], SPECS[1], SPECS[2]]):
        assert tabs.coef[off[k]:off[k + 1]].tobytes() == np.ascontiguousarray(_table(spec).coef, np.float32).tobytes()
    assert tabs.coef.dtype == np.float32 and tabs.coef.shape == (16, S.NCOEF)
    assert not tabs.uniform and S.build_tables([SPECS[1]] * 3).uniform
    # who is active where, and the model time of a held item is its clamped row's
    assert tabs.active_at(0).tolist() == [True, False, True, True, False] and tabs.active_at(5).all()
    assert tabs.t_model_at(0)[1] == _table(SPECS[1]).coef[0, 0] and tabs.t_model_at(3)[1] == _table(SPECS[1]).coef[2, 0]
    assert S.build_tables(specs, starts=[0, 0, 2, 1, 3]).steps == 8
    for bad, match in ((dict(solver="unipc", steps=6, foo=1), r"schedules\[1\].*foo"), (dict(solver="heun", steps=6), r"schedules\[1\].*solver"),
                       (dict(solver="unipc", steps=6, method="singlestep"), r"schedules\[1\].*multistep"), (dict(solver="unipc", steps=0), r"schedules\[1\]"),
                       (dict(solver="unipc", steps=2, order=3), r"schedules\[1\]")):
        with pytest.raises(ValueError, match=match):
            S.build_tables([SPECS[0], bad])


# ---- Denoiser.sample(schedules=): argument errors and routing (the recording engine of tests/recording_engine.py, no device) ---------
BAD = [(dict(schedules=[SPECS[0]]), "one schedule .* per item"),
       (dict(schedules=SPECS[0]), "one schedule .* per item"),
       (dict(schedules=[SPECS[0], dict(solver="unipc", steps=5, stride=2)]), r"schedules\[1\].*stride"),
       (dict(schedules=[SPECS[0], dict(solver="euler", steps=5)]), r"schedules\[1\].*solver"),
       (dict(schedules=[SPECS[0], dict(solver="unipc", steps=5, method="singlestep")]), r"schedules\[1\].*multistep"),
       (dict(schedules=[SPECS[3], SPECS[0]], correcting_x0_fn="clamp"), r"schedules\[0\].*correcting_x0_fn"),
       (dict(schedules=[SPECS[0], dict(solver="ddpm", steps=10)]), r"schedules\[1\].*ddpm"),
       (dict(schedules=[SPECS[0], dict(solver="unipc", steps=1, order=2)]), r"schedules\[1\]")]


@pytest.mark.parametrize("kw,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_schedules_raise_before_any_engine_call(kw, match, monkeypatch):
    d, rec = _denoiser(monkeypatch)
    with pytest.raises(ValueError, match=match):
        d.sample(torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256)), solver="unipc", steps=5, **kw)
    assert rec.calls == []


def _loads(rec):
    return [(m, a) for _, m, a in rec.calls if m.startswith("load")]


def test_equal_schedules_take_the_shared_table_path(monkeypatch):
    d, rec = _denoiser(monkeypatch)
    c, p, x = torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256)), torch.zeros(2, 100, 16)
    d.sample(c, p, noise=x, solver="unipc", steps=9, schedules=[SPECS[1], dict(SPECS[1])])
    d.sample(c, p, noise=x, solver="dpmsolver++", steps=5, order=3, skip_type="logSNR", schedules=[None, SPECS[1]])     # None = the call's own
    (name, a), = _loads(rec)                                                                                 # (the second call finds the table loaded)
    assert (name, a["solver"], a["steps"], a["order"], a["eta"], a["options"]) == ("load_sampler", "dpmsolver++", 5, 3, 0.0, dict(skip_type="logSNR"))
    assert rec.engines[0].tables is None and [a["x"][1] for a in rec.of("sample")] == [[2, 100, 16]] * 2


def test_mixed_schedules_take_the_per_item_path(monkeypatch):
    d, rec = _denoiser(monkeypatch)
    c, p, x = torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256)), torch.zeros(2, 100, 16)
    d.sample(c, p, noise=x, solver="unipc", steps=6, schedules=[None, SPECS[3]], seeds=[1, 2])
    assert [m for m, _ in _loads(rec)] == ["load_samplers"] and rec.of("set_seeds") == [dict(seeds=[1, 2])] and rec.names()[-1] == "sample"
    eng = rec.engines[0]
    assert eng.tables.keys == (S.schedule_key(SPECS[0]), S.schedule_key(SPECS[3])) and eng.tables.start.tolist() == [0, 1]
    d.sample(c, p, noise=x, solver="unipc", steps=6, schedules=[None, SPECS[3]], seeds=[1, 2])           # the same schedules: nothing is loaded again
    d.sample(c, p, noise=x, solver="unipc", steps=6)                                                      # and back to a shared table
    assert [m for m, _ in _loads(rec)] == ["load_samplers", "load_sampler"]


def test_default_tail_is_the_largest_any_item_asks_for():
    from ns2vc_amd.pipeline import default_tail_fp32
    assert max(default_tail_fp32(k[0], k[2]) for k in S.build_tables(SPECS, None, B64).keys) == 4      # DPM-Solver++(3M)
    assert max(default_tail_fp32(k[0], k[2]) for k in S.build_tables([SPECS[0], SPECS[2]]).keys) == 1  # UniPC-3


def test_grouped_converter_plan_ignores_schedules():
    from ns2vc_amd.service import GroupedConverter, Segment
    g = GroupedConverter.__new__(GroupedConverter)
    g.max_batch = 4
    shapes = [(40, 12), (32, 12), (40, 12), (32, 12), (40, 12), (32, 12)]
    plain = [Segment(torch.zeros(256, T), torch.zeros(100, Lp)) for T, Lp in shapes]
    mixed = [Segment(torch.zeros(256, T), torch.zeros(100, Lp), schedule=SPECS[i % 3]) for i, (T, Lp) in enumerate(shapes)]
    assert Segment(torch.zeros(256, 4), torch.zeros(100, 4)).schedule is None
    assert g.plan(mixed) == g.plan(plain) == [[0, 2, 4], [1, 3, 5]]


# ---- exports --------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ns2vc_sampler_load_items", "ns2vc_k_solver_update_items")


def test_new_symbols_are_declared_bound_and_exported():
    from ns2vc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    assert "#define NS2VC_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.PROTOTYPES
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.ns2vc_abi_version() == 7
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)


def test_null_handle_is_an_error_not_a_crash():
    from ns2vc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    rows, idx, start = np.array([2], np.int32), np.array([0], np.int32), np.array([0], np.int32)
    coef = np.zeros((2, S.NCOEF), np.float32)
    assert lib.ns2vc_sampler_load_items(None, 1, rows.ctypes.data, coef.ctypes.data_as(C.POINTER(C.c_float)), 1, idx.ctypes.data, start.ctypes.data, None) != 0
    assert lib.ns2vc_last_error()
    assert lib.ns2vc_k_solver_update_items(None, 2, None, None, 1, None, None, None, 0, None, None, None, None, 0, 128, 1, None, None, None, 100, 0, 0.995, 1.0,
                                           None, None) != 0


# ---- register audit -------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch_and_the_old_count_stands():
    """the compiler's kernel-resource-usage remarks on misc.hip: 18 instantiations <TM, GD, TH> of solver_update_items_kernel, 3 of
    emb_items_from_table_kernel, 2 of abs_quantile_items_kernel -- no scratch, no spilled VGPR; still twelve solver_update_kernel"""
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
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and fn:
            out.setdefault(fn, {})[m.group(1)] = int(m.group(2))
    new = {n: v for n, v in out.items() if re.search(r"solver_update_items_kernel|emb_items_from_table_kernel|abs_quantile_items_kernel", n)}
    count = lambda s: len([n for n in new if s in n])      # noqa: E731
    assert (count("solver_update_items_kernel"), count("emb_items_from_table_kernel"), count("abs_quantile_items_kernel")) == (18, 3, 2), sorted(new)
    bad = [(n, v) for n, v in new.items() if v.get("ScratchSize [bytes/lane]", -1) != 0 or v.get("VGPRs Spill", -1) != 0]
    assert not bad, bad
    assert len([n for n in out if "solver_update_kernel" in n]) == 12
