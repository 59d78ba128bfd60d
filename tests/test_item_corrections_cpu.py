"""Per-item x0 correction, host side: the host statements with a per-item list against every item run alone under its own setting,
the routing and the refusals of the Python layer without a device, the new exports, and the register audit of the two new kernels."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from ns2vc_amd import noise as N
from ns2vc_amd import schedule as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B64 = S.linear_betas(1000, np.float64)
ITEM = (6, 10)          # one item's state: (channels, frames)
U2_4 = dict(solver="unipc", steps=4, order=2)
U3_5 = dict(solver="unipc", steps=5, order=3, variant="bh1")
D3_6 = dict(solver="dpmsolver++", steps=6, order=3, skip_type="logSNR")
D2_3 = dict(solver="dpmsolver++", steps=3, order=2)
DDIM_5 = dict(solver="ddim", steps=5, eta=1.0)
# off / dynamic / dynamic with another ratio and max_val / clamp, and a DDIM eta 1 item with None in the same batch
SPECS = [U2_4, U3_5, D3_6, D2_3, DDIM_5]
SETTINGS = [None, dict(mode="dynamic_thresholding", ratio=0.9, max_val=0.6), dict(mode="dynamic_thresholding", ratio=0.7, max_val=0.3),
            dict(mode="clamp", ratio=0.995, max_val=0.5), None]


def _x0(x, t):
    """per-item-independent toy model whose values pass 1 often, so that every setting above changes the trajectory"""
    t = np.asarray(t, np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    return (np.float32(1.6) * np.tanh(x * np.float32(0.9)) + np.float32(0.1) * np.sin(t * np.float32(0.01) + x)).astype(np.float32)


def _gauss(b, j):
    return N.gauss(77 + b, j, *ITEM)[0]


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / np.linalg.norm(b.astype(np.float64)))


def _alone(tab, x_T, setting, b):
    return S.run_table_numpy(tab, _x0, x_T[None], noise_fn=lambda j: _gauss(b, j)[None], correct_x0=setting)[0]


def test_run_tables_numpy_per_item_list_equals_every_item_alone():
    x_T = np.random.default_rng(11).standard_normal((len(SPECS),) + ITEM).astype(np.float32)
    tabs = S.build_tables(SPECS, None, B64)
    assert sorted(int(r) for r in tabs.item_rows) == [3, 4, 5, 5, 6]
    y = S.run_tables_numpy(tabs, _x0, x_T, noise_fn=_gauss, correct_x0=list(SETTINGS))
    for b in range(len(SPECS)):
        assert np.array_equal(y[b], _alone(tabs.table_of(b), x_T[b], SETTINGS[b], b)), b
        if SETTINGS[b] is not None:      # the setting matters ...
            assert _rel(y[b], _alone(tabs.table_of(b), x_T[b], None, b)) > 1e-3, b
    # ... and a swapped record cannot pass: two items given each other's settings differ
    for a, b in ((1, 2), (2, 3), (1, 3)):
        assert _rel(_alone(tabs.table_of(a), x_T[a], SETTINGS[b], a), y[a]) > 1e-3, (a, b)
        assert _rel(_alone(tabs.table_of(b), x_T[b], SETTINGS[a], b), y[b]) > 1e-3, (a, b)


def test_run_tables_numpy_per_item_lengths():
    """an entry's own ``lengths``: the quantile of that item runs over its own frames"""
    x_T = np.random.default_rng(12).standard_normal((2,) + ITEM).astype(np.float32)
    tabs = S.build_tables([U2_4, U2_4], None, B64)
    sets = [dict(SETTINGS[1], lengths=[7]), dict(SETTINGS[1], lengths=4)]
    y = S.run_tables_numpy(tabs, _x0, x_T, correct_x0=sets)
    for b, L in enumerate((7, 4)):
        assert np.array_equal(y[b], _alone(tabs.table_of(b), x_T[b], dict(SETTINGS[1], lengths=[L]), b))
    assert not np.array_equal(y[1], _alone(tabs.table_of(1), x_T[1], SETTINGS[1], 1))


def test_run_slots_numpy_fourth_tuple_element_with_an_admission_in_mid_loop():
    tab = [S.build_table(sp["solver"], sp["steps"], B64 if sp["solver"] in S.DISCRETE_SOLVERS else None, sp.get("order", 2), sp.get("eta", 0.0),
                         **{k: v for k, v in sp.items() if k not in ("solver", "steps", "order", "eta")}) for sp in SPECS]
    rng = np.random.default_rng(13)
    x = [rng.standard_normal(ITEM).astype(np.float32) for _ in range(6)]
    # slot 1 runs the clamped 3-step item, then takes the dynamic order-3 item at loop step 4 while slots 0 and 2 run across the admission
    tl = [[(tab[1], 0, x[0], SETTINGS[1]), (tab[4], 6, x[1], None)],
          [(tab[3], 0, x[2], SETTINGS[3]), (tab[2], 4, x[3], SETTINGS[2])],
          [(tab[4], 1, x[4], None), (tab[0], 7, x[5])]]
    res = S.run_slots_numpy(tl, _x0, (3,) + ITEM, noise_fn=lambda b, k, j: N.gauss(1000 * b + k, j, *ITEM)[0])
    for b, items in enumerate(tl):
        for k, item in enumerate(items):
            cor = item[3] if len(item) > 3 else None
            alone = S.run_table_numpy(item[0], _x0, item[2][None], noise_fn=lambda j, b=b, k=k: N.gauss(1000 * b + k, j, *ITEM), correct_x0=cor)[0]
            assert np.array_equal(res[b][k], alone), (b, k)
            if cor is not None:
                plain = S.run_table_numpy(item[0], _x0, item[2][None], correct_x0=None)[0]
                assert _rel(res[b][k], plain) > 1e-3, (b, k)


def test_host_statements_refuse_a_corrected_stochastic_item_and_keep_the_dict_form():
    x_T = np.zeros((2,) + ITEM, np.float32)
    tabs = S.build_tables([U2_4, DDIM_5], None, B64)
    with pytest.raises(ValueError, match="ddim / ddpm have no correction"):
        S.run_tables_numpy(tabs, _x0, x_T, noise_fn=_gauss, correct_x0=[None, SETTINGS[3]])
    with pytest.raises(ValueError, match="1 per-item x0 corrections for 2 items"):
        S.run_tables_numpy(tabs, _x0, x_T, noise_fn=_gauss, correct_x0=[None])
    with pytest.raises(ValueError, match="callable"):
        S.run_tables_numpy(tabs, _x0, x_T, noise_fn=_gauss, correct_x0=[dict(mode=lambda m: m), None])
    with pytest.raises(ValueError, match="stochastic item"):      # the dict form: its meaning and its refusal as before
        S.run_tables_numpy(tabs, _x0, x_T, noise_fn=_gauss, correct_x0=SETTINGS[3])
    S.run_tables_numpy(tabs, _x0, x_T, noise_fn=_gauss, correct_x0=[dict(mode=None), dict(mode=0)])      # mode off on a ddim item is no correction
    tab = tabs.table_of(1)
    with pytest.raises(ValueError, match="ddim / ddpm have no correction"):
        S.run_slots_numpy([[(tab, 0, x_T[0], SETTINGS[1])]], _x0, (1,) + ITEM, noise_fn=lambda b, k, j: _gauss(b, j))
    with pytest.raises(ValueError, match="not both"):
        S.run_slots_numpy([[(tabs.table_of(0), 0, x_T[0], SETTINGS[1])]], _x0, (1,) + ITEM, correct_x0=SETTINGS[3])


# ---- routing and refusals without a device (the recording engine of tests/recording_engine.py) ---------------------
def _den(monkeypatch, precision="fp32"):
    """the real constructor on the recording engine; ``den.rec`` is the recording: a refusal from the Python side leaves ``den.rec.calls`` empty"""
    import recording_engine
    return recording_engine.denoiser(monkeypatch, precision)[0]


DYN = dict(correcting_x0_fn="dynamic_thresholding", thresholding_max_val=0.5, dynamic_thresholding_ratio=0.9)
CLAMP = dict(correcting_x0_fn="clamp", thresholding_max_val=0.7)


def test_sample_routes_equal_entries_to_the_loop_wide_path(monkeypatch):
    """B equal entries: the call goes on as ``correcting_x0_fn=`` of that entry (and all None: as no correction at all)"""
    den = _den(monkeypatch)
    rec = den.rec
    c, p = torch.zeros(3, 256, 66), torch.zeros(3, 5, 256)
    den.sample(c, p, steps=4, corrections=[DYN, dict(DYN), DYN])
    assert rec.of("set_x0_correction") == [dict(mode="dynamic_thresholding", ratio=0.9, max_val=0.5)]
    assert not rec.of("set_x0_correction_items") and [m for m in rec.names() if m.startswith("load")] == ["load_sampler"]
    den.sample(c, p, steps=4, corrections=[None, None, None])
    assert rec.of("set_x0_correction")[1:] == [dict(mode=None, ratio=0.995, max_val=1.0)]      # (off again; nothing else)
    assert not rec.of("set_x0_correction_items") and [m for m in rec.names() if m.startswith("load")] == ["load_sampler"]
    den.sample(c, p, steps=4, corrections=[DYN, CLAMP, None])                                   # different entries go on to the engine: the per-item path
    assert rec.of("set_x0_correction_items") == [dict(modes=["dynamic_thresholding", "clamp", None], ratios=[0.9, 0.995, 0.995], max_vals=[0.5, 0.7, 1.0])]
    assert len(rec.of("set_x0_correction")) == 2 and [m for m in rec.names() if m.startswith("load")] == ["load_sampler", "load_samplers"]


def test_sample_refusals_reach_no_engine_call(monkeypatch):
    den = _den(monkeypatch)
    c, p = torch.zeros(3, 256, 66), torch.zeros(3, 5, 256)
    with pytest.raises(ValueError, match="exclude each other"):
        den.sample(c, p, steps=4, corrections=[DYN, None, None], correcting_x0_fn="clamp")
    with pytest.raises(ValueError, match=r"corrections\[2\].*ddim / ddpm have no correction"):
        den.sample(c, p, steps=4, corrections=[DYN, None, CLAMP], schedules=[None, None, dict(solver="ddim", steps=5, eta=1.0)])
    with pytest.raises(ValueError, match=r"one entry \(dict or None\) per item \(3\), got 2"):
        den.sample(c, p, steps=4, corrections=[DYN, None])
    with pytest.raises(ValueError, match=r"corrections\[1\].*callable"):
        den.sample(c, p, steps=4, corrections=[DYN, lambda m: m, None])
    with pytest.raises(ValueError, match=r"corrections\[0\].*callable"):
        den.sample(c, p, steps=4, corrections=[dict(correcting_x0_fn=lambda m: m), None, None])
    with pytest.raises(ValueError, match=r"corrections\[0\].*must be None, 'dynamic_thresholding' or 'clamp'"):
        den.sample(c, p, steps=4, corrections=[dict(correcting_x0_fn=1), None, None])      # names only
    with pytest.raises(ValueError, match=r"corrections\[1\].*thresholding_max_val"):
        den.sample(c, p, steps=4, corrections=[None, dict(CLAMP, thresholding_max_val=0.0), None])
    with pytest.raises(ValueError, match=r"corrections\[1\].*unknown keys"):
        den.sample(c, p, steps=4, corrections=[None, dict(CLAMP, ratio=0.5), None])
    with pytest.raises(ValueError, match="ddim"):      # a corrected ddim call without schedules=
        den.sample(c, p, solver="ddim", steps=5, eta=1.0, corrections=[DYN, None, None])
    assert den.rec.calls == []


def _loop(monkeypatch, precision="fp16", item_corrections=True, stochastic=True, order3=True, B=3, T=66, Lp=5):
    """an open slot loop on the recording engine (tensors on the host); the calls of opening it dropped"""
    den = _den(monkeypatch, precision)
    lp = den.open_slots(B, T, Lp, order3=order3, stochastic=stochastic, item_corrections=item_corrections)
    lp.dev = torch.device("cpu")
    den.rec.calls.clear()
    return lp


def test_open_slots_refuses_item_corrections_with_the_loop_wide_setting(monkeypatch):
    den = _den(monkeypatch)
    with pytest.raises(ValueError, match="exclude each other"):
        den.open_slots(3, 66, 5, item_corrections=True, correcting_x0_fn="clamp")
    from ns2vc_amd.service import ContinuousConverter
    with pytest.raises(ValueError, match="exclude each other"):
        ContinuousConverter(None, den, slots=3, max_frames=66, max_prompt=5, item_corrections=True, correcting_x0_fn="clamp")
    assert den.rec.calls == []


def test_slot_tail_needed_is_applied_per_request(monkeypatch):
    lp = _loop(monkeypatch, "fp16")
    assert lp.check_request(U2_4)[0] == S.schedule_key(U2_4)                       # uncorrected UniPC order 2 at fp16: no tail
    assert lp.check_request(U2_4, 1.0, None)[0] == S.schedule_key(U2_4)
    with pytest.raises(ValueError, match=r'corrected\) needs 1 trailing fp32 evaluation.*precision="fp32"'):
        lp.check_request(U2_4, 1.0, CLAMP)                                          # THIS request is corrected: corrected_tail_min
    lp.require_tail_free = False
    assert lp.check_request(U2_4, 1.0, CLAMP)[0] == S.schedule_key(U2_4)
    lp32 = _loop(monkeypatch, "fp32")
    for spec in (U2_4, U3_5, D3_6):
        assert lp32.check_request(spec, 1.0, DYN)[2] == S.table_flags(lp32._table(S.schedule_key(spec)))
    assert lp32.check_request(DDIM_5, 1.0, None)[2] == S.ITEM_NOISE              # stochastic and corrected requests share the loop ...
    with pytest.raises(ValueError, match="ddim / ddpm have no correction"):       # ... a corrected ddim request is refused
        lp32.check_request(DDIM_5, 1.0, CLAMP)
    with pytest.raises(ValueError, match="callable"):
        lp32.check_request(U2_4, 1.0, lambda m: m)
    with pytest.raises(ValueError, match="item_corrections=True"):
        _loop(monkeypatch, "fp32", item_corrections=False).check_request(U2_4, 1.0, CLAMP)
    lp32 = _loop(monkeypatch, "fp32")
    c, p, x = torch.zeros(256, 66), torch.zeros(5, 256), torch.zeros(100, 66)
    with pytest.raises(ValueError, match="ddim / ddpm have no correction"):       # through admit: no engine call is reached
        lp32.admit(0, c, p, x, schedule=DDIM_5, correction=CLAMP)
    with pytest.raises(ValueError, match="one correction"):
        lp32.admit_group([0, 1], [c, c], [p, p], [x, x], schedules=[U2_4, U2_4], corrections=[CLAMP])
    assert lp32.pool.rows_in_use() == 0 and lp32.corrections == [None] * 3 and lp32.den.rec.calls == []


def test_segment_correction_defaults_to_none():
    from ns2vc_amd.service import Segment
    assert Segment(torch.zeros(256, 4), torch.zeros(100, 4)).correction is None
    assert Segment(torch.zeros(256, 4), torch.zeros(100, 4), correction=CLAMP).correction == CLAMP


# ---- exports --------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ns2vc_sampler_set_x0_correction_items", "ns2vc_k_solver_update_items_corrected")


def test_new_symbols_are_declared_bound_and_exported():
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import Engine
    header = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    assert "#define NS2VC_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.PROTOTYPES
    assert callable(Engine.set_x0_correction_items) and "item_corrections" in Engine.open_slots.__code__.co_varnames
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.ns2vc_abi_version() == 7
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    mode, val = np.zeros(1, np.int32), np.ones(1, np.float32)
    assert lib.ns2vc_sampler_set_x0_correction_items(None, mode.ctypes.data, val.ctypes.data, val.ctypes.data, 1, None) != 0 and lib.ns2vc_last_error()
    assert lib.ns2vc_k_solver_update_items_corrected(None, 2, None, None, 1, None, None, None, 0, None, None, None, None, 0, 128, 1, None, None, None, 100,
                                                     mode.ctypes.data, val.ctypes.data, val.ctypes.data, None, None) != 0


# ---- register audit -------------------------------------------------------------------------------------------------
def test_mixed_kernels_use_no_scratch_and_the_old_counts_stand():
    """the compiler's kernel-resource-usage remarks on misc.hip: 6 instantiations <TM, GD> of solver_update_mixed_kernel and 2 <SRC> of
    abs_quantile_mixed_kernel -- no scratch, no spilled VGPR or SGPR; the counted kernels keep 12 / 18 / 24 / 2 and 3 emb_items"""
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
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and fn:
            out.setdefault(fn, {})[m.group(1)] = int(m.group(2))
    new = {n: v for n, v in out.items() if re.search(r"solver_update_mixed_kernel|abs_quantile_mixed_kernel", n)}
    count = lambda s: len([n for n in new if s in n])      # noqa: E731
    assert (count("solver_update_mixed_kernel"), count("abs_quantile_mixed_kernel")) == (6, 2), sorted(new)
    bad = [(n, v) for n, v in new.items() if v.get("ScratchSize [bytes/lane]", -1) != 0 or v.get("VGPRs Spill", -1) != 0 or v.get("SGPRs Spill", -1) != 0]
    assert not bad, bad
    old = lambda s: len([n for n in out if s in n])        # noqa: E731
    assert (old("solver_update_kernel"), old("solver_update_items_kernel"), old("solver_update_th_kernel"), old("abs_quantile_items_kernel")) == (12, 18, 24, 2)
    assert old("abs_quantile_kernel") == 3 and old("emb_items_from_table_kernel") == 3
