"""Continuous batching, host side: the slot timeline in numpy against every item run alone, the table pool, the scheduler, the new exports,
the register audit of the new kernels, and the refusals of a slot loop that are raised in front of the C call."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B64 = S.linear_betas(1000, np.float64)
U2_4, U2_6, U2_5 = (dict(solver="unipc", steps=n, order=2) for n in (4, 6, 5))
D3_5 = dict(solver="dpmsolver++", steps=5, order=3, skip_type="logSNR")
U3_4 = dict(solver="unipc", steps=4, order=3, variant="bh1", denoise_to_zero=True)
DDIM_5 = dict(solver="ddim", steps=5, eta=1.0)
ITEM = (6, 10)          # one item's state: (channels, frames)


def _table(spec):
    kw = {k: v for k, v in spec.items() if k not in ("solver", "steps", "order", "eta")}
    return S.build_table(spec["solver"], spec["steps"], B64 if spec["solver"] in S.DISCRETE_SOLVERS else None, spec.get("order", 2),
                         spec.get("eta", 0.0), **kw)


def _x0(x, t):
    """per-item-independent synthetic model: item b's value depends on its own x and its own model time only"""
    t = np.asarray(t, np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    return (np.tanh(x * np.float32(0.7)) * np.float32(0.9) + np.float32(0.05) * np.sin(t * np.float32(0.01) + x)).astype(np.float32)


def _seed(b, k):
    return 1000 * b + k + 3


def _gauss(b, k, j):
    return N.gauss(_seed(b, k), j, *ITEM)[0]


def _timeline(layout):
    """layout[b] = [(spec, start)] -> timeline[b] = [(table, start, x_T)], x_T drawn per (slot, item)"""
    return [[(_table(sp), st, np.random.default_rng(100 * b + k).standard_normal(ITEM).astype(np.float32)) for k, (sp, st) in enumerate(items)]
            for b, items in enumerate(layout)]


# the loop of the GPU test: slot 1 runs a 4-step item, is taken, and gets a 6-step item at loop step 4 while slots 0 and 2 run across the admission
LAYOUTS = {
    "order2": [[(U2_6, 0)], [(U2_4, 0), (U2_6, 4)], [(U2_5, 0)]],
    "order3": [[(D3_5, 1)], [(U2_4, 0), (U3_4, 4), (D3_5, 9)], [(U3_4, 2), (U2_4, 8)]],
    "ddim_eta1": [[(DDIM_5, 0), (U2_4, 7)], [(U2_4, 0), (DDIM_5, 4)], [(D3_5, 0)]],
}


@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_slot_timeline_equals_every_item_alone(name):
    tl = _timeline(LAYOUTS[name])
    trace = []
    res = S.run_slots_numpy(tl, _x0, (len(tl),) + ITEM, trace=trace, noise_fn=_gauss)
    assert len(trace) == max(st + tab.steps for items in tl for tab, st, _ in items)
    for b, items in enumerate(tl):
        for k, (tab, start, x_T) in enumerate(items):
            alone = S.run_table_numpy(tab, _x0, x_T[None], noise_fn=lambda j, b=b, k=k: _gauss(b, k, j)[None])
            assert np.array_equal(res[b][k], alone[0]), (name, b, k)
            # a finished item is held: its state stays until the slot's next admission
            nxt = items[k + 1][1] if k + 1 < len(items) else len(trace)
            for r in range(start + tab.steps - 1, nxt):
                assert np.array_equal(trace[r][b], alone[0]), (name, b, k, r)


def test_slot_timeline_agrees_with_run_tables_numpy_at_arbitrary_starts():
    specs, starts = [U2_6, D3_5, U3_4, DDIM_5], [3, 0, 5, 2]
    x_T = np.random.default_rng(5).standard_normal((4,) + ITEM).astype(np.float32)
    tabs = S.build_tables(specs, None, B64, starts=starts)
    y = S.run_tables_numpy(tabs, _x0, x_T, noise_fn=lambda b, j: _gauss(b, 0, j))
    res = S.run_slots_numpy([[(tabs.table_of(b), starts[b], x_T[b])] for b in range(4)], _x0, x_T.shape, noise_fn=_gauss)
    for b in range(4):
        assert np.array_equal(res[b][0], y[b])


def test_slot_timeline_refuses_overlapping_items():
    tl = _timeline([[(U2_6, 0), (U2_4, 5)]])
    with pytest.raises(ValueError, match="busy until 6"):
        S.run_slots_numpy(tl, _x0, (1,) + ITEM)
    with pytest.raises(ValueError, match="noise_fn"):
        S.run_slots_numpy(_timeline([[(DDIM_5, 0)]]), _x0, (1,) + ITEM)


# ---- the table pool -------------------------------------------------------------------------------------
def _coef(rows, tag):
    c = np.zeros((rows, S.NCOEF), np.float32)
    c[:, 0] = tag
    c[:, 1] = 1.0
    return c


def test_table_pool_dedupes_by_content():
    pool = S.TablePool(16)
    a, b = _coef(6, 1.0), _coef(4, 2.0)
    assert pool.acquire("a", a) == (0, True)
    assert pool.acquire("a-again", a.copy()) == (0, False)          # another key, the same rows: shared
    assert pool.acquire("b", b) == (6, True)
    assert pool.rows_in_use() == 10 and pool.resident() == 2
    pool.release("a")
    assert pool.rows_in_use() == 10                                  # "a-again" still walks them
    pool.release("a-again")
    assert pool.rows_in_use() == 4 and pool.resident() == 2          # unused, still resident: the next request of that schedule writes nothing
    assert pool.acquire("a", a) == (0, False)
    with pytest.raises(ValueError, match="not in use"):
        pool.release("never")


def test_table_pool_repacks_unused_tables_and_refuses_with_the_capacity():
    pool = S.TablePool(16)
    pool.acquire("a", _coef(6, 1.0))
    pool.acquire("b", _coef(6, 2.0))
    pool.release("a")
    assert pool.acquire("c", _coef(4, 3.0)) == (12, True)            # fits behind: nothing is dropped
    assert pool.resident() == 3
    assert pool.acquire("d", _coef(5, 4.0)) == (0, True)             # does not fit: the unused table goes, its rows are reused
    assert pool.resident() == 3 and pool.rows_in_use() == 15
    with pytest.raises(ValueError, match=r"6 rows does not fit.*capacity 16"):
        pool.acquire("a", _coef(6, 1.0))                             # live tables never move: refused, capacity named
    assert pool.rows_in_use() == 15                                  # a refusal changes nothing
    pool.release("b")
    assert pool.acquire("a", _coef(6, 1.0)) == (5, True)             # b's rows 6 .. 11 and row 5 are free now: first fit behind d
    with pytest.raises(ValueError, match="float32"):
        pool.acquire("bad", np.zeros((3, 5), np.float32))
    assert S.TablePool().capacity == 1024


# ---- the scheduler ----------------------------------------------------------------------------------------
def _check_plan(steps, n_slots, arrivals=None):
    ev = S.plan_slots(steps, n_slots, arrivals)
    arr = [0] * len(steps) if arrivals is None else arrivals
    admitted, taken, holder, busy_until = {}, {}, {}, {}
    last = -1
    for r, take, admit in ev:
        assert r > last
        last = r
        for b, i in take:
            assert holder.pop(b) == i and busy_until[b] == r         # taken exactly when it finishes
            taken[i] = r
        for b, i in admit:
            assert b not in holder, "slot double-booked"
            assert i not in admitted and arr[i] <= r
            holder[b], busy_until[b], admitted[i] = i, r + steps[i], r
    assert not holder and sorted(admitted) == sorted(taken) == list(range(len(steps)))      # every request served exactly once
    assert [i for _, _, a in ev for _, i in a] == list(range(len(steps)))                    # in queue order
    return ev, admitted, taken


def test_scheduler_serves_every_segment_once_and_never_double_books():
    rng = np.random.default_rng(0)
    for n_slots in (1, 3, 8):
        for n in (1, 7, 40):
            steps = [int(v) for v in rng.integers(1, 12, n)]
            _check_plan(steps, n_slots)
            arr = sorted(int(v) for v in rng.integers(0, 30, n))
            _check_plan(steps, n_slots, arr)
    with pytest.raises(ValueError):
        S.plan_slots([3, 0], 2)
    with pytest.raises(ValueError, match="non-decreasing"):
        S.plan_slots([3, 3], 2, [4, 1])
    assert S.plan_slots([], 3) == []


def test_scheduler_step_counts_are_minimal():
    """work-conserving list scheduling: a request starts at the earliest step at which it has arrived, everything in front of it in the queue
    has started and a slot is free -- checked against a direct simulation -- and the arithmetic of the measured workload (profiles/r18_continuous.txt)"""
    rng = np.random.default_rng(1)
    for n_slots, n in ((2, 9), (3, 7), (5, 30)):
        steps = [int(v) for v in rng.integers(1, 9, n)]
        arr = sorted(int(v) for v in rng.integers(0, 12, n))
        _, admitted, taken = _check_plan(steps, n_slots, arr)
        free, prev = [0] * n_slots, 0
        for i in range(n):
            b = min(range(n_slots), key=lambda k: free[k])
            start = max(free[b], arr[i], prev)
            assert admitted[i] == start and taken[i] == start + steps[i], i
            free[b], prev = start + steps[i], start
    # 7 segments on 3 slots with steps {4, 6} (the converter test): 34 slot-steps in 12 loop steps, the bound ceil(34 / 3) itself
    ev, _, taken = _check_plan([4, 6, 4, 6, 4, 6, 4], 3)
    assert max(taken.values()) == 12 and [r for r, _, _ in ev] == [0, 4, 6, 8, 10, 12]
    # the measurement's workload: 24 requests each at 10 / 20 / 30 / 50 steps on 32 slots (2640 slot-steps: no schedule under 82.5 loop steps;
    # closed batches of 32 sorted by steps: 20 + 30 + 50 = 100).  Longest first, by hand: 24 x 50 + 8 x 30 at 0; 8 x 30 at 30; 8 x 30 + 16 x 20 at
    # 50; 8 x 20 at 60; 16 x 10 at 70; 8 x 10 at 80 -> 90.  Shortest first leaves the 50-step requests to the end: the last 8 start at 50 -> 100.
    steps = [50] * 24 + [30] * 24 + [20] * 24 + [10] * 24
    assert max(_check_plan(steps, 32)[2].values()) == 90
    assert max(_check_plan(steps[::-1], 32)[2].values()) == 100


# ---- exports ----------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ns2vc_sampler_open", "ns2vc_sampler_rebase", "ns2vc_sampler_write_rows", "ns2vc_sampler_admit", "ns2vc_sampler_take", "ns2vc_sampler_slot_step",
               "ns2vc_unet_set_condition_items", "ns2vc_k_sampler_admit", "ns2vc_k_sampler_take")


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
    slots, rec, coef, step = np.array([0], np.int32), np.array([[0, 2, 0, 0]], np.int32), np.zeros((2, S.NCOEF), np.float32), C.c_int(7)
    assert lib.ns2vc_sampler_open(None, 0, 0, None) != 0 and lib.ns2vc_last_error()
    assert lib.ns2vc_sampler_write_rows(None, 0, 2, coef.ctypes.data_as(C.POINTER(C.c_float)), None) != 0
    assert lib.ns2vc_sampler_admit(None, 1, slots.ctypes.data, None, rec.ctypes.data, None) != 0
    assert lib.ns2vc_sampler_take(None, 1, slots.ctypes.data, None, None) != 0
    assert lib.ns2vc_unet_set_condition_items(None, 1, slots.ctypes.data, None, None, None, None) != 0
    assert lib.ns2vc_sampler_slot_step(None, C.byref(step)) != 0
    assert lib.ns2vc_k_sampler_admit(None, 100, 9, 1, slots.ctypes.data, 4, None, None, 0, None, None, None, None, 128, None, 0, None) != 0
    assert lib.ns2vc_k_sampler_take(None, 128, 100, 9, 1, slots.ctypes.data, 4, None, None) != 0


# ---- register audit ---------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch_and_the_old_counts_stand():
    """the compiler's kernel-resource-usage remarks on misc.hip: 3 instantiations <TM> of sampler_admit_kernel and of condition_items_kernel, one
    sampler_take_kernel -- no scratch, no spilled register; the per-item kernels keep their 18 + 3 + 2"""
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
    new = {n: v for n, v in out.items() if re.search(r"sampler_admit_kernel|sampler_take_kernel|condition_items_kernel", n)}
    count = lambda s: len([n for n in new if s in n])      # noqa: E731
    assert (count("sampler_admit_kernel"), count("sampler_take_kernel"), count("condition_items_kernel")) == (3, 1, 3), sorted(new)
    bad = [(n, v) for n, v in new.items() if v.get("ScratchSize [bytes/lane]", -1) != 0 or v.get("VGPRs Spill", -1) != 0 or v.get("SGPRs Spill", -1) != 0]
    assert not bad, bad
    old = lambda s: len([n for n in out if s in n])        # noqa: E731
    assert (old("solver_update_items_kernel"), old("emb_items_from_table_kernel"), old("abs_quantile_items_kernel")) == (18, 3, 2)
    assert old("solver_update_kernel") == 12


# ---- the refusals in front of the C call (no device) ----------------------------------------------------------------
def _loop(monkeypatch, precision="fp16", order3=False, stochastic=False, corr=None, uncond=None, B=3, T=66, Lp=5):
    """an open slot loop of the real constructors on the recording engine (tests/recording_engine.py), tensors on the host; the calls of opening it
    dropped, so that what the checks below raise from the Python side leaves ``lp.rec.calls`` empty.  ``corr`` = (name, ratio, max_val)."""
    import recording_engine
    den, rec = recording_engine.denoiser(monkeypatch, precision)
    kw = {} if corr is None else dict(correcting_x0_fn=corr[0], dynamic_thresholding_ratio=corr[1], thresholding_max_val=corr[2])
    lp = den.open_slots(B, T, Lp, order3=order3, stochastic=stochastic, unconditional_prompt=uncond, **kw)
    lp.dev, lp.rec = torch.device("cpu"), rec
    rec.calls.clear()
    return lp


def _busy(lp, spec, start=0, length=66, prompt_length=5):
    """what a slot of ``lp`` holds while a request of ``spec`` admitted at loop step ``start`` runs in it (no tensors)"""
    from ns2vc_amd.slots import SlotRequest, _Busy
    key, table, flags = lp.check_request(spec)
    return _Busy(start, SlotRequest(schedule=dict(spec), key=key, table=table, flags=flags, length=length, prompt_length=prompt_length, seed=0,
                                    guidance_scale=1.0, correction=None, known=None, known_mask=None, content=None, prompt=None))


def test_tail_refusal_names_fp32(monkeypatch):
    from ns2vc_amd.pipeline import slot_tail_needed
    assert slot_tail_needed("fp16", "unipc", 2) == 0 and slot_tail_needed("fp32", "dpmsolver++", 3, 7.0, True) == 0
    assert slot_tail_needed("fp16", "dpmsolver++", 2) == 2 and slot_tail_needed("fp16", "dpmsolver++", 3) == 4
    assert slot_tail_needed("fp16", "unipc", 3) == 1 and slot_tail_needed("fp16", "ddim", 2) == 1
    assert slot_tail_needed("fp16", "unipc", 2, 2.5) == 1            # guided_tail_extra
    assert slot_tail_needed("fp16", "unipc", 2, 1.0, True) == 1      # corrected_tail_min
    lp = _loop(monkeypatch, "fp16", order3=True, stochastic=True)
    assert lp.check_request(U2_6)[0] == S.schedule_key(U2_6)         # the 16-bit default: UniPC order 2, unguided -- tail 0
    for spec in (D3_5, U3_4, DDIM_5, dict(solver="dpmsolver++", steps=6)):
        with pytest.raises(ValueError, match=r'precision="fp32"'):
            lp.check_request(spec)
    with pytest.raises(ValueError, match=r'precision="fp32"'):
        _loop(monkeypatch, "fp16", corr=("clamp", 0.995, 1.0)).check_request(U2_6)
    with pytest.raises(ValueError, match=r'precision="fp32"'):
        _loop(monkeypatch, "fp16", uncond=torch.zeros(1, 2, 256)).check_request(U2_6, 2.5)
    lp32 = _loop(monkeypatch, "fp32", order3=True, stochastic=True)
    for spec in (U2_6, D3_5, U3_4, DDIM_5):
        key, table, flags = lp32.check_request(spec)
        assert flags == S.table_flags(_table(spec)) and table.steps == _table(spec).steps
    assert [S.table_flags(_table(s)) for s in (U2_6, D3_5, DDIM_5)] == [0, S.ITEM_HIST2, S.ITEM_NOISE]


def test_forms_fixed_at_open_are_checked_per_request(monkeypatch):
    lp = _loop(monkeypatch, "fp32")
    with pytest.raises(ValueError, match="order3=True"):
        lp.check_request(D3_5)
    with pytest.raises(ValueError, match="stochastic=True"):
        lp.check_request(DDIM_5)
    with pytest.raises(ValueError, match="unconditional_prompt"):
        lp.check_request(U2_6, 2.5)
    with pytest.raises(ValueError, match="finite"):
        lp.check_request(U2_6, float("nan"))
    with pytest.raises(ValueError, match="ddpm"):
        _loop(monkeypatch, "fp32", stochastic=True).check_request(dict(solver="ddpm", steps=10))
    with pytest.raises(ValueError, match="solver"):
        lp.check_request(dict(solver="heun", steps=4))
    with pytest.raises(ValueError, match="unipc / dpmsolver"):      # (open_slots itself refuses the pair ...
        _loop(monkeypatch, "fp32", stochastic=True, corr=("clamp", 0.995, 1.0))
    both = _loop(monkeypatch, "fp32", stochastic=True)
    both.corr = ("clamp", 0.995, 1.0)                                # ... and so does the request's own check)
    with pytest.raises(ValueError, match="unipc / dpmsolver"):
        both.check_request(DDIM_5)
    assert lp.rec.calls == [] and both.rec.calls == []


def test_admit_argument_checks_reach_no_engine_call(monkeypatch):
    lp = _loop(monkeypatch, "fp32")
    c, p, x = torch.zeros(256, 66), torch.zeros(5, 256), torch.zeros(100, 66)
    bad = [(dict(slot=3), "slots must be distinct"), (dict(schedule=None), "needs its schedule"), (dict(content=torch.zeros(256, 70)), "length 70 outside"),
           (dict(length=0), "length 0 outside"), (dict(length=67), "length 67 outside"), (dict(prompt_length=0), "prompt_length 0 outside"),
           (dict(prompt_length=6), "prompt_length 6 outside"), (dict(content=torch.zeros(255, 66)), "a request is content"),
           (dict(noise=torch.zeros(100, 40)), "length 66 outside"), (dict(prompt=torch.zeros(5, 128)), "a request is content")]
    for kw, match in bad:
        args = dict(slot=0, content=c, prompt=p, noise=x, schedule=U2_6)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            lp.admit(**args)
    lp.items[1] = _busy(lp, U2_6)
    with pytest.raises(ValueError, match=r"slot\(s\) \[1\] are busy"):
        lp.admit(1, c, p, x, schedule=U2_6)
    with pytest.raises(ValueError, match="no finished request"):
        lp.take([1])                                                 # (6 steps to go)
    with pytest.raises(ValueError, match="no finished request"):
        lp.take([0])                                                 # (idle)
    assert lp.idle() == [0, 2] and lp.finished() == [] and lp.run.__doc__
    assert lp.pool.rows_in_use() == 0                                # no refusal above left a table acquired
    assert lp.rec.calls == []                                        # ... or reached the engine


def test_continuous_converter_refuses_before_anything_runs(monkeypatch):
    from ns2vc_amd.service import ContinuousConverter, Segment

    class _Pre:
        def parameters(self):
            return iter([torch.zeros(1)])

    lp = _loop(monkeypatch, "fp16")
    conv = ContinuousConverter(_Pre(), lp.den, slots=3, max_frames=66, max_prompt=5, solver="unipc", steps=4)
    with pytest.raises(ValueError, match="segment 0 has 70 frames"):
        conv.convert([Segment(torch.zeros(256, 70), torch.zeros(100, 5))])
    assert Segment(torch.zeros(256, 4), torch.zeros(100, 4)).schedule is None and conv.own["steps"] == 4 and lp.rec.calls == []


def test_a_failed_admission_gives_its_tables_back(monkeypatch):
    """whichever engine call of an admission fails -- the rows, the lengths, the condition, the admit itself --, the pool's user counts go back
    and the slot stays idle with the per-slot vectors it had"""
    class _Failing:
        def __init__(self, bad):
            self.bad, self.calls = bad, []

        def __getattr__(self, name):
            def call(*a, **k):
                self.calls.append(name)
                if name == self.bad:
                    raise RuntimeError(name)
            return call

    c, p, x = torch.zeros(256, 66), torch.zeros(5, 256), torch.zeros(100, 66)
    for bad in ("write_sampler_rows", "set_lengths", "set_prompt_lengths", "set_condition_items", "admit"):
        lp = _loop(monkeypatch, "fp32")
        lp.den.engine = _Failing(bad)
        before = [v.copy() for v in (lp.lengths, lp.plens, lp.seeds, lp.scales)]
        with pytest.raises(RuntimeError, match=bad):
            lp.admit(0, c, p, x, schedule=U2_6, length=50, prompt_length=3, seed=9)      # (values the vectors do not hold yet)
        assert lp.den.engine.calls[-1] == bad and lp.pool.rows_in_use() == 0 and lp.idle() == [0, 1, 2], bad
        for was, now in zip(before, (lp.lengths, lp.plens, lp.seeds, lp.scales)):
            assert np.array_equal(was, now) and was.dtype == now.dtype, bad
    lp = _loop(monkeypatch, "fp32")
    lp.den.engine = _Failing(None)
    lp.admit(0, c, p, x, schedule=U2_6)
    assert lp.pool.rows_in_use() == 6 and lp.idle() == [1, 2] and lp.den.engine.calls[-1] == "admit"
