"""Suspend and resume of a slot's request, host side: the slot timeline in numpy with requests run in pieces against every request
run alone, the preemptive scheduler, SlotLoop.suspend / resume on the recording engine, the new exports and the register audit of the two kernels."""
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
U2_6 = dict(solver="unipc", steps=6, order=2)
U2_4 = dict(solver="unipc", steps=4, order=2)
U3_6 = dict(solver="unipc", steps=6, order=3)
D3_6 = dict(solver="dpmsolver++", steps=6, order=3, skip_type="logSNR")
DDIM_6 = dict(solver="ddim", steps=6, eta=1.0)
ITEM = (6, 10)          # one item's state: (channels, frames)


def _table(spec):
    kw = {k: v for k, v in spec.items() if k not in ("solver", "steps", "order", "eta")}
    return S.build_table(spec["solver"], spec["steps"], B64 if spec["solver"] in S.DISCRETE_SOLVERS else None, spec.get("order", 2),
                         spec.get("eta", 0.0), **kw)


def _x0(x, t):
    """per-item-independent synthetic model: item b's value depends on its own x and its own model time only"""
    t = np.asarray(t, np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    return (np.tanh(x * np.float32(0.7)) * np.float32(0.9) + np.float32(0.05) * np.sin(t * np.float32(0.01) + x)).astype(np.float32)


def _gauss(b, k, j):
    return N.gauss(77, j, *ITEM)[0]      # the request's own stream: keyed by its table row, whichever slot and piece runs it


# ---- 1. run_slots_numpy with pieces ---------------------------------------------------------------------------------------
def _known():
    rng = np.random.default_rng(8)
    mask = np.zeros((ITEM[1],), bool)
    mask[[0, 3, 9]] = True
    return rng.standard_normal(ITEM).astype(np.float32), mask


PIECE_CASES = {
    "unipc2": (U2_6, None, None),
    "unipc3": (U3_6, None, None),
    "dpmsolver3m": (D3_6, None, None),
    "ddim_eta1": (DDIM_6, None, None),
    "own_correction": (U2_6, dict(mode="dynamic_thresholding", ratio=0.9, max_val=0.5), None),
    "known_frames": (U2_6, None, _known),
}


@pytest.mark.parametrize("other_slot", [False, True], ids=["same_slot", "other_slot"])
@pytest.mark.parametrize("name", sorted(PIECE_CASES))
def test_a_request_run_in_pieces_equals_the_request_alone(name, other_slot):
    spec, corr, hold = PIECE_CASES[name]
    hold = None if hold is None else hold()
    tab = _table(spec)
    x_T = np.random.default_rng(3).standard_normal(ITEM).astype(np.float32)
    if hold is not None:
        x_T = S.known_start(x_T[None], hold[0][None], hold[1][None], tab.coef[0])[0]
    kw = {} if corr is None else dict(correct_x0=dict(corr, lengths=None))
    if hold is not None:
        kw["hold"] = (hold[0][None], hold[1][None])
    alone = S.run_table_numpy(tab, _x0, x_T[None], noise_fn=lambda j: _gauss(0, 0, j)[None], **kw)[0]
    other = _table(U2_4)
    y_T = np.random.default_rng(4).standard_normal(ITEM).astype(np.float32)
    other_alone = S.run_table_numpy(other, _x0, y_T[None])[0]
    for cut in (1, tab.steps // 2, tab.steps - 1):
        for gap in (0, 2, 4):      # resumed at once, after idle steps, after another request has run in the slot
            first = (tab, 0, x_T, corr, hold, ("r", 0, cut))
            second = (tab, cut + gap, None, corr, hold, ("r", cut, tab.steps))
            between = [(other, cut, y_T)] if gap == 4 else []
            if other_slot:
                tl = [[first] + between, [second], [(other, 1, y_T)]]
                where = (1, 0)
            else:
                tl = [[first] + between + [second], [], [(other, 1, y_T)]]
                where = (0, 1 + len(between))
            res = S.run_slots_numpy(tl, _x0, (3,) + ITEM, noise_fn=_gauss)
            assert res[0][0] is None, "a piece that is not the last has no result"
            assert np.array_equal(res[where[0]][where[1]], alone), (name, cut, gap)
            assert np.array_equal(res[2][0], other_alone)
            if between:
                assert np.array_equal(res[0][1], other_alone)


def test_three_pieces_across_three_slots_and_the_refusals():
    tab = _table(U3_6)
    x_T = np.random.default_rng(3).standard_normal(ITEM).astype(np.float32)
    alone = S.run_table_numpy(tab, _x0, x_T[None])[0]
    tl = [[(tab, 0, x_T, None, None, ("q", 0, 2))], [(tab, 5, None, None, None, ("q", 3, 6))], [(tab, 2, None, None, None, ("q", 2, 3))]]
    res = S.run_slots_numpy(tl, _x0, (3,) + ITEM)
    assert np.array_equal(res[1][0], alone) and res[0][0] is None and res[2][0] is None
    with pytest.raises(ValueError, match="no piece of request 'q' has ended at row 3"):      # the piece before it ends at the same step, not before
        S.run_slots_numpy([[(tab, 0, x_T, None, None, ("q", 0, 3))], [(tab, 2, None, None, None, ("q", 3, 6))]], _x0, (2,) + ITEM)
    with pytest.raises(ValueError, match=r"rows \[a, b\)"):
        S.run_slots_numpy([[(tab, 0, x_T, None, None, ("q", 2, 2))]], _x0, (1,) + ITEM)
    with pytest.raises(ValueError, match="busy until 2"):
        S.run_slots_numpy([[(tab, 0, x_T, None, None, ("q", 0, 2)), (tab, 1, None, None, None, ("q", 2, 6))]], _x0, (1,) + ITEM)


# ---- 2. the preemptive scheduler ------------------------------------------------------------------------------------------
def _replay(steps, n_slots, arr, pri):
    """walks the events and checks every property of the policy; returns (events, per request [(slot, loop step from, to, row from)])"""
    ev = S.plan_slots_preemptive(steps, n_slots, arr, pri)
    n = len(steps)
    holder, since, done = {}, {}, [0] * n
    pieces = [[] for _ in range(n)]
    finished = set()
    last = -1

    def leave(b, i, r):
        pieces[i].append((b, since[b], r, done[i]))
        done[i] += r - since[b]
        del holder[b], since[b]

    for r, take, suspend, admit in ev:
        assert r > last and (take or suspend or admit)
        # between the events nothing changes: nobody finished unnoticed, and a request that arrived in between found no slot and nobody to preempt
        for b, i in holder.items():
            assert done[i] + r - since[b] <= steps[i], "a finished request was held"
        for q in range(last + 1, r):
            late = [i for i in range(n) if i not in finished and i not in holder.values() and arr[i] <= q]
            if late:
                assert len(holder) == n_slots and max(pri[i] for i in late) <= min(pri[i] for i in holder.values()), (q, late)
        last = r
        for b, i in take:
            assert holder[b] == i and done[i] + r - since[b] == steps[i]
            leave(b, i, r)
            finished.add(i)
        placed_now = {b for b, _, _ in admit}
        for b, i, d in suspend:
            assert holder[b] == i and b in placed_now, "a suspended slot goes to the waiting request at once"
            assert d == done[i] + r - since[b] and 0 <= d < steps[i]
            leave(b, i, r)
        for b, i, d in admit:
            assert b not in holder, "slot double-booked"
            assert i not in finished and i not in holder.values() and arr[i] <= r and d == done[i]
            holder[b], since[b] = i, r
        waiting = [i for i in range(n) if i not in finished and i not in holder.values() and arr[i] <= r]
        if waiting:
            assert len(holder) == n_slots, "a slot idles while an arrived request waits"
            assert max(pri[i] for i in waiting) <= min(pri[i] for i in holder.values()), "a request waits beside a running one of lower priority"
        for b, i, d in suspend:      # never one placed at this same step
            assert all(not (pb == b and pi == i) for pb, pi, _ in admit)
    assert not holder and len(finished) == n
    for i in range(n):      # the pieces cover rows [0, steps) once, in order
        at = 0
        for b, r0, r1, row in pieces[i]:
            assert row == at and r1 > r0
            at += r1 - r0
        assert at == steps[i]
    return ev, pieces


def test_preemptive_scheduler_properties_over_random_workloads():
    rng = np.random.default_rng(0)
    n_suspended = 0
    for n_slots in (1, 2, 3, 8):
        for n in (1, 7, 40):
            for levels in (1, 2, 4):
                steps = [int(v) for v in rng.integers(1, 30, n)]
                arr = sorted(int(v) for v in rng.integers(0, 20, n))
                pri = [int(v) for v in rng.integers(0, levels, n)]
                ev, _ = _replay(steps, n_slots, arr, pri)
                n_suspended += sum(len(s) for _, _, s, _ in ev)
                if levels == 1:      # the degenerate case is plan_slots
                    assert [(r, t, [(b, i) for b, i, _ in a]) for r, t, _, a in ev] == S.plan_slots(steps, n_slots, arr)
                    assert all(not s and all(d == 0 for _, _, d in a) for _, _, s, a in ev)
                    assert S.plan_slots_preemptive(steps, n_slots, arr) == ev
    assert n_suspended > 10, "the workloads must exercise the suspension"
    assert S.plan_slots_preemptive([], 3) == []
    for bad in (dict(steps=[3, 0], n_slots=2), dict(steps=[3], n_slots=0), dict(steps=[3, 3], n_slots=2, arrivals=[4, 1]),
                dict(steps=[3, 3], n_slots=2, priorities=[1])):
        with pytest.raises(ValueError):
            S.plan_slots_preemptive(**bad)


def test_preemptive_scheduler_worked_example():
    """2 slots, steps [100, 100, 10], arrivals [0, 0, 3], priorities [0, 0, 1]: request 2 runs over loop steps 3 .. 13 in the higher slot, whose
    request has 3 rows done and ends at 110 instead of 100"""
    ev, pieces = _replay([100, 100, 10], 2, [0, 0, 3], [0, 0, 1])
    assert ev == [(0, [], [], [(0, 0, 0), (1, 1, 0)]), (3, [], [(1, 1, 3)], [(1, 2, 0)]), (13, [(1, 2)], [], [(1, 1, 3)]), (100, [(0, 0)], [], []),
                  (110, [(1, 1)], [], [])]
    assert pieces[2] == [(1, 3, 13, 0)] and pieces[1] == [(1, 0, 3, 0), (1, 13, 110, 3)] and pieces[0] == [(0, 0, 100, 0)]
    # the victim: lowest priority, then most rows left, then the highest slot
    ev = S.plan_slots_preemptive([20, 30, 30, 5], 3, [0, 0, 0, 4], [1, 0, 0, 2])
    assert ev[1] == (4, [], [(2, 2, 4)], [(2, 3, 0)])
    ev = S.plan_slots_preemptive([20, 30, 40, 5], 3, [0, 0, 0, 4], [0, 0, 0, 2])
    assert ev[1] == (4, [], [(2, 2, 4)], [(2, 3, 0)])
    ev = S.plan_slots_preemptive([20, 40, 30, 5], 3, [0, 0, 0, 4], [0, 0, 0, 2])
    assert ev[1] == (4, [], [(1, 1, 4)], [(1, 3, 0)])


# ---- 3. SlotLoop.suspend / resume on the recording engine -----------------------------------------------------------------
def _loop(monkeypatch, precision="fp32", **kw):
    import recording_engine
    rec = recording_engine.Recording()
    recording_engine.install(monkeypatch, rec)
    from ns2vc_amd.pipeline import Denoiser
    den = Denoiser({}, precision=precision, **dict(dict(ln_guard=None, precision_check=None, attn_fallback_limit=None), **kw.pop("den", {})))
    lp = den.open_slots(3, 66, 5, **kw)
    lp.dev, lp.rec = torch.device("cpu"), rec
    rec.calls.clear()
    return lp


def test_suspend_and_resume_routing(monkeypatch):
    from ns2vc_amd.pipeline import Suspended
    lp = _loop(monkeypatch, stochastic=True)
    c, p, x = torch.randn(256, 60), torch.randn(4, 256), torch.randn(100, 60)
    lp.admit(1, c, p, x, schedule=DDIM_6, seed=9)
    lp.admit(0, c, p, x, schedule=U2_4)
    lp.run(2)
    assert lp.pool.rows_in_use() == 10
    lp.rec.calls.clear()
    (q,) = lp.suspend([1])
    assert isinstance(q, Suspended) and q.done == 2 and q.steps == 6 and tuple(q.state.shape) == (4, 66, 128) and q.state.dtype == torch.float32
    assert (q.length, q.prompt_length, q.seed, q.guidance_scale, q.correction, q.known, q.known_mask) == (60, 4, 9, 1.0, None, None, None)
    assert q.key == S.schedule_key(DDIM_6) and q.flags == S.ITEM_NOISE and q.content is c and q.prompt is p and q.schedule == DDIM_6
    assert lp.rec.names() == ["suspend"] and lp.rec.of("suspend") == [dict(slots=[1], state_shape=[1, 4, 66, 128])]
    assert lp.idle() == [1, 2] and lp.pool.rows_in_use() == 4, "the suspended request's table is released"
    moved = q.to("cpu")
    assert moved is not q and torch.equal(moved.state, q.state) and moved.done == 2 and moved.content is c
    lp.run(3)                                                        # slot 0 finishes at 4
    lp.take([0])
    lp.rec.calls.clear()
    lp.resume([2], [q])
    names = lp.rec.names()
    # admit_group's sequence with resume in place of admit (the table stayed resident in the pool: its rows are not written again)
    assert names == ["set_lengths", "set_prompt_lengths", "set_seeds", "set_condition_items", "resume"], names
    r = lp.rec.of("resume")[0]
    assert r["slots"] == [2] and r["state"][1] == [1, 4, 66, 128]
    row0 = lp.pool.acquire(q.key, q.table.coef)[0]
    lp.pool.release(q.key)
    import recording_engine
    assert r["records"] == recording_engine.digest(np.array([[row0, 6, 2, S.ITEM_NOISE]], np.int32))
    assert lp.rec.of("set_lengths")[0]["lengths"][2] == 60 and lp.rec.of("set_prompt_lengths")[0]["prompt_lengths"][2] == 4
    assert lp.rec.of("set_seeds")[0]["seeds"][2] == 9
    assert lp.items[2].start == lp.step - 2 == 3 and lp.pool.rows_in_use() == 6
    assert lp.finished() == [] and lp.run() == [2] and lp.step == 9   # 4 rows to go
    lp.take([2])
    assert lp.idle() == [0, 1, 2] and lp.pool.rows_in_use() == 0


def test_suspend_and_resume_refusals_reach_no_engine_call(monkeypatch):
    lp = _loop(monkeypatch)
    c, p, x = torch.zeros(256, 66), torch.zeros(5, 256), torch.zeros(100, 66)
    lp.admit(1, c, p, x, schedule=U2_4)
    lp.rec.calls.clear()
    for slots, match in (([3], "distinct and in"), ([1, 1], "distinct and in"), ([], "distinct and in"), ([0], "no running request")):
        with pytest.raises(ValueError, match=match):
            lp.suspend(slots)
    lp.run(4)
    with pytest.raises(ValueError, match="no running request"):      # finished: it is taken
        lp.suspend([1])
    lp.take([1])
    lp.admit(1, c, p, x, schedule=U2_4)
    lp.run(1)
    (q,) = lp.suspend([1])
    lp.admit(0, c, p, x, schedule=U2_4)
    lp.rec.calls.clear()
    for args, match in ((([0], [q]), r"slot\(s\) \[0\] are busy"), (([1], []), "one Suspended per slot"), (([1], [object()]), "one Suspended per slot"),
                        (([1, 1], [q, q]), "distinct and in"), (([5], [q]), "distinct and in")):
        with pytest.raises(ValueError, match=match):
            lp.resume(*args)
    with pytest.raises(ValueError, match=r"done 4 outside \[0, 4\)"):
        lp.resume([1], [type(q)(**dict({k: getattr(q, k) for k in q.FIELDS}, done=4))])
    with pytest.raises(ValueError, match="same T and form"):
        lp.resume([1], [type(q)(**dict({k: getattr(q, k) for k in q.FIELDS}, state=torch.zeros(5, 66, 128)))])
    q3 = type(q)(**dict({k: getattr(q, k) for k in q.FIELDS}, schedule=U3_6))
    with pytest.raises(ValueError, match="order3=True"):
        lp.resume([1], [q3])
    with pytest.raises(ValueError, match="exactly the fields"):
        type(q)(state=None)
    assert lp.rec.calls == [] and lp.pool.rows_in_use() == 4 and lp.idle() == [1, 2]
    pending = _loop(monkeypatch, "fp16", den=dict(precision_check=1e-3))
    with pytest.raises(RuntimeError, match="self-check of this Denoiser is pending"):
        pending.resume([1], [q])
    assert pending.rec.calls == []


def test_a_failed_resume_gives_its_tables_back(monkeypatch):
    class _Failing:
        def __init__(self, bad):
            self.bad, self.calls = bad, []

        def state_shape(self):
            return (4, 66, 128)

        def __getattr__(self, name):
            def call(*a, **k):
                self.calls.append(name)
                if name == self.bad:
                    raise RuntimeError(name)
            return call

    c, p, x = torch.zeros(256, 66), torch.zeros(5, 256), torch.zeros(100, 66)
    for bad in ("write_sampler_rows", "set_lengths", "set_prompt_lengths", "set_condition_items", "resume", None):
        lp = _loop(monkeypatch)
        lp.admit(1, c, p, x, schedule=U2_4, length=50)
        lp.run(1)
        (q,) = lp.suspend([1])
        lp.pool = S.TablePool()                                        # (a pool that has to write the rows again)
        lp.den.engine = _Failing(bad)
        if bad is None:
            lp.resume([1], [q])
            assert lp.pool.rows_in_use() == 4 and lp.idle() == [0, 2] and lp.den.engine.calls[-1] == "resume"
            continue
        lengths = lp.lengths.copy()
        with pytest.raises(RuntimeError, match=bad):
            lp.resume([1], [q])
        assert lp.den.engine.calls[-1] == bad and lp.pool.rows_in_use() == 0 and lp.idle() == [0, 1, 2], bad
        assert np.array_equal(lp.lengths, lengths)


def test_preemptive_converter_arguments(monkeypatch):
    from ns2vc_amd.service import ContinuousConverter, Segment

    class _Pre:
        def parameters(self):
            return iter([torch.zeros(1)])

    lp = _loop(monkeypatch)
    assert Segment(torch.zeros(256, 4), torch.zeros(100, 4)).priority == 0
    with pytest.raises(ValueError, match="preempt=True does not go with overlap_frames"):
        ContinuousConverter(_Pre(), lp.den, slots=3, max_frames=66, max_prompt=5, preempt=True, overlap_frames=0)
    conv = ContinuousConverter(_Pre(), lp.den, slots=3, max_frames=66, max_prompt=5)
    assert conv.preempt is False
    with pytest.raises(ValueError, match="arrivals= does not go with chained chunks"):
        ContinuousConverter(_Pre(), lp.den, slots=3, max_frames=66, max_prompt=5, overlap_frames=8).convert(
            [Segment(torch.zeros(256, 70), torch.zeros(100, 5))], arrivals=[0])


# ---- 4. exports -----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ns2vc_sampler_state_shape", "ns2vc_sampler_suspend", "ns2vc_sampler_resume", "ns2vc_k_sampler_suspend", "ns2vc_k_sampler_resume")


def test_new_symbols_are_declared_bound_and_exported():
    from ns2vc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    assert "#define NS2VC_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.PROTOTYPES
    lib = _lib.load()
    assert lib.ns2vc_abi_version() == 7
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    slots, rec, done, v = np.array([0], np.int32), np.array([[0, 2, 0, 0]], np.int32), np.zeros(1, np.int32), C.c_int()
    assert lib.ns2vc_sampler_state_shape(None, C.byref(v), C.byref(v), C.byref(v)) != 0 and lib.ns2vc_last_error()
    assert lib.ns2vc_sampler_suspend(None, 1, slots.ctypes.data, None, done.ctypes.data, None) != 0
    assert lib.ns2vc_sampler_resume(None, 1, slots.ctypes.data, None, rec.ctypes.data, None) != 0
    assert lib.ns2vc_k_sampler_suspend(None, None, None, None, None, 9, 128, 1, slots.ctypes.data, 4, None, None, None) != 0
    assert lib.ns2vc_k_sampler_resume(None, 9, 128, 1, slots.ctypes.data, 4, None, None, None, None, 0, None, None, None, None, 0, None) != 0


# ---- 5. register audit ----------------------------------------------------------------------------------------------------
def test_the_two_kernels_use_no_scratch_and_the_old_counts_stand():
    """the compiler's kernel-resource-usage remarks on misc.hip: one sampler_suspend_kernel, 3 instantiations <TM> of sampler_resume_kernel -- no
    scratch, no spilled register; the slot kernels and the solver kernels in front of them keep their counts"""
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
    count = lambda s: len([n for n in out if s in n])      # noqa: E731
    assert (count("sampler_suspend_kernel"), count("sampler_resume_kernel")) == (1, 3), sorted(out)
    new = {n: v for n, v in out.items() if "sampler_suspend_kernel" in n or "sampler_resume_kernel" in n}
    bad = [(n, v) for n, v in new.items() if v.get("ScratchSize [bytes/lane]", -1) != 0 or v.get("VGPRs Spill", -1) != 0 or v.get("SGPRs Spill", -1) != 0]
    assert not bad, bad
    assert (count("sampler_admit_kernel"), count("sampler_take_kernel"), count("condition_items_kernel")) == (3, 1, 3)
    assert (count("solver_update_items_kernel"), count("emb_items_from_table_kernel"), count("abs_quantile_items_kernel")) == (18, 3, 2)
    assert count("solver_update_kernel") == 12
