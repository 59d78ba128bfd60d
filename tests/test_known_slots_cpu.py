"""Known frames in the slot loop, host side: held items in ``schedule.run_slots_numpy`` against every item run alone and against the
closed form, the properties of ``schedule.plan_chains``, the refusals of ``SlotLoop`` / ``Denoiser.open_slots`` in front of any engine call (on
the recording engine), the unchanged default call sequence, the exports, the register audit of the two new kernels, and the stitching
of ``ContinuousConverter(overlap_frames=)`` on a stub loop."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import recording_engine as R
from ns2vc_amd import noise as N
from ns2vc_amd import schedule as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B64 = S.linear_betas(1000, np.float64)
U2_4, U2_6, U2_5 = (dict(solver="unipc", steps=n, order=2) for n in (4, 6, 5))
D3_5 = dict(solver="dpmsolver++", steps=5, order=3, skip_type="logSNR")
DDIM_5 = dict(solver="ddim", steps=5, eta=1.0)
ITEM = (6, 10)          # one item's state: (channels, frames)
CLOSED_FORM_TOL = 2e-6  # the bound of tests/test_known_frames_cpu.py


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def _table(spec):
    kw = {k: v for k, v in spec.items() if k not in ("solver", "steps", "order", "eta")}
    return S.build_table(spec["solver"], spec["steps"], B64 if spec["solver"] in S.DISCRETE_SOLVERS else None, spec.get("order", 2),
                         spec.get("eta", 0.0), **kw)


def _x0(x, t):
    """per-item-independent synthetic model, frames not mixed"""
    t = np.asarray(t, np.float32).reshape((-1,) + (1,) * (x.ndim - 1))
    return (np.tanh(x * np.float32(0.7)) * np.float32(0.9) + np.float32(0.05) * np.sin(t * np.float32(0.01) + x)).astype(np.float32)


def _gauss(b, k, j):
    return N.gauss(1000 * b + k + 3, j, *ITEM)[0]


MASKS = {"head": np.arange(ITEM[1]) < 3, "island": (np.arange(ITEM[1]) >= 4) & (np.arange(ITEM[1]) < 7), "last": np.arange(ITEM[1]) == ITEM[1] - 1}
# slot 1: a held 4-step item, then (the slot reused after a held item) an unheld one admitted in mid-loop, then a held one again; an order-3 item and
# a ddim eta = 1 item run beside them; slot 2's second item is a held mid-loop admission
LAYOUT = [[(D3_5, 1, None)],
          [(U2_4, 0, "head"), (U2_6, 4, None), (U2_5, 11, "island")],
          [(DDIM_5, 0, None), (U2_6, 6, "last")]]


def _timeline():
    tl, extra = [], []
    for b, items in enumerate(LAYOUT):
        row, ex = [], []
        for k, (sp, st, mk) in enumerate(items):
            rng = np.random.default_rng(100 * b + k)
            tab, noise = _table(sp), rng.standard_normal(ITEM).astype(np.float32)
            hold = x_T = None
            if mk is not None:
                known = (0.7 * rng.standard_normal(ITEM)).astype(np.float32)
                hold = (known, MASKS[mk])
                x_T = S.known_start(noise[None], known[None], MASKS[mk][None], tab.coef[0])[0]
            row.append((tab, st, noise if x_T is None else x_T, None, hold))
            ex.append(noise)
        tl.append(row)
        extra.append(ex)
    return tl, extra


def test_held_items_in_a_slot_timeline_equal_themselves_alone_and_meet_the_closed_form():
    tl, noises = _timeline()
    res = S.run_slots_numpy(tl, _x0, (len(tl),) + ITEM, noise_fn=_gauss)
    sched = S.VPSchedule(S.linear_betas())
    held = 0
    for b, items in enumerate(tl):
        for k, (tab, start, x_T, _, hold) in enumerate(items):
            h = None if hold is None else (hold[0][None], hold[1][None])
            alone = S.run_table_numpy(tab, _x0, x_T[None], noise_fn=lambda j, b=b, k=k: _gauss(b, k, j)[None], hold=h)
            assert np.array_equal(res[b][k], alone[0]), (b, k)
            if hold is None:
                continue
            held += 1
            known, mask = hold
            t_end = float(tab.timesteps[-1])
            want = sched.alpha(t_end) * known.astype(np.float64) + sched.sigma(t_end) * noises[b][k].astype(np.float64)
            err = rel_l2(res[b][k][:, mask], want[:, mask])
            print(f"slot {b} item {k}: held frames against the closed form {err:.2e}")
            assert err < CLOSED_FORM_TOL
            plain = S.run_table_numpy(tab, _x0, x_T[None])[0]
            assert np.array_equal(res[b][k][:, ~mask], plain[:, ~mask])      # (the synthetic model mixes no frames)
    assert held == 3


def test_three_and_four_tuples_keep_their_bits_beside_five_tuples():
    tl, _ = _timeline()
    plain = [[(tab, st, x) for tab, st, x, _, _ in items] for items in tl]
    four = [[(tab, st, x, None) for tab, st, x, _, _ in items] for items in tl]
    unheld = [[(tab, st, x, None, None) for tab, st, x, _, _ in items] for items in tl]
    a, b, c = (S.run_slots_numpy(t, _x0, (len(tl),) + ITEM, noise_fn=_gauss) for t in (plain, four, unheld))
    for s in range(len(tl)):
        for k in range(len(tl[s])):
            assert np.array_equal(a[s][k], b[s][k]) and np.array_equal(a[s][k], c[s][k])


def test_a_hold_and_a_correction_are_refused_together():
    tab, x = _table(U2_4), np.zeros(ITEM, np.float32)
    hold = (np.zeros(ITEM, np.float32), MASKS["head"])
    corr = dict(mode="clamp", max_val=1.0)
    with pytest.raises(ValueError, match="rescale"):
        S.run_slots_numpy([[(tab, 0, x, corr, hold)]], _x0, (1,) + ITEM)
    with pytest.raises(ValueError):
        S.run_slots_numpy([[(tab, 0, x, None, hold)]], _x0, (1,) + ITEM, correct_x0=corr)
    with pytest.raises(ValueError, match="bool"):
        S.run_slots_numpy([[(tab, 0, x, None, (hold[0], hold[1].astype(np.uint8)))]], _x0, (1,) + ITEM)
    with pytest.raises(ValueError, match="pair"):
        S.run_slots_numpy([[(tab, 0, x, None, (hold[0], None))]], _x0, (1,) + ITEM)


# ---- plan_chains ---------------------------------------------------------------------------------------------------
def _check_chains(chains, n_slots):
    events = S.plan_chains(chains, n_slots)
    start, end, slot_of = {}, {}, {}
    holder = [None] * n_slots
    done = set()
    assert [r for r, _, _ in events] == sorted({r for r, _, _ in events})
    for r, take, admit in events:
        assert take or admit
        for b, req in take:
            assert holder[b] == req and end[req] <= r
            holder[b] = None
            done.add(req)
        for b, req in admit:
            assert holder[b] is None, "a slot is double-booked"
            assert req not in start, "a chunk is admitted twice"
            u, j = req
            if j > 0:
                assert (u, j - 1) in done and r >= end[(u, j - 1)]
            holder[b], start[req], end[req], slot_of[req] = req, r, r + chains[u][j], b
        # work conservation: a free slot at an event step means no ready request waits
        if any(h is None for h in holder):
            waiting = [(u, j) for u, c in enumerate(chains) for j in range(len(c)) if (u, j) not in start and (j == 0 or (u, j - 1) in done)]
            assert not waiting, (r, waiting)
        # the lowest free slots are taken
        if admit:
            free_after = [b for b in range(n_slots) if holder[b] is None]
            assert not free_after or max(b for b, _ in admit) < min(free_after)
    assert sorted(start) == sorted((u, j) for u, c in enumerate(chains) for j in range(len(c))), "every chunk is admitted exactly once"
    assert done == set(start)
    return events, start, end


def test_plan_chains_properties_over_random_chains():
    rng = np.random.default_rng(417)
    for _ in range(300):
        n_slots = int(rng.integers(1, 9))
        chains = [[int(s) for s in rng.integers(1, 51, size=int(rng.integers(1, 6)))] for _ in range(int(rng.integers(1, 12)))]
        _check_chains(chains, n_slots)


def test_plan_chains_of_single_chunks_is_plan_slots():
    rng = np.random.default_rng(5)
    for _ in range(100):
        n_slots = int(rng.integers(1, 9))
        steps = [int(s) for s in rng.integers(1, 51, size=int(rng.integers(1, 20)))]
        got = S.plan_chains([[s] for s in steps], n_slots)
        want = [(r, [(b, (i, 0)) for b, i in take], [(b, (i, 0)) for b, i in admit]) for r, take, admit in S.plan_slots(steps, n_slots)]
        assert got == want


def test_plan_chains_serves_successors_first_and_refuses_bad_input():
    # two slots, three utterances: at step 4 chunk (0, 1) goes before the queued first chunk of utterance 2
    ev = S.plan_chains([[4, 4], [6], [3]], 2)
    assert ev[0] == (0, [], [(0, (0, 0)), (1, (1, 0))])
    assert ev[1] == (4, [(0, (0, 0))], [(0, (0, 1))])
    assert ev[2] == (6, [(1, (1, 0))], [(1, (2, 0))])
    for bad in ([[]], [[0]], [[3, -1]]):
        with pytest.raises(ValueError):
            S.plan_chains(bad, 2)
    with pytest.raises(ValueError):
        S.plan_chains([[3]], 0)


# ---- the Python surface on the recording engine ------------------------------------------------------------------------
def _denoiser(monkeypatch, precision="fp32", rec_cls=R.Recording):
    from ns2vc_amd.pipeline import Denoiser
    rec = R.install(monkeypatch, rec_cls())
    d = Denoiser({}, precision=precision, ln_guard=None, precision_check=None, attn_fallback_limit=None)
    rec.calls.clear()
    return d, rec


def _loop(monkeypatch, known_frames=True, rec_cls=R.Recording, **kw):
    den, rec = _denoiser(monkeypatch, rec_cls=rec_cls)
    extra = dict(known_frames=True) if known_frames else {}
    lp = den.open_slots(3, 66, 5, **extra, **kw)
    lp.dev, lp.rec = torch.device("cpu"), rec
    return lp


def test_open_slots_refuses_known_frames_with_a_correction(monkeypatch):
    den, rec = _denoiser(monkeypatch)
    with pytest.raises(ValueError, match="known_frames"):
        den.open_slots(3, 66, 5, known_frames=True, correcting_x0_fn="clamp")
    with pytest.raises(ValueError, match="known_frames"):
        den.open_slots(3, 66, 5, known_frames=True, item_corrections=True)
    assert rec.calls == []


def test_admit_refuses_bad_known_frames_before_any_engine_call(monkeypatch):
    lp = _loop(monkeypatch)
    assert lp.rec.of("open_slots")[-1].get("known_frames") is True
    lp.rec.calls.clear()
    c, p, x = torch.zeros(256, 66), torch.zeros(5, 256), torch.zeros(100, 66)
    k, m = torch.zeros(100, 66), np.zeros(66, dtype=bool)
    m[:8] = True
    late = np.zeros(66, dtype=bool)
    late[40] = True
    bad = [(dict(known=k), "together"), (dict(known_mask=m), "together"),
           (dict(known=torch.zeros(100, 60), known_mask=m), "known must be a tensor"), (dict(known=torch.zeros(99, 66), known_mask=m), "known must be a tensor"),
           (dict(known=k, known_mask=m.astype(np.uint8)), "bool array"), (dict(known=k, known_mask=np.zeros((1, 66), dtype=bool)), "bool array"),
           (dict(known=k.to(torch.int32), known_mask=m), "floating-point"), (dict(known=k.numpy(), known_mask=m), "known must be a tensor"),
           (dict(known=torch.zeros(100, 70), known_mask=np.zeros(70, dtype=bool)), "known must be a tensor"),
           (dict(known=k, known_mask=late, length=40), "known frame 40 lies at or past the request's length 40")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            lp.admit(0, c, p, x, schedule=U2_6, **kw)
    with pytest.raises(ValueError, match="one entry"):
        lp.admit_group([0, 1], [c, c], [p, p], [x, x], schedules=[U2_6, U2_6], knowns=[k], known_masks=[m])
    assert lp.rec.calls == [] and lp.pool.rows_in_use() == 0 and lp.idle() == [0, 1, 2]
    plain = _loop(monkeypatch, known_frames=False)
    plain.rec.calls.clear()
    with pytest.raises(ValueError, match="known_frames=True"):
        plain.admit(0, c, p, x, schedule=U2_6, known=k, known_mask=m)
    assert plain.rec.calls == []


def test_an_admission_with_known_frames_sends_lengths_condition_known_items_admit(monkeypatch):
    lp = _loop(monkeypatch)
    lp.rec.calls.clear()
    g = torch.Generator().manual_seed(3)
    c, p, x = torch.randn((256, 50), generator=g), torch.randn((4, 256), generator=g), torch.randn((100, 50), generator=g)
    k, m = torch.randn((100, 50), generator=g), np.zeros(50, dtype=bool)
    m[:8] = True
    lp.admit_group([2, 0], [c, c], [p, p], [x, x], schedules=[U2_6, U2_4], knowns=[k, None], known_masks=[m, None])
    names = lp.rec.names()
    order = [names.index(n) for n in ("set_lengths", "set_condition_items", "set_known_items", "admit")]
    assert order == sorted(order) and names.count("set_known_items") == 1 and names[-1] == "admit"
    sent = lp.rec.of("set_known_items")[0]
    m_all = np.zeros((2, 66), dtype=bool)
    m_all[0, :8] = True
    k_all = torch.zeros((2, 100, 66))
    k_all[0, :, :50] = k
    assert sent == dict(slots=[2, 0], known=R.digest(k_all), mask=R.digest(m_all))
    # x_T: schedule.known_start by the request's own first table row on the held frames, the noise elsewhere
    x_all = np.zeros((2, 100, 66), np.float32)
    x_all[:, :, :50] = x.numpy()
    want = x_all.copy()
    want[0] = S.known_start(x_all[:1], k_all[:1].numpy(), m_all[:1], _table(U2_6).coef[0])[0]
    assert lp.rec.of("admit")[0]["x"] == R.digest(want)
    # an all-False mask is no hold
    lp.rec.calls.clear()
    lp.admit(1, c, p, x, schedule=U2_6, known=k, known_mask=np.zeros(50, dtype=bool))
    assert "set_known_items" not in lp.rec.names() and lp.rec.of("admit")[0]["x"] == R.digest(x_all[:1])


def test_the_default_call_sequence_is_unchanged(monkeypatch):
    """a loop opened without known_frames on the engine with the new methods sends what it sends to the recording engine without them: the keyword
    does not reach the engine, set_known_items is never called"""
    g = torch.Generator().manual_seed(4)
    c, p, x = torch.randn((256, 66), generator=g), torch.randn((5, 256), generator=g), torch.randn((100, 66), generator=g)
    seen = []
    for rec_cls in (R.Recording, R.Recording):
        lp = _loop(monkeypatch, known_frames=False, rec_cls=rec_cls)
        lp.admit(1, c, p, x, schedule=U2_6)
        lp.run()
        lp.take([1])
        lp.close()
        seen.append(lp.rec.calls)
    assert seen[0] == seen[1] and "known_frames" not in seen[0][[n for _, n, _ in seen[0]].index("open_slots")][2]
    assert "set_known_items" not in [n for _, n, _ in seen[0]]


def test_engine_open_slots_reaches_open_known_only_when_asked():
    from ns2vc_amd.engine import Engine
    from ns2vc_amd.spec import UNetConfig

    class _Lib:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def call(*a):
                self.calls.append(name)
                return 0
            return call

    e = object.__new__(Engine)
    e.lib, e.h, e.cfg, e.shape, e.guidance, e.x0_correction, e.x0_corrections = _Lib(), None, UNetConfig(), (3, 66, 5), None, None, None
    e.open_slots()
    e.open_slots(known_frames=True)
    assert e.lib.calls == ["ns2vc_sampler_open", "ns2vc_sampler_open_known"]
    e.x0_correction = ("clamp", 0.995, 1.0)
    with pytest.raises(ValueError, match="known_frames"):
        e.open_slots(known_frames=True)
    e.x0_correction = None
    k, m = torch.zeros((2, 100, 66)), np.zeros((2, 66), dtype=bool)
    for args in ((k, None), (None, m), (k[:1], m), (k, m[:, :60]), (k.double(), m)):
        with pytest.raises(ValueError):
            e.set_known_items([0, 2], *args)
    assert e.lib.calls[2:] == []


# ---- exports ----------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ns2vc_sampler_open_known", "ns2vc_sampler_set_known_items", "ns2vc_k_hold_slots", "ns2vc_k_known_items")


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


def test_null_handle_and_null_pointers_are_errors_not_crashes():
    from ns2vc_amd import _lib
    lib = _lib.load()
    slots, m = np.array([0], np.int32), np.zeros(8, np.uint8)
    assert lib.ns2vc_sampler_open_known(None, 0, 0, None) != 0 and lib.ns2vc_last_error()
    assert lib.ns2vc_sampler_set_known_items(None, 1, slots.ctypes.data, None, None, None) != 0
    assert lib.ns2vc_k_hold_slots(None, None, m.ctypes.data, 1, 8, 128, 100, 1, None) != 0
    assert lib.ns2vc_k_hold_slots(None, None, None, 1, 8, 128, 100, 1, None) != 0
    assert lib.ns2vc_k_known_items(None, None, 100, 8, 1, slots.ctypes.data, 4, None, None, 128, None) != 0
    assert lib.ns2vc_k_known_items(None, None, 100, 8, 1, None, 4, None, None, 128, None) != 0


# ---- register audit ---------------------------------------------------------------------------------------------
def test_new_kernels_use_no_scratch_and_the_old_counts_stand():
    """the compiler's kernel-resource-usage remarks on misc.hip: one hold_slots_kernel, one known_items_kernel -- no scratch, no spilled register;
    the counts of the existing audit (tests/test_continuous_cpu.py) stand, sampler_take_kernel is still one instantiation"""
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
    assert (count("hold_slots_kernel"), count("known_items_kernel")) == (1, 1), sorted(out)
    new = {n: v for n, v in out.items() if "hold_slots_kernel" in n or "known_items_kernel" in n}
    bad = [(n, v) for n, v in new.items() if v.get("ScratchSize [bytes/lane]", -1) != 0 or v.get("VGPRs Spill", -1) != 0 or v.get("SGPRs Spill", -1) != 0]
    assert not bad, bad
    assert (count("sampler_admit_kernel"), count("sampler_take_kernel"), count("condition_items_kernel")) == (3, 1, 3)
    assert (count("solver_update_items_kernel"), count("emb_items_from_table_kernel"), count("abs_quantile_items_kernel")) == (18, 3, 2)
    assert count("solver_update_kernel") == 12


# ---- ContinuousConverter(overlap_frames=) on a stub loop -----------------------------------------------------------------
class _Pre:
    """a front end that records its calls: content = 2 c, prompt = the clip transposed and repeated to 256 columns"""
    def __init__(self):
        self.calls = []

    def parameters(self):
        return iter([torch.zeros(1)])

    def infer(self, c, refer, lens, plens, exact_lengths=False, exact_prompt_lengths=False):
        assert exact_lengths and exact_prompt_lengths
        self.calls.append([int(v) for v in lens])
        return 2.0 * c, refer.transpose(1, 2).repeat(1, 1, 3)[..., :256].contiguous(), None


class _StubLoop:
    """SlotLoop's four calls on the host: ``take`` returns latents that name the request and the frame (request number * 1000 + frame)"""
    def __init__(self, B, T, known_frames):
        self.B, self.T, self.known_frames, self.step, self._tables = B, T, known_frames, 0, {}
        self.admitted, self.holder, self.taken, self.closed = [], [None] * B, [], False

    def check_request(self, *a):
        pass

    def run(self, n):
        self.step += n

    def admit_group(self, slots, contents, prompts, noises, lengths, plens, schedules, seeds, scales, corrections, knowns=None, known_masks=None):
        for k, b in enumerate(slots):
            assert self.holder[b] is None
            self.holder[b] = len(self.admitted)
            self.admitted.append(dict(slot=b, step=self.step, content=contents[k], prompt=prompts[k], noise=noises[k], length=lengths[k], seed=seeds[k],
                                      known=None if knowns is None else knowns[k], mask=None if known_masks is None else known_masks[k]))

    def take(self, slots):
        out = torch.zeros((len(slots), 100, self.T))
        for k, b in enumerate(slots):
            n = self.holder[b]
            L = self.admitted[n]["length"]
            out[k, :, :L] = 1000.0 * (n + 1) + torch.arange(L, dtype=torch.float32)[None, :]
            self.taken.append(n)
            self.holder[b] = None
        return out

    def close(self):
        self.closed = True


class _StubDen:
    precision = "fp32"

    def __init__(self):
        from ns2vc_amd.spec import UNetConfig
        self.cfg, self.betas64, self.loops, self.opened = UNetConfig(), B64, [], []

    def _betas_for(self, solver):
        return None

    def open_slots(self, B, T, Lp, **kw):
        self.opened.append(kw)
        self.loops.append(_StubLoop(B, T, kw.get("known_frames", False)))
        return self.loops[-1]


def test_continuous_converter_stitches_chained_chunks(monkeypatch):
    from ns2vc_amd.noise import derive_seed
    from ns2vc_amd.service import ContinuousConverter, Segment

    class _Stream:
        def synchronize(self):
            pass
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: _Stream())
    V, C_, seed = 8, 66, 77
    lens = [150, 40, 67]
    g = torch.Generator().manual_seed(1)
    segs = [Segment(torch.randn((256, L), generator=g), torch.randn((100, 3 + i), generator=g), tag=i) for i, L in enumerate(lens)]
    pre, den = _Pre(), _StubDen()
    with pytest.raises(ValueError, match="segment 0 has 150 frames"):
        ContinuousConverter(pre, den, slots=2, max_frames=C_, max_prompt=5, solver="unipc", steps=4).convert(segs)
    for bad in (-1, 66):
        with pytest.raises(ValueError, match="overlap_frames"):
            ContinuousConverter(pre, den, slots=2, max_frames=C_, max_prompt=5, overlap_frames=bad)
    assert den.loops == []
    conv = ContinuousConverter(pre, den, slots=2, max_frames=C_, max_prompt=5, solver="unipc", steps=4, seed=seed, overlap_frames=V)
    out = conv.convert(segs)
    loop = den.loops[-1]
    assert loop.closed and den.opened[-1].get("known_frames") is True
    chunks = [S.plan_chunks(L, C_, V) for L in lens]
    assert [len(c) for c in chunks] == [3, 1, 2]
    assert conv.last_plan == S.plan_chains([[4] * len(c) for c in chunks], 2)
    order = [req for _, _, admit in conv.last_plan for _, req in admit]
    assert order == [(0, 0), (1, 0), (0, 1), (2, 0), (0, 2), (2, 1)] and len(loop.admitted) == 6
    number = {req: n for n, req in enumerate(order)}
    # the front end ran once per long segment on its whole length, the short one in its own group
    assert sorted(pre.calls) == [[40], [67], [150]]
    for (i, j), a in zip(order, loop.admitted):
        start, stop = chunks[i][j]
        x_full = torch.randn((100, lens[i]), generator=torch.Generator().manual_seed(seed + i))
        assert a["length"] == stop - start and a["seed"] == int(derive_seed(seed, i))
        assert torch.equal(a["content"], 2.0 * segs[i].content[:, start:stop]) and torch.equal(a["noise"], x_full[:, start:stop])
        assert torch.equal(a["prompt"], segs[i].refer.t().repeat(1, 3)[:, :256])
        if j == 0:
            assert a["known"] is None and a["mask"] is None
            continue
        # chunk j holds its first V frames at the last V frames chunk j - 1 was taken with
        assert a["mask"].dtype == np.bool_ and a["mask"].shape == (stop - start,) and a["mask"][:V].all() and not a["mask"][V:].any()
        prev_len = chunks[i][j - 1][1] - chunks[i][j - 1][0]
        want = 1000.0 * (number[(i, j - 1)] + 1) + torch.arange(prev_len - V, prev_len, dtype=torch.float32)
        assert a["known"].shape == (100, stop - start) and torch.equal(a["known"][:, :V], want[None, :].expand(100, V)) and not a["known"][:, V:].any()
    # the output: chunk 0 whole, every later chunk from frame V on; every frame written exactly once
    for i, L in enumerate(lens):
        assert out[i].shape == (100, L)
        want = torch.zeros(L)
        for j, (start, stop) in enumerate(chunks[i]):
            keep = V if j > 0 else 0
            want[start + keep:stop] = 1000.0 * (number[(i, j)] + 1) + torch.arange(keep, stop - start, dtype=torch.float32)
        assert torch.equal(out[i], want[None, :].expand(100, L)), i
    cover = [np.zeros(L, int) for L in lens]
    for i in range(len(lens)):
        for j, (start, stop) in enumerate(chunks[i]):
            cover[i][start + (V if j > 0 else 0):stop] += 1
        assert (cover[i] == 1).all()
    # short segments alone take the plain path: plan_slots ids, no known_frames keyword
    conv.convert(segs[1:2])
    assert "known_frames" not in den.opened[-1] and conv.last_plan == S.plan_slots([4], 2)


def test_a_failed_admission_leaves_no_hold_on_its_slots(monkeypatch):
    """the admit fails after the known items went out: the slots' holds are cleared in the same call, so that a later request without known
    frames -- which sends none -- finds them clear; the admission's own error is the one raised"""
    lp = _loop(monkeypatch)
    eng = lp.den.engine

    def failing_admit(slots, x_T, records, stream=None):
        eng._note("admit", slots=list(slots))
        raise RuntimeError("admit failed")
    monkeypatch.setattr(eng, "admit", failing_admit)
    lp.rec.calls.clear()
    c, p, x = torch.zeros(256, 66), torch.zeros(5, 256), torch.zeros(100, 66)
    k, m = torch.zeros(100, 66), np.zeros(66, dtype=bool)
    m[:8] = True
    with pytest.raises(RuntimeError, match="admit failed"):
        lp.admit(2, c, p, x, schedule=U2_6, known=k, known_mask=m)
    names = lp.rec.names()
    assert names[-3:] == ["set_known_items", "admit", "set_known_items"]
    assert lp.rec.of("set_known_items")[-1] == dict(slots=[2], known=None, mask=None)
    assert lp.pool.rows_in_use() == 0 and lp.idle() == [0, 1, 2]
    lp.rec.calls.clear()
    with pytest.raises(RuntimeError, match="admit failed"):      # without known frames nothing is there to clear
        lp.admit(2, c, p, x, schedule=U2_6)
    assert "set_known_items" not in lp.rec.names()


def test_continuous_converter_refuses_an_overlap_with_a_correction_at_construction():
    from ns2vc_amd.service import ContinuousConverter
    den = _StubDen()
    for kw in (dict(correcting_x0_fn="clamp"), dict(item_corrections=True)):
        with pytest.raises(ValueError, match="overlap_frames > 0"):
            ContinuousConverter(_Pre(), den, slots=2, max_frames=66, max_prompt=5, overlap_frames=8, **kw)
        ContinuousConverter(_Pre(), den, slots=2, max_frames=66, max_prompt=5, overlap_frames=0, **kw)      # independent chunks hold nothing
        ContinuousConverter(_Pre(), den, slots=2, max_frames=66, max_prompt=5, **kw)
    assert den.loops == []
