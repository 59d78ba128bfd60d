"""Characterisation cases of ``Denoiser.sample`` and its siblings (``ns2vc_amd/pipeline.py``) on the recording engine of
tests/recording_engine.py: each case is a short SEQUENCE of calls on one ``Denoiser`` -- the state an earlier call leaves on the engine is what
the setup code has to undo -- with inputs from fixed seeds at B = 2 or 3, T = 16, Lp = 8.  tools/record_sample_calls.py writes what a PARENT
checkout does on them into tests/golden/sample_calls_v1.json; tests/test_sample_calls_cpu.py compares the tree against that record.

CASES is the ordered list of case ids; run_case(monkeypatch, id) -> one record per step of the case:
    {"step": label, "head": calls, "tail": calls, "error": [type, text], "warnings": [text], "result": 16 hex digits of its SHA-256}
(a key whose value is empty is left out) with the calls of an engine as one string "method:arguments method:arguments ...", the arguments as the first 8 hex digits of the SHA-256 of their
JSON (what the recording engine noted: streams dropped, tensors as dtype, shape and SHA-256), so that the record stays small enough to read;
run_case(..., full=True) gives the steps with "calls": [[role, method, arguments]] in full, for looking at a difference."""
import hashlib
import json
import warnings

import numpy as np
import torch

import recording_engine as R

T, LP = 16, 8


def _inputs(B, seed=0, t=T):
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.randn((B, 256, t), generator=g), torch.randn((B, LP, 256), generator=g), torch.randn((B, 100, t), generator=g))


def _uncond(n, lu, seed=0):
    return torch.randn((n, lu, 256), generator=torch.Generator().manual_seed(2000 + seed))


def _known(B, seed=0, t=T):
    k = torch.randn((B, 100, t), generator=torch.Generator().manual_seed(3000 + seed))
    m = np.zeros((B, t), dtype=bool)
    m[0, :3] = True
    m[B - 1, 5:8] = True
    return k, m


DYN = dict(correcting_x0_fn="dynamic_thresholding", thresholding_max_val=0.5, dynamic_thresholding_ratio=0.9)
CLAMP = dict(correcting_x0_fn="clamp", thresholding_max_val=0.7)
U5 = dict(solver="unipc", steps=5)
D6 = dict(solver="dpmsolver++", steps=6)
D3 = dict(solver="dpmsolver++", steps=6, order=3)
DDIM4 = dict(solver="ddim", steps=4, eta=0.5)


class Ctx:
    """one case in progress: the recording, the ``Denoiser`` and the step records"""

    def __init__(self, monkeypatch):
        self.rec = R.install(monkeypatch, R.Recording())
        self.steps = []
        self.d = None

    def denoiser(self, precision="fp32", **kw):
        from ns2vc_amd.pipeline import Denoiser
        if precision != "fp32":
            kw.setdefault("precision_check", None)
        self.step("init", lambda: setattr(self, "d", Denoiser({}, precision=precision, **kw)))
        return self.d

    def step(self, label, fn):
        n = len(self.rec.calls)
        out = dict(step=label, calls=None, error=None, warnings=[], result=None)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                r = fn()
                out["result"] = R.digest(r) if torch.is_tensor(r) else None
            except (ValueError, TypeError, RuntimeError) as e:
                out["error"] = [type(e).__name__, str(e)]
        out["warnings"] = [str(w.message) for w in caught]
        out["calls"] = [list(c) for c in self.rec.calls[n:]]
        self.steps.append(out)
        return out


# ---- the cases that run once per precision ("fp32": one engine; "fp16": a tail exists) -------------------------------------------------------
def plain_unipc(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2)
    x.step("plain", lambda: d.sample(c, p, None, n, steps=5))
    x.step("again", lambda: d.sample(c, p, None, n, steps=5))
    x.step("mask, eager", lambda: d.sample(c, p, torch.arange(LP)[None, :] < torch.tensor([[8], [5]]), n, steps=5, use_graph=False))


def dpmpp_order3(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2, 1)
    x.step("order 3, default tail", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6, order=3))
    x.step("tail_fp32=1", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6, order=3, tail_fp32=1))
    x.step("options", lambda: d.sample(c, p, None, n, solver="unipc", steps=5, order=3, skip_type="logSNR", denoise_to_zero=True))


def ddim_eta(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2, 2)
    x.step("seeds=", lambda: d.sample(c, p, None, n, solver="ddim", steps=5, eta=0.5, seeds=[3, 4]))
    x.step("generator=", lambda: d.sample(c, p, solver="ddim", steps=5, eta=0.5, generator=torch.Generator().manual_seed(7)))
    x.step("eta 0", lambda: d.sample(c, p, None, n, solver="ddim", steps=5))
    x.step("ddpm refused", lambda: d.sample(c, p, None, n, solver="ddpm", steps=10))


def guidance(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2, 3)
    x.step("scalar", lambda: d.sample(c, p, None, n, steps=5, guidance_scale=2.5, unconditional_prompt=_uncond(1, LP)))
    x.step("per item", lambda: d.sample(c, p, None, n, steps=5, guidance_scale=[2.5, 1.0], unconditional_prompt=_uncond(2, LP, 1)))
    x.step("all ones", lambda: d.sample(c, p, None, n, steps=5, guidance_scale=[1.0, 1.0], unconditional_prompt=_uncond(2, LP, 1)))
    pm = torch.arange(LP)[None, :] < torch.tensor([[8], [6]])
    x.step("Lu != Lp, masks", lambda: d.sample(c, p, pm, n, steps=5, guidance_scale=np.array([3.0, 0.5], np.float32), unconditional_prompt=_uncond(1, 3, 2),
                                               unconditional_prompt_mask=torch.tensor([[True, True, False]]), lengths=[16, 9], prompt_lengths=[8, 5],
                                               unconditional_content=_inputs(2, 30)[0]))
    x.step("uncond lengths, ddim", lambda: d.sample(c, p, None, n, solver="ddim", steps=4, eta=0.5, seeds=[1, 2], guidance_scale=2.0,
                                                    unconditional_prompt=_uncond(2, LP, 3), unconditional_prompt_lengths=[4, 8]))
    x.step("plain", lambda: d.sample(c, p, None, n, steps=5))


def correction_then_plain(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2, 4)
    x.step("off: the values go nowhere", lambda: d.sample(c, p, None, n, steps=5, thresholding_max_val=2.0, dynamic_thresholding_ratio=0.5))
    x.step("dynamic thresholding", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=5, order=3, correcting_x0_fn="dynamic_thresholding",
                                                    thresholding_max_val=2.0, dynamic_thresholding_ratio=0.9))
    x.step("clamp, guided", lambda: d.sample(c, p, None, n, steps=5, correcting_x0_fn="clamp", guidance_scale=2.5, unconditional_prompt=_uncond(1, LP)))
    x.step("plain", lambda: d.sample(c, p, None, n, steps=5))


def corrections(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(3, 5)
    x.step("all equal", lambda: d.sample(c, p, None, n, steps=5, corrections=[DYN, dict(DYN), DYN]))
    x.step("all None", lambda: d.sample(c, p, None, n, steps=5, corrections=[None, None, None]))
    x.step("mixed", lambda: d.sample(c, p, None, n, steps=5, corrections=[DYN, None, CLAMP]))
    x.step("mixed again", lambda: d.sample(c, p, None, n, steps=5, corrections=[DYN, None, CLAMP]))
    x.step("call-wide after the table", lambda: d.sample(c, p, None, n, steps=5, **CLAMP))
    x.step("mixed, guided", lambda: d.sample(c, p, None, n, steps=5, corrections=[None, CLAMP, None], guidance_scale=2.0, unconditional_prompt=_uncond(1, 3)))
    x.step("plain", lambda: d.sample(c, p, None, n, steps=5))


def schedules(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(3, 6)
    x.step("all equal", lambda: d.sample(c, p, None, n, steps=9, schedules=[D6, dict(D6), D6]))
    x.step("None = the call's own", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6, schedules=[None, D6, None], **CLAMP))
    x.step("mixed", lambda: d.sample(c, p, None, n, steps=5, schedules=[None, D3, DDIM4], seeds=[5, 6, 7]))
    x.step("mixed again", lambda: d.sample(c, p, None, n, steps=5, schedules=[None, D3, DDIM4], seeds=[5, 6, 7]))
    x.step("a ddim item with corrected neighbours", lambda: d.sample(c, p, None, n, steps=5, schedules=[U5, DDIM4, D6], corrections=[CLAMP, None, DYN],
                                                                     generator=torch.Generator().manual_seed(11)))
    x.step("mixed, call-wide correction, guided", lambda: d.sample(c, p, None, n, steps=5, schedules=[U5, D3, D6], guidance_scale=[2.0, 1.0, 3.0],
                                                                   unconditional_prompt=_uncond(1, LP), **DYN))
    x.step("equal schedules under corrections=", lambda: d.sample(c, p, None, n, steps=5, schedules=[U5, U5, U5], corrections=[CLAMP, None, None]))
    x.step("plain", lambda: d.sample(c, p, None, n, steps=5))


def ragged(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2, 7)
    x.step("lengths, prompt lengths", lambda: d.sample(c, p, None, n, steps=5, lengths=[16, 9], prompt_lengths=torch.tensor([8, 5])))
    x.step("dense", lambda: d.sample(c, p, None, n, steps=5))


def known_frames(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2, 8)
    k, m = _known(2)
    x.step("known, lengths", lambda: d.sample(c, p, None, n, steps=5, known=k, known_mask=m, lengths=[16, 9]))
    x.step("plain", lambda: d.sample(c, p, None, n, steps=5))
    x.step("known", lambda: d.sample(c, p, None, n, steps=5, known=k, known_mask=torch.from_numpy(m)))
    x.step("corrected", lambda: d.sample(c, p, None, n, steps=5, correcting_x0_fn="clamp"))
    x.step("all-False mask, corrected", lambda: d.sample(c, p, None, n, steps=5, known=k, known_mask=np.zeros_like(m), correcting_x0_fn="clamp"))
    x.step("known, guided", lambda: d.sample(c, p, None, n, steps=5, known=k, known_mask=m, guidance_scale=2.0, unconditional_prompt=_uncond(1, LP)))
    x.step("per-item corrections after a hold", lambda: d.sample(c, p, None, n, steps=5, corrections=[CLAMP, None], guidance_scale=2.0,
                                                                 unconditional_prompt=_uncond(1, LP)))


def known_under_schedules(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(3, 9)
    k, m = _known(3)
    x.step("mixed schedules", lambda: d.sample(c, p, None, n, steps=5, schedules=[U5, D3, dict(solver="ddim", steps=4)], known=k, known_mask=m))
    x.step("equal schedules", lambda: d.sample(c, p, None, n, steps=5, schedules=[D6, D6, D6], known=k, known_mask=m))
    x.step("plain", lambda: d.sample(c, p, None, n, steps=5))


def sample_long(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2, 10, t=40)
    kw = dict(chunk_frames=16, overlap_frames=4, lengths=[40, 20], solver="ddim", steps=4, eta=0.5, seeds=[7, 9],
              guidance_scale=np.array([2.0, 3.0], np.float32), unconditional_prompt=_uncond(1, LP), unconditional_content=_inputs(2, 31, t=40)[0],
              prompt_lengths=torch.tensor([8, 5]))
    x.step("two items, 3 and 2 chunks", lambda: d.sample_long(c, p, None, n, **kw))
    x.step("one chunk", lambda: d.sample_long(c, p, None, n, chunk_frames=64, overlap_frames=4, steps=5))
    x.step("noise from the generator", lambda: d.sample_long(c, p, chunk_frames=32, overlap_frames=8, steps=5, generator=torch.Generator().manual_seed(5)))
    for label, bad in (("schedules", dict(schedules=[None, None])), ("corrections", dict(corrections=[None, None])), ("seeds", dict(seeds=[1])),
                       ("known", dict(known=n)), ("known_mask", dict(known_mask=np.zeros((2, 40), bool))), ("lengths", dict(lengths=[40, 41])),
                       ("noise", dict(noise=n[:, :, :-1]))):
        x.step("refused: " + label, lambda bad=bad: d.sample_long(c, p, **dict(dict(noise=n, chunk_frames=16, overlap_frames=4), **bad)))


def sample_sharded(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(3, 11)
    x.step("world 1", lambda: d.sample_sharded(c, p, None, n, lengths=[16, 9, 12], prompt_lengths=[8, 5, 8], guidance_scale=[2.0, 1.0, 3.0],
                                                unconditional_prompt=_uncond(3, 3), unconditional_prompt_lengths=[3, 2, 3], steps=5,
                                                schedules=[U5, None, D6], corrections=[CLAMP, None, None]))
    x.step("discrete: seeds drawn for the global batch", lambda: d.sample_sharded(c, p, None, n, solver="ddim", steps=4, eta=0.5,
                                                                                  generator=torch.Generator().manual_seed(3)))
    x.step("schedules of the wrong length", lambda: d.sample_sharded(c, p, None, n, steps=5, schedules=[U5]))
    x.step("corrections of the wrong length", lambda: d.sample_sharded(c, p, None, n, steps=5, corrections=[None]))


def slots(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2, 12)
    k, m = _known(2)
    x.step("held call", lambda: d.sample(c, p, None, n, steps=5, known=k, known_mask=m))
    loop = []

    def opened():
        loop.append(d.open_slots(2, T, LP, unconditional_prompt=_uncond(1, 3), item_corrections=True, require_tail_free=False))
        loop[0].dev = torch.device("cpu")
    x.step("open_slots", opened)
    x.step("admit_group", lambda: loop[0].admit_group([1, 0], [c[0], c[1, :, :9]], [p[0], p[1, :5]], [n[0], n[1, :, :9]], schedules=[U5, dict(U5, steps=3)],
                                                      seeds=[1, 2], guidance_scales=[2.0, 1.0], corrections=[CLAMP, None]))
    x.step("run", lambda: loop[0].run())
    x.step("take", lambda: loop[0].take(loop[0].finished()))
    x.step("busy slot", lambda: loop[0].admit(1, c[0], p[0], n[0], schedule=U5))
    x.step("close", lambda: loop[0].close())
    x.step("plain", lambda: d.sample(c, p, None, n, steps=5))
    x.step("loop-wide correction and item_corrections", lambda: d.open_slots(2, T, LP, item_corrections=True, correcting_x0_fn="clamp"))


def denoise(x, prec):
    d = x.denoiser(prec)
    c, p, n = _inputs(2, 13)
    t = torch.tensor([500.0, 20.0])
    x.step("plain", lambda: d.denoise(n, t, c, p))
    x.step("lengths", lambda: d.denoise(n, t, c, p, None, [16, 9], [8, 5]))
    x.step("guided", lambda: d.denoise(n, t, c, p, guidance_scale=[2.0, 1.0], unconditional_prompt=_uncond(1, 3)))


MATRIX = [plain_unipc, dpmpp_order3, ddim_eta, guidance, correction_then_plain, corrections, schedules, ragged, known_frames, known_under_schedules,
          sample_long, sample_sharded, slots, denoise]


# ---- the first call of a Denoiser: precision self-check, LayerNorm guard, options ----------------------------------------------------------
def self_check_passes(x):
    d = x.denoiser("fp16", precision_check=-1.0)
    c, p, n = _inputs(2, 14)
    x.step("first call: no tail wants the fp32 engine", lambda: d.sample(c, p, None, n, steps=5))
    x.step("second call", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6))


def self_check_passes_and_keeps_the_tail(x):
    d = x.denoiser("fp16", precision_check=-1.0)
    c, p, n = _inputs(2, 14)
    k, m = _known(2)
    x.step("first call: guided, held, a tail", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6, known=k, known_mask=m, lengths=[16, 9],
                                                                 guidance_scale=2.0, unconditional_prompt=_uncond(1, 3)))
    x.step("second call", lambda: d.sample(c, p, None, n, steps=5))


def self_check_under_schedules(x):
    d = x.denoiser("fp16", precision_check=-1.0)
    c, p, n = _inputs(3, 14)
    x.step("first call", lambda: d.sample(c, p, None, n, steps=5, schedules=[U5, D3, DDIM4], seeds=[1, 2, 3]))


def self_check_fails(x):
    d = x.denoiser("fp16", precision_check=-1.0)
    x.rec.forward_error = 0.1
    c, p, n = _inputs(2, 15)
    x.step("first call: serving_fp32", lambda: d.sample(c, p, None, n, steps=5))
    x.step("second call, corrected", lambda: d.sample(c, p, None, n, steps=5, **CLAMP))
    x.step("third call, schedules, known", lambda: d.sample(c, p, None, n, steps=5, schedules=[U5, D6], known=_known(2)[0], known_mask=_known(2)[1]))
    x.step("denoise", lambda: d.denoise(n, torch.tensor([500.0, 20.0]), c, p))


def self_check_in_denoise(x):
    d = x.denoiser("fp16", precision_check=-1.0, tail_fp32=2)
    c, p, n = _inputs(2, 15)
    x.step("denoise", lambda: d.denoise(n, torch.tensor([500.0, 20.0]), c, p))
    x.step("sample", lambda: d.sample(c, p, None, n, steps=5))


def guard_redo(x):
    d = x.denoiser("fp16")
    x.rec.ln_ratio = 100.0
    c, p, n = _inputs(2, 16)
    x.step("first call: the redo", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6, lengths=[16, 9], guidance_scale=2.0,
                                                    unconditional_prompt=_uncond(1, 3), **CLAMP))
    x.step("second call", lambda: d.sample(c, p, None, n, steps=5))


def guard_redo_schedules(x):
    d = x.denoiser("fp32")
    x.rec.ln_ratio = 100.0
    c, p, n = _inputs(3, 16)
    k, m = _known(3)
    x.step("first call: the redo", lambda: d.sample(c, p, None, n, steps=5, schedules=[U5, D3, DDIM4], seeds=[4, 5, 6], known=k, known_mask=m,
                                                    prompt_lengths=[8, 5, 8]))


def guard_redo_denoise(x):
    d = x.denoiser("fp16")
    x.rec.ln_ratio = 100.0
    c, p, n = _inputs(2, 16)
    x.step("denoise: the redo", lambda: d.denoise(n, torch.tensor([500.0, 20.0]), c, p, None, [16, 9]))


def guard_late(x):
    d = x.denoiser("fp16")
    c, p, n = _inputs(2, 17)
    x.step("first call", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6))
    x.step("second call: posts", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6))
    x.rec.ln_ratio_poll = None
    x.step("third call: not yet", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6))
    x.rec.ln_ratio_poll = 100.0
    x.step("fourth call: the late switch", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6))
    x.step("fifth call", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6))


def attn_fallbacks(x):
    d = x.denoiser("fp16")
    x.rec.attn_fallbacks = 10 ** 9
    c, p, n = _inputs(2, 18)
    x.step("first call: the exact pass from now on", lambda: d.sample(c, p, None, n, steps=5))
    x.step("second call", lambda: d.sample(c, p, None, n, steps=5))


def set_option(x):
    d = x.denoiser("fp16")
    c, p, n = _inputs(2, 19)
    x.step("masked_rows before the tail exists", lambda: d.set_option("masked_rows", True))
    x.step("a call with a tail", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6, lengths=[16, 9]))
    x.step("masked_rows off, the tail exists", lambda: d.set_option("masked_rows", False))
    x.step("gn_coop: the head alone", lambda: d.set_option("gn_coop", False))
    x.step("the call again", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6, lengths=[16, 9]))


def masked_constructor(x):
    d = x.denoiser("fp16", masked_fuse=True, masked_attn=True, masked_rows=True, masked_ffn=True, masked_geglu=True)
    c, p, n = _inputs(2, 20)
    x.step("a call with a tail", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6, lengths=[16, 9]))


def tail_settings(x):
    d = x.denoiser("fp16", tail_fp32=3)
    c, p, n = _inputs(2, 21)
    x.step("the instance's tail", lambda: d.sample(c, p, None, n, steps=5))
    x.step("tail_fp32=0", lambda: d.sample(c, p, None, n, steps=5, tail_fp32=0))
    x.step("more than the loop has", lambda: d.sample(c, p, None, n, steps=5, tail_fp32=9))


def bf16_corrected(x):
    d = x.denoiser("bf16")
    c, p, n = _inputs(2, 21)
    x.step("corrected", lambda: d.sample(c, p, None, n, steps=6, correcting_x0_fn="clamp"))
    x.step("dpmsolver++ order 3, corrected", lambda: d.sample(c, p, None, n, solver="dpmsolver++", steps=6, order=3, correcting_x0_fn="dynamic_thresholding"))


SINGLE = [self_check_passes, self_check_passes_and_keeps_the_tail, self_check_under_schedules, self_check_fails, self_check_in_denoise, guard_redo,
          guard_redo_schedules, guard_redo_denoise, guard_late, attn_fallbacks, set_option, masked_constructor, tail_settings, bf16_corrected]


# ---- every ValueError the CPU tests expect, each with no engine call --------------------------------------------------------------------------
def _refusals():
    u = torch.zeros(1, 3, 256)
    k, m = torch.ones((2, 100, T)), _known(2)[1]
    sample2 = [
        ("guidance_scale shape", dict(guidance_scale=[1.0, 2.0, 3.0])),
        ("guidance_scale ndim", dict(guidance_scale=np.ones((2, 1)))),
        ("guidance_scale nan", dict(guidance_scale=float("nan"), unconditional_prompt=u)),
        ("guidance_scale inf", dict(guidance_scale=[2.0, float("inf")], unconditional_prompt=u)),
        ("unconditional_prompt batch", dict(guidance_scale=2.0, unconditional_prompt=torch.zeros(3, 3, 256))),
        ("unconditional_prompt ndim", dict(guidance_scale=2.0, unconditional_prompt=torch.zeros(3, 256))),
        ("unconditional_prompt_mask", dict(guidance_scale=2.0, unconditional_prompt=u, unconditional_prompt_mask=torch.ones(3, 3, dtype=torch.bool))),
        ("unconditional_prompt_lengths", dict(guidance_scale=2.0, unconditional_prompt=u, unconditional_prompt_lengths=[1, 2, 3])),
        ("unconditional_content", dict(guidance_scale=2.0, unconditional_prompt=u, unconditional_content=torch.zeros(3, 256, T))),
        ("no unconditional_prompt", dict(guidance_scale=2.0, unconditional_content=torch.zeros(2, 256, T))),
        ("correction: callable", dict(correcting_x0_fn=lambda x0, t: x0)),
        ("correction: name", dict(correcting_x0_fn="dynamic")),
        ("correction: number", dict(correcting_x0_fn=1)),
        ("correction: ratio 1.5", dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=1.5)),
        ("correction: ratio nan", dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=float("nan"))),
        ("correction: max_val 0", dict(correcting_x0_fn="clamp", thresholding_max_val=0.0)),
        ("correction: max_val while off", dict(correcting_x0_fn=None, thresholding_max_val=-1.0)),
        ("correction: ddim", dict(solver="ddim", correcting_x0_fn="clamp")),
        ("correction: ddpm", dict(solver="ddpm", steps=None, correcting_x0_fn="clamp")),
        ("ddpm steps", dict(solver="ddpm", steps=50)),
        ("eta for unipc", dict(eta=0.5)),
        ("eta for ddpm", dict(solver="ddpm", steps=None, eta=1.0)),
        ("eta < 0", dict(solver="ddim", eta=-0.5)),
        ("seeds", dict(solver="ddpm", steps=None, seeds=[1, 2, 3])),
        ("solver", dict(solver="euler")),
        ("option name", dict(stride=2)),
        ("order", dict(order=4)),
        ("method", dict(method="singlestep")),
        ("schedules: count", dict(schedules=[U5])),
        ("schedules: not a list", dict(schedules=U5)),
        ("schedules: key", dict(schedules=[U5, dict(solver="unipc", steps=5, stride=2)])),
        ("schedules: solver", dict(schedules=[U5, dict(solver="euler", steps=5)])),
        ("schedules: method", dict(schedules=[U5, dict(solver="unipc", steps=5, method="singlestep")])),
        ("schedules: corrected ddim item", dict(schedules=[DDIM4, U5], correcting_x0_fn="clamp")),
        ("schedules: ddpm steps", dict(schedules=[U5, dict(solver="ddpm", steps=10)])),
        ("schedules: steps < order", dict(schedules=[U5, dict(solver="unipc", steps=1, order=2)])),
        ("known alone", dict(known=k)),
        ("known_mask alone", dict(known_mask=m)),
        ("known: frames", dict(known=k[:, :, :-1], known_mask=m)),
        ("known: items", dict(known=k[:1], known_mask=m)),
        ("known_mask: frames", dict(known=k, known_mask=m[:, :-1])),
        ("known_mask: dtype", dict(known=k, known_mask=m.astype(np.uint8))),
        ("known with correcting_x0_fn", dict(known=k, known_mask=m, correcting_x0_fn="clamp")),
        ("known with corrections", dict(known=k, known_mask=m, corrections=[None, dict(correcting_x0_fn="clamp")])),
        ("known past lengths", dict(known=k, known_mask=m, lengths=[2, 16])),
        ("known: lengths count", dict(known=k, known_mask=m, lengths=[16])),
    ]
    sample3 = [
        ("corrections and correcting_x0_fn", dict(corrections=[DYN, None, None], correcting_x0_fn="clamp")),
        ("corrections: a ddim item", dict(corrections=[DYN, None, CLAMP], schedules=[None, None, dict(solver="ddim", steps=5, eta=1.0)])),
        ("corrections: count", dict(corrections=[DYN, None])),
        ("corrections: not a list", dict(corrections=DYN)),
        ("corrections: a callable entry", dict(corrections=[DYN, lambda v: v, None])),
        ("corrections: a callable name", dict(corrections=[dict(correcting_x0_fn=lambda v: v), None, None])),
        ("corrections: a number", dict(corrections=[dict(correcting_x0_fn=1), None, None])),
        ("corrections: max_val", dict(corrections=[None, dict(CLAMP, thresholding_max_val=0.0), None])),
        ("corrections: unknown keys", dict(corrections=[None, dict(CLAMP, ratio=0.5), None])),
        ("corrections: not a dict", dict(corrections=[None, "clamp", None])),
        ("corrections: a ddim call", dict(solver="ddim", eta=1.0, corrections=[DYN, None, None])),
        ("corrections: equal entries, ddim", dict(solver="ddim", corrections=[DYN, DYN, DYN])),
        ("corrections: schedules count", dict(corrections=[DYN, None, None], schedules=[U5])),
    ]
    return sample2, sample3


def refusals_sample(x):
    d = x.denoiser("fp32")
    sample2, sample3 = _refusals()
    c, p, n = _inputs(2, 22)
    for label, kw in sample2:
        x.step(label, lambda kw=kw: d.sample(c, p, None, n, **dict(dict(solver="unipc", steps=5), **kw)))
    c, p, n = _inputs(3, 22)
    for label, kw in sample3:
        x.step(label, lambda kw=kw: d.sample(c, p, None, n, **dict(dict(steps=5), **kw)))


def refusals_denoise(x):
    d = x.denoiser("fp32")
    c, p, n = _inputs(2, 22)
    for label, kw in _refusals()[0][:10]:
        x.step(label, lambda kw=kw: d.denoise(n, torch.zeros(2), c, p, **kw))


def refusals_slots(x):
    d = x.denoiser("fp16")
    c, p, n = _inputs(1, 23)
    c, p, n = c[0], p[0], n[0]
    x.step("B < 1", lambda: d.open_slots(0, T, LP))
    x.step("unconditional_prompt shape", lambda: d.open_slots(2, T, LP, unconditional_prompt=torch.zeros(2, 3, 256)))
    x.step("loop-wide correction, stochastic", lambda: d.open_slots(2, T, LP, stochastic=True, correcting_x0_fn="clamp"))
    loops = {}

    def opened(name, **kw):
        loops[name] = d.open_slots(3, T, LP, **kw)
        loops[name].dev = torch.device("cpu")
        loops[name].close()      # (the checks below need no open loop; the next one opens on the same engine)
    x.step("open: plain", lambda: opened("plain"))
    x.step("open: corrected", lambda: opened("corr", correcting_x0_fn="clamp", require_tail_free=False))
    x.step("open: everything", lambda: opened("all", order3=True, stochastic=True, item_corrections=True, require_tail_free=False))
    x.step("open: item corrections, tail free", lambda: opened("tailfree", item_corrections=True))
    checks = [
        ("plain", "order 3", (D3,)), ("plain", "stochastic", (DDIM4,)), ("plain", "guided", (U5, 2.5)), ("plain", "scale nan", (U5, float("nan"))),
        ("plain", "solver", (dict(solver="heun", steps=4),)), ("plain", "own correction", (U5, 1.0, CLAMP)), ("plain", "tail", (D6,)),
        ("all", "ddpm steps", (dict(solver="ddpm", steps=10),)), ("corr", "loop-wide correction, ddim", (DDIM4,)),
        ("all", "own correction, ddim", (DDIM4, 1.0, CLAMP)), ("all", "callable", (U5, 1.0, lambda v: v)),
        ("tailfree", "corrected needs a tail", (U5, 1.0, CLAMP)),
    ]
    for name, label, args in checks:
        x.step(f"check_request: {label}", lambda name=name, args=args: loops[name].check_request(*args))
    lp = loops["all"]
    for label, kw in (("slot", dict(slot=3)), ("schedule", dict(schedule=None)), ("content frames", dict(content=torch.zeros(256, 20))),
                      ("length 0", dict(length=0)), ("prompt_length", dict(prompt_length=9)), ("content channels", dict(content=torch.zeros(255, T))),
                      ("corrected ddim", dict(schedule=DDIM4, correction=CLAMP))):
        x.step(f"admit: {label}", lambda kw=kw: lp.admit(**dict(dict(slot=0, content=c, prompt=p, noise=n, schedule=U5), **kw)))
    x.step("admit_group: corrections count", lambda: lp.admit_group([0, 1], [c, c], [p, p], [n, n], schedules=[U5, U5], corrections=[CLAMP]))
    x.step("admit_group: counts", lambda: lp.admit_group([0, 1], [c], [p, p], [n, n], schedules=[U5, U5]))
    x.step("take: idle", lambda: lp.take([0]))
    x.step("run: n < 0", lambda: lp.run(-1))


REFUSALS = [refusals_sample, refusals_denoise, refusals_slots]

_BY_ID = {f"{fn.__name__}[{prec}]": (fn, prec) for fn in MATRIX for prec in ("fp32", "fp16")}
_BY_ID.update({fn.__name__: (fn, None) for fn in SINGLE + REFUSALS})
CASES = list(_BY_ID)


def _calls(step, role):
    return " ".join(f"{m}:{hashlib.sha256(json.dumps(a, sort_keys=True).encode()).hexdigest()[:8]}" for r, m, a in step["calls"] if r == role)


def run_case(monkeypatch, case, full=False):
    fn, prec = _BY_ID[case]
    x = Ctx(monkeypatch)
    fn(x, prec) if prec is not None else fn(x)
    if full:
        return x.steps
    steps = [dict(step=s["step"], head=_calls(s, "head"), tail=_calls(s, "tail"), error=s["error"], warnings=s["warnings"],
                  result=None if s["result"] is None else s["result"][2][:16]) for s in x.steps]
    return [{k: v for k, v in s.items() if v not in (None, "", [])} for s in steps]      # (what is empty is left out)


# ---- the bit record on the GPU: tools/record_sample_bits.py (on the parent) and tests/test_sample_bits_gpu.py ---------------------------------
BT, BLP = 72, 6
BIT_CALLS = ["plain", "order 3 with tail", "ddim eta 0.5, seeds", "guided per item", "corrected", "mixed corrections", "mixed schedules",
             "ragged, prompt lengths", "known frames", "plain after the hold", "sample_long, two chunks"]


def run_bits(denoiser):
    """the calls of BIT_CALLS in order on one real ``Denoiser`` -> {label: dict(sha256=, head_captures=, tail_captures=)}"""
    import hashlib
    dev = torch.device("cuda", torch.cuda.current_device())

    def inputs(B, seed):
        g = torch.Generator().manual_seed(4000 + seed)
        return (torch.randn((B, 256, BT), generator=g).to(dev), torch.randn((B, BLP, 256), generator=g).to(dev), torch.randn((B, 100, BT), generator=g).to(dev))

    d = denoiser
    c2, p2, n2 = inputs(2, 0)
    c3, p3, n3 = inputs(3, 1)
    u = torch.randn((1, 4, 256), generator=torch.Generator().manual_seed(4100)).to(dev)
    k = torch.randn((2, 100, BT), generator=torch.Generator().manual_seed(4200)).to(dev)
    m = np.zeros((2, BT), dtype=bool)
    m[0, :9] = True
    m[1, 30:37] = True
    calls = {
        "plain": lambda: d.sample(c2, p2, None, n2, steps=4),
        "order 3 with tail": lambda: d.sample(c2, p2, None, n2, solver="dpmsolver++", steps=6, order=3),
        "ddim eta 0.5, seeds": lambda: d.sample(c2, p2, None, n2, solver="ddim", steps=5, eta=0.5, seeds=[3, 4]),
        "guided per item": lambda: d.sample(c2, p2, None, n2, steps=4, guidance_scale=[2.5, 1.0], unconditional_prompt=u),
        "corrected": lambda: d.sample(c2, p2, None, n2, steps=4, **DYN),
        "mixed corrections": lambda: d.sample(c3, p3, None, n3, steps=4, corrections=[DYN, None, CLAMP]),
        "mixed schedules": lambda: d.sample(c3, p3, None, n3, steps=4, schedules=[None, D3, DDIM4], seeds=[5, 6, 7]),
        "ragged, prompt lengths": lambda: d.sample(c2, p2, None, n2, steps=4, lengths=[72, 41], prompt_lengths=[6, 4]),
        "known frames": lambda: d.sample(c2, p2, None, n2, steps=4, known=k, known_mask=m),
        "plain after the hold": lambda: d.sample(c2, p2, None, n2, steps=4),
        "sample_long, two chunks": lambda: d.sample_long(c2, p2, None, n2, chunk_frames=48, overlap_frames=8, lengths=[72, 40], steps=4),
    }
    out = {}
    for label in BIT_CALLS:
        y = calls[label]()
        torch.cuda.synchronize()
        out[label] = dict(sha256=hashlib.sha256(y.detach().cpu().contiguous().numpy().tobytes()).hexdigest(), head_captures=d.engine.graph_captures(),
                          tail_captures=None if d.tail_engine is None else d.tail_engine.graph_captures())
    return out
