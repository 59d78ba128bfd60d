"""Characterisation cases of the slot loop (``Denoiser.open_slots`` -> ``SlotLoop``) on the recording engine of tests/recording_engine.py: each
case is a SEQUENCE of labelled steps on one or two open loops at B = 3, T = 66, Lp = 5 with inputs from fixed seeds, reaching the loop only through
``Denoiser.open_slots`` and the names ``ns2vc_amd.pipeline`` exports, so that the same cases run on a parent checkout.
tools/record_slot_calls.py writes what a PARENT checkout does on them into tests/golden/slot_calls_v1.json; tests/test_slot_calls_cpu.py compares
the tree against that record.

CASES is the ordered list of case ids; run_case(monkeypatch, id) -> one record per step of the case:
    {"step": label, "calls": engine calls since the last step, "error": [type, text], "warnings": [text], "result": 16 hex digits,
     "suspended": [{field: 8 hex digits}], "state": [one entry per open loop]}
(a key whose value is empty is left out).  ``calls`` is one string "role.method:arguments ..." in the order the calls were made -- role "head" /
"tail" of the first ``Denoiser`` of the case, "head2" / "tail2" of the second --, the arguments as the first 8 hex digits of the SHA-256 of their
JSON (what the recording engine noted: streams dropped, tensors as dtype, shape and SHA-256).  ``state`` is the host state of every loop after
the step: {"idle", "finished", "step", "rows" = ``pool.rows_in_use()``, "vectors" = the digests of ``lengths``, ``plens``, ``seeds``, ``scales``
and ``corrections``}.  ``suspended`` has every field of each ``Suspended`` the step returned.  run_case(..., full=True) keeps the calls as
[[role, method, arguments]] in full, for looking at a difference."""
import hashlib
import json
import warnings

import numpy as np
import torch

import recording_engine as R

B, T, LP = 3, 66, 5
U2_4, U2_6 = dict(solver="unipc", steps=4, order=2), dict(solver="unipc", steps=6, order=2)
U3_6 = dict(solver="unipc", steps=6, order=3)
D3_6 = dict(solver="dpmsolver++", steps=6, order=3, skip_type="logSNR")
DDIM_6 = dict(solver="ddim", steps=6, eta=1.0)
DYN = dict(correcting_x0_fn="dynamic_thresholding", thresholding_max_val=0.5, dynamic_thresholding_ratio=0.9)
CLAMP = dict(correcting_x0_fn="clamp", thresholding_max_val=0.7)
VECTORS = ("lengths", "plens", "seeds", "scales", "corrections")
ADMISSION_FAILS = "admission fails in "      # (the steps whose recorded vectors a tree may differ from: tests/test_slot_calls_cpu.py)


def _h(v, n=8):
    return hashlib.sha256(json.dumps(v, sort_keys=True).encode()).hexdigest()[:n]


def _plain(v):
    """a result or a field as plain data: a sampler table as its steps and coefficients, the rest as ``recording_engine.digest`` has it"""
    if hasattr(v, "coef") and hasattr(v, "steps"):
        return ["table", int(v.steps), R.digest(np.asarray(v.coef))]
    if isinstance(v, (list, tuple)):
        return [_plain(e) for e in v]
    if isinstance(v, dict):
        return {str(k): _plain(e) for k, e in sorted(v.items())}
    return R.digest(v)


def _req(seed, L=T, lp=LP):
    """content (256, L), prompt (lp, 256), noise (100, L)"""
    g = torch.Generator().manual_seed(5000 + seed)
    return torch.randn((256, L), generator=g), torch.randn((lp, 256), generator=g), torch.randn((100, L), generator=g)


def _uncond(lu=3):
    return torch.randn((1, lu, 256), generator=torch.Generator().manual_seed(6000 + lu))


def _known(seed, L=T, frames=slice(0, 8)):
    k = torch.randn((100, L), generator=torch.Generator().manual_seed(7000 + seed))
    m = np.zeros((L,), dtype=bool)
    m[frames] = True
    return k, m


class Ctx:
    """one case in progress: the recordings (one per ``Denoiser``), the open loops and the step records"""

    def __init__(self, monkeypatch):
        self.mp, self.recs, self.loops, self.steps = monkeypatch, [], [], []

    def denoiser(self, precision="fp32", **kw):
        """a ``Denoiser`` on a recording of its own (the guard, the self-check and the attention read-out off unless ``kw`` says otherwise)"""
        from ns2vc_amd.pipeline import Denoiser
        self.recs.append(R.install(self.mp, R.Recording()))
        d = Denoiser({}, precision=precision, **dict(dict(ln_guard=None, precision_check=None, attn_fallback_limit=None), **kw))
        self.recs[-1].calls.clear()
        return d

    def open(self, den, **kw):
        lp = den.open_slots(B, T, LP, **kw)
        lp.dev = torch.device("cpu")
        self.loops.append(lp)
        return lp

    def state(self):
        return [dict(idle=lp.idle(), finished=lp.finished(), step=int(lp.step), rows=int(lp.pool.rows_in_use()),
                     vectors=" ".join(_h(_plain(list(v) if isinstance(v, list) else v)) for v in (getattr(lp, n) for n in VECTORS))) for lp in self.loops]

    def step(self, label, fn):
        from ns2vc_amd.pipeline import Suspended
        marks = [len(r.calls) for r in self.recs]
        out = dict(step=label)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                r = fn()
            except (ValueError, TypeError, RuntimeError) as e:
                r = None
                out["error"] = [type(e).__name__, str(e)]
        out["warnings"] = [str(w.message) for w in caught]
        got = [q for q in (r if isinstance(r, list) else [r]) if isinstance(q, Suspended)]
        if got:
            out["suspended"] = [{f: _h(_plain(getattr(q, f))) for f in q.FIELDS} for q in got]
        elif torch.is_tensor(r) or isinstance(r, (list, tuple)):
            out["result"] = _h(_plain(r), 16)
        marks += [0] * (len(self.recs) - len(marks))
        out["calls"] = [[role + ("" if i == 0 else str(i + 1)), m, a] for i, rec in enumerate(self.recs) for role, m, a in rec.calls[marks[i]:]]
        out["state"] = self.state()
        self.steps.append(out)
        return r

    def failing(self, eng, method, fn):
        """``fn`` while ``eng.method`` raises RuntimeError(method) (the call is noted without its arguments first)"""
        def call(*a, **k):
            eng._note(method)
            raise RuntimeError(method)
        setattr(eng, method, call)
        try:
            return fn()
        finally:
            delattr(eng, method)


# ---- the forms of a loop ------------------------------------------------------------------------------------------------------------------
def plain_loop(x):
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d))
    c, p, n = _req(0)
    x.step("admit", lambda: lp.admit(1, c, p, n, schedule=U2_6))
    (c1, p1, n1), (c2, p2, n2) = _req(1), _req(2, 60, 4)
    x.step("admit_group: lengths and prompt lengths shorter than the tensors",
           lambda: lp.admit_group([2, 0], [c1, c2], [p1, p2], [n1, n2], lengths=[50, 40], prompt_lengths=[3, 4], schedules=[U2_4, U2_6], seeds=[5, 6]))
    x.step("run: to the first finished slot", lambda: lp.run())
    x.step("run: nothing to do", lambda: lp.run())
    x.step("take", lambda: lp.take([2]))
    x.step("admit again: the table is resident", lambda: lp.admit(2, c1, p1, n1, length=30, schedule=U2_4))
    x.step("run(1)", lambda: lp.run(1))
    x.step("run", lambda: lp.run())
    x.step("take two", lambda: lp.take([1, 0]))
    x.step("close with a busy slot", lambda: lp.close())
    x.step("close twice", lambda: lp.close())
    x.step("run on an empty loop", lambda: lp.run())


def guided_loop(x):
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d, unconditional_prompt=_uncond(3)))
    (c1, p1, n1), (c2, p2, n2) = _req(3), _req(4, 60, 4)
    x.step("admit_group: two scales", lambda: lp.admit_group([2, 0], [c1, c2], [p1, p2], [n1, n2], lengths=[50, 40], prompt_lengths=[2, 4],
                                                             schedules=[U2_4, U2_6], guidance_scales=[2.5, 0.5]))
    x.step("admit: unguided beside them", lambda: lp.admit(1, c1, p1, n1, schedule=U2_4))
    x.step("run", lambda: lp.run())
    x.step("take", lambda: lp.take(lp.finished()))
    x.step("close", lambda: lp.close())


def every_form_loop(x):
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d, stochastic=True, order3=True, item_corrections=True))
    (c1, p1, n1), (c2, p2, n2), (c3, p3, n3) = _req(5), _req(6, 60, 4), _req(7, 44, 5)
    x.step("admit_group: ddim eta 1, order 3 thresholded, clamped",
           lambda: lp.admit_group([0, 1, 2], [c1, c2, c3], [p1, p2, p3], [n1, n2, n3], schedules=[DDIM_6, D3_6, U2_4], seeds=[9, 0, 0],
                                  corrections=[None, DYN, CLAMP]))
    x.step("run", lambda: lp.run())
    x.step("take: the slot's correction goes", lambda: lp.take([2]))
    x.step("admit: uncorrected into the freed slot", lambda: lp.admit(2, c3, p3, n3, schedule=U3_6))
    x.step("run", lambda: lp.run())
    x.step("take", lambda: lp.take(lp.finished()))
    x.step("close", lambda: lp.close())


def loop_wide_correction(x):
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d, order3=True, **DYN))
    c, p, n = _req(8, 50, 3)
    x.step("admit", lambda: lp.admit(0, c, p, n, schedule=D3_6))
    x.step("run", lambda: lp.run())
    x.step("take", lambda: lp.take([0]))
    x.step("close", lambda: lp.close())


def known_frames_loop(x):
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d, known_frames=True))
    (c1, p1, n1), (c2, p2, n2), (c3, p3, n3) = _req(9, 50, 4), _req(10), _req(11, 60, 5)
    k1, m1 = _known(0, 50)
    k3, m3 = _known(1, 60, slice(0, 0))
    x.step("admit_group: a mask, none, an all-False mask",
           lambda: lp.admit_group([2, 0, 1], [c1, c2, c3], [p1, p2, p3], [n1, n2, n3], schedules=[U2_4, U2_6, U2_6], knowns=[k1, None, k3],
                                  known_masks=[m1, None, m3]))
    x.step("run", lambda: lp.run())
    x.step("take", lambda: lp.take([2]))
    x.step("admit: no frames into the slot that held some", lambda: lp.admit(2, c2, p2, n2, schedule=U2_4))
    x.step("admit: busy", lambda: lp.admit(2, c2, p2, n2, schedule=U2_4))
    x.step("run", lambda: lp.run())
    x.step("take", lambda: lp.take(lp.finished()))
    x.step("admit: a mask given as a tensor, held to the request's end", lambda: lp.admit(
        0, c1, p1, n1, length=40, schedule=U2_4, known=k1, known_mask=torch.from_numpy(_known(0, 50, slice(30, 40))[1])))
    x.step("close", lambda: lp.close())


# ---- suspend and resume, once per form of the request --------------------------------------------------------------------------------------
FORMS = {
    "plain": (dict(), dict(schedule=U2_6)),
    "stochastic_order3": (dict(stochastic=True, order3=True), dict(schedule=DDIM_6, seed=9)),
    "guided": (dict(unconditional_prompt=_uncond(3)), dict(schedule=U2_6, guidance_scale=2.5)),
    "held": (dict(known_frames=True), dict(schedule=U2_6, known=_known(2, 50)[0], known_mask=_known(2, 50)[1])),
    "own_correction": (dict(item_corrections=True), dict(schedule=U2_6, correction=DYN)),
    "guided_own_correction_order3": (dict(unconditional_prompt=_uncond(2), item_corrections=True, order3=True),
                                     dict(schedule=D3_6, guidance_scale=3.0, correction=CLAMP)),
    "guided_held": (dict(unconditional_prompt=_uncond(3), known_frames=True),
                    dict(schedule=U2_6, guidance_scale=0.5, known=_known(3, 50, slice(20, 31))[0], known_mask=_known(3, 50, slice(20, 31))[1])),
}


def suspend_resume(x, form):
    opened, request = FORMS[form]
    d, d2 = x.denoiser(), x.denoiser()
    lp = x.step("open", lambda: x.open(d, **opened))
    other = x.step("open a second loop on a second Denoiser", lambda: x.open(d2, **opened))
    c, p, n = _req(12, 50, 4)
    c0, p0, n0 = _req(13)
    x.step("admit the request", lambda: lp.admit(1, c, p, n, **request))
    x.step("admit a neighbour", lambda: lp.admit(0, c0, p0, n0, schedule=U2_4))
    x.step("run(2)", lambda: lp.run(2))
    (q,) = x.step("suspend", lambda: lp.suspend([1]))
    x.step("resume: the same slot, the table resident", lambda: lp.resume([1], [q]))
    x.step("run(1)", lambda: lp.run(1))
    (q,) = x.step("suspend again", lambda: lp.suspend([1]))
    x.step("resume: another slot", lambda: lp.resume([2], [q]))
    x.step("run(1): the neighbour finishes", lambda: lp.run(1))
    (q,) = x.step("suspend a third time", lambda: lp.suspend([2]))
    spilled = x.step("to(cpu)", lambda: q.to("cpu"))
    x.step("the second loop runs", lambda: other.run(3))
    x.step("resume: the second loop, a fresh pool", lambda: other.resume([1], [spilled]))
    x.step("resume: busy there now", lambda: other.resume([1], [spilled]))
    x.step("run the second loop", lambda: other.run())
    x.step("take there", lambda: other.take([1]))
    x.step("take the neighbour", lambda: lp.take([0]))
    x.step("suspend two at once: refused, one is idle", lambda: lp.suspend([0, 1]))
    x.step("close", lambda: lp.close())
    x.step("close the second loop", lambda: other.close())


def suspend_group(x):
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d, order3=True))
    (c1, p1, n1), (c2, p2, n2) = _req(14, 50, 4), _req(15)
    x.step("admit_group", lambda: lp.admit_group([0, 2], [c1, c2], [p1, p2], [n1, n2], schedules=[U3_6, U2_6]))
    x.step("run(3)", lambda: lp.run(3))
    qs = x.step("suspend both", lambda: lp.suspend([2, 0]))
    x.step("resume both, slots swapped", lambda: lp.resume([2, 0], list(reversed(qs))))
    x.step("run", lambda: lp.run())
    x.step("take", lambda: lp.take([0, 2]))
    x.step("close", lambda: lp.close())


# ---- the precision self-check and the rebase ---------------------------------------------------------------------------------------------------
def _a_suspended(x):
    """a ``Suspended`` of the plain form from a loop on a Denoiser of its own (the loop is closed again)"""
    d = x.denoiser()
    lp = x.open(d)
    c, p, n = _req(16, 50, 4)
    lp.admit(1, c, p, n, schedule=U2_6)
    lp.run(2)
    (q,) = lp.suspend([1])
    lp.close()
    x.loops.remove(lp)
    x.recs.pop()
    return q


def self_check(x, forward_error):
    q = _a_suspended(x)
    d = x.denoiser("fp16", precision_check=1e-3)
    x.recs[-1].forward_error = forward_error
    lp = x.step("open", lambda: x.open(d, unconditional_prompt=_uncond(3), require_tail_free=False))
    x.step("resume while the check is pending", lambda: lp.resume([1], [q]))
    (c1, p1, n1), (c2, p2, n2) = _req(17, 50, 4), _req(18)
    group = dict(slots=[2, 0], contents=[c1, c2], prompts=[p1, p2], noises=[n1, n2], schedules=[U2_4, U2_6], guidance_scales=[1.0, 2.5])
    if forward_error:      # (a failed admission: the same group again, so that the vectors of the idle slots agree again afterwards)
        x.step(ADMISSION_FAILS + "the precision self-check", lambda: lp.admit_group(**group))
        x.step("the same admission again: no second check", lambda: lp.admit_group(**group))
    else:
        x.step("first admission: the self-check and the rebase", lambda: lp.admit_group(**group))
    x.step("second admission", lambda: lp.admit(1, c1, p1, n1, schedule=U2_4))
    x.step("run", lambda: lp.run())
    x.step("close", lambda: lp.close())


def rebase(x):
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d))
    c, p, n = _req(19, 50, 4)
    x.step("admit", lambda: lp.admit(1, c, p, n, schedule=U2_6))
    x.step("run(2)", lambda: lp.run(2))
    (q,) = x.step("suspend: the loop is drained", lambda: lp.suspend([1]))
    lp.step = lp.REBASE_AT - 1
    x.step("resume under REBASE_AT", lambda: lp.resume([1], [q]))
    (q,) = x.step("suspend", lambda: lp.suspend([1]))
    lp.step = lp.REBASE_AT
    x.step("resume at REBASE_AT: rebased", lambda: lp.resume([0], [q]))
    x.step("run", lambda: lp.run())
    x.step("take", lambda: lp.take([0]))
    lp.step = lp.REBASE_AT
    x.step("admit at REBASE_AT: rebased", lambda: lp.admit(1, c, p, n, schedule=U2_4))
    lp.step = lp.REBASE_AT + 5
    x.step("admit beside a busy slot: not rebased", lambda: lp.admit(0, c, p, n, schedule=U2_4))
    x.step("close", lambda: lp.close())


# ---- an engine that raises ----------------------------------------------------------------------------------------------------------------------
FAILING = ("write_sampler_rows", "set_lengths", "set_prompt_lengths", "set_condition_items", "set_known_items")


def engine_raises(x):
    d, d2 = x.denoiser(), x.denoiser()
    lp = x.step("open", lambda: x.open(d, known_frames=True))
    other = x.step("open a second loop on a second Denoiser", lambda: x.open(d2, known_frames=True))
    c0, p0, n0 = _req(20)
    x.step("admit a neighbour", lambda: lp.admit(0, c0, p0, n0, schedule=U2_4))
    c, p, n = _req(21, 60, 4)
    k, m = _known(4, 50)
    request = dict(length=50, prompt_length=3, seed=9, schedule=U2_6, known=k, known_mask=m)
    for method in FAILING + ("admit",):
        x.step(ADMISSION_FAILS + method, lambda: x.failing(d.engine, method, lambda: lp.admit(1, c, p, n, **request)))
    x.step("the admission", lambda: lp.admit(1, c, p, n, **request))
    x.step("run(1)", lambda: lp.run(1))
    (q,) = x.step("suspend", lambda: lp.suspend([1]))
    for method in FAILING + ("resume",):
        x.step("resume fails in " + method, lambda: x.failing(d2.engine, method, lambda: other.resume([2], [q])))
    x.step("the resume", lambda: other.resume([2], [q]))
    x.step("run", lambda: other.run())
    x.step("take", lambda: other.take([2]))
    x.step("close", lambda: lp.close())
    x.step("close the second loop", lambda: other.close())


# ---- every refusal the CPU tests of the slot loop expect, each with no engine call ------------------------------------------------------------
def refusals_open(x):
    d = x.denoiser("fp16")
    bad = [("B < 1", dict(B=0)), ("Lp < 1", dict(Lp=0)),
           ("unconditional_prompt: items", dict(unconditional_prompt=torch.zeros(2, 3, 256))),
           ("unconditional_prompt: longer than Lp", dict(unconditional_prompt=torch.zeros(1, 6, 256))),
           ("loop-wide correction, stochastic", dict(stochastic=True, correcting_x0_fn="clamp")),
           ("loop-wide correction and item_corrections", dict(item_corrections=True, correcting_x0_fn="clamp")),
           ("known_frames and a loop-wide correction", dict(known_frames=True, correcting_x0_fn="clamp")),
           ("known_frames and item_corrections", dict(known_frames=True, item_corrections=True)),
           ("correction: name", dict(correcting_x0_fn="dynamic")), ("correction: max_val 0", dict(correcting_x0_fn="clamp", thresholding_max_val=0.0))]
    for label, kw in bad:
        x.step(label, lambda kw=kw: d.open_slots(**dict(dict(B=B, T=T, Lp=LP), **kw)))


def refusals_check_request(x):
    d16, d32 = x.denoiser("fp16"), x.denoiser("fp32")
    loops = {}

    def opened(name, den, **kw):
        loops[name] = den.open_slots(B, T, LP, **kw)
        loops[name].dev = torch.device("cpu")
        loops[name].close()      # (the checks below need no open loop; the next one opens on the same engine)
    for name, den, kw in (("plain16", d16, dict()), ("all16", d16, dict(order3=True, stochastic=True, item_corrections=True)),
                          ("corr16", d16, dict(correcting_x0_fn="clamp")), ("guided16", d16, dict(unconditional_prompt=torch.zeros(1, 2, 256))),
                          ("plain32", d32, dict()), ("stochastic32", d32, dict(stochastic=True)),
                          ("all32", d32, dict(order3=True, stochastic=True, item_corrections=True))):
        x.step("open: " + name, lambda name=name, den=den, kw=kw: opened(name, den, **kw))
    checks = [
        ("plain16", "passes", (U2_6,)), ("all16", "order 3 needs a tail", (D3_6,)), ("all16", "unipc order 3 needs a tail", (U3_6,)),
        ("all16", "ddim needs a tail", (DDIM_6,)), ("all16", "dpmsolver++ needs a tail", (dict(solver="dpmsolver++", steps=6),)),
        ("corr16", "corrected needs a tail", (U2_6,)), ("guided16", "guided needs a tail", (U2_6, 2.5)),
        ("all16", "own correction needs a tail", (U2_4, 1.0, CLAMP)),
        ("plain32", "order 3", (D3_6,)), ("plain32", "stochastic", (DDIM_6,)), ("plain32", "guided", (U2_6, 2.5)),
        ("plain32", "scale nan", (U2_6, float("nan"))), ("stochastic32", "ddpm steps", (dict(solver="ddpm", steps=10),)),
        ("plain32", "solver", (dict(solver="heun", steps=4),)), ("plain32", "own correction", (U2_4, 1.0, CLAMP)),
        ("all32", "own correction, ddim", (DDIM_6, 1.0, CLAMP)), ("all32", "callable", (U2_4, 1.0, lambda m: m)),
        ("all32", "correction: unknown keys", (U2_4, 1.0, dict(CLAMP, ratio=0.5))), ("all32", "passes, corrected", (D3_6, 1.0, DYN)),
    ]
    for name, label, args in checks:
        x.step(f"check_request on {name}: {label}", lambda name=name, args=args: loops[name].check_request(*args))
    loops["stochastic32"].corr = ("clamp", 0.995, 1.0)      # (open_slots refuses the pair; the request's own check does too)
    x.step("check_request: loop-wide correction, ddim", lambda: loops["stochastic32"].check_request(DDIM_6))


def refusals_admit(x):
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d, order3=True, stochastic=True, item_corrections=True))
    c, p, n = _req(22)
    bad = [("slot", dict(slot=3)), ("slot < 0", dict(slot=-1)), ("schedule", dict(schedule=None)), ("content frames", dict(content=torch.zeros(256, 70))),
           ("length 0", dict(length=0)), ("length 67", dict(length=67)), ("prompt_length 0", dict(prompt_length=0)),
           ("prompt_length 6", dict(prompt_length=6)), ("content channels", dict(content=torch.zeros(255, 66))),
           ("noise frames", dict(noise=torch.zeros(100, 40))), ("prompt channels", dict(prompt=torch.zeros(5, 128))),
           ("corrected ddim", dict(schedule=DDIM_6, correction=CLAMP)), ("known frames in a loop without", dict(known=n, known_mask=np.ones(66, dtype=bool))),
           ("known alone", dict(known=n))]
    for label, kw in bad:
        x.step("admit: " + label, lambda kw=kw: lp.admit(**dict(dict(slot=0, content=c, prompt=p, noise=n, schedule=U2_6), **kw)))
    x.step("admit_group: corrections count", lambda: lp.admit_group([0, 1], [c, c], [p, p], [n, n], schedules=[U2_4, U2_4], corrections=[CLAMP]))
    x.step("admit_group: counts", lambda: lp.admit_group([0, 1], [c], [p, p], [n, n], schedules=[U2_4, U2_4]))
    x.step("admit_group: empty", lambda: lp.admit_group([], [], [], []))
    x.step("admit_group: a slot twice", lambda: lp.admit_group([1, 1], [c, c], [p, p], [n, n], schedules=[U2_4, U2_4]))
    x.step("take: idle", lambda: lp.take([0]))
    x.step("take: out of range", lambda: lp.take([3]))
    x.step("run: n < 0", lambda: lp.run(-1))
    x.step("admit", lambda: lp.admit(1, c, p, n, schedule=U2_6))
    x.step("admit: busy", lambda: lp.admit(1, c, p, n, schedule=U2_6))
    x.step("take: running", lambda: lp.take([1]))
    x.step("close", lambda: lp.close())


def refusals_known(x):
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d, known_frames=True))
    c, p, n = _req(23)
    k, m = torch.zeros(100, 66), np.zeros(66, dtype=bool)
    m[:8] = True
    late = np.zeros(66, dtype=bool)
    late[40] = True
    bad = [("known alone", dict(known=k)), ("known_mask alone", dict(known_mask=m)), ("known frames", dict(known=torch.zeros(100, 60), known_mask=m)),
           ("known channels", dict(known=torch.zeros(99, 66), known_mask=m)), ("mask dtype", dict(known=k, known_mask=m.astype(np.uint8))),
           ("mask ndim", dict(known=k, known_mask=np.zeros((1, 66), dtype=bool))), ("known dtype", dict(known=k.to(torch.int32), known_mask=m)),
           ("known: an array", dict(known=k.numpy(), known_mask=m)), ("longer than T", dict(known=torch.zeros(100, 70), known_mask=np.zeros(70, dtype=bool))),
           ("a frame past the length", dict(known=k, known_mask=late, length=40))]
    for label, kw in bad:
        x.step("admit: " + label, lambda kw=kw: lp.admit(**dict(dict(slot=0, content=c, prompt=p, noise=n, schedule=U2_6), **kw)))
    x.step("admit_group: knowns count", lambda: lp.admit_group([0, 1], [c, c], [p, p], [n, n], schedules=[U2_6, U2_6], knowns=[k], known_masks=[m]))
    x.step("admit_group: known without its mask", lambda: lp.admit_group([0, 1], [c, c], [p, p], [n, n], schedules=[U2_6, U2_6], knowns=[k, None],
                                                                         known_masks=[None, None]))
    x.step("close", lambda: lp.close())


def refusals_suspend_resume(x):
    from ns2vc_amd.pipeline import Suspended
    held = _a_suspended_held(x)
    d = x.denoiser()
    lp = x.step("open", lambda: x.open(d))
    c, p, n = _req(24)
    x.step("admit", lambda: lp.admit(1, c, p, n, schedule=U2_4))
    for label, slots in (("out of range", [3]), ("a slot twice", [1, 1]), ("empty", []), ("idle", [0])):
        x.step("suspend: " + label, lambda slots=slots: lp.suspend(slots))
    x.step("run(4)", lambda: lp.run(4))
    x.step("suspend: finished", lambda: lp.suspend([1]))
    x.step("take", lambda: lp.take([1]))
    x.step("admit", lambda: lp.admit(1, c, p, n, schedule=U2_4))
    x.step("run(1)", lambda: lp.run(1))
    (q,) = x.step("suspend", lambda: lp.suspend([1]))
    x.step("admit", lambda: lp.admit(0, c, p, n, schedule=U2_4))
    fields = {k: getattr(q, k) for k in q.FIELDS}
    x.step("resume: busy", lambda: lp.resume([0], [q]))
    x.step("resume: none", lambda: lp.resume([1], []))
    x.step("resume: not a Suspended", lambda: lp.resume([1], [object()]))
    x.step("resume: a slot twice", lambda: lp.resume([1, 1], [q, q]))
    x.step("resume: out of range", lambda: lp.resume([5], [q]))
    x.step("resume: empty", lambda: lp.resume([], []))
    x.step("resume: done", lambda: lp.resume([1], [Suspended(**dict(fields, done=4))]))
    x.step("resume: state shape", lambda: lp.resume([1], [Suspended(**dict(fields, state=torch.zeros(5, 66, 128)))]))
    x.step("resume: state dtype", lambda: lp.resume([1], [Suspended(**dict(fields, state=q.state.double()))]))
    x.step("resume: an order-3 schedule", lambda: lp.resume([1], [Suspended(**dict(fields, schedule=U3_6))]))
    x.step("resume: another table than where it ran", lambda: lp.resume([1], [Suspended(**dict(fields, schedule=U2_6))]))
    x.step("resume: length", lambda: lp.resume([1], [Suspended(**dict(fields, length=67))]))
    x.step("resume: prompt_length", lambda: lp.resume([1], [Suspended(**dict(fields, prompt_length=0))]))
    x.step("resume: known frames in a loop without", lambda: lp.resume([1], [held]))
    x.step("Suspended: a field missing", lambda: Suspended(state=None))
    x.step("Suspended: a field too many", lambda: Suspended(**dict(fields, extra=1)))
    x.step("close", lambda: lp.close())


def _a_suspended_held(x):
    d = x.denoiser()
    lp = x.open(d, known_frames=True)
    c, p, n = _req(25, 50, 4)
    k, m = _known(5, 50)
    lp.admit(1, c, p, n, schedule=U2_4, known=k, known_mask=m)
    lp.run(1)
    (q,) = lp.suspend([1])
    lp.close()
    x.loops.remove(lp)
    x.recs.pop()
    return q


_BY_ID = {fn.__name__: (fn, ()) for fn in (plain_loop, guided_loop, every_form_loop, loop_wide_correction, known_frames_loop)}
_BY_ID.update({f"suspend_resume[{form}]": (suspend_resume, (form,)) for form in FORMS})
_BY_ID.update({"suspend_group": (suspend_group, ()), "self_check[passes]": (self_check, (0.0,)), "self_check[fails]": (self_check, (0.1,)),
               "rebase": (rebase, ()), "engine_raises": (engine_raises, ())})
_BY_ID.update({fn.__name__: (fn, ()) for fn in (refusals_open, refusals_check_request, refusals_admit, refusals_known, refusals_suspend_resume)})
CASES = list(_BY_ID)


def run_case(monkeypatch, case, full=False):
    fn, args = _BY_ID[case]
    x = Ctx(monkeypatch)
    fn(x, *args)
    if full:
        return x.steps
    steps = [dict(s, calls=" ".join(f"{role}.{m}:{_h(a)}" for role, m, a in s["calls"])) for s in x.steps]
    return [{k: v for k, v in s.items() if v not in (None, "", [])} for s in steps]      # (what is empty is left out)
