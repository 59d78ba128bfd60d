"""Suspend and resume of a slot's request on the MI355X: the two kernels alone (ns2vc_k_sampler_suspend, ns2vc_k_sampler_resume) in
fp32, fp16 and bf16, guided and not, with and without mprev2; the contract of the loop -- a request suspended at any row and resumed into the slot
index it left ends on the bits of the uninterrupted run, its neighbours on theirs, nothing recaptures -- in every form a slot loop runs; the move
to another slot and to another engine; ContinuousConverter(preempt=True); the refusals of the ABI.  Shapes are tests/test_continuous_gpu.py's."""
import numpy as np
import pytest

from test_continuous_gpu import (CASES, DDIM6, LENS, PLENS, SHAPE, U3_6, U4, U5, U6, _bits, _case, _request, _tensor, _uncond, denoisers, pre_model,  # noqa: F401
                                 weights)
from test_solvers_gpu import FP16_TOL, FP32_TOL
from util import rel_l2

pytestmark = pytest.mark.gpu

# ---- 1. the two kernels alone --------------------------------------------------------------------------------------
T9, LD, NI = 9, 128, 4
PER = T9 * LD
PREC = {"fp32": 0, "bf16": 1, "fp16": 2}
IDLE = np.array([0, 1, 0x7fffffff, 0], np.int32)
NAMES = ("xe", "xbar", "d1", "mprev", "mprev2")


def _state(rng, items):
    v = rng.standard_normal((items, T9, LD)).astype(np.float32)
    v[:, 1, 3] = -0.0                 # a negative zero, a pad column that is not zero and a tiny value travel as they are
    v[:, 2, LD - 1] = 7.25
    v[:, 3, 0] = 1e-30
    return v


@pytest.mark.parametrize("hist2", [False, True], ids=["h1", "h2"])
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_k_sampler_suspend_and_resume(prec, guided, hist2):
    from ns2vc_amd import _lib, schedule as S
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    pr = PREC[prec]
    rng = np.random.default_rng(18)
    halves = 2 if guided else 1
    items = halves * NI
    P = 5 if hist2 else 4
    planes = NAMES[:P]
    st = {k: _state(rng, items) for k in NAMES}
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    m2 = bufs["mprev2"].ptr if hist2 else None
    rec0 = np.arange(4 * NI, dtype=np.int32).reshape(NI, 4) + 100
    rec = DevBuf.from_numpy(rec0)
    # -- suspend: slots 2 and 0, an entry outside the range between them
    slots = np.array([2, NI + 3, 0], np.int32)
    out0 = np.full((3, P, T9, LD), 0x5A5A5A5A, np.uint32)
    out = DevBuf.from_numpy(out0)
    _lib.check(lib.ns2vc_k_sampler_suspend(bufs["xe"].ptr, bufs["xbar"].ptr, bufs["d1"].ptr, bufs["mprev"].ptr, m2, T9, LD, 3, slots.ctypes.data, NI, out.ptr,
                                           rec.ptr, None), "k_sampler_suspend")
    got = out.to_numpy(out0.shape, dtype=np.uint32)
    for k, b in ((0, 2), (2, 0)):
        for p, name in enumerate(planes):
            assert np.array_equal(got[k, p], st[name][b].view(np.uint32)), (b, name)
    assert np.array_equal(got[1], out0[1]), "the entry outside the range wrote to the state buffer"
    r = rec.to_numpy((NI, 4), dtype=np.int32)
    assert np.array_equal(r[2], IDLE) and np.array_equal(r[0], IDLE) and np.array_equal(r[[1, 3]], rec0[[1, 3]])
    for name in NAMES:      # suspend reads: every tensor keeps every byte
        assert np.array_equal(_bits(bufs[name].to_numpy((items, T9, LD))), _bits(st[name])), name
    # -- the reference operand copy: the solver update's own xe' and xe_op' (one row of a UniPC table on NI items)
    table = S.build_table("unipc", 6, order=3 if hist2 else 2)
    coef, stp = DevBuf.from_numpy(np.ascontiguousarray(table.coef, np.float32)), DevBuf.from_numpy(np.array([2, 0, 0, 0], np.int32))
    ub = {k: DevBuf.from_numpy(_state(rng, NI)) for k in ("x0",) + NAMES}
    uop = DevBuf.from_numpy(np.zeros(NI * PER * 4, np.uint8))
    _lib.check(lib.ns2vc_k_solver_update(coef.ptr, stp.ptr, ub["x0"].ptr, ub["xe"].ptr, uop.ptr, pr, ub["xbar"].ptr, ub["d1"].ptr, ub["mprev"].ptr,
                                         ub["mprev2"].ptr if hist2 else None, NI * PER, LD, None), "k_solver_update")
    lib.ns2vc_dev_sync()
    xe_u = ub["xe"].to_numpy((NI, T9, LD))
    op_u = uop.to_numpy((NI * PER * 4,), dtype=np.uint8).reshape(NI, PER * 4)
    assert np.isfinite(xe_u).all()
    # -- resume: entries 0 and 2 of a state buffer into slots 1 and 3, an entry outside the range between them
    src = np.stack([np.stack([xe_u[k]] + [_state(rng, 1)[0] for _ in range(P - 1)]) for k in range(3)])
    src[0, 0, 4, 7] = -0.0
    slots = np.array([1, -1, 3], np.int32)
    recs = np.array([[5, 6, -2, int(hist2)], [9, 9, 9, 0], [40, 6, 3, int(hist2)]], np.int32)
    op0 = np.full((items, PER * 4), 0x5A, np.uint8)
    op = DevBuf.from_numpy(op0)
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    rec = DevBuf.from_numpy(rec0)
    sd = DevBuf.from_numpy(src)
    _lib.check(lib.ns2vc_k_sampler_resume(sd.ptr, T9, LD, 3, slots.ctypes.data, NI, recs.ctypes.data, rec.ptr, bufs["xe"].ptr, op.ptr, pr, bufs["xbar"].ptr,
                                          bufs["d1"].ptr, bufs["mprev"].ptr, bufs["mprev2"].ptr if hist2 else None, int(guided), None), "k_sampler_resume")
    got = {k: bufs[k].to_numpy((items, T9, LD)) for k in NAMES}
    got_op = op.to_numpy(op0.shape, dtype=np.uint8)
    zero = _bits(np.zeros((T9, LD), np.float32))
    for k, b in ((0, 1), (2, 3)):
        for p, name in enumerate(planes):
            assert np.array_equal(_bits(got[name][b]), _bits(src[k, p])), (b, name)
        if k == 2:      # (entry 0 carries a negative zero the update did not write: its operand copy is checked through the guided half below)
            assert np.array_equal(got_op[b], op_u[k]), f"slot {b}: xe_op differs from the solver update's for the same xe"
        else:
            keep = np.ones((T9, LD), bool)
            keep[4, 7] = False
            w = got_op[b].reshape(T9, -1)
            u = op_u[k].reshape(T9, -1)
            if prec == "fp32":
                assert np.array_equal(w.view(np.uint32)[keep], u.view(np.uint32)[keep])
                assert w.view(np.uint32)[4, 7] == 0x80000000
            else:
                assert np.array_equal(w.view(np.uint16)[:, :LD][keep], u.view(np.uint16)[:, :LD][keep])
                assert np.array_equal(w.view(np.uint16)[:, LD:][keep], u.view(np.uint16)[:, LD:][keep])
                assert w.view(np.uint16)[4, 7] == 0x8000 and w.view(np.uint16)[4, LD + 7] == 0
        if not hist2:
            assert np.array_equal(_bits(got["mprev2"][b]), _bits(st["mprev2"][b])), b
        if guided:      # the second half as an admission writes it: xe and its operand copy, the histories zero
            assert np.array_equal(_bits(got["xe"][b + NI]), _bits(src[k, 0])) and np.array_equal(got_op[b + NI], got_op[b]), b
            for name in planes[1:]:
                assert np.array_equal(_bits(got[name][b + NI]), zero), (b, name)
    for b in (0, 2):      # unlisted slots keep the pattern in every tensor, in both halves
        for h in range(halves):
            for name in NAMES:
                assert np.array_equal(_bits(got[name][b + h * NI]), _bits(st[name][b + h * NI])), (b, h, name)
            assert np.array_equal(got_op[b + h * NI], op0[b + h * NI]), (b, h)
    r = rec.to_numpy((NI, 4), dtype=np.int32)
    assert np.array_equal(r[1], recs[0]) and np.array_equal(r[3], recs[2]) and np.array_equal(r[[0, 2]], rec0[[0, 2]])


# ---- 2. the loop ---------------------------------------------------------------------------------------------------
DT = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=0.9, thresholding_max_val=0.5)


def _known_request():
    rq = _request("K", 1, U6)
    mask = np.zeros((LENS[1],), bool)
    mask[[0, 1, 2, 17, 40, 64]] = True
    return dict(rq, known=_tensor("sr.K.k", (100, LENS[1])), known_mask=mask)


# per form: the loop's options and the requests A (slot 0, 6 steps), B (slot 1: the one that is suspended, 6 steps), C (slot 2, 5 steps) and
# D (4 steps: what runs in slot 1 while B is out)
FORMS = {
    "order2": (dict(), lambda: dict(A=_request("A", 0, U6), B=_request("B2", 1, U6), C=_request("C", 2, U5), D=_request("B1", 1, U4))),
    "ddim_eta1": (dict(stochastic=True), lambda: dict(A=_request("A", 0, U6, seed=11), B=_request("B2", 1, DDIM6, seed=14), C=_request("C", 2, DDIM6, seed=13),
                                                      D=_request("B1", 1, U4, seed=12))),
    "guided": (dict(unconditional_prompt=_uncond), lambda: dict(A=_request("A", 0, U6, scale=2.5), B=_request("B2", 1, U6, scale=3.0),
                                                                C=_request("C", 2, U5, scale=0.5), D=_request("B1", 1, U4, scale=1.0))),
    "dynamic_thresholding": (dict(DT), lambda: dict(A=_request("A", 0, U6), B=_request("B2", 1, U6), C=_request("C", 2, U5), D=_request("B1", 1, U4))),
    "item_corrections": (dict(item_corrections=True),
                         lambda: dict(A=dict(_request("A", 0, U6), correction=dict(correcting_x0_fn="clamp", thresholding_max_val=0.7)),
                                      B=dict(_request("B2", 1, U6), correction=dict(DT)), C=_request("C", 2, U5), D=_request("B1", 1, U4))),
    "order3": (dict(order3=True), lambda: dict(A=_request("A", 0, U6), B=_request("B2", 1, U3_6), C=_request("C", 2, U5), D=_request("B1", 1, U4))),
    "known_frames": (dict(known_frames=True), lambda: dict(A=_request("A", 0, U6), B=_known_request(), C=_request("C", 2, U5), D=_request("B1", 1, U4))),
}


def _form(name):
    forms, reqs = FORMS[name]
    return {k: (v() if callable(v) else v) for k, v in forms.items()}, reqs()


def _run(den, forms, rq, graph=True, cut=None, variant="at_once", dest=1, who=("A", "B", "C"), mover=None):
    """admits ``who`` at loop step 0 and steps the loop one step at a time, taking what finishes.  ``cut``: B is suspended after ``cut`` of its
    rows and resumed into slot ``dest`` -- at once, after 2 idle steps, or after D has run in slot 1 (``variant``); ``mover(q)``: what happens to
    the Suspended in between.  Returns ({name: latent}, captures after the first step, captures at the end)."""
    loop = den.open_slots(*SHAPE, use_graph=graph, require_tail_free=False, **forms)
    out, held, caps = {}, {}, [None]
    try:
        def advance(n=None):
            k = 0
            while (held if n is None else k < n):
                loop.run(1)
                k += 1
                if caps[0] is None:
                    caps[0] = den.engine.graph_captures()
                fin = loop.finished()
                if fin:
                    lat = loop.take(fin)
                    for i, b in enumerate(fin):
                        out[held.pop(b)] = lat[i]
        for name in who:
            loop.admit(**rq[name])
            held[rq[name]["slot"]] = name
        if cut is not None:
            advance(cut)
            (q,) = loop.suspend([1])
            assert q.done == cut and held.pop(1) == "B" and 1 in loop.idle()
            if variant == "idle2":
                advance(2)
            elif variant == "other_between":
                loop.admit(**rq["D"])
                held[1] = "D"
                advance(4)
                assert "D" in out
            if mover is not None:
                q = mover(q)
            loop.resume([dest], [q])
            held[dest] = "B"
        advance()
        assert loop.idle() == [0, 1, 2]
    finally:
        loop.close()
    return {k: v.cpu().numpy() for k, v in out.items()}, caps[0], den.engine.graph_captures()


def _check_form(den, name, graph=True):
    forms, rq = _form(name)
    ref, _, _ = _run(den, forms, rq, graph)
    assert sorted(ref) == ["A", "B", "C"] and all(np.isfinite(v).all() for v in ref.values())
    steps = rq["B"]["schedule"]["steps"]
    for cut in (1, 3, steps - 1):
        for variant in ("at_once", "idle2", "other_between"):
            got, caps0, caps1 = _run(den, forms, rq, graph, cut, variant)
            tag = f"{name}, done {cut}, {variant}"
            assert np.array_equal(got["B"], ref["B"]), f"{tag}: the resumed request left the bits of the uninterrupted run"
            for k in ("A", "C"):
                assert np.array_equal(got[k], ref[k]), f"{tag}: neighbour {k} depends on the suspension beside it"
            for k in ("A", "B", "C"):      # frames past the request's length stay zero
                L = LENS[rq[k]["slot"]]
                assert not got[k][:, L:].any() and got[k][:, :L].any(), (tag, k)
            if graph:
                assert caps1 == caps0, f"{tag}: suspend / resume recaptured the step graph ({caps0} -> {caps1})"
    # done = 0: suspended straight after its admission, the state is the admission's
    got, _, _ = _run(den, forms, rq, graph, 0, "at_once")
    for k in ("A", "B", "C"):
        assert np.array_equal(got[k], ref[k]), f"{name}: done 0, {k}"


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_suspend_and_resume_in_the_same_slot(prec, graph, denoisers):
    _check_form(denoisers[prec], "order2", graph)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["ddim_eta1", "guided", "dynamic_thresholding", "item_corrections", "order3", "known_frames"])
def test_suspend_and_resume_forms(name, prec, denoisers):
    _check_form(denoisers[prec], name)


# ---- 3. another slot, another engine -----------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,tol", [("fp32", FP32_TOL), ("fp16", FP16_TOL)])
def test_resume_into_another_slot(prec, tol, denoisers, diag):
    """slot 1's request continues in slot 2 of the same loop: the project's sampled-latent gate against the uninterrupted run (slot independence
    has never been pinned bit for bit; the outcome is reported)"""
    den = denoisers[prec]
    forms, rq = _form("order2")
    ref, _, _ = _run(den, forms, rq, who=("A", "B"))
    got, _, _ = _run(den, forms, rq, cut=3, dest=2, who=("A", "B"))
    err = rel_l2(got["B"], ref["B"])
    diag(f"suspend in slot 1, resume in slot 2 ({prec}): rel_l2 {err:.3e} (bar {tol:g}), bits equal: {bool(np.array_equal(got['B'], ref['B']))}")
    assert np.array_equal(got["A"], ref["A"])
    assert err < tol and not got["B"][:, LENS[1]:].any()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_resume_on_another_engine_by_way_of_host_memory(prec, weights, denoisers):
    """the state spilled to host memory and resumed into the same slot index of a second Denoiser of the same weights and precision"""
    import torch
    from ns2vc_amd.pipeline import Denoiser
    den = denoisers[prec]
    forms, rq = _form("order2")
    ref, _, _ = _run(den, forms, rq)
    loop = den.open_slots(*SHAPE, require_tail_free=False, **forms)
    try:
        for name in ("A", "B", "C"):
            loop.admit(**rq[name])
        loop.run(3)
        (q,) = loop.suspend([1])
        q = q.to("cpu")
        torch.cuda.synchronize()
        assert q.state.device.type == "cpu" and q.done == 3
    finally:
        loop.close()
    other = Denoiser(weights, precision=prec, precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None)
    loop = other.open_slots(*SHAPE, require_tail_free=False, **forms)
    try:
        loop.resume([1], [q.to(torch.device("cuda", 0))])
        assert loop.run() == [1] and loop.step == 3
        got = loop.take([1])[0].cpu().numpy()
    finally:
        loop.close()
    assert np.array_equal(got, ref["B"])


# ---- 4. the service --------------------------------------------------------------------------------------------------------
def _front():
    """a front end of elementwise operations only, with PreModel.infer's signature.  The real one is not reproducible bit for bit from one call to
    the next (two conversions of the same segments through it differ by 1.5e-6, profiles/r18_continuous.txt), which would hide what this test is
    about: the bits the LOOP gives a segment."""
    import torch

    class Front(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))

        def infer(self, c, refer, lens, plens, exact_lengths=False, exact_prompt_lengths=False):
            r = refer.transpose(1, 2)      # (n, Lp, 100) -> 256 channels
            return c * 0.5, torch.cat([r, r, r[..., :56]], dim=-1) * 0.5, None
    return Front().to(torch.device("cuda", 0))


def test_preemptive_converter_against_the_plain_one(denoisers, diag):
    """three 6-step segments fill the 3 slots at loop step 0; a 4-step segment of priority 1 arrives at loop step 1.  preempt=True suspends the
    segment in the highest slot for it and resumes that one, in the same slot, when it has finished at loop step 5.  Both runs admit the same
    groups, so the front end's tensors are the same; a segment that stays in its slot index keeps its bits, the priority segment, which lands in
    slot 2 instead of slot 0, is held to the sampled-latent gate."""
    import torch
    from ns2vc_amd.service import ContinuousConverter, Segment
    from ns2vc_amd.weights import hash_normal
    shapes = [(66, 5), (65, 3), (33, 5), (48, 4)]
    segs = [Segment(torch.from_numpy(hash_normal(f"pc.c{i}", (256, T))), torch.from_numpy(hash_normal(f"pc.r{i}", (100, L))), tag=i,
                    schedule=dict(solver="unipc", steps=(6, 6, 6, 4)[i], order=2), priority=int(i == 3)) for i, (T, L) in enumerate(shapes)]
    arrivals = [0, 0, 0, 1]
    den = denoisers["fp32"]
    pre_model = _front()
    plain = ContinuousConverter(pre_model, den, slots=3, max_frames=66, max_prompt=5)
    a = [t.cpu().numpy() for t in plain.convert(segs, arrivals=arrivals)]
    assert plain.last_plan == [(0, [], [(0, 0), (1, 1), (2, 2)]), (6, [(0, 0), (1, 1), (2, 2)], [(0, 3)]), (10, [(0, 3)], [])]
    pre = ContinuousConverter(pre_model, den, slots=3, max_frames=66, max_prompt=5, preempt=True)
    b = [t.cpu().numpy() for t in pre.convert(segs, arrivals=arrivals)]
    assert pre.last_plan == [(0, [], [], [(0, 0, 0), (1, 1, 0), (2, 2, 0)]), (1, [], [(2, 2, 1)], [(2, 3, 0)]), (5, [(2, 3)], [], [(2, 2, 1)]),
                             (6, [(0, 0), (1, 1)], [], []), (10, [(2, 2)], [], [])]
    assert sum(len(s) for _, _, s, _ in pre.last_plan) >= 1
    for i in (0, 1, 2):      # the same slot index in both runs
        assert np.array_equal(a[i], b[i]), f"segment {i} keeps its slot and lost its bits"
    err = rel_l2(b[3], a[3])
    diag(f"preemptive converter: the priority segment in slot 2 instead of slot 0 (fp32): rel_l2 {err:.3e}, bits equal: {bool(np.array_equal(a[3], b[3]))}")
    assert err < FP32_TOL and all(np.isfinite(v).all() for v in b)
    with pytest.raises(ValueError, match="overlap_frames"):
        ContinuousConverter(pre_model, den, slots=3, max_frames=66, max_prompt=5, preempt=True, overlap_frames=8)


# ---- 5. refusals of the ABI ----------------------------------------------------------------------------------------------
def test_refusals(weights):
    import torch
    from ns2vc_amd import schedule as S
    from ns2vc_amd._lib import Ns2vcError, check
    from ns2vc_amd.engine import Engine
    e = Engine(precision="fp32")
    try:
        e.load_state_dict(weights)
        e.prepare(*SHAPE)
        e.set_lengths([66, 66, 66])
        e.set_prompt_lengths([5, 5, 5])
        x = _tensor("rf.x", (1, 100, 66))
        st = torch.zeros((1, 4, 66, 128), device="cuda")
        with pytest.raises(Ns2vcError, match="no slot loop"):
            e.suspend([0], st)
        with pytest.raises(Ns2vcError, match="no slot loop"):
            e.resume([0], st, [[0, 4, 1, 0]])
        with pytest.raises(Ns2vcError, match="no slot loop"):
            e.state_shape()
        e.open_slots()
        assert e.state_shape() == (4, 66, 128)
        tab, tab3, tabn = S.build_table("unipc", 4), S.build_table("unipc", 6, order=3), S.build_table("ddim", 4, S.linear_betas(1000, np.float64), eta=1.0)
        with pytest.raises(Ns2vcError, match="never written"):
            e.resume([0], st, [[0, 4, 1, 0]])
        e.write_sampler_rows(0, tab.coef)
        e.write_sampler_rows(8, tab3.coef)
        e.write_sampler_rows(16, tabn.coef)
        with pytest.raises(Ns2vcError, match="null argument"):
            e.suspend([0], None)
        with pytest.raises(Ns2vcError, match="null argument"):
            e.resume([0], None, [[0, 4, 1, 0]])
        one, d = np.zeros(1, np.int32), np.zeros(1, np.int32)
        with pytest.raises(Ns2vcError, match="needs 1 .. 3 entries"):
            check(e.lib.ns2vc_sampler_suspend(e.h, 0, one.ctypes.data, st.data_ptr(), d.ctypes.data, None), "sampler_suspend")
        with pytest.raises(Ns2vcError, match="needs 1 .. 3 entries"):
            check(e.lib.ns2vc_sampler_resume(e.h, 0, one.ctypes.data, st.data_ptr(), np.array([[0, 4, 1, 0]], np.int32).ctypes.data, None), "sampler_resume")
        with pytest.raises(Ns2vcError, match="is idle: nothing to suspend"):
            e.suspend([0], st)
        e.admit([0], x, [[0, 4, 0, 0]])
        e.admit([2], x, [[0, 4, 3, 0]])
        with pytest.raises(Ns2vcError, match="has not started"):
            e.suspend([2], st)
        with pytest.raises(Ns2vcError, match=r"outside \[0, 3\)"):
            e.suspend([3], st)
        with pytest.raises(Ns2vcError, match="listed twice"):
            e.suspend([0, 0], torch.zeros((2, 4, 66, 128), device="cuda"))
        with pytest.raises(Ns2vcError, match="slot 0 is busy"):
            e.resume([0], st, [[0, 4, 1, 0]])
        with pytest.raises(Ns2vcError, match=r"outside \[0, 3\)"):
            e.resume([-1], st, [[0, 4, 1, 0]])
        with pytest.raises(Ns2vcError, match="listed twice"):
            e.resume([1, 1], torch.zeros((2, 4, 66, 128), device="cuda"), [[0, 4, 1, 0], [0, 4, 1, 0]])
        for done in (-1, 4):
            with pytest.raises(Ns2vcError, match=r"done -?\d+ outside \[0, 4\)"):
                e.resume([1], st, [[0, 4, done, 0]])
        with pytest.raises(Ns2vcError, match="flags"):
            e.resume([1], st, [[0, 4, 1, 1]])
        with pytest.raises(Ns2vcError, match="opened without it"):
            e.resume([1], st, [[8, 6, 2, 1]])
        with pytest.raises(Ns2vcError, match="opened without noise"):
            e.resume([1], st, [[16, 4, 2, 2]])
        e.sample_steps(4)
        with pytest.raises(Ns2vcError, match="has finished"):
            e.suspend([0], st)
        assert e.suspend([2], st) == [1]
        out = torch.empty_like(x)
        e.take([0], out)
        e.rebase_slots()
        e.resume([1], st, [[0, 4, 3, 0]])              # after a rebase the record's start lies below 0
        e.sample_steps(1)
        e.take([1], out)
        torch.cuda.synchronize()
        # a guided loop whose halves' lengths differ, and a known frame at or past the length
        e.prepare(6, 66, 5)
        e.set_lengths([66, 66, 66, 66, 66, 66])
        e.set_prompt_lengths([5] * 6)
        e.set_guidance([1.0, 2.0, 1.0])
        e.open_slots()
        e.write_sampler_rows(0, tab.coef)
        e.set_lengths([66, 60, 66, 66, 66, 66])
        with pytest.raises(Ns2vcError, match=r"lengths\[1\] and lengths\[4\] differ"):
            e.resume([1], st, [[0, 4, 1, 0]])
        e.set_guidance(None)
        e.prepare(*SHAPE)
        e.set_lengths([66, 66, 66])
        e.set_prompt_lengths([5, 5, 5])
        e.open_slots(known_frames=True)
        e.write_sampler_rows(0, tab.coef)
        mask = np.zeros((1, 66), bool)
        mask[0, 50] = True
        e.set_known_items([1], x, mask)
        e.set_lengths([66, 40, 66])
        with pytest.raises(Ns2vcError, match="known frame 50 of slot 1 lies at or past its length 40"):
            e.resume([1], st, [[0, 4, 1, 0]])
    finally:
        e.close()
