"""Continuous batching on the MI355X: the admit / take kernels alone (ns2vc_k_sampler_admit, ns2vc_k_sampler_take), the per-item condition
scatter, and the slot loop's contract -- an item admitted in mid-loop ends on the bits it gets alone in its slot from loop step 0, its neighbours
on the bits they have without the admission, nothing recaptures -- in fp32 and fp16, captured and eager, beside a DDIM eta 1 item, on a guided
engine, under dynamic thresholding and with an order-3 item; accuracy against oracle/sampler_ref.py; ContinuousConverter; the refusals."""
import json
import os

import numpy as np
import pytest

from test_engine_gpu import FP32_SAMPLED_TOL
from test_solvers_gpu import FP16_TOL
from util import procedural_params, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (3, 66, 5)
LENS, PLENS = (66, 65, 33), (5, 1, 3)      # per slot: 33 -> 17 -> 9 -> 5 sits on the planner's level thresholds; prompt lengths are in [1, Lp]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


# ---- 1. the two state kernels alone ----------------------------------------------------------------------------
T9, LD, NI, NC = 9, 128, 4, 100
PER = T9 * LD
SLOTS9 = np.array([2, 0], np.int32)
LENS9 = np.array([9, 5, 7, 9], np.int32)


def _begin_state(x_T, L, prec):
    """what ns2vc_sampler_begin leaves for one item: channels-last fp32 rows, pad channels and rows t >= L zero, and the operand copy
    (fp32: the rows; fp16: [hi | lo] with hi = the fp16 rounding, lo = the fp16 rounding of the rest), as bytes"""
    v = np.zeros((T9, LD), np.float32)
    v[:L, :NC] = x_T.T[:L]
    if prec == "fp32":
        return v, _bits(v)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float16)
    return v, _bits(np.concatenate([hi, lo], axis=1))


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_k_sampler_admit_and_take(prec, guided):
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    pr = {"fp32": 0, "fp16": 2}[prec]
    rng = np.random.default_rng(9)
    halves = 2 if guided else 1
    n = halves * NI * PER
    names = ("xe", "xbar", "d1", "mprev", "mprev2")
    st = {k: rng.standard_normal(n).astype(np.float32) for k in names}
    op0 = np.full(n * 4, 0x5A, np.uint8)           # fp32: n floats; fp16: the hi + lo pair, 2 n halves
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    op = DevBuf.from_numpy(op0)
    x_T = rng.standard_normal((2, NC, T9)).astype(np.float32)
    x_T[0, 3, 1] = -0.0
    xd, lens = DevBuf.from_numpy(x_T), DevBuf.from_numpy(LENS9)
    _lib.check(lib.ns2vc_k_sampler_admit(xd.ptr, NC, T9, 2, SLOTS9.ctypes.data, NI, bufs["xe"].ptr, op.ptr, pr, bufs["xbar"].ptr, bufs["d1"].ptr,
                                         bufs["mprev"].ptr, bufs["mprev2"].ptr, LD, lens.ptr, int(guided), None), "k_sampler_admit")
    got = {k: bufs[k].to_numpy((halves * NI, T9, LD)) for k in names}
    got_op = op.to_numpy(op0.shape, dtype=np.uint8).reshape(halves * NI, -1)
    op0 = op0.reshape(halves * NI, -1)
    pat = {k: v.reshape(halves * NI, T9, LD) for k, v in st.items()}
    zero = _bits(np.zeros((T9, LD), np.float32))
    for k, b in enumerate(SLOTS9):
        v, vop = _begin_state(x_T[k], int(LENS9[b]), prec)
        assert np.array_equal(_bits(got["xe"][b]), _bits(v)) and np.array_equal(_bits(got["xbar"][b]), _bits(v)), b
        assert np.array_equal(got_op[b], vop.reshape(-1)), b
        for name in ("d1", "mprev", "mprev2"):
            assert np.array_equal(_bits(got[name][b]), zero), (b, name)
        if guided:      # the conditional half evaluates at the same point; the histories live in the first half, the second is zero
            assert np.array_equal(_bits(got["xe"][b + NI]), _bits(v)) and np.array_equal(got_op[b + NI], vop.reshape(-1)), b
            for name in ("xbar", "d1", "mprev", "mprev2"):
                assert np.array_equal(_bits(got[name][b + NI]), zero), (b, name)
    for b in (1, 3):      # unlisted slots: every state tensor and the operand buffer keep the pattern, in both halves
        for h in range(halves):
            for name in names:
                assert np.array_equal(_bits(got[name][b + h * NI]), _bits(pat[name][b + h * NI])), (b, h, name)
            assert np.array_equal(got_op[b + h * NI], op0[b + h * NI]), (b, h)
    # take: the rows peek's kernel gives for those items
    out, full = DevBuf(2 * NC * T9 * 4), DevBuf(NI * NC * T9 * 4)
    _lib.check(lib.ns2vc_k_sampler_take(bufs["xe"].ptr, LD, NC, T9, 2, SLOTS9.ctypes.data, NI, out.ptr, None), "k_sampler_take")
    _lib.check(lib.ns2vc_k_btc_to_nct(bufs["xe"].ptr, LD, NC, T9, NI, full.ptr, None), "k_btc_to_nct")
    lib.ns2vc_dev_sync()
    o, f = out.to_numpy((2, NC, T9)), full.to_numpy((NI, NC, T9))
    assert np.array_equal(_bits(o), _bits(f[SLOTS9]))
    assert np.array_equal(o[0, :, :7], x_T[0, :, :7]) and not o[0, :, 7:].any()
    # a bad list is refused before anything is launched
    for bad in (np.array([0, 0], np.int32), np.array([4, 1], np.int32), np.array([-1, 1], np.int32)):
        assert lib.ns2vc_k_sampler_take(bufs["xe"].ptr, LD, NC, T9, 2, bad.ctypes.data, NI, out.ptr, None) != 0


# ---- 2. the loop ---------------------------------------------------------------------------------------------------
U4, U6, U5 = (dict(solver="unipc", steps=n, order=2) for n in (4, 6, 5))
DDIM6 = dict(solver="ddim", steps=6, eta=1.0)
U3_6 = dict(solver="unipc", steps=6, order=3)


def _tensor(tag, shape):
    import torch
    from ns2vc_amd.weights import hash_normal
    return torch.from_numpy(hash_normal(tag, shape)).to(torch.device("cuda", 0))


def _request(name, slot, schedule, seed=0, scale=1.0):
    L, lp = LENS[slot], PLENS[slot]
    return dict(slot=slot, content=_tensor(f"cb.{name}.c", (256, L)), prompt=_tensor(f"cb.{name}.p", (lp, 256)), noise=_tensor(f"cb.{name}.x", (100, L)),
                schedule=schedule, seed=seed, guidance_scale=scale)


def _drive(den, reqs, graph=True, **forms):
    """reqs: {name: (request, start)} -> ({name: latent (100, T)}, captures after the first steps, captures at the end).  Finished slots are
    taken as soon as the loop reaches their end, requests admitted at their start."""
    loop = den.open_slots(*SHAPE, use_graph=graph, require_tail_free=False, **forms)
    out, held, caps = {}, {}, None
    pending = sorted(reqs.items(), key=lambda kv: kv[1][1])
    while pending or held:
        fin = loop.finished()
        if fin:
            lat = loop.take(fin)
            for k, b in enumerate(fin):
                out[held.pop(b)] = lat[k]
        for name, (rq, start) in [p for p in pending if p[1][1] == loop.step]:
            loop.admit(**rq)
            held[rq["slot"]] = name
        pending = [p for p in pending if p[1][1] > loop.step]
        nexts = [it["start"] + it["steps"] for it in loop.items if it is not None] + [p[1][1] for p in pending]
        if not nexts:
            break
        loop.run(min(nexts) - loop.step)
        if caps is None:
            caps = den.engine.graph_captures()
    assert loop.idle() == [0, 1, 2]
    return {k: v.cpu().numpy() for k, v in out.items()}, caps, den.engine.graph_captures()


@pytest.fixture(scope="module")
def denoisers(weights):
    from ns2vc_amd.pipeline import Denoiser
    return {prec: Denoiser(weights, precision=prec, precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None) for prec in ("fp32", "fp16")}


def _uncond():
    return _tensor("cb.u", (1, 2, 256))


# slot 1 runs a 4-step item, is taken, and gets a 6-step item at loop step 4; slots 0 and 2 run 6- and 5-step items across the admission
CASES = {
    "order2": (dict(), lambda: dict(A=_request("A", 0, U6), B1=_request("B1", 1, U4), C=_request("C", 2, U5), B2=_request("B2", 1, U6))),
    "ddim_eta1": (dict(stochastic=True),
                  lambda: dict(A=_request("A", 0, U6, seed=11), B1=_request("B1", 1, U4, seed=12), C=_request("C", 2, U5, seed=13),
                               B2=_request("B2", 1, DDIM6, seed=14))),
    "guided": (dict(unconditional_prompt=_uncond),
               lambda: dict(A=_request("A", 0, U6, scale=2.5), B1=_request("B1", 1, U4, scale=1.0), C=_request("C", 2, U5, scale=0.5),
                            B2=_request("B2", 1, U6, scale=3.0))),
    "dynamic_thresholding": (dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=0.9, thresholding_max_val=0.5),
                             lambda: dict(A=_request("A", 0, U6), B1=_request("B1", 1, U4), C=_request("C", 2, U5), B2=_request("B2", 1, U6))),
    "order3": (dict(order3=True), lambda: dict(A=_request("A", 0, U6), B1=_request("B1", 1, U4), C=_request("C", 2, U5), B2=_request("B2", 1, U3_6))),
}


def _case(name):
    forms, reqs = CASES[name]
    return {k: (v() if callable(v) else v) for k, v in forms.items()}, reqs()


def _check_loop(den, name, graph):
    forms, rq = _case(name)
    full, caps0, caps1 = _drive(den, dict(A=(rq["A"], 0), B1=(rq["B1"], 0), C=(rq["C"], 0), B2=(rq["B2"], 4)), graph, **forms)
    # the same loop without the admission: the neighbours' bits
    without, _, _ = _drive(den, dict(A=(rq["A"], 0), B1=(rq["B1"], 0), C=(rq["C"], 0)), graph, **forms)
    # the admitted item alone, in the same slot, from loop step 0, the other slots idle
    alone, _, _ = _drive(den, dict(B2=(rq["B2"], 0)), graph, **forms)
    assert sorted(full) == ["A", "B1", "B2", "C"] and all(np.isfinite(v).all() for v in full.values())
    assert np.array_equal(full["B2"], alone["B2"]), f"{name}: the admitted item depends on when it was admitted or on its neighbours"
    for k in ("A", "B1", "C"):
        assert np.array_equal(full[k], without[k]), f"{name}: item {k} depends on the admission beside it"
    for k, v in full.items():      # frames past the request's length stay zero
        assert not v[:, LENS[rq[k]["slot"]]:].any() and v[:, :LENS[rq[k]["slot"]]].any(), k
    if graph:
        assert caps1 == caps0, f"{name}: admissions recaptured the step graph ({caps0} -> {caps1})"
    return full


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_admission_in_mid_loop(prec, graph, denoisers):
    _check_loop(denoisers[prec], "order2", graph)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", ["ddim_eta1", "guided", "dynamic_thresholding", "order3"])
def test_admission_in_mid_loop_forms(name, prec, denoisers):
    _check_loop(denoisers[prec], name, True)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_graph_and_eager_agree_and_slots_filled_at_step_0_are_the_closed_loop(prec, denoisers):
    """every slot admitted at loop step 0 is ns2vc_sampler_begin's job: the slot loop must end on the bits of Denoiser.sample with per-item
    schedules, lengths and prompt lengths (begin's state, set_condition's tensors), captured and eager"""
    import torch
    den = denoisers[prec]
    _, rq = _case("order2")
    reqs = dict(A=(rq["A"], 0), B1=(rq["B1"], 0), C=(rq["C"], 0))
    g, _, _ = _drive(den, reqs, True)
    e, _, _ = _drive(den, reqs, False)
    c, p, x = (torch.zeros((3, 256, 66), device="cuda"), torch.zeros((3, 5, 256), device="cuda"), torch.zeros((3, 100, 66), device="cuda"))
    for k in ("A", "B1", "C"):
        b = rq[k]["slot"]
        c[b, :, :LENS[b]], p[b, :PLENS[b]], x[b, :, :LENS[b]] = rq[k]["content"], rq[k]["prompt"], rq[k]["noise"]
    closed = den.sample(c, p, None, x, schedules=[rq["A"]["schedule"], rq["B1"]["schedule"], rq["C"]["schedule"]], lengths=list(LENS),
                        prompt_lengths=list(PLENS)).cpu().numpy()
    for k in ("A", "B1", "C"):
        assert np.array_equal(g[k], e[k]), k
        assert np.array_equal(g[k], closed[rq[k]["slot"]]), k


def test_first_fill_runs_the_precision_self_check_and_keeps_the_bits(weights, denoisers):
    from ns2vc_amd.pipeline import Denoiser
    _, rq = _case("order2")
    reqs = dict(B1=(rq["B1"], 0), A=(rq["A"], 2))
    ref, _, _ = _drive(denoisers["fp16"], reqs)
    den = Denoiser(weights, precision="fp16", ln_guard=None, attn_fallback_limit=None)
    assert not den._precision_checked
    got, _, _ = _drive(den, reqs)
    assert den._precision_checked and not den.serving_fp32 and 0 < den.precision_error_seen < 1e-3
    for k in ref:
        assert np.array_equal(got[k], ref[k]), k


# ---- 3. accuracy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,tol", [("fp32", FP32_SAMPLED_TOL), ("fp16", FP16_TOL)])
def test_admitted_item_against_the_oracle(prec, tol, weights, denoisers, diag):
    """the item admitted at loop step 4 (UniPC order 2, 6 steps, 65 frames, 1 prompt frame) against oracle/sampler_ref.py on it alone"""
    import torch
    from ns2vc_amd.spec import UNetConfig
    from oracle import sampler_ref, unet_ref
    forms, rq = _case("order2")
    full, _, _ = _drive(denoisers[prec], dict(A=(rq["A"], 0), B1=(rq["B1"], 0), C=(rq["C"], 0), B2=(rq["B2"], 4)))
    P = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}
    r = rq["B2"]
    c, p, x = r["content"].cpu()[None], r["prompt"].cpu()[None], r["noise"].cpu()[None]
    ref = sampler_ref.unipc_bh2(lambda xx, tt: unet_ref.denoiser(P, UNetConfig(), xx, c, p, None, tt), sampler_ref.linear_betas(), x, 6, order=2).numpy()
    err = rel_l2(full["B2"][:, :LENS[1]], ref[0])
    diag(f"continuous batching: item admitted at loop step 4 vs oracle ({prec}): {err:.3e} (bar {tol:g})")
    assert err < tol


# ---- 4. the per-item condition ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_set_condition_items_keeps_the_other_items_bits(prec, weights):
    """forward before and after one item's condition is replaced: the others keep their bits, the replaced item gets those of a whole-batch
    set_condition with the new tensors"""
    import torch
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    e.prepare(*SHAPE)
    try:
        x, c, p = _tensor("ci.x", (3, 100, 66)), _tensor("ci.c", (3, 256, 66)), _tensor("ci.p", (3, 5, 256))
        c1, p1 = _tensor("ci.c1", (1, 256, 66)), _tensor("ci.p1", (1, 5, 256))
        t = torch.tensor([700.0, 300.5, 20.0], device="cuda")
        e.set_lengths(list(LENS))
        e.set_prompt_lengths(list(PLENS))

        def fwd():
            o = torch.empty_like(x)
            e.forward(x, t, o)
            torch.cuda.synchronize()
            return o.cpu().numpy()
        e.set_condition(c, p, None)
        before = fwd()
        e.set_condition_items([1], c1, p1, None)
        after = fwd()
        c2, p2 = c.clone(), p.clone()
        c2[1], p2[1] = c1[0], p1[0]
        e.set_condition(c2, p2, None)
        whole = fwd()
    finally:
        e.close()
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
    assert np.array_equal(after, whole) and not np.array_equal(after[1], before[1])


# ---- 5. ContinuousConverter ---------------------------------------------------------------------------------------------
PRE_CFG = {"phoneme_encoder": {"in_channels": 256, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2},
           "prompt_encoder": {"in_channels": 100, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2}}


@pytest.fixture(scope="module")
def pre_model():
    import torch
    from ns2vc_amd.frontend import PreModel
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "pre_model_state_keys.json")))
    m = PreModel(PRE_CFG).eval()
    m.load_state_dict(procedural_params(keys["keys"], "pre"), strict=True)
    return m.to(torch.device("cuda", 0))


def test_continuous_converter_against_every_segment_alone(pre_model, denoisers, weights, diag):
    """7 segments on 3 slots with steps {4, 6} in fp32: every segment against Denoiser.sample of it alone (GroupedConverter with batches of one:
    the same x_T and seed per segment).  The engine shapes differ -- (3, 66, 5) against the segment's own -- so bits are not expected."""
    import torch
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import ContinuousConverter, GroupedConverter, Segment
    from ns2vc_amd.weights import hash_normal
    shapes = [(66, 5), (65, 3), (33, 5), (48, 4), (66, 2), (40, 5), (57, 3)]
    segs = [Segment(torch.from_numpy(hash_normal(f"cc.c{i}", (256, T))), torch.from_numpy(hash_normal(f"cc.r{i}", (100, L))), tag=i,
                    schedule=dict(solver="unipc", steps=(4, 6)[i % 2], order=2)) for i, (T, L) in enumerate(shapes)]
    den = denoisers["fp32"]
    conv = ContinuousConverter(pre_model, den, slots=3, max_frames=66, max_prompt=5, solver="unipc", steps=5)
    out = conv.convert(segs)
    assert [r for r, _, _ in conv.last_plan] == [0, 4, 6, 8, 10, 12]      # 34 slot-steps on 3 slots in 12 loop steps
    ref_den = Denoiser(weights, precision="fp32", precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None)
    one = GroupedConverter(pre_model, ref_den, max_batch=1, solver="unipc", steps=5).convert(segs)
    errs = []
    for i, (T, _) in enumerate(shapes):
        assert out[i].shape == (100, T) and torch.isfinite(out[i]).all()
        errs.append(rel_l2(out[i].cpu().numpy(), one[i].cpu().numpy()))
    diag("continuous converter, 7 segments on 3 slots (fp32) vs each alone: " + " ".join(f"{v:.2e}" for v in errs))
    assert max(errs) < FP32_SAMPLED_TOL, errs


# ---- 6. refusals -------------------------------------------------------------------------------------------------------
def test_refusals(weights):
    import torch
    from ns2vc_amd import schedule as S
    from ns2vc_amd._lib import Ns2vcError, check
    from ns2vc_amd.engine import Engine
    engs = [Engine(precision="fp32") for _ in range(2)]
    try:
        for e in engs:
            e.load_state_dict(weights)
            e.prepare(*SHAPE)
            e.set_lengths([66, 66, 66])
            e.set_prompt_lengths([5, 5, 5])
        e, other = engs
        with pytest.raises(Ns2vcError, match="no slot loop"):
            e.admit([0], _tensor("rf.x", (1, 100, 66)), [[0, 4, 0, 0]])
        e.open_slots()
        assert e.slot_step() == 0 and other.slot_step() == -1
        tab = S.build_table("unipc", 4)
        x = _tensor("rf.x", (1, 100, 66))
        with pytest.raises(Ns2vcError, match="never written"):
            e.admit([0], x, [[0, 4, 0, 0]])
        e.write_sampler_rows(0, tab.coef)
        e.admit([0], x, [[0, 4, 0, 0]])
        with pytest.raises(Ns2vcError, match="slot 0 is busy"):
            e.admit([0], x, [[0, 4, 0, 0]])                              # admission into a busy slot
        with pytest.raises(Ns2vcError, match="in use"):
            e.write_sampler_rows(2, tab.coef[:2])                       # rows a running slot walks
        with pytest.raises(Ns2vcError, match="flags"):
            e.admit([1], x, [[0, 4, 0, 1]])
        with pytest.raises(Ns2vcError, match="has not finished"):
            e.take([0], torch.empty_like(x))
        e.sample_steps(2)
        assert e.slot_step() == 2
        with pytest.raises(Ns2vcError, match="lies in the past"):
            e.admit([1], x, [[0, 4, 1, 0]])                              # start in the past
        other.load_sampler("unipc", 4)
        with pytest.raises(Ns2vcError, match="cannot be handed off"):
            check(e.lib.ns2vc_sampler_handoff(other.h, e.h, None), "sampler_handoff")      # handoff from a slot loop
        with pytest.raises(Ns2vcError, match="busy slots"):
            e.load_sampler("unipc", 4)
        with pytest.raises(Ns2vcError, match="drained"):
            e.rebase_slots()
        tab3 = S.build_table("unipc", 6, order=3)
        assert S.table_flags(tab3) == S.ITEM_HIST2
        e.write_sampler_rows(8, tab3.coef)
        with pytest.raises(Ns2vcError, match="opened without it"):
            e.admit([2], x, [[8, 6, 2, 1]])                              # an order-3 item in a loop opened without history 2
        e.sample_steps(2)
        out = torch.empty_like(x)
        e.take([0], out)
        with pytest.raises(Ns2vcError, match="idle"):
            e.take([0], out)
        e.rebase_slots()
        assert e.slot_step() == 0
        e.admit([0], x, [[0, 4, 0, 0]])                                  # a rebased loop goes on: same item, same bits
        e.sample_steps(4)
        again = torch.empty_like(x)
        e.take([0], again)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), again.cpu().numpy()) and torch.isfinite(out).all()
        e.load_sampler("unipc", 4)                                        # drained: a shared table leaves slot mode
        assert e.slot_step() == -1
        y = torch.zeros((3, 100, 66), device="cuda")
        y[0] = x[0]
        e.sample(y)
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy()[0], out.cpu().numpy()[0])   # ... and the closed loop (zero condition, as open left it) gives the item the same bits
    finally:
        for e in engs:
            e.close()


def test_an_error_in_mid_queue_leaves_the_denoiser_usable(pre_model, denoisers, diag):
    """decode_fn fails on the first retired segment, with other slots still busy: convert closes its loop on the way out, so the next convert, the
    next slot loop and the next Denoiser.sample run.  The engine's own results keep their bits across the failure; two conversions (whose front
    end is PyTorch's) agree at the bar of a sampled fp32 latent."""
    import torch
    from ns2vc_amd.service import ContinuousConverter, Segment
    from ns2vc_amd.weights import hash_normal
    den = denoisers["fp32"]
    _, rq = _case("order2")
    reqs = dict(A=(rq["A"], 0), B1=(rq["B1"], 0), B2=(rq["B2"], 4))
    before, _, _ = _drive(den, reqs)
    segs = [Segment(torch.from_numpy(hash_normal(f"ce.c{i}", (256, 40 + i))), torch.from_numpy(hash_normal(f"ce.r{i}", (100, 4))), tag=i,
                    schedule=dict(solver="unipc", steps=(4, 6, 6, 4)[i], order=2)) for i in range(4)]

    def broken(x):
        raise RuntimeError("vocoder down")
    with pytest.raises(RuntimeError, match="vocoder down"):
        ContinuousConverter(pre_model, den, decode_fn=broken, slots=3, max_frames=66, max_prompt=5).convert(segs)
    assert den.engine.slot_step() == -1
    after, _, _ = _drive(den, reqs)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    good = ContinuousConverter(pre_model, den, slots=3, max_frames=66, max_prompt=5)
    a = [t.cpu().numpy() for t in good.convert(segs)]
    b = [t.cpu().numpy() for t in good.convert(segs)]
    errs = [rel_l2(u, v) for u, v in zip(a, b)]
    diag("continuous converter after a failed conversion, two runs of 4 segments (fp32): " + " ".join(f"{v:.2e}" for v in errs))
    assert all(np.isfinite(u).all() for u in a) and max(errs) < FP32_SAMPLED_TOL, errs
    x = den.sample(rq["A"]["content"][None], rq["A"]["prompt"][None], None, rq["A"]["noise"][None], solver="unipc", steps=4)
    assert torch.isfinite(x).all()
