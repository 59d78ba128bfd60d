"""Per-item sampler schedules on the MI355X: the items update alone (ns2vc_k_solver_update_items) against the shared-table hooks and the fp64
recurrence, a mixed batch against the reference's own loops (golden_v5 g15), and the loop's properties -- an item gets the bits the shared
table gives it (plain, ragged, guided, corrected, stochastic), graph == eager, hand-off at every split, what recaptures, GroupedConverter."""
import json
import os

import numpy as np
import pytest

from test_solvers_gpu import FP16_LOCAL_TOL, FP16_TOL, FP32_LOCAL_TOL, FP32_TOL, _golden_inputs, _update_numpy
from util import TOL_SOLVER, fmt_local, local_errors, procedural_params, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_v5.npz")
# UniPC-2 6 steps, DPM-Solver++(3M) 5 steps, UniPC-3 4 steps: S = 6, starts 0 / 1 / 2
SPECS = [dict(solver="unipc", steps=6, order=2), dict(solver="dpmsolver++", steps=5, order=3), dict(solver="unipc", steps=4, order=3)]
SHAPE = (3, 66, 5)


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---- 6. the update alone ---------------------------------------------------------------------------
T6, LD6, NI6 = 9, 128, 4
PER6 = T6 * LD6
STEP6 = 4
# (row0, steps, start, flags): active order 2 (j = 2); active history 2 on an order-3 row (j = 4); not yet started (j = -1); finished (j = 4 >= 4)
ITEMS6 = np.array([[0, 6, 2, 0], [6, 10, 0, 1], [0, 6, 5, 0], [6, 4, 0, 1]], np.int32)
ACTIVE6, HELD6 = (0, 1), (2, 3)


def _tables6():
    from ns2vc_amd import schedule as S
    a, b = S.build_table("unipc", 6, order=2), S.build_table("unipc", 10, order=3, skip_type="logSNR")
    assert b.coef[4, 10] != 0 and b.coef[4, 11] != 0 and not a.coef[:, 10:12].any()
    return np.ascontiguousarray(np.concatenate([a.coef, b.coef]), np.float32)


def _state6(guided, seed):
    rng = np.random.default_rng(seed)
    n = NI6 * PER6
    st = {k: rng.standard_normal(n).astype(np.float32) for k in ("xbar", "d1", "mprev", "mprev2")}
    st["x0"] = rng.standard_normal(2 * n if guided else n).astype(np.float32)
    xe = rng.standard_normal(n).astype(np.float32)
    st["xe"] = np.concatenate([xe, xe]) if guided else xe          # (a guided loop holds the same point in both halves)
    return st


def _op_bytes(prec, n):
    return n * 4          # fp32: n floats; fp16: the hi + lo pair, 2 n halves


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_k_solver_update_items(prec, guided, diag):
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    pr = {"fp32": 0, "fp16": 2}[prec]
    coef_h = _tables6()
    coef = DevBuf.from_numpy(coef_h)
    stepb = DevBuf.from_numpy(np.array([STEP6, 0, 0, 0], np.int32))
    n, halves = NI6 * PER6, 2 if guided else 1
    st = _state6(guided, 6)
    scales_h = np.array([2.5, 1.0, 0.5, 3.0], np.float32)
    scales = DevBuf.from_numpy(scales_h) if guided else None
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    op0 = np.full(_op_bytes(prec, halves * n), 0x5A, np.uint8)      # the pre-filled operand buffer
    op = DevBuf.from_numpy(op0)
    _lib.check(lib.ns2vc_k_solver_update_items(coef.ptr, coef_h.shape[0], stepb.ptr, ITEMS6.ctypes.data, NI6, bufs["x0"].ptr, bufs["xe"].ptr, op.ptr, pr,
                                               bufs["xbar"].ptr, bufs["d1"].ptr, bufs["mprev"].ptr, bufs["mprev2"].ptr, n, LD6, T6,
                                               scales.ptr if guided else None, None, None, 100, 0, 0.995, 1.0, None, None), "k_solver_update_items")
    lib.ns2vc_dev_sync()
    got = {k: bufs[k].to_numpy(st[k].shape) for k in st}
    got_op = op.to_numpy(op0.shape, dtype=np.uint8)

    def item(a, b, half=0):      # item b's elements of a state tensor (half 1: the conditional half of x0 / xe)
        return a[half * n + b * PER6: half * n + (b + 1) * PER6]

    def op_item(a, b, half=0):
        w = _op_bytes(prec, PER6)
        return a[(half * NI6 + b) * w: (half * NI6 + b + 1) * w]

    # held items: every state tensor and the operand buffer keep their bits
    for b in HELD6:
        for k in ("xbar", "d1", "mprev", "mprev2"):
            assert np.array_equal(item(got[k], b), item(st[k], b)), (b, k)
        for h in range(halves):
            assert np.array_equal(item(got["xe"], b, h), item(st["xe"], b, h)), (b, h)
            assert np.array_equal(op_item(got_op, b, h), op_item(op0, b, h)), (b, h)
    # active items: the bits of the shared-table hook on the item's data with its row, and the fp64 recurrence
    for b in ACTIVE6:
        row, h2 = int(ITEMS6[b, 0] + STEP6 - ITEMS6[b, 2]), bool(ITEMS6[b, 3] & 1)
        ref = {k: DevBuf.from_numpy(np.ascontiguousarray(item(st[k], b))) for k in ("xbar", "d1", "mprev", "mprev2")}
        ref["x0"] = DevBuf.from_numpy(np.concatenate([item(st["x0"], b, h) for h in range(halves)]))
        ref["xe"] = DevBuf.from_numpy(np.concatenate([item(st["xe"], b, h) for h in range(halves)]))
        rop = DevBuf.from_numpy(np.full(_op_bytes(prec, halves * PER6), 0x5A, np.uint8))
        rstep = DevBuf.from_numpy(np.array([row, 0, 0, 0], np.int32))
        if guided:
            sc = DevBuf.from_numpy(scales_h[b:b + 1])
            _lib.check(lib.ns2vc_k_solver_update_guided(coef.ptr, rstep.ptr, ref["x0"].ptr, ref["xe"].ptr, rop.ptr, pr, ref["xbar"].ptr, ref["d1"].ptr,
                                                        ref["mprev"].ptr, ref["mprev2"].ptr if h2 else None, PER6, LD6, sc.ptr, T6, None, None, 100, None),
                       "k_solver_update_guided")
        else:
            _lib.check(lib.ns2vc_k_solver_update(coef.ptr, rstep.ptr, ref["x0"].ptr, ref["xe"].ptr, rop.ptr, pr, ref["xbar"].ptr, ref["d1"].ptr,
                                                 ref["mprev"].ptr, ref["mprev2"].ptr if h2 else None, PER6, LD6, None), "k_solver_update")
        lib.ns2vc_dev_sync()
        for k in ("xbar", "d1", "mprev", "mprev2"):
            assert np.array_equal(item(got[k], b), ref[k].to_numpy((PER6,))), (b, k)
        rxe, ropb = ref["xe"].to_numpy((halves * PER6,)), rop.to_numpy((_op_bytes(prec, halves * PER6),), dtype=np.uint8)
        w = _op_bytes(prec, PER6)
        for h in range(halves):
            assert np.array_equal(item(got["xe"], b, h), rxe[h * PER6:(h + 1) * PER6]), (b, h)
            assert np.array_equal(op_item(got_op, b, h), ropb[h * w:(h + 1) * w]), (b, h)
        if not h2:
            assert np.array_equal(item(got["mprev2"], b), item(st["mprev2"], b))      # an order-2 item's m_prev2 is untouched
        f64 = {k: item(st[k], b).astype(np.float64) for k in ("xbar", "d1", "mprev", "mprev2")}
        x0 = item(st["x0"], b).astype(np.float64)
        if guided and scales_h[b] != 1.0:
            x0 = x0 + float(scales_h[b]) * (item(st["x0"], b, 1).astype(np.float64) - x0)
        elif guided:
            x0 = item(st["x0"], b, 1).astype(np.float64)
        ne, nb, nd, m = _update_numpy(coef_h[row], x0, item(st["xe"], b).astype(np.float64), f64["xbar"], f64["d1"], f64["mprev"], f64["mprev2"] if h2 else None)
        errs = {"xe": rel_l2(item(got["xe"], b), ne), "xbar": rel_l2(item(got["xbar"], b), nb), "d1": rel_l2(item(got["d1"], b), nd),
                "mprev": rel_l2(item(got["mprev"], b), m)}
        diag(f"k_solver_update_items {prec} guided={guided} item {b}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v < TOL_SOLVER, (b, k)


def test_k_solver_update_items_dynamic_thresholding_leaves_held_thresholds():
    """mode 1: active items get the bits (and the threshold) of ns2vc_k_solver_update_corrected on their data; a held item's thr keeps its value"""
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    coef_h = _tables6()
    coef, stepb = DevBuf.from_numpy(coef_h), DevBuf.from_numpy(np.array([STEP6, 0, 0, 0], np.int32))
    n = NI6 * PER6
    st = _state6(False, 7)
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    op = DevBuf(n * 4)
    thr0 = np.array([-1.0, -2.0, -3.0, -4.0], np.float32)
    thr = DevBuf.from_numpy(thr0)
    _lib.check(lib.ns2vc_k_solver_update_items(coef.ptr, coef_h.shape[0], stepb.ptr, ITEMS6.ctypes.data, NI6, bufs["x0"].ptr, bufs["xe"].ptr, op.ptr, 0,
                                               bufs["xbar"].ptr, bufs["d1"].ptr, bufs["mprev"].ptr, bufs["mprev2"].ptr, n, LD6, T6, None, None, None, 100,
                                               1, 0.9, 0.5, thr.ptr, None), "k_solver_update_items")
    lib.ns2vc_dev_sync()
    got, gthr = {k: bufs[k].to_numpy((n,)) for k in st}, thr.to_numpy((4,))
    for b in HELD6:
        assert gthr[b] == thr0[b]
        for k in ("xe", "xbar", "d1", "mprev", "mprev2"):
            assert np.array_equal(got[k][b * PER6:(b + 1) * PER6], st[k][b * PER6:(b + 1) * PER6]), (b, k)
    for b in ACTIVE6:
        row, h2 = int(ITEMS6[b, 0] + STEP6 - ITEMS6[b, 2]), bool(ITEMS6[b, 3] & 1)
        ref = {k: DevBuf.from_numpy(np.ascontiguousarray(st[k][b * PER6:(b + 1) * PER6])) for k in st}
        rop, rthr, rstep = DevBuf(PER6 * 4), DevBuf.from_numpy(np.zeros(4, np.float32)), DevBuf.from_numpy(np.array([row, 0, 0, 0], np.int32))
        _lib.check(lib.ns2vc_k_solver_update_corrected(coef.ptr, rstep.ptr, ref["x0"].ptr, ref["xe"].ptr, rop.ptr, 0, ref["xbar"].ptr, ref["d1"].ptr,
                                                       ref["mprev"].ptr, ref["mprev2"].ptr if h2 else None, PER6, LD6, T6, None, None, 100, 1, 0.9, 0.5,
                                                       rthr.ptr, None), "k_solver_update_corrected")
        lib.ns2vc_dev_sync()
        assert gthr[b] == rthr.to_numpy((4,))[0] and gthr[b] > 0
        for k in ("xe", "xbar", "d1", "mprev") + (("mprev2",) if h2 else ()):
            assert np.array_equal(got[k][b * PER6:(b + 1) * PER6], ref[k].to_numpy((PER6,))), (b, k)


# ---- 7. a mixed batch against the reference's own loops ---------------------------------------------
def test_mixed_batch_parity_with_reference_loops(weights, gold, diag):
    """g15 inputs (B = 2, T = 188, Lp = 469): item 0 runs unipc3_logSNR_10, item 1 dpmpp3_time_uniform_20, in ONE loop of 20 steps"""
    from ns2vc_amd.pipeline import Denoiser
    x_T, c, p, mask = _golden_inputs(gold)
    sch = [dict(solver="unipc", steps=10, order=3, skip_type="logSNR"), dict(solver="dpmsolver++", steps=20, order=3, skip_type="time_uniform")]
    refs = [gold["g15.unipc3_logSNR_10.y"][0:1], gold["g15.dpmpp3_time_uniform_20.y"][1:2]]
    y32 = Denoiser(weights, precision="fp32").sample(c, p, mask, x_T, schedules=sch).cpu().numpy()
    den = Denoiser(weights, precision="fp16")
    y16 = den.sample(c, p, mask, x_T, schedules=sch).cpu().numpy()
    assert den.engine.tables is not None and den.engine.tables.steps == 20 and not den.serving_fp32
    for b, ref in enumerate(refs):
        e32, l32 = rel_l2(y32[b:b + 1], ref), local_errors(y32[b:b + 1], ref)
        e16, l16 = rel_l2(y16[b:b + 1], ref), local_errors(y16[b:b + 1], ref)
        diag(f"mixed batch item {b} ({sch[b]['solver']} {sch[b]['steps']}) vs reference: fp32 {e32:.2e} {fmt_local(l32)}; fp16 (default tail) {e16:.2e} "
             f"{fmt_local(l16)}; self-check {den.precision_error_seen}")
        assert e32 < FP32_TOL and l32["frame"] < FP32_LOCAL_TOL and l32["chan"] < FP32_LOCAL_TOL
        assert e16 < FP16_TOL and l16["frame"] < FP16_LOCAL_TOL and l16["chan"] < FP16_LOCAL_TOL


# ---- 8. an item gets what the shared table gives it ---------------------------------------------------
def _inputs(tag, B=SHAPE[0], T=SHAPE[1], Lp=SHAPE[2]):
    import torch
    from ns2vc_amd.weights import hash_normal
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(hash_normal(tag + ".x", (B, 100, T))).to(dev), torch.from_numpy(hash_normal(tag + ".c", (B, 256, T))).to(dev),
            torch.from_numpy(hash_normal(tag + ".p", (B, Lp, 256))).to(dev))


def _engine(weights, prec, shape=SHAPE):
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    e.prepare(*shape)
    return e


def _load_shared(e, spec):
    kw = {k: v for k, v in spec.items() if k not in ("solver", "steps", "order", "eta")}
    e.load_sampler(spec["solver"], spec["steps"], None, spec.get("order", 2), spec.get("eta", 0.0), **kw)


def _loop(e, x_T, graph=True, **kw):
    import torch
    x = x_T.clone()
    e.sample(x, use_graph=graph, **kw)
    torch.cuda.synchronize()
    return x.cpu().numpy()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_item_gets_the_shared_table_bits(prec, weights):
    x_T, c, p = _inputs("is8")
    e = _engine(weights, prec)
    try:
        e.set_condition(c, p, None)
        shared = []
        for spec in SPECS:
            _load_shared(e, spec)
            shared.append(_loop(e, x_T))
        tabs = e.load_samplers(SPECS)
        assert tabs.steps == 6 and tabs.start.tolist() == [0, 1, 2] and e.loop_steps == 6
        g, ea, g2 = _loop(e, x_T, True), _loop(e, x_T, False), _loop(e, x_T, True)
    finally:
        e.close()
    for k in range(3):
        assert np.array_equal(g[k], shared[k][k]), SPECS[k]
    assert np.array_equal(g, ea) and np.array_equal(g, g2)


# ---- 9. compositions, through Denoiser.sample ---------------------------------------------------------
@pytest.fixture(scope="module")
def denoisers(weights):
    from ns2vc_amd.pipeline import Denoiser
    return {prec: Denoiser(weights, precision=prec, precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None) for prec in ("fp32", "fp16")}


def _uncond():
    import torch
    from ns2vc_amd.weights import hash_normal
    return torch.from_numpy(hash_normal("is9.u", (1, 3, 256))).to(torch.device("cuda", 0))


DDIM = dict(solver="ddim", steps=5, eta=1.0)
COMPOSITIONS = {
    "ragged": (SPECS, lambda: dict(lengths=[66, 41, 17])),
    "guided": (SPECS, lambda: dict(guidance_scale=[2.5, 1.0, 0.5], unconditional_prompt=_uncond())),
    "clamp": (SPECS, lambda: dict(correcting_x0_fn="clamp", thresholding_max_val=0.8)),
    "dynamic_thresholding": (SPECS, lambda: dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=0.9, thresholding_max_val=0.5)),
    "ddim_beside_unipc": ([SPECS[0], DDIM, SPECS[2]], lambda: dict(seeds=np.array([21, 22, 23], np.uint64))),
}


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("name", sorted(COMPOSITIONS))
def test_compositions_keep_the_shared_table_bits(name, prec, denoisers):
    import torch
    specs, kw = COMPOSITIONS[name]
    kw = kw()
    x_T, c, p = _inputs("is9")
    if "lengths" in kw:
        x_T = x_T * (torch.arange(SHAPE[1], device=x_T.device)[None, None, :] < torch.tensor(kw["lengths"], device=x_T.device)[:, None, None])
    den = denoisers[prec]
    mixed = den.sample(c, p, None, x_T, schedules=specs, **kw).cpu().numpy()
    assert den.engine.tables is not None
    for k, spec in enumerate(specs):
        own = den.sample(c, p, None, x_T, schedules=[spec] * 3, **kw).cpu().numpy()      # equal schedules: the shared-table loop of item k's own
        assert den.engine.tables is None
        assert np.array_equal(mixed[k], own[k]), (name, spec)
    assert np.isfinite(mixed).all()


# ---- 10. hand-off ------------------------------------------------------------------------------------
def test_handoff_at_every_split(weights):
    """a mixed fp32 loop split after S - k steps for k = 1 .. S - 1 (k = 5, 4: item 2, then item 1, has not started when the state moves)"""
    import torch
    x_T, c, p = _inputs("is10")
    engs = [_engine(weights, "fp32") for _ in range(2)]
    try:
        for e in engs:
            e.load_samplers(SPECS)
            e.set_condition(c, p, None)
        whole = _loop(engs[0], x_T)
        for k in range(1, 6):
            assert np.array_equal(_loop(engs[0], x_T, tail=engs[1], tail_steps=k), whole), f"tail of {k}"
        engs[1].load_samplers([SPECS[0], SPECS[1], SPECS[1]])           # other schedules on the tail: refused
        from ns2vc_amd._lib import Ns2vcError
        with pytest.raises(Ns2vcError):
            engs[0].sample(x_T.clone(), tail=engs[1], tail_steps=2)
        torch.cuda.synchronize()
    finally:
        for e in engs:
            e.close()


# ---- 11. what recaptures ---------------------------------------------------------------------------------
def test_recapture_rules(weights):
    x_T, c, p = _inputs("is11")
    other = [dict(solver="unipc", steps=5, order=2), dict(solver="dpmsolver++", steps=6, order=3), dict(solver="unipc", steps=3, order=3)]
    seq = [("items", SPECS), ("items", other), ("shared", SPECS[1]), ("items", SPECS)]

    def load(e, kind, what):
        e.load_samplers(what) if kind == "items" else _load_shared(e, what)

    e = _engine(weights, "fp16")
    try:
        e.set_condition(c, p, None)
        got, caps = [], []
        for kind, what in seq:
            load(e, kind, what)
            got.append(_loop(e, x_T))
            caps.append(e.graph_captures())
    finally:
        e.close()
    # new schedules of the same form and union flags replay the graph; to a shared table and back recaptures twice
    assert caps[1] == caps[0] and caps[2] == caps[1] + 1 and caps[3] == caps[2] + 1, caps
    assert np.array_equal(got[0], got[3])
    for (kind, what), g in list(zip(seq, got))[1:3]:
        f = _engine(weights, "fp16")
        try:
            f.set_condition(c, p, None)
            load(f, kind, what)
            assert np.array_equal(_loop(f, x_T), g), kind
        finally:
            f.close()


def test_union_flags_recapture_and_capacity(weights):
    """a stochastic item joins: the union "needs seeds" changes and the graph is captured again; begin wants seeds; too many rows are refused"""
    from ns2vc_amd import schedule as S
    from ns2vc_amd._lib import Ns2vcError
    x_T, c, p = _inputs("is11")
    b64 = S.linear_betas(1000, np.float64)
    e = _engine(weights, "fp16")
    try:
        e.set_condition(c, p, None)
        e.load_samplers(SPECS)
        _loop(e, x_T)
        c0 = e.graph_captures()
        e.load_samplers([SPECS[0], DDIM, SPECS[2]], discrete_betas=b64)
        with pytest.raises(Ns2vcError, match="seeds"):
            e.sample(x_T.clone())
        e.set_seeds(np.array([1, 2, 3], np.uint64))
        _loop(e, x_T)
        assert e.graph_captures() == c0 + 1
        with pytest.raises(Ns2vcError, match="1024"):
            e.load_samplers([dict(solver="ddim", steps=600), dict(solver="ddim", steps=500), SPECS[0]], discrete_betas=b64)
    finally:
        e.close()


# ---- 12. GroupedConverter ---------------------------------------------------------------------------------
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


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("fp16", 2e-3)])      # (tests/test_service_gpu.py: a batched against a differently batched run)
def test_grouped_converter_serves_mixed_schedules_in_one_batch(pre_model, denoisers, precision, tol, diag):
    import torch
    from ns2vc_amd.service import GroupedConverter, Segment
    from ns2vc_amd.weights import hash_normal
    den = denoisers[precision]
    shapes = [(80, 24), (64, 24), (80, 24), (64, 24), (80, 24), (64, 24)]
    segs = [Segment(torch.from_numpy(hash_normal(f"is12.c{i}", (256, T))), torch.from_numpy(hash_normal(f"is12.r{i}", (100, L))), tag=i, schedule=SPECS[i % 3])
            for i, (T, L) in enumerate(shapes)]
    conv = GroupedConverter(pre_model, den, max_batch=4, solver="unipc", steps=6)
    assert conv.plan(segs) == [[0, 2, 4], [1, 3, 5]]
    calls = []
    orig = den.sample
    den.sample = lambda *a, **k: (calls.append(k.get("schedules")), orig(*a, **k))[1]
    try:
        out = conv.convert(segs)
    finally:
        del den.sample
    assert len(calls) == 2 and all(s is not None and len(s) == 3 for s in calls)      # one denoiser call per shape group
    errs = []
    for k, spec in enumerate(SPECS):      # ... and every segment what a converter built for its schedule gives it
        kw = {a: b for a, b in spec.items() if a not in ("solver", "steps", "order")}
        plain = [Segment(s.content, s.refer, tag=s.tag) for s in segs]
        one = GroupedConverter(pre_model, den, max_batch=4, solver=spec["solver"], steps=spec["steps"], order=spec["order"], **kw).convert(plain)
        for i in range(k, 6, 3):
            assert out[i].shape == (100, shapes[i][0]) and torch.isfinite(out[i]).all()
            errs.append(rel_l2(out[i].cpu().numpy(), one[i].cpu().numpy()))
    diag(f"grouped converter with per-segment schedules ({precision}) vs converters of one schedule: max rel {max(errs):.3e}")
    assert max(errs) < tol
