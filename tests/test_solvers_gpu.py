"""Order-3 UniPC / DPM-Solver++ and the other ``sample()`` options on the MI355X: the history-2 solver update alone
(ns2vc_k_solver_update), the captured loop against the reference's own loops (tests/golden/golden_v5.npz g15, make_golden_v5.py), and
the loop's properties -- graph == eager, handoff across the warm-up, table switching, fuse_solver, ragged batches, the Python surface."""
import os

import numpy as np
import pytest

from util import TOL_SOLVER, f16_round, fmt_local, local_errors, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_v5.npz")
# fp32 engine vs the reference's fp32 CPU loop: the repo's fp32 sampled-latent gate (test_engine_gpu.py, test_stochastic_gpu.py)
# measured: UniPC-3 1.2e-6 - 1.5e-6, DPM-Solver++(3M) time_uniform 20 1.9e-5 (its last third-order updates amplify the reference's own
# float32 rounding as much as the engine's)
FP32_TOL = 5e-5
FP32_LOCAL_TOL = 2e-4       # per frame / channel, tests/test_engine_gpu.py LOCAL_TOL["fp32"]; measured <= 2.8e-5 (3M), <= 2.6e-6 (UniPC-3)
# the parity bar; fp16 with the default order-3 tails measured 1.6e-4 - 2.2e-4 for UniPC-3 (tail 1) and 3.0e-4 for DPM-Solver++(3M)
# (tail 4; 1.2e-3 with tail 3) (profiles/r08_order3_solvers.txt)
FP16_TOL = 1e-3
FP16_LOCAL_TOL = 3.2e-3     # per frame / channel, tests/test_engine_gpu.py LOCAL_TOL["fp16"]; measured <= 4.5e-4
# the g15 cases: (solver, steps, order, skip_type, lower_order_final, extra options)
G15 = [("unipc", 10, 3, "logSNR", True, {}), ("unipc", 20, 3, "time_uniform", True, {}), ("dpmsolver++", 20, 3, "time_uniform", True, {}),
       ("unipc", 15, 3, "time_quadratic", True, {"variant": "bh1", "denoise_to_zero": True})]


def case_tag(solver, steps, order, skip, lof, extra):
    t = f"{'unipc' if solver == 'unipc' else 'dpmpp'}{order}_{skip}_{steps}" + ("" if lof else "_nolof")
    for k in sorted(extra):
        v = extra[k]
        t += f"_{k}" if v is True else f"_{k}{v}".replace(".", "p")
    return t


def opts(case):
    solver, steps, order, skip, lof, extra = case
    return dict(order=order, skip_type=skip, lower_order_final=lof, **extra)


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _golden_inputs(gold):
    """the inputs of the g15 loops: make_golden_v5.py draws them with make_golden.inputs("g15", 2, 188, 469) (hash_normal)"""
    import torch
    from ns2vc_amd.weights import hash_normal
    dev = torch.device("cuda", 0)
    B, T, Lp = 2, 188, 469
    x_T = torch.from_numpy(hash_normal("g15.x", (B, 100, T))).to(dev)
    c = torch.from_numpy(hash_normal("g15.content", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("g15.prompt", (B, Lp, 256))).to(dev)
    lens = torch.from_numpy(gold["g15.lens"])
    mask = (torch.arange(p.shape[1])[None, :] < lens[:, None]).to(device=dev, dtype=torch.uint8)
    return x_T, c, p, mask


# ---- the update alone ------------------------------------------------------------------------------
def _update_numpy(row, x0, xe, xb, d1, mp, mp2):
    """schedule.py's recurrence in float64 (mp2 None: without the history-2 terms)"""
    a, s, g0, g1, A, Bc, d1c, pc = (float(v) for v in row[1:9])
    d2c, pe = float(row[10]), float(row[11])
    eps = (xe - a * x0) / s
    m = (xe - s * eps) / a
    x = xb - g0 * d1 - g1 * (m - mp)
    nb = A * x - Bc * m
    nd = d1c * (mp - m) + (d2c * (mp2 - m) if mp2 is not None else 0.0)
    ne = nb - pc * nd - (pe * (mp2 - m) if mp2 is not None else 0.0)
    return ne, nb, nd, m


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("hist2", [True, False])
def test_k_solver_update_against_numpy(prec, hist2, diag):
    from ns2vc_amd import _lib
    from ns2vc_amd import schedule as S
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    rows, ld = 96, 128
    n = rows * ld
    table = S.build_table("unipc", 10, order=3, skip_type="logSNR")
    step = 4                                   # an order-3 row: d2c and pe both nonzero
    assert table.coef[step, 10] != 0 and table.coef[step, 11] != 0
    rng = np.random.default_rng(3)
    st = {k: rng.standard_normal(n).astype(np.float32) for k in ("x0", "xe", "xbar", "d1", "mprev", "mprev2")}
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    coef = DevBuf.from_numpy(np.ascontiguousarray(table.coef, np.float32))
    stepb = DevBuf.from_numpy(np.array([step, 0, 0, 0], np.int32))
    pr = {"fp32": 0, "fp16": 2}[prec]
    op = DevBuf(n * 4 if prec == "fp32" else n * 4)            # fp16: the hi + lo pair, 2 * n halves
    _lib.check(lib.ns2vc_k_solver_update(coef.ptr, stepb.ptr, bufs["x0"].ptr, bufs["xe"].ptr, op.ptr, pr, bufs["xbar"].ptr, bufs["d1"].ptr,
                                         bufs["mprev"].ptr, bufs["mprev2"].ptr if hist2 else None, n, ld, None), "k_solver_update")
    lib.ns2vc_dev_sync()
    got = {k: bufs[k].to_numpy((n,)) for k in st}
    f64 = {k: v.astype(np.float64) for k, v in st.items()}
    ne, nb, nd, m = _update_numpy(table.coef[step], f64["x0"], f64["xe"], f64["xbar"], f64["d1"], f64["mprev"], f64["mprev2"] if hist2 else None)
    errs = {"xe": rel_l2(got["xe"], ne), "xbar": rel_l2(got["xbar"], nb), "d1": rel_l2(got["d1"], nd), "mprev": rel_l2(got["mprev"], m)}
    diag(f"k_solver_update {prec} hist2={hist2}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < TOL_SOLVER, k
    if hist2:
        assert np.array_equal(got["mprev2"], st["mprev"])       # m_{i-1} moves down the history
    else:
        assert np.array_equal(got["mprev2"], st["mprev2"])      # untouched
    if prec == "fp32":
        assert np.array_equal(op.to_numpy((n,)), got["xe"])
    else:
        pair = op.to_numpy((rows, 2 * ld), dtype=np.float16).astype(np.float32)
        hi = f16_round(got["xe"].reshape(rows, ld))
        assert np.array_equal(pair[:, :ld], hi)
        assert np.array_equal(pair[:, ld:], f16_round(got["xe"].reshape(rows, ld) - hi))


def test_k_solver_update_history2_off_rows_agree():
    """on an order <= 2 row (d2c = pe = 0) the history-2 form gives the order-2 form's values"""
    from ns2vc_amd import _lib
    from ns2vc_amd import schedule as S
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    n, ld = 64 * 128, 128
    table = S.build_table("unipc", 10, order=3, skip_type="logSNR")
    step = 1                                   # warm-up row: order 2
    assert not table.coef[step, 10:12].any()
    rng = np.random.default_rng(4)
    st = {k: rng.standard_normal(n).astype(np.float32) for k in ("x0", "xe", "xbar", "d1", "mprev", "mprev2")}
    coef = DevBuf.from_numpy(np.ascontiguousarray(table.coef, np.float32))
    stepb = DevBuf.from_numpy(np.array([step, 0, 0, 0], np.int32))
    outs = []
    for h2 in (False, True):
        b = {k: DevBuf.from_numpy(v) for k, v in st.items()}
        op = DevBuf(n * 4)
        _lib.check(lib.ns2vc_k_solver_update(coef.ptr, stepb.ptr, b["x0"].ptr, b["xe"].ptr, op.ptr, 0, b["xbar"].ptr, b["d1"].ptr,
                                             b["mprev"].ptr, b["mprev2"].ptr if h2 else None, n, ld, None), "k_solver_update")
        lib.ns2vc_dev_sync()
        outs.append([b[k].to_numpy((n,)) for k in ("xe", "xbar", "d1", "mprev")])
    for a, c in zip(*outs):
        assert np.array_equal(a, c)


# ---- parity with the reference (goldens g15) -------------------------------------------------------
@pytest.mark.parametrize("case", G15, ids=[case_tag(*c) for c in G15])
def test_parity_with_reference_loops(case, weights, gold, diag):
    from ns2vc_amd.pipeline import Denoiser
    x_T, c, p, mask = _golden_inputs(gold)
    ref = gold[f"g15.{case_tag(*case)}.y"]
    solver, steps = case[0], case[1]
    y32 = Denoiser(weights, precision="fp32").sample(c, p, mask, x_T, solver=solver, steps=steps, **opts(case)).cpu().numpy()
    den = Denoiser(weights, precision="fp16")
    y16 = den.sample(c, p, mask, x_T, solver=solver, steps=steps, **opts(case)).cpu().numpy()
    e32, l32, e16, l16 = rel_l2(y32, ref), local_errors(y32, ref), rel_l2(y16, ref), local_errors(y16, ref)
    diag(f"{case_tag(*case)} vs reference: fp32 {e32:.2e} {fmt_local(l32)}; fp16 (default tail) {e16:.2e} {fmt_local(l16)}; "
         f"self-check {den.precision_error_seen}")
    assert not den.serving_fp32
    assert e32 < FP32_TOL
    assert l32["frame"] < FP32_LOCAL_TOL and l32["chan"] < FP32_LOCAL_TOL
    assert e16 < FP16_TOL
    assert l16["frame"] < FP16_LOCAL_TOL and l16["chan"] < FP16_LOCAL_TOL


# ---- loop properties -------------------------------------------------------------------------------
def _engine(weights, prec, shape):
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    e.prepare(*shape)
    return e


def _loop(e, x_T, c, p, mask, graph=True, seeds=None):
    import torch
    if seeds is not None:
        e.set_seeds(seeds)
    e.set_condition(c, p, mask)
    x = x_T.clone()
    e.sample(x, use_graph=graph)
    torch.cuda.synchronize()
    return x.cpu().numpy()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("solver", ["unipc", "dpmsolver++"])
def test_graph_equals_eager(prec, solver, weights, gold):
    x_T, c, p, mask = _golden_inputs(gold)
    e = _engine(weights, prec, (2, 188, 469))
    try:
        e.load_sampler(solver, 10, order=3, skip_type="logSNR")
        g = _loop(e, x_T, c, p, mask, True)
        ea = _loop(e, x_T, c, p, mask, False)
        g2 = _loop(e, x_T, c, p, mask, True)
    finally:
        e.close()
    assert np.array_equal(g, ea) and np.array_equal(g, g2)


def test_handoff_across_the_warm_up(weights, gold, diag):
    """begin / steps(k) / handoff to a second fp32 engine / steps(rest) / end == one loop, for every k up to past the step at which
    m_prev2 first holds a model value (after evaluation 1) and is first read (row 2)"""
    import torch
    x_T, c, p, mask = _golden_inputs(gold)
    engs = [_engine(weights, "fp32", (2, 188, 469)) for _ in range(2)]
    try:
        for e in engs:
            e.load_sampler("unipc", 10, order=3, skip_type="logSNR")
            e.set_condition(c, p, mask)
        whole = _loop(engs[0], x_T, c, p, mask)
        for k in range(1, 6):
            x = x_T.clone()
            engs[0].sample(x, tail=engs[1], tail_steps=10 - k)
            torch.cuda.synchronize()
            assert np.array_equal(x.cpu().numpy(), whole), f"handoff after {k} steps"
        x = x_T.clone()                   # and the other direction (the second engine's buffer already exists)
        engs[1].sample(x, tail=engs[0], tail_steps=7)
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy(), whole)
    finally:
        for e in engs:
            e.close()


def test_table_switching(weights, gold):
    """order 3 -> order 2 -> DDIM eta 1 -> order 3 on one engine == each on a fresh engine (a stale graph or m_prev2 would show)"""
    from ns2vc_amd import schedule as S
    x_T, c, p, mask = _golden_inputs(gold)
    b64 = S.linear_betas(1000, np.float64)
    seeds = np.array([11, 12], np.uint64)
    seq = [(("dpmsolver++", 10, None, 3, 0.0), {"skip_type": "logSNR"}), (("dpmsolver++", 10, None, 2, 0.0), {}),
           (("ddim", 20, b64, 2, 1.0), {}), (("unipc", 12, None, 3, 0.0), {"skip_type": "time_quadratic"})]
    e = _engine(weights, "fp16", (2, 188, 469))
    try:
        shared = []
        for args, kw in seq:
            e.load_sampler(*args, **kw)
            shared.append(_loop(e, x_T, c, p, mask, seeds=seeds if args[0] == "ddim" else None))
    finally:
        e.close()
    for (args, kw), got in zip(seq, shared):
        f = _engine(weights, "fp16", (2, 188, 469))
        try:
            f.load_sampler(*args, **kw)
            fresh = _loop(f, x_T, c, p, mask, seeds=seeds if args[0] == "ddim" else None)
        finally:
            f.close()
        assert np.array_equal(got, fresh), args


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_fuse_solver_leaves_order3_unfolded(prec, weights, gold):
    x_T, c, p, mask = _golden_inputs(gold)
    out = []
    for fuse in (False, True):
        e = _engine(weights, prec, (2, 188, 469))
        try:
            if fuse:
                e.set_option("fuse_solver", True)
                e.prepare(2, 188, 469)
            e.load_sampler("unipc", 10, order=3, skip_type="logSNR")
            out.append(_loop(e, x_T, c, p, mask))
        finally:
            e.close()
    assert np.array_equal(out[0], out[1])


def test_ragged_batch_items_equal_items_alone(weights, diag):
    """B=3 ragged, UniPC-3 logSNR: item b on [0, L_b) == item b alone at T = L_b (fp32, 1e-5), exact zeros beyond"""
    import torch
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.weights import hash_normal
    lens, Lp = [188, 131, 64], 40
    T = max(lens)
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("so.c", (3, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("so.p", (1, Lp, 256))).expand(3, -1, -1).contiguous().to(dev)
    x_T = torch.zeros(3, 100, T, device=dev)
    for b, L in enumerate(lens):
        x_T[b, :, :L] = torch.from_numpy(hash_normal(f"so.x{b}", (100, L))).to(dev)
    den = Denoiser(weights, precision="fp32")
    for solver in ("unipc", "dpmsolver++"):
        y = den.sample(c, p, None, x_T, solver=solver, steps=10, order=3, skip_type="logSNR", lengths=lens).cpu().numpy()
        worst = 0.0
        for b, L in enumerate(lens):
            assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0
            one = den.sample(c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), None, x_T[b:b + 1, :, :L].contiguous(), solver=solver,
                             steps=10, order=3, skip_type="logSNR").cpu().numpy()
            worst = max(worst, rel_l2(y[b, :, :L], one[0]))
        diag(f"ragged {solver}-3 logSNR fp32: worst item vs alone {worst:.2e}")
        assert worst < 1e-5


def test_denoiser_matches_engine_loop(weights, gold):
    """Denoiser.sample(order=3, skip_type=...) is the engine loop on the same table, bit for bit (fp32: no tail)"""
    from ns2vc_amd.pipeline import Denoiser
    x_T, c, p, mask = _golden_inputs(gold)
    den = Denoiser(weights, precision="fp32")
    y = den.sample(c, p, mask, x_T, solver="dpmsolver++", steps=12, order=3, skip_type="logSNR", denoise_to_zero=True).cpu().numpy()
    assert den.engine.table.steps == 13
    e = _engine(weights, "fp32", (2, 188, 469))
    try:
        e.load_sampler("dpmsolver++", 12, order=3, skip_type="logSNR", denoise_to_zero=True)
        ref = _loop(e, x_T, c, p, mask)
    finally:
        e.close()
    assert np.array_equal(y, ref)
    with pytest.raises(TypeError, match="unknown"):
        den.sample(c, p, mask, x_T, solver="unipc", steps=10, order=3, skiptype="logSNR")
    with pytest.raises(ValueError, match="multistep"):
        den.sample(c, p, mask, x_T, solver="unipc", steps=10, order=3, method="singlestep")


def test_grouped_converter_passes_options(weights):
    """GroupedConverter(order=3, skip_type=...) runs the denoiser on that table"""
    import json
    import torch
    from ns2vc_amd import schedule as S
    from ns2vc_amd.frontend import PreModel
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import GroupedConverter, Segment
    from ns2vc_amd.weights import hash_normal
    from util import procedural_params
    cfg = {"phoneme_encoder": {"in_channels": 256, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2},
           "prompt_encoder": {"in_channels": 100, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2}}
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "pre_model_state_keys.json")))
    pre = PreModel(cfg).eval()
    pre.load_state_dict(procedural_params(keys["keys"], "pre"), strict=True)
    pre = pre.to(torch.device("cuda", 0))
    segs = [Segment(torch.from_numpy(hash_normal(f"sog.c{i}", (256, 96))), torch.from_numpy(hash_normal("sog.r", (100, 40))), tag=i)
            for i in range(2)]
    den = Denoiser(weights, precision="fp32")
    outs = {}
    for skip in ("logSNR", "time_uniform"):
        outs[skip] = GroupedConverter(pre, den, max_batch=2, solver="unipc", steps=10, order=3, skip_type=skip).convert(segs)
        want = S.build_table("unipc", 10, den.betas, 3, skip_type=skip)
        assert np.array_equal(den.engine.table.coef, want.coef)
    for i in range(2):
        assert torch.isfinite(outs["logSNR"][i]).all()
        assert rel_l2(outs["logSNR"][i].cpu().numpy(), outs["time_uniform"][i].cpu().numpy()) > 1e-4
