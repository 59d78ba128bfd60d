"""Length-masked batches on the MI355X (ns2vc_unet_set_lengths): item b of a batch padded to T gives, on frames [0, L_b), what the
engine gives for that item alone at T = L_b (to the precision's rounding), and exactly 0 beyond -- forward, sampling loop (eager and
captured), every plan option, the precision self-check / LayerNorm guard and the ragged service."""
import os

import numpy as np
import pytest

from util import local_errors, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"fp32": 1e-5, "fp16": 1e-3}
FRAME_TOL = {"fp32": 4e-5, "fp16": 3.2e-3}     # per frame / channel (local_errors): tests/test_engine_gpu.py FP32_LOCAL_TOL, LOCAL_TOL["fp16"]
LENS = [938, 937, 700, 263, 131, 129, 127, 125, 3, 2, 1]
OPTIONS = ["ln_linear", "fold_ff", "fuse_ffn", "fuse_ffn_pre", "fuse_geglu", "fuse_rows", "fuse_rows_gn", "fuse_gn_gemm", "fuse_gn_cat", "gn_coop",
           "slice_rows", "attn_fp8", "attn_optimistic", "conv_ts", "conv_wtiled", "gn_inloop", "fuse_solver", "fuse_xattn", "fork_temb", "exact_io", "split_io"]


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


def _inputs(B, T, Lp, tag):
    import torch
    from ns2vc_amd.weights import hash_normal
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(hash_normal(f"{tag}.x", (B, 100, T))).to(dev)
    c = torch.from_numpy(hash_normal(f"{tag}.c", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal(f"{tag}.p", (1, Lp, 256))).expand(B, -1, -1).contiguous().to(dev)
    t = torch.linspace(50.0, 900.0, B, device=dev)
    return x, c, p, t


def _forward(e, x, c, p, t, lengths=None):
    import torch
    B, _, T = x.shape
    if e.shape != (B, T, p.shape[1]):
        e.prepare(B, T, p.shape[1])
    e.set_lengths(lengths)
    e.set_condition(c, p, None)
    out = torch.empty_like(x)
    e.forward(x, t, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_forward_padded_batch_equals_items_alone(prec, weights, diag):
    import torch
    from ns2vc_amd.engine import Engine
    from ns2vc_amd.spec import UNetConfig
    from oracle import unet_ref
    T, Lp = max(LENS), 40
    x, c, p, t = _inputs(len(LENS), T, Lp, "rg1")
    for b, L in enumerate(LENS):           # the caller's padding is arbitrary: the engine must not read it
        x[b, :, L:] = 7.0
        c[b, :, L:] = -3.0
    e = Engine(precision=prec)
    try:
        e.load_state_dict(weights)
        y = _forward(e, x, c, p, t, LENS)
        worst = (0.0, 0.0)
        P = None
        for b, L in enumerate(LENS):
            assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0, b
            assert np.isfinite(y[b]).all()
            if L >= 8:
                ref = _forward(e, x[b:b + 1, :, :L].contiguous(), c[b:b + 1, :, :L].contiguous(),
                               p[b:b + 1].contiguous(), t[b:b + 1].contiguous())
            else:                          # (the engine needs T >= 8: items shorter than that against the CPU oracle alone)
                if P is None:
                    P = {k: torch.from_numpy(v) for k, v in weights.items()}
                ref = unet_ref.denoiser(P, UNetConfig(), x[b:b + 1, :, :L].cpu(), c[b:b + 1, :, :L].cpu(), p[b:b + 1].cpu(), None,
                                        t[b:b + 1].cpu()).numpy()
            m = local_errors(y[b:b + 1, :, :L], ref)
            worst = (max(worst[0], m["item"]), max(worst[1], m["frame"]))
            diag(f"ragged forward {prec} L={L}: item {m['item']:.2e} frame {m['frame']:.2e} chan {m['chan']:.2e}")
            if prec != "bf16":
                # (a 16-bit item against the fp32 ORACLE carries the operand rounding of both sides' distance, not of two 16-bit runs: one frame
                #  averages nothing, measured 1.2e-3 at L = 1 -- twice the bar there)
                tol = TOL[prec] * (2 if (L < 8 and prec != "fp32") else 1)
                assert m["item"] < tol, (L, m)
                assert m["frame"] < FRAME_TOL[prec] and m["chan"] < FRAME_TOL[prec], (L, m)   # a leaking halo / statistic is O(1) on the last frames
            if prec == "fp32" and 8 <= L <= 263:
                # ... and the independent CPU oracle on the item alone (the lengths around the 32 / 64 / 66-frame planner thresholds of the deep levels)
                if P is None:
                    P = {k: torch.from_numpy(v) for k, v in weights.items()}
                ro = unet_ref.denoiser(P, UNetConfig(), x[b:b + 1, :, :L].cpu(), c[b:b + 1, :, :L].cpu(), p[b:b + 1].cpu(), None, t[b:b + 1].cpu()).numpy()
                mo = local_errors(y[b:b + 1, :, :L], ro)
                diag(f"ragged forward fp32 L={L} vs oracle alone: item {mo['item']:.2e} frame {mo['frame']:.2e}")
                assert mo["item"] < TOL["fp32"] and mo["frame"] < FRAME_TOL["fp32"] and mo["chan"] < FRAME_TOL["fp32"], (L, mo)
        diag(f"ragged forward {prec}: worst item {worst[0]:.2e}, worst frame {worst[1]:.2e}")
    finally:
        e.close()


def test_dense_restore_and_full_lengths(weights, diag):
    from ns2vc_amd.engine import Engine
    B, T, Lp = 3, 300, 40
    x, c, p, t = _inputs(B, T, Lp, "rg2")
    e = Engine(precision="fp16")
    try:
        e.load_state_dict(weights)
        y0 = _forward(e, x, c, p, t)
        n0 = len(e.op_info(0))
        yf = _forward(e, x, c, p, t, [T] * B)
        y1 = _forward(e, x, c, p, t, None)
        assert len(e.op_info(0)) == n0
        with pytest.raises(Exception):
            e.set_lengths([T + 1, 1, 1])
        with pytest.raises(Exception):
            e.set_lengths([0, 1, 1])
        y2 = _forward(e, x, c, p, t, None)
        e.prepare(B, T, Lp)                 # a new prepare is dense again
        assert e.lengths is None
        y3 = _forward(e, x, c, p, t)
    finally:
        e.close()
    assert np.array_equal(y0, y1) and np.array_equal(y0, y2) and np.array_equal(y0, y3)      # dense restored bit for bit
    ef = rel_l2(yf, y0)
    diag(f"lengths == T (masked plan) vs dense plan, fp16: {ef:.2e}")
    assert ef < TOL["fp16"]


@pytest.mark.parametrize("solver,steps,tail", [("unipc", 20, 0), ("dpmsolver++", 50, 3)])
def test_sampled_padded_batch_equals_items_alone(solver, steps, tail, weights, diag):
    import torch
    from ns2vc_amd.pipeline import Denoiser
    lens = [300, 211, 97, 64, 9]
    T, Lp = max(lens), 40
    _, c, p, _ = _inputs(len(lens), T, Lp, "rg3")
    noise = torch.zeros(len(lens), 100, T, device=c.device)
    for b, L in enumerate(lens):
        noise[b, :, :L] = torch.randn((100, L), generator=torch.Generator().manual_seed(b)).to(c.device)
    den = Denoiser(weights, precision="fp16")
    outs = {}
    for g in (True, False):
        outs[g] = den.sample(c, p, None, noise, solver=solver, steps=steps, use_graph=g, tail_fp32=tail, lengths=lens).cpu().numpy()
    assert not den.serving_fp32 and not den._ln_switched         # no false fallback from the self-check or the LayerNorm guard
    worst = 0.0
    for b, L in enumerate(lens):
        assert float(np.abs(outs[True][b, :, L:]).max() if L < T else 0.0) == 0.0
        one = den.sample(c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), None, noise[b:b + 1, :, :L].contiguous(), solver=solver, steps=steps,
                         use_graph=True, tail_fp32=tail).cpu().numpy()
        e = rel_l2(outs[True][b, :, :L], one[0])
        worst = max(worst, e)
        assert rel_l2(outs[False][b, :, :L], one[0]) < 2.5e-3
    diag(f"ragged sampling {solver}-{steps} fp16 (fp32 tail {tail}): worst item vs alone {worst:.2e}; graph vs eager {rel_l2(outs[True], outs[False]):.2e}")
    assert worst < 2.5e-3


def test_graph_captured_under_other_lengths(weights, diag):
    import torch
    from ns2vc_amd.engine import Engine
    B, T, Lp = 4, 256, 40
    _, c, p, _ = _inputs(B, T, Lp, "rg4")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(3)).to(c.device)
    A, Bl = [256, 200, 100, 9], [17, 256, 255, 64]
    e = Engine(precision="fp16")
    try:
        e.load_state_dict(weights)
        e.prepare(B, T, Lp)
        e.load_sampler("unipc", 10)
        e.set_lengths(A)
        e.set_condition(c, p, None)
        xa = xT.clone()
        e.sample(xa, use_graph=True)          # captured under A
        e.set_lengths(Bl)
        e.set_condition(c, p, None)
        xg = xT.clone()
        e.sample(xg, use_graph=True)          # the same graph replayed under B
        xe = xT.clone()
        e.sample(xe, use_graph=False)
        torch.cuda.synchronize()
    finally:
        e.close()
    xg, xe = xg.cpu().numpy(), xe.cpu().numpy()
    assert np.array_equal(xg, xe)
    for b, L in enumerate(Bl):
        assert float(np.abs(xg[b, :, L:]).max() if L < T else 0.0) == 0.0


def _sample(e, c, p, xT, lens, graph, steps=4):
    import torch
    B, _, T = xT.shape
    if e.shape != (B, T, p.shape[1]):
        e.prepare(B, T, p.shape[1])
    e.load_sampler("unipc", steps)
    e.set_lengths(lens)
    e.set_condition(c, p, None)
    x = xT.clone()
    e.sample(x, use_graph=graph)
    torch.cuda.synchronize()
    return x.cpu().numpy()


def test_every_plan_option_under_lengths(weights, diag):
    """each plan option, switched from its default, either gives what the default plan gives under the same lengths or refuses -- through one
    forward AND through a short sampling loop, captured and eager (fuse_solver and fork_temb act in the sampler's step only), with the frames
    past every item's end exactly zero"""
    import torch
    from ns2vc_amd.engine import Engine
    from ns2vc_amd import _lib
    lens = [300, 131, 66, 64, 33, 9]
    B, T, Lp = len(lens), 300, 40
    x, c, p, t = _inputs(B, T, Lp, "rg5")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(5)).to(c.device)

    def zero_tail(y):
        for b, L in enumerate(lens):
            assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0, (b, L)

    e = Engine(precision="fp16")
    try:
        e.load_state_dict(weights)
        y0 = _forward(e, x, c, p, t, lens)
        s0 = _sample(e, c, p, xT, lens, True)
        assert np.array_equal(s0, _sample(e, c, p, xT, lens, False))
        zero_tail(s0)
    finally:
        e.close()
    for opt in OPTIONS:
        f = Engine(precision="fp16")
        try:
            f.load_state_dict(weights)
            try:
                f.set_option(opt, opt in ("attn_fp8", "gn_inloop", "fuse_solver", "fuse_xattn", "fork_temb", "exact_io"))
            except _lib.Ns2vcError:
                continue                  # not available on this device (gn_coop without the placement)
            y = _forward(f, x, c, p, t, lens)
            sg = _sample(f, c, p, xT, lens, True)
            se = _sample(f, c, p, xT, lens, False)
        finally:
            f.close()
        e1, eg, ee = rel_l2(y, y0), rel_l2(sg, s0), rel_l2(se, s0)
        diag(f"option {opt} flipped under lengths vs the default plan: forward {e1:.2e}, sampled graph {eg:.2e} eager {ee:.2e}")
        tol = 6e-3 if opt == "attn_fp8" else 2e-3
        assert e1 < tol and eg < tol and ee < tol, opt
        assert rel_l2(sg, se) < 1e-6, opt
        for yy in (y, sg, se):
            zero_tail(yy)


def test_ragged_service_equals_equal_shape_grouping(diag):
    import json
    import torch
    from ns2vc_amd.frontend import PreModel
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import GroupedConverter, Segment
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    from util import procedural_params
    cfg = {"phoneme_encoder": {"in_channels": 256, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2},
           "prompt_encoder": {"in_channels": 100, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2}}
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "pre_model_state_keys.json")))
    pre = PreModel(cfg).eval()
    pre.load_state_dict(procedural_params(keys["keys"], "pre"), strict=True)
    pre = pre.to(torch.device("cuda", 0))
    lengths = [96, 130, 97, 64, 131, 9, 250]
    segs = [Segment(torch.from_numpy(hash_normal(f"rgs.c{i}", (256, T))), torch.from_numpy(hash_normal("rgs.r", (100, 40))), tag=i)
            for i, T in enumerate(lengths)]
    den = Denoiser(procedural_state_dict(seed=0), precision="fp16")
    rag = GroupedConverter(pre, den, max_batch=4, solver="unipc", steps=8, ragged=True)
    assert rag.plan(segs) == [[6, 4, 1, 2], [0, 3, 5]]
    out = rag.convert(segs)
    ref = GroupedConverter(pre, den, max_batch=4, solver="unipc", steps=8).convert(segs)
    errs = []
    for i, (a, b) in enumerate(zip(out, ref)):
        assert a.shape == (100, lengths[i]) and torch.isfinite(a).all()
        errs.append(rel_l2(a.cpu().numpy(), b.cpu().numpy()))
    diag(f"ragged service vs equal-shape grouping, fp16: max {max(errs):.2e}")
    assert max(errs) < 2.5e-3
