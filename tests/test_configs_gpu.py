"""The HIP engine on every non-default configuration of tests/configs.py, against the oracle on the CPU (pinned to the reference on the
same matrix by tests/test_configs_cpu.py / golden_v6): forward parity in every precision and block by block in fp32, every plan option,
length-masked batches, the captured sampling loops (deterministic and stochastic), the device noise at every channel count the
matrix reaches, and the drop-in module.  Each configuration is held to the bars of the stock one (tests/test_engine_gpu.py)."""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

from configs import CONFIGS, ENGINE_REFUSED, ctor_kwargs
from test_engine_gpu import (BF16_TOL, BIT_IDENTICAL, FP32_LOCAL_TOL, FP32_SAMPLED_TOL, FP32_TOL, LOCAL_TOL, OPTION_DEFAULTS, PARITY_TOL,
                             SAMPLED_VS_FP32, SIXTEEN_BIT_ONLY, run_forward, run_sampler)
from util import fmt_local, local_errors, rel_l2

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v6.npz")
TOL = {"fp32": FP32_TOL, "fp16": PARITY_TOL, "bf16": BF16_TOL}
CIDS = sorted(CONFIGS)
# the forward shape of the matrix: odd T, not a multiple of 2^(levels - 1); items of different scale, timestep and prompt length
B, T, LP = 3, 45, 21


@functools.lru_cache(maxsize=None)
def weights(cid):
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(CONFIGS[cid], 0)


@functools.lru_cache(maxsize=None)
def inputs(cid, B=B, T=T, Lp=LP):
    from ns2vc_amd.weights import hash_normal
    cfg = CONFIGS[cid]
    s = np.array([1.0, 4.0, 0.25][:B] + [1.0] * max(0, B - 3), dtype=np.float32)[:, None, None]
    x = hash_normal(f"cfg.{cid}.x", (B, cfg.latent_channels, T)) * s
    c = hash_normal(f"cfg.{cid}.c", (B, cfg.content_channels, T)) * s
    p = hash_normal(f"cfg.{cid}.p", (B, Lp, cfg.cross_attention_dim))
    lens = np.array([Lp, Lp // 2 + 1, 1, Lp][:B])
    mask = np.arange(Lp)[None, :] < lens[:, None]
    t = np.array([999.0, 500.5, 3.0, 250.0][:B], dtype=np.float32)
    return x, c, p, mask, t


def oracle(cid, x, c, p, mask, t, taps=None):
    import torch
    from oracle import unet_ref
    P = _torch_weights(cid)
    m = None if mask is None else torch.from_numpy(mask)
    sample = torch.cat([torch.from_numpy(x), torch.from_numpy(c)], dim=1)
    return unet_ref.unet_forward(P, CONFIGS[cid], sample, torch.from_numpy(np.asarray(t, dtype=np.float32)), torch.from_numpy(p), m,
                                 taps=taps).numpy()


@functools.lru_cache(maxsize=None)
def _torch_weights(cid):
    import torch
    return {k: torch.from_numpy(v) for k, v in weights(cid).items()}


@functools.lru_cache(maxsize=None)
def oracle_forward(cid):
    return oracle(cid, *inputs(cid))


@pytest.fixture(scope="module")
def engine():
    """engine(cid, prec): one engine per (configuration, precision) for the whole module"""
    from ns2vc_amd.engine import Engine
    cache = {}

    def get(cid, prec):
        if (cid, prec) not in cache:
            e = Engine(CONFIGS[cid], precision=prec)
            e.load_state_dict(weights(cid))
            cache[cid, prec] = e
        return cache[cid, prec]
    yield get
    for e in cache.values():
        e.close()


def check_forward(prec, y, y_or, what):
    e, m = rel_l2(y, y_or), local_errors(y, y_or)
    assert np.isfinite(y).all(), what
    assert e < TOL[prec], (what, prec, e)
    if prec == "fp32":
        assert m["frame"] < FP32_LOCAL_TOL and m["chan"] < FP32_LOCAL_TOL, (what, m)
    else:
        for k, v in LOCAL_TOL[prec].items():
            assert m[k] < v, (what, prec, k, m)
    return f"rel_l2 {e:.3e} {fmt_local(m)}"


# ---- 1. forward parity ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("cid", CIDS)
def test_forward_parity(cid, prec, engine, diag):
    """B = 3, T = 45, a ragged prompt mask, timesteps 999 / 500.5 / 3: whole tensor and per frame / channel at the stock bars"""
    x, c, p, mask, t = inputs(cid)
    y = run_forward(engine(cid, prec), x, c, p, mask, t)
    diag(f"config {cid} forward {prec}: " + check_forward(prec, y, oracle_forward(cid), cid))


@pytest.mark.parametrize("cid", CIDS)
def test_forward_block_by_block_fp32(cid, engine, diag):
    """the golden_v6 b2 inputs (the reference's own output is the final check): every block tap of the fp32 engine against the oracle's,
    so that a failure names its block; channel lanes the engine pads (latent < 128) must hold zeros"""
    from configs import golden_inputs
    x, c, p, mask, t = golden_inputs(cid, "b2")
    eng = engine(cid, "fp32")
    try:
        y = run_forward(eng, x, c, p, mask, t, debug=True)
        etaps = eng.taps()
    finally:
        eng.set_debug(False)
    otaps = {}
    y_or = oracle(cid, x, c, p, mask, t, taps=otaps)
    assert set(otaps) - {"emb"} <= set(etaps), sorted(set(otaps) - set(etaps))
    worst = ("", 0.0)
    for name, a in etaps.items():
        if name == "aug":
            continue
        o = otaps[name].numpy()
        if o.ndim == 3:
            o = o.transpose(0, 2, 1).reshape(-1, o.shape[1])
        assert a.shape[0] == o.shape[0] and a.shape[1] >= o.shape[1], (name, a.shape, o.shape)
        assert not a[:, o.shape[1]:].any(), (cid, name, "padded lanes")
        e = rel_l2(a[:, :o.shape[1]], o)
        assert e < FP32_TOL, (cid, name, e)
        worst = max(worst, (name, e), key=lambda w: w[1])
    e_gold = rel_l2(y, np.load(GOLD)[f"{cid}.b2.y"])
    diag(f"config {cid} fp32 block by block: worst tap {worst[0]} {worst[1]:.3e}; forward vs oracle {rel_l2(y, y_or):.3e}, vs reference {e_gold:.3e}")
    assert e_gold < FP32_TOL and rel_l2(y, y_or) < FP32_TOL


# ---- 2. plan options ------------------------------------------------------------------------------
def _loop(eng, x, c, p, mask):
    return (run_sampler(eng, "unipc", 3, 2, x, c, p, mask, True), run_sampler(eng, "unipc", 3, 2, x, c, p, mask, False))


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("cid", ["lat98_h128", "h4_w256", "lat128_h512"])
def test_every_plan_option(cid, prec, engine, diag):
    """each plan option away from its default (tests/test_engine_gpu.py OPTION_DEFAULTS): forward against the oracle at the bars; a
    bit-identical option equals the default plan bit for bit (forward and the 3-step UniPC loop); graph == eager; the loop within
    bounds of the fp32 engine's default plan"""
    x, c, p, mask, t = inputs(cid)
    y_or = oracle_forward(cid)
    eng = engine(cid, prec)
    s32 = run_sampler(engine(cid, "fp32"), "unipc", 3, 2, x, c, p, mask, True)
    y0 = run_forward(eng, x, c, p, mask, t)
    g0, _ = _loop(eng, x, c, p, mask)
    for opt, dflt in OPTION_DEFAULTS.items():
        if prec == "fp32" and opt in SIXTEEN_BIT_ONLY:
            continue
        eng.set_option(opt, not dflt)
        try:
            y1 = run_forward(eng, x, c, p, mask, t)
            g1, e1 = _loop(eng, x, c, p, mask)
        finally:
            eng.set_option(opt, bool(dflt))
        es = rel_l2(g1, s32)
        if opt == "attn_fp8":
            assert np.isfinite(y1).all() and rel_l2(y1, y_or) < 5e-2, (cid, opt)
            msg = f"rel_l2 {rel_l2(y1, y_or):.3e}"
        else:
            msg = check_forward(prec, y1, y_or, f"{cid} {opt}")
        diag(f"config {cid} option {opt}={int(not dflt)} {prec}: forward {msg}; same as default forward {np.array_equal(y1, y0)} "
             f"loop {np.array_equal(g1, g0)}; graph == eager {np.array_equal(g1, e1)}; loop vs fp32 engine {es:.3e}")
        assert np.array_equal(g1, e1), (cid, opt, prec)
        assert es < (5e-2 if opt == "attn_fp8" else SAMPLED_VS_FP32[prec]), (cid, opt, prec, es)
        if opt in BIT_IDENTICAL:
            assert np.array_equal(y1, y0) and np.array_equal(g1, g0), (cid, opt, prec)


# ---- 3. length-masked batches -----------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("cid", ["lat98_h128", "lpb1_g4", "lv3"])
def test_ragged_batch_items_equal_oracle_alone(cid, prec, engine, diag):
    """item b of a batch padded to T = 45 (lengths not multiples of 2^(levels - 1)) against the oracle run on that item alone at its own
    length; the caller's padding holds garbage, the engine's output past each item's end is exactly 0"""
    from ns2vc_amd.engine import DevBuf, sync
    cfg = CONFIGS[cid]
    lens = [45, 37, 11, 3]
    x, c, p, mask, t = inputs(cid, B=4)
    x, c = x.copy(), c.copy()
    for b, L in enumerate(lens):
        x[b, :, L:] = 7.0
        c[b, :, L:] = -3.0
    eng = engine(cid, prec)
    eng.set_debug(False)
    eng.prepare(4, T, LP)
    try:
        eng.set_lengths(lens)
        d_x, d_c, d_p, d_m = DevBuf.from_numpy(x), DevBuf.from_numpy(c), DevBuf.from_numpy(p), DevBuf.from_numpy(mask.astype(np.uint8))
        d_t, d_o = DevBuf.from_numpy(t), DevBuf(x.nbytes)
        d_o.upload(np.full(x.shape, np.nan, np.float32))
        eng.set_condition(d_c, d_p, d_m)
        eng.forward(d_x, d_t, d_o)
        sync()
        y = d_o.to_numpy(x.shape)
    finally:
        eng.prepare(4, T, LP)           # (prepare resets the lengths: the cached engine is dense again)
        eng.shape = None
    tol = {"fp32": (FP32_TOL, FP32_LOCAL_TOL), "fp16": (1.5e-3, LOCAL_TOL["fp16"]["frame"])}[prec]
    for b, L in enumerate(lens):
        assert not np.abs(y[b, :, L:]).any(), (cid, b)
        ref = oracle(cid, x[b:b + 1, :, :L], c[b:b + 1, :, :L], p[b:b + 1], mask[b:b + 1], t[b:b + 1])
        m = local_errors(y[b:b + 1, :, :L], ref)
        diag(f"config {cid} ragged {prec} L={L} of {T}: {fmt_local(m)}")
        assert np.isfinite(y[b]).all() and m["item"] < tol[0] and m["frame"] < tol[1], (cid, b, L, m)
    assert cfg.latent_channels == y.shape[1]


# ---- 4. sampling -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _x0_torch(cid, B_):
    import torch
    x, c, p, mask, _ = inputs(cid, B=B_)
    from oracle import unet_ref
    P, cfg = _torch_weights(cid), CONFIGS[cid]
    ct, pt, mt = torch.from_numpy(c), torch.from_numpy(p), torch.from_numpy(mask)
    return lambda xx, tt: unet_ref.denoiser(P, cfg, xx, ct, pt, mt, tt.float())


@pytest.mark.parametrize("cid", CIDS)
def test_sampling_loops_fp32(cid, engine, diag):
    """UniPC order 2 (5 steps) against the reference-restating sampler (oracle/sampler_ref.py) and DPM-Solver++ order 3 (6 steps)
    against the host executor of its table (ns2vc_amd.schedule.run_table_numpy), both driven by the oracle; graph == eager"""
    import torch
    from ns2vc_amd.schedule import build_table, run_table_numpy
    from oracle import sampler_ref
    x, c, p, mask, _ = inputs(cid, B=2)
    f = _x0_torch(cid, 2)
    eng = engine(cid, "fp32")
    ref_u = sampler_ref.unipc_bh2(f, sampler_ref.linear_betas(), torch.from_numpy(x), 5, order=2).numpy()
    g_u = run_sampler(eng, "unipc", 5, 2, x, c, p, mask, True)
    e_u = run_sampler(eng, "unipc", 5, 2, x, c, p, mask, False)
    ref_d = run_table_numpy(build_table("dpmsolver++", 6, order=3), lambda xx, tt: f(torch.from_numpy(xx), torch.from_numpy(tt)).numpy(), x)
    g_d = run_sampler(eng, "dpmsolver++", 6, 3, x, c, p, mask, True)
    e_d = run_sampler(eng, "dpmsolver++", 6, 3, x, c, p, mask, False)
    eu, ed = rel_l2(g_u, ref_u), rel_l2(g_d, ref_d)
    diag(f"config {cid} sampled fp32: unipc2 x5 {eu:.3e} {fmt_local(local_errors(g_u, ref_u))}; dpm++3 x6 {ed:.3e} {fmt_local(local_errors(g_d, ref_d))}")
    assert np.array_equal(g_u, e_u) and np.array_equal(g_d, e_d), "hipGraph replay must be bit-identical to eager launches"
    assert eu < FP32_SAMPLED_TOL and ed < FP32_SAMPLED_TOL, (eu, ed)


@pytest.mark.parametrize("solver,steps,eta", [("ddim", 6, 1.0), ("ddpm", 100, 0.0)], ids=["ddim6_eta1", "ddpm100"])
@pytest.mark.parametrize("cid", ["lat98_h128", "mel80_h384"])
def test_stochastic_loops_fp32(cid, solver, steps, eta, engine, diag):
    """DDIM with eta = 1 (1000-step schedule) and DDPM over a 100-step schedule, on the device's noise, against the host executor with the
    host statement of that noise (ns2vc_amd.noise.gauss) injected, driven by the oracle; graph == eager"""
    import torch
    from ns2vc_amd import noise as N
    from ns2vc_amd.engine import DevBuf, Stream, sync
    from ns2vc_amd.schedule import linear_betas, run_table_numpy
    cfg = CONFIGS[cid]
    x, c, p, mask, _ = inputs(cid, B=2)
    seeds = np.array([0x0123456789ABCDEF, 42], dtype=np.uint64)
    betas = linear_betas(1000 if solver == "ddim" else steps, np.float64)
    eng = engine(cid, "fp32")
    eng.set_debug(False)
    eng.prepare(2, T, LP)
    outs = []
    try:
        table = eng.load_sampler(solver, steps, betas=betas, eta=eta)
        for graph in (True, False):
            st = Stream()
            d_x = DevBuf.from_numpy(x)
            eng.set_seeds(seeds, stream=st)
            eng.set_condition(DevBuf.from_numpy(c), DevBuf.from_numpy(p), DevBuf.from_numpy(mask.astype(np.uint8)), stream=st)
            eng.sample(d_x, use_graph=graph, stream=st)
            st.sync()
            sync()
            outs.append(d_x.to_numpy(x.shape))
    finally:
        eng.shape = None
    f = _x0_torch(cid, 2)
    ref = run_table_numpy(table, lambda xx, tt: f(torch.from_numpy(xx), torch.from_numpy(tt)).numpy(), x,
                          noise_fn=lambda i: N.gauss(seeds, i, cfg.latent_channels, T))
    e = rel_l2(outs[0], ref)
    diag(f"config {cid} {solver} x{steps} eta {eta} fp32 vs host loop with gauss(): {e:.3e} {fmt_local(local_errors(outs[0], ref))}")
    assert np.array_equal(outs[0], outs[1])
    assert e < FP32_SAMPLED_TOL, e


# ---- 5. the noise kernel at the matrix's channel counts ------------------------------------------------
@pytest.mark.parametrize("nc", [1, 3, 98, 127, 128])
def test_k_noise_channel_counts(nc, diag):
    """ns2vc_k_noise into 128-wide rows for nc channels (partial Philox quads at 1, 3, 98, 127): lanes c >= nc and frames past an item's
    length receive no noise (the kernel writes zeros there over a NaN poison), the rest equals the host statement"""
    from ns2vc_amd import _lib
    from ns2vc_amd import noise as N
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    seeds = np.array([0x0123456789ABCDEF, 1, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    Tn, ld, lens = 45, 128, [45, 30, 1]
    d_s, d_l = DevBuf.from_numpy(seeds), DevBuf.from_numpy(np.asarray(lens, dtype=np.int32))
    poison = np.full((3, Tn, ld), np.nan, np.float32)
    out = DevBuf.from_numpy(poison)
    _lib.check(lib.ns2vc_k_noise(d_s.ptr, 3, nc, Tn, ld, 7, d_l.ptr, out.ptr, None), "k_noise")
    lib.ns2vc_dev_sync()
    dev = out.to_numpy((3, Tn, ld))
    host = N.gauss(seeds, 7, nc, Tn, lens).transpose(0, 2, 1)
    assert (dev[:, :, nc:] == 0).all(), "noise in lanes past nc"
    for b, L in enumerate(lens):
        assert (dev[b, L:] == 0).all(), (b, "noise in frames past the item's length")
        d = np.abs(dev[b, :L, :nc].astype(np.float64) - host[b, :L])
        ulp = d / np.spacing(np.maximum(np.abs(host[b, :L]), 1.0).astype(np.float32))
        assert ulp.max() <= 8, (nc, b, ulp.max())
    diag(f"k_noise nc={nc} ld={ld}: lanes >= nc and frames past each length zero; valid lanes within 8 ulp of gauss()")


# ---- 6. the drop-in module -------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["mel80_h384", "lat98_h128", "lat128_h512"])
def test_dropin_module_on_the_matrix(cid, diag):
    """UNet1DConditionModel built with the reference's ctor kwargs, loaded strictly, called as the reference is called (cat([x, content])):
    fp32 matches the oracle; "auto" picks the engine its self-check measured"""
    import torch
    from unet1d import UNet1DConditionModel
    x, c, p, mask, t = inputs(cid)
    y_or = oracle_forward(cid)
    dev = torch.device("cuda", 0)
    args = (torch.cat([torch.from_numpy(x), torch.from_numpy(c)], dim=1).to(dev), torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev))
    out = {}
    for prec in ("fp32", "auto"):
        m = UNet1DConditionModel(engine_precision=prec, **ctor_kwargs(CONFIGS[cid]))
        m.load_state_dict(_torch_weights(cid), strict=True)
        m = m.to(dev).eval()
        with torch.no_grad():
            out[prec] = m(*args, encoder_attention_mask=torch.from_numpy(mask).to(dev)).sample.cpu().numpy()
        assert m.autograd_calls == 0 and (prec != "fp32" or m.engine_calls == 1)
        if prec == "auto":
            seen = m.precision_error_seen
            assert seen is not None
            worst = m.precision_error_worst_item
            ok = seen <= m.precision_check and worst <= m.precision_check
            assert m._precision == ("fp16" if ok else "fp32"), (seen, worst, m._precision)
            chosen = m._precision
    e32, ea = rel_l2(out["fp32"], y_or), rel_l2(out["auto"], y_or)
    diag(f"config {cid} drop-in: fp32 {e32:.3e}; auto chose {chosen} (self-check {seen:.2e}, worst item {worst:.2e}) -> {ea:.3e}")
    assert e32 < FP32_TOL
    assert ea < (PARITY_TOL if chosen == "fp16" else FP32_TOL)


@pytest.mark.parametrize("rid", sorted(ENGINE_REFUSED))
def test_dropin_module_refuses_loudly(rid):
    """validate() accepts these, the engine does not: the first forward raises an error naming the field, never returns a result"""
    import torch
    from ns2vc_amd._lib import Ns2vcError
    from ns2vc_amd.weights import procedural_state_dict
    from unet1d import UNet1DConditionModel
    cfg, field = ENGINE_REFUSED[rid]
    m = UNet1DConditionModel(engine_precision="fp32", **ctor_kwargs(cfg))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg, 0).items()}, strict=True)
    dev = torch.device("cuda", 0)
    m = m.to(dev).eval()
    sample = torch.zeros(1, cfg.in_channels, 16, device=dev)
    prompt = torch.zeros(1, 4, cfg.cross_attention_dim, device=dev)
    with torch.no_grad(), pytest.raises(Ns2vcError, match=field):
        m(sample, torch.tensor([10.0], device=dev), prompt)
