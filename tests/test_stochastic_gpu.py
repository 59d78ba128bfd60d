"""The stochastic samplers on the MI355X: the device noise generator (ns2vc_k_noise against ns2vc_amd.noise, its statistics, its zeros),
DDIM / DDPM loops against the reference's own ddim_sample / p_sample_loop (tests/golden/golden_v4.npz g13), and the loop's properties --
graph == eager, seeds, fuse_solver, handoff, independence from the batch, the bench shape."""
import os

import numpy as np
import pytest

from util import NOISE_ULP, fmt_local, local_errors, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_v4.npz")
# fp32 engine vs the reference's fp32 CPU loop: the fp32 grade of the other sampled-latent bounds (test_engine_gpu.py: 5e-5);
# measured 1.5e-6 for all three loops of golden_v4 (profiles/r08_stochastic.txt)
FP32_TOL = 5e-5
# the parity bar; fp16 with the default tail of one fp32 evaluation measured 1.3e-4 - 1.5e-4 against golden_v4 and 1.4e-4 against
# the fp32 engine at the bench shape (7.6e-4 - 7.8e-4 without a tail)
FP16_TOL = 1e-3
FP16_LOCAL_TOL = 3.2e-3     # per frame / channel, tests/test_engine_gpu.py LOCAL_TOL["fp16"]; measured <= 3.3e-4 (<= 1.5e-3 without a tail)
G13 = [("ddim", 100, 0.0), ("ddim", 30, 1.0), ("ddpm", 1000, 0.0)]


def tag(solver, steps, eta):
    return f"{solver}{steps}_eta{eta:g}".replace(".", "p")


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _k_noise(seeds, C, T, ld, step, lens=None):
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    B = len(seeds)
    d_s = DevBuf.from_numpy(np.asarray(seeds, dtype=np.uint64))
    d_l = DevBuf.from_numpy(np.asarray(lens, dtype=np.int32)) if lens is not None else None
    out = DevBuf(B * T * ld * 4)
    _lib.check(lib.ns2vc_k_noise(d_s.ptr, B, C, T, ld, step, d_l.ptr if d_l else None, out.ptr, None), "k_noise")
    lib.ns2vc_dev_sync()
    return out.to_numpy((B, T, ld))


# ---- the generator -----------------------------------------------------------------------------
@pytest.mark.parametrize("step", [0, 5, 999])
def test_k_noise_equals_host_statement(step, diag):
    from ns2vc_amd import noise as N
    seeds = np.array([0x0123456789ABCDEF, 1, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    lens = [517, 300, 1]
    dev = _k_noise(seeds, 100, 517, 128, step, lens)
    host = N.gauss(seeds, step, 100, 517, lens).transpose(0, 2, 1)
    assert not dev[:, :, 100:].any()                       # padding channels
    for b, L in enumerate(lens):
        assert not dev[b, L:].any()                        # frames past the item's end
    d = np.abs(dev[:, :, :100].astype(np.float64) - host)
    ulp = d / np.spacing(np.maximum(np.abs(host), 1.0).astype(np.float32))
    diag(f"k_noise step {step} vs noise.gauss: max |d| {d.max():.2e}, max {ulp.max():.1f} ulp of max(|z|, 1)")
    assert ulp.max() <= NOISE_ULP


def test_k_noise_statistics(diag):
    """>= 1e7 normals: moments and the correlations between neighbouring steps, items, frames and channels against N(0, 1) and
    independence, each within 5 sigma (the seeds fix the data: deterministic)"""
    seeds = np.arange(1, 5, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    T = 25000
    z0 = _k_noise(seeds, 100, T, 100, 17).astype(np.float64)        # (4, T, 100): 1e7
    z1 = _k_noise(seeds, 100, T, 100, 18).astype(np.float64)
    n = z0.size
    m, v = z0.mean(), z0.var()
    k = ((z0 - m) ** 4).mean() / v ** 2
    corr = {"step": (z0 * z1).mean(), "item": (z0[1:] * z0[:-1]).mean(), "frame": (z0[:, 1:] * z0[:, :-1]).mean(),
            "channel": (z0[:, :, 1:] * z0[:, :, :-1]).mean(), "pair": (z0[:, :, 0::2] * z0[:, :, 1::2]).mean()}
    diag(f"k_noise statistics over {n:.1e}: mean {m:.2e} var {v:.5f} kurtosis {k:.4f}; correlations " +
         " ".join(f"{a} {b:.1e}" for a, b in corr.items()) + f" (1 sigma = {1 / np.sqrt(n):.1e})")
    assert abs(m) < 5 / np.sqrt(n)
    assert abs(v - 1) < 5 * np.sqrt(2 / n)
    assert abs(k - 3) < 5 * np.sqrt(24 / n)
    for name, c in corr.items():
        assert abs(c) < 5 / np.sqrt(n / 2), name
    assert z0.min() > -8 and z0.max() < 8


# ---- parity with the reference (goldens g13) ----------------------------------------------------------
def _golden_inputs(gold):
    """the inputs of the g13 loops: make_golden_v4.py draws them with hash_normal (make_golden.inputs("g13", 2, 188, 469)) and stores
    only the prompt lengths and seeds"""
    import torch
    from ns2vc_amd.weights import hash_normal
    dev = torch.device("cuda", 0)
    B, T, Lp = 2, 188, 469
    x_T = torch.from_numpy(hash_normal("g13.x", (B, 100, T))).to(dev)
    c = torch.from_numpy(hash_normal("g13.content", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("g13.prompt", (B, Lp, 256))).to(dev)
    lens = torch.from_numpy(gold["g13.lens"])
    mask = (torch.arange(p.shape[1])[None, :] < lens[:, None]).to(device=dev, dtype=torch.uint8)
    return x_T, c, p, mask


@pytest.mark.parametrize("solver,steps,eta", G13, ids=[tag(*c) for c in G13])
def test_parity_with_reference_loops(solver, steps, eta, weights, gold, diag):
    from ns2vc_amd.pipeline import Denoiser
    x_T, c, p, mask = _golden_inputs(gold)
    ref = gold[f"g13.{tag(solver, steps, eta)}.y"]
    seeds = gold["g13.seeds"]
    y32 = Denoiser(weights, precision="fp32").sample(c, p, mask, x_T, solver=solver, steps=steps, eta=eta, seeds=seeds).cpu().numpy()
    den = Denoiser(weights, precision="fp16")
    y16 = den.sample(c, p, mask, x_T, solver=solver, steps=steps, eta=eta, seeds=seeds).cpu().numpy()
    e32, e16, loc = rel_l2(y32, ref), rel_l2(y16, ref), local_errors(y16, ref)
    diag(f"{tag(solver, steps, eta)} vs reference: fp32 {e32:.2e}; fp16 (tail {den.tail_fp32}) {e16:.2e} {fmt_local(loc)}; "
         f"self-check {den.precision_error_seen}")
    assert not den.serving_fp32
    assert e32 < FP32_TOL
    assert e16 < FP16_TOL
    assert loc["frame"] < FP16_LOCAL_TOL and loc["chan"] < FP16_LOCAL_TOL


# ---- loop properties ----------------------------------------------------------------------------------
def _engine_loop(e, x_T, c, p, mask, seeds, graph=True):
    import torch
    e.set_seeds(seeds)
    e.set_condition(c, p, mask)
    x = x_T.clone()
    e.sample(x, use_graph=graph)
    torch.cuda.synchronize()
    return x.cpu().numpy()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_loop_properties(prec, weights, gold, diag):
    """graph == eager bitwise; the same seeds give the same bits, other seeds other latents; fuse_solver on == off (a stochastic
    table runs the stand-alone update); a begin without seeds is refused"""
    from ns2vc_amd import schedule as S
    from ns2vc_amd._lib import Ns2vcError
    from ns2vc_amd.engine import Engine
    x_T, c, p, mask = _golden_inputs(gold)
    B, _, T = x_T.shape
    e = Engine(precision=prec)
    try:
        e.load_state_dict(weights)
        e.prepare(B, T, p.shape[1])
        e.load_sampler("ddim", 30, S.linear_betas(1000, np.float64), eta=1.0)
        e.set_condition(c, p, mask)
        with pytest.raises(Ns2vcError, match="seeds"):
            e.sample(x_T.clone())
        s1, s2 = np.array([1, 2], np.uint64), np.array([1, 3], np.uint64)
        g = _engine_loop(e, x_T, c, p, mask, s1, True)
        g2 = _engine_loop(e, x_T, c, p, mask, s1, True)
        ea = _engine_loop(e, x_T, c, p, mask, s1, False)
        o = _engine_loop(e, x_T, c, p, mask, s2, True)
        e.set_option("fuse_solver", True)           # (drops the plan)
        e.prepare(B, T, p.shape[1])
        e.load_sampler("ddim", 30, S.linear_betas(1000, np.float64), eta=1.0)
        f = _engine_loop(e, x_T, c, p, mask, s1, True)
    finally:
        e.close()
    assert np.array_equal(g, ea) and np.array_equal(g, g2) and np.array_equal(g, f)
    assert np.array_equal(g[0], o[0])                     # item 0 kept its seed
    d = rel_l2(o[1], g[1])
    diag(f"ddim30 eta 1 {prec}: item 1 with another seed moves by {d:.2e}")
    assert d > 1e-2


def test_handoff_continues_the_noise_stream(weights, gold, diag):
    """fp32 -> fp32 handoff in mid-loop == one fp32 loop (the seeds travel); fp16 head + fp32 tail within the fp16 bar of it"""
    import torch
    from ns2vc_amd import schedule as S
    from ns2vc_amd.engine import Engine
    x_T, c, p, mask = _golden_inputs(gold)
    B, _, T = x_T.shape
    seeds = gold["g13.seeds"]
    engs = {}
    try:
        for name, prec in (("a", "fp32"), ("b", "fp32"), ("h", "fp16")):
            e = Engine(precision=prec)
            e.load_state_dict(weights)
            e.prepare(B, T, p.shape[1])
            e.load_sampler("ddpm", 1000, S.linear_betas(1000, np.float64))
            e.set_condition(c, p, mask)
            engs[name] = e
        whole = _engine_loop(engs["a"], x_T, c, p, mask, seeds)
        out = {}
        for head in ("a", "h"):
            engs[head].set_seeds(seeds)                   # the tail engine gets them from the handoff
            x = x_T.clone()
            engs[head].sample(x, tail=engs["b"], tail_steps=300)
            torch.cuda.synchronize()
            out[head] = x.cpu().numpy()
    finally:
        for e in engs.values():
            e.close()
    e32, e16 = rel_l2(out["a"], whole), rel_l2(out["h"], whole)
    diag(f"ddpm1000 handoff at 700: fp32 head {e32:.2e}, fp16 head {e16:.2e} vs the fp32 loop")
    assert e32 < 1e-6                 # measured 0: the same arithmetic on both fp32 engines
    assert e16 < FP16_TOL             # measured 1.3e-6: 300 fp32 steps of DDPM forget the fp16 head's rounding


def test_ragged_batch_items_equal_items_alone(weights, diag):
    """B=3 ragged, own seeds: item b on [0, L_b) == item b alone at T = L_b (fp32, 1e-5), exact zeros beyond"""
    import torch
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.weights import hash_normal
    lens, Lp = [188, 131, 37], 40
    T = max(lens)
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("st.c", (3, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("st.p", (1, Lp, 256))).expand(3, -1, -1).contiguous().to(dev)
    x_T = torch.zeros(3, 100, T, device=dev)
    for b, L in enumerate(lens):
        x_T[b, :, :L] = torch.from_numpy(hash_normal(f"st.x{b}", (100, L))).to(dev)
    seeds = np.array([5, 6, 7], np.uint64)
    den = Denoiser(weights, precision="fp32")
    for solver, steps, eta in (("ddim", 30, 1.0), ("ddpm", 1000, 0.0)):
        y = den.sample(c, p, None, x_T, solver=solver, steps=steps, eta=eta, seeds=seeds, lengths=lens).cpu().numpy()
        worst = 0.0
        for b, L in enumerate(lens):
            assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0
            one = den.sample(c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), None, x_T[b:b + 1, :, :L].contiguous(), solver=solver,
                             steps=steps, eta=eta, seeds=seeds[b:b + 1]).cpu().numpy()
            worst = max(worst, rel_l2(y[b, :, :L], one[0]))
        diag(f"ragged {solver}{steps} fp32: worst item vs alone {worst:.2e}")
        assert worst < 1e-5           # measured 1.7e-6 / 1.8e-6


def test_ragged_service_ddpm_per_segment(diag):
    """GroupedConverter(solver="ddpm", ragged=True): each segment == the same segment converted in a batch of its own"""
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
    lengths = [96, 130, 9]
    segs = [Segment(torch.from_numpy(hash_normal(f"sts.c{i}", (256, T))), torch.from_numpy(hash_normal("sts.r", (100, 40))), tag=i)
            for i, T in enumerate(lengths)]
    den = Denoiser(procedural_state_dict(seed=0), precision="fp32")
    out = GroupedConverter(pre, den, max_batch=4, solver="ddpm", ragged=True).convert(segs)
    single = GroupedConverter(pre, den, max_batch=1, solver="ddpm", ragged=True).convert(segs)    # every segment in a batch of its own
    errs = []
    for i in range(len(segs)):
        assert out[i].shape == (100, lengths[i]) and torch.isfinite(out[i]).all()
        errs.append(rel_l2(out[i].cpu().numpy(), single[i].cpu().numpy()))
    diag(f"ragged service ddpm1000 fp32, batch of 3 vs batches of 1: max {max(errs):.2e}")
    assert max(errs) < 1e-5           # measured 2.1e-6


def test_bench_shape_ddpm(weights, diag):
    """DDPM-1000 at B=32, T=938: fp16 (default tail) against the fp32 engine on the same seeds"""
    import torch
    from ns2vc_amd.pipeline import DEFAULT_TAIL_FP32, Denoiser
    from ns2vc_amd.weights import hash_normal
    B, T, Lp = 32, 938, 469
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal("stb.c", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("stb.p", (B, Lp, 256))).to(dev)
    mask = (torch.arange(Lp)[None, :] < torch.randint(100, Lp + 1, (B,), generator=torch.Generator().manual_seed(0))[:, None]).to(dev)
    x_T = torch.from_numpy(hash_normal("stb.x", (B, 100, T))).to(dev)
    seeds = np.arange(B, dtype=np.uint64) + np.uint64(1000)
    y32 = Denoiser(weights, precision="fp32").sample(c, p, mask, x_T, solver="ddpm", seeds=seeds).cpu().numpy()
    y16 = Denoiser(weights, precision="fp16").sample(c, p, mask, x_T, solver="ddpm", seeds=seeds).cpu().numpy()
    e, loc = rel_l2(y16, y32), local_errors(y16, y32)
    diag(f"bench shape ddpm1000 fp16 (tail {DEFAULT_TAIL_FP32['ddpm']}) vs fp32: {e:.2e} {fmt_local(loc)}")
    assert e < FP16_TOL
    assert loc["frame"] < FP16_LOCAL_TOL and loc["chan"] < FP16_LOCAL_TOL
