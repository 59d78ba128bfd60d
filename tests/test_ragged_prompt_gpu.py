"""Per-item prompt lengths on the MI355X (ns2vc_unet_set_prompt_lengths): item b of a batch whose prompts are padded to one Lp gives what
the engine gives for that item alone with a prompt of P_b frames and no mask (to the precision's rounding), and nothing a padded prompt row
holds reaches any result -- forward (bias path and k_lens path), both axes ragged, the captured sampling loop, the errors, the service.

Shapes: B = 4, T = 128 (levels 128 / 64 / 32 / 16: the fused feed-forward and the short-level fallbacks both run), Lp = 130 with
P = (130, 65, 64, 1): the full prompt, one key past a 64-key tile edge, exactly the edge, a single key.  Every padded prompt row is NaN.

Gates (all taken from the existing tests, none from what this code gives):
  fp32: tests/test_engine_gpu.py FP32_TOL (rel-L2 per item) and FP32_LOCAL_TOL = 4 x FP32_TOL (per frame / channel, util.local_errors);
  fp16 / bf16 item == alone: the bars of test_full_size_batch_independence / the seam cases there -- 1.5e-3 / BF16_TOL per item (two 16-bit
    runs that round differently settle at sqrt(2) x the activation rounding noise apart), LOCAL_TOL per frame;
  fp16 against the fp32 engine: the 1e-3 parity bar (PARITY_TOL).  That bar is the project's gate for fp16, its default 16-bit precision; bf16
    sits at 6.5e-3 from fp32 by its number format (include/ns2vc_hip.h) and is held to BF16_TOL, the bound tests/test_engine_gpu.py keeps for it."""
import json
import os

import numpy as np
import pytest

from util import local_errors, procedural_params, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL, FP32_LOCAL_TOL = 1e-5, 4e-5
PARITY_TOL, BF16_TOL = 1e-3, 1e-2
ALONE_TOL = {"fp32": FP32_TOL, "fp16": 1.5e-3, "bf16": BF16_TOL}
FRAME_TOL = {"fp32": FP32_LOCAL_TOL, "fp16": 3.2e-3, "bf16": 2.3e-2}
CHAN_TOL = {"fp32": FP32_LOCAL_TOL, "fp16": 3.1e-3, "bf16": 2.2e-2}
VS_FP32_TOL = {"fp16": PARITY_TOL, "bf16": BF16_TOL}
B, T, LP = 4, 128, 130
PLENS = [130, 65, 64, 1]
LENS = [128, 97, 64, 1]
MASKED = ["masked_fuse", "masked_attn", "masked_rows", "masked_ffn", "masked_geglu"]


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


@pytest.fixture(scope="module")
def data():
    """x, content, t and the prompts: `p` clean (every row a prompt row), `pn` the same with the rows past P_b NaN"""
    import torch
    from ns2vc_amd.weights import hash_normal
    dev = torch.device("cuda", 0)
    x = torch.from_numpy(hash_normal("rp.x", (B, 100, T))).to(dev)
    c = torch.from_numpy(hash_normal("rp.c", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal("rp.p", (B, LP, 256))).to(dev)
    t = torch.linspace(50.0, 900.0, B, device=dev)
    pn = p.clone()
    for b, P in enumerate(PLENS):
        pn[b, P:] = float("nan")
    return {"x": x, "c": c, "p": p, "pn": pn, "t": t}


def _engine(weights, prec, options=(), debug=False):
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    for o in options:
        e.set_option(o, True)
    e.set_debug(debug)
    return e


def _forward(e, x, c, p, t, lengths=None, plens=None, mask=None):
    import torch
    Bq, _, Tq = x.shape
    if e.shape != (Bq, Tq, p.shape[1]):
        e.prepare(Bq, Tq, p.shape[1])
    e.set_lengths(lengths)
    e.set_prompt_lengths(plens)
    e.set_condition(c, p, mask)
    out = torch.empty_like(x)
    e.forward(x, t, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


_ALONE = {}


def _alone(weights, data, prec):
    """item b alone with its own prompt of P_b rows, no mask, full T: (forward, aug tap row) per item, computed once per precision"""
    if prec not in _ALONE:
        e = _engine(weights, prec, debug=True)
        try:
            res = []
            for b, P in enumerate(PLENS):
                y = _forward(e, data["x"][b:b + 1].contiguous(), data["c"][b:b + 1].contiguous(), data["p"][b:b + 1, :P].contiguous(),
                             data["t"][b:b + 1].contiguous())
                res.append((y, e.taps()["aug"].copy()))
            _ALONE[prec] = res
        finally:
            e.close()
    return _ALONE[prec]


def _check_items(y, alone, prec, diag, what):
    worst = {"item": 0.0, "frame": 0.0, "chan": 0.0}
    for b in range(B):
        assert np.isfinite(y[b]).all(), (what, b)
        m = local_errors(y[b:b + 1], alone[b][0])
        diag(f"ragged prompts {what} {prec} item {b} (P = {PLENS[b]}) vs alone: item {m['item']:.2e} frame {m['frame']:.2e} chan {m['chan']:.2e}")
        for k in worst:
            worst[k] = max(worst[k], m[k])
    assert worst["item"] < ALONE_TOL[prec], (what, worst)
    assert worst["frame"] < FRAME_TOL[prec] and worst["chan"] < CHAN_TOL[prec], (what, worst)


@pytest.mark.parametrize("masked_attn", [False, True])
def test_padded_prompts_equal_items_alone_fp32(masked_attn, weights, data, diag):
    """fp32 engine, bias path (masked_attn off) and k_lens path (on): the add_embedding row of every item has the bits of the alone run, the forward
    is inside the fp32 gate per item and per frame, one item also against the CPU oracle at its own Lp; and the gap this closes -- the same
    batch under a prompt_mask alone (finite padding) is further from the alone run than the gate"""
    import torch
    from ns2vc_amd.spec import UNetConfig
    from oracle import unet_ref
    alone = _alone(weights, data, "fp32")
    what = "k_lens" if masked_attn else "bias"
    e = _engine(weights, "fp32", ["masked_attn"] if masked_attn else [], debug=True)
    try:
        y = _forward(e, data["x"], data["c"], data["pn"], data["t"], plens=PLENS)
        aug = e.taps()["aug"].copy()
        assert "cond.prompt.mask" in [n for n, _, _, _ in e.op_info(1)]
        for b in range(B):
            assert np.array_equal(aug[b], alone[b][1][0]), (what, b, float(np.abs(aug[b] - alone[b][1][0]).max()))
        _check_items(y, alone, "fp32", diag, what)
        b = 1
        P = {k: torch.from_numpy(v) for k, v in weights.items()}
        ro = unet_ref.denoiser(P, UNetConfig(), data["x"][b:b + 1].cpu(), data["c"][b:b + 1].cpu(), data["p"][b:b + 1, :PLENS[b]].cpu(), None,
                               data["t"][b:b + 1].cpu()).numpy()
        mo = local_errors(y[b:b + 1], ro)
        diag(f"ragged prompts {what} fp32 item {b} vs oracle at Lp = {PLENS[b]}: item {mo['item']:.2e} frame {mo['frame']:.2e}")
        assert mo["item"] < FP32_TOL and mo["frame"] < FP32_LOCAL_TOL and mo["chan"] < FP32_LOCAL_TOL, mo
        if not masked_attn:
            # for the record: a mask keeps the padding out of cross-attention only -- both attention poolings still see it
            mask = (torch.arange(LP, device=data["p"].device)[None, :] < torch.tensor(PLENS, device=data["p"].device)[:, None]).to(torch.uint8).contiguous()
            pz = torch.nan_to_num(data["pn"], nan=0.0)
            ym = _forward(e, data["x"], data["c"], pz, data["t"], mask=mask)
            gaps = [rel_l2(ym[b:b + 1], alone[b][0]) for b in range(B)]
            diag("ragged prompts: prompt_mask alone (zero padding) vs alone, fp32: " + " ".join(f"{g:.2e}" for g in gaps))
            assert gaps[0] < FP32_TOL                      # (the full prompt has no padding)
            assert min(gaps[1:]) > FP32_TOL
    finally:
        e.close()


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_padded_prompts_equal_items_alone_16bit(prec, weights, data, diag):
    alone = _alone(weights, data, prec)
    e32 = _engine(weights, "fp32")
    try:
        y32 = _forward(e32, data["x"], data["c"], data["pn"], data["t"], plens=PLENS)
    finally:
        e32.close()
    for masked_attn in (False, True):
        what = "k_lens" if masked_attn else "bias"
        e = _engine(weights, prec, ["masked_attn"] if masked_attn else [], debug=True)
        try:
            y = _forward(e, data["x"], data["c"], data["pn"], data["t"], plens=PLENS)
            aug = e.taps()["aug"].copy()
        finally:
            e.close()
        for b in range(B):
            # the same first clause as in fp32: cond.pool.cast and cond.pool.qkv run in the engine's precision on B (Lp + 1) rows here and on
            # P_b + 1 rows alone, and the add_embedding row must still have the alone run's bits
            diag(f"ragged prompts {what} {prec} item {b}: aug row vs alone {rel_l2(aug[b], alone[b][1][0]):.2e}")
            assert np.array_equal(aug[b], alone[b][1][0]), (what, prec, b, float(np.abs(aug[b] - alone[b][1][0]).max()))
        _check_items(y, alone, prec, diag, what)
        ev = max(rel_l2(y[b], y32[b]) for b in range(B))
        diag(f"ragged prompts {what} {prec} vs the fp32 engine on the same padded batch: batch {rel_l2(y, y32):.2e} worst item {ev:.2e}")
        assert rel_l2(y, y32) < VS_FP32_TOL[prec]          # (relative L2 over the batch: the parity bar's own measure)
        assert ev < VS_FP32_TOL[prec]                      # ... and the worst single item


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_both_axes_ragged(prec, masked, weights, data, diag):
    """latent lengths (128, 97, 64, 1) together with the prompt lengths, the five masked_* options all off / all on: item == the item alone at
    its own T and Lp, exact zeros past L_b.
    The engine needs T >= 8, so the one-frame item is held (a) against the CPU oracle alone: in fp32 at the item bar FP32_TOL with the options
    off, as tests/test_ragged_gpu.py holds it (measured 1.6e-6); in 16 bits at twice the parity bar, as there.  With the options on the fp32 bar is
    the per-frame gate FP32_LOCAL_TOL: a one-frame item IS one frame -- nothing averages over T -- and at T = 128 masked_fuse takes the GroupNorm
    sums of levels 0 / 1 from the int64 fixed-point epilogue statistics, whose quantum does not average out over a single frame (measured 1.1e-5,
    and the same 1.1e-5 for this latent batch with latent lengths alone and a dense one-row prompt, no prompt lengths involved).  And (b) against the same engine on the
    same latent batch with the item's own prompt rows given densely (Lp = P_b, no prompt lengths), at the item == alone bar: the prompt axis
    by itself."""
    import torch
    from ns2vc_amd.spec import UNetConfig
    from oracle import unet_ref
    x, c = data["x"].clone(), data["c"].clone()
    for b, L in enumerate(LENS):           # the caller's latent padding is arbitrary too
        x[b, :, L:] = 7.0
        c[b, :, L:] = -3.0
    e = _engine(weights, prec, MASKED if masked else [])
    what = "both axes, masked_* " + ("on" if masked else "off")
    try:
        y = _forward(e, x, c, data["pn"], data["t"], lengths=LENS, plens=PLENS)
        for b, (L, P) in enumerate(zip(LENS, PLENS)):
            assert np.isfinite(y[b]).all(), b
            assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0, b
            xb, cb, pb, tb = x[b:b + 1, :, :L].contiguous(), c[b:b + 1, :, :L].contiguous(), data["p"][b:b + 1, :P].contiguous(), data["t"][b:b + 1].contiguous()
            if L >= 8:
                ref, tol = _forward(e, xb, cb, pb, tb), ALONE_TOL[prec]
            else:
                Pw = {k: torch.from_numpy(v) for k, v in weights.items()}
                ref = unet_ref.denoiser(Pw, UNetConfig(), xb.cpu(), cb.cpu(), pb.cpu(), None, tb.cpu()).numpy()
                tol = (FP32_LOCAL_TOL if masked else FP32_TOL) if prec == "fp32" else 2 * PARITY_TOL
                yd = _forward(e, x, c, pb.expand(B, -1, -1).contiguous(), data["t"], lengths=LENS)
                md = local_errors(y[b:b + 1, :, :L], yd[b:b + 1, :, :L])
                diag(f"ragged prompts {what} {prec} item {b} (L = {L}, P = {P}) vs latent lengths alone with its prompt dense: item {md['item']:.2e}")
                assert md["item"] < ALONE_TOL[prec], (b, md)
            m = local_errors(y[b:b + 1, :, :L], ref)
            diag(f"ragged prompts {what} {prec} item {b} (L = {L}, P = {P}): item {m['item']:.2e} frame {m['frame']:.2e} chan {m['chan']:.2e}")
            assert m["item"] < tol, (b, m)
            if L >= 8:
                assert m["frame"] < FRAME_TOL[prec] and m["chan"] < CHAN_TOL[prec], (b, m)
    finally:
        e.close()


def test_in_kernel_cross_attention_reads_the_bias_row(weights, data, diag):
    """option fuse_xattn: the cross-attention of the dim-128 / 256 blocks runs inside the fused feed-forward kernel, which has no k_lens -- under
    prompt lengths it reads the bias row (att_bias) whether masked_attn is on or not.  Item == the item alone under the same option, fp16 bars."""
    e = _engine(weights, "fp16", ["fuse_xattn", "masked_attn"])
    try:
        y = _forward(e, data["x"], data["c"], data["pn"], data["t"], plens=PLENS)
        assert any("attn2.sdpa+to_out" in n for n, _, _, _ in e.op_info(0))          # the in-kernel form is in the plan
        alone = []
        for b, P in enumerate(PLENS):
            alone.append((_forward(e, data["x"][b:b + 1].contiguous(), data["c"][b:b + 1].contiguous(), data["p"][b:b + 1, :P].contiguous(),
                                   data["t"][b:b + 1].contiguous()), None))
        _check_items(y, alone, "fp16", diag, "fuse_xattn")
    finally:
        e.close()


def _loop(e, c, p, xT, plens, graph):
    import torch
    e.set_prompt_lengths(plens)
    e.set_condition(c, p, None)
    x = xT.clone()
    e.sample(x, use_graph=graph)
    torch.cuda.synchronize()
    return x.cpu().numpy()


@pytest.mark.parametrize("masked_attn", [False, True])
def test_captured_loop_under_changing_prompt_lengths(masked_attn, weights, data, diag):
    """6-step UniPC, captured: new prompt lengths for the same shape replay the graph that was captured under the old ones (no new capture) and
    give, bit for bit, what a fresh engine gives under them, captured or eager; set_prompt_lengths(None) restores the dense engine bit for bit"""
    import torch
    c, p, pn = data["c"], data["p"], data["pn"]
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(11)).to(c.device)
    first = [LP, 1, 129, 64]
    pn1 = p.clone()
    for b, P in enumerate(first):
        pn1[b, P:] = float("nan")
    opts = ["masked_attn"] if masked_attn else []
    e = _engine(weights, "fp16", opts)
    f = _engine(weights, "fp16", opts)
    d = _engine(weights, "fp16", opts)
    try:
        for g in (e, f, d):
            g.prepare(B, T, LP)
            g.load_sampler("unipc", 6)
        _loop(e, c, pn1, xT, first, True)                # captured under `first`
        n0 = e.graph_captures()
        assert n0 == 1
        xg = _loop(e, c, pn, xT, PLENS, True)            # the same graph under PLENS
        assert e.graph_captures() == n0
        xe = _loop(e, c, pn, xT, PLENS, False)
        xf = _loop(f, c, pn, xT, PLENS, True)            # an engine that only ever saw PLENS
        assert np.isfinite(xg).all()
        assert np.array_equal(xg, xe) and np.array_equal(xg, xf)
        xr = _loop(e, c, pn, xT, PLENS, True)            # a repeat of the current lengths
        assert np.array_equal(xr, xg) and e.graph_captures() == n0
        x0 = _loop(e, c, p, xT, None, True)              # dense again: a plan change, so one more capture -- and the dense engine's bits
        xd = _loop(d, c, p, xT, None, True)
        assert e.prompt_lengths is None and np.array_equal(x0, xd)
        assert e.graph_captures() == n0 + 1 and d.graph_captures() == 1
        diag(f"ragged prompts captured loop (masked_attn {int(masked_attn)}): padded vs dense prompts differ by {rel_l2(xg, xd):.2e}")
        assert rel_l2(xg, xd) > 1e-2                     # (the lengths did something)
    finally:
        for g in (e, f, d):
            g.close()


def test_bad_prompt_lengths_are_refused_and_change_nothing(weights, data):
    from ns2vc_amd import _lib
    e = _engine(weights, "fp16")
    try:
        y0 = _forward(e, data["x"], data["c"], data["pn"], data["t"], plens=PLENS)
        for bad in ([0, 1, 1, 1], [LP + 1, 1, 1, 1], [LP, 65, 64, -3]):
            with pytest.raises(_lib.Ns2vcError):
                e.set_prompt_lengths(bad)
        for bad in ([LP, 65, 64], [LP, 65, 64, 1, 1]):
            with pytest.raises(ValueError):
                e.set_prompt_lengths(bad)
        assert list(e.prompt_lengths) == PLENS
        import torch
        e.set_condition(data["c"], data["pn"], None)      # the lengths in force are still PLENS: the NaN rows stay out
        out = torch.empty_like(data["x"])
        e.forward(data["x"], data["t"], out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), y0)
        e.prepare(B, T, LP)                                # a new prepare is dense again
        assert e.prompt_lengths is None
    finally:
        e.close()


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("fp16", 2e-3)])
def test_service_with_three_reference_clips(precision, tol, diag):
    """GroupedConverter(ragged=True, ragged_prompts=True): six segments, three reference clips of different lengths, one batch; every result is
    what the segment's own conversion gives (the default converter at max_batch = 1), inside the bars tests/test_service_gpu.py holds
    grouped == per-segment to"""
    import torch
    from ns2vc_amd.frontend import PreModel
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import GroupedConverter, Segment
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    cfg = {"phoneme_encoder": {"in_channels": 256, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2},
           "prompt_encoder": {"in_channels": 100, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2}}
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "pre_model_state_keys.json")))
    pre = PreModel(cfg).eval()
    pre.load_state_dict(procedural_params(keys["keys"], "pre"), strict=True)
    pre = pre.to(torch.device("cuda", 0))
    lengths, clip_lens = [96, 130, 97, 64, 131, 80], [40, 65, 13]
    clips = [torch.from_numpy(hash_normal(f"rps.r{k}", (100, L))) for k, L in enumerate(clip_lens)]
    segs = [Segment(torch.from_numpy(hash_normal(f"rps.c{i}", (256, Tq))), clips[i % 3], tag=i) for i, Tq in enumerate(lengths)]
    den = Denoiser(procedural_state_dict(seed=0), precision=precision)
    rag = GroupedConverter(pre, den, max_batch=8, solver="unipc", steps=6, ragged=True, ragged_prompts=True)
    assert rag.plan(segs) == [[4, 1, 2, 0, 5, 3]]
    assert len(GroupedConverter(pre, den, max_batch=8, solver="unipc", steps=6, ragged=True).plan(segs)) == 3
    out = rag.convert(segs)
    one = GroupedConverter(pre, den, max_batch=1, solver="unipc", steps=6).convert(segs)
    errs = []
    for i, (a, b) in enumerate(zip(out, one)):
        assert a.shape == (100, lengths[i]) and torch.isfinite(a).all()
        errs.append(rel_l2(a.cpu().numpy(), b.cpu().numpy()))
    diag(f"ragged-prompt service ({precision}) vs per-segment runs: " + " ".join(f"{v:.2e}" for v in errs))
    assert max(errs) < tol
