"""Length-aware attention (ns2vc_attn_args.q_lens / k_lens, engine option ``masked_attn``).

Kernel level: item b of a padded launch gives, on its valid rows, BIT FOR BIT what the dense kernel gives for that item alone at
Lq = Lk = L_b (the same tiles in the same order, the same clamp and -inf tail), exact zeros past its end, with the padded rows of q, k and v
holding NaN or Inf and `out` inside guard bands.  Engine level: with the option on a masked plan drops the self-attention key-bias row and both
`.sdpa.mask` launches of every transformer block and still gives every item as if alone.

Bounds: tol_attention (tests/util.py) and the constants of tests/test_ragged_gpu.py (TOL, FRAME_TOL, 2.5e-3 sampled, 2e-3 / 1e-6 for a flipped
option), imported, not restated."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard as G                                  # noqa: E402
from attn_launch import OUT_FILL, PREC_IDS, _launch, _lib, _ref_item, _rounded, _vals      # noqa: E402  (moved there unchanged: shared with test_attn_positions_gpu.py)
import test_ragged_gpu as RG                      # noqa: E402  (the existing constants and helpers: one statement of the bars)
from test_ragged_gpu import FRAME_TOL, TOL, _forward, _inputs, _sample      # noqa: E402,F401
from util import local_errors, rel_l2, tol_attention      # noqa: E402

pytestmark = pytest.mark.gpu

B0, H0, L0 = 7, 2, 200                             # two 128-query tiles, four 64-key / two 128-key tiles
LENS0 = [200, 129, 128, 127, 65, 64, 1]            # full; one past / at / one below a query-tile and 128-key-tile edge; one past / at a 64-key edge; one frame


def _poison(a, lens, bad):
    a = a.copy()
    for b, L in enumerate(lens):
        a[b, L:] = bad
    return a


@functools.lru_cache(maxsize=None)
def _self_data(hd):
    rng = np.random.default_rng(1000 + hd)
    D = H0 * hd
    return tuple(rng.standard_normal((B0, L0, D)).astype(np.float32) for _ in range(3))


@functools.lru_cache(maxsize=None)
def _self_ref(hd, prec):
    """fp64 attention of every item over its own keys, computed once per (head width, operand type) and shared by the cases"""
    q, k, v = (_rounded(t, prec) for t in _self_data(hd))
    return tuple(_ref_item(q[b, :L], k[b, :L], v[b, :L], None, H0, hd) for b, L in enumerate(LENS0))


SELF_CASES = [(prec, hd, keys, opt) for prec in (0, 1, 2) for hd in (16, 32, 48, 64)
              for keys in ((64, 128) if prec != 0 and hd <= 32 else (64,))        # 128-key tiles exist for the 16-bit types at head width 16 / 32
              for opt in ((1, 0) if prec != 0 else (0,))]                        # fp32 has no optimistic pass: the exact one is all there is


@pytest.mark.parametrize("prec,hd,keys,opt", SELF_CASES,
                         ids=[f"{PREC_IDS[p]}-hd{h}-keys{k}-{'optimistic' if o else 'exact'}" for p, h, k, o in SELF_CASES])
def test_self_attention_form(prec, hd, keys, opt, diag):
    q, k, v = _self_data(hd)
    ref = _self_ref(hd, prec)
    tol = tol_attention(prec)
    # the dense kernel on every item alone, Lq = Lk = L_b, same rows, key-tile width and pass
    alone = []
    for b, L in enumerate(LENS0):
        rc, bits, viol, _ = _launch(prec, hd, q[b:b + 1, :L], k[b:b + 1, :L], v[b:b + 1, :L], keys=keys, optimistic=opt)
        assert rc == 0 and not viol, (b, viol)
        alone.append(bits[0])
    worst = 0.0
    for fill in ("nan", "inf"):
        bad = np.nan if fill == "nan" else np.inf
        rc, bits, viol, _ = _launch(prec, hd, _poison(q, LENS0, bad), _poison(k, LENS0, bad), _poison(v, LENS0, bad), q_lens=LENS0, k_lens=LENS0,
                                    keys=keys, optimistic=opt, fill=fill)
        assert rc == 0, _lib()[1].ns2vc_last_error()
        assert not viol, viol
        out = _vals(bits, prec)
        for b, L in enumerate(LENS0):
            e = rel_l2(out[b, :L], ref[b])
            worst = max(worst, e)
            assert np.isfinite(out[b]).all(), (fill, b)
            assert e < tol, (fill, b, L, e)
            assert np.array_equal(bits[b, :L], alone[b]), (fill, b, L, int((bits[b, :L] != alone[b]).sum()))
            assert not bits[b, L:].any(), (fill, b, L)                           # exact zeros: every storage word 0
    diag(f"masked attention self form {PREC_IDS[prec]} hd {hd} keys {keys} {'optimistic' if opt else 'exact'}: worst item vs fp64 {worst:.2e} "
         f"(bar {tol:.1e}); bit-identical to the dense kernel on every item alone; zeros past the ends; guards intact")


CROSS_CASES = [(prec, hd, Lk) for prec in (0, 1, 2) for hd in (16, 32, 48, 64) for Lk in (40, 100)]


@pytest.mark.parametrize("prec,hd,Lk", CROSS_CASES, ids=[f"{PREC_IDS[p]}-hd{h}-Lk{k}" for p, h, k in CROSS_CASES])
def test_cross_attention_form(prec, hd, Lk, diag):
    """q_lens only: every key row is valid, a bias row switches a ragged tail of the prompt off"""
    rng = np.random.default_rng(2000 + hd + Lk)
    D = H0 * hd
    q = rng.standard_normal((B0, L0, D)).astype(np.float32)
    k = rng.standard_normal((B0, Lk, D)).astype(np.float32)
    v = rng.standard_normal((B0, Lk, D)).astype(np.float32)
    plen = [Lk - (b * (Lk - 3)) // B0 for b in range(B0)]                        # prompt lengths Lk down to a few keys
    bias = np.where(np.arange(Lk)[None, :] < np.array(plen)[:, None], 0.0, -10000.0).astype(np.float32)
    qr, kr, vr = (_rounded(t, prec) for t in (q, k, v))
    tol = tol_attention(prec)
    alone = []
    for b, L in enumerate(LENS0):
        rc, bits, viol, _ = _launch(prec, hd, q[b:b + 1, :L], k[b:b + 1], v[b:b + 1], bias=bias[b:b + 1])
        assert rc == 0 and not viol, (b, viol)
        alone.append(bits[0])
    worst = 0.0
    for fill in ("nan", "inf"):
        bad = np.nan if fill == "nan" else np.inf
        rc, bits, viol, _ = _launch(prec, hd, _poison(q, LENS0, bad), k, v, bias=bias, q_lens=LENS0, fill=fill)
        assert rc == 0, _lib()[1].ns2vc_last_error()
        assert not viol, viol
        out = _vals(bits, prec)
        for b, L in enumerate(LENS0):
            e = rel_l2(out[b, :L], _ref_item(qr[b, :L], kr[b], vr[b], bias[b].astype(np.float64), H0, hd))
            worst = max(worst, e)
            assert np.isfinite(out[b]).all() and e < tol, (fill, b, L, e)
            assert np.array_equal(bits[b, :L], alone[b]), (fill, b, L)
            assert not bits[b, L:].any(), (fill, b, L)
    diag(f"masked attention cross form {PREC_IDS[prec]} hd {hd} Lk {Lk}: worst item vs fp64 {worst:.2e} (bar {tol:.1e}); bit-identical to the dense "
         f"kernel on each item's first L_b rows")


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_optimistic_fallback_under_lengths(prec, diag):
    """the construction of test_attention_optimistic_pass_and_its_fallback (scores rising after the first key tile: q x 4, k x 3 x a ramp along the
    keys).  (a) in an item's valid rows: the optimistic pass is repeated, counted, and the result is the exact pass's; (b) only in rows past q_lens
    (as numbers, and as NaN): no workgroup repeats anything -- while the same tensors without the lengths do."""
    rng = np.random.default_rng(91)
    B, H, hd, Lq, Lk = 2, 8, 16, 200, 333
    D = H * hd
    v = rng.standard_normal((B, Lk, D)).astype(np.float32)
    ramp = np.linspace(0.1, 3.0, Lk, dtype=np.float32)[None, :, None]
    k = rng.standard_normal((B, Lk, D)).astype(np.float32) * 3.0 * ramp
    q = rng.standard_normal((B, Lq, D)).astype(np.float32)
    # ---- (a): item 1 has a query tile wholly past its end (rows 128..199 of 100 valid): it neither repeats nor counts
    ql, kl = [200, 100], [333, 300]
    qa = _poison(q * 4.0, ql, np.nan)
    ka, va = _poison(k, kl, np.nan), _poison(v, kl, np.nan)
    rc, b_opt, viol, nfb = _launch(prec, hd, qa, ka, va, H=H, q_lens=ql, k_lens=kl, count=True)
    assert rc == 0 and not viol, viol
    rc, b_ex, viol, nfb_ex = _launch(prec, hd, qa, ka, va, H=H, q_lens=ql, k_lens=kl, optimistic=0, count=True)
    assert rc == 0 and not viol, viol
    live = H * sum((L + 127) // 128 for L in ql)                                 # workgroups that hold a valid row
    diag(f"masked attention, rising scores in valid rows {PREC_IDS[prec]}: {nfb} of {live} live workgroups repeated the pass "
         f"({H * B * 2} launched); exact-only run counted {nfb_ex}; bitwise equal to the exact pass = {np.array_equal(b_opt, b_ex)}")
    assert nfb_ex == 0 and 0 < nfb <= live
    o_opt, o_ex = _vals(b_opt, prec), _vals(b_ex, prec)
    assert np.isfinite(o_opt).all() and np.isfinite(o_ex).all()
    qr, kr, vr = (_rounded(t, prec) for t in (q * 4.0, k, v))
    from util import eps16
    for b in range(B):
        ref = _ref_item(qr[b, :ql[b]], kr[b, :kl[b]], vr[b, :kl[b]], None, H, hd)
        assert rel_l2(o_opt[b, :ql[b]], ref) < 16 * eps16(prec) and rel_l2(o_ex[b, :ql[b]], ref) < 16 * eps16(prec)      # (the existing test's bar for this case)
        assert not b_opt[b, ql[b]:].any() and not b_ex[b, ql[b]:].any()
    if prec == 2:                                  # fp16: the check rejects the optimistic pass in every live workgroup (as in the dense test)
        assert nfb == live and np.array_equal(b_opt, b_ex)
    # ---- (b): ordinary scores in the valid rows, the rising ones only past q_lens, in tiles that also hold valid rows
    ql = [130, 100]
    qb = q * 0.25
    for b, L in enumerate(ql):
        qb[b, L:] = q[b, L:] * 4.0
    rc, _, viol, nfb_dense = _launch(prec, hd, qb, k, v, H=H, count=True)       # control: without lengths those rows do send their workgroups back
    assert rc == 0 and not viol and nfb_dense > 0, nfb_dense
    rc, bits, viol, nfb_num = _launch(prec, hd, qb, k, v, H=H, q_lens=ql, count=True)
    assert rc == 0 and not viol, viol
    rc, bits_nan, viol, nfb_nan = _launch(prec, hd, _poison(qb, ql, np.nan), k, v, H=H, q_lens=ql, count=True)
    assert rc == 0 and not viol, viol
    diag(f"masked attention, rising scores only past q_lens {PREC_IDS[prec]}: fallbacks {nfb_num} (numbers) / {nfb_nan} (NaN) with lengths, "
         f"{nfb_dense} without")
    assert nfb_num == 0 and nfb_nan == 0
    assert np.array_equal(bits, bits_nan) and np.isfinite(_vals(bits, prec)).all()


@pytest.mark.parametrize("prec", [0, 2], ids=["fp32", "fp16"])
def test_skipped_work_is_skipped(prec, diag):
    """every item one frame long inside 200: nothing of rows 1.. is read (they hold NaN), softmax over one key returns its value row"""
    hd = 16
    q, k, v = _self_data(hd)
    ones = [1] * B0
    rc, bits, viol, _ = _launch(prec, hd, _poison(q, ones, np.nan), _poison(k, ones, np.nan), _poison(v, ones, np.nan), q_lens=ones, k_lens=ones)
    assert rc == 0 and not viol, viol
    out = _vals(bits, prec)
    assert np.isfinite(out).all()
    e = rel_l2(out[:, 0], _rounded(v, prec)[:, 0])
    diag(f"masked attention, q_lens = k_lens = 1 of {L0} {PREC_IDS[prec]}: row 0 vs its value row {e:.2e}")
    assert e < tol_attention(prec)
    assert not bits[:, 1:].any()


def test_refusals(diag):
    """a count outside its range and a form without a masked instantiation are errors, and `out` keeps what it held"""
    hd, prec = 16, 2
    q, k, v = _self_data(hd)
    fill_bits = G.encode(np.full(1, OUT_FILL, np.float32), G.OP_KIND[prec])[0]
    cases = {"q_lens 0": dict(q_lens=[200, 0, 5, 5, 5, 5, 5], k_lens=LENS0), "k_lens 0": dict(q_lens=LENS0, k_lens=[0] + LENS0[1:]),
             "q_lens above Lq": dict(q_lens=[201] + LENS0[1:]), "k_lens above Lk": dict(k_lens=LENS0[:-1] + [201]),
             "pv_fp8 with lengths": dict(q_lens=LENS0, k_lens=LENS0, pv_fp8=1), "pv_fp8 with k_lens": dict(k_lens=LENS0, pv_fp8=1)}
    for name, kw in cases.items():
        rc, bits, viol, _ = _launch(prec, hd, q, k, v, **kw)
        msg = _lib()[1].ns2vc_last_error().decode()
        diag(f"masked attention refusal, {name}: status {rc} ({msg})")
        assert rc != 0, name
        assert not viol and np.all(bits == fill_bits), name
    rc, bits, viol, _ = _launch(0, hd, q, k, v, q_lens=LENS0, pv_fp8=1)         # (fp32 has no fp8 form at all)
    assert rc != 0 and np.all(bits == G.encode(np.full(1, OUT_FILL, np.float32), "f32")[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level (B <= 8, T <= 300)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


def _engine(prec, weights, fuse=True, attn=True):
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    e.set_option("masked_fuse", fuse)
    e.set_option("masked_attn", attn)
    return e


def _zero_tails(y, lens, T):
    for b, L in enumerate(lens):
        assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0, (b, L)


@pytest.mark.parametrize("fuse", [True, False], ids=["masked_fuse", "unfused"])
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_masked_attn_forward_equals_items_alone(prec, fuse, weights, diag):
    lens = [300, 263, 131, 129, 128, 127, 64, 9]
    T, Lp = 300, 40
    x, c, p, t = _inputs(len(lens), T, Lp, "ma1")
    for b, L in enumerate(lens):
        x[b, :, L:] = 7.0
        c[b, :, L:] = -3.0
    e = _engine(prec, weights, fuse)
    try:
        y = _forward(e, x, c, p, t, lens)
        assert np.isfinite(y).all()
        _zero_tails(y, lens, T)
        worst = (0.0, 0.0)
        for b, L in enumerate(lens):
            ref = _forward(e, x[b:b + 1, :, :L].contiguous(), c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), t[b:b + 1].contiguous())
            m = local_errors(y[b:b + 1, :, :L], ref)
            worst = (max(worst[0], m["item"]), max(worst[1], m["frame"]))
            diag(f"masked_attn forward {prec} masked_fuse={int(fuse)} L={L}: item {m['item']:.2e} frame {m['frame']:.2e} chan {m['chan']:.2e}")
            assert m["item"] < TOL[prec], (L, m)
            assert m["frame"] < FRAME_TOL[prec] and m["chan"] < FRAME_TOL[prec], (L, m)
        diag(f"masked_attn forward {prec} masked_fuse={int(fuse)}: worst item {worst[0]:.2e} (bar {TOL[prec]:.0e}), worst frame {worst[1]:.2e}")
    finally:
        e.close()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_masked_attn_on_vs_off(prec, weights, diag):
    import torch
    lens = [300, 131, 66, 64, 33, 9]
    B, T, Lp = len(lens), 300, 40
    x, c, p, t = _inputs(B, T, Lp, "rg5")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(5)).to(c.device)
    res = {}
    for attn in (False, True):
        e = _engine(prec, weights, True, attn)
        try:
            res[attn] = (_forward(e, x, c, p, t, lens), _sample(e, c, p, xT, lens, True), _sample(e, c, p, xT, lens, False))
        finally:
            e.close()
    e1, eg, ee = (rel_l2(res[True][i], res[False][i]) for i in range(3))
    gve = rel_l2(res[True][1], res[True][2])
    same = [bool(np.array_equal(res[True][i], res[False][i])) for i in range(3)]
    diag(f"masked_attn on vs off under lengths {prec}: forward {e1:.2e}, sampled graph {eg:.2e} eager {ee:.2e}; graph vs eager {gve:.2e}; "
         f"bit-identical (forward, graph, eager) = {same}")
    assert e1 < 2e-3 and eg < 2e-3 and ee < 2e-3
    assert gve < 1e-6
    if prec == "fp32":
        assert e1 < TOL["fp32"]
    for y in res[True]:
        _zero_tails(y, lens, T)


def _names(e):
    return [o[0] for o in e.op_info(0)]


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_masked_attn_launch_list(prec, weights, diag):
    """with the option on, a masked plan (fused or not) is the same plan without its `.sdpa.mask` launches, name for name and in order"""
    B, T, Lp = 4, 300, 40
    lens = [300, 200, 131, 70]
    got = {}
    e = _engine(prec, weights, True, False)
    try:
        e.prepare(B, T, Lp)
        dense = _names(e)
        for fuse in (True, False):
            for attn in (False, True):
                e.set_option("masked_fuse", fuse)
                e.set_option("masked_attn", attn)
                e.prepare(B, T, Lp)
                assert _names(e) == dense                              # dense plans ignore both options
                e.set_lengths(lens)
                got[(fuse, attn)] = _names(e)
                e.set_lengths(None)
                assert _names(e) == dense
    finally:
        e.close()
    for fuse in (True, False):
        off, on = got[(fuse, False)], got[(fuse, True)]
        sweepers = [n for n in off if n.endswith(".sdpa.mask")]
        blocks = len([n for n in off if n.endswith(".attn1.sdpa")])
        assert blocks > 0 and len(sweepers) == 2 * blocks == len([n for n in off if n.endswith(".sdpa")])
        assert on == [n for n in off if not n.endswith(".sdpa.mask")], [(a, b) for a, b in zip(on, off) if a != b][:6]
        diag(f"launches {prec} masked_fuse={int(fuse)}: {len(off)} -> {len(on)} with masked_attn ({len(sweepers)} .sdpa.mask launches gone); dense {len(dense)}")
    assert got[(True, False)] != got[(False, False)]


def test_masked_attn_graph_captured_under_other_lengths(weights, diag):
    import torch
    B, T, Lp = 4, 256, 40
    _, c, p, _ = _inputs(B, T, Lp, "rg4")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(3)).to(c.device)
    A, Bl = [256, 200, 100, 9], [17, 256, 255, 64]
    e = _engine("fp16", weights)
    try:
        e.prepare(B, T, Lp)
        e.load_sampler("unipc", 10)
        e.set_lengths(None)
        e.set_condition(c, p, None)
        xd0 = xT.clone()
        e.sample(xd0, use_graph=True)
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
        e.set_lengths(None)                   # dense again: bit for bit what it was
        e.set_condition(c, p, None)
        xd1 = xT.clone()
        e.sample(xd1, use_graph=True)
        torch.cuda.synchronize()
    finally:
        e.close()
    xg, xe = xg.cpu().numpy(), xe.cpu().numpy()
    assert np.isfinite(xg).all()
    assert np.array_equal(xg, xe)
    assert np.array_equal(xd0.cpu().numpy(), xd1.cpu().numpy())
    _zero_tails(xg, Bl, T)


def test_masked_attn_sampled_padded_batch_equals_items_alone(weights, diag):
    import torch
    from ns2vc_amd.pipeline import Denoiser
    lens = [300, 211, 97, 64, 9]
    T, Lp = max(lens), 40
    _, c, p, _ = _inputs(len(lens), T, Lp, "rg3")
    noise = torch.zeros(len(lens), 100, T, device=c.device)
    for b, L in enumerate(lens):
        noise[b, :, :L] = torch.randn((100, L), generator=torch.Generator().manual_seed(b)).to(c.device)
    off = Denoiser(weights, precision="fp16", masked_fuse=True)
    off.sample(c, p, None, noise, solver="unipc", steps=20, use_graph=True, lengths=lens)
    rate_off = off.attn_fallback_rate_seen
    den = Denoiser(weights, precision="fp16", masked_fuse=True, masked_attn=True)
    out = den.sample(c, p, None, noise, solver="unipc", steps=20, use_graph=True, lengths=lens).cpu().numpy()
    rate_on = den.attn_fallback_rate_seen
    assert not den.serving_fp32 and not den._ln_switched
    assert rate_on is not None and rate_off is not None and rate_on <= rate_off, (rate_on, rate_off)
    _zero_tails(out, lens, T)
    worst = 0.0
    for b, L in enumerate(lens):
        one = den.sample(c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), None, noise[b:b + 1, :, :L].contiguous(), solver="unipc", steps=20,
                         use_graph=True).cpu().numpy()
        worst = max(worst, rel_l2(out[b, :, :L], one[0]))
    diag(f"masked_attn ragged sampling unipc-20 fp16: worst item vs alone {worst:.2e} (bar 2.5e-3); attention fallback rate {rate_on} (option off: {rate_off})")
    assert not den.serving_fp32 and not den._ln_switched
    assert worst < 2.5e-3
