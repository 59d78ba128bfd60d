"""Length-masked fused feed-forward (ns2vc_ffn_args.lens, engine option ``masked_ffn``).

Kernel level: item b of a padded launch gives, on its valid rows, BIT FOR BIT what the dense kernel gives for that item alone at T = M = L_b (a lane
owns one token, so a token's arithmetic does not depend on its place in a block), exact zeros past its end in both outputs, with the padded rows
of every input holding NaN or Inf and both outputs pre-filled inside guard bands; ln_health is the maximum of the alone launches' read-outs; the
GroupNorm statistics of the result do not depend on what the padded rows hold and agree with the fp64 sums over the valid rows of the launch's own
fp32 result.  Engine level: with the option on, a masked plan keeps the pre-stage launch of every dim-128 / 256 transformer block and still gives
every item as if alone.

Bounds: TOL_STATS (tests/util.py), the fixed-point half units of tests/epilogue_ref.py, and the constants of tests/test_ragged_gpu.py (TOL,
FRAME_TOL; 2.5e-3 sampled, 2e-3 / 1e-6 for a flipped option as test_every_plan_option_under_lengths states them) -- nothing of this file's own;
bf16 takes the factor tests/test_masked_rows_gpu.py states and derives (`_bar`)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard as G                                  # noqa: E402
from epilogue_ref import HALF_Q, SQ_SCALE, SUM_SCALE                                # noqa: E402
from test_masked_rows_gpu import B0, LENS0, OUT_FILL, PREC_IDS, T0, _bar, _dev, _item, _lib, _rounded, _zero_tails      # noqa: E402
from test_ragged_fused_gpu import _block_of, _names, _poison_rows, _stats_ref      # noqa: E402
from test_ragged_gpu import FRAME_TOL, TOL, _forward, _inputs, _sample            # noqa: E402
from util import TOL_STATS, local_errors, rel_l2                                  # noqa: E402

pytestmark = pytest.mark.gpu

M0 = B0 * T0                                       # 780 rows: 13 blocks of 64 tokens, the last one 12 rows long; rows 704 .. 767 wholly padded
FFN_NAME = ".ffn[attn2.to_out+geglu+ff.out+proj_out]"


@functools.lru_cache(maxsize=None)
def _weights(dim, prec, pre):
    """host matrices with the engine's pack-time folds, as test_ffn_fused builds them (LayerNorm gamma / beta into W1 / b1, [Wpo W2 | Wpo], value |
    gate row interleave), and the packed device stream / constants: built once per (dim, operand type, form) and shared by the cases"""
    L, lib = _lib()
    rng = np.random.default_rng(8100 + dim)
    d = dim
    Wo, bo = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), (0.3 * rng.standard_normal(d)).astype(np.float32)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(d)), 0.2 * rng.standard_normal(d)
    W1, b1 = rng.standard_normal((8 * d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(8 * d)
    W2, b2 = rng.standard_normal((d, 4 * d)) / np.sqrt(4 * d), 0.3 * rng.standard_normal(d)
    Wpo, bpo = rng.standard_normal((d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(d)
    W1f, b1f = W1 * gamma[None, :], b1 + W1 @ beta
    order = np.concatenate([np.concatenate([np.arange(32 * g, 32 * g + 32), 4 * d + np.arange(32 * g, 32 * g + 32)]) for g in range(4 * d // 32)])
    W1p, b1p = np.ascontiguousarray(W1f[order].astype(np.float32)), b1f[order].astype(np.float32)
    w2f = np.ascontiguousarray(np.concatenate([Wpo @ W2, Wpo], axis=1).astype(np.float32))
    bias2 = (Wpo @ b2 + bpo).astype(np.float32)
    consts = np.stack([_rounded(W1p, prec).sum(1), b1p.astype(np.float64)], axis=1).astype(np.float32)
    stream = C.c_void_p()
    if pre:
        L.check(lib.ns2vc_pack_ffn_pre(W1p.ctypes.data, w2f.ctypes.data, np.ascontiguousarray(Wo).ctypes.data, d, prec, C.byref(stream)), "pack_ffn_pre")
    else:
        L.check(lib.ns2vc_pack_ffn(W1p.ctypes.data, w2f.ctypes.data, d, prec, C.byref(stream)), "pack_ffn")
    return dict(stream=stream, d_c=_dev(consts), d_b2=_dev(bias2), d_bo=_dev(bo))


@functools.lru_cache(maxsize=None)
def _rows(dim):
    """o (attention rows), y (rows with a common offset: pre_res of the pre-stage form, the raw rows of the plain form), x (block residual) and the
    LayerNorm-by-linearity statistics of y as a producer GEMM's `rowstats` leaves them"""
    rng = np.random.default_rng(400 + dim)
    o = rng.standard_normal((M0, dim)).astype(np.float32)
    y = (rng.standard_normal((M0, dim)) + 1.5 * rng.standard_normal((M0, 1))).astype(np.float32)
    x = rng.standard_normal((M0, dim)).astype(np.float32)
    ys = y.astype(np.float64).reshape(M0, dim // 64, 64)
    st = np.stack([ys.sum(2), (ys ** 2).sum(2)], axis=-1).astype(np.float32).reshape(M0, dim // 64 * 2)
    return dict(o=o, y=y, x=x, st=st)


def _launch(prec, dim, pre, B, T, rows, *, lens=None, fill="nan", att=False, M=None):
    """one ns2vc_k_ffn launch on guarded tensors -> (status, out_f32 words (M, dim), out_op words (M, dim), int64 stats (B, dim / 16, 2), guard
    violations, ln_health).  rows: dict(o, y, x, st) of (B * T)-row arrays (NaN / Inf allowed); both outputs hold OUT_FILL before the launch."""
    L, lib = _lib()
    w = _weights(dim, prec, pre)
    bk = G.DeviceBackend()
    kind, d, Mr = G.OP_KIND[prec], dim, B * T
    gs = {}
    if pre:
        gs["o"] = G.Guarded(bk, Mr, d, kind, data=rows["o"], fill=fill, name="pre_a")
        gs["yp"] = G.Guarded(bk, Mr, d, "f32", data=rows["y"], fill=fill, name="pre_res")
    else:
        gs["yn"] = G.Guarded(bk, Mr, d, kind, data=rows["y"], fill=fill, name="yn")
        gs["st"] = G.Guarded(bk, Mr, d // 64 * 2, "f32", data=rows["st"], fill=fill, name="ln_stats")
    gs["x"] = G.Guarded(bk, Mr, d, "f32", data=rows["x"], fill=fill, name="res")
    gs["of"] = G.Guarded(bk, Mr, d, "f32", data=np.full((Mr, d), OUT_FILL, np.float32), fill=fill, name="out_f32")
    gs["oo"] = G.Guarded(bk, Mr, d, kind, data=np.full((Mr, d), OUT_FILL, np.float32), fill=fill, name="out_op")
    gs["gs"] = G.Guarded(bk, B, d // 16 * 2, "i64", data=np.zeros((B, d // 16 * 2), np.int64), fill=fill, name="stats")
    d_health = _dev(np.zeros(16, dtype=np.uint32), np.uint32)
    d_lens = _dev(lens, np.int32) if lens is not None else None
    f = L.FfnArgs()
    f.ln_eps = 1e-5
    f.wstream = w["stream"].value; f.consts = w["d_c"].ptr; f.bias2 = w["d_b2"].ptr
    f.res = gs["x"].ptr; f.ldres = d
    f.out_f32 = gs["of"].ptr; f.ldo_f32 = d; f.out_op = gs["oo"].ptr; f.ldo_op = d
    f.stats = gs["gs"].ptr
    f.B, f.T, f.M, f.dim = B, T, (Mr if M is None else M), d
    f.ln_health = d_health.ptr
    if pre:
        f.pre_a = gs["o"].ptr; f.pre_lda = d; f.pre_bias = w["d_bo"].ptr; f.pre_res = gs["yp"].ptr; f.pre_ldres = d
    else:
        f.yn = gs["yn"].ptr; f.ldy = d; f.ln_stats = gs["st"].ptr
    if att:          # (only to be refused: the pointers are never followed)
        f.att_q = gs["o"].ptr; f.att_ldq = d; f.att_kv = gs["o"].ptr; f.att_scale = 0.25; f.att_Lk = 32
    if d_lens is not None:
        f.lens = d_lens.ptr
    rc = lib.ns2vc_k_ffn(C.byref(f), prec, None)
    L.check(lib.ns2vc_dev_sync(), "sync")
    ob, pb = gs["of"].read_bits(), gs["oo"].read_bits()
    st = gs["gs"].read_bits().view(np.int64).reshape(B, d // 16, 2)
    viol = sum((g.violations() for g in gs.values()), [])
    health = float(d_health.to_numpy((16,), dtype=np.uint32)[:1].view(np.float32)[0])
    for g in gs.values():
        g.free()
    return rc, ob, pb, st, viol, health


def _alone_rows(R, b, L):
    """the rows of item b for its own launch: L rows at T = L, or -- under the kernel's 64-frame minimum -- 64 rows: the item's, then finite
    stand-ins (valid rows of item 0, whose LayerNorm read-out the padded launch sees anyway)"""
    if L >= 64:
        return {k: _item(v, b, L) for k, v in R.items()}, L
    return {k: np.concatenate([_item(v, b, L), v[:64 - L]]) for k, v in R.items()}, 64


KERNEL_CASES = [(2, 128, True), (2, 128, False), (2, 256, True), (2, 256, False), (1, 256, True), (1, 256, False)]


@pytest.mark.parametrize("prec,dim,pre", KERNEL_CASES, ids=[f"{PREC_IDS[p]}-dim{d}-{'pre' if s else 'plain'}" for p, d, s in KERNEL_CASES])
def test_kernel_equals_items_alone(prec, dim, pre, diag):
    R = _rows(dim)
    kind = G.OP_KIND[prec]
    tag = f"masked ffn {PREC_IDS[prec]} dim {dim} {'pre-stage' if pre else 'plain'}"
    alone = []
    for b, L in enumerate(LENS0):
        rows, Ta = _alone_rows(R, b, L)
        rc, ob, pb, _, viol, h = _launch(prec, dim, pre, 1, Ta, rows)
        assert rc == 0 and not viol, (tag, b, viol, _lib()[1].ns2vc_last_error())
        assert np.isfinite(G.decode(ob.reshape(-1), "f32")).all()
        alone.append((ob[:L], pb[:L], h))
    want_h = max(h for _, _, h in alone)
    runs = {}
    for fill in ("nan", "inf"):
        bad = np.nan if fill == "nan" else np.inf
        rows = {k: _poison_rows(v, B0, T0, LENS0, bad) for k, v in R.items()}
        rc, ob, pb, st, viol, h = _launch(prec, dim, pre, B0, T0, rows, lens=LENS0, fill=fill)
        assert rc == 0, (tag, _lib()[1].ns2vc_last_error())
        assert not viol, (tag, fill, viol)                                    # guard bands of every tensor
        for b, L in enumerate(LENS0):
            oa, pa = _item(ob, b, L), _item(pb, b, L)
            assert np.array_equal(oa, alone[b][0]), (tag, fill, "out_f32", b, L, int((oa != alone[b][0]).sum()))
            assert np.array_equal(pa, alone[b][1]), (tag, fill, "out_op", b, L, int((pa != alone[b][1]).sum()))
            assert not ob[b * T0 + L:(b + 1) * T0].any(), (tag, fill, "out_f32 rows past the end", b, L)      # exact zeros: every storage word 0
            assert not pb[b * T0 + L:(b + 1) * T0].any(), (tag, fill, "out_op rows past the end", b, L)
        diag(f"{tag} fill={fill}: ln_health {h!r}, maximum of the items alone {want_h!r}")
        assert h == want_h, (tag, fill, h, want_h)
        runs[fill] = (ob, st)
    # statistics: the same integers whatever the padded rows hold ...
    assert np.array_equal(runs["nan"][1], runs["inf"][1]), tag
    # ... and the fp64 sums over the valid rows of the launch's own fp32 result, relative to the largest (as test_ffn_fused computes them)
    ob, st = runs["nan"]
    out = G.decode(ob.reshape(-1), "f32").reshape(M0, dim)
    want = _stats_ref(out, B0, T0, LENS0)
    got = np.stack([st[..., 0] / SUM_SCALE, st[..., 1] / SQ_SCALE], axis=-1)
    e_s = np.abs(got[..., 0] - want[..., 0]).max() / np.abs(want[..., 0]).max()
    e_q = np.abs(got[..., 1] - want[..., 1]).max() / want[..., 1].max()
    # the item with one valid row against its OWN sums: one commit per (block, moment), each off by at most half a fixed-point unit
    b1 = LENS0.index(1)
    lim = [TOL_STATS * np.abs(want[b1, :, k]).max() + HALF_Q[k] for k in range(2)]
    d1 = [np.abs(got[b1, :, k] - want[b1, :, k]).max() for k in range(2)]
    diag(f"{tag}: stats sum {e_s:.2e} sumsq {e_q:.2e} (bar {TOL_STATS:.0e}); one-row item: sum off by {d1[0]:.2e} (limit {lim[0]:.2e}), "
         f"sumsq {d1[1]:.2e} (limit {lim[1]:.2e})")
    assert e_s < TOL_STATS and e_q < TOL_STATS
    assert d1[0] <= lim[0] and d1[1] <= lim[1]


def test_refusals(diag):
    """`lens` together with the in-kernel cross-attention, and with M != B * T, are errors: nothing is launched, the outputs keep what they held.
    Only the first case reaches ffn_masks_rows: launch_ffn turns M != B * T away on its first line with or without `lens`, so the second case
    holds the launcher to what it did before, now that the frame of a row is derived from T."""
    prec, dim = 2, 256
    R = _rows(dim)
    fill_f = G.encode(np.full(1, OUT_FILL, np.float32), "f32")[0]
    fill_o = G.encode(np.full(1, OUT_FILL, np.float32), "f16")[0]
    for name, kw in {"lens with att_q": dict(att=True), "lens with M != B * T": dict(M=M0 - 1)}.items():
        rc, ob, pb, st, viol, h = _launch(prec, dim, True, B0, T0, R, lens=LENS0, **kw)
        msg = _lib()[1].ns2vc_last_error().decode()
        diag(f"masked ffn refusal, {name}: status {rc} ({msg})")
        assert rc != 0, name
        assert not viol and np.all(ob == fill_f) and np.all(pb == fill_o) and not st.any() and h == 0.0, name


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


def _engine(prec, weights, fuse=True, attn=True, rows=True, ffn=True):
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    for name, on in (("masked_fuse", fuse), ("masked_attn", attn), ("masked_rows", rows), ("masked_ffn", ffn)):
        e.set_option(name, on)
    return e


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_masked_ffn_forward_equals_items_alone(prec, weights, diag):
    lens = [131, 127, 66]
    T, Lp = 131, 40
    x, c, p, t = _inputs(len(lens), T, Lp, "mr1")
    for b, L in enumerate(lens):
        x[b, :, L:] = 7.0
        c[b, :, L:] = -3.0
    e = _engine(prec, weights)
    try:
        # every item's own batch-1 forward (dense plans ignore the four options)
        refs = [_forward(e, x[b:b + 1, :, :L].contiguous(), c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), t[b:b + 1].contiguous())
                for b, L in enumerate(lens)]
        y = _forward(e, x, c, p, t, lens)
        assert len([n for n in _names(e) if n.endswith(FFN_NAME)]) > 0                  # the option took effect in this plan
    finally:
        e.close()
    assert np.isfinite(y).all()
    _zero_tails(y, lens, T)
    for b, L in enumerate(lens):
        m = local_errors(y[b:b + 1, :, :L], refs[b])
        diag(f"masked_ffn forward {prec} (all four options on) L={L}: item {m['item']:.2e} (bar {_bar(TOL, prec):.0e}) frame {m['frame']:.2e} "
             f"chan {m['chan']:.2e} (bar {_bar(FRAME_TOL, prec):.1e})")
        assert m["item"] < _bar(TOL, prec), (L, m)
        assert m["frame"] < _bar(FRAME_TOL, prec) and m["chan"] < _bar(FRAME_TOL, prec), (L, m)


def test_masked_ffn_sampled_on_vs_off(weights, diag):
    """the flipped-option bars through a short sampling loop, captured and eager"""
    import torch
    lens = [131, 127, 66]
    B, T, Lp = len(lens), 131, 40
    _, c, p, _ = _inputs(B, T, Lp, "mr1")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(5)).to(c.device)
    res = {}
    e = _engine("fp16", weights)
    try:
        for ffn in (False, True):
            e.set_option("masked_ffn", ffn)
            res[ffn] = (_sample(e, c, p, xT, lens, True), _sample(e, c, p, xT, lens, False))
            assert bool([n for n in _names(e) if n.endswith(FFN_NAME)]) == ffn
    finally:
        e.close()
    eg, ee = (rel_l2(res[True][i], res[False][i]) for i in range(2))
    gve = rel_l2(res[True][0], res[True][1])
    diag(f"masked_ffn on vs off under lengths fp16: sampled graph {eg:.2e} eager {ee:.2e}; graph vs eager {gve:.2e}")
    assert eg < 2e-3 and ee < 2e-3
    assert gve < 1e-6
    for y in res[True]:
        _zero_tails(y, lens, T)


def test_fp32_engine_ignores_the_option(weights, diag):
    lens = [131, 127, 66]
    T, Lp = 131, 40
    x, c, p, t = _inputs(len(lens), T, Lp, "mr1")
    e = _engine("fp32", weights, ffn=False)
    try:
        y0 = _forward(e, x, c, p, t, lens)
        n0 = _names(e)
        e.set_option("masked_ffn", True)
        y1 = _forward(e, x, c, p, t, lens)
        assert _names(e) == n0 and not [n for n in n0 if ".ffn[" in n]
    finally:
        e.close()
    assert np.array_equal(y0, y1)
    _zero_tails(y1, lens, T)


def _replaced(n):
    """is this one of the launches the kept feed-forward launch stands for, or a mask_rows sweep behind one of them?"""
    base = n[:-len(".mask")] if n.endswith(".mask") else n
    return base.endswith(".attn2.to_out") or base.endswith(".norm3") or ".ff.geglu" in base or base.endswith(".ff.out+proj_out")


@pytest.mark.parametrize("T", [520, 300], ids=["levels_520_260_130_65", "levels_300_150_75_38"])
def test_masked_ffn_launch_list(T, weights, diag):
    """with the option on, every transformer block that runs the pre-stage form in the dense plan (dim 128 / 256, a level of 64 frames or more) runs
    it under lengths too, in place of attn2.to_out, norm3, ff.geglu, ff.out+proj_out and their sweeps; every other block, and everything outside the
    blocks, shows today's names.  T = 520: every level has 64 frames or more; T = 300: the deepest level has 38."""
    from ns2vc_amd.engine import Engine
    B, Lp = 2, 40
    lens = [T, T - 169]
    got = {}
    e = Engine(precision="fp16")                                       # the option never set
    e.load_state_dict(weights)
    try:
        e.prepare(B, T, Lp)
        dense = _names(e)
        for others in (True, False):
            for name in ("masked_fuse", "masked_attn", "masked_rows"):
                e.set_option(name, others)
            e.prepare(B, T, Lp)
            e.set_lengths(lens)
            got[(others, None)] = _names(e)
            e.set_lengths(None)
            for ffn in (True, False):
                e.set_option("masked_ffn", ffn)
                e.prepare(B, T, Lp)
                assert _names(e) == dense                              # dense plans ignore the option
                e.set_lengths(lens)
                got[(others, ffn)] = _names(e)
                e.set_lengths(None)
                assert _names(e) == dense
    finally:
        e.close()
    kept = sorted({_block_of(n) for n in dense if n.endswith(FFN_NAME)})
    blocks = sorted({_block_of(n) for n in dense if _block_of(n)})
    assert kept and len(kept) < len(blocks)                            # dim 384 / 512 blocks exist and are not eligible
    for others in (True, False):
        never, off, on = got[(others, None)], got[(others, False)], got[(others, True)]
        assert off == never                                            # option off = option never set, name for name
        assert not [n for n in off if ".ffn[" in n]                    # today's fallback
        assert [n for n in on if _block_of(n) is None] == [n for n in off if _block_of(n) is None]       # nothing outside the blocks changes
        for P in blocks:
            b_off, b_on = [n for n in off if _block_of(n) == P], [n for n in on if _block_of(n) == P]
            if P not in kept:
                assert b_on == b_off, (P, b_on, b_off)                 # today's names
                continue
            assert [n for n in b_off if _replaced(n)], (P, b_off)
            # the block's list is today's without the replaced launches and their sweeps, then the one kept launch (with no .mask behind it)
            assert b_on == [n for n in b_off if not _replaced(n)] + [P + FFN_NAME], (P, b_on, b_off)
            assert not [n for n in b_on if _replaced(n)]
            diag(f"launches T={T} others={int(others)} {P}: {len(b_off)} -> {len(b_on)} with masked_ffn")
        diag(f"launches T={T} B={B} others={int(others)}: {len(off)} -> {len(on)} with masked_ffn; dense {len(dense)}")


def test_masked_ffn_graph_captured_under_other_lengths(weights, diag):
    """a UniPC loop of 4 steps captured under one set of lengths and replayed under another: graph == eager bit for bit, every item == alone (2.5e-3,
    the sampled bar of test_sampled_padded_batch_equals_items_alone), dense before == dense after"""
    import torch
    B, T, Lp = 4, 256, 40
    _, c, p, _ = _inputs(B, T, Lp, "rg4")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(3)).to(c.device)
    A, Bl = [256, 200, 100, 9], [17, 256, 255, 64]
    e = _engine("fp16", weights)
    try:
        xd0 = torch.from_numpy(_sample(e, c, p, xT, None, True))
        _sample(e, c, p, xT, A, True)                                  # captured under A
        assert [n for n in _names(e) if n.endswith(FFN_NAME)]
        e.set_lengths(Bl)                                              # no prepare, no load_sampler in between: the same graph replayed under B
        e.set_condition(c, p, None)
        xg = xT.clone()
        e.sample(xg, use_graph=True)
        xe = xT.clone()
        e.sample(xe, use_graph=False)
        e.set_lengths(None)                                            # dense again: bit for bit what it was
        e.set_condition(c, p, None)
        xd1 = xT.clone()
        e.sample(xd1, use_graph=True)
        torch.cuda.synchronize()
        xg, xe = xg.cpu().numpy(), xe.cpu().numpy()
        assert np.isfinite(xg).all()
        assert np.array_equal(xg, xe)
        assert np.array_equal(xd0.numpy(), xd1.cpu().numpy())
        _zero_tails(xg, Bl, T)
        worst = 0.0
        for b, L in enumerate(Bl):
            one = _sample(e, c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), xT[b:b + 1, :, :L].contiguous(), None, True)
            worst = max(worst, rel_l2(xg[b, :, :L], one[0]))
        diag(f"masked_ffn unipc-4 fp16 replayed under other lengths: graph == eager; worst item vs alone {worst:.2e} (bar 2.5e-3)")
        assert worst < 2.5e-3
    finally:
        e.close()
