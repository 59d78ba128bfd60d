"""Length-masked token-stationary GEGLU (ns2vc_geglu_args.T / lens, engine option ``masked_geglu``).

Kernel level, with ln_stats given: item b of a padded launch gives, on its valid rows, BIT FOR BIT what the dense kernel gives for that item alone at
M = L_b (a lane owns one token, so a token's arithmetic does not depend on its place in a block), exact zeros past its end, with the padded rows of
yn and ln_stats holding NaN or Inf and out_op pre-filled inside guard bands; ln_health is the maximum of the alone launches' read-outs.  With
ln_stats NULL the kernel takes the LayerNorm sums from the rounded operand row: the same statements against the masked kernel on the item alone
(B = 1, T = L_b), and the valid rows against numpy fp64 with mean / var of the rounded row.  Engine level: with the option on, a masked plan keeps
the token-stationary launch of every dim-384 block, without norm3 and without a sweep behind it, and still gives every item as if alone.

Shapes.  A: B = 5, T = 200, lens = [200, 129, 33, 1, 72] (M = 1000, 8 token blocks): item ends in three different 32-token quarters, an item that
starts mid-quarter, block 4 (rows 512 .. 639) with row 600 as its only valid row -- one token quarter's two waves have a live token, the other six
have none --, block 5 (640 .. 767) wholly padded, the short last block (896 .. 999) wholly padded.  B: B = 60, T = 5, lens cycling 5, 4, 3, 2, 1
(M = 300): about 25 items per block, a short last block with valid rows.

Bounds: eps16 / GEGLU_FLIPS (tests/util.py, the bars of test_geglu_token_stationary) and the constants of tests/test_ragged_gpu.py (TOL, FRAME_TOL;
2.5e-3 sampled, 2e-3 / 1e-6 for a flipped option as test_every_plan_option_under_lengths states them) -- nothing of this file's own; bf16 takes the
factor tests/test_masked_rows_gpu.py states and derives (`_bar`)."""
import contextlib
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard as G                                  # noqa: E402
from test_masked_rows_gpu import OUT_FILL, PREC_IDS, _bar, _dev, _item, _lib, _rounded, _zero_tails      # noqa: E402
from test_ragged_fused_gpu import _block_of, _names, _poison_rows                 # noqa: E402
from test_ragged_gpu import FRAME_TOL, TOL, _forward, _inputs, _sample            # noqa: E402
from util import GEGLU_FLIPS, eps16, gelu_erf, local_errors, rel_l2               # noqa: E402

pytestmark = pytest.mark.gpu

D = 384
SHAPES = {"A": (5, 200, [200, 129, 33, 1, 72]), "B": (60, 5, [5, 4, 3, 2, 1] * 12)}
LDO_EXTRA = {"A": 0, "B": 64}                      # an output pitch wider than 4 dim once: the columns past 4 dim are gap columns of the guarded tensor
TS_NAME = ".ff.geglu[token-stationary]"


@functools.lru_cache(maxsize=None)
def _weights(prec):
    """host matrices with the engine's pack-time folds, as test_geglu_token_stationary builds them (LayerNorm gamma / beta into W1 / b1, value | gate
    row interleave), and the packed device stream / constants: built once per operand type and shared by the cases"""
    L, lib = _lib()
    rng = np.random.default_rng(9100)
    d = D
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(d)), 0.2 * rng.standard_normal(d)
    W1, b1 = rng.standard_normal((8 * d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(8 * d)
    W1f, b1f = W1 * gamma[None, :], b1 + W1 @ beta
    order = np.concatenate([np.concatenate([np.arange(32 * g, 32 * g + 32), 4 * d + np.arange(32 * g, 32 * g + 32)]) for g in range(4 * d // 32)])
    W1p, b1p = np.ascontiguousarray(W1f[order].astype(np.float32)), np.ascontiguousarray(b1f[order].astype(np.float32))
    stream, consts = C.c_void_p(), C.c_void_p()
    L.check(lib.ns2vc_pack_geglu(W1p.ctypes.data, b1p.ctypes.data, d, prec, C.byref(stream), C.byref(consts)), "pack_geglu")
    return dict(W1r=_rounded(W1p, prec), b1p=b1p.astype(np.float64), stream=stream, consts=consts)


@functools.lru_cache(maxsize=None)
def _rows(shape):
    """y (rows with a common offset of 1.5 sigma) and its LayerNorm-by-linearity statistics as a producer GEMM's `rowstats` leaves them"""
    B, T, _ = SHAPES[shape]
    M = B * T
    rng = np.random.default_rng(500 + M)
    y = (rng.standard_normal((M, D)) + 1.5 * rng.standard_normal((M, 1))).astype(np.float32)
    ys = y.astype(np.float64).reshape(M, D // 64, 64)
    st = np.stack([ys.sum(2), (ys ** 2).sum(2)], axis=-1).astype(np.float32).reshape(M, D // 64 * 2)
    return y, st


def _launch(prec, M, y, st, *, T=0, lens=None, fill="nan", ldo_extra=0, twice=False):
    """one ns2vc_k_geglu launch on guarded tensors -> (status, out_op storage words (M, 4 dim), guard violations, ln_health).  y: (M, dim) rows (NaN /
    Inf allowed); st: (M, dim / 64 * 2) statistics rows or None (ln_stats = NULL); out_op holds OUT_FILL before the launch.  twice: the launch is
    repeated into a second output and both results are returned as a pair."""
    L, lib = _lib()
    w = _weights(prec)
    bk = G.DeviceBackend()
    kind = G.OP_KIND[prec]
    ldo = 4 * D + ldo_extra
    gs = {"yn": G.Guarded(bk, M, D, kind, data=y, fill=fill, name="yn")}
    if st is not None:
        gs["st"] = G.Guarded(bk, M, D // 64 * 2, "f32", data=st, fill=fill, name="ln_stats")
    outs = ["out"] + (["out2"] if twice else [])
    for o in outs:
        gs[o] = G.Guarded(bk, M, 4 * D, kind, ld=ldo, data=np.full((M, 4 * D), OUT_FILL, np.float32), fill=fill, name=o)
    d_health = _dev(np.zeros(16, dtype=np.uint32), np.uint32)
    d_lens = _dev(lens, np.int32) if lens is not None else None
    f = L.GegluArgs()
    f.yn = gs["yn"].ptr; f.ldy = D
    f.ln_stats = gs["st"].ptr if st is not None else None
    f.ln_eps = 1e-5
    f.wstream = w["stream"].value; f.consts = w["consts"].value
    f.ldo = ldo; f.M = M; f.dim = D; f.ln_health = d_health.ptr
    f.T = T
    if d_lens is not None:
        f.lens = d_lens.ptr
    rc = 0
    for o in outs:
        f.out_op = gs[o].ptr
        rc = rc or lib.ns2vc_k_geglu(C.byref(f), prec, None)
    L.check(lib.ns2vc_dev_sync(), "sync")
    bits = [gs[o].read_bits() for o in outs]
    viol = sum((g.violations() for g in gs.values()), [])
    health = float(d_health.to_numpy((16,), dtype=np.uint32)[:1].view(np.float32)[0])
    for g in gs.values():
        g.free()
    return rc, (tuple(bits) if twice else bits[0]), viol, health


def _check_items(tag, bits, alone, lens, T, fill):
    for b, L in enumerate(lens):
        got = _item(bits, b, L, T)
        assert np.array_equal(got, alone[b][0]), (tag, fill, "valid rows", b, L, int((got != alone[b][0]).sum()))
        assert not bits[b * T + L:(b + 1) * T].any(), (tag, fill, "rows past the end", b, L)      # exact zeros: every storage word 0


@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_kernel_with_stats_equals_dense_items_alone(prec, shape, diag):
    B, T, lens = SHAPES[shape]
    M = B * T
    y, st = _rows(shape)
    tag = f"masked geglu {PREC_IDS[prec]} shape {shape} (ln_stats given)"
    alone = []
    for b, L in enumerate(lens):           # the dense kernel (no lens) on the item alone at M = L_b
        rc, bits, viol, h = _launch(prec, L, _item(y, b, L, T), _item(st, b, L, T))
        assert rc == 0 and not viol, (tag, b, viol, _lib()[1].ns2vc_last_error())
        assert np.isfinite(G.decode(bits.reshape(-1), G.OP_KIND[prec])).all()
        alone.append((bits, h))
    want_h = max(h for _, h in alone)
    runs = {}
    for fill in ("nan", "inf"):
        bad = np.nan if fill == "nan" else np.inf
        rc, bits, viol, h = _launch(prec, M, _poison_rows(y, B, T, lens, bad), _poison_rows(st, B, T, lens, bad), T=T, lens=lens, fill=fill,
                                    ldo_extra=LDO_EXTRA[shape])
        assert rc == 0, (tag, _lib()[1].ns2vc_last_error())
        assert not viol, (tag, fill, viol)           # guard bands of every tensor, and the columns past 4 dim of out_op
        _check_items(tag, bits, alone, lens, T, fill)
        diag(f"{tag} fill={fill}: ln_health {h!r}, maximum of the items alone {want_h!r}")
        assert h == want_h, (tag, fill, h, want_h)
        runs[fill] = bits
    assert np.array_equal(runs["nan"], runs["inf"]), tag       # the result does not depend on what the padded rows hold


def _reference(prec, y):
    """numpy fp64 of the projection with the kernel's rounding points and mean / var taken from the ROUNDED row"""
    w = _weights(prec)
    yr = _rounded(y, prec)
    mean, var = yr.mean(1, keepdims=True), yr.var(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    W1r = w["W1r"]
    pre = rstd * (yr @ W1r.T - mean * W1r.sum(1).astype(np.float32).astype(np.float64)[None, :]) + w["b1p"][None, :]
    pg = pre.reshape(len(y), 4 * D // 32, 2, 32)
    return (pg[:, :, 0] * gelu_erf(pg[:, :, 1])).reshape(len(y), 4 * D)


@pytest.mark.parametrize("shape", ["A", "B"])
@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_kernel_own_stats_equals_items_alone_and_fp64(prec, shape, diag):
    B, T, lens = SHAPES[shape]
    M = B * T
    y, _ = _rows(shape)
    kind = G.OP_KIND[prec]
    tag = f"masked geglu {PREC_IDS[prec]} shape {shape} (ln_stats NULL)"
    alone = []
    for b, L in enumerate(lens):           # the masked kernel on the item alone: B = 1, T = L_b, lens = [L_b]
        rc, bits, viol, h = _launch(prec, L, _item(y, b, L, T), None, T=L, lens=[L])
        assert rc == 0 and not viol, (tag, b, viol, _lib()[1].ns2vc_last_error())
        alone.append((bits, h))
    want_h = max(h for _, h in alone)
    valid = np.concatenate([np.arange(b * T, b * T + L) for b, L in enumerate(lens)])
    ref = _reference(prec, y[valid])
    runs = {}
    for fill in ("nan", "inf"):
        bad = np.nan if fill == "nan" else np.inf
        rc, (bits, bits2), viol, h = _launch(prec, M, _poison_rows(y, B, T, lens, bad), None, T=T, lens=lens, fill=fill, ldo_extra=LDO_EXTRA[shape],
                                             twice=True)
        assert rc == 0, (tag, _lib()[1].ns2vc_last_error())
        assert not viol, (tag, fill, viol)
        _check_items(tag, bits, alone, lens, T, fill)
        assert np.array_equal(bits, bits2), (tag, fill)            # the same launch twice: bitwise equal
        assert h == want_h, (tag, fill, h, want_h)
        runs[fill] = bits
    assert np.array_equal(runs["nan"], runs["inf"]), tag
    out = G.decode(runs["nan"].reshape(-1), kind).reshape(M, 4 * D)[valid].astype(np.float64)
    e = rel_l2(out, ref)
    flips = float(np.mean(G.encode(out.astype(np.float32), kind) != G.encode(ref.astype(np.float32), kind)))
    diag(f"{tag}: vs fp64 with the rounded row's mean / var, {len(valid)} valid rows: rel_l2 {e:.3e} (bar {eps16(prec):.1e}) flips {flips:.4f} "
         f"(bar {GEGLU_FLIPS}); ln_health {want_h:.3f}")
    assert np.isfinite(out).all() and e < eps16(prec) and flips < GEGLU_FLIPS


def test_refusals(diag):
    """`lens` with T < 1, `lens` with M % T != 0, and a NULL ln_stats without `lens` are errors: nothing is launched, out_op keeps what it held"""
    prec = 2
    B, T, lens = SHAPES["A"]
    M = B * T
    y, st = _rows("A")
    fill_o = G.encode(np.full(1, OUT_FILL, np.float32), "f16")[0]
    cases = {"lens with T = 0": dict(st=st, T=0, lens=lens), "lens with T = -3": dict(st=st, T=-3, lens=lens),
             "lens with M % T != 0": dict(st=st, T=7, lens=[7] * (M // 7)), "NULL ln_stats without lens": dict(st=None, T=T, lens=None)}
    for name, kw in cases.items():
        rc, bits, viol, h = _launch(prec, M, y, kw["st"], T=kw["T"], lens=kw["lens"])
        msg = _lib()[1].ns2vc_last_error().decode()
        diag(f"masked geglu refusal, {name}: status {rc} ({msg})")
        assert rc != 0, name
        assert not viol and np.all(bits == fill_o) and h == 0.0, name


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level: B = 4, T = 520 (levels 520 / 260 / 130 / 65; the dim-384 level has 520 rows, far below the dense crossover)
# ---------------------------------------------------------------------------------------------------------------------------------
EB, ET, ELP = 4, 520, 40
ELENS = [520, 389, 131, 66]
OTHERS = ("masked_fuse", "masked_attn", "masked_rows", "masked_ffn")


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


def _engine(prec, weights, others=True, geglu=True):
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    for name in OTHERS:
        e.set_option(name, others)
    e.set_option("masked_geglu", geglu)
    return e


@contextlib.contextmanager
def _no_crossover(e):
    """the planner's row threshold for the token-stationary kernel at 0 while the block runs; it is process-global, so it is restored whatever
    happens and the engine's plan rebuilt under the restored value before the engine is closed"""
    lib = _lib()[1]
    lib.ns2vc_debug_set_geglu_min_rows(0)
    try:
        yield e
    finally:
        lib.ns2vc_debug_set_geglu_min_rows(-1)
        try:
            e.prepare(EB, ET, ELP)
        finally:
            e.close()


def _poisoned_inputs(tag, lens, T):
    x, c, p, t = _inputs(len(lens), T, ELP, tag)
    for b, L in enumerate(lens):
        x[b, :, L:] = 7.0
        c[b, :, L:] = -3.0
    return x, c, p, t


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_masked_geglu_forward_equals_items_alone(prec, weights, diag):
    x, c, p, t = _poisoned_inputs("mg1", ELENS, ET)
    with _no_crossover(_engine(prec, weights)) as e:
        # every item's own batch-1 forward (dense plans ignore the five options)
        refs = [_forward(e, x[b:b + 1, :, :L].contiguous(), c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), t[b:b + 1].contiguous())
                for b, L in enumerate(ELENS)]
        ys = {}
        for others in (True, False):       # all five options on; masked_geglu alone
            for name in OTHERS:
                e.set_option(name, others)
            ys[others] = _forward(e, x, c, p, t, ELENS)
            names = _names(e)
            kept = {_block_of(n) for n in names if n.endswith(TS_NAME)}
            assert kept and not [n for n in names if n.endswith(".norm3") and _block_of(n) in kept]       # the option took effect in this plan
    for others, y in ys.items():
        assert np.isfinite(y).all()
        _zero_tails(y, ELENS, ET)
        for b, L in enumerate(ELENS):
            m = local_errors(y[b:b + 1, :, :L], refs[b])
            diag(f"masked_geglu forward {prec} (other four options {'on' if others else 'off'}) L={L}: item {m['item']:.2e} (bar {_bar(TOL, prec):.0e}) "
                 f"frame {m['frame']:.2e} chan {m['chan']:.2e} (bar {_bar(FRAME_TOL, prec):.1e})")
            assert m["item"] < _bar(TOL, prec), (others, L, m)
            assert m["frame"] < _bar(FRAME_TOL, prec) and m["chan"] < _bar(FRAME_TOL, prec), (others, L, m)


def _expected_block(b_off):
    """today's launches of a dim-384 block under lengths -> the list with the option on: no norm3, the token-stationary launch in the place of
    the GEGLU GEMM, no sweep behind it; everything else (attn2.to_out and ff.out+proj_out with their sweeps included) name for name"""
    out = []
    for n in b_off:
        base = n[:-len(".mask")] if n.endswith(".mask") else n
        if base.endswith(".norm3") or (base.endswith(".ff.geglu") and n.endswith(".mask")):
            continue
        out.append(n + "[token-stationary]" if n.endswith(".ff.geglu") else n)
    return out


def test_masked_geglu_launch_list(weights, diag):
    from ns2vc_amd.engine import Engine
    got = {}
    e = Engine(precision="fp16")                                       # the option never set
    e.load_state_dict(weights)
    # under the shipped crossover (4608 rows) the option changes nothing at this shape: the dim-384 level has 520 rows
    e.prepare(EB, ET, ELP)
    e.set_lengths(ELENS)
    shipped_never = _names(e)
    e.set_option("masked_geglu", True)
    e.prepare(EB, ET, ELP)
    e.set_lengths(ELENS)
    shipped_on = _names(e)
    e.set_option("masked_geglu", False)
    with _no_crossover(e):
        e.prepare(EB, ET, ELP)
        dense = _names(e)
        for others in (True, False):
            for name in OTHERS:
                e.set_option(name, others)
            e.prepare(EB, ET, ELP)
            e.set_lengths(ELENS)
            got[(others, None)] = _names(e)
            e.set_lengths(None)
            for on in (True, False):
                e.set_option("masked_geglu", on)
                e.prepare(EB, ET, ELP)
                assert _names(e) == dense                              # dense plans ignore the option
                e.set_lengths(ELENS)
                got[(others, on)] = _names(e)
                e.set_lengths(None)
                assert _names(e) == dense
    assert shipped_on == shipped_never and not [n for n in shipped_on if n.endswith(TS_NAME)]
    kept = sorted({_block_of(n) for n in dense if n.endswith(TS_NAME)})          # the dim-384 blocks: the dense plan runs the kernel there
    blocks = sorted({_block_of(n) for n in dense if _block_of(n)})
    assert kept and len(kept) < len(blocks)
    for others in (True, False):
        never, off, on = got[(others, None)], got[(others, False)], got[(others, True)]
        assert off == never                                            # option off = option never set, name for name
        assert not [n for n in off if n.endswith(TS_NAME)]             # today's fallback
        assert [n for n in on if _block_of(n) is None] == [n for n in off if _block_of(n) is None]       # nothing outside the blocks changes
        for P in blocks:
            b_off, b_on = [n for n in off if _block_of(n) == P], [n for n in on if _block_of(n) == P]
            if P not in kept:
                assert b_on == b_off, (P, b_on, b_off)                 # dim 128 / 256 / 512: today's names
                continue
            assert [n for n in b_off if n.endswith(".norm3")] and [n for n in b_off if n.endswith(".ff.geglu")], (P, b_off)
            assert b_on == _expected_block(b_off), (P, b_on, b_off)
            assert len([n for n in b_on if n.endswith(TS_NAME)]) == 1
            assert not [n for n in b_on if n.endswith(".norm3") or n.endswith(TS_NAME + ".mask")]
            assert [n for n in b_on if ".attn2.to_out" in n] == [n for n in b_off if ".attn2.to_out" in n]
            diag(f"launches others={int(others)} {P}: {len(b_off)} -> {len(b_on)} with masked_geglu")
        diag(f"launches B={EB} T={ET} others={int(others)}: {len(off)} -> {len(on)} with masked_geglu; dense {len(dense)}")


def test_fp32_engine_ignores_the_option(weights, diag):
    x, c, p, t = _inputs(EB, ET, ELP, "mg1")
    with _no_crossover(_engine("fp32", weights, geglu=False)) as e:
        y0 = _forward(e, x, c, p, t, ELENS)
        n0 = _names(e)
        e.set_option("masked_geglu", True)
        y1 = _forward(e, x, c, p, t, ELENS)
        assert _names(e) == n0 and not [n for n in n0 if n.endswith(TS_NAME)]
    assert np.array_equal(y0, y1)
    _zero_tails(y1, ELENS, ET)


def test_masked_geglu_sampled_on_vs_off(weights, diag):
    """the flipped-option bars through a short sampling loop, captured and eager"""
    import torch
    _, c, p, _ = _inputs(EB, ET, ELP, "mg1")
    xT = torch.randn((EB, 100, ET), generator=torch.Generator().manual_seed(5)).to(c.device)
    res = {}
    with _no_crossover(_engine("fp16", weights)) as e:
        for on in (False, True):
            e.set_option("masked_geglu", on)
            res[on] = (_sample(e, c, p, xT, ELENS, True), _sample(e, c, p, xT, ELENS, False))
            assert bool([n for n in _names(e) if n.endswith(TS_NAME)]) == on
    eg, ee = (rel_l2(res[True][i], res[False][i]) for i in range(2))
    gve = rel_l2(res[True][0], res[True][1])
    diag(f"masked_geglu on vs off under lengths fp16: sampled graph {eg:.2e} eager {ee:.2e}; graph vs eager {gve:.2e}")
    assert eg < 2e-3 and ee < 2e-3
    assert gve < 1e-6
    for y in res[True]:
        _zero_tails(y, ELENS, ET)


def test_masked_geglu_graph_captured_under_other_lengths(weights, diag):
    """a UniPC loop of 4 steps captured under one set of lengths and replayed under another: graph == eager bit for bit, every item == alone (2.5e-3,
    the sampled bar of test_sampled_padded_batch_equals_items_alone), dense before == dense after"""
    import torch
    _, c, p, _ = _inputs(EB, ET, ELP, "mg4")
    xT = torch.randn((EB, 100, ET), generator=torch.Generator().manual_seed(3)).to(c.device)
    A, Bl = [520, 400, 200, 9], [17, 520, 519, 130]
    with _no_crossover(_engine("fp16", weights)) as e:
        xd0 = torch.from_numpy(_sample(e, c, p, xT, None, True))
        _sample(e, c, p, xT, A, True)                                  # captured under A
        assert [n for n in _names(e) if n.endswith(TS_NAME)]
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
        _zero_tails(xg, Bl, ET)
        worst = 0.0
        for b, L in enumerate(Bl):
            one = _sample(e, c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), xT[b:b + 1, :, :L].contiguous(), None, True)
            worst = max(worst, rel_l2(xg[b, :, :L], one[0]))
        diag(f"masked_geglu unipc-4 fp16 replayed under other lengths: graph == eager; worst item vs alone {worst:.2e} (bar 2.5e-3)")
        assert worst < 2.5e-3
