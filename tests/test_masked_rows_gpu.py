"""Length-masked row chains (ns2vc_rowchain_args.lens, engine option ``masked_rows``).

Kernel level: item b of a padded launch gives, on its valid rows, BIT FOR BIT what the dense kernel gives for that item alone at M = L_b (a lane
owns one token, so a token's arithmetic does not depend on its place in a block), exact zeros past its end in both outputs, with the padded rows
of the inputs holding NaN or Inf and both outputs pre-filled inside guard bands; ln_health is the maximum of the alone launches' read-outs.
Engine level: with the option on, a masked plan keeps the two row-chain launches of every transformer block and still gives every item as if alone.

Bounds: TOL_ROWCHAIN_Y / eps16 (tests/util.py, the bar of test_rowchain_fused) and the constants of tests/test_ragged_gpu.py (TOL, FRAME_TOL;
2.5e-3 sampled, 2e-3 / 1e-6 for a flipped option as test_every_plan_option_under_lengths states them), imported where they have a name.  bf16
has no entry in TOL / FRAME_TOL: two bf16 runs of one item differ by operand roundings of unit roundoff 2^-9 where two fp16 runs differ by
2^-12, so its bars are the fp16 ones times eps16(bf16) / eps16(fp16) = 8."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard as G                                  # noqa: E402
import test_ragged_gpu as RG                      # noqa: E402  (the existing constants and helpers: one statement of the bars)
from test_ragged_fused_gpu import _block_of, _names, _poison_rows, _stats_ref      # noqa: E402
from test_ragged_gpu import FRAME_TOL, TOL, _forward, _inputs, _sample            # noqa: E402
from util import TOL_ROWCHAIN_Y, eps16, local_errors, rel_l2                      # noqa: E402

pytestmark = pytest.mark.gpu

PREC_IDS = {1: "bf16", 2: "fp16"}
OUT_FILL = 3.25                                    # what the outputs hold before a launch (non-zero, exact in every operand type)
B0, T0 = 6, 130                                    # item ends inside the first, second and third 64-token block; item boundaries mid-block
LENS0 = [130, 129, 65, 64, 63, 1]
GN_SUM_SCALE, GN_SQ_SCALE = 2.0 ** 28, 2.0 ** 16   # the int64 fixed point of ns2vc_gemm_args.stats (as test_rowchain_groupnorm_prologue builds it)


def _bar(table, prec):
    return table[prec] if prec in table else table["fp16"] * eps16(1) / eps16(2)


def _lib():
    from ns2vc_amd import _lib as L
    return L, L.load()


def _dev(a, dtype=np.float32):
    from ns2vc_amd.engine import DevBuf
    return DevBuf.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def _rounded(a, prec):
    kind = G.OP_KIND[prec]
    return G.decode(G.encode(a, kind), kind).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _weights(dim, mult, prec, slices):
    """host matrices and the packed device stream / constants of one chain, built once per (dim, n2, operand type, slicing) and shared by the cases"""
    L, lib = _lib()
    rng = np.random.default_rng(7000 + dim + mult)
    d, n2 = dim, mult * dim
    W1, b1 = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), (0.3 * rng.standard_normal(d)).astype(np.float32)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(d)), 0.2 * rng.standard_normal(d)
    W2, b2 = rng.standard_normal((n2, d)) / np.sqrt(d), 0.3 * rng.standard_normal(n2)
    W2f, b2f = np.ascontiguousarray((W2 * gamma[None, :]).astype(np.float32)), (b2 + W2 @ beta).astype(np.float32)
    consts = np.stack([_rounded(W2f, prec).sum(1), b2f.astype(np.float64)], axis=1).astype(np.float32)
    stream = C.c_void_p()
    if slices:
        L.check(lib.ns2vc_pack_rowchain_sliced(W1.ctypes.data, W2f.ctypes.data, d, n2, slices, prec, C.byref(stream)), "pack_rowchain_sliced")
    else:
        L.check(lib.ns2vc_pack_rowchain(W1.ctypes.data, W2f.ctypes.data, d, n2, prec, C.byref(stream)), "pack_rowchain")
    return dict(W1=W1, b1=b1, W2f=W2f, b2f=b2f, consts=consts, stream=stream, d_b1=_dev(b1), d_c=_dev(consts))


def _launch(prec, dim, mult, M, *, a=None, res=None, inplace=False, lens=None, T=0, nt=1, slices=0, fill="nan", gn=None):
    """one ns2vc_k_rowchain launch on guarded tensors -> (status, y storage words (M, dim), z storage words (M, n2), guard violations, ln_health).
    a: operand rows (M, dim) float32 (NaN / Inf allowed), or gn = dict(x, stats, gamma, beta, G) for the GroupNorm prologue; res: fp32 residual
    rows, which out1 holds before the launch when `inplace` (res aliases out1, as the engine uses it); otherwise both outputs hold OUT_FILL."""
    L, lib = _lib()
    w = _weights(dim, mult, prec, slices)
    bk = G.DeviceBackend()
    kind = G.OP_KIND[prec]
    d, n2 = dim, mult * dim
    gs = {}
    if gn is None:
        gs["a"] = G.Guarded(bk, M, d, kind, data=a, fill=fill, name="a_op")
    else:
        gs["x"] = G.Guarded(bk, M, d, "f32", data=gn["x"], fill=fill, name="gn_x")
    assert res is None or inplace
    gs["y"] = G.Guarded(bk, M, d, "f32", data=res if inplace else np.full((M, d), OUT_FILL, np.float32), fill=fill, name="out1_f32")
    gs["z"] = G.Guarded(bk, M, n2, kind, data=np.full((M, n2), OUT_FILL, np.float32), fill=fill, name="out2_op")
    d_health = _dev(np.zeros(16, dtype=np.uint32), np.uint32)
    keep = [_dev(lens, np.int32) if lens is not None else None]
    f = L.RowchainArgs()
    f.a_op = gs["a"].ptr if gn is None else None
    f.lda = d; f.wstream = w["stream"].value; f.bias1 = w["d_b1"].ptr; f.consts2 = w["d_c"].ptr
    f.res = gs["y"].ptr if inplace else None
    f.ldres = d; f.out1_f32 = gs["y"].ptr; f.ldo1 = d; f.out2_op = gs["z"].ptr; f.ldo2 = n2
    f.ln_eps = 1e-5; f.M = M; f.dim = d; f.n2 = n2; f.ln_health = d_health.ptr
    f.T = T; f.slices = slices
    if gn is not None:
        keep += [_dev(gn["stats"], np.int64), _dev(gn["gamma"]), _dev(gn["beta"])]
        f.gn_x = gs["x"].ptr; f.ldx = d; f.gn_stats = keep[1].ptr; f.gn_gamma = keep[2].ptr; f.gn_beta = keep[3].ptr; f.gn_eps = 1e-6; f.G = gn["G"]
    if lens is not None:
        f.lens = keep[0].ptr
    L.check(lib.ns2vc_debug_set_rowchain_tokens(nt), "set_rowchain_tokens")
    try:
        rc = lib.ns2vc_k_rowchain(C.byref(f), prec, None)
        L.check(lib.ns2vc_dev_sync(), "sync")
    finally:
        lib.ns2vc_debug_set_rowchain_tokens(0)
    ybits, zbits = gs["y"].read_bits(), gs["z"].read_bits()
    viol = sum((g.violations() for g in gs.values()), [])
    health = float(d_health.to_numpy((16,), dtype=np.uint32)[:1].view(np.float32)[0])
    for g in gs.values():
        g.free()
    return rc, ybits, zbits, viol, health


@functools.lru_cache(maxsize=None)
def _rows(dim):
    rng = np.random.default_rng(300 + dim)
    A = rng.standard_normal((B0 * T0, dim)).astype(np.float32)
    R = (rng.standard_normal((B0 * T0, dim)) + 1.5 * rng.standard_normal((B0 * T0, 1))).astype(np.float32)
    return A, R


def _item(a, b, L, T=T0):
    return a[b * T:b * T + L]


def _check_against_alone(tag, masked, alone, lens, T, diag):
    """masked = {fill: (ybits, zbits, health)}, alone = [(ybits, zbits, health)] per item"""
    for fill, (yb, zb, health) in masked.items():
        for b, L in enumerate(lens):
            ya, za = _item(yb, b, L, T), _item(zb, b, L, T)
            assert np.array_equal(ya, alone[b][0]), (tag, fill, "y", b, L, int((ya != alone[b][0]).sum()))
            assert np.array_equal(za, alone[b][1]), (tag, fill, "z", b, L, int((za != alone[b][1]).sum()))
            assert not yb[b * T + L:(b + 1) * T].any(), (tag, fill, "y rows past the end", b, L)      # exact zeros: every storage word 0
            assert not zb[b * T + L:(b + 1) * T].any(), (tag, fill, "z rows past the end", b, L)
        want = max(h for _, _, h in alone)
        diag(f"{tag} fill={fill}: ln_health {health!r}, maximum of the items alone {want!r}")
        assert health == want, (tag, fill, health, want)


PLAIN_CASES = ([(2, 128, mult, nt, 0, res) for nt in (1, 2) for mult in (1, 3) for res in (False, True)] +
               [(2, 256, mult, 1, 0, res) for mult in (1, 3) for res in (False, True)] +
               [(2, 384, mult, 1, sl, res) for sl in (0, 2) for mult in (1, 3) for res in (False, True)] +
               [(1, 256, mult, 1, 0, res) for mult in (1, 3) for res in (False, True)])


@pytest.mark.parametrize("prec,dim,mult,nt,slices,res", PLAIN_CASES,
                         ids=[f"{PREC_IDS[p]}-dim{d}-n2x{m}-nt{n}-slices{s}-{'inplace_res' if r else 'nores'}" for p, d, m, n, s, r in PLAIN_CASES])
def test_kernel_plain_form(prec, dim, mult, nt, slices, res, diag):
    A, R = _rows(dim)
    M, n2 = B0 * T0, mult * dim
    tag = f"masked rowchain {PREC_IDS[prec]} dim {dim} n2 {n2} nt {nt} slices {slices} res {int(res)}"
    if slices and res:
        # two slices would race on y: refused with lengths as without, and nothing is stored
        rc, yb, zb, viol, _ = _launch(prec, dim, mult, M, a=A, res=R, inplace=True, lens=LENS0, T=T0, nt=nt, slices=slices)
        assert rc != 0 and not viol
        assert np.array_equal(yb, G.encode(R, "f32").reshape(M, dim)) and np.all(zb == G.encode(np.full(1, OUT_FILL, np.float32), G.OP_KIND[prec])[0])
        return
    alone = []
    for b, L in enumerate(LENS0):
        rc, yb, zb, viol, h = _launch(prec, dim, mult, L, a=_item(A, b, L), res=_item(R, b, L) if res else None, inplace=res, nt=nt, slices=slices)
        assert rc == 0 and not viol, (tag, b, viol, _lib()[1].ns2vc_last_error())
        alone.append((yb, zb, h))
    # one accuracy check of an alone launch against numpy fp64 with the kernel's rounding points (the bar of test_rowchain_fused)
    w = _weights(dim, mult, prec, slices)
    Ar, W1r, W2r = _rounded(A[:T0], prec), _rounded(w["W1"], prec), _rounded(w["W2f"], prec)
    y = Ar @ W1r.T + w["b1"].astype(np.float64)[None, :] + (R[:T0].astype(np.float64) if res else 0.0)
    yr = _rounded(y.astype(np.float32), prec)
    z = (yr @ W2r.T - y.mean(1, keepdims=True) * w["consts"][:, 0].astype(np.float64)[None, :]) / np.sqrt(y.var(1, keepdims=True) + 1e-5) + \
        w["b2f"].astype(np.float64)[None, :]
    e_y = rel_l2(G.decode(alone[0][0].reshape(-1), "f32").reshape(T0, dim), y)
    e_z = rel_l2(G.decode(alone[0][1].reshape(-1), G.OP_KIND[prec]).reshape(T0, n2), z)
    diag(f"{tag}: item 0 alone vs fp64 y {e_y:.2e} (bar {TOL_ROWCHAIN_Y:.0e}) z {e_z:.2e} (bar {eps16(prec):.1e})")
    assert e_y < TOL_ROWCHAIN_Y and e_z < eps16(prec)
    masked = {}
    for fill in ("nan", "inf"):
        bad = np.nan if fill == "nan" else np.inf
        rc, yb, zb, viol, h = _launch(prec, dim, mult, M, a=_poison_rows(A, B0, T0, LENS0, bad), res=_poison_rows(R, B0, T0, LENS0, bad) if res else None,
                                      inplace=res, lens=LENS0, T=T0, nt=nt, slices=slices, fill=fill)
        assert rc == 0, (tag, _lib()[1].ns2vc_last_error())
        assert not viol, (tag, fill, viol)
        masked[fill] = (yb, zb, h)
    _check_against_alone(tag, masked, alone, LENS0, T0, diag)


@pytest.mark.parametrize("Gn", [8, 4])
def test_kernel_groupnorm_form(Gn, diag):
    prec, dim, B, T = 2, 256, 4, 130
    lens = [130, 100, 65, 64]
    rng = np.random.default_rng(900 + Gn)
    x = (rng.standard_normal((B, T, dim)) * (1.0 + rng.random((B, 1, dim))) + rng.standard_normal((B, 1, dim))).astype(np.float32).reshape(B * T, dim)
    gam, bet = (1.0 + 0.2 * rng.standard_normal(dim)).astype(np.float32), (0.2 * rng.standard_normal(dim)).astype(np.float32)
    # the statistics as the masked conv epilogue leaves them: int64 fixed point over the valid rows only
    sr = _stats_ref(x, B, T, lens)
    st = np.stack([np.rint(sr[..., 0] * GN_SUM_SCALE), np.rint(sr[..., 1] * GN_SQ_SCALE)], axis=-1).astype(np.int64)
    for mult in (3, 1):
        tag = f"masked rowchain+GroupNorm fp16 dim {dim} G {Gn} n2 {mult * dim}"
        alone = []
        for b, L in enumerate(lens):
            gn = dict(x=_item(x, b, L, T), stats=st[b:b + 1], gamma=gam, beta=bet, G=Gn)
            rc, yb, zb, viol, h = _launch(prec, dim, mult, L, gn=gn, T=L)
            assert rc == 0 and not viol, (tag, b, viol, _lib()[1].ns2vc_last_error())
            assert np.isfinite(G.decode(zb.reshape(-1), "f16")).all()
            alone.append((yb, zb, h))
        gn = dict(x=_poison_rows(x, B, T, lens, np.nan), stats=st, gamma=gam, beta=bet, G=Gn)
        rc, yb, zb, viol, h = _launch(prec, dim, mult, B * T, gn=gn, lens=lens, T=T)
        assert rc == 0, (tag, _lib()[1].ns2vc_last_error())
        assert not viol, (tag, viol)
        _check_against_alone(tag, {"nan": (yb, zb, h)}, alone, lens, T, diag)


def test_refusals(diag):
    """`lens` with T = 0, with M % T != 0, and with a GroupNorm prologue under 64 frames are errors, and the outputs keep what they held.
    (The list of refused shapes is empty -- tests/test_masked_rows_cpu.py -- so there is no shape to try.)"""
    prec, dim = 2, 256
    A, _ = _rows(dim)
    M = B0 * T0
    fill_y = G.encode(np.full(1, OUT_FILL, np.float32), "f32")[0]
    fill_z = G.encode(np.full(1, OUT_FILL, np.float32), "f16")[0]
    rng = np.random.default_rng(5)
    B, T = 13, 60                                  # 13 x 60 = 780 rows: M % T == 0, T >= 1, but a prologue needs T >= 64
    st = np.ones((B, dim // 16, 2), dtype=np.int64)
    gn = dict(x=A, stats=st, gamma=rng.standard_normal(dim).astype(np.float32), beta=rng.standard_normal(dim).astype(np.float32), G=8)
    cases = {"T = 0": dict(a=A, lens=LENS0, T=0), "M % T != 0": dict(a=A, lens=LENS0, T=T0 + 1), "T < 0": dict(a=A, lens=LENS0, T=-T0),
             "GroupNorm prologue at T = 60": dict(gn=gn, lens=[60] * B, T=T)}
    for name, kw in cases.items():
        rc, yb, zb, viol, _ = _launch(prec, dim, 1, M, **kw)
        msg = _lib()[1].ns2vc_last_error().decode()
        diag(f"masked rowchain refusal, {name}: status {rc} ({msg})")
        assert rc != 0, name
        assert not viol and np.all(yb == fill_y) and np.all(zb == fill_z), name
    rc, yb, zb, viol, _ = _launch(prec, dim, 1, M, a=A, lens=[60] * B, T=T)      # control: the plain form takes T = 60 (b is derived per lane)
    assert rc == 0 and not viol


# ---------------------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


def _engine(prec, weights, fuse=True, attn=True, rows=True):
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    e.set_option("masked_fuse", fuse)
    e.set_option("masked_attn", attn)
    e.set_option("masked_rows", rows)
    return e


def _zero_tails(y, lens, T):
    for b, L in enumerate(lens):
        assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0, (b, L)


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_masked_rows_forward_equals_items_alone(prec, weights, diag):
    lens = [131, 127, 66]
    T, Lp = 131, 40
    x, c, p, t = _inputs(len(lens), T, Lp, "mr1")
    for b, L in enumerate(lens):
        x[b, :, L:] = 7.0
        c[b, :, L:] = -3.0
    e = _engine(prec, weights)
    try:
        # every item's own batch-1 forward, once (dense plans ignore the three options)
        refs = [_forward(e, x[b:b + 1, :, :L].contiguous(), c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), t[b:b + 1].contiguous())
                for b, L in enumerate(lens)]
        for fuse in (False, True):
            for attn in (False, True):
                ys = {}
                for rows in (False, True):
                    e.set_option("masked_fuse", fuse)
                    e.set_option("masked_attn", attn)
                    e.set_option("masked_rows", rows)
                    ys[rows] = _forward(e, x, c, p, t, lens)
                    if rows:
                        assert len([n for n in _names(e) if ".rows[" in n]) > 0          # the option took effect in this plan
                y = ys[True]
                assert np.isfinite(y).all()
                _zero_tails(y, lens, T)
                worst = (0.0, 0.0)
                for b, L in enumerate(lens):
                    m = local_errors(y[b:b + 1, :, :L], refs[b])
                    worst = (max(worst[0], m["item"]), max(worst[1], m["frame"]))
                    diag(f"masked_rows forward {prec} masked_fuse={int(fuse)} masked_attn={int(attn)} L={L}: item {m['item']:.2e} frame {m['frame']:.2e} "
                         f"chan {m['chan']:.2e}")
                    assert m["item"] < _bar(TOL, prec), (fuse, attn, L, m)
                    assert m["frame"] < _bar(FRAME_TOL, prec) and m["chan"] < _bar(FRAME_TOL, prec), (fuse, attn, L, m)
                flip = rel_l2(ys[True], ys[False])
                diag(f"masked_rows forward {prec} masked_fuse={int(fuse)} masked_attn={int(attn)}: worst item {worst[0]:.2e} (bar {_bar(TOL, prec):.0e}), "
                     f"worst frame {worst[1]:.2e}; option on vs off {flip:.2e}")
                assert flip < 2e-3 * (_bar(TOL, prec) / TOL["fp16"])       # the flipped-option bar of test_every_plan_option_under_lengths (fp16)
    finally:
        e.close()


def test_masked_rows_sampled_on_vs_off(weights, diag):
    """the flipped-option bars through a short sampling loop, captured and eager"""
    import torch
    lens = [131, 127, 66]
    B, T, Lp = len(lens), 131, 40
    _, c, p, _ = _inputs(B, T, Lp, "mr1")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(5)).to(c.device)
    res = {}
    e = _engine("fp16", weights)
    try:
        for rows in (False, True):
            e.set_option("masked_rows", rows)
            res[rows] = (_sample(e, c, p, xT, lens, True), _sample(e, c, p, xT, lens, False))
    finally:
        e.close()
    eg, ee = (rel_l2(res[True][i], res[False][i]) for i in range(2))
    gve = rel_l2(res[True][0], res[True][1])
    diag(f"masked_rows on vs off under lengths fp16: sampled graph {eg:.2e} eager {ee:.2e}; graph vs eager {gve:.2e}")
    assert eg < 2e-3 and ee < 2e-3
    assert gve < 1e-6
    for y in res[True]:
        _zero_tails(y, lens, T)


def test_fp32_engine_ignores_the_option(weights, diag):
    lens = [131, 127, 66]
    T, Lp = 131, 40
    x, c, p, t = _inputs(len(lens), T, Lp, "mr1")
    e = _engine("fp32", weights, rows=False)
    try:
        y0 = _forward(e, x, c, p, t, lens)
        n0 = _names(e)
        e.set_option("masked_rows", True)
        y1 = _forward(e, x, c, p, t, lens)
        assert _names(e) == n0 and not [n for n in n0 if ".rows[" in n]
    finally:
        e.close()
    assert np.array_equal(y0, y1)
    _zero_tails(y1, lens, T)


CHAIN_NAMES = (".proj_in", ".norm1", ".attn1.qkv", ".attn1.to_out", ".norm2", ".attn2.to_q")


@pytest.mark.parametrize("T", [520, 300], ids=["levels_520_260_130_65", "levels_300_150_75_38"])
def test_masked_rows_launch_list(T, weights, diag):
    """with the option on, every transformer block whose dim is row-chain eligible (= that runs row chains in the dense plan) runs exactly its two
    row chains under lengths and none of the launches they replace, and its plan is at least 5 launches shorter.  T = 520: every level has 64
    frames or more; T = 300: the deepest level has 38 frames (the shape of test_fused_launch_list)."""
    B, Lp = 2, 40
    lens = [T, T - 169]
    got = {}
    e = _engine("fp16", weights, True, True, False)
    try:
        e.prepare(B, T, Lp)
        dense = _names(e)
        for fuse in (True, False):
            for rows in (False, True):
                e.set_option("masked_fuse", fuse)
                e.set_option("masked_rows", rows)
                e.prepare(B, T, Lp)
                assert _names(e) == dense                              # dense plans ignore the option
                e.set_lengths(lens)
                got[(fuse, rows)] = _names(e)
                e.set_lengths(None)
                assert _names(e) == dense
    finally:
        e.close()
    blocks = sorted({_block_of(n) for n in dense if ".rows[" in n})
    assert blocks
    for fuse in (True, False):
        off, on = got[(fuse, False)], got[(fuse, True)]
        assert not [n for n in off if ".rows[" in n]                   # today's fallback
        assert [n for n in on if _block_of(n) is None] == [n for n in off if _block_of(n) is None]       # nothing outside the blocks changes
        for P in blocks:
            was = [n for n in dense if _block_of(n) == P]
            b_off, b_on = [n for n in off if _block_of(n) == P], [n for n in on if _block_of(n) == P]
            chains = [n for n in b_on if ".rows[" in n]
            assert len(chains) == 2 and "attn1.to_out+attn2.to_q" in chains[1], (P, b_on)
            for n in b_on:
                assert not any(n.endswith(s) or n.endswith(s + ".mask") for s in CHAIN_NAMES), (P, n)
            assert not [n for n in b_on if ".rows[" in n and n.endswith(".mask")]
            gn_dense = any("rows[norm+proj_in+qkv]" in n for n in was)
            if fuse and gn_dense:
                assert "rows[norm+proj_in+qkv]" in chains[0], (P, chains)
            else:                                                      # no producer statistics under lengths (unfused), or a level under 64 frames
                assert "rows[proj_in+qkv]" in chains[0] and P + ".norm.gn_apply" in b_on, (P, b_on)
            # what stays exactly as it is: everything from attn2.sdpa on, and the self-attention launch
            tail = lambda names: names[[i for i, n in enumerate(names) if n.endswith(".attn2.sdpa")][0]:]
            assert tail(b_on) == tail(b_off), (P, tail(b_on), tail(b_off))
            saved = len(b_off) - len(b_on)
            diag(f"launches T={T} masked_fuse={int(fuse)} {P}: {len(b_off)} -> {len(b_on)} with masked_rows (dense {len(was)})")
            assert saved >= 5, (P, b_off, b_on)
        diag(f"launches T={T} masked_fuse={int(fuse)}: {len(off)} -> {len(on)} with masked_rows; dense {len(dense)}")


def test_masked_rows_graph_captured_under_other_lengths(weights, diag):
    """a UniPC loop of 4 steps captured under one set of lengths and replayed under another: graph == eager, every item == alone (2.5e-3, the
    sampled bar of test_sampled_padded_batch_equals_items_alone), dense before == dense after"""
    import torch
    B, T, Lp = 4, 256, 40
    _, c, p, _ = _inputs(B, T, Lp, "rg4")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(3)).to(c.device)
    A, Bl = [256, 200, 100, 9], [17, 256, 255, 64]
    e = _engine("fp16", weights)
    try:
        xd0 = torch.from_numpy(_sample(e, c, p, xT, None, True))
        _sample(e, c, p, xT, A, True)                                  # captured under A
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
        diag(f"masked_rows unipc-4 fp16 replayed under other lengths: graph == eager; worst item vs alone {worst:.2e} (bar 2.5e-3)")
        assert worst < 2.5e-3
    finally:
        e.close()
