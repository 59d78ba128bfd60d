"""The length-masked row-chain, feed-forward and GEGLU kernels (RowchainArgs.lens, FfnArgs.lens, GegluArgs.T / lens) under the length vectors of
tests/masked_matrix.py, kernel case by kernel case, through the C ABI (ctypes + numpy).  The vectors put an item's start and an item's first dead
row on every row of a 64- and of a 128-token block, and produce wholly dead blocks, blocks whose only live row is the first or the last, blocks
with a dead first row and live rows later, blocks of three and more items, a partial last block and counts outside 0 .. T (the census and why each
vector is there: masked_matrix.py; that the earlier single vector T0 = 130, LENS0 has 5 of the 64 end positions and 6 of the 64 start positions,
and which wrong kernels it lets through: tests/test_masked_matrix_cpu.py).

Every (kernel case, vector) is: the launch under `lens` twice -- NaN, then Inf in the dead rows of every input and around every tensor
(tests/guard.py) --, ONE reference launch, and the launch once more with one count changed across a block seam; masked_matrix.check_launch holds
them to the contract the three kernels share (its checks 1 - 7).  The reference is the compacted dense twin: a lane owns one token, so one dense
launch (lens = NULL) over the live rows of all items concatenated gives every live row's words and the same ln_health maximum -- row chain
M = sum L, feed-forward B = 1, T = M = sum L, GEGLU with ln_stats M = sum L.  Two forms have no such twin:
  GEGLU with ln_stats = NULL (the masked kernel only): bit for bit the masked kernel on the compacted rows (B = 1, T = lens[0] = sum L: no row is
  dead, no decision of the mask is left), which in turn is held to the dense kernel fed the LayerNorm sums of the rounded operand row under
  eps16 / GEGLU_FLIPS, the bars of test_masked_geglu_gpu.test_kernel_own_stats_equals_items_alone_and_fp64;
  the row chain with the GroupNorm prologue (T >= 64; the divisor is the item's own count): per item, the dense launch of the item alone at
  T = L for L >= 64 and the masked launch of the item alone (B = 1, same T, lens = [L]) under that, concatenated; item 0's rows also against numpy
  fp64 under TOL_ROWCHAIN_GN_Y / eps16.  Vectors: masked_matrix.GN_VECTORS.
The helpers (_launch, _weights, _rounded, _poison_rows, OUT_FILL) are those of tests/test_masked_rows_gpu.py, test_masked_ffn_gpu.py and
test_masked_geglu_gpu.py; the last test holds the (kernel case, vector) pairs that ran to a spelled-out table.

Bounds: TOL_STATS / HALF_Q (check 6, inside masked_matrix.py), eps16 / GEGLU_FLIPS and TOL_ROWCHAIN_GN_Y / eps16 as named above -- imported, nothing
of this file's own; everything else is bitwise.

Measured on an MI355X: all 42 kernel cases of EXPECTED with every vector of theirs (234 pairs, 24 of them the refused slices + residual pair): checks 1 - 5 and 7 bit for bit in every case -- no defect
found; check 6 (feed-forward statistics) at most 0.02 of its limit; GEGLU with its own sums vs the dense kernel fed the rounded row's sums: rel_l2
at most 0.08 eps16, at most 0.0013 of the words differ; GroupNorm form, item 0 vs fp64: y at most 7.6e-6 (bar 2e-5), z 0.84 - 0.89 eps16 (the
rounding of the fp16 result itself).  The file takes under 30 s."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard as G                                   # noqa: E402
import masked_matrix as MM                          # noqa: E402
import test_masked_ffn_gpu as FF                    # noqa: E402
import test_masked_geglu_gpu as GG                  # noqa: E402
import test_masked_rows_gpu as RC                   # noqa: E402
from test_masked_rows_gpu import GN_SQ_SCALE, GN_SUM_SCALE, OUT_FILL, PREC_IDS, _poison_rows, _rounded      # noqa: E402
from test_ragged_fused_gpu import _stats_ref       # noqa: E402
from util import GEGLU_FLIPS, TOL_ROWCHAIN_GN_Y, eps16, rel_l2          # noqa: E402

pytestmark = pytest.mark.gpu

MMAX = max(len(lens) * T for T, lens in MM.VECTORS.values())
FILLS = (("nan", np.nan), ("inf", np.inf))
RAN = {}                      # kernel case id -> vectors that ran to the end of their checks


def _fill_word(kind):
    return G.encode(np.full(1, OUT_FILL, np.float32), kind)[0]


def _vec(vec, table=MM.VECTORS):
    T, lens = table[vec]
    return T, lens, MM.clamped(T, lens), len(lens), len(lens) * T


def _changed(T, lens, W):
    cb, cL = MM.seam_change(T, lens, W)
    lens2 = list(lens)
    lens2[cb] = cL
    return cb, cL, lens2, MM.clamped(T, lens2)


def _finish(case, vec, rec, diag, extra=""):
    diag(f"masked matrix {case} [{vec}]: {len(rec)} violation(s){extra}")
    assert not rec, [r["text"] for r in rec[:6]]
    RAN.setdefault(case, set()).add(vec)


# ---------------------------------------------------------------------------------------------------------------------------------
# row chain, plain form
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rc_pool(dim):
    rng = np.random.default_rng(3100 + dim)
    A = rng.standard_normal((MMAX, dim)).astype(np.float32)
    R = (rng.standard_normal((MMAX, dim)) + 1.5 * rng.standard_normal((MMAX, 1))).astype(np.float32)
    return A, R


def _rc_id(p, d, m, n, s, r):
    return f"{PREC_IDS[p]}-dim{d}-n2x{m}-nt{n}-slices{s}-{'inplace_res' if r else 'nores'}"


def _rc_run(prec, dim, mult, nt, slices, res, M, A, R, **kw):
    rc, yb, zb, viol, h = RC._launch(prec, dim, mult, M, a=A, res=R if res else None, inplace=res, nt=nt, slices=slices, **kw)
    return dict(status=rc, outs=dict(out1_f32=yb, out2_op=zb), viol=viol, health=h)


@pytest.mark.parametrize("prec,dim,mult,nt,slices,res", RC.PLAIN_CASES, ids=[_rc_id(*c) for c in RC.PLAIN_CASES])
def test_rowchain_plain(prec, dim, mult, nt, slices, res, diag):
    case = "rowchain " + _rc_id(prec, dim, mult, nt, slices, res)
    W = 64 * nt
    zfill = _fill_word(G.OP_KIND[prec])
    for vec in MM.KERNEL_VECTORS["rowchain"][0]:
        T, lens, lc, B, M = _vec(vec)
        A, R = (a[:M] for a in _rc_pool(dim))
        if slices and res:
            # two slices would race on y: refused with lengths as without, and nothing is stored
            run = _rc_run(prec, dim, mult, nt, slices, res, M, A, R, lens=lens, T=T)
            assert run["status"] != 0 and not run["viol"], (case, vec)
            assert np.array_equal(run["outs"]["out1_f32"], G.encode(R, "f32").reshape(M, dim)) and np.all(run["outs"]["out2_op"] == zfill), (case, vec)
            RAN.setdefault(case, set()).add(vec)
            continue
        masked = {fill: _rc_run(prec, dim, mult, nt, slices, res, M, _poison_rows(A, B, T, lc, bad), _poison_rows(R, B, T, lc, bad), lens=lens, T=T,
                                fill=fill) for fill, bad in FILLS}
        live = MM.live_rows(T, lens)
        ref = _rc_run(prec, dim, mult, nt, slices, res, int(live.sum()), A[live], R[live])
        assert ref["status"] == 0 and not ref["viol"], (case, vec, ref["viol"], RC._lib()[1].ns2vc_last_error())
        cb, cL, lens2, lc2 = _changed(T, lens, W)
        run2 = _rc_run(prec, dim, mult, nt, slices, res, M, _poison_rows(A, B, T, lc2, np.nan), _poison_rows(R, B, T, lc2, np.nan), lens=lens2, T=T)
        pre_y = G.encode(_poison_rows(R, B, T, lc, np.nan), "f32").reshape(M, dim) if res else _fill_word("f32")
        rec = MM.check_launch(case, vec, T, lens, masked, ref, out_fill=dict(out1_f32=pre_y, out2_op=zfill), W=W, changed=(cb, cL, run2))
        _finish(case, vec, rec, diag, f"; ln_health {masked['nan']['health']!r}")


# ---------------------------------------------------------------------------------------------------------------------------------
# row chain, GroupNorm-prologue form
# ---------------------------------------------------------------------------------------------------------------------------------
GN_DIM, GN_PREC = 256, 2
GN_CASES = [(Gn, mult) for Gn in (8, 4) for mult in (1, 3)]


@functools.lru_cache(maxsize=None)
def _gn_pool(vec):
    T, lens, lc, B, M = _vec(vec, MM.GN_VECTORS)
    rng = np.random.default_rng(3900 + M)
    x = (rng.standard_normal((B, T, GN_DIM)) * (1.0 + rng.random((B, 1, GN_DIM))) + rng.standard_normal((B, 1, GN_DIM))).astype(np.float32).reshape(M, GN_DIM)
    gam, bet = (1.0 + 0.2 * rng.standard_normal(GN_DIM)).astype(np.float32), (0.2 * rng.standard_normal(GN_DIM)).astype(np.float32)
    return x, gam, bet


def _gn_stats(x, B, T, lc):
    """the statistics as the masked conv epilogue leaves them: int64 fixed point over the valid rows only"""
    sr = _stats_ref(x, B, T, lc)
    return np.stack([np.rint(sr[..., 0] * GN_SUM_SCALE), np.rint(sr[..., 1] * GN_SQ_SCALE)], axis=-1).astype(np.int64)


def _gn_run(mult, M, gn, **kw):
    rc, yb, zb, viol, h = RC._launch(GN_PREC, GN_DIM, mult, M, gn=gn, **kw)
    return dict(status=rc, outs=dict(out1_f32=yb, out2_op=zb), viol=viol, health=h)


def _gn_fp64(x0, Gn, mult, gam, bet):
    """numpy fp64 of the item's rows with the kernel's rounding points (GroupNorm over the item's own rows, as test_rowchain_groupnorm_prologue)"""
    w = RC._weights(GN_DIM, mult, GN_PREC, 0)
    L, d = x0.shape
    xg = x0.astype(np.float64).reshape(L, Gn, d // Gn)
    mean, var = xg.mean(axis=(0, 2), keepdims=True), xg.var(axis=(0, 2), keepdims=True)
    a = ((xg - mean) / np.sqrt(var + 1e-6)).reshape(L, d) * gam.astype(np.float64) + bet.astype(np.float64)
    y = _rounded(a.astype(np.float32), GN_PREC) @ _rounded(w["W1"], GN_PREC).T + w["b1"].astype(np.float64)[None, :]
    yr = _rounded(y.astype(np.float32), GN_PREC)
    z = (yr @ _rounded(w["W2f"], GN_PREC).T - y.mean(1, keepdims=True) * w["consts"][:, 0].astype(np.float64)[None, :]) / \
        np.sqrt(y.var(1, keepdims=True) + 1e-5) + w["b2f"].astype(np.float64)[None, :]
    return y, z


@pytest.mark.parametrize("Gn,mult", GN_CASES, ids=[f"G{g}-n2x{m}" for g, m in GN_CASES])
def test_rowchain_groupnorm(Gn, mult, diag):
    case = f"rowchain+GroupNorm fp16-dim{GN_DIM}-G{Gn}-n2x{mult}"
    n2 = mult * GN_DIM
    for vec in MM.GN_VECTORS:
        T, lens, lc, B, M = _vec(vec, MM.GN_VECTORS)
        x, gam, bet = _gn_pool(vec)
        st = _gn_stats(x, B, T, lc)
        gn = lambda xx, ss: dict(x=xx, stats=ss, gamma=gam, beta=bet, G=Gn)      # noqa: E731
        masked = {fill: _gn_run(mult, M, gn(_poison_rows(x, B, T, lc, bad), st), lens=lens, T=T, fill=fill) for fill, bad in FILLS}
        outs, health = dict(out1_f32=[], out2_op=[]), 0.0
        for b, L in enumerate(lc):
            if L == 0:
                continue
            if L >= 64:             # the dense launch of the item alone at T = L
                one = _gn_run(mult, L, gn(x[b * T:b * T + L], st[b:b + 1]), T=L)
            else:                   # under the prologue's 64-frame minimum: the masked launch of the item alone, same T
                one = _gn_run(mult, T, gn(_poison_rows(x[b * T:(b + 1) * T], 1, T, [L], np.nan), st[b:b + 1]), lens=[L], T=T)
                assert not one["outs"]["out1_f32"][L:].any() and not one["outs"]["out2_op"][L:].any(), (case, vec, b)
            assert one["status"] == 0 and not one["viol"], (case, vec, b, one["viol"], RC._lib()[1].ns2vc_last_error())
            for k in outs:
                outs[k].append(one["outs"][k][:L])
            health = max(health, one["health"])
            if b == 0:
                y, z = _gn_fp64(x[:L], Gn, mult, gam, bet)
                e_y = rel_l2(G.decode(one["outs"]["out1_f32"][:L].reshape(-1), "f32").reshape(L, GN_DIM), y)
                e_z = rel_l2(G.decode(one["outs"]["out2_op"][:L].reshape(-1), "f16").reshape(L, n2), z)
                diag(f"masked matrix {case} [{vec}]: item 0 (L = {L}) vs fp64 y {e_y:.2e} (bar {TOL_ROWCHAIN_GN_Y:.0e}) z {e_z:.2e} (bar {eps16(GN_PREC):.1e})")
                assert e_y < TOL_ROWCHAIN_GN_Y and e_z < eps16(GN_PREC), (case, vec, e_y, e_z)
        ref = dict(outs={k: np.concatenate(v) for k, v in outs.items()}, health=health)
        cb, cL, lens2, lc2 = _changed(T, lens, 64)
        run2 = _gn_run(mult, M, gn(_poison_rows(x, B, T, lc2, np.nan), _gn_stats(x, B, T, lc2)), lens=lens2, T=T)
        rec = MM.check_launch(case, vec, T, lens, masked, ref, out_fill=dict(out1_f32=_fill_word("f32"), out2_op=_fill_word("f16")), W=64,
                              changed=(cb, cL, run2), changed_item_rows=False)
        _finish(case, vec, rec, diag, f"; ln_health {masked['nan']['health']!r}")


# ---------------------------------------------------------------------------------------------------------------------------------
# fused feed-forward
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _ff_pool(dim):
    rng = np.random.default_rng(4100 + dim)
    o = rng.standard_normal((MMAX, dim)).astype(np.float32)
    y = (rng.standard_normal((MMAX, dim)) + 1.5 * rng.standard_normal((MMAX, 1))).astype(np.float32)
    x = rng.standard_normal((MMAX, dim)).astype(np.float32)
    ys = y.astype(np.float64).reshape(MMAX, dim // 64, 64)
    st = np.stack([ys.sum(2), (ys ** 2).sum(2)], axis=-1).astype(np.float32).reshape(MMAX, dim // 64 * 2)
    return dict(o=o, y=y, x=x, st=st)


def _ff_id(p, d, s):
    return f"{PREC_IDS[p]}-dim{d}-{'pre' if s else 'plain'}"


def _ff_run(prec, dim, pre, B, T, rows, **kw):
    rc, ob, pb, st, viol, h = FF._launch(prec, dim, pre, B, T, rows, **kw)
    return dict(status=rc, outs=dict(out_f32=ob, out_op=pb), viol=viol, health=h, stats=st)


@pytest.mark.parametrize("prec,dim,pre", FF.KERNEL_CASES, ids=[_ff_id(*c) for c in FF.KERNEL_CASES])
def test_ffn(prec, dim, pre, diag):
    case = "ffn " + _ff_id(prec, dim, pre)
    for vec in MM.KERNEL_VECTORS["ffn"][0]:
        T, lens, lc, B, M = _vec(vec)
        P = {k: v[:M] for k, v in _ff_pool(dim).items()}
        masked = {fill: _ff_run(prec, dim, pre, B, T, {k: _poison_rows(v, B, T, lc, bad) for k, v in P.items()}, lens=lens, fill=fill) for fill, bad in FILLS}
        live = MM.live_rows(T, lens)
        ref = _ff_run(prec, dim, pre, 1, int(live.sum()), {k: v[live] for k, v in P.items()})
        assert ref["status"] == 0 and not ref["viol"], (case, vec, ref["viol"], FF._lib()[1].ns2vc_last_error())
        cb, cL, lens2, lc2 = _changed(T, lens, 64)
        run2 = _ff_run(prec, dim, pre, B, T, {k: _poison_rows(v, B, T, lc2, np.nan) for k, v in P.items()}, lens=lens2)
        rec = MM.check_launch(case, vec, T, lens, masked, ref, out_fill=dict(out_f32=_fill_word("f32"), out_op=_fill_word(G.OP_KIND[prec])), W=64,
                              changed=(cb, cL, run2), stats_from="out_f32")
        worst = MM.stats_figures(T, lens, masked["nan"], "out_f32") if masked["nan"]["status"] == 0 else (np.nan, np.nan)
        _finish(case, vec, rec, diag, f"; stats error / limit of check 6: sum {worst[0]:.3f} sumsq {worst[1]:.3f}; ln_health {masked['nan']['health']!r}")


# ---------------------------------------------------------------------------------------------------------------------------------
# token-stationary GEGLU
# ---------------------------------------------------------------------------------------------------------------------------------
GG_CASES = [(prec, own, extra) for prec in (1, 2) for own in (False, True) for extra in (0, 64)]


@functools.lru_cache(maxsize=None)
def _gg_pool():
    rng = np.random.default_rng(5100)
    y = (rng.standard_normal((MMAX, GG.D)) + 1.5 * rng.standard_normal((MMAX, 1))).astype(np.float32)
    return y, _gg_sums(y.astype(np.float64))


def _gg_sums(y64):
    """LayerNorm-by-linearity statistics rows as a producer GEMM's `rowstats` leaves them: (sum, sum of squares) per 64 channels"""
    ys = y64.reshape(len(y64), GG.D // 64, 64)
    return np.stack([ys.sum(2), (ys ** 2).sum(2)], axis=-1).astype(np.float32).reshape(len(y64), GG.D // 64 * 2)


def _gg_id(p, own, extra):
    return f"{PREC_IDS[p]}-{'own_sums' if own else 'ln_stats'}-ldo+{extra}"


def _gg_run(prec, M, y, st, **kw):
    rc, bits, viol, h = GG._launch(prec, M, y, st, **kw)
    return dict(status=rc, outs=dict(out_op=bits), viol=viol, health=h)


@pytest.mark.parametrize("prec,own,extra", GG_CASES, ids=[_gg_id(*c) for c in GG_CASES])
def test_geglu(prec, own, extra, diag):
    case = "geglu " + _gg_id(prec, own, extra)
    kind = G.OP_KIND[prec]
    for vec in MM.KERNEL_VECTORS["geglu"][0]:
        T, lens, lc, B, M = _vec(vec)
        y, st = (a[:M] for a in _gg_pool())
        sts = lambda c, bad: None if own else _poison_rows(st, B, T, c, bad)      # noqa: E731
        masked = {fill: _gg_run(prec, M, _poison_rows(y, B, T, lc, bad), sts(lc, bad), T=T, lens=lens, fill=fill, ldo_extra=extra) for fill, bad in FILLS}
        live = MM.live_rows(T, lens)
        n = int(live.sum())
        note = ""
        if own:
            # no dense form: the masked kernel on the compacted rows, where no row is dead, ...
            ref = _gg_run(prec, n, y[live], None, T=n, lens=[n], ldo_extra=extra)
            # ... held to the dense kernel fed the sums of the rounded operand row (what the masked kernel takes them from)
            dense = _gg_run(prec, n, y[live], _gg_sums(_rounded(y[live], prec)), ldo_extra=extra)
            assert dense["status"] == 0 and not dense["viol"], (case, vec, dense["viol"])
            a, d = (G.decode(r["outs"]["out_op"].reshape(-1), kind).reshape(n, 4 * GG.D).astype(np.float64) for r in (ref, dense))
            e, flips = rel_l2(a, d), float(np.mean(ref["outs"]["out_op"] != dense["outs"]["out_op"]))
            note = f"; own sums vs the dense kernel fed the rounded row's sums: rel_l2 {e:.3e} (bar {eps16(prec):.1e}) flips {flips:.4f} (bar {GEGLU_FLIPS})"
            assert np.isfinite(a).all() and e < eps16(prec) and flips < GEGLU_FLIPS, (case, vec, e, flips)
        else:
            ref = _gg_run(prec, n, y[live], st[live], ldo_extra=extra)
        assert ref["status"] == 0 and not ref["viol"], (case, vec, ref["viol"], GG._lib()[1].ns2vc_last_error())
        cb, cL, lens2, lc2 = _changed(T, lens, 128)
        run2 = _gg_run(prec, M, _poison_rows(y, B, T, lc2, np.nan), sts(lc2, np.nan), T=T, lens=lens2, ldo_extra=extra)
        rec = MM.check_launch(case, vec, T, lens, masked, ref, out_fill=dict(out_op=_fill_word(kind)), W=128, changed=(cb, cL, run2))
        _finish(case, vec, rec, diag, note + f"; ln_health {masked['nan']['health']!r}")


# ---------------------------------------------------------------------------------------------------------------------------------
# what must have run: spelled out, not derived from the parametrisations above
# ---------------------------------------------------------------------------------------------------------------------------------
_ALL6 = {"V65", "VDEAD", "VSHORT", "VCLAMP", "VLONG", "VLAST"}
_T64 = {"V65", "VDEAD", "VCLAMP", "VLONG", "VLAST"}
_GN = {"V65x24", "VDEAD", "VCLAMP"}
EXPECTED = {}
EXPECTED.update({f"rowchain fp16-dim128-n2x{m}-nt{n}-slices0-{r}": _ALL6 for m in (1, 3) for n in (1, 2) for r in ("nores", "inplace_res")})
EXPECTED.update({f"rowchain {p}-dim256-n2x{m}-nt1-slices0-{r}": _ALL6 for p in ("fp16", "bf16") for m in (1, 3) for r in ("nores", "inplace_res")})
EXPECTED.update({f"rowchain fp16-dim384-n2x{m}-nt1-slices{s}-{r}": _ALL6 for m in (1, 3) for s in (0, 2) for r in ("nores", "inplace_res")})
EXPECTED.update({f"rowchain+GroupNorm fp16-dim256-G{g}-n2x{m}": _GN for g in (8, 4) for m in (1, 3)})
EXPECTED.update({f"ffn {c}": _T64 for c in ("fp16-dim128-pre", "fp16-dim128-plain", "fp16-dim256-pre", "fp16-dim256-plain", "bf16-dim256-pre", "bf16-dim256-plain")})
EXPECTED.update({f"geglu {p}-{s}-ldo+{x}": _ALL6 for p in ("bf16", "fp16") for s in ("ln_stats", "own_sums") for x in (0, 64)})


def test_every_pair_of_the_table_ran():
    """(last in the file) a parametrisation that was dropped, or a vector a case did not reach, fails here"""
    assert len(EXPECTED) == 24 + 4 + 6 + 8
    gone = {c: sorted(v - RAN.get(c, set())) for c, v in EXPECTED.items() if v - RAN.get(c, set())}
    assert not gone, gone
    assert set(RAN) == set(EXPECTED), sorted(set(RAN) ^ set(EXPECTED))
