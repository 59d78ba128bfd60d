"""Which key, row, head and item every attention output came from, read off the output itself (patterns: tests/attn_patterns.py; their validity and
what they catch: tests/test_attn_positions_cpu.py).

attn_kernel.  All 40 rows of the table (built from attn_patterns.attn_table_rows, which restates the table's own macros; the count is asserted
against ns2vc_debug_kernel_table), each at B = 3, H = 5, Lq = 200 (30 workgroups: the remainder branch of the XCD remap; two query blocks with a
tail) with Lk 65 and 200, the Lk = 469 cross case under a bias mask, and -- the masked instantiations -- q_lens [200, 129, 1] with the k_lens
launches of attn_patterns.K_LENS.  COUNT runs at every shape with the optimistic pass on and off.  ROUTE runs
    fp32 rows            gaps 11.5, 12.5 (THRESH -+ 0.5: whether the reference moves), 40 (a key that dominates outright)
    fp8 PV rows          gaps 7.5, 8.5 (THRESH is 8 there), 40
    other 16-bit rows    (a) AttnArgs.exact_only = 1 at gaps 11.5, 12.5, 19, 40
                         (b) optimistic pass at gap 17: p = 2^13 under the acceptance limit 2^14 (margin 4): the fallback counter reads 0
                         (c) optimistic pass at gaps 19 and 40: p = 2^15 and beyond, rejected: the counter equals the live workgroups and the bits
                             are those of (a).  At the shapes of attn_patterns.REJECT_CASES, where every live workgroup holds a row whose match lies
                             behind the first key tile (a 65-key launch under 128-key tiles has one tile and nothing to reject).
Every launch is on guarded tensors (no violation), finite, exact zeros past q_lens.  Bounds: tol_attn_count, tol_attn_route (tests/util.py).

ffn_kernel's in-kernel cross-attention (32-key tiles on ns2vc_k_xattn_pack's k | v image): dim 128 / 256, bf16 / fp16, B = 2, T = 70,
Lk in {1, 31, 32, 33, 69} with and without a bias mask.  ns2vc_pack_ffn_pre takes plain matrices, so the identity path exists: Wo = I, W1 = 0 (the
hidden tensor is GEGLU(0) = 0 whatever the LayerNorm row is), the y columns of W2 = I, zero biases and residuals -- the fused output IS the attention
output and decodes like the attention kernel's.  COUNT (V scaled by Lk so that the result is O(1)) and ROUTE run through the fused launch and through
the two-launch path (ns2vc_k_attention into pre_a) on the same data; both decode, and row by row max |fused - two-launch| / RMS(row) stays under the
file's fused-vs-two-launch bound (TOL_FFN_XATTN_ROW).  The ROUTE gaps are 24 and 40: this attention takes the row maximum in a pass of its own and has
no threshold to straddle, and at these gaps the non-matching mass (under 2^-20) cannot move a 16-bit result across a rounding boundary, so the two
paths may differ by nothing the bound has to absorb.  With V = 0 both outputs must be exact zeros (a K-image defect alone cannot produce
anything else but a non-finite row: it separates the two images when something fails)."""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_patterns as P                           # noqa: E402
import guard as G                                   # noqa: E402
from attn_launch import PREC_IDS, _launch, _lib, _vals      # noqa: E402
from util import TOL_FFN_XATTN_ROW, tol_attn_count, tol_attn_route      # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = P.attn_table_rows()
GAPS_EXACT = (11.5, 12.5, 19.0, 40.0)
GAP_ACCEPT, GAPS_REJECT = 17.0, (19.0, 40.0)
GAPS_FP32 = (11.5, 12.5, 40.0)
GAPS_FP8 = (7.5, 8.5, 40.0)
GAPS_FFN = (24.0, 40.0)


def _row_id(r):
    prec, hd, keys, fp8, masked = r
    return f"{PREC_IDS[prec]}-hd{hd}-keys{keys}{'-fp8' if fp8 else ''}-{'masked' if masked else 'dense'}"


@functools.lru_cache(maxsize=None)
def _cases(masked, tile):
    return P.attn_cases(masked, tile)


@functools.lru_cache(maxsize=None)
def _count_data(masked, tile, name, hd):
    return P.build_count(_cases(masked, tile)[name], hd)


@functools.lru_cache(maxsize=None)
def _route_data(masked, tile, name, hd, gap, prec):
    """the tensors and the fp64 attention of the rounded operands: computed once, shared by the passes, left unchanged"""
    case = _cases(masked, tile)[name]
    q, k, v, sets, want = P.build_route(case, hd, gap, prec)
    qr, kr, vr = (P.round_op(t, prec) for t in (q, k, v))
    lo, hi, _, _ = P.realised_gaps(qr, kr, case, hd, sets)
    return q, k, v, want, P.attend(qr, kr, vr, case, hd), max(abs(lo - gap), abs(hi - gap))


def _run(case, prec, hd, keys, fp8, q, k, v, **kw):
    rc, bits, viol, nfb = _launch(prec, hd, q, k, v, H=case.H, bias=case.bias(), q_lens=case.q_lens, k_lens=case.k_lens, keys=keys, pv_fp8=fp8, **kw)
    assert rc == 0, _lib()[1].ns2vc_last_error()
    assert not viol, viol
    out = _vals(bits, prec)
    assert np.isfinite(out).all()
    for b in range(case.B):
        assert not bits[b, case.nq(b):].any(), b                                # exact zeros past q_lens: every storage word 0
    return bits, out, nfb


def test_the_matrix_is_the_table():
    assert len(ROWS) == len(set(ROWS)) == 40
    n = C.c_int(-1)
    assert _lib()[1].ns2vc_debug_kernel_table(3, C.byref(n), None) == 0 and n.value == 40


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_count(row, diag):
    prec, hd, keys, fp8, masked = row
    two_pass = prec != 0 and not fp8
    worst, t0, n = 0.0, time.time(), 0
    for name, case in _cases(masked, keys).items():
        q, k, v, sets = _count_data(masked, keys, name, hd)
        for opt in ((1, 0) if two_pass else (1,)):
            _, out, nfb = _run(case, prec, hd, keys, fp8, q, k, v, optimistic=opt, count=True)
            err, nonzero, bad, ratio = P.check_count(out, case, hd, sets, tol=lambda m: tol_attn_count(prec, m))
            worst = max(worst, err)
            n += 1
            assert nonzero == 0 and ratio <= 1.0, (name, opt, err, nonzero, bad)
            assert nfb == 0, (name, opt, nfb)
    diag(f"attention COUNT {_row_id(row)}: {n} launches, worst |out n - 1| {worst:.2e} (bar 2 eps + n 2^-23 = {tol_attn_count(prec, 65):.2e} at n = 65), "
         f"excluded positions exact zeros, {time.time() - t0:.1f} s")


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_route(row, diag):
    prec, hd, keys, fp8, masked = row
    two_pass = prec != 0 and not fp8
    cases = _cases(masked, keys)
    worst, t0, n, off = (0.0, 0.0, ""), time.time(), 0, 0.0
    passes = []

    def one(name, gap, **kw):
        nonlocal worst, n, off
        case = cases[name]
        q, k, v, want, ref, goff = _route_data(masked, keys, name, hd, gap, prec)
        off = max(off, goff)
        bits, out, nfb = _run(case, prec, hd, keys, fp8, q, k, v, count=True, **kw)
        wrong, dev, bad = P.check_route(out, case, hd, want)
        err = float(np.abs(out - ref).max())
        tol = tol_attn_route(prec, bool(fp8), case.Lk)
        worst = max(worst, (err / tol, err, f"{name} gap {gap:g}"))
        n += 1
        assert wrong == 0, (name, gap, kw, wrong, bad)
        assert err <= tol, (name, gap, kw, err, tol)
        return bits, nfb

    if not two_pass:
        for name in cases:
            for gap in (GAPS_FP8 if fp8 else GAPS_FP32):
                _, nfb = one(name, gap)
                assert nfb == 0
    else:
        exact = {}
        for name in cases:                                        # (a)
            for gap in GAPS_EXACT:
                exact[(name, gap)], nfb = one(name, gap, exact_only=1)
                assert nfb == 0, (name, gap, nfb)
        passes.append(f"(a) exact_only {len(exact)} launches, fallbacks 0")
        for name in cases:                                        # (b)
            _, nfb = one(name, GAP_ACCEPT)
            assert nfb == 0, (name, nfb)
        passes.append(f"(b) optimistic accepted at gap {GAP_ACCEPT:g}: {len(cases)} launches, fallbacks 0")
        seen = []
        for name in P.REJECT_CASES[masked]:                       # (c)
            live = cases[name].live_workgroups()
            for gap in GAPS_REJECT:
                bits, nfb = one(name, gap)
                seen.append(f"{nfb}/{live}")
                assert nfb == live, (name, gap, nfb, live)
                assert np.array_equal(bits, exact[(name, gap)]), (name, gap, int((bits != exact[(name, gap)]).sum()))
        passes.append(f"(c) optimistic rejected at gaps {GAPS_REJECT}: fallbacks / live workgroups {' '.join(seen)}, bits equal (a)")
    diag(f"attention ROUTE {_row_id(row)}: {n} launches, every row decodes to (its key, head, item), worst |out - fp64| {worst[1]:.2e} = "
         f"{worst[0]:.2f} of its bar ({worst[2]}), realised gaps within {off:.2f} of the wanted ones" + "".join("; " + p for p in passes) + f", {time.time() - t0:.1f} s")


# ---------------------------------------------------------------------------------------------------------------------------------
# the in-kernel cross-attention of ffn_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
class _Op:
    """device tensor in a 16-bit operand type"""

    def __init__(self, a, prec):
        from ns2vc_amd.engine import DevBuf
        self.kind, self.shape = G.OP_KIND[prec], a.shape
        self.buf = DevBuf.from_numpy(np.ascontiguousarray(G.encode(a, self.kind)))
        self.ptr = self.buf.ptr


def _f32(a):
    from ns2vc_amd.engine import DevBuf
    return DevBuf.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


@functools.lru_cache(maxsize=None)
def _identity_stream(d, prec):
    """ns2vc_pack_ffn_pre of Wo = I, W1 = 0, W2 = [0 | I]: out = y = the attention rows (kept for the session: four small weight streams)"""
    L, lib = _lib()
    W1p = np.zeros((8 * d, d), np.float32)
    w2f = np.concatenate([np.zeros((d, 4 * d), np.float32), np.eye(d, dtype=np.float32)], axis=1)
    Wo = np.eye(d, dtype=np.float32)
    stream = C.c_void_p()
    L.check(lib.ns2vc_pack_ffn_pre(np.ascontiguousarray(W1p).ctypes.data, np.ascontiguousarray(w2f).ctypes.data, np.ascontiguousarray(Wo).ctypes.data,
                                   d, prec, C.byref(stream)), "pack_ffn_pre")
    return stream


def _ffn_pair(case, d, prec, q, k, v):
    """-> (fused, two-launch) fp32 outputs (B, T, d) of ns2vc_k_ffn on the identity weights, zero pre_res / pre_bias / res / bias2"""
    from ns2vc_amd.engine import DevBuf, sync
    L, lib = _lib()
    B, T, Lk, H = case.B, case.Lq, case.Lk, case.H
    M, hd = B * T, d // H
    kv_ld = 2 * d + 64                                             # k | v side by side inside wider rows, as in the engine's hoisted projection
    kv = np.zeros((B, Lk, kv_ld), np.float32)
    kv[..., :d], kv[..., d:2 * d] = k, v
    d_q, d_kv = _Op(q.reshape(M, d), prec), _Op(kv.reshape(B * Lk, kv_ld), prec)
    bias = case.bias()
    d_bias = _f32(bias) if bias is not None else None
    d_vt = DevBuf(int(lib.ns2vc_xattn_pack_bytes(B, Lk, hd)))
    L.check(lib.ns2vc_k_xattn_pack(d_kv.ptr, kv_ld, d_kv.ptr + 2 * d, kv_ld, B, Lk, hd, d_vt.ptr, prec, None), "xattn_pack")
    d_c, d_b2, d_x, d_bo, d_yp = _f32(np.zeros((8 * d, 2))), _f32(np.zeros(d)), _f32(np.zeros((M, d))), _f32(np.zeros(d)), _f32(np.zeros((M, d)))
    outs = []
    for fused in (1, 0):
        d_o = _f32(np.full((M, d), np.nan))
        d_gs = DevBuf.from_numpy(np.zeros((B, d // 16, 2), dtype=np.int64))
        f = L.FfnArgs()
        f.wstream = _identity_stream(d, prec).value; f.consts = d_c.ptr; f.bias2 = d_b2.ptr
        f.res = d_x.ptr; f.ldres = d
        f.out_f32 = d_o.ptr; f.ldo_f32 = d
        f.stats = d_gs.ptr
        f.B, f.T, f.M, f.dim = B, T, M, d
        f.ln_eps = 1e-5
        f.pre_bias = d_bo.ptr; f.pre_res = d_yp.ptr; f.pre_ldres = d
        if fused:
            f.att_q = d_q.ptr; f.att_ldq = d; f.att_kv = d_vt.ptr
            f.att_bias = d_bias.ptr if d_bias is not None else None
            f.att_scale = 1.0 / np.sqrt(hd); f.att_Lk = Lk
        else:
            d_ao = _Op(np.full((M, d), np.nan, dtype=np.float32), prec)
            a = L.AttnArgs()
            a.q = d_q.ptr; a.k = d_kv.ptr; a.v = d_kv.ptr + 2 * d; a.ldq = d; a.ldk = kv_ld; a.ldv = kv_ld
            a.B, a.H, a.Lq, a.Lk = B, H, T, Lk
            a.bias = d_bias.ptr if d_bias is not None else None
            a.scale = 1.0 / np.sqrt(hd); a.out = d_ao.ptr; a.ldo = d
            L.check(lib.ns2vc_k_attention(C.byref(a), hd, prec, None), "k_attention")
            f.pre_a = d_ao.ptr; f.pre_lda = d
        L.check(lib.ns2vc_k_ffn(C.byref(f), prec, None), "k_ffn")
        sync()
        outs.append(d_o.to_numpy((M, d)).astype(np.float64).reshape(B, T, d))
    return outs


def _row_gap(fused, two):
    """max over rows of max |fused - two-launch| / RMS(row of the two-launch output); rows that are zero on both sides count 0, on one side inf"""
    diff = np.abs(fused - two).max(-1)
    rms = np.sqrt((two * two).mean(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(diff == 0, 0.0, diff / rms)
    return float(np.nan_to_num(r, nan=np.inf).max())


FFN_CASES = [(prec, dim, Lk, mk) for prec in (1, 2) for dim in (128, 256) for Lk in P.LK_FFN for mk in (0, 1)]


@pytest.mark.parametrize("prec,dim,Lk,mk", FFN_CASES, ids=[f"{PREC_IDS[p]}-dim{d}-Lk{k}-{'bias' if m else 'nobias'}" for p, d, k, m in FFN_CASES])
def test_ffn_cross_attention_positions(prec, dim, Lk, mk, diag):
    case = P.ffn_cases()[(Lk, mk)]
    hd = dim // case.H
    bar = TOL_FFN_XATTN_ROW[prec]
    # ---- COUNT, V scaled by Lk
    q, k, v, sets = P.build_count(case, hd, vamp=float(Lk))
    fused, two = _ffn_pair(case, dim, prec, q, k, v)
    assert np.isfinite(fused).all() and np.isfinite(two).all()
    worst_c = 0.0
    for nm, o in (("fused", fused), ("two-launch", two)):
        err, nonzero, bad, ratio = P.check_count(o, case, hd, sets, vamp=float(Lk), tol=lambda m: tol_attn_count(prec, m))
        worst_c = max(worst_c, err)
        assert nonzero == 0 and ratio <= 1.0, (nm, err, nonzero, bad)
    g_c = _row_gap(fused, two)
    assert g_c <= bar, ("COUNT fused vs two-launch", g_c)
    # ---- K only: with V = 0 both paths give exact zeros
    f0, t0 = _ffn_pair(case, dim, prec, q, k, np.zeros_like(v))
    assert not f0.any() and not t0.any()
    # ---- ROUTE
    worst_r, g_r = 0.0, 0.0
    for gap in GAPS_FFN:
        q, k, v, _, want = P.build_route(case, hd, gap, prec)
        ref = P.attend(*(P.round_op(t, prec) for t in (q, k, v)), case, hd)
        fused, two = _ffn_pair(case, dim, prec, q, k, v)
        assert np.isfinite(fused).all() and np.isfinite(two).all()
        for nm, o in (("fused", fused), ("two-launch", two)):
            wrong, dev, bad = P.check_route(o, case, hd, want)
            err = float(np.abs(o - ref).max())
            worst_r = max(worst_r, err)
            assert wrong == 0, (nm, gap, wrong, bad)
            assert err <= tol_attn_route(prec), (nm, gap, err)
        g_r = max(g_r, _row_gap(fused, two))
        assert g_r <= bar, ("ROUTE fused vs two-launch", gap, g_r)
    diag(f"ffn in-kernel cross-attention positions {PREC_IDS[prec]} dim {dim} Lk {Lk} bias={mk}: COUNT worst |out n / Lk - 1| {worst_c:.2e} "
         f"(bar {tol_attn_count(prec, Lk):.2e}), ROUTE decodes on both paths, worst |out - fp64| {worst_r:.2e} (bar {tol_attn_route(prec):.2e}); "
         f"fused vs two-launch per row: COUNT {g_c:.2e} ROUTE {g_r:.2e} (bar {bar:.0e}); V = 0: exact zeros")
