"""GPU parity tests of the individual HIP kernels, driven through the C ABI
(ctypes + numpy only, no torch).  References are plain numpy float64 restatements
of the ATen ops the reference dispatches: conv1d / linear
(+GroupNorm/LayerNorm-apply prologues, GEGLU / bias / residual epilogues),
scaled_dot_product_attention, group_norm statistics, layer_norm statistics.

Tolerances (relative L2 on the whole output):
  fp32 "parity" kernels  : 2e-5   (exact-fp32 MFMA, only summation order differs)
  bf16 kernels           : 6e-3 vs a float64 reference fed the SAME bf16-rounded operands
"""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest

from util import (GEGLU_FLIPS, TOL_ATTN_FP8, TOL_FFN, TOL_ROWCHAIN_GN_Y, TOL_ROWCHAIN_Y, TOL_STATS, bf16_round, eps16, f16_round, gather_rows, gelu_erf, rel_l2, silu,
                  tol_attention, tol_ffn_xattn, tol_gnp_rows, tol_groupnorm, tol_layernorm_apply, tol_ln_linear, tol_pair_rows)

pytestmark = pytest.mark.gpu

PRECS, PREC_IDS = [0, 1, 2], ["fp32", "bf16", "fp16"]       # include/ns2vc_hip.h NS2VC_PREC_*
TOL = {0: 2e-5, 1: 2e-5, 2: 2e-5}      # operands are pre-rounded to the operand type, accumulation is fp32 in every mode


def _lib():
    from ns2vc_amd import _lib
    return _lib.load()


def _dev(a):
    from ns2vc_amd.engine import DevBuf
    return DevBuf.from_numpy(np.ascontiguousarray(a))


def _pack(W, prec):
    lib = _lib()
    from ns2vc_amd._lib import check
    W = np.ascontiguousarray(W, dtype=np.float32)
    p = C.c_void_p()
    check(lib.ns2vc_pack_weight(W.ctypes.data, W.shape[0], W.shape[1], prec, C.byref(p)), "pack_weight")
    return p


class OpBuf:
    """device buffer in the engine's operand type (bf16 for prec 1, fp32 for prec 0)"""

    def __init__(self, a, prec):
        from ns2vc_amd._lib import check
        a = np.ascontiguousarray(a, dtype=np.float32)
        self.prec, self.n, self.shape = prec, a.size, a.shape
        p = C.c_void_p()
        check(_lib().ns2vc_to_operand(a.ctypes.data, a.size, prec, C.byref(p)), "to_operand")
        self.ptr = p.value
        self.esz = 4 if prec == 0 else 2

    def read(self, shape=None):
        from ns2vc_amd._lib import check
        out = np.empty(self.n, dtype=np.float32)
        check(_lib().ns2vc_from_operand(self.ptr, self.n, self.prec, out.ctypes.data), "from_operand")
        return out.reshape(shape or self.shape)

    def __del__(self):
        try:
            _lib().ns2vc_dev_free(self.ptr)
        except Exception:
            pass


def rnd(a, prec):
    a = np.asarray(a, dtype=np.float32)
    return bf16_round(a) if prec == 1 else (f16_round(a) if prec == 2 else a)


def _pack_tiled(W, ctot, c2, prec):
    """device copy of the k = 3 conv weight W [N][3 * ctot + c2] in the tap-sharing kernel's tile-major layout (ns2vc_pack_conv3_tiled)"""
    from ns2vc_amd._lib import check
    lib = _lib()
    W = np.ascontiguousarray(W, dtype=np.float32)
    out = C.c_void_p()
    check(lib.ns2vc_pack_conv3_tiled(W.ctypes.data_as(C.c_void_p), W.shape[0], ctot, c2, prec, C.byref(out)), "pack_conv3_tiled")
    return out


def run_gemm(rng, prec, B, Tin, Tout, c0, c1, N, taps, tmode, bias_on, res_on, geglu, dual, tile=(0, 0, 0), tiled=False):
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    Ct = c0 + c1
    K = taps * Ct
    M = B * Tout
    a0 = rnd(rng.standard_normal((B, Tin, c0)), prec)
    a1 = rnd(rng.standard_normal((B, Tin, c1)), prec) if c1 else None
    W = rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec)
    bias = rng.standard_normal(N).astype(np.float32) if bias_on else None
    Nout = N // 2 if geglu else N
    res = rng.standard_normal((M, Nout)).astype(np.float32) if res_on else None
    A = (a0 if a1 is None else np.concatenate([a0, a1], axis=-1)).astype(np.float64)
    G = gather_rows(A, B, Tin, Tout, taps, tmode).reshape(M, K)
    ref = G @ W.astype(np.float64).T
    if bias is not None:
        ref = ref + bias
    if geglu:
        r3 = ref.reshape(M, N // 64, 2, 32)
        ref = (r3[:, :, 0, :] * gelu_erf(r3[:, :, 1, :])).reshape(M, N // 2)
    if res is not None:
        ref = ref + res

    d_a0, d_a1 = OpBuf(a0, prec), (OpBuf(a1, prec) if a1 is not None else None)
    d_w = _pack(W, prec)
    d_bias = _dev(bias) if bias is not None else None
    d_res = _dev(res) if res is not None else None
    d_out = DevBuf(M * Nout * 4)
    d_out.upload(np.full((M, Nout), np.nan, dtype=np.float32))
    d_oop = OpBuf(np.full((M, Nout), np.nan, dtype=np.float32), prec) if dual else None
    g = GemmArgs()
    g.a0 = d_a0.ptr; g.lda0 = c0; g.c0 = c0
    if d_a1 is not None:
        g.a1 = d_a1.ptr; g.lda1 = c1; g.c1 = c1
    g.B, g.Tin, g.Tout, g.M = B, Tin, Tout, M
    g.taps, g.tmode = taps, tmode
    g.w = d_w.value; g.K = K; g.N = N
    d_wt = _pack_tiled(W, Ct, 0, prec) if (tiled and taps == 3) else None
    if d_wt is not None:
        g.w_tiled = d_wt.value
    if d_bias is not None:
        g.bias = d_bias.ptr
    if d_res is not None:
        g.res = d_res.ptr; g.ldres = Nout
    g.geglu = int(geglu)
    g.out_f32 = d_out.ptr; g.ldo_f32 = Nout
    if d_oop is not None:
        g.out_op = d_oop.ptr; g.ldo_op = Nout
    check(lib.ns2vc_debug_set_gemm_tile(*tile), "set tile")
    try:
        check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
        sync()
    finally:
        lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
    out = d_out.to_numpy((M, Nout))
    out_op = d_oop.read() if d_oop is not None else None
    lib.ns2vc_dev_free(d_w)
    if d_wt is not None:
        lib.ns2vc_dev_free(d_wt)
    return out, ref, out_op


GEMM_CASES = [
    # name, B, Tin, Tout, c0, c1, N, taps, tmode, bias, res, geglu, dual
    ("linear_plain", 2, 75, 75, 128, 0, 128, 1, 0, 1, 0, 0, 0),
    ("linear_res_tail_dual", 3, 41, 41, 256, 0, 192, 1, 0, 1, 1, 0, 1),
    ("linear_k_long", 2, 33, 33, 1024, 0, 256, 1, 0, 1, 1, 0, 0),
    ("linear_k_one_tile", 2, 50, 50, 64, 0, 128, 1, 0, 0, 0, 0, 0),
    ("conv3", 2, 37, 37, 128, 0, 128, 3, 0, 1, 0, 0, 0),
    ("conv3_concat_res", 2, 37, 37, 128, 64, 128, 3, 0, 1, 1, 0, 1),
    ("conv1_concat_shortcut", 2, 37, 37, 192, 128, 256, 1, 0, 1, 0, 0, 0),
    # T >= 66: the tap-sharing kernel (convts.hip) under the default heuristic; N = 192 only has 64-column tiles
    ("conv3_ts", 2, 70, 70, 128, 0, 128, 3, 0, 1, 0, 0, 0),
    ("conv3_ts_concat_res_dual", 3, 131, 131, 128, 64, 192, 3, 0, 1, 1, 0, 1),
    ("conv3_ts_long", 2, 300, 300, 256, 128, 256, 3, 0, 1, 1, 0, 1),
    ("down2_odd", 2, 37, 19, 128, 0, 128, 3, 1, 1, 0, 0, 0),
    ("down2_even", 2, 38, 19, 128, 0, 128, 3, 1, 1, 0, 0, 0),
    ("up2_odd", 2, 19, 37, 128, 0, 128, 3, 2, 1, 0, 0, 0),
    ("up2_even", 2, 19, 38, 128, 0, 128, 3, 2, 1, 0, 0, 0),
    ("qkv_op_only_like", 2, 50, 50, 128, 0, 384, 1, 0, 1, 0, 0, 1),
    ("geglu", 2, 50, 50, 128, 0, 1024, 1, 0, 1, 0, 1, 1),
    ("temb_m_small", 3, 1, 1, 512, 0, 640, 1, 0, 1, 0, 0, 0),
]


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("case", GEMM_CASES, ids=[c[0] for c in GEMM_CASES])
def test_gemm_cases(case, prec, diag):
    name, *args = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    out, ref, out_op = run_gemm(rng, prec, *args)
    e = rel_l2(out, ref)
    diag(f"gemm {name} prec={prec} rel_l2={e:.3e} nan={int(np.isnan(out).sum())}")
    if not (e < TOL[prec]):
        bad = np.argwhere(~(np.abs(out - ref) <= 1e-2 + 1e-2 * np.abs(ref)))
        diag(f"  FAIL {name}: {len(bad)} bad of {out.size}; first {bad[:6].tolist()} rows_bad={sorted(set(bad[:, 0].tolist()))[:12]} cols_bad={sorted(set(bad[:, 1].tolist()))[:12]}")
    assert e < TOL[prec], (name, e)
    if out_op is not None:      # operand-typed copy == the fp32 result rounded to the operand type
        assert np.array_equal(out_op, rnd(out, prec)), name


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(128, 128, 13), (64, 128, 13), (128, 128, 23), (64, 128, 23)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_cases_ksplit_kernel(tile, prec, diag):
    """Every feature case (taps, stride 2, upsample, concat, residual, GEGLU, dual outputs) through the 8-wave K-split kernel."""
    for name, *args in GEMM_CASES:
        if args[5] % 128:
            continue
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        out, ref, out_op = run_gemm(rng, prec, *args, tile=tile)
        e = rel_l2(out, ref)
        diag(f"gemm4 {name} tile={tile} prec={prec} rel_l2={e:.3e}")
        assert e < TOL[prec], (name, e)
        if out_op is not None:
            assert np.array_equal(out_op, rnd(out, prec)), name


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(64, 128, 2), (64, 64, 2), (64, 64, 3), (64, 64, 4),
                                  # stages 12 / 13 = the 8-wave K-split kernel (gemm4_kernel) with ring depth 2 / 3
                                  (128, 128, 12), (128, 128, 13), (64, 128, 12), (64, 128, 13),
                                  # stage 23 = the same kernel with loader / consumer wave specialisation (4 + 4 waves), ring 3
                                  (128, 128, 23), (64, 128, 23)],
                         ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_every_tile(tile, prec, diag):
    rng = np.random.default_rng(tile[0] * 1000 + tile[1])
    # M = 3*167 = 501 rows (tail in every tile size), concat + conv3 + bias + residual, K = 3*192 (9 / 18 tiles)
    out, ref, _ = run_gemm(rng, prec, 3, 167, 167, 128, 64, 256, 3, 0, 1, 1, 0, 0, tile=tile)
    e = rel_l2(out, ref)
    diag(f"gemm tile={tile} prec={prec} rel_l2={e:.3e}")
    assert e < TOL[prec]
    # K of exactly 1, 2 and 3 tiles exercises the pipeline prologue / tail waits
    for kk in (1, 2, 3):
        out, ref, _ = run_gemm(rng, prec, 2, 90, 90, (64 if prec else 32) * kk, 0, 128, 1, 0, 1, 0, 0, 0, tile=tile)
        e = rel_l2(out, ref)
        diag(f"gemm tile={tile} prec={prec} ktiles={kk} rel_l2={e:.3e}")
        assert e < TOL[prec]
    if tile[1] == 128:
        out, ref, _ = run_gemm(rng, prec, 2, 90, 90, 256, 0, 512, 1, 0, 1, 0, 1, 0, tile=tile)
        e = rel_l2(out, ref)
        diag(f"gemm geglu tile={tile} prec={prec} rel_l2={e:.3e}")
        assert e < TOL[prec]


TS_STAGES = (54, 58, 64, 68)     # ns2vc_debug_set_gemm_tile(128, BN, 50 + loader waves): the tap-sharing conv kernel (convts.hip), BN 64 | 128; 60 + loader waves: BN 64 with the K-split consumer layout


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(128, 64, 54), (128, 128, 54), (128, 64, 58), (128, 128, 58), (128, 64, 64), (128, 64, 68)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_conv_tapshare_kernel(tile, prec, diag):
    """conv3ts_kernel (k = 3, stride 1: resnet.py:591-641 conv1 / conv2, unet_1d_condition.py:943,1032) against numpy fp64 AND against
    gemm4_kernel on the same operands: every tile (BN 64 / 128, 4 / 8 loader waves); items shorter, equal to and longer than a 126-row tile
    (T = 66, 70, 125, 126, 127, 300: pad rows at every position of a tile, tiles inside one item, items inside one tile); 1, 2, 3 and many
    channel chunks; the concat of two sources; the fused 1x1 segment (single-tap chunks behind the main ones); bias, residual that aliases
    nothing, fp32 + operand outputs; NaN-prefilled outputs (every row written exactly where it belongs, nothing else touched); and the same launches
    reading tile-major weights (ns2vc_gemm_args.w_tiled, ns2vc_pack_conv3_tiled): bit-identical."""
    lib = _lib()
    rng = np.random.default_rng(tile[1] * 7 + tile[2])
    ck = 64 if prec else 32
    cases = [(B, T, ck * nc, 0) for (B, T, nc) in ((3, 66, 1), (2, 70, 2), (3, 125, 3), (2, 126, 4), (3, 127, 2), (2, 300, 6), (5, 67, 2))]
    cases += [(3, 131, 2 * ck, ck), (2, 90, ck, 3 * ck), (4, 70, 4 * ck, 4 * ck)]
    for (B, T, c0, c1) in cases:
        for N in (128, 256):
            out, ref, out_op = run_gemm(rng, prec, B, T, T, c0, c1, N, 3, 0, 1, 1, 0, 1, tile=tile)
            e = rel_l2(out, ref)
            out4, _, _ = run_gemm(np.random.default_rng(1), prec, B, T, T, c0, c1, N, 3, 0, 1, 1, 0, 0, tile=(64, 128, 23))
            outs, _, _ = run_gemm(np.random.default_rng(1), prec, B, T, T, c0, c1, N, 3, 0, 1, 1, 0, 0, tile=tile)
            outt, _, _ = run_gemm(np.random.default_rng(1), prec, B, T, T, c0, c1, N, 3, 0, 1, 1, 0, 0, tile=tile, tiled=True)
            assert np.array_equal(outs, outt), "tile-major weights (w_tiled): same products in the same order, only another source layout"
            e4 = rel_l2(outs, out4)
            diag(f"conv3ts tile={tile} prec={prec} B={B} T={T} c={c0}+{c1} N={N}: vs fp64 {e:.3e}  vs gemm4_kernel {e4:.3e}  nan={int(np.isnan(out).sum())}")
            assert e < TOL[prec] and e4 < (1e-5 if prec == 0 else 1e-5), (B, T, c0, c1, N, e, e4)
            assert np.array_equal(out_op, rnd(out, prec))
    # the fused 1x1 segment on a third operand tensor (resnet conv2 + conv_shortcut), with epilogue statistics
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    for (B, T, c0, c2, N) in ((3, 70, 4 * ck, 10 * ck, 256), (2, 131, 2 * ck, ck, 128), (3, 97, 8 * ck, 16 * ck, 512)):
        M = B * T
        hn, x = rnd(rng.standard_normal((B, T, c0)), prec), rnd(rng.standard_normal((B, T, c2)), prec)
        W = rnd(rng.standard_normal((N, 3 * c0 + c2)) / np.sqrt(3 * c0 + c2), prec)
        bias = rng.standard_normal(N).astype(np.float32)
        G = gather_rows(hn.astype(np.float64), B, T, T, 3, 0).reshape(M, 3 * c0)
        ref = G @ W[:, :3 * c0].astype(np.float64).T + x.reshape(M, c2).astype(np.float64) @ W[:, 3 * c0:].astype(np.float64).T + bias
        d_h, d_x, d_w, d_b = OpBuf(hn, prec), OpBuf(x, prec), _pack(W, prec), _dev(bias)
        d_o = DevBuf(M * N * 4)
        d_o.upload(np.full((M, N), np.nan, dtype=np.float32))
        d_s = DevBuf.from_numpy(np.zeros((B, N // 16, 2), dtype=np.int64))
        g = GemmArgs()
        g.a0 = d_h.ptr; g.lda0 = c0; g.c0 = c0
        g.a2 = d_x.ptr; g.lda2 = c2; g.c2 = c2
        g.B, g.Tin, g.Tout, g.M = B, T, T, M
        g.taps, g.tmode = 3, 0
        g.w = d_w.value; g.K = 3 * c0 + c2; g.N = N; g.bias = d_b.ptr
        g.out_f32 = d_o.ptr; g.ldo_f32 = N
        g.stats = d_s.ptr
        d_wt = _pack_tiled(W, c0, c2, prec)
        outs2 = []
        for use_tiled in (True, False):
            g.w_tiled = d_wt.value if use_tiled else None
            d_o.upload(np.full((M, N), np.nan, dtype=np.float32))
            d_s.upload(np.zeros((B, N // 16, 2), dtype=np.int64))
            check(lib.ns2vc_debug_set_gemm_tile(*tile), "tile")
            try:
                check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
                sync()
            finally:
                lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
            outs2.append(d_o.to_numpy((M, N)))
        lib.ns2vc_dev_free(d_wt)
        assert np.array_equal(outs2[0], outs2[1]), "tile-major weights with a fused 1x1 segment"
        out = outs2[1]
        e = rel_l2(out, ref)
        st = d_s.to_numpy((B, N // 16, 2), dtype=np.int64).astype(np.float64)
        blk = out.astype(np.float64).reshape(B, T, N // 16, 16)
        ref_s, ref_q = blk.sum(axis=(1, 3)), (blk ** 2).sum(axis=(1, 3))
        e_s = np.abs(st[..., 0] / 2 ** 28 - ref_s).max() / np.abs(ref_s).max()
        e_q = np.abs(st[..., 1] / 2 ** 16 - ref_q).max() / np.abs(ref_q).max()
        diag(f"conv3ts + 1x1 segment tile={tile} prec={prec} {(B, T, c0, c2, N)}: {e:.3e}  statistics {e_s:.1e} / {e_q:.1e}")
        assert e < TOL[prec] and e_s < TOL_STATS and e_q < TOL_STATS
        lib.ns2vc_dev_free(d_w)


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(0, 0, 0), (64, 128, 13), (128, 128, 13), (64, 128, 23), (128, 128, 23), (128, 64, 54), (128, 128, 54), (128, 64, 58), (128, 64, 68)],
                         ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_groupnorm_prologue(tile, prec, diag):
    """ns2vc_gemm_args.gnp_*: the GEMM writes act(GroupNorm(x)) for the rows its tiles read into its own A operand and then runs as
    usual (resnet.py:606-629 norm -> act -> conv, transformer_1d.py:268 norm -> proj_in) -- against the two-launch path
    (ns2vc_k_groupnorm_stats + the same GEMM) BIT FOR BIT: operand rows and results, for k = 3 and k = 1, with and without the
    time scale / shift and SiLU, row tiles that straddle up to three batch items (T = 70 / 131 / 167 is no multiple of 64), several
    column tiles per row panel (N = 384), an operand buffer that starts as NaN, and a reference in numpy fp64 on top."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    for (B, T, Cc, N, taps, temb_on, silu, Gn) in ((3, 167, 128, 128, 3, 1, 1, 8), (2, 131, 256, 384, 3, 0, 1, 8), (3, 140, 384, 384, 1, 0, 0, 8),
                                                   (4, 131, 512, 256, 3, 1, 1, 8), (5, 70, 256, 256, 3, 1, 1, 8)):
        if tile[2] in TS_STAGES and (taps != 3 or N % tile[1]):
            continue                                     # (a forced tap-sharing tile only takes k = 3)
        rng = np.random.default_rng(B * 1000 + T + Cc + taps)
        M, K = B * T, taps * Cc
        x = (rng.standard_normal((B, T, Cc)) * (1.0 + rng.random((B, 1, Cc))) + rng.standard_normal((B, 1, Cc))).astype(np.float32)
        gam, bet = (1.0 + 0.2 * rng.standard_normal(Cc)).astype(np.float32), (0.2 * rng.standard_normal(Cc)).astype(np.float32)
        ldt, toff = 2 * Cc + 24, 8                       # (scale | shift) pairs somewhere inside a wider per-item row, as in the engine
        temb = (0.3 * rng.standard_normal((B, ldt))).astype(np.float32)
        blk = x.astype(np.float64).reshape(B, T, Cc // 16, 16)
        st = np.stack([np.rint(blk.sum(axis=(1, 3)) * 2.0 ** 28), np.rint((blk ** 2).sum(axis=(1, 3)) * 2.0 ** 16)], axis=-1).astype(np.int64)
        W = rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec)
        bias = rng.standard_normal(N).astype(np.float32)
        d_x, d_g, d_b, d_t, d_st = _dev(x.reshape(M, Cc)), _dev(gam), _dev(bet), _dev(temb), DevBuf.from_numpy(st)
        d_w, d_bias = _pack(W, prec), _dev(bias)
        t_ptr = (d_t.ptr + 4 * toff) if temb_on else None
        outs, ops = [], []
        # 2: the cooperative form (gnp_sync: the column tiles of a row block build a share of its rows each), twice; 3: arrival words with bit 62
        # set = "do not wait" -- every workgroup takes the path of one that waited in vain for a sibling and builds all its rows itself
        nsync = (M + 63) // 64
        d_sync = DevBuf.from_numpy(np.zeros(nsync, dtype=np.uint64))
        d_poison = DevBuf.from_numpy(np.full(nsync, 1 << 62, dtype=np.uint64))
        d_alone = DevBuf.from_numpy(np.zeros(2, dtype=np.uint32))       # workgroups that waited in vain: [cooperative runs, poisoned run]
        for fused in (0, 1, 2, 2, 3):
            d_a = OpBuf(np.full((M, Cc), np.nan, dtype=np.float32), prec)
            d_o = DevBuf(M * N * 4)
            d_o.upload(np.full((M, N), np.nan, dtype=np.float32))
            g = GemmArgs()
            g.a0 = d_a.ptr; g.lda0 = Cc; g.c0 = Cc
            g.B, g.Tin, g.Tout, g.M = B, T, T, M
            g.taps, g.tmode = taps, 0
            g.w = d_w.value; g.K = K; g.N = N; g.bias = d_bias.ptr
            g.out_f32 = d_o.ptr; g.ldo_f32 = N
            g.algo = 2                                   # (the materialising prologue: the in-loop form of the tap-sharing kernel has its own test below)
            if fused:
                g.gnp_x = d_x.ptr; g.gnp_ldx = Cc; g.gnp_stats = d_st.ptr; g.gnp_gamma = d_g.ptr; g.gnp_beta = d_b.ptr
                g.gnp_temb = t_ptr; g.gnp_ldtemb = ldt; g.gnp_eps = 1e-5; g.gnp_G = Gn; g.gnp_silu = silu
                if fused == 2:
                    d_sync.upload(np.zeros(nsync, dtype=np.uint64))          # (the arrival words start every launch at zero: the engine's per-forward clear)
                g.gnp_sync = d_sync.ptr if fused == 2 else (d_poison.ptr if fused == 3 else None)
                g.gnp_alone = d_alone.ptr + 4 * (fused == 3)
            else:
                check(lib.ns2vc_k_groupnorm_stats(d_x.ptr, Cc, Cc, d_st.ptr, B, T, Gn, 1e-5, d_g.ptr, d_b.ptr, d_t.ptr if temb_on else None, ldt, toff, silu,
                                                  d_a.ptr, prec, None), "groupnorm_stats")
            check(lib.ns2vc_debug_set_gemm_tile(*tile), "set tile")
            try:
                check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
                sync()
            finally:
                lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
            outs.append(d_o.to_numpy((M, N)))
            ops.append(d_a.read())
        lib.ns2vc_dev_free(d_w)
        # fp64 reference of the normalised rows and of the product on the device's operand rows
        xg = x.astype(np.float64).reshape(B, T, Gn, Cc // Gn)
        mean, var = xg.mean(axis=(1, 3), keepdims=True), xg.var(axis=(1, 3), keepdims=True)
        y = ((xg - mean) / np.sqrt(var + 1e-5)).reshape(B, T, Cc) * gam.astype(np.float64) + bet.astype(np.float64)
        if temb_on:
            y = y * (1.0 + temb[:, None, toff:toff + Cc].astype(np.float64)) + temb[:, None, toff + Cc:toff + 2 * Cc].astype(np.float64)
        if silu:
            y = y / (1.0 + np.exp(-y))
        e_op = rel_l2(ops[1], y.reshape(M, Cc))
        Gr = gather_rows(ops[1].astype(np.float64).reshape(B, T, Cc), B, T, T, taps, 0).reshape(M, K)
        e_out = rel_l2(outs[1], Gr @ W.astype(np.float64).T + bias)
        same_op, same_out = all(np.array_equal(ops[0], o) for o in ops[1:]), all(np.array_equal(outs[0], o) for o in outs[1:])
        counts = d_sync.to_numpy((nsync,), dtype=np.uint64)
        alone = d_alone.to_numpy((2,), dtype=np.uint32)
        # column tiles that share a row block: N / 128 in gemm4_kernel, N / BN in the tap-sharing kernel (k = 3; BN = 64 at these sizes by default)
        ts = taps == 3 and (tile == (0, 0, 0) or tile[2] in TS_STAGES)
        nshare = N // (tile[1] if tile[2] in TS_STAGES else 64) if ts else N // 128
        assert alone[0] == 0 and (alone[1] > 0) == (nshare > 1), f"workgroups that waited in vain: {alone}"
        per = nshare if nshare > 1 else 0
        arrivals, nibbles = counts & np.uint64(0xffff), (counts >> np.uint64(16)) & np.uint64(0xffffffff)
        assert np.isin(arrivals, (0, per)).all() and arrivals[0] == per, "a cooperative launch adds one arrival per column tile to a row block's word"
        # ... each also counted in the nibble of the XCC it ran on: one nibble holds them all (the siblings shared an XCD)
        assert all(int(n) in [per << (4 * k) for k in range(8)] for n, a in zip(nibbles, arrivals) if a), [hex(int(c)) for c in counts[:4]]
        diag(f"gemm+GroupNorm prologue tile={tile} prec={prec} B={B} T={T} C={Cc} N={N} taps={taps} temb={temb_on} silu={silu}: "
             f"rows vs fp64 {e_op:.2e}  result vs fp64 {e_out:.2e}  rows==two-launch {same_op}  result==two-launch {same_out}")
        assert np.isfinite(ops[1]).all() and np.isfinite(outs[1]).all()          # every row the tiles read was produced
        assert same_op and same_out
        assert e_op < tol_gnp_rows(prec)[0] and e_out < TOL[prec]


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(0, 0, 0), (64, 128, 23), (128, 128, 23), (128, 64, 54), (128, 128, 54), (128, 128, 58), (128, 64, 64)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_groupnorm_prologue_of_a_concat(tile, prec, diag):
    """The prologue on the channel concat of TWO tensors, each with its own epilogue statistics (resnet.py:591 on torch.cat([h, skip]) in the
    up blocks: 128+128 ... 512+512 channels, 512+384 with groups that straddle the two sources), plus the un-normalised operand copy the
    1x1 shortcut reads (gnp_raw) -- against ns2vc_k_groupnorm_stats2 + the same GEMM BIT FOR BIT (normalised rows, raw rows, result), in
    the redundant and in the cooperative form, and the normalised rows against numpy fp64."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    # (the last two: the 128 + 256 / 256 + 128 concats of the non-default configurations, tests/configs.py, in 4 groups of 96 -- the
    #  seam inside the second / third group)
    for (B, T, c0, c1, N, taps, Gn) in ((3, 167, 128, 128, 128, 3, 8), (2, 131, 512, 384, 512, 3, 8), (3, 70, 512, 512, 256, 3, 8), (2, 140, 256, 384, 384, 1, 8),
                                        (2, 131, 128, 256, 128, 3, 4), (3, 70, 256, 128, 256, 3, 4)):
        if tile[2] in TS_STAGES and (taps != 3 or N % tile[1]):
            continue
        rng = np.random.default_rng(B * 1000 + T + c0 + c1)
        Cc = c0 + c1
        M, K = B * T, taps * Cc
        x0 = (rng.standard_normal((B, T, c0)) * (1.0 + rng.random((B, 1, c0))) + rng.standard_normal((B, 1, c0))).astype(np.float32)
        x1 = (rng.standard_normal((B, T, c1)) * 0.5 + rng.standard_normal((B, 1, c1))).astype(np.float32)
        ld0, ld1 = c0 + 8, c1                                # (the first source sits inside wider rows)
        x0w = np.zeros((B, T, ld0), np.float32); x0w[..., :c0] = x0
        gam, bet = (1.0 + 0.2 * rng.standard_normal(Cc)).astype(np.float32), (0.2 * rng.standard_normal(Cc)).astype(np.float32)

        def stats(x):
            blk = x.astype(np.float64).reshape(B, T, x.shape[-1] // 16, 16)
            return np.stack([np.rint(blk.sum(axis=(1, 3)) * 2.0 ** 28), np.rint((blk ** 2).sum(axis=(1, 3)) * 2.0 ** 16)], axis=-1).astype(np.int64)
        W = rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec)
        d_x0, d_x1, d_g, d_b = _dev(x0w.reshape(M, ld0)), _dev(x1.reshape(M, c1)), _dev(gam), _dev(bet)
        d_s0, d_s1, d_w = DevBuf.from_numpy(stats(x0)), DevBuf.from_numpy(stats(x1)), _pack(W, prec)
        d_sync = DevBuf.from_numpy(np.zeros((M + 63) // 64, dtype=np.uint64))
        outs, ops, raws = [], [], []
        for fused in (0, 1, 2, 2):
            d_a, d_r = OpBuf(np.full((M, Cc), np.nan, dtype=np.float32), prec), OpBuf(np.full((M, Cc), np.nan, dtype=np.float32), prec)
            d_o = DevBuf(M * N * 4)
            d_o.upload(np.full((M, N), np.nan, dtype=np.float32))
            g = GemmArgs()
            g.a0 = d_a.ptr; g.lda0 = Cc; g.c0 = Cc
            g.B, g.Tin, g.Tout, g.M = B, T, T, M
            g.taps, g.tmode = taps, 0
            g.w = d_w.value; g.K = K; g.N = N
            g.out_f32 = d_o.ptr; g.ldo_f32 = N
            g.algo = 2
            if fused:
                g.gnp_x = d_x0.ptr; g.gnp_ldx = ld0; g.gnp_stats = d_s0.ptr; g.gnp_gamma = d_g.ptr; g.gnp_beta = d_b.ptr
                g.gnp_eps = 1e-5; g.gnp_G = Gn; g.gnp_silu = 1
                g.gnp_x1 = d_x1.ptr; g.gnp_ldx1 = ld1; g.gnp_c1 = c1; g.gnp_stats1 = d_s1.ptr; g.gnp_raw = d_r.ptr
                if fused == 2:
                    d_sync.upload(np.zeros((M + 63) // 64, dtype=np.uint64))
                g.gnp_sync = d_sync.ptr if fused == 2 else None
            else:
                check(lib.ns2vc_k_groupnorm_stats2(d_x0.ptr, ld0, c0, d_s0.ptr, d_x1.ptr, ld1, c1, d_s1.ptr, B, T, Gn, 1e-5, d_g.ptr, d_b.ptr, None, 0, 0, 1,
                                                   d_a.ptr, d_r.ptr, prec, None), "groupnorm_stats2")
            check(lib.ns2vc_debug_set_gemm_tile(*tile), "set tile")
            try:
                check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
                sync()
            finally:
                lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
            outs.append(d_o.to_numpy((M, N))); ops.append(d_a.read()); raws.append(d_r.read())
        lib.ns2vc_dev_free(d_w)
        x = np.concatenate([x0, x1], axis=-1)
        xg = x.astype(np.float64).reshape(B, T, Gn, Cc // Gn)
        mean, var = xg.mean(axis=(1, 3), keepdims=True), xg.var(axis=(1, 3), keepdims=True)
        y = ((xg - mean) / np.sqrt(var + 1e-5)).reshape(B, T, Cc) * gam.astype(np.float64) + bet.astype(np.float64)
        y = y / (1.0 + np.exp(-y))
        e_op, e_raw = rel_l2(ops[1], y.reshape(M, Cc)), rel_l2(raws[1], x.reshape(M, Cc))
        same = all(np.array_equal(ops[0], o) for o in ops[1:]) and all(np.array_equal(raws[0], o) for o in raws[1:]) and \
            all(np.array_equal(outs[0], o) for o in outs[1:])
        diag(f"gemm+GroupNorm prologue of a concat tile={tile} prec={prec} B={B} T={T} C={c0}+{c1} N={N} taps={taps}: rows vs fp64 {e_op:.2e}  raw copy vs input "
             f"{e_raw:.2e}  rows, raw rows and result == two-launch path (redundant, cooperative x2): {same}")
        assert np.isfinite(ops[1]).all() and np.isfinite(raws[1]).all() and np.isfinite(outs[1]).all()
        assert same
        assert e_op < tol_gnp_rows(prec)[0] and e_raw < tol_gnp_rows(prec)[1]


IN_LOOP_CASES = [  # B, T, c0, c1, N, temb, silu, raw copy, fused 1x1 segment channels
    (3, 167, 128, 0, 128, 1, 1, 0, 0), (2, 131, 256, 0, 384, 0, 1, 0, 0), (4, 131, 512, 0, 256, 1, 1, 0, 0), (5, 70, 256, 0, 256, 1, 1, 0, 0),
    (3, 167, 128, 128, 128, 0, 1, 1, 0), (2, 131, 512, 384, 512, 0, 1, 1, 0), (3, 70, 512, 512, 256, 0, 1, 1, 0), (2, 300, 128, 0, 128, 1, 0, 1, 0),
    (2, 131, 256, 0, 256, 1, 1, 0, 128), (3, 97, 64, 0, 128, 1, 1, 0, 64), (2, 938, 128, 0, 128, 1, 1, 0, 0)]


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(0, 0, 0), (128, 64, 58), (128, 128, 58)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_conv_groupnorm_in_loop(tile, prec, diag):
    """r6: GroupNorm (+ time scale / shift) (+ SiLU) applied INSIDE the K loop of the tap-sharing conv kernel (ns2vc_gemm_args.algo = 0 with gnp_x
    set; gnpro.h GnInloop): four of the kernel's non-consumer waves load the fp32 rows, normalise them and write the operand values straight into the
    activation ring.  Nothing is materialised in global memory -- the operand tensor a0 must stay untouched -- and the result must equal the two-launch
    path (ns2vc_k_groupnorm_stats[2] + the same conv) BIT FOR BIT: same arithmetic per element, same operand rounding, same summation order.  Cases:
    time embedding on / off, SiLU on / off, row tiles over up to three batch items (T = 70, 97), the channel concat of two sources with groups that straddle
    them, the un-normalised operand copy (gnp_raw, written by the first column tile), a fused 1x1 segment behind the main chunks (its rows still come
    by DMA: one and several main chunks in front), 1 .. 8 column tiles per row block, with and without the cooperative tile order (gnp_sync)."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    bke = 32 if prec == 0 else 64
    for (B, T, c0, c1, N, temb_on, silu, raw_on, c2) in IN_LOOP_CASES:
        if (tile[2] in TS_STAGES and N % tile[1]) or c0 % bke or c1 % bke or c2 % bke:
            continue
        rng = np.random.default_rng(B * 1000 + T + c0 + c1 + c2)
        Cc, Gn, taps = c0 + c1, 8, 3
        if (Cc // Gn) % 16:
            Gn = 4
        M, K = B * T, taps * Cc + c2
        x0 = (rng.standard_normal((B, T, c0)) * (1.0 + rng.random((B, 1, c0))) + rng.standard_normal((B, 1, c0))).astype(np.float32)
        x1 = (rng.standard_normal((B, T, max(c1, 16))) * 0.5 + rng.standard_normal((B, 1, max(c1, 16)))).astype(np.float32)
        ld0, ld1 = c0 + 8, max(c1, 16)
        x0w = np.zeros((B, T, ld0), np.float32); x0w[..., :c0] = x0
        gam, bet = (1.0 + 0.2 * rng.standard_normal(Cc)).astype(np.float32), (0.2 * rng.standard_normal(Cc)).astype(np.float32)
        ldt, toff = 2 * Cc + 24, 8
        temb = (0.3 * rng.standard_normal((B, ldt))).astype(np.float32)
        a2 = rnd(rng.standard_normal((M, max(c2, 16))), prec)

        def stats(x):
            blk = x.astype(np.float64).reshape(B, T, x.shape[-1] // 16, 16)
            return np.stack([np.rint(blk.sum(axis=(1, 3)) * 2.0 ** 28), np.rint((blk ** 2).sum(axis=(1, 3)) * 2.0 ** 16)], axis=-1).astype(np.int64)
        W = rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec)
        bias = rng.standard_normal(N).astype(np.float32)
        d_x0, d_x1, d_g, d_b, d_t = _dev(x0w.reshape(M, ld0)), _dev(x1.reshape(M, ld1)), _dev(gam), _dev(bet), _dev(temb)
        d_s0, d_s1, d_w, d_bias = DevBuf.from_numpy(stats(x0)), DevBuf.from_numpy(stats(x1[..., :max(c1, 16)])), _pack(W, prec), _dev(bias)
        d_a2 = OpBuf(a2, prec)
        d_sync = DevBuf.from_numpy(np.zeros((M + 63) // 64, dtype=np.uint64))
        t_ptr = (d_t.ptr + 4 * toff) if temb_on else None
        outs, ops, raws = [], [], []
        for mode in (0, 1, 2):                           # 0: two launches; 1: in the loop; 2: in the loop, cooperative tile order
            d_a, d_r = OpBuf(np.full((M, Cc), np.nan, dtype=np.float32), prec), OpBuf(np.full((M, Cc), np.nan, dtype=np.float32), prec)
            d_o = DevBuf(M * N * 4)
            d_o.upload(np.full((M, N), np.nan, dtype=np.float32))
            g = GemmArgs()
            g.a0 = d_a.ptr; g.lda0 = Cc; g.c0 = Cc
            g.B, g.Tin, g.Tout, g.M = B, T, T, M
            g.taps, g.tmode = taps, 0
            g.w = d_w.value; g.K = K; g.N = N; g.bias = d_bias.ptr
            g.out_f32 = d_o.ptr; g.ldo_f32 = N
            if c2:
                g.a2 = d_a2.ptr; g.lda2 = max(c2, 16); g.c2 = c2
            g.algo = 0
            if mode:
                g.gnp_x = d_x0.ptr; g.gnp_ldx = ld0; g.gnp_stats = d_s0.ptr; g.gnp_gamma = d_g.ptr; g.gnp_beta = d_b.ptr
                g.gnp_temb = t_ptr; g.gnp_ldtemb = ldt; g.gnp_eps = 1e-5; g.gnp_G = Gn; g.gnp_silu = silu
                if c1:
                    g.gnp_x1 = d_x1.ptr; g.gnp_ldx1 = ld1; g.gnp_c1 = c1; g.gnp_stats1 = d_s1.ptr
                if raw_on:
                    g.gnp_raw = d_r.ptr
                g.gnp_sync = d_sync.ptr if mode == 2 else None
            elif c1:
                check(lib.ns2vc_k_groupnorm_stats2(d_x0.ptr, ld0, c0, d_s0.ptr, d_x1.ptr, ld1, c1, d_s1.ptr, B, T, Gn, 1e-5, d_g.ptr, d_b.ptr,
                                                   d_t.ptr if temb_on else None, ldt, toff, silu, d_a.ptr, d_r.ptr if raw_on else None, prec, None), "groupnorm_stats2")
            else:
                check(lib.ns2vc_k_groupnorm_stats(d_x0.ptr, ld0, c0, d_s0.ptr, B, T, Gn, 1e-5, d_g.ptr, d_b.ptr, d_t.ptr if temb_on else None, ldt, toff, silu,
                                                  d_a.ptr, prec, None), "groupnorm_stats")
                if raw_on:                               # (the single-source launch has no raw copy: the operand rounding of x itself)
                    d_r = OpBuf(x0.reshape(M, c0), prec)
            check(lib.ns2vc_debug_set_gemm_tile(*tile), "set tile")
            try:
                check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
                sync()
            finally:
                lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
            outs.append(d_o.to_numpy((M, N))); ops.append(d_a.read()); raws.append(d_r.read())
        lib.ns2vc_dev_free(d_w)
        same_out = all(np.array_equal(outs[0], o) for o in outs[1:])
        same_raw = (not raw_on) or all(np.array_equal(raws[0], r) for r in raws[1:])
        untouched = all(bool(np.isnan(o).all()) for o in ops[1:])
        # ... and the two-launch path itself against numpy fp64 (rows, then the product on the device's operand rows)
        x = np.concatenate([x0, x1[..., :c1]], axis=-1) if c1 else x0
        xg = x.astype(np.float64).reshape(B, T, Gn, Cc // Gn)
        mean, var = xg.mean(axis=(1, 3), keepdims=True), xg.var(axis=(1, 3), keepdims=True)
        y = ((xg - mean) / np.sqrt(var + 1e-5)).reshape(B, T, Cc) * gam.astype(np.float64) + bet.astype(np.float64)
        if temb_on:
            y = y * (1.0 + temb[:, None, toff:toff + Cc].astype(np.float64)) + temb[:, None, toff + Cc:toff + 2 * Cc].astype(np.float64)
        if silu:
            y = y / (1.0 + np.exp(-y))
        e_op = rel_l2(ops[0], y.reshape(M, Cc))
        Gr = gather_rows(ops[0].astype(np.float64).reshape(B, T, Cc), B, T, T, taps, 0).reshape(M, taps * Cc)
        ref = Gr @ W[:, :taps * Cc].astype(np.float64).T + bias
        if c2:
            ref = ref + a2[:, :c2].astype(np.float64) @ W[:, taps * Cc:].astype(np.float64).T
        e_out = rel_l2(outs[1], ref)
        diag(f"conv + in-loop GroupNorm tile={tile} prec={prec} B={B} T={T} C={c0}+{c1} N={N} temb={temb_on} silu={silu} raw={raw_on} c2={c2}: result == two-launch path "
             f"{same_out}  raw copy == {same_raw}  operand tensor untouched {untouched}  rows vs fp64 {e_op:.2e}  result vs fp64 {e_out:.2e}")
        assert np.isfinite(outs[1]).all() and same_out and same_raw and untouched
        assert e_op < tol_gnp_rows(prec)[0] and e_out < TOL[prec]



@pytest.mark.parametrize("prec", [p for p in PRECS if p != 0], ids=[i for p, i in zip(PRECS, PREC_IDS) if p != 0])
@pytest.mark.parametrize("tile", [(0, 0, 0), (128, 64, 58), (128, 128, 58)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_conv_on_hi_lo_operand_pairs(tile, prec, diag):
    """r6 (ns2vc_gemm_args.gnp_pair; the engine's split_io option): the GroupNorm prologue writes act(GN(x)) as a hi + lo operand pair -- hi = the operand type's rounding,
    lo = the rounding of what that dropped -- and the k = 3 conv runs over [hi | lo] (a0, c0 = 2 C) then hi once more (a1 = a0, c1 = C) against weights packed
    (hi(w) | hi(w) | lo(w)) per tap: x * w to ~2^-2p instead of 2^-p relative.  Checked: the hi plane equals the plain prologue's rows bit for bit, hi + lo
    reproduces the fp64 rows to fp32 accuracy, and the result is >= 50x closer to the fp64 convolution of the UNROUNDED rows and weights than the plain launch.
    The pair prologue is its own instantiation of the tap-sharing kernel (both column tiles); other kernels refuse the flag (algo = 1)."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    for (B, T, Cc, N, temb_on, silu) in [(2, 200, 128, 128, 0, 1), (3, 97, 128, 256, 1, 1), (2, 131, 256, 128, 1, 0)]:
        rng = np.random.default_rng(B * 100 + T + Cc)
        Gn, taps, M = 8, 3, B * T
        x = (rng.standard_normal((B, T, Cc)) * (1.0 + rng.random((B, 1, Cc))) + rng.standard_normal((B, 1, Cc))).astype(np.float32)
        gam, bet = (1.0 + 0.2 * rng.standard_normal(Cc)).astype(np.float32), (0.2 * rng.standard_normal(Cc)).astype(np.float32)
        ldt = 2 * Cc
        temb = (0.3 * rng.standard_normal((B, ldt))).astype(np.float32)
        W = (rng.standard_normal((N, taps, Cc)) / np.sqrt(taps * Cc)).astype(np.float32)
        Whi = rnd(W, prec)
        Wp = np.concatenate([W, W, W - Whi], axis=2).reshape(N, taps * 3 * Cc)      # (the packer rounds each third)
        bias = rng.standard_normal(N).astype(np.float32)
        blk = x.astype(np.float64).reshape(B, T, Cc // 16, 16)
        st = np.stack([np.rint(blk.sum(axis=(1, 3)) * 2.0 ** 28), np.rint((blk ** 2).sum(axis=(1, 3)) * 2.0 ** 16)], axis=-1).astype(np.int64)
        d_x, d_g, d_b, d_t, d_s, d_bias = _dev(x.reshape(M, Cc)), _dev(gam), _dev(bet), _dev(temb), DevBuf.from_numpy(st), _dev(bias)
        d_w, d_wp = _pack(W.reshape(N, taps * Cc), prec), _pack(Wp, prec)
        outs, planes = [], []
        for pair in (0, 1):
            wd = 2 * Cc if pair else Cc
            d_a = OpBuf(np.full((M, wd), np.nan, dtype=np.float32), prec)
            d_o = DevBuf(M * N * 4)
            d_o.upload(np.full((M, N), np.nan, dtype=np.float32))
            g = GemmArgs()
            g.a0 = d_a.ptr; g.lda0 = wd; g.c0 = wd
            if pair:
                g.a1 = d_a.ptr; g.lda1 = wd; g.c1 = Cc; g.gnp_pair = 1
            g.B, g.Tin, g.Tout, g.M = B, T, T, M
            g.taps, g.tmode = taps, 0
            g.w = (d_wp if pair else d_w).value; g.K = taps * (3 if pair else 1) * Cc; g.N = N; g.bias = d_bias.ptr
            g.out_f32 = d_o.ptr; g.ldo_f32 = N
            g.algo = 2
            g.gnp_x = d_x.ptr; g.gnp_ldx = Cc; g.gnp_stats = d_s.ptr; g.gnp_gamma = d_g.ptr; g.gnp_beta = d_b.ptr
            g.gnp_temb = d_t.ptr if temb_on else None; g.gnp_ldtemb = ldt; g.gnp_eps = 1e-5; g.gnp_G = Gn; g.gnp_silu = silu
            check(lib.ns2vc_debug_set_gemm_tile(*tile), "set tile")
            try:
                check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
                sync()
                if pair:
                    g.algo = 1
                    assert lib.ns2vc_k_gemm(C.byref(g), prec, None) != 0
            finally:
                lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
            outs.append(d_o.to_numpy((M, N))); planes.append(d_a.read())
        lib.ns2vc_dev_free(d_w); lib.ns2vc_dev_free(d_wp)
        xg = x.astype(np.float64).reshape(B, T, Gn, Cc // Gn)
        mean, var = xg.mean(axis=(1, 3), keepdims=True), xg.var(axis=(1, 3), keepdims=True)
        y = ((xg - mean) / np.sqrt(var + 1e-5)).reshape(B, T, Cc) * gam.astype(np.float64) + bet.astype(np.float64)
        if temb_on:
            y = y * (1.0 + temb[:, None, :Cc].astype(np.float64)) + temb[:, None, Cc:2 * Cc].astype(np.float64)
        if silu:
            y = y / (1.0 + np.exp(-y))
        ref = gather_rows(y, B, T, T, taps, 0).reshape(M, taps * Cc) @ W.reshape(N, taps * Cc).astype(np.float64).T + bias
        hi, lo = planes[1][:, :Cc], planes[1][:, Cc:]
        same_hi = np.array_equal(hi, planes[0])
        e_pair = rel_l2(hi.astype(np.float64) + lo.astype(np.float64), y.reshape(M, Cc))
        e0, e1 = rel_l2(outs[0], ref), rel_l2(outs[1], ref)
        diag(f"conv on hi + lo operand pairs tile={tile} prec={prec} B={B} T={T} C={Cc} N={N} temb={temb_on} silu={silu}: hi plane == plain rows {same_hi}; hi + lo vs fp64 rows {e_pair:.2e}; "
             f"result vs the fp64 conv of unrounded rows and weights: plain {e0:.2e}, pair {e1:.2e}")
        assert same_hi and np.isfinite(outs[1]).all()
        assert e_pair < tol_pair_rows(prec) and e1 < 0.02 * e0


@pytest.mark.parametrize("algo", [2, 0], ids=["prologue", "inloop"])
@pytest.mark.parametrize("level", [(938, 128, 128), (235, 384, 384), (118, 512, 512)], ids=lambda l: f"T{l[0]}c{l[1]}")
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_gemm_groupnorm_prologue_is_reproducible_at_the_bench_shape(prec, level, algo, diag):
    """The fused launch at the bench shape (32 x 938 rows, 128 -> 128 channels, k = 3; the loader / consumer tiles), eight times:
    operand rows and results equal the two-launch path bit for bit EVERY time.  This is the probe that showed round 3's
    "gamma reads zero" failure (a packed fp32 product formed under outstanding LDS reads came back as 0.0 for lanes 48-63 of a
    few waves per launch; tools/gnp_probe.py, profiles/r04_gn_prologue_rootcause.txt): it failed 22 of 22 launches before the
    fix and must stay at zero.  The coarser levels (384 / 512 channels: 3 / 4 column tiles per row block) run the COOPERATIVE form
    (gnp_sync), the arrival words zeroed before every launch as the engine's per-forward clear does: same bits, and no workgroup waits in
    vain for a sibling."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    B, taps = 32, 3
    T, Cc, N = level
    rng = np.random.default_rng(0)
    M, K = B * T, taps * Cc
    x = rng.standard_normal((B, T, Cc)).astype(np.float32)
    gam, bet = (1.0 + np.arange(Cc) / 256.0).astype(np.float32), (np.arange(Cc) / 64.0 + 0.25).astype(np.float32)
    blk = x.astype(np.float64).reshape(B, T, Cc // 16, 16)
    st = np.stack([np.rint(blk.sum(axis=(1, 3)) * 2.0 ** 28), np.rint((blk ** 2).sum(axis=(1, 3)) * 2.0 ** 16)], axis=-1).astype(np.int64)
    W = rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec)
    d_x, d_g, d_b, d_st, d_w = _dev(x.reshape(M, Cc)), _dev(gam), _dev(bet), DevBuf.from_numpy(st), _pack(W, prec)
    d_sync, d_alone = DevBuf.from_numpy(np.zeros((M + 63) // 64, dtype=np.uint64)), DevBuf.from_numpy(np.zeros(1, dtype=np.uint32))

    def run(fused, rep):
        d_a = OpBuf(np.full((M, Cc), np.nan, dtype=np.float32), prec)
        d_o = DevBuf(M * N * 4)
        d_o.upload(np.full((M, N), float(rep), dtype=np.float32))
        g = GemmArgs()
        g.a0 = d_a.ptr; g.lda0 = Cc; g.c0 = Cc
        g.B, g.Tin, g.Tout, g.M = B, T, T, M
        g.taps, g.tmode = taps, 0
        g.w = d_w.value; g.K = K; g.N = N
        g.out_f32 = d_o.ptr; g.ldo_f32 = N
        g.algo = algo                                    # 2: the materialising prologue; 0: the tap-sharing kernel normalises inside its K loop (r6; a0 stays untouched)
        if fused:
            g.gnp_x = d_x.ptr; g.gnp_ldx = Cc; g.gnp_stats = d_st.ptr; g.gnp_gamma = d_g.ptr; g.gnp_beta = d_b.ptr
            g.gnp_eps = 1e-5; g.gnp_G = 8; g.gnp_silu = 1
            d_sync.upload(np.zeros((M + 63) // 64, dtype=np.uint64))
            g.gnp_sync = d_sync.ptr; g.gnp_alone = d_alone.ptr
        else:
            check(lib.ns2vc_k_groupnorm_stats(d_x.ptr, Cc, Cc, d_st.ptr, B, T, 8, 1e-5, d_g.ptr, d_b.ptr, None, 0, 0, 1, d_a.ptr, prec, None), "groupnorm_stats")
        check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
        sync()
        return d_a.read(), d_o.to_numpy((M, N))

    ref_a, ref_o = run(0, 0)
    bad = 0
    for rep in range(8):
        a, o = run(1, rep + 1)
        rows_ok = np.array_equal(a, ref_a) if algo == 2 else bool(np.isnan(a).all())      # (in-loop: nothing is written to the operand tensor)
        bad += int(not (rows_ok and np.array_equal(o, ref_o)))
    lib.ns2vc_dev_free(d_w)
    alone = int(d_alone.to_numpy((1,), dtype=np.uint32)[0])
    diag(f"gemm+GroupNorm prologue at the bench shape T={T} C={Cc} N={N} prec={prec}: {bad} of 8 fused launches differ from the two-launch path; "
         f"{alone} workgroups waited in vain for a sibling")
    assert bad == 0 and alone == 0



@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_gemm_epilogue_groupnorm_stats(prec, diag):
    """The epilogue's int64 fixed-point (sum, sumsq) per (batch item, 16-channel block) == numpy on the stored result,
    for every tile shape, with row tiles that straddle batch boundaries (T = 167 is not a multiple of 32)."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(5)
    B, T, c0, N = 3, 167, 128, 256
    for tile in [(0, 0, 0), (64, 128, 2), (64, 64, 2), (128, 128, 13), (64, 128, 13), (128, 128, 23), (64, 128, 23), (128, 64, 54), (128, 128, 54), (128, 64, 58), (128, 128, 58), (128, 64, 64), (128, 64, 68)]:
        a0 = rnd(rng.standard_normal((B, T, c0)), prec)
        W = rnd(rng.standard_normal((N, 3 * c0)) / np.sqrt(3 * c0), prec)
        bias = rng.standard_normal(N).astype(np.float32)
        res = rng.standard_normal((B * T, N)).astype(np.float32)
        d_a, d_w, d_b, d_r = OpBuf(a0, prec), _pack(W, prec), _dev(bias), _dev(res)
        d_o = DevBuf(B * T * N * 4)
        d_s = DevBuf.from_numpy(np.zeros((B, N // 16, 2), dtype=np.int64))
        g = GemmArgs()
        g.a0 = d_a.ptr; g.lda0 = c0; g.c0 = c0
        g.B, g.Tin, g.Tout, g.M = B, T, T, B * T
        g.taps, g.tmode = 3, 0
        g.w = d_w.value; g.K = 3 * c0; g.N = N
        g.bias = d_b.ptr; g.res = d_r.ptr; g.ldres = N
        g.out_f32 = d_o.ptr; g.ldo_f32 = N
        g.stats = d_s.ptr
        check(lib.ns2vc_debug_set_gemm_tile(*tile), "tile")
        try:
            check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
            sync()
        finally:
            lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
        out = d_o.to_numpy((B, T, N)).astype(np.float64)
        st = d_s.to_numpy((B, N // 16, 2), dtype=np.int64).astype(np.float64)
        blk = out.reshape(B, T, N // 16, 16)
        ref_s, ref_q = blk.sum(axis=(1, 3)), (blk ** 2).sum(axis=(1, 3))
        e_s = np.abs(st[..., 0] / 2 ** 28 - ref_s).max() / np.abs(ref_s).max()
        e_q = np.abs(st[..., 1] / 2 ** 16 - ref_q).max() / np.abs(ref_q).max()
        diag(f"gemm epilogue stats tile={tile} prec={prec}: sum {e_s:.2e} sumsq {e_q:.2e}")
        assert e_s < 1e-5 and e_q < 1e-5
        lib.ns2vc_dev_free(d_w)


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(0, 0, 0), (64, 128, 2), (64, 64, 2), (64, 128, 13), (128, 128, 13), (64, 128, 23), (128, 128, 23)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_layernorm_by_linearity(tile, prec, diag):
    """LayerNorm(y) @ W'^T without a normalisation pass (attention.py:83,102,118): the producer GEMM leaves (sum, sumsq)
    per row and 64-column slice and an operand copy of y; the consumer GEMM reads the raw copy and applies
    rstd * (acc - mean * rowsum(W')) + b in its epilogue.  Checked against numpy LayerNorm -> matmul in fp64,
    plain and GEGLU consumers, rows with a large mean (cancellation) included."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(11)
    B, T, D = 3, 83, 256                      # M = 249: row tail in every tile
    M = B * T
    # ---- producer: y = a @ W1^T + b1 + res  (fp32 + operand copy + row statistics)
    a = rnd(rng.standard_normal((M, D)), prec)
    W1 = rnd(rng.standard_normal((D, D)) / np.sqrt(D), prec)
    b1 = rng.standard_normal(D).astype(np.float32)
    res = (rng.standard_normal((M, D)) + 3.0 * rng.standard_normal((M, 1))).astype(np.float32)   # per-row offsets: |mean| up to ~3 sigma
    d_a, d_w1, d_b1, d_res = OpBuf(a, prec), _pack(W1, prec), _dev(b1), _dev(res)
    d_y = DevBuf(M * D * 4)
    d_yop = DevBuf(M * D * (4 if prec == 0 else 2))
    d_rs = DevBuf.from_numpy(np.full((M, D // 64, 2), np.nan, dtype=np.float32))     # every slot must be written
    g = GemmArgs()
    g.a0 = d_a.ptr; g.lda0 = D; g.c0 = D
    g.B, g.Tin, g.Tout, g.M = B, T, T, M
    g.taps, g.tmode = 1, 0
    g.w = d_w1.value; g.K = D; g.N = D; g.bias = d_b1.ptr
    g.res = d_res.ptr; g.ldres = D
    g.out_f32 = d_y.ptr; g.ldo_f32 = D
    g.out_op = d_yop.ptr; g.ldo_op = D
    g.rowstats = d_rs.ptr
    try:
        check(lib.ns2vc_debug_set_gemm_tile(*(tile if tile[1] != 64 else (0, 0, 0))), "tile")   # producers need 64-column wave tiles
        check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "producer gemm")
        sync()
        check(lib.ns2vc_debug_set_gemm_tile(*tile), "tile")
        y = d_y.to_numpy((M, D)).astype(np.float64)
        st = d_rs.to_numpy((M, D // 64, 2)).astype(np.float64)
        ys = y.reshape(M, D // 64, 64)
        e_s = np.abs(st[..., 0] - ys.sum(2)).max() / np.abs(ys.sum(2)).max()
        e_q = np.abs(st[..., 1] - (ys ** 2).sum(2)).max() / (ys ** 2).sum(2).max()
        diag(f"ln-linear producer tile={tile} prec={prec}: slice sums {e_s:.2e} slice sumsq {e_q:.2e}")
        assert e_s < TOL_STATS and e_q < TOL_STATS
        # ---- consumers
        mu = y.mean(1, keepdims=True)
        yn = (y - mu) / np.sqrt(y.var(1, keepdims=True) + 1e-5)
        for geglu, N in ((0, 384), (1, 512)):
            W2 = rnd(rng.standard_normal((N, D)) / np.sqrt(D), prec)
            b2 = rng.standard_normal(N).astype(np.float32)
            d_w2, d_b2 = _pack(W2, prec), _dev(b2)
            ws = C.c_void_p()
            W2c = np.ascontiguousarray(W2, dtype=np.float32)
            check(lib.ns2vc_weight_rowsum(W2c.ctypes.data, N, D, prec, C.byref(ws)), "rowsum")
            Nout = N // 2 if geglu else N
            d_o = DevBuf(M * Nout * 4)
            g2 = GemmArgs()
            g2.a0 = d_yop.ptr; g2.lda0 = D; g2.c0 = D
            g2.B, g2.Tin, g2.Tout, g2.M = B, T, T, M
            g2.taps, g2.tmode = 1, 0
            g2.w = d_w2.value; g2.K = D; g2.N = N; g2.bias = d_b2.ptr
            g2.geglu = geglu
            g2.out_f32 = d_o.ptr; g2.ldo_f32 = Nout
            g2.ln_stats = d_rs.ptr; g2.ln_wsum = ws.value; g2.ln_eps = 1e-5; g2.ln_dim = D
            if geglu and tile[1] not in (0, 128):
                continue
            check(lib.ns2vc_k_gemm(C.byref(g2), prec, None), "consumer gemm")
            sync()
            out = d_o.to_numpy((M, Nout)).astype(np.float64)
            pre = yn @ W2.astype(np.float64).T + b2
            if geglu:   # packed layout: groups of (32 value | 32 gate) columns
                from scipy.special import erf
                pg = pre.reshape(M, N // 64, 2, 32)
                ref = (pg[:, :, 0] * 0.5 * pg[:, :, 1] * (1.0 + erf(pg[:, :, 1] / np.sqrt(2.0)))).reshape(M, Nout)
            else:
                ref = pre
            e = rel_l2(out, ref)
            diag(f"ln-linear consumer tile={tile} prec={prec} geglu={geglu}: rel_l2 {e:.3e}")
            # fp32: exact up to rounding; 16-bit: the raw operand copy is rounded BEFORE normalisation (eps of |y|, not of |y - mean|)
            assert e < tol_ln_linear(prec)
            lib.ns2vc_dev_free(d_w2); lib.ns2vc_dev_free(ws)
    finally:
        lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
    lib.ns2vc_dev_free(d_w1)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_layernorm_plans_vs_row_offset(prec, diag):
    """LayerNorm by linearity multiplies the RAW rows (rounded to the operand type BEFORE centring) and fixes
    the mean up afterwards, so in the 16-bit modes its error on a row grows with |mean| / std; the explicit plan
    (ln_apply kernel: normalise in fp32, then round) does not.  Both plans against numpy fp64 for row offsets of
    0 / 10 / 100 standard deviations; the health word reports the ratio that Denoiser's guard keys on."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(23)
    B, T, D, N = 2, 150, 256, 384
    M = B * T
    W = rnd(rng.standard_normal((N, D)) / np.sqrt(D), prec)
    bias = rng.standard_normal(N).astype(np.float32)
    d_w, d_b = _pack(W, prec), _dev(bias)
    ws = C.c_void_p()
    Wc = np.ascontiguousarray(W, dtype=np.float32)
    check(lib.ns2vc_weight_rowsum(Wc.ctypes.data, N, D, prec, C.byref(ws)), "rowsum")
    eps = eps16(prec)
    res = {}
    for off in (0.0, 10.0, 100.0):
        y = (rng.standard_normal((M, D)) + off * np.sign(rng.standard_normal((M, 1)))).astype(np.float32)
        mu = y.astype(np.float64).mean(1, keepdims=True)
        yn = (y - mu) / np.sqrt(y.astype(np.float64).var(1, keepdims=True) + 1e-5)
        ref = yn @ W.astype(np.float64).T + bias
        # ---- linear plan: raw operand copy + per-slice statistics (what a producer GEMM's epilogue leaves)
        ys = y.astype(np.float64).reshape(M, D // 64, 64)
        stats = np.stack([ys.sum(2), (ys ** 2).sum(2)], axis=-1).astype(np.float32)
        d_raw, d_st = OpBuf(y, prec), _dev(stats)
        d_health = DevBuf.from_numpy(np.zeros(16, dtype=np.uint32))
        d_o = DevBuf(M * N * 4)
        g = GemmArgs()
        g.a0 = d_raw.ptr; g.lda0 = D; g.c0 = D
        g.B, g.Tin, g.Tout, g.M = B, T, T, M
        g.taps, g.tmode = 1, 0
        g.w = d_w.value; g.K = D; g.N = N; g.bias = d_b.ptr
        g.out_f32 = d_o.ptr; g.ldo_f32 = N
        g.ln_stats = d_st.ptr; g.ln_wsum = ws.value; g.ln_eps = 1e-5; g.ln_dim = D
        g.ln_health = d_health.ptr
        check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "consumer gemm")
        sync()
        e_lin = rel_l2(d_o.to_numpy((M, N)), ref)
        ratio = float(d_health.to_numpy((16,), dtype=np.uint32)[:1].view(np.float32)[0])
        # ---- explicit plan: ln_apply kernel (fp32 rows -> normalised operand rows), then the plain GEMM
        d_y = _dev(y)
        d_n = OpBuf(np.zeros((M, D), dtype=np.float32), prec)
        check(lib.ns2vc_k_layernorm_apply(d_y.ptr, D, M, D, 1e-5, d_n.ptr, prec, None), "ln_apply")
        g2 = GemmArgs()
        g2.a0 = d_n.ptr; g2.lda0 = D; g2.c0 = D
        g2.B, g2.Tin, g2.Tout, g2.M = B, T, T, M
        g2.taps, g2.tmode = 1, 0
        g2.w = d_w.value; g2.K = D; g2.N = N; g2.bias = d_b.ptr
        g2.out_f32 = d_o.ptr; g2.ldo_f32 = N
        check(lib.ns2vc_k_gemm(C.byref(g2), prec, None), "plain gemm")
        sync()
        e_exp = rel_l2(d_o.to_numpy((M, N)), ref)
        res[off] = (e_lin, e_exp, ratio)
        diag(f"LayerNorm plans prec={prec} row offset {off:5.1f} sigma: by linearity {e_lin:.3e}  explicit {e_exp:.3e}  reported |mean|/std {ratio:.2f}")
        assert e_exp < 2 * eps                                   # explicit: the precision's own rounding, whatever the offset
        assert e_lin < 2 * eps * max(1.0, 1.5 * off)             # linearity: grows ~linearly with the offset ...
        assert (ratio < 1.0) if off == 0 else (abs(ratio - off) < 0.35 * off)      # ... which the health word reports
    assert res[100.0][0] > 10 * res[100.0][1]                    # (the documented weakness is real: that is why the guard exists)
    lib.ns2vc_dev_free(d_w); lib.ns2vc_dev_free(ws)


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_gemm_fused_shortcut_segment(prec, diag):
    """conv3(hn) + conv1x1(x) in one launch: K = taps*c0 + c2 with the second segment on another operand tensor
    (taps = 3: resnet conv2 + shortcut; taps = 1: ff.net.2 folded into proj_out, [Wpo W2 | Wpo] [g | y] + residual)."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(9)
    for (B, T, c0, c2, N, taps) in [(2, 37, 128, 192, 128, 3), (3, 70, 256, 640, 256, 3), (2, 83, 512, 128, 128, 1), (3, 70, 1024, 256, 256, 1)]:
        M = B * T
        hn = rnd(rng.standard_normal((B, T, c0)), prec)
        x = rnd(rng.standard_normal((B, T, c2)), prec)
        W = rnd(rng.standard_normal((N, taps * c0 + c2)) / np.sqrt(taps * c0 + c2), prec)
        bias = rng.standard_normal(N).astype(np.float32)
        res = rng.standard_normal((M, N)).astype(np.float32)
        G = gather_rows(hn.astype(np.float64), B, T, T, taps, 0).reshape(M, taps * c0)
        ref = G @ W[:, :taps * c0].astype(np.float64).T + x.reshape(M, c2).astype(np.float64) @ W[:, taps * c0:].astype(np.float64).T + bias + res
        d_h, d_x, d_w, d_b, d_r = OpBuf(hn, prec), OpBuf(x, prec), _pack(W, prec), _dev(bias), _dev(res)
        d_o = DevBuf(M * N * 4)
        g = GemmArgs()
        g.a0 = d_h.ptr; g.lda0 = c0; g.c0 = c0
        g.a2 = d_x.ptr; g.lda2 = c2; g.c2 = c2
        g.B, g.Tin, g.Tout, g.M = B, T, T, M
        g.taps, g.tmode = taps, 0
        g.w = d_w.value; g.K = taps * c0 + c2; g.N = N; g.bias = d_b.ptr
        g.res = d_r.ptr; g.ldres = N
        g.out_f32 = d_o.ptr; g.ldo_f32 = N
        check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
        sync()
        e = rel_l2(d_o.to_numpy((M, N)), ref)
        diag(f"gemm fused second K segment {(B, T, c0, c2, N, taps)} prec={prec}: {e:.3e}")
        assert e < TOL[prec]
        lib.ns2vc_dev_free(d_w)


def test_fp16_operand_stores_saturate(diag):
    """fp16 operand stores clamp finite overflow to +-65504 (MODE.FP16_OVFL, set at kernel entry) instead of producing inf:
    a GEMM whose results reach ~2e5 writes an operand copy equal to the fp32 result clipped to +-65504 and then rounded."""
    from ns2vc_amd._lib import GemmArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(31)
    B, T, K, N = 2, 70, 128, 128
    M = B * T
    a = rnd(1000.0 * rng.standard_normal((B, T, K)), 2)
    W = rnd(10.0 * rng.standard_normal((N, K)), 2)
    d_a, d_w = OpBuf(a, 2), _pack(W, 2)
    d_o = DevBuf(M * N * 4)
    d_op = OpBuf(np.zeros((M, N), dtype=np.float32), 2)
    g = GemmArgs()
    g.a0 = d_a.ptr; g.lda0 = K; g.c0 = K
    g.B, g.Tin, g.Tout, g.M = B, T, T, M
    g.taps, g.tmode = 1, 0
    g.w = d_w.value; g.K = K; g.N = N
    g.out_f32 = d_o.ptr; g.ldo_f32 = N
    g.out_op = d_op.ptr; g.ldo_op = N
    check(lib.ns2vc_k_gemm(C.byref(g), 2, None), "k_gemm")
    sync()
    out, op = d_o.to_numpy((M, N)), d_op.read()
    n_over = int((np.abs(out) > 65504).sum())
    diag(f"fp16 saturating stores: {n_over} of {out.size} results beyond 65504, max |result| {np.abs(out).max():.3e}, max |operand copy| {np.abs(op).max():.1f}")
    assert n_over > 100 and np.isfinite(op).all()
    assert np.array_equal(op, f16_round(np.clip(out, -65504.0, 65504.0)))
    lib.ns2vc_dev_free(d_w)


def test_gemm_heuristic_large(diag):
    """A level-0 sized problem (M = 4*938) goes through the tile heuristic."""
    rng = np.random.default_rng(7)
    for prec in PRECS:
        out, ref, _ = run_gemm(rng, prec, 4, 938, 938, 128, 0, 128, 3, 0, 1, 1, 0, 0)
        e = rel_l2(out, ref)
        diag(f"gemm level0 prec={prec} rel_l2={e:.3e}")
        assert e < TOL[prec]


# (name, B, T of the level, c0, c1, N, taps, geglu): the GEMM shapes of the BENCH plan (10 s x batch 32) that take the
# heuristic's big-M branches (M >= 7000 / >= 12000 rows), which no small test reaches
BENCH_GEMMS = [
    ("l0.linear", 32, 938, 128, 0, 128, 1, 0),        # to_out / proj: 64x128 ring 3
    ("l0.qkv", 32, 938, 128, 0, 384, 1, 0),           # short K, N > 128: 128x128 ring 2
    ("l0.geglu", 32, 938, 128, 0, 1024, 1, 1),        # narrow GEGLU: 4-wave kernel
    ("l0.conv3_concat", 32, 938, 128, 128, 128, 3, 0),  # K = 12 tiles: 128x128 ring 3
    ("l1.geglu", 32, 469, 256, 0, 2048, 1, 1),        # wide GEGLU: 128x128 ring 2
    ("l1.qkv", 32, 469, 256, 0, 768, 1, 0),
    ("l2.conv3", 32, 235, 384, 0, 384, 3, 0),         # M = 7520: big_m with long K
]


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", BENCH_GEMMS, ids=[c[0] for c in BENCH_GEMMS])
def test_gemm_bench_shapes(case, prec, diag):
    """The exact (M, N, K) of the benchmarked launch plan, default tile heuristic, against numpy fp64."""
    name, B, T, c0, c1, N, taps, geglu = case
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    out, ref, out_op = run_gemm(rng, prec, B, T, T, c0, c1, N, taps, 0, 1, 0 if geglu else 1, geglu, 1)
    e = rel_l2(out, ref)
    diag(f"gemm bench shape {name} prec={prec} M={B * T} rel_l2={e:.3e}")
    assert e < TOL[prec]
    assert np.array_equal(out_op, rnd(out, prec)), name


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M,ldo_extra", [(7520, 0), (128, 0), (97, 64), (1, 0), (1285, 8)], ids=str)
def test_geglu_token_stationary(M, ldo_extra, prec, diag):
    """The token-stationary GEGLU projection (csrc/geglu.hip, dim 384) against numpy fp64 of
        h = (n W1v^T + b1v) * gelu(n W1g^T + b1g),  n = LayerNorm(y)
    with the engine's pack-time folds (gamma / beta into W1 / b1, value|gate row interleave) and the kernel's rounding points (operands rounded,
    LayerNorm by linearity from the per-64-channel row sums).  Row counts: the benchmarked 7520 (59 token blocks, the last one short), one full
    block, a short one, a single row, an odd count; an output pitch wider than 4 dim leaves the columns beyond untouched.  Every result element
    is written exactly once: the buffer starts as NaN."""
    from scipy.special import erf
    from ns2vc_amd._lib import GegluArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    d = 384
    rng = np.random.default_rng(M * 7 + prec)
    y = (rng.standard_normal((M, d)) + 1.5 * rng.standard_normal((M, 1))).astype(np.float32)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(d)), 0.2 * rng.standard_normal(d)
    W1, b1 = rng.standard_normal((8 * d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(8 * d)
    W1f, b1f = W1 * gamma[None, :], b1 + W1 @ beta
    order = np.concatenate([np.concatenate([np.arange(32 * g, 32 * g + 32), 4 * d + np.arange(32 * g, 32 * g + 32)]) for g in range(4 * d // 32)])
    W1p, b1p = np.ascontiguousarray(W1f[order].astype(np.float32)), np.ascontiguousarray(b1f[order].astype(np.float32))
    W1r, yr = rnd(W1p, prec).astype(np.float64), rnd(y, prec).astype(np.float64)
    y64 = y.astype(np.float64)
    mean, var = y64.mean(1, keepdims=True), y64.var(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    pre = rstd * (yr @ W1r.T - mean * W1r.sum(1).astype(np.float32).astype(np.float64)[None, :]) + b1p.astype(np.float64)[None, :]
    pg = pre.reshape(M, 4 * d // 32, 2, 32)
    ref = (pg[:, :, 0] * 0.5 * pg[:, :, 1] * (1.0 + erf(pg[:, :, 1] / np.sqrt(2.0)))).reshape(M, 4 * d)
    ys = y64.reshape(M, d // 64, 64)
    stats = np.stack([ys.sum(2), (ys ** 2).sum(2)], axis=-1).astype(np.float32)
    stream, consts = C.c_void_p(), C.c_void_p()
    check(lib.ns2vc_pack_geglu(W1p.ctypes.data, b1p.ctypes.data, d, prec, C.byref(stream), C.byref(consts)), "pack_geglu")
    ldo = 4 * d + ldo_extra
    d_y, d_st = OpBuf(y, prec), _dev(stats)
    d_h = OpBuf(np.full((M, ldo), np.nan, dtype=np.float32), prec)
    d_health = DevBuf.from_numpy(np.zeros(16, dtype=np.uint32))
    f = GegluArgs()
    f.yn = d_y.ptr; f.ldy = d; f.ln_stats = d_st.ptr; f.ln_eps = 1e-5
    f.wstream = stream.value; f.consts = consts.value
    f.out_op = d_h.ptr; f.ldo = ldo; f.M = M; f.dim = d; f.ln_health = d_health.ptr
    check(lib.ns2vc_k_geglu(C.byref(f), prec, None), "k_geglu")
    sync()
    h = d_h.read().reshape(M, ldo)
    out = h[:, :4 * d]
    e = rel_l2(out, ref)
    ratio = float(d_health.to_numpy((16,), dtype=np.uint32)[:1].view(np.float32)[0])
    diag(f"geglu token-stationary M={M} ldo={ldo} prec={prec}: rel_l2 {e:.3e} (rounding {eps16(prec):.1e}) nan={int(np.isnan(out).sum())} |mean|/std {ratio:.2f}")
    # the result is stored in the operand type: it must be the rounded reference up to one-ulp flips where fp32 accumulation moved a value across a tie
    flips = float(np.mean(out != rnd(ref.astype(np.float32), prec)))
    if not (e < eps16(prec) and flips < 0.03):
        err = np.abs(out - ref)
        bad = np.argwhere(~(err <= 2e-2 + 2e-2 * np.abs(ref)))
        diag(f"  FAIL: flips {flips:.4f}; {len(bad)} bad of {out.size}; rows {sorted(set(bad[:, 0].tolist()))[:16]} cols {sorted(set(bad[:, 1].tolist()))[:24]}")
    assert np.isfinite(out).all() and e < eps16(prec) and flips < GEGLU_FLIPS
    assert np.isnan(h[:, 4 * d:]).all()
    assert (0.2 if M > 1 else 0.0) < ratio < 12.0      # (max over rows of |mean| / std: a single row can have any)
    # the same launch twice: bitwise equal (no accumulation order depends on timing)
    d_h2 = OpBuf(np.full((M, ldo), np.nan, dtype=np.float32), prec)
    f.out_op = d_h2.ptr
    check(lib.ns2vc_k_geglu(C.byref(f), prec, None), "k_geglu")
    sync()
    assert np.array_equal(d_h2.read().reshape(M, ldo)[:, :4 * d], out)
    # refused: any other dim, a misaligned output
    f.dim = 256
    assert lib.ns2vc_k_geglu(C.byref(f), prec, None) != 0
    f.dim = d; f.out_op = d_h2.ptr + 2
    assert lib.ns2vc_k_geglu(C.byref(f), prec, None) != 0
    f.out_op = d_h2.ptr; f.ldo = 4 * d - 8          # an output pitch narrower than the hidden width
    assert lib.ns2vc_k_geglu(C.byref(f), prec, None) != 0
    lib.ns2vc_dev_free(stream); lib.ns2vc_dev_free(consts)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("prestage", [False, True], ids=["plain", "pre"])
@pytest.mark.parametrize("dim,B,T", [(128, 3, 150), (256, 2, 97), (128, 1, 64), (256, 5, 200)], ids=str)
def test_ffn_fused(dim, B, T, prestage, prec, diag):
    """The fused feed-forward + proj_out kernel (csrc/ffn.hip) against numpy fp64 of
        out = Wpo (y + W2 (GEGLU(LayerNorm(y) W1^T + b1)) + b2) + bpo + x
    with the engine's pack-time folds (LayerNorm gamma/beta into W1/b1, [Wpo W2 | Wpo], value|gate row interleave), the
    kernel's own rounding points modelled (operands and the hidden tensor are rounded to the operand type), rows with a
    common offset (LayerNorm by linearity), a row count that is no multiple of 64 and 64-token blocks that straddle batch
    items (GroupNorm statistics of the result per item).  prestage: y itself is computed inside the kernel as
    y = o Wo^T + bo + y_prev (attn2.to_out + residual) from operand-typed attention rows o and never stored."""
    from scipy.special import erf
    from ns2vc_amd._lib import FfnArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(dim * 1000 + B * 10 + T)
    d, M = dim, B * T
    y = (rng.standard_normal((M, d)) + 1.5 * rng.standard_normal((M, 1))).astype(np.float32)
    x = rng.standard_normal((M, d)).astype(np.float32)
    if prestage:  # y = o Wo^T + bo + y_prev with the kernel's rounding points (o and Wo rounded, fp32 accumulation)
        o = rng.standard_normal((M, d)).astype(np.float32)
        Wo, bo = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), (0.3 * rng.standard_normal(d)).astype(np.float32)
        y_prev = y
        y = (rnd(o, prec).astype(np.float64) @ rnd(Wo, prec).astype(np.float64).T + bo + y_prev).astype(np.float32)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(d)), 0.2 * rng.standard_normal(d)
    W1, b1 = rng.standard_normal((8 * d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(8 * d)
    W2, b2 = rng.standard_normal((d, 4 * d)) / np.sqrt(4 * d), 0.3 * rng.standard_normal(d)
    Wpo, bpo = rng.standard_normal((d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(d)
    # ---- pack-time folds (pack.cpp pack_all), fp64
    W1f, b1f = W1 * gamma[None, :], b1 + W1 @ beta
    order = np.concatenate([np.concatenate([np.arange(32 * g, 32 * g + 32), 4 * d + np.arange(32 * g, 32 * g + 32)]) for g in range(4 * d // 32)])
    W1p, b1p = W1f[order].astype(np.float32), b1f[order].astype(np.float32)
    w2f = np.concatenate([Wpo @ W2, Wpo], axis=1).astype(np.float32)
    bias2 = (Wpo @ b2 + bpo).astype(np.float32)
    W1r, w2r, yr = rnd(W1p, prec).astype(np.float64), rnd(w2f, prec).astype(np.float64), rnd(y, prec).astype(np.float64)
    consts = np.stack([W1r.sum(1), b1p.astype(np.float64)], axis=1).astype(np.float32)
    # ---- reference with the kernel's rounding points
    y64 = y.astype(np.float64)
    mean, var = y64.mean(1, keepdims=True), y64.var(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    pre = rstd * (yr @ W1r.T - mean * consts[:, 0].astype(np.float64)[None, :]) + b1p.astype(np.float64)[None, :]
    pg = pre.reshape(M, 4 * d // 32, 2, 32)
    h = (pg[:, :, 0] * 0.5 * pg[:, :, 1] * (1.0 + erf(pg[:, :, 1] / np.sqrt(2.0)))).reshape(M, 4 * d)
    hr = rnd(h.astype(np.float32), prec).astype(np.float64)
    ref = hr @ w2r[:, :4 * d].T + yr @ w2r[:, 4 * d:].T + bias2 + x
    # ---- device
    ys = y64.reshape(M, d // 64, 64)
    stats = np.stack([ys.sum(2), (ys ** 2).sum(2)], axis=-1).astype(np.float32)
    stream = C.c_void_p()
    if prestage:
        check(lib.ns2vc_pack_ffn_pre(np.ascontiguousarray(W1p).ctypes.data, np.ascontiguousarray(w2f).ctypes.data, np.ascontiguousarray(Wo).ctypes.data,
                                     d, prec, C.byref(stream)), "pack_ffn_pre")
    else:
        check(lib.ns2vc_pack_ffn(np.ascontiguousarray(W1p).ctypes.data, np.ascontiguousarray(w2f).ctypes.data, d, prec, C.byref(stream)), "pack_ffn")
    d_y, d_st, d_c, d_b2, d_x = OpBuf(y, prec), _dev(stats), _dev(consts), _dev(bias2), _dev(x)
    d_o = DevBuf(M * d * 4)
    d_o.upload(np.full((M, d), np.nan, dtype=np.float32))
    d_op = OpBuf(np.full((M, d), np.nan, dtype=np.float32), prec)
    d_gs = DevBuf.from_numpy(np.zeros((B, d // 16, 2), dtype=np.int64))
    d_health = DevBuf.from_numpy(np.zeros(16, dtype=np.uint32))
    f = FfnArgs()
    f.yn = d_y.ptr; f.ldy = d; f.ln_stats = d_st.ptr; f.ln_eps = 1e-5
    f.wstream = stream.value; f.consts = d_c.ptr; f.bias2 = d_b2.ptr
    f.res = d_x.ptr; f.ldres = d
    f.out_f32 = d_o.ptr; f.ldo_f32 = d; f.out_op = d_op.ptr; f.ldo_op = d
    f.stats = d_gs.ptr
    f.B, f.T, f.M, f.dim = B, T, M, d
    f.ln_health = d_health.ptr
    if prestage:
        d_oa, d_bo, d_yp = OpBuf(o, prec), _dev(bo), _dev(y_prev)
        f.yn = None; f.ln_stats = None
        f.pre_a = d_oa.ptr; f.pre_lda = d; f.pre_bias = d_bo.ptr; f.pre_res = d_yp.ptr; f.pre_ldres = d
    check(lib.ns2vc_k_ffn(C.byref(f), prec, None), "k_ffn")
    sync()
    out, op = d_o.to_numpy((M, d)), d_op.read()
    e = rel_l2(out, ref)
    gs = d_gs.to_numpy((B, d // 16, 2), dtype=np.int64).astype(np.float64)
    blk = out.astype(np.float64).reshape(B, T, d // 16, 16)
    e_s = np.abs(gs[..., 0] / 2 ** 28 - blk.sum(axis=(1, 3))).max() / np.abs(blk.sum(axis=(1, 3))).max()
    e_q = np.abs(gs[..., 1] / 2 ** 16 - (blk ** 2).sum(axis=(1, 3))).max() / (blk ** 2).sum(axis=(1, 3)).max()
    ratio = float(d_health.to_numpy((16,), dtype=np.uint32)[:1].view(np.float32)[0])
    diag(f"ffn fused dim={d} B={B} T={T} pre={prestage} prec={prec}: rel_l2 {e:.3e} nan={int(np.isnan(out).sum())}  stats sum {e_s:.2e} sumsq {e_q:.2e}  |mean|/std {ratio:.2f}")
    if not e < 2e-4:
        err = np.abs(out - ref)
        bad = np.argwhere(~(err <= 1e-2 + 1e-2 * np.abs(ref)))
        diag(f"  FAIL: {len(bad)} bad of {out.size}; rows {sorted(set(bad[:, 0].tolist()))[:16]} cols {sorted(set(bad[:, 1].tolist()))[:16]}")
    assert np.isfinite(out).all() and e < TOL_FFN
    assert np.array_equal(op, rnd(out, prec))
    assert e_s < TOL_STATS and e_q < TOL_STATS
    assert 0.5 < ratio < 12.0
    lib.ns2vc_dev_free(stream)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dim,B,T,Lk,masked", [(128, 3, 150, 69, True), (256, 2, 97, 130, True), (128, 2, 64, 469, False), (256, 3, 200, 33, True), (128, 1, 70, 1, False)], ids=str)
def test_ffn_fused_with_cross_attention(dim, B, T, Lk, masked, prec, diag):
    """r6 (ns2vc_ffn_args.att_*): the prompt cross-attention of attn2 (attention_processor.py:1032, mask bias unet_1d_condition.py:816-818) computed INSIDE the
    fused feed-forward kernel -- one wave per head, two passes over the keys, K and V^T fragments from ns2vc_k_xattn_pack's image of the hoisted k | v rows -- in front of
    attn2.to_out + residual -> LayerNorm -> GEGLU -> ff.net.2 -> proj_out.  Against (a) numpy fp64 of the whole chain with the kernel's rounding points (q, k, v,
    the probabilities and the attention output rounded to the operand type) and (b) the two-launch path on the device (ns2vc_k_attention + the pre-stage kernel):
    token blocks are cut per batch item (T no multiple of 64), keys no multiple of 32, ragged masks, a single key."""
    from scipy.special import erf
    from ns2vc_amd._lib import AttnArgs, FfnArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(dim * 1000 + B * 10 + T + Lk)
    d, M, H = dim, B * T, 8
    hd = d // H
    q = rnd(rng.standard_normal((B, T, d)), prec)
    kv_ld = 2 * d + 64                                             # k | v side by side inside wider rows, as in the engine's hoisted projection
    kv = np.zeros((B, Lk, kv_ld), np.float32)
    kv[..., :2 * d] = rnd(rng.standard_normal((B, Lk, 2 * d)), prec)
    k, v = kv[..., :d], kv[..., d:2 * d]
    bias = None
    if masked:
        lens = np.maximum(1, (Lk * (0.4 + 0.6 * rng.random(B))).astype(int)); lens[0] = Lk
        bias = ((np.arange(Lk)[None, :] >= lens[:, None]) * -10000.0).astype(np.float32)
    # attention reference with the kernel's rounding: probabilities relative to the row maximum, rounded; denominator from the rounded ones; output rounded
    qh = q.reshape(B, T, H, hd).transpose(0, 2, 1, 3).astype(np.float64)
    kh = k.reshape(B, Lk, H, hd).transpose(0, 2, 1, 3).astype(np.float64)
    vh = v.reshape(B, Lk, H, hd).transpose(0, 2, 1, 3).astype(np.float64)
    sc = qh @ kh.transpose(0, 1, 3, 2) / np.sqrt(hd)
    if bias is not None:
        sc = sc + bias[:, None, None, :]
    p = np.exp(sc - sc.max(-1, keepdims=True))
    pr_ = rnd(p.astype(np.float32), prec).astype(np.float64)
    o = ((pr_ @ vh) / pr_.sum(-1, keepdims=True)).transpose(0, 2, 1, 3).reshape(M, d)
    o_r = rnd(o.astype(np.float32), prec)
    y_prev = (rng.standard_normal((M, d)) + 1.5 * rng.standard_normal((M, 1))).astype(np.float32)
    x = rng.standard_normal((M, d)).astype(np.float32)
    Wo, bo = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), (0.3 * rng.standard_normal(d)).astype(np.float32)
    y = (o_r.astype(np.float64) @ rnd(Wo, prec).astype(np.float64).T + bo + y_prev).astype(np.float32)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(d)), 0.2 * rng.standard_normal(d)
    W1, b1 = rng.standard_normal((8 * d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(8 * d)
    W2, b2 = rng.standard_normal((d, 4 * d)) / np.sqrt(4 * d), 0.3 * rng.standard_normal(d)
    Wpo, bpo = rng.standard_normal((d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(d)
    W1f, b1f = W1 * gamma[None, :], b1 + W1 @ beta
    order = np.concatenate([np.concatenate([np.arange(32 * g, 32 * g + 32), 4 * d + np.arange(32 * g, 32 * g + 32)]) for g in range(4 * d // 32)])
    W1p, b1p = W1f[order].astype(np.float32), b1f[order].astype(np.float32)
    w2f = np.concatenate([Wpo @ W2, Wpo], axis=1).astype(np.float32)
    bias2 = (Wpo @ b2 + bpo).astype(np.float32)
    W1r, w2r, yr = rnd(W1p, prec).astype(np.float64), rnd(w2f, prec).astype(np.float64), rnd(y, prec).astype(np.float64)
    consts = np.stack([W1r.sum(1), b1p.astype(np.float64)], axis=1).astype(np.float32)
    y64 = y.astype(np.float64)
    mean, var = y64.mean(1, keepdims=True), y64.var(1, keepdims=True)
    pre = (1.0 / np.sqrt(var + 1e-5)) * (yr @ W1r.T - mean * consts[:, 0].astype(np.float64)[None, :]) + b1p.astype(np.float64)[None, :]
    pg = pre.reshape(M, 4 * d // 32, 2, 32)
    hcol = (pg[:, :, 0] * 0.5 * pg[:, :, 1] * (1.0 + erf(pg[:, :, 1] / np.sqrt(2.0)))).reshape(M, 4 * d)
    ref = rnd(hcol.astype(np.float32), prec).astype(np.float64) @ w2r[:, :4 * d].T + yr @ w2r[:, 4 * d:].T + bias2 + x
    # ---- device
    stream = C.c_void_p()
    check(lib.ns2vc_pack_ffn_pre(np.ascontiguousarray(W1p).ctypes.data, np.ascontiguousarray(w2f).ctypes.data, np.ascontiguousarray(Wo).ctypes.data,
                                 d, prec, C.byref(stream)), "pack_ffn_pre")
    d_q, d_kv = OpBuf(q.reshape(M, d), prec), OpBuf(kv.reshape(B * Lk, kv_ld), prec)
    d_bias = _dev(bias) if bias is not None else None
    d_vt = DevBuf(int(lib.ns2vc_xattn_pack_bytes(B, Lk, hd)))
    check(lib.ns2vc_k_xattn_pack(d_kv.ptr, kv_ld, d_kv.ptr + 2 * d, kv_ld, B, Lk, hd, d_vt.ptr, prec, None), "xattn_pack")
    d_c, d_b2, d_x, d_bo, d_yp = _dev(consts), _dev(bias2), _dev(x), _dev(bo), _dev(y_prev)
    outs = []
    for fused in (1, 0):
        d_o = DevBuf(M * d * 4)
        d_o.upload(np.full((M, d), np.nan, dtype=np.float32))
        d_gs = DevBuf.from_numpy(np.zeros((B, d // 16, 2), dtype=np.int64))
        f = FfnArgs()
        f.wstream = stream.value; f.consts = d_c.ptr; f.bias2 = d_b2.ptr
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
            d_ao = OpBuf(np.full((M, d), np.nan, dtype=np.float32), prec)
            a = AttnArgs()
            a.q = d_q.ptr; a.k = d_kv.ptr; a.v = d_kv.ptr + 2 * d; a.ldq = d; a.ldk = kv_ld; a.ldv = kv_ld
            a.B, a.H, a.Lq, a.Lk = B, H, T, Lk
            a.bias = d_bias.ptr if d_bias is not None else None
            a.scale = 1.0 / np.sqrt(hd); a.out = d_ao.ptr; a.ldo = d
            check(lib.ns2vc_k_attention(C.byref(a), hd, prec, None), "k_attention")
            f.pre_a = d_ao.ptr; f.pre_lda = d
        check(lib.ns2vc_k_ffn(C.byref(f), prec, None), "k_ffn")
        sync()
        outs.append((d_o.to_numpy((M, d)), d_gs.to_numpy((B, d // 16, 2), dtype=np.int64).astype(np.float64)))
    out, gs = outs[0]
    e, e2, e12 = rel_l2(out, ref), rel_l2(outs[1][0], ref), rel_l2(out, outs[1][0])
    blk = out.astype(np.float64).reshape(B, T, d // 16, 16)
    e_s = np.abs(gs[..., 0] / 2 ** 28 - blk.sum(axis=(1, 3))).max() / np.abs(blk.sum(axis=(1, 3))).max()
    diag(f"ffn + in-kernel cross-attention dim={d} B={B} T={T} Lk={Lk} mask={masked} prec={prec}: vs fp64 {e:.3e} (two-launch path {e2:.3e}; fused vs two-launch {e12:.3e})  "
         f"nan={int(np.isnan(out).sum())}  stats sum {e_s:.2e}")
    assert np.isfinite(out).all() and e < tol_ffn_xattn(prec) and e12 < (6e-4 if prec == 2 else 5e-3)
    assert e_s < TOL_STATS
    lib.ns2vc_dev_free(stream)


def ref_attention(q, k, v, bias, H, prec):
    B, Lq, D = q.shape
    Lk = k.shape[1]
    hd = D // H
    qh = q.reshape(B, Lq, H, hd).transpose(0, 2, 1, 3).astype(np.float64)
    kh = k.reshape(B, Lk, H, hd).transpose(0, 2, 1, 3).astype(np.float64)
    vh = v.reshape(B, Lk, H, hd).transpose(0, 2, 1, 3).astype(np.float64)
    s = qh @ kh.transpose(0, 1, 3, 2) / np.sqrt(hd)
    if bias is not None:
        s = s + bias[:, None, None, :]
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    p = p / p.sum(-1, keepdims=True)
    o = p @ vh
    return o.transpose(0, 2, 1, 3).reshape(B, Lq, D)


ATTN_CASES = [
    # name, B, H, hd, Lq, Lk, bias, packed_qkv
    ("self_hd16", 2, 8, 16, 150, 150, False, True),
    ("self_hd32", 2, 8, 32, 75, 75, False, True),
    ("self_hd48", 1, 8, 48, 130, 130, False, True),
    ("self_hd64", 2, 4, 64, 64, 64, False, True),
    ("self_tiny", 1, 2, 16, 5, 5, False, True),
    ("cross_hd16_mask", 2, 8, 16, 150, 69, True, False),
    ("cross_hd32_mask", 2, 8, 32, 70, 130, True, False),
    ("cross_hd48_mask", 2, 8, 48, 33, 21, True, False),
    ("cross_hd64_mask", 2, 8, 64, 40, 469, True, False),
    ("self_hd16_long", 1, 8, 16, 470, 470, False, True),
    ("cross_hd32_469", 2, 8, 32, 100, 469, True, False),
    ("cross_hd16_129", 1, 8, 16, 140, 129, True, False),
]


@pytest.mark.parametrize("keys", [0, 128], ids=["keys64", "keys128"])
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("case", ATTN_CASES, ids=[c[0] for c in ATTN_CASES])
def test_attention(case, prec, keys, diag):
    """keys: K/V tile size -- 0 = the default 64-key tiles; 128 = the 128-key kernels of the 16-bit hd 16 / 32 cases (tuning
    hook; measured slower in the step, kept tested)"""
    from ns2vc_amd._lib import AttnArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    name, B, H, hd, Lq, Lk, use_bias, packed = case
    lib = _lib()
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    D = H * hd
    q = rng.standard_normal((B, Lq, D)).astype(np.float32)
    k = rng.standard_normal((B, Lk, D)).astype(np.float32)
    v = rng.standard_normal((B, Lk, D)).astype(np.float32)
    bias = None
    if use_bias:
        keep = rng.random((B, Lk)) > 0.3
        keep[:, 0] = True
        keep[0, Lk // 2:] = False          # a padded tail, like a ragged prompt batch
        bias = np.where(keep, 0.0, -10000.0).astype(np.float32)
    ref = ref_attention(rnd(q, prec), rnd(k, prec), rnd(v, prec), bias, H, prec)
    a = AttnArgs()
    esz = 4 if prec == 0 else 2
    if packed:   # q|k|v interleaved per row, as the fused QKV GEMM writes them
        d_qkv = OpBuf(np.concatenate([q, k, v], axis=-1), prec)
        a.q, a.k, a.v = d_qkv.ptr, d_qkv.ptr + D * esz, d_qkv.ptr + 2 * D * esz
        a.ldq = a.ldk = a.ldv = 3 * D
    else:        # k|v side by side with extra columns around, as the hoisted cross K/V buffer
        pad = 64
        kv = np.concatenate([np.zeros((B, Lk, pad), np.float32), k, v, np.zeros((B, Lk, pad), np.float32)], axis=-1)
        d_q, d_kv = OpBuf(q, prec), OpBuf(kv, prec)
        a.q, a.k, a.v = d_q.ptr, d_kv.ptr + pad * esz, d_kv.ptr + (pad + D) * esz
        a.ldq, a.ldk, a.ldv = D, 2 * D + 2 * pad, 2 * D + 2 * pad
    a.B, a.H, a.Lq, a.Lk = B, H, Lq, Lk
    d_bias = _dev(bias) if bias is not None else None
    if d_bias is not None:
        a.bias = d_bias.ptr
    a.scale = 1.0 / np.sqrt(hd)
    d_out = OpBuf(np.full((B, Lq, D), np.nan, dtype=np.float32), prec)
    a.out, a.ldo = d_out.ptr, D
    check(lib.ns2vc_debug_set_attn_keys(keys), "set_attn_keys")
    try:
        check(lib.ns2vc_k_attention(C.byref(a), hd, prec, None), "k_attention")
        sync()
    finally:
        lib.ns2vc_debug_set_attn_keys(0)
    out = d_out.read((B, Lq, D))
    e = rel_l2(out, ref)
    diag(f"attn {name} prec={prec} rel_l2={e:.3e} nan={int(np.isnan(out).sum())}")
    tol = tol_attention(prec)
    if not e < tol:
        err = np.abs(out - ref).reshape(B, Lq, H, hd)
        diag(f"  FAIL {name}: per-head max err {err.max(axis=(0, 1, 3)).round(4).tolist()} per-d max {err.max(axis=(0, 1, 2)).round(3).tolist()[:16]}")
        diag(f"  per-q (b0,h0) {err[0, :, 0, :].max(-1).round(3).tolist()[:40]}")
    assert e < tol, (name, e)


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_attention_reference_shift_extremes(prec, diag):
    """The kernel keeps a per-query softmax REFERENCE instead of the running max (moved only when a score exceeds it by
    2^12): large logits, a sharply growing maximum, and a first key tile that is entirely masked must all stay exact."""
    from ns2vc_amd._lib import AttnArgs, check
    from ns2vc_amd.engine import sync
    lib = _lib()
    rng = np.random.default_rng(77)
    B, H, hd, Lq, Lk = 2, 4, 32, 96, 300
    D = H * hd
    q = (4.0 * rng.standard_normal((B, Lq, D))).astype(np.float32)          # logits of +-60 and more
    k = (3.0 * rng.standard_normal((B, Lk, D))).astype(np.float32)
    k *= np.linspace(0.2, 2.5, Lk, dtype=np.float32)[None, :, None]          # later keys produce ever larger scores
    v = rng.standard_normal((B, Lk, D)).astype(np.float32)
    keep = np.ones((B, Lk), dtype=bool)
    keep[0, :70] = False                                                       # the whole first 64-key tile is masked
    keep[1, 200:] = False
    bias = np.where(keep, 0.0, -10000.0).astype(np.float32)
    qr, kr, vr = (rnd(t, prec) for t in (q, k, v))
    ref = ref_attention(qr, kr, vr, bias, H, prec)
    esz = 4 if prec == 0 else 2
    a = AttnArgs()
    d_q, d_kv = OpBuf(q, prec), OpBuf(np.concatenate([k, v], axis=-1), prec)
    a.q, a.k, a.v = d_q.ptr, d_kv.ptr, d_kv.ptr + D * esz
    a.ldq, a.ldk, a.ldv = D, 2 * D, 2 * D
    a.B, a.H, a.Lq, a.Lk = B, H, Lq, Lk
    d_bias = _dev(bias)
    a.bias = d_bias.ptr
    a.scale = 1.0 / np.sqrt(hd)
    d_out = OpBuf(np.full((B, Lq, D), np.nan, dtype=np.float32), prec)
    a.out, a.ldo = d_out.ptr, D
    check(lib.ns2vc_k_attention(C.byref(a), hd, prec, None), "k_attention")
    sync()
    out = d_out.read((B, Lq, D))
    e = rel_l2(out, ref)
    diag(f"attn reference-shift extremes prec={prec}: rel_l2={e:.3e} nan={int(np.isnan(out).sum())} inf={int(np.isinf(out).sum())}")
    assert np.isfinite(out).all()
    assert e < (3e-5 if prec == 0 else 16 * eps16(prec)), e        # 16-bit: near one-hot softmax over rounded P / scaled Q


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
def test_attention_optimistic_pass_and_its_fallback(prec, diag):
    """16-bit attention first runs an OPTIMISTIC pass (reference = first tile's maximum + a margin, no per-tile maximum) and
    falls back to the exact pass when the denominator says a probability may have left the fp16 range (csrc/attn.hip OPT).
    (a) ordinary logits: both passes are within the operand rounding of fp64 and of each other; (b) scores that grow by far
    more than the margin along the keys, and a fully masked first tile: the optimistic result is rejected and the output is
    BITWISE the exact pass's (ns2vc_debug_set_attn_optimistic(0) = exact pass only)."""
    from ns2vc_amd._lib import AttnArgs, check
    from ns2vc_amd.engine import sync
    lib = _lib()
    rng = np.random.default_rng(91)
    B, H, hd, Lq, Lk = 2, 8, 16, 200, 333
    D = H * hd
    v = rng.standard_normal((B, Lk, D)).astype(np.float32)
    for case in ("ordinary", "growing", "masked_first_tile"):
        q = rng.standard_normal((B, Lq, D)).astype(np.float32) * (1.0 if case != "growing" else 4.0)
        k = rng.standard_normal((B, Lk, D)).astype(np.float32) * (1.0 if case != "growing" else 3.0)
        if case == "growing":
            k *= np.linspace(0.1, 3.0, Lk, dtype=np.float32)[None, :, None]
        keep = np.ones((B, Lk), dtype=bool)
        if case == "masked_first_tile":
            keep[:, :64] = False
            k[:, 64:] *= 6.0                                   # ... and what follows sits far from the reference the masked tile left
            q *= 2.0
        bias = np.where(keep, 0.0, -10000.0).astype(np.float32)
        qr, kr, vr = (rnd(t, prec) for t in (q, k, v))
        ref = ref_attention(qr, kr, vr, bias, H, prec)
        a = AttnArgs()
        d_q, d_kv, d_bias = OpBuf(q, prec), OpBuf(np.concatenate([k, v], axis=-1), prec), _dev(bias)
        a.q, a.k, a.v = d_q.ptr, d_kv.ptr, d_kv.ptr + D * 2
        a.ldq, a.ldk, a.ldv = D, 2 * D, 2 * D
        a.B, a.H, a.Lq, a.Lk = B, H, Lq, Lk
        a.bias = d_bias.ptr
        a.scale = 1.0 / np.sqrt(hd)
        outs = []
        d_cnt = _dev(np.zeros(4, dtype=np.float32))
        a.fallbacks = d_cnt.ptr
        for opt in (1, 0):
            d_out = OpBuf(np.full((B, Lq, D), np.nan, dtype=np.float32), prec)
            a.out, a.ldo = d_out.ptr, D
            check(lib.ns2vc_debug_set_attn_optimistic(opt), "set_attn_optimistic")
            try:
                check(lib.ns2vc_k_attention(C.byref(a), hd, prec, None), "k_attention")
                sync()
            finally:
                lib.ns2vc_debug_set_attn_optimistic(1)
            outs.append(d_out.read((B, Lq, D)))
        e_opt, e_exact, same = rel_l2(outs[0], ref), rel_l2(outs[1], ref), np.array_equal(outs[0], outs[1])
        nfb, nwg = int(d_cnt.to_numpy((4,)).view(np.uint32)[0]), ((Lq + 127) // 128) * H * B
        diag(f"attn optimistic pass prec={prec} {case}: default {e_opt:.3e} exact-only {e_exact:.3e} vs fp64; bitwise equal = {same}; "
             f"fallback workgroups {nfb} of {nwg}")
        assert nfb == 0 if case == "ordinary" else (nfb == nwg if prec == 2 else nfb <= nwg)      # the counter counts exactly the repeated workgroups
        # the per-launch switch (what the engine option attn_optimistic sets) selects the exact pass too
        a.exact_only = 1
        d_out = OpBuf(np.full((B, Lq, D), np.nan, dtype=np.float32), prec)
        a.out = d_out.ptr
        check(lib.ns2vc_k_attention(C.byref(a), hd, prec, None), "k_attention"); sync()
        a.exact_only = 0
        assert np.array_equal(d_out.read((B, Lq, D)), outs[1])
        assert np.isfinite(outs[0]).all() and np.isfinite(outs[1]).all()
        tol = 16 * eps16(prec) if case != "ordinary" else 2 * eps16(prec)
        assert e_opt < tol and e_exact < tol
        if case != "ordinary" and prec == 2:
            assert same                                         # fp16: the check rejected the optimistic pass in every workgroup


def test_attention_fallback_rate_and_cost_at_the_bench_shape(diag):
    """VERDICT r3 item 5 / ADVICE: the optimistic attention pass was only ever timed on procedural weights, where no workgroup
    falls back.  Level-0 self-attention of the bench workload (32 x 8 heads x 938 x 938, hd 16, fp16) with (a) ordinary scores,
    (b) a LATE-RISING maximum -- a fraction of the queries meets a key in the last third of the row whose score lies ~25 log2
    units above everything before it -- for 0 %, 1 %, 10 % and 100 % of the queries: the fallback counter gives the share of
    workgroups that ran twice, hipEvent timing what that costs; results must equal the exact pass in every case."""
    import torch
    from ns2vc_amd._lib import AttnArgs, check
    from ns2vc_amd.engine import sync
    lib = _lib()
    prec, B, H, hd, L = 2, 32, 8, 16, 938
    D = H * hd
    rng = np.random.default_rng(7)
    q0 = rng.standard_normal((B, L, D)).astype(np.float32)
    k0 = rng.standard_normal((B, L, D)).astype(np.float32)
    v = rng.standard_normal((B, L, D)).astype(np.float32)
    rows = []
    for frac in (0.0, 0.01, 0.1, 1.0):
        q, k = q0.copy(), k0.copy()
        hot_q = rng.random((B, L)) < frac
        # hot queries point along e_0 of every head with norm 12; one late key per item does too (score 12 * 12 / 4 * log2e ~ 52 above the rest)
        for h_ in range(H):
            q[:, :, h_ * hd][hot_q] = 12.0
            k[:, 700, h_ * hd] = 12.0
        a = AttnArgs()
        d_q, d_kv = OpBuf(q, prec), OpBuf(np.concatenate([k, v], axis=-1), prec)
        d_cnt = _dev(np.zeros(4, dtype=np.float32))
        a.q, a.k, a.v = d_q.ptr, d_kv.ptr, d_kv.ptr + D * 2
        a.ldq, a.ldk, a.ldv = D, 2 * D, 2 * D
        a.B, a.H, a.Lq, a.Lk = B, H, L, L
        a.scale = 1.0 / np.sqrt(hd)
        a.fallbacks = d_cnt.ptr
        res = {}
        for exact in (0, 1):
            d_out = OpBuf(np.zeros((B, L, D), dtype=np.float32), prec)
            a.out, a.ldo, a.exact_only = d_out.ptr, D, exact
            check(lib.ns2vc_k_attention(C.byref(a), hd, prec, None), "k_attention"); sync()      # warm
            d_cnt.upload(np.zeros(4, dtype=np.float32))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st = torch.cuda.current_stream()
            e0.record(st)
            for _ in range(10):
                check(lib.ns2vc_k_attention(C.byref(a), hd, prec, st.cuda_stream), "k_attention")
            e1.record(st); st.synchronize()
            res[exact] = (e0.elapsed_time(e1) * 100.0, d_out.read((B, L, D)), int(d_cnt.to_numpy((4,)).view(np.uint32)[0]) // 10)
        nwg = ((L + 127) // 128) * H * B
        same = np.array_equal(res[0][1], res[1][1]) if frac in (0.0, 1.0) else None
        rows.append((frac, res[0][2], nwg, res[0][0], res[1][0]))
        diag(f"attention hd 16 at the bench shape, {100 * frac:g} % of the queries with a late-rising maximum: {res[0][2]} of {nwg} workgroups fell back; "
             f"{res[0][0]:.1f} us per launch (exact pass only: {res[1][0]:.1f} us)" + ("" if same is None else f"; bitwise equal to the exact pass = {same}"))
        assert np.isfinite(res[0][1]).all() and rel_l2(res[0][1], res[1][1]) < 2 * eps16(prec)
        if frac == 0.0:
            assert res[0][2] == 0
        if frac == 1.0:
            assert res[0][2] == nwg and same
    # a workgroup that falls back pays about twice: the all-fallback launch must not cost more than ~2.3x the exact pass
    assert rows[-1][3] < 2.3 * rows[-1][4] + 5.0


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("shape", [(2, 37, 128, 0), (2, 90, 512, 384), (3, 200, 384, 256), (1, 5, 128, 128), (2, 938, 128, 0),
                                   # (B, T, c0, c1, G) of the non-default configurations (tests/configs.py): 24- and 40-wide groups (192 / 8,
                                   # 320 / 8, the seam at 192 inside a group), 1 / 2 / 4 groups, 80-wide groups across a 192 + 128 seam
                                   (2, 37, 192, 0, 8), (2, 45, 192, 128, 8), (2, 45, 128, 192, 8), (2, 45, 128, 0, 1), (2, 45, 128, 0, 2),
                                   (3, 45, 256, 0, 4), (2, 45, 192, 128, 4), (2, 23, 256, 0, 2)], ids=str)
def test_groupnorm(shape, prec, diag):
    """group_norm (+ the resnet's time scale/shift, + SiLU) over a two-source concat whose groups straddle the seam."""
    from ns2vc_amd._lib import check
    lib = _lib()
    B, T, c0, c1 = shape[:4]
    G = shape[4] if len(shape) > 4 else 8
    C_ = c0 + c1
    rng = np.random.default_rng(B * 1000 + T)
    a0 = (rng.standard_normal((B, T, c0)) * 2 + 0.7).astype(np.float32)
    a1 = (rng.standard_normal((B, T, c1)) - 0.4).astype(np.float32) if c1 else None
    gamma = (1 + 0.1 * rng.standard_normal(C_)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(C_)).astype(np.float32)
    temb = rng.standard_normal((B, 2 * C_ + 64)).astype(np.float32) * 0.2
    off = 64
    A = (a0 if a1 is None else np.concatenate([a0, a1], -1)).astype(np.float64)
    Ag = A.reshape(B, T, G, C_ // G)
    mean = Ag.mean(axis=(1, 3), keepdims=True)
    var = Ag.var(axis=(1, 3), keepdims=True)
    gn = ((Ag - mean) / np.sqrt(var + 1e-5)).reshape(B, T, C_) * gamma + beta
    d_a0, d_a1 = _dev(a0), (_dev(a1) if a1 is not None else None)
    d_g, d_b, d_t = _dev(gamma), _dev(beta), _dev(temb)
    for with_t, silu_on in ((False, 1), (True, 1), (False, 0)):
        ref = gn
        if with_t:
            ref = ref * (1 + temb[:, None, off:off + C_]) + temb[:, None, off + C_:off + 2 * C_]
        if silu_on:
            ref = silu(ref)
        d_o = OpBuf(np.full((B, T, C_), np.nan, np.float32), prec)
        d_r = OpBuf(np.full((B, T, C_), np.nan, np.float32), prec)
        check(lib.ns2vc_k_groupnorm(d_a0.ptr, c0, c0, d_a1.ptr if d_a1 else None, c1, c1, B, T, G, 1e-5, d_g.ptr, d_b.ptr,
                                    d_t.ptr if with_t else None, temb.shape[1], off, silu_on, d_o.ptr, d_r.ptr, prec, None), "groupnorm")
        e1, e2 = rel_l2(d_o.read(), ref), rel_l2(d_r.read(), A)
        diag(f"groupnorm {shape} prec={prec} temb={with_t} silu={silu_on}: out {e1:.2e} raw {e2:.2e}")
        assert e1 < tol_groupnorm(prec)[0] and e2 < tol_groupnorm(prec)[1]


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("shape", [(77, 128), (300, 512), (5, 384), (1000, 256)], ids=str)
def test_layernorm_apply(shape, prec, diag):
    from ns2vc_amd._lib import check
    from ns2vc_amd.engine import sync
    lib = _lib()
    M, C_ = shape
    rng = np.random.default_rng(M)
    x = (rng.standard_normal((M, C_)) * 1.5 + 0.3).astype(np.float32)
    d_x = _dev(x)
    d_o = OpBuf(np.full((M, C_), np.nan, np.float32), prec)
    check(lib.ns2vc_k_layernorm_apply(d_x.ptr, C_, M, C_, 1e-5, d_o.ptr, prec, None), "ln_apply")
    sync()
    xd = x.astype(np.float64)
    ref = (xd - xd.mean(-1, keepdims=True)) / np.sqrt(xd.var(-1, keepdims=True) + 1e-5)
    e = rel_l2(d_o.read(), ref)
    diag(f"layernorm_apply {shape} prec={prec} rel_l2={e:.3e}")
    assert e < tol_layernorm_apply(prec)


def test_layout_roundtrip(diag):
    from ns2vc_amd._lib import check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(3)
    for (B, C_, T, cpad) in [(2, 100, 37, 128), (3, 256, 188, 256), (1, 100, 938, 128)]:
        x = rng.standard_normal((B, C_, T)).astype(np.float32)
        d_x, d_y, d_z = _dev(x), DevBuf(B * T * cpad * 4), DevBuf(B * C_ * T * 4)
        d_y.upload(np.full((B, T, cpad), np.nan, np.float32))
        check(lib.ns2vc_k_nct_to_btc(d_x.ptr, C_, T, B, d_y.ptr, cpad, cpad, None), "nct_to_btc")
        check(lib.ns2vc_k_btc_to_nct(d_y.ptr, cpad, C_, T, B, d_z.ptr, None), "btc_to_nct")
        sync()
        y = d_y.to_numpy((B, T, cpad))
        assert np.array_equal(y[:, :, :C_], x.transpose(0, 2, 1))
        assert np.all(y[:, :, C_:] == 0)
        assert np.array_equal(d_z.to_numpy((B, C_, T)), x)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dim,mult,M,res,nt", [(128, 3, 450, False, 1), (128, 1, 450, True, 1), (256, 3, 194, False, 1), (256, 1, 1000, True, 1),
                                               (128, 3, 64, False, 1), (256, 1, 5, True, 1), (128, 3, 450, False, 2), (128, 1, 333, True, 2),
                                               (128, 1, 70, True, 2), (128, 3, 18000, False, 0), (384, 3, 194, False, 1), (384, 1, 450, True, 1),
                                               (384, 3, 7520, False, 0), (384, 1, 7, True, 0), (384, 3, 450, False, -2), (384, 1, 194, False, -2),
                                               (384, 3, 7520, False, -2), (384, 3, 7, False, -2)], ids=str)
def test_rowchain_fused(dim, mult, M, res, nt, prec, diag):
    """Two token-local GEMMs with a LayerNorm in between in one launch (csrc/rowchain.hip) against numpy fp64 of
        y = A W1^T + b1 (+ res);   z = LayerNorm(y) W2^T + b2
    with the engine's pack-time fold (gamma/beta into W2/b2), the kernel's rounding points modelled (A, the weights and y's
    operand copy are rounded to the operand type; statistics from the fp32 y), rows with a common offset (LayerNorm by
    linearity), row counts that are no multiple of 64, res aliasing out1 (as the engine uses it), NaN-filled outputs, and
    both workgroup sizes (nt = 1: 64 tokens, 2: 128 tokens, 0: the launcher's choice -- 128 once M > 256 x 64 at dim 128); nt = -2 (r4):
    TWO N-slices per token block (dim 384: each workgroup repeats stage 1 and takes 5 + 4 / 2 + 1 of the stage-2 row blocks)."""
    from ns2vc_amd._lib import RowchainArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(dim * 1000 + mult * 10 + M)
    d, n2 = dim, mult * dim
    A = rng.standard_normal((M, d)).astype(np.float32)
    R = (rng.standard_normal((M, d)) + 1.5 * rng.standard_normal((M, 1))).astype(np.float32)
    W1, b1 = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), (0.3 * rng.standard_normal(d)).astype(np.float32)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(d)), 0.2 * rng.standard_normal(d)
    W2, b2 = rng.standard_normal((n2, d)) / np.sqrt(d), 0.3 * rng.standard_normal(n2)
    W2f, b2f = (W2 * gamma[None, :]).astype(np.float32), (b2 + W2 @ beta).astype(np.float32)
    Ar, W1r, W2r = rnd(A, prec).astype(np.float64), rnd(W1, prec).astype(np.float64), rnd(W2f, prec).astype(np.float64)
    consts = np.stack([W2r.sum(1), b2f.astype(np.float64)], axis=1).astype(np.float32)
    # ---- reference with the kernel's rounding points
    y = Ar @ W1r.T + b1.astype(np.float64)[None, :] + (R.astype(np.float64) if res else 0.0)
    y32 = y.astype(np.float32)
    yr = rnd(y32, prec).astype(np.float64)
    mean, var = y.mean(1, keepdims=True), y.var(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    z = rstd * (yr @ W2r.T - mean * consts[:, 0].astype(np.float64)[None, :]) + b2f.astype(np.float64)[None, :]
    # ---- device
    stream = C.c_void_p()
    slices = 2 if nt == -2 else 0
    nt = max(nt, 0)
    if slices:
        check(lib.ns2vc_pack_rowchain_sliced(np.ascontiguousarray(W1).ctypes.data, np.ascontiguousarray(W2f).ctypes.data, d, n2, slices, prec, C.byref(stream)), "pack_rowchain_sliced")
    else:
        check(lib.ns2vc_pack_rowchain(np.ascontiguousarray(W1).ctypes.data, np.ascontiguousarray(W2f).ctypes.data, d, n2, prec, C.byref(stream)), "pack_rowchain")
    d_a, d_b1, d_c = OpBuf(A, prec), _dev(b1), _dev(consts)
    d_y = DevBuf(M * d * 4)
    d_y.upload(R if res else np.full((M, d), np.nan, dtype=np.float32))          # res aliases out1 (in-place residual stream)
    d_z = OpBuf(np.full((M, n2), np.nan, dtype=np.float32), prec)
    d_health = DevBuf.from_numpy(np.zeros(16, dtype=np.uint32))
    f = RowchainArgs()
    f.a_op = d_a.ptr; f.lda = d; f.wstream = stream.value; f.bias1 = d_b1.ptr; f.consts2 = d_c.ptr
    f.res = d_y.ptr if res else None; f.ldres = d
    f.out1_f32 = d_y.ptr; f.ldo1 = d; f.out2_op = d_z.ptr; f.ldo2 = n2
    f.ln_eps = 1e-5; f.M = M; f.dim = d; f.n2 = n2; f.ln_health = d_health.ptr
    f.slices = slices
    check(lib.ns2vc_debug_set_rowchain_tokens(nt), "set_rowchain_tokens")
    try:
        check(lib.ns2vc_k_rowchain(C.byref(f), prec, None), "k_rowchain")
        sync()
    finally:
        lib.ns2vc_debug_set_rowchain_tokens(0)
    if slices:          # an in-place residual (res aliasing out1) is refused: two slices would race on y
        f.res = d_y.ptr
        assert lib.ns2vc_k_rowchain(C.byref(f), prec, None) != 0
    yo, zo = d_y.to_numpy((M, d)), d_z.read()
    e_y, e_z = rel_l2(yo, y), rel_l2(zo, z)
    ratio = float(d_health.to_numpy((16,), dtype=np.uint32)[:1].view(np.float32)[0])
    diag(f"rowchain dim={d} n2={n2} M={M} res={res} nt={nt} prec={prec}: y {e_y:.3e} z {e_z:.3e} nan={int(np.isnan(zo).sum())}  |mean|/std {ratio:.2f}")
    if not (e_y < 1e-6 and e_z < eps16(prec)):
        err = np.abs(zo - z)
        bad = np.argwhere(~(err <= 2e-2 + 2e-2 * np.abs(z)))
        diag(f"  FAIL: {len(bad)} bad of {zo.size}; rows {sorted(set(bad[:, 0].tolist()))[:16]} cols {sorted(set(bad[:, 1].tolist()))[:24]}")
    assert np.isfinite(zo).all() and np.isfinite(yo).all()
    assert e_y < TOL_ROWCHAIN_Y             # fp32 accumulation of exactly rounded operands
    assert e_z < eps16(prec)                # one operand rounding of the result on top of a near-exact value
    want = (np.abs(y.mean(1)) / np.sqrt(y.var(1) + 1e-5)).max()
    assert abs(ratio - want) < 1e-3 * want


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dim,B,T,nt", [(128, 3, 150, 1), (128, 5, 64, 2), (256, 2, 97, 1), (128, 2, 300, 2), (256, 4, 64, 1), (384, 3, 97, 1),
                                        (384, 2, 235, 1), (384, 3, 235, -2)], ids=str)
def test_rowchain_groupnorm_prologue(dim, B, T, nt, prec, diag):
    _rowchain_groupnorm_prologue(dim, B, T, nt, 8, prec, diag)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dim,B,T,nt,G", [(128, 3, 150, 1, 4), (256, 2, 97, 1, 4), (384, 3, 97, 1, 4), (128, 2, 300, 2, 2), (128, 4, 64, 1, 1),
                                          (256, 3, 235, 1, 2)], ids=str)
def test_rowchain_groupnorm_prologue_groups(dim, B, T, nt, G, prec, diag):
    """the same with the group counts of the non-default configurations (tests/configs.py: 4 groups of lpb1_g4, and 1 / 2; groups of at
    most 128 channels, what ns2vc_unet_create admits)"""
    _rowchain_groupnorm_prologue(dim, B, T, nt, G, prec, diag)


def _rowchain_groupnorm_prologue(dim, B, T, nt, Gn, prec, diag):
    """The row-chain kernel with the transformer's GroupNorm in its prologue: A = GroupNorm(x) (8 groups, affine, eps 1e-6) is
    built inside the kernel from the fp32 rows and the int64 per-(item, 16-channel block) statistics a producer's epilogue
    leaves, for token blocks that straddle up to three batch items and both workgroup sizes.  Reference: numpy fp64 with the
    kernel's rounding points; additionally the GroupNorm rows the kernel builds are compared with gn_apply's
    (ns2vc_k_groupnorm), observed through y with W1 = identity."""
    from ns2vc_amd._lib import RowchainArgs, check
    from ns2vc_amd.engine import DevBuf, sync
    lib = _lib()
    rng = np.random.default_rng(dim + 7 * B + T)
    d, M = dim, B * T
    x = (rng.standard_normal((B, T, d)) * (1.0 + rng.random((B, 1, d))) + rng.standard_normal((B, 1, d))).astype(np.float32)
    gam, bet = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32), (0.2 * rng.standard_normal(d)).astype(np.float32)
    blk = x.astype(np.float64).reshape(B, T, d // 16, 16)
    st = np.stack([np.rint(blk.sum(axis=(1, 3)) * 2.0 ** 28), np.rint((blk ** 2).sum(axis=(1, 3)) * 2.0 ** 16)], axis=-1).astype(np.int64)
    xg = x.astype(np.float64).reshape(B, T, Gn, d // Gn)
    mean, var = xg.mean(axis=(1, 3), keepdims=True), xg.var(axis=(1, 3), keepdims=True)
    A = (((xg - mean) / np.sqrt(var + 1e-6)).reshape(B, T, d) * gam.astype(np.float64) + bet.astype(np.float64)).reshape(M, d)
    # gn_apply's own output (operand-typed) for the bit-for-bit comparison
    d_x, d_gam, d_bet = _dev(x.reshape(M, d)), _dev(gam), _dev(bet)
    d_gn = OpBuf(np.zeros((M, d), dtype=np.float32), prec)
    check(lib.ns2vc_k_groupnorm(d_x.ptr, d, d, None, 0, 0, B, T, Gn, 1e-6, d_gam.ptr, d_bet.ptr, None, 0, 0, 0, d_gn.ptr, None, prec, None), "groupnorm")
    sync()
    a_gn = d_gn.read()
    assert rel_l2(a_gn, A) < eps16(prec)
    for mult, W1 in ((3, (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32)), (1, np.eye(d, dtype=np.float32))):
        n2 = mult * d
        b1 = (0.3 * rng.standard_normal(d)).astype(np.float32) if mult == 3 else np.zeros(d, dtype=np.float32)
        W2f, b2f = (rng.standard_normal((n2, d)) / np.sqrt(d)).astype(np.float32), (0.3 * rng.standard_normal(n2)).astype(np.float32)
        W1r, W2r = rnd(W1, prec).astype(np.float64), rnd(W2f, prec).astype(np.float64)
        consts = np.stack([W2r.sum(1), b2f.astype(np.float64)], axis=1).astype(np.float32)
        y = a_gn.astype(np.float64) @ W1r.T + b1.astype(np.float64)[None, :]          # A as the device rounds it (checked above)
        yr = rnd(y.astype(np.float32), prec).astype(np.float64)
        mu, vv = y.mean(1, keepdims=True), y.var(1, keepdims=True)
        z = (yr @ W2r.T - mu * consts[:, 0].astype(np.float64)[None, :]) / np.sqrt(vv + 1e-5) + b2f.astype(np.float64)[None, :]
        stream = C.c_void_p()
        slices = 2 if nt == -2 else 0
        if slices:
            check(lib.ns2vc_pack_rowchain_sliced(np.ascontiguousarray(W1).ctypes.data, np.ascontiguousarray(W2f).ctypes.data, d, n2, slices, prec, C.byref(stream)), "pack_rowchain_sliced")
        else:
            check(lib.ns2vc_pack_rowchain(np.ascontiguousarray(W1).ctypes.data, np.ascontiguousarray(W2f).ctypes.data, d, n2, prec, C.byref(stream)), "pack_rowchain")
        d_b1, d_c, d_st, d_g, d_b = _dev(b1), _dev(consts), DevBuf.from_numpy(st), _dev(gam), _dev(bet)
        d_y = DevBuf(M * d * 4)
        d_y.upload(np.full((M, d), np.nan, dtype=np.float32))
        d_z = OpBuf(np.full((M, n2), np.nan, dtype=np.float32), prec)
        f = RowchainArgs()
        f.a_op = None; f.lda = d; f.wstream = stream.value; f.bias1 = d_b1.ptr; f.consts2 = d_c.ptr
        f.res = None; f.ldres = d; f.out1_f32 = d_y.ptr; f.ldo1 = d; f.out2_op = d_z.ptr; f.ldo2 = n2
        f.ln_eps = 1e-5; f.M = M; f.dim = d; f.n2 = n2; f.ln_health = None
        f.gn_x = d_x.ptr; f.ldx = d; f.gn_stats = d_st.ptr; f.gn_gamma = d_g.ptr; f.gn_beta = d_b.ptr; f.gn_eps = 1e-6; f.T = T; f.G = Gn
        f.slices = slices
        check(lib.ns2vc_debug_set_rowchain_tokens(max(nt, 0)), "set_rowchain_tokens")
        try:
            check(lib.ns2vc_k_rowchain(C.byref(f), prec, None), "k_rowchain")
            sync()
        finally:
            lib.ns2vc_debug_set_rowchain_tokens(0)
        yo, zo = d_y.to_numpy((M, d)), d_z.read()
        e_y, e_z = rel_l2(yo, y), rel_l2(zo, z)
        diag(f"rowchain+GroupNorm dim={d} G={Gn} B={B} T={T} nt={nt} n2={n2} prec={prec}: y {e_y:.3e} z {e_z:.3e}")
        # (ns2vc_k_groupnorm finalises its statistics from a separate fp64 pass, the prologue from the int64 epilogue sums: the two
        # normalised rows agree except where a value sits on a rounding boundary of the operand type -- a ~1e-4 fraction of
        # elements, one operand ulp each; inside the engine both paths read the same int64 sums and are bit-identical,
        # tests/test_engine_gpu.py::test_rows_groupnorm_prologue_is_bit_identical)
        assert np.isfinite(zo).all() and e_y < TOL_ROWCHAIN_GN_Y and e_z < eps16(prec)
        if mult == 1:                                  # W1 = I, b1 = 0: y IS the panel the prologue built
            assert (yo != a_gn).mean() < 2e-3 and np.abs(yo - a_gn).max() <= eps16(prec) * 4 * np.abs(a_gn).max()


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", [c for c in ATTN_CASES if c[0] in ("self_hd16", "self_hd32", "cross_hd48_mask", "cross_hd64_mask", "self_hd16_long", "cross_hd16_129")],
                         ids=lambda c: c[0])
def test_attention_fp8_pv(case, prec, diag):
    """pv_fp8: the PV product on the fp8 MFMA (V and the probabilities rounded to OCP e4m3 inside the kernel; QK^T, softmax state
    and accumulators unchanged).  Against the exact fp64 attention the error is the fp8 rounding of P and V averaged over the
    keys -- a few 1e-2 at most, well above the 16-bit kernel's, which is also asserted (so the test notices if the flag were ignored)."""
    from ns2vc_amd._lib import AttnArgs, check
    from ns2vc_amd.engine import sync
    name, B, H, hd, Lq, Lk, use_bias, packed = case
    lib = _lib()
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 8)
    D = H * hd
    q, k, v = (rng.standard_normal((B, L, D)).astype(np.float32) for L in (Lq, Lk, Lk))
    bias = None
    if use_bias:
        keep = rng.random((B, Lk)) > 0.3
        keep[:, 0] = True
        bias = ((1.0 - keep.astype(np.float32)) * -10000.0).astype(np.float32)
    ref = ref_attention(rnd(q, prec), rnd(k, prec), rnd(v, prec), bias, H, prec)
    errs = {}
    for flag in (0, 1):
        a = AttnArgs()
        d_q, d_k, d_v = OpBuf(q, prec), OpBuf(k, prec), OpBuf(v, prec)
        a.q, a.k, a.v = d_q.ptr, d_k.ptr, d_v.ptr
        a.ldq = a.ldk = a.ldv = D
        a.B, a.H, a.Lq, a.Lk = B, H, Lq, Lk
        d_bias = _dev(bias) if bias is not None else None
        if d_bias is not None:
            a.bias = d_bias.ptr
        a.scale = 1.0 / np.sqrt(hd)
        d_out = OpBuf(np.full((B, Lq, D), np.nan, dtype=np.float32), prec)
        a.out, a.ldo = d_out.ptr, D
        a.pv_fp8 = flag
        check(lib.ns2vc_k_attention(C.byref(a), hd, prec, None), "k_attention")
        sync()
        out = d_out.read()
        assert np.isfinite(out).all()
        errs[flag] = rel_l2(out, ref)
    diag(f"attention {name} prec={prec}: 16-bit PV {errs[0]:.3e}, fp8 PV {errs[1]:.3e}")
    assert errs[1] < TOL_ATTN_FP8 and errs[1] > 2 * errs[0]
    a32 = AttnArgs()
    a32.pv_fp8 = 1
    assert lib.ns2vc_k_attention(C.byref(a32), hd, 0, None) != 0          # no fp8 variant of the exact-fp32 kernel: loud

