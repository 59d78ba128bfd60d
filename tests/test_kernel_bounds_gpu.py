"""Guard-band tests of the kernel entry points of include/ns2vc_hip.h: a call reads and writes only the logical elements of the tensors
it is given.  Every launch here runs three times on identical logical data inside guarded blocks (tests/guard.py: front guard, rows at a
pitch wider than the tensor, back guard) whose guards and gap columns hold the quiet NaN, +Inf and zero of the element type, and

  P1  no guard / gap byte of ANY buffer of the call changed (inputs, bias / constant vectors and statistics included; packed weights and
      tile streams are allocated inside ns2vc_pack_* and are the only exemption);
  P2  the logical outputs of the three runs are finite and bitwise equal (nothing outside a tensor took part in a result);
  P3  the strided launch is right: the numpy fp64 reference and tolerance of the entry point's test in tests/test_kernels_gpu.py.

Shapes are small, every row count leaves a ragged last tile, B >= 2 (so "row -1" / "row T" of an inner item are real neighbours and those
of the first / last item are guard rows).  Nothing here passes a kernel a size that could leave the block the test owns; that the harness
can fail is shown by tests/test_guard_cpu.py and by the positive control at the end (a wrong EXPECTATION, not a wrong launch).
Each case logs entry point / variant / fill before the launch and P1 P2 P3 after it (the `diag` fixture), so a launch that faults or hangs is
named by the last line of the diag file."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest

from guard import FILLS, OP_KIND, DeviceBackend, Guarded, decode, pattern_mismatches
from test_kernels_gpu import TOL, ref_attention, rnd
from util import (GEGLU_FLIPS, NOISE_ULP, TOL_ATTN_FP8, TOL_FFN, TOL_ROWCHAIN_GN_Y, TOL_ROWCHAIN_Y, TOL_SOLVER, TOL_STATS, eps16, gather_rows, gelu_erf, rel_l2,
                  silu, tol_attention, tol_ffn_xattn, tol_gnp_rows, tol_groupnorm, tol_layernorm_apply, tol_ln_linear, tol_pair_rows)

pytestmark = pytest.mark.gpu

PRECS, PREC_IDS = [0, 1, 2], ["fp32", "bf16", "fp16"]
_BE = None


def _be():
    global _BE
    if _BE is None:
        _BE = DeviceBackend()
    return _BE


def _lib():
    return _be().lib


def _check(rc, what):
    _be().check(rc, what)


class Ctx:
    """the guarded buffers of ONE launch under one fill"""

    def __init__(self, fill, skew=0):
        self.fill, self.skew, self.bufs = fill, skew, []

    def t(self, name, rows, width, kind, pad=0, col0=0, data=None):
        g = Guarded(_be(), rows, width, kind, ld=col0 + width + pad, col0=col0, fill=self.fill, data=data, skew=self.skew, name=name)
        self.bufs.append(g)
        return g

    def vec(self, name, data, kind="f32"):
        data = np.asarray(data)
        return self.t(name, 1, data.size, kind, data=data.reshape(1, -1))

    def violations(self):
        return [v for g in self.bufs for v in g.violations()]

    def free(self):
        for g in self.bufs:
            g.free()


def run_bounds(diag, label, body, skew=0, fills=FILLS):
    """body(ctx) launches on ctx's buffers and returns {name: Guarded} of the outputs.  Asserts P1 and P2; returns the decoded outputs (for P3)."""
    runs = {}
    for fill in fills:
        ctx = Ctx(fill, skew)
        diag(f"bounds {label} fill={fill}: launch")
        outs = body(ctx)
        viol = ctx.violations()               # (synchronises the device first)
        diag(f"bounds {label} fill={fill}: P1 {'ok' if not viol else 'FAIL ' + '; '.join(viol[:6])}")
        runs[fill] = {k: (g.read_bits(), g.kind) for k, g in outs.items()}
        ctx.free()
        assert not viol, (label, fill, viol[:8])
    p2 = pattern_mismatches(runs)
    diag(f"bounds {label}: P2 {'ok' if not p2 else 'FAIL ' + '; '.join(p2[:6])}")
    assert not p2, (label, p2[:8])
    return {k: decode(b, kind) for k, (b, kind) in runs[fills[0]].items()}


def _pack(W, prec):
    W = np.ascontiguousarray(W, dtype=np.float32)
    p = C.c_void_p()
    _check(_lib().ns2vc_pack_weight(W.ctypes.data, W.shape[0], W.shape[1], prec, C.byref(p)), "pack_weight")
    return p


def _pack_tiled(W, ctot, c2, prec):
    W = np.ascontiguousarray(W, dtype=np.float32)
    p = C.c_void_p()
    _check(_lib().ns2vc_pack_conv3_tiled(W.ctypes.data, W.shape[0], ctot, c2, prec, C.byref(p)), "pack_conv3_tiled")
    return p


def _launch_gemm(g, prec, tile):
    lib = _lib()
    _check(lib.ns2vc_debug_set_gemm_tile(*tile), "set tile")
    try:
        _check(lib.ns2vc_k_gemm(C.byref(g), prec, None), "k_gemm")
    finally:
        lib.ns2vc_debug_set_gemm_tile(0, 0, 0)


def _gn_stats(x, B, T, Cc):
    """the int64 fixed-point statistics a producer's epilogue leaves: [B][C/16][2] = (sum * 2^28, sum of squares * 2^16)"""
    blk = x.astype(np.float64).reshape(B, T, Cc // 16, 16)
    return np.stack([np.rint(blk.sum(axis=(1, 3)) * 2.0 ** 28), np.rint((blk ** 2).sum(axis=(1, 3)) * 2.0 ** 16)], axis=-1).astype(np.int64)


def _gn_ref(x, B, T, Cc, G, gam, bet, temb=None, act=False):
    xg = x.astype(np.float64).reshape(B, T, G, Cc // G)
    y = ((xg - xg.mean(axis=(1, 3), keepdims=True)) / np.sqrt(xg.var(axis=(1, 3), keepdims=True) + 1e-5)).reshape(B, T, Cc) * gam + bet
    if temb is not None:
        y = y * (1.0 + temb[0][:, None, :]) + temb[1][:, None, :]
    return silu(y) if act else y


# ---------------------------------------------------------------------------------------------------------------------------------------
# ns2vc_k_gemm
# ---------------------------------------------------------------------------------------------------------------------------------------
TS_STAGES = (54, 58, 64, 68)
GEMM_TILES = [(0, 0, 0), (64, 128, 2), (64, 64, 3), (128, 128, 13), (64, 128, 23), (128, 128, 23), (128, 64, 54), (128, 128, 58), (128, 64, 68)]
GEMM_FEATURES = [
    # name, B, Tin, Tout, c0, c1, c2, N, taps, tmode, bias, res, geglu, dual, stats
    ("linear_res_dual", 3, 41, 41, 128, 0, 0, 128, 1, 0, 1, 1, 0, 1, 0),
    ("linear_n192_res", 3, 41, 41, 256, 0, 0, 192, 1, 0, 1, 1, 0, 1, 0),
    ("linear_concat_stats", 2, 67, 67, 192, 128, 0, 256, 1, 0, 1, 0, 0, 0, 1),
    ("conv3_concat_seg_res_dual", 2, 37, 37, 128, 64, 64, 128, 3, 0, 1, 1, 0, 1, 0),
    ("conv3_long_concat_seg_res_dual_stats", 3, 70, 70, 128, 64, 64, 128, 3, 0, 1, 1, 0, 1, 1),
    ("conv3_long_n256", 2, 131, 131, 64, 0, 0, 256, 3, 0, 0, 1, 0, 0, 0),
    ("down2_odd", 2, 37, 19, 128, 0, 0, 128, 3, 1, 1, 0, 0, 0, 0),
    ("down2_even", 2, 38, 19, 128, 0, 0, 128, 3, 1, 1, 0, 0, 0, 0),
    ("up2_odd", 2, 19, 37, 128, 0, 0, 128, 3, 2, 1, 0, 0, 0, 0),
    ("up2_even", 2, 19, 38, 128, 0, 0, 128, 3, 2, 1, 0, 0, 0, 0),
    ("geglu_dual", 2, 50, 50, 128, 0, 0, 256, 1, 0, 1, 0, 1, 1, 0),
    ("temb_m_small", 3, 1, 1, 512, 0, 0, 640, 1, 0, 1, 0, 0, 0, 0),       # M = 3: the whole tile but three rows is outside
]


def _gemm_applies(feat, tile):
    _, B, Tin, Tout, c0, c1, c2, N, taps, tmode, bias, res, geglu, dual, stats = feat
    if tile == (0, 0, 0):
        return True
    if N % tile[1] or (geglu and tile[1] != 128):
        return False
    if tile[2] in TS_STAGES:          # the tap-sharing kernel: k = 3, stride 1, T >= 66
        return taps == 3 and tmode == 0 and Tin >= 66 and not geglu
    return True


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", GEMM_TILES, ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_bounds(tile, prec, diag):
    """Every GEMM family (heuristic, 4-wave, K-split, loader / consumer, tap-sharing) on every feature it takes: linear, k = 3 same / stride 2 /
    nearest-up (odd and even T), the concat a0 | a1 at different pitches with a0 a column slice of a wider row, the fused 1x1 segment a2, bias,
    GEGLU, out_f32 + out_op at different pitches, epilogue statistics, tile-major weights, M = 3 -- and the residual BOTH as a separate tensor and
    aliasing out_f32 element for element (the engine's transformer-block residual GEMMs): the two give the same bits."""
    from ns2vc_amd._lib import GemmArgs
    lib = _lib()
    kind = OP_KIND[prec]
    ran, ran_names = 0, []
    for feat in GEMM_FEATURES:
        if not _gemm_applies(feat, tile):
            continue
        name, B, Tin, Tout, c0, c1, c2, N, taps, tmode, bias_on, res_on, geglu, dual, stats_on = feat
        ran_names.append(name)
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        Ct, M = c0 + c1, B * Tout
        K = taps * Ct + c2
        a0 = rnd(rng.standard_normal((B, Tin, c0)), prec)
        a1 = rnd(rng.standard_normal((B, Tin, c1)), prec) if c1 else None
        a2 = rnd(rng.standard_normal((B, Tin, c2)), prec) if c2 else None
        W = rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec)
        bias = rng.standard_normal(N).astype(np.float32) if bias_on else None
        Nout = N // 2 if geglu else N
        res = rng.standard_normal((M, Nout)).astype(np.float32) if res_on else None
        A = (a0 if a1 is None else np.concatenate([a0, a1], axis=-1)).astype(np.float64)
        ref = gather_rows(A, B, Tin, Tout, taps, tmode).reshape(M, taps * Ct) @ W[:, :taps * Ct].astype(np.float64).T
        if c2:
            ref = ref + a2.reshape(M, c2).astype(np.float64) @ W[:, taps * Ct:].astype(np.float64).T
        if bias is not None:
            ref = ref + bias
        if geglu:
            r3 = ref.reshape(M, N // 64, 2, 32)
            ref = (r3[:, :, 0, :] * gelu_erf(r3[:, :, 1, :])).reshape(M, N // 2)
        if res is not None:
            ref = ref + res
        d_w = _pack(W, prec)
        ts_kernel = taps == 3 and tmode == 0 and Tin >= 66 and not geglu and (tile == (0, 0, 0) or tile[2] in TS_STAGES)
        d_wt = _pack_tiled(W, Ct, c2, prec) if ts_kernel else None
        variants = ["sep"] + (["alias"] if res_on else []) + (["tiled"] if d_wt is not None else [])
        got = {}
        for variant in variants:
            def body(ctx):
                g = GemmArgs()
                d_a0 = ctx.t("a0", B * Tin, c0, kind, pad=8, col0=16, data=a0)      # a column slice of a wider row
                g.a0, g.lda0, g.c0 = d_a0.ptr, d_a0.ld, c0
                if c1:
                    d_a1 = ctx.t("a1", B * Tin, c1, kind, pad=40, data=a1)
                    g.a1, g.lda1, g.c1 = d_a1.ptr, d_a1.ld, c1
                if c2:
                    d_a2 = ctx.t("a2", B * Tin, c2, kind, pad=72, col0=8, data=a2)
                    g.a2, g.lda2, g.c2 = d_a2.ptr, d_a2.ld, c2
                g.B, g.Tin, g.Tout, g.M = B, Tin, Tout, M
                g.taps, g.tmode = taps, tmode
                g.w, g.K, g.N = d_w.value, K, N
                if variant == "tiled":
                    g.w_tiled = d_wt.value
                if bias is not None:
                    g.bias = ctx.vec("bias", bias).ptr
                g.geglu = int(geglu)
                # alias: the fp32 output starts as the residual and is its own `res`
                d_o = ctx.t("out_f32", M, Nout, "f32", pad=24, col0=4, data=res if variant == "alias" else None)
                g.out_f32, g.ldo_f32 = d_o.ptr, d_o.ld
                if res is not None:
                    if variant == "alias":
                        g.res, g.ldres = d_o.ptr, d_o.ld
                    else:
                        d_r = ctx.t("res", M, Nout, "f32", pad=12, data=res)
                        g.res, g.ldres = d_r.ptr, d_r.ld
                outs = {"out_f32": d_o}
                if dual:
                    d_op = ctx.t("out_op", M, Nout, kind, pad=56, col0=8)
                    g.out_op, g.ldo_op = d_op.ptr, d_op.ld
                    outs["out_op"] = d_op
                if stats_on:
                    d_s = ctx.t("stats", B, N // 16 * 2, "i64", data=np.zeros((B, N // 16 * 2), np.int64))
                    g.stats = d_s.ptr
                    outs["stats"] = d_s
                _launch_gemm(g, prec, tile)
                return outs
            label = f"ns2vc_k_gemm / {name} {variant} tile={tile} prec={prec}"
            got[variant] = o = run_bounds(diag, label, body, skew=int(variant == "sep" and tile == (0, 0, 0)))
            e = rel_l2(o["out_f32"], ref)
            ok = e < TOL[prec] and ("out_op" not in o or np.array_equal(o["out_op"], rnd(o["out_f32"], prec)))
            if stats_on:
                st = o["stats"].reshape(B, N // 16, 2).astype(np.float64)
                blk = o["out_f32"].astype(np.float64).reshape(B, Tout, N // 16, 16)
                rs, rq = blk.sum(axis=(1, 3)), (blk ** 2).sum(axis=(1, 3))
                e_s, e_q = np.abs(st[..., 0] / 2 ** 28 - rs).max() / np.abs(rs).max(), np.abs(st[..., 1] / 2 ** 16 - rq).max() / np.abs(rq).max()
                ok = ok and e_s < TOL_STATS and e_q < TOL_STATS
            diag(f"bounds {label}: P3 rel_l2 {e:.3e} {'ok' if ok else 'FAIL'}")
            assert ok, (label, e)
            ran += 1
        for v in variants[1:]:      # the aliased residual / the tile-major weights: the same products in the same order
            assert all(got["sep"][k].tobytes() == got[v][k].tobytes() for k in got["sep"]), (name, v)
        lib.ns2vc_dev_free(d_w)
        if d_wt is not None:
            lib.ns2vc_dev_free(d_wt)
    # what each family must have run (a filter change cannot quietly empty one): every family runs the residual both ways
    want = [f[0] for f in GEMM_FEATURES if _gemm_applies(f, tile)]
    assert ran_names == want and want, (tile, ran_names)
    assert set(want) >= EXPECTED_GEMM_FEATURES[tile], (tile, want)
    assert any(f[11] for f in GEMM_FEATURES if f[0] in want), "the aliased residual runs on every family"


# the least each forced family must cover; spelled out, not derived from _gemm_applies
_TS_SET = {"conv3_long_concat_seg_res_dual_stats", "conv3_long_n256"}
_ALL128 = {"linear_res_dual", "linear_concat_stats", "conv3_concat_seg_res_dual", "conv3_long_concat_seg_res_dual_stats", "conv3_long_n256",
           "down2_odd", "down2_even", "up2_odd", "up2_even", "geglu_dual", "temb_m_small"}
EXPECTED_GEMM_FEATURES = {(0, 0, 0): _ALL128 | {"linear_n192_res"}, (64, 128, 2): _ALL128, (64, 64, 3): (_ALL128 - {"geglu_dual"}) | {"linear_n192_res"},
                          (128, 128, 13): _ALL128, (64, 128, 23): _ALL128, (128, 128, 23): _ALL128,
                          (128, 64, 54): _TS_SET, (128, 128, 58): _TS_SET, (128, 64, 68): _TS_SET}


GNP_TILES = [(0, 0, 0), (128, 128, 13), (64, 128, 23), (128, 64, 54), (128, 128, 58)]


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", GNP_TILES, ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_groupnorm_prologue_bounds(tile, prec, diag):
    """ns2vc_gemm_args.gnp_*: the materialising prologue (algo = 2) in its redundant and cooperative (gnp_sync) form and the in-loop form
    (algo = 0), k = 3 and k = 1, gnp_temb inside a wider per-item row.  a0 (written by the prologue), the arrival words and gnp_alone are
    outputs: their logical region may change, their surroundings may not.  T = 70: row tiles straddle the three items."""
    from ns2vc_amd._lib import GemmArgs
    lib = _lib()
    kind = OP_KIND[prec]
    B, T, Cc, N, Gn = 3, 70, 128, 256, 8
    M = B * T
    ran = 0
    for taps in (3, 1):
        if tile[2] in TS_STAGES and (taps != 3 or N % tile[1]):
            continue
        K = taps * Cc
        rng = np.random.default_rng(700 + taps)
        x = (rng.standard_normal((B, T, Cc)) * (1.0 + rng.random((B, 1, Cc))) + rng.standard_normal((B, 1, Cc))).astype(np.float32)
        gam, bet = (1.0 + 0.2 * rng.standard_normal(Cc)).astype(np.float32), (0.2 * rng.standard_normal(Cc)).astype(np.float32)
        temb = (0.3 * rng.standard_normal((B, 2 * Cc))).astype(np.float32)
        st = _gn_stats(x, B, T, Cc)
        W = rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec)
        bias = rng.standard_normal(N).astype(np.float32)
        d_w = _pack(W, prec)
        y = _gn_ref(x, B, T, Cc, Gn, gam.astype(np.float64), bet.astype(np.float64), (temb[:, :Cc].astype(np.float64), temb[:, Cc:].astype(np.float64)), True)
        rows = {}
        for form in ("redundant", "coop", "inloop"):
            if form == "inloop" and not (taps == 3 and (tile == (0, 0, 0) or tile[2] in TS_STAGES)):
                continue

            def body(ctx):
                g = GemmArgs()
                # cooperative form: a0 on a 128-byte line, whole lines per row (64 extra elements: 128 / 256 bytes)
                d_a = ctx.t("a0", M, Cc, kind, pad=64)
                g.a0, g.lda0, g.c0 = d_a.ptr, d_a.ld, Cc
                g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, M, taps, 0
                g.w, g.K, g.N = d_w.value, K, N
                g.bias = ctx.vec("bias", bias).ptr
                d_o = ctx.t("out_f32", M, N, "f32", pad=8)
                g.out_f32, g.ldo_f32 = d_o.ptr, d_o.ld
                d_x = ctx.t("gnp_x", M, Cc, "f32", pad=20, col0=4, data=x)
                g.gnp_x, g.gnp_ldx = d_x.ptr, d_x.ld
                g.gnp_stats = ctx.t("gnp_stats", B, Cc // 16 * 2, "i64", data=st.reshape(B, -1)).ptr
                g.gnp_gamma, g.gnp_beta = ctx.vec("gnp_gamma", gam).ptr, ctx.vec("gnp_beta", bet).ptr
                d_t = ctx.t("gnp_temb", B, 2 * Cc, "f32", pad=16, col0=8, data=temb)     # (scale | shift) inside a wider per-item row
                g.gnp_temb, g.gnp_ldtemb = d_t.ptr, d_t.ld
                g.gnp_eps, g.gnp_G, g.gnp_silu = 1e-5, Gn, 1
                g.algo = 0 if form == "inloop" else 2
                outs = {"out_f32": d_o}
                d_al = ctx.t("gnp_alone", 1, 4, "u32", data=np.zeros((1, 4), np.uint32))
                g.gnp_alone = d_al.ptr
                if form == "coop":
                    d_sy = ctx.t("gnp_sync", 1, (M + 63) // 64, "u64", data=np.zeros((1, (M + 63) // 64), np.uint64))
                    g.gnp_sync = d_sy.ptr
                if form != "inloop":
                    outs["a0"] = d_a
                _launch_gemm(g, prec, tile)
                return outs
            label = f"ns2vc_k_gemm / groupnorm prologue {form} taps={taps} tile={tile} prec={prec}"
            o = run_bounds(diag, label, body)
            if "a0" in o:
                rows[form] = o["a0"]
            a_rows = rows.get(form, rows.get("redundant"))
            e_op = rel_l2(a_rows, y.reshape(M, Cc))
            Gr = gather_rows(a_rows.astype(np.float64).reshape(B, T, Cc), B, T, T, taps, 0).reshape(M, K)
            e_out = rel_l2(o["out_f32"], Gr @ W.astype(np.float64).T + bias)
            # in-loop: the rows never leave the kernel; same values, another summation order over K than the rows' product in fp64 -> TOL all the same
            diag(f"bounds {label}: P3 rows {e_op:.2e} result {e_out:.2e}")
            assert e_op < tol_gnp_rows(prec)[0] and e_out < TOL[prec], (label, e_op, e_out)
            ran += 1
        if "coop" in rows:
            assert np.array_equal(rows["coop"], rows["redundant"])
        lib.ns2vc_dev_free(d_w)
    assert ran > 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# ns2vc_k_attention
# ---------------------------------------------------------------------------------------------------------------------------------------
ATTN_BOUNDS = [
    # name, B, H, hd, Lq, Lk, bias, layout ("qkv" = packed q|k|v rows, "kv" = the hoisted k|v view with columns around it)
    ("self_hd16_65", 2, 8, 16, 65, 65, False, "qkv"),
    ("self_hd32_129", 2, 8, 32, 129, 129, False, "qkv"),
    ("self_hd48_1", 2, 8, 48, 1, 1, False, "qkv"),
    ("self_hd64_65", 2, 4, 64, 65, 65, False, "qkv"),
    ("cross_hd16_469", 2, 8, 16, 70, 469, True, "kv"),
    ("cross_hd32_1key", 2, 8, 32, 65, 1, False, "kv"),
    ("cross_hd32_129_mask", 2, 8, 32, 1, 129, True, "kv"),
    ("cross_hd48_65_mask", 2, 8, 48, 129, 65, True, "kv"),
    ("cross_hd64_469", 2, 8, 64, 33, 469, True, "kv"),
]


@pytest.mark.parametrize("prec,mode", [(p, m) for p in PRECS for m in ("keys64", "keys128", "exact_only", "pv_fp8") if not (p == 0 and m == "pv_fp8")],
                         ids=lambda v: PREC_IDS[v] if isinstance(v, int) else v)     # (fp32 x pv_fp8: a row of EXPECTED_REFUSALS)
def test_attention_bounds(prec, mode, diag):
    """hd 16 / 32 / 48 / 64; Lq, Lk of one row, of a tile + 1 (65, 129) and of 469; bias on / off; packed q|k|v views and the hoisted k|v view;
    64- and 128-key tiles; the exact pass alone; the fp8 PV product.  Rows past Lk are fetched from somewhere: what lies there must not matter."""
    from ns2vc_amd._lib import AttnArgs
    lib = _lib()
    kind = OP_KIND[prec]
    for name, B, H, hd, Lq, Lk, use_bias, layout in ATTN_BOUNDS:
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        D = H * hd
        q, k, v = (rng.standard_normal((B, L, D)).astype(np.float32) for L in (Lq, Lk, Lk))
        bias = None
        if use_bias:
            keep = rng.random((B, Lk)) > 0.3
            keep[:, 0] = True
            keep[0, Lk // 2:] = False
            bias = np.where(keep, 0.0, -10000.0).astype(np.float32)
        ref = ref_attention(rnd(q, prec), rnd(k, prec), rnd(v, prec), bias, H, prec)

        def body(ctx):
            a = AttnArgs()
            esz = 4 if prec == 0 else 2
            if layout == "qkv":
                d = ctx.t("qkv", B * Lq, 3 * D, kind, pad=24, col0=8, data=np.concatenate([q, k, v], axis=-1))
                a.q, a.k, a.v = d.ptr, d.ptr + D * esz, d.ptr + 2 * D * esz
                a.ldq = a.ldk = a.ldv = d.ld
            else:
                d_q = ctx.t("q", B * Lq, D, kind, pad=16, data=q)
                d_kv = ctx.t("kv", B * Lk, 2 * D, kind, pad=40, col0=64, data=np.concatenate([k, v], axis=-1))
                a.q, a.k, a.v = d_q.ptr, d_kv.ptr, d_kv.ptr + D * esz
                a.ldq, a.ldk, a.ldv = d_q.ld, d_kv.ld, d_kv.ld
            a.B, a.H, a.Lq, a.Lk = B, H, Lq, Lk
            if bias is not None:
                a.bias = ctx.t("bias", 1, B * Lk, "f32", data=bias.reshape(1, -1)).ptr     # [B][Lk] contiguous: no pitch to widen
            a.scale = 1.0 / np.sqrt(hd)
            d_o = ctx.t("out", B * Lq, D, kind, pad=72, col0=8)
            a.out, a.ldo = d_o.ptr, d_o.ld
            a.exact_only = int(mode == "exact_only")
            a.pv_fp8 = int(mode == "pv_fp8")
            d_f = ctx.t("fallbacks", 1, 4, "u32", data=np.zeros((1, 4), np.uint32))
            a.fallbacks = d_f.ptr
            _check(lib.ns2vc_debug_set_attn_keys(128 if mode == "keys128" else 0), "set_attn_keys")
            try:
                _check(lib.ns2vc_k_attention(C.byref(a), hd, prec, None), "k_attention")
            finally:
                lib.ns2vc_debug_set_attn_keys(0)
            return {"out": d_o}
        label = f"ns2vc_k_attention / {name} {mode} prec={prec}"
        o = run_bounds(diag, label, body, skew=int(mode == "keys64"))
        e = rel_l2(o["out"], ref.reshape(B * Lq, D))
        tol = TOL_ATTN_FP8 if mode == "pv_fp8" else tol_attention(prec)
        diag(f"bounds {label}: P3 rel_l2 {e:.3e} (bound {tol:.1e})")
        assert e < tol, (label, e)


# ---------------------------------------------------------------------------------------------------------------------------------------
# normalisation, layout, noise and solver kernels
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("entry", ["groupnorm", "groupnorm_stats", "groupnorm_stats2"])
def test_groupnorm_bounds(entry, prec, diag):
    """ns2vc_k_groupnorm / _stats / _stats2: two sources at different pitches whose groups straddle the seam (192 + 128 channels in 4 groups of
    80), the time scale / shift inside a wider per-item row, SiLU, the raw operand copy.  The outputs have no pitch of their own (rows of
    c0 + c1): their guards still see a row past the end."""
    lib = _lib()
    kind = OP_KIND[prec]
    B, T = 3, 45
    c0, c1, G = (256, 0, 8) if entry == "groupnorm_stats" else (192, 128, 4)
    Cc, off = c0 + c1, 8
    rng = np.random.default_rng(c0 + len(entry))
    a0 = (rng.standard_normal((B, T, c0)) * 2 + 0.7).astype(np.float32)
    a1 = (rng.standard_normal((B, T, c1)) - 0.4).astype(np.float32) if c1 else None
    gam, bet = (1 + 0.1 * rng.standard_normal(Cc)).astype(np.float32), (0.1 * rng.standard_normal(Cc)).astype(np.float32)
    temb = (0.2 * rng.standard_normal((B, 2 * Cc))).astype(np.float32)
    A = a0 if a1 is None else np.concatenate([a0, a1], -1)
    ref = _gn_ref(A, B, T, Cc, G, gam.astype(np.float64), bet.astype(np.float64), (temb[:, :Cc].astype(np.float64), temb[:, Cc:].astype(np.float64)), True)

    def body(ctx):
        d_a0 = ctx.t("a0", B * T, c0, "f32", pad=12, col0=4, data=a0)
        d_a1 = ctx.t("a1", B * T, c1, "f32", pad=36, data=a1) if c1 else None
        d_g, d_b = ctx.vec("gamma", gam), ctx.vec("beta", bet)
        d_t = ctx.t("temb", B, 2 * Cc + off, "f32", pad=24, data=np.concatenate([np.zeros((B, off), np.float32), temb], axis=1))
        d_o = ctx.t("out_op", B * T, Cc, kind)
        outs = {"out_op": d_o}
        if entry == "groupnorm":
            d_r = ctx.t("raw_op", B * T, Cc, kind)
            outs["raw_op"] = d_r
            _check(lib.ns2vc_k_groupnorm(d_a0.ptr, d_a0.ld, c0, d_a1.ptr, d_a1.ld, c1, B, T, G, 1e-5, d_g.ptr, d_b.ptr, d_t.ptr, d_t.ld, off, 1,
                                         d_o.ptr, d_r.ptr, prec, None), entry)
        elif entry == "groupnorm_stats":
            d_s = ctx.t("stats0", B, c0 // 16 * 2, "i64", data=_gn_stats(a0, B, T, c0).reshape(B, -1))
            _check(lib.ns2vc_k_groupnorm_stats(d_a0.ptr, d_a0.ld, c0, d_s.ptr, B, T, G, 1e-5, d_g.ptr, d_b.ptr, d_t.ptr, d_t.ld, off, 1, d_o.ptr, prec, None), entry)
        else:
            d_s0 = ctx.t("stats0", B, c0 // 16 * 2, "i64", data=_gn_stats(a0, B, T, c0).reshape(B, -1))
            d_s1 = ctx.t("stats1", B, c1 // 16 * 2, "i64", data=_gn_stats(a1, B, T, c1).reshape(B, -1))
            d_r = ctx.t("raw_op", B * T, Cc, kind)
            outs["raw_op"] = d_r
            _check(lib.ns2vc_k_groupnorm_stats2(d_a0.ptr, d_a0.ld, c0, d_s0.ptr, d_a1.ptr, d_a1.ld, c1, d_s1.ptr, B, T, G, 1e-5, d_g.ptr, d_b.ptr,
                                                d_t.ptr, d_t.ld, off, 1, d_o.ptr, d_r.ptr, prec, None), entry)
        return outs
    label = f"ns2vc_k_{entry} / B={B} T={T} c={c0}+{c1} G={G} prec={prec}"
    o = run_bounds(diag, label, body, skew=1)
    e1 = rel_l2(o["out_op"], ref.reshape(B * T, Cc))
    e2 = rel_l2(o["raw_op"], A.reshape(B * T, Cc)) if "raw_op" in o else 0.0
    diag(f"bounds {label}: P3 out {e1:.2e} raw {e2:.2e}")
    assert e1 < tol_groupnorm(prec)[0] and e2 < tol_groupnorm(prec)[1]


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
def test_layernorm_apply_bounds(prec, diag):
    lib = _lib()
    for (M, Cc) in ((77, 128), (5, 384), (301, 512)):
        x = (np.random.default_rng(M).standard_normal((M, Cc)) * 1.5 + 0.3).astype(np.float32)

        def body(ctx):
            d_x = ctx.t("x", M, Cc, "f32", pad=28, col0=12, data=x)
            d_o = ctx.t("out_op", M, Cc, OP_KIND[prec])
            _check(lib.ns2vc_k_layernorm_apply(d_x.ptr, d_x.ld, M, Cc, 1e-5, d_o.ptr, prec, None), "ln_apply")
            return {"out_op": d_o}
        label = f"ns2vc_k_layernorm_apply / M={M} C={Cc} prec={prec}"
        o = run_bounds(diag, label, body)
        xd = x.astype(np.float64)
        e = rel_l2(o["out_op"], (xd - xd.mean(-1, keepdims=True)) / np.sqrt(xd.var(-1, keepdims=True) + 1e-5))
        diag(f"bounds {label}: P3 rel_l2 {e:.3e}")
        assert e < tol_layernorm_apply(prec)


def test_layout_bounds(diag):
    """ns2vc_k_nct_to_btc with cpad > C (the pad columns are written: zeros; the columns after them are not) and ns2vc_k_btc_to_nct from rows
    at a wider pitch; T = 37 / 188 leave ragged 32 x 32 tiles in both directions."""
    lib = _lib()
    for (B, Cc, T, cpad) in ((2, 100, 37, 128), (3, 98, 188, 104)):
        x = np.random.default_rng(T).standard_normal((B, Cc, T)).astype(np.float32)

        def fwd(ctx):
            d_x = ctx.t("src_nct", 1, B * Cc * T, "f32", data=x.reshape(1, -1))
            d_y = ctx.t("dst_btc", B * T, cpad, "f32", pad=24, col0=4)
            _check(lib.ns2vc_k_nct_to_btc(d_x.ptr, Cc, T, B, d_y.ptr, d_y.ld, cpad, None), "nct_to_btc")
            return {"dst": d_y}
        label = f"ns2vc_k_nct_to_btc / B={B} C={Cc} T={T} cpad={cpad}"
        y = run_bounds(diag, label, fwd)["dst"].reshape(B, T, cpad)
        ok = np.array_equal(y[:, :, :Cc], x.transpose(0, 2, 1)) and np.all(y[:, :, Cc:] == 0)
        diag(f"bounds {label}: P3 {'ok' if ok else 'FAIL'}")
        assert ok                                                           # test_layout_roundtrip: exact

        def back(ctx):
            d_y = ctx.t("src_btc", B * T, Cc, "f32", pad=28 + -Cc % 4, col0=8, data=x.transpose(0, 2, 1))
            d_z = ctx.t("dst_nct", 1, B * Cc * T, "f32")
            _check(lib.ns2vc_k_btc_to_nct(d_y.ptr, d_y.ld, Cc, T, B, d_z.ptr, None), "btc_to_nct")
            return {"dst": d_z}
        label = f"ns2vc_k_btc_to_nct / B={B} C={Cc} T={T}"
        z = run_bounds(diag, label, back, skew=1)["dst"].reshape(B, Cc, T)
        diag(f"bounds {label}: P3 {'ok' if np.array_equal(z, x) else 'FAIL'}")
        assert np.array_equal(z, x)


@pytest.mark.parametrize("Cc", [1, 98, 127])
@pytest.mark.parametrize("with_lens", [False, True], ids=["dense", "lens"])
def test_noise_bounds(with_lens, Cc, diag):
    """ns2vc_k_noise writes whole rows of ld columns (z for c < C and t < L_b, zeros elsewhere): the rows have no gap, the tensor has an end."""
    from ns2vc_amd import noise as Nz
    lib = _lib()
    B, T, ld, step = 3, 53, 128, 5
    seeds = np.array([0x0123456789ABCDEF, 1, 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)
    lens = [53, 30, 1] if with_lens else None

    def body(ctx):
        d_s = ctx.t("seeds", 1, B + 1, "u64", data=np.concatenate([seeds, np.zeros(1, np.uint64)]).reshape(1, -1))     # (an even count keeps 16-byte alignment)
        d_l = ctx.t("lens", 1, 4, "i32", data=np.array([lens + [0]], np.int32)) if lens else None
        d_o = ctx.t("out", B * T, ld, "f32")
        _check(lib.ns2vc_k_noise(d_s.ptr, B, Cc, T, ld, step, d_l.ptr if d_l else None, d_o.ptr, None), "k_noise")
        return {"out": d_o}
    label = f"ns2vc_k_noise / C={Cc} lens={lens}"
    dev = run_bounds(diag, label, body)["out"].reshape(B, T, ld)
    host = Nz.gauss(seeds, step, Cc, T, lens if lens else [T] * B).transpose(0, 2, 1)
    ulp = np.abs(dev[:, :, :Cc].astype(np.float64) - host) / np.spacing(np.maximum(np.abs(host), 1.0).astype(np.float32))
    zeros = not dev[:, :, Cc:].any() and all(not dev[b, L:].any() for b, L in enumerate(lens or []))
    diag(f"bounds {label}: P3 max {ulp.max():.1f} ulp, zeros {zeros}")
    assert ulp.max() <= NOISE_ULP and zeros


@pytest.mark.parametrize("prec", [0, 2], ids=["fp32", "fp16"])
@pytest.mark.parametrize("hist2", [True, False])
def test_solver_update_bounds(hist2, prec, diag):
    """ns2vc_k_solver_update, both history forms, the fp32 copy and the 16-bit hi + lo pair output.  The state tensors are contiguous rows of ld."""
    from ns2vc_amd import schedule as S
    from test_solvers_gpu import _update_numpy
    from util import f16_round
    lib = _lib()
    rows, ld, step = 37, 104, 4
    n = rows * ld
    table = S.build_table("unipc", 10, order=3, skip_type="logSNR")
    rng = np.random.default_rng(3)
    names = ("x0", "xe", "xbar", "d1", "mprev", "mprev2")
    st = {k: rng.standard_normal((rows, ld)).astype(np.float32) for k in names}

    def body(ctx):
        b = {k: ctx.t(k, rows, ld, "f32", data=st[k]) for k in names}
        coef = ctx.t("coef", table.coef.shape[0], table.coef.shape[1], "f32", data=np.ascontiguousarray(table.coef, np.float32))
        stepb = ctx.t("step", 1, 4, "i32", data=np.array([[step, 0, 0, 0]], np.int32))
        op = ctx.t("xe_op", rows, ld if prec == 0 else 2 * ld, OP_KIND[prec])
        _check(lib.ns2vc_k_solver_update(coef.ptr, stepb.ptr, b["x0"].ptr, b["xe"].ptr, op.ptr, prec, b["xbar"].ptr, b["d1"].ptr, b["mprev"].ptr,
                                         b["mprev2"].ptr if hist2 else None, n, ld, None), "k_solver_update")
        return {**{k: b[k] for k in names}, "xe_op": op}
    label = f"ns2vc_k_solver_update / hist2={hist2} prec={prec}"
    got = run_bounds(diag, label, body, skew=1)
    f64 = {k: v.astype(np.float64) for k, v in st.items()}
    ne, nb, nd, m = _update_numpy(table.coef[step], f64["x0"], f64["xe"], f64["xbar"], f64["d1"], f64["mprev"], f64["mprev2"] if hist2 else None)
    errs = {"xe": rel_l2(got["xe"], ne), "xbar": rel_l2(got["xbar"], nb), "d1": rel_l2(got["d1"], nd), "mprev": rel_l2(got["mprev"], m)}
    diag(f"bounds {label}: P3 " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert all(v < TOL_SOLVER for v in errs.values()), errs
    assert np.array_equal(got["x0"], st["x0"]) and np.array_equal(got["mprev2"], st["mprev"] if hist2 else st["mprev2"])
    if prec == 0:
        assert np.array_equal(got["xe_op"], got["xe"])
    else:
        hi = f16_round(got["xe"])
        assert np.array_equal(got["xe_op"][:, :ld], hi) and np.array_equal(got["xe_op"][:, ld:], f16_round(got["xe"] - hi))


# ---------------------------------------------------------------------------------------------------------------------------------------
# ns2vc_k_geglu
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("M", [97, 3 * 67])
def test_geglu_bounds(M, prec, diag):
    """The token-stationary GEGLU projection (dim 384): 128-token workgroups with a ragged last block, rows past M "arrive as zeros" and "the
    hardware drops" their stores -- here with NaN / Inf behind the last row of yn and ln_stats and an output pitch wider than 4 dim."""
    from scipy.special import erf
    from ns2vc_amd._lib import GegluArgs
    lib = _lib()
    d = 384
    rng = np.random.default_rng(M * 7 + prec)
    y = (rng.standard_normal((M, d)) + 1.5 * rng.standard_normal((M, 1))).astype(np.float32)
    W1, b1 = rng.standard_normal((8 * d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(8 * d)
    order = np.concatenate([np.concatenate([np.arange(32 * g, 32 * g + 32), 4 * d + np.arange(32 * g, 32 * g + 32)]) for g in range(4 * d // 32)])
    W1p, b1p = np.ascontiguousarray(W1[order].astype(np.float32)), np.ascontiguousarray(b1[order].astype(np.float32))
    W1r, yr, y64 = rnd(W1p, prec).astype(np.float64), rnd(y, prec).astype(np.float64), y.astype(np.float64)
    rstd = 1.0 / np.sqrt(y64.var(1, keepdims=True) + 1e-5)
    pre = rstd * (yr @ W1r.T - y64.mean(1, keepdims=True) * W1r.sum(1).astype(np.float32).astype(np.float64)[None, :]) + b1p.astype(np.float64)[None, :]
    pg = pre.reshape(M, 4 * d // 32, 2, 32)
    ref = (pg[:, :, 0] * 0.5 * pg[:, :, 1] * (1.0 + erf(pg[:, :, 1] / np.sqrt(2.0)))).reshape(M, 4 * d)
    ys = y64.reshape(M, d // 64, 64)
    stats = np.stack([ys.sum(2), (ys ** 2).sum(2)], axis=-1).astype(np.float32).reshape(M, -1)
    stream, consts = C.c_void_p(), C.c_void_p()
    _check(lib.ns2vc_pack_geglu(W1p.ctypes.data, b1p.ctypes.data, d, prec, C.byref(stream), C.byref(consts)), "pack_geglu")

    def body(ctx):
        f = GegluArgs()
        d_y = ctx.t("yn", M, d, OP_KIND[prec], pad=24, col0=8, data=y)
        d_st = ctx.t("ln_stats", M, d // 64 * 2, "f32", data=stats)
        d_h = ctx.t("out_op", M, 4 * d, OP_KIND[prec], pad=40, col0=16)
        d_he = ctx.t("ln_health", 1, 4, "u32", data=np.zeros((1, 4), np.uint32))
        f.yn, f.ldy, f.ln_stats, f.ln_eps = d_y.ptr, d_y.ld, d_st.ptr, 1e-5
        f.wstream, f.consts = stream.value, consts.value
        f.out_op, f.ldo, f.M, f.dim, f.ln_health = d_h.ptr, d_h.ld, M, d, d_he.ptr
        _check(lib.ns2vc_k_geglu(C.byref(f), prec, None), "k_geglu")
        return {"out_op": d_h}
    label = f"ns2vc_k_geglu / M={M} prec={prec}"
    out = run_bounds(diag, label, body)["out_op"]
    lib.ns2vc_dev_free(stream); lib.ns2vc_dev_free(consts)
    e, flips = rel_l2(out, ref), float(np.mean(out != rnd(ref.astype(np.float32), prec)))
    diag(f"bounds {label}: P3 rel_l2 {e:.3e} flips {flips:.4f}")
    assert e < eps16(prec) and flips < GEGLU_FLIPS


# ---------------------------------------------------------------------------------------------------------------------------------------
# ns2vc_k_rowchain
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dim,mult,M,res,nt", [(128, 3, 201, False, 1), (128, 1, 201, True, 1), (128, 3, 201, True, 2), (256, 1, 97, True, 1),
                                               (384, 3, 97, False, 0), (384, 1, 201, False, -2), (384, 3, 7, False, -2)], ids=str)
def test_rowchain_bounds(dim, mult, M, res, nt, prec, diag):
    """y = A W1^T + b1 (+ res), z = LayerNorm(y) W2'^T + b2' in one launch: 64- and 128-token workgroups (nt 1 / 2), the in-place residual (res
    aliases out1_f32 element for element, as the engine runs it), two N-slices (nt = -2, dim 384).  Rows past M "arrive as zeros" and "the
    hardware drops" their stores: here the rows behind A, res and the outputs hold NaN / Inf."""
    from ns2vc_amd._lib import RowchainArgs
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
    y = Ar @ W1r.T + b1.astype(np.float64)[None, :] + (R.astype(np.float64) if res else 0.0)
    yr = rnd(y.astype(np.float32), prec).astype(np.float64)
    rstd = 1.0 / np.sqrt(y.var(1, keepdims=True) + 1e-5)
    z = rstd * (yr @ W2r.T - y.mean(1, keepdims=True) * consts[:, 0].astype(np.float64)[None, :]) + b2f.astype(np.float64)[None, :]
    stream = C.c_void_p()
    slices = 2 if nt == -2 else 0
    if slices:
        _check(lib.ns2vc_pack_rowchain_sliced(np.ascontiguousarray(W1).ctypes.data, np.ascontiguousarray(W2f).ctypes.data, d, n2, slices, prec, C.byref(stream)), "pack_rowchain_sliced")
    else:
        _check(lib.ns2vc_pack_rowchain(np.ascontiguousarray(W1).ctypes.data, np.ascontiguousarray(W2f).ctypes.data, d, n2, prec, C.byref(stream)), "pack_rowchain")

    def body(ctx):
        f = RowchainArgs()
        d_a = ctx.t("a_op", M, d, OP_KIND[prec], pad=24, col0=8, data=A)
        d_y = ctx.t("out1_f32", M, d, "f32", pad=20, col0=4, data=R if res else None)
        d_z = ctx.t("out2_op", M, n2, OP_KIND[prec], pad=72, col0=16)
        f.a_op, f.lda, f.wstream = d_a.ptr, d_a.ld, stream.value
        f.bias1, f.consts2 = ctx.vec("bias1", b1).ptr, ctx.vec("consts2", consts).ptr
        if res:
            f.res, f.ldres = d_y.ptr, d_y.ld
        f.out1_f32, f.ldo1, f.out2_op, f.ldo2 = d_y.ptr, d_y.ld, d_z.ptr, d_z.ld
        f.ln_eps, f.M, f.dim, f.n2, f.slices = 1e-5, M, d, n2, slices
        f.ln_health = ctx.t("ln_health", 1, 4, "u32", data=np.zeros((1, 4), np.uint32)).ptr
        _check(lib.ns2vc_debug_set_rowchain_tokens(max(nt, 0)), "set_rowchain_tokens")
        try:
            _check(lib.ns2vc_k_rowchain(C.byref(f), prec, None), "k_rowchain")
        finally:
            lib.ns2vc_debug_set_rowchain_tokens(0)
        return {"out1_f32": d_y, "out2_op": d_z}
    label = f"ns2vc_k_rowchain / dim={d} n2={n2} M={M} res={'in place' if res else 'none'} nt={nt} prec={prec}"
    o = run_bounds(diag, label, body, skew=int(nt == 1))
    lib.ns2vc_dev_free(stream)
    e_y, e_z = rel_l2(o["out1_f32"], y), rel_l2(o["out2_op"], z)
    diag(f"bounds {label}: P3 y {e_y:.3e} z {e_z:.3e}")
    assert e_y < TOL_ROWCHAIN_Y and e_z < eps16(prec)


# ---------------------------------------------------------------------------------------------------------------------------------------
# ns2vc_k_gemm: LayerNorm by linearity, the two-source prologue, hi + lo pairs, the solver epilogue
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(0, 0, 0), (64, 128, 2), (128, 128, 13), (64, 128, 23)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_layernorm_by_linearity_bounds(tile, prec, diag):
    """rowstats producer (fp32 + operand copy + per-slice row sums, every slot written once) and ln_stats consumer (plain and GEGLU) on the rows
    the producer left, M = 249: a row tail in every tile."""
    from ns2vc_amd._lib import GemmArgs
    lib = _lib()
    kind = OP_KIND[prec]
    rng = np.random.default_rng(11)
    B, T, D = 3, 83, 256
    M = B * T
    a = rnd(rng.standard_normal((M, D)), prec)
    W1 = rnd(rng.standard_normal((D, D)) / np.sqrt(D), prec)
    b1 = rng.standard_normal(D).astype(np.float32)
    res = (rng.standard_normal((M, D)) + 3.0 * rng.standard_normal((M, 1))).astype(np.float32)
    d_w1 = _pack(W1, prec)

    def producer(ctx):
        g = GemmArgs()
        d_a = ctx.t("a0", M, D, kind, pad=24, col0=8, data=a)
        g.a0, g.lda0, g.c0 = d_a.ptr, d_a.ld, D
        g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, M, 1, 0
        g.w, g.K, g.N, g.bias = d_w1.value, D, D, ctx.vec("bias", b1).ptr
        d_r = ctx.t("res", M, D, "f32", pad=12, data=res)
        g.res, g.ldres = d_r.ptr, d_r.ld
        d_y, d_yop = ctx.t("out_f32", M, D, "f32", pad=20, col0=4), ctx.t("out_op", M, D, kind, pad=40)
        g.out_f32, g.ldo_f32, g.out_op, g.ldo_op = d_y.ptr, d_y.ld, d_yop.ptr, d_yop.ld
        d_rs = ctx.t("rowstats", M, D // 64 * 2, "f32")
        g.rowstats = d_rs.ptr
        _launch_gemm(g, prec, tile)
        return {"out_f32": d_y, "out_op": d_yop, "rowstats": d_rs}
    label = f"ns2vc_k_gemm / rowstats producer tile={tile} prec={prec}"
    po = run_bounds(diag, label, producer)
    lib.ns2vc_dev_free(d_w1)
    y = po["out_f32"].astype(np.float64)
    st, ys = po["rowstats"].reshape(M, D // 64, 2).astype(np.float64), y.reshape(M, D // 64, 64)
    e = rel_l2(y, a.astype(np.float64) @ W1.astype(np.float64).T + b1 + res)
    e_s, e_q = np.abs(st[..., 0] - ys.sum(2)).max() / np.abs(ys.sum(2)).max(), np.abs(st[..., 1] - (ys ** 2).sum(2)).max() / (ys ** 2).sum(2).max()
    diag(f"bounds {label}: P3 rel_l2 {e:.3e} slice sums {e_s:.2e} sumsq {e_q:.2e}")
    assert e < TOL[prec] and np.array_equal(po["out_op"], rnd(po["out_f32"], prec)) and e_s < TOL_STATS and e_q < TOL_STATS
    yn = (y - y.mean(1, keepdims=True)) / np.sqrt(y.var(1, keepdims=True) + 1e-5)
    for geglu, N in ((0, 384), (1, 512)):
        W2 = np.ascontiguousarray(rnd(rng.standard_normal((N, D)) / np.sqrt(D), prec), dtype=np.float32)
        b2 = rng.standard_normal(N).astype(np.float32)
        d_w2, ws = _pack(W2, prec), C.c_void_p()
        _check(lib.ns2vc_weight_rowsum(W2.ctypes.data, N, D, prec, C.byref(ws)), "rowsum")
        wsum = np.empty(N, np.float32)                    # (allocated inside the library: copied into a guarded vector)
        _check(lib.ns2vc_memcpy_d2h(wsum.ctypes.data, ws, N * 4), "d2h")
        lib.ns2vc_dev_free(ws)
        Nout = N // 2 if geglu else N

        def consumer(ctx):
            g = GemmArgs()
            d_a = ctx.t("a0", M, D, kind, pad=56, col0=16, data=po["out_op"])
            g.a0, g.lda0, g.c0 = d_a.ptr, d_a.ld, D
            g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, M, 1, 0
            g.w, g.K, g.N, g.bias, g.geglu = d_w2.value, D, N, ctx.vec("bias", b2).ptr, geglu
            d_o = ctx.t("out_f32", M, Nout, "f32", pad=8)
            g.out_f32, g.ldo_f32 = d_o.ptr, d_o.ld
            g.ln_stats = ctx.t("ln_stats", M, D // 64 * 2, "f32", data=po["rowstats"]).ptr
            g.ln_wsum, g.ln_eps, g.ln_dim = ctx.vec("ln_wsum", wsum).ptr, 1e-5, D
            g.ln_health = ctx.t("ln_health", 1, 4, "u32", data=np.zeros((1, 4), np.uint32)).ptr
            _launch_gemm(g, prec, tile)
            return {"out_f32": d_o}
        label = f"ns2vc_k_gemm / ln_stats consumer geglu={geglu} tile={tile} prec={prec}"
        out = run_bounds(diag, label, consumer, skew=1)["out_f32"]
        lib.ns2vc_dev_free(d_w2)
        pre = yn @ W2.astype(np.float64).T + b2
        if geglu:
            pg = pre.reshape(M, N // 64, 2, 32)
            pre = (pg[:, :, 0] * gelu_erf(pg[:, :, 1])).reshape(M, Nout)
        e = rel_l2(out, pre)
        diag(f"bounds {label}: P3 rel_l2 {e:.3e}")
        assert e < tol_ln_linear(prec)


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(0, 0, 0), (64, 128, 23), (128, 64, 54), (128, 128, 58)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_groupnorm_prologue_of_a_concat_bounds(tile, prec, diag):
    """gnp_x1 / gnp_stats1 / gnp_raw: the prologue on the concat of two fp32 tensors at different pitches (256 + 128 channels in 4 groups of 96:
    the seam inside a group), writing the normalised rows into a0 and the raw operand copy into gnp_raw; redundant and cooperative."""
    from ns2vc_amd._lib import GemmArgs
    lib = _lib()
    kind = OP_KIND[prec]
    B, T, c0, c1, N, taps, Gn = 3, 70, 256, 128, 256, 3, 4
    Cc, M, K = c0 + c1, B * T, taps * (c0 + c1)
    rng = np.random.default_rng(77)
    x0 = (rng.standard_normal((B, T, c0)) * (1.0 + rng.random((B, 1, c0))) + rng.standard_normal((B, 1, c0))).astype(np.float32)
    x1 = (rng.standard_normal((B, T, c1)) * 0.5 + rng.standard_normal((B, 1, c1))).astype(np.float32)
    gam, bet = (1.0 + 0.2 * rng.standard_normal(Cc)).astype(np.float32), (0.2 * rng.standard_normal(Cc)).astype(np.float32)
    W = rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec)
    d_w = _pack(W, prec)
    x = np.concatenate([x0, x1], axis=-1)
    y = _gn_ref(x, B, T, Cc, Gn, gam.astype(np.float64), bet.astype(np.float64), None, True)
    got = {}
    for form in ("redundant", "coop"):
        def body(ctx):
            g = GemmArgs()
            d_a, d_raw = ctx.t("a0", M, Cc, kind, pad=64), ctx.t("gnp_raw", M, Cc, kind, pad=64)       # (gnp_raw: same layout as a0)
            g.a0, g.lda0, g.c0 = d_a.ptr, d_a.ld, Cc
            g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, M, taps, 0
            g.w, g.K, g.N = d_w.value, K, N
            d_o = ctx.t("out_f32", M, N, "f32", pad=8)
            g.out_f32, g.ldo_f32, g.algo = d_o.ptr, d_o.ld, 2
            d_x0, d_x1 = ctx.t("gnp_x", M, c0, "f32", pad=8, data=x0), ctx.t("gnp_x1", M, c1, "f32", pad=28, col0=4, data=x1)
            g.gnp_x, g.gnp_ldx, g.gnp_x1, g.gnp_ldx1, g.gnp_c1 = d_x0.ptr, d_x0.ld, d_x1.ptr, d_x1.ld, c1
            g.gnp_stats = ctx.t("gnp_stats", B, c0 // 16 * 2, "i64", data=_gn_stats(x0, B, T, c0).reshape(B, -1)).ptr
            g.gnp_stats1 = ctx.t("gnp_stats1", B, c1 // 16 * 2, "i64", data=_gn_stats(x1, B, T, c1).reshape(B, -1)).ptr
            g.gnp_gamma, g.gnp_beta = ctx.vec("gnp_gamma", gam).ptr, ctx.vec("gnp_beta", bet).ptr
            g.gnp_eps, g.gnp_G, g.gnp_silu, g.gnp_raw = 1e-5, Gn, 1, d_raw.ptr
            if form == "coop":
                g.gnp_sync = ctx.t("gnp_sync", 1, (M + 63) // 64, "u64", data=np.zeros((1, (M + 63) // 64), np.uint64)).ptr
            _launch_gemm(g, prec, tile)
            return {"a0": d_a, "gnp_raw": d_raw, "out_f32": d_o}
        label = f"ns2vc_k_gemm / two-source prologue {form} tile={tile} prec={prec}"
        got[form] = o = run_bounds(diag, label, body)
        e_op, e_raw = rel_l2(o["a0"], y.reshape(M, Cc)), rel_l2(o["gnp_raw"], x.reshape(M, Cc))
        Gr = gather_rows(o["a0"].astype(np.float64).reshape(B, T, Cc), B, T, T, taps, 0).reshape(M, K)
        e_out = rel_l2(o["out_f32"], Gr @ W.astype(np.float64).T)
        diag(f"bounds {label}: P3 rows {e_op:.2e} raw {e_raw:.2e} result {e_out:.2e}")
        assert e_op < tol_gnp_rows(prec)[0] and e_raw < tol_gnp_rows(prec)[1] and e_out < TOL[prec]
    assert all(got["coop"][k].tobytes() == got["redundant"][k].tobytes() for k in got["coop"])
    lib.ns2vc_dev_free(d_w)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("tile", [(0, 0, 0), (128, 64, 58), (128, 128, 58)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_hi_lo_pair_bounds(tile, prec, diag):
    """gnp_pair: the prologue writes [hi | lo] planes into a0 (c0 = 2 C) and the launch reads the hi plane once more through a1 = a0."""
    from ns2vc_amd._lib import GemmArgs
    lib = _lib()
    kind = OP_KIND[prec]
    B, T, Cc, N, Gn, taps = 3, 97, 128, 256, 8, 3
    M = B * T
    rng = np.random.default_rng(B * 100 + T + Cc)
    x = (rng.standard_normal((B, T, Cc)) * (1.0 + rng.random((B, 1, Cc))) + rng.standard_normal((B, 1, Cc))).astype(np.float32)
    gam, bet = (1.0 + 0.2 * rng.standard_normal(Cc)).astype(np.float32), (0.2 * rng.standard_normal(Cc)).astype(np.float32)
    temb = (0.3 * rng.standard_normal((B, 2 * Cc))).astype(np.float32)
    W = (rng.standard_normal((N, taps, Cc)) / np.sqrt(taps * Cc)).astype(np.float32)
    Wp = np.concatenate([W, W, W - rnd(W, prec)], axis=2).reshape(N, taps * 3 * Cc)
    bias = rng.standard_normal(N).astype(np.float32)
    d_w, d_wp = _pack(W.reshape(N, taps * Cc), prec), _pack(Wp, prec)
    y = _gn_ref(x, B, T, Cc, Gn, gam.astype(np.float64), bet.astype(np.float64), (temb[:, :Cc].astype(np.float64), temb[:, Cc:].astype(np.float64)), True)
    ref = gather_rows(y, B, T, T, taps, 0).reshape(M, taps * Cc) @ W.reshape(N, taps * Cc).astype(np.float64).T + bias
    got = {}
    for pair in (0, 1):
        wd = 2 * Cc if pair else Cc

        def body(ctx):
            g = GemmArgs()
            d_a = ctx.t("a0", M, wd, kind, pad=24, col0=8)
            g.a0, g.lda0, g.c0 = d_a.ptr, d_a.ld, wd
            if pair:
                g.a1, g.lda1, g.c1, g.gnp_pair = d_a.ptr, d_a.ld, Cc, 1
            g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, M, taps, 0
            g.w, g.K, g.N, g.bias = (d_wp if pair else d_w).value, taps * (3 if pair else 1) * Cc, N, ctx.vec("bias", bias).ptr
            d_o = ctx.t("out_f32", M, N, "f32", pad=16)
            g.out_f32, g.ldo_f32, g.algo = d_o.ptr, d_o.ld, 2
            d_x = ctx.t("gnp_x", M, Cc, "f32", pad=12, data=x)
            g.gnp_x, g.gnp_ldx = d_x.ptr, d_x.ld
            g.gnp_stats = ctx.t("gnp_stats", B, Cc // 16 * 2, "i64", data=_gn_stats(x, B, T, Cc).reshape(B, -1)).ptr
            g.gnp_gamma, g.gnp_beta = ctx.vec("gnp_gamma", gam).ptr, ctx.vec("gnp_beta", bet).ptr
            d_t = ctx.t("gnp_temb", B, 2 * Cc, "f32", pad=8, col0=4, data=temb)
            g.gnp_temb, g.gnp_ldtemb, g.gnp_eps, g.gnp_G, g.gnp_silu = d_t.ptr, d_t.ld, 1e-5, Gn, 1
            _launch_gemm(g, prec, tile)
            return {"a0": d_a, "out_f32": d_o}
        label = f"ns2vc_k_gemm / gnp_pair={pair} tile={tile} prec={prec}"
        got[pair] = run_bounds(diag, label, body, skew=pair)
    lib.ns2vc_dev_free(d_w); lib.ns2vc_dev_free(d_wp)
    hi, lo = got[1]["a0"][:, :Cc], got[1]["a0"][:, Cc:]
    e_pair = rel_l2(hi.astype(np.float64) + lo.astype(np.float64), y.reshape(M, Cc))
    e0, e1 = rel_l2(got[0]["out_f32"], ref), rel_l2(got[1]["out_f32"], ref)
    diag(f"bounds ns2vc_k_gemm / gnp_pair tile={tile} prec={prec}: P3 hi + lo {e_pair:.2e} plain {e0:.2e} pair {e1:.2e}")
    assert np.array_equal(hi, got[0]["a0"]) and e_pair < tol_pair_rows(prec) and e1 < 0.02 * e0        # test_conv_on_hi_lo_operand_pairs


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("tile", [(0, 0, 0), (128, 128, 54), (128, 128, 58)], ids=lambda t: f"{t[0]}x{t[1]}s{t[2]}")
def test_gemm_solver_epilogue_bounds(tile, prec, diag):
    """sol_*: the solver update in the epilogue of a one-column-tile k = 3 conv (N = 128), with sol_op_pair for the 16-bit precisions.  x0 is the
    conv's own fp32 result of the same launch; the state tensors are rows of sol_ld and are outputs: logical region only."""
    from ns2vc_amd import schedule as S
    from ns2vc_amd._lib import GemmArgs
    from test_solvers_gpu import _update_numpy
    lib = _lib()
    kind = OP_KIND[prec]
    B, T, Cc, N, ld, step = 3, 70, 128, 128, 128, 3
    M = B * T
    table = S.build_table("unipc", 10)
    row = table.coef[step]
    assert row[9] == 0 and row[10] == 0 and row[11] == 0          # an order <= 2, noise-free row: what the epilogue serves
    rng = np.random.default_rng(5)
    a0 = rnd(rng.standard_normal((B, T, Cc)), prec)
    W = rnd(rng.standard_normal((N, 3 * Cc)) / np.sqrt(3 * Cc), prec)
    bias = rng.standard_normal(N).astype(np.float32)
    names = ("sol_xe", "sol_xbar", "sol_d1", "sol_mprev")
    st = {k: rng.standard_normal((M, ld)).astype(np.float32) for k in names}
    d_w = _pack(W, prec)

    def body(ctx):
        g = GemmArgs()
        d_a = ctx.t("a0", M, Cc, kind, pad=8, col0=16, data=a0)
        g.a0, g.lda0, g.c0 = d_a.ptr, d_a.ld, Cc
        g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, M, 3, 0
        g.w, g.K, g.N, g.bias, g.conv_bn = d_w.value, 3 * Cc, N, ctx.vec("bias", bias).ptr, 128
        d_o = ctx.t("out_f32", M, N, "f32", pad=24)
        g.out_f32, g.ldo_f32 = d_o.ptr, d_o.ld
        b = {k: ctx.t(k, M, ld, "f32", data=st[k]) for k in names}
        g.sol_coef = ctx.t("sol_coef", table.coef.shape[0], 12, "f32", data=np.ascontiguousarray(table.coef, np.float32)).ptr
        g.sol_step, g.sol_ncoef = ctx.t("sol_step", 1, 4, "i32", data=np.array([[step, 0, 0, 0]], np.int32)).ptr, 12
        d_op = ctx.t("sol_xe_op", M, ld if prec == 0 else 2 * ld, kind)
        g.sol_xe, g.sol_xbar, g.sol_d1, g.sol_mprev, g.sol_xe_op = b["sol_xe"].ptr, b["sol_xbar"].ptr, b["sol_d1"].ptr, b["sol_mprev"].ptr, d_op.ptr
        g.sol_ld, g.sol_op_pair = ld, int(prec != 0)
        _launch_gemm(g, prec, tile)
        return {**b, "sol_xe_op": d_op, "out_f32": d_o}
    label = f"ns2vc_k_gemm / solver epilogue tile={tile} prec={prec}"
    o = run_bounds(diag, label, body)
    lib.ns2vc_dev_free(d_w)
    e = rel_l2(o["out_f32"], gather_rows(a0.astype(np.float64), B, T, T, 3, 0).reshape(M, 3 * Cc) @ W.astype(np.float64).T + bias)
    f64 = {k: v.astype(np.float64) for k, v in st.items()}
    ne, nb, nd, m = _update_numpy(row, o["out_f32"].astype(np.float64), f64["sol_xe"], f64["sol_xbar"], f64["sol_d1"], f64["sol_mprev"], None)
    errs = {"xe": rel_l2(o["sol_xe"], ne), "xbar": rel_l2(o["sol_xbar"], nb), "d1": rel_l2(o["sol_d1"], nd), "mprev": rel_l2(o["sol_mprev"], m)}
    diag(f"bounds {label}: P3 conv {e:.2e} " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert e < TOL[prec] and all(v < TOL_SOLVER for v in errs.values()), errs
    if prec == 0:
        assert np.array_equal(o["sol_xe_op"], o["sol_xe"])
    else:
        hi = rnd(o["sol_xe"], prec)
        assert np.array_equal(o["sol_xe_op"][:, :ld], hi) and np.array_equal(o["sol_xe_op"][:, ld:], rnd(o["sol_xe"] - hi, prec))


# ---------------------------------------------------------------------------------------------------------------------------------------
# ns2vc_k_xattn_pack, ns2vc_k_ffn
# ---------------------------------------------------------------------------------------------------------------------------------------
def _xattn_image(k, v, hd, prec):
    """the fragment image as include/ns2vc_hip.h states it, as VALUES [B * 8][tiles][hd / 16 + 2][64 lanes][8]; k, v: (B, Lk, 8 hd) operand-rounded"""
    B, Lk, _ = k.shape
    nt, nsl = (Lk + 31) // 32, hd // 16
    kp = np.zeros((B, nt * 32, 8, hd), np.float32); kp[:, :Lk] = k.reshape(B, Lk, 8, hd)
    vp = np.zeros((B, nt * 32, 8, hd), np.float32); vp[:, :Lk] = v.reshape(B, Lk, 8, hd)
    img = np.zeros((B, 8, nt, nsl + 2, 64, 8), np.float32)
    k5, v5 = kp.reshape(B, nt, 32, 8, hd), vp.reshape(B, nt, 32, 8, hd)          # [b][tile][key in tile][head][channel]
    for lane in range(64):
        l31, hi = lane & 31, lane >> 5
        for e in range(8):
            for s_ in range(nsl):         # K fragment s: lane (key, half) = k[key][16 s + 8 half .. + 7]
                img[:, :, :, s_, lane, e] = k5[:, :, l31, :, 16 * s_ + 8 * hi + e].transpose(0, 2, 1)
            for j in range(2):            # V^T fragment j: lane (d, half) = v[key(slot)][d], slots 16 j + 8 half .. + 7, key bits 2 and 3 swapped
                slot = 16 * j + 8 * hi + e
                key = (slot & ~12) | ((slot & 4) << 1) | ((slot & 8) >> 1)
                if l31 < hd:
                    img[:, :, :, nsl + j, lane, e] = v5[:, :, key, :, l31].transpose(0, 2, 1)
                elif l31 == 16 and hd == 16:
                    img[:, :, :, nsl + j, lane, e] = 1.0      # the ones row: the softmax denominator rides the P V product
    return img.reshape(B * 8, nt, nsl + 2, 64, 8)


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("hd", [16, 32])
@pytest.mark.parametrize("Lk", [1, 33, 130])
def test_xattn_pack_bounds(Lk, hd, prec, diag):
    """The image is fully determined by the Lk keys: keys beyond Lk are zero whatever follows k / v (NaN / Inf behind the last row of the k | v
    view), bit for bit the layout the header states."""
    lib = _lib()
    kind = OP_KIND[prec]
    B, D = 2, 8 * hd
    rng = np.random.default_rng(Lk + hd)
    kv = rnd(rng.standard_normal((B, Lk, 2 * D)), prec)
    nel = int(lib.ns2vc_xattn_pack_bytes(B, Lk, hd)) // 2
    ref = _xattn_image(kv[..., :D], kv[..., D:], hd, prec)
    assert ref.size == nel

    def body(ctx):
        d_kv = ctx.t("kv", B * Lk, 2 * D, kind, pad=40, col0=64, data=kv)
        d_o = ctx.t("image", 1, nel, kind)
        _check(lib.ns2vc_k_xattn_pack(d_kv.ptr, d_kv.ld, d_kv.ptr + D * 2, d_kv.ld, B, Lk, hd, d_o.ptr, prec, None), "xattn_pack")
        return {"image": d_o}
    label = f"ns2vc_k_xattn_pack / Lk={Lk} hd={hd} prec={prec}"
    img = run_bounds(diag, label, body)["image"]
    same = np.array_equal(img.reshape(-1), ref.reshape(-1))
    diag(f"bounds {label}: P3 image == header layout {same}")
    assert same


FFN_CASES = [("plain", 128, 3, 70, 0, False), ("plain", 256, 2, 97, 0, False), ("pre", 128, 3, 70, 0, False), ("pre", 256, 2, 97, 0, False),
             ("att", 128, 3, 70, 1, False), ("att", 256, 2, 97, 33, True), ("att", 128, 2, 97, 130, True)]


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", FFN_CASES, ids=lambda c: f"{c[0]}-d{c[1]}-B{c[2]}-T{c[3]}-Lk{c[4]}")
def test_ffn_bounds(case, prec, diag):
    """ns2vc_k_ffn: plain (yn + ln_stats), the pre-stage (attn2.to_out + residual inside the kernel) and the in-kernel cross-attention with att_Lk
    1 / 33 / 130; 64-token blocks with a ragged last one, blocks that straddle batch items (plain / pre) or are cut per item (att)."""
    from scipy.special import erf
    from ns2vc_amd._lib import FfnArgs
    lib = _lib()
    kind = OP_KIND[prec]
    form, d, B, T, Lk, masked = case
    M, H = B * T, 8
    hd = d // H
    rng = np.random.default_rng(d * 1000 + B * 10 + T + Lk)
    y = (rng.standard_normal((M, d)) + 1.5 * rng.standard_normal((M, 1))).astype(np.float32)
    x = rng.standard_normal((M, d)).astype(np.float32)
    Wo, bo = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), (0.3 * rng.standard_normal(d)).astype(np.float32)
    y_prev, o_in, bias = y, None, None
    if form == "att":
        q = rnd(rng.standard_normal((B, T, d)), prec)
        kv = rnd(rng.standard_normal((B, Lk, 2 * d)), prec)
        if masked:
            lens = np.maximum(1, (Lk * (0.4 + 0.6 * rng.random(B))).astype(int)); lens[0] = Lk
            bias = ((np.arange(Lk)[None, :] >= lens[:, None]) * -10000.0).astype(np.float32)
        qh = q.reshape(B, T, H, hd).transpose(0, 2, 1, 3).astype(np.float64)
        kh = kv[..., :d].reshape(B, Lk, H, hd).transpose(0, 2, 1, 3).astype(np.float64)
        vh = kv[..., d:].reshape(B, Lk, H, hd).transpose(0, 2, 1, 3).astype(np.float64)
        sc = qh @ kh.transpose(0, 1, 3, 2) / np.sqrt(hd)
        if bias is not None:
            sc = sc + bias[:, None, None, :]
        pr_ = rnd(np.exp(sc - sc.max(-1, keepdims=True)).astype(np.float32), prec).astype(np.float64)
        o_in = ((pr_ @ vh) / pr_.sum(-1, keepdims=True)).transpose(0, 2, 1, 3).reshape(M, d).astype(np.float32)
        image = _xattn_image(kv[..., :d], kv[..., d:], hd, prec)          # (what ns2vc_k_xattn_pack writes: test_xattn_pack_bounds)
    elif form == "pre":
        o_in = rng.standard_normal((M, d)).astype(np.float32)
    if form != "plain":
        y = (rnd(o_in, prec).astype(np.float64) @ rnd(Wo, prec).astype(np.float64).T + bo + y_prev).astype(np.float32)
    gamma, beta = (1.0 + 0.2 * rng.standard_normal(d)), 0.2 * rng.standard_normal(d)
    W1, b1 = rng.standard_normal((8 * d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(8 * d)
    W2, b2 = rng.standard_normal((d, 4 * d)) / np.sqrt(4 * d), 0.3 * rng.standard_normal(d)
    Wpo, bpo = rng.standard_normal((d, d)) / np.sqrt(d), 0.3 * rng.standard_normal(d)
    W1f, b1f = W1 * gamma[None, :], b1 + W1 @ beta
    order = np.concatenate([np.concatenate([np.arange(32 * g, 32 * g + 32), 4 * d + np.arange(32 * g, 32 * g + 32)]) for g in range(4 * d // 32)])
    W1p, b1p = np.ascontiguousarray(W1f[order].astype(np.float32)), b1f[order].astype(np.float32)
    w2f = np.ascontiguousarray(np.concatenate([Wpo @ W2, Wpo], axis=1).astype(np.float32))
    bias2 = (Wpo @ b2 + bpo).astype(np.float32)
    W1r, w2r, yr, y64 = rnd(W1p, prec).astype(np.float64), rnd(w2f, prec).astype(np.float64), rnd(y, prec).astype(np.float64), y.astype(np.float64)
    consts = np.stack([W1r.sum(1), b1p.astype(np.float64)], axis=1).astype(np.float32)
    pre = (1.0 / np.sqrt(y64.var(1, keepdims=True) + 1e-5)) * (yr @ W1r.T - y64.mean(1, keepdims=True) * consts[:, 0].astype(np.float64)[None, :]) + b1p.astype(np.float64)[None, :]
    pg = pre.reshape(M, 4 * d // 32, 2, 32)
    h = (pg[:, :, 0] * 0.5 * pg[:, :, 1] * (1.0 + erf(pg[:, :, 1] / np.sqrt(2.0)))).reshape(M, 4 * d)
    ref = rnd(h.astype(np.float32), prec).astype(np.float64) @ w2r[:, :4 * d].T + yr @ w2r[:, 4 * d:].T + bias2 + x
    ys = y64.reshape(M, d // 64, 64)
    stats = np.stack([ys.sum(2), (ys ** 2).sum(2)], axis=-1).astype(np.float32).reshape(M, -1)
    stream = C.c_void_p()
    if form == "plain":
        _check(lib.ns2vc_pack_ffn(W1p.ctypes.data, w2f.ctypes.data, d, prec, C.byref(stream)), "pack_ffn")
    else:
        _check(lib.ns2vc_pack_ffn_pre(W1p.ctypes.data, w2f.ctypes.data, np.ascontiguousarray(Wo).ctypes.data, d, prec, C.byref(stream)), "pack_ffn_pre")

    def body(ctx):
        f = FfnArgs()
        f.wstream, f.consts, f.bias2 = stream.value, ctx.vec("consts", consts).ptr, ctx.vec("bias2", bias2).ptr
        d_x = ctx.t("res", M, d, "f32", pad=12, col0=4, data=x)
        f.res, f.ldres = d_x.ptr, d_x.ld
        d_o, d_op = ctx.t("out_f32", M, d, "f32", pad=24), ctx.t("out_op", M, d, kind, pad=56, col0=8)
        f.out_f32, f.ldo_f32, f.out_op, f.ldo_op = d_o.ptr, d_o.ld, d_op.ptr, d_op.ld
        d_gs = ctx.t("stats", B, d // 16 * 2, "i64", data=np.zeros((B, d // 16 * 2), np.int64))
        f.stats, f.B, f.T, f.M, f.dim, f.ln_eps = d_gs.ptr, B, T, M, d, 1e-5
        f.ln_health = ctx.t("ln_health", 1, 4, "u32", data=np.zeros((1, 4), np.uint32)).ptr
        if form == "plain":
            d_y = ctx.t("yn", M, d, kind, pad=24, col0=8, data=y)
            f.yn, f.ldy, f.ln_stats = d_y.ptr, d_y.ld, ctx.t("ln_stats", M, d // 64 * 2, "f32", data=stats).ptr
        else:
            d_yp = ctx.t("pre_res", M, d, "f32", pad=20, data=y_prev)
            f.pre_bias, f.pre_res, f.pre_ldres = ctx.vec("pre_bias", bo).ptr, d_yp.ptr, d_yp.ld
            if form == "pre":
                d_oa = ctx.t("pre_a", M, d, kind, pad=40, col0=16, data=o_in)
                f.pre_a, f.pre_lda = d_oa.ptr, d_oa.ld
            else:
                d_q = ctx.t("att_q", M, d, kind, pad=72, col0=8, data=q)
                f.att_q, f.att_ldq, f.att_kv = d_q.ptr, d_q.ld, ctx.t("att_kv", 1, image.size, kind, data=image.reshape(1, -1)).ptr
                if bias is not None:
                    f.att_bias = ctx.t("att_bias", 1, B * Lk, "f32", data=bias.reshape(1, -1)).ptr
                f.att_scale, f.att_Lk = 1.0 / np.sqrt(hd), Lk
        _check(lib.ns2vc_k_ffn(C.byref(f), prec, None), "k_ffn")
        return {"out_f32": d_o, "out_op": d_op, "stats": d_gs}
    label = f"ns2vc_k_ffn / {form} dim={d} B={B} T={T} Lk={Lk} prec={prec}"
    o = run_bounds(diag, label, body, skew=int(form == "pre"))
    lib.ns2vc_dev_free(stream)
    out = o["out_f32"]
    e = rel_l2(out, ref)
    gs, blk = o["stats"].reshape(B, d // 16, 2).astype(np.float64), out.astype(np.float64).reshape(B, T, d // 16, 16)
    e_s = np.abs(gs[..., 0] / 2 ** 28 - blk.sum(axis=(1, 3))).max() / np.abs(blk.sum(axis=(1, 3))).max()
    e_q = np.abs(gs[..., 1] / 2 ** 16 - (blk ** 2).sum(axis=(1, 3))).max() / (blk ** 2).sum(axis=(1, 3)).max()
    diag(f"bounds {label}: P3 rel_l2 {e:.3e} stats {e_s:.2e} / {e_q:.2e}")
    assert e < (tol_ffn_xattn(prec) if form == "att" else TOL_FFN) and e_s < TOL_STATS and e_q < TOL_STATS
    assert np.array_equal(o["out_op"], rnd(out, prec))


@pytest.mark.parametrize("prec", [1, 2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("dim,B,T,nt,Gn", [(128, 3, 70, 1, 8), (128, 3, 70, 2, 4), (256, 2, 97, 1, 8), (384, 3, 97, 0, 8), (384, 3, 97, -2, 8)], ids=str)
def test_rowchain_groupnorm_prologue_bounds(dim, B, T, nt, Gn, prec, diag):
    """ns2vc_k_rowchain with A = GroupNorm(gn_x) built inside the kernel from fp32 rows at a wider pitch and the int64 statistics: token blocks
    that straddle the items, both workgroup sizes, two N-slices."""
    from ns2vc_amd._lib import RowchainArgs
    lib = _lib()
    kind = OP_KIND[prec]
    rng = np.random.default_rng(dim + 7 * B + T)
    d, M, n2 = dim, B * T, 3 * dim
    x = (rng.standard_normal((B, T, d)) * (1.0 + rng.random((B, 1, d))) + rng.standard_normal((B, 1, d))).astype(np.float32)
    gam, bet = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32), (0.2 * rng.standard_normal(d)).astype(np.float32)
    # the rows as the device's GroupNorm rounds them (the reference of _rowchain_groupnorm_prologue)
    c0 = Ctx("zero")
    g_x, g_o = c0.t("x", M, d, "f32", data=x), c0.t("gn", M, d, kind)
    _check(lib.ns2vc_k_groupnorm(g_x.ptr, d, d, None, 0, 0, B, T, Gn, 1e-6, c0.vec("g", gam).ptr, c0.vec("b", bet).ptr, None, 0, 0, 0, g_o.ptr, None, prec, None), "groupnorm")
    a_gn = g_o.read()
    c0.free()
    W1, b1 = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float32), (0.3 * rng.standard_normal(d)).astype(np.float32)
    W2f, b2f = (rng.standard_normal((n2, d)) / np.sqrt(d)).astype(np.float32), (0.3 * rng.standard_normal(n2)).astype(np.float32)
    W1r, W2r = rnd(W1, prec).astype(np.float64), rnd(W2f, prec).astype(np.float64)
    consts = np.stack([W2r.sum(1), b2f.astype(np.float64)], axis=1).astype(np.float32)
    y = a_gn.astype(np.float64) @ W1r.T + b1.astype(np.float64)[None, :]
    yr = rnd(y.astype(np.float32), prec).astype(np.float64)
    z = (yr @ W2r.T - y.mean(1, keepdims=True) * consts[:, 0].astype(np.float64)[None, :]) / np.sqrt(y.var(1, keepdims=True) + 1e-5) + b2f.astype(np.float64)[None, :]
    stream, slices = C.c_void_p(), (2 if nt == -2 else 0)
    if slices:
        _check(lib.ns2vc_pack_rowchain_sliced(W1.ctypes.data, W2f.ctypes.data, d, n2, slices, prec, C.byref(stream)), "pack_rowchain_sliced")
    else:
        _check(lib.ns2vc_pack_rowchain(W1.ctypes.data, W2f.ctypes.data, d, n2, prec, C.byref(stream)), "pack_rowchain")

    def body(ctx):
        f = RowchainArgs()
        d_x = ctx.t("gn_x", M, d, "f32", pad=20, col0=4, data=x)
        d_y, d_z = ctx.t("out1_f32", M, d, "f32", pad=12), ctx.t("out2_op", M, n2, kind, pad=40, col0=8)
        f.lda, f.wstream, f.bias1, f.consts2 = d, stream.value, ctx.vec("bias1", b1).ptr, ctx.vec("consts2", consts).ptr
        f.out1_f32, f.ldo1, f.out2_op, f.ldo2 = d_y.ptr, d_y.ld, d_z.ptr, d_z.ld
        f.ln_eps, f.M, f.dim, f.n2, f.slices = 1e-5, M, d, n2, slices
        f.gn_x, f.ldx = d_x.ptr, d_x.ld
        f.gn_stats = ctx.t("gn_stats", B, d // 16 * 2, "i64", data=_gn_stats(x, B, T, d).reshape(B, -1)).ptr
        f.gn_gamma, f.gn_beta, f.gn_eps, f.T, f.G = ctx.vec("gn_gamma", gam).ptr, ctx.vec("gn_beta", bet).ptr, 1e-6, T, Gn
        _check(lib.ns2vc_debug_set_rowchain_tokens(max(nt, 0)), "set_rowchain_tokens")
        try:
            _check(lib.ns2vc_k_rowchain(C.byref(f), prec, None), "k_rowchain")
        finally:
            lib.ns2vc_debug_set_rowchain_tokens(0)
        return {"out1_f32": d_y, "out2_op": d_z}
    label = f"ns2vc_k_rowchain / GroupNorm prologue dim={d} B={B} T={T} nt={nt} G={Gn} prec={prec}"
    o = run_bounds(diag, label, body)
    lib.ns2vc_dev_free(stream)
    e_y, e_z = rel_l2(o["out1_f32"], y), rel_l2(o["out2_op"], z)
    diag(f"bounds {label}: P3 y {e_y:.3e} z {e_z:.3e}")
    assert e_y < TOL_ROWCHAIN_GN_Y and e_z < eps16(prec)


# ---------------------------------------------------------------------------------------------------------------------------------------
# layouts a launcher refuses: the ONLY cases of this file that are not run.  Each row: entry point, layout, the header sentence that forbids
# it.  None of them is a layout plan.cpp's Planner passes (its lda* / ldo* are channel counts, multiples of 64 elements, and its workspace
# slices are 256-byte aligned).  If a launcher starts accepting one, the test fails until the row is removed and the layout is run above.
# ---------------------------------------------------------------------------------------------------------------------------------------
EXPECTED_REFUSALS = [
    ("ns2vc_k_gemm", "lda0 = c0 + 4 elements: rows that do not start on 16 bytes",
     "Conventions: operand-typed source tensors ... row pitches that are multiples of 16 bytes -- a pitch that is not is refused"),
    ("ns2vc_k_gemm", "gnp_sync with a0 16 bytes past a 128-byte line",
     "ns2vc_gemm_args.gnp_sync: Needs a0 128-byte aligned and whole 128-byte lines per row"),
    # per-item valid lengths where no masked kernel form exists: refused, never run unmasked
    ("ns2vc_k_gemm", "lens with a forced 4-wave tile: (64, 128, 2)",
     "ns2vc_gemm_args.lens: Served by the masked instantiations of the tap-sharing conv kernel ... and of the 8-wave GEMM kernel ...; every other combination is refused"),
    ("ns2vc_k_gemm", "lens with N = 192 on a linear launch: the 64-column tiles of the 4-wave kernel",
     "ns2vc_gemm_args.lens: N % 128 != 0 ... outside it"),
    ("ns2vc_k_gemm", "lens with GEGLU N = 1024 under the heuristic: the 4-wave kernel",
     "ns2vc_gemm_args.lens: a narrow GEGLU (N < 2048) outside it"),
    ("ns2vc_k_gemm", "lens with ln_stats: a LayerNorm-by-linearity consumer",
     "ns2vc_gemm_args.lens: rowstats, ln_stats"),
    ("ns2vc_k_gemm", "lens with sol_coef: the solver epilogue",
     "ns2vc_gemm_args.lens: sol_coef"),
    ("ns2vc_k_gemm", "lens with gnp_x and algo = 1: the prologue on the 8-wave kernel",
     "ns2vc_gemm_args.lens: gnp_x outside the tap-sharing kernel"),
    ("ns2vc_k_gemm", "lens with M != B * Tout: M one row short",
     "ns2vc_gemm_args.lens: The per-item period of the rows is Tout"),
    ("ns2vc_k_gemm", "stats with Tout = 63: below the smallest period the statistics take",
     "ns2vc_gemm_args.stats: needs Tout >= 64"),
    ("ns2vc_k_geglu", "ldo = 4 dim - 8: an output pitch narrower than the hidden width",
     "ns2vc_geglu_args: out_op [M][ldo] (>= 4 dim columns)"),
    ("ns2vc_k_attention", "pv_fp8 with fp32 operands",
     "ns2vc_attn_args.pv_fp8: 16-bit precisions only"),
    ("ns2vc_k_noise", "ld = 102: rows that are no multiple of 4 floats",
     "ns2vc_k_noise: out = fp32 rows [B*T][ld] (ld % 4 == 0)"),
]


@pytest.mark.parametrize("row", EXPECTED_REFUSALS, ids=lambda r: r[0] + ":" + r[1].split(":")[0].replace(" ", "_"))
def test_expected_refusals(row, diag):
    """non-zero return, no launch: every buffer the refused call names is untouched (logical region included)"""
    from ns2vc_amd._lib import AttnArgs, GegluArgs, GemmArgs
    lib = _lib()
    entry, layout, _ = row
    ctx = Ctx("nan")
    prec, kind = 2, "f16"
    diag(f"bounds refusal {entry} / {layout}: call")
    if entry == "ns2vc_k_gemm" and (layout.startswith("lens") or layout.startswith("stats")):
        # an otherwise ordinary launch on owned buffers (outputs prefilled with NaN); only what the row names is wrong
        what = layout.split(":")[0]
        B, T, Cc, N, taps = 2, (63 if "Tout = 63" in what else 70), 128, 128, 1
        geglu = "GEGLU" in what
        if "N = 192" in what:
            N = 192
        if geglu:
            N = 1024
        if "gnp_x" in what or "sol_coef" in what:
            taps = 3                                     # (sol_coef: k = 3, T >= 66, N = 128 -- the tap-sharing kernel's own solver epilogue, were lens not set)
        M, K, Nout = B * T, taps * Cc, (N // 2 if geglu else N)
        rng = np.random.default_rng(3)
        d_w = _pack(rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec), prec)
        g = GemmArgs()
        x = rng.standard_normal((M, Cc)).astype(np.float32)
        d_a = ctx.t("a0", M, Cc, kind, data=rnd(x, prec))
        g.a0, g.c0, g.lda0 = d_a.ptr, Cc, d_a.ld
        g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, (M - 1 if "M != B" in what else M), taps, 0
        g.w, g.K, g.N, g.geglu = d_w.value, K, N, int(geglu)
        d_o = ctx.t("out_f32", M, Nout, "f32", pad=8)
        d_op = ctx.t("out_op", M, Nout, kind, pad=8)
        g.out_f32, g.ldo_f32, g.out_op, g.ldo_op = d_o.ptr, d_o.ld, d_op.ptr, d_op.ld
        if what.startswith("lens"):
            g.lens = ctx.t("lens", 1, B, "i32", data=np.array([[T, T // 2]], np.int32)).ptr
        else:
            g.stats = ctx.t("stats", B, N // 16 * 2, "i64", data=np.zeros((B, N // 16 * 2), np.int64)).ptr
        if "ln_stats" in what:
            g.ln_stats = ctx.t("ln_stats", M, 4, "f32", data=np.ones((M, 4))).ptr
            g.ln_wsum, g.ln_eps, g.ln_dim = ctx.vec("ln_wsum", np.zeros(N, np.float32)).ptr, 1e-5, Cc
        if "sol_coef" in what:
            g.sol_coef, g.sol_ncoef = ctx.t("sol_coef", 2, 12, "f32", data=np.ones((2, 12))).ptr, 12
            g.sol_step = ctx.t("sol_step", 1, 4, "i32", data=np.zeros((1, 4), np.int32)).ptr
            state = [ctx.t(n_, M, N, "f32", data=np.ones((M, N))) for n_ in ("sol_xe", "sol_xbar", "sol_d1", "sol_mprev")]
            g.sol_xe, g.sol_xbar, g.sol_d1, g.sol_mprev, g.sol_ld = state[0].ptr, state[1].ptr, state[2].ptr, state[3].ptr, N
            g.sol_xe_op = ctx.t("sol_xe_op", M, N, kind, data=np.ones((M, N))).ptr
        if "gnp_x" in what:
            g.gnp_x, g.gnp_ldx = ctx.t("gnp_x", M, Cc, "f32", data=x).ptr, Cc
            g.gnp_stats = ctx.t("gnp_stats", B, Cc // 16 * 2, "i64", data=_gn_stats(x, B, T, Cc).reshape(B, -1)).ptr
            g.gnp_gamma, g.gnp_beta = ctx.vec("g", np.ones(Cc, np.float32)).ptr, ctx.vec("b", np.zeros(Cc, np.float32)).ptr
            g.gnp_eps, g.gnp_G, g.algo = 1e-5, 8, 1
        tile = (64, 128, 2) if "4-wave tile" in what else (0, 0, 0)
        _check(lib.ns2vc_debug_set_gemm_tile(*tile), "set tile")
        try:
            rc = lib.ns2vc_k_gemm(C.byref(g), prec, None)
            msg = lib.ns2vc_last_error()
            untouched = all(np.array_equal(g_._download(), g_.image) for g_ in ctx.bufs)
            # the control: what the row names is the ONLY thing wrong -- the same launch without `lens` (a `stats` row: without `stats`) runs
            if "M != B" in what:
                g.M = M
            elif what.startswith("lens"):
                g.lens = None
            else:
                g.stats = None
            rc_twin = lib.ns2vc_k_gemm(C.byref(g), prec, None)
            msg_twin = lib.ns2vc_last_error() if rc_twin else b""
            _check(lib.ns2vc_dev_sync(), "sync")
        finally:
            lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
        lib.ns2vc_dev_free(d_w)
        diag(f"bounds refusal {entry} / {layout}: rc {rc} ({msg.decode() if msg else ''}) buffers untouched {untouched}; without it rc {rc_twin} ({msg_twin.decode()})")
        ctx.free()
        assert rc != 0 and untouched and b"refused by the argument check" in msg, (rc, msg)
        assert rc_twin == 0, msg_twin
        return
    elif entry == "ns2vc_k_gemm":
        B, T, Cc, N = 2, 70, 128, 256
        M = B * T
        W = np.zeros((N, Cc), np.float32)
        d_w = _pack(W, prec)
        g = GemmArgs()
        sync_case = "gnp_sync" in layout
        d_a = Guarded(_be(), M, Cc, kind, ld=Cc + 64, col0=8 if sync_case else 0, fill="nan", name="a0", data=None if sync_case else np.ones((M, Cc)))
        ctx.bufs.append(d_a)
        g.a0, g.c0, g.lda0 = d_a.ptr, Cc, (d_a.ld if sync_case else Cc + 4)
        g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, M, 1, 0
        g.w, g.K, g.N = d_w.value, Cc, N
        d_o = ctx.t("out_f32", M, N, "f32", pad=8)
        g.out_f32, g.ldo_f32 = d_o.ptr, d_o.ld
        if sync_case:
            x = np.random.default_rng(0).standard_normal((B, T, Cc)).astype(np.float32)
            g.gnp_x, g.gnp_ldx = ctx.t("gnp_x", M, Cc, "f32", data=x).ptr, Cc
            g.gnp_stats = ctx.t("gnp_stats", B, Cc // 16 * 2, "i64", data=_gn_stats(x, B, T, Cc).reshape(B, -1)).ptr
            g.gnp_gamma, g.gnp_beta = ctx.vec("g", np.ones(Cc, np.float32)).ptr, ctx.vec("b", np.zeros(Cc, np.float32)).ptr
            g.gnp_eps, g.gnp_G, g.algo = 1e-5, 8, 2
            g.gnp_sync = ctx.t("gnp_sync", 1, 4, "u64", data=np.zeros((1, 4), np.uint64)).ptr
        rc = lib.ns2vc_k_gemm(C.byref(g), prec, None)
        lib.ns2vc_dev_free(d_w)
    elif entry == "ns2vc_k_geglu":
        d, M = 384, 5
        f = GegluArgs()
        d_y = ctx.t("yn", M, d, kind, data=np.ones((M, d)))
        d_h = ctx.t("out_op", M, 4 * d, kind)
        f.yn, f.ldy, f.ln_eps = d_y.ptr, d, 1e-5
        f.ln_stats = ctx.t("ln_stats", M, 12, "f32", data=np.ones((M, 12))).ptr
        f.wstream = f.consts = d_y.ptr                   # (never read: the call is refused before anything is launched)
        f.out_op, f.ldo, f.M, f.dim = d_h.ptr, 4 * d - 8, M, d
        rc = lib.ns2vc_k_geglu(C.byref(f), prec, None)
    elif entry == "ns2vc_k_attention":       # an otherwise valid fp32 launch on owned buffers: only the flag is wrong
        Bq, L, D = 2, 5, 128
        a = AttnArgs()
        d_q = ctx.t("qkv", Bq * L, 3 * D, "f32", pad=8, data=np.ones((Bq * L, 3 * D)))
        d_o = ctx.t("out", Bq * L, D, "f32", pad=8)
        a.q, a.k, a.v, a.ldq, a.ldk, a.ldv = d_q.ptr, d_q.ptr + 4 * D, d_q.ptr + 8 * D, d_q.ld, d_q.ld, d_q.ld
        a.B, a.H, a.Lq, a.Lk, a.scale, a.out, a.ldo, a.pv_fp8 = Bq, 8, L, L, 0.25, d_o.ptr, d_o.ld, 1
        rc = lib.ns2vc_k_attention(C.byref(a), 16, 0, None)
    else:
        d_s = ctx.t("seeds", 1, 2, "u64", data=np.array([[1, 2]], np.uint64))
        d_o = ctx.t("out", 2 * 8, 104, "f32")
        rc = lib.ns2vc_k_noise(d_s.ptr, 2, 100, 8, 102, 0, None, d_o.ptr, None)
    msg = lib.ns2vc_last_error()
    untouched = all(np.array_equal(g_._download(), g_.image) for g_ in ctx.bufs)
    diag(f"bounds refusal {entry} / {layout}: rc {rc} ({msg.decode() if msg else ''}) buffers untouched {untouched}")
    ctx.free()
    assert rc != 0 and untouched


# ---------------------------------------------------------------------------------------------------------------------------------------
# positive control: the harness notices stores outside what it was TOLD the tensor is.  Safe by construction: the harness lays the block out at
# a pitch 8 elements WIDER than the pitch the kernel is given, so the kernel's rows drift into what the harness holds to be gap columns and
# stay inside the owned block (M rows at the narrower pitch end before M rows at the wider one) -- a wrong expectation, not a wrong launch.
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_positive_control_gemm_and_btc_to_nct(diag):
    from ns2vc_amd._lib import GemmArgs
    lib = _lib()
    prec, B, T, Cc, N = 2, 2, 41, 128, 128
    M = B * T
    rng = np.random.default_rng(9)
    a0, W = rnd(rng.standard_normal((M, Cc)), prec), rnd(rng.standard_normal((N, Cc)) / np.sqrt(Cc), prec)
    d_w = _pack(W, prec)
    ctx = Ctx("nan")
    d_a = ctx.t("a0", M, Cc, "f16", pad=8, data=a0)
    d_o = ctx.t("out_f32", M, N, "f32", pad=16)
    g = GemmArgs()
    g.a0, g.lda0, g.c0 = d_a.ptr, d_a.ld, Cc
    g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, M, 1, 0
    g.w, g.K, g.N = d_w.value, Cc, N
    g.out_f32, g.ldo_f32 = d_o.ptr, d_o.ld - 8
    assert N <= g.ldo_f32 < d_o.ld
    diag("bounds positive control ns2vc_k_gemm: launch")
    _launch_gemm(g, prec, (0, 0, 0))
    v = d_o.violations(limit=10 ** 6)
    diag(f"bounds positive control ns2vc_k_gemm: {len(v)} violations, first {v[:2]}")
    assert v and all("out_f32: gap row" in s_ for s_ in v)
    assert d_a.violations() == []
    assert rel_l2(d_o.read()[0], a0[0].astype(np.float64) @ W.astype(np.float64).T) < TOL[prec]   # row 0 sits where both agree
    lib.ns2vc_dev_free(d_w)
    ctx.free()

    Bc, Cn, Tn = 2, 100, 40
    x = rng.standard_normal((Bc, Tn, Cn)).astype(np.float32)
    ctx = Ctx("inf")
    d_y = ctx.t("src_btc", Bc * Tn, Cn, "f32", pad=12, data=x)
    d_z = ctx.t("dst_nct", Bc * Cn, Tn, "f32", pad=8)         # the kernel writes (b, c) rows of T contiguous floats: pitch T, not T + 8
    diag("bounds positive control ns2vc_k_btc_to_nct: launch")
    _check(lib.ns2vc_k_btc_to_nct(d_y.ptr, d_y.ld, Cn, Tn, Bc, d_z.ptr, None), "btc_to_nct")
    v = d_z.violations(limit=10 ** 6)
    diag(f"bounds positive control ns2vc_k_btc_to_nct: {len(v)} violations, first {v[:2]}")
    assert v and all("dst_nct: gap row" in s_ for s_ in v)
    assert d_y.violations() == []
    ctx.free()
