"""The epilogue of csrc/epilogue.h under per-item valid lengths (ns2vc_gemm_args.lens), kernel instance by kernel instance and in all three operand
precisions, through the C ABI (ctypes + numpy).  Every launch of the table in tests/epilogue_ref.py runs under three `lens` vectors (all full, all 1,
and one that puts an item's end on every tile row of epilogue_ref.GEMM_RESIDUES / CONV_RESIDUES; the short-item cases: a hand-made mix) next to its
dense twin on the same inputs -- same forced instance, lens = NULL -- and once more with ONE length changed; epilogue_ref.check_launch holds each to
the header's contract (its checks 1-8), and tests/test_epilogue_ref_cpu.py shows that this checker reports eight subtly wrong kernels at these shapes.

Inputs under lengths: the residual's rows past an item's end hold NaN (residue / mixed vector) or Inf (all-1 vector); the operand rows there hold
the same for taps = 1 and zeros for k = 3 (the row invariant).  Every buffer of a launch sits in a guarded block (tests/guard.py).

Bounds: TOL of tests/test_kernels_gpu.py, TOL_STATS of tests/util.py, the fixed-point half units of the header's scales -- nothing of this file's own.

Case C5 (the conv instances): the masked GroupNorm prologue of the tap-sharing kernel (gnpro.h MASKED) in all three precisions -- one source, and
a concat of two (a group straddles the seam) with the raw operand copy; time scale / shift and SiLU on and off; algo 2, algo 0 (run as 2) and the
cooperative form (gnp_sync), which must give the same bits.  Operand rows against fp64 from the int64 statistics the launch is handed, divisor
L_b * C_g, per item and over the tensor: util.tol_gnp_rows(prec); rows of an item with L_b >= 66 bitwise equal to the dense prologue launched for that
item alone (B = 1, T = L_b).  Measured on an MI355X: bitwise in every instance and precision (largest ulp distance 0)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import epilogue_ref as R
from guard import OP_KIND, DeviceBackend, Guarded
from test_kernels_gpu import TOL
from util import gather_rows, rel_l2, tol_gnp_rows

pytestmark = pytest.mark.gpu

PRECS, PREC_IDS = [0, 1, 2], ["fp32", "bf16", "fp16"]
_G64, _G32 = R.geometry("gemm", 128, 64), R.geometry("gemm", 64, 32)
_G2 = R.geometry("gemm", 64, 32, commits=1)             # the 4-wave kernel: one wave, one commit per wave tile
# name -> kinds of launch it takes, forced tile, conv_bn, row tiling (tile rows, rows per wave commit), masked (has a masked epilogue)
INSTANCES = {
    "g4_128x128s12": dict(kinds=("gemm",), tile=(128, 128, 12), geom={"gemm": _G64}, masked=True),
    "g4_128x128s13": dict(kinds=("gemm",), tile=(128, 128, 13), geom={"gemm": _G64}, masked=True),
    "g4_64x128s12": dict(kinds=("gemm",), tile=(64, 128, 12), geom={"gemm": _G32}, masked=True),
    "g4_64x128s13": dict(kinds=("gemm",), tile=(64, 128, 13), geom={"gemm": _G32}, masked=True),
    "g4_128x128s23": dict(kinds=("gemm",), tile=(128, 128, 23), geom={"gemm": _G64}, masked=True),
    "g4_64x128s23": dict(kinds=("gemm",), tile=(64, 128, 23), geom={"gemm": _G32}, masked=True),
    "ts_conv_bn64": dict(kinds=("conv",), tile=(0, 0, 0), conv_bn=64, geom={"conv": R.geometry("conv", wave_rows=32)}, masked=True),
    "ts_conv_bn128": dict(kinds=("conv",), tile=(0, 0, 0), conv_bn=128, geom={"conv": R.geometry("conv", wave_rows=64)}, masked=True),
    "ts_128x64s58": dict(kinds=("conv",), tile=(128, 64, 58), geom={"conv": R.geometry("conv", wave_rows=32)}, masked=True),
    "ts_128x128s58": dict(kinds=("conv",), tile=(128, 128, 58), geom={"conv": R.geometry("conv", wave_rows=64)}, masked=True),
    # the heuristic at these sizes: a 64 x 128 tile (ring 13 or 23; the wide GEGLU: 128 x 128, see _geom) and the 64-column conv tile
    "heuristic": dict(kinds=("gemm", "conv"), tile=(0, 0, 0), geom={"gemm": _G32, "conv": R.geometry("conv", wave_rows=32)}, masked=True),
    # the 4-wave kernel: no masked epilogue (a refusal row of tests/test_kernel_bounds_gpu.py), the dense-only rows
    "g2_64x128s2": dict(kinds=("gemm",), tile=(64, 128, 2), geom={"gemm": _G2}, masked=False),
    "g2_64x64s2": dict(kinds=("gemm",), tile=(64, 64, 2), geom={"gemm": _G2}, masked=False),
    "g2_64x64s3": dict(kinds=("gemm",), tile=(64, 64, 3), geom={"gemm": _G2}, masked=False),
    "g2_64x64s4": dict(kinds=("gemm",), tile=(64, 64, 4), geom={"gemm": _G2}, masked=False),
}
# a forced 4-loader / K-split conv tile under lens runs the 8-loader plain masked form: the bits of the conv_bn launch
TS_ALIASES = {64: [(128, 64, 54), (128, 64, 58), (128, 64, 64), (128, 64, 68)], 128: [(128, 128, 54), (128, 128, 58)]}


def _geom(inst, name, case):
    """row tiling of the instance that runs `case`.  The heuristic (launch_typed, gemm.hip): GEGLU with N >= 2048 -> the 128 x 128 tile; N <= 512 with
    M < 7000 rows -> a 64-row tile (ring 13 or 23: the same row tiling)"""
    if name == "heuristic" and case["geglu"] and case["N"] >= 2048:
        return _G64
    return inst["geom"][case["kern"]]


def _applies(case, name):
    inst = INSTANCES[name]
    if case["kern"] not in inst["kinds"]:
        return False
    if case["name"] == "G7_geglu_n2048":
        return name == "heuristic"                      # (the wide GEGLU: the heuristic's own 128 x 128 tile)
    if case["name"] == "G7_geglu_n256":
        return name != "heuristic"                      # (narrow GEGLU under the heuristic = the 4-wave kernel: a refusal row)
    if case["kern"] == "conv" and case["N"] % 128 and (inst.get("conv_bn") == 128 or inst["tile"][1] == 128):
        return False                                    # N = 64 / 192: the 64-column tile only
    return True


# the least each instance must have run; spelled out, not derived from _applies
_G = {"G1_linear_res_dual_stats", "G2_linear_alias_f32only_stats", "G3_linear_op_only", "G4_conv3_8wave_concat_seg_slice_stats", "G5_stride2_odd_stats",
      "G5_stride2_even_stats", "G6_up2_odd_stats", "G6_up2_even_stats", "G8_short_linear_T24", "G8_short_linear_T19", "G8_short_conv3_T24", "G8_short_conv3_T19"}
_C128 = {"C1_conv_n128", "C1_conv_n256", "C2_conv_concat_seg_alias_stats"}
_C128 |= {"C5_gnp_one", "C5_gnp_concat_raw"}
_C64 = _C128 | {"C3_conv_n64", "C3_conv_n192"}
_DG = {"D_stride2_stats", "D_up2_stats", "D_linear_T64_stats", "D_linear_T65_stats", "D_conv3_T64_stats", "D_conv3_T65_stats"}
_DC = {"D_conv_T66_stats", "D_conv_T67_stats"}
EXPECTED_CASES = {n: (_G | {"G7_geglu_n256"} | _DG) for n in INSTANCES if n.startswith("g4_")}
EXPECTED_CASES.update({"ts_conv_bn64": _C64 | _DC, "ts_128x64s58": _C64 | _DC, "ts_conv_bn128": _C128 | _DC, "ts_128x128s58": _C128 | _DC,
                       "heuristic": _G | {"G7_geglu_n2048"} | _C64 | _DG | _DC})
EXPECTED_CASES.update({n: _DG for n in INSTANCES if n.startswith("g2_")})

_BE = None
_INPUTS = {}            # (case, prec, vector) -> inputs with their fp64 reference: computed once, shared by every instance, never written to


def _be():
    global _BE
    if _BE is None:
        _BE = DeviceBackend()
    return _BE


def _inputs(case, prec, vec_name, lens, fill):
    key = (case["name"], prec, vec_name)
    if key not in _INPUTS:
        inp = R.make_inputs(case, prec, lens, fill)
        inp["_ref"] = R.reference(inp)
        _INPUTS[key] = inp
    return _INPUTS[key]


class Weights:
    def __init__(self, inp, tiled):
        lib, case = _be().lib, inp["case"]
        W = np.ascontiguousarray(inp["W"], dtype=np.float32)
        self.w, self.wt = C.c_void_p(), None
        _be().check(lib.ns2vc_pack_weight(W.ctypes.data, W.shape[0], W.shape[1], inp["prec"], C.byref(self.w)), "pack_weight")
        if tiled:
            self.wt = C.c_void_p()
            _be().check(lib.ns2vc_pack_conv3_tiled(W.ctypes.data, W.shape[0], case["c0"] + case["c1"], case["c2"], inp["prec"], C.byref(self.wt)), "pack_conv3_tiled")

    def free(self):
        for p in (self.w, self.wt):
            if p is not None:
                _be().lib.ns2vc_dev_free(p)


def launch(inp, wts, tile, conv_bn=0, masked=True, tiled=False, fill="nan"):
    """one ns2vc_k_gemm launch of inp's case on guarded buffers -> {out_f32, out_op, stats, viol}; masked = False: the dense twin (lens = NULL)"""
    from ns2vc_amd._lib import GemmArgs
    be, lib = _be(), _be().lib
    case, prec = inp["case"], inp["prec"]
    kind = OP_KIND[prec]
    B, Tin, Tout, N, Nout = case["B"], case["Tin"], case["Tout"], case["N"], inp["Nout"]
    M = B * Tout
    bufs = []

    def t(name, rows, width, k, pad=0, col0=0, data=None):
        g_ = Guarded(be, rows, width, k, ld=col0 + width + pad, col0=col0, fill=fill, data=data, name=name)
        bufs.append(g_)
        return g_

    g = GemmArgs()
    d_a0 = t("a0", B * Tin, case["c0"], kind, pad=8 if case["slice"] else 0, col0=16 if case["slice"] else 0, data=inp["a0"])
    g.a0, g.lda0, g.c0 = d_a0.ptr, d_a0.ld, case["c0"]
    if case["c1"]:
        d_a1 = t("a1", B * Tin, case["c1"], kind, pad=40, data=inp["a1"])
        g.a1, g.lda1, g.c1 = d_a1.ptr, d_a1.ld, case["c1"]
    if case["c2"]:
        d_a2 = t("a2", B * Tin, case["c2"], kind, pad=72, col0=8, data=inp["a2"])
        g.a2, g.lda2, g.c2 = d_a2.ptr, d_a2.ld, case["c2"]
    g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, Tin, Tout, M, case["taps"], case["tmode"]
    g.w, g.K, g.N = wts.w.value, inp["W"].shape[1], N
    if tiled:
        g.w_tiled = wts.wt.value
    if inp["bias"] is not None:
        g.bias = t("bias", 1, N, "f32", data=inp["bias"].reshape(1, -1)).ptr
    g.geglu, g.algo, g.conv_bn = case["geglu"], case["algo"], conv_bn
    d_o = d_op = d_s = None
    if case["out"] in ("both", "f32"):
        d_o = t("out_f32", M, Nout, "f32", pad=24, col0=4, data=inp["res"] if case["res"] == "alias" else None)
        g.out_f32, g.ldo_f32 = d_o.ptr, d_o.ld
    if case["res"] == "alias":
        g.res, g.ldres = d_o.ptr, d_o.ld
    elif case["res"]:
        d_r = t("res", M, Nout, "f32", pad=12, data=inp["res"])
        g.res, g.ldres = d_r.ptr, d_r.ld
    if case["out"] in ("both", "op"):
        d_op = t("out_op", M, Nout, kind, pad=56, col0=8)
        g.out_op, g.ldo_op = d_op.ptr, d_op.ld
    if case["stats"]:
        d_s = t("stats", B, N // 16 * 2, "i64", data=np.zeros((B, N // 16 * 2), np.int64))
        g.stats = d_s.ptr
    if masked:
        g.lens = t("lens", 1, B, "i32", data=inp["lens"].reshape(1, -1)).ptr
    be.check(lib.ns2vc_debug_set_gemm_tile(*tile), "set tile")
    try:
        be.check(lib.ns2vc_k_gemm(C.byref(g), prec, None), f"k_gemm {case['name']} tile={tile} conv_bn={conv_bn} masked={masked}")
        be.check(lib.ns2vc_dev_sync(), "sync")
    finally:
        lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
    out = dict(out_f32=None if d_o is None else d_o.read().copy(), out_op=None if d_op is None else np.asarray(d_op.read(), np.float32).copy(),
               stats=None if d_s is None else d_s.read().reshape(B, N // 16, 2).astype(np.int64), viol=[v for b_ in bufs for v in b_.violations()])
    for b_ in bufs:
        b_.free()
    return out


def _same_bits(a, b):
    for k in ("out_f32", "out_op"):
        if (a[k] is None) != (b[k] is None) or (a[k] is not None and not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32))):
            return False
    return (a["stats"] is None and b["stats"] is None) or np.array_equal(a["stats"], b["stats"])


# ---------------------------------------------------------------------------------------------------------------------------------------
# C5: the masked GroupNorm prologue of the tap-sharing kernel
# ---------------------------------------------------------------------------------------------------------------------------------------
C5_B, C5_T, C5_N = 5, 131, 256                          # 660 padded rows = 6 row blocks; N = 256: 4 | 2 column tiles share a row block (gnp_sync)
C5_LENS = np.array([131, 127, 66, 1, 40], np.int32)     # three items the prologue also takes alone (L_b >= 66), an L = 1 item, a short one
# channels of gnp_x, of gnp_x1, groups.  concat: C_g = 32, group 2 = channels 64 .. 95 straddles the seam at 80; the raw copy (gnp_raw) is on
C5_SOURCES = {"C5_gnp_one": (128, 0, 8), "C5_gnp_concat_raw": (80, 48, 4)}
_C5 = {}


def _c5_inputs(src, prec):
    if (src, prec) in _C5:
        return _C5[(src, prec)]
    c0, c1, Gn = src
    B, T, N, Cn, lens = C5_B, C5_T, C5_N, c0 + c1, C5_LENS
    rng = np.random.default_rng(1000 + c0)
    x = (rng.standard_normal((B, T, Cn)) * (1.0 + 0.5 * rng.random((B, 1, Cn))) + 0.3 * rng.standard_normal((B, 1, Cn))).astype(np.float32)
    d = dict(src=src, x=x, gamma=(1.0 + 0.2 * rng.standard_normal(Cn)).astype(np.float32), beta=(0.2 * rng.standard_normal(Cn)).astype(np.float32),
             temb=(0.3 * rng.standard_normal((B, 2 * Cn))).astype(np.float32), bias=rng.standard_normal(N).astype(np.float32),
             W=R.rnd(rng.standard_normal((N, 3 * Cn)) / np.sqrt(3 * Cn), prec))
    # the statistics a masked producer leaves: over the valid rows, per source
    d["stats"] = [R.stats_fixed(x[..., a:b].reshape(B * T, b - a), B, T, lens) for a, b in ((0, c0), (c0, Cn)) if b > a]
    # fp64 rows from THOSE integers (they are the launch's input), divisor L_b * C_g
    st = np.concatenate(d["stats"], axis=1).astype(np.float64)
    Cg = Cn // Gn
    S = (st[..., 0] / R.SUM_SCALE).reshape(B, Gn, Cg // 16).sum(-1)
    Q = (st[..., 1] / R.SQ_SCALE).reshape(B, Gn, Cg // 16).sum(-1)
    n = (lens.astype(np.float64) * Cg)[:, None]
    mean = S / n
    var = Q / n - mean * mean
    xg = x.astype(np.float64).reshape(B, T, Gn, Cg)
    d["norm"] = ((xg - mean[:, None, :, None]) / np.sqrt(var[:, None, :, None] + 1e-5)).reshape(B, T, Cn) * d["gamma"].astype(np.float64) + d["beta"].astype(np.float64)
    _C5[(src, prec)] = d
    return d


def _c5_rows(d, temb_on, silu):
    y = d["norm"]
    Cn = y.shape[-1]
    if temb_on:
        y = y * (1.0 + d["temb"][:, None, :Cn].astype(np.float64)) + d["temb"][:, None, Cn:].astype(np.float64)
    if silu:
        y = y / (1.0 + np.exp(-y))
    return y * R.valid_mask(C5_B, C5_T, C5_LENS).reshape(C5_B, C5_T, 1)


def c5_launch(d, wts, prec, tile, conv_bn, algo, sync, temb_on, silu, item=None):
    """the prologue launch under C5_LENS; item = b: the DENSE materialising prologue for item b alone (B = 1, T = L_b, lens = NULL)"""
    from ns2vc_amd._lib import GemmArgs
    be, lib = _be(), _be().lib
    kind = OP_KIND[prec]
    c0, c1, Gn = d["src"]
    Cn, N = c0 + c1, C5_N
    if item is None:
        B, T, x, temb, stats = C5_B, C5_T, R._poison(d["x"].reshape(C5_B * C5_T, Cn), C5_B, C5_T, C5_LENS, np.float32(np.nan)), d["temb"], d["stats"]
    else:
        B, T = 1, int(C5_LENS[item])
        x, temb, stats = d["x"][item, :T], d["temb"][item:item + 1], [s_[item:item + 1] for s_ in d["stats"]]
    M = B * T
    bufs = []

    def t(name, rows, width, k, pad=0, col0=0, data=None):
        g_ = Guarded(be, rows, width, k, ld=col0 + width + pad, col0=col0, fill="nan", data=data, name=name)
        bufs.append(g_)
        return g_

    g = GemmArgs()
    d_a = t("a0", M, Cn, kind)                                                   # (whole 128-byte lines per row, 128-byte aligned: what gnp_sync asks)
    g.a0, g.lda0, g.c0 = d_a.ptr, d_a.ld, Cn
    g.B, g.Tin, g.Tout, g.M, g.taps, g.tmode = B, T, T, M, 3, 0
    g.w, g.K, g.N, g.bias = wts.w.value, 3 * Cn, N, t("bias", 1, N, "f32", data=d["bias"].reshape(1, -1)).ptr
    d_o = t("out_f32", M, N, "f32", pad=8)
    g.out_f32, g.ldo_f32 = d_o.ptr, d_o.ld
    d_x = t("gnp_x", M, c0, "f32", pad=8, data=x.reshape(M, Cn)[:, :c0])
    g.gnp_x, g.gnp_ldx = d_x.ptr, d_x.ld
    g.gnp_stats = t("gnp_stats", B, c0 // 16 * 2, "i64", data=stats[0].reshape(B, -1)).ptr
    g.gnp_gamma, g.gnp_beta = t("gnp_gamma", 1, Cn, "f32", data=d["gamma"].reshape(1, -1)).ptr, t("gnp_beta", 1, Cn, "f32", data=d["beta"].reshape(1, -1)).ptr
    if temb_on:
        d_t = t("gnp_temb", B, 2 * Cn, "f32", pad=16, col0=8, data=temb)             # (scale | shift) inside a wider per-item row
        g.gnp_temb, g.gnp_ldtemb = d_t.ptr, d_t.ld
    g.gnp_eps, g.gnp_G, g.gnp_silu, g.algo, g.conv_bn = 1e-5, Gn, silu, algo, conv_bn
    d_r = None
    if c1:
        d_x1 = t("gnp_x1", M, c1, "f32", pad=4, col0=4, data=x.reshape(M, Cn)[:, c0:])
        g.gnp_x1, g.gnp_ldx1, g.gnp_c1 = d_x1.ptr, d_x1.ld, c1
        g.gnp_stats1 = t("gnp_stats1", B, c1 // 16 * 2, "i64", data=stats[1].reshape(B, -1)).ptr
        d_r = t("gnp_raw", M, Cn, kind)
        g.gnp_raw = d_r.ptr
    if sync:
        g.gnp_sync = t("gnp_sync", 1, (M + 63) // 64, "u64", data=np.zeros((1, (M + 63) // 64), np.uint64)).ptr
    if item is None:
        g.lens = t("lens", 1, B, "i32", data=C5_LENS.reshape(1, -1)).ptr
    be.check(lib.ns2vc_debug_set_gemm_tile(*tile), "set tile")
    try:
        be.check(lib.ns2vc_k_gemm(C.byref(g), prec, None), f"k_gemm C5 {d['src']} tile={tile} conv_bn={conv_bn} algo={algo} sync={sync} item={item}")
        be.check(lib.ns2vc_dev_sync(), "sync")
    finally:
        lib.ns2vc_debug_set_gemm_tile(0, 0, 0)
    out = dict(a0=np.asarray(d_a.read(), np.float32).copy(), raw=None if d_r is None else np.asarray(d_r.read(), np.float32).copy(), out=d_o.read().copy(),
               a0_bits=d_a.read_bits(), raw_bits=None if d_r is None else d_r.read_bits(),
               viol=[v for b_ in bufs for v in b_.violations()])
    for b_ in bufs:
        b_.free()
    return out


def run_c5(src, prec, tile, conv_bn, diag, label):
    """-> (violations, figures) of the masked prologue on one conv instance"""
    d = _c5_inputs(src, prec)
    B, T, N, lens = C5_B, C5_T, C5_N, C5_LENS
    Cn = src[0] + src[1]
    valid = R.valid_mask(B, T, lens)
    tol_rows, tol_raw = tol_gnp_rows(prec)
    bad, fig = [], dict(rows=0.0, rows_item=0.0, raw=0.0, out=0.0, alone_ulp=0, alone_bitwise=True)
    wts = Weights(dict(W=d["W"], prec=prec, case=None), tiled=False)
    try:
        for temb_on in (1, 0):
            for silu in (1, 0):
                tag = f"temb={temb_on} silu={silu}"
                diag(f"{label} {tag}: launch")
                forms = {"algo2": c5_launch(d, wts, prec, tile, conv_bn, 2, False, temb_on, silu),
                         "algo0": c5_launch(d, wts, prec, tile, conv_bn, 0, False, temb_on, silu),
                         "coop": c5_launch(d, wts, prec, tile, conv_bn, 2, True, temb_on, silu)}
                o = forms["algo2"]
                for fname, f in forms.items():
                    if f["viol"]:
                        bad.append(f"{tag} {fname}: guard bands: " + "; ".join(f["viol"][:3]))
                    for k in ("a0", "raw", "out"):
                        if o[k] is not None and not np.array_equal(R._bits(f[k]), R._bits(o[k])):
                            bad.append(f"{tag} {fname}: {k} has other bits than algo 2 ({int((R._bits(f[k]) != R._bits(o[k])).sum())} elements)")
                ref = _c5_rows(d, temb_on, silu)
                for k, v in (("a0", o["a0"]), ("raw", o["raw"]), ("out", o["out"])):
                    if v is None:
                        continue
                    if not np.isfinite(v).all():
                        bad.append(f"{tag}: {k} not finite")
                    if (R._bits(v)[~valid] != 0).any():
                        bad.append(f"{tag}: {k} rows past an item's end not +0.0 ({int((R._bits(v)[~valid] != 0).sum())} elements)")
                a0 = np.nan_to_num(o["a0"].astype(np.float64)).reshape(B, T, Cn)
                e = rel_l2(a0, ref)
                e_item = max(rel_l2(a0[b, :L], ref[b, :L]) for b, L in enumerate(lens))
                fig["rows"], fig["rows_item"] = max(fig["rows"], e), max(fig["rows_item"], e_item)
                if not (e < tol_rows and e_item < tol_rows):
                    bad.append(f"{tag}: operand rows vs fp64: rel_l2 {e:.3e}, worst item {e_item:.3e} >= {tol_rows:.1e}")
                if o["raw"] is not None:
                    xm = d["x"].astype(np.float64) * valid.reshape(B, T, 1)
                    fig["raw"] = max(fig["raw"], rel_l2(np.nan_to_num(o["raw"].astype(np.float64)).reshape(B, T, Cn), xm))
                    if not fig["raw"] < tol_raw:
                        bad.append(f"{tag}: raw copy vs x: rel_l2 {fig['raw']:.3e} >= {tol_raw:.1e}")
                # the product on the device's own operand rows
                y = gather_rows(a0, B, T, T, 3, 0).reshape(B * T, 3 * Cn) @ d["W"].astype(np.float64).T + d["bias"].astype(np.float64)
                e_out = rel_l2(np.nan_to_num(o["out"].astype(np.float64)), y * valid[:, None])
                fig["out"] = max(fig["out"], e_out)
                if not e_out < TOL[prec]:
                    bad.append(f"{tag}: out_f32 vs fp64: rel_l2 {e_out:.3e} >= {TOL[prec]:.1e}")
                # an item with L_b >= 66: the dense prologue launched for it alone writes the same bits
                for b, L in enumerate(lens):
                    if L < 66:
                        continue
                    alone = c5_launch(d, wts, prec, tile, conv_bn, 2, False, temb_on, silu, item=b)
                    if alone["viol"]:
                        bad.append(f"{tag} item {b} alone: guard bands: " + "; ".join(alone["viol"][:3]))
                    for k in ("a0_bits", "raw_bits"):
                        if o[k] is None:
                            continue
                        got, want = o[k].reshape(B, T, Cn)[b, :L].astype(np.int64), alone[k].astype(np.int64)
                        if not np.array_equal(got, want):
                            # ulp distance in the operand type (sign-magnitude words -> a monotone integer line)
                            sb = 1 << (31 if prec == 0 else 15)
                            line = lambda w: np.where(w & sb, -(w & (sb - 1)), w & (sb - 1))
                            ulp = int(np.abs(line(got) - line(want)).max())
                            fig["alone_ulp"], fig["alone_bitwise"] = max(fig["alone_ulp"], ulp), False
                            bad.append(f"{tag}: {k[:-5]} rows of item {b} (L = {L}) differ from the item-alone dense prologue: "
                                       f"{int((got != want).sum())} elements, largest distance {ulp} ulp")
    finally:
        wts.free()
    diag(f"{label}: operand rows {fig['rows']:.2e} (worst item {fig['rows_item']:.2e}) raw {fig['raw']:.2e} result {fig['out']:.2e} "
         f"alone_bitwise {fig['alone_bitwise']} (largest {fig['alone_ulp']} ulp)" + (" ok" if not bad else " FAIL " + " | ".join(bad[:6])))
    return bad, fig


@pytest.mark.parametrize("prec", PRECS, ids=PREC_IDS)
@pytest.mark.parametrize("name", list(INSTANCES), ids=list(INSTANCES))
def test_epilogue_matrix(name, prec, diag):
    """GEGLU under lengths against its dense twin: held to TOL; whether it was bitwise is in the diag line (`geglu_bitwise`): on an MI355X it was, in
    every instance and precision.  Worst figures measured there (45 parameters): out_f32 against fp64 2.3e-07 rel-L2 in all three precisions (operands
    pre-rounded), the out_op-only launch 1.67e-03 bf16 / 2.07e-04 fp16 (bound TOL + eps16); statistics 7.7e-08 (sums) and 1.8e-07 (squares) of the largest
    entry; per item at most 0.04 of its bound."""
    inst = INSTANCES[name]
    tile, conv_bn, tol = inst["tile"], inst.get("conv_bn", 0), TOL[prec]
    ran, fails = set(), []
    worst = dict(rel_l2=0.0, stats_sum=0.0, stats_sumsq=0.0, stats_item=0.0)
    geglu_bitwise = []

    def note(fig):
        worst["rel_l2"] = max(worst["rel_l2"], fig.get("rel_l2", fig.get("rel_l2_op", 0.0)))
        worst["stats_sum"], worst["stats_sumsq"] = max(worst["stats_sum"], fig.get("stats_sum", 0.0)), max(worst["stats_sumsq"], fig.get("stats_sumsq", 0.0))
        worst["stats_item"] = max(worst["stats_item"], fig.get("stats_sum_item", 0.0), fig.get("stats_sumsq_item", 0.0))

    for case in (R.MASKED_CASES if inst["masked"] else []):
        if not _applies(case, name):
            continue
        geom = _geom(inst, name, case)
        vectors = R.lens_vectors(case, R.geometry(case["kern"]))
        B, T = case["B"], case["Tout"]
        if "residue" in vectors:                        # the coverage the shapes were chosen for, computed from (B, T, lens)
            g0 = R.geometry(case["kern"])
            assert R.rows_hit(B, T, vectors["residue"], g0["tile_rows"], g0["pad"]) >= set(g0["residues"]), case["name"]
            assert R.second_item_length_matters(B, T, vectors["residue"], geom), case["name"]
        else:
            assert R.items_per_span(B, T, _G64) >= 3
        wts = Weights(_inputs(case, prec, "full", vectors["full"], "nan"), tiled=case["kern"] == "conv")
        try:
            for vec, lens in vectors.items():
                fill = "inf" if vec == "ones" else "nan"
                inp = _inputs(case, prec, vec, lens, fill)
                diag(f"epilogue matrix {name} {PREC_IDS[prec]} {case['name']} [{vec}]: launch")
                out = launch(inp, wts, tile, conv_bn, True, fill=fill)
                dense = launch(inp, wts, tile, conv_bn, False, fill=fill)
                other = None
                if vec in ("residue", "mixed"):
                    inp2 = _inputs(case, prec, vec + "+1", R.perturbed(lens, T), fill)
                    other = (inp2, launch(inp2, wts, tile, conv_bn, True, fill=fill))
                fig = {}
                bad = R.check_launch(inp, out, dense, tol=tol, geom=geom, other=other, figures=fig)
                note(fig)
                if case["geglu"]:
                    geglu_bitwise.append(all(v for k, v in fig.items() if k.startswith("bitwise")))
                if case["kern"] == "conv" and vec == "residue":
                    # C4: the tile-major weights give the same bits; forced 4-loader / K-split tiles run the 8-loader plain masked form
                    if not _same_bits(out, launch(inp, wts, tile, conv_bn, True, tiled=True, fill=fill)):
                        bad.append("C4 w_tiled: other bits than the row-major weights")
                    bn = conv_bn or (tile[1] if tile[0] else 0)
                    for alias in (TS_ALIASES.get(bn, []) if case["name"] == "C1_conv_n128" else []):
                        if not _same_bits(out, launch(inp, wts, alias, 0, True, fill=fill)):
                            bad.append(f"forced conv tile {alias} under lens: other bits than the 8-loader plain masked form")
                diag(f"epilogue matrix {name} {PREC_IDS[prec]} {case['name']} [{vec}] lens={lens.tolist()}: "
                     + " ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items()) + (" ok" if not bad else " FAIL " + " | ".join(bad)))
                fails += [f"{case['name']} [{vec}]: {b}" for b in bad]
        finally:
            wts.free()
        ran.add(case["name"])
    c5_bitwise = []
    if inst["masked"] and "conv" in inst["kinds"]:
        for cname, src in C5_SOURCES.items():
            bad, fig = run_c5(src, prec, tile, conv_bn, diag, f"epilogue matrix {name} {PREC_IDS[prec]} {cname}")
            c5_bitwise.append(fig["alone_bitwise"])
            fails += [f"{cname}: {b}" for b in bad]
            ran.add(cname)
    for case in R.DENSE_CASES:
        if case["kern"] not in inst["kinds"]:
            continue
        geom = inst["geom"][case["kern"]]
        inp = _inputs(case, prec, "dense", None, "nan")
        wts = Weights(inp, tiled=False)
        try:
            diag(f"epilogue matrix {name} {PREC_IDS[prec]} {case['name']} [dense]: launch")
            out = launch(inp, wts, tile, conv_bn, False)
        finally:
            wts.free()
        fig = {}
        bad = R.check_launch(inp, out, None, tol=tol, geom=geom, figures=fig)
        note(fig)
        diag(f"epilogue matrix {name} {PREC_IDS[prec]} {case['name']} [dense]: " + " ".join(f"{k} {v:.2e}" for k, v in fig.items()) + (" ok" if not bad else " FAIL " + " | ".join(bad)))
        fails += [f"{case['name']} [dense]: {b}" for b in bad]
        ran.add(case["name"])
    diag(f"epilogue matrix {name} {PREC_IDS[prec]}: {len(ran)} cases, worst rel_l2 {worst['rel_l2']:.2e}, stats sum {worst['stats_sum']:.2e} sumsq {worst['stats_sumsq']:.2e}, "
         f"per-item stats error / bound {worst['stats_item']:.2f}, geglu_bitwise {all(geglu_bitwise) if geglu_bitwise else '-'}, prologue_alone_bitwise {all(c5_bitwise) if c5_bitwise else '-'}, {len(fails)} violations")
    assert ran >= EXPECTED_CASES[name], (name, sorted(EXPECTED_CASES[name] - ran))
    assert not fails, fails[:12]
