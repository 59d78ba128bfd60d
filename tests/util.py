"""numpy references and helpers shared by the tests (test-side code, not product)."""
from __future__ import annotations

import numpy as np


def rel_l2(a, b) -> float:
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def local_errors(y, r) -> dict:
    """Localized error figures of a (B, C, T) result `y` against its reference `r` (float64).  One whole-tensor rel_l2 dilutes an
    error confined to one frame or one channel by sqrt(B T) or sqrt(B C); these do not:
      frame       max over (b, t) of |y[b,:,t] - r[b,:,t]| / rms_b, rms_b = |r[b]| / sqrt(T)  (the item's RMS frame norm: quiet frames do not inflate it)
      chan        max over (b, c) of |y[b,c,:] - r[b,c,:]| / (|r[b]| / sqrt(C))
      item        max over b of rel_l2(y[b], r[b])
      frame_ratio worst frame error / median frame error (spread-out rounding noise: ~1 + a few / sqrt(C); a local defect: large)"""
    y = np.asarray(y, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    assert y.shape == r.shape and y.ndim == 3, (y.shape, r.shape)
    _, C, T = r.shape
    d = y - r
    nr = np.maximum(np.sqrt((r * r).sum(axis=(1, 2))), 1e-30)                 # |r[b]|
    fe = np.sqrt((d * d).sum(axis=1)) / (nr / np.sqrt(T))[:, None]            # (B, T)
    ce = np.sqrt((d * d).sum(axis=2)) / (nr / np.sqrt(C))[:, None]            # (B, C)
    item = np.sqrt((d * d).sum(axis=(1, 2))) / nr
    med = float(np.median(fe))
    return {"frame": float(fe.max()), "chan": float(ce.max()), "item": float(item.max()),
            "frame_ratio": float(fe.max() / med) if med > 0 else (0.0 if fe.max() == 0 else float("inf"))}


def fmt_local(m: dict) -> str:
    return " ".join(f"{k} {m[k]:.3e}" if k != "frame_ratio" else f"{k} {m[k]:.2f}" for k in ("frame", "chan", "item", "frame_ratio"))


def bf16_round(a: np.ndarray) -> np.ndarray:
    """round-to-nearest-even to bfloat16, returned as float32"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(a.shape)


def f16_round(a: np.ndarray) -> np.ndarray:
    """round-to-nearest-even to IEEE binary16 (overflow -> inf), returned as float32"""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


# ---- bounds shared by the kernel tests (tests/test_kernels_gpu.py, test_solvers_gpu.py, test_stochastic_gpu.py) and the guard-band tests
# (tests/test_kernel_bounds_gpu.py): one definition, so the strided launches are held to exactly what the tight ones are
def eps16(prec):
    """unit roundoff of the operand type (round to nearest): 2^-9 bf16, 2^-12 fp16"""
    return {0: 2.0 ** -25, 1: 2.0 ** -9, 2: 2.0 ** -12}[prec]


TOL_STATS = 1e-5            # epilogue statistics (int64 fixed point / per-slice row sums) vs fp64 sums of the result, relative to the largest
TOL_ATTN_FP8 = 4e-2         # pv_fp8 attention vs exact fp64 attention
GEGLU_FLIPS = 0.03          # token-stationary GEGLU: fraction of results one operand ulp off the rounded reference
TOL_ROWCHAIN_Y = 1e-6       # rowchain y: fp32 accumulation of exactly rounded operands
TOL_ROWCHAIN_GN_Y = 2e-5    # ... with the GroupNorm prologue (rows from the int64 sums)
TOL_FFN = 2e-4              # fused feed-forward vs fp64 with the kernel's rounding points
NOISE_ULP = 8               # ns2vc_k_noise vs ns2vc_amd.noise.gauss, ulps of max(|z|, 1)
TOL_SOLVER = 1e-6           # ns2vc_k_solver_update vs the fp64 recurrence


def tol_attention(prec):    # 16-bit: scaled Q, P and the output are rounded to the operand type
    return 2e-5 if prec == 0 else 8 * eps16(prec)


# ---- the position patterns of tests/attn_patterns.py (tests/test_attn_positions_*.py).  Derived, not tuned.
def tol_attn_count(prec, n):
    """COUNT: |out * n - 1| of a valid seam key among n equally weighted keys.  Every probability is the same power of two and V is 0 / 1, so the
    numerator is exact and the denominator is n times that power: what is left is one reciprocal, one product and one rounding to the operand type
    (2 eps16 covers the three for the 16-bit types; for fp32 eps16 is 2^-25), plus n * 2^-23 for an fp32 accumulation of n equal addends should
    v_exp_f32 not return an exact power of two.  A key counted twice reads 2n / (n + 1), a dropped one 0; excluded positions must be exactly 0."""
    return 2 * eps16(prec) + n * 2.0 ** -23


def tol_attn_route(prec, pv_fp8=False, n=0):
    """ROUTE: |out - ref64| per element (values in [0, 1]) against the fp64 attention of the same rounded operands, n keys.  16-bit: P, the
    denominator's P and the result are rounded to the operand type, and the rounded scaled Q moves the weight of the non-matching keys (a few 1e-3 of
    the row at the smallest gap) by a fraction of itself: 4 eps16.  fp8 PV form: one e4m3 rounding of P (2^-4 relative), mass at most 1.
    fp32 (eps16 = 2^-25, so 4 eps16 is one ulp of 1): the rounding that bound leaves out is the fp32 ACCUMULATION of numerator and denominator.  Once
    the match (p = 1 after the reference moved, or p = 2^gap on an unmoved reference when the gap is under THRESH) is in the accumulator, every later
    addend -- 2^-gap or 1 for a seam key, 2^-6 of that for a background key -- is rounded to the accumulator's ulp as it is added: up to 2^-24 relative
    per addition, n additions each for numerator and denominator, n 2^-23 in all -- the term tol_attn_count carries for the same reason.  The
    background addends are all equal, so they round the same way and the drift grows with n, not sqrt(n).  Measured: 5.4e-7 at n = 65 (gap 11.5) and
    9.5e-6 at n = 469 (gap 12.5), where 4 eps16 is 1.2e-7 and the bound with the term 7.9e-6 and 5.6e-5.  The 16-bit forms accumulate in fp32 too;
    there the term (5.6e-5 at n = 469) is a few percent of 4 eps16 and is NOT added: they are held to 4 eps16 alone."""
    if pv_fp8:
        return 2.0 ** -4
    return 4 * eps16(prec) + (n * 2.0 ** -23 if prec == 0 else 0.0)


TOL_FFN_XATTN_ROW = {1: 5e-3, 2: 6e-4}      # fused feed-forward with the in-kernel cross-attention vs the two-launch path: the bound of
#                                             test_ffn_fused_with_cross_attention, applied per row (max |fused - two-launch| over the row's RMS)


def tol_ln_linear(prec):    # LayerNorm-by-linearity consumer (16-bit: the raw operand copy is rounded BEFORE normalisation)
    return 2e-5 if prec == 0 else 8 * eps16(prec)


def tol_groupnorm(prec):    # (normalised rows, raw copy)
    return (5e-6 if prec == 0 else 2 * eps16(prec)), (1e-7 if prec == 0 else 2 * eps16(prec))


def tol_gnp_rows(prec):     # GroupNorm-prologue rows of a GEMM: (normalised rows, raw copy)
    return (1e-6 if prec == 0 else eps16(prec)), (1e-7 if prec == 0 else eps16(prec))


def tol_pair_rows(prec):    # hi + lo operand pair vs the fp64 rows
    return 2e-5 if prec == 1 else 1e-6


def tol_layernorm_apply(prec):
    return 2e-6 if prec == 0 else 2 * eps16(prec)


def tol_ffn_xattn(prec):    # fused feed-forward with the in-kernel cross-attention vs fp64
    return 4e-4 if prec == 2 else 3e-3


def synthetic_x0(x, t, cond=None):
    """the closed-form stand-in denoisers of the golden generators (float32): make_golden_v4.py / v5 (cond None) and make_golden_v7.py / v8, which
    keep their own torch copies"""
    f = np.float32
    tt = np.asarray(t, f).reshape(-1, 1, 1)
    xx = x.astype(f) if cond is None else (x.astype(f) + cond.astype(f)).astype(f)
    return (f(0.9) * np.tanh(xx) + f(0.05) * np.cos(f(0.01) * tt)).astype(f)


def silu(x):
    return x / (1.0 + np.exp(-x))


def gelu_erf(x):
    from math import erf
    return 0.5 * x * (1.0 + np.vectorize(erf)(x / np.sqrt(2.0)))


def gather_rows(a: np.ndarray, B: int, Tin: int, Tout: int, taps: int, tmode: int) -> np.ndarray:
    """a: [B, Tin, C] -> [B, Tout, taps, C] with the conv's zero padding / stride / nearest-upsample indexing."""
    C = a.shape[-1]
    out = np.zeros((B, Tout, taps, C), dtype=a.dtype)
    for t in range(Tout):
        for tap in range(taps):
            if tmode == 0:
                tt = t + tap - taps // 2
                ok = 0 <= tt < Tin
            elif tmode == 1:
                tt = 2 * t + tap - 1
                ok = 0 <= tt < Tin
            else:
                u = t + tap - 1
                ok = 0 <= u < Tout
                tt = min(u >> 1, Tin - 1)
            if ok:
                out[:, t, tap, :] = a[:, tt, :]
    return out


# ---- shared with tests/golden/make_golden_v2.py (the generator and the tests must build identical data) ----
def g7_summary(y: np.ndarray) -> dict:
    """what is stored of a (1, 100, 2813) output instead of its 1.1 MB"""
    T = y.shape[-1]
    mid = (T // 2) // 64 * 64
    return {"head": y[:, :, :256].copy(), "mid": y[:, :, mid:mid + 256].copy(), "tail": y[:, :, T - 256:].copy(), "mid_start": np.array([mid]),
            "chan_sum": y.astype(np.float64).sum(-1), "chan_sq": (y.astype(np.float64) ** 2).sum(-1),
            "frame_sum": y.astype(np.float64).sum(1), "frame_sq": (y.astype(np.float64) ** 2).sum(1)}


def tte_state(prefix: str, dim: int, out_dim: int) -> dict:
    """procedural parameters of a TextTimeEmbedding(dim, out_dim, heads), reference parameter names (torch tensors)"""
    import torch
    from ns2vc_amd.weights import hash_normal
    s = dim ** -0.5
    sd = {"norm1.weight": 1.0 + 0.1 * hash_normal(prefix + "n1w", (dim,)), "norm1.bias": 0.1 * hash_normal(prefix + "n1b", (dim,)),
          "pool.positional_embedding": s * hash_normal(prefix + "pos", (1, dim)),
          "proj.weight": s * hash_normal(prefix + "pw", (out_dim, dim)), "proj.bias": 0.1 * hash_normal(prefix + "pb", (out_dim,)),
          "norm2.weight": 1.0 + 0.1 * hash_normal(prefix + "n2w", (out_dim,)), "norm2.bias": 0.1 * hash_normal(prefix + "n2b", (out_dim,))}
    for p in ("k_proj", "q_proj", "v_proj"):
        sd[f"pool.{p}.weight"] = s * hash_normal(prefix + p + "w", (dim, dim))
        sd[f"pool.{p}.bias"] = 0.1 * hash_normal(prefix + p + "b", (dim,))
    return {k: torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)) for k, v in sd.items()}


def procedural_params(shapes, tag: str) -> dict:
    """deterministic parameters for a {name: shape} list (torch tensors): matrices ~ N(0, 1/fan_in), norm weights ~ 1,
    biases / vectors ~ 0.1 N(0, 1); the same integer-hash generator as the denoiser's procedural weights"""
    import torch
    from ns2vc_amd.weights import hash_normal
    out = {}
    for name, shape in shapes:
        shape = tuple(shape)
        v = hash_normal(f"{tag}.{name}", shape)
        if len(shape) >= 2:
            fan_in = int(np.prod(shape[1:])) if "conv.weight" not in name else shape[0] * shape[1]
            v = v / np.sqrt(max(fan_in, 1))
        elif "norm" in name and name.endswith("weight"):
            v = 1.0 + 0.1 * v
        else:
            v = 0.1 * v
        out[name] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return out
