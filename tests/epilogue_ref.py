"""Float64 statement of the ns2vc_k_gemm contract (include/ns2vc_hip.h, ns2vc_gemm_args) with per-item valid lengths, the launch table of
tests/test_epilogue_matrix_gpu.py, the `lens` vectors that put an item's end on every tile row that matters, and ONE checker, check_launch,
which the GPU test calls on device results and tests/test_epilogue_ref_cpu.py calls on numpy "kernels" that carry one defect each.
Test-side code (numpy only), a plain module like util.py / guard.py.

The contract (the header's words): an output row (b, t) with t >= lens[b] is exact zeros in out_f32 and out_op -- bias and residual not added,
whatever the accumulator, the residual row or the operand rows behind it hold -- and adds nothing to `stats`; every other row is what the dense
launch gives on the same inputs.  ("As if the item ran alone" is the ENGINE's contract, held by tests/test_ragged_fused_gpu.py.)

Bounds: none of its own.  `tol` is TOL[prec] of tests/test_kernels_gpu.py (handed in by the caller), TOL_STATS is util's, the fixed-point quanta
follow from the header's scales (sum * 2^28, sum of squares * 2^16: one llrint per wave commit is off by at most half a unit, 2^-29 / 2^-17; the
commits that can touch an item are counted from M, T and the row tiling, see geometry), and an
operand-typed result without an fp32 twin is allowed the unit roundoff of its type on top of `tol` (|rnd(y) - r| <= |y - r| + eps |y|)."""
from __future__ import annotations

import zlib

import numpy as np

from util import TOL_STATS, bf16_round, eps16, f16_round, gather_rows, gelu_erf, rel_l2

SUM_SCALE, SQ_SCALE = 2.0 ** 28, 2.0 ** 16
HALF_Q = (2.0 ** -29, 2.0 ** -17)          # half a fixed-point unit of (sum, sum of squares)

# an item's end (its LAST valid row) must land on each of these rows of a row tile
GEMM_TILE_ROWS, GEMM_RESIDUES = 128, (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 127)
CONV_TILE_ROWS, CONV_RESIDUES = 126, (0, 1, 15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 125)      # (padded row space: item b starts at b * (T + 1))


def rnd(a, prec):
    a = np.asarray(a, dtype=np.float32)
    return bf16_round(a) if prec == 1 else (f16_round(a) if prec == 2 else a)


def _gelu(x):
    try:
        from scipy.special import erf
        return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))
    except ImportError:
        return gelu_erf(x)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the launches.  kern: "gemm" = the 8-wave GEMM kernel (and the 4-wave one for the dense-only rows), "conv" = the tap-sharing conv kernel.
# res: None | "sep" | "alias" (the residual IS out_f32).  out: "both" | "f32" | "op".  slice: a0 is a column slice of wider rows.
# ---------------------------------------------------------------------------------------------------------------------------------------
def _case(name, kern, B, Tin, Tout, c0, N, taps=1, tmode=0, c1=0, c2=0, bias=1, res=None, out="both", geglu=0, stats=0, algo=0, slice_=0, vectors=None):
    return dict(name=name, kern=kern, B=B, Tin=Tin, Tout=Tout, c0=c0, c1=c1, c2=c2, N=N, taps=taps, tmode=tmode, bias=bias, res=res, out=out,
                geglu=geglu, stats=stats, algo=algo, slice=slice_, vectors=vectors)


G8_LENS = {24: [24, 1, 7, 24, 13, 1, 24, 2, 19], 19: [19, 1, 5, 19, 12, 3, 1, 19, 8]}      # 64 rows hold three (T = 24) or four (T = 19) items with different ends

MASKED_CASES = [
    _case("G1_linear_res_dual_stats", "gemm", 15, 97, 97, 128, 128, res="sep", stats=1),
    _case("G2_linear_alias_f32only_stats", "gemm", 16, 81, 81, 128, 128, res="alias", out="f32", stats=1),
    _case("G3_linear_op_only", "gemm", 16, 74, 74, 64, 128, out="op"),
    _case("G4_conv3_8wave_concat_seg_slice_stats", "gemm", 15, 97, 97, 64, 128, taps=3, c1=64, c2=64, res="sep", stats=1, algo=1, slice_=1),
    _case("G5_stride2_odd_stats", "gemm", 16, 161, 81, 64, 128, taps=3, tmode=1, out="f32", stats=1),
    _case("G5_stride2_even_stats", "gemm", 16, 148, 74, 64, 128, taps=3, tmode=1, out="f32", stats=1),
    _case("G6_up2_odd_stats", "gemm", 16, 41, 81, 64, 128, taps=3, tmode=2, out="f32", stats=1),
    _case("G6_up2_even_stats", "gemm", 16, 37, 74, 64, 128, taps=3, tmode=2, out="f32", stats=1),
    _case("G7_geglu_n256", "gemm", 16, 74, 74, 64, 256, res="sep", geglu=1),
    _case("G7_geglu_n2048", "gemm", 16, 74, 74, 64, 2048, res="sep", geglu=1),
    _case("G8_short_linear_T24", "gemm", 9, 24, 24, 64, 128, res="sep", vectors="short"),
    _case("G8_short_linear_T19", "gemm", 9, 19, 19, 64, 128, res="sep", vectors="short"),
    _case("G8_short_conv3_T24", "gemm", 9, 24, 24, 64, 128, taps=3, res="sep", vectors="short"),
    _case("G8_short_conv3_T19", "gemm", 9, 19, 19, 64, 128, taps=3, res="sep", vectors="short"),
    _case("C1_conv_n128", "conv", 14, 131, 131, 64, 128, taps=3, res="sep", stats=1),
    _case("C1_conv_n256", "conv", 16, 97, 97, 64, 256, taps=3, res="sep", stats=1),
    _case("C2_conv_concat_seg_alias_stats", "conv", 16, 97, 97, 64, 128, taps=3, c1=64, c2=64, res="alias", out="f32", stats=1, slice_=1),
    _case("C3_conv_n64", "conv", 14, 131, 131, 64, 64, taps=3, res="sep", stats=1),
    _case("C3_conv_n192", "conv", 16, 97, 97, 64, 192, taps=3, res="sep", stats=1),
]
# dense-only rows: statistics on a stride-2 / nearest-up launch, and at the smallest Tout the launcher takes them at (64; the tap-sharing kernel
# itself starts at T = 66), B = 5: item starts exactly on a wave's first row, on its last row and one past it
DENSE_CASES = [
    _case("D_stride2_stats", "gemm", 3, 133, 67, 64, 128, taps=3, tmode=1, out="f32", stats=1),
    _case("D_up2_stats", "gemm", 3, 34, 67, 64, 128, taps=3, tmode=2, out="f32", stats=1),
    _case("D_linear_T64_stats", "gemm", 5, 64, 64, 64, 128, res="sep", stats=1),
    _case("D_linear_T65_stats", "gemm", 5, 65, 65, 64, 128, res="sep", stats=1),
    _case("D_conv3_T64_stats", "gemm", 5, 64, 64, 64, 128, taps=3, out="f32", stats=1),
    _case("D_conv3_T65_stats", "gemm", 5, 65, 65, 64, 128, taps=3, out="f32", stats=1),
    _case("D_conv_T66_stats", "conv", 5, 66, 66, 64, 128, taps=3, out="f32", stats=1),
    _case("D_conv_T67_stats", "conv", 5, 67, 67, 64, 128, taps=3, out="f32", stats=1),
]


def geometry(kern, tile_rows=None, wave_rows=32, commits=2):
    """row tiling of a kernel instance: tile rows, rows of one wave tile (the span whose rows choose between items b0 and b0 + 1), statistics commits
    per wave tile, pad rows between items (the conv kernel's padded row space).  commits: in the 8-wave GEMM kernel and in the tap-sharing kernel the
    eight epilogue waves each move 16 rows of every 32-row slab out, so a wave tile's rows are committed by TWO waves (kg = 0, 1), each with its own
    llrint; the 4-wave kernel commits once per wave tile (commits = 1)."""
    if kern == "conv":
        return dict(tile_rows=CONV_TILE_ROWS, wave_rows=wave_rows, pad=1, panel=128, residues=CONV_RESIDUES, commits=commits)
    return dict(tile_rows=tile_rows or GEMM_TILE_ROWS, wave_rows=wave_rows, pad=0, panel=tile_rows or GEMM_TILE_ROWS, residues=GEMM_RESIDUES, commits=commits)


# ---------------------------------------------------------------------------------------------------------------------------------------
# lens vectors
# ---------------------------------------------------------------------------------------------------------------------------------------
def rows_hit(B, T, lens, tile_rows, pad):
    """tile rows on which an item's last valid row lands"""
    return {(b * (T + pad) + int(L) - 1) % tile_rows for b, L in zip(range(B), lens)}


def wave_spans(B, T, geom):
    """[lo, hi) row ranges (padded row space for the conv kernel) of the wave commits of a launch"""
    rows = B * (T + geom["pad"])
    out = []
    for t0 in range(0, rows, geom["tile_rows"]):
        for w0 in range(0, geom["panel"], geom["wave_rows"]):
            lo, hi = t0 + w0, min(t0 + w0 + geom["wave_rows"], t0 + geom["tile_rows"], rows)
            if lo < hi:
                out.append((lo, hi))
    return out


def second_item_length_matters(B, T, lens, geom):
    """a wave span that holds the start of item b + 1 behind rows of item b, where masking item b + 1's rows of the span with lens[b] instead of
    lens[b + 1] gives another result (an end of one of the two inside the span): where `first` / `second` / len0 / len1 decide between two items"""
    P = T + geom["pad"]
    for lo, hi in wave_spans(B, T, geom):
        for b in range(B - 1):
            s1 = (b + 1) * P
            if lo < s1 < hi and lens[b] != lens[b + 1] and min(int(lens[b]), int(lens[b + 1])) < min(hi - s1, T):
                return True
    return False


def items_per_span(B, T, geom):
    """the largest number of items one wave span holds rows of"""
    P = T + geom["pad"]
    return max((hi - 1) // P - lo // P + 1 for lo, hi in wave_spans(B, T, geom))


def perturbed(lens, T):
    """the same lengths with ONE item (a middle one) changed: for check 7"""
    out = np.array(lens, np.int32)
    j = len(out) // 2
    out[j] = T if out[j] <= T // 2 else max(1, int(out[j]) // 3)
    return out


def residue_lens(B, T, geom):
    """one length per item so that the items' last valid rows cover geom['residues'] (bipartite matching items x residues), the spare items
    short ones placed inside a wave span behind a longer item.  Raises if the set cannot be covered with B items."""
    tile, pad, need = geom["tile_rows"], geom["pad"], list(geom["residues"])
    P = T + pad
    opts = {r: [b for b in range(B) if ((r - b * P) % tile) + 1 <= T] for r in need}          # L = ((r - b P) mod tile) + 1, the smallest that hits r
    owner = {}                                                                                # item -> residue

    def assign(r, seen):
        for b in opts[r]:
            if b in seen:
                continue
            seen.add(b)
            if b not in owner or assign(owner[b], seen):
                owner[b] = r
                return True
        return False

    for r in sorted(need, key=lambda r_: len(opts[r_])):
        if not assign(r, set()):
            raise ValueError(f"residue {r} cannot be covered: B={B} T={T} tile={tile}")
    lens = np.full(B, T, dtype=np.int32)
    for b, r in owner.items():
        L = ((r - b * P) % tile) + 1
        while L + tile <= T and (b + L) % 3 == 0:            # (where two lengths hit the row, take the longer one for a third of the items)
            L += tile
        lens[b] = L
    for b in range(1, B):                                    # spare items: 2 valid rows, so that a wave span holds both ends of the item
        if b not in owner:
            lens[b] = 2
    return lens


def lens_vectors(case, geom):
    B, T = case["B"], case["Tout"]
    if case["vectors"] == "short":
        return {"full": np.full(B, T, np.int32), "ones": np.ones(B, np.int32), "mixed": np.array(G8_LENS[T], np.int32)}
    return {"full": np.full(B, T, np.int32), "ones": np.ones(B, np.int32), "residue": residue_lens(B, T, geom)}


def lens_in_of(case, lens):
    """valid INPUT rows per item: the lengths the producer of the operand rows was masked with"""
    lens = np.asarray(lens)
    if case["tmode"] == 1:
        lin = np.minimum(2 * lens - (np.arange(len(lens)) & 1), case["Tin"])                          # odd and even input lengths, ceil(Lin / 2) = L
        return np.where(lens == case["Tout"], case["Tin"], lin).astype(np.int32)                      # (a full item is the whole input)
    if case["tmode"] == 2:
        return ((lens + 1) // 2).astype(np.int32)
    return lens.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------------
# inputs and the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------------------
def _poison(a, B, T, lens, value):
    a = a.reshape(B, T, -1).copy()
    for b, L in enumerate(lens):
        a[b, int(L):] = value
    return a.reshape(B * T, -1)


def make_inputs(case, prec, lens=None, fill="nan"):
    """operands pre-rounded to the operand type.  Under `lens`: the residual's padded rows hold NaN / Inf; the operand rows past an item's end hold
    NaN / Inf for taps = 1 and zeros for k = 3 (the row invariant a producer keeps)."""
    rng = np.random.default_rng(zlib.crc32(case["name"].encode()))
    B, Tin, Tout, N = case["B"], case["Tin"], case["Tout"], case["N"]
    Ct, M = case["c0"] + case["c1"], B * Tout
    K = case["taps"] * Ct + case["c2"]
    inp = dict(case=case, prec=prec, lens=None if lens is None else np.asarray(lens, np.int32))
    inp["a0"] = rnd(rng.standard_normal((B * Tin, case["c0"])), prec)
    inp["a1"] = rnd(rng.standard_normal((B * Tin, case["c1"])), prec) if case["c1"] else None
    inp["a2"] = rnd(rng.standard_normal((B * Tin, case["c2"])), prec) if case["c2"] else None
    inp["W"] = rnd(rng.standard_normal((N, K)) / np.sqrt(K), prec)
    inp["bias"] = rng.standard_normal(N).astype(np.float32) if case["bias"] else None
    Nout = N // 2 if case["geglu"] else N
    inp["res"] = rng.standard_normal((M, Nout)).astype(np.float32) if case["res"] else None
    inp["Nout"] = Nout
    if lens is not None:
        bad = np.float32(np.nan if fill == "nan" else np.inf)
        lin = inp["lens_in"] = lens_in_of(case, lens)
        for k in ("a0", "a1", "a2"):
            if inp[k] is not None:
                inp[k] = _poison(inp[k], B, Tin, lin, bad if case["taps"] == 1 else 0.0)
        if inp["res"] is not None:
            inp["res"] = _poison(inp["res"], B, Tout, lens, bad)
    return inp


def valid_mask(B, T, lens):
    return (np.arange(T)[None, :] < np.asarray(lens)[:, None]).reshape(B * T)


def reference(inp):
    """fp64: {out: [M][Nout] (rows past an item's end zero), pre: the pre-epilogue rows (accumulator + bias, before GEGLU / residual) for the numpy kernels}"""
    case = inp["case"]
    B, Tin, Tout, N, taps, tmode = case["B"], case["Tin"], case["Tout"], case["N"], case["taps"], case["tmode"]
    Ct, M = case["c0"] + case["c1"], B * Tout
    lens = inp["lens"]

    def clean(a):                                            # rows past the input's end never reach a valid row of a k = 1 launch; k = 3: they are zeros already
        return a.astype(np.float64) if lens is None else _poison(a, B, Tin, inp["lens_in"], 0.0).astype(np.float64)

    A = clean(inp["a0"]) if inp["a1"] is None else np.concatenate([clean(inp["a0"]), clean(inp["a1"])], axis=1)
    W = inp["W"].astype(np.float64)
    acc = gather_rows(A.reshape(B, Tin, Ct), B, Tin, Tout, taps, tmode).reshape(M, taps * Ct) @ W[:, :taps * Ct].T
    if inp["a2"] is not None:
        acc = acc + clean(inp["a2"]) @ W[:, taps * Ct:].T
    pre = acc + inp["bias"].astype(np.float64) if inp["bias"] is not None else acc
    y = pre
    if case["geglu"]:
        r3 = pre.reshape(M, N // 64, 2, 32)                                                    # packed (32 value | 32 gate) column order
        y = (r3[:, :, 0, :] * _gelu(r3[:, :, 1, :])).reshape(M, N // 2)
    if inp["res"] is not None:
        res = inp["res"].astype(np.float64)
        y = y + (res if lens is None else _poison(res, B, Tout, lens, 0.0))
    if lens is not None:
        y = y * valid_mask(B, Tout, lens)[:, None]
    return dict(out=y, acc=acc)


def stats_of(y, B, T, lens=None):
    """fp64 (sum, sum of squares) per item and 16-channel block over the valid rows of y [B*T][N] -> [B][N/16][2]"""
    N = y.shape[1]
    v = y.astype(np.float64).reshape(B, T, N // 16, 16)
    if lens is not None:
        v = v * valid_mask(B, T, lens).reshape(B, T, 1, 1)
    return np.stack([v.sum(axis=(1, 3)), (v * v).sum(axis=(1, 3))], axis=-1)


def stats_fixed(y, B, T, lens=None):
    """the statistics as the header stores them: int64 (sum * 2^28, sum of squares * 2^16)"""
    s = stats_of(y, B, T, lens)
    return np.stack([np.rint(s[..., 0] * SUM_SCALE), np.rint(s[..., 1] * SQ_SCALE)], axis=-1).astype(np.int64)


def commits_per_item(B, T, lens, geom):
    """wave commits that can hold a valid row of item b: geom['commits'] per wave tile with such a row"""
    P = T + geom["pad"]
    spans = wave_spans(B, T, geom)
    return geom["commits"] * np.array([sum(1 for lo, hi in spans if lo < b * P + int(lens[b]) and hi > b * P) for b in range(B)])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _first_bad(mask, case, lens, geom):
    """(row, col) of the first set element + where that row sits: item, frame, tile row, tile row of the item's end"""
    idx = np.argwhere(mask)
    if not len(idx):
        return ""
    m, n = int(idx[0][0]), int(idx[0][1])
    T, P = case["Tout"], case["Tout"] + geom["pad"]
    b, t = divmod(m, T)
    s = f"{len(idx)} elements, first (row {m}, col {n}) = item {b} frame {t}, tile row {(b * P + t) % geom['tile_rows']}"
    if lens is not None:
        s += f", lens[{b}] = {int(lens[b])}, item end on tile row {(b * P + int(lens[b]) - 1) % geom['tile_rows']}"
    return s


def check_launch(inp, out, dense=None, *, tol, geom, tol_stats=TOL_STATS, other=None, figures=None):
    """inp: make_inputs(...).  out / dense: {out_f32, out_op: float32 [M][Nout] (decoded) or None; stats: int64 [B][N/16][2] or None; viol: guard violations}
    of the launch under inp['lens'] and of its dense twin (same instance, same inputs, lens = NULL; None for a dense-only row, where `out` IS the dense
    launch).  other = (inp2, out2): the same launch under lengths that differ from inp['lens'] in ONE item (check 7).
    Returns the list of violations (empty = the launch keeps the contract); `figures` (a dict) receives the measured errors."""
    case, prec, lens = inp["case"], inp["prec"], inp["lens"]
    B, T = case["B"], case["Tout"]
    fig = figures if figures is not None else {}
    bad = []
    if "_ref" not in inp:
        inp["_ref"] = reference(inp)
    ref = inp["_ref"]["out"]
    valid = np.ones(B * T, bool) if lens is None else valid_mask(B, T, lens)
    of, oo = out.get("out_f32"), out.get("out_op")
    # 8. guard bands
    if out.get("viol"):
        bad.append("8 guard bands: " + "; ".join(out["viol"][:4]))
    # 2. finite
    for name, v in (("out_f32", of), ("out_op", oo)):
        if v is not None and not np.isfinite(v).all():
            bad.append(f"2 {name} not finite: " + _first_bad(~np.isfinite(v), case, lens, geom))
    # 1. against fp64
    if of is not None:
        fig["rel_l2"] = e = rel_l2(np.nan_to_num(of.astype(np.float64), nan=1e30, posinf=1e30, neginf=-1e30), ref)
        if not e < tol:
            bad.append(f"1 out_f32 vs fp64: rel_l2 {e:.3e} >= {tol:.1e}: " + _first_bad(~(np.abs(of - ref) <= 1e-2 + 1e-2 * np.abs(ref)), case, lens, geom))
    elif oo is not None:
        fig["rel_l2_op"] = e = rel_l2(np.nan_to_num(oo.astype(np.float64), nan=1e30, posinf=1e30, neginf=-1e30), ref)
        lim = tol + (eps16(prec) if prec else 0.0)
        if not e < lim:
            bad.append(f"1 out_op vs fp64: rel_l2 {e:.3e} >= {lim:.1e}: " + _first_bad(~(np.abs(oo - ref) <= 2e-2 + 2e-2 * np.abs(ref)), case, lens, geom))
    # 3. rows past an item's end are zero BITS; out_op == rnd(out_f32) everywhere
    for name, v in (("out_f32", of), ("out_op", oo)):
        if v is not None and (_bits(v)[~valid] != 0).any():
            bad.append(f"3 {name} rows past an item's end not +0.0: " + _first_bad((_bits(v) != 0) & ~valid[:, None], case, lens, geom))
    if of is not None and oo is not None and not np.array_equal(_bits(oo), _bits(rnd(of, prec))):
        bad.append("3 out_op != rnd(out_f32): " + _first_bad(_bits(oo) != _bits(rnd(of, prec)), case, lens, geom))
    # 4. valid rows against the dense twin: bitwise where the epilogue only adds, tol under GEGLU
    if dense is not None:
        for name, v in (("out_f32", of), ("out_op", oo)):
            d = dense.get(name)
            if v is None or d is None:
                continue
            same = np.array_equal(_bits(v)[valid], _bits(d)[valid])
            fig[f"bitwise_{name}"] = same
            if case["geglu"]:
                e = rel_l2(v[valid], d[valid].astype(np.float64))
                if not e < tol:
                    bad.append(f"4 {name} valid rows vs the dense launch (GEGLU): rel_l2 {e:.3e} >= {tol:.1e}")
            elif not same:
                bad.append(f"4 {name} valid rows differ from the dense launch: " + _first_bad((_bits(v) != _bits(d)) & valid[:, None], case, lens, geom))
    # 5. statistics against fp64 sums of the device's own stored valid rows
    st = out.get("stats")
    if st is not None and of is not None:
        got = np.stack([st[..., 0] / SUM_SCALE, st[..., 1] / SQ_SCALE], axis=-1)
        want = stats_of(np.nan_to_num(of), B, T, lens)
        nc = commits_per_item(B, T, lens if lens is not None else np.full(B, T), geom)
        for k, mom in enumerate(("sum", "sumsq")):
            d = np.abs(got[..., k] - want[..., k])
            fig[f"stats_{mom}"] = e = float(d.max() / max(np.abs(want[..., k]).max(), 1e-30))
            if not e < tol_stats:
                bad.append(f"5 stats {mom}: {e:.2e} of the largest entry >= {tol_stats:.0e}")
            lim = tol_stats * np.abs(want[..., k]).max(axis=1) + nc * HALF_Q[k]                # per item: its own largest entry + half a unit per commit
            worst = d.max(axis=1)
            fig[f"stats_{mom}_item"] = float((worst / np.maximum(lim, 1e-300)).max())
            if (worst > lim).any():
                b = int(np.argmax(worst / np.maximum(lim, 1e-300)))
                L = T if lens is None else int(lens[b])
                bad.append(f"5 stats {mom} of item {b} (L = {L}, {nc[b]} commits): off by {worst[b]:.3e} > {lim[b]:.3e}, block {int(np.argmax(d[b]))}, "
                           f"item end on tile row {(b * (T + geom['pad']) + L - 1) % geom['tile_rows']}")
    # 6. full lengths: everything equals the dense launch bitwise, the statistics included (int64 adds commute)
    if dense is not None and lens is not None and (lens == T).all():
        for name in ("out_f32", "out_op"):
            if out.get(name) is not None and not np.array_equal(_bits(out[name]), _bits(dense[name])):
                bad.append(f"6 full lengths: {name} differs from the dense launch")
        if st is not None and not np.array_equal(st, dense["stats"]):
            bad.append(f"6 full lengths: stats differ from the dense launch in {int((st != dense['stats']).sum())} entries")
    # 7. another length for ONE item leaves every other item's rows and statistics as they were
    if other is not None:
        inp2, out2 = other
        js = np.flatnonzero(inp2["lens"] != lens)
        assert len(js) == 1, "check 7 takes lengths that differ in one item"
        keep = np.repeat(np.arange(B) != js[0], T)
        for name in ("out_f32", "out_op"):
            if out.get(name) is not None and not np.array_equal(_bits(out[name])[keep], _bits(out2[name])[keep]):
                bad.append(f"7 lens[{js[0]}] {int(lens[js[0]])} -> {int(inp2['lens'][js[0]])} changed {name} of another item: "
                           + _first_bad((_bits(out[name]) != _bits(out2[name])) & keep[:, None], case, lens, geom))
        if st is not None and not np.array_equal(np.delete(st, js[0], axis=0), np.delete(out2["stats"], js[0], axis=0)):
            bad.append(f"7 lens[{js[0]}] changed the statistics of another item")
    return bad
