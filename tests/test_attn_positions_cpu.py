"""The position patterns of tests/attn_patterns.py, checked on the CPU before any kernel sees them.

(1) The patterns are valid.  For every operand type, head width and gap that tests/test_attn_positions_gpu.py uses, the fp64 attention of the ROUNDED
operands (with P rounded to e4m3 for the fp8 PV form) decodes every ROUTE row to (its own seam key, its head, its item) with every element within
0.25 of its 0 / 1 code, the realised gap lies within 0.1 of the wanted one (0.25 at gap 40 in bf16), the other seam keys score exactly 0 and the
background about -6, and every COUNT element is within tol_attn_count.  At the shapes of passes (b) and (c) every live workgroup holds a row whose
match lies behind the first key tile.

(2) The decoders would catch a subtly wrong kernel.  Seven mutants are applied to the numpy reference (never to a kernel) at every shape of the GPU
file; each must be flagged by COUNT or ROUTE wherever it changes what an item reads (a dense launch has no padding key to admit, a launch without
a bias no bias row to shift, a one-key item no 64-key tile to lose a key from).

What the whole-tensor bounds make of the same mutants, on unit-normal data at B = 3, H = 5, hd = 16, Lq = 200: rel_l2 of the mutated fp64 attention
against the right one, (a) the mutant in every row (worst item), (b) the same mutant in ONE wave (32 rows) of one head of item 0 (that item's figure).
tol_attention is 1.6e-2 for bf16 and 2.0e-3 for fp16, TOL_ATTN_FP8 4e-2.  Shapes: q_lens [200, 129, 1] with k_lens [129, 200, 129] at Lk = 200, and
the bias prefixes [469, 256, 129] at Lk = 469.  Printed by test_whole_tensor_bounds_on_the_mutants; the data there are exact, a kernel's own rounding
(bf16: a few 1e-3) comes on top and takes its part of the bound.

    mutant                                      Lk 200 (a)   (b)       Lk 469 (a)   (b)       flagged at 1.6e-2: (a) / (b)     by COUNT or ROUTE
    tail_twice  last valid key counted twice     7.2e-2      2.0e-2     9.1e-2      7.8e-3     yes / 200: barely, 469: no        COUNT, every shape
    seam_drop   key 63 dropped                   1.0e-1      3.7e-2     6.7e-2      7.0e-3     yes / 200: yes, 469: no           both, every shape
    pad_admit   first padding key admitted       7.8e-2      1.4e-2     1.0e-1      (none)     yes / no                          both, every shape
    bias_shift  bias row shifted by one          --          --         1.0e-1      7.9e-3     yes / no                          both, every shape
    row_rotate  rows rotated inside a block      1.1         2.0e-1     1.2         2.0e-1     yes / yes                         ROUTE, every shape
    head_swap   heads 0 and 1 swapped            9.3e-1      2.7e-1     9.4e-1      2.6e-1     yes / yes                         ROUTE (COUNT at 16 of 30)
    item_next   item b reads item b + 1's keys   1.5         2.2e-1     1.5         2.5e-1     yes / yes                         ROUTE (COUNT at 16 of 30)

Read honestly: averaged unit-normal values make |out| about sqrt(e / n), so one key carries about 1 / sqrt(n) of a row's NORM, not 1 / n, and a miscount
in every row of a launch IS seen by the random-data tests at these sizes (4 - 6 times the bf16 bound, under twice the fp8 one).  What they let through
is the miscount that hits a part of the launch -- one wave, one head, one tile path: column (b) is at or below the bf16 bound at Lk = 200 and half of
it at Lk = 469, and nothing in a relative L2 says where it sits.  The patterns flag each of these by an integer per row, name the key, row, head and
item, and hold the weight of a key to 2 eps16 instead of a share of 8 eps16.  The three misroutings are gross on random data; they are here because
the bit-identity tests run the same code on both sides and would share them."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_patterns as P                           # noqa: E402
from util import rel_l2, tol_attention, tol_attn_count, tol_attn_route      # noqa: E402

PREC_IDS = {0: "fp32", 1: "bf16", 2: "fp16"}
GAPS_FP32 = (11.5, 12.5, 40.0)                      # THRESH -+ 0.5 of the exact pass; a key that dominates outright
GAPS_16 = (11.5, 12.5, 17.0, 19.0, 40.0)            # ... and the optimistic pass: p = 2^13 accepted, 2^15 rejected (limit 2^14, margin 4)
GAPS_FP8 = (7.5, 8.5, 40.0)                         # THRESH is 8 in the fp8 PV form
GAPS_FFN = (24.0, 40.0)                             # see test_attn_positions_gpu.py: the in-kernel cross-attention has no threshold to straddle


def gaps_of(prec, fp8):
    return GAPS_FP8 if fp8 else GAPS_FP32 if prec == 0 else GAPS_16


@functools.lru_cache(maxsize=None)
def _cases(masked, tile):
    return P.attn_cases(masked, tile)


def _validate(case, hd, prec, fp8, gaps, name):
    p_round = P.e4m3_round if fp8 else None
    # ---- COUNT
    q, k, v, sets = P.build_count(case, hd)
    qr, kr, vr = (P.round_op(t, prec) for t in (q, k, v))
    out = P.attend(qr, kr, vr, case, hd, p_round=p_round)
    worst, nonzero, bad, ratio = P.check_count(out, case, hd, sets, tol=lambda n: tol_attn_count(prec, n))
    assert nonzero == 0 and ratio <= 1.0, (name, worst, nonzero, bad)
    # ---- ROUTE
    for gap in gaps:
        q, k, v, sets, want = P.build_route(case, hd, gap, prec)
        qr, kr, vr = (P.round_op(t, prec) for t in (q, k, v))
        assert np.array_equal(vr, v) and set(np.unique(v)) <= {0.0, 1.0}
        out = P.attend(qr, kr, vr, case, hd, p_round=p_round)
        wrong, dev, bad = P.check_route(out, case, hd, want)
        assert wrong == 0 and dev < 0.25, (name, gap, wrong, dev, bad)
        lo, hi, other, back = P.realised_gaps(qr, kr, case, hd, sets)
        slack = 0.25 if (prec == 1 and gap > 20) else 0.1          # (bf16: three 2^-9 roundings of a product of amplitudes, times the gap)
        assert abs(lo - gap) <= slack and abs(hi - gap) <= slack, (name, gap, lo, hi)
        assert other in (0.0, -np.inf) and (back == -np.inf or abs(back + P.BACKGROUND) < 0.1), (name, gap, other, back)
    return worst


MATRIX = [(prec, hd, fp8) for prec in (0, 1, 2) for hd in (16, 32, 48, 64) for fp8 in ((0, 1) if prec else (0,))]


@pytest.mark.parametrize("prec,hd,fp8", MATRIX, ids=[f"{PREC_IDS[p]}-hd{h}{'-fp8' if f else ''}" for p, h, f in MATRIX])
def test_patterns_are_valid(prec, hd, fp8):
    """every shape at head width 16 (both key tiles); the other head widths change nothing but the amplitude and the zero dims behind the code, so they
    take the largest dense shape, the bias shape and one ragged launch"""
    tiles = (64, 128) if (prec and hd <= 32 and not fp8) else (64,)
    for tile in tiles:
        for masked in ((0,) if fp8 else (0, 1)):
            cs = _cases(masked, tile)
            names = list(cs) if hd == 16 else [n for n in ("Lk200", "cross469", "kB") if n in cs]
            for name in names:
                _validate(cs[name], hd, prec, fp8, gaps_of(prec, fp8), (name, masked, tile))


@pytest.mark.parametrize("prec,hd", [(p, h) for p in (1, 2) for h in (16, 32)], ids=lambda x: str(x))
def test_ffn_patterns_are_valid(prec, hd):
    for key, case in P.ffn_cases().items():
        _validate(case, hd, prec, 0, GAPS_FFN, key)


def test_reject_shapes_send_every_live_workgroup_back():
    """passes (b) and (c) of the GPU file: at their shapes every live workgroup holds a valid row whose match lies behind the first key tile (so the
    fallback counter of a rejected pass must equal the live workgroups), every head keeps a seam key inside the first tile (so the first tile's
    maximum is 0 or the match, never the background), and at least half of the rows match behind the first tile, at least a third inside it"""
    for masked in (0, 1):
        for tile in (64, 128):
            for name in P.REJECT_CASES[masked]:
                case = _cases(masked, tile)[name]
                sets = P.route_sets(case)
                assert P.later_tile_workgroups(case, sets) == case.live_workgroups(), (masked, tile, name)
                frac = P.later_tile_fraction(case, sets)
                assert 0.5 <= frac <= 2 / 3, (masked, tile, name, frac)
                assert all(min(s) < tile for per in sets for s in per)


def test_table_description_yields_the_forty_rows():
    rows = P.attn_table_rows()
    assert len(rows) == len(set(rows)) == 40
    assert sum(1 for r in rows if r[0] == 0) == 8 and all(sum(1 for r in rows if r[0] == p) == 16 for p in (1, 2))
    from ns2vc_amd import _lib
    if os.path.exists(_lib.LIB_PATH):              # the built table agrees (no HIP call: works without a device)
        n = C.c_int(-1)
        assert _lib.load().ns2vc_debug_kernel_table(3, C.byref(n), None) == 0 and n.value == len(rows)


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------------------------------------------------------------
def _flags(case, hd, prec, fp8, gap, mutant):
    """(flagged by COUNT, flagged by ROUTE) with the bounds the GPU file applies"""
    p_round = P.e4m3_round if fp8 else None
    q, k, v, sets = P.build_count(case, hd)
    qr, kr, vr = (P.round_op(t, prec) for t in (q, k, v))
    _, nonzero, _, ratio = P.check_count(P.attend(qr, kr, vr, case, hd, p_round=p_round, mutant=mutant), case, hd, sets, tol=lambda n: tol_attn_count(prec, n))
    by_count = nonzero > 0 or ratio > 1.0
    q, k, v, sets, want = P.build_route(case, hd, gap, prec)
    qr, kr, vr = (P.round_op(t, prec) for t in (q, k, v))
    ref = P.attend(qr, kr, vr, case, hd)
    out = P.attend(qr, kr, vr, case, hd, p_round=p_round, mutant=mutant)
    wrong, _, _ = P.check_route(out, case, hd, want)
    by_route = wrong > 0 or float(np.abs(out - ref).max()) > tol_attn_route(prec, bool(fp8), case.Lk)
    return by_count, by_route


def _all_shapes():
    for masked in (0, 1):
        for tile in (64, 128):
            for name, case in _cases(masked, tile).items():
                yield f"attn-{'masked' if masked else 'dense'}-keys{tile}-{name}", case
    for (Lk, mk), case in P.ffn_cases().items():
        yield f"ffn-Lk{Lk}-{'bias' if mk else 'nobias'}", case


@pytest.mark.parametrize("prec,fp8,gap", [(1, 0, 11.5), (1, 1, 7.5), (2, 0, 40.0)], ids=["bf16-gap11.5", "bf16-fp8-gap7.5", "fp16-gap40"])
def test_every_mutant_is_flagged_at_every_shape(prec, fp8, gap):
    """bf16 has the widest COUNT and ROUTE bounds, the fp8 form the widest ROUTE bound at the smallest gap; no mutant of the reference itself
    (mutant None) is flagged"""
    table = {}
    for name, case in _all_shapes():
        assert _flags(case, 16, prec, fp8, gap, None) == (False, False), name
        for m in P.MUTANTS:
            if not P.mutant_applies(case, m):
                continue
            c, r = _flags(case, 16, prec, fp8, gap, m)
            assert c or r, (name, m)
            t = table.setdefault(m, [0, 0, 0])
            t[0] += 1
            t[1] += c
            t[2] += r
    for m in P.MUTANTS:
        print(f"mutant {m}: applies at {table[m][0]} shapes, flagged by COUNT at {table[m][1]}, by ROUTE at {table[m][2]}")
        assert table[m][0] > 0


def test_whole_tensor_bounds_on_the_mutants():
    """the table of the module docstring: the four miscounts stay under the bf16 whole-tensor bound on unit-normal data (this is the gap the patterns
    close); the fp16 bound, three times the figure, is spent on the kernel's own rounding"""
    rng = np.random.default_rng(7)
    hd = 16
    shapes = {"Lk200 masked": P.Case(P.B_ATT, P.H_ATT, P.LQ_ATT, 200, q_lens=P.Q_LENS, k_lens=[129, 200, 129]),
              "Lk469 bias": P.Case(P.B_ATT, P.H_ATT, P.LQ_ATT, 469, plen=[469, 256, 129])}
    for name, case in shapes.items():
        D = case.H * hd
        q, k, v = (rng.standard_normal((case.B, L, D)) for L in (case.Lq, case.Lk, case.Lk))
        ref = P.attend(q, k, v, case, hd)
        for m in P.MUTANTS:
            if not P.mutant_applies(case, m):
                continue
            out = P.attend(q, k, v, case, hd, mutant=m)
            e = rel_l2(out, ref)                      # (rows past q_lens are zeros on both sides)
            items = [rel_l2(out[b, :case.nq(b)], ref[b, :case.nq(b)]) for b in range(case.B)]
            one = ref.copy()                          # the same defect in one wave (32 rows) of one head of item 0 only
            one[0, :32, :hd] = out[0, :32, :hd]
            print(f"whole-tensor view of {m} at {name}: rel_l2 {e:.2e}, per item {' '.join(f'{x:.1e}' for x in items)}, confined to one wave of one "
                  f"head: item {rel_l2(one[0], ref[0]):.1e} (bf16 bar {tol_attention(1):.1e}, fp16 bar {tol_attention(2):.1e})")
            assert e > 0 and np.isfinite(e)
