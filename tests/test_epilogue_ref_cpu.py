"""CPU tests of tests/epilogue_ref.py: the float64 reference is right (against torch's conv1d / linear in float64), the `lens` vectors of the GPU
matrix hit every tile row they are meant to, and check_launch -- the ONE checker tests/test_epilogue_matrix_gpu.py runs on device results --
reports each of eight subtly wrong numpy "kernels" at every shape the GPU test uses (positive controls, in the style of tests/test_guard_cpu.py)."""
from __future__ import annotations

import numpy as np
import pytest

import epilogue_ref as R
from test_kernels_gpu import TOL                      # (importable without a GPU: the bound check_launch is handed on the device, too)

PREC = 2                                              # the shipped default operand type; the numpy kernels round like it
GEOMS = {"gemm": [R.geometry("gemm", 128, 64), R.geometry("gemm", 64, 32)], "conv": [R.geometry("conv", wave_rows=32), R.geometry("conv", wave_rows=64)]}


def _vectors(case):
    return R.lens_vectors(case, R.geometry(case["kern"]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tmode,Tin,Tout", [(0, 37, 37), (1, 37, 19), (1, 38, 19), (2, 19, 37), (2, 19, 38)])
def test_reference_equals_torch_conv1d(tmode, Tin, Tout):
    import torch
    import torch.nn.functional as F
    case = R._case("ref_conv", "gemm", 2, Tin, Tout, 64, 128, taps=3, tmode=tmode, c1=64, c2=64 if tmode == 0 else 0, res="sep")
    inp = R.make_inputs(case, 0)
    ref = R.reference(inp)["out"]
    x = torch.from_numpy(np.concatenate([inp["a0"], inp["a1"]], axis=1).astype(np.float64).reshape(2, Tin, 128)).permute(0, 2, 1)
    W = torch.from_numpy(inp["W"].astype(np.float64))
    w3 = W[:, :3 * 128].reshape(128, 3, 128).permute(0, 2, 1)                                    # k = tap * Ct + c -> (n, c, tap)
    if tmode == 2:                                                                               # nearest-upsample to Tout rows, then the conv
        x = x[:, :, torch.clamp(torch.arange(Tout) >> 1, max=Tin - 1)]
        np.testing.assert_array_equal(R.gather_rows(np.arange(Tin, dtype=np.float64).reshape(1, Tin, 1), 1, Tin, Tout, 3, 2)[0, :, 1, 0],
                                      np.minimum(np.arange(Tout) >> 1, Tin - 1))
    y = F.conv1d(x, w3, bias=torch.from_numpy(inp["bias"].astype(np.float64)), stride=2 if tmode == 1 else 1, padding=1)
    y = y.permute(0, 2, 1).reshape(2 * Tout, 128)
    if case["c2"]:
        y = y + torch.from_numpy(inp["a2"].astype(np.float64)) @ W[:, 3 * 128:].T
    y = y.numpy() + inp["res"]
    assert y.shape == ref.shape and np.abs(y - ref).max() < 1e-12 * max(1.0, np.abs(ref).max())


def test_reference_linear_and_geglu():
    import torch
    case = R._case("ref_geglu", "gemm", 2, 9, 9, 64, 256, res="sep", geglu=1)
    inp = R.make_inputs(case, 0)
    pre = torch.from_numpy(inp["a0"].astype(np.float64)) @ torch.from_numpy(inp["W"].astype(np.float64)).T + torch.from_numpy(inp["bias"].astype(np.float64))
    p = pre.reshape(18, 4, 2, 32)                                                                # packed (32 value | 32 gate)
    y = (p[:, :, 0] * torch.nn.functional.gelu(p[:, :, 1])).reshape(18, 128).numpy() + inp["res"]
    assert np.abs(y - R.reference(inp)["out"]).max() < 1e-12


@pytest.mark.parametrize("case", R.MASKED_CASES, ids=lambda c: c["name"])
def test_masked_reference(case):
    """full lengths = the dense reference; under lengths the valid rows are the dense rows and the others zero, whatever the padded rows hold"""
    v = _vectors(case)
    dense = R.reference(R.make_inputs(case, PREC))["out"]
    assert np.array_equal(R.reference(R.make_inputs(case, PREC, v["full"]))["out"], dense)
    for name in [k for k in v if k != "full"]:
        for fill in ("nan", "inf"):
            inp = R.make_inputs(case, PREC, v[name], fill)
            y = R.reference(inp)["out"]
            ok = R.valid_mask(case["B"], case["Tout"], v[name])
            assert np.isfinite(y).all() and np.all(y[~ok] == 0.0)
            if case["taps"] == 1:                      # k = 3 reads the neighbour rows, which the row invariant zeroes: the dense launch ON THOSE inputs
                assert np.array_equal(y[ok], dense[ok])
            if inp["res"] is not None:
                assert not np.isfinite(inp["res"][~ok]).any()
    s = R.stats_fixed(dense, case["B"], case["Tout"], v["ones"]) if not case["geglu"] else None
    if s is not None:
        first = dense.reshape(case["B"], case["Tout"], -1, 16)[:, 0]
        assert np.array_equal(s[..., 0], np.rint(first.sum(-1) * 2.0 ** 28).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------------
# coverage control: the lens vectors put an item's end where the kernels decide something
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.MASKED_CASES if c["vectors"] is None], ids=lambda c: c["name"])
def test_residue_vector_covers_every_tile_row(case):
    g = R.geometry(case["kern"])
    lens = _vectors(case)["residue"]
    B, T = case["B"], case["Tout"]
    assert B <= 16 and T <= 200 and lens.min() >= 1 and lens.max() <= T
    hit = R.rows_hit(B, T, lens, g["tile_rows"], g["pad"])
    assert hit >= set(g["residues"]), sorted(set(g["residues"]) - hit)
    for geom in GEOMS[case["kern"]]:
        assert R.second_item_length_matters(B, T, lens, geom), (case["name"], geom)
    j = np.flatnonzero(R.perturbed(lens, T) != lens)
    assert len(j) == 1


def test_residue_vector_feasibility_table():
    """the (T, items) pairs the shapes were chosen from: feasible with B <= 16.  T = 64 is not (an item start is always on tile row 0 or 64, so eleven of
    the rows have eight items to share), so no residue vector uses it; the tap-sharing kernel's T = 66 only just is, with a matching, and is left to the
    dense-only rows"""
    for kern, Ts, need in (("gemm", (97, 81, 74), 15), ("conv", (131, 97), 13)):
        g = R.geometry(kern)
        for T in Ts:
            B = next(b for b in range(1, 17) if _feasible(b, T, g))
            assert B <= need + 1, (kern, T, B)
    assert not _feasible(16, 64, R.geometry("gemm"))


def _feasible(B, T, g):
    try:
        lens = R.residue_lens(B, T, g)
    except ValueError:
        return False
    return R.rows_hit(B, T, lens, g["tile_rows"], g["pad"]) >= set(g["residues"])


@pytest.mark.parametrize("case", [c for c in R.MASKED_CASES if c["vectors"] == "short"], ids=lambda c: c["name"])
def test_short_items_share_a_wave_tile(case):
    B, T = case["B"], case["Tout"]
    lens = _vectors(case)["mixed"]
    assert T in (19, 24) and B == 9 and {1, T} <= set(lens.tolist()) and len(set(lens.tolist())) >= 5
    assert R.items_per_span(B, T, R.geometry("gemm", 128, 64)) >= (4 if T == 19 else 3)
    if T == 19:
        assert R.items_per_span(B, T, R.geometry("gemm", 64, 32)) >= 3


# ---------------------------------------------------------------------------------------------------------------------------------------
# positive controls: a numpy "kernel" with the row rule of csrc/epilogue.h, and one defect at a time
# ---------------------------------------------------------------------------------------------------------------------------------------
DEFECTS = {
    "a_bias_on_masked_rows": lambda c: bool(c["bias"]),
    "b_residual_on_masked_rows": lambda c: c["res"] is not None,
    "c_masked_row_in_stats": lambda c: bool(c["stats"]),
    "d_second_item_masked_with_first_length": lambda c: True,
    "e_item_end_off_by_one": lambda c: True,
    "f_masked_rows_unwritten": lambda c: True,
    "g_out_op_not_zeroed": lambda c: c["out"] in ("both", "op"),
    "h_third_item_takes_b0_plus_1": lambda c: c["vectors"] == "short",
}


# the checks of check_launch (their numbers lead every violation) that are MEANT to catch each defect -- at least one of them fires -- and every
# check the defect can rightly trip besides: 1 (the fp64 comparison sees any wrong row), 2 (a leaked NaN), 5 and 7 (statistics and other items
# follow the rows).  Nothing outside ALLOWED may fire: 6 (full lengths) and 8 (guards) never do here.
MEANT = {"a": {"3"}, "b": {"2", "3"}, "c": {"5"}, "d": {"3", "4"}, "e": {"3"}, "f": {"3"}, "g": {"3"}, "h": {"3", "4"}}
ALLOWED = {k: v | {"1", "2", "5", "7"} for k, v in MEANT.items()}
ALLOWED["c"] = {"5", "7"}                                                # (the rows are right: only the statistics checks may speak)
ALLOWED["g"] = {"1", "3"}                                                # (out_f32 is right: out_op's zero rows / out_op == rnd(out_f32); 1 where out_op is the only output)


def numpy_kernel(inp, geom, defect=None, dense=False):
    """what a kernel with epilogue.h's row rule stores: fp32 accumulator of the fp64 products, bias / GEGLU / residual in fp32, live rows only"""
    case, prec = inp["case"], inp["prec"]
    B, T, N = case["B"], case["Tout"], case["N"]
    M, P = B * T, T + geom["pad"]
    if "_ref" not in inp:
        inp["_ref"] = R.reference(inp)
    acc = inp["_ref"]["acc"].astype(np.float32)
    lens = np.full(B, T) if (dense or inp["lens"] is None) else inp["lens"]
    b_of, t_of = np.divmod(np.arange(M), T)
    used = lens[b_of].copy()                                                # the length each row is masked with
    if defect in ("d_second_item_masked_with_first_length", "h_third_item_takes_b0_plus_1"):
        q = b_of * P + t_of                                                 # (padded) row -> its wave span -> the span's first item b0
        for lo, hi in R.wave_spans(B, T, geom):
            rows = np.flatnonzero((q >= lo) & (q < hi))
            b0 = min(lo // P, B - 1)
            if defect[0] == "d":
                used[rows] = np.where(b_of[rows] > b0, lens[b0], used[rows])
            else:
                used[rows] = lens[np.minimum(b_of[rows], b0 + 1)]
    if defect == "e_item_end_off_by_one":
        used = np.minimum(used + 1, T)
    live = t_of < used
    v = acc + inp["bias"] if inp["bias"] is not None else acc.copy()
    if case["geglu"]:
        p = v.reshape(M, N // 64, 2, 32)
        v = (p[:, :, 0] * R._gelu(p[:, :, 1].astype(np.float64)).astype(np.float32)).reshape(M, N // 2)
    nores = v.copy()
    if inp["res"] is not None:
        v = v + inp["res"]
    y = np.where(live[:, None], v, np.float32(0.0)).astype(np.float32)
    yo = R.rnd(y, prec)
    if defect == "a_bias_on_masked_rows":
        y = np.where(live[:, None], y, np.broadcast_to(inp["bias"][:y.shape[1]], y.shape)).astype(np.float32)
        yo = R.rnd(y, prec)
    if defect == "b_residual_on_masked_rows":
        y = np.where(live[:, None], y, inp["res"]).astype(np.float32)
        yo = R.rnd(y, prec)
    if defect == "f_masked_rows_unwritten":                                 # what the buffer held: the NaN prefill, or the aliased residual
        y = np.where(live[:, None], y, inp["res"] if case["res"] == "alias" else np.float32(np.nan)).astype(np.float32)
        yo = np.where(live[:, None], yo, np.float32(np.nan)).astype(np.float32)
    if defect == "g_out_op_not_zeroed":
        yo = np.where(live[:, None], yo, R.rnd(nores, prec)).astype(np.float32)
    out = dict(out_f32=y if case["out"] in ("both", "f32") else None, out_op=yo if case["out"] in ("both", "op") else None, stats=None, viol=[])
    if case["stats"]:
        counted = np.ones(M, bool) if defect == "c_masked_row_in_stats" else live
        s = np.where(counted[:, None], np.where(live[:, None], np.nan_to_num(y), nores), 0.0).astype(np.float64).reshape(B, T, N // 16, 16)
        with np.errstate(all="ignore"):                                       # (a dense twin sums the poisoned rows as well: garbage, never compared)
            out["stats"] = np.stack([np.rint(s.sum(axis=(1, 3)) * R.SUM_SCALE), np.rint((s * s).sum(axis=(1, 3)) * R.SQ_SCALE)], axis=-1).astype(np.int64)
    return out


def _run(case, vec_name, geom, defect, fill="nan"):
    v = _vectors(case)
    lens = v[vec_name]
    inp = R.make_inputs(case, PREC, lens, fill)
    inp2 = R.make_inputs(case, PREC, R.perturbed(lens, case["Tout"]), fill)
    fig = {}
    bad = R.check_launch(inp, numpy_kernel(inp, geom, defect), numpy_kernel(inp, geom, None, dense=True), tol=TOL[PREC], geom=geom,
                         other=(inp2, numpy_kernel(inp2, geom, defect)), figures=fig)
    return bad, fig


@pytest.mark.parametrize("case", R.MASKED_CASES, ids=lambda c: c["name"])
def test_checker_accepts_the_correct_kernel(case):
    for geom in GEOMS[case["kern"]]:
        for name in _vectors(case):
            for fill in ("nan", "inf"):
                bad, fig = _run(case, name, geom, None, fill)
                assert not bad, (case["name"], name, fill, bad)
                assert case["geglu"] or all(v for k, v in fig.items() if k.startswith("bitwise"))


@pytest.mark.parametrize("case", R.DENSE_CASES, ids=lambda c: c["name"])
def test_checker_accepts_the_correct_dense_kernel(case):
    for geom in GEOMS[case["kern"]]:
        inp = R.make_inputs(case, PREC)
        assert not R.check_launch(inp, numpy_kernel(inp, geom), None, tol=TOL[PREC], geom=geom)


@pytest.mark.parametrize("defect", list(DEFECTS), ids=list(DEFECTS))
def test_checker_reports_defect(defect):
    """every defect is reported at EVERY shape of the GPU matrix it can show at, under the residue (or mixed) vector, for either row tiling; (c) also
    under the all-1 vector, where a wrongly counted row is large against the item's own sums and small against a full item's"""
    ran = 0
    for case in R.MASKED_CASES:
        if not DEFECTS[defect](case):
            continue
        for geom in GEOMS[case["kern"]]:
            if defect[0] == "h" and R.items_per_span(case["B"], case["Tout"], geom) < 3:
                continue
            vec = "mixed" if case["vectors"] == "short" else "residue"
            bad, _ = _run(case, vec, geom, defect)
            assert bad, (defect, case["name"], geom["tile_rows"], geom["wave_rows"])
            # ... and by the check that is there for it, not by some other one going red
            got = {b.split()[0] for b in bad}
            assert got & MEANT[defect[0]], (defect, case["name"], bad)
            assert got <= ALLOWED[defect[0]], (defect, case["name"], bad)
            ran += 1
    assert ran >= (5 if defect[0] == "h" else 8), (defect, ran)


def test_stats_of_a_short_item_cannot_hide_behind_a_full_one():
    """ONE masked row counted for an L = 1 item next to full items: the whole-tensor figure (relative to the largest entry) stays under
    TOL_STATS-like levels only if it is small; the per-item bound reports it whatever the neighbours hold"""
    case = R._case("stats_hide", "gemm", 3, 97, 97, 64, 128, stats=1, out="f32")
    geom = R.geometry("gemm", 128, 64)
    lens = np.array([97, 1, 97], np.int32)
    inp = R.make_inputs(case, PREC, lens)
    out = numpy_kernel(inp, geom)
    assert not R.check_launch(inp, out, None, tol=TOL[PREC], geom=geom)
    row = inp["_ref"]["acc"][97 + 1].astype(np.float32) + inp["bias"]                      # item 1, frame 1: one row too many, scaled down to hide
    s = (2e-4 * row.astype(np.float64)).reshape(8, 16)
    out["stats"] = out["stats"].copy()
    out["stats"][1, :, 0] += np.rint(s.sum(-1) * R.SUM_SCALE).astype(np.int64)
    out["stats"][1, :, 1] += np.rint((s * s).sum(-1) * R.SQ_SCALE).astype(np.int64)
    bad = R.check_launch(inp, out, None, tol=TOL[PREC], geom=geom)
    assert bad and all(b.startswith("5 stats sum of item 1") for b in bad), bad
