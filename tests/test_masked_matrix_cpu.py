"""tests/masked_matrix.py without a GPU: the shipped length vectors produce every block position and block kind REQUIRED asks for, the one vector the
masked row-chain and feed-forward tests ran before (T0 = 130, LENS0) does not, and check_launch -- the statement of the contract that
tests/test_masked_matrix_gpu.py holds the kernels to -- passes a right numpy model of a masked launch on every vector and reports ten wrong ones
(masked_matrix.MUTANTS), each on a shipped vector and with an item and a block position that the mutant truly gets wrong.  The table at the end says
which of the ten the earlier shapes would have let through."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import masked_matrix as MM                          # noqa: E402

KERNELS = sorted(MM.KERNEL_VECTORS)


def _vectors(kernel):
    names, widths = MM.KERNEL_VECTORS[kernel]
    return {n: MM.VECTORS[n] for n in names}, widths


@pytest.mark.parametrize("kernel", KERNELS)
def test_shipped_vectors_meet_required(kernel):
    vecs, widths = _vectors(kernel)
    for W in widths:
        gone = MM.missing(vecs, W, three_items=kernel != "ffn")
        assert not gone, (kernel, gone)
    if kernel == "ffn":
        assert all(T >= 64 for T, _ in vecs.values())
        assert not any(MM.census(T, lens, 64)["three_items"] for T, lens in vecs.values())


def test_vectors_are_what_the_module_says():
    T, lens = MM.VECTORS["V65"]
    assert len(lens) == 257 and len(lens) * T == 16705 == 261 * 64 + 1 and min(lens) == 33 and max(lens) == 65
    for W in MM.WIDTHS:             # the first 256 items alone: every position, for the starts and for the ends of the items with L >= 33
        c = MM.census(T, lens[:256], W)
        assert c["starts"] == list(range(W)) and c["first_dead"] == list(range(W))
    assert MM.census(T, lens, 64)["first_dead_long"] == list(range(64))
    assert MM.census(T, lens, 64)["last_partial"] and MM.census(T, lens, 128)["last_partial"]
    c64, c128 = (MM.census(*MM.VECTORS["VDEAD"], W) for W in MM.WIDTHS)
    assert c64["dead_full_blocks"] == 7 and c128["dead_full_blocks"] == 2
    assert c64["only_first_live"] == [0] and c128["only_first_live"] == [0]
    assert len(c64["dead_first_live_later"]) == 2 and len(c128["dead_first_live_later"]) == 2
    T, lens = MM.VECTORS["VSHORT"]
    assert T == 19 and len(lens) == 64 and sorted(set(lens)) == list(range(1, 20))
    for W, lo, hi in ((64, 4, 5), (128, 7, 8)):
        per_block = [len({m // T for m in range(k * W, (k + 1) * W)}) for k in range(len(lens) * T // W)]
        assert lo <= min(per_block) and max(per_block) <= hi
    T, lens = MM.VECTORS["VCLAMP"]
    assert sorted(set(lens) - set(MM.VECTORS["V65"][1])) == [-7, 0, T + 9] and len(lens) == 16
    assert MM.census(*MM.VECTORS["VLONG"], 128)["first_dead_long"] == list(range(128))
    for W in MM.WIDTHS:
        assert MM.census(*MM.VECTORS["VLAST"], W)["only_last_live"], W
    # without the two vectors of the module's own the census is not complete
    rest = {n: v for n, v in MM.VECTORS.items() if n not in ("VLONG", "VLAST")}
    assert any("first_dead_long" in s for s in MM.missing(rest, 128)) and any("only_last_live" in s for s in MM.missing(rest, 128))
    assert any("only_last_live" in s for s in MM.missing(rest, 64))


def test_the_earlier_vector_does_not_meet_required():
    """(T0, LENS0): first dead rows on positions {3, 5, 6, 7, 11} of a 64-row block only (the full item 0 has none: row 130, position 2, is item 1's
    first row), starts on {0, 2, .., 10}, no item end on position 0, 1, 31 - 33 or 63, no wholly dead full 128-row block"""
    T, lens = MM.TODAY_ROWS["T0_LENS0"]
    c = MM.census(T, lens, 64)
    assert c["first_dead"] == [3, 5, 6, 7, 11] and c["starts"] == [0, 2, 4, 6, 8, 10]
    assert MM.census(T, lens, 128)["dead_full_blocks"] == 0
    for W in MM.WIDTHS:
        gone = MM.missing(MM.TODAY_ROWS, W)
        print(f"(T0, LENS0) at W = {W} lacks: " + "; ".join(re.sub(r"\[(.*?)\]", lambda m: f"[{len(m.group(1).split(','))} of {W}]", s) for s in gone))
        assert any("first_dead:" in s for s in gone) and any("starts:" in s for s in gone)
        assert any("only_last_live" in s for s in gone) and any("three_items" in s for s in gone)
    assert MM.missing(MM.TODAY_GEGLU, 128)            # the two GEGLU shapes: not complete either


@pytest.mark.parametrize("W", MM.WIDTHS)
def test_right_model_passes_on_every_vector(W):
    for name, (T, lens) in {**MM.VECTORS, **MM.GN_VECTORS, **MM.TODAY_ROWS, **MM.TODAY_GEGLU}.items():
        masked, ref, changed = MM.model_case(T, lens, W)
        rec = MM.check_launch("model", name, T, lens, masked, ref, out_fill=MM.MODEL_OUT_FILL, W=W, changed=changed, stats_from="out_f32")
        assert not rec, [r["text"] for r in rec[:4]]


def _caught(T, lens, W, mutant, name):
    masked, ref, changed = MM.model_case(T, lens, W, mutant)
    return MM.check_launch(f"mutant {mutant}", name, T, lens, masked, ref, out_fill=MM.MODEL_OUT_FILL, W=W, changed=changed, stats_from="out_f32")


# the smallest shipped vectors that must report each mutant (V65 and VLONG are left to the right-model test above: the model is a Python loop)
WHERE = {"a": "VDEAD", "b": "VDEAD", "c": "VDEAD", "d": "VDEAD", "e": "VSHORT", "f": "VLAST", "g": "VCLAMP", "h": "VDEAD", "i": "VLAST", "j": "VDEAD"}


@pytest.mark.parametrize("mutant", sorted(MM.MUTANTS))
def test_every_mutant_is_reported_where_it_is_wrong(mutant):
    name = WHERE[mutant]
    T, lens = MM.VECTORS[name]
    for W in MM.WIDTHS:
        rec = _caught(T, lens, W, mutant, name)
        assert rec, (mutant, MM.MUTANTS[mutant], name, W)
        items, rows = MM.model_affected(T, lens, W, mutant)
        assert items or rows
        for r in rec:
            assert f"[{name}]" in r["text"] and f"mutant {mutant}" in r["text"]
            if r["out"] == "ln_health":
                assert -1 in items, r
                continue
            assert r["item"] in items, (mutant, W, r, sorted(items))
            if r["out"] != "stats":                   # a row is named: it is one the mutant gets wrong, at the position the message says
                assert r["row"] in rows and r["pos"] == r["row"] % W and f"position {r['pos']} of a {W}-row block" in r["text"] or r["out"] == "guard", r


def test_table_of_what_the_earlier_shapes_let_through():
    """every mutant against the earlier shapes, at both widths: printed, and the ones the issue names as passing today are asserted"""
    earlier = {**MM.TODAY_ROWS, **{"geglu " + k: v for k, v in MM.TODAY_GEGLU.items()}}
    passes = {}
    print("mutant  " + "  ".join(f"{n}@{W}" for n in earlier for W in MM.WIDTHS) + "    (P = passes check_launch there, x = reported)")
    for mutant in sorted(MM.MUTANTS):
        row = []
        for n, (T, lens) in earlier.items():
            for W in MM.WIDTHS:
                passes[(mutant, n, W)] = not _caught(T, lens, W, mutant, n)
                row.append("P" if passes[(mutant, n, W)] else "x")
        print(f"  ({mutant})   " + "  ".join(f"{c:^{len(n) + 1 + len(str(W))}}" for c, (n, W) in zip(row, ((n, W) for n in earlier for W in MM.WIDTHS)))
              + f"    {MM.MUTANTS[mutant]}")
    # more than two items in a block, a row behind M under a full last item, a count outside 0 .. T: nothing the row-chain / feed-forward vector has
    for mutant in ("e", "f", "g"):
        assert passes[(mutant, "T0_LENS0", 64)] and passes[(mutant, "T0_LENS0", 128)], mutant
    for n in earlier:                                 # no earlier shape has a count outside 0 .. T or a full last item in front of a partial block
        assert all(passes[(m, n, W)] for m in ("f", "g") for W in MM.WIDTHS), n
