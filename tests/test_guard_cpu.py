"""The guard harness (tests/guard.py) proves on the CPU that it can fail: the "device" is a host byte array, the kernels are numpy
functions that address it exactly like a device kernel (flat element index = base + row * ld + col), and each faulty one makes one of
the mistakes the GPU bounds tests (tests/test_kernel_bounds_gpu.py) exist to catch.  A harness that compared the wrong bytes would
pass those tests for ever; it cannot pass this file."""
from __future__ import annotations

import numpy as np
import pytest

from guard import FILLS, KINDS, Guarded, HostBackend, decode, encode, guard_elems, pattern_mismatches

M, N, TILE = 37, 24, 16          # 37 rows: a ragged last tile of 16


def _f32(g):
    return g.mem.view(np.float32)


def k_good(x, y, scale):
    """(a) y[r][c] = scale * x[r][c], logical elements only"""
    xm, ym = _f32(x), _f32(y)
    for r in range(M):
        ym[y.base + r * y.ld: y.base + r * y.ld + N] = scale * xm[x.base + r * x.ld: x.base + r * x.ld + N]


def k_gap_store(x, y, scale):
    """(b) one element into the gap columns behind row 5"""
    k_good(x, y, scale)
    _f32(y)[y.base + 5 * y.ld + N] = 1.0


def k_row_past_m(x, y, scale):
    """(c) the last tile stores its first discarded row too: row M of y, in the back guard, computed from row M of x, in ITS back guard"""
    k_good(x, y, scale)
    with np.errstate(invalid="ignore"):
        _f32(y)[y.base + M * y.ld: y.base + M * y.ld + N] = scale * _f32(x)[x.base + M * x.ld: x.base + M * x.ld + N]


def k_front_store(x, y, scale):
    """(d) "row -1" of the first item"""
    k_good(x, y, scale)
    _f32(y)[y.base - y.ld + 3] = 2.0


def k_gap_times_zero(x, y, scale):
    """(e) a zero-padded weight column times whatever follows the row: + 0 * x[r][N]"""
    k_good(x, y, scale)
    xm, ym = _f32(x), _f32(y)
    with np.errstate(invalid="ignore"):
        for r in range(M):
            ym[y.base + r * y.ld] += np.float32(0.0) * xm[x.base + r * x.ld + N]


def k_tile_reduction(x, s):
    """(f) a column sum per tile of TILE rows that does not stop at M: the last tile reads rows M .. into the back guard"""
    xm, sm = _f32(x), _f32(s)
    with np.errstate(invalid="ignore"):
        for t in range((M + TILE - 1) // TILE):
            acc = np.zeros(N, dtype=np.float32)
            for r in range(t * TILE, (t + 1) * TILE):
                acc += xm[x.base + r * x.ld: x.base + r * x.ld + N]
            sm[s.base + t * s.ld: s.base + t * s.ld + N] = acc


def k_tile_reduction_good(x, s):
    xm, sm = _f32(x), _f32(s)
    for t in range((M + TILE - 1) // TILE):
        acc = np.zeros(N, dtype=np.float32)
        for r in range(t * TILE, min((t + 1) * TILE, M)):
            acc += xm[x.base + r * x.ld: x.base + r * x.ld + N]
        sm[s.base + t * s.ld: s.base + t * s.ld + N] = acc


def _run(kernel, reduction=False):
    """the GPU tests' protocol: the same logical data under every fill; returns ({fill: violations}, P2 mismatches)"""
    be = HostBackend()
    data = np.random.default_rng(1).standard_normal((M, N)).astype(np.float32)
    viol, runs = {}, {}
    for fill in FILLS:
        x = Guarded(be, M, N, "f32", ld=N + 8, col0=4, fill=fill, data=data, name="x")
        if reduction:
            y = Guarded(be, (M + TILE - 1) // TILE, N, "f32", ld=N + 12, fill=fill, name="sums")
            kernel(x, y)
        else:
            y = Guarded(be, M, N, "f32", ld=N + 16, col0=8, fill=fill, skew=1, name="y")
            kernel(x, y, np.float32(-3.0))
        viol[fill] = x.violations() + y.violations()
        runs[fill] = {"y": y}
    return viol, pattern_mismatches(runs), runs


def test_a_good_kernel_passes():
    viol, p2, runs = _run(k_good)
    assert all(v == [] for v in viol.values()) and p2 == []
    data = np.random.default_rng(1).standard_normal((M, N)).astype(np.float32)
    assert np.array_equal(runs["nan"]["y"].read(), np.float32(-3.0) * data)
    viol, p2, _ = _run(k_tile_reduction_good, reduction=True)
    assert all(v == [] for v in viol.values()) and p2 == []


@pytest.mark.parametrize("kernel,region", [(k_gap_store, "y: gap row 5 col 24"), (k_row_past_m, "y: back (element +8, row 37 col 0)"),
                                           (k_front_store, "y: front (element -29, 1 row(s) before row 0)")],
                         ids=["b_gap_column", "c_row_past_M", "d_front"])
def test_stray_stores_are_reported_with_their_region(kernel, region):
    viol, _, _ = _run(kernel)
    # a stray store of a value COMPUTED from the neighbour's fill can reproduce the fill's own bytes (-3 * NaN is the same NaN): that is why
    # the protocol has three fills and compares bytes -- -3 * Inf = -Inf and -3 * 0 = -0.0 are both seen
    fills = ("inf", "zero") if kernel is k_row_past_m else FILLS
    for fill in fills:
        assert viol[fill], f"{kernel.__name__} under fill {fill}: not noticed"
        assert viol[fill][0].startswith(region), viol[fill][0]
        assert all(v.startswith("y: ") for v in viol[fill])          # the input's guards are intact
    if kernel is k_row_past_m:                                        # the whole stray row: N elements, all in the back guard
        assert len(viol["inf"]) == N and all("back" in v for v in viol["inf"])


def test_e_gap_value_times_zero_is_reported_by_the_pattern_comparison():
    viol, p2, runs = _run(k_gap_times_zero)
    assert all(v == [] for v in viol.values()), "nothing was stored out of place: P1 cannot see this one"
    assert p2 and any("non-finite" in m for m in p2) and any("differ" in m for m in p2), p2
    # ... and under the zero fill alone (what a tight, zero-initialised buffer amounts to) the result is right: the old tests' blind spot
    data = np.random.default_rng(1).standard_normal((M, N)).astype(np.float32)
    assert np.array_equal(runs["zero"]["y"].read(), np.float32(-3.0) * data)


def test_f_reduction_over_a_discarded_row_is_reported_by_the_pattern_comparison():
    viol, p2, runs = _run(k_tile_reduction, reduction=True)
    assert all(v == [] for v in viol.values())
    assert p2 and any("y [nan]" in m and "non-finite" in m for m in p2) and any("y [inf]" in m for m in p2), p2
    last = (M + TILE - 1) // TILE - 1
    assert np.isfinite(runs["nan"]["y"].read()[:last]).all() and np.isnan(runs["nan"]["y"].read()[last]).all()    # only the ragged tile


def test_finite_garbage_is_caught_by_bitwise_equality_alone():
    """two fills that are both finite still disagree when a neighbour leaks: equality, not finiteness, is the check"""
    a = {"y": (encode(np.array([[1.0, 2.0]]), "f32"), "f32")}
    b = {"y": (encode(np.array([[1.0, 2.0000002]]), "f32"), "f32")}
    assert pattern_mismatches({"zero": a, "inf": a}) == []
    assert len(pattern_mismatches({"zero": a, "inf": b})) == 1


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_layout_patterns_and_alignment(kind):
    be = HostBackend()
    sdt, pats = KINDS[kind]
    esz = np.dtype(sdt).itemsize
    per = max(16 // esz, 1)
    rows, width, col0, ld = 5, 3 * per, per, 6 * per
    vals = np.arange(rows * width).reshape(rows, width)
    for fill in FILLS:
        for skew in (0, 1):
            g = Guarded(be, rows, width, kind, ld=ld, col0=col0, fill=fill, data=vals, skew=skew)
            # derived guard: (128 + 2) rows of the pitch, in whole 4 KB, on each side
            assert g.front * esz >= 130 * ld * esz and g.back * esz >= 130 * ld * esz and (g.back * esz) % 4096 == 0
            assert g.back == guard_elems(ld, esz)
            assert g.ptr % 16 == 0 and (g.ptr - col0 * esz) % 128 == (16 if skew else 0)
            m = g.mem
            assert (m[:g.front] == pats[fill]).all() and (m[g.front + rows * ld:] == pats[fill]).all()
            body = m[g.front:g.front + rows * ld].reshape(rows, ld)
            assert (body[:, :col0] == pats[fill]).all() and (body[:, col0 + width:] == pats[fill]).all()
            assert np.array_equal(g.read().astype(np.float64), vals.astype(np.float64))
            assert g.violations() == []
            # an output: the logical region starts as the NaN of the type whatever the fill
            o = Guarded(be, rows, width, kind, ld=ld, col0=col0, fill=fill)
            assert (o.read_bits() == pats["nan"]).all()
    # the bit patterns are the IEEE ones
    assert np.isnan(decode(np.array([KINDS["f32"][1]["nan"]], np.uint32), "f32")).all() and np.isposinf(decode(np.array([0x7F800000], np.uint32), "f32")).all()
    assert np.isnan(decode(np.array([0x7FC0], np.uint16), "bf16")).all() and np.isposinf(decode(np.array([0x7F80], np.uint16), "bf16")).all()
    assert np.isnan(decode(np.array([0x7E00], np.uint16), "f16")).all() and np.isposinf(decode(np.array([0x7C00], np.uint16), "f16")).all()
    assert np.isnan(np.array([KINDS["i64"][1]["nan"]], np.uint64).view(np.float32)).all()      # an int64 neighbour read as two floats


def test_a_changed_byte_that_decodes_equal_is_still_a_violation():
    """violations() compares bytes: -0.0 over +0.0, or another NaN payload over the NaN fill, is a store"""
    be = HostBackend()
    g = Guarded(be, 4, 8, "f32", ld=16, fill="zero", data=np.ones((4, 8)))
    g.mem[g.base + 8] = 0x80000000
    assert g.violations() == ["f32: gap row 0 col 8: 0x0 -> 0x80000000"]
    h = Guarded(be, 4, 8, "bf16", ld=16, fill="nan", data=np.ones((4, 8)))
    h.mem[h.base + 3 * 16 + 9] = 0x7FC1
    assert h.violations() == ["bf16: gap row 3 col 9: 0x7fc0 -> 0x7fc1"]
    # a logical element may change freely
    h.mem[h.base] = 0
    assert len(h.violations()) == 1
