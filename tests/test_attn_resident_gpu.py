"""The K/V-resident attention kernel (csrc/attn_resident.hip: one 16-wave workgroup per (item, head), the head's K / V^T staged once) against the tiled
kernel it stands in for (csrc/attn.hip), through ns2vc_k_attention with the hook ns2vc_debug_set_attn_resident at 1 (whenever the launch fits) and 0 (never).

The two kernels share the arithmetic of a key tile (csrc/attn_common.h) and walk the tiles in the same order, so the bar is equality of every storage
word -- in the accepted optimistic pass, in the rejected one, and in the exact pass alone -- and equality of the fallback counter, whose unit is the tiled
kernel's workgroup (128 queries of one head).  No tolerance is involved there.  The COUNT / ROUTE patterns (tests/attn_patterns.py) run on the resident
kernel under the bounds of tests/util.py (tol_attn_count, tol_attn_route), as they do on the tiled one in tests/test_attn_positions_gpu.py.

Shapes (B = 2, H = 8 = 16 workgroups, the remainder-free branch of the XCD remap; the patterns' B = 3, H = 5 take the other one):
    Lk   1, 63, 64, 65, 129, 469 and the capacity (1024 keys at hd 16, 640 at hd 32); one past it is refused
    Lq   1, 31, 33 (one partial query tile, 15 idle waves; two tiles), 511, 513 (a second round of the 16 waves with one live row), 545 (uneven rounds)
    bias none, a -10000 suffix, and a -10000 PREFIX that masks the whole first key tile (the first tile's reference is 14427 log2 units too low: every row is rejected)
Every launch runs on guarded tensors (tests/guard.py): no store outside `out`, no word outside a tensor touched; `out` has exactly B * Lq rows, so a store
to a query row >= Lq of one item lands in the next item's rows or in the guard band and shows as a difference from the tiled kernel or as a violation."""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_patterns as P                           # noqa: E402
from attn_launch import PREC_IDS, _launch, _lib, _vals      # noqa: E402
from util import tol_attn_count, tol_attn_route     # noqa: E402

pytestmark = pytest.mark.gpu

B0, H0 = 2, 8
CAPACITY = {16: 1024, 32: 640}                      # keys: 160 KB of LDS / one stage (64 keys) of the tiled kernel's layout
LKS = (1, 63, 64, 65, 129, 469)
LQS = (1, 31, 33, 511, 513, 545)
ROWS = [(prec, hd) for prec in (1, 2) for hd in (16, 32)]
NEG = -10000.0


def _row_id(r):
    return f"{PREC_IDS[r[0]]}-hd{r[1]}"


def _resident(mode, *a, **kw):
    """_launch with the resident hook at `mode`; -> (bits, fallbacks, resident launches it made)"""
    lib = _lib()[1]
    assert lib.ns2vc_debug_set_attn_resident(mode) == 0
    n0 = lib.ns2vc_debug_attn_resident_launches()
    try:
        rc, bits, viol, nfb = _launch(*a, **kw)
    finally:
        lib.ns2vc_debug_set_attn_resident(-1)
    assert rc == 0, lib.ns2vc_last_error()
    assert not viol, viol
    return bits, nfb, lib.ns2vc_debug_attn_resident_launches() - n0


def _pair(prec, hd, q, k, v, want_resident=True, **kw):
    """the launch on the resident kernel (hook 1) and on the tiled one (hook 0): equal bits, equal counters; -> (bits, fallbacks)"""
    kw.setdefault("count", True)
    kw.setdefault("H", H0)
    bits1, nfb1, n1 = _resident(1, prec, hd, q, k, v, **kw)
    bits0, nfb0, n0 = _resident(0, prec, hd, q, k, v, **kw)
    assert n0 == 0 and n1 == (1 if want_resident else 0), (n0, n1)
    diff = int((bits1 != bits0).sum())
    assert diff == 0, (diff, np.argwhere(bits1 != bits0)[:4].tolist())
    assert nfb1 == nfb0, (nfb1, nfb0)
    return bits1, nfb1


@functools.lru_cache(maxsize=None)
def _operands(Lq, Lk, D, seed=0):
    """unit-normal q / k / v (B0, L, D), computed once per shape and left unchanged"""
    rng = np.random.default_rng(1000 * Lq + Lk + seed)
    return tuple(rng.standard_normal((B0, L, D)).astype(np.float32) for L in (Lq, Lk, Lk))


def _bias(kind, Lk):
    if kind == "suffix":                            # the reference's mask bias: the last third of item 0's keys, the last key of item 1
        return np.where(np.arange(Lk)[None, :] < np.array([max(Lk - Lk // 3, 1), max(Lk - 1, 1)])[:, None], 0.0, NEG).astype(np.float32)
    if kind == "prefix":                            # the whole first key tile masked (item 0), and one key more (item 1)
        return np.where(np.arange(Lk)[None, :] >= np.array([64, 65])[:, None], 0.0, NEG).astype(np.float32)
    return None


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_resident_equals_tiled_bits(row, diag):
    prec, hd = row
    D, cap = H0 * hd, CAPACITY[hd]
    shapes = [(545, Lk, None) for Lk in LKS + (cap,)] + [(Lq, 129, None) for Lq in LQS]
    shapes += [(Lq, Lk, kind) for kind in ("suffix", "prefix") for Lq, Lk in ((545, 469), (33, 129), (513, cap))]
    t0, nfb_prefix = time.time(), []
    for Lq, Lk, kind in shapes:
        q, k, v = _operands(Lq, Lk, D)
        for opt in (1, 0):                          # the optimistic pass with its per-wave repeat, and the exact pass alone
            bits, nfb = _pair(prec, hd, q, k, v, bias=_bias(kind, Lk), optimistic=opt)
            assert np.isfinite(_vals(bits, prec)).all(), (Lq, Lk, kind, opt)
            if opt == 0:
                assert nfb == 0, (Lq, Lk, kind, nfb)
            elif kind == "prefix":                  # the reference comes from masked keys, the later tiles exceed it by far more than 2^14: every block repeats
                assert nfb == B0 * H0 * ((Lq + 127) // 128), (Lq, Lk, nfb)
                nfb_prefix.append(nfb)
    diag(f"resident attention {_row_id(row)}: {2 * len(shapes)} shapes x (resident, tiled), every storage word and every fallback count equal; "
         f"first-tile-masked launches counted {nfb_prefix} blocks, {time.time() - t0:.1f} s")


REFUSED = [("Lk one past capacity, hd 16", dict(prec=2, hd=16, Lk=1025)), ("Lk one past capacity, hd 32", dict(prec=1, hd=32, Lk=641)),
           ("fp32", dict(prec=0, hd=16, Lk=129)), ("fp8 PV", dict(prec=2, hd=16, Lk=129, pv_fp8=1)), ("q_lens", dict(prec=2, hd=32, Lk=129, q_lens=[33, 7])),
           ("k_lens", dict(prec=1, hd=16, Lk=129, k_lens=[129, 65])), ("hd 48", dict(prec=2, hd=48, Lk=129))]


@pytest.mark.parametrize("name,spec", REFUSED, ids=[n for n, _ in REFUSED])
def test_refused_launches_stay_on_the_tiled_kernel(name, spec):
    """with the hook at 1 the predicate still refuses these: no resident launch is made and the bits are the tiled kernel's"""
    spec = dict(spec)
    prec, hd, Lk = spec.pop("prec"), spec.pop("hd"), spec.pop("Lk")
    q, k, v = _operands(33, Lk, H0 * hd, seed=7)
    _pair(prec, hd, q, k, v, want_resident=False, **spec)


@functools.lru_cache(maxsize=None)
def _cases():
    return P.attn_cases(0, 64)


@functools.lru_cache(maxsize=None)
def _route_data(name, hd, gap, prec):
    case = _cases()[name]
    q, k, v, sets, want = P.build_route(case, hd, gap, prec)
    qr, kr, vr = (P.round_op(t, prec) for t in (q, k, v))
    return q, k, v, want, P.attend(qr, kr, vr, case, hd)


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_count_and_route_on_the_resident_kernel(row, diag):
    """the dense cases of tests/test_attn_positions_gpu.py (Lk 65, Lk 200, the Lk 469 cross case under a bias mask; B = 3, H = 5, Lq = 200) on the resident
    kernel: COUNT with the optimistic pass on and off, ROUTE accepted at gap 17 and exact-only at gaps 11.5 / 12.5 (whether the reference moves)"""
    prec, hd = row
    t0, worst_c, worst_r = time.time(), 0.0, 0.0
    for name, case in _cases().items():
        q, k, v, sets = P.build_count(case, hd)
        for opt in (1, 0):
            bits, nfb, n = _resident(1, prec, hd, q, k, v, H=case.H, bias=case.bias(), optimistic=opt, count=True)
            err, nonzero, bad, ratio = P.check_count(_vals(bits, prec), case, hd, sets, tol=lambda m: tol_attn_count(prec, m))
            worst_c = max(worst_c, err)
            assert n == 1 and nfb == 0 and nonzero == 0 and ratio <= 1.0, (name, opt, n, nfb, err, nonzero, bad)
        for gap, kw in ((17.0, {}), (11.5, dict(exact_only=1)), (12.5, dict(exact_only=1))):
            q, k, v, want, ref = _route_data(name, hd, gap, prec)
            bits, nfb, n = _resident(1, prec, hd, q, k, v, H=case.H, bias=case.bias(), count=True, **kw)
            out = _vals(bits, prec)
            wrong, dev, bad = P.check_route(out, case, hd, want)
            err = float(np.abs(out - ref).max())
            worst_r = max(worst_r, err / tol_attn_route(prec, False, case.Lk))
            assert n == 1 and nfb == 0 and wrong == 0 and err <= tol_attn_route(prec, False, case.Lk), (name, gap, n, nfb, wrong, bad, err)
    diag(f"resident attention patterns {_row_id(row)}: COUNT worst |out n - 1| {worst_c:.2e}, excluded positions exact zeros; ROUTE decodes every row, "
         f"worst error {worst_r:.2f} of its bar, {time.time() - t0:.1f} s")


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_rejected_optimistic_pass(row, diag):
    """ROUTE at gaps 19 and 40 (p = 2^15 and beyond: rejected) at the shapes where every live 128-query block holds a row whose match lies behind the first
    key tile: bits and counter equal the tiled kernel's, the counter equals the live blocks, every row decodes.  Then the same data with every query row
    zeroed except rows 32 .. 63 of each item: only the second wave of the first block can fail, and the block still counts once."""
    prec, hd = row
    seen = []
    for name in P.REJECT_CASES[0]:
        case = _cases()[name]
        for gap in (19.0, 40.0):
            q, k, v, want, ref = _route_data(name, hd, gap, prec)
            bits, nfb = _pair(prec, hd, q, k, v, H=case.H, bias=case.bias())
            out = _vals(bits, prec)
            wrong, _, bad = P.check_route(out, case, hd, want)
            assert nfb == case.live_workgroups() and wrong == 0, (name, gap, nfb, case.live_workgroups(), wrong, bad)
            assert float(np.abs(out - ref).max()) <= tol_attn_route(prec, False, case.Lk)
            seen.append(nfb)
        q1 = np.zeros_like(q)
        q1[:, 32:64] = q[:, 32:64]
        _, nfb = _pair(prec, hd, q1, k, v, H=case.H, bias=case.bias())
        assert nfb == case.B * case.H, (name, nfb)                                # one block per (item, head): the first
        seen.append(nfb)
    diag(f"resident attention, rejected optimistic pass {_row_id(row)}: bits = tiled, fallback blocks {seen}")


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine: B = 32 (B * H = 256 workgroups: the rule selects the kernel), T = 131, Lp = 65
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPE = (32, 131, 65)


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


def _inputs(tag):
    import torch
    from ns2vc_amd.weights import hash_normal
    B, T, Lp = SHAPE
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(hash_normal(tag + ".x", (B, 100, T))).to(dev), torch.from_numpy(hash_normal(tag + ".c", (B, 256, T))).to(dev),
            torch.from_numpy(hash_normal(tag + ".p", (B, Lp, 256))).to(dev), torch.linspace(50.0, 900.0, B, device=dev))


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
def test_engine_option_attn_resident(prec, weights, diag):
    import torch
    from ns2vc_amd.engine import Engine
    lib = _lib()[1]
    x, c, p, t = _inputs("ares")
    outs, launches, made, loops = {}, {}, {}, {}
    for on in (1, 0):
        e = Engine(precision=prec)
        try:
            e.load_state_dict(weights)
            e.set_option("attn_resident", bool(on))
            e.prepare(*SHAPE)
            e.set_condition(c, p, None)
            n0 = lib.ns2vc_debug_attn_resident_launches()
            out = torch.empty_like(x)
            e.forward(x, t, out)
            torch.cuda.synchronize()
            made[on] = lib.ns2vc_debug_attn_resident_launches() - n0
            outs[on], launches[on] = out.cpu().numpy(), e.launches()
            if on:                                   # captured loop = eager loop, 3 steps
                e.load_sampler("unipc", 3)
                for graph in (True, False):
                    xs = x.clone()
                    e.sample(xs, use_graph=graph)
                    torch.cuda.synchronize()
                    loops[graph] = xs.cpu().numpy()
        finally:
            e.close()
    assert made[1] > 0 and made[0] == 0, made
    assert launches[1] == launches[0], launches
    assert np.isfinite(outs[1]).all() and np.array_equal(outs[1].view(np.uint32), outs[0].view(np.uint32))
    assert np.isfinite(loops[True]).all() and np.array_equal(loops[True].view(np.uint32), loops[False].view(np.uint32))
    diag(f"engine option attn_resident {prec} at B, T, Lp = {SHAPE}: {made[1]} resident launches per forward with it on, 0 with it off, {launches[1]} "
         f"launches either way, forward bit-identical; captured 3-step loop = eager loop with it on")
