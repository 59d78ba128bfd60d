"""The K/V-resident attention kernel under per-item length tables (csrc/attn_resident.hip: attnres_lens_kernel; plan option ``masked_attn_resident``)
against the masked tiled kernel it stands in for (csrc/attn.hip: attn_kernel<..., MASKED>), through ns2vc_k_attention with the hook
ns2vc_debug_set_attn_resident_lens at 1 (whenever the launch fits) and 0 (never).

The two kernels run the same key-tile arithmetic (csrc/attn_common.h) over the same tiles of an item in the same order, so the bar is equality of
every storage word of `out` -- the valid rows and the zero rows past an item's end, in the accepted optimistic pass, the rejected one and the exact pass
alone -- and equality of the fallback counter (unit: a live 128-query block of one head).  No tolerance is involved.  Every kernel-level launch runs on
guarded tensors (tests/guard.py) whose padded rows of q / k / v hold NaN in one pass and Inf in another: a read past an item's end shows in the bits,
a store outside `out` as a violation.

ns2vc_k_attention refuses a count below 1, so the lengths start at 1: the Lqb = 0 path of the kernel (zeros, then return before staging) is reached
through the kernel's own clamp only and is not driven from here.

Lengths at Lq = Lk = 545 (18 query tiles: a second round of the 16 waves; 9 key tiles, which fits hd 32): one past / at a key tile (65 / 64, 513 / 512,
129 / 128), a 32-query tile (33 / 32 / 31), a 128-query block (129 / 128 / 127), the second wave round (545 / 513 / 512 / 511) and one frame."""
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard as G                                  # noqa: E402
from attn_launch import OUT_FILL, PREC_IDS, _launch, _lib      # noqa: E402

pytestmark = pytest.mark.gpu

L0 = 545
GEOMS = {"B8H8": (8, 8, [545, 513, 512, 129, 128, 65, 64, 1]),       # B * H = 64: the remainder-free branch of the XCD remap
         "B7H5": (7, 5, [545, 511, 127, 63, 33, 32, 31])}            # B * H = 35: the other one
CAPACITY = {16: 1024, 32: 640}                      # keys: 160 KB of LDS / one 64-key stage
ROWS = [(prec, hd) for prec in (2, 1) for hd in (16, 32)]
NEG = -10000.0


def _row_id(r):
    return f"{PREC_IDS[r[0]]}-hd{r[1]}"


def _hooked(mode, *a, old=None, **kw):
    """_launch with the lens hook at `mode` (and the dense hook at `old`, if given); -> (status, bits, fallbacks, lens launches, dense launches)"""
    lib = _lib()[1]
    assert lib.ns2vc_debug_set_attn_resident_lens(mode) == 0
    if old is not None:
        assert lib.ns2vc_debug_set_attn_resident(old) == 0
    n0, d0 = lib.ns2vc_debug_attn_resident_lens_launches(), lib.ns2vc_debug_attn_resident_launches()
    kw.setdefault("count", True)
    try:
        rc, bits, viol, nfb = _launch(*a, **kw)
    finally:
        lib.ns2vc_debug_set_attn_resident_lens(-1)
        lib.ns2vc_debug_set_attn_resident(-1)
    assert not viol, viol
    return rc, bits, nfb, lib.ns2vc_debug_attn_resident_lens_launches() - n0, lib.ns2vc_debug_attn_resident_launches() - d0


def _pair(prec, hd, q, k, v, want=1, **kw):
    """the launch with the lens hook at 1 and at 0: equal status, equal bits, equal fallback counts; the lens counter reads `want` against 0 and the
    dense kernel's counter 0 in both; -> (status, bits, fallbacks)"""
    rc1, bits1, nfb1, n1, d1 = _hooked(1, prec, hd, q, k, v, **kw)
    rc0, bits0, nfb0, n0, d0 = _hooked(0, prec, hd, q, k, v, **kw)
    assert rc1 == rc0, (rc1, rc0, _lib()[1].ns2vc_last_error())
    assert (n1, n0, d1, d0) == (want, 0, 0, 0), (n1, n0, d1, d0)
    diff = int((bits1 != bits0).sum())
    assert diff == 0, (diff, np.argwhere(bits1 != bits0)[:4].tolist())
    assert nfb1 == nfb0, (nfb1, nfb0)
    return rc1, bits1, nfb1


def _poison(a, lens, bad):
    a = a.copy()
    for b, L in enumerate(lens):
        a[b, L:] = bad
    return a


@functools.lru_cache(maxsize=None)
def _operands(B, Lq, Lk, D, seed=0):
    """unit-normal q / k / v, computed once per shape and left unchanged"""
    rng = np.random.default_rng(100000 * B + 1000 * Lq + Lk + seed)
    return tuple(rng.standard_normal((B, L, D)).astype(np.float32) for L in (Lq, Lk, Lk))


def _zeros_past(bits, lens):
    for b, L in enumerate(lens):
        assert not bits[b, L:].any(), (b, L)                                   # exact zeros: every storage word 0


# ---- 1. self form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_self_form(row, geom, diag):
    prec, hd = row
    B, H, lens = GEOMS[geom]
    q, k, v = _operands(B, L0, L0, H * hd)
    t0 = time.time()
    for opt in (1, 0):                              # the optimistic pass with its per-wave repeat, and the exact pass alone
        alone = None
        if geom == "B8H8":                          # the dense tiled kernel on every item alone at Lq = Lk = L_b
            alone = []
            for b, L in enumerate(lens):
                rc, bits, _, n, d = _hooked(0, prec, hd, q[b:b + 1, :L], k[b:b + 1, :L], v[b:b + 1, :L], old=0, H=H, optimistic=opt)
                assert rc == 0 and n == 0 and d == 0
                alone.append(bits[0])
        for fill in ("nan", "inf"):
            bad = np.nan if fill == "nan" else np.inf
            rc, bits, nfb = _pair(prec, hd, _poison(q, lens, bad), _poison(k, lens, bad), _poison(v, lens, bad), H=H, q_lens=lens, k_lens=lens,
                                  optimistic=opt, fill=fill)
            assert rc == 0, _lib()[1].ns2vc_last_error()
            _zeros_past(bits, lens)
            if opt == 0:
                assert nfb == 0
            if alone is not None:
                for b, L in enumerate(lens):
                    assert np.array_equal(bits[b, :L], alone[b]), (fill, opt, b, L, int((bits[b, :L] != alone[b]).sum()))
    diag(f"resident attention under lengths, self form {_row_id(row)} {geom} lens {lens}: (optimistic, exact) x (NaN, Inf) pads, every storage word and "
         f"fallback count = the masked tiled kernel's" + ("; valid rows = the dense tiled kernel on each item alone" if geom == "B8H8" else "") +
         f", {time.time() - t0:.1f} s")


# ---- 2. capacity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_capacity_and_one_key_past_it(row, diag):
    prec, hd = row
    B, H, cap = 2, 8, CAPACITY[hd]
    for L, want in ((cap, 1), (cap + 1, 0)):        # the last length that fits; one key more: the predicate refuses, the tiled kernel runs
        lens = [L, L - 63]
        q, k, v = _operands(B, L, L, H * hd)
        rc, bits, _ = _pair(prec, hd, _poison(q, lens, np.nan), _poison(k, lens, np.nan), _poison(v, lens, np.nan), want=want, H=H, q_lens=lens, k_lens=lens)
        assert rc == 0
        _zeros_past(bits, lens)
    diag(f"resident attention under lengths {_row_id(row)}: {cap} keys run on it, {cap + 1} on the tiled kernel; equal bits either way")


# ---- 3. cross form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lk", [40, 100, 469])
@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_cross_form(row, Lk, diag):
    prec, hd = row
    B, H, ql = GEOMS["B7H5"]
    q, k, v = _operands(B, L0, Lk, H * hd, seed=3)
    plen = [int(round(x)) for x in np.linspace(Lk, 3, B)]                      # prompt lengths from Lk down to 3
    suffix = np.where(np.arange(Lk)[None, :] < np.array(plen)[:, None], 0.0, NEG).astype(np.float32)      # the reference's mask bias
    holes = suffix.copy()
    for b, P in enumerate(plen):
        holes[b, P // 2] = NEG                      # ... with a masked key below P_b as well, which k_lens cannot express
    for fill in ("nan", "inf"):
        bad = np.nan if fill == "nan" else np.inf
        qp = _poison(q, ql, bad)
        # q_lens only: every key row is valid, the bias row switches the tail of the prompt off
        rc, bits, _ = _pair(prec, hd, qp, k, v, H=H, q_lens=ql, bias=suffix, fill=fill)
        assert rc == 0
        _zeros_past(bits, ql)
        # q_lens + k_lens: the key rows past the prompt hold NaN / Inf; without a bias, and with the row that has a hole
        kp, vp = _poison(k, plen, bad), _poison(v, plen, bad)
        for bias in (None, holes):
            rc, bits, _ = _pair(prec, hd, qp, kp, vp, H=H, q_lens=ql, k_lens=plen, bias=bias, fill=fill)
            assert rc == 0
            _zeros_past(bits, ql)
    diag(f"resident attention under lengths, cross form {_row_id(row)} Lk {Lk}: q_lens + suffix bias, q_lens + k_lens {plen} without / with a bias "
         f"row with holes: bits = the masked tiled kernel's")


# ---- 4. rejected optimistic pass ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_rejected_optimistic_pass(row, diag):
    """a -10000 prefix bias masks the whole first key tile (and one key more in every other item): the first tile's reference is 14427 log2 units too
    low, every live row is rejected and every live 128-query block counts once"""
    prec, hd = row
    B, H = 8, 8
    lens = [545, 513, 512, 300, 257, 129, 128, 66]
    q, k, v = _operands(B, L0, L0, H * hd)
    bias = np.where(np.arange(L0)[None, :] >= (64 + np.arange(B) % 2)[:, None], 0.0, NEG).astype(np.float32)
    rc, bits, nfb = _pair(prec, hd, _poison(q, lens, np.nan), _poison(k, lens, np.nan), _poison(v, lens, np.nan), H=H, q_lens=lens, k_lens=lens, bias=bias)
    assert rc == 0
    _zeros_past(bits, lens)
    want = sum(H * ((L + 127) // 128) for L in lens)
    assert nfb == want, (nfb, want)
    diag(f"resident attention under lengths, first key tile masked {_row_id(row)}: bits = tiled, {nfb} fallback blocks = sum_b H ceil(Lqb / 128)")


# ---- 5. selection ---------------------------------------------------------------------------------------------------------------------
SELECT = [("dense launch", dict(prec=2, hd=16, Lk=129), False), ("fp32", dict(prec=0, hd=16, Lk=129), True), ("hd 48", dict(prec=2, hd=48, Lk=129), True),
          ("over capacity hd 16", dict(prec=1, hd=16, Lk=1025), True), ("over capacity hd 32", dict(prec=2, hd=32, Lk=641), True),
          ("fp8 PV with a table", dict(prec=2, hd=16, Lk=129, pv_fp8=1), True)]


@pytest.mark.parametrize("name,spec,tables", SELECT, ids=[n for n, _, _ in SELECT])
def test_launches_the_predicate_refuses(name, spec, tables):
    """with the hook at 1 these stay where they were: no launch on the new kernel, status and bits the tiled kernel's (the fp8 PV form with a table is
    refused outright, as before, and `out` keeps what it held)"""
    spec = dict(spec)
    prec, hd, Lk = spec.pop("prec"), spec.pop("hd"), spec.pop("Lk")
    B, H = 2, 8
    q, k, v = _operands(B, 33, Lk, H * hd, seed=7)
    if tables:
        spec.update(q_lens=[33, 7], k_lens=[Lk, Lk - 64])
    rc, bits, _ = _pair(prec, hd, q, k, v, want=0, H=H, **spec)
    if "pv_fp8" in spec:
        assert rc != 0 and np.all(bits == G.encode(np.full(1, OUT_FILL, np.float32), G.OP_KIND[prec])[0])
    else:
        assert rc == 0


def test_the_dense_hook_does_not_move_a_masked_launch():
    """the dense kernel's hook at 1 and the new one at its default (the rule): a q_lens launch of B * H = 16 workgroups runs on neither resident kernel"""
    B, H, hd = 2, 8, 32
    q, k, v = _operands(B, 33, 129, H * hd, seed=7)
    rc, _, _, n, d = _hooked(-1, 2, hd, q, k, v, old=1, H=H, q_lens=[33, 7])
    assert rc == 0 and (n, d) == (0, 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the engine: B = 32 (B * H = 256 workgroups: the rule selects the kernel), T = 131, Lp = 65
# ---------------------------------------------------------------------------------------------------------------------------------
SHAPE = (32, 131, 65)
ELENS = [131, 129, 128, 65, 64, 1] + [int(x) for x in np.linspace(2, 130, 26).round()]


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
def test_engine_option_masked_attn_resident(prec, weights, diag):
    import torch
    from ns2vc_amd.engine import Engine
    lib = _lib()[1]
    assert len(ELENS) == SHAPE[0] and min(ELENS) == 1 and max(ELENS) == SHAPE[1]
    x, c, p, t = _inputs("aresl")
    outs, launches, made, loops = {}, {}, {}, {}
    # (masked_attn, masked_attn_resident, attn_resident)
    configs = {"on": (1, 1, 1), "off": (1, 0, 1), "alone": (0, 1, 1), "neither": (0, 0, 1), "no_resident": (1, 1, 0)}
    e = Engine(precision=prec)
    try:
        e.load_state_dict(weights)
        for name, (ma, mar, ar) in configs.items():
            e.set_option("masked_attn", bool(ma))
            e.set_option("masked_attn_resident", bool(mar))
            e.set_option("attn_resident", bool(ar))
            e.prepare(*SHAPE)
            e.set_lengths(ELENS)
            e.set_condition(c, p, None)
            n0 = lib.ns2vc_debug_attn_resident_lens_launches()
            out = torch.empty_like(x)
            e.forward(x, t, out)
            torch.cuda.synchronize()
            made[name] = lib.ns2vc_debug_attn_resident_lens_launches() - n0
            outs[name], launches[name] = out.cpu().numpy(), e.launches()
            if name == "on":                         # captured loop = eager loop, 3 steps
                e.load_sampler("unipc", 3)
                e.set_lengths(ELENS)
                e.set_condition(c, p, None)
                for graph in (True, False):
                    xs = x.clone()
                    e.sample(xs, use_graph=graph)
                    torch.cuda.synchronize()
                    loops[graph] = xs.cpu().numpy()
    finally:
        e.close()

    def same(a, b):
        return np.array_equal(outs[a].view(np.uint32), outs[b].view(np.uint32))
    assert made["on"] > 0 and made["off"] == 0, made
    assert launches["on"] == launches["off"], launches
    assert np.isfinite(outs["on"]).all() and same("on", "off")
    assert np.isfinite(loops[True]).all() and np.array_equal(loops[True].view(np.uint32), loops[False].view(np.uint32))
    assert made["alone"] == 0 and made["neither"] == 0 and same("alone", "neither") and launches["alone"] == launches["neither"], made
    assert made["no_resident"] == 0 and same("no_resident", "off"), made
    diag(f"engine option masked_attn_resident {prec} at B, T, Lp = {SHAPE}, lengths 1 .. 131: {made['on']} launches per forward on the resident kernel's "
         f"masked form with it on, 0 with it off, without masked_attn and without attn_resident; {launches['on']} launches either way, forward "
         f"bit-identical; captured 3-step loop = eager loop with it on")


# ---------------------------------------------------------------------------------------------------------------------------------
# 7. a slot loop
# ---------------------------------------------------------------------------------------------------------------------------------
def test_slot_loop_runs_on_it(weights, diag):
    import torch
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.weights import hash_normal
    lib = _lib()[1]
    dev = torch.device("cuda", 0)
    B, T, Lp = SHAPE
    reqs = [(0, 131, 65, 4), (5, 64, 33, 3), (31, 1, 1, 5)]                    # (slot, frames, prompt frames, steps)

    def tensor(tag, shape):
        return torch.from_numpy(hash_normal(tag, shape)).to(dev)

    def drive(**opts):
        den = Denoiser(weights, precision="fp16", precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None, masked_attn=True, **opts)
        n0 = lib.ns2vc_debug_attn_resident_lens_launches()
        loop = den.open_slots(B, T, Lp)
        for slot, L, lp, steps in reqs:
            loop.admit(slot, tensor(f"sl.c{slot}", (256, L)), tensor(f"sl.p{slot}", (lp, 256)), tensor(f"sl.x{slot}", (100, L)),
                       schedule=dict(solver="unipc", steps=steps, order=2))
        out, caps = {}, None
        while any(it is not None for it in loop.items):
            loop.run(1)
            if caps is None:
                caps = den.engine.graph_captures()
            fin = loop.finished()
            if fin:
                lat = loop.take(fin)
                for k, b in enumerate(fin):
                    out[b] = lat[k].cpu().numpy()
        caps1 = den.engine.graph_captures()
        loop.close()
        torch.cuda.synchronize()
        return out, caps, caps1, lib.ns2vc_debug_attn_resident_lens_launches() - n0

    on, caps0, caps1, made_on = drive(masked_attn_resident=True)
    off, _, _, made_off = drive()
    assert sorted(on) == sorted(off) == [0, 5, 31]
    for slot, L, _, _ in reqs:
        assert np.isfinite(on[slot]).all() and on[slot][:, :L].any() and not on[slot][:, L:].any(), slot
        assert np.array_equal(on[slot].view(np.uint32), off[slot].view(np.uint32)), slot
    assert made_on > 0 and made_off == 0, (made_on, made_off)
    assert caps1 == caps0, (caps0, caps1)
    diag(f"slot loop {SHAPE} fp16 with masked_attn + masked_attn_resident: three requests (131 / 64 / 1 frames) bit-identical to the loop without the "
         f"option; {made_on} launches issued or captured on the resident kernel's masked form; graph captures {caps0} after the first step, {caps1} at the end")
