"""Length-masked batches on the fused kernels (engine option ``masked_fuse``): with the option on, a plan built under per-item lengths keeps
the dense plan's fused launches wherever the kernel masks its own rows -- the tap-sharing conv kernel (epilogue + GroupNorm prologue) and the
8-wave GEMM kernel's epilogue -- and must give what the unfused masked plan gives: every item as if alone, exact zeros past its end.

Families that have no masked kernel form yet and keep today's unfused launches under the option (enumerated by the launch-list test):
the transformer's token-local kernels (row chains, fused feed-forward / GEGLU, LayerNorm by linearity), the attention's result rows, the
narrow GEGLU GEMM on the 4-wave kernel.

Bounds: the constants of tests/test_ragged_gpu.py (TOL, FRAME_TOL, 2.5e-3 sampled, 2e-3 / 1e-6 for a flipped option), imported, not restated."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_ragged_gpu as RG                      # noqa: E402  (the existing constants and helpers: one statement of the bars)
from util import local_errors, rel_l2             # noqa: E402

pytestmark = pytest.mark.gpu
TOL, FRAME_TOL, LENS = RG.TOL, RG.FRAME_TOL, RG.LENS


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


def _engine(prec, weights, fuse=True):
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    e.set_option("masked_fuse", fuse)
    return e


def _check_items_alone(e, prec, x, c, p, t, lens, weights, diag, tag, oracle_upto=263):
    import torch
    from ns2vc_amd.spec import UNetConfig
    from oracle import unet_ref
    T = x.shape[2]
    y = RG._forward(e, x, c, p, t, lens)
    P = None
    worst = (0.0, 0.0)
    for b, L in enumerate(lens):
        assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0, (tag, b, L)
        assert np.isfinite(y[b]).all(), (tag, b)
        if L >= 8:
            ref = RG._forward(e, x[b:b + 1, :, :L].contiguous(), c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), t[b:b + 1].contiguous())
        else:
            if P is None:
                P = {k: torch.from_numpy(v) for k, v in weights.items()}
            ref = unet_ref.denoiser(P, UNetConfig(), x[b:b + 1, :, :L].cpu(), c[b:b + 1, :, :L].cpu(), p[b:b + 1].cpu(), None, t[b:b + 1].cpu()).numpy()
        m = local_errors(y[b:b + 1, :, :L], ref)
        worst = (max(worst[0], m["item"]), max(worst[1], m["frame"]))
        diag(f"fused ragged forward {tag} {prec} L={L}: item {m['item']:.2e} frame {m['frame']:.2e} chan {m['chan']:.2e}")
        if prec != "bf16":
            tol = TOL[prec] * (2 if (L < 8 and prec != "fp32") else 1)
            assert m["item"] < tol, (tag, L, m)
            assert m["frame"] < FRAME_TOL[prec] and m["chan"] < FRAME_TOL[prec], (tag, L, m)
        if prec == "fp32" and 8 <= L <= oracle_upto:
            if P is None:
                P = {k: torch.from_numpy(v) for k, v in weights.items()}
            ro = unet_ref.denoiser(P, UNetConfig(), x[b:b + 1, :, :L].cpu(), c[b:b + 1, :, :L].cpu(), p[b:b + 1].cpu(), None, t[b:b + 1].cpu()).numpy()
            mo = local_errors(y[b:b + 1, :, :L], ro)
            diag(f"fused ragged forward {tag} fp32 L={L} vs oracle alone: item {mo['item']:.2e} frame {mo['frame']:.2e}")
            assert mo["item"] < TOL["fp32"] and mo["frame"] < FRAME_TOL["fp32"] and mo["chan"] < FRAME_TOL["fp32"], (tag, L, mo)
    diag(f"fused ragged forward {tag} {prec}: worst item {worst[0]:.2e}, worst frame {worst[1]:.2e}")
    return y


@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_fused_forward_padded_batch_equals_items_alone(prec, weights, diag):
    """the cases of test_forward_padded_batch_equals_items_alone with masked_fuse = 1: same LENS, caller padding 7.0 / -3.0, same bars"""
    T, Lp = max(LENS), 40
    x, c, p, t = RG._inputs(len(LENS), T, Lp, "rg1")
    for b, L in enumerate(LENS):
        x[b, :, L:] = 7.0
        c[b, :, L:] = -3.0
    e = _engine(prec, weights)
    try:
        _check_items_alone(e, prec, x, c, p, t, LENS, weights, diag, "LENS")
    finally:
        e.close()


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_fused_item_end_at_every_tile_position(prec, weights, diag):
    """an item's end at every position of a 126-row conv tile (padded row space: item b starts at b * (T + 1)), lengths on both sides of the
    64 / 66-frame planner thresholds of the deep levels (125 / 127 / 129 / 131 / 263 of the seam tests), and one item with L = T"""
    T, Lp = 263, 40
    lens = [263, 131, 129, 127, 125, 262, 200, 137] + [138 + 9 * k for k in range(14)]      # ends 138 .. 255: with the 8 above, residues spread over the tile
    x, c, p, t = RG._inputs(len(lens), T, Lp, "rf2")
    for b, L in enumerate(lens):
        x[b, :, L:] = 7.0
        c[b, :, L:] = -3.0
    e = _engine(prec, weights)
    try:
        _check_items_alone(e, prec, x, c, p, t, lens, weights, diag, "tile", oracle_upto=131)
    finally:
        e.close()
    # EVERY position of the item's end inside a 126-row tile (126 consecutive lengths), fused against the unfused masked plan on the same inputs,
    # per item / frame / channel under the item-alone bars (a wrong boundary frame is O(1) there); the unfused plan is itself held item-alone
    # to the same bars by tests/test_ragged_gpu.py, and the two plans differ by summation order only
    B, T2 = 2, 300
    x, c, p, t = RG._inputs(B, T2, Lp, "rf3")
    e, f = _engine(prec, weights), _engine(prec, weights, fuse=False)
    try:
        worst = (0.0, 0.0, 0.0)
        for L in range(150, 150 + 126):
            ya = RG._forward(e, x, c, p, t, [L, T2])
            yb = RG._forward(f, x, c, p, t, [L, T2])
            assert float(np.abs(ya[0, :, L:]).max()) == 0.0, L
            for b, Lb in ((0, L), (1, T2)):
                m = local_errors(ya[b:b + 1, :, :Lb], yb[b:b + 1, :, :Lb])
                worst = (max(worst[0], m["item"]), max(worst[1], m["frame"]), max(worst[2], m["chan"]))
                assert m["item"] < TOL[prec], (L, b, m)
                assert m["frame"] < FRAME_TOL[prec] and m["chan"] < FRAME_TOL[prec], (L, b, m)
        diag(f"fused vs unfused masked plan, item end at each of 126 tile positions, {prec}: worst item {worst[0]:.2e} frame {worst[1]:.2e} chan {worst[2]:.2e}")
    finally:
        e.close()
        f.close()


@pytest.mark.parametrize("solver,steps,tail", [("unipc", 20, 0), ("dpmsolver++", 50, 3)])
def test_fused_sampled_padded_batch_equals_items_alone(solver, steps, tail, weights, diag):
    """test_sampled_padded_batch_equals_items_alone with Denoiser(masked_fuse=True) (bar 2.5e-3); also self-check and LayerNorm guard quiet"""
    import torch
    from ns2vc_amd.pipeline import Denoiser
    lens = [300, 211, 97, 64, 9]
    T, Lp = max(lens), 40
    _, c, p, _ = RG._inputs(len(lens), T, Lp, "rg3")
    noise = torch.zeros(len(lens), 100, T, device=c.device)
    for b, L in enumerate(lens):
        noise[b, :, :L] = torch.randn((100, L), generator=torch.Generator().manual_seed(b)).to(c.device)
    den = Denoiser(weights, precision="fp16", masked_fuse=True)
    outs = {}
    for g in (True, False):
        outs[g] = den.sample(c, p, None, noise, solver=solver, steps=steps, use_graph=g, tail_fp32=tail, lengths=lens).cpu().numpy()
    assert not den.serving_fp32 and not den._ln_switched
    worst = 0.0
    for b, L in enumerate(lens):
        assert float(np.abs(outs[True][b, :, L:]).max() if L < T else 0.0) == 0.0
        one = den.sample(c[b:b + 1, :, :L].contiguous(), p[b:b + 1].contiguous(), None, noise[b:b + 1, :, :L].contiguous(), solver=solver, steps=steps,
                         use_graph=True, tail_fp32=tail).cpu().numpy()
        worst = max(worst, rel_l2(outs[True][b, :, :L], one[0]))
        assert rel_l2(outs[False][b, :, :L], one[0]) < 2.5e-3
    diag(f"fused ragged sampling {solver}-{steps} fp16 (fp32 tail {tail}): worst item vs alone {worst:.2e}; graph vs eager {rel_l2(outs[True], outs[False]):.2e}")
    assert worst < 2.5e-3


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_fused_vs_unfused_masked_plan(prec, weights, diag):
    """same inputs, option on vs off: the two plans differ by summation order only"""
    import torch
    lens = [300, 131, 66, 64, 33, 9]
    B, T, Lp = len(lens), 300, 40
    x, c, p, t = RG._inputs(B, T, Lp, "rg5")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(5)).to(c.device)
    res = {}
    for fuse in (False, True):
        e = _engine(prec, weights, fuse)
        try:
            res[fuse] = (RG._forward(e, x, c, p, t, lens), RG._sample(e, c, p, xT, lens, True), RG._sample(e, c, p, xT, lens, False))
        finally:
            e.close()
    e1, eg, ee = (rel_l2(res[True][i], res[False][i]) for i in range(3))
    gve = rel_l2(res[True][1], res[True][2])
    diag(f"masked_fuse on vs off under lengths {prec}: forward {e1:.2e}, sampled graph {eg:.2e} eager {ee:.2e}; fused graph vs eager {gve:.2e}")
    assert e1 < 2e-3 and eg < 2e-3 and ee < 2e-3
    assert gve < 1e-6
    if prec == "fp32":
        assert e1 < TOL["fp32"]
    for y in res[True]:
        for b, L in enumerate(lens):
            assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0


def _names(e):
    return [o[0] for o in e.op_info(0)]


def _block_of(name):
    """'down_blocks.1.attentions.0' for a launch of that transformer block, else None"""
    k = name.find(".attentions.")
    return None if k < 0 else name[:k] + ".attentions." + name[k + len(".attentions."):].split(".")[0]


@pytest.mark.parametrize("prec", ["fp16", "fp32"])
def test_fused_launch_list(prec, weights, diag):
    """The plan under lengths with the option on, launch by launch.
    Outside the transformer blocks it IS the dense plan's list, name for name and in order (every resnet conv and conv_out with its
    `[+norm]` prologue where the dense plan has one, the same `gn_stats` passes and no other), plus one `upsample.nearest` per upsampler.
    Inside a transformer block -- families 3 and 4 fell back in this change -- the list is exactly the one written out below: no other
    launch, no further mask_rows / gn_partial.  So: launches(fused) = launches(dense) + the enumerated exceptions, an equality."""
    B, T, Lp = 4, 300, 40          # levels of 300 / 150 / 75 / 38 frames: the last one below the 64 / 66-frame thresholds
    lens = [300, 200, 131, 70]
    e = _engine(prec, weights)
    try:
        e.prepare(B, T, Lp)
        dense = _names(e)
        e.set_lengths(lens)
        fused = _names(e)
        e.set_lengths(None)
        assert _names(e) == dense
        e.set_option("masked_fuse", False)
        e.prepare(B, T, Lp)
        e.set_lengths(lens)
        unfused = _names(e)
    finally:
        e.close()
    # ---- outside the transformer blocks: the dense list + the materialised upsampling ("stays as it is")
    nearest = [n for n in fused if n.endswith(".upsample.nearest")]
    assert len(nearest) == len([n for n in dense if n.endswith(".upsample")]) > 0
    f_out = [n for n in fused if _block_of(n) is None and not n.endswith(".upsample.nearest")]
    d_out = [n for n in dense if _block_of(n) is None]
    assert f_out == d_out, [(a, b) for a, b in zip(f_out, d_out) if a != b][:8]
    n_pro = len([n for n in d_out if "[+norm]" in n])
    assert n_pro > 0 and len([n for n in f_out if "[+norm]" in n]) == n_pro          # every resnet / conv_out prologue of the dense plan
    assert not [n for n in f_out if n.endswith(".mask")]                              # no mask_rows behind any conv, down- or upsampling conv
    # ---- inside a transformer block: the fallback of families 3 (token-local kernels) and 4 (attention result rows), by name
    blocks = sorted({_block_of(n) for n in fused if _block_of(n)})
    assert blocks == sorted({_block_of(n) for n in dense if _block_of(n)}) and blocks
    extra = len(nearest)
    for P in blocks:
        t = P + ".transformer_blocks.0"
        got = [n for n in fused if _block_of(n) == P]
        was = [n for n in dense if _block_of(n) == P]
        want = [P + ".norm.gn_apply", P + ".proj_in", t + ".norm1", t + ".attn1.qkv", t + ".attn1.sdpa", t + ".attn1.sdpa.mask",
                t + ".attn1.to_out", t + ".norm2", t + ".attn2.to_q", t + ".attn2.sdpa", t + ".attn2.sdpa.mask", t + ".attn2.to_out",
                t + ".norm3", t + ".ff.geglu", P + ".ff.out+proj_out"]
        if P + ".norm.gn_stats" in was:                      # (a level below 64 frames: the dense plan has the statistics pass too)
            want.insert(0, P + ".norm.gn_stats")
        if t + ".ff.geglu.mask" in got:                      # the narrow GEGLU GEMM (dim 128) runs on the 4-wave kernel: no masked epilogue
            want.insert(want.index(t + ".ff.geglu") + 1, t + ".ff.geglu.mask")
        assert got == want, (P, got, want)
        extra += len(got) - len(was)
    assert len(fused) == len(dense) + extra
    stats = lambda names: sorted(n for n in names if n.endswith(".gn_stats"))
    assert stats(fused) == stats(dense)
    diag(f"launches {prec} B={B} T={T}: dense {len(dense)}, masked unfused {len(unfused)}, masked fused {len(fused)} = dense + {extra} "
         f"({len(nearest)} upsample.nearest, the rest the transformer fallback of {len(blocks)} blocks); [+norm] prologues {n_pro} as dense; "
         f"gn_stats {len(stats(fused))} as dense, unfused plan {len(stats(unfused))}")
    assert len(fused) < len(unfused) and not [n for n in unfused if "[+norm]" in n]


def test_fused_graph_captured_under_other_lengths(weights, diag):
    import torch
    B, T, Lp = 4, 256, 40
    _, c, p, _ = RG._inputs(B, T, Lp, "rg4")
    xT = torch.randn((B, 100, T), generator=torch.Generator().manual_seed(3)).to(c.device)
    A, Bl = [256, 200, 100, 9], [17, 256, 255, 64]
    e = _engine("fp16", weights)
    try:
        e.prepare(B, T, Lp)
        e.load_sampler("unipc", 10)
        e.set_lengths(None)
        e.set_condition(c, p, None)
        xd0 = xT.clone()
        e.sample(xd0, use_graph=True)
        e.set_lengths(A)
        e.set_condition(c, p, None)
        xa = xT.clone()
        e.sample(xa, use_graph=True)          # captured under A
        e.set_lengths(Bl)
        e.set_condition(c, p, None)
        xg = xT.clone()
        e.sample(xg, use_graph=True)          # the same graph replayed under B
        xe = xT.clone()
        e.sample(xe, use_graph=False)
        e.set_lengths(None)                   # dense again: bit for bit what it was
        e.set_condition(c, p, None)
        xd1 = xT.clone()
        e.sample(xd1, use_graph=True)
        torch.cuda.synchronize()
    finally:
        e.close()
    xg, xe = xg.cpu().numpy(), xe.cpu().numpy()
    assert np.array_equal(xg, xe)
    assert np.array_equal(xd0.cpu().numpy(), xd1.cpu().numpy())
    for b, L in enumerate(Bl):
        assert float(np.abs(xg[b, :, L:]).max() if L < T else 0.0) == 0.0


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel level: ns2vc_k_gemm with GemmArgs.lens against numpy fp64, padded rows of the inputs poisoned, guard bands around every output
# ---------------------------------------------------------------------------------------------------------------------------------
def _lib():
    from ns2vc_amd import _lib as L
    return L, L.load()


def _dev(a, dtype):
    L, lib = _lib()
    a = np.ascontiguousarray(a, dtype=dtype)
    p = C.c_void_p()
    L.check(lib.ns2vc_dev_malloc(C.byref(p), a.nbytes), "malloc")
    L.check(lib.ns2vc_memcpy_h2d(p, a.ctypes.data, a.nbytes), "h2d")
    return p


def _pack(w, prec):
    L, lib = _lib()
    w = np.ascontiguousarray(w, dtype=np.float32)
    p = C.c_void_p()
    L.check(lib.ns2vc_pack_weight(w.ctypes.data, w.shape[0], w.shape[1], prec, C.byref(p)), "pack_weight")
    return p


def _poison_rows(a, B, T, lens, value):
    """rows t >= lens[b] of a (B*T, C) array -> value"""
    a = a.copy().reshape(B, T, -1)
    for b, L in enumerate(lens):
        a[b, L:] = value
    return a.reshape(B * T, -1)


def _stats_ref(y, B, T, lens):
    """(sum, sumsq) per item and 16-channel block over the valid rows, fp64"""
    N = y.shape[1]
    y = y.reshape(B, T, N // 16, 16).astype(np.float64)
    out = np.zeros((B, N // 16, 2))
    for b, L in enumerate(lens):
        out[b, :, 0] = y[b, :L].sum(axis=(0, 2))
        out[b, :, 1] = (y[b, :L] ** 2).sum(axis=(0, 2))
    return out


def _conv3(x, w, B, T, C, stride=1):
    """x (B*T, C) channels-last, w (N, 3*C) with k = tap * C + c, zero padding 1 -> (B*Tout, N) in fp64"""
    x = x.reshape(B, T, C).astype(np.float64)
    xp = np.zeros((B, T + 2, C))
    xp[:, 1:T + 1] = x
    Tout = (T + stride - 1) // stride
    w3 = w.reshape(-1, 3, C).astype(np.float64)
    out = np.zeros((B, Tout, w.shape[0]))
    for k in range(3):
        out += np.einsum("btc,nc->btn", xp[:, k:k + stride * Tout:stride][:, :Tout], w3[:, k])
    return out.reshape(B * Tout, -1)


@pytest.mark.parametrize("fill", ["nan", "inf"])
@pytest.mark.parametrize("case", ["conv3ts", "conv3ts_n64", "gemm4_stride2", "gemm4_linear", "gemm4_conv3"])
def test_kernel_masked_epilogue(case, fill, diag):
    """zero rows past an item's end (fp32 stream and operand copy), bias / residual not added there, int64 statistics over the valid rows only;
    the padded rows of the residual (and, for the token-local GEMM, of the operand rows) hold NaN / Inf; guard bands intact"""
    import guard as G
    L, lib = _lib()
    bk = G.DeviceBackend()
    rng = np.random.default_rng(7)
    B, C0, prec = 3, 64, 0
    bad = np.nan if fill == "nan" else np.inf
    if case == "gemm4_stride2":
        Tin, taps, tmode, N = 161, 3, 1, 128
        Tout = (Tin + 1) // 2
        lens_in = [161, 100, 67]
        lens = [(v + 1) // 2 for v in lens_in]
    elif case == "gemm4_linear":
        Tin = Tout = 97
        taps, tmode, N, lens = 1, 0, 128, [97, 64, 1]
        lens_in = lens
    else:
        Tin = Tout = 131
        taps, tmode, N = 3, 0, (64 if case == "conv3ts_n64" else 128 if case == "gemm4_conv3" else 256)
        lens = lens_in = [131, 126, 66]
    x = rng.standard_normal((B * Tin, C0)).astype(np.float32)
    x = _poison_rows(x, B, Tin, lens_in, 0.0)                       # the row invariant: an operand tensor's padded rows are zero ...
    if taps == 1:
        x = _poison_rows(x, B, Tin, lens_in, bad)                   # ... token-local: whatever they hold must stay in their own (zeroed) row
    w = (rng.standard_normal((N, taps * C0)) / np.sqrt(taps * C0)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    res = _poison_rows(rng.standard_normal((B * Tout, N)).astype(np.float32), B, Tout, lens, bad)
    xz = _poison_rows(x, B, Tin, lens_in, 0.0)
    ref = (_conv3(xz, w, B, Tin, C0, 2 if tmode == 1 else 1) if taps == 3 else xz.astype(np.float64) @ w.astype(np.float64).T)
    ref = ref + bias[None] + _poison_rows(res, B, Tout, lens, 0.0)
    ref = _poison_rows(ref, B, Tout, lens, 0.0)
    g_x = G.Guarded(bk, B * Tin, C0, "f32", data=x, fill=fill, name="a0")
    g_res = G.Guarded(bk, B * Tout, N, "f32", data=res, fill=fill, name="res")
    g_of = G.Guarded(bk, B * Tout, N, "f32", ld=N + 8, fill=fill, name="out_f32")
    g_oo = G.Guarded(bk, B * Tout, N, "f32", fill=fill, name="out_op")
    g_st = G.Guarded(bk, B, (N // 16) * 2, "i64", data=np.zeros((B, (N // 16) * 2), dtype=np.int64), fill=fill, name="stats")
    d_w, d_b, d_l = _pack(w, prec), _dev(bias, np.float32), _dev(lens, np.int32)
    a = L.GemmArgs()
    a.a0, a.lda0, a.c0 = g_x.ptr, C0, C0
    a.B, a.Tin, a.Tout, a.M, a.taps, a.tmode = B, Tin, Tout, B * Tout, taps, tmode
    a.w, a.K, a.N, a.bias = d_w, taps * C0, N, d_b
    a.res, a.ldres = g_res.ptr, N
    a.out_f32, a.ldo_f32, a.out_op, a.ldo_op = g_of.ptr, N + 8, g_oo.ptr, N
    a.stats = g_st.ptr
    a.lens = d_l
    a.algo = 1 if case == "gemm4_conv3" else 0          # (1: the k = 3 / stride-1 conv on the 8-wave kernel instead of the tap-sharing one)
    try:
        L.check(lib.ns2vc_k_gemm(C.byref(a), prec, None), "k_gemm")
        L.check(lib.ns2vc_dev_sync(), "sync")
        y, yo = g_of.read().astype(np.float64), g_oo.read().astype(np.float64)
        st = g_st.read().astype(np.float64).reshape(B, N // 16, 2)
        viol = sum((g.violations() for g in (g_x, g_res, g_of, g_oo, g_st)), [])
    finally:
        for p in (d_w, d_b, d_l):
            lib.ns2vc_dev_free(p)
        for g in (g_x, g_res, g_of, g_oo, g_st):
            g.free()
    assert not viol, viol
    assert np.isfinite(y).all() and np.isfinite(yo).all()
    pad = _poison_rows(np.ones_like(y), B, Tout, lens, 0.0) == 0.0
    assert np.all(y[pad] == 0.0) and np.all(yo[pad] == 0.0)
    err = np.abs(y - ref).max() / np.abs(ref).max()
    sref = _stats_ref(ref, B, Tout, lens)
    s_got = np.stack([st[..., 0] / 2.0 ** 28, st[..., 1] / 2.0 ** 16], axis=-1)
    serr = np.abs(s_got - sref).max() / np.abs(sref).max()
    diag(f"masked epilogue {case} [{fill}]: result {err:.2e}, statistics {serr:.2e}")
    # fp32 operands on the exact-fp32 MFMA, K <= 192 products: 1e-5 relative to the largest element is ~50 ulps of headroom over sqrt(K) * 2^-24;
    # the statistics are fp32 partial sums of <= 64 rows x 4 columns per lane (2^-24 * sqrt(256) ~ 1e-6) + the 2^-16 fixed-point step of the squares
    assert err < 1e-5 and np.array_equal(y, yo)
    assert serr < 1e-4


@pytest.mark.parametrize("fill", ["nan", "inf"])
@pytest.mark.parametrize("case", ["one", "concat"])
def test_kernel_masked_prologue(case, fill, diag):
    """GroupNorm prologue of the tap-sharing conv kernel under lengths: per-item divisor L_b * Cg, zero operand rows past L_b (a0 and gnp_raw),
    one source and a concat of two; the padded rows of the fp32 sources hold NaN / Inf"""
    import guard as G
    L, lib = _lib()
    bk = G.DeviceBackend()
    rng = np.random.default_rng(11)
    B, T, N, Gn, prec = 3, 131, 256, 8, 0
    lens = [131, 127, 66]
    bad = np.nan if fill == "nan" else np.inf
    c0, c1 = (128, 0) if case == "one" else (128, 128)
    Ct = c0 + c1
    xs = [(rng.standard_normal((B * T, cc)) * 1.5 + 0.3).astype(np.float32) for cc in (c0, c1) if cc]
    xcat = np.concatenate(xs, axis=1)
    gamma, beta = rng.standard_normal(Ct).astype(np.float32), rng.standard_normal(Ct).astype(np.float32)
    w = (rng.standard_normal((N, 3 * Ct)) / np.sqrt(3 * Ct)).astype(np.float32)
    # reference: GroupNorm over the item's own L_b frames, SiLU, zero rows past L_b, then the conv with its zero padding
    xr = xcat.reshape(B, T, Gn, Ct // Gn).astype(np.float64)
    a_ref = np.zeros((B, T, Ct))
    for b, Lb in enumerate(lens):
        v = xr[b, :Lb]
        mu, var = v.mean(axis=(0, 2), keepdims=True), v.var(axis=(0, 2), keepdims=True)
        n = ((v - mu) / np.sqrt(var + 1e-5)).reshape(Lb, Ct) * gamma[None] + beta[None]
        a_ref[b, :Lb] = n / (1.0 + np.exp(-n))
    a_ref = a_ref.reshape(B * T, Ct)
    y_ref = _poison_rows(_conv3(a_ref, w, B, T, Ct), B, T, lens, 0.0)
    stats = []
    for xx in xs:
        s = _stats_ref(xx, B, T, lens)
        stats.append(np.stack([np.rint(s[..., 0] * 2.0 ** 28), np.rint(s[..., 1] * 2.0 ** 16)], axis=-1).astype(np.int64))
    g_xs = [G.Guarded(bk, B * T, xx.shape[1], "f32", data=_poison_rows(xx, B, T, lens, bad), fill=fill, name=f"gnp_x{i}") for i, xx in enumerate(xs)]
    g_a0 = G.Guarded(bk, B * T, Ct, "f32", fill=fill, name="a0")
    g_raw = G.Guarded(bk, B * T, Ct, "f32", fill=fill, name="gnp_raw")
    g_of = G.Guarded(bk, B * T, N, "f32", fill=fill, name="out_f32")
    d = [_pack(w, prec), _dev(gamma, np.float32), _dev(beta, np.float32), _dev(lens, np.int32)] + [_dev(s, np.int64) for s in stats]
    a = L.GemmArgs()
    a.a0, a.lda0, a.c0 = g_a0.ptr, Ct, Ct
    a.B, a.Tin, a.Tout, a.M, a.taps, a.tmode = B, T, T, B * T, 3, 0
    a.w, a.K, a.N = d[0], 3 * Ct, N
    a.out_f32, a.ldo_f32 = g_of.ptr, N
    a.gnp_x, a.gnp_ldx, a.gnp_stats, a.gnp_gamma, a.gnp_beta = g_xs[0].ptr, c0, d[4], d[1], d[2]
    a.gnp_eps, a.gnp_G, a.gnp_silu = 1e-5, Gn, 1
    a.gnp_raw = g_raw.ptr
    if c1:
        a.gnp_x1, a.gnp_ldx1, a.gnp_c1, a.gnp_stats1 = g_xs[1].ptr, c1, c1, d[5]
    a.algo = 2
    a.lens = d[3]
    try:
        L.check(lib.ns2vc_k_gemm(C.byref(a), prec, None), "k_gemm")
        L.check(lib.ns2vc_dev_sync(), "sync")
        a0, raw, y = g_a0.read().astype(np.float64), g_raw.read().astype(np.float64), g_of.read().astype(np.float64)
        viol = sum((g.violations() for g in g_xs + [g_a0, g_raw, g_of]), [])
    finally:
        for p in d:
            lib.ns2vc_dev_free(p)
        for g in g_xs + [g_a0, g_raw, g_of]:
            g.free()
    assert not viol, viol
    for name, v in (("a0", a0), ("gnp_raw", raw), ("out", y)):
        assert np.isfinite(v).all(), name
        assert np.all(v[_poison_rows(np.ones_like(v), B, T, lens, 0.0) == 0.0] == 0.0), name
    ea = np.abs(a0 - a_ref).max() / np.abs(a_ref).max()
    er = np.abs(raw - _poison_rows(xcat, B, T, lens, 0.0)).max()
    ey = np.abs(y - y_ref).max() / np.abs(y_ref).max()
    diag(f"masked prologue {case} [{fill}]: operand rows {ea:.2e}, raw copy {er:.2e}, conv result {ey:.2e}")
    # fp32 throughout; the kernel's SiLU uses the hardware exp / reciprocal (1 ulp-class, ~1e-6 relative) and an rsqrt + one Newton step
    assert ea < 1e-5 and er == 0.0 and ey < 2e-5


def test_kernel_masked_pair_prologue(diag):
    """gnp_pair (16-bit, conv_out's form): both planes of the hi + lo operand pair are zero past an item's end, the result too"""
    import guard as G
    L, lib = _lib()
    bk = G.DeviceBackend()
    rng = np.random.default_rng(13)
    B, T, Cn, N, Gn, prec = 2, 140, 128, 128, 8, 2
    lens = [140, 71]
    x = (rng.standard_normal((B * T, Cn)) + 0.2).astype(np.float32)
    gamma, beta = rng.standard_normal(Cn).astype(np.float32), rng.standard_normal(Cn).astype(np.float32)
    wc = (rng.standard_normal((N, 3, Cn)) / np.sqrt(3 * Cn)).astype(np.float32)
    whi = wc.astype(np.float16).astype(np.float32)
    wlo = wc - whi
    # K layout of the launch: per tap [hi(C) | lo(C) | hi(C)] activations against [hi(w) | hi(w) | lo(w)]
    w = np.concatenate([whi, whi, wlo], axis=2).reshape(N, 9 * Cn)
    xr = x.reshape(B, T, Gn, Cn // Gn).astype(np.float64)
    a_ref = np.zeros((B, T, Cn))
    for b, Lb in enumerate(lens):
        v = xr[b, :Lb]
        n = ((v - v.mean(axis=(0, 2), keepdims=True)) / np.sqrt(v.var(axis=(0, 2), keepdims=True) + 1e-5)).reshape(Lb, Cn) * gamma[None] + beta[None]
        a_ref[b, :Lb] = n / (1.0 + np.exp(-n))
    y_ref = _poison_rows(_conv3(a_ref.reshape(B * T, Cn), wc.reshape(N, 3 * Cn), B, T, Cn), B, T, lens, 0.0)
    s = _stats_ref(x, B, T, lens)
    st = np.stack([np.rint(s[..., 0] * 2.0 ** 28), np.rint(s[..., 1] * 2.0 ** 16)], axis=-1).astype(np.int64)
    g_x = G.Guarded(bk, B * T, Cn, "f32", data=_poison_rows(x, B, T, lens, np.nan), name="gnp_x")
    g_a0 = G.Guarded(bk, B * T, 2 * Cn, "f16", name="a0")
    g_of = G.Guarded(bk, B * T, N, "f32", name="out_f32")
    d = [_pack(w, prec), _dev(gamma, np.float32), _dev(beta, np.float32), _dev(lens, np.int32), _dev(st, np.int64)]
    a = L.GemmArgs()
    a.a0, a.lda0, a.c0 = g_a0.ptr, 2 * Cn, 2 * Cn
    a.a1, a.lda1, a.c1 = g_a0.ptr, 2 * Cn, Cn
    a.B, a.Tin, a.Tout, a.M, a.taps, a.tmode = B, T, T, B * T, 3, 0
    a.w, a.K, a.N = d[0], 9 * Cn, N
    a.out_f32, a.ldo_f32 = g_of.ptr, N
    a.gnp_x, a.gnp_ldx, a.gnp_stats, a.gnp_gamma, a.gnp_beta = g_x.ptr, Cn, d[4], d[1], d[2]
    a.gnp_eps, a.gnp_G, a.gnp_silu, a.gnp_pair = 1e-5, Gn, 1, 1
    a.algo = 2
    a.lens = d[3]
    try:
        L.check(lib.ns2vc_k_gemm(C.byref(a), prec, None), "k_gemm")
        L.check(lib.ns2vc_dev_sync(), "sync")
        a0, y = g_a0.read().astype(np.float64), g_of.read().astype(np.float64)
        viol = sum((g.violations() for g in (g_x, g_a0, g_of)), [])
    finally:
        for p in d:
            lib.ns2vc_dev_free(p)
        for g in (g_x, g_a0, g_of):
            g.free()
    assert not viol, viol
    assert np.isfinite(a0).all() and np.isfinite(y).all()
    assert np.all(a0[_poison_rows(np.ones_like(a0), B, T, lens, 0.0) == 0.0] == 0.0)
    assert np.all(y[_poison_rows(np.ones_like(y), B, T, lens, 0.0) == 0.0] == 0.0)
    ea = np.abs(a0[:, :Cn] + a0[:, Cn:] - a_ref.reshape(B * T, Cn)).max() / np.abs(a_ref).max()
    ey = np.abs(y - y_ref).max() / np.abs(y_ref).max()
    diag(f"masked pair prologue fp16: hi + lo rows {ea:.2e}, conv result {ey:.2e}")
    # a hi + lo fp16 pair carries ~2^-21 relative (22 bits of significand between the two planes); the product form drops lo(x) * lo(w): 2^-22
    assert ea < 4e-6 and ey < 2e-5


def test_kernel_lens_refused_where_no_masked_kernel(diag):
    """a launch that has no masked form is an error, never a silent unmasked run: a LayerNorm-statistics producer under lens"""
    L, lib = _lib()
    B, T, C0, N = 2, 80, 128, 128
    x, w = np.zeros((B * T, C0), np.float32), np.zeros((N, C0), np.float32)
    d = [_dev(x, np.float32), _pack(w, 0), _dev([80, 40], np.int32), _dev(np.zeros((B * T, N), np.float32), np.float32), _dev(np.zeros((B * T, 2, 2), np.float32), np.float32)]
    a = L.GemmArgs()
    a.a0, a.lda0, a.c0, a.B, a.Tin, a.Tout, a.M, a.taps = d[0], C0, C0, B, T, T, B * T, 1
    a.w, a.K, a.N, a.out_f32, a.ldo_f32, a.rowstats, a.lens = d[1], C0, N, d[3], N, d[4], d[2]
    try:
        assert lib.ns2vc_k_gemm(C.byref(a), 0, None) != 0
        lib.ns2vc_dev_sync()
    finally:
        for p in d:
            lib.ns2vc_dev_free(p)
