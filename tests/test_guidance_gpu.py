"""Classifier-free guidance on the MI355X: the guided solver update alone (ns2vc_k_solver_update_guided) against the fp64 recurrence and on
guarded tensors, the guided loop against the oracle, its identities (scale 1, equal conditions, batch independence), the captured graph under
new scales, the stochastic / ragged loop, the hand-off to an fp32 tail, and ``Denoiser.denoise`` guided."""
import os

import numpy as np
import pytest

from util import TOL_SOLVER, bf16_round, f16_round, fmt_local, local_errors, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_TOL = 1e-5              # tests/test_engine_gpu.py: a forward of the fp32 engine
FP32_SAMPLED_TOL = 5e-5      # tests/test_engine_gpu.py: sampled latents of the fp32 engine
FP32_LOCAL_TOL = 2e-4        # per frame / channel of a sampled latent (tests/test_solvers_gpu.py)
PARITY_TOL = 1e-3            # the project's bar for the 16-bit engine
PREC = {"fp32": 0, "bf16": 1, "fp16": 2}
LD, NC = 128, 100
# (n, T): item boundaries inside one thread block | 17 000 rows against the 16 384 one sweep of the capped 2048-block grid covers, so the
# stride loop's second pass lands in the last item, which has its own scale
SHAPES = {"small": (3, 5), "big": (17, 1000)}


def _case(shape):
    n, T = SHAPES[shape]
    rng = np.random.default_rng(n * 1000 + T)
    if shape == "small":
        scales, lens = np.array([0.0, 1.0, 2.5], np.float32), np.array([5, 3, 1], np.int32)
    else:
        scales = rng.uniform(-1.0, 8.0, n).astype(np.float32)
        scales[5], scales[-1] = 1.0, 6.25
        lens = rng.integers(1, T + 1, n).astype(np.int32)
        lens[-1] = T
    rows = n * T
    st = {"x0": rng.standard_normal((2 * rows, LD)).astype(np.float32), "xe": rng.standard_normal((2 * rows, LD)).astype(np.float32)}
    for k in ("xbar", "d1", "mprev", "mprev2"):      # second halves: a sentinel the kernel must leave alone
        st[k] = rng.standard_normal((2 * rows, LD)).astype(np.float32)
    seeds = (np.arange(n, dtype=np.uint64) + np.uint64(7)) * np.uint64(0x9E3779B97F4A7C15)
    return n, T, rows, scales, lens, seeds, st


def _table(form):
    from ns2vc_amd import schedule as S
    if form == "noise":
        t = S.build_table("ddim", 8, S.linear_betas(1000, np.float64), eta=1.0)
        step = 3
        assert t.coef[step, 9] != 0
    else:
        t = S.build_table("unipc", 10, order=3, skip_type="logSNR")
        step = 4
        assert t.coef[step, 10] != 0 and t.coef[step, 11] != 0
    return t, step


def _reference(form, table, step, n, T, rows, scales, lens, seeds, st):
    """guided_x0 then the fp64 recurrence row of tests/test_solvers_gpu.py (+ the host noise of ns2vc_amd/noise.py on a stochastic row)"""
    from ns2vc_amd import noise as N
    from ns2vc_amd import schedule as S
    from test_solvers_gpu import _update_numpy
    f64 = {k: v.astype(np.float64) for k, v in st.items()}
    x0g = S.guided_x0(f64["x0"][:rows].reshape(n, T, LD), f64["x0"][rows:].reshape(n, T, LD), scales.astype(np.float64)).reshape(rows, LD)
    row = table.coef[step]
    ne, nb, nd, m = _update_numpy(row, x0g, f64["xe"][:rows], f64["xbar"][:rows], f64["d1"][:rows], f64["mprev"][:rows],
                                  f64["mprev2"][:rows] if form == "h2" else None)
    if form == "noise":
        z = np.zeros((n, T, LD))
        z[:, :, :NC] = N.gauss(seeds, step, NC, T, [int(v) for v in lens]).transpose(0, 2, 1)
        nb = nb + float(row[9]) * z.reshape(rows, LD)
        ne = nb - float(row[8]) * nd
    return ne, nb, nd, m


def _launch(lib, prec, form, table, step, n, T, rows, scales, lens, seeds, ptr, n_half=None, ld=LD, T_arg=None):
    """ptr: {name: device pointer} of x0, xe, xe_op, xbar, d1, mprev, mprev2, coef, step, scale, seeds, lens"""
    return lib.ns2vc_k_solver_update_guided(ptr["coef"], ptr["step"], ptr["x0"], ptr["xe"], ptr["xe_op"], PREC[prec], ptr["xbar"], ptr["d1"], ptr["mprev"],
                                            ptr["mprev2"] if form == "h2" else None, rows * LD if n_half is None else n_half, ld, ptr["scale"],
                                            T if T_arg is None else T_arg, ptr["seeds"] if form == "noise" else None,
                                            ptr["lens"] if form == "noise" else None, NC, None)


def _check_outputs(prec, form, got, op, ref, rows, st, diag, label):
    ne, nb, nd, m = ref
    errs = {"xe": rel_l2(got["xe"][:rows], ne), "xbar": rel_l2(got["xbar"][:rows], nb), "d1": rel_l2(got["d1"][:rows], nd),
            "mprev": rel_l2(got["mprev"][:rows], m)}
    diag(f"{label}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < TOL_SOLVER, (k, v)
    assert np.array_equal(got["xe"][rows:], got["xe"][:rows])                 # both halves of xe, bit for bit
    assert np.array_equal(op[rows:], op[:rows])                               # ... and of its operand copy
    for k in ("xbar", "d1", "mprev", "mprev2"):
        assert np.array_equal(got[k][rows:], st[k][rows:]), f"second half of {k} touched"
    assert np.array_equal(got["x0"], st["x0"])
    assert np.array_equal(got["mprev2"][:rows], st["mprev"][:rows] if form == "h2" else st["mprev2"][:rows])
    if prec == "fp32":
        assert np.array_equal(op, got["xe"])
    else:
        rnd = f16_round if prec == "fp16" else bf16_round
        hi = rnd(got["xe"])
        assert np.array_equal(op[:, :LD], hi)
        assert np.array_equal(op[:, LD:], rnd(got["xe"] - hi))


# ---- 1. the kernel against fp64 numpy -----------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("form", ["h1", "h2", "noise"])
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_k_solver_update_guided_against_numpy(prec, form, shape, diag):
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    n, T, rows, scales, lens, seeds, st = _case(shape)
    table, step = _table(form)
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    pw = LD if prec == "fp32" else 2 * LD
    op = DevBuf(2 * rows * pw * (4 if prec == "fp32" else 2))
    aux = {"coef": DevBuf.from_numpy(np.ascontiguousarray(table.coef, np.float32)), "step": DevBuf.from_numpy(np.array([step, 0, 0, 0], np.int32)),
           "scale": DevBuf.from_numpy(np.concatenate([scales, np.zeros(-n % 4, np.float32)])), "seeds": DevBuf.from_numpy(seeds),
           "lens": DevBuf.from_numpy(lens)}
    ptr = {**{k: b.ptr for k, b in bufs.items()}, **{k: b.ptr for k, b in aux.items()}, "xe_op": op.ptr}
    _lib.check(_launch(lib, prec, form, table, step, n, T, rows, scales, lens, seeds, ptr), "k_solver_update_guided")
    lib.ns2vc_dev_sync()
    got = {k: bufs[k].to_numpy((2 * rows, LD)) for k in st}
    opv = op.to_numpy((2 * rows, pw), dtype=np.float32 if prec == "fp32" else (np.float16 if prec == "fp16" else np.uint16))
    if prec == "bf16":
        opv = (opv.astype(np.uint32) << 16).view(np.float32)
    opv = opv.astype(np.float32)
    ref = _reference(form, table, step, n, T, rows, scales, lens, seeds, st)
    _check_outputs(prec, form, got, opv, ref, rows, st, diag, f"k_solver_update_guided {prec} {form} {shape}")
    if form == "noise":      # (the unguided export has no noise term to compare a scale-1 item with)
        return
    # the item with scale 1 == the unguided update fed that item's conditional rows, bit for bit
    b1 = int(np.flatnonzero(scales == 1.0)[0])
    r0, r1 = b1 * T, (b1 + 1) * T
    one = {k: DevBuf.from_numpy(np.ascontiguousarray(st[k][r0:r1])) for k in ("xe", "xbar", "d1", "mprev", "mprev2")}
    one["x0"] = DevBuf.from_numpy(np.ascontiguousarray(st["x0"][rows + r0:rows + r1]))
    op1 = DevBuf(T * pw * 4)
    _lib.check(lib.ns2vc_k_solver_update(ptr["coef"], ptr["step"], one["x0"].ptr, one["xe"].ptr, op1.ptr, PREC[prec], one["xbar"].ptr, one["d1"].ptr,
                                         one["mprev"].ptr, one["mprev2"].ptr if form == "h2" else None, T * LD, LD, None), "k_solver_update")
    lib.ns2vc_dev_sync()
    for k in ("xe", "xbar", "d1", "mprev"):
        assert np.array_equal(one[k].to_numpy((T, LD)), got[k][r0:r1]), f"scale-1 item: {k} differs from the unguided update"


def test_k_solver_update_guided_refuses_bad_arguments():
    """a scale pointer with T <= 0, n_half not a multiple of T * ld, ld & 3: refused, and nothing runs (the state keeps its bits)"""
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    n, T, rows, scales, lens, seeds, st = _case("small")
    table, step = _table("h1")
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    op = DevBuf(2 * rows * LD * 4)
    aux = {"coef": DevBuf.from_numpy(np.ascontiguousarray(table.coef, np.float32)), "step": DevBuf.from_numpy(np.array([step, 0, 0, 0], np.int32)),
           "scale": DevBuf.from_numpy(np.concatenate([scales, np.zeros(1, np.float32)])), "seeds": DevBuf.from_numpy(seeds), "lens": DevBuf.from_numpy(lens)}
    ptr = {**{k: b.ptr for k, b in bufs.items()}, **{k: b.ptr for k, b in aux.items()}, "xe_op": op.ptr}
    args = (lib, "fp32", "h1", table, step, n, T, rows, scales, lens, seeds, ptr)
    assert _launch(*args, T_arg=0) != 0
    assert _launch(*args, T_arg=-3) != 0
    assert _launch(*args, n_half=rows * LD - LD) != 0               # whole rows, not whole items
    assert _launch(*args, T_arg=4) != 0                             # 15 rows are no multiple of T = 4
    assert _launch(*args, n_half=rows * 126, ld=126) != 0           # ld & 3
    assert _launch(*args, n_half=0) != 0
    bad = dict(ptr, scale=None)
    assert _launch(lib, "fp32", "h1", table, step, n, T, rows, scales, lens, seeds, bad) != 0      # no scales: not the unguided update either
    lib.ns2vc_dev_sync()
    for k in st:
        assert np.array_equal(bufs[k].to_numpy((2 * rows, LD)), st[k]), k


# ---- 2. guard bands -----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
@pytest.mark.parametrize("form", ["h1", "h2"])
def test_k_solver_update_guided_bounds(form, prec, diag):
    """The same launch on guarded tensors (tests/guard.py): x0, xe and xe_op hold both halves, the history tensors ONE half with the guard band
    right behind it -- a store to their second half, or anywhere around a tensor, is a violation; NaN / Inf / zero fills must give the same bits."""
    from guard import OP_KIND
    from test_kernel_bounds_gpu import _check, _lib as be_lib, run_bounds
    lib = be_lib()
    n, T, rows, scales, lens, seeds, st = _case("small")
    table, step = _table(form)
    hist = ("xbar", "d1", "mprev", "mprev2")

    def body(ctx):
        b = {k: ctx.t(k, 2 * rows, LD, "f32", data=st[k]) for k in ("x0", "xe")}
        b.update({k: ctx.t(k, rows, LD, "f32", data=st[k][:rows]) for k in hist})
        op = ctx.t("xe_op", 2 * rows, LD if prec == "fp32" else 2 * LD, OP_KIND[PREC[prec]])
        ptr = {k: g.ptr for k, g in b.items()}
        ptr.update(xe_op=op.ptr, coef=ctx.t("coef", table.coef.shape[0], table.coef.shape[1], "f32", data=np.ascontiguousarray(table.coef, np.float32)).ptr,
                   step=ctx.t("step", 1, 4, "i32", data=np.array([[step, 0, 0, 0]], np.int32)).ptr,
                   scale=ctx.t("scale", 1, 4, "f32", data=np.concatenate([scales, np.zeros(1, np.float32)]).reshape(1, -1)).ptr, seeds=None, lens=None)
        _check(_launch(lib, prec, form, table, step, n, T, rows, scales, lens, seeds, ptr), "k_solver_update_guided")
        return {**b, "xe_op": op}
    label = f"ns2vc_k_solver_update_guided / {form} {prec}"
    got = run_bounds(diag, label, body, skew=1)
    ne, nb, nd, m = _reference(form, table, step, n, T, rows, scales, lens, seeds, st)
    errs = {"xe": rel_l2(got["xe"][:rows], ne), "xbar": rel_l2(got["xbar"], nb), "d1": rel_l2(got["d1"], nd), "mprev": rel_l2(got["mprev"], m)}
    diag(f"bounds {label}: P3 " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert all(v < TOL_SOLVER for v in errs.values()), errs
    assert np.array_equal(got["xe"][rows:], got["xe"][:rows]) and np.array_equal(got["xe_op"][rows:], got["xe_op"][:rows])
    assert np.array_equal(got["x0"], st["x0"])


# ---- the engine ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


@pytest.fixture(scope="module")
def oracle_weights(weights):
    import torch
    return {k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}


def _inputs(tag, n, T, Lp, Lu):
    import torch
    from ns2vc_amd.weights import hash_normal
    dev = torch.device("cuda", 0)
    mk = lambda name, shape: torch.from_numpy(hash_normal(f"gd.{tag}.{name}", shape)).to(dev)
    return mk("x", (n, 100, T)), mk("c", (n, 256, T)), mk("p", (n, Lp, 256)), mk("u", (n, Lu, 256))


def _engine(weights, prec, shape):
    from ns2vc_amd.engine import Engine
    e = Engine(precision=prec)
    e.load_state_dict(weights)
    e.prepare(*shape)
    return e


def _pad(p, L):
    import torch
    return p if p.shape[1] == L else torch.cat([p, p.new_zeros((p.shape[0], L - p.shape[1], p.shape[2]))], dim=1)


def _set_guided(e, c, p, u, scales, lengths=None, seeds=None):
    """the condition of a guided loop on an engine prepared for (2n, T, max(Lp, Lu)): cat([unconditional, conditional])"""
    import torch
    n, Lp, Lu = c.shape[0], p.shape[1], u.shape[1]
    L = max(Lp, Lu)
    e.set_lengths(None if lengths is None else list(lengths) * 2)
    e.set_prompt_lengths(None if Lp == Lu else [Lu] * n + [Lp] * n)
    e.set_guidance(scales)
    if seeds is not None:
        e.set_seeds(seeds)
    e.set_condition(torch.cat([c, c]).contiguous(), torch.cat([_pad(u, L), _pad(p, L)]).contiguous(), None)


def _guided_loop(e, x_T, c, p, u, scales, graph=True, lengths=None, seeds=None, tail=None, tail_steps=0):
    import torch
    _set_guided(e, c, p, u, scales, lengths, seeds)
    if tail is not None:      # (the tail's scales and seeds arrive through the hand-off alone)
        n, Lp, Lu = c.shape[0], p.shape[1], u.shape[1]
        tail.set_lengths(None if lengths is None else list(lengths) * 2)
        tail.set_prompt_lengths(None if Lp == Lu else [Lu] * n + [Lp] * n)
        tail.set_condition(torch.cat([c, c]).contiguous(), torch.cat([_pad(u, max(Lp, Lu)), _pad(p, max(Lp, Lu))]).contiguous(), None)
    x = x_T.clone()
    e.sample(x, use_graph=graph, tail=tail, tail_steps=tail_steps)
    torch.cuda.synchronize()
    return x.cpu().numpy()


def _unguided_loop(e, x_T, c, p, graph=True):
    import torch
    e.set_lengths(None)
    e.set_prompt_lengths(None)
    e.set_guidance(None)
    e.set_condition(c, p, None)
    x = x_T.clone()
    e.sample(x, use_graph=graph)
    torch.cuda.synchronize()
    return x.cpu().numpy()


def _oracle_x0(P, c, p, u, scales):
    """guided_x0 of two oracle forwards per evaluation, every item with its own prompt and its own unconditional prompt (numpy in / out)"""
    import torch
    from ns2vc_amd import schedule as S
    from ns2vc_amd.spec import UNetConfig
    from oracle import unet_ref
    cc, pc, uc = c.cpu(), p.cpu(), u.cpu()

    def f(xx, tt):
        xt, t = torch.from_numpy(np.asarray(xx, np.float32)), torch.from_numpy(np.asarray(tt, np.float32))
        x0_u = unet_ref.denoiser(P, UNetConfig(), xt, cc, uc, None, t).numpy()
        x0_c = unet_ref.denoiser(P, UNetConfig(), xt, cc, pc, None, t).numpy()
        return S.guided_x0(x0_u, x0_c, np.asarray(scales, np.float32))
    return f


# ---- 3. the loop against the oracle -------------------------------------------------------------
N3, T3, LP3, LU3, SC3 = 2, 66, 5, 1, (2.5, 0.5)
CASES3 = {"unipc2": ("unipc", 6, 2), "dpmpp3": ("dpmsolver++", 6, 3)}


@pytest.fixture(scope="module")
def oracle_loops(oracle_weights):
    """the guided reference latents, computed once: UniPC order 2 by oracle/sampler_ref.py; DPM-Solver++ order 3, which that file does not
    restate, by the host executor of its table (schedule.run_table_numpy, pinned to the reference's own guided loops by golden_v7), both driven
    by guided_x0 of two oracle forwards per step"""
    import torch
    from ns2vc_amd import schedule as S
    from oracle import sampler_ref
    x, c, p, u = _inputs("t3", N3, T3, LP3, LU3)
    f = _oracle_x0(oracle_weights, c, p, u, SC3)
    ft = lambda xx, tt: torch.from_numpy(f(xx.numpy(), tt.numpy()))
    return {"unipc2": sampler_ref.unipc_bh2(ft, sampler_ref.linear_betas(), x.cpu(), 6, order=2).numpy(),
            "dpmpp3": S.run_table_numpy(S.build_table("dpmsolver++", 6, order=3), f, x.cpu().numpy())}


@pytest.mark.parametrize("case", list(CASES3))
def test_guided_loop_against_oracle_fp32(case, weights, oracle_loops, diag):
    """fp32 engine, n = 2, T = 66, Lp = 5, Lu = 1, scales (2.5, 0.5): every item against the oracle alone, FP32_SAMPLED_TOL; captured == eager."""
    solver, steps, order = CASES3[case]
    x, c, p, u = _inputs("t3", N3, T3, LP3, LU3)
    e = _engine(weights, "fp32", (2 * N3, T3, max(LP3, LU3)))
    try:
        e.load_sampler(solver, steps, order=order)
        g = _guided_loop(e, x, c, p, u, SC3, True)
        ea = _guided_loop(e, x, c, p, u, SC3, False)
    finally:
        e.close()
    ref = oracle_loops[case]
    errs = [rel_l2(g[b], ref[b]) for b in range(N3)]
    diag(f"guided {case} fp32 vs oracle, per item: " + " ".join(f"{v:.2e}" for v in errs) + f" {fmt_local(local_errors(g, ref))}")
    assert np.array_equal(g, ea), "hipGraph replay must be bit-identical to eager launches"
    assert max(errs) < FP32_SAMPLED_TOL, errs


@pytest.mark.parametrize("case", list(CASES3))
def test_guided_loop_against_oracle_fp16(case, weights, oracle_loops, diag):
    """fp16 Denoiser with its default fp32 tail (unguided: none for UniPC, 4 evaluations for DPM-Solver++ order 3), same case, gated at the project's bar of
    1e-3 relative L2 on the sampled latent (guidance scales amplify per-evaluation rounding; the bar stays).  Under guidance the default tail
    gains ``guided_tail_extra(scales)`` = 1 evaluation at scale 2.5.  Measured: UniPC 3.50e-4 (tail 1; 1.12e-3, OVER the bar, with the unguided
    default of no tail, 8.2e-5 with 2), DPM-Solver++(3M) 7.67e-6 (tail 5 of 6; 9.35e-6 with 4) -- profiles/r15_guidance.txt."""
    from ns2vc_amd.pipeline import Denoiser
    solver, steps, order = CASES3[case]
    x, c, p, u = _inputs("t3", N3, T3, LP3, LU3)
    den = Denoiser(weights, precision="fp16")
    y = den.sample(c, p, None, x, solver=solver, steps=steps, order=order, guidance_scale=list(SC3), unconditional_prompt=u).cpu().numpy()
    ref = oracle_loops[case]
    e = rel_l2(y, ref)
    diag(f"guided {case} fp16 (default tail) vs oracle: {e:.2e} per item " + " ".join(f"{rel_l2(y[b], ref[b]):.2e}" for b in range(N3)) +
         f"; self-check {den.precision_error_seen}; serving_fp32 {den.serving_fp32}")
    assert den.engine.shape == (2 * N3, T3, LP3) and den.engine.guidance is not None
    assert e < PARITY_TOL, e


# ---- 4. identities through the engine -----------------------------------------------------------
def test_guided_identities_fp32(weights, diag):
    """n = 3, T = 66: (a) unconditional = conditional condition, scales (0, 3, 7) == the unguided loop; (b) scales (1, 2.5, 1): items 0 and 2 ==
    their unguided results; (c) each item of a guided batch == the same item as a guided batch of one."""
    n, T, Lp = 3, 66, 7
    x, c, p, u = _inputs("t4", n, T, Lp, Lp)
    e3 = _engine(weights, "fp32", (n, T, Lp))
    e6 = _engine(weights, "fp32", (2 * n, T, Lp))
    e2 = _engine(weights, "fp32", (2, T, Lp))
    try:
        for e in (e3, e6, e2):
            e.load_sampler("unipc", 6, order=2)
        plain = _unguided_loop(e3, x, c, p)
        same = _guided_loop(e6, x, c, p, p, (0.0, 3.0, 7.0))
        sel = _guided_loop(e6, x, c, p, u, (1.0, 2.5, 1.0))
        alone = np.concatenate([_guided_loop(e2, x[b:b + 1], c[b:b + 1], p[b:b + 1], u[b:b + 1], (s,)) for b, s in enumerate((1.0, 2.5, 1.0))])
    finally:
        for e in (e3, e6, e2):
            e.close()
    ea = [rel_l2(same[b], plain[b]) for b in range(n)]
    eb = [rel_l2(sel[b], plain[b]) for b in (0, 2)]
    lc = local_errors(sel, alone)
    diag(f"guided identities fp32: (a) u == c, scales (0, 3, 7) vs unguided {' '.join(f'{v:.2e}' for v in ea)} (bit-identical: {np.array_equal(same, plain)}); "
         f"(b) scale-1 items vs unguided {' '.join(f'{v:.2e}' for v in eb)} (bit-identical: {np.array_equal(sel[[0, 2]], plain[[0, 2]])}); "
         f"(c) batch vs alone {rel_l2(sel, alone):.2e} {fmt_local(lc)}")
    assert max(ea) < FP32_SAMPLED_TOL and max(eb) < FP32_SAMPLED_TOL
    assert rel_l2(sel[1], plain[1]) > 1e-3                       # the guided item did move
    assert rel_l2(sel, alone) < FP32_TOL and lc["frame"] < FP32_LOCAL_TOL and lc["chan"] < FP32_LOCAL_TOL


# ---- 5. the graph stays valid -------------------------------------------------------------------
def test_new_scales_replay_the_captured_graph(weights):
    n, T, Lp, Lu = 2, 66, 5, 3
    x, c, p, u = _inputs("t5", n, T, Lp, Lu)
    vecs = [(2.5, 0.5), (0.0, 4.0), (1.0, 1.5)]
    e = _engine(weights, "fp32", (2 * n, T, Lp))
    try:
        e.load_sampler("unipc", 5, order=2)
        base = e.graph_captures()
        outs = [_guided_loop(e, x, c, p, u, s) for s in vecs]
        assert e.graph_captures() == base + 1
        e.set_guidance(None)                                   # off and on again: recaptured
        again = _guided_loop(e, x, c, p, u, vecs[0])
        assert e.graph_captures() == base + 2
    finally:
        e.close()
    fresh = []
    for s in vecs:
        f = _engine(weights, "fp32", (2 * n, T, Lp))
        try:
            f.load_sampler("unipc", 5, order=2)
            fresh.append(_guided_loop(f, x, c, p, u, s))
        finally:
            f.close()
    for a, b in zip(outs, fresh):
        assert np.array_equal(a, b)
    assert np.array_equal(again, fresh[0])
    assert rel_l2(outs[1], outs[0]) > 1e-3


# ---- 6. stochastic and ragged -------------------------------------------------------------------
def test_guided_stochastic_ragged_loop(weights, oracle_weights, diag):
    """DDIM, 8 steps, eta = 1, n = 2, T = 70, lengths (70, 41), per-item seeds: the guided loop == run_table_numpy with the engine's noise stream
    (ns2vc_amd.noise.gauss) injected and a guided oracle x0_fn per item at its own length; frames past L_b are exact zeros."""
    import torch
    from ns2vc_amd import noise as N
    from ns2vc_amd import schedule as S
    n, T, Lp, Lu, lens, scales = 2, 70, 5, 1, (70, 41), (2.5, 0.5)
    seeds = np.array([0x0123456789ABCDEF, 42], dtype=np.uint64)
    x, c, p, u = _inputs("t6", n, T, Lp, Lu)
    for b, L in enumerate(lens):
        x[b, :, L:] = 0
    e = _engine(weights, "fp32", (2 * n, T, Lp))
    try:
        table = e.load_sampler("ddim", 8, S.linear_betas(1000, np.float64), eta=1.0)
        g = _guided_loop(e, x, c, p, u, scales, True, lengths=lens, seeds=seeds)
        ea = _guided_loop(e, x, c, p, u, scales, False, lengths=lens, seeds=seeds)
        with pytest.raises(Exception, match="differ"):           # the two halves must hold the same latent lengths
            e.set_lengths([70, 41, 70, 40])
            e.sample(x.clone())
    finally:
        e.close()
    assert np.array_equal(g, ea)
    errs = []
    for b, L in enumerate(lens):
        assert L == T or float(np.abs(g[b, :, L:]).max()) == 0.0
        f = _oracle_x0(oracle_weights, c[b:b + 1, :, :L], p[b:b + 1], u[b:b + 1], scales[b:b + 1])
        ref = S.run_table_numpy(table, f, x[b:b + 1, :, :L].cpu().numpy(), noise_fn=lambda i: N.gauss(seeds[b:b + 1], i, 100, L))
        errs.append(rel_l2(g[b, :, :L], ref[0]))
    diag("guided ddim8 eta 1 ragged fp32 vs host loop with gauss(), per item: " + " ".join(f"{v:.2e}" for v in errs))
    assert max(errs) < FP32_SAMPLED_TOL, errs


# ---- 7. hand-off --------------------------------------------------------------------------------
def test_guided_handoff_fp16_to_fp32_tail(weights, diag):
    """fp16 engine + fp32 tail of 2, guided == the loop on the fp32 engine alone within the 16-bit bar; the tail never sees set_guidance"""
    n, T, Lp, Lu, scales = 2, 66, 5, 1, (2.5, 0.5)
    x, c, p, u = _inputs("t7", n, T, Lp, Lu)
    e16, e32, ref = (_engine(weights, pr, (2 * n, T, Lp)) for pr in ("fp16", "fp32", "fp32"))
    try:
        for e in (e16, e32, ref):
            e.load_sampler("dpmsolver++", 8, order=2)
        whole = _guided_loop(ref, x, c, p, u, scales)
        assert e32.guidance is None
        y = _guided_loop(e16, x, c, p, u, scales, tail=e32, tail_steps=2)
        assert e32.guidance is not None and np.array_equal(e32.guidance, np.asarray(scales, np.float32))
        y32 = _guided_loop(ref, x, c, p, u, scales, tail=e32, tail_steps=3)        # fp32 -> fp32: the same arithmetic
    finally:
        for e in (e16, e32, ref):
            e.close()
    err = rel_l2(y, whole)
    diag(f"guided dpm++2 x8 handoff: fp16 head + fp32 tail of 2 vs fp32 loop {err:.2e}; fp32 head {rel_l2(y32, whole):.2e}")
    assert np.array_equal(y32, whole)
    assert err < PARITY_TOL, err


# ---- 8. denoise guided --------------------------------------------------------------------------
def test_denoise_guided_equals_two_calls_combined(weights, diag):
    import torch
    from ns2vc_amd import schedule as S
    from ns2vc_amd.pipeline import Denoiser
    n, T, Lp, Lu = 3, 66, 5, 2
    x, c, p, u = _inputs("t8", n, T, Lp, Lu)
    t = torch.tensor([700.0, 250.5, 3.0], device=x.device)
    scales = np.array([1.0, 2.5, 0.0], np.float32)
    den = Denoiser(weights, precision="fp32")
    y = den.denoise(x, t, c, p, guidance_scale=scales, unconditional_prompt=u).cpu().numpy()
    x0_c = den.denoise(x, t, c, p).cpu().numpy()
    x0_u = den.denoise(x, t, c, u).cpu().numpy()
    ref = S.guided_x0(x0_u, x0_c, scales)
    e = rel_l2(y, ref)
    diag(f"denoise guided fp32 vs two calls combined on the host: {e:.2e}")
    assert e < FP32_TOL
    assert rel_l2(y[1], x0_c[1]) > 1e-3
    assert np.array_equal(den.denoise(x, t, c, p, guidance_scale=3.0).cpu().numpy(), x0_c)      # no unconditional prompt: nothing guided runs
