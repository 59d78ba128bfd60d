"""The x0 correction of the captured sampling loop on the MI355X (dynamic thresholding / clamp: ns2vc_sampler_set_x0_correction): the exact
per-item |.| quantile (ns2vc_k_abs_quantile) on guarded tensors against ``schedule.abs_quantile``, one corrected update
(ns2vc_k_solver_update_corrected) against the fp64 recurrence, the loop against ``run_table_numpy(correct_x0=...)`` with the oracle UNet,
captured == eager, ragged == alone, guided, the hand-off, the 16-bit engines with their default tails, and mode 0 == no keywords."""
import numpy as np
import pytest

from test_guidance_gpu import (FP32_SAMPLED_TOL, FP32_TOL, LD, NC, PARITY_TOL, PREC, SHAPES, _case, _check_outputs, _engine, _guided_loop, _inputs,
                               _oracle_x0, _table)
from util import TOL_SOLVER, fmt_local, local_errors, rel_l2

pytestmark = pytest.mark.gpu


# ---- 1. the quantile kernel ---------------------------------------------------------------------
# (n items, T, nc, ld, lens): item boundaries inside one block | n = 1 | small | n_b = 100 000 > 65 536 (a 16-bit counter would wrap; ~25 sweeps
# of the 1024-thread block per pass)
QSHAPES = {"3x5": (3, 5, 100, 128, (5, 3, 1)), "one": (1, 1, 1, 4, (1,)), "2x7": (2, 7, 12, 16, (7, 2)), "big": (2, 1000, 100, 128, (1000, 657))}
CONTENTS = ("normal", "equal", "low8", "exponent", "zeros", "pad1e30")
PS = (0.0, 0.5, 0.995, 1.0)


def _content(kind, rows, nc, rng):
    f = np.float32
    sign = np.where(rng.random((rows, nc)) < 0.5, f(-1), f(1))
    if kind in ("normal", "pad1e30"):
        return rng.standard_normal((rows, nc)).astype(f)
    if kind == "equal":                       # one bin holds everything in every pass
        return sign * f(0.37)
    if kind == "low8":                        # differ in the low 8 mantissa bits only: the first two passes see one bin
        bits = (np.float32(1.5).view(np.uint32) & np.uint32(0xFFFFFF00)) | rng.integers(0, 256, (rows, nc)).astype(np.uint32)
        return sign * bits.view(f)
    if kind == "exponent":                    # powers of two: the last two passes see one bin each, v_hi lies in another first-pass bin
        return sign * np.exp2(rng.integers(-20, 21, (rows, nc))).astype(f)
    if kind == "zeros":                       # +-0, denormals and a few normals
        v = (rng.integers(0, 50, (rows, nc)).astype(np.uint32)).view(f)          # bit patterns 0 .. 49: zero and the smallest denormals
        pick = rng.random((rows, nc))
        v = np.where(pick < 0.1, rng.standard_normal((rows, nc)).astype(f), v)
        return (sign * v).astype(f)
    raise KeyError(kind)


def _quantile_ref(vals, p):
    from ns2vc_amd import schedule as S
    f = np.float32
    v = np.sort(np.abs(vals.astype(f)).reshape(-1))
    pos = f(p) * f(v.size - 1)
    lo = int(np.floor(pos))
    return S.abs_quantile(vals, p), float(f(pos - f(lo))) == 0.0, v[lo]


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", list(QSHAPES))
def test_k_abs_quantile_exact_on_guarded_buffers(shape, content, diag):
    """thr[b] against the float32 rule of torch.quantile on the item's live elements: bit-equal to the order statistic where w = 0, within 2 ulp
    otherwise (the order statistics are exact; the lerp is one fused multiply-add).  Rows past lens hold 1e30, and so do the padded columns of
    the ``pad1e30`` content (elsewhere they are the guard fill: NaN / Inf / 0): none of them may be seen, nothing outside thr may be written."""
    from test_kernel_bounds_gpu import _check, _lib as be_lib, run_bounds
    lib = be_lib()
    n, T, nc, ld, lens = QSHAPES[shape]
    rng = np.random.default_rng(list(QSHAPES).index(shape) * 16 + CONTENTS.index(content))
    data = _content(content, n * T, nc, rng)
    live = [data[b * T:b * T + lens[b]].copy() for b in range(n)]
    for b in range(n):
        data[b * T + lens[b]:(b + 1) * T] = np.float32(1e30)
    width = nc
    if content == "pad1e30":
        data = np.concatenate([data, np.full((n * T, ld - nc), 1e30, np.float32)], axis=1)
        width = ld

    def body(ctx):
        v = ctx.t("values", n * T, width, "f32", pad=ld - width, data=data)
        ln = ctx.t("lens", 1, n, "i32", data=np.asarray(lens, np.int32).reshape(1, -1))
        outs = {}
        for p in PS:
            thr = ctx.t(f"thr{p}", 1, n, "f32")
            _check(lib.ns2vc_k_abs_quantile(v.ptr, n, T, ld, nc, ln.ptr, p, thr.ptr, None), "k_abs_quantile")
            outs[f"thr{p}"] = thr
        return outs
    got = run_bounds(diag, f"ns2vc_k_abs_quantile / {shape} {content}", body, skew=1)
    worst = 0.0
    for p in PS:
        for b in range(n):
            ref, exact, vlo = _quantile_ref(live[b], p)
            g = np.float32(got[f"thr{p}"][0, b])
            if exact:
                assert g.tobytes() == np.float32(vlo).tobytes(), (shape, content, p, b, g, vlo)
            ulp = abs(float(g) - float(ref)) / float(np.spacing(np.float32(max(abs(float(ref)), 1e-45))))
            worst = max(worst, ulp)
            assert ulp <= 2.0, (shape, content, p, b, g, ref, ulp)
    diag(f"k_abs_quantile {shape} {content}: worst {worst:.1f} ulp over p = {PS}")


def test_k_abs_quantile_without_lens_and_bad_arguments():
    from ns2vc_amd import _lib, schedule as S
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    rng = np.random.default_rng(5)
    v = rng.standard_normal((2 * 9, 16)).astype(np.float32)
    d, thr = DevBuf.from_numpy(v), DevBuf(16)
    _lib.check(lib.ns2vc_k_abs_quantile(d.ptr, 2, 9, 16, 10, None, 0.9, thr.ptr, None), "k_abs_quantile")
    lib.ns2vc_dev_sync()
    got = thr.to_numpy((4,))[:2]
    ref = [S.abs_quantile(v[b * 9:(b + 1) * 9, :10], 0.9) for b in range(2)]
    assert np.array_equal(got, np.asarray(ref, np.float32)), (got, ref)
    for bad in (dict(ld=18), dict(nc=17), dict(nc=0), dict(T=0), dict(p=1.5), dict(p=-0.1), dict(p=float("nan")), dict(n=0)):
        a = dict(n=2, T=9, ld=16, nc=10, p=0.9, **{})
        a.update(bad)
        assert lib.ns2vc_k_abs_quantile(d.ptr, a["n"], a["T"], a["ld"], a["nc"], None, a["p"], thr.ptr, None) != 0, bad
    assert lib.ns2vc_k_abs_quantile(None, 2, 9, 16, 10, None, 0.9, thr.ptr, None) != 0


# ---- 2. the corrected update against fp64 -------------------------------------------------------
RATIO2, MAXVAL2 = {1: 0.9, 2: 0.995}, {1: 1.645, 2: 1.0}      # mode 1: |N(0,1)| has its 0.9 quantile at 1.64 -- max_val wins for some items, the quantile for others


def _reference_c(form, table, step, n, T, rows, scales, lens, st, guided, mode):
    """(guided_x0,) the round trip, the correction in fp64 (np.quantile, linear, over the live rows and channels), the recurrence row"""
    from ns2vc_amd import schedule as S
    f64 = {k: v.astype(np.float64) for k, v in st.items()}
    x0 = f64["x0"][:rows]
    if guided:
        x0 = S.guided_x0(x0.reshape(n, T, LD), f64["x0"][rows:].reshape(n, T, LD), scales.astype(np.float64)).reshape(rows, LD)
    row = table.coef[step]
    a, s, g0, g1, A, Bc, d1c, pc = (float(v) for v in row[1:9])
    d2c, pe = float(row[10]), float(row[11])
    xe, xb, d1, mp = f64["xe"][:rows], f64["xbar"][:rows], f64["d1"][:rows], f64["mprev"][:rows]
    mp2 = f64["mprev2"][:rows] if form == "h2" else None
    m = (xe - s * ((xe - a * x0) / s)) / a
    thr = np.zeros(n)
    m3 = m.reshape(n, T, LD).copy()
    for b in range(n):
        sb = MAXVAL2[mode]
        if mode == 1:
            v = np.sort(np.abs(m3[b, :lens[b], :NC]).reshape(-1))      # fp64 order statistics at the float32 position rule of torch.quantile
            pos = np.float32(RATIO2[mode]) * np.float32(v.size - 1)
            lo, hi = int(np.floor(pos)), int(np.ceil(pos))
            thr[b] = v[lo] + (v[hi] - v[lo]) * float(np.float32(pos - np.float32(lo)))
            sb = max(thr[b], sb)
        m3[b] = np.clip(m3[b], -sb, sb) / (sb if mode == 1 else 1.0)
    m = m3.reshape(rows, LD)
    x = xb - g0 * d1 - g1 * (m - mp)
    nb = A * x - Bc * m
    nd = d1c * (mp - m) + (d2c * (mp2 - m) if mp2 is not None else 0.0)
    ne = nb - pc * nd - (pe * (mp2 - m) if mp2 is not None else 0.0)
    return (ne, nb, nd, m), thr


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("form", ["h1", "h2"])
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_k_solver_update_corrected_against_numpy(prec, form, guided, shape, diag):
    """mode 1 and mode 2, each against the fp64 recurrence at TOL_SOLVER (the quantile is 1-Lipschitz in max |dm|); guided: both halves of xe and
    its operand copy identical, the second halves of the histories untouched"""
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    n, T, rows, scales, lens, seeds, st = _case(shape)
    table, step = _table(form)
    pw = LD if prec == "fp32" else 2 * LD
    aux = {"coef": DevBuf.from_numpy(np.ascontiguousarray(table.coef, np.float32)), "step": DevBuf.from_numpy(np.array([step, 0, 0, 0], np.int32)),
           "scale": DevBuf.from_numpy(np.concatenate([scales, np.zeros(-n % 4, np.float32)])), "lens": DevBuf.from_numpy(lens)}
    for mode in (1, 2):
        bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
        op = DevBuf(2 * rows * pw * (4 if prec == "fp32" else 2))
        thr = DevBuf.from_numpy(np.full((n + 3) // 4 * 4, -1.0, np.float32))
        _lib.check(lib.ns2vc_k_solver_update_corrected(aux["coef"].ptr, aux["step"].ptr, bufs["x0"].ptr, bufs["xe"].ptr, op.ptr, PREC[prec], bufs["xbar"].ptr,
                                                       bufs["d1"].ptr, bufs["mprev"].ptr, bufs["mprev2"].ptr if form == "h2" else None, rows * LD, LD, T,
                                                       aux["scale"].ptr if guided else None, aux["lens"].ptr, NC, mode, RATIO2[mode], MAXVAL2[mode],
                                                       thr.ptr, None), "k_solver_update_corrected")
        lib.ns2vc_dev_sync()
        got = {k: bufs[k].to_numpy((2 * rows, LD)) for k in st}
        opv = op.to_numpy((2 * rows, pw), dtype=np.float32 if prec == "fp32" else (np.float16 if prec == "fp16" else np.uint16))
        if prec == "bf16":
            opv = (opv.astype(np.uint32) << 16).view(np.float32)
        opv = opv.astype(np.float32)
        ref, thr_ref = _reference_c(form, table, step, n, T, rows, scales, lens, st, guided, mode)
        label = f"k_solver_update_corrected mode {mode} {prec} {form} {'guided' if guided else 'plain'} {shape}"
        thr_got = thr.to_numpy(((n + 3) // 4 * 4,))[:n]
        if mode == 1:
            e_thr = float(np.max(np.abs(thr_got - thr_ref) / thr_ref))
            diag(f"{label}: thr max rel {e_thr:.1e}; items with s = max_val: {int((thr_ref < MAXVAL2[1]).sum())} of {n}")
            assert e_thr < TOL_SOLVER, (thr_got, thr_ref)
            assert shape == "small" or 0 < int((thr_ref < MAXVAL2[1]).sum()) < n      # both branches of max(thr, max_val) are taken
        else:
            assert np.all(thr_got == -1.0)                                            # the clamp has no quantile launch
        assert float(np.mean(np.abs(ref[3]) >= (1.0 if mode == 1 else MAXVAL2[2]) * (1 - 1e-12))) > 1e-3      # the clamp does bite
        if guided:
            _check_outputs(prec, form, got, opv, ref, rows, st, diag, label)
            continue
        ne, nb, nd, m = ref
        errs = {"xe": rel_l2(got["xe"][:rows], ne), "xbar": rel_l2(got["xbar"][:rows], nb), "d1": rel_l2(got["d1"][:rows], nd),
                "mprev": rel_l2(got["mprev"][:rows], m)}
        diag(f"{label}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v < TOL_SOLVER, (k, v)
        for k in ("xe", "xbar", "d1", "mprev", "mprev2", "x0"):      # the unguided launch covers the first half only
            assert np.array_equal(got[k][rows:], st[k][rows:]), f"rows past n of {k} touched"
        assert np.array_equal(got["x0"], st["x0"])
        assert np.array_equal(got["mprev2"][:rows], st["mprev"][:rows] if form == "h2" else st["mprev2"][:rows])


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("form", ["h1", "h2"])
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_clamp_no_value_reaches_is_the_plain_update_bitwise(prec, form, guided, diag):
    """mode 2 with max_val = 3e38: the clamp changes nothing, so solver_update_th_kernel must give the bits of solver_update_kernel -- state,
    operand pair, guided mirror -- on the "big" shape (the stride loop's second pass included).  Pins the two kernel bodies together."""
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    n, T, rows, scales, lens, seeds, st = _case("big")
    table, step = _table(form)
    pw = LD if prec == "fp32" else 2 * LD
    coef, stp = DevBuf.from_numpy(np.ascontiguousarray(table.coef, np.float32)), DevBuf.from_numpy(np.array([step, 0, 0, 0], np.int32))
    sc = DevBuf.from_numpy(np.concatenate([scales, np.zeros(-n % 4, np.float32)]))
    outs = []
    for corrected in (False, True):
        bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
        op = DevBuf.from_numpy(np.zeros(2 * rows * pw * (2 if prec == "fp32" else 1), np.uint16))
        m2 = bufs["mprev2"].ptr if form == "h2" else None
        head = (coef.ptr, stp.ptr, bufs["x0"].ptr, bufs["xe"].ptr, op.ptr, PREC[prec], bufs["xbar"].ptr, bufs["d1"].ptr, bufs["mprev"].ptr, m2, rows * LD, LD)
        if corrected:
            rc = lib.ns2vc_k_solver_update_corrected(*head, T, sc.ptr if guided else None, None, NC, 2, 0.5, 3e38, None, None)
        elif guided:
            rc = lib.ns2vc_k_solver_update_guided(*head, sc.ptr, T, None, None, NC, None)
        else:
            rc = lib.ns2vc_k_solver_update(*head, None)
        _lib.check(rc, "solver update")
        lib.ns2vc_dev_sync()
        outs.append({**{k: bufs[k].to_numpy((2 * rows, LD)).view(np.uint32) for k in st}, "xe_op": op.to_numpy((2 * rows * pw * (2 if prec == "fp32" else 1),), dtype=np.uint16)})
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), f"{k}: the corrected kernel with an idle clamp differs from the plain update"
    assert not np.array_equal(outs[0]["xe"], st["xe"].view(np.uint32))


def test_k_solver_update_corrected_refuses_bad_arguments():
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    n, T, rows, scales, lens, seeds, st = _case("small")
    table, step = _table("h1")
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    op, thr = DevBuf(2 * rows * LD * 4), DevBuf(16)
    coef, stp = DevBuf.from_numpy(np.ascontiguousarray(table.coef, np.float32)), DevBuf.from_numpy(np.array([step, 0, 0, 0], np.int32))

    def call(mode=1, ratio=0.9, max_val=1.0, n_el=rows * LD, ld=LD, T_=T, thr_p=thr.ptr):
        return lib.ns2vc_k_solver_update_corrected(coef.ptr, stp.ptr, bufs["x0"].ptr, bufs["xe"].ptr, op.ptr, 0, bufs["xbar"].ptr, bufs["d1"].ptr,
                                                   bufs["mprev"].ptr, None, n_el, ld, T_, None, None, NC, mode, ratio, max_val, thr_p, None)
    for kw in (dict(mode=0), dict(mode=3), dict(ratio=1.5), dict(ratio=float("nan")), dict(max_val=0.0), dict(max_val=-1.0), dict(n_el=rows * LD - LD),
               dict(T_=0), dict(T_=4), dict(ld=126, n_el=rows * 126), dict(thr_p=None), dict(n_el=0)):
        assert call(**kw) != 0, kw
    lib.ns2vc_dev_sync()
    for k in st:
        assert np.array_equal(bufs[k].to_numpy((2 * rows, LD)), st[k]), k


# ---- the engine ---------------------------------------------------------------------------------
N3, T3, LP3, LU3, STEPS3 = 2, 66, 5, 1, 6
RATIO3 = 0.9
CASES3 = {"unipc2": ("unipc", 2), "dpmpp3": ("dpmsolver++", 3)}


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


@pytest.fixture(scope="module")
def oracle_weights(weights):
    import torch
    return {k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}


def _plain_x0(P, c, p):
    import torch
    from ns2vc_amd.spec import UNetConfig
    from oracle import unet_ref
    cc, pc = c.cpu(), p.cpu()
    return lambda xx, tt: unet_ref.denoiser(P, UNetConfig(), torch.from_numpy(np.asarray(xx, np.float32)), cc, pc, None,
                                            torch.from_numpy(np.asarray(tt, np.float32))).numpy()


@pytest.fixture(scope="module")
def setting(oracle_weights):
    """max_val from the ORACLE's first evaluation: 0.8 x the smallest per-item ``RATIO3`` quantile of |x0(x_T)|, so that at the first step every
    item's threshold is its own quantile (s > max_val: the division acts) and 1 - RATIO3 of its elements are clamped -- asserted here"""
    from ns2vc_amd import schedule as S
    x, c, p, u = _inputs("x0c", N3, T3, LP3, LU3)
    t0 = S.build_table("unipc", STEPS3).t_model[0]
    m0 = _plain_x0(oracle_weights, c, p)(x.cpu().numpy(), np.full((N3,), t0, np.float32))
    q = [float(S.abs_quantile(m0[b], RATIO3)) for b in range(N3)]
    max_val = 0.8 * min(q)
    clamped = [float(np.mean(np.abs(m0[b]) > max(q[b], max_val))) for b in range(N3)]
    assert min(clamped) > 0.05 and all(v > max_val for v in q), (q, max_val, clamped)
    return {"max_val": max_val, "q": q, "inputs": (x, c, p, u)}


def _corr(setting, mode="dynamic_thresholding", lengths=None):
    return dict(mode=mode, ratio=RATIO3, max_val=setting["max_val"] if mode == "dynamic_thresholding" else min(setting["q"]), lengths=lengths)


@pytest.fixture(scope="module")
def oracle_loops(oracle_weights, setting):
    """the corrected reference latents, once: run_table_numpy(correct_x0=...) (pinned to the reference's own corrected loops by golden_v8) driven by
    the oracle UNet"""
    from ns2vc_amd import schedule as S
    x, c, p, u = setting["inputs"]
    f = _plain_x0(oracle_weights, c, p)
    out = {}
    for case, (solver, order) in CASES3.items():
        out[case] = S.run_table_numpy(S.build_table(solver, STEPS3, order=order), f, x.cpu().numpy(), correct_x0=_corr(setting))
    out["unipc2.clamp"] = S.run_table_numpy(S.build_table("unipc", STEPS3, order=2), f, x.cpu().numpy(), correct_x0=_corr(setting, "clamp"))
    out["unipc2.off"] = S.run_table_numpy(S.build_table("unipc", STEPS3, order=2), f, x.cpu().numpy())
    out["unipc2.guided"] = S.run_table_numpy(S.build_table("unipc", STEPS3, order=2), _oracle_x0(oracle_weights, c, p, u, (2.5, 0.5)), x.cpu().numpy(),
                                             correct_x0=_corr(setting))
    return out


def _loop(e, x, c, p, graph=True, lengths=None, tail=None, tail_steps=0):
    import torch
    e.set_lengths(lengths)
    e.set_prompt_lengths(None)
    e.set_guidance(None)
    e.set_condition(c, p, None)
    if tail is not None:
        tail.set_lengths(lengths)
        tail.set_prompt_lengths(None)
        tail.set_condition(c, p, None)
    y = x.clone()
    e.sample(y, use_graph=graph, tail=tail, tail_steps=tail_steps)
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ---- 3. the loop against the oracle -------------------------------------------------------------
@pytest.mark.parametrize("case", ["unipc2", "dpmpp3", "unipc2.clamp"])
def test_corrected_loop_against_oracle_fp32(case, weights, oracle_loops, setting, diag):
    """fp32 engine, n = 2, T = 66, 6 steps: dynamic thresholding (history 1 and history 2 tables) and the clamp within FP32_SAMPLED_TOL of the host
    loop with the oracle UNet; captured == eager bit for bit; and the correction did change the latent"""
    solver, order = CASES3[case.split(".")[0]]
    mode = "clamp" if case.endswith(".clamp") else "dynamic_thresholding"
    x, c, p, u = setting["inputs"]
    e = _engine(weights, "fp32", (N3, T3, LP3))
    try:
        e.load_sampler(solver, STEPS3, order=order)
        k = _corr(setting, mode)
        e.set_x0_correction(k["mode"], k["ratio"], k["max_val"])
        g = _loop(e, x, c, p, True)
        ea = _loop(e, x, c, p, False)
    finally:
        e.close()
    ref = oracle_loops[case]
    errs = [rel_l2(g[b], ref[b]) for b in range(N3)]
    diag(f"x0 correction {case} fp32 vs oracle, per item: " + " ".join(f"{v:.2e}" for v in errs) + f" {fmt_local(local_errors(g, ref))}")
    assert np.array_equal(g, ea), "hipGraph replay must be bit-identical to eager launches"
    assert max(errs) < FP32_SAMPLED_TOL, errs
    assert rel_l2(oracle_loops["unipc2"], oracle_loops["unipc2.off"]) > 1e-2 and rel_l2(oracle_loops["unipc2.clamp"], oracle_loops["unipc2.off"]) > 1e-3


def test_corrected_ragged_item_equals_the_item_alone(weights, setting, diag):
    """lengths (66, 41): item 1 of the padded batch against the same item alone at T = 41 (its quantile runs over its own 41 frames), zeros past
    its end.  The comparison is by tolerance (FP32_TOL, measured 1.7e-6), not bitwise, as in the project's other ragged tests: an engine prepared
    for T = 41 tiles its GEMMs and reduces its GroupNorm sums differently from one prepared for T = 66, so the forwards differ in float32
    rounding.  The QUANTILE is exact either way; a threshold taken over the wrong frames would show at the 1e-2 level."""
    x, c, p, u = setting["inputs"]
    L = 41
    xr = x.clone()
    xr[1, :, L:] = 0
    e2, e1 = _engine(weights, "fp32", (N3, T3, LP3)), _engine(weights, "fp32", (1, L, LP3))
    try:
        for e in (e2, e1):
            e.load_sampler("unipc", STEPS3, order=2)
            e.set_x0_correction("dynamic_thresholding", RATIO3, setting["max_val"])
        g = _loop(e2, xr, c, p, True, lengths=[T3, L])
        alone = _loop(e1, xr[1:2, :, :L].contiguous(), c[1:2, :, :L].contiguous(), p[1:2], True)
        full = _loop(e2, x, c, p, True)      # (dense again: item 0 is the same either way)
    finally:
        e2.close()
        e1.close()
    err = rel_l2(g[1, :, :L], alone[0])
    lc = local_errors(g[1:2, :, :L], alone)
    diag(f"x0 correction ragged: item 1 (41 of 66 frames) vs alone {err:.2e} {fmt_local(lc)}; item 0 vs the dense batch {rel_l2(g[0], full[0]):.2e}")
    assert float(np.abs(g[1, :, L:]).max()) == 0.0
    assert err < FP32_TOL, err
    assert rel_l2(g[0], full[0]) < FP32_TOL


def test_corrected_guided_loop_fp32(weights, oracle_loops, setting, diag):
    """scales (2.5, 0.5) with dynamic thresholding: the threshold is the quantile of the GUIDED x0"""
    x, c, p, u = setting["inputs"]
    e = _engine(weights, "fp32", (2 * N3, T3, max(LP3, LU3)))
    try:
        e.load_sampler("unipc", STEPS3, order=2)
        e.set_x0_correction("dynamic_thresholding", RATIO3, setting["max_val"])
        g = _guided_loop(e, x, c, p, u, (2.5, 0.5), True)
        ea = _guided_loop(e, x, c, p, u, (2.5, 0.5), False)
    finally:
        e.close()
    ref = oracle_loops["unipc2.guided"]
    errs = [rel_l2(g[b], ref[b]) for b in range(N3)]
    diag(f"x0 correction guided (2.5, 0.5) fp32 vs oracle, per item: " + " ".join(f"{v:.2e}" for v in errs))
    assert np.array_equal(g, ea)
    assert max(errs) < FP32_SAMPLED_TOL, errs
    assert rel_l2(ref, oracle_loops["unipc2"]) > 1e-2


def test_corrected_handoff_carries_the_setting(weights, setting, diag):
    """fp32 head + fp32 tail of 3 in mid-loop == the loop on one engine, bit for bit; the tail never sees set_x0_correction; a tail that held
    ANOTHER setting takes the head's"""
    x, c, p, u = setting["inputs"]
    head, tail = _engine(weights, "fp32", (N3, T3, LP3)), _engine(weights, "fp32", (N3, T3, LP3))
    try:
        for e in (head, tail):
            e.load_sampler("dpmsolver++", STEPS3, order=3)
        head.set_x0_correction("dynamic_thresholding", RATIO3, setting["max_val"])
        whole = _loop(head, x, c, p)
        assert tail.x0_correction is None
        y = _loop(head, x, c, p, tail=tail, tail_steps=3)
        assert tail.x0_correction == head.x0_correction and tail.x0_correction[0] == 1
        tail.set_x0_correction("clamp", 0.5, 3.0)
        y2 = _loop(head, x, c, p, tail=tail, tail_steps=2)
        plain_tail = _loop(tail, x, c, p)     # the tail on its own now corrects as the head does
    finally:
        head.close()
        tail.close()
    diag(f"x0 correction hand-off: head + tail of 3 vs one engine {rel_l2(y, whole):.2e}")
    assert np.array_equal(y, whole) and np.array_equal(y2, whole) and np.array_equal(plain_tail, whole)


def test_only_values_a_launch_takes_recapture(weights, setting):
    """the ratio under the clamp, and any value while off, reach no launch: the captured graph is replayed"""
    x, c, p, u = setting["inputs"]
    e = _engine(weights, "fp32", (N3, T3, LP3))
    try:
        e.load_sampler("unipc", STEPS3, order=2)
        e.set_x0_correction("clamp", 0.5, 0.7)
        a = _loop(e, x, c, p)
        caps = e.graph_captures()
        e.set_x0_correction("clamp", 0.9, 0.7)
        assert np.array_equal(_loop(e, x, c, p), a) and e.graph_captures() == caps
        e.set_x0_correction("clamp", 0.9, 0.6)
        assert not np.array_equal(_loop(e, x, c, p), a) and e.graph_captures() == caps + 1
        e.set_x0_correction(None, 0.1, 5.0)
        off = _loop(e, x, c, p)
        e.set_x0_correction(None, 0.7, 2.0)
        assert np.array_equal(_loop(e, x, c, p), off) and e.graph_captures() == caps + 2
    finally:
        e.close()


def test_correction_refuses_stochastic_tables(weights, setting):
    import torch
    from ns2vc_amd import schedule as S
    x, c, p, u = setting["inputs"]
    e = _engine(weights, "fp32", (N3, T3, LP3))
    try:
        e.load_sampler("ddim", 4, S.linear_betas(1000, np.float64), eta=1.0)
        e.set_seeds(np.arange(N3, dtype=np.uint64))
        e.set_x0_correction("clamp", 0.9, 1.0)
        e.set_condition(c, p, None)
        with pytest.raises(Exception, match="stochastic"):
            e.sample(x.clone())
        e.set_x0_correction(None)
        e.sample(x.clone())
        torch.cuda.synchronize()
    finally:
        e.close()


@pytest.mark.parametrize("prec", ["fp16", "bf16"])
@pytest.mark.parametrize("case", ["unipc2", "dpmpp3"])
def test_corrected_loop_16bit_default_tail(case, prec, weights, oracle_loops, setting, diag):
    """the 16-bit Denoiser with its DEFAULT fp32 tail under dynamic thresholding against the oracle, every case at the project's bar of 1e-3.
    The defaults of an uncorrected loop do not suffice: with them (none for UniPC order 2) fp16 UniPC measured 9.34e-4, 7 % inside the bar on one
    setting, and bf16 UniPC 6.6e-3, outside it.  Under a correction the default tail is therefore at least ``corrected_tail_min(precision)``
    evaluations (ns2vc_amd/pipeline.py states the rule: the rounding of an evaluation reaches a corrected value twice, through the element and
    through the threshold) -- 1 for fp16, 3 for bf16.  DESIGN 4.10 records what each case measures with it."""
    from ns2vc_amd.pipeline import corrected_tail_min, default_tail_fp32
    from ns2vc_amd.pipeline import Denoiser
    solver, order = CASES3[case]
    x, c, p, u = setting["inputs"]
    den = Denoiser(weights, precision=prec)
    y = den.sample(c, p, None, x, solver=solver, steps=STEPS3, order=order, correcting_x0_fn="dynamic_thresholding", thresholding_max_val=setting["max_val"],
                   dynamic_thresholding_ratio=RATIO3).cpu().numpy()
    ref = oracle_loops[case]
    e = rel_l2(y, ref)
    diag(f"x0 correction {case} {prec} (default tail) vs oracle: {e:.2e} per item " + " ".join(f"{rel_l2(y[b], ref[b]):.2e}" for b in range(N3)) +
         f"; tail {max(default_tail_fp32(solver, order), corrected_tail_min(prec))} of {STEPS3}; serving_fp32 {den.serving_fp32}")
    assert den.engine.x0_correction is not None and den.engine.x0_correction[0] == 1
    assert e < PARITY_TOL, e


# ---- 4. identity --------------------------------------------------------------------------------
def test_mode_off_is_the_call_without_the_keywords(weights, setting, diag):
    """correcting_x0_fn=None (whatever the other two hold) == no keywords, bit for bit, and nothing is recaptured; the SAME setting again replays
    the captured graph; a new max_val or ratio recaptures (they are launch arguments: the recapture form)"""
    from ns2vc_amd.pipeline import Denoiser
    x, c, p, u = setting["inputs"]
    den = Denoiser(weights, precision="fp32")
    kw = dict(solver="unipc", steps=STEPS3, order=2)
    a = den.sample(c, p, None, x, **kw).cpu().numpy()
    caps = den.engine.graph_captures()
    b = den.sample(c, p, None, x, correcting_x0_fn=None, thresholding_max_val=0.25, dynamic_thresholding_ratio=0.5, **kw).cpu().numpy()
    assert np.array_equal(a, b) and den.engine.graph_captures() == caps
    on = dict(correcting_x0_fn="dynamic_thresholding", thresholding_max_val=setting["max_val"], dynamic_thresholding_ratio=RATIO3)
    y1 = den.sample(c, p, None, x, **on, **kw).cpu().numpy()
    assert den.engine.graph_captures() == caps + 1
    y2 = den.sample(c, p, None, x, **on, **kw).cpu().numpy()
    assert den.engine.graph_captures() == caps + 1 and np.array_equal(y1, y2)
    y3 = den.sample(c, p, None, x, **dict(on, thresholding_max_val=2 * setting["max_val"]), **kw).cpu().numpy()
    assert den.engine.graph_captures() == caps + 2 and not np.array_equal(y3, y1)
    z = den.sample(c, p, None, x, **kw).cpu().numpy()
    assert np.array_equal(z, a) and den.engine.x0_correction is None
    diag(f"x0 correction identity: off == no keywords; on moved the latent by {rel_l2(y1, a):.2e}")
    assert rel_l2(y1, a) > 1e-2
