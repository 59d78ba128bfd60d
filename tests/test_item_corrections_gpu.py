"""Per-item x0 correction on the MI355X (ns2vc_sampler_set_x0_correction_items): the step's two launches alone
(ns2vc_k_solver_update_items_corrected) against the loop-wide hook bit for bit on guarded buffers, their refusals, and the loop -- an item ends on
the bits it has when its record is the loop-wide setting: through Denoiser.sample(corrections=) with and without per-item schedules, guided,
ragged, captured and eager, across the hand-off, in a slot loop beside a DDIM item, and through the two converters; what recaptures."""
import numpy as np
import pytest

from guard import OP_KIND, DeviceBackend, Guarded
from test_continuous_gpu import DDIM6, LENS, U3_6, U4, U6, _drive, _request, pre_model  # noqa: F401  (pre_model: a fixture)
from test_guidance_gpu import FP32_SAMPLED_TOL, PREC, _engine, _inputs
from test_x0_correction_gpu import _plain_x0
from util import rel_l2

pytestmark = pytest.mark.gpu
LD, NC = 128, 100
B64 = np.linspace(1e-4, 0.02, 1000, dtype=np.float64)      # schedule.linear_betas(1000, np.float64)


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


# ---- 1. the hook, bit for bit -------------------------------------------------------------------------------------------------------
STEP = 4
NOISE_ROW0 = 16
# (row0, steps, start, flags) at loop step 4: rows 0-5 UniPC order 2, 6-15 UniPC order 3 (history 2), 16-23 DDIM eta 1 (noise)
ITEMS7 = np.array([[0, 6, 2, 0], [NOISE_ROW0, 8, 1, 2], [0, 6, 1, 0], [0, 6, 0, 0], [0, 6, 3, 0], [6, 10, 0, 1], [0, 6, 5, 0]], np.int32)
MODES7 = np.array([0, 0, 1, 1, 2, 1, 1], np.int32)      # (the held item 6 asks for mode 1: its threshold must still keep its fill)
RATIOS7 = np.array([0.995, 0.5, 0.37, 0.9, 0.2, 0.8, 0.6], np.float32)
MAXV7 = np.array([1.0, 2.0, 0.4, 50.0, 0.7, 0.3, 0.5], np.float32)      # item 3: max_val above its quantile, so max_val is the threshold
LENS7 = np.array([67, 66, 33, 1, 40, 67, 50], np.int32)
HELD7 = 6
SCALES7 = np.array([2.5, 1.0, 0.5, 3.0, 0.0, 1.5, 7.0], np.float32)
SEEDS7 = np.arange(7, dtype=np.uint64) * np.uint64(7919) + np.uint64(5)


def _tables7():
    from ns2vc_amd import schedule as S
    a, b = S.build_table("unipc", 6, order=2), S.build_table("unipc", 10, order=3, skip_type="logSNR")
    c = S.build_table("ddim", 8, S.linear_betas(1000, np.float64), eta=1.0)
    assert b.coef[4, 10] != 0 and b.coef[4, 11] != 0 and c.coef[3, 9] != 0
    return np.ascontiguousarray(np.concatenate([a.coef, b.coef, c.coef]), np.float32)


def _state(n_items, T, guided, seed):
    rng = np.random.default_rng(seed)
    rows = n_items * T
    st = {k: rng.standard_normal((rows, LD)).astype(np.float32) for k in ("xbar", "d1", "mprev", "mprev2")}
    st["x0"] = rng.standard_normal(((2 if guided else 1) * rows, LD)).astype(np.float32)
    xe = rng.standard_normal((rows, LD)).astype(np.float32)
    st["xe"] = np.concatenate([xe, xe]) if guided else xe      # (a guided loop holds the same point in both halves)
    return st


class _Run:
    """one launch of a hook on fresh guarded copies of the same inputs"""

    def __init__(self, be, st, prec, n_items, thr0):
        pr = PREC[prec]
        self.g = {k: Guarded(be, v.shape[0], LD, "f32", data=v, name=k) for k, v in st.items()}
        halves = st["xe"].shape[0]
        opw = LD if pr == 0 else 2 * LD      # (16-bit: the hi + lo pair)
        self.g["xe_op"] = Guarded(be, halves, opw, OP_KIND[pr], data=np.full((halves, opw), 0.5, np.float32), name="xe_op")
        self.g["thr"] = Guarded(be, 1, n_items, "f32", data=thr0, name="thr")

    def bits(self):
        return {k: g.read_bits() for k, g in self.g.items() if k != "x0"}

    def violations(self):
        return [v for g in self.g.values() for v in g.violations()]


def _hook_case(prec, guided, n_items, T, items, modes, ratios, maxv, lens, seed):
    """the new hook on all items at once against the existing hook with item b's record loop-wide, for every b: bytes of item b"""
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib, be = _lib.load(), DeviceBackend()
    pr = PREC[prec]
    coef_h = _tables7()
    coef, stepb = DevBuf.from_numpy(coef_h), DevBuf.from_numpy(np.array([STEP, 0, 0, 0], np.int32))
    scales = DevBuf.from_numpy(np.ascontiguousarray(SCALES7[:n_items])) if guided else None
    seeds, lens_d = DevBuf.from_numpy(np.ascontiguousarray(SEEDS7[:n_items])), DevBuf.from_numpy(np.ascontiguousarray(lens))
    st = _state(n_items, T, guided, seed)
    thr0 = -1.0 - np.arange(n_items, dtype=np.float32)
    n = n_items * T * LD
    new = _Run(be, st, prec, n_items, thr0)
    g = new.g
    _lib.check(lib.ns2vc_k_solver_update_items_corrected(coef.ptr, coef_h.shape[0], stepb.ptr, items.ctypes.data, n_items, g["x0"].ptr, g["xe"].ptr,
                                                         g["xe_op"].ptr, pr, g["xbar"].ptr, g["d1"].ptr, g["mprev"].ptr, g["mprev2"].ptr, n, LD, T,
                                                         scales.ptr if guided else None, seeds.ptr, lens_d.ptr, NC, modes.ctypes.data, ratios.ctypes.data,
                                                         maxv.ctypes.data, g["thr"].ptr, None), "k_solver_update_items_corrected")
    lib.ns2vc_dev_sync()
    assert not new.violations(), new.violations()
    got = new.bits()
    rows = lambda b, h=0, tot=n_items: slice((h * tot + b) * T, (h * tot + b + 1) * T)      # noqa: E731
    halves = 2 if guided else 1
    noisy = [b for b in range(n_items) if items[b, 3] & 2]
    for b in range(n_items):
        rec = items.copy()
        if b not in noisy:      # (the loop-wide hook refuses a correction beside a stochastic item: hold those; nothing in a step mixes items)
            for k in noisy:
                rec[k] = (0, 6, STEP + 1, 0)
        ref = _Run(be, st, prec, n_items, thr0)
        r = ref.g
        _lib.check(lib.ns2vc_k_solver_update_items(coef.ptr, coef_h.shape[0], stepb.ptr, rec.ctypes.data, n_items, r["x0"].ptr, r["xe"].ptr, r["xe_op"].ptr, pr,
                                                   r["xbar"].ptr, r["d1"].ptr, r["mprev"].ptr, r["mprev2"].ptr, n, LD, T, scales.ptr if guided else None,
                                                   seeds.ptr if b in noisy else None, lens_d.ptr, NC, int(modes[b]) if b not in noisy else 0,
                                                   float(ratios[b]), float(maxv[b]), r["thr"].ptr, None), "k_solver_update_items")
        lib.ns2vc_dev_sync()
        want = ref.bits()
        active = 0 <= STEP - items[b, 2] < items[b, 1]
        for k in ("xbar", "d1", "mprev", "mprev2"):
            assert np.array_equal(got[k][rows(b)], want[k][rows(b)]), (prec, guided, b, k)
        for h in range(halves):
            assert np.array_equal(got["xe"][rows(b, h)], want["xe"][rows(b, h)]), (prec, guided, b, "xe", h)
            assert np.array_equal(got["xe_op"][rows(b, h)], want["xe_op"][rows(b, h)]), (prec, guided, b, "xe_op", h)
        if active and modes[b] == 1:
            assert got["thr"][0, b] == want["thr"][0, b] and got["thr"][0, b] != thr0.view(np.uint32)[b], (prec, guided, b, "thr")
        else:      # held, uncorrected or clamped: the fill pattern stays
            assert got["thr"][0, b] == thr0.view(np.uint32)[b], (prec, guided, b, "thr fill")
        if not active:      # a held item keeps every byte
            for k in ("xbar", "d1", "mprev", "mprev2", "xe"):
                assert np.array_equal(got[k][rows(b)], st[k][rows(b)].view(np.uint32)), (b, k)
            assert (np.asarray(got["xe_op"][rows(b)]) == got["xe_op"][rows(b)][0, 0]).all()
        elif modes[b] != 0:      # the record acts: the corrected item differs from the uncorrected update of the same inputs
            assert not np.array_equal(got["mprev"][rows(b)], _uncorrected(lib, _lib, be, st, prec, n_items, T, items, coef, coef_h, stepb, scales, seeds,
                                                                           lens_d, guided, thr0)["mprev"][rows(b)]), (b, "mode has no effect")
    return got


_PLAIN = {}


def _uncorrected(lib, _lib, be, st, prec, n_items, T, items, coef, coef_h, stepb, scales, seeds, lens_d, guided, thr0):
    key = (prec, guided, n_items, T)
    if key not in _PLAIN:
        run = _Run(be, st, prec, n_items, thr0)
        r = run.g
        _lib.check(lib.ns2vc_k_solver_update_items(coef.ptr, coef_h.shape[0], stepb.ptr, items.ctypes.data, n_items, r["x0"].ptr, r["xe"].ptr, r["xe_op"].ptr,
                                                   PREC[prec], r["xbar"].ptr, r["d1"].ptr, r["mprev"].ptr, r["mprev2"].ptr, n_items * T * LD, LD, T,
                                                   scales.ptr if guided else None, seeds.ptr, lens_d.ptr, NC, 0, 0.995, 1.0, None, None), "k_solver_update_items")
        lib.ns2vc_dev_sync()
        _PLAIN[key] = run.bits()
    return _PLAIN[key]


@pytest.mark.parametrize("guided", [False, True], ids=["plain", "guided"])
@pytest.mark.parametrize("prec", ["fp32", "fp16", "bf16"])
def test_hook_every_item_has_the_bits_of_its_record_loop_wide(prec, guided):
    """T = 67, ld = 128, nc = 100, 7 items: mode 0 | mode 0 with noise | dynamic p = 0.37 | dynamic p = 0.9 under a max_val above the quantile |
    clamp | history 2 + dynamic | held; lens 67, 66, 33, 1, 40, 67, 50"""
    _hook_case(prec, guided, 7, 67, ITEMS7, MODES7, RATIOS7, MAXV7, LENS7, 70 + guided)


def test_hook_second_trip_of_the_grid_stride_loop():
    """3 items at T = 5500: n4 = 528 000 quads > 2048 x 256, so the quads of the last item are reached in the loop's second trip"""
    items = np.ascontiguousarray(ITEMS7[[2, 5, 4]])
    assert 3 * 5500 * LD // 4 > 2048 * 256
    _hook_case("fp32", False, 3, 5500, items, np.array([1, 1, 2], np.int32), np.array([0.37, 0.8, 0.5], np.float32), np.array([0.4, 0.3, 0.7], np.float32),
               np.array([5500, 4097, 5500], np.int32), 73)


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_hook_and_the_setter(weights):
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    coef_h = _tables7()
    coef, stepb = DevBuf.from_numpy(coef_h), DevBuf.from_numpy(np.array([STEP, 0, 0, 0], np.int32))
    T, n_items = 9, 2
    n = n_items * T * LD
    st = {k: np.random.default_rng(1).standard_normal(n).astype(np.float32) for k in ("x0", "xe", "xbar", "d1", "mprev", "mprev2")}
    bufs = {k: DevBuf.from_numpy(v) for k, v in st.items()}
    op, thr, seeds = DevBuf.from_numpy(np.zeros(n, np.float32)), DevBuf.from_numpy(np.zeros(4, np.float32)), DevBuf.from_numpy(np.arange(2, dtype=np.uint64))
    items = np.array([[0, 6, 2, 0], [NOISE_ROW0, 8, 1, 2]], np.int32)

    def hook(modes, ratios, maxv, it=items, table=True, thr_ptr=thr.ptr):
        m, r, v = np.array(modes, np.int32), np.array(ratios, np.float32), np.array(maxv, np.float32)
        return lib.ns2vc_k_solver_update_items_corrected(coef.ptr, coef_h.shape[0], stepb.ptr, it.ctypes.data, n_items, bufs["x0"].ptr, bufs["xe"].ptr, op.ptr, 0,
                                                         bufs["xbar"].ptr, bufs["d1"].ptr, bufs["mprev"].ptr, bufs["mprev2"].ptr, n, LD, T, None, seeds.ptr, None,
                                                         NC, m.ctypes.data if table else None, r.ctypes.data if table else None,
                                                         v.ctypes.data if table else None, thr_ptr, None)

    bad = [dict(modes=[3, 0], ratios=[0.5, 0.5], maxv=[1, 1]), dict(modes=[-1, 0], ratios=[0.5, 0.5], maxv=[1, 1]),
           dict(modes=[1, 0], ratios=[1.5, 0.5], maxv=[1, 1]), dict(modes=[1, 0], ratios=[-0.1, 0.5], maxv=[1, 1]),
           dict(modes=[1, 0], ratios=[float("nan"), 0.5], maxv=[1, 1]), dict(modes=[2, 0], ratios=[0.5, 0.5], maxv=[0.0, 1]),
           dict(modes=[2, 0], ratios=[0.5, 0.5], maxv=[float("inf"), 1]), dict(modes=[2, 0], ratios=[0.5, 0.5], maxv=[float("nan"), 1]),
           dict(modes=[0, 2], ratios=[0.5, 0.5], maxv=[1, 1]),                  # a corrected record on the noise item
           dict(modes=[0, 0], ratios=[0.5, 0.5], maxv=[1, 1], table=False),     # a NULL record table
           dict(modes=[1, 0], ratios=[0.5, 0.5], maxv=[1, 1], thr_ptr=None)]
    for kw in bad:
        assert hook(**kw) != 0 and lib.ns2vc_last_error(), kw
    lib.ns2vc_dev_sync()
    for k, v in st.items():      # nothing was launched
        assert np.array_equal(bufs[k].to_numpy((n,)), v), k
    assert hook([1, 0], [0.5, 0.5], [0.4, 1.0]) == 0      # (the same call with good records runs)

    x, c, p, _ = _inputs("icr", 2, 66, 5, 1)
    e = _engine(weights, "fp32", (2, 66, 5))
    try:
        for modes, ratios, maxv in (([3, 0], None, None), ([1, 0], [1.5, 0.5], None), (["clamp", None], None, [0.0, 1.0])):
            with pytest.raises(ValueError):      # the binding's own check (schedule.check_x0_correction)
                e.set_x0_correction_items(modes, ratios, maxv)
        one, two = np.ones(2, np.float32), np.array([1, 0], np.int32)
        for m, r, v in ((np.array([3, 0], np.int32), one * 0.5, one), (two, one * 1.5, one), (two, one * 0.5, one * 0), (two, one * 0.5, one * np.inf),
                        (two, one * 0.5, one * np.nan)):
            assert e.lib.ns2vc_sampler_set_x0_correction_items(e.h, m.ctypes.data, r.ctypes.data, v.ctypes.data, 2, None) != 0
        assert e.lib.ns2vc_sampler_set_x0_correction_items(e.h, two.ctypes.data, one.ctypes.data, one.ctypes.data, 3, None) != 0      # n != loop items
        assert e.lib.ns2vc_sampler_set_x0_correction_items(e.h, two.ctypes.data, None, one.ctypes.data, 2, None) != 0
        # the table together with the loop-wide setting, both ways, naming both calls
        e.set_x0_correction("clamp", 0.5, 0.7)
        with pytest.raises(Exception, match="ns2vc_sampler_set_x0_correction .*ns2vc_sampler_set_x0_correction_items"):
            e.set_x0_correction_items(["clamp", None])
        e.set_x0_correction(None)
        e.set_x0_correction_items(["clamp", None], None, [0.7, 1.0])
        with pytest.raises(Exception, match="ns2vc_sampler_set_x0_correction_items.*ns2vc_sampler_set_x0_correction"):
            e.set_x0_correction("clamp", 0.5, 0.7)
        e.set_x0_correction(None)      # (mode 0 is no setting: legal beside the table)
        # begin on a shared table with the table on
        e.load_sampler("unipc", 4, order=2)
        e.set_condition(c, p, None)
        y = x.clone()
        with pytest.raises(Exception, match="ns2vc_sampler_load_items"):
            e.sample(y, use_graph=True)
        assert np.array_equal(y.cpu().numpy(), x.cpu().numpy())
        # a corrected record on a stochastic item: refused when the schedules load, and again when the loop begins
        with pytest.raises(Exception, match="ddim / ddpm have no correction"):
            e.load_samplers([dict(solver="ddim", steps=4, eta=1.0), dict(solver="unipc", steps=4, order=2)], None, B64)
        e.set_x0_correction_items([None, "clamp"], None, [1.0, 0.7])
        e.load_samplers([dict(solver="ddim", steps=4, eta=1.0), dict(solver="unipc", steps=4, order=2)], None, B64)      # corrected and stochastic items share a loop
        e.set_x0_correction_items(["clamp", None], None, [0.7, 1.0])
        e.set_seeds([1, 2])
        with pytest.raises(Exception, match="ddim / ddpm have no correction"):
            e.sample(y, use_graph=True)
        e.set_x0_correction_items(None)
        e.sample(y, use_graph=True)      # off again: the loop runs
    finally:
        e.close()


# ---- 3. the loop through the engine ------------------------------------------------------------------------------------------------
B3, T3, LP3, STEPS3 = 4, 66, 5, 6
SCH3 = [dict(solver="ddim", steps=5, eta=1.0), dict(solver="unipc", steps=6, order=2), dict(solver="dpmsolver++", steps=5, order=3),
        dict(solver="unipc", steps=4, order=2)]
SEEDS3 = [11, 12, 13, 14]


def _kw(cor):
    """a corrections= entry -> the call-wide keywords of the same setting"""
    return {} if cor is None else dict(cor)


def _host(cor):
    """a corrections= entry -> the host statement's dict"""
    return None if cor is None else dict(mode=cor["correcting_x0_fn"], ratio=cor.get("dynamic_thresholding_ratio", 0.995),
                                         max_val=cor.get("thresholding_max_val", 1.0))


@pytest.fixture(scope="module")
def den32(weights):
    from ns2vc_amd.pipeline import Denoiser
    return Denoiser(weights, precision="fp32", precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None)


@pytest.fixture(scope="module")
def den16(weights):
    from ns2vc_amd.pipeline import Denoiser
    return Denoiser(weights, precision="fp16", precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None)


@pytest.fixture(scope="module")
def setting(weights):
    """the four settings from the ORACLE's first evaluation, as test_x0_correction_gpu.py derives its one: max_val = 0.8 x the smallest per-item
    quantile, so every dynamic item's threshold is its own quantile at step 0; asserted here: every corrected item clamps > 5 % of its elements at
    step 0, and the four settings give pairwise different latents in the host statement"""
    import torch
    from ns2vc_amd import schedule as S
    P = {k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}
    x, c, p, u = _inputs("ic3", B3, T3, LP3, 1)
    f = _plain_x0(P, c, p)
    t0 = S.build_table("unipc", STEPS3).t_model[0]
    m0 = f(x.cpu().numpy(), np.full((B3,), t0, np.float32))
    q = {r: [float(S.abs_quantile(m0[b], r)) for b in range(B3)] for r in (0.9, 0.7)}
    mv = 0.8 * min(q[0.9] + q[0.7])
    cors = [None, dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=0.9, thresholding_max_val=mv),
            dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=0.7, thresholding_max_val=0.75 * mv),
            dict(correcting_x0_fn="clamp", thresholding_max_val=min(q[0.9]))]
    s0 = [None, max(q[0.9][1], mv), max(q[0.7][2], 0.75 * mv), min(q[0.9])]
    clamped = [float(np.mean(np.abs(m0[b]) > s0[b])) for b in (1, 2, 3)]
    assert min(clamped) > 0.05, clamped
    f1 = _plain_x0(P, c[1:2], p[1:2])
    tab = S.build_table("unipc", STEPS3, order=2)
    lat = [S.run_table_numpy(tab, f1, x[1:2].cpu().numpy(), correct_x0=_host(cor)) for cor in cors]
    for i in range(4):
        for j in range(i + 1, 4):
            assert rel_l2(lat[i], lat[j]) > 1e-3, (i, j)
    return dict(cors=cors, inputs=(x, c, p, u), oracle=f, P=P)


def _sample(den, setting, graph=True, **kw):
    import torch
    x, c, p, u = setting["inputs"]
    y = den.sample(c, p, None, x, solver="unipc", steps=STEPS3, order=2, use_graph=graph, seeds=SEEDS3, **kw)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _per_item_equals_call_wide(den, setting, schedules=None, **kw):
    """item b of the mixed call == item b of the same call with b's setting call-wide (a DDIM item: with the uncorrected call)"""
    cors = setting["cors"]
    extra = {} if schedules is None else dict(schedules=schedules)
    y = _sample(den, setting, corrections=cors, **extra, **kw)
    assert np.isfinite(y).all()
    for b in range(B3):
        if schedules is not None and cors[b] is not None:      # (the call-wide setting is refused beside a DDIM item: hold a UniPC item in its place)
            ref_sch = [dict(solver="unipc", steps=5, order=2) if s["solver"] == "ddim" else s for s in schedules]
            ref = _sample(den, setting, schedules=ref_sch, **_kw(cors[b]), **kw)
        else:
            ref = _sample(den, setting, **extra, **_kw(cors[b]), **kw)
        assert np.array_equal(y[b], ref[b]), f"item {b} does not have the bits of its setting call-wide"
    return y


@pytest.mark.parametrize("mixed", [False, True], ids=["one-schedule", "schedules"])
def test_loop_items_have_the_bits_of_their_setting_call_wide(mixed, den32, setting, diag):
    """fp32, B = 4, T = 66, Lp = 5, 6 steps; corrections [None, dyn(0.9), dyn(0.7, other max_val), clamp], without and with schedules that mix DDIM
    eta 1 (item 0, None), UniPC order 2 and DPM-Solver++ order 3; captured == eager; every item within FP32_SAMPLED_TOL of run_tables_numpy driven
    by the oracle UNet"""
    from ns2vc_amd import noise as N
    from ns2vc_amd import schedule as S
    sch = SCH3 if mixed else None
    y = _per_item_equals_call_wide(den32, setting, sch)
    eager = _sample(den32, setting, graph=False, corrections=setting["cors"], **({} if sch is None else dict(schedules=sch)))
    assert den32.engine.x0_corrections is not None and den32.engine.tables is not None      # (the per-item path: records and the table)
    assert np.array_equal(y, eager), "hipGraph replay must be bit-identical to eager launches"
    x = setting["inputs"][0].cpu().numpy()
    specs = sch if mixed else [dict(solver="unipc", steps=STEPS3, order=2)] * B3
    tabs = S.build_tables(specs, None, S.linear_betas(1000, np.float64))
    ref = S.run_tables_numpy(tabs, setting["oracle"], x, noise_fn=lambda b, j: N.gauss(SEEDS3[b], j, 100, T3)[0],
                             correct_x0=[_host(cor) for cor in setting["cors"]])
    errs = [rel_l2(y[b], ref[b]) for b in range(B3)]
    diag(f"per-item x0 correction fp32 ({'mixed schedules' if mixed else 'one schedule'}) vs oracle, per item: " + " ".join(f"{v:.2e}" for v in errs))
    assert max(errs) < FP32_SAMPLED_TOL, errs


def test_guided_loop_items_have_the_bits_of_their_setting_call_wide(den32, setting):
    u = setting["inputs"][3]
    _per_item_equals_call_wide(den32, setting, guidance_scale=[2.5, 0.5, 1.0, 7.0], unconditional_prompt=u)


def test_ragged_loop_items_have_the_bits_of_their_setting_call_wide(den32, setting):
    """lengths (66, 65, 33, 41): the quantile of item b runs over its own L_b frames"""
    y = _per_item_equals_call_wide(den32, setting, lengths=[66, 65, 33, 41])
    for b, L in enumerate((66, 65, 33, 41)):
        assert not y[b, :, L:].any() and y[b, :, :L].any()


# ---- 4. no recapture ------------------------------------------------------------------------------------------------------------------
def test_values_replay_and_the_table_on_off_recaptures(weights, setting):
    import torch
    x, c, p, u = setting["inputs"]
    e = _engine(weights, "fp32", (B3, T3, LP3))

    def loop():
        y = x.clone()
        e.sample(y, use_graph=True)
        torch.cuda.synchronize()
        return y.cpu().numpy()

    try:
        e.set_condition(c, p, None)
        e.load_samplers([dict(solver="unipc", steps=4, order=2)] * 2 + [dict(solver="dpmsolver++", steps=4, order=3)] * 2)
        e.set_x0_correction_items([None, "dynamic_thresholding", "clamp", "dynamic_thresholding"], [0.5, 0.9, 0.5, 0.7], [1.0, 0.5, 0.7, 0.4])
        a = loop()
        caps = e.graph_captures()
        assert np.array_equal(loop(), a) and e.graph_captures() == caps
        e.set_x0_correction_items(["clamp", "dynamic_thresholding", None, "dynamic_thresholding"], [0.5, 0.8, 0.5, 0.6], [0.6, 0.45, 0.7, 0.3])
        b = loop()
        assert e.graph_captures() == caps, "new records must replay the captured step graph"
        assert all(not np.array_equal(a[k], b[k]) for k in range(4))
        e.set_x0_correction_items(None)
        off = loop()
        assert e.graph_captures() == caps + 1
        e.set_x0_correction_items([None] * 4)
        assert np.array_equal(loop(), off) and e.graph_captures() == caps + 2      # every record off == the table off
        # the loop-wide path as before: a value no launch takes replays, one a launch takes recaptures
        e.set_x0_correction_items(None)
        e.load_sampler("unipc", 4, order=2)
        e.set_x0_correction("clamp", 0.5, 0.7)
        w = loop()
        caps = e.graph_captures()
        e.set_x0_correction("clamp", 0.9, 0.7)
        assert np.array_equal(loop(), w) and e.graph_captures() == caps
        e.set_x0_correction("clamp", 0.9, 0.6)
        assert not np.array_equal(loop(), w) and e.graph_captures() == caps + 1
    finally:
        e.close()


# ---- 5. the hand-off ------------------------------------------------------------------------------------------------------------------
def test_handoff_carries_the_table(den16, setting):
    """fp16 head with an fp32 tail of 2 evaluations under the mixed table: per item the bits of the same loop with its setting call-wide"""
    _per_item_equals_call_wide(den16, setting, tail_fp32=2)
    assert den16.tail_engine is not None


# ---- 6. the slot loop -----------------------------------------------------------------------------------------------------------------
DYN6 = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=0.9, thresholding_max_val=0.5)
DYN6B = dict(correcting_x0_fn="dynamic_thresholding", dynamic_thresholding_ratio=0.7, thresholding_max_val=0.3)
CLAMP6 = dict(correcting_x0_fn="clamp", thresholding_max_val=0.8)
FORMS6 = dict(order3=True, stochastic=True, item_corrections=True)


def _rq(name, slot, schedule, correction, seed=0):
    return dict(_request(name, slot, schedule, seed=seed), correction=correction)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_slot_loop_requests_bring_their_own_correction(prec, den32, den16):
    """admissions at loop steps 0, 2 and 5 with different corrections, a DDIM eta 1 request with None among them, slot 1 reused after its take:
    every result is the request alone in its slot from loop step 0 with the others idle, by bits; nothing recaptures"""
    den = den32 if prec == "fp32" else den16
    rq = dict(A=(_rq("A", 0, U6, DYN6, 21), 0), B1=(_rq("B1", 1, U4, CLAMP6, 22), 0), C=(_rq("C", 2, DDIM6, None, 23), 2),
              B2=(_rq("B2", 1, U3_6, DYN6B, 24), 5))
    full, caps0, caps1 = _drive(den, rq, True, **FORMS6)
    assert sorted(full) == ["A", "B1", "B2", "C"] and all(np.isfinite(v).all() for v in full.values())
    assert caps1 == caps0, f"admissions recaptured the step graph ({caps0} -> {caps1})"
    for name, (r, _) in rq.items():
        alone, _, _ = _drive(den, {name: (r, 0)}, True, **FORMS6)
        assert np.array_equal(full[name], alone[name]), f"{name} depends on when it was admitted or on its neighbours"
        assert not full[name][:, LENS[r["slot"]]:].any()
    plain, _, _ = _drive(den, dict(A=(_rq("A", 0, U6, None, 21), 0)), True, **FORMS6)
    assert rel_l2(full["A"], plain["A"]) > 1e-3      # the request's correction acts


def test_slot_loop_equals_the_loop_wide_slot_loop(den32):
    """a corrected request in a loop opened with the table == the same request in a loop opened with its setting loop-wide"""
    a, _, _ = _drive(den32, dict(A=(_rq("A", 0, U6, DYN6, 21), 0), B=(_rq("B", 1, U4, CLAMP6, 22), 1)), True, order3=True, item_corrections=True)
    for name, slot, sch, cor, start in (("A", 0, U6, DYN6, 0), ("B", 1, U4, CLAMP6, 1)):
        w, _, _ = _drive(den32, {name: (_request(name, slot, sch, seed=0), start)}, True, order3=True, **cor)
        assert np.array_equal(a[name], w[name]), name


def test_converters_honour_segment_correction(pre_model, den32, weights, diag):  # noqa: F811
    """5 segments with three different corrections on 3 slots: every segment against the segment converted alone (GroupedConverter, batches of one,
    the same x_T per segment; engine shapes differ, so the project's bound for fp32 sampled latents, not bits); a group of segments with different
    corrections through GroupedConverter(ragged) too"""
    import torch
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import ContinuousConverter, GroupedConverter, Segment
    from ns2vc_amd.weights import hash_normal
    shapes = [(66, 5), (65, 3), (33, 5), (48, 4), (66, 2)]
    cors = [DYN6, None, CLAMP6, DYN6B, DYN6]
    segs = [Segment(torch.from_numpy(hash_normal(f"ic.c{i}", (256, T))), torch.from_numpy(hash_normal(f"ic.r{i}", (100, L))), tag=i,
                    schedule=dict(solver="unipc", steps=(4, 6)[i % 2], order=2), correction=cors[i]) for i, (T, L) in enumerate(shapes)]
    out = ContinuousConverter(pre_model, den32, slots=3, max_frames=66, max_prompt=5, solver="unipc", steps=5, item_corrections=True).convert(segs)
    ref_den = Denoiser(weights, precision="fp32", precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None)
    one = GroupedConverter(pre_model, ref_den, max_batch=1, solver="unipc", steps=5).convert(segs)
    plain = GroupedConverter(pre_model, ref_den, max_batch=1, solver="unipc", steps=5).convert([Segment(s.content, s.refer, s.tag, s.schedule) for s in segs])
    grouped = GroupedConverter(pre_model, ref_den, max_batch=5, solver="unipc", steps=5, ragged=True, ragged_prompts=True).convert(segs)
    errs, gerrs = [], []
    for i, (T, _) in enumerate(shapes):
        assert out[i].shape == (100, T) and torch.isfinite(out[i]).all()
        errs.append(rel_l2(out[i].cpu().numpy(), one[i].cpu().numpy()))
        gerrs.append(rel_l2(grouped[i].cpu().numpy(), one[i].cpu().numpy()))
        if cors[i] is not None:
            assert rel_l2(one[i].cpu().numpy(), plain[i].cpu().numpy()) > 1e-3, i
    diag("per-item corrections, 5 segments: continuous vs alone " + " ".join(f"{v:.2e}" for v in errs) + "; grouped vs alone " +
         " ".join(f"{v:.2e}" for v in gerrs))
    assert max(errs) < FP32_SAMPLED_TOL, errs
    assert max(gerrs) < 1e-4, gerrs      # (tests/test_item_schedules_gpu.py: a batched against a differently batched fp32 run)


# ---- 7. old paths keep their kernels ---------------------------------------------------------------------------------------------------
def test_calls_without_the_feature_leave_the_table_off(den32, setting):
    """a call without corrections= and a slot loop opened without item_corrections run with the table off (the parent's launches), also after a
    call that had it on"""
    _sample(den32, setting, corrections=setting["cors"])
    assert den32.engine.x0_corrections is not None
    a = _sample(den32, setting)
    assert den32.engine.x0_corrections is None and den32.engine.x0_correction is None
    b = _sample(den32, setting, **_kw(setting["cors"][3]))
    assert den32.engine.x0_corrections is None and den32.engine.x0_correction is not None
    assert np.array_equal(_sample(den32, setting), a) and not np.array_equal(a[3], b[3])
    _drive(den32, dict(A=(_request("A", 0, U6), 0)), True)
    assert den32.engine.x0_corrections is None
