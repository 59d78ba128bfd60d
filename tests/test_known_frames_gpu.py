"""Known frames on the MI355X: the hold launch alone on guarded tensors (ns2vc_k_hold_x0), the captured loop against the closed form
x_end = alpha_end k + sigma_end eps of a held frame and against ``schedule.run_table_numpy(hold=)``, graph == eager and what recaptures, the fp16
engine with its tail, guidance, ragged batches, per-item schedules, ``denoise_to_zero`` and ``Denoiser.sample_long``."""
import numpy as np
import pytest

from guard import DeviceBackend, Guarded
from util import fmt_local, local_errors, rel_l2

pytestmark = pytest.mark.gpu
FP32_TOL = 5e-5             # the project's fp32 sampled-latent gate (tests/test_solvers_gpu.py); also the bound of a held frame against the closed
CLOSED_TOL = 5e-5           # form in EVERY precision: the update runs in fp32 on an fp32 x0 whatever the operand type
FP32_LOCAL_TOL = 2e-4       # per frame / channel (tests/test_solvers_gpu.py)
FP16_TOL = 1e-3             # the parity bar
LP = 16


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


@pytest.fixture(scope="module")
def den32(weights):
    from ns2vc_amd.pipeline import Denoiser
    return Denoiser(weights, precision="fp32")


def _inputs(tag, B, T, Lp=LP):
    import torch
    from ns2vc_amd.weights import hash_normal
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(hash_normal(f"kf.{tag}.c", (B, 256, T))).to(dev)
    p = torch.from_numpy(hash_normal(f"kf.{tag}.p", (B, Lp, 256))).to(dev)
    x = torch.from_numpy(hash_normal(f"kf.{tag}.x", (B, 100, T))).to(dev)
    k = torch.from_numpy((0.6 * hash_normal(f"kf.{tag}.k", (B, 100, T))).astype(np.float32)).to(dev)
    return c, p, x, k


def _end(table):
    """(alpha, sigma) of the point the table's last row lands on; (1, 0) where that row returns x_start (denoise_to_zero, ddim)"""
    from ns2vc_amd import schedule as S
    if table.coef[-1, 5] == 0 and table.coef[-1, 6] == -1:
        return 1.0, 0.0
    sched = S.VPSchedule(S.linear_betas())
    t = float(table.timesteps[-1])
    return sched.alpha(t), sched.sigma(t)


def _closed_err(y, k, x, mask, table):
    """rel-L2 of the held frames of y (one item or a batch) against alpha_end k + sigma_end eps"""
    a, s = _end(table)
    m3 = np.broadcast_to(mask[..., None, :], y.shape)
    want = a * k.astype(np.float64) + s * x.astype(np.float64)
    return rel_l2(y[m3], want[m3])


# ---- 1. the launch alone ---------------------------------------------------------------------------------------------------------------------
def _masks(n, T):
    isl = np.zeros((n, T), dtype=bool)
    isl[0, T // 3:T // 3 + max(1, T // 4)] = True
    isl[n - 1, T // 2] = True
    first, last = np.zeros((n, T), dtype=bool), np.zeros((n, T), dtype=bool)
    first[:, 0] = True
    last[1:, T - 1] = True
    return {"none": np.zeros((n, T), dtype=bool), "all": np.ones((n, T), dtype=bool), "first": first, "last": last, "island": isl}


@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("nc", [100, 80])
@pytest.mark.parametrize("T", [1, 5, 67])
def test_k_hold_x0_writes_the_held_rows_and_nothing_else(T, nc, halves):
    from ns2vc_amd import _lib
    lib, be = _lib.load(), DeviceBackend()
    n, ld = 3, 128
    rng = np.random.default_rng(T * 1000 + nc + halves)
    x0_host = rng.standard_normal((halves * n * T, ld)).astype(np.float32)
    kn_host = rng.standard_normal((n * T, ld)).astype(np.float32)          # (the pad columns hold values too: they must not arrive)
    for name, mask in _masks(n, T).items():
        x0 = Guarded(be, halves * n * T, ld, "f32", data=x0_host, name="x0")
        kn = Guarded(be, n * T, ld, "f32", data=kn_host, name="known")
        m8 = np.ascontiguousarray(mask, dtype=np.uint8)
        _lib.check(lib.ns2vc_k_hold_x0(x0.ptr, kn.ptr, m8.ctypes.data, n, T, ld, nc, halves, None), "k_hold_x0")
        got = x0.read_bits().reshape(halves, n * T, ld)
        held = mask.reshape(-1)
        want = x0_host.view(np.uint32).reshape(halves, n * T, ld).copy()
        want[:, held, :nc] = kn_host.view(np.uint32)[held, :nc]          # the known values, bit for bit, in every half
        want[:, held, nc:] = 0                                            # the pad columns of a held row: +0.0
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
        assert np.array_equal(kn.read_bits(), kn_host.view(np.uint32))
        assert x0.violations() == [] and kn.violations() == [], name
        x0.free()
        kn.free()


@pytest.mark.parametrize("T,nc,halves,which", [(5, 98, 2, "island"), (67, 98, 1, "all"), (5, 2, 1, "all"), (1500, 100, 2, "all"), (1500, 98, 1, "most")])
def test_k_hold_x0_partial_quads_and_a_second_grid_pass(T, nc, halves, which):
    """nc no multiple of 4 (latent 98: the last quad of a row is half known, half pad; nc = 2: the first quad is) and more held rows than the
    grid covers in one pass (512 workgroups x 256 threads / 32 quads = 4096 rows < 3 x 1500)"""
    from ns2vc_amd import _lib
    lib, be = _lib.load(), DeviceBackend()
    n, ld = 3, 128
    rng = np.random.default_rng(T + nc)
    x0_host = rng.standard_normal((halves * n * T, ld)).astype(np.float32)
    kn_host = rng.standard_normal((n * T, ld)).astype(np.float32)
    if which == "most":
        mask = rng.random((n, T)) < 0.95
        mask[:, -1] = True
    else:
        mask = _masks(n, T)[which]
    x0 = Guarded(be, halves * n * T, ld, "f32", data=x0_host, name="x0")
    kn = Guarded(be, n * T, ld, "f32", data=kn_host, name="known")
    m8 = np.ascontiguousarray(mask, dtype=np.uint8)
    _lib.check(lib.ns2vc_k_hold_x0(x0.ptr, kn.ptr, m8.ctypes.data, n, T, ld, nc, halves, None), "k_hold_x0")
    got = x0.read_bits().reshape(halves, n * T, ld)
    held = mask.reshape(-1)
    want = x0_host.view(np.uint32).reshape(halves, n * T, ld).copy()
    want[:, held, :nc] = kn_host.view(np.uint32)[held, :nc]
    want[:, held, nc:] = 0
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert x0.violations() == [] and kn.violations() == []


def test_k_hold_x0_refuses_bad_arguments():
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    buf = DevBuf(4 * 128 * 4)
    m = np.ones((1, 4), dtype=np.uint8)
    for n, T, ld, nc, halves in ((0, 4, 128, 100, 1), (1, 4, 126, 100, 1), (1, 4, 128, 129, 1), (1, 4, 128, 0, 1), (1, 4, 128, 100, 3)):
        assert lib.ns2vc_k_hold_x0(buf.ptr, buf.ptr, m.ctypes.data, n, T, ld, nc, halves, None) != 0
    assert lib.ns2vc_k_hold_x0(buf.ptr, None, m.ctypes.data, 1, 4, 128, 100, 1, None) != 0


# ---- 2. the fp32 loop --------------------------------------------------------------------------------------------------------------------------
def _mask_2(T=131):
    m = np.zeros((3, T), dtype=bool)
    m[0, :7] = True
    m[2, 60:70] = True
    m[2, 130] = True
    return m


@pytest.fixture(scope="module")
def loop32(den32):
    """the fp32 loop of test 2, run once: inputs, the held result, the unheld result"""
    c, p, x, k = _inputs("l32", 3, 131)
    mask = _mask_2()
    y = den32.sample(c, p, None, x, solver="unipc", steps=8, order=2, known=k, known_mask=mask).cpu().numpy()
    plain = den32.sample(c, p, None, x, solver="unipc", steps=8, order=2).cpu().numpy()
    return dict(c=c, p=p, x=x, k=k, mask=mask, y=y, plain=plain)


def test_fp32_loop_held_frames_follow_the_closed_form(loop32, diag):
    from ns2vc_amd import schedule as S
    table = S.build_table("unipc", 8, order=2)
    e = _closed_err(loop32["y"], loop32["k"].cpu().numpy(), loop32["x"].cpu().numpy(), loop32["mask"], table)
    diag(f"known frames fp32 unipc-2 8 steps: held frames vs the closed form {e:.2e}")
    assert e < CLOSED_TOL


def test_fp32_loop_matches_the_host_statement(loop32, den32, diag):
    import torch
    from ns2vc_amd import schedule as S
    table = S.build_table("unipc", 8, order=2)
    c, p, mask = loop32["c"], loop32["p"], loop32["mask"]
    x, k = loop32["x"].cpu().numpy(), loop32["k"].cpu().numpy()

    def x0_fn(xx, tt):
        dev = c.device
        return den32.denoise(torch.from_numpy(np.ascontiguousarray(xx)).to(dev), torch.from_numpy(np.ascontiguousarray(tt)).to(dev), c, p).cpu().numpy()

    ref = S.run_table_numpy(table, x0_fn, S.known_start(x, k, mask, table.coef[0]), hold=(k, mask))
    e, loc = rel_l2(loop32["y"], ref), local_errors(loop32["y"], ref)
    diag(f"known frames fp32 unipc-2 8 steps: latent vs run_table_numpy(hold=) {e:.2e}  {fmt_local(loc)}")
    assert e < FP32_TOL and loc["frame"] < FP32_LOCAL_TOL and loc["chan"] < FP32_LOCAL_TOL


def test_fp32_loop_an_item_without_known_frames_keeps_its_bits(loop32):
    y, plain, mask = loop32["y"], loop32["plain"], loop32["mask"]
    assert np.array_equal(y[1], plain[1])                                   # item 1 holds nothing
    assert not np.array_equal(y[0][:, ~mask[0]], plain[0][:, ~mask[0]])     # item 0's free frames were generated next to the held ones


# ---- 3. graph and eager, and what recaptures -----------------------------------------------------------------------------------------------------
def test_graph_equals_eager_and_new_values_replay(loop32, den32):
    c, p, x, k, mask = (loop32[n] for n in ("c", "p", "x", "k", "mask"))
    kw = dict(solver="unipc", steps=8, order=2)
    g = den32.sample(c, p, None, x, known=k, known_mask=mask, **kw).cpu().numpy()
    n0 = den32.engine.graph_captures()
    ea = den32.sample(c, p, None, x, use_graph=False, known=k, known_mask=mask, **kw).cpu().numpy()
    assert np.array_equal(g, ea) and np.array_equal(g, loop32["y"])
    mask2 = np.roll(mask, 3, axis=1)
    mask2[1, 40:44] = True
    g2 = den32.sample(c, p, None, x, known=(k * 0.5).contiguous(), known_mask=mask2, **kw).cpu().numpy()
    assert den32.engine.graph_captures() == n0                              # new values, a new mask of the same shape: a replay
    assert not np.array_equal(g2, g)
    den32.sample(c, p, None, x, **kw)
    n1 = den32.engine.graph_captures()
    assert n1 == n0 + 1                                                     # off: the step loses a launch
    g3 = den32.sample(c, p, None, x, known=k, known_mask=mask, **kw).cpu().numpy()
    assert den32.engine.graph_captures() == n1 + 1                          # and on again
    assert np.array_equal(g3, g)


def test_the_engine_refuses_what_the_hold_excludes(weights):
    import torch
    from ns2vc_amd.engine import Engine
    from ns2vc_amd._lib import Ns2vcError
    e = Engine(precision="fp32")
    try:
        e.load_state_dict(weights)
        e.prepare(2, 16, LP)
        k = torch.zeros((2, 100, 16), device="cuda")
        m = np.zeros((2, 16), dtype=bool)
        m[0, 15] = True
        e.set_known(k, m)
        for call in (lambda: e.set_x0_correction("clamp"), lambda: e.set_x0_correction_items(["clamp", None]), lambda: e.open_slots()):
            with pytest.raises(Ns2vcError, match="known frames"):
                call()
        e.set_lengths([15, 16])
        e.load_sampler("unipc", 4)
        with pytest.raises(Ns2vcError, match="at or past its length"):
            e.sample_begin(k)
        with pytest.raises(Ns2vcError, match="at or past its length"):
            e.set_known(k, m)
        e.set_known(None, None)
        e.set_x0_correction("clamp")
        with pytest.raises(Ns2vcError, match="x0 correction"):
            e.set_known(k, np.zeros((2, 16), dtype=bool))
        e.set_x0_correction(None)
        torch.cuda.synchronize()
    finally:
        e.close()


def test_handoff_and_slot_loop_refusals(weights):
    """two engines that disagree on the hold do not hand a loop over; an open slot loop takes no known frames"""
    import torch
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import Engine
    from ns2vc_amd._lib import Ns2vcError
    engs = [Engine(precision="fp32") for _ in range(2)]
    try:
        c, p, x, k = _inputs("ho", 2, 16)
        m = np.zeros((2, 16), dtype=bool)
        m[1, 4:9] = True
        for e in engs:
            e.load_state_dict(weights)
            e.prepare(2, 16, LP)
            e.load_sampler("unipc", 4)
            e.set_condition(c, p, None)
        engs[0].set_known(k, m)
        xx = x.clone()
        with pytest.raises(Ns2vcError, match="disagree on known frames"):
            engs[0].sample(xx, tail=engs[1], tail_steps=2)
        engs[0].sample_end(xx)                                  # (the refused hand-off left the head's loop open)
        xx = x.clone()
        with pytest.raises(Ns2vcError, match="disagree on known frames"):
            engs[1].sample(xx, tail=engs[0], tail_steps=2)
        engs[1].sample_end(xx)
        engs[1].set_known(k, m)                                 # on both: the loop runs, and equals the one-engine loop
        xx, one = x.clone(), x.clone()
        engs[0].sample(xx, tail=engs[1], tail_steps=2)
        engs[0].sample(one)
        torch.cuda.synchronize()
        assert torch.equal(xx, one)
        engs[1].set_known(None, None)
        engs[1].open_slots()
        with pytest.raises(Ns2vcError, match="slot loop is open"):
            engs[1].set_known(k, m)
        assert _lib.load().ns2vc_dev_sync() == 0
    finally:
        for e in engs:
            e.close()


def test_open_slots_after_a_held_call_at_the_same_shape(den32):
    """the hold a sample(known=) left in the engine does not stand in the way of a slot loop at the same shape"""
    c, p, x, k = _inputs("os", 2, 66)
    m = np.zeros((2, 66), dtype=bool)
    m[0, :9] = True
    den32.sample(c, p, None, x, solver="unipc", steps=4, known=k, known_mask=m)
    assert den32.engine.hold is not None
    loop = den32.open_slots(2, 66, LP)
    try:
        assert den32.engine.hold is None and loop.idle() == [0, 1]
    finally:
        loop.close()


# ---- 4. fp16 with its default tail ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["unipc", "dpmsolver++"])      # (default tails 0 and 2: the second hands the loop to the fp32 engine, hold and all)
def test_fp16_loop_with_its_default_tail(solver, weights, loop32, den32, diag):
    from ns2vc_amd import schedule as S
    from ns2vc_amd.pipeline import Denoiser
    c, p, x, k, mask = (loop32[n] for n in ("c", "p", "x", "k", "mask"))
    kw = dict(solver=solver, steps=8, order=2)
    y16 = Denoiser(weights, precision="fp16").sample(c, p, None, x, known=k, known_mask=mask, **kw).cpu().numpy()
    y32 = loop32["y"] if solver == "unipc" else den32.sample(c, p, None, x, known=k, known_mask=mask, **kw).cpu().numpy()
    e_closed = _closed_err(y16, k.cpu().numpy(), x.cpu().numpy(), mask, S.build_table(solver, 8, order=2))
    e = rel_l2(y16, y32)
    diag(f"known frames fp16 {solver}-2 8 steps: held frames vs the closed form {e_closed:.2e}, latent vs the fp32 engine {e:.2e}")
    assert e_closed < CLOSED_TOL
    assert e < FP16_TOL


# ---- 5. guidance -----------------------------------------------------------------------------------------------------------------------------------
def test_guided_loop_holds_both_halves(den32, diag):
    import torch
    from ns2vc_amd import schedule as S
    from ns2vc_amd.weights import hash_normal
    c, p, x, k = _inputs("gd", 2, 66)
    up = torch.from_numpy(hash_normal("kf.gd.up", (1, LP, 256))).to(c.device)
    mask = np.zeros((2, 66), dtype=bool)
    mask[0, 10:20] = True
    mask[1, :5] = True
    mask[1, 65] = True
    y = den32.sample(c, p, None, x, solver="unipc", steps=8, order=2, guidance_scale=np.array([2.5, 1.0], np.float32), unconditional_prompt=up,
                     known=k, known_mask=mask).cpu().numpy()
    table = S.build_table("unipc", 8, order=2)
    for b in range(2):
        e = _closed_err(y[b], k[b].cpu().numpy(), x[b].cpu().numpy(), mask[b], table)
        diag(f"known frames guided item {b} (scale {[2.5, 1.0][b]}): held frames vs the closed form {e:.2e}")
        assert e < CLOSED_TOL
    assert np.isfinite(y).all()


# ---- 6. ragged -------------------------------------------------------------------------------------------------------------------------------------
def test_ragged_batch_holds_up_to_each_items_last_frame(den32, diag):
    from ns2vc_amd import schedule as S
    lens = [131, 90, 66]
    T = max(lens)
    c, p, x, k = _inputs("rg", 3, T)
    mask = np.zeros((3, T), dtype=bool)
    for b, L in enumerate(lens):
        mask[b, L - 4:L] = True           # ... the item's last valid frame among them
    mask[1, :6] = True
    kw = dict(solver="unipc", steps=8, order=2)
    y = den32.sample(c, p, None, x, lengths=lens, known=k, known_mask=mask, **kw).cpu().numpy()
    table = S.build_table("unipc", 8, order=2)
    worst = 0.0
    for b, L in enumerate(lens):
        assert float(np.abs(y[b, :, L:]).max() if L < T else 0.0) == 0.0
        e = _closed_err(y[b], k[b].cpu().numpy(), x[b].cpu().numpy(), mask[b], table)
        assert e < CLOSED_TOL, b
        one = den32.sample(c[b:b + 1, :, :L].contiguous(), p[b:b + 1], None, x[b:b + 1, :, :L].contiguous(), known=k[b:b + 1, :, :L].contiguous(),
                           known_mask=mask[b:b + 1, :L], **kw).cpu().numpy()
        worst = max(worst, rel_l2(y[b, :, :L], one[0]))
    diag(f"known frames ragged fp32: worst item vs alone {worst:.2e}")
    assert worst < 1e-5


# ---- 7. per-item schedules -------------------------------------------------------------------------------------------------------------------------
def test_per_item_schedules_each_item_its_own_closed_form(den32, diag):
    from ns2vc_amd import schedule as S
    c, p, x, k = _inputs("it", 3, 66)
    specs = [dict(solver="unipc", steps=6), dict(solver="dpmsolver++", steps=8, order=3), dict(solver="ddim", steps=5, eta=0.5)]
    mask = np.zeros((3, 66), dtype=bool)
    mask[0, :8] = True
    mask[1, 30:40] = True
    mask[2, 50:66] = True
    y = den32.sample(c, p, None, x, schedules=specs, seeds=[3, 4, 5], known=k, known_mask=mask).cpu().numpy()
    b64 = S.linear_betas(1000, np.float64)
    tables = [S.build_table("unipc", 6), S.build_table("dpmsolver++", 8, order=3), S.build_table("ddim", 5, b64, 2, 0.5)]
    for b, table in enumerate(tables):
        e = _closed_err(y[b], k[b].cpu().numpy(), x[b].cpu().numpy(), mask[b], table)
        diag(f"known frames per-item schedules, item {b} ({table.solver}): held frames vs its closed form {e:.2e}")
        assert e < CLOSED_TOL, b
    assert rel_l2(y[2][:, mask[2]], k[2].cpu().numpy()[:, mask[2]]) < CLOSED_TOL      # the ddim item ends on k itself


# ---- 8. denoise_to_zero ------------------------------------------------------------------------------------------------------------------------------
def test_denoise_to_zero_ends_on_the_known_latent(loop32, den32, diag):
    c, p, x, k, mask = (loop32[n] for n in ("c", "p", "x", "k", "mask"))
    y = den32.sample(c, p, None, x, solver="unipc", steps=8, order=2, denoise_to_zero=True, known=k, known_mask=mask).cpu().numpy()
    m3 = np.broadcast_to(mask[:, None, :], y.shape)
    e = rel_l2(y[m3], k.cpu().numpy()[m3])
    diag(f"known frames denoise_to_zero: held frames vs k {e:.2e}")
    assert e < CLOSED_TOL


# ---- 9. sample_long ------------------------------------------------------------------------------------------------------------------------------------
def test_sample_long_is_the_chain_of_held_chunks(den32, diag):
    import torch
    from ns2vc_amd import schedule as S
    lens, chunk, V = [300, 170], 128, 16
    c, p, x, _ = _inputs("lg", 2, 300)
    kw = dict(solver="unipc", steps=6)
    y = den32.sample_long(c, p, None, x, chunk_frames=chunk, overlap_frames=V, lengths=lens, **kw)
    # the chain by hand
    plans = [S.plan_chunks(L, chunk, V) for L in lens]
    assert plans == [[(0, 128), (112, 240), (224, 300)], [(0, 128), (112, 170)]]
    want = torch.zeros_like(y)
    heads = {}
    for j in range(3):
        items = [b for b in range(2) if len(plans[b]) > j]
        Lj = [plans[b][j][1] - plans[b][j][0] for b in items]
        Tj = max(Lj)
        cj, xj, kj = c.new_zeros((len(items), 256, Tj)), x.new_zeros((len(items), 100, Tj)), x.new_zeros((len(items), 100, Tj))
        mj = np.zeros((len(items), Tj), dtype=bool)
        for i, b in enumerate(items):
            s0, s1 = plans[b][j]
            cj[i, :, :s1 - s0], xj[i, :, :s1 - s0] = c[b, :, s0:s1], x[b, :, s0:s1]
            if j:
                kj[i, :, :V], mj[i, :V] = want[b, :, s0:s0 + V], True
        hold = dict(known=kj, known_mask=mj) if j else {}
        yj = den32.sample(cj, p[items], None, xj, lengths=np.asarray(Lj, np.int32), **hold, **kw)
        for i, b in enumerate(items):
            s0, s1 = plans[b][j]
            keep = V if j else 0
            want[b, :, s0 + keep:s1] = yj[i, :, keep:s1 - s0]
            heads[(b, j)] = yj[i, :, :V].clone()
    assert torch.equal(y, want)
    y = y.cpu().numpy()
    for b, L in enumerate(lens):
        assert float(np.abs(y[b, :, L:]).max() if L < 300 else 0.0) == 0.0
    # the overlap frames of the output are the EARLIER chunk's; the later chunk's own copy of them stands on the closed form, beside them
    assert not torch.equal(heads[(0, 1)], want[0, :, 112:128])
    # behind a seam the chained chunks differ from independent ones; in front of the first seam they are the same chunk 0
    ind = den32.sample_long(c, p, None, x, chunk_frames=chunk, overlap_frames=0, lengths=lens, **kw).cpu().numpy()
    assert np.array_equal(ind[:, :, :112], y[:, :, :112])
    assert not np.array_equal(ind[0, :, 128:240], y[0, :, 128:240]) and not np.array_equal(ind[1, :, 128:170], y[1, :, 128:170])
    # an utterance batch that fits one chunk is the plain call
    cs, xs = c[:, :, :100].contiguous(), x[:, :, :100].contiguous()
    a = den32.sample_long(cs, p, None, xs, chunk_frames=chunk, overlap_frames=V, **kw)
    assert torch.equal(a, den32.sample(cs, p, None, xs, **kw))
    a = den32.sample_long(cs, p, None, xs, chunk_frames=chunk, overlap_frames=V, lengths=[100, 70], **kw)
    assert torch.equal(a, den32.sample(cs, p, None, xs, lengths=[100, 70], **kw))
