"""Known frames in the slot loop on the MI355X: the two kernels alone on guarded / patterned tensors (ns2vc_k_hold_slots,
ns2vc_k_known_items), the slot loop's contract extended by the hold -- closed form of a held frame, a held request admitted in mid-loop ends on the
bits it gets alone, every slot filled at step 0 is ``Denoiser.sample(known=)``, unheld requests keep plain-loop bits, a take clears its slot --
in fp32 and fp16, guided, with ddim, against ``schedule.run_slots_numpy``, captured and eager, the engine's refusals, and
``ContinuousConverter(overlap_frames=)`` against the hand-written chain of ``Denoiser.sample(known=)`` calls."""
import numpy as np
import pytest

from guard import DeviceBackend, Guarded
from util import fmt_local, local_errors, rel_l2

pytestmark = pytest.mark.gpu
FP32_TOL = 5e-5             # the project's fp32 sampled-latent gate
CLOSED_TOL = 5e-5           # a held frame against the closed form, in every precision (tests/test_known_frames_gpu.py)
FP32_LOCAL_TOL = 2e-4       # per frame / channel
SHAPE = (3, 66, 5)          # the slot shape of tests/test_continuous_gpu.py
LENS, PLENS = (66, 65, 33), (5, 1, 3)


@pytest.fixture(scope="module")
def weights():
    from ns2vc_amd.weights import procedural_state_dict
    return procedural_state_dict(seed=0)


@pytest.fixture(scope="module")
def denoisers(weights):
    from ns2vc_amd.pipeline import Denoiser
    return {prec: Denoiser(weights, precision=prec, precision_check=None, tail_fp32=0, ln_guard=None, attn_fallback_limit=None) for prec in ("fp32", "fp16")}


# ---- 1. the two kernels alone -------------------------------------------------------------------------------------------------------------------
def _masks(n, T):
    rows = n * T
    flat = lambda idx: np.isin(np.arange(rows), idx).reshape(n, T)      # noqa: E731
    out = {"none": np.zeros((n, T), dtype=bool), "all": np.ones((n, T), dtype=bool), "first": flat([0]), "last": flat([rows - 1]),
           "wave": flat([r for r in (63, 64) if r < rows]), "second": (np.arange(rows) % 2 == 1).reshape(n, T)}
    isl = np.zeros((n, T), dtype=bool)
    isl[n - 1, T // 3:T // 3 + max(1, T // 4)] = True
    out["island"] = isl
    return out


@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("nc,ld", [(100, 128), (80, 128), (3, 4)])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 131])
def test_k_hold_slots_writes_the_held_rows_and_nothing_else(T, nc, ld, halves):
    from ns2vc_amd import _lib
    lib, be = _lib.load(), DeviceBackend()
    n = 3
    rng = np.random.default_rng(T * 1000 + nc + halves)
    x0_host = rng.standard_normal((halves * n * T, ld)).astype(np.float32)
    kn_host = rng.standard_normal((n * T, ld)).astype(np.float32)          # (the pad columns hold values too: they must not arrive)
    for name, mask in _masks(n, T).items():
        x0 = Guarded(be, halves * n * T, ld, "f32", data=x0_host, name="x0")
        kn = Guarded(be, n * T, ld, "f32", data=kn_host, name="known")
        m8 = np.ascontiguousarray(mask, dtype=np.uint8)
        _lib.check(lib.ns2vc_k_hold_slots(x0.ptr, kn.ptr, m8.ctypes.data, n, T, ld, nc, halves, None), "k_hold_slots")
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


def test_k_hold_slots_halves_1_leaves_a_second_half_alone_and_bad_arguments_are_errors():
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib, be = _lib.load(), DeviceBackend()
    n, T, ld, nc = 3, 65, 128, 100
    rng = np.random.default_rng(1)
    x0_host = rng.standard_normal((2 * n * T, ld)).astype(np.float32)      # two halves allocated, halves = 1 asked
    kn_host = rng.standard_normal((n * T, ld)).astype(np.float32)
    x0 = Guarded(be, 2 * n * T, ld, "f32", data=x0_host, name="x0")
    kn = Guarded(be, n * T, ld, "f32", data=kn_host, name="known")
    m8 = np.ones((n, T), dtype=np.uint8)
    _lib.check(lib.ns2vc_k_hold_slots(x0.ptr, kn.ptr, m8.ctypes.data, n, T, ld, nc, 1, None), "k_hold_slots")
    got = x0.read_bits().reshape(2, n * T, ld)
    assert np.array_equal(got[1], x0_host.view(np.uint32).reshape(2, n * T, ld)[1]) and x0.violations() == []
    assert np.array_equal(got[0][:, :nc], kn_host.view(np.uint32)[:, :nc]) and not got[0][:, nc:].any()
    buf = DevBuf(4 * 128 * 4)
    m = np.ones((1, 4), dtype=np.uint8)
    for a in ((0, 4, 128, 100, 1), (1, 0, 128, 100, 1), (1, 4, 126, 100, 1), (1, 4, 128, 129, 1), (1, 4, 128, 0, 1), (1, 4, 128, 100, 3)):
        assert lib.ns2vc_k_hold_slots(buf.ptr, buf.ptr, m.ctypes.data, *a, None) != 0
    assert lib.ns2vc_k_hold_slots(buf.ptr, None, m.ctypes.data, 1, 4, 128, 100, 1, None) != 0
    assert lib.ns2vc_k_hold_slots(buf.ptr, buf.ptr, None, 1, 4, 128, 100, 1, None) != 0


@pytest.mark.parametrize("C,ld,T", [(100, 128, 37), (3, 4, 64)])
def test_k_known_items_scatters_the_listed_slots_only(C, ld, T):
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    nslots = 4
    rng = np.random.default_rng(C + T)
    rows0 = np.full((nslots * T, ld), 0x5A5A5A5A, np.uint32)
    mask0 = np.full((nslots, T), 0x5A, np.uint8)
    for slots in ([2, -1, 0], [nslots, 1, 3]):
        n = len(slots)
        known = rng.standard_normal((n, C, T)).astype(np.float32)
        known[0, 0, 1] = -0.0
        mask = rng.random((n, T)) < 0.4
        mask[:, 0], mask[:, T - 1] = True, (np.arange(n) % 2 == 0)
        kd, rows, md = DevBuf.from_numpy(known), DevBuf.from_numpy(rows0), DevBuf.from_numpy(mask0)
        sl, m8 = np.array(slots, np.int32), np.ascontiguousarray(mask.astype(np.uint8) * 7)      # (any nonzero byte means held, written as 1)
        _lib.check(lib.ns2vc_k_known_items(kd.ptr, m8.ctypes.data, C, T, n, sl.ctypes.data, nslots, rows.ptr, md.ptr, ld, None), "k_known_items")
        got_r = rows.to_numpy((nslots, T, ld), dtype=np.uint32)
        got_m = md.to_numpy((nslots, T), dtype=np.uint8)
        want_r, want_m = rows0.reshape(nslots, T, ld).copy(), mask0.copy()
        for k, b in enumerate(slots):
            if 0 <= b < nslots:      # an entry of -1 or nslots is skipped
                want_r[b, :, :C] = known[k].T.view(np.uint32)
                want_r[b, :, C:] = 0
                want_m[b] = mask[k]
        assert np.array_equal(got_r, want_r) and np.array_equal(got_m, want_m), slots
        # the clear form: the listed slots' mask bytes become zero, nothing else changes
        clear = np.array([slots[1], slots[2]], np.int32)
        _lib.check(lib.ns2vc_k_known_items(None, None, C, T, 2, clear.ctypes.data, nslots, rows.ptr, md.ptr, ld, None), "k_known_items(clear)")
        for b in clear:
            if 0 <= b < nslots:
                want_m[b] = 0
        assert np.array_equal(rows.to_numpy((nslots, T, ld), dtype=np.uint32), want_r)
        assert np.array_equal(md.to_numpy((nslots, T), dtype=np.uint8), want_m)
    sl = np.array([0], np.int32)
    buf = DevBuf(4096)
    assert lib.ns2vc_k_known_items(buf.ptr, None, 3, 4, 1, sl.ctypes.data, 4, buf.ptr, buf.ptr, 4, None) != 0      # one of the pair
    assert lib.ns2vc_k_known_items(None, None, 5, 4, 1, sl.ctypes.data, 4, buf.ptr, buf.ptr, 4, None) != 0         # C > ld
    assert lib.ns2vc_k_known_items(None, None, 3, 4, 0, sl.ctypes.data, 4, buf.ptr, buf.ptr, 4, None) != 0


# ---- 2. the loop ------------------------------------------------------------------------------------------------------------------------------
U4, U6, U5 = (dict(solver="unipc", steps=n, order=2) for n in (4, 6, 5))
DDIM6 = dict(solver="ddim", steps=6, eta=1.0)
HEAD, ISLAND, TAIL = "head", "island", "tail"


def _tensor(tag, shape, scale=1.0):
    import torch
    from ns2vc_amd.weights import hash_normal
    return torch.from_numpy((scale * hash_normal(tag, shape)).astype(np.float32)).to(torch.device("cuda", 0))


def _mask(kind, L):
    m = np.zeros((L,), dtype=bool)
    if kind == HEAD:
        m[:8] = True
    elif kind == ISLAND:
        m[10:17] = True
        m[L - 1] = True
    elif kind == TAIL:
        m[L - 5:] = True
    return m


def _request(name, slot, schedule, hold=None, seed=0, scale=1.0):
    L, lp = LENS[slot], PLENS[slot]
    r = dict(slot=slot, content=_tensor(f"ks.{name}.c", (256, L)), prompt=_tensor(f"ks.{name}.p", (lp, 256)), noise=_tensor(f"ks.{name}.x", (100, L)),
             schedule=schedule, seed=seed, guidance_scale=scale)
    if hold is not None:
        r.update(known=_tensor(f"ks.{name}.k", (100, L), 0.6), known_mask=_mask(hold, L))
    return r


def _unheld(r):
    return {k: v for k, v in r.items() if k not in ("known", "known_mask")}


def _drive(den, reqs, graph=True, **forms):
    """reqs: {name: (request, start)} -> ({name: latent (100, T)}, captures after the first steps, captures at the end); test_continuous_gpu's
    driver: finished slots are taken as soon as the loop reaches their end, requests admitted at their start"""
    forms.setdefault("known_frames", True)
    loop = den.open_slots(*SHAPE, use_graph=graph, require_tail_free=False, **forms)
    out, held, caps = {}, {}, None
    try:
        pending = sorted(reqs.items(), key=lambda kv: kv[1][1])
        while pending or held:
            fin = loop.finished()
            if fin:
                lat = loop.take(fin)
                for k, b in enumerate(fin):
                    out[held.pop(b)] = lat[k]
            for name, (rq, start) in [p for p in pending if p[1][1] == loop.step]:
                loop.admit(**rq)
                held[rq["slot"]] = name
            pending = [p for p in pending if p[1][1] > loop.step]
            nexts = [it["start"] + it["steps"] for it in loop.items if it is not None] + [p[1][1] for p in pending]
            if not nexts:
                break
            loop.run(min(nexts) - loop.step)
            if caps is None:
                caps = den.engine.graph_captures()
        assert loop.idle() == [0, 1, 2]
    finally:
        loop.close()
    return {k: v.cpu().numpy() for k, v in out.items()}, caps, den.engine.graph_captures()


def _end(table):
    from ns2vc_amd import schedule as S
    if table.coef[-1, 5] == 0 and table.coef[-1, 6] == -1:
        return 1.0, 0.0
    sched = S.VPSchedule(S.linear_betas())
    t = float(table.timesteps[-1])
    return sched.alpha(t), sched.sigma(t)


def _closed_err(y, rq):
    """rel-L2 of the held frames of y (100, T) against alpha_end k + sigma_end eps of the request"""
    from ns2vc_amd import schedule as S
    sp = rq["schedule"]
    table = S.build_table(sp["solver"], sp["steps"], S.linear_betas(1000, np.float64) if sp["solver"] in S.DISCRETE_SOLVERS else None, sp.get("order", 2),
                          sp.get("eta", 0.0))
    a, s = _end(table)
    m = rq["known_mask"]
    L = m.shape[0]
    want = a * rq["known"].cpu().numpy().astype(np.float64) + s * rq["noise"].cpu().numpy().astype(np.float64)
    return rel_l2(y[:, :L][:, m], want[:, m])


def _requests():
    """slot 1 runs a held 4-step item, is taken, and gets a held 6-step item with another mask and other values at loop step 4; slots 0 and 2 run a
    held and a plain item across the admission"""
    return dict(A=_request("A", 0, U6, HEAD), B1=_request("B1", 1, U4, ISLAND), C=_request("C", 2, U5), B2=_request("B2", 1, U6, TAIL))


@pytest.fixture(scope="module")
def runs(denoisers):
    """the loops the tests below share, run once per precision"""
    out = {}
    for prec, den in denoisers.items():
        rq = _requests()
        full, caps0, caps1 = _drive(den, dict(A=(rq["A"], 0), B1=(rq["B1"], 0), C=(rq["C"], 0), B2=(rq["B2"], 4)))
        out[prec] = dict(rq=rq, full=full, caps=(caps0, caps1))
    return out


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_held_frames_meet_the_closed_form_and_free_frames_move(prec, runs, denoisers, diag):
    rq, full = runs[prec]["rq"], runs[prec]["full"]
    for k in ("A", "B1", "B2"):
        e = _closed_err(full[k], rq[k])
        diag(f"known frames in a slot loop ({prec}), item {k}: held frames vs the closed form {e:.2e} (bar {CLOSED_TOL:g})")
        assert e < CLOSED_TOL, (k, e)
        L = LENS[rq[k]["slot"]]
        assert not full[k][:, L:].any()
    plain, _, _ = _drive(denoisers[prec], dict(A=(_unheld(rq["A"]), 0)))
    free = ~rq["A"]["known_mask"]
    assert not np.array_equal(full["A"][:, :66][:, free], plain["A"][:, :66][:, free])      # generated next to the held frames


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_a_held_request_admitted_in_mid_loop(prec, runs, denoisers):
    den, rq, full = denoisers[prec], runs[prec]["rq"], runs[prec]["full"]
    caps0, caps1 = runs[prec]["caps"]
    without, _, _ = _drive(den, dict(A=(rq["A"], 0), B1=(rq["B1"], 0), C=(rq["C"], 0)))
    alone, _, _ = _drive(den, dict(B2=(rq["B2"], 0)))
    assert sorted(full) == ["A", "B1", "B2", "C"] and all(np.isfinite(v).all() for v in full.values())
    assert np.array_equal(full["B2"], alone["B2"]), "the held item depends on when it was admitted or on its neighbours"
    for k in ("A", "B1", "C"):
        assert np.array_equal(full[k], without[k]), f"item {k} depends on the admission beside it"
    assert caps1 == caps0, f"admissions with other masks and values recaptured the step graph ({caps0} -> {caps1})"


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_slots_filled_at_step_0_are_the_closed_loop_with_known_frames(prec, denoisers):
    import torch
    den = denoisers[prec]
    rq = _requests()
    names = ("A", "B1", "C")
    g, _, _ = _drive(den, {k: (rq[k], 0) for k in names}, True)
    e, _, _ = _drive(den, {k: (rq[k], 0) for k in names}, False)
    c, p, x = (torch.zeros((3, 256, 66), device="cuda"), torch.zeros((3, 5, 256), device="cuda"), torch.zeros((3, 100, 66), device="cuda"))
    kn, km = torch.zeros((3, 100, 66), device="cuda"), np.zeros((3, 66), dtype=bool)
    for k in names:
        b = rq[k]["slot"]
        c[b, :, :LENS[b]], p[b, :PLENS[b]], x[b, :, :LENS[b]] = rq[k]["content"], rq[k]["prompt"], rq[k]["noise"]
        if "known" in rq[k]:
            kn[b, :, :LENS[b]], km[b, :LENS[b]] = rq[k]["known"], rq[k]["known_mask"]
    closed = den.sample(c, p, None, x, schedules=[rq[k]["schedule"] for k in names], lengths=list(LENS), prompt_lengths=list(PLENS), known=kn,
                        known_mask=km).cpu().numpy()
    for k in names:
        assert np.array_equal(g[k], e[k]), k
        assert np.array_equal(g[k], closed[rq[k]["slot"]]), k


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_requests_without_known_frames_keep_plain_loop_bits(prec, denoisers):
    """in a known_frames=True loop, beside held neighbours and in a slot whose previous request held frames (the take cleared it)"""
    den = denoisers[prec]
    rq = _requests()
    b2 = _unheld(rq["B2"])
    plain, _, _ = _drive(den, dict(A=(_unheld(rq["A"]), 0), C=(rq["C"], 0), B2=(b2, 0)), known_frames=False)
    got, _, _ = _drive(den, dict(A=(_unheld(rq["A"]), 0), B1=(rq["B1"], 0), C=(rq["C"], 0), B2=(b2, 4)))
    for k in ("A", "C", "B2"):      # (B2: admitted at step 4 into the slot B1 held frames in; a plain loop gives it the bits of step 0)
        assert np.array_equal(got[k], plain[k]), k


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_guided_loop_holds_both_halves(prec, denoisers, diag):
    den = denoisers[prec]
    rq = dict(A=_request("gA", 0, U6, HEAD, scale=2.5), B=_request("gB", 1, U4, ISLAND, scale=1.0), C=_request("gC", 2, U5, scale=0.5),
              B2=_request("gB2", 1, U6, TAIL, scale=3.0))
    forms = dict(unconditional_prompt=_tensor("ks.u", (1, 2, 256)))
    full, caps0, caps1 = _drive(den, dict(A=(rq["A"], 0), B=(rq["B"], 0), C=(rq["C"], 0), B2=(rq["B2"], 4)), **forms)
    alone, _, _ = _drive(den, dict(B2=(rq["B2"], 0)), **forms)
    assert np.array_equal(full["B2"], alone["B2"]) and caps0 == caps1
    for k in ("A", "B", "B2"):
        e = _closed_err(full[k], rq[k])
        diag(f"known frames in a guided slot loop ({prec}), item {k} scale {rq[k]['guidance_scale']}: closed form {e:.2e}")
        assert e < CLOSED_TOL, (k, e)


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_a_ddim_request_ends_on_the_known_latent(prec, denoisers, diag):
    den = denoisers[prec]
    rq = dict(A=_request("dA", 0, U6, seed=11), D=_request("dD", 1, DDIM6, ISLAND, seed=14))
    full, _, _ = _drive(den, dict(A=(rq["A"], 0), D=(rq["D"], 2)), stochastic=True)
    m = rq["D"]["known_mask"]
    k = rq["D"]["known"].cpu().numpy()
    e = rel_l2(full["D"][:, :65][:, m], k[:, m])
    diag(f"known frames in a slot loop ({prec}), ddim eta 1: held frames vs k {e:.2e}")
    assert e < CLOSED_TOL


def test_fp32_loop_against_the_host_statement(denoisers, diag):
    """one item per slot, two of them held, one admitted in mid-loop: run_slots_numpy with the engine's own denoise as x0_fn"""
    import torch
    from ns2vc_amd import schedule as S
    den = denoisers["fp32"]
    rq = dict(A=_request("hA", 0, U6, HEAD), B=_request("hB", 1, U5, TAIL), C=_request("hC", 2, U4))
    starts = dict(A=0, B=2, C=0)
    got, _, _ = _drive(den, {k: (rq[k], starts[k]) for k in rq})
    dev = rq["A"]["content"].device
    c, p = torch.zeros((3, 256, 66), device=dev), torch.zeros((3, 5, 256), device=dev)
    timeline = [None] * 3
    for k, r in rq.items():
        b, L = r["slot"], LENS[r["slot"]]
        c[b, :, :L], p[b, :PLENS[b]] = r["content"], r["prompt"]
        table = S.build_table("unipc", r["schedule"]["steps"], order=2)
        x = np.zeros((100, 66), np.float32)
        x[:, :L] = r["noise"].cpu().numpy()
        hold = None
        if "known" in r:
            kn, km = np.zeros((100, 66), np.float32), np.zeros((66,), dtype=bool)
            kn[:, :L], km[:L] = r["known"].cpu().numpy(), r["known_mask"]
            hold = (kn, km)
            x = S.known_start(x[None], kn[None], km[None], table.coef[0])[0]
        timeline[b] = [(table, starts[k], x, None, hold)]

    def x0_fn(xx, tt):
        y = den.denoise(torch.from_numpy(np.ascontiguousarray(xx)).to(dev), torch.from_numpy(np.ascontiguousarray(tt)).to(dev), c, p, lengths=list(LENS),
                        prompt_lengths=list(PLENS)).cpu().numpy()
        for b in range(3):
            y[b, :, LENS[b]:] = 0
        return y

    ref = S.run_slots_numpy(timeline, x0_fn, (3, 100, 66))
    for k, r in rq.items():
        b, L = r["slot"], LENS[r["slot"]]
        y, want = got[k][None, :, :L], ref[b][0][None, :, :L]
        e, loc = rel_l2(y, want), local_errors(y, want)
        diag(f"known frames in a slot loop (fp32), item {k} vs run_slots_numpy: {e:.2e}  {fmt_local(loc)}")
        assert e < FP32_TOL and loc["frame"] < FP32_LOCAL_TOL and loc["chan"] < FP32_LOCAL_TOL, k


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_graph_equals_eager_and_the_form_recaptures_once_each_way(prec, runs, denoisers):
    den, rq, full = denoisers[prec], runs[prec]["rq"], runs[prec]["full"]
    reqs = dict(A=(rq["A"], 0), B1=(rq["B1"], 0), C=(rq["C"], 0), B2=(rq["B2"], 4))
    eager, _, _ = _drive(den, reqs, False)
    for k in full:
        assert np.array_equal(full[k], eager[k]), k
    plain = dict(A=(_unheld(rq["A"]), 0))
    _drive(den, plain, known_frames=False)
    n0 = den.engine.graph_captures()
    _drive(den, plain, known_frames=False)
    assert den.engine.graph_captures() == n0                  # the form off twice: a replay
    _drive(den, reqs)
    assert den.engine.graph_captures() == n0 + 1              # on: the step gains a launch
    again, _, _ = _drive(den, reqs)
    assert den.engine.graph_captures() == n0 + 1              # on again, other loops in between or not: a replay
    _drive(den, plain, known_frames=False)
    assert den.engine.graph_captures() == n0 + 2              # and off
    for k in full:
        assert np.array_equal(full[k], again[k]), k


def test_engine_refusals_and_the_engine_serves_on(weights):
    import torch
    from ns2vc_amd import schedule as S
    from ns2vc_amd._lib import Ns2vcError
    from ns2vc_amd.engine import Engine
    e = Engine(precision="fp32")
    try:
        e.load_state_dict(weights)
        e.prepare(*SHAPE)
        e.set_lengths([66, 40, 66])
        e.set_prompt_lengths([5, 5, 5])
        k, m = _tensor("ks.rf.k", (1, 100, 66)), np.zeros((1, 66), dtype=bool)
        m[0, :8] = True
        x = _tensor("ks.rf.x", (1, 100, 66))
        with pytest.raises(Ns2vcError, match="no slot loop"):
            e.set_known_items([0], k, m)
        e.open_slots()
        with pytest.raises(Ns2vcError, match="opened without known frames"):
            e.set_known_items([0], k, m)
        e.set_x0_correction("clamp")
        with pytest.raises(ValueError, match="known_frames"):
            e.open_slots(known_frames=True)              # (Engine.open_slots itself)
        with pytest.raises(Ns2vcError, match="rescale the known frames"):
            _check(e.lib.ns2vc_sampler_open_known(e.h, 0, 0, None))      # ... and the library
        e.set_x0_correction(None)
        e.open_slots(known_frames=True)
        late = np.zeros((1, 66), dtype=bool)
        late[0, 40] = True
        with pytest.raises(Ns2vcError, match="at or past its length 40"):
            e.set_known_items([1], k, late)
        with pytest.raises(Ns2vcError, match="outside"):
            e.set_known_items([3], k, m)
        with pytest.raises(Ns2vcError, match="rescale"):
            e.set_x0_correction("clamp")
        e.write_sampler_rows(0, S.build_table("unipc", 4).coef)
        late[0, 40], late[0, 39] = False, True
        e.set_known_items([1], k, late)
        e.set_lengths([66, 39, 66])                      # lengths set after the frames: the admission checks its mirror
        with pytest.raises(Ns2vcError, match="known frame 39 of slot 1"):
            e.admit([1], x, [[0, 4, 0, 0]])
        e.set_known_items([1], None, None)
        e.admit([1], x, [[0, 4, 0, 0]])
        with pytest.raises(Ns2vcError, match="slot 1 is busy"):
            e.set_known_items([1], k, m)
        with pytest.raises(Ns2vcError, match="slot 1 is busy"):
            e.set_known_items([1], None, None)
        e.sample_steps(4)
        out = torch.empty_like(x)
        e.take([1], out)
        e.sample_end(torch.empty((3, 100, 66), device="cuda"))
        # afterwards: a closed loop and a plain slot loop
        e.load_sampler("unipc", 4)
        y = torch.zeros((3, 100, 66), device="cuda")
        y[1, :, :39] = x[0, :, :39]
        e.sample(y)
        torch.cuda.synchronize()
        assert np.array_equal(y.cpu().numpy()[1], out.cpu().numpy()[0]) and torch.isfinite(y).all()
        e.open_slots()
        assert e.slot_step() == 0
    finally:
        e.close()


def _check(rc):
    from ns2vc_amd._lib import check
    check(rc, "call")


# ---- 3. ContinuousConverter(overlap_frames=) ----------------------------------------------------------------------------------------------------
class _Pre:
    """a front end of elementwise operations only, so that two calls on the same frames give the same bits: content = tanh(c), prompt = the clip
    transposed and repeated to 256 columns"""
    def __init__(self):
        import torch
        self.p = torch.zeros(1, device="cuda")
        self.calls = []

    def parameters(self):
        return iter([self.p])

    def infer(self, c, refer, lens, plens, exact_lengths=False, exact_prompt_lengths=False):
        import torch
        self.calls.append([int(v) for v in lens])
        return torch.tanh(c), (0.5 * refer.transpose(1, 2)).repeat(1, 1, 3)[..., :256].contiguous(), None


def test_continuous_converter_chains_long_segments(denoisers, diag):
    import torch
    from ns2vc_amd import schedule as S
    from ns2vc_amd.noise import derive_seed
    from ns2vc_amd.service import ContinuousConverter, Segment
    from ns2vc_amd.weights import hash_normal
    den, V, seed = denoisers["fp32"], 8, 1234
    shapes = [(150, 5), (40, 3), (67, 4)]
    segs = [Segment(torch.from_numpy(hash_normal(f"kc.c{i}", (256, T))), torch.from_numpy(hash_normal(f"kc.r{i}", (100, L))), tag=i)
            for i, (T, L) in enumerate(shapes)]
    pre = _Pre()
    conv = ContinuousConverter(pre, den, slots=3, max_frames=66, max_prompt=5, solver="unipc", steps=4, seed=seed, overlap_frames=V)
    out = [t.cpu().numpy() for t in conv.convert(segs)]
    chunks = [S.plan_chunks(T, 66, V) for T, _ in shapes]
    assert [len(c) for c in chunks] == [3, 1, 2] and sorted(pre.calls) == [[40], [67], [150]]
    slot_of = {req: b for _, _, admit in conv.last_plan for b, req in admit}
    dev = torch.device("cuda", 0)
    dummy = dict(solver="unipc", steps=5, order=2)      # (the other items of a closed batch: per-item schedules, as the slot loop runs them)
    own = dict(solver="unipc", steps=4, order=2)
    cover = [np.zeros(T, int) for T, _ in shapes]
    for i, (T, lp) in enumerate(shapes):
        content, prompt, _ = pre.infer(segs[i].content.to(dev)[None], segs[i].refer.to(dev)[None], [T], [lp], True, True)
        x_full = torch.randn((100, T), generator=torch.Generator().manual_seed(seed + i)).to(dev)
        want = np.zeros((100, T), np.float32)
        prev = None
        for j, (start, stop) in enumerate(chunks[i]):      # the hand-written chain, each chunk in the slot it ran in
            b, L = slot_of[(i, j)], stop - start
            c, p, x = torch.zeros((3, 256, 66), device=dev), torch.zeros((3, 5, 256), device=dev), torch.zeros((3, 100, 66), device=dev)
            c[b, :, :L], p[b, :lp], x[b, :, :L] = content[0, :, start:stop], prompt[0, :lp], x_full[:, start:stop]
            lens, plens = [66, 66, 66], [5, 5, 5]
            lens[b], plens[b] = L, lp
            kw = {}
            if j > 0:
                kn, km = torch.zeros((3, 100, 66), device=dev), np.zeros((3, 66), dtype=bool)
                kn[b, :, :V], km[b, :V] = prev, True
                kw = dict(known=kn, known_mask=km)
            y = den.sample(c, p, None, x, schedules=[own if s == b else dummy for s in range(3)], lengths=lens, prompt_lengths=plens, **kw)
            keep = V if j > 0 else 0
            want[:, start + keep:stop] = y[b, :, keep:L].cpu().numpy()
            cover[i][start + keep:stop] += 1
            prev = y[b, :, L - V:L].clone()
        assert (cover[i] == 1).all(), "every output frame is written exactly once"
        assert out[i].shape == (100, T) and np.isfinite(out[i]).all()
        if len(chunks[i]) > 1:
            assert np.array_equal(out[i], want), f"segment {i}: the chained result differs from the hand-written chain"
    # the short segment equals itself alone: the same slot of the same loop shape, every other slot idle
    b = slot_of[(1, 0)]
    T, lp = shapes[1]
    content, prompt, _ = pre.infer(segs[1].content.to(dev)[None], segs[1].refer.to(dev)[None], [T], [lp], True, True)
    loop = den.open_slots(3, 66, 5)
    try:
        loop.admit(b, content[0], prompt[0], torch.randn((100, T), generator=torch.Generator().manual_seed(seed + 1)).to(dev), schedule=own,
                   seed=int(derive_seed(seed, 1)))
        loop.run()
        alone = loop.take([b])[0, :, :T].cpu().numpy()
    finally:
        loop.close()
    assert np.array_equal(out[1], alone)
