"""The top-level ``sampler`` package on the MI355X: the flat solver step ``ns2vc_k_solver_step_flat`` against
``ns2vc_k_solver_update`` and the host statement, the ``device`` path against the reference's own loops (g14 of golden_v5.npz), and the
hand-off of a recognised drop-in module to the captured loop (``captured``) against the direct ``Denoiser.sample`` and the oracle."""
import os

import numpy as np
import pytest

from util import TOL_SOLVER, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "golden_v5.npz")
SYN_TOL = 5e-6              # tests/test_solvers_cpu.py: the bar for agreement with the reference's loops on the closed-form denoiser
FP32_SAMPLED_TOL = 5e-5     # tests/test_engine_gpu.py: sampled latents of the fp32 engine
FP16_TOL = 1e-3             # the parity bar
PLANES = ("xe", "xbar", "d1", "mprev", "mprev2")
B, T, LP = 2, 66, 5         # the smallest shape the loop tests use (below 66 frames the levels change plan)


# ---- the kernel -----------------------------------------------------------------------------------------------------------------
def _table():
    from ns2vc_amd import schedule as S
    table = S.build_table("unipc", 10, order=3, skip_type="logSNR")
    assert table.coef[4, 10] != 0 and table.coef[4, 11] != 0      # row 4: an order-3 row, d2c and pe both nonzero
    return table


def _state(n, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal(n).astype(np.float32) for k in ("out",) + PLANES}


class _Plain:
    """a device buffer with four sentinel floats either side of the tensor, for a tensor too large for guard.Guarded's row-tile bands"""

    def __init__(self, data, sent):
        from ns2vc_amd.engine import DevBuf
        self.n, self.sent = len(data), sent
        self.buf = DevBuf.from_numpy(np.concatenate([np.full(4, sent, np.float32), data, np.full(4, sent, np.float32)]))
        self.ptr = self.buf.ptr + 16

    def violations(self):
        v = self.buf.to_numpy((self.n + 8,))
        return [] if np.array_equal(np.concatenate([v[:4], v[-4:]]), np.full(8, self.sent, np.float32)) else ["a sentinel changed"]

    def read(self):
        return self.buf.to_numpy((self.n + 8,))[None, 4:-4]


class _Flat:
    """one launch of the flat step on guarded buffers: plane k starts ``offs[k]`` floats past a 16-byte boundary"""

    def __init__(self, st, offs=None, m_out=False, guarded=True):
        from guard import DeviceBackend, Guarded
        from ns2vc_amd import _lib
        from ns2vc_amd.engine import DevBuf
        self.lib, self.check = _lib.load(), _lib.check
        self.n = len(st["out"])
        self.offs = dict(offs or {})
        names = ("out",) + PLANES + (("m_out",) if m_out else ())
        be = DeviceBackend()
        self.sent = np.float32(-7.25)
        self.g = {}
        for k in names:
            o = self.offs.get(k, 0)
            v = st[k] if k in st else np.full(self.n, np.nan, np.float32)
            data = np.concatenate([np.full(o, self.sent, np.float32), v])
            self.g[k] = Guarded(be, 1, o + self.n, "f32", data=data, name=k) if guarded else _Plain(data, self.sent)
        self.table = _table()
        self.coef = DevBuf.from_numpy(np.ascontiguousarray(self.table.coef, np.float32))

    def ptr(self, k):
        return self.g[k].ptr + 4 * self.offs.get(k, 0)

    def run(self, kind, hist2, row=4, out="out", form=False):
        rc = self.lib.ns2vc_k_solver_step_flat(self.coef.ptr, self.table.steps, row, kind, self.ptr(out), self.ptr("xe"), self.ptr("xbar"), self.ptr("d1"),
                                               self.ptr("mprev"), self.ptr("mprev2") if hist2 else None, self.ptr("m_out") if form else None, self.n, None)
        self.check(rc, "ns2vc_k_solver_step_flat")
        self.lib.ns2vc_dev_sync()
        return self

    def read(self):
        """every plane's values; the guard bands and the floats in front of an offset plane must hold what was uploaded"""
        got = {}
        for k, g in self.g.items():
            assert g.violations() == [], k
            v = g.read()[0]
            o = self.offs.get(k, 0)
            assert np.array_equal(v[:o], np.full(o, self.sent, np.float32)), f"{k}: the {o} float(s) in front of the plane changed"
            got[k] = v[o:].copy()
        return got


def _update(st, hist2, row=4):
    """ns2vc_k_solver_update in fp32 on the same values (ld = 4; n padded to a multiple of 4, the padding cut off again)"""
    from ns2vc_amd import _lib
    from ns2vc_amd.engine import DevBuf
    lib = _lib.load()
    n = len(st["out"])
    npad = (n + 3) // 4 * 4
    pad = lambda v: np.concatenate([v, np.ones(npad - n, np.float32)])      # noqa: E731
    b = {k: DevBuf.from_numpy(pad(st[k])) for k in ("out",) + PLANES}
    coef = DevBuf.from_numpy(np.ascontiguousarray(_table().coef, np.float32))
    step = DevBuf.from_numpy(np.array([row, 0, 0, 0], np.int32))
    op = DevBuf(npad * 4)
    _lib.check(lib.ns2vc_k_solver_update(coef.ptr, step.ptr, b["out"].ptr, b["xe"].ptr, op.ptr, 0, b["xbar"].ptr, b["d1"].ptr, b["mprev"].ptr,
                                         b["mprev2"].ptr if hist2 else None, npad, 4, None), "k_solver_update")
    lib.ns2vc_dev_sync()
    return {k: b[k].to_numpy((npad,))[:n] for k in PLANES}


@pytest.mark.parametrize("hist2", [False, True], ids=["hist1", "hist2"])
@pytest.mark.parametrize("n", [4, 1024, 7400])
def test_kind0_has_the_bits_of_k_solver_update(n, hist2):
    st = _state(n, n)
    got, want = _Flat(st).run(0, hist2).read(), _update(st, hist2)
    for k in PLANES:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["out"], st["out"])
    assert np.array_equal(got["mprev2"], st["mprev"] if hist2 else st["mprev2"])


OFFSETS = {"spread": dict(out=0, xe=1, xbar=2, d1=3, mprev=0, mprev2=1, m_out=2), "rotated": dict(out=3, xe=2, xbar=1, d1=0, mprev=3, mprev2=2, m_out=1),
           "common1": {k: 1 for k in ("out", "m_out") + PLANES}, "common3": {k: 3 for k in ("out", "m_out") + PLANES}}


@pytest.mark.parametrize("offs", sorted(OFFSETS))
@pytest.mark.parametrize("n", [1, 3, 5, 1027])
def test_any_alignment_gives_the_aligned_bits(n, offs):
    """planes 0 .. 3 floats off a 16-byte boundary, each on a phase of its own (scalar throughout) or all on one (scalar head, float4 body,
    scalar tail): element for element the aligned run's bits; nothing outside the n elements of any plane is written"""
    st = _state(n, 100 + n)
    for kind, hist2 in ((0, True), (0, False), (2, True)):
        want = _Flat(st).run(kind, hist2).read()
        got = _Flat(st, OFFSETS[offs]).run(kind, hist2).read()
        for k in ("out",) + PLANES:
            assert np.array_equal(got[k], want[k]), (kind, hist2, k)
    want = _Flat(st, m_out=True).run(1, False, form=True).read()
    got = _Flat(st, OFFSETS[offs], m_out=True).run(1, False, form=True).read()
    for k in ("out", "m_out") + PLANES:
        assert np.array_equal(got[k], want[k]), ("form", k)


def test_past_one_trip_of_the_grid():
    """n = 5 past what one trip of the capped grid covers: a second trip of the float4 loop and a tail; the bits of ns2vc_k_solver_update"""
    from ns2vc_amd import _lib
    n = _lib.FLAT_TRIP + 5
    st = _state(n, 7)
    got, want = _Flat(st, guarded=False).run(0, True).read(), _update(st, True)
    for k in PLANES:
        assert np.array_equal(got[k], want[k]), k
    shifted = _Flat(st, OFFSETS["common1"], guarded=False).run(0, True).read()
    for k in PLANES:
        assert np.array_equal(shifted[k], want[k]), k


def _host_m(kind, c, out, xe):
    """m of a model output of ``kind`` in float32 (the flat kernel's header comment)"""
    f = np.float32
    alpha, sigma = f(c[1]), f(c[2])
    if kind == 4:
        return out
    eps = out if kind == 1 else (alpha * out + sigma * xe if kind == 2 else -sigma * out)
    return (xe - sigma * eps) / alpha


@pytest.mark.parametrize("hist2", [False, True], ids=["hist1", "hist2"])
@pytest.mark.parametrize("kind", [1, 2, 3, 4])
def test_kinds_against_the_host_statement(kind, hist2, diag):
    """noise, v, score and data against ``schedule.solver_update`` (float32) fed with m formed per kind, at the tolerance of the existing comparison
    of ns2vc_k_solver_update with its host twin (tests/test_solvers_gpu.py: TOL_SOLVER)"""
    from ns2vc_amd import schedule as S
    n = 1027
    st = _state(n, 40 + kind)
    got = _Flat(st).run(kind, hist2).read()
    c = _table().coef[4]
    new = S.solver_update(c, hist2, _host_m(kind, c, st["out"], st["xe"]), st["xe"], st["xbar"], st["d1"], st["mprev"], st["mprev2"])
    errs = {k: rel_l2(got[k], v) for k, v in zip(PLANES[:4], new[:4])}
    diag(f"k_solver_step_flat kind {kind} hist2={hist2}: " + " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v < TOL_SOLVER, k
    assert np.array_equal(got["mprev2"], st["mprev"] if hist2 else st["mprev2"])


@pytest.mark.parametrize("hist2", [False, True], ids=["hist1", "hist2"])
@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
def test_form_writes_m_alone_and_form_then_data_is_the_step(kind, hist2):
    st = _state(1027, 60 + kind)
    f = _Flat(st, m_out=True).run(kind, hist2, form=True)
    formed = f.read()
    for k in ("out",) + PLANES:
        assert np.array_equal(formed[k], st[k]), k      # FORM leaves every state plane unchanged
    assert np.isfinite(formed["m_out"]).all()
    two = f.run(4, hist2, out="m_out").read()           # ... and kind 4 on that m
    one = _Flat(st).run(kind, hist2).read()
    for k in PLANES:
        assert np.array_equal(two[k], one[k]), k
    assert np.array_equal(one["mprev"], formed["m_out"])


def test_refusals():
    f = _Flat(_state(8, 1), m_out=True)
    p = {k: f.ptr(k) for k in f.g}

    def step(coef=f.coef.ptr, rows=f.table.steps, row=0, kind=0, out=p["out"], xe=p["xe"], xbar=p["xbar"], d1=p["d1"], mprev=p["mprev"], mprev2=None,
             m_out=None, n=8):
        return f.lib.ns2vc_k_solver_step_flat(coef, rows, row, kind, out, xe, xbar, d1, mprev, mprev2, m_out, n, None)

    for kw in (dict(coef=None), dict(out=None), dict(xe=None), dict(xbar=None), dict(d1=None), dict(mprev=None), dict(n=0), dict(kind=5), dict(kind=-1),
               dict(row=f.table.steps), dict(row=-1), dict(rows=0), dict(d1=p["d1"] + 2), dict(m_out=p["m_out"] + 1)):
        assert step(**kw) != 0 and f.lib.ns2vc_last_error(), kw
    assert step() == 0 and step(mprev2=p["mprev2"]) == 0 and step(m_out=p["m_out"]) == 0
    f.lib.ns2vc_dev_sync()
    f.read()


# ---- the device path --------------------------------------------------------------------------------------------------------------
DEVICE_CASES = [("unipc", 10, 2, "time_uniform", True, {}), ("unipc", 10, 3, "logSNR", True, {}), ("dpmsolver++", 10, 2, "time_uniform", True, {}),
                ("dpmsolver++", 10, 3, "logSNR", True, {}), ("unipc", 10, 3, "time_uniform", True, {"denoise_to_zero": True}),
                ("dpmsolver++", 10, 3, "logSNR", True, {"t_start": 0.9, "t_end": 0.005})]


def _case_tag(solver, steps, order, skip, lof, extra):
    t = f"{'unipc' if solver == 'unipc' else 'dpmpp'}{order}_{skip}_{steps}" + ("" if lof else "_nolof")
    for k in sorted(extra):
        v = extra[k]
        t += f"_{k}" if v is True else f"_{k}{v}".replace(".", "p")
    return t


def _synthetic_x0(x, t):
    """tests/util.synthetic_x0 in torch, on the tensors' device"""
    import torch
    return 0.9 * torch.tanh(x) + 0.05 * torch.cos(0.01 * t.to(x.dtype).reshape(-1, 1, 1))


def _solver(case, model, model_type="x_start", **ctor):
    import torch
    from ns2vc_amd import schedule as S
    from sampler import dpm_solver, uni_pc
    solver, steps, order, skip, lof, extra = case
    extra = dict(extra)
    module = uni_pc if solver == "unipc" else dpm_solver
    ns = module.NoiseScheduleVP(schedule="discrete", betas=torch.from_numpy(S.linear_betas()))
    fn = module.model_wrapper(model, ns, model_type=model_type)
    s = module.UniPC(fn, ns, variant=extra.pop("variant", "bh2"), **ctor) if solver == "unipc" else module.DPM_Solver(fn, ns, **ctor)
    return s, dict(steps=steps, order=order, skip_type=skip, method="multistep", lower_order_final=lof, **extra)


@pytest.mark.parametrize("case", DEVICE_CASES, ids=[_case_tag(*c) for c in DEVICE_CASES])
def test_device_path_against_reference_loops(case, diag):
    import torch
    gold = np.load(GOLD)
    s, kw = _solver(case, _synthetic_x0)
    y = s.sample(torch.from_numpy(gold["g14.x_T"]).cuda(), **kw)
    assert s.last_path == "device" and y.is_cuda and y.dtype == torch.float32
    e = rel_l2(y.cpu().numpy(), gold[f"g14.{_case_tag(*case)}.y"])
    diag(f"sampler device path {_case_tag(*case)}: {e:.3e} (bar {SYN_TOL:g})")
    assert e <= SYN_TOL, e


def test_device_loop_waits_for_nothing(monkeypatch):
    """a second call of the same schedule (table and times already on the device): no host wait and no host read of device data from the
    package -- torch's sync debug mode where this torch honours it, and counting patches of the calls that wait either way"""
    import torch
    gold = np.load(GOLD)
    x = torch.from_numpy(gold["g14.x_T"]).cuda()
    s, kw = _solver(DEVICE_CASES[1], _synthetic_x0)
    want = s.sample(x, **kw)
    torch.cuda.synchronize()
    counts = {}

    def counting(owner, name):
        real = getattr(owner, name)

        def patched(*a, **k):
            counts[name] = counts.get(name, 0) + 1
            return real(*a, **k)
        monkeypatch.setattr(owner, name, patched)

    for owner, name in ((torch.Tensor, "item"), (torch.Tensor, "cpu"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy"), (torch.cuda, "synchronize")):
        counting(owner, name)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.ones(1, device="cuda").nonzero()
        except RuntimeError:
            honoured = True
        y = s.sample(x, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert counts == {}, counts
    print("sync debug mode honoured:", honoured)
    assert s.last_path == "device" and torch.equal(y, want)


@pytest.mark.parametrize("correction", ["dynamic_thresholding", "callable"])
def test_device_corrections_against_the_host_path(correction, diag):
    """FORM, the correction in torch, the update with kind data -- against the same call on CPU tensors, at the fp32 sampled-latent gate"""
    import torch
    gold = np.load(GOLD)
    x = 3.0 * torch.from_numpy(gold["g14.x_T"])
    if correction == "callable":
        ctor = dict(correcting_x0_fn=lambda x0, t: x0.clamp(-0.5, 0.5))
    else:
        ctor = dict(correcting_x0_fn="dynamic_thresholding", thresholding_max_val=0.5, dynamic_thresholding_ratio=0.9)
    got = {}
    for dev in ("cuda", "cpu"):
        s, kw = _solver(DEVICE_CASES[1], _synthetic_x0, **ctor)
        got[dev] = s.sample(x.to(dev), **kw).cpu().numpy()
        assert s.last_path == ("device" if dev == "cuda" else "host")
    s, kw = _solver(DEVICE_CASES[1], _synthetic_x0)
    plain = s.sample(x.cuda(), **kw).cpu().numpy()
    e = rel_l2(got["cuda"], got["cpu"])
    diag(f"sampler device path, {correction}: {e:.3e} vs host (bar {FP32_SAMPLED_TOL:g}); uncorrected differs by {rel_l2(plain, got['cpu']):.2e}")
    assert e <= FP32_SAMPLED_TOL and rel_l2(plain, got["cpu"]) > 1e-2


def test_device_path_dtype_and_views():
    """x in float16 and as a non-contiguous view: float32 arithmetic on a contiguous state, the result in x.dtype"""
    import torch
    gold = np.load(GOLD)
    x = torch.from_numpy(gold["g14.x_T"]).cuda()
    s, kw = _solver(DEVICE_CASES[0], _synthetic_x0)
    want = s.sample(x, **kw)
    wide = torch.zeros((2, 4, 16), device="cuda")
    wide[:, :, 3:11] = x
    assert torch.equal(s.sample(wide[:, :, 3:11], **kw), want)
    y16 = s.sample(x.half(), **kw)
    assert y16.dtype == torch.float16 and rel_l2(y16.float().cpu().numpy(), want.cpu().numpy()) < 5e-3


# ---- the hand-off -----------------------------------------------------------------------------------------------------------------
UNET_KW = dict(in_channels=356, out_channels=100, block_out_channels=(128, 256, 384, 512), norm_num_groups=8, cross_attention_dim=256,
               attention_head_dim=8, addition_embed_type="text", resnet_time_scale_shift="scale_shift")
SOLVERS = {"unipc": ("unipc", 6, 2, "time_uniform", True, {}), "dpmsolver++": ("dpmsolver++", 6, 2, "time_uniform", True, {})}


def _weights(seed):
    import torch
    from ns2vc_amd.weights import procedural_state_dict
    return {k: torch.from_numpy(v) for k, v in procedural_state_dict(seed=seed).items()}


def _module(prec, seed=0):
    from unet1d import UNet1DConditionModel
    m = UNet1DConditionModel(engine_precision=prec, **UNET_KW)
    m.load_state_dict(_weights(seed), strict=True)
    return m.cuda().eval()


@pytest.fixture(scope="module")
def modules():
    return {prec: _module(prec) for prec in ("fp32", "fp16")}


@pytest.fixture(scope="module")
def inputs():
    import torch
    from ns2vc_amd.weights import hash_normal
    x = torch.from_numpy(hash_normal("pkg.x", (B, 100, T))).cuda()
    content = torch.from_numpy(hash_normal("pkg.content", (B, 256, T))).cuda()
    prompt = torch.from_numpy(hash_normal("pkg.prompt", (B, LP, 256))).cuda()
    plens = torch.tensor([LP, 3]).cuda()
    return x, content, prompt, plens


class StandIn:
    """the reference's call pattern around the UNet (model.py forward / sample_fun / my_wrapper): the cat with the content, the prompt mask,
    ``.sample``, and a side effect per call -- a counter where the reference moves its progress bar"""

    def __init__(self, unet):
        self.unet, self.count = unet, 0

    def sample_fun(self, x, t, data=None):
        import torch
        content, prompt, plens = data
        mask = (torch.arange(prompt.shape[1], device=x.device)[None, :] < plens[:, None]).to(torch.bool)
        return self.unet(torch.cat([x, content], dim=1), t, prompt, encoder_attention_mask=mask).sample

    def wrapped(self, x, t, **kwargs):
        ret = self.sample_fun(x, t, **kwargs)
        self.count += 1
        return ret


def _mask(inputs):
    import torch
    return torch.arange(LP, device="cuda")[None, :] < inputs[3][:, None]


def _run(model, inputs, solver="unipc", model_type="x_start"):
    import torch
    s, kw = _solver(SOLVERS[solver], model, model_type)
    s.model_fn.model_kwargs = {"data": inputs[1:]}
    with torch.no_grad():
        return s, s.sample(inputs[0], **kw)


def _direct(module, inputs, solver):
    from ns2vc_amd import schedule as S
    from ns2vc_amd.pipeline import Denoiser
    den = Denoiser(module.state_dict(), module.cfg, precision=module._precision, betas=S.linear_betas())
    return den.sample(inputs[1], inputs[2], _mask(inputs), inputs[0], solver=solver, steps=6, order=2)


@pytest.mark.parametrize("solver", sorted(SOLVERS))
@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_recognised_module_runs_the_captured_loop(prec, solver, modules, inputs, monkeypatch, diag):
    import sampler
    import torch
    m = modules[prec]
    monkeypatch.setattr(sampler, "capture", True)
    st, calls = StandIn(m), m.engine_calls
    s, y = _run(st.wrapped, inputs, solver)
    assert s.last_path == "captured"
    assert m.engine_calls == calls + 1 and st.count == 1      # the probe alone
    want = _direct(m, inputs, solver)
    assert y.dtype == torch.float32 and np.array_equal(y.cpu().numpy(), want.cpu().numpy())
    monkeypatch.setattr(sampler, "capture", False)
    st, calls = StandIn(m), m.engine_calls
    s, per_step = _run(st.wrapped, inputs, solver)
    assert s.last_path == "device"
    assert m.engine_calls == calls + 6 and st.count == 6
    e = rel_l2(per_step.cpu().numpy(), y.cpu().numpy())
    tol = FP32_SAMPLED_TOL if prec == "fp32" else FP16_TOL
    diag(f"sampler package {solver} {prec}: a call per step vs the captured loop {e:.3e} (bar {tol:g})")
    assert e < tol


def test_captured_fp32_against_the_oracle(modules, inputs, monkeypatch, diag):
    import sampler
    import torch
    from ns2vc_amd.spec import UNetConfig
    from oracle import sampler_ref, unet_ref
    monkeypatch.setattr(sampler, "capture", True)
    s, y = _run(StandIn(modules["fp32"]).wrapped, inputs, "unipc")
    assert s.last_path == "captured"
    P = {k: v for k, v in _weights(0).items()}
    x, c, p = (v.cpu() for v in inputs[:3])
    mask = _mask(inputs).cpu()
    ref = sampler_ref.unipc_bh2(lambda xx, tt: unet_ref.denoiser(P, UNetConfig(), xx, c, p, mask, tt), sampler_ref.linear_betas(), x, 6, order=2).numpy()
    e = rel_l2(y.cpu().numpy(), ref)
    diag(f"sampler package unipc fp32 captured vs oracle: {e:.3e} (bar {FP32_SAMPLED_TOL:g})")
    assert e < FP32_SAMPLED_TOL


@pytest.mark.parametrize("what", ["scaled", "twice", "noise", "not-the-module"])
def test_unrecognised_models_run_the_device_path(what, modules, inputs, monkeypatch, diag):
    """each is served a call per step, never refused, and agrees with an explicit per-step loop (``schedule.run_table_numpy`` around the same x0)"""
    import sampler
    import torch
    from ns2vc_amd import schedule as S
    monkeypatch.setattr(sampler, "capture", True)
    m = modules["fp32"]
    st = StandIn(m)
    data = {"data": inputs[1:]}
    if what == "scaled":
        x0 = lambda x, t, **kw: 0.5 * st.wrapped(x, t, **kw)      # noqa: E731
    elif what == "twice":
        x0 = lambda x, t, **kw: 0.5 * (st.wrapped(x, t, **kw) + st.wrapped(0.5 * x, t, **kw))      # noqa: E731
    elif what == "not-the-module":
        x0 = lambda x, t, **kw: _synthetic_x0(x, t)      # noqa: E731
    else:
        x0 = st.wrapped
    model, model_type = x0, "x_start"
    if what == "noise":
        sched = S.VPSchedule(S.linear_betas())

        def model(x, t_input, **kw):      # eps = (x - alpha x0) / sigma at the continuous time of t_input
            t = float(t_input[0]) / 1000.0 + 1e-3
            return (x - np.float32(sched.alpha(t)) * x0(x, t_input, **kw)) / np.float32(sched.sigma(t))
        model_type = "noise"
    calls = m.engine_calls
    s, y = _run(model, inputs, "unipc", model_type)
    assert s.last_path == "device"
    per_call = {"scaled": 1, "twice": 2, "noise": 1, "not-the-module": 0}[what]
    assert m.engine_calls == calls + 6 * per_call      # (the probe's evaluation is the loop's first)
    table = S.build_table("unipc", 6, order=2)
    with torch.no_grad():
        ref = S.run_table_numpy(table, lambda xx, tt: x0(torch.from_numpy(xx).cuda(), torch.from_numpy(tt).cuda(), **data).cpu().numpy(),
                                inputs[0].cpu().numpy())
    e = rel_l2(y.cpu().numpy(), ref)
    diag(f"sampler package, unrecognised ({what}): device path vs an explicit per-step loop {e:.3e} (bar {FP32_SAMPLED_TOL:g})")
    assert e < FP32_SAMPLED_TOL


def test_new_weights_rebuild_the_cached_denoiser(inputs, monkeypatch):
    import sampler
    monkeypatch.setattr(sampler, "capture", True)
    m = _module("fp32")
    s, y0 = _run(StandIn(m).wrapped, inputs)
    s, again = _run(StandIn(m).wrapped, inputs)
    held = m._sampler_denoiser[1]
    assert s.last_path == "captured" and np.array_equal(again.cpu().numpy(), y0.cpu().numpy())
    m.load_state_dict(_weights(1), strict=True)
    s, y1 = _run(StandIn(m).wrapped, inputs)
    assert s.last_path == "captured" and m._sampler_denoiser[1] is not held
    assert np.array_equal(y1.cpu().numpy(), _direct(m, inputs, "unipc").cpu().numpy())
    assert rel_l2(y1.cpu().numpy(), y0.cpu().numpy()) > 1e-2
