"""CPU checks of classifier-free guidance: the host statement ``schedule.guided_x0`` and ``run_table_numpy`` against the reference's own guided
loops (tests/golden/golden_v7.npz, make_golden_v7.py), the argument checks and the routing of ``Denoiser.sample``, the exports, the register
audit of the update kernel."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from ns2vc_amd import schedule as S
from recording_engine import denoiser as _denoiser      # the real Denoiser constructor on the recording engine -> (denoiser, recording)
from util import synthetic_x0

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden", "golden_v7.npz")

SCALES = (0.0, 0.5, 1.0, 2.5, 7.0)
SKIPS = ("logSNR", "time_uniform", "time_quadratic")
# the g16 grid of make_golden_v7.py: (solver, steps, order, skip_type, variant, scale)
CASES = [(sv, n, o, "logSNR", v, s) for sv, vs in (("unipc", ("bh2", "bh1")), ("dpmsolver++", (None,))) for v in vs for o in (1, 2, 3)
         for n in (5, 8) for s in SCALES]
CASES += [(sv, 8, 2, k, v, 2.5) for sv, v in (("unipc", "bh2"), ("dpmsolver++", None)) for k in SKIPS[1:]]
# Relative L2 of run_table_numpy (float32) against the reference's float32 loop, measured on this grid.  The reference combines eps_u + s (eps_c -
# eps_u) with eps = (x - alpha x0) / sigma rounded to float32 in each half; the table combines x0 and rounds eps once, so the two differ by
# float32 rounding that the scale multiplies.  Worst case per scale over the 94 cases: 0 -> 1.54e-6, 0.5 -> 1.85e-6, 1 -> 1.39e-6,
# 2.5 -> 5.54e-6, 7 -> 8.04e-5 (unipc3_logSNR_8_s7).  Each gate is twice the worst case observed at that scale.
GUIDED_TOL = {0.0: 3.1e-6, 0.5: 3.7e-6, 1.0: 2.8e-6, 2.5: 1.11e-5, 7.0: 1.61e-4}


def case_tag(solver, steps, order, skip, variant, scale):
    return (f"{'unipc' if solver == 'unipc' else 'dpmpp'}{order}_{skip}_{steps}" + ("_bh1" if variant == "bh1" else "") + f"_s{scale:g}").replace(".", "p")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_golden_grid_is_the_one_asked_for(gold):
    """orders 1-3, both solvers, bh1 and bh2, 5 and 8 steps, the five scales, the three time grids at one scale"""
    assert len(CASES) == 94 and len({case_tag(*c) for c in CASES}) == 94
    assert sorted(k[4:-2] for k in gold.files if k.endswith(".y")) == sorted(case_tag(*c) for c in CASES)
    assert {c[5] for c in CASES} == set(SCALES) and {c[3] for c in CASES} == set(SKIPS) and {c[2] for c in CASES} == {1, 2, 3}


@pytest.mark.parametrize("case", CASES, ids=[case_tag(*c) for c in CASES])
def test_run_table_numpy_guided_against_reference(case, gold):
    """``run_table_numpy`` with x0_fn = guided_x0(x0(x, t, u), x0(x, t, c), s) reproduces the reference's guided loop.
    Measured: worst 8.04e-5 (scale 7), 5.54e-6 at scale 2.5, <= 1.85e-6 at scales <= 1; gated at twice the worst per scale (GUIDED_TOL)."""
    solver, steps, order, skip, variant, scale = case
    tag = case_tag(*case)
    t = S.build_table(solver, steps, order=order, skip_type=skip, **({"variant": variant} if variant else {}))
    ref, times = gold[f"g16.{tag}.y"], gold[f"g16.{tag}.times"]
    assert t.steps == len(times)       # (a guided evaluation is ONE model call of two items, also at scale 1: one call either way)
    np.testing.assert_allclose(t.t_model, times, rtol=1e-6, atol=2e-4)
    u, c = gold["g16.uncond"], gold["g16.cond"]
    y = S.run_table_numpy(t, lambda x, tm: S.guided_x0(synthetic_x0(x, tm, u), synthetic_x0(x, tm, c), np.float32(scale)), gold["g16.x_T"])
    e = rel_l2(y, ref)
    print(f"{tag}: {e:.3e}")
    assert e <= GUIDED_TOL[scale], e


def test_guidance_matters_in_the_goldens(gold):
    """the scales give different latents (a test that passes with the scale ignored shows nothing)"""
    ys = [gold[f"g16.{case_tag('unipc', 8, 2, 'logSNR', 'bh2', s)}.y"] for s in SCALES]
    for a, b in zip(ys, ys[1:]):
        assert rel_l2(a, b) > 1e-2


def test_guided_x0_select_and_broadcast():
    f = np.float32
    rng = np.random.default_rng(0)
    u, c = rng.standard_normal((3, 4, 5)).astype(f), rng.standard_normal((3, 4, 5)).astype(f)
    un = u.copy()
    un[1, 2, 3] = np.nan
    un[0, 0, 0] = np.inf
    assert S.guided_x0(un, c, 1.0).tobytes() == c.tobytes()                  # scale 1 IS x0_c, whatever x0_u holds
    assert S.guided_x0(un, c, f(1)).dtype == f
    np.testing.assert_array_equal(S.guided_x0(u, c, 0.0), u)                  # scale 0 is x0_u
    s = np.array([0.0, 1.0, 2.5], f)
    y = S.guided_x0(u, c, s)
    np.testing.assert_array_equal(y[0], u[0])
    assert y[1].tobytes() == c[1].tobytes()
    np.testing.assert_array_equal(y[2], u[2] + f(2.5) * (c[2] - u[2]))
    y = S.guided_x0(un, c, s)                                                  # a NaN of item 1's x0_u reaches nothing
    assert y[1].tobytes() == c[1].tobytes() and np.isfinite(y[2]).all()
    with pytest.raises(ValueError):
        S.guided_x0(u, c, np.ones(2, f))
    with pytest.raises(ValueError):
        S.guided_x0(u, c, np.ones((3, 1), f))


# ---- Denoiser: argument errors before anything runs, routing --------------------------------------
def _shapes(args):
    return tuple(None if v is None else tuple(v[1]) for v in args.values())


BAD = [
    (dict(guidance_scale=[1.0, 2.0, 3.0]), "guidance_scale"),                                        # scale shape: not (B,)
    (dict(guidance_scale=np.ones((2, 1))), "guidance_scale"),
    (dict(guidance_scale=float("nan"), unconditional_prompt=torch.zeros(1, 3, 256)), "finite"),
    (dict(guidance_scale=[2.0, float("inf")], unconditional_prompt=torch.zeros(1, 3, 256)), "finite"),
    (dict(guidance_scale=2.0, unconditional_prompt=torch.zeros(3, 3, 256)), "unconditional_prompt"),   # wrong batch
    (dict(guidance_scale=2.0, unconditional_prompt=torch.zeros(3, 256)), "unconditional_prompt"),
    (dict(guidance_scale=2.0, unconditional_prompt=torch.zeros(1, 3, 256), unconditional_prompt_mask=torch.ones(3, 3, dtype=torch.bool)), "mask"),
    (dict(guidance_scale=2.0, unconditional_prompt=torch.zeros(1, 3, 256), unconditional_prompt_lengths=[1, 2, 3]), "lengths"),
    (dict(guidance_scale=2.0, unconditional_prompt=torch.zeros(1, 3, 256), unconditional_content=torch.zeros(3, 256, 16)), "unconditional_content"),
    (dict(guidance_scale=2.0, unconditional_content=torch.zeros(2, 256, 16)), "need an unconditional_prompt"),
]


@pytest.mark.parametrize("kw,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_bad_guidance_arguments_raise_before_any_engine_call(kw, match, monkeypatch):
    """the checks run in ``SampleRequest.parse`` / ``check_guidance``, in front of everything: no engine call is recorded"""
    from ns2vc_amd.request import SampleRequest
    d, rec = _denoiser(monkeypatch)
    c, p = torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256))
    with pytest.raises(ValueError, match=match):
        SampleRequest.parse(d, c, p, solver="unipc", steps=5, **kw)
    with pytest.raises(ValueError, match=match):
        d.sample(c, p, solver="unipc", steps=5, **kw)
    with pytest.raises(ValueError, match=match):
        d.denoise(torch.zeros(2, 100, 16), torch.zeros(2), c, p, **kw)
    assert rec.calls == []


@pytest.mark.parametrize("kw", [dict(), dict(guidance_scale=3.0), dict(guidance_scale=1.0, unconditional_prompt=torch.zeros(1, 3, 256)),
                                dict(guidance_scale=[1.0, 1.0], unconditional_prompt=torch.zeros(2, 3, 256))],
                         ids=["default", "no-uncond", "scale-1", "all-scales-1"])
def test_unguided_routes_never_prepare_2b(kw, monkeypatch):
    """every scale 1, or no unconditional prompt: today's B-item path (the reference's short cut, uni_pc.py:222-223)"""
    d, rec = _denoiser(monkeypatch)
    c, p = torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256))
    y = d.sample(c, p, noise=torch.zeros(2, 100, 16), solver="unipc", steps=5, **kw)
    assert tuple(y.shape) == (2, 100, 16)
    assert rec.of("prepare") == [dict(B=2, T=16, Lp=8)]
    assert not rec.of("set_guidance")
    assert [_shapes(a) for a in rec.of("set_condition")] == [((2, 256, 16), (2, 8, 256), None)] and [a["x"][1] for a in rec.of("sample")] == [[2, 100, 16]]


def test_guided_route_prepares_2b_and_builds_the_condition(monkeypatch):
    """cat([unconditional, conditional]); Lu != Lp: zero-padded to the longer, every row its own frame count; B items in and out"""
    d, rec = _denoiser(monkeypatch)
    c, p = torch.randn((2, 256, 16)), torch.randn((2, 8, 256))
    u = torch.randn((1, 3, 256))
    y = d.sample(c, p, noise=torch.zeros(2, 100, 16), solver="unipc", steps=5, guidance_scale=[2.5, 1.0], unconditional_prompt=u, lengths=[16, 9])
    assert tuple(y.shape) == (2, 100, 16)
    assert rec.calls[0][1:] == ("prepare", dict(B=4, T=16, Lp=8)) and rec.calls[1][1:] == ("set_guidance", dict(scales=[2.5, 1.0]))
    assert rec.of("set_lengths") == [dict(lengths=[16, 9, 16, 9])] and rec.of("set_prompt_lengths") == [dict(prompt_lengths=[3, 3, 8, 8])]
    assert [_shapes(a) for a in rec.of("set_condition")] == [((4, 256, 16), (4, 8, 256), None)] and [a["x"][1] for a in rec.of("sample")] == [[2, 100, 16]]
    from ns2vc_amd.pipeline import Denoiser
    c2, p2, m2, l2, pl2 = Denoiser._guided_condition(c, p, None, None, [8, 5], u, torch.tensor([[True, True, False]]), None, None)
    assert torch.equal(c2, torch.cat([c, c])) and torch.equal(p2[2:], p) and torch.equal(p2[0, :3], u[0]) and not p2[:2, 3:].any()
    assert m2.tolist() == [[True, True, False] + [False] * 5] * 2 + [[True] * 8] * 2 and l2 is None and pl2.tolist() == [3, 3, 8, 5]
    # a later unguided call on the same instance leaves the engine's guidance off again (the B-item prepare clears it, as Engine.prepare does)
    assert rec.engines[0].guidance is not None
    d.sample(c, p, noise=torch.zeros(2, 100, 16), solver="unipc", steps=5)
    assert rec.names()[-1] == "sample" and rec.engines[0].guidance is None and rec.of("prepare")[-1] == dict(B=2, T=16, Lp=8)


def test_guided_tail_extra():
    """ceil(log3 of the rounding gain sqrt((1 - s)^2 + s^2) of the largest scale); nothing for scales in [0, 1]"""
    from ns2vc_amd.pipeline import guided_tail_extra
    assert [guided_tail_extra(v) for v in ([0.0], [0.5, 1.0], [1.5], [2.5, 0.5], [3.0], [4.0], [7.0], [-1.0])] == [0, 0, 1, 1, 2, 2, 3, 1]


def test_engine_set_guidance_validates_on_the_host():
    from ns2vc_amd.engine import Engine
    e = Engine.__new__(Engine)       # (no device: only the argument checks in front of the C call)
    e.shape, e.guidance = (6, 100, 20), None
    with pytest.raises(ValueError, match="B = 4"):
        e.set_guidance([1.0, 2.0])
    with pytest.raises(ValueError, match="finite"):
        e.set_guidance([1.0, float("nan"), 2.0])


def test_grouped_converter_halves_its_batches_under_guidance():
    from ns2vc_amd.service import GroupedConverter
    u = torch.zeros(1, 3, 256)
    assert GroupedConverter(None, None, max_batch=8, guidance_scale=2.0, unconditional_prompt=u).max_batch == 4
    assert GroupedConverter(None, None, max_batch=8, guidance_scale=1.0, unconditional_prompt=u).max_batch == 8
    assert GroupedConverter(None, None, max_batch=8, guidance_scale=2.0).max_batch == 8
    g = GroupedConverter(None, None, max_batch=8, guidance_scale=2.0, unconditional_prompt=u)
    assert g.kw["guidance_scale"] == 2.0 and g.kw["unconditional_prompt"] is u


# ---- sample_sharded slices the per-item guidance arguments with the batch (gloo, world 2) ------------
_SHARD_WORKER = r'''
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, sys.argv[1])
from ns2vc_amd.dist import shard_range
from ns2vc_amd.pipeline import Denoiser
from ns2vc_amd.spec import UNetConfig
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
n, T, Lp, Lu = 5, 8, 4, 2                            # uneven shards: 3 + 2
lo, hi = shard_range(n, rank, world)
d = Denoiser.__new__(Denoiser)
d.cfg = UNetConfig()
seen = {}
def fake_sample(content, prompt, prompt_mask=None, noise=None, **kw):
    seen.update(kw, content=content)
    s = torch.as_tensor(np.asarray(kw["guidance_scale"], np.float32)).reshape(-1, 1, 1)
    u = kw["unconditional_prompt"]
    return noise + s + u.sum(dim=(1, 2)).reshape(-1, 1, 1) + kw["unconditional_content"].sum(dim=(1, 2)).reshape(-1, 1, 1)
d.sample = fake_sample
content, prompt, noise = torch.zeros(n, 256, T), torch.zeros(n, Lp, 256), torch.zeros(n, 100, T)
scales = np.arange(n, dtype=np.float32) + 0.5
up = torch.arange(n, dtype=torch.float32).reshape(n, 1, 1).expand(n, Lu, 256) * 1e-3
uc = torch.arange(n, dtype=torch.float32).reshape(n, 1, 1).expand(n, 256, T) * 1e-4
um, ul = torch.ones(n, Lu, dtype=torch.bool), np.arange(n) % Lu + 1
out = d.sample_sharded(content, prompt, None, noise, guidance_scale=scales, unconditional_prompt=up, unconditional_prompt_mask=um,
                       unconditional_prompt_lengths=ul, unconditional_content=uc, solver="unipc", steps=4)
assert np.array_equal(np.asarray(seen["guidance_scale"]), scales[lo:hi]) and seen["content"].shape[0] == hi - lo
assert torch.equal(seen["unconditional_prompt"], up[lo:hi]) and torch.equal(seen["unconditional_content"], uc[lo:hi])
assert seen["unconditional_prompt_mask"].shape[0] == hi - lo and np.array_equal(seen["unconditional_prompt_lengths"], ul[lo:hi])
want = torch.from_numpy(scales).reshape(-1, 1, 1) + up.sum(dim=(1, 2)).reshape(-1, 1, 1) + uc.sum(dim=(1, 2)).reshape(-1, 1, 1) + noise
assert out.shape == (n, 100, T) and torch.equal(out, want)
# a scalar scale and ONE shared unconditional prompt go to every rank whole
out = d.sample_sharded(content, prompt, None, noise, guidance_scale=2.0, unconditional_prompt=up[:1], unconditional_content=uc, solver="unipc", steps=4)
assert seen["guidance_scale"] == 2.0 and torch.equal(seen["unconditional_prompt"], up[:1]) and out.shape == (n, 100, T)
dist.barrier(); dist.destroy_process_group()
'''


def test_sample_sharded_slices_guidance_arguments_gloo_world2(tmp_path):
    import subprocess
    import sys
    script = tmp_path / "worker.py"
    script.write_text(_SHARD_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29523", WORLD_SIZE="2")
    procs = [subprocess.Popen([sys.executable, str(script), ROOT], env=dict(env, RANK=str(r)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    logs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), logs


# ---- the library ------------------------------------------------------------------------------
def test_library_exports_guidance_symbols_abi_still_7():
    from ns2vc_amd import _lib
    lib = _lib.load()
    assert lib.ns2vc_abi_version() == 7
    hdr = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    assert re.search(r"#define NS2VC_ABI_VERSION 7\b", hdr)
    raw = C.CDLL(lib._name)
    for sym in ("ns2vc_sampler_set_guidance", "ns2vc_k_solver_update_guided"):
        assert hasattr(raw, sym), sym
        assert re.search(r"\bint " + sym + r"\(", hdr), sym
    assert lib.ns2vc_sampler_set_guidance(None, None, 0, None) != 0      # a null handle is an error, not a crash
    assert b"null engine handle" in lib.ns2vc_last_error()


def test_solver_update_kernels_use_no_scratch():
    """all twelve instantiations <TM, H2, GD> of solver_update_kernel in the gfx950 code object: no scratch, no spilled VGPR"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I../../include", "-Rpass-analysis=kernel-resource-usage", "-c", "misc.hip",
                        "-o", os.devnull], cwd=os.path.join(ROOT, "ns2vc_amd", "csrc"), capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out, fn = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and fn:
            out.setdefault(fn, {})[m.group(1)] = int(m.group(2))
    k = {n: v for n, v in out.items() if "solver_update_kernel" in n}
    assert len(k) == 12 and len([n for n in k if re.search(r"Lb[01]ELb1EE+v", n)]) == 6, sorted(k)
    bad = [(n, v) for n, v in k.items() if v.get("ScratchSize [bytes/lane]", -1) != 0 or v.get("VGPRs Spill", -1) != 0]
    assert not bad, bad
