"""Known frames on the host: the closed form of a held frame on ``schedule.run_table_numpy(hold=)``, independence of the items,
``plan_chunks``, the argument checks of ``Denoiser.sample(known=, known_mask=)`` / ``sample_long`` on a stub engine, and the exports."""
import os
import re

import numpy as np
import pytest
import torch

from ns2vc_amd import schedule as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, C, T = 3, 6, 19


def rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)) / np.linalg.norm(np.asarray(b, np.float64)))


def _data(seed=0):
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal((B, C, T)).astype(np.float32)
    known = (0.7 * rng.standard_normal((B, C, T))).astype(np.float32)
    mask = np.zeros((B, T), dtype=bool)
    mask[0, :5] = True           # a head, as a chunk of sample_long holds it
    mask[2, 7:11] = True         # an island and the last frame; item 1 holds nothing
    mask[2, T - 1] = True
    return noise, known, mask


def _x0_fn(x, t):
    """a nonlinear stand-in for the UNet that mixes neither items nor frames: what it gives on a held frame is overwritten anyway"""
    return (0.5 * np.tanh(x) + 1e-4 * t[:, None, None]).astype(np.float32)


def _end_coefficients(table):
    """(alpha, sigma) of the point the table's last row lands on; (1, 0) where the last row returns x_start (denoise_to_zero, ddim)"""
    if table.coef[-1, 5] == 0 and table.coef[-1, 6] == -1:
        return 1.0, 0.0
    sched = S.VPSchedule(S.linear_betas())
    t_end = float(table.timesteps[-1])
    return sched.alpha(t_end), sched.sigma(t_end)


# the ten cases of the issue: (solver, steps, order, eta, options)
CASES = [
    ("unipc", 20, 1, 0.0, {}),
    ("unipc", 20, 2, 0.0, {}),
    ("unipc", 20, 2, 0.0, dict(variant="bh1")),
    ("unipc", 10, 3, 0.0, dict(skip_type="logSNR")),
    ("unipc", 8, 2, 0.0, dict(t_start=0.6)),
    ("dpmsolver++", 20, 2, 0.0, {}),
    ("dpmsolver++", 20, 2, 0.0, dict(solver_type="taylor")),
    ("dpmsolver++", 12, 3, 0.0, {}),
    ("unipc", 20, 2, 0.0, dict(denoise_to_zero=True)),
    ("ddim", 10, 2, 0.0, {}),
]
CLOSED_FORM_TOL = 2e-6      # the issue's bound: three times the worst case measured on the host statement (6.0e-7, DPM-Solver++ 3M)


def _table(solver, steps, order, eta, opts):
    betas = S.linear_betas(1000, np.float64) if solver in S.DISCRETE_SOLVERS else None
    return S.build_table(solver, steps, betas, order, eta, **opts)


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-o{c[2]}-{'-'.join(map(str, c[4].values())) or 'plain'}" for c in CASES])
def test_held_frames_follow_the_forward_marginal(case):
    """x_i = alpha_i k + sigma_i eps on a held frame, at every order and for both continuous solvers; k itself where the table ends on x_start"""
    table = _table(*case)
    noise, known, mask = _data()
    x_T = S.known_start(noise, known, mask, table.coef[0])
    trace = []
    out = S.run_table_numpy(table, _x0_fn, x_T, hold=(known, mask), trace=trace)
    a_end, s_end = _end_coefficients(table)
    m3 = np.broadcast_to(mask[:, None, :], out.shape)
    want = a_end * known.astype(np.float64) + s_end * noise.astype(np.float64)
    err = rel_l2(out[m3], want[m3])
    print(f"{case}: rel-L2 of the held frames against the closed form {err:.2e}")
    assert err < CLOSED_FORM_TOL
    # ... and on the way: after row i the state stands at the NEXT row's (alpha, sigma)
    for i in range(table.steps - 1):
        a, s = np.float64(table.coef[i + 1, 1]), np.float64(table.coef[i + 1, 2])
        assert rel_l2(trace[i][m3], (a * known + s * noise)[m3]) < 10 * CLOSED_FORM_TOL, i
    # the free frames are the model's: they moved away from the unheld run only through nothing at all here (x0_fn mixes no frames)
    plain = S.run_table_numpy(table, _x0_fn, x_T)
    assert np.array_equal(out[~m3], plain[~m3])


def test_known_start_and_hold_x0_touch_the_masked_frames_only():
    noise, known, mask = _data(1)
    table = S.build_table("unipc", 6)
    x_T = S.known_start(noise, known, mask, table.coef[0])
    m3 = np.broadcast_to(mask[:, None, :], noise.shape)
    assert np.array_equal(x_T[~m3], noise[~m3])
    a, s = np.float32(table.coef[0, 1]), np.float32(table.coef[0, 2])
    assert np.array_equal(x_T[m3], (a * known + s * noise)[m3]) and x_T.dtype == np.float32
    rows = np.stack([S.build_table("unipc", 6).coef[0], S.build_table("dpmsolver++", 8, t_start=0.5).coef[0], table.coef[0]])
    per_item = S.known_start(noise, known, mask, rows)
    assert np.array_equal(per_item[0], x_T[0]) and np.array_equal(per_item[2], x_T[2])
    x0 = S.hold_x0(noise, (known, mask))
    assert np.array_equal(x0[m3], known[m3]) and np.array_equal(x0[~m3], noise[~m3])
    assert S.hold_x0(noise, None) is noise
    for bad in ((known, None), (known[:, :, :-1], mask), (known, mask.astype(np.uint8)), (known, mask[:2])):
        with pytest.raises(ValueError):
            S.run_table_numpy(table, _x0_fn, noise, hold=bad)
    with pytest.raises(ValueError, match="correction"):
        S.run_table_numpy(table, _x0_fn, noise, hold=(known, mask), correct_x0=dict(mode="clamp"))
    with pytest.raises(ValueError, match="coef_row0"):
        S.known_start(noise, known, mask, rows[:2])


def test_a_held_item_in_a_batch_equals_the_item_alone():
    """bit for bit, in run_table_numpy and in run_tables_numpy with mixed schedules (a stochastic item among them)"""
    noise, known, mask = _data(2)
    table = S.build_table("dpmsolver++", 7, order=3)
    x_T = S.known_start(noise, known, mask, table.coef[0])
    full = S.run_table_numpy(table, _x0_fn, x_T, hold=(known, mask))
    for b in range(B):
        alone = S.run_table_numpy(table, _x0_fn, x_T[b:b + 1], hold=(known[b:b + 1], mask[b:b + 1]))
        assert np.array_equal(full[b:b + 1], alone), b
    specs = [dict(solver="unipc", steps=6), dict(solver="dpmsolver++", steps=8, order=3), dict(solver="ddim", steps=5, eta=0.5)]
    betas64 = S.linear_betas(1000, np.float64)
    tabs = S.build_tables(specs, None, betas64)
    x_T = S.known_start(noise, known, mask, np.stack([tabs.table_of(b).coef[0] for b in range(B)]))
    rng = np.random.default_rng(5)
    z = rng.standard_normal((B, 16, C, T)).astype(np.float32)
    full = S.run_tables_numpy(tabs, _x0_fn, x_T, noise_fn=lambda b, j: z[b, j], hold=(known, mask))
    for b in range(B):
        one = S.build_tables([specs[b]], None, betas64)
        alone = S.run_tables_numpy(one, _x0_fn, x_T[b:b + 1], noise_fn=lambda _, j, b=b: z[b, j], hold=(known[b:b + 1], mask[b:b + 1]))
        assert np.array_equal(full[b:b + 1], alone), b
    m3 = np.broadcast_to(mask[:, None, :], full.shape)
    assert rel_l2(full[2][m3[2]], known[2][m3[2]]) < CLOSED_FORM_TOL      # the ddim item ends on k


@pytest.mark.parametrize("chunk", [8, 128])
def test_plan_chunks_properties(chunk):
    for overlap in (0, 1, 7, chunk - 1):
        for L in range(1, 401):
            ch = S.plan_chunks(L, chunk, overlap)
            assert ch[0][0] == 0 and ch[-1][1] == L                                    # they cover [0, L) ...
            for (a0, a1), (b0, b1) in zip(ch, ch[1:]):
                assert a1 - b0 == overlap and b1 > a1                                   # ... share exactly `overlap` frames, each adds a new one
            assert all(0 < b - a <= chunk for a, b in ch)
            assert [a for a, _ in ch] == [j * (chunk - overlap) for j in range(len(ch))]
            assert all(b == min(a + chunk, L) for a, b in ch)
            assert len(ch) == 1 or ch[-1][0] + overlap < L


def test_plan_chunks_refuses_bad_arguments():
    for args in ((0, 8, 0), (10, 0, 0), (10, 8, 8), (10, 8, -1), (10, 8, 9)):
        with pytest.raises(ValueError):
            S.plan_chunks(*args)


# ---- Denoiser.sample on the recording engine (tests/recording_engine.py) ----------------------------------------------------------------
def _denoiser(monkeypatch):
    """the real constructor on the recording engine; ``d.rec`` is the recording"""
    import recording_engine
    return recording_engine.denoiser(monkeypatch)[0]


def _args(n=2, t=16):
    c, p = torch.zeros((n, 256, t)), torch.zeros((n, 8, 256))
    x = torch.arange(n * 100 * t, dtype=torch.float32).reshape(n, 100, t) / 1000
    k = torch.ones((n, 100, t))
    m = np.zeros((n, t), dtype=bool)
    m[0, :3] = True
    return c, p, x, k, m


def test_every_refusal_raises_before_any_engine_call(monkeypatch):
    d = _denoiser(monkeypatch)
    c, p, x, k, m = _args()
    bad = [
        (dict(known=k), "given together"),
        (dict(known_mask=m), "given together"),
        (dict(known=k[:, :, :-1], known_mask=m), r"known must be \(2, 100, 16\)"),
        (dict(known=k[:1], known_mask=m), r"known must be \(2, 100, 16\)"),
        (dict(known=k, known_mask=m[:, :-1]), r"known_mask must be a bool \(2, 16\)"),
        (dict(known=k, known_mask=m.astype(np.uint8)), "known_mask must be a bool"),
        (dict(known=k, known_mask=m, correcting_x0_fn="clamp"), r"correcting_x0_fn= / corrections="),
        (dict(known=k, known_mask=m, corrections=[None, dict(correcting_x0_fn="clamp")]), r"correcting_x0_fn= / corrections="),
        (dict(known=k, known_mask=m, lengths=[2, 16]), r"known_mask\[0\] holds frame 2, at or past lengths\[0\] = 2"),
        (dict(known=k, known_mask=m, lengths=[16]), "one entry per item"),
    ]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            d.sample(c, p, noise=x, solver="unipc", steps=5, **kw)
    assert d.rec.calls == []
    d.sample(c, p, noise=x, solver="unipc", steps=5, known=k, known_mask=m, lengths=[3, 16])      # (the last held frame is the item's last)
    assert d.rec.of("set_known")


def test_an_all_false_mask_routes_to_the_plain_call(monkeypatch):
    import recording_engine as R
    d = _denoiser(monkeypatch)
    rec, eng = d.rec, d.engine
    c, p, x, k, m = _args()
    d.sample(c, p, noise=x, solver="unipc", steps=5, known=k, known_mask=np.zeros_like(m))
    assert not rec.of("set_known")
    assert rec.of("sample")[-1]["x"] == R.digest(x)                                     # x_T untouched
    # held: the mask reaches the engine after its lengths, x_T is known_start, and a later plain call switches the hold off again
    d.sample(c, p, noise=x, solver="unipc", steps=5, known=k, known_mask=m, lengths=[16, 9])
    names = rec.names()
    i = max(j for j, n in enumerate(names) if n == "set_known")
    assert "set_lengths" in names[:i] and names[i + 1] == "sample"
    assert rec.calls[i][2]["mask"] == R.digest(m) and rec.calls[i][2]["known"][1] == [2, 100, 16]
    want = S.known_start(x.numpy(), k.numpy(), m, eng.table.coef[0])
    assert rec.of("sample")[-1]["x"] == R.digest(want)
    d.sample(c, p, noise=x, solver="unipc", steps=5)
    assert rec.calls[-2][1:] == ("set_known", dict(known=None, mask=None)) and eng.hold is None
    # a correction after a hold: the hold goes first (the engine refuses the pair)
    d.sample(c, p, noise=x, solver="unipc", steps=5, known=k, known_mask=m)
    d.sample(c, p, noise=x, solver="unipc", steps=5, correcting_x0_fn="clamp")
    names = rec.names()
    j = max(q for q, n in enumerate(names) if n == "set_x0_correction")
    assert rec.calls[j - 1][1:] == ("set_known", dict(known=None, mask=None))


@pytest.mark.parametrize("item_corrections", [False, True])
def test_open_slots_after_a_held_call_at_the_same_shape(monkeypatch, item_corrections):
    """the hold an earlier sample(known=) left in the engine is switched off before the slot loop opens (same shape: no prepare clears it)"""
    d = _denoiser(monkeypatch)
    c, p, x, k, m = _args()
    d.sample(c, p, noise=x, solver="unipc", steps=5, known=k, known_mask=m)
    assert d.engine.hold is not None
    d.open_slots(2, 16, 8, item_corrections=item_corrections)
    names = d.rec.names()
    assert names[-1] == "open_slots" and d.engine.hold is None
    i = max(j for j, n in enumerate(names) if n == "set_known")
    assert d.rec.calls[i][2] == dict(known=None, mask=None) and i > names.index("sample")
    assert names.count("prepare") == 1                                                # (the shape did not change)


def test_an_all_false_mask_with_a_correction_is_the_corrected_call(monkeypatch):
    d = _denoiser(monkeypatch)
    c, p, x, k, m = _args()
    d.sample(c, p, noise=x, solver="unipc", steps=5, known=k, known_mask=np.zeros_like(m), correcting_x0_fn="clamp")
    assert d.engine.x0_correction is not None and not d.rec.of("set_known")


def test_sample_long_chains_the_chunks(monkeypatch):
    """on a stub ``sample``: the batches, their lengths, the known frames they hold and the stitching"""
    d = _denoiser(monkeypatch)
    Ttot, chunk, V = 50, 16, 4
    c = torch.arange(2 * Ttot, dtype=torch.float32).reshape(2, 1, Ttot).repeat(1, 256, 1)
    p = torch.zeros((2, 8, 256))
    noise = torch.randn((2, 100, Ttot))
    lens = [50, 20]
    seen = []

    def fake_sample(content, prompt, prompt_mask=None, noise=None, lengths=None, seeds=None, known=None, known_mask=None, **kw):
        seen.append(dict(content=content, noise=noise, lengths=lengths, seeds=seeds, known=known, known_mask=known_mask, kw=kw))
        return content[:, :100, :] + 1000.0 * len(seen)

    d.sample = fake_sample
    out = d.sample_long(c, p, noise=noise, chunk_frames=chunk, overlap_frames=V, lengths=lens, solver="unipc", steps=5, seeds=[7, 9])
    plans = [S.plan_chunks(L, chunk, V) for L in lens]
    assert len(seen) == len(plans[0]) == 4 and len(plans[1]) == 2
    for j, call in enumerate(seen):
        items = [b for b in range(2) if len(plans[b]) > j]
        assert call["content"].shape[0] == len(items) and list(call["seeds"]) == [[7, 9][b] for b in items]
        assert list(call["lengths"]) == [plans[b][j][1] - plans[b][j][0] for b in items]
        assert call["kw"] == dict(solver="unipc", steps=5)
        for i, b in enumerate(items):
            s0, s1 = plans[b][j]
            assert torch.equal(call["noise"][i, :, :s1 - s0], noise[b, :, s0:s1])
            assert torch.equal(call["content"][i, 0, :s1 - s0], c[b, 0, s0:s1])
            if j == 0:
                assert call["known"] is None and call["known_mask"] is None
            else:
                assert call["known_mask"][i, :V].all() and not call["known_mask"][i, V:].any()
                assert torch.equal(call["known"][i, :, :V], out[b, :, s0:s0 + V])      # the earlier chunk's last frames, as the output has them
    for b in range(2):
        assert torch.equal(out[b, :, lens[b]:], torch.zeros_like(out[b, :, lens[b]:]))
        for j, (s0, s1) in enumerate(plans[b]):
            lo = s0 + (V if j else 0)
            assert torch.equal(out[b, 0, lo:s1], c[b, 0, lo:s1] + 1000.0 * (j + 1))
    # per-item keywords go with the items of a batch, shared ones to every batch whole
    seen.clear()
    up = torch.zeros((1, 8, 256))
    d.sample_long(c, p, noise=noise, chunk_frames=chunk, overlap_frames=V, lengths=lens, guidance_scale=np.array([2.0, 3.0], np.float32),
                  prompt_lengths=torch.tensor([8, 5]), unconditional_prompt=up)
    assert list(seen[1]["kw"]["guidance_scale"]) == [2.0, 3.0] and list(seen[2]["kw"]["guidance_scale"]) == [2.0]
    assert seen[1]["kw"]["prompt_lengths"].tolist() == [8, 5] and seen[3]["kw"]["prompt_lengths"].tolist() == [8]
    assert all(call["kw"]["unconditional_prompt"] is up for call in seen)
    # one chunk: the plain call with the caller's own arguments
    seen.clear()
    d.sample_long(c, p, noise=noise, chunk_frames=64, overlap_frames=V, solver="unipc", steps=5)
    assert len(seen) == 1 and seen[0]["content"] is c and seen[0]["lengths"] is None and seen[0]["known"] is None
    for kw in (dict(schedules=[None, None]), dict(corrections=[None, None]), dict(seeds=[1]), dict(known=noise), dict(known_mask=np.zeros((2, Ttot), bool))):
        with pytest.raises(ValueError):
            d.sample_long(c, p, noise=noise, chunk_frames=chunk, overlap_frames=V, **kw)
    with pytest.raises(ValueError):
        d.sample_long(c, p, noise=noise, chunk_frames=chunk, overlap_frames=chunk)


def test_engine_set_known_validates_on_the_host():
    from ns2vc_amd.engine import Engine
    from ns2vc_amd.spec import UNetConfig
    e = Engine.__new__(Engine)       # (no device: only the argument checks in front of the C call)
    e.cfg, e.shape, e.guidance, e.hold = UNetConfig(), (2, 16, 8), None, None
    k, m = torch.zeros((2, 100, 16)), np.zeros((2, 16), dtype=bool)
    for a in ((k, None), (None, m), (k, m[:1]), (k, m[:, :-1]), (k[:, :, :-1], m), (k.double(), m)):
        with pytest.raises(ValueError):
            e.set_known(*a)


# ---- exports ---------------------------------------------------------------------------------------------------------------------------------
def test_the_two_new_symbols_are_declared_bound_and_exported():
    from ns2vc_amd import _lib
    header = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    assert "#define NS2VC_ABI_VERSION 7" in header and _lib.ABI_VERSION == 7
    lib = _lib.load()
    assert lib.ns2vc_abi_version() == 7
    for name in ("ns2vc_sampler_set_known", "ns2vc_k_hold_x0"):
        assert re.search(r"\bint " + name + r"\(", header), name
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None, name
    for unit in ("misc.hip", "common.h"):
        assert "launch_hold_x0" in open(os.path.join(ROOT, "ns2vc_amd", "csrc", unit)).read()
