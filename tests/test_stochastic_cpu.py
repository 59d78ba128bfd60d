"""CPU tests of the stochastic samplers (DDPM, DDIM): the host statement of the device noise stream (ns2vc_amd/noise.py) and the
``ddim`` / ``ddpm`` solver tables against the reference's own loops (tests/golden/golden_v4.npz, make_golden_v4.py)."""
import os

import numpy as np
import pytest
import torch

from ns2vc_amd import noise as N
from ns2vc_amd import schedule as S
from util import synthetic_x0

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "golden_v4.npz")
SYN_CASES = [("ddim", s, e) for s in (26, 30, 100, 1000) for e in (0.0, 0.5, 1.0)] + [("ddpm", 1000, 0.0)]


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def case_tag(solver, steps, eta):
    return f"{solver}{steps}_eta{eta:g}".replace(".", "p")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---- the generator -------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, expect):
    """the Random123 known-answer vectors of Philox4x32-10"""
    assert tuple(int(v) for v in N.philox4x32_10(ctr, key)) == expect


def _philox_scalar(ctr, key):
    """a plain-integer Philox4x32-10, written from the paper independently of the vectorised one"""
    c, k = list(ctr), list(key)
    M = 0xFFFFFFFF
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) & M, (k[1] + 0xBB67AE85) & M]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M, (p0 >> 32) ^ c[3] ^ k[1], p0 & M]
    return tuple(c)


def test_gauss_layout_matches_the_counter_contract():
    """gauss(seed, step)[b, c, t] = Box-Muller of Philox(key = seed, counter = (t, c // 4, step, 0)), lane c % 4"""
    seeds = np.array([0x0123456789ABCDEF, 42], dtype=np.uint64)
    z = N.gauss(seeds, 7, 10, 5)
    assert z.shape == (2, 10, 5) and z.dtype == np.float32
    for b, t, c in [(0, 0, 0), (0, 4, 9), (1, 3, 5), (1, 2, 2)]:
        x = _philox_scalar((t, c // 4, 7, 0), N.seed_key(int(seeds[b])))
        a, bb = (x[0], x[1]) if c % 4 < 2 else (x[2], x[3])
        u1, u2 = (float(np.float32(a)) + 1.0) * 2.0 ** -32, float(np.float32(bb)) * 2.0 ** -32
        r = np.sqrt(-2.0 * np.log(u1))
        want = r * (np.cos if c % 2 == 0 else np.sin)(2 * np.pi * u2)
        assert abs(z[b, c, t] - want) < 1e-5 * max(1.0, abs(want)), (b, t, c)


def test_gauss_does_not_depend_on_the_batch():
    """an item's noise is a function of its seed, step, frame and channel alone: batch position, batch size, padded length"""
    seeds = np.array([11, 22, 33], dtype=np.uint64)
    full = N.gauss(seeds, 3, 100, 40, lengths=[40, 25, 7])
    for b, L in enumerate([40, 25, 7]):
        alone = N.gauss(seeds[b:b + 1], 3, 100, L)[0]
        assert np.array_equal(full[b, :, :L], alone)
        assert not full[b, :, L:].any()
    assert not np.array_equal(N.gauss([11], 3, 100, 8), N.gauss([11], 4, 100, 8))


def test_gauss_moments_host():
    z = N.gauss(np.arange(4, dtype=np.uint64), 0, 100, 2500).astype(np.float64).ravel()      # 1e6 samples
    n = z.size
    assert abs(z.mean()) < 5 / np.sqrt(n)
    assert abs(z.var() - 1) < 5 * np.sqrt(2 / n)
    assert abs((z ** 4).mean() - 3) < 5 * np.sqrt(96 / n)


def test_derived_seeds_depend_on_index_only():
    assert N.derive_seed(1234, 5) == N.derive_seed(1234, 5)
    assert len({N.derive_seed(1234, i) for i in range(100)}) == 100
    assert N.derive_seed(1234, 5) != N.derive_seed(1235, 5)


# ---- the tables against the reference's own loops (goldens g12) ----------------------------------
@pytest.mark.parametrize("solver,steps,eta", SYN_CASES, ids=[case_tag(*c) for c in SYN_CASES])
def test_discrete_tables_match_reference_loops(gold, solver, steps, eta):
    """build_table + run_table_numpy with the golden noise stream == the reference's ddim_sample / p_sample_loop (synthetic model):
    the evaluation times exactly (float32 truncation grid, the final (t, -1) pair), the latent to 1e-6"""
    tag = case_tag(solver, steps, eta)
    table = S.build_table(solver, steps, S.linear_betas(1000, np.float64), eta=eta)
    assert table.coef.shape == (steps, S.NCOEF) and table.coef.dtype == np.float32
    assert table.coef[:, 0].astype(np.int64).tolist() == gold[f"g12.{tag}.times"].tolist()
    seeds, x_T = gold["g12.seeds"], gold["g12.x_T"]
    B, C, T = x_T.shape
    got = S.run_table_numpy(table, synthetic_x0, x_T, noise_fn=lambda i: N.gauss(seeds, i, C, T))
    assert rel_l2(got, gold[f"g12.{tag}.y"]) <= 1e-6


def test_ddim_time_grid_is_the_float32_one():
    """26 steps: torch's float32 linspace puts knot 13 at 498.99997 -> 498; a float64 grid gives 499.0 -> 499"""
    t = S.ddim_times(26, 1000)
    assert t[-1] == -1 and t[-2] == 37 and 498 in t and 499 not in t
    assert 499 in np.linspace(-1, 999, 27).astype(np.int64).tolist()


def test_discrete_table_rows():
    b = S.linear_betas(1000, np.float64)
    ddpm = S.build_table("ddpm", 1000, b)
    assert ddpm.coef[0, 0] == 999 and ddpm.coef[-1, 0] == 0
    assert ddpm.coef[-1, 9] == 0 and (ddpm.coef[:-1, 9] > 0).all()            # no noise at t = 0
    assert not ddpm.coef[:, [3, 4, 7, 8]].any()                                 # first order: no multistep terms
    d0 = S.build_table("ddim", 100, b, eta=0.0)
    assert not d0.coef[:, 9].any()
    assert d0.coef[-1, 5] == 0 and d0.coef[-1, 6] == -1                         # (0, -1): x_start
    d1 = S.build_table("ddim", 100, b, eta=1.0)
    assert (d1.coef[:-1, 9] > 0).all() and d1.coef[-1, 9] == 0


def test_continuous_tables_have_no_noise():
    for solver in ("unipc", "dpmsolver++"):
        for steps in (1, 2, 6, 20, 50):
            for order in (1, 2):
                if steps >= order:
                    assert not S.build_table(solver, steps, order=order).coef[:, 9].any()


def test_discrete_table_errors():
    b = S.linear_betas(1000, np.float64)
    with pytest.raises(ValueError, match="len\\(betas\\)"):
        S.build_table("ddpm", 999, b)
    with pytest.raises(ValueError, match="betas"):
        S.build_table("ddpm", 1000)
    with pytest.raises(ValueError, match="eta"):
        S.build_table("ddpm", 1000, b, eta=0.5)
    with pytest.raises(ValueError, match="eta"):
        S.build_table("unipc", 20, eta=0.5)
    with pytest.raises(ValueError):
        S.build_table("ddim", 0, b)
    with pytest.raises(ValueError):
        S.build_table("ddim", 1001, b)
    with pytest.raises(ValueError):
        S.build_table("ddim", 10, b, eta=-1.0)
    t = S.build_table("ddpm", 1000, b)
    with pytest.raises(ValueError, match="noise_fn"):
        S.run_table_numpy(t, synthetic_x0, np.zeros((1, 4, 3), np.float32))


def test_denoiser_rejects_misuse_before_running(monkeypatch):
    """argument errors of Denoiser.sample surface before any device work: the recording engine (tests/recording_engine.py) sees no call"""
    import recording_engine
    d, rec = recording_engine.denoiser(monkeypatch)
    c, p = torch.zeros((2, 256, 16)), torch.zeros((2, 8, 256))
    with pytest.raises(ValueError, match="ddpm"):
        d.sample(c, p, solver="ddpm", steps=50)
    with pytest.raises(ValueError, match="eta"):
        d.sample(c, p, solver="unipc", eta=0.5)
    with pytest.raises(ValueError, match="eta"):
        d.sample(c, p, solver="ddpm", eta=1.0)
    with pytest.raises(ValueError, match="seed"):
        d.sample(c, p, solver="ddpm", seeds=[1, 2, 3])
    with pytest.raises(ValueError, match="solver"):
        d.sample(c, p, solver="euler")
    assert rec.calls == []
