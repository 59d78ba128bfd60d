"""The engine's Gaussian noise stream, restated on the host (numpy).

DDPM and DDIM with eta > 0 add fresh noise at every step.  The engine draws it inside the captured step graph
(csrc/common.h ``philox_gauss4``), from a counter-based generator, so nothing is pre-drawn and nothing is launched per step
from the host.  This module is the contract of that stream; tests and the golden generator use it.

- Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC 2011).
- Key: the item's 64-bit seed, (lo, hi).  Counter: (t, c // 4, step, 0), with t the frame within the item, c // 4 the
  channel quad and step the row of the solver table.  Nothing about the batch (B, padded T, position) enters, so an item's
  noise is the same alone, batched, ragged or sharded.
- One call gives four uint32s x0..x3, the normals of channels 4q..4q+3 at frame t, by two Box-Muller pairs (float32):
  u1 = (float(x0) + 1) * 2^-32, u2 = float(x1) * 2^-32, r = sqrt(-2 ln u1), (r cos 2 pi u2, r sin 2 pi u2); the same for (x2, x3).
  u1 lies in (0, 1], so r is finite.  The device uses precise logf / sincosf: this restatement agrees to a few float32 ulps.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
TWO_PI_F32 = np.float32(6.2831853071795864769)
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 on broadcastable uint32 arrays: ctr = (c0, c1, c2, c3), key = (k0, k1) -> (x0, x1, x2, x3) as uint32"""
    c = [np.asarray(v, dtype=np.uint64) & _U32 for v in ctr]
    k0, k1 = (np.asarray(v, dtype=np.uint64) & _U32 for v in key)
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _U32, (k1 + np.uint64(PHILOX_W1)) & _U32
        p0 = np.uint64(PHILOX_M0) * c[0]
        p1 = np.uint64(PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _U32]
    return tuple(v.astype(np.uint32) for v in c)


def _box_muller(a: np.ndarray, b: np.ndarray):
    f = np.float32
    u1 = (a.astype(f) + f(1.0)) * f(2.0 ** -32)
    u2 = b.astype(f) * f(2.0 ** -32)
    r = np.sqrt(-2.0 * np.log(u1.astype(np.float64))).astype(f)
    th = (u2 * TWO_PI_F32).astype(np.float64)
    return (r * np.cos(th).astype(f)).astype(f), (r * np.sin(th).astype(f)).astype(f)


def seed_key(seed: int):
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def gauss(seeds, step: int, C: int, T: int, lengths: Optional[Sequence[int]] = None) -> np.ndarray:
    """the normals the engine adds at table row ``step``: (B, C, T) float32 for the (B,) 64-bit ``seeds`` (NCT, the
    reference's layout).  ``lengths``: frames t >= lengths[b] are 0 (a padded batch)."""
    seeds = np.atleast_1d(np.asarray(seeds, dtype=np.uint64))
    B, Q = seeds.shape[0], (C + 3) // 4
    out = np.zeros((B, 4 * Q, T), dtype=np.float32)
    t = np.arange(T, dtype=np.uint64)[None, :]
    q = np.arange(Q, dtype=np.uint64)[:, None]
    for b in range(B):
        k0, k1 = seed_key(int(seeds[b]))
        x0, x1, x2, x3 = philox4x32_10((t, q, np.uint64(step), np.uint64(0)), (k0, k1))
        z0, z1 = _box_muller(x0, x1)
        z2, z3 = _box_muller(x2, x3)
        out[b, 0::4], out[b, 1::4], out[b, 2::4], out[b, 3::4] = z0, z1, z2, z3
        if lengths is not None:
            out[b, :, int(lengths[b]):] = 0.0
    return out[:, :C]


def draw_seeds(n: int, generator=None) -> np.ndarray:
    """(n,) uint64 seeds from a torch generator (None = torch's default one): ``generator=`` then reproduces a run"""
    import torch
    dev = generator.device if generator is not None else "cpu"
    lo = torch.randint(0, 2 ** 32, (n,), dtype=torch.int64, generator=generator, device=dev).cpu()
    hi = torch.randint(0, 2 ** 32, (n,), dtype=torch.int64, generator=generator, device=dev).cpu()
    return (hi.numpy().astype(np.uint64) << np.uint64(32)) | lo.numpy().astype(np.uint64)


def derive_seed(base: int, index: int) -> int:
    """a 64-bit seed for item ``index`` of a run seeded with ``base`` (one Philox call), so per-segment noise does not
    depend on how segments are grouped into batches"""
    k0, k1 = seed_key(base)
    x = philox4x32_10((np.uint64(int(index) & 0xFFFFFFFF), np.uint64((int(index) >> 32) & 0xFFFFFFFF), np.uint64(0x5EED), np.uint64(0)), (k0, k1))
    return (int(x[1]) << 32) | int(x[0])
