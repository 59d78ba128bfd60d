"""The configuration matrix on the CPU: the oracle against the reference's outputs on every configuration of tests/configs.py
(golden_v6, written by tests/golden/make_golden_v6.py), param_spec against the reference's key list, and the engine's acceptance predicate
(``ns2vc_unet_create`` validates before it touches a device) against its plain-Python statement, ``spec.engine_supports``."""
from __future__ import annotations

import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from configs import CONFIGS, ENGINE_REFUSED, GOLDEN_SHAPES, _cfg, golden_inputs
from util import rel_l2

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v6.npz")
ORACLE_TOL = 1e-6       # measured 0.0 (the oracle restates the reference op for op)
# what a config that passes validation meets on a box without a device: the first device call after validation
DEVICE_MESSAGE = "kernel attribute setup failed"


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_matrix_is_accepted_by_both_predicates():
    from ns2vc_amd.spec import engine_supports
    for cid, cfg in CONFIGS.items():
        cfg.validate()
        assert engine_supports(cfg) is None, (cid, engine_supports(cfg))
    for cid, (cfg, field) in ENGINE_REFUSED.items():
        cfg.validate()
        r = engine_supports(cfg)
        assert r is not None and field in r, (cid, r)


@pytest.mark.parametrize("shape_id", sorted(GOLDEN_SHAPES))
@pytest.mark.parametrize("cid", sorted(CONFIGS))
def test_oracle_matches_reference_on_the_matrix(cid, shape_id, gold):
    from ns2vc_amd.weights import procedural_state_dict
    from oracle import unet_ref
    cfg = CONFIGS[cid]
    x, c, p, mask, ts = golden_inputs(cid, shape_id)
    P = {k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg, 0).items()}
    y = unet_ref.unet_forward(P, cfg, torch.cat([torch.from_numpy(x), torch.from_numpy(c)], dim=1), torch.from_numpy(ts),
                              torch.from_numpy(p), torch.from_numpy(mask)).numpy()
    ref = gold[f"{cid}.{shape_id}.y"]
    assert y.shape == ref.shape == (len(ts), cfg.latent_channels, x.shape[-1])
    assert rel_l2(y, ref) <= ORACLE_TOL, (cid, shape_id, rel_l2(y, ref))


@pytest.mark.parametrize("cid", sorted(CONFIGS))
def test_param_spec_matches_reference_keys(cid, gold):
    import hashlib
    from ns2vc_amd.spec import param_spec
    spec = param_spec(CONFIGS[cid])
    s = "\n".join(f"{k}:{','.join(str(int(d)) for d in shape)}" for k, shape in spec.items())
    assert hashlib.sha256(s.encode()).digest() == gold[f"{cid}.keys_sha256"].tobytes(), cid


# ---- the acceptance predicate -----------------------------------------------------------------------------
def _create(cfg, pool_heads=64):
    """ns2vc_unet_create on ``cfg`` (block types are not part of the C ABI): (status, last error)"""
    from ns2vc_amd import _lib
    lib = _lib.load()
    c = _lib.UnetCfg()
    c.latent_channels, c.content_channels = cfg.latent_channels, cfg.content_channels
    c.n_levels = len(cfg.block_out_channels)
    for i, v in enumerate(cfg.block_out_channels[:_lib.MAX_LEVELS]):
        c.block_out_channels[i] = v
    c.norm_num_groups, c.cross_attention_dim, c.heads = cfg.norm_num_groups, cfg.cross_attention_dim, cfg.heads
    c.layers_per_block, c.pool_heads = cfg.layers_per_block, pool_heads
    h = C.c_void_p()
    r = lib.ns2vc_unet_create(C.byref(c), C.byref(h))
    msg = (lib.ns2vc_last_error() or b"").decode()
    if r == 0:
        lib.ns2vc_unet_destroy(h)
    return r, msg


def _grid():
    chans = {2: (128, 256), 4: (128, 256, 384, 512), 8: (128,) * 8}
    out = []
    for heads in (1, 2, 4, 8, 16):
        out.append(("heads", _cfg(heads=heads)))
        out.append(("heads", _cfg(heads=heads, chans=(128, 128, 256, 256))))
    for g in (1, 2, 4, 8, 16):
        out.append(("norm_num_groups", _cfg(groups=g)))
    for lat in (0, 1, 98, 128, 129):
        out.append(("latent_channels", _cfg(latent=lat)))
    for content in (64, 96, 192):
        out.append(("content_channels", _cfg(content=content)))
    for cross in (64, 128, 192, 512, 640):
        out.append(("cross_attention_dim", _cfg(cross=cross)))
    out.append(("block_out_channels", _cfg(chans=(192, 256, 384, 512))))      # c0 != 128
    out.append(("block_out_channels", _cfg(chans=(128, 256, 384, 576))))      # > 512
    out.append(("block_out_channels", _cfg(chans=(128, 256, 352, 512))))      # not a multiple of 64
    for n in (1, 2, 8, 9):
        ch = chans.get(n, (128,) * n)
        out.append(("n_levels", _cfg(chans=ch)))
    for lpb in (0, 1, 3):
        out.append(("layers_per_block", _cfg(lpb=lpb)))
    # two fields off at once: the message names the first the engine checks, whichever it is
    for heads, g in itertools.product((4, 16), (4, 16)):
        out.append(("", _cfg(heads=heads, groups=g)))
    return out


@pytest.mark.parametrize("field,cfg", _grid(), ids=lambda v: v if isinstance(v, str) else None)
def test_create_refuses_exactly_what_engine_supports_refuses(field, cfg):
    """the C predicate and its statement agree on the grid: a refused configuration comes back nonzero with a message that names the
    offending field (the statement's message, word for word); an accepted one gets past validation -- here, on a box without a device,
    to the first device call."""
    from ns2vc_amd.spec import engine_supports
    n = len(cfg.block_out_channels)
    if n > 8:            # the C struct holds 8 levels: the statement must refuse, the C side is given a 9-level count
        assert engine_supports(cfg).startswith("n_levels=9")
    want = engine_supports(cfg)
    r, msg = _create(cfg)
    if want is None:
        assert r == 0 or DEVICE_MESSAGE in msg, (field, msg)
    else:
        assert r != 0 and msg == want, (field, want, msg)
        if field:
            assert msg.startswith(field) or f"{field}[" in msg or f" {field}=" in msg, (field, msg)


@pytest.mark.parametrize("pool_heads", [0, 16, 32, 64])
def test_create_refuses_pool_heads_wider_than_8(pool_heads):
    """cross_attention_dim 256 over 16 pool heads is 16 wide; 0 pool heads must be refused, not divided by"""
    r, msg = _create(_cfg(), pool_heads=pool_heads)
    if pool_heads < 32:
        assert r != 0 and "pool_heads" in msg and "cross_attention_dim" in msg, msg
    else:
        assert r == 0 or DEVICE_MESSAGE in msg, msg


@pytest.mark.parametrize("field,value", [("heads", 0), ("norm_num_groups", 0), ("norm_num_groups", -8), ("content_channels", 0),
                                         ("cross_attention_dim", 0), ("latent_channels", -1)])
def test_create_range_checks_before_it_divides(field, value):
    """a zero divisor used to reach `c % heads` / `c % norm_num_groups` before any range check (SIGFPE in the caller's process)"""
    from ns2vc_amd import _lib
    lib = _lib.load()
    c = _lib.UnetCfg()
    c.latent_channels, c.content_channels, c.n_levels = 100, 256, 4
    for i, v in enumerate((128, 256, 384, 512)):
        c.block_out_channels[i] = v
    c.norm_num_groups, c.cross_attention_dim, c.heads, c.layers_per_block, c.pool_heads = 8, 256, 8, 2, 64
    setattr(c, field, value)
    h = C.c_void_p()
    assert lib.ns2vc_unet_create(C.byref(c), C.byref(h)) != 0
    assert lib.ns2vc_last_error().decode().startswith(field)


def test_engine_refuses_block_types_it_does_not_build():
    """the C ABI carries no block types; the engine builds cross-attention at every level but the deepest and refuses anything else
    before it reaches the library"""
    from ns2vc_amd.engine import Engine
    from ns2vc_amd.spec import UNetConfig
    cfg = UNetConfig(down_block_types=("CrossAttnDownBlock2D",) * 4, up_block_types=("CrossAttnUpBlock2D",) * 4)
    cfg.validate()
    with pytest.raises(ValueError, match="block_types"):
        Engine(cfg, precision="fp32")
