"""The non-default UNet configurations the engine accepts, shared by tests/golden/make_golden_v6.py, tests/test_configs_cpu.py and
tests/test_configs_gpu.py.  Each entry passes both ``UNetConfig.validate()`` and ``ns2vc_unet_create``; the comment names the engine path it
reaches that the stock ``UNetConfig()`` never does."""
from __future__ import annotations

from ns2vc_amd.spec import UNetConfig, engine_block_types


def _cfg(latent=100, content=256, cross=256, chans=(128, 256, 384, 512), groups=8, heads=8, lpb=2) -> UNetConfig:
    down, up = engine_block_types(len(chans))
    return UNetConfig(in_channels=latent + content, out_channels=latent, block_out_channels=tuple(chans), norm_num_groups=groups,
                      cross_attention_dim=cross, attention_head_dim=heads, layers_per_block=lpb, down_block_types=down, up_block_types=up)


CONFIGS = {
    # config.json out_channels 80, hidden_channels 384: pad lanes 80..127, pool head width 6, conv_in K 1152
    "mel80_h384": _cfg(latent=80, content=384, cross=384),
    # a partial Philox channel quad (98 % 4 = 2), pool head width 2, to_k / to_v K 128
    "lat98_h128": _cfg(latent=98, content=128, cross=128),
    # no pad lanes at all, pool head width 8, conv_in K 1536
    "lat128_h512": _cfg(latent=128, content=512, cross=512),
    # content != cross, a conv_in K (576) that is not a multiple of 128
    "content192": _cfg(content=192),
    # a 2-deep skip stack per level, 4 groups: group widths 32 .. 128 (the 256 + 256 concat).  (The stock channels with 4 groups are refused:
    # the 512 + 512 concat would need 256-wide groups, ENGINE_REFUSED)
    "lpb1_g4": _cfg(chans=(128, 256, 256, 256), lpb=1, groups=4),
    # a level without a shortcut conv (256 -> 256), 256 + 256 concats, 4 skips per level
    "lpb3_rep": _cfg(chans=(128, 256, 256, 512), lpb=3),
    # 4 heads (no fused cross-attention; head widths 32 / 32 / 64 / 64), 128 + 256 concats.  (Widths that are not multiples of 128, such as
    # 192, are refused: the transformer's LayerNorm kernels take rows of 128k channels, ENGINE_REFUSED; the explicit-LayerNorm path is
    # reached through the ln_linear option in test_every_plan_option)
    "h4_w256": _cfg(chans=(128, 128, 256, 256), heads=4),
    # 3 levels (Engine / Denoiser only: the drop-in ctor fixes 4 levels)
    "lv3": _cfg(chans=(128, 256, 512)),
    # 2 levels, shortest T 2
    "lv2": _cfg(chans=(128, 256)),
}

# the reference ctor kwargs of a configuration (model.py:391-400 with config.json's diffusion_encoder widths)
def ctor_kwargs(cfg: UNetConfig) -> dict:
    return dict(in_channels=cfg.in_channels, out_channels=cfg.out_channels, block_out_channels=cfg.block_out_channels,
                layers_per_block=cfg.layers_per_block, norm_num_groups=cfg.norm_num_groups, cross_attention_dim=cfg.cross_attention_dim,
                attention_head_dim=cfg.attention_head_dim, addition_embed_type="text", resnet_time_scale_shift="scale_shift",
                down_block_types=cfg.down_block_types, up_block_types=cfg.up_block_types)


# validate() accepts these, the engine does not (the field its message must name)
ENGINE_REFUSED = {
    "heads4_stock": (_cfg(heads=4), "heads"),                  # head width 96 at 384 channels
    "cross192": (_cfg(cross=192), "cross_attention_dim"),
    "groups4_stock": (_cfg(groups=4), "norm_num_groups"),     # the up block's 512 + 512 concat in 4 groups of 256
    "width192": (_cfg(chans=(128, 128, 192, 256), heads=4), "block_out_channels"),   # a transformer width that is not a multiple of 128
}

# the golden_v6 shapes: (B, T, prompt length, valid prompt keys per item, timesteps); T odd and not a multiple of 2^(levels-1)
GOLDEN_SHAPES = {"b2": (2, 37, 21, (21, 13), (999.0, 500.5)), "b3": (3, 11, 9, (9, 4, 1), (999.0, 500.5, 3.0))}


def golden_inputs(cfg_id: str, shape_id: str):
    """(sample = cat[x, content], timesteps, prompt, mask) as numpy, drawn with hash_normal"""
    import numpy as np
    from ns2vc_amd.weights import hash_normal
    cfg = CONFIGS[cfg_id]
    B, T, Lp, lens, ts = GOLDEN_SHAPES[shape_id]
    tag = f"v6.{cfg_id}.{shape_id}"
    x = hash_normal(f"{tag}.x", (B, cfg.latent_channels, T))
    c = hash_normal(f"{tag}.content", (B, cfg.content_channels, T))
    p = hash_normal(f"{tag}.prompt", (B, Lp, cfg.cross_attention_dim))
    mask = np.arange(Lp)[None, :] < np.array(lens)[:, None]
    return x, c, p, mask, np.array(ts, dtype=np.float32)
