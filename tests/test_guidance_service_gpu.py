"""Classifier-free guidance through the service layer on the MI355X: ``GroupedConverter(guidance_scale=, unconditional_prompt=)``."""
import json
import os

import numpy as np
import pytest

from util import procedural_params, rel_l2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grouped_converter_guided_equals_per_segment(diag):
    """three segments of one shape under guidance: batches of two (max_batch 4, halved) == every segment in a guided batch of its own
    (fp32, the item-vs-alone bar of the other service tests); the guidance reaches the latents"""
    import torch
    from ns2vc_amd.frontend import PreModel
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import GroupedConverter, Segment
    from ns2vc_amd.weights import hash_normal, procedural_state_dict
    cfg = {"phoneme_encoder": {"in_channels": 256, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2},
           "prompt_encoder": {"in_channels": 100, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2}}
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "pre_model_state_keys.json")))
    pre = PreModel(cfg).eval()
    pre.load_state_dict(procedural_params(keys["keys"], "pre"), strict=True)
    dev = torch.device("cuda", 0)
    pre = pre.to(dev)
    segs = [Segment(torch.from_numpy(hash_normal(f"gds.c{i}", (256, 96))), torch.from_numpy(hash_normal(f"gds.r{i}", (100, 40))), tag=i) for i in range(3)]
    den = Denoiser(procedural_state_dict(seed=0), precision="fp32")
    u = torch.zeros((1, 3, 256), device=dev)
    kw = dict(solver="unipc", steps=6, guidance_scale=2.0, unconditional_prompt=u)
    conv = GroupedConverter(pre, den, max_batch=4, **kw)
    assert conv.max_batch == 2 and conv.plan(segs) == [[0, 1], [2]]
    out = conv.convert(segs)
    assert den.engine.guidance is not None and den.engine.shape[0] == 2           # (the last batch: one segment, two items)
    single = GroupedConverter(pre, den, max_batch=2, **kw).convert(segs)
    plain = GroupedConverter(pre, den, max_batch=4, solver="unipc", steps=6).convert(segs)
    assert den.engine.guidance is None
    errs = [rel_l2(out[i].cpu().numpy(), single[i].cpu().numpy()) for i in range(3)]
    moved = [rel_l2(out[i].cpu().numpy(), plain[i].cpu().numpy()) for i in range(3)]
    diag(f"guided service unipc6 fp32, batches of 2 vs batches of 1: max {max(errs):.2e}; guided vs unguided: min {min(moved):.2e}")
    for o in out:
        assert o.shape == (100, 96) and torch.isfinite(o).all()
    assert max(errs) < 1e-5
    assert min(moved) > 1e-3
