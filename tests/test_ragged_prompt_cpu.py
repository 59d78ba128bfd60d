"""Per-item prompt lengths (ragged prompts), the parts that need no GPU: the padded front end, the service's batch planner, the length
validation in front of the C call, the C ABI declaration and binding, the resources of the new kernels."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRE_CFG = {"phoneme_encoder": {"in_channels": 256, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2},
           "prompt_encoder": {"in_channels": 100, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2}}


@pytest.fixture(scope="module")
def pre_model():
    from ns2vc_amd.frontend import PreModel
    from util import procedural_params
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "pre_model_state_keys.json")))
    m = PreModel(PRE_CFG).eval()
    m.load_state_dict(procedural_params(keys["keys"], "pre"), strict=True)
    return m


def _padded_job():
    """four segments with four reference clips of their own: latent lengths and prompt lengths both ragged (a clip of one frame, clips shorter
    and longer than the k = 9 conv's halo), zero-padded to the batch's longest"""
    import torch
    from ns2vc_amd.weights import hash_normal
    lens, plens = [70, 53, 9, 1], [24, 13, 3, 1]
    T, Lp = max(lens), max(plens)
    segs = [torch.from_numpy(hash_normal(f"rp.c{b}", (256, L))) for b, L in enumerate(lens)]
    clips = [torch.from_numpy(hash_normal(f"rp.r{b}", (100, P))) for b, P in enumerate(plens)]
    c, refer = torch.zeros(len(lens), 256, T), torch.zeros(len(lens), 100, Lp)
    for b in range(len(lens)):
        c[b, :, :lens[b]] = segs[b]
        refer[b, :, :plens[b]] = clips[b]
    return lens, plens, segs, clips, c, refer


def test_padded_prompts_equal_clips_alone(pre_model):
    """PreModel.infer(exact_prompt_lengths=True) on a batch whose reference clips are zero-padded to one Lp gives per item what the item gives
    alone with its own clip: the prompt rows, the content (which the pooled ``ref_enc`` vector enters through spk_proj) and that vector."""
    import torch
    from util import rel_l2
    lens, plens, segs, clips, c, refer = _padded_job()
    T, Lp = max(lens), max(plens)
    m = pre_model
    with torch.no_grad():
        content, prompt, mask = m.infer(c, refer, torch.tensor(lens), torch.tensor(plens), exact_lengths=True, exact_prompt_lengths=True)
        g = m.ref_enc(refer.transpose(1, 2), torch.tensor(plens))
        for b, (L, P) in enumerate(zip(lens, plens)):
            c1, p1, m1 = m.infer(segs[b][None], clips[b][None], torch.tensor([L]), torch.tensor([P]))
            g1 = m.ref_enc(clips[b][None].transpose(1, 2))
            assert rel_l2(prompt[b, :P].numpy(), p1[0].numpy()) < 1e-5, b
            assert rel_l2(content[b, :, :L].numpy(), c1[0].numpy()) < 1e-5, b
            assert rel_l2(g[b].numpy(), g1[0].numpy()) < 1e-5, b
            assert float(prompt[b, P:].abs().max() if P < Lp else 0.0) == 0.0
            assert float(content[b, :, L:].abs().max() if L < T else 0.0) == 0.0
            assert mask[b].tolist() == [t < P for t in range(Lp)] and bool(m1.all())
        # the gap the flag closes: the reference's batched arithmetic pools ref_enc over the padding too
        content0, _, _ = m.infer(c, refer, torch.tensor(lens), torch.tensor(plens), exact_lengths=True)
        c1, _, _ = m.infer(segs[1][None], clips[1][None], torch.tensor([lens[1]]), torch.tensor([plens[1]]))
        assert rel_l2(content0[1, :, :lens[1]].numpy(), c1[0].numpy()) > 1e-3


def test_pooling_with_lengths_ignores_what_the_padding_holds():
    """TextTimeEmbedding / AttentionPooling(lengths=): NaN in the frames past an item's length reaches nothing, full lengths give the unmasked
    result to rounding, and the default call is the arithmetic it was"""
    import torch
    from unet1d.embeddings import TextTimeEmbedding
    from util import rel_l2, tte_state
    tte = TextTimeEmbedding(100, 100, 1).eval()
    tte.load_state_dict(tte_state("rp.tte.", 100, 100))
    from ns2vc_amd.weights import hash_normal
    x = torch.from_numpy(hash_normal("rp.tte.x", (3, 12, 100)))
    lens = torch.tensor([12, 5, 1])
    with torch.no_grad():
        full = tte(x)
        assert rel_l2(tte(x, torch.tensor([12, 12, 12])).numpy(), full.numpy()) < 1e-6
        xn = x.clone()
        for b, L in enumerate(lens.tolist()):
            xn[b, L:] = float("nan")
        # (LayerNorm of a NaN frame is a NaN frame: the pooling itself must drop it)
        y = tte.norm2(tte.proj(tte.pool(tte.norm1(xn), lens)))
        assert torch.isfinite(y).all()
        for b, L in enumerate(lens.tolist()):
            assert rel_l2(y[b].numpy(), tte(x[b:b + 1, :L])[0].numpy()) < 1e-5, b


def test_default_front_end_is_bit_identical(pre_model):
    """without the flag PreModel.infer computes what it computed: the same bits as the un-flagged arithmetic restated here"""
    import torch
    lens, plens, _, _, c, refer = _padded_job()
    m = pre_model
    with torch.no_grad():
        content, prompt, mask = m.infer(c, refer, torch.tensor(lens), torch.tensor(plens))
        e_content, e_prompt, _ = m.infer(c, refer, torch.tensor(lens), torch.tensor(plens), exact_lengths=False, exact_prompt_lengths=False)
        g = m.ref_enc.norm2(m.ref_enc.proj(m.ref_enc.pool(m.ref_enc.norm1(refer.transpose(1, 2))))).unsqueeze(-1)
        r_prompt = m.prompt_encoder(refer, torch.tensor(plens))
        r_content = m.phoneme_encoder(c, torch.tensor(lens), g, False).transpose(1, 2)
    assert torch.equal(content, r_content.float().contiguous()) and torch.equal(prompt, r_prompt.float().contiguous())
    assert torch.equal(content, e_content) and torch.equal(prompt, e_prompt)
    assert mask.tolist() == [[t < P for t in range(max(plens))] for P in plens]


def _segs(lengths, rlens):
    import torch
    from ns2vc_amd.service import Segment
    return [Segment(torch.zeros(256, T), torch.zeros(100, L), tag=i) for i, (T, L) in enumerate(zip(lengths, rlens))]


def test_grouped_converter_plan_with_ragged_prompts():
    from ns2vc_amd.service import GroupedConverter
    lengths = [96, 130, 97, 64, 131, 96, 500, 80]
    rlens = [40, 64, 40, 64, 64, 40, 40, 50]
    segs = _segs(lengths, rlens)
    # the flag off: exactly today's plans, in both modes (the figures of tests/test_ragged_cpu.py)
    assert GroupedConverter(None, None, max_batch=3, ragged=True).plan(segs) == [[4, 1, 3], [7], [6, 2, 0], [5]]
    assert GroupedConverter(None, None, max_batch=3, ragged=True, ragged_prompts=False).plan(segs) == [[4, 1, 3], [7], [6, 2, 0], [5]]
    assert GroupedConverter(None, None, max_batch=3).plan(segs) == [[6], [4], [1], [2], [0, 5], [7], [3]]
    # ragged + ragged_prompts: all segments longest first (stable), cut into batches: 3 batches instead of 4, and prompt lengths mix
    g = GroupedConverter(None, None, max_batch=3, ragged=True, ragged_prompts=True).plan(segs)
    assert g == [[6, 4, 1], [2, 0, 5], [7, 3]]
    assert len({int(segs[i].refer.shape[-1]) for i in g[0]}) == 2
    # default mode + ragged_prompts: by T only, longest first, input order inside
    g = GroupedConverter(None, None, max_batch=3, ragged_prompts=True).plan(segs)
    assert g == [[6], [4], [1], [2], [0, 5], [7], [3]]          # (T = 96: segments 0 and 5 shared a prompt length anyway)
    segs2 = _segs([96, 96, 96, 64], [40, 64, 50, 64])
    assert GroupedConverter(None, None, max_batch=4).plan(segs2) == [[1], [2], [0], [3]]
    assert GroupedConverter(None, None, max_batch=4, ragged_prompts=True).plan(segs2) == [[0, 1, 2], [3]]
    assert sorted(i for b in g for i in b) == list(range(len(segs)))


def test_engine_set_prompt_lengths_validates_on_the_host():
    from ns2vc_amd.engine import Engine
    e = Engine.__new__(Engine)       # (no device: only the argument check in front of the C call)
    e.shape = (3, 100, 20)
    with pytest.raises(ValueError):
        e.set_prompt_lengths([20, 5])                  # a wrong count
    with pytest.raises(ValueError):
        e.set_prompt_lengths([20, 5, 3, 1])
    e.shape = None
    with pytest.raises(ValueError):
        e.set_prompt_lengths([20, 5, 3])               # nothing prepared: no batch to count against


def test_set_prompt_lengths_declared_and_bound():
    from ns2vc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    assert re.search(r"int ns2vc_unet_set_prompt_lengths\(ns2vc_unet\* h, const int32_t\* plens_b, void\* stream\);", hdr)
    assert re.search(r"int ns2vc_unet_graph_captures\(ns2vc_unet\* h, unsigned long long\* count\);", hdr)
    assert "#define NS2VC_ABI_VERSION 7" in hdr
    assert "ns2vc_unet_set_prompt_lengths" in _lib.PROTOTYPES and "ns2vc_unet_graph_captures" in _lib.PROTOTYPES
    lib = _lib.load()
    assert hasattr(lib, "ns2vc_unet_set_prompt_lengths")
    assert lib.ns2vc_unet_set_prompt_lengths(None, None, None) != 0         # a null handle is an error, not a crash
    assert b"null engine handle" in lib.ns2vc_last_error()
    assert lib.ns2vc_unet_graph_captures(None, None) != 0


def test_prompt_length_kernels_use_no_scratch():
    """the two pooling kernels' forms under prompt lengths and the bias-row kernel (misc.hip) spill nothing, and the dense forms they stand
    beside are still there: same hipcc remarks check as the conv kernels"""
    import shutil
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    src = os.path.join(ROOT, "ns2vc_amd", "csrc")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I../../include", "-Rpass-analysis=kernel-resource-usage", "-c", "misc.hip",
                        "-o", os.devnull], cwd=src, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    want = ("pool_cls_kernel", "pool_cls_lens_kernel", "pool_attn_kernel", "pool_attn_lens_kernel", "prompt_bias_kernel", "mask_bias_kernel")
    name, seen, bad = None, {}, []
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name:
            for w in want:
                if re.search(r"\d" + w + r"[A-Z]", name):       # (the mangled name: <length><name><parameter codes>)
                    seen.setdefault(w, set()).add(m.group(1))
                    if int(m.group(2)) != 0:
                        bad.append((name, m.group(1), int(m.group(2))))
    assert sorted(seen) == sorted(want), sorted(seen)
    assert all(v == {"ScratchSize [bytes/lane]", "VGPRs Spill"} for v in seen.values()), seen
    assert not bad, bad
