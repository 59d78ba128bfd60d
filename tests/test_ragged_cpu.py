"""Per-item valid lengths (length-masked batches), the parts that need no GPU: the level-length table, the ragged batch planner of
the service, the C ABI declaration and binding, the padded front end, the resources of the new kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_item_level_lengths_match_spec_per_item():
    from ns2vc_amd.spec import item_level_lengths, level_lengths
    lens = [938, 937, 700, 263, 131, 129, 127, 125, 3, 2, 1]
    tab = item_level_lengths(lens, 938, 4)
    assert len(tab) == 4 and all(len(row) == len(lens) for row in tab)
    for b, L in enumerate(lens):
        assert [tab[l][b] for l in range(4)] == level_lengths(L, 4)
    assert [tab[l][-1] for l in range(4)] == [1, 1, 1, 1]          # a one-frame item stays one frame deep down
    assert [tab[l][0] for l in range(4)] == level_lengths(938, 4)
    for bad in ([0], [939], [-1]):
        with pytest.raises(ValueError):
            item_level_lengths(bad, 938, 4)


def _segs(lengths, rlens):
    import torch
    from ns2vc_amd.service import Segment
    return [Segment(torch.zeros(256, T), torch.zeros(100, L), tag=i) for i, (T, L) in enumerate(zip(lengths, rlens))]


def test_grouped_converter_ragged_plan():
    from ns2vc_amd.service import GroupedConverter
    lengths = [96, 130, 97, 64, 131, 96, 500, 80]
    rlens = [40, 64, 40, 64, 64, 40, 40, 50]
    segs = _segs(lengths, rlens)
    g = GroupedConverter(None, None, max_batch=3, ragged=True).plan(segs)
    # by prompt length only (largest first), longest segment first inside a group (stable), at most max_batch per batch
    assert g == [[4, 1, 3], [7], [6, 2, 0], [5]]
    for batch in g:
        assert len({int(segs[i].refer.shape[-1]) for i in batch}) == 1
        assert [int(segs[i].content.shape[-1]) for i in batch] == sorted((int(segs[i].content.shape[-1]) for i in batch), reverse=True)
    assert sorted(i for b in g for i in b) == list(range(len(segs)))
    # the default mode is unchanged: exact (T, Lp) groups
    assert GroupedConverter(None, None, max_batch=3).plan(segs) == [[6], [4], [1], [2], [0, 5], [7], [3]]


def test_set_lengths_declared_and_bound():
    from ns2vc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    assert re.search(r"int ns2vc_unet_set_lengths\(ns2vc_unet\* h, const int32_t\* lengths_b, void\* stream\);", hdr)
    assert "#define NS2VC_ABI_VERSION 7" in hdr
    assert "ns2vc_unet_set_lengths" in _lib.PROTOTYPES
    lib = _lib.load()
    assert hasattr(lib, "ns2vc_unet_set_lengths")
    assert lib.ns2vc_unet_set_lengths(None, None, None) != 0         # a null handle is an error, not a crash
    assert b"null engine handle" in lib.ns2vc_last_error()


def test_engine_set_lengths_validates_on_the_host():
    from ns2vc_amd.engine import Engine
    e = Engine.__new__(Engine)       # (no device: only the argument check in front of the C call)
    e.shape = (3, 100, 20)
    with pytest.raises(ValueError):
        e.set_lengths([100, 50])


def test_padded_front_end_equals_segments_alone():
    """PreModel.infer(exact_lengths=True) on a zero-padded batch gives, on each segment's frames, what the segment gives alone (the
    default, the reference's batched arithmetic, lets LayerNorm(0) of the padding into the k = 9 conv halo of a segment's last frames)"""
    import json
    import torch
    from ns2vc_amd.frontend import PreModel
    from ns2vc_amd.weights import hash_normal
    from util import procedural_params, rel_l2
    cfg = {"phoneme_encoder": {"in_channels": 256, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2},
           "prompt_encoder": {"in_channels": 100, "hidden_channels": 256, "out_channels": 256, "n_layers": 6, "p_dropout": 0.2}}
    keys = json.load(open(os.path.join(ROOT, "tests", "golden", "pre_model_state_keys.json")))
    m = PreModel(cfg).eval()
    m.load_state_dict(procedural_params(keys["keys"], "pre"), strict=True)
    lens, Lp = [70, 53, 9, 1], 24
    T = max(lens)
    refer = torch.from_numpy(hash_normal("rg.refer", (1, 100, Lp))).expand(len(lens), -1, -1).contiguous()
    c = torch.zeros(len(lens), 256, T)
    segs = [torch.from_numpy(hash_normal(f"rg.c{b}", (256, L))) for b, L in enumerate(lens)]
    for b, s in enumerate(segs):
        c[b, :, :lens[b]] = s
    with torch.no_grad():
        content, prompt, _ = m.infer(c, refer, torch.tensor(lens), torch.full((len(lens),), Lp), exact_lengths=True)
        for b, L in enumerate(lens):
            c1, p1, _ = m.infer(segs[b][None], refer[:1], torch.tensor([L]), torch.tensor([Lp]))
            assert rel_l2(content[b, :, :L].numpy(), c1[0].numpy()) < 1e-5, b
            assert rel_l2(prompt[b].numpy(), p1[0].numpy()) < 1e-5, b
            assert float(content[b, :, L:].abs().max() if L < T else 0.0) == 0.0


def test_masked_kernels_use_no_scratch():
    """the masked GroupNorm-apply instantiation and the row-mask kernel (misc.hip) spill nothing: same hipcc remarks check as the conv kernels"""
    import shutil
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    src = os.path.join(ROOT, "ns2vc_amd", "csrc")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I../../include", "-Rpass-analysis=kernel-resource-usage", "-c", "misc.hip",
                        "-o", os.devnull], cwd=src, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen, bad = None, set(), []
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and name and ("gn_apply_kernel" in name or "mask_rows_kernel" in name):
            seen.add(name)
            if int(m.group(2)) != 0:
                bad.append((name, m.group(1), int(m.group(2))))
    assert any("mask_rows_kernel" in n for n in seen)
    assert sum(1 for n in seen if "gn_apply_kernel" in n) == 6        # 3 operand types x (dense, masked)
    assert not bad, bad
