"""CPU checks of the masked fused feed-forward instantiations (engine option ``masked_ffn``, ns2vc_ffn_args.lens): every dense instantiation
without the in-kernel cross-attention has exactly one masked twin, none of the twins uses scratch or spills a register, each sits in its twin's
waves-per-SIMD bracket, and the cross-attention form has none; the option is known by name and off by default; the new ABI field closes its struct."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_masked_attn_cpu import _waves_per_simd      # noqa: E402  (one statement of the register table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ns2vc_amd", "csrc")


def _ffn_kernels():
    """{(operand type, dim, PRE, ATT, MASKED): {remark: value}} of ffn.hip, compiled as the Makefile compiles it (the %.hip rule)"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-I../../include",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "ffn.hip", "-o", os.devnull], cwd=SRC, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out, key = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"ffn_kernelINS_\d(\w+?)ELi(\d+)ELb([01])ELb([01])ELb([01])EE", m.group(1))
            key = (k.group(1), int(k.group(2)), int(k.group(3)), int(k.group(4)), int(k.group(5))) if k else None
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and key:
            out.setdefault(key, {})[m.group(1)] = int(m.group(2))
    return out


def test_masked_ffn_kernels_exist_and_keep_their_resources():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    ks = _ffn_kernels()
    dense = {k[:3]: v for k, v in ks.items() if k[3] == 0 and k[4] == 0}
    masked = {k[:3]: v for k, v in ks.items() if k[3] == 0 and k[4] == 1}
    att = [k for k in ks if k[3] == 1]
    # the dense list itself: both 16-bit types x dim 128 | 256 x plain | pre-stage, and the cross-attention form of each (type, dim)
    assert {k[1:] for k in dense} == {(128, 0), (128, 1), (256, 0), (256, 1)} and len(dense) == 8 and len({k[0] for k in dense}) == 2, sorted(dense)
    assert len(att) == 4 and all(k[2] == 1 for k in att), att
    # exactly one masked twin per dense instantiation: 8 in all; the cross-attention form has none
    assert sorted(masked) == sorted(dense) and len(masked) == 8, (sorted(masked), sorted(dense))
    assert not [k for k in att if k[4] == 1], att
    assert len(ks) == 8 + 8 + 4, sorted(ks)
    for k, v in masked.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        d = dense[k]
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0, (k, d)
        assert _waves_per_simd(v["VGPRs"] + v["AGPRs"]) == _waves_per_simd(d["VGPRs"] + d["AGPRs"]), (k, v, d)


def test_option_known_and_length_field_last():
    txt = open(os.path.join(SRC, "engine.cpp")).read()
    opts = re.search(r"kOptions\[\] = \{(.*?)\};", txt, re.S).group(1)
    assert '{"masked_ffn", "NS2VC_MASKED_FFN", &ns2vc_unet::masked_ffn}' in opts
    assert re.search(r"bool masked_ffn = false;", open(os.path.join(SRC, "engine_internal.h")).read())      # default off
    hdr = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    body = re.search(r"typedef struct ns2vc_ffn_args \{(.*?)\} ns2vc_ffn_args;", hdr, re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls[-1] == "const int32_t* lens" and decls[-2] == "int32_t att_Lk"
    assert "NS2VC_ABI_VERSION 7" in hdr and "int ns2vc_sizeof_ffn_args(void);" in hdr
    assert '"masked_ffn" 1|0' in hdr
    from ns2vc_amd import _lib
    assert _lib.ABI_VERSION == 7
    names = [f[0] for f in _lib.FfnArgs._fields_]
    assert names[-1] == "lens" and names[-2] == "att_Lk"
    # the field sits at the end, 8-byte aligned: everything in front of it keeps its offset, and a zero-filled struct means "no lengths"
    assert _lib.FfnArgs.lens.offset == (_lib.FfnArgs.att_Lk.offset + 4 + 7) // 8 * 8 and _lib.FfnArgs.lens.offset % 8 == 0
    assert C.sizeof(_lib.FfnArgs) == _lib.FfnArgs.lens.offset + 8
    assert not _lib.FfnArgs().lens
    assert "ns2vc_sizeof_ffn_args" in _lib.PROTOTYPES


def test_library_reports_ffn_struct_size():
    """the built library and the binding agree on sizeof(ns2vc_ffn_args) (a GPU is not needed to load the library)"""
    from ns2vc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.ns2vc_sizeof_ffn_args() == C.sizeof(_lib.FfnArgs)
    assert lib.ns2vc_abi_version() == 7


def test_python_surface_passes_the_option_on(monkeypatch):
    import inspect
    import recording_engine
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import GroupedConverter
    assert inspect.signature(Denoiser.__init__).parameters["masked_ffn"].default is False
    assert inspect.signature(GroupedConverter.__init__).parameters["masked_ffn"].default is None
    recording_engine.check_masked_option(monkeypatch, "masked_ffn")      # the constructor, set_option and the default, on both engines
    assert "--masked-ffn" in open(os.path.join(ROOT, "tools", "ragged_bench.py")).read()
