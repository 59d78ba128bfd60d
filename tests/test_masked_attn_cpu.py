"""CPU checks of the masked attention instantiations (engine option ``masked_attn``, ns2vc_attn_args.q_lens / k_lens): every dense
instantiation without the fp8 PV product has a masked twin, none of them uses scratch or spills a register, each sits in its twin's
waves-per-SIMD bracket; the option is known by name and off by default; the new ABI fields close their struct."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ns2vc_amd", "csrc")


def _attn_kernels():
    """{(operand type, head width, key tile, P8, MASKED): {remark: value}} of attn.hip, compiled as the Makefile compiles it (attention keeps its
    MFMA accumulators in VGPRs: the extra -mllvm flag of the attn.o rule)"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I../../include", "-mllvm", "-amdgpu-mfma-vgpr-form",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "attn.hip", "-o", os.devnull], cwd=SRC, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out, key = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"attn_kernelI(\w+?)Li(\d+)ELi(\d+)ELb([01])ELb([01])EE", m.group(1))
            key = (k.group(1), int(k.group(2)), int(k.group(3)), int(k.group(4)), int(k.group(5))) if k else None
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and key:
            out.setdefault(key, {})[m.group(1)] = int(m.group(2))
    return out


def _waves_per_simd(regs):
    """512 registers per lane and SIMD, allocated in units of 8, at most 8 waves (MI355X micro-architecture notes, the VGPR + AGPR table:
    <= 64 -> 8, 72 -> 7, 80 -> 6, 88-96 -> 5, 104-128 -> 4, 136-168 -> 3, 176-256 -> 2, 264-512 -> 1)"""
    return min(8, 512 // ((regs + 7) // 8 * 8))


def test_waves_per_simd_formula():
    for regs, waves in ((64, 8), (72, 7), (80, 6), (88, 5), (96, 5), (104, 4), (124, 4), (128, 4), (136, 3), (168, 3), (176, 2), (256, 2), (264, 1), (512, 1)):
        assert _waves_per_simd(regs) == waves, regs


def test_masked_attention_kernels_exist_and_keep_their_resources():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    ks = _attn_kernels()
    dense = {k[:3]: v for k, v in ks.items() if k[3] == 0 and k[4] == 0}
    masked = {k[:3]: v for k, v in ks.items() if k[4] == 1}
    # the dense list itself: 3 operand types x 4 head widths on 64-key tiles + the 128-key tiles of the two 16-bit types at head width 16 / 32
    assert len(dense) == 3 * 4 + 2 * 2, sorted(dense)
    assert {k[1] for k in dense} == {16, 32, 48, 64} and {k[2] for k in dense} == {64, 128} and len({k[0] for k in dense}) == 3
    # one masked twin per dense instantiation without the fp8 PV product, and no masked fp8 form (refused by the launcher)
    assert sorted(masked) == sorted(dense), (sorted(masked), sorted(dense))
    assert not [k for k in ks if k[3] == 1 and k[4] == 1]
    for k, v in masked.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (k, v)
        d = dense[k]
        assert _waves_per_simd(v["VGPRs"] + v["AGPRs"]) == _waves_per_simd(d["VGPRs"] + d["AGPRs"]), (k, v, d)
    # the hd-16 kernels of the 16-bit types hide their exponentials behind 4 waves per SIMD
    for k, v in masked.items():
        if k[1] == 16 and k[2] == 64 and k[0] != "f":
            assert _waves_per_simd(v["VGPRs"] + v["AGPRs"]) == 4, (k, v)


def test_option_known_and_length_fields_last():
    txt = open(os.path.join(SRC, "engine.cpp")).read()
    opts = re.search(r"kOptions\[\] = \{(.*?)\};", txt, re.S).group(1)
    assert '{"masked_attn", "NS2VC_MASKED_ATTN", &ns2vc_unet::masked_attn}' in opts
    assert re.search(r"bool masked_attn = false;", open(os.path.join(SRC, "engine_internal.h")).read())      # default off
    hdr = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    body = re.search(r"typedef struct ns2vc_attn_args \{(.*?)\} ns2vc_attn_args;", hdr, re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls[-2:] == ["const int32_t* q_lens", "const int32_t* k_lens"] and decls[-3] == "unsigned* fallbacks"
    assert "NS2VC_ABI_VERSION 7" in hdr
    from ns2vc_amd import _lib
    names = [f[0] for f in _lib.AttnArgs._fields_]
    assert names[-2:] == ["q_lens", "k_lens"] and names[-3] == "fallbacks"
    # the fields sit at the end: everything in front of them keeps its offset, and a zero-filled struct means "no lengths"
    assert _lib.AttnArgs.q_lens.offset == _lib.AttnArgs.fallbacks.offset + 8 and _lib.AttnArgs.k_lens.offset == _lib.AttnArgs.q_lens.offset + 8
    assert C.sizeof(_lib.AttnArgs) == _lib.AttnArgs.k_lens.offset + 8
    a = _lib.AttnArgs()
    assert not a.q_lens and not a.k_lens


def test_library_reports_attn_struct_size():
    """the built library and the binding agree on sizeof(ns2vc_attn_args) (a GPU is not needed to load the library)"""
    from ns2vc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.ns2vc_sizeof_attn_args() == C.sizeof(_lib.AttnArgs)


def test_python_surface_passes_the_option_on(monkeypatch):
    import inspect
    import recording_engine
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import GroupedConverter
    assert inspect.signature(Denoiser.__init__).parameters["masked_attn"].default is False
    assert inspect.signature(GroupedConverter.__init__).parameters["masked_attn"].default is None
    recording_engine.check_masked_option(monkeypatch, "masked_attn")      # the constructor, set_option and the default, on both engines
    assert "--masked-attn" in open(os.path.join(ROOT, "tools", "ragged_bench.py")).read()
