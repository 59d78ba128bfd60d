"""CPU checks of the masked token-stationary GEGLU instantiations (engine option ``masked_geglu``, ns2vc_geglu_args.T / lens): each of the two dense
instantiations has exactly one masked twin, none of the four uses scratch or spills a register, each twin sits in its dense twin's waves-per-SIMD
bracket; the option is known by name and off by default; the two new ABI fields close their struct; the Python layers pass the option on."""
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


def _geglu_kernels():
    """{(operand type, dim, MASKED): {remark: value}} of geglu.hip, compiled as the Makefile compiles it (the %.hip rule)"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-I../../include",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "geglu.hip", "-o", os.devnull], cwd=SRC, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out, key = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"geglu_kernelINS_\d(\w+?)ELi(\d+)ELb([01])EE", m.group(1))
            key = (k.group(1), int(k.group(2)), int(k.group(3))) if k else None
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and key:
            out.setdefault(key, {})[m.group(1)] = int(m.group(2))
    return out


def test_masked_geglu_kernels_exist_and_keep_their_resources():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    ks = _geglu_kernels()
    dense = {k[:2]: v for k, v in ks.items() if k[2] == 0}
    masked = {k[:2]: v for k, v in ks.items() if k[2] == 1}
    # exactly two dense instantiations (both 16-bit types, dim 384) and one masked twin of each: four kernels in all
    assert len(dense) == 2 and {k[1] for k in dense} == {384} and len({k[0] for k in dense}) == 2, sorted(ks)
    assert sorted(masked) == sorted(dense) and len(ks) == 4, sorted(ks)
    for k, v in masked.items():
        d = dense[k]
        for w in (v, d):
            assert w["ScratchSize [bytes/lane]"] == 0 and w["VGPRs Spill"] == 0 and w["SGPRs Spill"] == 0, (k, w)
        assert _waves_per_simd(v["VGPRs"] + v["AGPRs"]) == _waves_per_simd(d["VGPRs"] + d["AGPRs"]), (k, v, d)


def test_option_known_and_length_fields_last():
    txt = open(os.path.join(SRC, "engine.cpp")).read()
    opts = re.search(r"kOptions\[\] = \{(.*?)\};", txt, re.S).group(1)
    assert '{"masked_geglu", "NS2VC_MASKED_GEGLU", &ns2vc_unet::masked_geglu}' in opts
    assert re.search(r"bool masked_geglu = false;", open(os.path.join(SRC, "engine_internal.h")).read())      # default off
    hdr = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    body = re.search(r"typedef struct ns2vc_geglu_args \{(.*?)\} ns2vc_geglu_args;", hdr, re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls[-1] == "const int32_t* lens" and decls[-2] == "int32_t T" and decls[-3] == "unsigned* ln_health"
    assert "NS2VC_ABI_VERSION 7" in hdr and "int ns2vc_sizeof_geglu_args(void);" in hdr
    assert '"masked_geglu" 1|0' in hdr
    assert "bool geglu_masks_rows(const ::ns2vc_geglu_args& a, int prec);" in open(os.path.join(SRC, "common.h")).read()
    from ns2vc_amd import _lib
    assert _lib.ABI_VERSION == 7
    names = [f[0] for f in _lib.GegluArgs._fields_]
    assert names[-2:] == ["T", "lens"] and names[-3] == "ln_health"
    # the fields sit at the end: everything in front of them keeps its offset, and a zero-filled struct means "no lengths"
    assert _lib.GegluArgs.T.offset == _lib.GegluArgs.ln_health.offset + 8
    assert _lib.GegluArgs.lens.offset == _lib.GegluArgs.T.offset + 8 and _lib.GegluArgs.lens.offset % 8 == 0
    assert C.sizeof(_lib.GegluArgs) == _lib.GegluArgs.lens.offset + 8
    z = _lib.GegluArgs()
    assert not z.lens and z.T == 0
    assert "ns2vc_sizeof_geglu_args" in _lib.PROTOTYPES


def test_library_reports_geglu_struct_size():
    """the built library and the binding agree on sizeof(ns2vc_geglu_args) (a GPU is not needed to load the library)"""
    from ns2vc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.ns2vc_sizeof_geglu_args() == C.sizeof(_lib.GegluArgs)
    assert lib.ns2vc_abi_version() == 7


def test_python_surface_passes_the_option_on(monkeypatch):
    import inspect
    import recording_engine
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import GroupedConverter
    assert inspect.signature(Denoiser.__init__).parameters["masked_geglu"].default is False
    assert inspect.signature(GroupedConverter.__init__).parameters["masked_geglu"].default is None
    recording_engine.check_masked_option(monkeypatch, "masked_geglu")      # the constructor, set_option and the default, on both engines
    assert "--masked-geglu" in open(os.path.join(ROOT, "tools", "ragged_bench.py")).read()
