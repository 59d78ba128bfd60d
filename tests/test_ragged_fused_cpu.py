"""CPU checks of the masked kernel instantiations (engine option ``masked_fuse``): no scratch and no spilled register in the masked forms of
the tap-sharing conv kernel and the 8-wave GEMM kernel, the option known by name, the new ABI field at the end of its struct.

The token-local kernels (rowchain.hip, ffn.hip, geglu.hip) and attn.hip have no masked instantiation in this change: the plan keeps their
unfused launches under the option (README), so there is nothing of theirs to audit here."""
import ctypes as C
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ns2vc_amd", "csrc")


def _remarks(name):
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I../../include", "-Rpass-analysis=kernel-resource-usage", "-c", name,
                        "-o", os.devnull], cwd=SRC, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out, fn = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            fn = m.group(1)
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill): (\d+)", line)
        if m and fn:
            out.setdefault(fn, {})[m.group(1)] = int(m.group(2))
    return out


def test_masked_conv_and_gemm_kernels_use_no_scratch():
    """MASKED is the last template argument of gemm4_kernel: the mangled names of its instantiations end in ...Lb1EEEv"""
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    with ThreadPoolExecutor(2) as ex:
        conv, gemm = ex.map(_remarks, ["convts.hip", "gemm.hip"])
    # (conv3ts_kernel carries the flag as GNP + 4: <TM, BN, NL = 8, GNP = 4 | 5 | 7, KS = false, SOL = false>)
    masked_conv = {k: v for k, v in conv.items() if "conv3ts_kernel" in k and re.search(r"Li8ELi[457]ELb0ELb0EE+v", k)}
    masked_gemm = {k: v for k, v in gemm.items() if "gemm4_kernel" in k and re.search(r"Lb1EE+v", k)}
    # conv: 3 operand types x 2 column tiles x (no prologue, prologue) + 2 sixteen-bit types x 2 tiles with the hi + lo pair prologue
    assert len(masked_conv) == 16, sorted(masked_conv)
    # gemm4: 3 operand types x (4 plain tiles + 2 loader / consumer tiles)
    assert len(masked_gemm) == 18, sorted(masked_gemm)
    bad = [(k, v) for k, v in list(masked_conv.items()) + list(masked_gemm.items())
           if v.get("ScratchSize [bytes/lane]", -1) != 0 or v.get("VGPRs Spill", -1) != 0]
    assert not bad, bad


def test_option_known_and_lens_field_last():
    txt = open(os.path.join(SRC, "engine.cpp")).read()
    opts = re.search(r"kOptions\[\] = \{(.*?)\};", txt, re.S).group(1)
    assert '{"masked_fuse", "NS2VC_MASKED_FUSE", &ns2vc_unet::masked_fuse}' in opts
    assert re.search(r"bool masked_fuse = false;", open(os.path.join(SRC, "engine_internal.h")).read())      # default off
    hdr = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    body = re.search(r"typedef struct ns2vc_gemm_args \{(.*?)\} ns2vc_gemm_args;", hdr, re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls[-1] == "const int32_t* lens" and decls[-2] == "int32_t gnp_pair, sol_op_pair"
    from ns2vc_amd import _lib
    names = [f[0] for f in _lib.GemmArgs._fields_]
    assert names[-1] == "lens" and names[-3:-1] == ["gnp_pair", "sol_op_pair"]
    # the field sits at the end: everything in front of it keeps its offset, and a zero-filled struct means "no lengths"
    assert _lib.GemmArgs.lens.offset == _lib.GemmArgs.sol_op_pair.offset + 4 + (-(_lib.GemmArgs.sol_op_pair.offset + 4) % 8)
    assert C.sizeof(_lib.GemmArgs) == _lib.GemmArgs.lens.offset + 8
    assert not _lib.GemmArgs().lens


def test_library_reports_struct_size():
    """the built library and the binding agree on sizeof(ns2vc_gemm_args) (a GPU is not needed to load the library)"""
    from ns2vc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    src = os.path.join(SRC, "abi_kernels.cpp")
    assert "ns2vc_sizeof_gemm_args" in open(src).read()
    lib = _lib.load()
    assert lib.ns2vc_sizeof_gemm_args() == C.sizeof(_lib.GemmArgs)


def test_python_surface_passes_the_option_on(monkeypatch):
    import recording_engine
    recording_engine.check_masked_option(monkeypatch, "masked_fuse")
