"""CPU checks of the masked row-chain instantiations (engine option ``masked_rows``, ns2vc_rowchain_args.lens): every dense instantiation has
a masked twin or stands in the launcher's refused list, none of the twins uses scratch or spills a register, each sits in its twin's
waves-per-SIMD bracket; the option is known by name and off by default; the new ABI field closes its struct."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ns2vc_amd", "csrc")

# (dim, stage-2 row blocks per workgroup, 64-token blocks per workgroup) for which the launcher refuses `lens`: rowchain_masks_rows (rowchain.hip)
# and this list say the same thing -- empty: every instantiation has a masked twin inside its twin's resources
REFUSED = []


def _rowchain_kernels():
    """{(operand type, dim, R2, NT, MASKED): {remark: value}} of rowchain.hip, compiled as the Makefile compiles it (the %.hip rule)"""
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-I../../include",
                        "-Rpass-analysis=kernel-resource-usage", "-c", "rowchain.hip", "-o", os.devnull], cwd=SRC, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    out, key = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            k = re.search(r"rowchain_kernelINS_\d(\w+?)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE", m.group(1))
            key = (k.group(1), int(k.group(2)), int(k.group(3)), int(k.group(4)), int(k.group(5))) if k else None
            continue
        m = re.search(r"remark:\s+(VGPRs|AGPRs|ScratchSize \[bytes/lane\]|VGPRs Spill|SGPRs Spill): (\d+)", line)
        if m and key:
            out.setdefault(key, {})[m.group(1)] = int(m.group(2))
    return out


def _waves_per_simd(regs):
    """512 registers per lane and SIMD, allocated in units of 8, at most 8 waves (as tests/test_masked_attn_cpu.py)"""
    return min(8, 512 // ((regs + 7) // 8 * 8))


def test_masked_rowchain_kernels_exist_and_keep_their_resources():
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    ks = _rowchain_kernels()
    dense = {k[:4]: v for k, v in ks.items() if k[4] == 0}
    masked = {k[:4]: v for k, v in ks.items() if k[4] == 1}
    # the dense list itself, as launch_rc_tm selects: both 16-bit types x (dim 128: n2 = dim | 3 dim on 64- and 128-token blocks; dim 256: both n2;
    # dim 384: both n2 whole (3 | 9 row blocks) and as the larger of two slices (2 | 5))
    shapes = {(128, 1, 1), (128, 3, 1), (128, 1, 2), (128, 3, 2), (256, 2, 1), (256, 6, 1), (384, 3, 1), (384, 9, 1), (384, 2, 1), (384, 5, 1)}
    assert {k[1:] for k in dense} == shapes and len(dense) == 2 * len(shapes) and len({k[0] for k in dense}) == 2, sorted(dense)
    # one masked twin per dense instantiation, except what the launcher refuses
    refused = {k for k in dense if k[1:] in REFUSED}
    assert sorted(masked) == sorted(set(dense) - refused), (sorted(masked), sorted(dense))
    for k, v in masked.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (k, v)
        d = dense[k]
        assert d["ScratchSize [bytes/lane]"] == 0 and d["VGPRs Spill"] == 0, (k, d)
        assert _waves_per_simd(v["VGPRs"] + v["AGPRs"]) == _waves_per_simd(d["VGPRs"] + d["AGPRs"]), (k, v, d)


def test_refused_list_is_what_the_launcher_enforces():
    """rowchain_masks_rows refuses on T alone (T < 1, M % T, a prologue under 64 frames): no shape of launch_rc_tm is turned away, as REFUSED says"""
    txt = open(os.path.join(SRC, "rowchain.hip")).read()
    body = re.search(r"bool rowchain_masks_rows\(const RowchainArgs& a, int prec\) \{(.*?)\n\}", txt, re.S).group(1)
    assert "a.T < 1" in body and "a.M % a.T" in body and "a.T >= 64" in body
    assert REFUSED == [] and "a.dim ==" not in body and "a.n2 ==" not in body and "a.slices" not in body
    # refused, never run unmasked: the masked instantiations are the only ones a launch with `lens` can reach
    assert re.search(r"if \(a\.lens\) \{\s*if \(!rowchain_masks_rows\(a, prec\)\) return hipErrorInvalidValue;", txt)


def test_option_known_and_length_field_last():
    txt = open(os.path.join(SRC, "engine.cpp")).read()
    opts = re.search(r"kOptions\[\] = \{(.*?)\};", txt, re.S).group(1)
    assert '{"masked_rows", "NS2VC_MASKED_ROWS", &ns2vc_unet::masked_rows}' in opts
    assert re.search(r"bool masked_rows = false;", open(os.path.join(SRC, "engine_internal.h")).read())      # default off
    hdr = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    body = re.search(r"typedef struct ns2vc_rowchain_args \{(.*?)\} ns2vc_rowchain_args;", hdr, re.S).group(1)
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if d.strip()]
    assert decls[-1] == "const int32_t* lens" and decls[-2] == "int32_t slices"
    assert "NS2VC_ABI_VERSION 7" in hdr and "int ns2vc_sizeof_rowchain_args(void);" in hdr
    assert '"masked_rows" 1|0' in hdr
    from ns2vc_amd import _lib
    assert _lib.ABI_VERSION == 7
    names = [f[0] for f in _lib.RowchainArgs._fields_]
    assert names[-1] == "lens" and names[-2] == "slices"
    # the field sits at the end: everything in front of it keeps its offset, and a zero-filled struct means "no lengths"
    assert _lib.RowchainArgs.lens.offset == (_lib.RowchainArgs.slices.offset + 4 + 7) // 8 * 8
    assert C.sizeof(_lib.RowchainArgs) == _lib.RowchainArgs.lens.offset + 8
    assert not _lib.RowchainArgs().lens


def test_library_reports_rowchain_struct_size():
    """the built library and the binding agree on sizeof(ns2vc_rowchain_args) (a GPU is not needed to load the library)"""
    from ns2vc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    assert lib.ns2vc_sizeof_rowchain_args() == C.sizeof(_lib.RowchainArgs)
    assert lib.ns2vc_abi_version() == 7


def test_python_surface_passes_the_option_on(monkeypatch):
    import inspect
    import recording_engine
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.service import GroupedConverter
    assert inspect.signature(Denoiser.__init__).parameters["masked_rows"].default is False
    assert inspect.signature(GroupedConverter.__init__).parameters["masked_rows"].default is None
    recording_engine.check_masked_option(monkeypatch, "masked_rows")      # the constructor, set_option and the default, on both engines
    assert "--masked-rows" in open(os.path.join(ROOT, "tools", "ragged_bench.py")).read()
