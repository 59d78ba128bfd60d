"""CPU checks of the K/V-resident attention kernel's plumbing (csrc/attn_resident.hip): its table's rows are exactly the compiled attnres_kernel
instantiations (the method of tests/test_kernel_tables_cpu.py, for the one table that is not a family of ns2vc_debug_kernel_table), the header
declares and the library exports its hooks, and neither the ABI version nor ns2vc_attn_args moved."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ns2vc_amd", "csrc")
HOOKS = ("ns2vc_debug_set_attn_resident", "ns2vc_debug_attnres_table", "ns2vc_debug_attn_resident_launches")
ROWS = 4                 # fp16 / bf16 x hd 16 / 32
ATTN_ARGS_BYTES = 120    # sizeof(ns2vc_attn_args) of ABI v7, as the library before this kernel reports it


def _lib():
    from ns2vc_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        pytest.skip("library not built")
    return L, L.load()


def test_table_rows_are_the_compiled_instantiations():
    _, lib = _lib()
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-I../../include", "-mllvm",
                        "-amdgpu-mfma-vgpr-form", "--offload-device-only", "-S", "attn_resident.hip", "-o", "-"], cwd=SRC, capture_output=True, text=True,
                       timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    syms = [s for s in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", r.stdout, re.M) if re.match(r"_ZN5ns2vc\d+attnres_kernelI", s)]
    rows = C.c_int(-1)
    assert lib.ns2vc_debug_attnres_table(C.byref(rows)) == 0          # (no HIP call: works without a device)
    assert len(set(syms)) == len(syms) == rows.value == ROWS, (syms, rows.value)
    assert not re.search(r"\.amdhsa_kernel\s+_ZN5ns2vc\d+attn_kernelI", r.stdout)      # the tiled template is instantiated in attn.hip alone
    assert lib.ns2vc_debug_attnres_table(None) != 0
    # every instantiation keeps 4 waves per SIMD at 1024 threads (<= 128 VGPRs) and uses no scratch
    for name, body in re.findall(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", r.stdout, re.S):
        if name in syms:
            assert int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1)) <= 128, name
            assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0, name


def test_hooks_are_declared_bound_and_exported():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    for name in HOOKS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in L.PROTOTYPES and getattr(lib, name) is not None, name
    assert lib.ns2vc_debug_set_attn_resident(2) != 0 and lib.ns2vc_debug_set_attn_resident(-2) != 0
    for mode in (0, 1, -1):
        assert lib.ns2vc_debug_set_attn_resident(mode) == 0
    rows = C.c_int(-1)
    assert lib.ns2vc_debug_kernel_table(7, C.byref(rows), None) != 0          # the new table is not an eighth family


def test_abi_did_not_move():
    L, lib = _lib()
    assert lib.ns2vc_abi_version() == 7 == L.ABI_VERSION
    assert lib.ns2vc_sizeof_attn_args() == C.sizeof(L.AttnArgs) == ATTN_ARGS_BYTES
