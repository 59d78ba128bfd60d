"""CPU check of the kernel tables (csrc/kernel_table.h): for each of the seven kernel templates, the number of instantiations in the gfx950 device
code equals the number of rows of its table (ns2vc_debug_kernel_table) and equals the count recorded here.  With "every row is a distinct
instantiation" (distinct keys name distinct template arguments) this says that nothing of these templates is compiled outside its table -- every
compiled kernel can be launched and has its LDS attribute set -- and that no instantiation was added or dropped unnoticed."""
import concurrent.futures as cf
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ns2vc_amd", "csrc")

# (template, file, instantiations) in the order of ns2vc_debug_kernel_table's `family`
FAMILIES = [("gemm2_kernel", "gemm.hip", 24), ("gemm4_kernel", "gemm.hip", 72), ("conv3ts_kernel", "convts.hip", 70), ("attn_kernel", "attn.hip", 40),
            ("ffn_kernel", "ffn.hip", 20), ("geglu_kernel", "geglu.hip", 4), ("rowchain_kernel", "rowchain.hip", 40)]


def _device_asm(name):
    """the gfx950 assembly of one kernel file, compiled as the Makefile compiles it"""
    extra = ["-mllvm", "-amdgpu-mfma-vgpr-form"] if name == "attn.hip" else []
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-I../../include"] + extra +
                       ["--offload-device-only", "-S", name, "-o", "-"], cwd=SRC, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.fixture(scope="module")
def compiled_kernels():
    """{file: [.amdhsa_kernel symbols]}: the six files compiled once, in parallel"""
    from ns2vc_amd import _lib
    if shutil.which("hipcc") is None:
        pytest.skip("hipcc not on PATH")
    if not os.path.exists(_lib.LIB_PATH):          # (before the compiles: a skip costs nothing)
        pytest.skip("library not built")
    files = sorted({f for _, f, _ in FAMILIES})
    with cf.ThreadPoolExecutor(len(files)) as ex:
        asm = dict(zip(files, ex.map(_device_asm, files)))
    return {f: re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", a, re.M) for f, a in asm.items()}


def test_compiled_instantiations_are_the_table_rows(compiled_kernels):
    from ns2vc_amd import _lib
    lib = _lib.load()
    for family, (tmpl, name, want) in enumerate(FAMILIES):
        rows = C.c_int(-1)
        assert lib.ns2vc_debug_kernel_table(family, C.byref(rows), None) == 0          # (no HIP call: works without a device)
        syms = [s for s in compiled_kernels[name] if re.match(r"_ZN5ns2vc\d+%sI" % tmpl, s)]
        assert len(set(syms)) == len(syms)
        assert len(syms) == rows.value == want, (tmpl, len(syms), rows.value, want)
    rows = C.c_int(-1)
    assert lib.ns2vc_debug_kernel_table(len(FAMILIES), C.byref(rows), None) != 0       # an unknown family is an error
    assert lib.ns2vc_debug_kernel_table(-1, C.byref(rows), None) != 0
