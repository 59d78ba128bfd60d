"""CPU checks of the K/V-resident attention kernel's masked form (csrc/attn_resident.hip: attnres_lens_kernel, plan option ``masked_attn_resident``), by
the method of tests/test_attn_resident_cpu.py: its table's rows are exactly the compiled attnres_lens_kernel instantiations, each of them keeps 4 waves
per SIMD at 1024 threads and uses no scratch, the header declares and the library exports its three hooks, neither the ABI version nor
ns2vc_attn_args moved, its table is no eighth family of ns2vc_debug_kernel_table, and the Python layers pass the option on."""
import ctypes as C
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "ns2vc_amd", "csrc")
HOOKS = ("ns2vc_debug_set_attn_resident_lens", "ns2vc_debug_attnres_lens_table", "ns2vc_debug_attn_resident_lens_launches")
ROWS = 4                 # fp16 / bf16 x hd 16 / 32
ATTN_ARGS_BYTES = 120    # sizeof(ns2vc_attn_args) of ABI v7


def _lib():
    from ns2vc_amd import _lib as L
    return L, L.load()


def test_table_rows_are_the_compiled_instantiations():
    _, lib = _lib()
    r = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-I../../include", "-mllvm",
                        "-amdgpu-mfma-vgpr-form", "--offload-device-only", "-S", "attn_resident.hip", "-o", "-"], cwd=SRC, capture_output=True, text=True,
                       timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    syms = [s for s in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", r.stdout, re.M) if re.match(r"_ZN5ns2vc\d+attnres_lens_kernelI", s)]
    rows = C.c_int(-1)
    assert lib.ns2vc_debug_attnres_lens_table(C.byref(rows)) == 0     # (no HIP call: works without a device)
    assert len(set(syms)) == len(syms) == rows.value == ROWS, (syms, rows.value)
    assert lib.ns2vc_debug_attnres_lens_table(None) != 0
    # both operand types at both head widths: the template arguments as the symbol spells them
    assert sorted(re.search(r"attnres_lens_kernelINS_(\w+?)ELi(\d+)EE", s).groups() for s in syms) == \
        sorted((f"{len(t)}{t}", hd) for t in ("bf16_t", "f16_t") for hd in ("16", "32")), syms
    # every instantiation keeps 4 waves per SIMD at 1024 threads (<= 128 VGPRs) and uses no scratch
    seen = 0
    for name, body in re.findall(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", r.stdout, re.S):
        if name in syms:
            seen += 1
            assert int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1)) <= 128, name
            assert int(re.search(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", body).group(1)) == 0, name
    assert seen == ROWS


def test_hooks_are_declared_bound_and_exported_and_the_abi_did_not_move():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    for name in HOOKS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in L.PROTOTYPES and getattr(lib, name) is not None, name
    assert lib.ns2vc_debug_set_attn_resident_lens(2) != 0 and lib.ns2vc_debug_set_attn_resident_lens(-2) != 0
    for mode in (0, 1, -1):
        assert lib.ns2vc_debug_set_attn_resident_lens(mode) == 0
    assert isinstance(lib.ns2vc_debug_attn_resident_lens_launches(), int)
    # ... and the three new symbols moved neither the ABI version nor ns2vc_attn_args, and the new table is no eighth family
    assert lib.ns2vc_abi_version() == 7 == L.ABI_VERSION
    assert lib.ns2vc_sizeof_attn_args() == C.sizeof(L.AttnArgs) == ATTN_ARGS_BYTES
    rows = C.c_int(-1)
    assert lib.ns2vc_debug_kernel_table(7, C.byref(rows), None) != 0          # the new table is not an eighth family
    assert lib.ns2vc_debug_kernel_table(6, C.byref(rows), None) == 0 and rows.value > 0


def test_option_known_off_by_default_and_passed_on(monkeypatch):
    import inspect
    import recording_engine
    from ns2vc_amd.pipeline import MASKED_OPTIONS, Denoiser
    from ns2vc_amd.service import GroupedConverter
    opts = re.search(r"kOptions\[\] = \{(.*?)\};", open(os.path.join(SRC, "engine.cpp")).read(), re.S).group(1)
    assert '{"masked_attn_resident", "NS2VC_MASKED_ATTN_RESIDENT", &ns2vc_unet::masked_attn_resident}' in opts
    assert re.search(r"bool masked_attn_resident = false;", open(os.path.join(SRC, "engine_internal.h")).read())      # default off
    assert '"masked_attn_resident" 1|0' in open(os.path.join(ROOT, "include", "ns2vc_hip.h")).read()
    assert "masked_attn_resident" in MASKED_OPTIONS
    assert inspect.signature(Denoiser.__init__).parameters["masked_attn_resident"].default is False
    assert inspect.signature(GroupedConverter.__init__).parameters["masked_attn_resident"].default is None
    recording_engine.check_masked_option(monkeypatch, "masked_attn_resident")      # the constructor, set_option and the default, on both engines
