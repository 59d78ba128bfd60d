#!/usr/bin/env python3
"""Is the device code of two source trees the same, kernel by kernel?

    tools/kernel_code_diff.py [--allow-moved] TREE_A TREE_B [make-style defines, e.g. -DNS2VC_TS_CHUNK=0]

Every ns2vc_amd/csrc/*.hip of both trees is compiled for gfx950 with the Makefile's flags plus --offload-device-only --no-gpu-bundle-output -c
(a plain ELF code object), its symbols are read with llvm-readelf -s, and for every kernel (a FUNC symbol with a `<name>.kd` descriptor) the
function's bytes and the 64-byte descriptor are compared.  Whole-file comparison would not do: the __hip_cuid_* symbol differs between any two
trees.  Prints the symbol-set differences and the kernels whose code or descriptor differ; exit status 0 iff there are none.  A descriptor that
differs in nothing but kernel_code_entry_byte_offset (bytes 16 .. 23: the distance from the descriptor to the code, i.e. where the linker put the
kernel) is named as `moved`: a difference like any other, unless --allow-moved says that a changed layout is expected.  No GPU needed."""
import concurrent.futures as cf
import glob
import os
import shutil
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-I../../include"]
EXTRA = {"attn.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"], "attn_resident.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"]}


def _readelf():
    exe = shutil.which("llvm-readelf")
    if exe:
        return exe
    hipcc = shutil.which("hipcc")
    cand = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "llvm-readelf") if hipcc else ""
    if not os.path.exists(cand):
        sys.exit("llvm-readelf not found (PATH, or llvm/bin beside hipcc)")
    return cand


def kernels(tree, name, defs, tmp):
    """{kernel symbol: (code bytes, descriptor bytes)} of one .hip file"""
    src = os.path.join(tree, "ns2vc_amd", "csrc")
    obj = os.path.join(tmp, name + ".co")
    subprocess.run(["hipcc"] + FLAGS + defs + EXTRA.get(name, []) + ["--offload-device-only", "--no-gpu-bundle-output", "-c", name, "-o", obj],
                   cwd=src, check=True, capture_output=True)
    txt = subprocess.run([_readelf(), "-S", "-s", "--wide", obj], check=True, capture_output=True, text=True).stdout
    sect, syms = {}, {}          # section index -> (address, file offset);  symbol -> (value, size, type, section index)
    for ln in txt.splitlines():
        f = ln.replace("[ ", "[").split()
        if len(f) >= 6 and f[0].startswith("[") and f[0].endswith("]") and f[0][1:-1].isdigit():
            sect[int(f[0][1:-1])] = (int(f[3], 16), int(f[4], 16))
        elif len(f) == 8 and f[0].endswith(":") and f[0][:-1].isdigit() and f[6].isdigit():
            syms[f[7]] = (int(f[1], 16), int(f[2]), f[3], int(f[6]))
    data = open(obj, "rb").read()

    def body(sym):
        val, size, _, ndx = syms[sym]
        addr, off = sect[ndx]
        return data[val - addr + off: val - addr + off + size]
    out = {}
    for s, (_, _, typ, _) in syms.items():
        if typ == "FUNC" and s + ".kd" in syms:
            assert syms[s + ".kd"][1] == 64, s
            out[s] = (body(s), body(s + ".kd"))
    return out


def main():
    argv = [x for x in sys.argv[1:] if x != "--allow-moved"]
    allow_moved = len(argv) != len(sys.argv) - 1
    a, b, defs = argv[0], argv[1], argv[2:]
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(a, "ns2vc_amd", "csrc", "*.hip")))
    names_b = sorted(os.path.basename(p) for p in glob.glob(os.path.join(b, "ns2vc_amd", "csrc", "*.hip")))
    bad = n_moved = 0
    if names != names_b:
        print("file sets differ:", sorted(set(names) ^ set(names_b)))
        bad += 1
        names = sorted(set(names) & set(names_b))
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb, cf.ThreadPoolExecutor(min(8, os.cpu_count() or 2)) as ex:
        jobs = {n: (ex.submit(kernels, a, n, defs, ta), ex.submit(kernels, b, n, defs, tb)) for n in names}
        for n in names:
            ka, kb = jobs[n][0].result(), jobs[n][1].result()
            only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
            code = [s for s in sorted(set(ka) & set(kb)) if ka[s][0] != kb[s][0]]
            desc = [s for s in sorted(set(ka) & set(kb)) if ka[s][1][:16] + ka[s][1][24:] != kb[s][1][:16] + kb[s][1][24:]]
            moved = [s for s in sorted(set(ka) & set(kb)) if ka[s][1] != kb[s][1] and s not in desc]
            print(f"{n}: {len(ka)} | {len(kb)} kernels, {sum(len(v[0]) for v in ka.values())} | {sum(len(v[0]) for v in kb.values())} code bytes; "
                  f"only in A {len(only_a)}, only in B {len(only_b)}, code differs {len(code)}, descriptor differs {len(desc)}, moved {len(moved)}")
            n_moved += len(moved)
            for tag, lst in (("only in A", only_a), ("only in B", only_b), ("code differs", code), ("descriptor differs", desc), ("moved", moved)):
                for s in lst:
                    print(f"  {tag}: {s}")
            bad += len(only_a) + len(only_b) + len(code) + len(desc) + (0 if allow_moved else len(moved))
    print(f"IDENTICAL: same kernel symbols, every kernel's code byte-identical, every descriptor byte-identical"
          + (f" but for the entry offset of {n_moved} kernels that moved inside their code object" if n_moved else "") if not bad else f"DIFFERENT: {bad} finding(s)")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
