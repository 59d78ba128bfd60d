#!/usr/bin/env python
"""Print the engine's launch plan as text, for diffing two builds of the library (NS2VC_LIB selects the build).

For every (configuration, precision, shape, mode) one block: a line per launch of the per-step plan (Engine.op_info(0)) and of the
condition plan (Engine.op_info(1)) -- index, name, kind, algorithmic FLOPs, algorithmic bytes --, then workspace_bytes, the launch
counts and, with debug taps on, the tap names and shapes.  Modes: dense | mask (a prompt keep-mask) | lengths (per-item valid frames,
set_lengths) | debug (taps).  Two builds plan the same launches in the same arena iff their outputs are identical:

    python tools/plan_dump.py --all > a.txt;  NS2VC_LIB=.../libns2vc_hip.so python tools/plan_dump.py --all > b.txt;  diff a.txt b.txt

Needs a GPU (the engine has no CPU path); launches nothing but the small copies of set_mask / set_lengths.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

from ns2vc_amd import engine as E  # noqa: E402
from ns2vc_amd.spec import UNetConfig  # noqa: E402
from ns2vc_amd.weights import procedural_state_dict  # noqa: E402

MODES = ("dense", "mask", "lengths", "debug")
BENCH_SHAPE = (32, 938, 469)        # bench.py: batch 32, 10 s of latent frames, prompt of 469
OPTION_TEST_SHAPE = (3, 131, 129)   # tests/test_engine_gpu.py test_every_plan_option
CONFIG_SHAPE = (2, 37, 21)          # tests/configs.py GOLDEN_SHAPES["b2"]


def tap_names(eng: E.Engine):
    name = C.create_string_buffer(256)
    rows, cols = C.c_int(), C.c_int()
    out = []
    for i in range(eng.lib.ns2vc_unet_num_taps(eng.h)):
        E.check(eng.lib.ns2vc_unet_tap_info(eng.h, i, name, 256, C.byref(rows), C.byref(cols)), "tap_info")
        out.append(f"{name.value.decode()}[{rows.value}x{cols.value}]")
    return out


def dump(eng: E.Engine, title: str) -> None:
    print(f"== {title}")
    for which, tag in ((0, "step"), (1, "cond")):
        for i, (name, kind, flops, nbytes) in enumerate(eng.op_info(which)):
            print(f"{tag} {i:3d} {name} kind={kind} flops={flops!r} bytes={nbytes!r}")
    nf, nc = eng.launches()
    print(f"workspace_bytes={eng.workspace_bytes()} launches_per_step={nf} launches_per_condition={nc}")
    if eng._debug:
        print("taps: " + " ".join(tap_names(eng)))


def run(cfg_name: str, cfg: UNetConfig, weights, prec: str, shape, modes) -> None:
    B, T, Lp = shape
    eng = E.Engine(cfg, precision=prec)
    eng.load_state_dict(weights)
    st = E.Stream()
    for mode in modes:
        eng.set_debug(mode == "debug")
        eng.prepare(B, T, Lp)
        if mode == "mask":
            keep = np.arange(Lp)[None, :] < (Lp - np.arange(B) % Lp)[:, None]
            d_keep = E.DevBuf.from_numpy(keep.astype(np.uint8))
            eng.set_mask(d_keep, stream=st)
        elif mode == "lengths":
            eng.set_lengths(np.maximum(1, T - (np.arange(B) * T) // (2 * B)), stream=st)
        st.sync()
        dump(eng, f"{cfg_name} {prec} B={B} T={T} Lp={Lp} {mode}")
    eng.close()


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--precision", nargs="+", default=["fp32", "fp16", "bf16"], choices=["fp32", "fp16", "bf16"])
    ap.add_argument("--shape", nargs=3, type=int, metavar=("B", "T", "LP"), default=list(BENCH_SHAPE))
    ap.add_argument("--mode", nargs="+", default=list(MODES), choices=MODES)
    ap.add_argument("--config", default="default", help="'default' (the stock UNetConfig) or a name of tests/configs.py CONFIGS")
    ap.add_argument("--all", action="store_true",
                    help="the stock configuration at the bench shape and at test_every_plan_option's, and every configuration of "
                         "tests/configs.py at its golden shape, in every precision and mode")
    a = ap.parse_args()
    from configs import CONFIGS
    if a.all:
        jobs = [("default", UNetConfig(), s) for s in (BENCH_SHAPE, OPTION_TEST_SHAPE)] + [(k, c, CONFIG_SHAPE) for k, c in CONFIGS.items()]
    else:
        jobs = [(a.config, UNetConfig() if a.config == "default" else CONFIGS[a.config], tuple(a.shape))]
    weights = {}
    for name, cfg, shape in jobs:
        if name not in weights:
            weights = {name: procedural_state_dict(cfg, 0)}      # (one configuration's weights at a time)
        for prec in a.precision:
            run(name, cfg, weights[name], prec, shape, a.mode)


if __name__ == "__main__":
    main()
