#!/usr/bin/env python3
"""golden_v6: the reference UNet on every non-default configuration of tests/configs.py (CONFIGS).

Run only in the build container (needs /root/reference, read-only; imported at run time).  For every configuration it
  1. builds the reference ``UNet1DConditionModel`` with the configuration's ctor kwargs (block types included),
  2. asserts that its state-dict keys and shapes equal ``param_spec(cfg)``, name for name, in order,
  3. loads ``procedural_state_dict(cfg, 0)`` strictly,
  4. runs the two GOLDEN_SHAPES (odd T, a partly masked prompt, timesteps 999 / 500.5 / 3) and stores the outputs (float32) and a
     hash of the key list -- data only,
  5. asserts that the oracle (oracle/unet_ref.py) reproduces every output within 1e-6.

Usage:  python tests/golden/make_golden_v6.py      # writes tests/golden/golden_v6.npz and golden_v6_report.json
Rerunning writes the same arrays (the inputs and weights are integer-hash draws; the npz is written without timestamps).
"""
from __future__ import annotations

import hashlib
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True

from configs import CONFIGS, GOLDEN_SHAPES, ctor_kwargs, golden_inputs  # noqa: E402
from ns2vc_amd.spec import param_spec  # noqa: E402
from ns2vc_amd.weights import procedural_state_dict  # noqa: E402
from oracle import unet_ref  # noqa: E402

ORACLE_TOL = 1e-6


def key_hash(items) -> str:
    """sha256 of 'name:d0,d1,..' lines, in registration order"""
    s = "\n".join(f"{k}:{','.join(str(int(d)) for d in shape)}" for k, shape in items)
    return hashlib.sha256(s.encode()).hexdigest()


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def save_npz_deterministic(path: str, arrays: dict) -> None:
    """np.savez with a fixed zip timestamp, so that a rerun is byte-identical"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main() -> None:
    torch.set_num_threads(8)
    sys.path.insert(0, REF)
    from unet1d.unet_1d_condition import UNet1DConditionModel  # type: ignore  (the reference, read-only)
    out, report = {}, {}
    for cid, cfg in CONFIGS.items():
        ref = UNet1DConditionModel(**ctor_kwargs(cfg)).eval()
        sd = ref.state_dict()
        spec = param_spec(cfg)
        assert list(sd.keys()) == list(spec.keys()), (cid, "param_spec names / order differ from the reference")
        for k, v in sd.items():
            assert tuple(v.shape) == tuple(spec[k]), (cid, k, tuple(v.shape), spec[k])
        h = key_hash((k, tuple(v.shape)) for k, v in sd.items())
        assert h == key_hash(spec.items())
        P = {k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg, 0).items()}
        ref.load_state_dict(P, strict=True)
        out[f"{cid}.keys_sha256"] = np.frombuffer(bytes.fromhex(h), dtype=np.uint8)
        report[cid] = {"n_tensors": len(spec), "keys_sha256": h}
        for sid in GOLDEN_SHAPES:
            x, c, p, mask, ts = golden_inputs(cid, sid)
            sample = torch.cat([torch.from_numpy(x), torch.from_numpy(c)], dim=1)
            m = torch.from_numpy(mask)
            with torch.no_grad():
                y_ref = ref(sample, torch.from_numpy(ts), torch.from_numpy(p), encoder_attention_mask=m).sample.float().numpy()
            y_or = unet_ref.unet_forward(P, cfg, sample, torch.from_numpy(ts), torch.from_numpy(p), m).numpy()
            e = rel_l2(y_or, y_ref)
            assert e <= ORACLE_TOL, (cid, sid, e)
            out[f"{cid}.{sid}.y"] = y_ref.astype(np.float32)
            report[cid][f"{sid}.oracle_vs_ref"] = e
            print(f"{cid:12s} {sid}: out {y_ref.shape}, oracle vs reference rel_l2 {e:.2e}")
    save_npz_deterministic(os.path.join(HERE, "golden_v6.npz"), out)
    with open(os.path.join(HERE, "golden_v6_report.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote golden_v6.npz ({os.path.getsize(os.path.join(HERE, 'golden_v6.npz'))} bytes)")


if __name__ == "__main__":
    main()
