"""Golden vectors of the reference's discrete samplers, ``NaturalSpeech2.ddim_sample`` and ``p_sample_loop`` -> golden_v4.npz.

BUILD CONTAINER ONLY (reads the reference checkout).  The reference's own ``model.py`` runs; the generator only feeds it:
``pre_model.infer`` returns a fixed (content, refer), and ``torch.randn`` / ``torch.randn_like`` (as model.py sees them) return
x_T and then, at table row i, the engine's documented noise stream ``ns2vc_amd.noise.gauss(seeds, i, ...)`` -- so the engine,
fed the same seeds, must follow the reference to its precision.  What is committed is data only.

  g12.*  synthetic loops: ``diff_model`` replaced by the closed form ``synthetic_x0`` (restated in tests/test_stochastic_cpu.py),
         B=2, T=8: DDIM S in {26, 30, 100, 1000} x eta in {0, 0.5, 1} and DDPM-1000 -> time lists, x_T, final latents
  g13.*  full-UNet loops with the procedural weights of v1-v3 (seed 0), B=2, T=188, Lp=469 (prompt lengths 469, 300):
         DDIM-100 eta 0, DDIM-30 eta 1, DDPM-1000 -> seeds, prompt lengths, time lists, final latents.  The inputs are not stored:
         x_T, content and prompt are make_golden.inputs("g13", ...), i.e. ns2vc_amd.weights.hash_normal("g13.x" / ".content" /
         ".prompt"), which the tests regenerate bit for bit.

Run: python tests/golden/make_golden_v4.py   (DDPM-1000 through the full UNet on CPU takes several minutes)
"""
import json
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from make_golden import REF, import_reference_model, inputs  # noqa: E402
sys.path.insert(0, REF)

from ns2vc_amd import noise as N  # noqa: E402
from ns2vc_amd.spec import UNetConfig  # noqa: E402
from ns2vc_amd.weights import procedural_state_dict  # noqa: E402

SYN_B, SYN_T = 2, 8
SYN_SEEDS = np.array([0x0123456789ABCDEF, 7], dtype=np.uint64)
SYN_CASES = [("ddim", s, e) for s in (26, 30, 100, 1000) for e in (0.0, 0.5, 1.0)] + [("ddpm", 1000, 0.0)]
UNET_SEEDS = np.array([20261015, 0xFEEDFACECAFEBEEF], dtype=np.uint64)
UNET_CASES = [("ddim", 100, 0.0), ("ddim", 30, 1.0), ("ddpm", 1000, 0.0)]


def synthetic_x0(x, t):
    """a cheap, smooth, contractive stand-in for the denoiser: x (B, C, T), t (B,) -> x0"""
    tt = t.to(x.dtype).reshape(-1, 1, 1)
    return 0.9 * torch.tanh(x) + 0.05 * torch.cos(0.01 * tt)


class Synthetic(torch.nn.Module):
    def forward(self, x, data, t):
        return synthetic_x0(x, t)


def case_tag(solver, steps, eta):
    return f"{solver}{steps}_eta{eta:g}".replace(".", "p")


def run_reference(nat, solver, steps, eta, x_T, seeds, content_tbc, refer_tbc, refer_lengths):
    """the reference's own loop, fed x_T and the engine's noise stream; returns (final latent, model times in call order)"""
    nat.sampling_timesteps = steps
    nat.ddim_sampling_eta = eta
    B, C, T = x_T.shape
    times, state = [], {"randn": 0}
    orig_mp, orig_randn, orig_randn_like = nat.model_predictions, torch.randn, torch.randn_like

    def model_predictions(x, t, data=None):
        times.append(int(t[0]))
        return orig_mp(x, t, data)

    def randn(*shape, **kw):
        assert state["randn"] == 0, "x_T is drawn once"
        state["randn"] += 1
        return x_T.clone()

    def randn_like(x, **kw):
        # noise of table row i = the row whose evaluation just ran
        return torch.from_numpy(N.gauss(seeds, len(times) - 1, C, T))

    nat.model_predictions = model_predictions
    nat.pre_model.infer = lambda data, auto_predict_f0=True: (content_tbc, refer_tbc)
    torch.randn, torch.randn_like = randn, randn_like
    try:
        with torch.no_grad():
            lengths = torch.full((B,), T)
            if solver == "ddim":
                y = nat.ddim_sample(None, None, lengths, refer_lengths, None, None)
            else:
                y = nat.p_sample_loop(None, None, lengths, refer_lengths, None, None)
    finally:
        torch.randn, torch.randn_like = orig_randn, orig_randn_like
        nat.model_predictions = orig_mp
    return y, times


def main():
    t0 = time.time()
    M = import_reference_model()
    cfgj = json.load(open(os.path.join(REF, "config.json")))
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        nat = M.NaturalSpeech2(cfgj).eval()
    finally:
        os.chdir(cwd)
    print(f"[{time.time()-t0:.1f}s] reference model built ({nat.num_timesteps} timesteps)")
    out, report = {}, {}

    # ---- g12: synthetic-model loops (pin the tables, the time grid and the t = 0 rule on CPU)
    nat.diff_model = Synthetic()
    x_T = torch.from_numpy(np.random.default_rng(12).standard_normal((SYN_B, 100, SYN_T)).astype(np.float32))
    dummy = torch.zeros((SYN_T, SYN_B, 4)), torch.zeros((3, SYN_B, 4))
    out["g12.x_T"], out["g12.seeds"] = x_T.numpy(), SYN_SEEDS
    for solver, steps, eta in SYN_CASES:
        y, times = run_reference(nat, solver, steps, eta, x_T, SYN_SEEDS, *dummy, torch.tensor([3, 3]))
        tag = case_tag(solver, steps, eta)
        out[f"g12.{tag}.times"] = np.array(times, dtype=np.int16)
        out[f"g12.{tag}.y"] = y.numpy()
        report[f"g12.{tag}"] = {"evals": len(times), "y_rms": float(y.pow(2).mean().sqrt())}
    print(f"[{time.time()-t0:.1f}s] g12: {len(SYN_CASES)} synthetic loops")

    # ---- g13: full-UNet loops with the procedural weights
    cfg = UNetConfig()
    enc = M.Diffusion_Encoder(**cfgj["diffusion_encoder"]).eval()
    enc.unet.load_state_dict({k: torch.from_numpy(v) for k, v in procedural_state_dict(cfg, seed=0).items()}, strict=True)
    nat.diff_model = enc
    B, T, Lp = 2, 188, 469
    x_T, content, prompt = inputs("g13", B, T, Lp, cfg)
    lens = torch.tensor([469, 300])
    out["g13.lens"], out["g13.seeds"] = lens.numpy(), UNET_SEEDS
    for solver, steps, eta in UNET_CASES:
        tt = time.time()
        y, times = run_reference(nat, solver, steps, eta, x_T, UNET_SEEDS, content.permute(2, 0, 1), prompt.permute(1, 0, 2), lens)
        tag = case_tag(solver, steps, eta)
        out[f"g13.{tag}.y"] = y.numpy()
        out[f"g13.{tag}.times"] = np.array(times, dtype=np.int16)
        report[f"g13.{tag}"] = {"evals": len(times), "y_rms": float(y.pow(2).mean().sqrt()), "seconds": round(time.time() - tt, 1)}
        print(f"[{time.time()-t0:.1f}s] g13 {tag}: {len(times)} evaluations in {time.time()-tt:.1f}s")

    np.savez_compressed(os.path.join(HERE, "golden_v4.npz"), **out)
    with open(os.path.join(HERE, "golden_v4_report.json"), "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
    print(json.dumps(report, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
