"""What a zero-change deployment gets from the top-level ``sampler`` package: the reference's 30-step UniPC call pattern (model.py:654-687:
NoiseScheduleVP, model_wrapper(x_start) around a wrapper with a side effect, UniPC(variant="bh2").sample(steps=30, order=2, time_uniform,
multistep)) on the drop-in module, 10 s x batch 32.  Three legs, each timed as whole ``sample`` calls after one warm call:

  capture off   sampler.capture = False: a model call per step + one ns2vc_k_solver_step_flat launch (the ``device`` path)
  capture on    the probe evaluation, then the captured loop (the ``captured`` path)
  direct        Denoiser.sample on the same weights, the hand-edited model.py of INTEGRATION section 2

The stand-in for model.py's branch is written here (the reference is not needed): the cat with the content, the prompt mask, ``.sample``,
and the per-step ``isnan`` assert of model.py:404 with its host wait.  The reference's own Python loop (its sampler/ files) is NOT timed:
the reference is not on the GPU machine, so there is no "before" figure here."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sampler  # noqa: E402
from sampler.uni_pc import NoiseScheduleVP, UniPC, model_wrapper  # noqa: E402
from ns2vc_amd import schedule as S  # noqa: E402
from ns2vc_amd.pipeline import Denoiser  # noqa: E402
from ns2vc_amd.weights import procedural_state_dict  # noqa: E402
from unet1d import UNet1DConditionModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--frames", type=int, default=938)
ap.add_argument("--prompt", type=int, default=469)
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--precision", default="fp16")
ap.add_argument("--out", default="")
a = ap.parse_args()
dev = torch.device("cuda", 0)
B, T, Lp, K = a.batch, a.frames, a.prompt, a.steps
W = {k: torch.from_numpy(v) for k, v in procedural_state_dict(seed=0).items()}
unet = UNet1DConditionModel(in_channels=356, out_channels=100, block_out_channels=(128, 256, 384, 512), norm_num_groups=8, cross_attention_dim=256,
                            attention_head_dim=8, addition_embed_type="text", resnet_time_scale_shift="scale_shift", engine_precision=a.precision)
unet.load_state_dict(W, strict=True)
unet = unet.to(dev).eval()
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn((B, 100, T), device=dev, generator=g)
content = torch.randn((B, 256, T), device=dev, generator=g)
prompt = torch.randn((B, Lp, 256), device=dev, generator=g)
plens = torch.full((B,), Lp, device=dev)
betas = torch.from_numpy(S.linear_betas()).to(dev)
ticks = [0]


def forward(x, data, t):      # model.py:403-415
    assert torch.isnan(x).any() == False      # noqa: E712  (the reference's host wait, once per step)
    content, prompt, plens = data
    mask = (torch.arange(prompt.shape[1], device=x.device)[None, :] < plens[:, None]).to(torch.bool)
    return unet(torch.cat([x, content], dim=1), t, prompt, encoder_attention_mask=mask).sample


def wrapped(x, t, **kwargs):      # model.py:658-664: my_wrapper(self.sample_fun)
    ret = forward(x, kwargs["data"], t)
    ticks[0] += 1
    return ret


def reference_branch():      # model.py:654-687
    ns = NoiseScheduleVP(schedule="discrete", betas=betas)
    fn = model_wrapper(wrapped, ns, model_type="x_start", model_kwargs={"data": (content, prompt, plens)})
    s = UniPC(fn, ns, variant="bh2")
    with torch.no_grad():
        y = s.sample(x, steps=K, order=2, skip_type="time_uniform", method="multistep")
    return s, y


def timed(fn):
    fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(a.reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


lines = [f"sampler drop-in bench: B={B} T={T} Lp={Lp}, UniPC bh2 order 2, {K} steps, time_uniform, multistep; {a.precision} engine; best of {a.reps} calls after a warm one"]
res = {}
for name, cap in (("capture off", False), ("capture on", True)):
    sampler.capture = cap
    s, y = reference_branch()
    ticks[0], calls = 0, unet.engine_calls
    res[name] = (timed(reference_branch), y)
    n = a.reps + 1
    lines.append(f"  {name:12s} {res[name][0] * 1e3:9.2f} ms per sample call ({res[name][0] * 1e3 / K:.3f} ms/step)  path={s.last_path}  "
                 f"model calls per sample: {(unet.engine_calls - calls) / n:g}, wrapper side effects: {ticks[0] / n:g}")
den = Denoiser(unet.state_dict(), unet.cfg, precision=unet._precision, betas=S.linear_betas())
mask = torch.ones((B, Lp), dtype=torch.bool, device=dev)
direct = lambda: den.sample(content, prompt, mask, x, solver="unipc", steps=K, order=2)      # noqa: E731
t_direct = timed(direct)
y_direct = direct()
lines.append(f"  {'direct':12s} {t_direct * 1e3:9.2f} ms per Denoiser.sample call ({t_direct * 1e3 / K:.3f} ms/step)")
with torch.no_grad():
    t_probe = timed(lambda: wrapped(x, torch.full((B,), 999.0, device=dev), data=(content, prompt, plens)))
on, off = res["capture on"][0], res["capture off"][0]
rel = lambda u, v: float((u - v).norm() / v.norm())      # noqa: E731
lines.append(f"  one probe evaluation (the stand-in's forward, eager): {t_probe * 1e3:.2f} ms; capture on - direct = {(on - t_direct) * 1e3:.2f} ms")
lines.append(f"  capture on vs off: {off / on:.3f}x; captured == direct bit for bit: {bool(torch.equal(res['capture on'][1], y_direct))}; "
             f"capture off vs on rel L2 {rel(res['capture off'][1], res['capture on'][1]):.2e}")
lines.append("  (the reference's own Python loop is not timed here: its sampler/ files are not on the GPU machine)")
print("\n".join(lines))
if a.out:
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
