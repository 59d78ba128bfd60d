"""The reference's solver classes as drivers of ``ns2vc_amd.schedule``: one fp64 coefficient table per ``sample`` call
(``schedule.build_table``), the float32 recurrence of ``schedule.solver_update``, and three ways to run it:

  host      x on the CPU: ``schedule.solver_update`` on float32 arrays, the model called on the caller's tensors
  device    x on the GPU, any model: five fp32 state tensors shaped like x, per evaluation one call of the model and one launch of
            ``ns2vc_k_solver_step_flat``; nothing in the loop waits for the device or reads from it
  captured  x on the GPU and the model recognised as ``unet1d.UNet1DConditionModel`` behind an x_start wrapper: one probe evaluation,
            then the whole loop inside ``ns2vc_amd.pipeline.Denoiser.sample`` (the captured loop of ``ns2vc_sampler_run``)

``solver.last_path`` names the way the last call took.  What the classes refuse is refused with a ValueError that names the keyword.
Nothing here imports ``oracle``; ``libns2vc_hip.so`` is loaded when a CUDA tensor first needs it."""
from __future__ import annotations

import hashlib
import inspect
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from ns2vc_amd import schedule as S

MODEL_TYPES = ("noise", "x_start", "v", "score")
GUIDANCE_TYPES = ("uncond", "classifier", "classifier-free")
_TABLES: "OrderedDict[tuple, S.SolverTable]" = OrderedDict()      # (schedule, solver, steps, order, options) -> table
_DEVICE_TABLES: "OrderedDict[tuple, tuple]" = OrderedDict()      # (table, device) -> its rows, model times and labels on the device, uploaded once
_CACHE_ROOM = 64


def _cached(cache, key, make):
    if key in cache:
        cache.move_to_end(key)
        return cache[key]
    v = cache[key] = make()
    while len(cache) > _CACHE_ROOM:
        cache.popitem(last=False)
    return v


class NoiseScheduleVP:
    """The discrete VP schedule on top of ``schedule.VPSchedule``: log alpha piecewise linear over t in [1/N, 1] between the model's N
    timesteps.  The methods take and return torch tensors (any shape, the tensor's device; evaluated in float64 by torch ops on that
    device, so a CUDA argument costs no host wait, and returned in ``dtype``)."""

    def __init__(self, schedule="discrete", betas=None, alphas_cumprod=None, continuous_beta_0=0.1, continuous_beta_1=20., dtype=torch.float32):
        if schedule != "discrete":
            raise ValueError(f"schedule must be 'discrete' (the continuous 'linear' / 'cosine' schedules have no table in ns2vc_amd.schedule), got {schedule!r}")
        if betas is None and alphas_cumprod is None:
            raise ValueError("betas or alphas_cumprod must be given for schedule='discrete', got neither")
        self.schedule = schedule
        self.dtype = dtype
        self.betas: Optional[np.ndarray] = None
        if betas is not None:
            self.betas = torch.as_tensor(betas).detach().to("cpu", torch.float32).numpy().reshape(-1).copy()
            self.vp = S.VPSchedule(self.betas)
        else:
            self.vp = S.VPSchedule.from_alphas_cumprod(torch.as_tensor(alphas_cumprod).detach().to("cpu", torch.float32).numpy())
        self.total_N = self.vp.N
        self.T = 1.
        self.key = hashlib.sha256(self.vp.log_alpha.tobytes()).hexdigest()      # what the table caches know this schedule by
        self._knots: Dict[torch.device, tuple] = {}

    def _on(self, device):
        if device not in self._knots:
            self._knots[device] = (torch.from_numpy(self.vp.knots).to(device), torch.from_numpy(self.vp.log_alpha).to(device))
        return self._knots[device]

    @staticmethod
    def _interp(x, xp, yp):
        """piecewise linear through (xp, yp), xp ascending, the end segments extrapolated (``VPSchedule.log_alpha_at``)"""
        i = torch.clamp(torch.searchsorted(xp, x.contiguous()) - 1, 0, xp.shape[0] - 2)
        return yp[i] + (x - xp[i]) * (yp[i + 1] - yp[i]) / (xp[i + 1] - xp[i])

    def _log_alpha(self, t):
        t = torch.as_tensor(t)
        knots, la = self._on(t.device)
        return self._interp(t.to(torch.float64), knots, la)

    def marginal_log_mean_coeff(self, t):
        return self._log_alpha(t).to(self.dtype)

    def marginal_alpha(self, t):
        return torch.exp(self._log_alpha(t)).to(self.dtype)

    def marginal_std(self, t):
        return torch.sqrt(1. - torch.exp(2. * self._log_alpha(t))).to(self.dtype)

    def marginal_lambda(self, t):
        la = self._log_alpha(t)
        return (la - 0.5 * torch.log(1. - torch.exp(2. * la))).to(self.dtype)

    def inverse_lambda(self, lamb):
        lamb = torch.as_tensor(lamb)
        knots, la = self._on(lamb.device)
        lam64 = lamb.to(torch.float64)
        log_alpha = -0.5 * torch.logaddexp(torch.zeros_like(lam64), -2. * lam64)
        return self._interp(log_alpha, torch.flip(la, [0]), torch.flip(knots, [0])).to(self.dtype)

    def model_time(self, t_continuous):
        """the discrete model's time input of a continuous label, (t - 1/N) * 1000 in the label's own precision"""
        return (t_continuous - 1. / self.total_N) * 1000.


class ModelFn:
    """What ``model_wrapper`` returns: ``model_fn(x, t_continuous) -> noise`` that carries its own description -- the raw model, what it
    predicts, its keywords, the guidance -- so a solver class can see what it is made of and call the raw model itself."""

    def __init__(self, model, noise_schedule, model_type, model_kwargs, guidance_type, condition, unconditional_condition, guidance_scale,
                 classifier_fn, classifier_kwargs):
        self.model, self.noise_schedule, self.model_type, self.model_kwargs = model, noise_schedule, model_type, dict(model_kwargs or {})
        self.guidance_type, self.condition, self.unconditional_condition = guidance_type, condition, unconditional_condition
        self.guidance_scale, self.classifier_fn, self.classifier_kwargs = guidance_scale, classifier_fn, dict(classifier_kwargs or {})

    @staticmethod
    def _like(v, x):
        return v.reshape(v.shape + (1,) * (x.dim() - v.dim()))

    def noise_pred(self, x, t_continuous, cond=None):
        ns = self.noise_schedule
        t_input = ns.model_time(t_continuous)
        out = self.model(x, t_input, **self.model_kwargs) if cond is None else self.model(x, t_input, cond, **self.model_kwargs)
        if self.model_type == "noise":
            return out
        alpha, sigma = self._like(ns.marginal_alpha(t_continuous), x), self._like(ns.marginal_std(t_continuous), x)
        if self.model_type == "x_start":
            return (x - alpha * out) / sigma
        if self.model_type == "v":
            return alpha * out + sigma * x
        return -sigma * out      # score

    def __call__(self, x, t_continuous):
        if self.guidance_type == "uncond":
            return self.noise_pred(x, t_continuous)
        if self.guidance_type == "classifier":
            t_input = self.noise_schedule.model_time(t_continuous)
            with torch.enable_grad():
                x_in = x.detach().requires_grad_(True)
                log_prob = self.classifier_fn(x_in, t_input, self.condition, **self.classifier_kwargs)
                grad = torch.autograd.grad(log_prob.sum(), x_in)[0]
            sigma = self._like(self.noise_schedule.marginal_std(t_continuous), x)
            return self.noise_pred(x, t_continuous) - self.guidance_scale * sigma * grad
        if self.guidance_scale == 1. or self.unconditional_condition is None:
            return self.noise_pred(x, t_continuous, cond=self.condition)
        both = self.noise_pred(torch.cat([x] * 2), torch.cat([t_continuous] * 2), cond=torch.cat([self.unconditional_condition, self.condition]))
        noise_u, noise_c = both.chunk(2)
        return noise_u + self.guidance_scale * (noise_c - noise_u)


def model_wrapper(model, noise_schedule, model_type="noise", model_kwargs={}, guidance_type="uncond", condition=None,
                  unconditional_condition=None, guidance_scale=1., classifier_fn=None, classifier_kwargs={}):
    """``model(x, t_input[, cond], **model_kwargs)`` with the discrete time input ``(t - 1/N) * 1000`` -> ``model_fn(x, t_continuous)``
    that returns the predicted noise, under no guidance, classifier guidance or classifier-free guidance (the unconditional half first
    in one batch of 2B)."""
    if model_type not in MODEL_TYPES:
        raise ValueError(f"model_type must be one of {MODEL_TYPES}, got {model_type!r}")
    if guidance_type not in GUIDANCE_TYPES:
        raise ValueError(f"guidance_type must be one of {GUIDANCE_TYPES}, got {guidance_type!r}")
    if guidance_type == "classifier" and classifier_fn is None:
        raise ValueError("classifier_fn must be given for guidance_type='classifier', got None")
    return ModelFn(model, noise_schedule, model_type, model_kwargs, guidance_type, condition, unconditional_condition, guidance_scale,
                   classifier_fn, classifier_kwargs)


class Solver:
    """What ``DPM_Solver`` and ``UniPC`` share: the checks, the table, the three paths."""
    solver = ""

    def __init__(self, model_fn, noise_schedule, correcting_x0_fn, correcting_xt_fn, thresholding_max_val, dynamic_thresholding_ratio, variant="bh2"):
        if not isinstance(noise_schedule, NoiseScheduleVP):
            raise ValueError(f"noise_schedule must be this package's NoiseScheduleVP, got {type(noise_schedule).__name__}")
        if correcting_xt_fn is not None:
            raise ValueError(f"correcting_xt_fn must be None (a correction of the state between steps has no place in the table's recurrence), got {correcting_xt_fn!r}")
        if not (correcting_x0_fn is None or correcting_x0_fn == "dynamic_thresholding" or callable(correcting_x0_fn)):
            raise ValueError(f"correcting_x0_fn must be None, 'dynamic_thresholding' or a callable (x0, t) -> x0, got {correcting_x0_fn!r}")
        S.check_x0_correction("dynamic_thresholding", dynamic_thresholding_ratio, thresholding_max_val)
        if not callable(model_fn):
            raise ValueError(f"model_fn must be callable, got {model_fn!r}")
        self.model_fn = model_fn      # (a bare callable is taken as a noise-prediction function of (x, t_continuous))
        self.noise_schedule = noise_schedule
        self.correcting_x0_fn, self.correcting_xt_fn = correcting_x0_fn, correcting_xt_fn
        self.thresholding_max_val, self.dynamic_thresholding_ratio = thresholding_max_val, dynamic_thresholding_ratio
        self.variant = variant
        self.last_path: Optional[str] = None
        self.last_table: Optional[S.SolverTable] = None

    # ---- the table ---------------------------------------------------------------------------------------------------------------
    def _table(self, steps, order, options) -> S.SolverTable:
        key = (self.noise_schedule.key, self.solver, int(steps), order, S.table_options(options))
        return _cached(_TABLES, key, lambda: S.build_table(self.solver, int(steps), self.noise_schedule.vp, order, **options))

    def _sample(self, x, steps, order, method, return_intermediate, options):
        if method != "multistep":
            raise ValueError(f"method must be 'multistep' (singlestep / adaptive solvers are not served by the captured loop), got {method!r}")
        if return_intermediate:
            raise ValueError(f"return_intermediate must be False (the loop keeps its state on the device and hands back the sample alone), got {return_intermediate!r}")
        if not (torch.is_tensor(x) and x.is_floating_point() and x.dim() >= 1):
            raise ValueError("x must be a floating-point tensor of shape (B, ...)")
        table = self._table(steps, order, options)
        self.last_table = table
        if not x.is_cuda:
            self.last_path = "host"
            return self._run_host(x, table)
        with torch.cuda.device(x.device):
            first = None
            if self._may_capture(x):
                y, first = self._try_captured(x, table, steps, order, options)
                if y is not None:
                    self.last_path = "captured"
                    return y
            self.last_path = "device"
            return self._run_device(x, table, first)

    # ---- one evaluation ----------------------------------------------------------------------------------------------------------
    def _times(self, table, device):
        """per row the raw model's time input and the continuous label, as float32 tensors on ``device`` (uploaded once per table)"""
        return self._device_rows(table, device)[1:]

    def _device_rows(self, table, device):
        """(the coefficient rows, the model times, the continuous labels) of ``table`` on ``device``: uploaded once and cached"""
        def upload():
            t_cont = np.asarray(table.timesteps, dtype=np.float64)[:table.steps].astype(np.float32)      # (denoise_to_zero: one more row, at the last label t_0)
            return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device) for a in (table.coef, table.coef[:, 0], t_cont))
        return _cached(_DEVICE_TABLES, (self.solver, table.coef.tobytes(), np.asarray(table.timesteps).tobytes(), str(device)), upload)

    def _direct(self) -> bool:
        """the solver calls the raw model itself and hands its kind to the update (a wrapper of this package, no guidance)"""
        return isinstance(self.model_fn, ModelFn) and self.model_fn.guidance_type == "uncond"

    def _evaluate(self, xe, B, t_model, t_cont, dtype):
        """the model at xe -> (its output as float32, what the output is)"""
        fn = self.model_fn
        xin = xe.to(dtype)
        if self._direct():
            return fn.model(xin, t_model.expand(B), **fn.model_kwargs).to(torch.float32), fn.model_type
        return fn(xin, t_cont.expand(B)).to(torch.float32), "noise"

    def _correction(self):
        c = self.correcting_x0_fn
        if c is None:
            return None
        if c == "dynamic_thresholding":
            return dict(mode="dynamic_thresholding", ratio=float(self.dynamic_thresholding_ratio), max_val=float(self.thresholding_max_val))
        return c

    # ---- host --------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _host_x0(kind, c, out, xe):
        """the predicted x0 of a model output of ``kind`` in float32 -- what ``solver_update`` takes as x0"""
        f = np.float32
        alpha, sigma = f(c[1]), f(c[2])
        if kind == "x_start":
            return out
        eps = out if kind == "noise" else (alpha * out + sigma * xe if kind == "v" else -sigma * out)
        return (xe - sigma * eps) / alpha

    def _run_host(self, x, table):
        state = S._start_state(x.detach().to(torch.float32).numpy().copy())
        hist2 = S.has_history2(table)
        corr = self._correction()
        t_model, t_cont = self._times(table, x.device)
        B = x.shape[0]
        for i in range(table.steps):
            c = table.coef[i]
            xe = state[0]
            out, kind = self._evaluate(torch.from_numpy(xe), B, t_model[i], t_cont[i], x.dtype)
            x0 = self._host_x0(kind, c, out.detach().numpy(), xe)
            correct = None
            if callable(corr):      # m as the update forms it, the caller's correction on it, and the corrected m as the step's x0
                f = np.float32
                m = (xe - f(c[2]) * ((xe - f(c[1]) * x0) / f(c[2]))) / f(c[1])
                x0 = corr(torch.from_numpy(m), t_cont[i].expand(B)).detach().to(torch.float32).numpy()
            elif corr is not None:
                correct = corr
            state = list(S.solver_update(c, hist2, x0, *state, correct))
        return torch.from_numpy(np.ascontiguousarray(state[0])).to(x.dtype)

    # ---- device ------------------------------------------------------------------------------------------------------------------
    def _threshold(self, m, B):
        """dynamic thresholding of m on the device: the per-item quantile of |m|, at least max_val; clamp and divide"""
        s = torch.quantile(m.abs().reshape(B, -1), float(self.dynamic_thresholding_ratio), dim=1)
        s = torch.maximum(s, torch.full_like(s, float(self.thresholding_max_val))).reshape((B,) + (1,) * (m.dim() - 1))
        return torch.clamp(m, -s, s) / s

    def _run_device(self, x, table, first=None):
        from ns2vc_amd import _lib
        lib = _lib.load()
        dev, B, n = x.device, x.shape[0], x.numel()
        if n == 0:
            return x.clone()
        hist2 = S.has_history2(table)
        corr = self._correction()
        coef, t_model, t_cont = self._device_rows(table, dev)
        x32 = x.detach().to(torch.float32).contiguous()
        xe, xbar = x32.clone(), x32.clone()
        d1, mprev = torch.zeros_like(x32), torch.zeros_like(x32)
        mprev2 = torch.zeros_like(x32) if hist2 else None
        stream = torch.cuda.current_stream(dev).cuda_stream

        def step(row, kind, out, m_out=None):
            _lib.check(lib.ns2vc_k_solver_step_flat(coef.data_ptr(), table.steps, row, _lib.FLAT_KINDS[kind], out.data_ptr(), xe.data_ptr(), xbar.data_ptr(),
                                                    d1.data_ptr(), mprev.data_ptr(), None if mprev2 is None else mprev2.data_ptr(),
                                                    None if m_out is None else m_out.data_ptr(), n, stream), "ns2vc_k_solver_step_flat")

        for i in range(table.steps):
            if i == 0 and first is not None:      # (the probe of the captured path evaluated exactly this point)
                out, kind = first.to(torch.float32), self.model_fn.model_type
            else:
                out, kind = self._evaluate(xe, B, t_model[i], t_cont[i], x.dtype)
            if tuple(out.shape) != tuple(x.shape):
                raise ValueError(f"the model returned shape {tuple(out.shape)} for an x of shape {tuple(x.shape)}")
            out = out.contiguous()
            if corr is None:
                step(i, kind, out)
                continue
            m = torch.empty_like(x32)
            step(i, kind, out, m_out=m)      # FORM: m alone
            m = self._threshold(m, B) if isinstance(corr, dict) else corr(m, t_cont[i].expand(B)).to(torch.float32)
            step(i, "data", m.contiguous())
        return xe.to(x.dtype)

    # ---- captured ----------------------------------------------------------------------------------------------------------------
    def _may_capture(self, x) -> bool:
        import sampler
        fn = self.model_fn
        return bool(sampler.capture) and isinstance(fn, ModelFn) and fn.model_type == "x_start" and fn.guidance_type == "uncond" and x.dim() == 3 \
            and (self.correcting_x0_fn is None or self.correcting_x0_fn == "dynamic_thresholding") and self.noise_schedule.betas is not None

    def _try_captured(self, x, table, steps, order, options):
        """The probe: the raw model once at (x, the model time of row 0) while every call into a ``unet1d.UNet1DConditionModel`` is
        observed.  -> (the sample, None) when the model is that module behind a plain concatenation, else (None, the probe's output:
        the device path's first evaluation)."""
        from unet1d import UNet1DConditionModel
        fn = self.model_fn
        B, C, T = x.shape
        seen, before = [], {}

        def pre_hook(module, args):
            if isinstance(module, UNet1DConditionModel):
                before.setdefault(id(module), module.engine_calls)

        def hook(module, args, kwargs, output):
            if isinstance(module, UNet1DConditionModel):
                seen.append((module, args, kwargs, output))

        t_model, _ = self._times(table, x.device)
        t0 = t_model[0].expand(B)
        handles = (torch.nn.modules.module.register_module_forward_pre_hook(pre_hook),
                   torch.nn.modules.module.register_module_forward_hook(hook, with_kwargs=True))
        try:
            out = fn.model(x, t0, **fn.model_kwargs)
        finally:
            for h in handles:
                h.remove()
        if len(seen) != 1:
            return None, out
        module, args, kwargs, output = seen[0]
        calls_after = before[id(module)] + 1      # its engine route: one forward served by the HIP engine
        try:
            a = inspect.signature(module.forward).bind(*args, **kwargs).arguments
        except TypeError:
            return None, out
        sample, ts, prompt, mask = a.get("sample"), a.get("timestep"), a.get("encoder_hidden_states"), a.get("encoder_attention_mask")
        cfg = module.cfg
        unet_out = output.sample if hasattr(output, "sample") else output[0]
        ok = (torch.is_tensor(sample) and sample.is_cuda and torch.is_tensor(prompt) and prompt.dim() == 3 and C == cfg.latent_channels
              and tuple(sample.shape) == (B, C + cfg.content_channels, T) and module._engine is not None and module.engine_calls == calls_after
              and torch.is_tensor(out) and tuple(out.shape) == tuple(x.shape) and tuple(unet_out.shape) == tuple(x.shape))
        if ok:
            tv = ts if torch.is_tensor(ts) else torch.tensor([float(ts)], device=x.device)
            tv = tv.to(device=x.device, dtype=torch.float32).reshape(-1)
            ok = tv.numel() in (1, B)
        if ok:      # the compares that wait for the device: once per sample call
            ok = bool(torch.equal(tv.expand(B), t0) and torch.equal(sample[:, :C], x) and torch.equal(out, unet_out))
        if not ok:
            return None, out
        den = self._denoiser_of(module)
        kw = dict(options)
        if self.solver != "unipc":
            kw.pop("variant", None)
        if self.solver != "dpmsolver++":
            kw.pop("solver_type", None)
        pm = None if mask is None else mask.reshape(B, -1).to(torch.bool)
        y = den.sample(sample[:, C:], prompt, prompt_mask=pm, noise=x, solver=self.solver, steps=int(steps), order=order,
                       correcting_x0_fn=self.correcting_x0_fn, thresholding_max_val=self.thresholding_max_val,
                       dynamic_thresholding_ratio=self.dynamic_thresholding_ratio, **kw)
        return y.to(x.dtype), None

    def _denoiser_of(self, module):
        """the Denoiser that runs the loop for ``module``: its own engine (a second copy of the packed weights and workspace beside the
        module's), kept on the module under its weights key -- new weights, another precision or other betas rebuild it"""
        from ns2vc_amd.pipeline import Denoiser
        key = (module._weights_key(), self.noise_schedule.key)
        held = getattr(module, "_sampler_denoiser", None)
        if held is not None and held[0] == key:
            return held[1]
        if held is not None:
            for eng in (held[1].engine, held[1].tail_engine):
                if eng is not None:
                    eng.close()
        den = Denoiser({k: v.detach() for k, v in module.state_dict().items()}, module.cfg, precision=module._precision, betas=self.noise_schedule.betas)
        object.__setattr__(module, "_sampler_denoiser", (key, den))
        return den
