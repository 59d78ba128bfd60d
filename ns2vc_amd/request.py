"""What one ``Denoiser.sample`` call asks for, checked and normalised once (``SampleRequest.parse``), and the per-item rules that ``sample``,
the slot loop and the converters share.  Host only: nothing here touches an engine."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from .schedule import (DISCRETE_SOLVERS, SOLVERS, ItemTables, build_table, build_tables, check_x0_correction, schedule_key, table_options)

CORRECTION_KEYS = ("correcting_x0_fn", "thresholding_max_val", "dynamic_thresholding_ratio")
# the keywords of ``Denoiser.sample`` that hold one entry per item (a scalar, or one shared (1, ...) row, in their place goes to every item)
PER_ITEM_KEYS = ("content", "prompt", "prompt_mask", "noise", "lengths", "seeds", "prompt_lengths", "guidance_scale", "unconditional_prompt",
                 "unconditional_prompt_mask", "unconditional_prompt_lengths", "unconditional_content", "schedules", "corrections", "known", "known_mask")


def host_array(v) -> np.ndarray:
    """a tensor (on any device), array or sequence as a numpy array on the host"""
    return np.asarray(v.detach().cpu() if hasattr(v, "detach") else v)


def item_correction_entry(c, what: str = "correction"):
    """One item's own x0 correction (``sample(corrections=)``, ``SlotLoop.admit(correction=)``, ``service.Segment.correction``): None or
    ``dict(correcting_x0_fn=, thresholding_max_val=, dynamic_thresholding_ratio=)``, names only -> None (off) or (name, ratio, max_val);
    ValueError naming ``what`` otherwise."""
    if c is None:
        return None
    if callable(c):
        raise ValueError(f"{what}: a callable cannot run inside the captured loop; pass None or a dict with correcting_x0_fn "
                         f"'dynamic_thresholding' or 'clamp'")
    if not isinstance(c, dict):
        raise ValueError(f"{what} must be None or dict(correcting_x0_fn=, thresholding_max_val=, dynamic_thresholding_ratio=), got {c!r}")
    extra = sorted(set(c) - set(CORRECTION_KEYS))
    if extra:
        raise ValueError(f"{what}: unknown keys {extra} (an x0 correction has {CORRECTION_KEYS})")
    name, ratio, max_val = c.get("correcting_x0_fn"), c.get("dynamic_thresholding_ratio", 0.995), c.get("thresholding_max_val", 1.0)
    try:
        mode = check_x0_correction(name, ratio, max_val, names_only=True)
    except ValueError as e:
        raise ValueError(f"{what}: {e}") from None
    return None if mode == 0 else (name, float(ratio), float(max_val))


def check_item_schedule(spec: Tuple, who: Optional[str], n_betas: int, corrected: bool) -> None:
    """The two rules every item's schedule ``spec`` = ``schedule_key(...)`` obeys wherever it runs: ddim / ddpm take no x0 correction, and ddpm
    runs every timestep.  ``who`` words the refusal as its caller always has: None = the call's own schedule, ``"schedules[b]"`` /
    ``"corrections[b]"`` = item b of ``sample``, ``"slot"`` / ``"correction"`` = a slot loop's request under the loop-wide / its own correction."""
    solver, steps = spec[0], spec[1]
    at = f"{who}: " if who not in (None, "slot") else ""
    if corrected and solver in DISCRETE_SOLVERS:
        if who in ("slot", "correction"):
            raise ValueError(f"{at}correcting_x0_fn applies to unipc / dpmsolver++ only, not {solver!r}" +
                             (" (ddim / ddpm have no correction)" if who == "correction" else ""))
        own = ": ddim / ddpm have no correction" if who is not None and who.startswith("corrections") else ""
        raise ValueError(f"{at}correcting_x0_fn applies to unipc / dpmsolver++ only (the reference's {solver} sampler has no correction{own})")
    if solver == "ddpm" and steps != n_betas:
        raise ValueError(f"{at}ddpm runs every timestep of the schedule: steps must be {n_betas}{' (or None)' if who is None else ''}, got {steps}")


def call_wide_kwargs(solver, correcting_x0_fn=None, thresholding_max_val=1.0, dynamic_thresholding_ratio=0.995, guidance_scale=1.0,
                     unconditional_prompt=None, **more) -> dict:
    """The call-wide x0 correction and guidance keywords a converter or pipeline passes through to every ``Denoiser.sample`` call: the correction
    where one is named (checked; refused for ``solver`` ddim / ddpm -- None: every request is checked on its own), the guidance where there is
    an unconditional prompt (``more``: its mask / lengths)."""
    kw = {}
    if check_x0_correction(correcting_x0_fn, dynamic_thresholding_ratio, thresholding_max_val, names_only=True):
        check_item_schedule((solver, 0), "slot", 0, True)
        kw.update(correcting_x0_fn=correcting_x0_fn, thresholding_max_val=thresholding_max_val, dynamic_thresholding_ratio=dynamic_thresholding_ratio)
    if unconditional_prompt is not None:
        kw.update(guidance_scale=guidance_scale, unconditional_prompt=unconditional_prompt, **more)
    return kw


def check_guidance(B: int, guidance_scale=1.0, unconditional_prompt=None, unconditional_prompt_mask=None, unconditional_prompt_lengths=None,
                   unconditional_content=None) -> Optional[np.ndarray]:
    """The argument errors of the guidance keywords (``sample``, ``denoise``) -> the (B,) float32 scales of a guided call, or None where nothing
    guided runs: no unconditional prompt, or every scale 1 (the reference's short cut, sampler/uni_pc.py:222-223)."""
    g = host_array(guidance_scale)
    if g.ndim > 1 or (g.ndim == 1 and g.shape[0] != B) or g.dtype.kind not in "fiu":
        raise ValueError(f"guidance_scale must be a float or hold one scale per item ({B},), got shape {tuple(g.shape)}")
    g = np.array(np.broadcast_to(g.astype(np.float32), (B,)))      # (a writable copy)
    if not np.all(np.isfinite(g)):
        raise ValueError("guidance_scale must be finite")
    if unconditional_prompt is None or np.all(g == 1.0):
        g = None
    if unconditional_prompt is None:
        if unconditional_prompt_mask is not None or unconditional_prompt_lengths is not None or unconditional_content is not None:
            raise ValueError("unconditional_prompt_mask / _lengths / unconditional_content need an unconditional_prompt")
        return g
    if len(unconditional_prompt.shape) != 3 or unconditional_prompt.shape[0] not in (1, B):
        raise ValueError(f"unconditional_prompt must be ({B} | 1, Lu, C), got {tuple(unconditional_prompt.shape)}")
    if unconditional_prompt_mask is not None and (tuple(unconditional_prompt_mask.shape) not in
                                                  ((1, unconditional_prompt.shape[1]), (B, unconditional_prompt.shape[1]))):
        raise ValueError(f"unconditional_prompt_mask must be ({B} | 1, {unconditional_prompt.shape[1]}), got {tuple(unconditional_prompt_mask.shape)}")
    if unconditional_prompt_lengths is not None and host_array(unconditional_prompt_lengths).reshape(-1).shape[0] not in (1, B):
        raise ValueError(f"unconditional_prompt_lengths must hold {B} (or 1) entries, got {host_array(unconditional_prompt_lengths).reshape(-1).shape[0]}")
    if unconditional_content is not None and unconditional_content.shape[0] != B:
        raise ValueError(f"unconditional_content must hold {B} items, got {unconditional_content.shape[0]}")
    return g


# default number of trailing fp32 evaluations of a 16-bit sampling loop, per solver (``Denoiser(tail_fp32=None)``):
# DPM-Solver++(2M) takes its LAST update at second order over the largest log-SNR step of the schedule (no lower_order_final
# for steps >= 10, dpm_solver.py:1198-1201), which amplifies the rounding noise of the last two evaluations ~2.7x (50 steps:
# fp16 1.7e-3 on the sampled latent, with the last two evaluations in fp32 ~2e-4); UniPC-bh2 ends at first order and keeps
# the single-evaluation noise (8.6e-4 at 20 steps), so it stays pure 16-bit unless asked.  DDPM and DDIM end on x_start of their
# last evaluation (weight ~1), so that evaluation's rounding is the latent's: at the bench shape fp16 DDPM-1000 / DDIM-100 are
# 7.7e-4 from the fp32 engine with no tail (worst item 8.0e-4), 1.4e-4 / 1.3e-4 with one fp32 evaluation, 6.7e-5 / 7.5e-5 with two
# (profiles/r08_stochastic.txt): one is the smallest tail that holds the 1e-3 bar with margin.
DEFAULT_TAIL_FP32 = {"dpmsolver++": 2, "unipc": 0, "ddim": 1, "ddpm": 1}
# ... and for order-3 tables, from tools/solver_bench.py at the bench shape, 20 steps, fp16 against the fp32 engine (profiles/r08_order3_solvers.txt).
# UniPC-3 ends at first order like UniPC-2 and has its rounding: 7.6e-4 with no tail, but 1.4e-3 on the worst frame; one fp32 evaluation
# gives 1.6e-4 (worst frame 3.6e-4), the smallest tail with margin, as for DDPM / DDIM.  DPM-Solver++(3M) takes its last updates at third
# order over the largest log-SNR steps (no lower_order_final for steps >= 10, as the reference), and each extrapolates from three model
# values, so the rounding of the last four evaluations reaches the latent: tail 0 / 1 / 2 / 3 / 4 give 7.6e-3 / 7.5e-3 / 4.5e-3 / 1.2e-3 /
# 3.1e-4 (worst item 3.3e-4, worst frame 7.4e-4).  Four is the smallest tail inside the bar.
DEFAULT_TAIL_FP32_ORDER3 = {"dpmsolver++": 4, "unipc": 1}


def default_tail_fp32(solver: str, order: int) -> int:
    """trailing fp32 evaluations of a 16-bit loop when the caller sets none"""
    return (DEFAULT_TAIL_FP32_ORDER3 if order == 3 and solver in DEFAULT_TAIL_FP32_ORDER3 else DEFAULT_TAIL_FP32).get(solver, 0)


def guided_tail_extra(scales) -> int:
    """fp32 evaluations a guided 16-bit loop adds to its default tail.  A guided x0 is (1 - s) x0_u + s x0_c of two evaluations whose 16-bit
    rounding errors are independent, so it carries g = sqrt((1 - s)^2 + s^2) times the error of one (2.9 at s = 2.5, 9.2 at s = 7; <= 1 for
    s in [0, 1]), and the last evaluations set the error of the sampled latent (class docstring of ``Denoiser``).  Every fp32 evaluation at
    the end of a loop lowers that error about threefold or more (1.12e-3 -> 3.5e-4 -> 8.2e-5 for UniPC at s = 2.5), so
    ceil(log3 g) of them offset the gain of the largest scale."""
    s = np.asarray(scales, dtype=np.float64).reshape(-1)
    g = float(np.sqrt((1.0 - s) ** 2 + s ** 2).max()) if s.size else 1.0
    return 0 if g <= 1.0 else int(np.ceil(np.log(g) / np.log(3.0) - 1e-9))


# relative L2 of ONE evaluation of a 16-bit engine against the exact result at the bench shape (README "parity"; bf16: the upper end of the
# 6.4e-3 .. 7.0e-3 that tests/test_engine_gpu.py measures), and the bar a sampled latent is held to
EVALUATION_ERROR = {"fp16": 7.2e-4, "bf16": 7.0e-3}
PARITY_BAR = 1e-3


def corrected_tail_min(precision: str, scales=None) -> int:
    """fewest trailing fp32 evaluations of a 16-bit loop that runs an x0 correction (``correcting_x0_fn``).  A corrected model value is
    clamp(m, -s, s) / s with s an order statistic of the same evaluation's |m|, so the 16-bit rounding of an evaluation reaches it twice:
    d(m / s) = dm / s - m ds / s^2, the element's own error and the threshold's, which moves every element of the item the same way and is not
    averaged down over the item.  Each is bounded by one evaluation's relative error e1 (``EVALUATION_ERROR``), so a corrected last evaluation
    carries up to g e1 with g = 2 (times sqrt((1 - s)^2 + s^2) of the largest guidance scale, as ``guided_tail_extra``), and every fp32
    evaluation at the end of a loop lowers the latent's error about threefold (same docstring).  ceil(log3(g e1 / bar)) of them bring it under the
    bar: 1 for fp16 (2 x 7.2e-4 = 1.44e-3), 3 for bf16 (1.4e-2).  It is a floor under the default tail (+ ``guided_tail_extra``), not an
    addition: a default tail that already runs as many evaluations in fp32 needs no more."""
    e1 = EVALUATION_ERROR.get(precision)
    if e1 is None:
        return 0
    g = 2.0
    if scales is not None:
        s = np.asarray(scales, dtype=np.float64).reshape(-1)
        g *= max(1.0, float(np.sqrt((1.0 - s) ** 2 + s ** 2).max())) if s.size else 1.0
    return max(0, int(np.ceil(np.log(g * e1 / PARITY_BAR) / np.log(3.0) - 1e-9)))


def slot_tail_needed(precision: str, solver: str, order: int, scale: float = 1.0, corrected: bool = False) -> int:
    """trailing fp32 evaluations ``Denoiser.sample`` would give a request with this schedule at this precision (``default_tail_fp32`` +
    ``guided_tail_extra``, floored by ``corrected_tail_min``); a slot loop serves a request only when this is 0"""
    if precision == "fp32":
        return 0
    n = default_tail_fp32(solver, order)
    guided = float(scale) != 1.0
    if guided:
        n += guided_tail_extra([scale])
    if corrected:
        n = max(n, corrected_tail_min(precision, [scale] if guided else None))
    return n


def _item_list(v, B: int, name: str, entry: str):
    if not isinstance(v, (list, tuple)) or len(v) != B:
        raise ValueError(f"{name} must be a list of one {entry} (dict or None) per item ({B}), got "
                         f"{len(v) if isinstance(v, (list, tuple)) else type(v).__name__}")
    return v


@dataclass(frozen=True)
class SampleRequest:
    """One ``Denoiser.sample`` call after its checks: B items as the caller gave them, every short cut resolved.  Exactly one of ``schedule`` /
    ``tabs`` is set, at most one of ``corr`` / ``entries``; ``known`` is None where nothing is held."""
    content: object
    prompt: object
    prompt_mask: object
    noise: object
    lengths: object                       # as given (the engine takes sequences, arrays and tensors), or None = dense
    prompt_lengths: object
    seeds: object
    scales: Optional[np.ndarray]          # (B,) float32, or None = nothing guided runs
    uncond: Tuple                         # (unconditional_prompt, _mask, _lengths, unconditional_content)
    schedule: Optional[Tuple]             # (solver, steps, order, eta, table_options): the shared table ...
    tabs: Optional[ItemTables]            # ... or the per-item schedules
    corr: Optional[Tuple]                 # the call-wide x0 correction (name, ratio, max_val) ...
    entries: Optional[list]               # ... or one None | (name, ratio, max_val) per item
    known: object
    known_mask: Optional[np.ndarray]      # (B, T) bool
    use_graph: bool
    tail_fp32: Optional[int]
    generator: object

    @property
    def table_key(self) -> Tuple:
        return self.schedule if self.tabs is None else ("items", self.tabs.keys, tuple(int(v) for v in self.tabs.start))

    @property
    def solver_orders(self):
        """(solver, order) of every distinct schedule of the call"""
        return [(k[0], k[2]) for k in ([self.schedule] if self.tabs is None else self.tabs.keys)]

    @staticmethod
    def take(kw: dict, items, B: int) -> dict:
        """``kw`` (keywords of ``sample``, its four positional arguments included) for the ``items`` (a slice or a list of indices) of its B:
        every PER_ITEM_KEYS entry whose first dimension is B goes with its items; scalars, shared (1, ...) rows and call-wide keywords stay whole"""
        def part(v):
            if v is None or np.ndim(v) == 0:
                return v
            if isinstance(v, (list, tuple)):
                return v if len(v) != B else list(v[items]) if isinstance(items, slice) else [v[b] for b in items]
            if v.shape[0] != B:
                return v
            if isinstance(items, slice) or not hasattr(v, "detach"):
                return v[items]
            import torch
            return v[torch.as_tensor(items, device=v.device)]
        return {k: part(v) if k in PER_ITEM_KEYS else v for k, v in kw.items()}

    @classmethod
    def parse(cls, den, content, prompt, prompt_mask=None, noise=None, solver="unipc", steps=None, order=2, use_graph=True, generator=None,
              tail_fp32=None, lengths=None, eta=0.0, seeds=None, prompt_lengths=None, guidance_scale=1.0, unconditional_prompt=None,
              unconditional_prompt_mask=None, unconditional_prompt_lengths=None, unconditional_content=None, correcting_x0_fn=None,
              thresholding_max_val=1.0, dynamic_thresholding_ratio=0.995, schedules=None, corrections=None, known=None, known_mask=None,
              **options) -> "SampleRequest":
        """the argument errors of ``Denoiser.sample`` (ValueError; an unknown option: TypeError), raised before anything runs, and its two short
        cuts resolved: B equal ``corrections=`` are the call-wide correction, B equal ``schedules=`` the call's own schedule"""
        B, _, T = content.shape
        n_betas = len(den.betas64)
        uncond = (unconditional_prompt, unconditional_prompt_mask, unconditional_prompt_lengths, unconditional_content)
        scales = check_guidance(B, guidance_scale, *uncond)
        if solver not in SOLVERS:
            raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
        corr = (correcting_x0_fn, float(dynamic_thresholding_ratio), float(thresholding_max_val)) \
            if check_x0_correction(correcting_x0_fn, dynamic_thresholding_ratio, thresholding_max_val, names_only=True) else None
        if steps is None:
            steps = {"ddim": 100, "ddpm": n_betas}.get(solver, 20)   # model.py sample(): sampling_timesteps=100; p_sample_loop: every timestep

        def own_schedule(solver, steps, order, eta, options):
            """the checks of the call's own schedule -> its key"""
            check_item_schedule((solver, steps), None, n_betas, corr is not None)
            key = (solver, int(steps), order, eta, table_options(options))      # (unknown option names: TypeError)
            if eta != 0.0 and solver != "ddim":
                raise ValueError(f"eta is DDIM's noise scale (ddim_sampling_eta); solver {solver!r} takes none")
            if eta < 0.0:
                raise ValueError(f"eta must be >= 0, got {eta}")
            if seeds is not None and host_array(seeds).reshape(-1).shape[0] != B:
                raise ValueError(f"seeds must hold one seed per item ({B})")
            if (options or order != 2) and key != den._table_key:
                build_table(solver, int(steps), den._betas_for(solver), order, eta, **options)      # the table's own checks (order, skip_type, ...), host only
            return key

        schedule = own_schedule(solver, steps, order, eta, options)
        known, known_mask = cls._check_known(den, known, known_mask, B, T, lengths, corr is not None or corrections is not None)
        entries = None
        if corrections is not None:
            if correcting_x0_fn is not None:
                raise ValueError("corrections= (one x0 correction per item) and correcting_x0_fn= (one for the call) exclude each other")
            entries = [item_correction_entry(c, f"corrections[{b}]") for b, c in enumerate(_item_list(corrections, B, "corrections", "entry"))]
            if all(e == entries[0] for e in entries):      # one correction for everybody: the call-wide setting, its kernels and its bits
                corr, entries = entries[0], None
                if corr is not None:
                    check_item_schedule(schedule, None, n_betas, True)
        tabs = None
        if schedules is not None or entries is not None:
            own = dict(solver=solver, steps=int(steps), order=order, eta=eta, **options)
            specs = [dict(own) if sp is None else sp for sp in _item_list([None] * B if schedules is None else schedules, B, "schedules", "schedule")]
            keys = []
            for b, sp in enumerate(specs):
                keys.append(schedule_key(sp, b))
                check_item_schedule(keys[b], f"schedules[{b}]", n_betas, corr is not None)
            if entries is None and all(k == keys[0] for k in keys):      # one schedule for everybody: the shared-table loop, its kernels and its bits
                schedule = own_schedule(*keys[0][:4], dict(keys[0][4]))
            else:
                for b, k in enumerate(keys):
                    check_item_schedule(k, f"corrections[{b}]", n_betas, entries is not None and entries[b] is not None)
                # (under corrections= the table reads item records: one schedule B times is deduplicated)
                schedule, tabs = None, build_tables(specs, den.betas, den.betas64)
        return cls(content, prompt, prompt_mask, noise, lengths, prompt_lengths, seeds, scales, uncond, schedule, tabs, corr, entries, known, known_mask,
                   use_graph, tail_fp32, generator)

    @staticmethod
    def _check_known(den, known, known_mask, B: int, T: int, lengths, corrected: bool):
        """the argument errors of ``known=, known_mask=`` -> (known, mask (B, T) numpy bool), or (None, None) where nothing is held: neither given,
        or an all-False mask"""
        if known is None and known_mask is None:
            return None, None
        if known is None or known_mask is None:
            raise ValueError("known= (the latent) and known_mask= (its frames) are given together")
        m = host_array(known_mask)
        if m.shape != (B, T) or m.dtype != np.bool_:
            raise ValueError(f"known_mask must be a bool ({B}, {T}), got {m.dtype} {tuple(m.shape)}")
        if tuple(known.shape) != (B, den.cfg.latent_channels, T):
            raise ValueError(f"known must be ({B}, {den.cfg.latent_channels}, {T}), got {tuple(known.shape)}")
        if not m.any():      # nothing held: the call without them, a correction included
            return None, None
        if corrected:
            raise ValueError("known frames do not run with an x0 correction (correcting_x0_fn= / corrections=): it would rescale the held frames")
        if lengths is not None:
            L = host_array(lengths).reshape(-1)
            if L.shape[0] != B:
                raise ValueError(f"lengths must hold one entry per item ({B}), got {L.shape[0]}")
            for b in range(B):
                if m[b, max(int(L[b]), 0):].any():
                    raise ValueError(f"known_mask[{b}] holds frame {int(np.nonzero(m[b])[0][-1])}, at or past lengths[{b}] = {int(L[b])}")
        return known, np.ascontiguousarray(m)

