"""High-level denoiser sampling API on torch CUDA tensors (torch = memory/stream plumbing).

This is what a maintainer calls from ``NaturalSpeech2.sample`` instead of the
reference's per-step Python loop (``model.py:620-687``): the step-invariant
condition work is hoisted once, the N-step DPM-Solver++ / UniPC loop replays one
captured hipGraph per step, and nothing synchronises with the host until the end.
"""
from __future__ import annotations

import warnings
from dataclasses import replace
from typing import Dict, Optional

import numpy as np

from . import dist as _dist
from .engine import DEFAULT_PRECISION, Engine
from .noise import draw_seeds
from .request import CORRECTION_KEYS, SampleRequest, call_wide_kwargs, check_guidance, check_item_schedule, host_array, item_correction_entry
from .schedule import (DISCRETE_SOLVERS, ITEM_HIST2, ITEM_NOISE, TablePool, build_table, check_x0_correction, known_start_torch, linear_betas,
                       schedule_key, table_flags, table_options)
from .spec import UNetConfig, attention_workgroups_per_forward

# The engine options that keep a ragged batch (``lengths=``) on its fused launches: each is a constructor parameter of ``Denoiser`` of the same
# name (default off), reaches the 16-bit engine and the fp32 engine of the tail / self-check alike, and is independent of the others.
MASKED_OPTIONS = (
    "masked_fuse",      # the plan keeps its fused launches where the kernels mask their own rows
    "masked_attn",      # the attention launches skip the keys and query tiles past an item's end themselves (no key-bias row, no sweeper launch)
    "masked_rows",      # the transformer blocks keep their two row-chain launches, which zero the rows past an item's end themselves (the fp32
                        # engine has no row chains and ignores it)
    "masked_ffn",       # the dim-128 / 256 transformer blocks keep the pre-stage launch of the fused feed-forward, which zeroes the rows past an
                        # item's end itself (the fp32 engine ignores it)
    "masked_geglu",     # the dim-384 transformer blocks keep the token-stationary GEGLU launch, which takes the LayerNorm sums from its own
                        # operand rows and zeroes the rows past an item's end itself
)


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



# LayerNorm-by-linearity guard thresholds on max |mean|/std (see Denoiser): 16-bit modes lose ~ratio * 2^-11 on a row,
# fp32 loses ~ratio^2 * 2^-24 in the variance E[x^2] - mean^2
LN_GUARD_DEFAULT = {"fp16": 8.0, "bf16": 8.0, "fp32": 32.0}


class Denoiser:
    """``precision``: "fp16" (default: 16-bit MFMA operands, 7e-4 vs the reference fp32 path -- inside the 1e-3 parity
    bar), "fp32" (exact-fp32 MFMA, 1e-6) or "bf16" (same speed as fp16, 5.7e-3; kept for range-critical checkpoints).

    ``tail_fp32``: evaluations at the END of every sampling loop that run on a second, fp32 engine (the solver state is
    handed over on the device, ``Engine.sample(tail=...)``).  None = ``DEFAULT_TAIL_FP32[solver]`` for the 16-bit
    precisions (2 for DPM-Solver++, 0 for UniPC; order 3: ``DEFAULT_TAIL_FP32_ORDER3``, 4 and 1), 0 = never.  The fp32 engine (weights + workspace) is built on first use.

    ``ln_guard``: LayerNorm by linearity (the default plan) lets the 16-bit modes round a LayerNorm's RAW input before
    centring, so their error on a row grows with |mean| / std of that row (and the fp32 variance E[x^2] - mean^2 with its
    square).  The engine records the maximum of that ratio.  It is read after the FIRST evaluation with a new shape /
    set of weights (one wait on the denoiser's stream; above the threshold the plan is switched to explicit LayerNorm
    passes, ``ln_linear`` 0: ~4 % slower, immune, and the evaluation is repeated) and, because the ratio also depends on
    the content, the prompt and the timestep, after EVERY later call without blocking: the read-out is enqueued behind
    the call and collected at the start of the next one (``ln_ratio_seen`` = running maximum); a late excess switches
    the plan for all following calls and warns that the previous result was computed above the threshold.
    ``None`` disables the check; a float sets the threshold (default 8 for the 16-bit modes, 32 for fp32).

    ``precision_check``: the 7e-4 of the fp16 mode was measured on procedural weights; a trained checkpoint with a few hot
    channels can land on either side of the 1e-3 bar (or saturate fp16 operands outright).  So a 16-bit Denoiser MEASURES
    itself ONCE PER SET OF WEIGHTS (the first call; ``recheck_precision()`` forces another): evaluations are run on the 16-bit
    engine and on the exact-fp32 engine (pinned to the reference at 1e-6) on the caller's own inputs.  ``sample`` checks at
    THREE points of its own trajectory -- the first, the middle and the last evaluation point of the loaded table (x_e taken
    from a preliminary 16-bit loop; the last evaluations are the ones that set the sampled latent) --, ``denoise`` at the
    given (x, t).  Two figures are kept and BOTH gated against ``precision_check`` (default 1e-3 for fp16; None disables;
    bf16: 2e-2, its own level): the relative L2 over the batch -- the parity bar's own measure -- in ``precision_error_seen``
    and the worst single utterance in ``precision_error_worst_item`` (maxima over the points; ``precision_errors`` has the
    per-point list).  Above it the Denoiser warns and serves this and all later calls from the fp32 engine (3.6x the step time,
    inside the bar by construction).  The verdict belongs to the weights, not to a shape: new shapes do NOT repeat it (they
    used to: an fp32 re-prepare, two extra forwards and two host waits per group of ``GroupedConverter``), and the fp32 engine is
    released again after a passed check unless a tail needs it (it is rebuilt on demand).

    ``attn_fallback_limit`` (r4): the 16-bit attention kernels first run an optimistic pass without the per-tile maximum (-10 % of their time) and
    repeat a workgroup exactly when a row's scores rose far above its first 64 keys.  With procedural weights that never happens; on a
    checkpoint with sharp attention it can: measured at the bench shape, 1 % of such rows sends 66 % of the workgroups through both passes
    (86 us instead of 45 per launch; the exact pass alone takes 50).  So the first loop / evaluation with a set of weights reads the engine's
    fallback counter (one host wait, once) and, above this share of workgroups (default 0.10, about the break-even), switches the engine to
    ``attn_optimistic`` 0 with a warning; ``attn_fallback_rate_seen`` keeps the measured share.  None disables."""

    def __init__(self, state: Dict[str, object], cfg: UNetConfig = UNetConfig(), precision: str = DEFAULT_PRECISION,
                 betas: Optional[np.ndarray] = None, ln_guard: Optional[float] = -1.0, tail_fp32: Optional[int] = None,
                 precision_check: Optional[float] = -1.0, attn_fallback_limit: Optional[float] = 0.10, masked_fuse: bool = False,
                 masked_attn: bool = False, masked_rows: bool = False, masked_ffn: bool = False, masked_geglu: bool = False):
        given = locals()
        self.cfg = cfg
        for name in MASKED_OPTIONS:
            setattr(self, name, bool(given[name]))
        self.attn_fallback_limit = attn_fallback_limit if precision not in ("fp32", "f32") else None
        self.attn_fallback_rate_seen: Optional[float] = None
        self._attn_checked = False
        self.precision = {"f32": "fp32", "f16": "fp16"}.get(precision, precision)
        self.engine = Engine(cfg, precision=precision)
        self.engine.load_state_dict(state)
        self._masked_options(self.engine)
        self._state = state
        self.betas = linear_betas() if betas is None else np.asarray(betas, dtype=np.float32)
        # ddim / ddpm index the model's own float32 buffers, which the reference derives from the float64 betas
        self.betas64 = linear_betas(dtype=np.float64) if betas is None else np.asarray(betas, dtype=np.float64)
        self._shape = None
        self._table_key = None
        self.ln_guard = LN_GUARD_DEFAULT[self.precision] if (ln_guard is not None and ln_guard < 0) else ln_guard
        self.ln_ratio_seen: Optional[float] = None
        self._ln_checked = False
        self._ln_pending = False
        self._ln_switched = False
        self.tail_fp32 = tail_fp32
        self.tail_engine: Optional[Engine] = None
        if precision_check is not None and precision_check < 0:
            precision_check = {"fp16": 1e-3, "bf16": 2e-2}.get(self.precision)
        self.precision_check = precision_check if self.precision != "fp32" else None
        self.precision_error_seen: Optional[float] = None
        self.precision_error_worst_item: Optional[float] = None
        self.precision_errors: list = []          # [(timestep, batch rel-L2, worst utterance)] of the last self-check
        self._precision_checked = False
        self.serving_fp32 = False        # set by a failed precision check: every call then runs on the fp32 engine
        self._tail_shape = None
        self._tail_table_key = None

    # ---- LayerNorm-by-linearity guard ---------------------------------------------------------------------------------
    def _note_ratio(self, r: float) -> bool:
        self.ln_ratio_seen = r if self.ln_ratio_seen is None else max(self.ln_ratio_seen, r)
        return self.ln_guard is not None and r > self.ln_guard

    def _switch_plan(self, r: float, late: bool) -> None:
        warnings.warn(f"LayerNorm inputs with |mean|/std up to {r:.1f} (> {self.ln_guard}): switching the "
                      f"{self.engine.precision} engine to explicit LayerNorm passes (ln_linear=0)" +
                      ("; the PREVIOUS result was computed above the threshold" if late else ""))
        self.engine.set_option("ln_linear", False)
        if self.tail_engine is not None:     # the fp32 engine loses ~ratio^2 * 2^-24 under the same plan: switch it too
            self.tail_engine.set_option("ln_linear", False)
            self._tail_shape = None
        self._ln_switched = True
        self._shape = None
        self._ln_checked = True          # the explicit plan does not depend on the ratio
        self.ln_guard = None

    def _guard_before(self) -> None:
        """collect the read-out enqueued behind the previous call (non-blocking)"""
        if self.ln_guard is None or not self._ln_pending:
            return
        r = self.engine.ln_ratio_poll()
        if r is None:
            return
        self._ln_pending = False
        if self._note_ratio(r):
            self._switch_plan(r, late=True)

    def _guard_after(self, stream, redo):
        if self.ln_guard is None:
            return None
        if not self._ln_checked:         # first call on this plan: wait for the value, repeat the call if it is too large
            self._ln_checked = True
            r = self.engine.ln_ratio(stream)
            if self._note_ratio(r):
                self._switch_plan(r, late=False)
                return redo()
            return None
        if not self._ln_pending:         # later calls: enqueue, collect next time
            self.engine.ln_ratio_post(stream)
            self._ln_pending = True
        return None

    def _prepare(self, B: int, T: int, Lp: int) -> None:
        if self._shape != (B, T, Lp):
            import torch
            torch.cuda.synchronize()
            self.engine.prepare(B, T, Lp)
            self._shape = (B, T, Lp)
            self._ln_checked = False                # a new shape is a new set of rows: check synchronously once
            self._ln_pending = False

    def _masked_options(self, eng) -> None:
        for name in MASKED_OPTIONS:      # (the defaults reach no engine)
            if getattr(self, name):
                eng.set_option(name, True)

    def set_option(self, name: str, value: bool) -> None:
        """A plan option of the engine (``Engine.set_option``; e.g. ``gn_coop`` off for a pipeline that runs the denoiser on a CU partition).
        The plan and the sampler table are rebuilt by the next ``sample``."""
        self.engine.set_option(name, value)
        if name in MASKED_OPTIONS:
            setattr(self, name, bool(value))
            if self.tail_engine is not None:
                self.tail_engine.set_option(name, value)
                self._tail_shape = None
                self._tail_table_key = None
        self._shape = None
        self._table_key = None

    @staticmethod
    def _correct(eng, corr, entries=None, stream=None) -> None:
        """The x0 correction on ``eng`` in the form the call has it: ``entries`` = the per-item table, one None or (correcting_x0_fn, ratio,
        max_val) per loop item (set the guidance first), else ``corr`` = the loop-wide (correcting_x0_fn, ratio, max_val) or None.  The other
        form goes off first (the two exclude each other), and so do known frames an earlier call left on (the engine refuses the pair);
        nothing reaches an engine that is off and stays off."""
        other = eng.x0_correction if entries is not None else eng.x0_corrections
        if other is not None:
            eng.set_x0_correction(None) if entries is not None else eng.set_x0_correction_items(None)
        if (entries is not None or corr is not None) and eng.hold is not None:
            eng.set_known(None, None)
        if entries is not None:
            eng.set_x0_correction_items([None if e is None else e[0] for e in entries], [0.995 if e is None else e[1] for e in entries],
                                        [1.0 if e is None else e[2] for e in entries], stream=stream)
        elif corr is not None:
            eng.set_x0_correction(*corr)
        elif eng.x0_correction is not None:
            eng.set_x0_correction(None)

    def _setup(self, eng, req: SampleRequest, stream, table_key_attr: str, seeds=None):
        """The sampler state of ``req`` on ``eng`` -- the 16-bit head (``_table_key``) and the fp32 tail (``_tail_table_key``) alike, in the one
        order the engine wants: guidance (the per-item records below cover the loop's items), x0 correction (the schedules are checked against
        it when they load), table, seeds.  Returns the seeds of a stochastic loop (``seeds``, the request's, or drawn from its generator: pass
        them to the other engine), None for a deterministic one."""
        if req.scales is not None or eng.guidance is not None:
            eng.set_guidance(req.scales, stream=stream)
        self._correct(eng, req.corr, req.entries, stream)
        key = req.table_key
        if req.tabs is not None and eng is not self.engine:      # (the tail alone has always loaded its records again when the guidance came or went)
            key += (None if req.scales is None else len(req.scales),)
        if getattr(self, table_key_attr) != key:
            if req.tabs is not None:
                eng.load_samplers(req.tabs, stream=stream)
            else:
                solver, steps, order, eta, options = req.schedule
                eng.load_sampler(solver, steps, self._betas_for(solver), order, eta, **dict(options))
            setattr(self, table_key_attr, key)
        if not (self._loop_table(eng).coef[:, 9] != 0).any():
            return None
        if seeds is None:
            seeds = req.seeds if req.seeds is not None else draw_seeds(req.content.shape[0], req.generator)
        eng.set_seeds(seeds, stream=stream)
        return seeds

    def _bind(self, eng, cond, stream) -> None:
        """the condition of a call on ``eng``: ``cond`` = (content, prompt, mask, lengths, prompt_lengths, known, known_mask).  The known frames
        go behind the lengths: set, or switched off where an earlier call left them on"""
        self._condition(eng, *cond[:3], stream, *cond[3:5])
        if cond[5] is not None or eng.hold is not None:
            eng.set_known(cond[5], cond[6], stream=stream)

    def _betas_for(self, solver: str) -> np.ndarray:
        return self.betas64 if solver in DISCRETE_SOLVERS else self.betas

    @staticmethod
    def _loop_table(eng):
        """the loaded loop of ``eng``: the per-item schedules, or the shared table"""
        return eng.tables if eng.tables is not None else eng.table

    def _fp32_engine(self) -> Engine:
        """the exact-fp32 engine (tail of a 16-bit loop, precision self-check, fallback), prepared for the current shape"""
        if self.tail_engine is None:
            self.tail_engine = Engine(self.cfg, precision="fp32")
            self.tail_engine.load_state_dict(self._state)
            if self._ln_switched:
                self.tail_engine.set_option("ln_linear", False)
            self._masked_options(self.tail_engine)
            self._tail_shape = None
            self._tail_table_key = None
        if self._tail_shape != self._shape:
            import torch
            torch.cuda.synchronize()
            self.tail_engine.prepare(*self._shape)
            self._tail_shape = self._shape
        return self.tail_engine

    def _tail(self, n_tail: int) -> Optional[Engine]:
        """the fp32 engine if a loop with ``n_tail`` trailing fp32 evaluations needs one -- to finish a 16-bit loop, or to run all of it after a
        failed precision check --, else None"""
        return self._fp32_engine() if (n_tail > 0 or self.serving_fp32) and self.precision != "fp32" else None

    def _default_tail(self, req: SampleRequest) -> int:
        """trailing fp32 evaluations of ``req`` where neither the call nor the instance sets them: the largest tail any item's own schedule asks
        for (right-aligned, the last k loop steps are every item's last); guidance multiplies the 16-bit rounding of the last evaluations
        (``guided_tail_extra``), and a correction lets it in twice (``corrected_tail_min``)"""
        if self.precision == "fp32":
            return 0
        n = max(default_tail_fp32(solver, order) for solver, order in req.solver_orders)
        if req.scales is not None:
            n += guided_tail_extra(req.scales)
        if req.corr is not None or req.entries is not None:
            n = max(n, corrected_tail_min(self.precision, req.scales))
        return n

    def _attn_check(self, evals: int, stream) -> None:
        """once per set of weights: share of attention workgroups that needed the exact fallback during the last ``evals`` evaluations"""
        if self.attn_fallback_limit is None or self._attn_checked or evals <= 0:
            return
        self._attn_checked = True
        B, T, _ = self._shape
        n = self.engine.attn_fallbacks(reset=True, stream=stream)
        self.attn_fallback_rate_seen = n / float(max(1, evals * attention_workgroups_per_forward(self.cfg, B, T)))
        if self.attn_fallback_rate_seen > self.attn_fallback_limit:
            warnings.warn(f"{100 * self.attn_fallback_rate_seen:.0f} % of the attention workgroups needed the exact fallback on this checkpoint / input "
                          f"(> {100 * self.attn_fallback_limit:.0f} %): each of them ran twice -- switching the engine to the exact pass only (attn_optimistic=0)")
            self.engine.set_option("attn_optimistic", False)
            self._shape = None

    def recheck_precision(self) -> None:
        """forget the verdict of the precision self-check (after the weights were changed in place): the next call measures again"""
        self._precision_checked = False
        self.serving_fp32 = False
        self._attn_checked = False

    def _self_check(self, points, c32, p32, mask, stream, keep_fp32: bool, lengths=None, prompt_lengths=None) -> None:
        """once per set of weights: the same evaluations on the 16-bit and on the fp32 engine (class docstring, ``precision_check``);
        ``points`` = [(x, t)] with x (B,100,T) fp32 and t (B,) fp32.  With ``lengths`` both engines return exact zeros past every item's
        end, so the per-utterance figures cover its valid frames only."""
        import torch
        if self.precision_check is None or self._precision_checked:
            return
        self._precision_checked = True
        e32 = self._fp32_engine()
        self._condition(self.engine, c32, p32, mask, stream, lengths, prompt_lengths)
        self._condition(e32, c32, p32, mask, stream, lengths, prompt_lengths)
        self.precision_errors = []
        err, worst = 0.0, 0.0
        for x, t in points:
            outs = []
            for eng in (self.engine, e32):
                o = torch.empty_like(x, dtype=torch.float32)
                eng.forward(x, t, o, stream=stream)
                outs.append(o)
            num = (outs[0] - outs[1]).flatten(1).norm(dim=1)
            den = outs[1].flatten(1).norm(dim=1).clamp_min(1e-30)
            finite = bool(torch.isfinite(outs[0]).all())
            # the parity bar's own measure: relative L2 over the whole batch; the worst single utterance beside it
            e_b = float(num.norm() / den.norm()) if finite else float("inf")
            e_w = float((num / den).max()) if finite else float("inf")
            self.precision_errors.append((float(t.flatten()[0]), e_b, e_w))
            err, worst = max(err, e_b), max(worst, e_w)
        self.precision_error_seen, self.precision_error_worst_item = err, worst
        if not (err <= self.precision_check and worst <= self.precision_check):
            warnings.warn(f"{self.precision} engine is {err:.2e} (relative L2 over the batch; worst utterance {worst:.2e}) from the exact-fp32 "
                          f"engine on this checkpoint / input (> {self.precision_check:g}): serving from the fp32 engine from now on "
                          f"(precision_check=None disables)")
            self.serving_fp32 = True
        elif not keep_fp32:      # passed and no tail wants it: do not keep a second set of weights + workspace resident
            self.tail_engine = None
            self._tail_shape = None
            self._tail_table_key = None

    @staticmethod
    def _condition(eng, c32, p32, mask, stream, lengths, prompt_lengths=None) -> None:
        """per-item valid frames and prompt frames (None = dense) first -- the padded content and prompt frames are zeroed by set_condition --
        then the condition"""
        eng.set_lengths(lengths, stream=stream)
        eng.set_prompt_lengths(prompt_lengths, stream=stream)
        eng.set_condition(c32, p32, mask, stream=stream)

    def _trajectory_points(self, x_T, use_graph, stream, rep: int = 1):
        """(x_e, t) at the first, middle and last evaluation of the loaded table, from a preliminary loop on the 16-bit engine
        (its condition must be set).  ``rep`` = 2 under guidance: the loop gives B items, the evaluations take the point in both halves."""
        import torch
        tabs = self.engine.tables      # per-item schedules: the points of the loop as run, t = every item's own model time there
        tm = None if tabs is not None else np.asarray(self.engine.table.t_model, dtype=np.float32)
        n = tabs.steps if tabs is not None else len(tm)
        idx = sorted({0, n // 2, n - 1})
        B = x_T.shape[0]
        pts, pos = [], 0
        self.engine.sample_begin(x_T, stream=stream)
        for i in idx:
            self.engine.sample_steps(i - pos, use_graph=use_graph, stream=stream)
            pos = i
            xe = torch.empty_like(x_T)
            self.engine.sample_peek(xe, stream=stream)
            t = torch.full((B * rep,), float(tm[i]), dtype=torch.float32, device=x_T.device) if tabs is None else \
                torch.from_numpy(np.tile(tabs.t_model_at(i), rep)).to(x_T.device)
            pts.append((xe if rep == 1 else xe.repeat(rep, 1, 1), t))
        scratch = torch.empty_like(x_T)
        self.engine.sample_end(scratch, stream=stream)
        return pts

    @staticmethod
    def _guided_condition(content, prompt, prompt_mask, lengths, prompt_lengths, unconditional_prompt, unconditional_prompt_mask,
                          unconditional_prompt_lengths, unconditional_content):
        """The condition of a guided call on the engine of 2B items: cat([unconditional, conditional]) as the reference batches it
        (sampler/uni_pc.py:222-229) for content, prompt, mask, latent lengths and prompt lengths.  Prompts of different lengths are
        zero-padded to the longer and every row gets its own frame count (``Engine.set_prompt_lengths``)."""
        import torch
        B, Lp, Lu = content.shape[0], prompt.shape[1], unconditional_prompt.shape[1]
        dev = content.device
        L = max(Lp, Lu)

        def pad(p, n):      # (b, l, ...) -> (b, n, ...) with zeros behind
            p = p.to(dev)
            return p if p.shape[1] == n else torch.cat([p, p.new_zeros((p.shape[0], n - p.shape[1]) + tuple(p.shape[2:]))], dim=1)

        def ints(v, n, fill):
            if v is None:
                return np.full((n,), fill, dtype=np.int32)
            return np.ascontiguousarray(np.broadcast_to(host_array(v).reshape(-1).astype(np.int32), (n,)))

        up = unconditional_prompt.float().expand(B, -1, -1)
        prompt2 = torch.cat([pad(up, L), pad(prompt.float(), L)], dim=0).contiguous()
        uc = content if unconditional_content is None else unconditional_content.to(dev)
        content2 = torch.cat([uc.float(), content.float()], dim=0).contiguous()
        mask2 = None
        if prompt_mask is not None or unconditional_prompt_mask is not None:
            um = torch.ones((B, Lu), dtype=torch.bool, device=dev) if unconditional_prompt_mask is None else unconditional_prompt_mask.to(dev).bool().expand(B, -1)
            cm = torch.ones((B, Lp), dtype=torch.bool, device=dev) if prompt_mask is None else prompt_mask.to(dev).bool()
            mask2 = torch.cat([pad(um, L), pad(cm, L)], dim=0).contiguous()
        plens2 = None
        if Lu != Lp or prompt_lengths is not None or unconditional_prompt_lengths is not None:
            plens2 = np.concatenate([ints(unconditional_prompt_lengths, B, Lu), ints(prompt_lengths, B, Lp)])
        lens2 = None if lengths is None else np.concatenate([ints(lengths, B, 0)] * 2)
        return content2, prompt2, mask2, lens2, plens2

    def denoise(self, x, t, content, prompt, prompt_mask=None, lengths=None, prompt_lengths=None, guidance_scale=1.0, unconditional_prompt=None,
                unconditional_prompt_mask=None, unconditional_prompt_lengths=None, unconditional_content=None):
        """One evaluation: x (B,100,T), t (B,), content (B,256,T), prompt (B,Lp,256), mask (B,Lp) bool -> x0_pred.
        ``lengths`` (B,) ints in [1, T] or None: item b is a segment of lengths[b] frames padded to T (``Engine.set_lengths``); its
        result on those frames is what it gives alone, and 0 beyond.
        ``prompt_lengths`` (B,) ints in [1, Lp] or None: item b's prompt is its first prompt_lengths[b] rows (``Engine.set_prompt_lengths``); its
        result is what it gives alone with that prompt and no mask, whatever the rows past them hold.
        ``guidance_scale`` (float or (B,)) with ``unconditional_prompt`` (B | 1, Lu, 256): classifier-free guidance -- ONE evaluation of the batch
        cat([unconditional, conditional]) of 2B items and ``schedule.guided_x0`` of its halves in torch (see ``sample`` for the keywords)."""
        import torch
        B, _, T = x.shape
        scales = check_guidance(B, guidance_scale, unconditional_prompt, unconditional_prompt_mask, unconditional_prompt_lengths, unconditional_content)
        if scales is not None:
            c2, p2, m2, l2, pl2 = self._guided_condition(content, prompt, prompt_mask, lengths, prompt_lengths, unconditional_prompt,
                                                         unconditional_prompt_mask, unconditional_prompt_lengths, unconditional_content)
            o = self.denoise(torch.cat([x, x], dim=0), torch.cat([t, t], dim=0), c2, p2, m2, l2, pl2)
            sc = torch.from_numpy(scales).to(o.device).view(B, 1, 1)
            return torch.where(sc == 1.0, o[B:], o[:B] + sc * (o[B:] - o[:B]))      # (the select of guided_x0)
        self._guard_before()
        self._prepare(B, T, prompt.shape[1])
        s = torch.cuda.current_stream(x.device)
        mask = None if prompt_mask is None else prompt_mask.to(torch.uint8).contiguous()
        c32, p32, x32, t32 = content.float().contiguous(), prompt.float().contiguous(), x.float().contiguous(), t.float().contiguous()
        self._self_check([(x32, t32)], c32, p32, mask, s, keep_fp32=bool(self.tail_fp32), lengths=lengths, prompt_lengths=prompt_lengths)
        eng = self._fp32_engine() if self.serving_fp32 else self.engine
        self._condition(eng, c32, p32, mask, s, lengths, prompt_lengths)
        out = torch.empty_like(x, dtype=torch.float32)
        first_attn = not self.serving_fp32 and not self._attn_checked and self.attn_fallback_limit is not None
        if first_attn:
            eng.attn_fallbacks(reset=True, stream=s)          # count this evaluation alone
        eng.forward(x32, t32, out, stream=s)
        if self.serving_fp32:
            return out
        redone = self._guard_after(s, lambda: self.denoise(x, t, content, prompt, prompt_mask, lengths, prompt_lengths))
        if first_attn and redone is None:
            self._attn_check(1, s)                            # (after the guard's read-out: a switch drops the plan)
        return out if redone is None else redone

    def sample(self, content, prompt, prompt_mask=None, noise=None, solver: str = "unipc", steps: Optional[int] = None, order: int = 2,
               use_graph: bool = True, generator=None, tail_fp32: Optional[int] = None, lengths=None, eta: float = 0.0, seeds=None,
               prompt_lengths=None, guidance_scale=1.0, unconditional_prompt=None, unconditional_prompt_mask=None,
               unconditional_prompt_lengths=None, unconditional_content=None, correcting_x0_fn=None, thresholding_max_val: float = 1.0,
               dynamic_thresholding_ratio: float = 0.995, schedules=None, corrections=None, known=None, known_mask=None, **options):
        """content (B,256,T), prompt (B,Lp,256), mask (B,Lp) bool; ``noise`` (B,100,T) = x_T (drawn with
        torch.randn like model.py:635 if None).  Returns the sampled latent (B,100,T) fp32.
        ``solver``: ``unipc`` | ``dpmsolver++`` (``order`` 1 | 2 | 3, multistep) or the reference's discrete samplers ``ddim`` (``eta`` =
        ddim_sampling_eta) | ``ddpm`` (p_sample_loop: steps = every timestep).  ``steps`` None: 20, ddim 100, ddpm len(betas).
        ``seeds`` (B,) ints: the per-item noise streams of ddpm / ddim with eta > 0 (ns2vc_amd.noise; item b's noise depends on
        seeds[b] alone), drawn from ``generator`` after x_T if None, so ``generator=`` reproduces a run.
        ``lengths`` (B,) ints in [1, T] or None: per-item valid frames of a padded batch (see ``denoise``); x_T is zeroed past them.
        ``prompt_lengths`` (B,) ints in [1, Lp] or None: per-item prompt frames of a batch whose prompts are padded to one Lp (see ``denoise``).
        ``tail_fp32`` overrides the instance's setting for this call (see the class docstring).
        ``guidance_scale`` (float or (B,) per item) with ``unconditional_prompt`` (B | 1, Lu, 256): classifier-free guidance, the reference's
        ``model_wrapper(guidance_type="classifier-free", condition, unconditional_condition, guidance_scale)`` (sampler/uni_pc.py:155-233)
        inside the captured loop: the engine (and the fp32 tail) run 2B items, cat([unconditional, conditional]), and every solver update
        combines ``x0_u + s * (x0_c - x0_u)`` (``schedule.guided_x0``) first.  ``unconditional_prompt_mask`` (B | 1, Lu),
        ``unconditional_prompt_lengths`` and ``unconditional_content`` (default: ``content``) describe the unconditional half; Lu may differ
        from Lp.  An item with scale 1 follows its unguided trajectory; with every scale 1, or no unconditional prompt, nothing guided runs
        and the call is today's B-item loop (uni_pc.py:222-223).
        ``correcting_x0_fn`` None | "dynamic_thresholding" | "clamp" with ``thresholding_max_val`` and ``dynamic_thresholding_ratio``: the
        constructor options of the reference's ``UniPC`` / ``DPM_Solver`` (uni_pc.py:236-294, dpm_solver.py:338-442) inside the captured loop,
        on the 16-bit engine and the fp32 tail alike (``Engine.set_x0_correction``, ``schedule.correct_x0``): every step corrects the (guided)
        predicted x0 in front of the update -- per item s = max(quantile_ratio(|x0|), max_val) over the item's own frames, clamp(x0, -s, s) / s;
        "clamp" is clamp(x0, -max_val, max_val), the common callable.  unipc / dpmsolver++ only; a callable, or anything else but these names,
        is refused (ValueError).  A 16-bit loop under a correction runs at least ``corrected_tail_min(precision, scales)`` trailing
        evaluations on the fp32 engine unless ``tail_fp32`` says otherwise (1 for fp16, 3 for bf16).
        ``options`` (keyword-only): the reference's ``UniPC.sample`` / ``DPM_Solver.sample`` keywords that ``schedule.build_table`` serves
        -- ``skip_type``, ``lower_order_final``, ``denoise_to_zero`` (one more evaluation), ``variant`` (UniPC), ``solver_type``
        (DPM-Solver++), ``t_start``, ``t_end``, ``method`` ("multistep" only).
        ``schedules``: a list of B per-item schedules -- dicts with the keys ``solver``, ``steps``, ``order``, ``eta`` and the ``options``
        above, or None = this call's own -- served by ONE captured loop of max(evaluations) steps (``Engine.load_samplers``,
        ``schedule.run_tables_numpy``): the items are right-aligned, a shorter item is held (evaluated, not updated) until its turn, and every
        item ends on what its schedule gives it in a call of its own.  B equal schedules take the shared-table path of that schedule.  The
        default ``tail_fp32`` is the largest any item's schedule asks for.
        ``corrections``: a list of B per-item x0 corrections -- None, or ``dict(correcting_x0_fn=, thresholding_max_val=,
        dynamic_thresholding_ratio=)`` with the names above -- instead of the call-wide ``correcting_x0_fn=`` (both: ValueError).  Item b is
        corrected by its own entry inside the one captured loop (``Engine.set_x0_correction_items``) and ends on the bits it has
        when its entry is the call-wide setting; a ddim / ddpm item takes None and may share the batch with corrected items.  B equal
        entries take the call-wide path of that entry.  The default ``tail_fp32`` counts the call as corrected when any item is.
        ``known`` (B,100,T) with ``known_mask`` (B,T) bool: known frames (``Engine.set_known``) -- on the frames of the mask the
        predicted x0 of every evaluation IS ``known`` (values off the mask are ignored), inside the captured loop on the 16-bit engine and the
        fp32 tail alike, under guidance in both halves.  x_T there is ``alpha_0 * known + sigma_0 * noise`` (``schedule.known_start``; under
        ``schedules=`` each item's own first row), so a held frame ends on ``alpha_end * known + sigma_end * noise`` -- on ``known`` itself with
        ``denoise_to_zero`` and for ddim -- while the free frames are generated next to it: the fixed context of ``sample_long``, or the part a
        partial re-synthesis keeps.  An all-False mask is the call without them.  Refused (ValueError): one of the pair without the other,
        wrong shapes, a held frame at or past ``lengths[b]``, and ``correcting_x0_fn=`` / ``corrections=``, which would rescale the held frames."""
        return self._run(SampleRequest.parse(
            self, content, prompt, prompt_mask, noise, solver, steps, order, use_graph, generator, tail_fp32, lengths, eta, seeds, prompt_lengths,
            guidance_scale, unconditional_prompt, unconditional_prompt_mask, unconditional_prompt_lengths, unconditional_content, correcting_x0_fn,
            thresholding_max_val, dynamic_thresholding_ratio, schedules, corrections, known, known_mask, **options))

    def _run(self, req: SampleRequest):
        """``sample`` behind its checks: guided condition, prepare, setup, x_T (noise, known start), self-check, tail, run, guard"""
        import torch
        B, _, T = req.content.shape
        dev = req.content.device
        content, prompt, prompt_mask, lengths, prompt_lengths = req.content, req.prompt, req.prompt_mask, req.lengths, req.prompt_lengths
        rep = 1
        if req.scales is not None:      # the engine's batch is cat([unconditional, conditional]); the loop still takes and gives B items
            content, prompt, prompt_mask, lengths, prompt_lengths = self._guided_condition(content, prompt, prompt_mask, lengths, prompt_lengths, *req.uncond)
            rep = 2
        self._guard_before()
        self._prepare(rep * B, T, prompt.shape[1])
        s = torch.cuda.current_stream(dev)
        noise = req.noise if req.noise is not None else torch.randn((B, self.cfg.latent_channels, T), device=dev, generator=req.generator)
        seeds = self._setup(self.engine, req, s, "_table_key")      # (drawn behind x_T, so ``generator=`` reproduces a run)
        table = self._loop_table(self.engine)
        nfe = table.steps      # (steps + 1 with denoise_to_zero; per-item schedules: the longest item's)
        n_tail = req.tail_fp32 if req.tail_fp32 is not None else self.tail_fp32
        n_tail = max(0, min(int(self._default_tail(req) if n_tail is None else n_tail), nfe))
        x = noise.to(device=dev, dtype=torch.float32).contiguous().clone()
        kn = None
        if req.known is not None:      # x_T of the known frames: alpha_0 k + sigma_0 noise in float32, by each item's own first table row (schedule.known_start)
            kn = req.known.to(device=dev, dtype=torch.float32).contiguous()
            x = known_start_torch(x, kn, req.known_mask, table.coef[0] if req.tabs is None else np.stack([req.tabs.table_of(b).coef[0] for b in range(B)]))
        mask = None if prompt_mask is None else prompt_mask.to(device=dev, dtype=torch.uint8).contiguous()
        cond = (content.float().contiguous(), prompt.float().contiguous(), mask, lengths, prompt_lengths, kn, req.known_mask)
        if self.precision_check is not None and not self._precision_checked:
            self._bind(self.engine, cond, s)
            self._self_check(self._trajectory_points(x, req.use_graph, s, rep), *cond[:3], s, keep_fp32=n_tail > 0, lengths=lengths,
                             prompt_lengths=prompt_lengths)
        tail = self._tail(n_tail)
        if tail is not None:
            self._setup(tail, req, s, "_tail_table_key", seeds)
        if self.serving_fp32:            # a failed precision check: the whole loop on the fp32 engine
            self._bind(tail, cond, s)
            tail.sample(x, use_graph=req.use_graph, stream=s)
            return x
        self._bind(self.engine, cond, s)
        if tail is not None:
            self._bind(tail, cond, s)      # (the hand-off wants the two engines to agree, as on the seeds)
        first_attn = not self._attn_checked and self.attn_fallback_limit is not None
        if first_attn:
            self.engine.attn_fallbacks(reset=True, stream=s)      # count this loop alone (the self-check's evaluations are behind us)
        self.engine.sample(x, use_graph=req.use_graph, stream=s, tail=tail, tail_steps=n_tail if tail is not None else 0)
        # (a redo runs the same request from the same x_T and seeds)
        redone = self._guard_after(s, lambda: self._run(replace(req, noise=noise, seeds=seeds if seeds is not None else req.seeds)))
        if first_attn and redone is None:
            self._attn_check(nfe - (n_tail if tail is not None else 0), s)      # (after the guard's read-out: a switch drops the plan)
        return x if redone is None else redone

    def sample_long(self, content, prompt, prompt_mask=None, noise=None, chunk_frames: int = 938, overlap_frames: int = 64, lengths=None,
                    **sample_kwargs):
        """Utterances longer than one engine shape: content (B,256,Ttot) is cut per item by ``schedule.plan_chunks(lengths[b] or Ttot,
        chunk_frames, overlap_frames)`` and chunk j + 1 is sampled with the last ``overlap_frames`` latent frames of chunk j as known frames
        (``sample(known=, known_mask=)``), so the model generates every new chunk next to latents it already committed to.
        Batch j holds the items that have a chunk j, padded to the longest of them; its ``lengths=`` are their chunk lengths (left out where
        every item fills the batch and the call has no ``lengths=``: the dense plan).  Each item's x_T is its slice of the full-length ``noise``
        (B,100,Ttot), drawn once from ``generator=`` if None.  Returns (B,100,Ttot): chunk 0 whole, then every later chunk from frame
        ``overlap_frames`` on -- the overlap frames are the earlier chunk's, which the later one held --, zero past ``lengths``.  With
        ``overlap_frames=0`` the chunks are independent; where no item has a second chunk this IS ``sample``.  ``sample_kwargs``: the call-wide
        keywords of ``sample`` (solver, steps, guidance, ...) for every chunk, the per-item ones (``seeds``, ``prompt_lengths``, a per-item
        ``guidance_scale``, the ``unconditional_*`` rows) sliced per batch, the seeds reused per chunk; ``schedules=``, ``corrections=``,
        ``known=`` and ``known_mask=`` are refused."""
        import torch
        from .schedule import plan_chunks
        B, _, Ttot = content.shape
        dev = content.device
        refused = ("schedules", "corrections", "known", "known_mask")
        for k in refused:
            if sample_kwargs.get(k) is not None:
                raise ValueError(f"sample_long takes call-wide options only (plus per-item seeds): {k}= is refused")
        kw = {k: v for k, v in sample_kwargs.items() if k not in refused}
        seeds = kw.pop("seeds", None)
        if seeds is not None:
            seeds = host_array(seeds).reshape(-1)
            if seeds.shape[0] != B:
                raise ValueError(f"seeds must hold one seed per item ({B}), got {seeds.shape[0]}")
        if lengths is None:
            L = np.full((B,), Ttot, dtype=np.int64)
        else:
            L = host_array(lengths).reshape(-1).astype(np.int64)
            if L.shape[0] != B or (L < 1).any() or (L > Ttot).any():
                raise ValueError(f"lengths must hold {B} entries in [1, {Ttot}]")
        V = int(overlap_frames)
        chunks = [plan_chunks(int(L[b]), chunk_frames, V) for b in range(B)]
        if noise is not None and tuple(noise.shape) != (B, self.cfg.latent_channels, Ttot):
            raise ValueError(f"noise must be ({B}, {self.cfg.latent_channels}, {Ttot}), got {tuple(noise.shape)}")
        if max(len(c) for c in chunks) == 1:      # nothing to chain: the plain call, its shapes and its bits
            return self.sample(content, prompt, prompt_mask, noise, lengths=lengths, seeds=seeds, **kw)
        if noise is None:
            noise = torch.randn((B, self.cfg.latent_channels, Ttot), device=dev, generator=kw.get("generator"))
        noise = noise.to(device=dev, dtype=torch.float32)
        out = torch.zeros((B, self.cfg.latent_channels, Ttot), dtype=torch.float32, device=dev)
        min_t = 2 ** (len(self.cfg.block_out_channels) - 1)      # (the shortest T the engine prepares)

        per_item = dict(kw, prompt=prompt, prompt_mask=prompt_mask, seeds=seeds)      # (the frames of content, noise and unconditional_content are cut below)
        for j in range(max(len(c) for c in chunks)):
            items = [b for b in range(B) if len(chunks[b]) > j]
            span = [chunks[b][j] for b in items]
            Lj = [stop - start for start, stop in span]
            Tj = max(max(Lj), min_t)
            c_j = content.new_zeros((len(items), content.shape[1], Tj))
            n_j = noise.new_zeros((len(items), self.cfg.latent_channels, Tj))
            for i, (b, (start, stop)) in enumerate(zip(items, span)):
                c_j[i, :, :stop - start] = content[b, :, start:stop]
                n_j[i, :, :stop - start] = noise[b, :, start:stop]
            kw_j = SampleRequest.take(per_item, items, B)
            uc = kw_j.get("unconditional_content")
            if uc is not None:
                kw_j["unconditional_content"] = uc.new_zeros((len(items), uc.shape[1], Tj))
                for i, (start, stop) in enumerate(span):
                    kw_j["unconditional_content"][i, :, :stop - start] = uc[i, :, start:stop]
            if j > 0 and V > 0:      # the frames the earlier chunk ended on, held at the head of this one
                k_j = out.new_zeros((len(items), self.cfg.latent_channels, Tj))
                m_j = np.zeros((len(items), Tj), dtype=bool)
                for i, (b, (start, stop)) in enumerate(zip(items, span)):
                    k_j[i, :, :V] = out[b, :, start:start + V]
                    m_j[i, :V] = True
                kw_j.update(known=k_j, known_mask=m_j)
            ragged = lengths is not None or any(l != Tj for l in Lj)
            x_j = self.sample(c_j, noise=n_j, lengths=np.asarray(Lj, dtype=np.int32) if ragged else None, **kw_j)
            for i, (b, (start, stop)) in enumerate(zip(items, span)):
                keep = V if j > 0 else 0
                out[b, :, start + keep:stop] = x_j[i, :, keep:stop - start]
        return out

    def open_slots(self, B: int, T: int, Lp: int, order3: bool = False, stochastic: bool = False, unconditional_prompt=None,
                   correcting_x0_fn=None, thresholding_max_val: float = 1.0, dynamic_thresholding_ratio: float = 0.995,
                   use_graph: bool = True, require_tail_free: bool = True, item_corrections: bool = False,
                   known_frames: bool = False) -> "SlotLoop":
        """Continuous batching: a ``SlotLoop`` over an engine prepared for B slots of up to T frames and Lp prompt frames, whose slots are
        filled (``admit``), run (``run``) and emptied (``take``) independently while one captured step graph keeps replaying.  Fixed here,
        because the graph bakes them in: ``order3`` / ``stochastic`` (requests with order-3 / ddim-eta / ddpm schedules may come),
        ``unconditional_prompt`` (1, Lu <= Lp, C) (a guided loop: the engine runs 2 B items, every request brings its own scale) and the
        x0 correction -- either the loop-wide ``correcting_x0_fn=`` or ``item_corrections=True``: every request then brings its own
        (``SlotLoop.admit(correction=)``), which also goes with ``stochastic=True`` and ``order3=True``; both: ValueError.
        ``require_tail_free`` False admits requests that ``sample`` would give trailing fp32 evaluations anyway (previews: their
        latent carries the 16-bit rounding of its last evaluations).  ``known_frames=True``: requests may bring known frames
        (``SlotLoop.admit(known=, known_mask=)``) -- the step gets the per-slot hold launch; with ``correcting_x0_fn=`` or
        ``item_corrections=True``: ValueError (a correction would rescale held frames).  See ``SlotLoop``."""
        return SlotLoop(self, B, T, Lp, order3, stochastic, unconditional_prompt, correcting_x0_fn, thresholding_max_val,
                        dynamic_thresholding_ratio, use_graph, require_tail_free, item_corrections, known_frames)

    def sample_sharded(self, content, prompt, prompt_mask, noise, lengths=None, seeds=None, prompt_lengths=None, guidance_scale=1.0,
                       unconditional_prompt=None, unconditional_prompt_mask=None, unconditional_prompt_lengths=None, unconditional_content=None, **kw):
        """Data-parallel: every rank receives the GLOBAL batch description, runs its contiguous slice and the
        finished latents are all-gathered (RCCL).  The noise (and ``seeds``, for ddpm / ddim with eta > 0: drawn for the global
        batch from ``generator`` if None) is drawn for the global batch and sliced, so an utterance's
        result does not depend on the world size beyond the precision's rounding noise (fp32: ~1e-6; 16-bit: a shard of
        3 and a shard of 2 round differently, ~7e-4 -- tests/test_dropin_gpu.py::test_sample_sharded_rccl_*)."""
        import torch
        import torch.distributed as td
        rank = td.get_rank() if td.is_initialized() else 0
        world = td.get_world_size() if td.is_initialized() else 1
        n = content.shape[0]
        lo, hi = _dist.shard_range(n, rank, world)
        if hi == lo:      # fewer utterances than ranks: this rank has nothing to denoise but must still join the collective
            local = torch.zeros((0, self.cfg.latent_channels, content.shape[2]), dtype=torch.float32, device=content.device)
        else:
            if seeds is None and kw.get("solver") in DISCRETE_SOLVERS:
                seeds = draw_seeds(n, kw.get("generator"))
            for k, entry in (("schedules", "schedule"), ("corrections", "entry")):      # (the global count: the slice would name the shard's)
                if kw.get(k) is not None and len(kw[k]) != n:
                    raise ValueError(f"{k} must be a list of one {entry} (dict or None) per item ({n}), got {len(kw[k])}")
            # the per-item arguments go with the batch; a scalar / one shared row goes to every rank whole
            local = self.sample(**SampleRequest.take(dict(
                kw, content=content, prompt=prompt, prompt_mask=prompt_mask, noise=noise, lengths=lengths, seeds=seeds, prompt_lengths=prompt_lengths,
                guidance_scale=guidance_scale, unconditional_prompt=unconditional_prompt, unconditional_prompt_mask=unconditional_prompt_mask,
                unconditional_prompt_lengths=unconditional_prompt_lengths, unconditional_content=unconditional_content), slice(lo, hi), n))
        return _dist.gather_latents(local, n)


class OverlappedPipeline:
    """Three-stage utterance-batch pipeline on three HIP streams: the PyTorch-ROCm front end (ContentVec / ``Pre_model.infer``,
    reference ``model.py:359-376``) and back end (``vocos.decode``, ``model.py:689-696``) overlap the denoiser instead of
    running before / after it (BASELINE.json north_star):

        pre(k+1)   |   denoise(k)   |   post(k-1)

    ``pre_fn(item)`` runs on the front-end stream and returns a dict with torch CUDA tensors ``content`` (B,256,T),
    ``prompt`` (B,Lp,256) and optionally ``prompt_mask`` (B,Lp) bool, ``noise`` (B,100,T), ``lengths``, ``prompt_lengths`` and ``schedules`` (``Denoiser.sample``); ``post_fn(latent, item)``
    runs on the back-end stream with the sampled latent (B,100,T) fp32.  Ordering is by events only -- the host never
    blocks until the end of ``run`` -- and the denoiser still replays one captured hipGraph per step on its own stream.
    """

    def __init__(self, denoiser: Denoiser, pre_fn, post_fn, solver: str = "unipc", steps: Optional[int] = 20, order: int = 2,
                 use_graph: bool = True, pre_device=None, post_device=None, stage_cus=None, denoiser_cus=None, eta: float = 0.0,
                 guidance_scale=1.0, unconditional_prompt=None, unconditional_prompt_mask=None, unconditional_prompt_lengths=None,
                 correcting_x0_fn=None, thresholding_max_val: float = 1.0, dynamic_thresholding_ratio: float = 0.995, **options):
        """``pre_device`` / ``post_device`` (r4): run the front / back end on ANOTHER ROCm device of the node.  On one GPU the three streams
        serialise (the denoiser's launches hold every CU: 7.8 % of the stages' kernel time overlaps, profiles/r03_overlap_trace.txt); a stage
        on its own device overlaps by construction and only its tensors cross xGMI -- content + prompt 35 MB per 32 x 10 s batch in, the
        latent 12 MB out, stream-ordered peer copies behind the stage's event.  ``pre_fn`` then runs with ``pre_device`` current and must
        return tensors on it; ``post_fn`` receives the latent on ``post_device``.  None = the denoiser's device (the one-GPU pipeline).
        NOT measured on two devices yet (no multi-GPU box this round).
        ``guidance_scale`` / ``unconditional_prompt`` (1, Lu, 256) / ``unconditional_prompt_mask`` / ``unconditional_prompt_lengths``: classifier-free
        guidance with one unconditional prompt for every item of every batch (``Denoiser.sample``), passed through.
        ``correcting_x0_fn`` / ``thresholding_max_val`` / ``dynamic_thresholding_ratio``: the x0 correction of ``Denoiser.sample``, passed through.
        ``options``: the keyword-only sampler options of ``Denoiser.sample`` (``skip_type``, ``denoise_to_zero``, ...), passed through."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("OverlappedPipeline needs a ROCm device (there is no CPU path)")
        self.denoiser, self.pre_fn, self.post_fn = denoiser, pre_fn, post_fn
        table_options(options)
        self.kw = dict(solver=solver, steps=steps, order=order, use_graph=use_graph, eta=eta, **options)
        self.kw.update(call_wide_kwargs(solver, correcting_x0_fn, thresholding_max_val, dynamic_thresholding_ratio, guidance_scale, unconditional_prompt,
                                        unconditional_prompt_mask=unconditional_prompt_mask, unconditional_prompt_lengths=unconditional_prompt_lengths))
        dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        self.pre_device = torch.device(pre_device) if pre_device is not None else dev
        self.post_device = torch.device(post_device) if post_device is not None else dev
        for d in (self.pre_device, self.post_device):
            if d.type != "cuda" or (d.index is not None and d.index >= torch.cuda.device_count()):
                raise ValueError(f"stage device {d} is not a visible ROCm device")
        self.s_pre = torch.cuda.Stream(self.pre_device)
        self.s_den = torch.cuda.Stream(dev)
        self.s_post = torch.cuda.Stream(self.post_device)
        # r5: a CU partition of ONE device (hipExtStreamCreateWithCUMask through the C ABI, wrapped as torch external streams): the two
        # PyTorch stages on `stage_cus`, the denoiser on `denoiser_cus` (iterables of CU indices; None = the whole chip).  Measured in
        # tools/overlap_partition.py / profiles/r05_overlap_partition.txt.
        self._masked = []
        if stage_cus is not None or denoiser_cus is not None:
            from .engine import Stream as _EStream
            if stage_cus is not None and self.pre_device == dev and self.post_device == dev:
                a, b = _EStream(cu_mask=stage_cus), _EStream(cu_mask=stage_cus)
                self._masked += [a, b]
                self.s_pre, self.s_post = torch.cuda.ExternalStream(a.ptr, device=dev), torch.cuda.ExternalStream(b.ptr, device=dev)
            if denoiser_cus is not None:
                c = _EStream(cu_mask=denoiser_cus)
                self._masked.append(c)
                self.s_den = torch.cuda.ExternalStream(c.ptr, device=dev)

    def _launch_pre(self, item):
        import torch
        with torch.cuda.device(self.pre_device), torch.cuda.stream(self.s_pre):
            cond = self.pre_fn(item)
            ev = torch.cuda.Event()
            ev.record(self.s_pre)
        return item, cond, ev

    def run(self, items):
        """Process an iterable of work items; returns ``[post_fn(latent_k, item_k) for k]`` (all streams drained)."""
        import torch
        it = iter(items)
        first = next(it, None)
        cur = self._launch_pre(first) if first is not None else None
        results = []
        while cur is not None:
            item, cond, ev_pre = cur
            nxt = next(it, None)
            nxt_pre = self._launch_pre(nxt) if nxt is not None else None     # front end of batch k+1 under denoise(k)
            with torch.cuda.device(self.device), torch.cuda.stream(self.s_den):
                self.s_den.wait_event(ev_pre)
                for k_, v in list(cond.items()):
                    if isinstance(v, torch.Tensor):
                        v.record_stream(self.s_den)
                        if v.device != self.device:          # front end on another device: peer copy, ordered behind its event on the denoiser's stream
                            cond[k_] = v.to(self.device, non_blocking=True)
                kw = self.kw
                if cond.get("corrections") is not None:      # the batch's items bring their own x0 corrections: in place of the call-wide one
                    kw = dict({k: v for k, v in kw.items() if k not in CORRECTION_KEYS}, corrections=cond["corrections"])
                latent = self.denoiser.sample(cond["content"], cond["prompt"], cond.get("prompt_mask"), cond.get("noise"), lengths=cond.get("lengths"),
                                              seeds=cond.get("seeds"), prompt_lengths=cond.get("prompt_lengths"), schedules=cond.get("schedules"), **kw)
                ev_den = torch.cuda.Event()
                ev_den.record(self.s_den)
            with torch.cuda.device(self.post_device), torch.cuda.stream(self.s_post):
                self.s_post.wait_event(ev_den)
                latent.record_stream(self.s_post)
                if latent.device != self.post_device:        # back end on another device: the latent crosses behind the denoiser's event
                    latent = latent.to(self.post_device, non_blocking=True)
                results.append(self.post_fn(latent, item))                   # back end of batch k under denoise(k+1)
            cur = nxt_pre
        self.s_post.synchronize()
        self.s_den.synchronize()
        return results


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


class Suspended:
    """A request taken out of a running slot loop (``SlotLoop.suspend``): its solver ``state`` (planes, T, ld) fp32 -- xe, xbar,
    d1, mprev and, in a loop opened with ``order3=True``, mprev2 --, its position ``done`` = rows of its table already run, and everything
    ``SlotLoop.resume`` sends again as an admission sends it: the ``schedule`` with its pool ``key`` and ``table``, ``length`` and
    ``prompt_length``, ``seed``, ``guidance_scale``, ``correction``, ``known`` / ``known_mask``, ``content`` and ``prompt``."""

    FIELDS = ("state", "done", "schedule", "key", "table", "flags", "length", "prompt_length", "seed", "guidance_scale", "correction", "known",
              "known_mask", "content", "prompt")

    def __init__(self, **kw):
        missing = [k for k in self.FIELDS if k not in kw]
        if missing or len(kw) != len(self.FIELDS):
            raise ValueError(f"Suspended takes exactly the fields {self.FIELDS}")
        for k in self.FIELDS:
            setattr(self, k, kw[k])

    @property
    def steps(self) -> int:
        return int(self.table.steps)

    def to(self, device) -> "Suspended":
        """the same request with its state tensor on ``device`` ("cpu": spilled to host memory; a CUDA device: ready for ``resume`` there)"""
        return Suspended(**dict({k: getattr(self, k) for k in self.FIELDS}, state=self.state.to(device)))


class SlotLoop:
    """A running loop of B slots (``Denoiser.open_slots``).  ``admit`` puts a request into an idle slot at the current loop
    step, ``run`` steps the loop until the next busy slot finishes (or by ``n`` steps), ``take`` fetches finished slots' latents and frees
    them, ``idle`` lists the free slots, ``close`` ends the loop (also with busy slots: the way out after an error).  A request ends on the bits it gets in the same slot of the same loop shape with every other slot
    idle, whatever its neighbours do.  The loop always runs with per-item lengths and prompt lengths (an admission copies tables, never
    rebuilds the plan) and replays ONE captured step graph.  Everything is enqueued on the current torch stream of the request's device;
    nothing waits for the device.

    A slot loop has no mixed-precision tail (the slots stand at different rows): a request whose schedule, guidance scale or correction
    asks for trailing fp32 evaluations at the engine's precision is refused -- run the loop on a ``Denoiser(precision="fp32")``.  The
    16-bit default, UniPC order 2 unguided and uncorrected, needs none.  The precision self-check runs once per set of weights on the first
    admission into an all-idle loop, at the request's first evaluation point; the LayerNorm guard's read-outs are not taken inside a slot
    loop (a plan switch would end it).  The 32-bit loop step is rebased to 0 by ``admit`` whenever the loop is drained and has passed 2^30."""

    REBASE_AT = 1 << 30
    item_corrections = False      # (set by open_slots(item_corrections=True): every request brings its own x0 correction)
    known_frames = False          # (set by open_slots(known_frames=True): a request may bring known frames)

    def __init__(self, den: "Denoiser", B: int, T: int, Lp: int, order3: bool, stochastic: bool, unconditional_prompt, correcting_x0_fn,
                 thresholding_max_val: float, dynamic_thresholding_ratio: float, use_graph: bool, require_tail_free: bool = True,
                 item_corrections: bool = False, known_frames: bool = False):
        import torch
        self.require_tail_free = bool(require_tail_free)
        self.item_corrections = bool(item_corrections)
        self.known_frames = bool(known_frames)
        if self.known_frames and (self.item_corrections or check_x0_correction(correcting_x0_fn, dynamic_thresholding_ratio, thresholding_max_val,
                                                                               names_only=True)):
            raise ValueError("known_frames=True does not go with an x0 correction (correcting_x0_fn=, item_corrections=True): it would rescale "
                             "the held frames")
        if self.item_corrections and correcting_x0_fn is not None:
            raise ValueError("item_corrections=True (every request brings its own x0 correction) and the loop-wide correcting_x0_fn= exclude each other")
        if min(int(B), int(T), int(Lp)) < 1:
            raise ValueError("open_slots needs B, T, Lp >= 1")
        self.den, self.B, self.T, self.Lp, self.use_graph = den, int(B), int(T), int(Lp), bool(use_graph)
        self.order3, self.stochastic = bool(order3), bool(stochastic)
        self.corr = None
        if check_x0_correction(correcting_x0_fn, dynamic_thresholding_ratio, thresholding_max_val, names_only=True):
            if self.stochastic:
                raise ValueError("correcting_x0_fn applies to unipc / dpmsolver++ only: a slot loop that takes stochastic requests runs without it")
            self.corr = (correcting_x0_fn, float(dynamic_thresholding_ratio), float(thresholding_max_val))
        self.uncond = None
        if unconditional_prompt is not None:
            if len(unconditional_prompt.shape) != 3 or unconditional_prompt.shape[0] != 1 or unconditional_prompt.shape[1] > self.Lp:
                raise ValueError(f"unconditional_prompt must be (1, Lu <= Lp = {self.Lp}, C), got {tuple(unconditional_prompt.shape)}")
            self.uncond = unconditional_prompt
        self.rep = 2 if self.uncond is not None else 1
        self.pool = TablePool()
        self._tables: Dict[tuple, object] = {}
        self.items = [None] * self.B            # per slot: None (idle) or dict(key=, start=, steps=, length=)
        self.step = 0
        self.lengths = np.full((self.rep * self.B,), self.T, dtype=np.int32)
        self.plens = np.full((self.rep * self.B,), self.Lp, dtype=np.int32)
        self.seeds = np.zeros((self.B,), dtype=np.uint64)
        self.scales = np.ones((self.B,), dtype=np.float32)
        self.corrections = [None] * self.B      # per slot: None or (name, ratio, max_val) (item_corrections)
        eng = den.engine
        den._guard_before()
        den._prepare(self.rep * self.B, self.T, self.Lp)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        s = torch.cuda.current_stream(self.dev)
        if eng.hold is not None:                 # (known frames left on by an earlier sample(known=): a slot loop does not run with them)
            eng.set_known(None, None, stream=s)
        eng.set_lengths(self.lengths, stream=s)
        eng.set_prompt_lengths(self.plens, stream=s)
        if self.uncond is not None or eng.guidance is not None:
            eng.set_guidance(self.scales if self.uncond is not None else None, stream=s)
        den._correct(eng, self.corr)
        if self.known_frames:      # (the keyword reaches the engine only when it is set: the default call is what it was)
            eng.open_slots(self.order3, self.stochastic, stream=s, item_corrections=self.item_corrections, known_frames=True)
        else:
            eng.open_slots(self.order3, self.stochastic, stream=s, item_corrections=self.item_corrections)
        if self.stochastic:
            eng.set_seeds(self.seeds, stream=s)
        den._table_key = None                    # (the engine's table belongs to the pool now)

    # -- bookkeeping -------------------------------------------------------------------------------------------------------
    def idle(self):
        return [b for b in range(self.B) if self.items[b] is None]

    def finished(self):
        return [b for b in range(self.B) if self.items[b] is not None and self.items[b]["start"] + self.items[b]["steps"] <= self.step]

    def _table(self, key):
        if key not in self._tables:
            solver, steps, order, eta, opts = key
            self._tables[key] = build_table(solver, steps, self.den._betas_for(solver), order, eta, **dict(opts))
        return self._tables[key]

    def check_request(self, schedule, guidance_scale: float = 1.0, correction=None):
        """the errors of a request that can be seen without its tensors (ValueError); returns (key, table, flags).  ``correction``: the
        request's own x0 correction (a loop opened with ``item_corrections=True``)."""
        own = item_correction_entry(correction, "correction")
        if own is not None and not self.item_corrections:
            raise ValueError("a request with its own x0 correction needs a slot loop opened with item_corrections=True")
        key = schedule_key(schedule)
        solver, steps, order, eta, _ = key
        check_item_schedule(key, "correction" if own is not None else "slot", len(self.den.betas64), self.corr is not None or own is not None)
        if not np.isfinite(float(guidance_scale)):
            raise ValueError("guidance_scale must be finite")
        if float(guidance_scale) != 1.0 and self.uncond is None:
            raise ValueError("a guided request needs a slot loop opened with unconditional_prompt=")
        n_tail = slot_tail_needed(self.den.precision, solver, order, guidance_scale, self.corr is not None or own is not None)
        if n_tail > 0 and self.require_tail_free:
            raise ValueError(f"this request ({solver}, order {order}, guidance scale {float(guidance_scale):g}"
                             f"{', corrected' if self.corr is not None or own is not None else ''}) needs {n_tail} trailing fp32 evaluation(s) at precision "
                             f"{self.den.precision!r}; a slot loop has no fp32 tail: open it on a Denoiser(precision=\"fp32\")")
        table = self._table(key)
        flags = table_flags(table)
        if flags & ITEM_HIST2 and not self.order3:
            raise ValueError("an order-3 request needs a slot loop opened with order3=True")
        if flags & ITEM_NOISE and not self.stochastic:
            raise ValueError(f"a stochastic request ({solver}) needs a slot loop opened with stochastic=True")
        return key, table, flags

    # -- the four calls ------------------------------------------------------------------------------------------------------
    def admit(self, slot: int, content, prompt, noise, length: Optional[int] = None, prompt_length: Optional[int] = None, schedule=None,
              seed: int = 0, guidance_scale: float = 1.0, correction=None, known=None, known_mask=None) -> None:
        """one request into the idle ``slot`` at the current loop step: ``content`` (256, L), ``prompt`` (lp, 256), ``noise`` = x_T
        (100, L) on the GPU, L <= T and lp <= Lp frames (``length`` / ``prompt_length`` default to them; shorter values use the first
        frames), ``schedule`` = dict(solver=, steps=, order=, eta=, table options), ``seed`` of its noise stream (stochastic schedules),
        ``guidance_scale`` (a guided loop), ``correction`` = the request's own x0 correction, None or ``dict(correcting_x0_fn=,
        thresholding_max_val=, dynamic_thresholding_ratio=)`` (a loop opened with ``item_corrections=True``).  ``known`` (100, L) on the GPU
        with ``known_mask`` (L,) bool (a loop opened with ``known_frames=True``): on the frames of the mask, all inside the
        request's length, the request holds ``known`` -- its x_T there is alpha_0 known + sigma_0 noise by its own first table row
        (``schedule.known_start``) and every evaluation's x0 is overwritten there; an all-False mask is no hold.  The frames last for this
        request: ``take`` clears the slot."""
        if (known is None) != (known_mask is None):
            raise ValueError("known and known_mask are given together")
        self.admit_group([slot], [content], [prompt], [noise], None if length is None else [length],
                         None if prompt_length is None else [prompt_length], [schedule], [seed], [guidance_scale], [correction],
                         None if known is None else [known], None if known_mask is None else [known_mask])

    def admit_group(self, slots, contents, prompts, noises, lengths=None, prompt_lengths=None, schedules=None, seeds=None, guidance_scales=None,
                    corrections=None, knowns=None, known_masks=None) -> None:
        """``admit`` for several requests at once (lists of per-request tensors): one condition rebuild and one admit launch for all;
        ``knowns`` / ``known_masks``: one entry per request, None for a request without known frames"""
        import torch
        n = len(slots)
        if n == 0 or not (len(contents) == len(prompts) == len(noises) == n):
            raise ValueError("admit_group needs one content, prompt and noise per slot")
        slots = [int(b) for b in slots]
        if len(set(slots)) != n or any(b < 0 or b >= self.B for b in slots):
            raise ValueError(f"slots must be distinct and in [0, {self.B}), got {slots}")
        busy = [b for b in slots if self.items[b] is not None]
        if busy:
            raise ValueError(f"slot(s) {busy} are busy: take them first")
        schedules = [None] * n if schedules is None else list(schedules)
        scales = [1.0] * n if guidance_scales is None else [float(g) for g in guidance_scales]
        seeds = [0] * n if seeds is None else [int(v) for v in seeds]
        corrections = [None] * n if corrections is None else list(corrections)
        if len(corrections) != n:
            raise ValueError("admit_group needs one correction (dict or None) per slot")
        cfg = self.den.cfg
        reqs = []
        for k in range(n):
            if schedules[k] is None:
                raise ValueError("a request needs its schedule: dict(solver=, steps=, ...)")
            key, table, flags = self.check_request(schedules[k], scales[k], corrections[k])
            c, p, x = contents[k], prompts[k], noises[k]
            if c.dim() != 2 or c.shape[0] != cfg.content_channels or p.dim() != 2 or p.shape[1] != cfg.cross_attention_dim or \
                    x.dim() != 2 or x.shape[0] != cfg.latent_channels:
                raise ValueError(f"a request is content ({cfg.content_channels}, L), prompt (lp, {cfg.cross_attention_dim}), noise ({cfg.latent_channels}, L); "
                                 f"got {tuple(c.shape)}, {tuple(p.shape)}, {tuple(x.shape)}")
            L = int(c.shape[1]) if lengths is None else int(lengths[k])
            lp = int(p.shape[0]) if prompt_lengths is None else int(prompt_lengths[k])
            if not (1 <= L <= min(self.T, int(c.shape[1]), int(x.shape[1]))):
                raise ValueError(f"length {L} outside [1, min(T = {self.T}, the content's {int(c.shape[1])} and the noise's {int(x.shape[1])} frames)]")
            if not (1 <= lp <= min(self.Lp, int(p.shape[0]))):
                raise ValueError(f"prompt_length {lp} outside [1, min(Lp = {self.Lp}, the prompt's {int(p.shape[0])} frames)]")
            reqs.append((key, table, flags, L, lp))
        holds = self._check_known(n, knowns, known_masks, [r[3] for r in reqs])
        dev = self.dev
        s = torch.cuda.current_stream(dev)
        eng = self.den.engine
        if not any(it is not None for it in self.items) and self.step >= self.REBASE_AT:      # drained: rebase the 32-bit loop step
            eng.rebase_slots(stream=s)
            self.step = 0
        c_all = torch.zeros((n, cfg.content_channels, self.T), dtype=torch.float32, device=dev)
        p_all = torch.zeros((n, self.Lp, cfg.cross_attention_dim), dtype=torch.float32, device=dev)
        x_all = torch.zeros((n, cfg.latent_channels, self.T), dtype=torch.float32, device=dev)
        for k, (key, table, flags, L, lp) in enumerate(reqs):
            c_all[k, :, :L] = contents[k][:, :L].to(dev, torch.float32)
            p_all[k, :lp] = prompts[k][:lp].to(dev, torch.float32)
            x_all[k, :, :L] = noises[k][:, :L].to(dev, torch.float32)
        k_all = m_all = None
        if any(h is not None for h in holds):      # known rows and masks of the whole group (no hold: a clear mask), and x_T on the held frames
            k_all = torch.zeros((n, cfg.latent_channels, self.T), dtype=torch.float32, device=dev)
            m_all = np.zeros((n, self.T), dtype=bool)
            for k, h in enumerate(holds):
                if h is None:
                    continue
                kn, mk = h
                Lk = mk.shape[0]
                k_all[k, :, :Lk] = kn.to(dev, torch.float32)
                m_all[k, :Lk] = mk
            x_all = known_start_torch(x_all, k_all, m_all, np.stack([r[1].coef[0] for r in reqs]))
        for k, b in enumerate(slots):
            L, lp = reqs[k][3], reqs[k][4]
            self.lengths[b], self.plens[b], self.seeds[b], self.scales[b] = L, lp, seeds[k], scales[k]
            if self.item_corrections:
                self.corrections[b] = item_correction_entry(corrections[k])
            if self.rep == 2:      # (the unconditional half comes first)
                self.lengths[b + self.B], self.plens[b], self.plens[b + self.B] = L, int(self.uncond.shape[1]), lp
        if self.den.precision_check is not None and not self.den._precision_checked and not any(it is not None for it in self.items):
            # the check's evaluations advance the engine's step counter and load the state of all items (zeros outside the admitted slots,
            # as an idle slot has): rebase afterwards
            self._self_check(slots, c_all, p_all, x_all, [r[1] for r in reqs], s)
            eng.rebase_slots(stream=s)
            self.step = 0
        self._place(slots, [r[:3] for r in reqs], [self.step] * n, c_all, p_all, k_all, m_all, s,
                    lambda records: eng.admit(slots, x_all, records, stream=s))
        for t in (c_all, p_all, x_all) + (() if k_all is None else (k_all,)):
            if t.is_cuda:
                t.record_stream(s)
        for k, b in enumerate(slots):
            self.items[b] = dict(key=reqs[k][0], start=self.step, steps=reqs[k][1].steps, length=reqs[k][3],
                                 req=dict(schedule=dict(schedules[k]), table=reqs[k][1], flags=reqs[k][2], prompt_length=reqs[k][4], seed=seeds[k],
                                          guidance_scale=scales[k], correction=corrections[k], known=None if holds[k] is None else holds[k][0],
                                          known_mask=None if holds[k] is None else holds[k][1], content=contents[k], prompt=prompts[k]))

    def _place(self, slots, entries, position, c_all, p_all, k_all, m_all, s, launch) -> None:
        """the engine calls that put requests into idle ``slots``, shared by ``admit_group`` and ``resume``: the tables' rows (``entries`` =
        [(key, table, flags)]; written where the pool says so), the per-slot vectors (lengths, prompt lengths, seeds, corrections, guidance),
        the condition, the known frames, then ``launch(records)`` with records {row0, steps, ``position[k]``, flags} -- the start of an
        admission, the rows already run of a resume.  On any error the tables' users go back and the slots hold no frames."""
        import torch
        cfg, eng, n = self.den.cfg, self.den.engine, len(slots)
        dev = c_all.device
        records = np.zeros((n, 4), dtype=np.int32)
        acquired = []
        known_sent = False
        try:
            for k, (key, table, flags) in enumerate(entries):
                row0, write = self.pool.acquire(key, table.coef)
                acquired.append(key)
                if write:
                    eng.write_sampler_rows(row0, table.coef, stream=s)
                records[k] = (row0, table.steps, position[k], flags)
            eng.set_lengths(self.lengths, stream=s)
            eng.set_prompt_lengths(self.plens, stream=s)
            if self.stochastic:
                eng.set_seeds(self.seeds, stream=s)
            if self.item_corrections:      # (the whole vector: only the placed slots' entries have changed)
                self.den._correct(eng, None, self.corrections, s)
            if self.rep == 2:
                eng.set_guidance(self.scales, stream=s)
                u = torch.zeros((n, self.Lp, cfg.cross_attention_dim), dtype=torch.float32, device=dev)
                u[:, :self.uncond.shape[1]] = self.uncond.to(dev, torch.float32)
                eng.set_condition_items(slots + [b + self.B for b in slots], torch.cat([c_all, c_all]), torch.cat([u, p_all]), None, stream=s)
            else:
                eng.set_condition_items(slots, c_all, p_all, None, stream=s)
            if k_all is not None:
                eng.set_known_items(slots, k_all, m_all, stream=s)
                known_sent = True
            launch(records)
        except Exception:          # nothing was placed: the tables' users go back (the slots stay idle)
            for key in acquired:
                self.pool.release(key)
            if known_sent:         # ... and hold no frames: a later request without known frames sends none and must find the slots clear
                try:
                    eng.set_known_items(slots, None, None, stream=s)
                except Exception:      # noqa: BLE001 (the placement's own error is the one to report)
                    pass
            raise

    # -- suspend and resume ------------------------------------------------------------------------------------
    def suspend(self, slots):
        """takes the running requests of ``slots`` out of the loop: one ``Suspended`` per slot, in order, holding the solver state bit for bit
        and the rows already run; the slots become idle and their tables' pool users are released.  Only a request with rows still to run
        (a finished one is taken).  One launch, no recapture, nothing waits for the device."""
        import torch
        slots = [int(b) for b in slots]
        if not slots or len(set(slots)) != len(slots) or any(b < 0 or b >= self.B for b in slots):
            raise ValueError(f"slots must be distinct and in [0, {self.B}), got {slots}")
        bad = [b for b in slots if self.items[b] is None or not 0 <= self.step - self.items[b]["start"] < self.items[b]["steps"]]
        if bad:
            raise ValueError(f"slot(s) {bad} hold no running request (an idle slot has none; a finished one is taken)")
        norec = [b for b in slots if "req" not in self.items[b]]
        if norec:
            raise ValueError(f"slot(s) {norec} were not admitted through this loop: nothing to send again on resume")
        eng = self.den.engine
        s = torch.cuda.current_stream(self.dev)
        P, T, ld = eng.state_shape()
        state = torch.empty((len(slots), P, T, ld), dtype=torch.float32, device=self.dev)
        done = eng.suspend(slots, state, stream=s)
        if state.is_cuda:
            state.record_stream(s)
        out = []
        for k, b in enumerate(slots):
            it = self.items[b]
            if int(done[k]) != self.step - it["start"]:
                raise RuntimeError(f"slot {b}: the engine reports {int(done[k])} rows run, the loop {self.step - it['start']}")
            out.append(Suspended(state=state[k], done=int(done[k]), key=it["key"], length=it["length"], **it["req"]))
            self.pool.release(it["key"])
            self.items[b] = None
            if self.item_corrections:
                self.corrections[b] = None
        return out

    def resume(self, slots, suspended) -> None:
        """puts the ``suspended`` requests back into the idle ``slots`` of this loop -- or of another loop of the same T, padded channels and
        form -- at the current loop step: ``admit_group``'s sequence (tables, lengths, seeds, corrections, guidance, condition, known frames)
        with the saved state in place of x_T.  Each continues at row ``done`` and, in the slot index it left, ends on the bits of the
        uninterrupted run.  Never runs the precision self-check: it raises while the denoiser's check is pending."""
        import torch
        slots = [int(b) for b in slots]
        suspended = list(suspended)
        n = len(slots)
        if n == 0 or len(suspended) != n or any(not isinstance(q, Suspended) for q in suspended):
            raise ValueError("resume needs one Suspended per slot")
        if len(set(slots)) != n or any(b < 0 or b >= self.B for b in slots):
            raise ValueError(f"slots must be distinct and in [0, {self.B}), got {slots}")
        busy = [b for b in slots if self.items[b] is not None]
        if busy:
            raise ValueError(f"slot(s) {busy} are busy: take or suspend them first")
        if self.den.precision_check is not None and not self.den._precision_checked:
            raise RuntimeError("the precision self-check of this Denoiser is pending: it runs on an admission into an idle loop, never on a "
                               "resume (admit a request first, or build the Denoiser with precision_check=None)")
        cfg = self.den.cfg
        eng = self.den.engine
        shape = eng.state_shape()
        for k, q in enumerate(suspended):
            key, table, flags = self.check_request(q.schedule, q.guidance_scale, q.correction)
            if key != q.key or flags != q.flags or table.steps != q.steps:
                raise ValueError(f"suspended[{k}]: its schedule gives another table here (key {key}, {table.steps} rows) than where it ran "
                                 f"(key {q.key}, {q.steps} rows)")
            if not 0 <= int(q.done) < q.steps:
                raise ValueError(f"suspended[{k}]: done {q.done} outside [0, {q.steps})")
            if tuple(q.state.shape) != tuple(shape) or q.state.dtype != torch.float32:
                raise ValueError(f"suspended[{k}]: state {tuple(q.state.shape)} {q.state.dtype}, this loop's is float32 {tuple(shape)} (planes, T, padded "
                                 f"channels): resume into a loop of the same T and form")
            if not (1 <= q.length <= self.T) or not (1 <= q.prompt_length <= self.Lp):
                raise ValueError(f"suspended[{k}]: length {q.length} / prompt_length {q.prompt_length} outside this loop's T = {self.T} / Lp = {self.Lp}")
            if q.known is not None and not self.known_frames:
                raise ValueError("a request with known frames needs a slot loop opened with known_frames=True")
        dev = self.dev
        s = torch.cuda.current_stream(dev)
        if not any(it is not None for it in self.items) and self.step >= self.REBASE_AT:
            eng.rebase_slots(stream=s)
            self.step = 0
        c_all = torch.zeros((n, cfg.content_channels, self.T), dtype=torch.float32, device=dev)
        p_all = torch.zeros((n, self.Lp, cfg.cross_attention_dim), dtype=torch.float32, device=dev)
        for k, q in enumerate(suspended):
            c_all[k, :, :q.length] = q.content[:, :q.length].to(dev, torch.float32)
            p_all[k, :q.prompt_length] = q.prompt[:q.prompt_length].to(dev, torch.float32)
        state = torch.stack([q.state.to(dev) for q in suspended]).contiguous()
        k_all = m_all = None
        if any(q.known is not None for q in suspended):
            k_all = torch.zeros((n, cfg.latent_channels, self.T), dtype=torch.float32, device=dev)
            m_all = np.zeros((n, self.T), dtype=bool)
            for k, q in enumerate(suspended):
                if q.known is not None:
                    Lk = q.known_mask.shape[0]
                    k_all[k, :, :Lk] = q.known.to(dev, torch.float32)
                    m_all[k, :Lk] = q.known_mask
        saved = (self.lengths.copy(), self.plens.copy(), self.seeds.copy(), self.scales.copy(), list(self.corrections))
        for k, b in enumerate(slots):
            q = suspended[k]
            self.lengths[b], self.plens[b], self.seeds[b], self.scales[b] = q.length, q.prompt_length, q.seed, q.guidance_scale
            if self.item_corrections:
                self.corrections[b] = item_correction_entry(q.correction)
            if self.rep == 2:
                self.lengths[b + self.B], self.plens[b], self.plens[b + self.B] = q.length, int(self.uncond.shape[1]), q.prompt_length
        try:
            self._place(slots, [(q.key, q.table, q.flags) for q in suspended], [q.done for q in suspended], c_all, p_all, k_all, m_all, s,
                        lambda records: eng.resume(slots, state, records, stream=s))
        except Exception:          # nothing was resumed: the slots stay idle with the vectors they had, the requests stay with the caller
            self.lengths, self.plens, self.seeds, self.scales, self.corrections = saved
            raise
        for t in (c_all, p_all, state) + (() if k_all is None else (k_all,)):
            if t.is_cuda:
                t.record_stream(s)
        for k, b in enumerate(slots):
            q = suspended[k]
            self.items[b] = dict(key=q.key, start=self.step - q.done, steps=q.steps, length=q.length,
                                 req=dict(schedule=dict(q.schedule), table=q.table, flags=q.flags, prompt_length=q.prompt_length, seed=q.seed,
                                          guidance_scale=q.guidance_scale, correction=q.correction, known=q.known, known_mask=q.known_mask,
                                          content=q.content, prompt=q.prompt))

    def _check_known(self, n, knowns, known_masks, lengths):
        """the known frames of an admission, checked before any engine call: per request None or (known (100, L') tensor, mask (L',) bool
        array), L' <= T; an all-False mask is None"""
        if knowns is None and known_masks is None:
            return [None] * n
        if knowns is None or known_masks is None or len(knowns) != n or len(known_masks) != n:
            raise ValueError("knowns and known_masks are given together, one entry (or None) per slot")
        nc = self.den.cfg.latent_channels
        out = []
        for k in range(n):
            kn, mk = knowns[k], known_masks[k]
            if kn is None and mk is None:
                out.append(None)
                continue
            if kn is None or mk is None:
                raise ValueError("known and known_mask are given together")
            if not self.known_frames:
                raise ValueError("a request with known frames needs a slot loop opened with known_frames=True")
            if hasattr(mk, "detach"):
                mk = mk.detach().cpu().numpy()
            mk = np.asarray(mk)
            if mk.dtype != np.bool_ or mk.ndim != 1:
                raise ValueError(f"known_mask must be a bool array (L,), got {mk.dtype} {mk.shape}")
            if not hasattr(kn, "dim") or kn.dim() != 2 or tuple(kn.shape) != (nc, mk.shape[0]) or mk.shape[0] > self.T:
                raise ValueError(f"known must be a tensor ({nc}, L) with known_mask (L,), L <= T = {self.T}; got "
                                 f"{tuple(kn.shape) if hasattr(kn, 'shape') else type(kn).__name__} and {mk.shape}")
            if not kn.dtype.is_floating_point:
                raise ValueError(f"known must be a floating-point tensor, got {kn.dtype}")
            if mk.any() and int(np.nonzero(mk)[0][-1]) >= lengths[k]:
                raise ValueError(f"known frame {int(np.nonzero(mk)[0][-1])} lies at or past the request's length {lengths[k]}")
            out.append((kn, mk) if mk.any() else None)
        return out

    def _self_check(self, slots, c_all, p_all, x_all, tables, s) -> None:
        """the Denoiser's precision self-check on the first fill: the admitted requests' first evaluation point, the other slots idle"""
        import torch
        den, nb = self.den, self.rep * self.B
        dev = c_all.device
        cfg = den.cfg
        c = torch.zeros((nb, cfg.content_channels, self.T), dtype=torch.float32, device=dev)
        p = torch.zeros((nb, self.Lp, cfg.cross_attention_dim), dtype=torch.float32, device=dev)
        x = torch.zeros((nb, cfg.latent_channels, self.T), dtype=torch.float32, device=dev)
        t = torch.zeros((nb,), dtype=torch.float32, device=dev)
        for k, b in enumerate(slots):
            for h in range(self.rep):
                c[b + h * self.B], x[b + h * self.B], t[b + h * self.B] = c_all[k], x_all[k], float(tables[k].coef[0, 0])
            p[b + (self.rep - 1) * self.B] = p_all[k]
            if self.rep == 2:
                p[b, :self.uncond.shape[1]] = self.uncond[0].to(dev, torch.float32)
        den._self_check([(x, t)], c, p, None, s, keep_fp32=False, lengths=self.lengths, prompt_lengths=self.plens)
        if den.serving_fp32:
            raise RuntimeError(f"the {den.precision} engine failed the precision self-check ({den.precision_error_seen:.2e}); a slot loop cannot "
                               f"fall back per call: open it on a Denoiser(precision=\"fp32\")")

    def run(self, n: Optional[int] = None):
        """steps the loop until the next busy slot finishes -- not at all when one already has -- or by exactly ``n`` steps; returns the
        finished slots (not yet taken)"""
        import torch
        if n is None:
            ends = [it["start"] + it["steps"] for it in self.items if it is not None]
            if not ends:
                return []
            n = max(0, min(ends) - self.step)
        if n < 0:
            raise ValueError("run(n) needs n >= 0")
        if n > 0:
            self.den.engine.sample_steps(int(n), use_graph=self.use_graph, stream=torch.cuda.current_stream(self.dev))
            self.step += int(n)
        return self.finished()

    def close(self) -> None:
        """ends the loop, whatever its slots hold (``ns2vc_sampler_end``: requests still running are dropped): the engine leaves slot mode
        and takes ``sample`` / ``open_slots`` again.  Safe to call twice, and after an error in mid-loop."""
        import torch
        eng = self.den.engine
        if eng.slot_step() >= 0:
            scratch = torch.empty((self.B, self.den.cfg.latent_channels, self.T), dtype=torch.float32, device=self.dev)
            eng.sample_end(scratch, stream=torch.cuda.current_stream(self.dev))
        for b in range(self.B):
            if self.items[b] is not None:
                self.pool.release(self.items[b]["key"])
                self.items[b] = None
        self.den._table_key = None

    def take(self, slots):
        """latents (n, 100, T) of the finished ``slots`` (zeros past each request's length); the slots become idle"""
        import torch
        slots = [int(b) for b in slots]
        bad = [b for b in slots if b < 0 or b >= self.B or self.items[b] is None or self.items[b]["start"] + self.items[b]["steps"] > self.step]
        if bad:
            raise ValueError(f"slot(s) {bad} hold no finished request")
        out = torch.empty((len(slots), self.den.cfg.latent_channels, self.T), dtype=torch.float32, device=self.dev)
        self.den.engine.take(slots, out, stream=torch.cuda.current_stream(self.dev))
        for b in slots:
            self.pool.release(self.items[b]["key"])
            self.items[b] = None
            if self.item_corrections:
                self.corrections[b] = None      # (reaches the engine with the next admission's vector; an idle slot reads nothing)
        return out
