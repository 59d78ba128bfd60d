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
from .request import (CORRECTION_KEYS, DEFAULT_TAIL_FP32, DEFAULT_TAIL_FP32_ORDER3, EVALUATION_ERROR, PARITY_BAR, SampleRequest, call_wide_kwargs,  # noqa: F401
                      check_guidance, check_item_schedule, corrected_tail_min, default_tail_fp32, guided_tail_extra, host_array, item_correction_entry,
                      slot_tail_needed)      # (the tail rules live in request.py and are exported from here as before)
from .schedule import (DISCRETE_SOLVERS, ITEM_HIST2, ITEM_NOISE, TablePool, build_table, check_x0_correction, known_start_torch, linear_betas,
                       schedule_key, table_flags, table_options)
from .slots import SlotLoop, Suspended      # noqa: F401 (the slot loop lives in slots.py; ``Denoiser.open_slots`` and the callers' imports find it here)
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
    "masked_attn_resident",     # the attention launches that masked_attn gave a length table run on the K/V-resident kernel's masked form where
                        # the engine's rule selects it (head width 16 / 32, B * heads >= the CUs); without masked_attn it does nothing, and the
                        # fp32 engine has no such kernel and ignores it
)

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
                 masked_attn: bool = False, masked_rows: bool = False, masked_ffn: bool = False, masked_geglu: bool = False,
                 masked_attn_resident: bool = False):
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
