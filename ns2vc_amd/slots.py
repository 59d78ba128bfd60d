"""The slot loop of ``Denoiser.open_slots`` (continuous batching): one request record (``SlotRequest``), the same record out of a
running loop (``Suspended``) and the loop itself (``SlotLoop``).  The loop drives ``den.engine``; torch is memory / stream plumbing."""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Dict, Optional

import numpy as np

from .request import check_item_schedule, item_correction_entry, slot_tail_needed
from .schedule import ITEM_HIST2, ITEM_NOISE, TablePool, build_table, check_x0_correction, known_start_torch, schedule_key, table_flags


@dataclass(frozen=True, eq=False)
class SlotRequest:
    """One request as a slot loop holds it, after its checks: what an admission sends to the engine and a resume sends again."""
    schedule: dict                        # dict(solver=, steps=, order=, eta=, table options) ...
    key: tuple                            # ... its ``schedule_key`` (the pool's), table and ``table_flags``
    table: object
    flags: int
    length: int                           # frames of content / x_T in use, <= T
    prompt_length: int                    # <= Lp
    seed: int
    guidance_scale: float
    correction: object                    # the request's own x0 correction as given: None or a dict (``item_correction_entry``)
    known: object                         # (100, L') tensor with ``known_mask`` (L',) bool array, or None, None: nothing held
    known_mask: Optional[np.ndarray]
    content: object                       # (256, >= length) and (>= prompt_length, 256), as the caller gave them
    prompt: object

    @property
    def steps(self) -> int:
        return int(self.table.steps)


class Suspended(SlotRequest):
    """A request taken out of a running slot loop (``SlotLoop.suspend``): its solver ``state`` (planes, T, ld) fp32 -- xe, xbar,
    d1, mprev and, in a loop opened with ``order3=True``, mprev2 --, its position ``done`` = rows of its table already run, and everything
    ``SlotLoop.resume`` sends again as an admission sends it: the fields of its ``SlotRequest``."""

    FIELDS = ("state", "done") + tuple(f.name for f in fields(SlotRequest))      # (FIELDS[2:]: the record's own)

    def __init__(self, **kw):
        if set(kw) != set(self.FIELDS):
            raise ValueError(f"Suspended takes exactly the fields {self.FIELDS}")
        for k in self.FIELDS:
            object.__setattr__(self, k, kw[k])

    def to(self, device) -> "Suspended":
        """the same request with its state tensor on ``device`` ("cpu": spilled to host memory; a CUDA device: ready for ``resume`` there)"""
        return Suspended(**dict({k: getattr(self, k) for k in self.FIELDS}, state=self.state.to(device)))


@dataclass(frozen=True)
class _Busy:
    """a busy slot: the loop step of its request's row 0 (a resumed request: ``done`` steps back) and the request; ``entry["start"]`` and
    ``entry["steps"]``, ``["key"]``, ``["length"]`` read them as callers that step a loop themselves always have"""
    start: int
    req: SlotRequest
    end = property(lambda self: self.start + self.req.steps)

    def __getitem__(self, name: str):
        return self.start if name == "start" else getattr(self.req, name)


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

    def __init__(self, den, B: int, T: int, Lp: int, order3: bool, stochastic: bool, unconditional_prompt, correcting_x0_fn,
                 thresholding_max_val: float, dynamic_thresholding_ratio: float, use_graph: bool, require_tail_free: bool = True,
                 item_corrections: bool = False, known_frames: bool = False):
        import torch
        self.require_tail_free = bool(require_tail_free)
        self.item_corrections = bool(item_corrections)      # (every request brings its own x0 correction)
        self.known_frames = bool(known_frames)              # (a request may bring known frames)
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
        self.items = [None] * self.B            # per slot: None (idle) or (start, req)
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
        return [b for b in range(self.B) if self.items[b] is not None and self.items[b].end <= self.step]

    def _table(self, key):
        if key not in self._tables:
            solver, steps, order, eta, opts = key
            self._tables[key] = build_table(solver, steps, self.den._betas_for(solver), order, eta, **dict(opts))
        return self._tables[key]

    def _slots(self, slots, busy: Optional[str] = None):
        """``slots`` as distinct ints in [0, B) (ValueError) -- all idle, where ``busy`` says what the caller is to do with a busy one first"""
        slots = [int(b) for b in slots]
        if not slots or len(set(slots)) != len(slots) or any(b < 0 or b >= self.B for b in slots):
            raise ValueError(f"slots must be distinct and in [0, {self.B}), got {slots}")
        held = [] if busy is None else [b for b in slots if self.items[b] is not None]
        if held:
            raise ValueError(f"slot(s) {held} are busy: {busy} them first")
        return slots

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
        n = len(slots)
        if n == 0 or not (len(contents) == len(prompts) == len(noises) == n):
            raise ValueError("admit_group needs one content, prompt and noise per slot")
        slots = self._slots(slots, busy="take")
        schedules = [None] * n if schedules is None else list(schedules)
        scales = [1.0] * n if guidance_scales is None else [float(g) for g in guidance_scales]
        seeds = [0] * n if seeds is None else [int(v) for v in seeds]
        corrections = [None] * n if corrections is None else list(corrections)
        if len(corrections) != n:
            raise ValueError("admit_group needs one correction (dict or None) per slot")
        cfg = self.den.cfg
        found = []
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
            found.append(dict(schedule=dict(schedules[k]), key=key, table=table, flags=flags, length=L, prompt_length=lp, seed=seeds[k],
                              guidance_scale=scales[k], correction=corrections[k], content=c, prompt=p))
        holds = self._check_known(n, knowns, known_masks, [f["length"] for f in found])
        reqs = [SlotRequest(known=kn, known_mask=mk, **f) for f, (kn, mk) in zip(found, holds)]
        self._enter(slots, reqs, noises=noises)

    def _enter(self, slots, reqs, done=None, state=None, noises=None) -> None:
        """the one way into idle ``slots``, for an admission (``noises``: the requests' x_T) and for a resume (``done``: the rows each request
        has run, ``state``: their stacked solver states): rebases a drained loop, stages the condition, the start latents and the known
        frames, writes the slots' entries of the five vectors, runs the pending precision self-check of an admission into an idle loop, then
        ``_place``.  On any error the vectors are what they were and the slots stay idle; else they hold ``(start, req)``."""
        import torch
        cfg, eng, n, dev = self.den.cfg, self.den.engine, len(slots), self.dev
        s = torch.cuda.current_stream(dev)
        if not any(self.items) and self.step >= self.REBASE_AT:      # drained: rebase the 32-bit loop step
            eng.rebase_slots(stream=s)
            self.step = 0
        c_all = torch.zeros((n, cfg.content_channels, self.T), dtype=torch.float32, device=dev)
        p_all = torch.zeros((n, self.Lp, cfg.cross_attention_dim), dtype=torch.float32, device=dev)
        x_all = state if done is not None else torch.zeros((n, cfg.latent_channels, self.T), dtype=torch.float32, device=dev)
        for k, q in enumerate(reqs):
            c_all[k, :, :q.length] = q.content[:, :q.length].to(dev, torch.float32)
            p_all[k, :q.prompt_length] = q.prompt[:q.prompt_length].to(dev, torch.float32)
            if done is None:
                x_all[k, :, :q.length] = noises[k][:, :q.length].to(dev, torch.float32)
        k_all = m_all = None
        if any(q.known is not None for q in reqs):      # known rows and masks of the whole group (no hold: a clear mask)
            k_all = torch.zeros((n, cfg.latent_channels, self.T), dtype=torch.float32, device=dev)
            m_all = np.zeros((n, self.T), dtype=bool)
            for k, q in enumerate(reqs):
                if q.known is not None:
                    Lk = q.known_mask.shape[0]
                    k_all[k, :, :Lk] = q.known.to(dev, torch.float32)
                    m_all[k, :Lk] = q.known_mask
            if done is None:      # x_T on the held frames: alpha_0 known + sigma_0 noise by each request's own first table row
                x_all = known_start_torch(x_all, k_all, m_all, np.stack([q.table.coef[0] for q in reqs]))
        saved = (self.lengths.copy(), self.plens.copy(), self.seeds.copy(), self.scales.copy(), list(self.corrections))
        try:
            for b, q in zip(slots, reqs):
                self.lengths[b], self.plens[b], self.seeds[b], self.scales[b] = q.length, q.prompt_length, q.seed, q.guidance_scale
                if self.item_corrections:
                    self.corrections[b] = item_correction_entry(q.correction)
                if self.rep == 2:      # (the unconditional half comes first)
                    self.lengths[b + self.B], self.plens[b], self.plens[b + self.B] = q.length, int(self.uncond.shape[1]), q.prompt_length
            if done is None and self.den.precision_check is not None and not self.den._precision_checked and not any(self.items):
                # the check's evaluations advance the engine's step counter and load the state of all items (zeros outside the admitted slots,
                # as an idle slot has): rebase afterwards
                self._self_check(slots, c_all, p_all, x_all, reqs, s)
                eng.rebase_slots(stream=s)
                self.step = 0
            # (an admission's records start at the current loop step, a resume's stand at row ``done``)
            self._place(slots, reqs, done or [self.step] * n, c_all, p_all, k_all, m_all, s,
                        lambda records: (eng.admit if done is None else eng.resume)(slots, x_all, records, stream=s))
        except Exception:          # nothing entered: the slots stay idle with the vectors they had, the requests stay with the caller
            self.lengths, self.plens, self.seeds, self.scales, self.corrections = saved
            raise
        for t in (c_all, p_all, x_all) + (() if k_all is None else (k_all,)):
            if t.is_cuda:
                t.record_stream(s)
        for k, b in enumerate(slots):
            self.items[b] = _Busy(self.step - (0 if done is None else done[k]), reqs[k])

    def _place(self, slots, reqs, position, c_all, p_all, k_all, m_all, s, launch) -> None:
        """the engine calls that put ``reqs`` into idle ``slots``: the tables' rows (written where the pool says so), the per-slot vectors
        (lengths, prompt lengths, seeds, corrections, guidance), the condition, the known frames, then ``launch(records)`` with records
        {row0, steps, ``position[k]``, flags} -- the start of an admission, the rows already run of a resume.  On any error the tables' users
        go back and the slots hold no frames."""
        import torch
        cfg, eng, n, dev = self.den.cfg, self.den.engine, len(slots), c_all.device
        records = np.zeros((n, 4), dtype=np.int32)
        acquired = []
        known_sent = False
        try:
            for k, q in enumerate(reqs):
                row0, write = self.pool.acquire(q.key, q.table.coef)
                acquired.append(q.key)
                if write:
                    eng.write_sampler_rows(row0, q.table.coef, stream=s)
                records[k] = (row0, q.table.steps, position[k], q.flags)
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
        slots = self._slots(slots)
        bad = [b for b in slots if self.items[b] is None or not self.items[b].start <= self.step < self.items[b].end]
        if bad:
            raise ValueError(f"slot(s) {bad} hold no running request (an idle slot has none; a finished one is taken)")
        eng = self.den.engine
        s = torch.cuda.current_stream(self.dev)
        state = torch.empty((len(slots),) + tuple(eng.state_shape()), dtype=torch.float32, device=self.dev)      # (n, planes, T, ld)
        done = eng.suspend(slots, state, stream=s)
        if state.is_cuda:
            state.record_stream(s)
        out = []
        for k, b in enumerate(slots):
            start, req = self.items[b].start, self.items[b].req
            if int(done[k]) != self.step - start:
                raise RuntimeError(f"slot {b}: the engine reports {int(done[k])} rows run, the loop {self.step - start}")
            out.append(Suspended(state=state[k], done=int(done[k]), **{f: getattr(req, f) for f in Suspended.FIELDS[2:]}))
            self._free(b)
        return out

    def resume(self, slots, suspended) -> None:
        """puts the ``suspended`` requests back into the idle ``slots`` of this loop -- or of another loop of the same T, padded channels and
        form -- at the current loop step: ``admit_group``'s sequence (tables, lengths, seeds, corrections, guidance, condition, known frames)
        with the saved state in place of x_T.  Each continues at row ``done`` and, in the slot index it left, ends on the bits of the
        uninterrupted run.  Never runs the precision self-check: it raises while the denoiser's check is pending."""
        import torch
        suspended = list(suspended)
        if len(slots) == 0 or len(suspended) != len(slots) or any(not isinstance(q, Suspended) for q in suspended):
            raise ValueError("resume needs one Suspended per slot")
        slots = self._slots(slots, busy="take or suspend")
        if self.den.precision_check is not None and not self.den._precision_checked:
            raise RuntimeError("the precision self-check of this Denoiser is pending: it runs on an admission into an idle loop, never on a "
                               "resume (admit a request first, or build the Denoiser with precision_check=None)")
        shape = self.den.engine.state_shape()
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
        # (the slots keep the requests without their states)
        self._enter(slots, [SlotRequest(*(getattr(q, f) for f in q.FIELDS[2:])) for q in suspended], done=[q.done for q in suspended],
                    state=torch.stack([q.state.to(self.dev) for q in suspended]).contiguous())

    def _check_known(self, n, knowns, known_masks, lengths):
        """the known frames of an admission, checked before any engine call: per request (known (100, L') tensor, mask (L',) bool
        array), L' <= T, or (None, None): no hold, which an all-False mask is too"""
        if knowns is None and known_masks is None:
            return [(None, None)] * n
        if knowns is None or known_masks is None or len(knowns) != n or len(known_masks) != n:
            raise ValueError("knowns and known_masks are given together, one entry (or None) per slot")
        nc = self.den.cfg.latent_channels
        out = []
        for k in range(n):
            kn, mk = knowns[k], known_masks[k]
            if kn is None and mk is None:
                out.append((None, None))
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
            out.append((kn, mk) if mk.any() else (None, None))
        return out

    def _self_check(self, slots, c_all, p_all, x_all, reqs, s) -> None:
        """the Denoiser's precision self-check on the first fill: the admitted requests' first evaluation point, the other slots idle"""
        import torch
        den, nb, dev, cfg = self.den, self.rep * self.B, c_all.device, self.den.cfg
        c = torch.zeros((nb, cfg.content_channels, self.T), dtype=torch.float32, device=dev)
        p = torch.zeros((nb, self.Lp, cfg.cross_attention_dim), dtype=torch.float32, device=dev)
        x = torch.zeros((nb, cfg.latent_channels, self.T), dtype=torch.float32, device=dev)
        t = torch.zeros((nb,), dtype=torch.float32, device=dev)
        for k, b in enumerate(slots):
            for h in range(self.rep):
                c[b + h * self.B], x[b + h * self.B], t[b + h * self.B] = c_all[k], x_all[k], float(reqs[k].table.coef[0, 0])
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
            ends = [it.end for it in self.items if it is not None]
            if not ends:
                return []
            n = max(0, min(ends) - self.step)
        if n < 0:
            raise ValueError("run(n) needs n >= 0")
        if n > 0:
            self.den.engine.sample_steps(int(n), use_graph=self.use_graph, stream=torch.cuda.current_stream(self.dev))
            self.step += int(n)
        return self.finished()

    def _free(self, b: int) -> None:
        """slot ``b`` becomes idle: its table's pool user goes back, and its own correction with it"""
        self.pool.release(self.items[b].req.key)
        self.items[b] = None
        if self.item_corrections:
            self.corrections[b] = None      # (reaches the engine with the next admission's vector; an idle slot reads nothing)

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
                self.pool.release(self.items[b].req.key)
                self.items[b] = None
        self.den._table_key = None

    def take(self, slots):
        """latents (n, 100, T) of the finished ``slots`` (zeros past each request's length); the slots become idle"""
        import torch
        slots = [int(b) for b in slots]
        bad = [b for b in slots if b < 0 or b >= self.B or self.items[b] is None or self.items[b].end > self.step]
        if bad:
            raise ValueError(f"slot(s) {bad} hold no finished request")
        out = torch.empty((len(slots), self.den.cfg.latent_channels, self.T), dtype=torch.float32, device=self.dev)
        self.den.engine.take(slots, out, stream=torch.cuda.current_stream(self.dev))
        for b in slots:
            self._free(b)
        return out
