"""Batched voice-conversion service on top of the denoiser engine -- SURVEY 8(f) rank 3.

The reference's ``Svc.infer`` (``inference/infer_tool.py:189-206``) converts ONE audio segment per call (batch 1,
``infer.py:99-140`` loops over the slicer's segments).  Here segments are converted in batches:

* segments are grouped by (latent length T, prompt length Lp) and never padded.  The reference applies no masking to
  padded LATENT frames (no self-attention / GroupNorm mask, ``model.py:411`` is commented out), and although padded
  PROMPT frames are masked out of cross-attention (``encoder_attention_mask``) they still enter both attention-pooled
  embeddings (``ref_enc`` ``model.py:362`` and the UNet's ``add_embedding``, which take no mask) -- so padding either
  side changes a segment's result (measured: 0.2-0.5 relative on the latent for a prompt padded 40 -> 64).  Grouping
  EQUAL shapes keeps every segment's result what the reference's batch-1 call gives, to within the precision's rounding
  noise (``ragged_prompts`` below lifts this for the prompt side).  A conversion job normally shares ONE reference clip over all its segments (``infer.py:92-122``: the segment loop sits inside the loop over reference clips), so Lp rarely
  splits a group.
* ``ragged=True``: segments are grouped by prompt length only, sorted longest first and packed into batches of at most
  ``max_batch``, each padded to its longest segment.  The denoiser runs the batch with per-item lengths
  (``Denoiser.sample(lengths=...)``, ``ns2vc_unet_set_lengths``): every GroupNorm statistic, self-attention softmax and
  convolution halo sees an item's own frames only, so a segment's result is what it gives alone, to the precision's rounding.
  Each segment's x_T is drawn as in the default mode, at its own length, then zero-padded.
* ``ragged_prompts=True``: the prompt length no longer splits a group.  The reference clips of a batch are zero-padded to the batch's
  longest, the front end runs with ``exact_prompt_lengths=True`` (the prompt encoder's conv halo and ``ref_enc``'s pooling see a clip's own
  frames only) and the denoiser with per-item prompt lengths (``Denoiser.sample(prompt_lengths=...)``, ``ns2vc_unet_set_prompt_lengths``):
  cross-attention AND the attention pooling of ``add_embedding`` take an item's own prompt frames, so a segment's result is what it gives
  alone with its own clip, to the precision's rounding -- the padding that costs 0.2-0.5 relative above reaches nothing.  Grouping is then by
  T only in the default mode, and one list of all segments, longest first, in ``ragged`` mode: a job with many reference clips still fills
  its batches.
* ``solver="ddim"`` (with ``eta``) / ``"ddpm"``: the reference's discrete samplers.  Their per-step noise comes from the segment's own
  seed (``noise.derive_seed(seed, index)``), so a segment's result does not depend on its group in either mode.
* ``Segment.schedule``: a segment's own sampler schedule (``Denoiser.sample(schedules=)``); it never splits a group -- a group whose segments differ runs as one batch, one captured loop.
* each group runs ``PreModel.infer`` -> ``Denoiser.sample`` -> ``decode_fn`` through ``OverlappedPipeline``: the
  PyTorch-ROCm front / back end of group k+1 / k-1 overlaps the HIP denoiser of group k on their own streams.

``decode_fn(latent (B, 100, T)) -> audio (B, samples)`` is the vocoder (Vocos in the reference, ``model.py:689-691``;
not a dependency of this repository: pass ``vocos.decode``); with ``decode_fn=None`` the latents are returned.
"""
from __future__ import annotations

from collections import defaultdict
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import torch

import numpy as np

from .frontend import PreModel
from .noise import derive_seed
from .pipeline import MASKED_OPTIONS, Denoiser, OverlappedPipeline
from .request import CORRECTION_KEYS, call_wide_kwargs
from .schedule import (ITEM_HIST2, ITEM_NOISE, build_table, plan_chains, plan_chunks, plan_slots, plan_slots_preemptive, schedule_key, table_flags,
                       table_options)


@dataclass
class Segment:
    """one unit of work: ContentVec features (256, T) already repeat-expanded to the mel frame rate
    (``utils.repeat_expand_2d``, ``infer_tool.py:158-168``) and the reference mel (100, Lp) (``infer_tool.py:170-182``)"""
    content: torch.Tensor
    refer: torch.Tensor
    tag: object = None
    # this segment's own sampler schedule -- dict(solver=, steps=, order=, eta=, table options), ``schedule.schedule_key`` -- or None = the
    # converter's.  Grouping ignores it: a group with different schedules runs as ONE batch (``Denoiser.sample(schedules=)``), and a
    # segment's result does not depend on its group
    schedule: Optional[dict] = None
    # this segment's own x0 correction -- dict(correcting_x0_fn=, thresholding_max_val=, dynamic_thresholding_ratio=), names only -- or None =
    # the converter's.  ``GroupedConverter`` serves a group whose segments differ through ``Denoiser.sample(corrections=)``,
    # ``ContinuousConverter(item_corrections=True)`` gives every request its own; a segment's result does not depend on its group
    correction: Optional[dict] = None
    # ``ContinuousConverter(preempt=True)``: a waiting segment of strictly higher priority suspends a running one of lower priority
    priority: int = 0


def segment_from_audio(content_encoder, wav16k: torch.Tensor, samples_at_target_rate: int, refer_mel: torch.Tensor, hop: int = 256,
                       tag: object = None, autocast=None) -> Segment:
    """``Svc.get_unit_f0_code`` minus the file I/O (``infer_tool.py:141-182``): the 16 kHz copy of ONE source segment -> ContentVec
    features (``ns2vc_amd.contentvec.ContentVec`` or anything with its ``content(wav16k, frames)``) stretched to the segment's latent
    frame count ``len(wav at 24 kHz) // hop`` (what the reference takes from its f0 track, ``utils.py:160``), plus the prompt mel."""
    frames = int(samples_at_target_rate) // hop
    return Segment(content=content_encoder.content(wav16k, frames, autocast=autocast)[0], refer=refer_mel, tag=tag)


class GroupedConverter:
    ragged = False      # the default mode (exact-shape groups), also for an instance that only plans (built without __init__)
    ragged_prompts = False

    def __init__(self, pre_model: PreModel, denoiser: Denoiser, decode_fn: Optional[Callable] = None, max_batch: int = 32,
                 solver: str = "unipc", steps: Optional[int] = 30, order: int = 2, seed: int = 1234, ragged: bool = False, eta: float = 0.0,
                 masked_fuse: Optional[bool] = None, masked_attn: Optional[bool] = None,
                 masked_rows: Optional[bool] = None, masked_ffn: Optional[bool] = None, masked_geglu: Optional[bool] = None,
                 masked_attn_resident: Optional[bool] = None,
                 ragged_prompts: bool = False, guidance_scale: float = 1.0, unconditional_prompt: Optional[torch.Tensor] = None,
                 correcting_x0_fn=None, thresholding_max_val: float = 1.0, dynamic_thresholding_ratio: float = 0.995, **options):
        """``correcting_x0_fn`` / ``thresholding_max_val`` / ``dynamic_thresholding_ratio``: the x0 correction of ``Denoiser.sample``, passed through.
        ``guidance_scale`` with ``unconditional_prompt`` (1, Lu, 256), one for every segment: classifier-free guidance
        (``Denoiser.sample``).  The engine then runs two items per segment, so a batch holds at most ``max_batch // 2`` segments."""
        self.pre, self.den, self.decode = pre_model, denoiser, decode_fn
        given = locals()
        for name in MASKED_OPTIONS:      # the denoiser's engine options of these names (ragged batches only); None leaves the denoiser's setting
            if given[name] is not None and bool(given[name]) != getattr(denoiser, name):
                denoiser.set_option(name, bool(given[name]))
        self.guided = unconditional_prompt is not None and float(guidance_scale) != 1.0
        if self.guided:
            if not np.isfinite(float(guidance_scale)):
                raise ValueError("guidance_scale must be finite")
            if len(unconditional_prompt.shape) != 3 or unconditional_prompt.shape[0] != 1:
                raise ValueError(f"unconditional_prompt must be (1, Lu, C), got {tuple(unconditional_prompt.shape)}")
            max_batch = max(1, max_batch // 2)
        self.max_batch, self.seed, self.ragged = max_batch, seed, ragged
        self.ragged_prompts = bool(ragged_prompts)
        if solver == "ddpm" and steps == 30:      # (the constructor's default step count is the continuous solvers'; ddpm runs every timestep)
            steps = None
        table_options(options)           # the keyword-only sampler options of Denoiser.sample (skip_type, denoise_to_zero, ...)
        self.kw = dict(solver=solver, steps=steps, order=order, eta=eta, **options)
        self.kw.update(call_wide_kwargs(solver, correcting_x0_fn, thresholding_max_val, dynamic_thresholding_ratio, float(guidance_scale),
                                        unconditional_prompt if self.guided else None))

    def _seeds(self, idx) -> np.ndarray:
        """per-SEGMENT noise seeds of the stochastic samplers, from the converter's seed and the segment's position in the input"""
        return np.array([derive_seed(self.seed, i) for i in idx], dtype=np.uint64)

    def plan(self, segments: Sequence[Segment]) -> List[List[int]]:
        """indices of `segments` grouped by (latent length, prompt length), groups of at most ``max_batch``, longest first;
        ``ragged``: grouped by prompt length only, each group's segments longest first (stable), cut into batches of at most ``max_batch``;
        ``ragged_prompts``: the prompt length splits nothing -- by latent length only, or (``ragged``) all segments longest first"""
        if self.ragged:
            by_lp: Dict[int, List[int]] = defaultdict(list)
            for i, s in enumerate(segments):
                by_lp[0 if self.ragged_prompts else int(s.refer.shape[-1])].append(i)
            groups = []
            for lp in sorted(by_lp, reverse=True):
                idx = sorted(by_lp[lp], key=lambda i: -int(segments[i].content.shape[-1]))
                groups += [idx[k:k + self.max_batch] for k in range(0, len(idx), self.max_batch)]
            return groups
        by_len: Dict[tuple, List[int]] = defaultdict(list)
        for i, s in enumerate(segments):
            by_len[(int(s.content.shape[-1]), 0 if self.ragged_prompts else int(s.refer.shape[-1]))].append(i)
        groups = []
        for key in sorted(by_len, reverse=True):
            idx = by_len[key]
            groups += [idx[k:k + self.max_batch] for k in range(0, len(idx), self.max_batch)]
        return groups

    def convert(self, segments: Sequence[Segment]) -> List[torch.Tensor]:
        """returns one tensor per segment, in input order: audio (samples,) with a ``decode_fn``, else the latent (100, T)"""
        dev = next(self.pre.parameters()).device
        groups = self.plan(segments)

        def padded_refer(idx):
            """ragged_prompts: the group's reference clips zero-padded to its longest, and their own lengths"""
            plens = [int(segments[i].refer.shape[-1]) for i in idx]
            refer = torch.zeros((len(idx), segments[idx[0]].refer.shape[0], max(plens)), dtype=torch.float32, device=dev)
            for b, i in enumerate(idx):
                refer[b, :, :plens[b]] = segments[i].refer.to(dev, torch.float32)
            return refer, plens

        def pre_fn(idx):
            cond = ragged_pre(idx) if self.ragged else dense_pre(idx)
            sch = [getattr(segments[i], "schedule", None) for i in idx]
            if any(v is not None for v in sch):
                cond["schedules"] = sch
            own = {k: self.kw[k] for k in CORRECTION_KEYS if k in self.kw} or None
            cor = [getattr(segments[i], "correction", None) for i in idx]
            if any(v is not None for v in cor):
                cond["corrections"] = [own if v is None else v for v in cor]
            return cond

        def dense_pre(idx):
            T, Lp = int(segments[idx[0]].content.shape[-1]), int(segments[idx[0]].refer.shape[-1])
            c = torch.stack([segments[i].content.to(dev, torch.float32) for i in idx])
            noise = torch.stack([torch.randn((self.den.cfg.latent_channels, T), generator=torch.Generator().manual_seed(self.seed + i)) for i in idx]).to(dev)
            if self.ragged_prompts:
                refer, plens = padded_refer(idx)
                content, prompt, _ = self.pre.infer(c, refer, torch.full((len(idx),), T, device=dev), torch.tensor(plens, device=dev),
                                                    exact_prompt_lengths=True)
                return {"content": content, "prompt": prompt, "prompt_mask": None, "noise": noise, "seeds": self._seeds(idx), "prompt_lengths": plens}
            refer = torch.stack([segments[i].refer.to(dev, torch.float32) for i in idx])
            content, prompt, mask = self.pre.infer(c, refer, torch.full((len(idx),), T, device=dev), torch.full((len(idx),), Lp, device=dev))
            # x_T per SEGMENT (seeded by its position in the input), so a segment's result does not depend on its group
            return {"content": content, "prompt": prompt, "prompt_mask": mask, "noise": noise, "seeds": self._seeds(idx)}

        def ragged_pre(idx):
            lens = [int(segments[i].content.shape[-1]) for i in idx]
            T, Lp = max(lens), int(segments[idx[0]].refer.shape[-1])
            c = torch.zeros((len(idx), segments[idx[0]].content.shape[0], T), dtype=torch.float32, device=dev)
            noise = torch.zeros((len(idx), self.den.cfg.latent_channels, T), dtype=torch.float32)
            for b, i in enumerate(idx):
                c[b, :, :lens[b]] = segments[i].content.to(dev, torch.float32)
                # x_T per SEGMENT at its own length (as in the default mode), zero-padded: its result does not depend on its batch
                noise[b, :, :lens[b]] = torch.randn((self.den.cfg.latent_channels, lens[b]), generator=torch.Generator().manual_seed(self.seed + i))
            if self.ragged_prompts:
                refer, plens = padded_refer(idx)
                content, prompt, _ = self.pre.infer(c, refer, torch.tensor(lens, device=dev), torch.tensor(plens, device=dev), exact_lengths=True,
                                                    exact_prompt_lengths=True)
                return {"content": content, "prompt": prompt, "prompt_mask": None, "noise": noise.to(dev), "lengths": lens, "seeds": self._seeds(idx),
                        "prompt_lengths": plens}
            refer = torch.stack([segments[i].refer.to(dev, torch.float32) for i in idx])
            content, prompt, mask = self.pre.infer(c, refer, torch.tensor(lens, device=dev), torch.full((len(idx),), Lp, device=dev),
                                                   exact_lengths=True)
            return {"content": content, "prompt": prompt, "prompt_mask": mask, "noise": noise.to(dev), "lengths": lens, "seeds": self._seeds(idx)}

        def post_fn(latent, idx):
            if self.ragged:     # one tensor per segment, cut to its own frames
                lat = [latent[b, :, :int(segments[i].content.shape[-1])] for b, i in enumerate(idx)]
                return lat if self.decode is None else [self.decode(x[None])[0] for x in lat]
            return latent if self.decode is None else self.decode(latent)

        outs = OverlappedPipeline(self.den, pre_fn, post_fn, **self.kw).run(groups)
        result: List[Optional[torch.Tensor]] = [None] * len(segments)
        for idx, o in zip(groups, outs):
            for b, i in enumerate(idx):
                result[i] = o[b]
        return result


class ContinuousConverter:
    """Continuous batching: the segments are a QUEUE drained through ``slots`` slots of one running loop
    (``Denoiser.open_slots``) instead of closed batches.  A slot that finishes is taken and gets the next segment of the queue at once, so
    a 10-step preview does not wait for the 50-step render beside it and no slot-step is spent holding a finished item; which slot takes
    which segment, how far the loop steps and when a slot is retired is decided by the pure function ``schedule.plan_slots``.  The engine
    is prepared once for (``slots``, ``max_frames``, ``max_prompt``); every segment runs with its own length and prompt length.  The front
    end runs per admitted group with exact lengths (``exact_lengths`` / ``exact_prompt_lengths``); x_T and the noise seed are per segment,
    drawn as ``GroupedConverter`` draws them, so a segment's result does not depend on its slot or its neighbours.  ``Segment.schedule``
    is honoured.  Options as ``GroupedConverter``'s; schedules that need an fp32 tail at the denoiser's precision are refused
    (``SlotLoop``).

    ``overlap_frames=V`` (0 <= V < ``max_frames``): a segment longer than ``max_frames`` is no longer refused but cut by
    ``schedule.plan_chunks(L, max_frames, V)``, and every chunk is a request of the same loop at its own length.  The front end runs once
    per long segment on its whole length -- its content is sliced per chunk, its prompt shared --, x_T is the segment's full-length draw,
    sliced, and the seed is reused per chunk, as in ``Denoiser.sample_long``.  Chunk j + 1 holds its first V frames at the last V latent
    frames chunk j's ``take`` returned (a device-side slice on the loop's stream: the host never waits between chunks), and becomes ready
    when chunk j has finished: the scheduling is ``schedule.plan_chains``, request ids ``(segment, chunk)`` in ``last_plan``.  The result is
    chunk 0 whole, then every later chunk from frame V on.  Short segments ride along unchanged.

    ``preempt=True``: the loop follows ``schedule.plan_slots_preemptive`` on ``Segment.priority`` -- when every slot is busy
    and a segment of strictly higher priority has arrived, the running segment of lowest priority is suspended (``SlotLoop.suspend``: its
    solver state is copied out, its slot freed) and resumed when a slot is free again (``SlotLoop.resume``), bit-exact where it returns to
    the slot index it left.  ``last_plan`` then holds that planner's 4-tuples ``(loop_step, take, suspend, admit)``.  ``convert(segments,
    arrivals=)`` replays a recorded arrival pattern: ``arrivals[i]`` = the loop step from which segment i may start (non-decreasing), as
    ``plan_slots`` takes them; an online submit / poll front is not part of this class.  Not together with ``overlap_frames``."""

    def __init__(self, pre_model: PreModel, denoiser: Denoiser, decode_fn: Optional[Callable] = None, slots: int = 32, max_frames: int = 938,
                 max_prompt: int = 469, solver: str = "unipc", steps: Optional[int] = 30, order: int = 2, seed: int = 1234, eta: float = 0.0,
                 guidance_scale: float = 1.0, unconditional_prompt: Optional[torch.Tensor] = None, correcting_x0_fn=None,
                 thresholding_max_val: float = 1.0, dynamic_thresholding_ratio: float = 0.995, use_graph: bool = True,
                 item_corrections: bool = False, overlap_frames: Optional[int] = None, preempt: bool = False, **options):
        """``item_corrections``: ``Segment.correction`` is honoured -- the loop is opened with the per-item x0 correction table and every
        segment is admitted with its own entry (None = uncorrected); not together with the loop-wide ``correcting_x0_fn=``."""
        self.pre, self.den, self.decode = pre_model, denoiser, decode_fn
        self.item_corrections = bool(item_corrections)
        self.overlap = None if overlap_frames is None else int(overlap_frames)
        self.preempt = bool(preempt)
        if self.preempt and overlap_frames is not None:
            raise ValueError("preempt=True does not go with overlap_frames (chained chunks are not suspended): use one or the other")
        if self.overlap is not None and not 0 <= self.overlap < int(max_frames):
            raise ValueError(f"overlap_frames must be in [0, max_frames = {int(max_frames)}), got {overlap_frames}")
        self.slots, self.max_frames, self.max_prompt, self.seed, self.use_graph = int(slots), int(max_frames), int(max_prompt), seed, use_graph
        self.guided = unconditional_prompt is not None and float(guidance_scale) != 1.0
        self.scale = float(guidance_scale) if self.guided else 1.0
        self.uncond = unconditional_prompt if self.guided else None
        if solver == "ddpm" and steps == 30:
            steps = None
        table_options(options)
        if steps is None:
            steps = {"ddim": 100, "ddpm": len(denoiser.betas64)}.get(solver, 20)
        self.own = dict(solver=solver, steps=int(steps), order=order, eta=eta, **options)
        self.corr = call_wide_kwargs(None, correcting_x0_fn, thresholding_max_val, dynamic_thresholding_ratio)      # (the loop checks every request's solver)
        if self.item_corrections and self.corr:
            raise ValueError("item_corrections=True (Segment.correction) and the loop-wide correcting_x0_fn= exclude each other")
        if self.overlap and (self.item_corrections or self.corr):
            raise ValueError("overlap_frames > 0 (chunks that hold known frames) does not go with an x0 correction (correcting_x0_fn=, "
                             "item_corrections=True): it would rescale the held frames")
        self.last_plan = None          # (events of the last convert: tests, utilisation figures)

    def convert(self, segments: Sequence[Segment], arrivals: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
        """returns one tensor per segment, in input order: audio (samples,) with a ``decode_fn``, else the latent (100, T_i).  ``arrivals``:
        None (all queued at once) or one non-decreasing loop step per segment from which it may start -- the replay of a recorded arrival
        pattern; not with chained chunks (``overlap_frames`` and a segment longer than ``max_frames``)."""
        dev = next(self.pre.parameters()).device
        if arrivals is not None and self.overlap is not None and any(int(s.content.shape[-1]) > self.max_frames for s in segments):
            raise ValueError("arrivals= does not go with chained chunks (a segment longer than max_frames under overlap_frames)")
        specs = [s.schedule if getattr(s, "schedule", None) is not None else self.own for s in segments]
        for i, s in enumerate(segments):
            if (int(s.content.shape[-1]) > self.max_frames and self.overlap is None) or int(s.refer.shape[-1]) > self.max_prompt:
                raise ValueError(f"segment {i} has {int(s.content.shape[-1])} frames and {int(s.refer.shape[-1])} prompt frames: the slots take "
                                 f"{self.max_frames} and {self.max_prompt}")
        built = {}                     # one table per distinct schedule, shared with the loop
        for i, sp in enumerate(specs):
            k = schedule_key(sp, i)
            if k not in built:
                built[k] = build_table(k[0], k[1], self.den._betas_for(k[0]), k[2], k[3], **dict(k[4]))
        tables = [built[schedule_key(sp)] for sp in specs]
        cors = [getattr(s, "correction", None) if self.item_corrections else None for s in segments]
        V = self.overlap or 0
        chunks = [plan_chunks(int(s.content.shape[-1]), self.max_frames, V) if self.overlap is not None else [(0, int(s.content.shape[-1]))]
                  for s in segments]
        chained = max((len(c) for c in chunks), default=1) > 1
        kw = dict(self.corr, known_frames=True) if chained and V > 0 else self.corr      # (the form only where a chunk holds frames: else the plain loop)
        loop = self.den.open_slots(self.slots, self.max_frames, self.max_prompt, order3=any(table_flags(t) & ITEM_HIST2 for t in tables),
                                   stochastic=any(table_flags(t) & ITEM_NOISE for t in tables), unconditional_prompt=self.uncond,
                                   use_graph=self.use_graph, item_corrections=self.item_corrections, **kw)
        loop._tables.update(built)
        try:
            for sp, cor in zip(specs, cors):      # every refusal before anything runs
                loop.check_request(sp, self.scale, cor)
            # requests are (segment, chunk); with one chunk per segment these are plan_slots' events, and last_plan shows them in its format
            if self.preempt:
                self.last_plan = plan_slots_preemptive([t.steps for t in tables], self.slots, arrivals,
                                                       [int(getattr(s, "priority", 0)) for s in segments])
                plan = [(r, [(b, (i, 0)) for b, i in take], suspend, [(b, (i, 0), d) for b, i, d in admit]) for r, take, suspend, admit in self.last_plan]
            else:
                if arrivals is not None:
                    events = [(r, [(b, (i, 0)) for b, i in take], [(b, (i, 0)) for b, i in admit])
                              for r, take, admit in plan_slots([t.steps for t in tables], self.slots, arrivals)]
                else:
                    events = plan_chains([[tables[i].steps] * len(chunks[i]) for i in range(len(segments))], self.slots)
                self.last_plan = events if chained else [(r, [(b, i) for b, (i, _) in take], [(b, i) for b, (i, _) in admit]) for r, take, admit in events]
                plan = [(r, take, [], [(b, q, 0) for b, q in admit]) for r, take, admit in events]
            held: Dict[int, object] = {}        # suspended segment -> its Suspended, until it is resumed
            result: List[Optional[torch.Tensor]] = [None] * len(segments)
            nc = self.den.cfg.latent_channels
            front: Dict[int, tuple] = {}        # long segment -> (content (256, L), prompt (lp, 256), x_T (100, L), latent (100, L)) until its last chunk
            tails: Dict[int, torch.Tensor] = {}  # long segment -> the last V latent frames of its latest chunk, until the next chunk is admitted

            def pre(idx):
                """the front end on the whole length of the segments ``idx``, with exact lengths"""
                lens = [int(segments[i].content.shape[-1]) for i in idx]
                plens = [int(segments[i].refer.shape[-1]) for i in idx]
                c = torch.zeros((len(idx), segments[idx[0]].content.shape[0], max(lens)), dtype=torch.float32, device=dev)
                refer = torch.zeros((len(idx), segments[idx[0]].refer.shape[0], max(plens)), dtype=torch.float32, device=dev)
                for k, i in enumerate(idx):
                    c[k, :, :lens[k]] = segments[i].content.to(dev, torch.float32)
                    refer[k, :, :plens[k]] = segments[i].refer.to(dev, torch.float32)
                content, prompt, _ = self.pre.infer(c, refer, torch.tensor(lens, device=dev), torch.tensor(plens, device=dev), exact_lengths=True,
                                                    exact_prompt_lengths=True)
                return content, prompt

            def draw(i):
                # x_T per SEGMENT at its own length, seeded by its position in the input (as GroupedConverter): its result does not depend on its slot
                return torch.randn((nc, int(segments[i].content.shape[-1])), generator=torch.Generator().manual_seed(self.seed + i)).to(dev)

            for r, take, suspend, placed in plan:
                if r > loop.step:
                    loop.run(r - loop.step)
                if take:
                    lat = loop.take([b for b, _ in take])
                    for k, (_, (i, j)) in enumerate(take):
                        start, stop = chunks[i][j]
                        x = lat[k, :, :stop - start]
                        if len(chunks[i]) > 1:      # chunk 0 whole, every later chunk from frame V on
                            keep = V if j > 0 else 0
                            front[i][3][:, start + keep:stop] = x[:, keep:]
                            if j + 1 < len(chunks[i]):
                                if V > 0:
                                    tails[i] = x[:, stop - start - V:]
                                continue
                            x = front.pop(i)[3]
                        result[i] = x if self.decode is None else self.decode(x[None])[0]
                if suspend:
                    for (_, i, _), q in zip(suspend, loop.suspend([b for b, _, _ in suspend])):
                        held[i] = q
                back = [(b, i) for b, (i, _), d in placed if d > 0]
                if back:
                    loop.resume([b for b, _ in back], [held.pop(i) for _, i in back])
                admit = [(b, q) for b, q, d in placed if d == 0]
                if admit:
                    short = [i for _, (i, _) in admit if len(chunks[i]) == 1]
                    if short:      # the short segments of the group in one front-end batch
                        content, prompt = pre(short)
                    cs, ps, xs, lens, plens, kns, kms = [], [], [], [], [], [], []
                    for _, (i, j) in admit:
                        L, lp = int(segments[i].content.shape[-1]), int(segments[i].refer.shape[-1])
                        start, stop = chunks[i][j]
                        if len(chunks[i]) == 1:
                            c_i, p_i, x_i = content[short.index(i)], prompt[short.index(i)], draw(i)
                        else:
                            if i not in front:      # the front end once per long segment; x_T its full-length draw; the stitched latent
                                c_w, p_w = pre([i])
                                front[i] = (c_w[0, :, :L], p_w[0, :lp], draw(i), torch.zeros((nc, L), dtype=torch.float32, device=dev))
                            c_i, p_i, x_i = front[i][0][:, start:stop], front[i][1], front[i][2][:, start:stop]
                        kn = km = None
                        if j > 0 and V > 0:      # the frames the earlier chunk ended on, held at the head of this one
                            kn = torch.zeros((nc, stop - start), dtype=torch.float32, device=dev)
                            kn[:, :V] = tails.pop(i)
                            km = np.zeros((stop - start,), dtype=bool)
                            km[:V] = True
                        for lst, v in ((cs, c_i), (ps, p_i), (xs, x_i), (lens, stop - start), (plens, lp), (kns, kn), (kms, km)):
                            lst.append(v)
                    idx = [i for _, (i, _) in admit]
                    hold = dict(knowns=kns, known_masks=kms) if any(k is not None for k in kns) else {}
                    loop.admit_group([b for b, _ in admit], cs, ps, xs, lens, plens, [specs[i] for i in idx], [int(derive_seed(self.seed, i)) for i in idx],
                                     [self.scale] * len(idx), [cors[i] for i in idx], **hold)
            torch.cuda.current_stream(dev).synchronize()
        finally:                       # also after an error in mid-queue: no busy slot is left behind, the denoiser serves the next call
            loop.close()
        return result
