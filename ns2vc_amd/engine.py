"""Host-side handle on the HIP denoiser engine (libns2vc_hip.so).

Pure ctypes + numpy: torch is optional and used only as a source of device
pointers / streams (plumbing).  Everything computes on the GPU through the C
ABI; there is no CPU path here — missing library or GPU raises ``Ns2vcError``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Tuple

import numpy as np

from . import _lib
from ._lib import Ns2vcError, PREC_BF16, PREC_F16, PREC_F32, check
from .schedule import NCOEF, ItemTables, SolverTable, build_table, build_tables, check_x0_correction
from .spec import UNetConfig, engine_block_types, engine_supports, param_spec

# operand precision of the MFMAs (include/ns2vc_hip.h): fp16 is the default 16-bit mode -- same speed and bytes as bf16,
# 7e-4 end-to-end error (inside the 1e-3 parity gate) instead of 5.7e-3
PRECISIONS = {"fp32": PREC_F32, "f32": PREC_F32, "bf16": PREC_BF16, "fp16": PREC_F16, "f16": PREC_F16}
DEFAULT_PRECISION = "fp16"


class DevBuf:
    """A raw device allocation made through the C ABI (torch-free tests / bench)."""

    def __init__(self, nbytes: int):
        self.lib = _lib.load()
        p = C.c_void_p()
        check(self.lib.ns2vc_dev_malloc(C.byref(p), nbytes), "ns2vc_dev_malloc")
        self.ptr = p.value
        self.nbytes = nbytes

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DevBuf":
        a = np.ascontiguousarray(a)
        b = cls(a.nbytes)
        check(b.lib.ns2vc_memcpy_h2d(b.ptr, a.ctypes.data, a.nbytes), "memcpy_h2d")
        return b

    def upload(self, a: np.ndarray) -> None:
        a = np.ascontiguousarray(a)
        assert a.nbytes <= self.nbytes
        check(self.lib.ns2vc_memcpy_h2d(self.ptr, a.ctypes.data, a.nbytes), "memcpy_h2d")

    def to_numpy(self, shape, dtype=np.float32) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(self.lib.ns2vc_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes), "memcpy_d2h")
        return out

    def free(self) -> None:
        if self.ptr:
            self.lib.ns2vc_dev_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr(x) -> int:
    """Device pointer of a DevBuf / torch CUDA tensor / raw int."""
    if x is None:
        return 0
    if isinstance(x, DevBuf):
        return x.ptr
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):          # torch tensor
        if not x.is_cuda:
            raise Ns2vcError("tensor must live on the GPU: the engine has no CPU path")
        if not x.is_contiguous():
            raise Ns2vcError("tensor must be contiguous")
        return x.data_ptr()
    raise TypeError(f"cannot take a device pointer of {type(x)}")


class Stream:
    """A HIP stream: non-blocking without a mask; with ``cu_mask`` it is created by hipExtStreamCreateWithCUMask, which makes a DEFAULT
    (blocking) stream -- it synchronises implicitly with the legacy null stream, so keep other work off the null stream when overlapping.  ``cu_mask`` (an iterable of CU indices, or None): restrict the stream's kernels to those CUs
    (``hipExtStreamCreateWithCUMask``) -- how a pipeline gives the PyTorch stages a slice of the chip beside the denoiser."""

    def __init__(self, cu_mask=None):
        self.lib = _lib.load()
        p = C.c_void_p()
        if cu_mask is None:
            check(self.lib.ns2vc_stream_create(C.byref(p)), "stream_create")
        else:
            cus = sorted(set(int(c) for c in cu_mask))
            if not cus or cus[0] < 0:
                raise ValueError("cu_mask must name at least one CU")
            nw = cus[-1] // 32 + 1
            words = (C.c_uint32 * nw)()
            for c in cus:
                words[c // 32] |= 1 << (c % 32)
            check(self.lib.ns2vc_stream_create_cu_mask(C.byref(p), words, nw), "stream_create_cu_mask")
        self.ptr = p.value

    def sync(self):
        check(self.lib.ns2vc_stream_sync(self.ptr), "stream_sync")

    def __del__(self):
        try:
            if self.ptr:
                self.lib.ns2vc_stream_destroy(self.ptr)
        except Exception:
            pass


class Event:
    def __init__(self):
        self.lib = _lib.load()
        p = C.c_void_p()
        check(self.lib.ns2vc_event_create(C.byref(p)), "event_create")
        self.ptr = p.value

    def record(self, stream) -> None:
        check(self.lib.ns2vc_event_record(self.ptr, _stream_ptr(stream)), "event_record")

    def elapsed_ms(self, end: "Event") -> float:
        ms = C.c_float()
        check(self.lib.ns2vc_event_elapsed_ms(self.ptr, end.ptr, C.byref(ms)), "event_elapsed")
        return float(ms.value)

    def __del__(self):
        try:
            if self.ptr:
                self.lib.ns2vc_event_destroy(self.ptr)
        except Exception:
            pass


def _stream_ptr(s) -> int:
    if s is None:
        return 0
    if isinstance(s, Stream):
        return s.ptr
    if isinstance(s, int):
        return s
    if hasattr(s, "cuda_stream"):       # torch.cuda.Stream
        return int(s.cuda_stream)
    raise TypeError(f"not a stream: {type(s)}")


def device_info() -> str:
    lib = _lib.load()
    buf = C.create_string_buffer(256)
    check(lib.ns2vc_device_name(buf, 256), "device_name")
    return buf.value.decode()


def set_device(index: int) -> None:
    check(_lib.load().ns2vc_set_device(int(index)), "set_device")


def xcd_round_robin() -> int:
    """1 when workgroup ids 8 apart share an XCD on the current device (probed once; what the cooperative GroupNorm prologue relies
    on, its default), 0 when not, -1 when the probe could not run."""
    n = C.c_int(0)
    check(_lib.load().ns2vc_device_xcd_round_robin(C.byref(n)), "xcd_round_robin")
    return int(n.value)


def device_count() -> int:
    lib = _lib.load()
    n = C.c_int()
    rc = lib.ns2vc_device_count(C.byref(n))
    return int(n.value) if rc == 0 else 0


class Engine:
    """One denoiser instance: weights + workspace for a (B, T, Lp) shape."""

    def __init__(self, cfg: UNetConfig = UNetConfig(), precision: str = DEFAULT_PRECISION):
        cfg.validate()
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(PRECISIONS)}")
        if (tuple(cfg.down_block_types), tuple(cfg.up_block_types)) != engine_block_types(len(cfg.block_out_channels)):
            raise ValueError(engine_supports(cfg))     # the C ABI does not carry block types: the engine would build another topology
        self.cfg = cfg
        self.precision = precision
        self.lib = _lib.load()
        c = _lib.UnetCfg()
        c.latent_channels = cfg.latent_channels
        c.content_channels = cfg.content_channels
        c.n_levels = len(cfg.block_out_channels)
        for i, v in enumerate(cfg.block_out_channels):
            c.block_out_channels[i] = v
        c.norm_num_groups = cfg.norm_num_groups
        c.cross_attention_dim = cfg.cross_attention_dim
        c.heads = cfg.heads
        c.layers_per_block = cfg.layers_per_block
        c.pool_heads = cfg.addition_embed_heads
        h = C.c_void_p()
        check(self.lib.ns2vc_unet_create(C.byref(c), C.byref(h)), "ns2vc_unet_create")
        self.h = h
        self.shape: Optional[Tuple[int, int, int]] = None
        self.lengths: Optional[np.ndarray] = None      # per-item valid frames (set_lengths), None = dense
        self.prompt_lengths: Optional[np.ndarray] = None   # per-item prompt frames (set_prompt_lengths), None = every item Lp
        self.guidance: Optional[np.ndarray] = None      # per-item guidance scales (set_guidance), None = unguided
        self.x0_correction = None                       # (mode 1 | 2, ratio, max_val) of set_x0_correction, None = off
        self.x0_corrections = None                      # (modes, ratios, max_vals) of set_x0_correction_items, None = off
        self.hold: Optional[np.ndarray] = None          # the (n, T) bool frame mask of set_known, None = no known frames
        self.table: Optional[SolverTable] = None
        self.tables: Optional[ItemTables] = None        # per-item schedules (load_samplers); None = the shared table
        self._weights_ready = False
        self._debug = False

    # -- weights ----------------------------------------------------------------
    def load_state_dict(self, state: Dict[str, object], strict: bool = True) -> None:
        """``state``: name -> numpy array / torch tensor (CPU or GPU), reference key names
        (optionally prefixed ``diff_model.unet.`` as in a full NS2VC checkpoint)."""
        spec = param_spec(self.cfg)
        prefix = "diff_model.unet."
        seen = set()
        for name, shape in spec.items():
            v = state.get(name, state.get(prefix + name))
            if v is None:
                if strict:
                    raise KeyError(f"missing weight {name}")
                continue
            seen.add(name)
            shp = (C.c_int64 * len(shape))(*shape)
            if hasattr(v, "data_ptr"):      # torch
                t = v.detach()
                if tuple(t.shape) != tuple(shape):
                    raise ValueError(f"{name}: shape {tuple(t.shape)} != {tuple(shape)}")
                import torch  # plumbing only
                t = t.to(dtype=torch.float32).contiguous()
                check(self.lib.ns2vc_unet_load_weight(self.h, name.encode(), t.data_ptr(), shp, len(shape)), name)
            else:
                a = np.ascontiguousarray(np.asarray(v), dtype=np.float32)
                if tuple(a.shape) != tuple(shape):
                    raise ValueError(f"{name}: shape {tuple(a.shape)} != {tuple(shape)}")
                check(self.lib.ns2vc_unet_load_weight(self.h, name.encode(), a.ctypes.data, shp, len(shape)), name)
        if strict:
            extra = [k for k in state if k not in spec and not (k.startswith(prefix) and k[len(prefix):] in spec)
                     and k.startswith(("conv_", "time_embedding", "add_embedding", "down_blocks", "up_blocks", "mid_block"))]
            if extra:
                raise KeyError(f"unexpected denoiser keys: {extra[:4]}")
        check(self.lib.ns2vc_unet_finalize_weights(self.h, PRECISIONS[self.precision]), "finalize_weights")
        self._weights_ready = True
        self.shape = None

    # -- workspace ----------------------------------------------------------------
    def set_debug(self, enable: bool) -> None:
        """Keep a copy of every block output (``taps()``).  Changing it drops the plan: call ``prepare`` afterwards."""
        check(self.lib.ns2vc_unet_set_debug(self.h, int(enable)), "set_debug")
        if bool(enable) != self._debug:
            self._debug = bool(enable)
            self.shape = None

    def set_option(self, name: str, value: bool) -> None:
        """Plan options ("ln_linear", "fold_ff", "fuse_gn_gemm", "attn_optimistic", ...; include/ns2vc_hip.h).  Changing one drops
        the plan: ``prepare`` again."""
        check(self.lib.ns2vc_unet_set_option(self.h, name.encode(), int(value)), f"set_option({name})")
        self.shape = None

    def ln_ratio(self, stream=None) -> float:
        """max |mean| / std over all LayerNorm input rows since the last read-out.  The read-and-reset is enqueued on
        ``stream`` (pass the stream the evaluations ran on) and only THAT stream is synchronised.  The 16-bit modes' error
        on a LayerNorm row grows with it under the default "ln_linear" plan; see ``Denoiser`` for the automatic guard."""
        r = C.c_float()
        check(self.lib.ns2vc_unet_ln_ratio(self.h, C.byref(r), _stream_ptr(stream)), "ln_ratio")
        return float(r.value)

    def ln_ratio_post(self, stream=None) -> None:
        """enqueue the read-and-reset on ``stream`` without waiting; collect it with ``ln_ratio_poll``"""
        check(self.lib.ns2vc_unet_ln_ratio_post(self.h, _stream_ptr(stream)), "ln_ratio_post")

    def ln_ratio_poll(self) -> Optional[float]:
        """value of the last ``ln_ratio_post`` if it has completed (non-blocking), else None"""
        r, ok = C.c_float(), C.c_int()
        check(self.lib.ns2vc_unet_ln_ratio_poll(self.h, C.byref(r), C.byref(ok)), "ln_ratio_poll")
        return float(r.value) if ok.value else None

    def prepare(self, B: int, T: int, Lp: int) -> None:
        check(self.lib.ns2vc_unet_prepare(self.h, B, T, Lp), "ns2vc_unet_prepare")
        self.shape = (B, T, Lp)
        self.lengths = None
        self.prompt_lengths = None
        self.guidance = None
        self.hold = None

    def workspace_bytes(self) -> int:
        n = C.c_size_t()
        check(self.lib.ns2vc_unet_workspace_bytes(self.h, C.byref(n)), "workspace_bytes")
        return int(n.value)

    def launches(self) -> Tuple[int, int]:
        a, b = C.c_int(), C.c_int()
        check(self.lib.ns2vc_unet_num_launches(self.h, C.byref(a), C.byref(b)), "num_launches")
        return int(a.value), int(b.value)

    # -- compute (device pointers in, device pointers out) --------------------------
    def set_condition(self, content, prompt, mask=None, stream=None) -> None:
        """content (B,256,T) fp32, prompt (B,Lp,256) fp32, mask (B,Lp) uint8/bool or None — all on the GPU."""
        check(self.lib.ns2vc_unet_set_condition(self.h, _ptr(content), _ptr(prompt), _ptr(mask), _stream_ptr(stream)), "set_condition")

    def set_content(self, content, stream=None) -> None:
        """only the content half of set_condition (the content part of conv_in)"""
        check(self.lib.ns2vc_unet_set_content(self.h, _ptr(content), _stream_ptr(stream)), "set_content")

    def set_prompt(self, prompt, mask=None, stream=None) -> None:
        """only the prompt half of set_condition (cross-attention K/V, add_embedding, mask bias)"""
        check(self.lib.ns2vc_unet_set_prompt(self.h, _ptr(prompt), _ptr(mask), _stream_ptr(stream)), "set_prompt")

    def set_mask(self, mask=None, stream=None) -> None:
        """only the keep-mask -> additive-bias conversion (None = no mask)"""
        check(self.lib.ns2vc_unet_set_mask(self.h, _ptr(mask), _stream_ptr(stream)), "set_mask")

    def set_lengths(self, lengths=None, stream=None) -> None:
        """Per-item valid frames of the prepared (B, T) batch: a sequence / array / tensor of B ints in [1, T], or None = dense.  Item b then
        gives on frames [0, L_b) what it gives alone at T = L_b, and 0 beyond.  Call before set_condition / set_content; prepare() resets it."""
        if lengths is None:
            check(self.lib.ns2vc_unet_set_lengths(self.h, None, _stream_ptr(stream)), "set_lengths")
            self.lengths = None
            return
        if hasattr(lengths, "detach"):
            lengths = lengths.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(lengths).reshape(-1), dtype=np.int32)
        if self.shape is not None and a.shape[0] != self.shape[0]:
            raise ValueError(f"lengths has {a.shape[0]} entries, the prepared batch {self.shape[0]}")
        check(self.lib.ns2vc_unet_set_lengths(self.h, a.ctypes.data, _stream_ptr(stream)), "set_lengths")
        self.lengths = a.copy()

    def set_prompt_lengths(self, prompt_lengths=None, stream=None) -> None:
        """Per-item prompt frames of the prepared (B, Lp) batch: a sequence / array / tensor of B ints in [1, Lp], or None = every item Lp.
        Item b then gives what it gives alone with a prompt of prompt_lengths[b] frames and no mask; whatever the prompt rows past them hold
        reaches no result.  Call before set_condition / set_prompt; prepare() resets it."""
        if prompt_lengths is None:
            check(self.lib.ns2vc_unet_set_prompt_lengths(self.h, None, _stream_ptr(stream)), "set_prompt_lengths")
            self.prompt_lengths = None
            return
        if hasattr(prompt_lengths, "detach"):
            prompt_lengths = prompt_lengths.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(prompt_lengths).reshape(-1), dtype=np.int32)
        if self.shape is None or a.shape[0] != self.shape[0]:
            raise ValueError(f"prompt_lengths has {a.shape[0]} entries, the prepared batch {None if self.shape is None else self.shape[0]}")
        check(self.lib.ns2vc_unet_set_prompt_lengths(self.h, a.ctypes.data, _stream_ptr(stream)), "set_prompt_lengths")
        self.prompt_lengths = a.copy()

    def set_seeds(self, seeds, stream=None) -> None:
        """(B,) 64-bit seeds of the per-item noise streams of a stochastic table (ns2vc_amd.noise), for the prepared batch;
        cleared by ``prepare``.  Asynchronous on ``stream``: a captured step graph stays valid."""
        if hasattr(seeds, "detach"):
            seeds = seeds.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(seeds).reshape(-1).astype(np.uint64))
        items = None if self.shape is None else (self.shape[0] if self.guidance is None else self.guidance.shape[0])
        if a.shape[0] != items:
            raise ValueError(f"seeds has {a.shape[0]} entries, the prepared batch {items}")
        check(self.lib.ns2vc_sampler_set_seeds(self.h, a.ctypes.data, _stream_ptr(stream)), "set_seeds")

    def set_guidance(self, scales=None, stream=None) -> None:
        """Classifier-free guidance of the sampling loop: (n,) finite per-item scales for an engine prepared with B = 2n whose condition is
        cat([unconditional, conditional]) (and whose ``lengths`` / ``prompt_lengths``, where set, have 2n entries, the latent lengths equal
        in both halves); None = off.  The loop's entry points (``sample*``, ``set_seeds``) then take and give n items, and every step
        combines ``x0_u + scale * (x0_c - x0_u)`` (``schedule.guided_x0``; scale 1 takes ``x0_c`` itself) in front of the solver update.
        Asynchronous on ``stream``: new values replay the captured step graph; on / off recaptures and clears the seeds.  ``prepare``
        turns it off."""
        if scales is None:
            check(self.lib.ns2vc_sampler_set_guidance(self.h, None, 0, _stream_ptr(stream)), "set_guidance")
            if self.guidance is not None:
                self.hold = None      # (on / off switches known frames off: their mask covered the other item count)
            self.guidance = None
            return
        if hasattr(scales, "detach"):
            scales = scales.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(scales).reshape(-1), dtype=np.float32)
        if self.shape is None or 2 * a.shape[0] != self.shape[0]:
            raise ValueError(f"guidance for {a.shape[0]} items needs an engine prepared with B = {2 * a.shape[0]}, "
                             f"not {None if self.shape is None else self.shape[0]}")
        if not np.all(np.isfinite(a)):
            raise ValueError("guidance scales must be finite")
        check(self.lib.ns2vc_sampler_set_guidance(self.h, a.ctypes.data, int(a.shape[0]), _stream_ptr(stream)), "set_guidance")
        if self.guidance is None:
            self.hold = None
        self.guidance = a.copy()

    def set_x0_correction(self, mode=None, ratio: float = 0.995, max_val: float = 1.0) -> None:
        """Correction of the predicted x0 inside the sampling loop, the reference solvers' ``correcting_x0_fn`` (``schedule.correct_x0``):
        ``mode`` None (off) | "dynamic_thresholding" (per item and step s = max(quantile_ratio(|m|), max_val), m = clamp(m, -s, s) / s, the
        quantile over the item's own frames and channels) | "clamp" (m = clamp(m, -max_val, max_val)).  ``mode`` may also be the engine's number 0 | 1 | 2.  A change of the
        mode, or of a value the active mode passes to its launches (clamp: max_val; dynamic thresholding: both), recaptures the step graph; ``prepare`` leaves the setting alone; a hand-off gives it to the tail.  Not with ddim / ddpm tables."""
        m = check_x0_correction(mode, ratio, max_val)
        check(self.lib.ns2vc_sampler_set_x0_correction(self.h, m, float(ratio), float(max_val)), "set_x0_correction")
        self.x0_correction = None if m == 0 else (m, float(np.float32(ratio)), float(np.float32(max_val)))

    def set_x0_correction_items(self, modes=None, ratios=None, max_vals=None, stream=None) -> None:
        """The x0 correction as a per-item table: loop item b is corrected by its own (modes[b], ratios[b], max_vals[b]) --
        one entry per loop item (n under guidance: set the guidance first), ``modes`` the names or numbers ``set_x0_correction`` takes;
        ``modes=None`` switches the table off.  Asynchronous on ``stream``: new values replay the captured step graph; on / off recaptures.
        Item b ends on the bits it has under ``set_x0_correction(modes[b], ratios[b], max_vals[b])``.  Not together with the loop-wide
        setting; needs per-item records (``load_samplers`` or a slot loop); a stochastic item takes mode None."""
        if modes is None:
            check(self.lib.ns2vc_sampler_set_x0_correction_items(self.h, None, None, None, 0, _stream_ptr(stream)), "set_x0_correction_items")
            self.x0_corrections = None
            return
        modes = list(modes)
        n = len(modes)
        ratios = [0.995] * n if ratios is None else list(ratios)
        max_vals = [1.0] * n if max_vals is None else list(max_vals)
        if len(ratios) != n or len(max_vals) != n:
            raise ValueError(f"{n} modes, {len(ratios)} ratios and {len(max_vals)} max_vals: one of each per loop item")
        m = np.ascontiguousarray([check_x0_correction(modes[b], ratios[b], max_vals[b]) for b in range(n)], dtype=np.int32)
        r = np.ascontiguousarray(ratios, dtype=np.float32)
        v = np.ascontiguousarray(max_vals, dtype=np.float32)
        check(self.lib.ns2vc_sampler_set_x0_correction_items(self.h, m.ctypes.data, r.ctypes.data, v.ctypes.data, n, _stream_ptr(stream)),
              "set_x0_correction_items")
        self.x0_corrections = (m.copy(), r.copy(), v.copy())

    def set_known(self, known=None, mask=None, stream=None) -> None:
        """Known frames of the sampling loop: ``known`` (n, latent, T) fp32 on the GPU, ``mask`` (n, T) bool on the host (array /
        tensor), n the loop items (set the guidance first).  Every step then overwrites the predicted x0 of the masked frames with ``known``
        in front of the solver update; start such a frame at ``schedule.known_start``.  Asynchronous on ``stream``: new values and new masks
        replay the captured step graph, on / off recaptures.  ``None, None`` switches it off; so do ``prepare`` and a change of guidance
        on / off.  Call after ``set_lengths`` (a held frame lies inside its item).  Not together with an x0 correction or a slot loop."""
        if known is None and mask is None:
            check(self.lib.ns2vc_sampler_set_known(self.h, None, None, 0, _stream_ptr(stream)), "set_known")
            self.hold = None
            return
        if known is None or mask is None:
            raise ValueError("known and mask are given together (None, None switches the hold off)")
        if hasattr(mask, "detach"):
            mask = mask.detach().cpu().numpy()
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        items = None if self.shape is None else (self.shape[0] if self.guidance is None else self.guidance.shape[0])
        if self.shape is None or m.shape != (items, self.shape[1]):
            raise ValueError(f"mask must be ({items}, {None if self.shape is None else self.shape[1]}) -- the loop's items and the prepared T --, got {m.shape}")
        if hasattr(known, "shape") and tuple(known.shape) != (items, self.cfg.latent_channels, self.shape[1]):
            raise ValueError(f"known must be ({items}, {self.cfg.latent_channels}, {self.shape[1]}), got {tuple(known.shape)}")
        if hasattr(known, "dtype") and "float32" not in str(known.dtype):
            raise ValueError(f"known must be float32, got {known.dtype}")
        check(self.lib.ns2vc_sampler_set_known(self.h, _ptr(known), m.ctypes.data, int(m.shape[0]), _stream_ptr(stream)), "set_known")
        self.hold = m.astype(bool)

    def forward(self, x, t, out, stream=None) -> None:
        """x (B,100,T), t (B,) fp32, out (B,100,T): one denoiser evaluation."""
        check(self.lib.ns2vc_unet_forward(self.h, _ptr(x), _ptr(t), _ptr(out), _stream_ptr(stream)), "forward")

    def load_sampler(self, solver: str, steps: int, betas: Optional[np.ndarray] = None, order: int = 2, eta: float = 0.0,
                     **options) -> SolverTable:
        """``build_table(solver, steps, betas, order, eta, **options)`` -> the engine (``options``: the keyword-only ``skip_type``,
        ``lower_order_final``, ``denoise_to_zero``, ``variant``, ``solver_type``, ``t_start``, ``t_end``, ``method``).  The loop runs
        ``table.steps`` evaluations (steps + 1 with ``denoise_to_zero``).  A stochastic table (``ddpm``, ``ddim`` with eta > 0) needs
        ``set_seeds`` before the loop begins."""
        table = build_table(solver, steps, betas, order, eta, **options)
        coef = np.ascontiguousarray(table.coef, dtype=np.float32)
        assert coef.shape == (table.steps, NCOEF)
        check(self.lib.ns2vc_sampler_load(self.h, table.steps, coef.ctypes.data_as(C.POINTER(C.c_float))), "sampler_load")
        self.table = table
        self.tables = None
        return table

    def load_samplers(self, specs, betas: Optional[np.ndarray] = None, discrete_betas: Optional[np.ndarray] = None, stream=None,
                      starts=None) -> ItemTables:
        """Per-item schedules: one dict per loop item (``schedule.schedule_key``: solver, steps, order, eta and the table options; the
        prepared B items, n under guidance -- set the guidance first) -> ``build_tables`` -> the engine (``ns2vc_sampler_load_items``).
        Every item walks its own table inside one captured loop of ``tables.steps`` = the longest table's evaluations, right-aligned
        (``starts`` overrides), and ends on what ``load_sampler`` with its schedule alone gives it, bit for bit.  Equal schedules still take
        this per-item form here (``Denoiser.sample`` routes them to ``load_sampler``).  ``sample(tail=, tail_steps=)`` works on engines
        that hold the same schedules.  Stochastic items need ``set_seeds``."""
        tabs = specs if isinstance(specs, ItemTables) else build_tables(specs, betas, discrete_betas, starts=starts)
        coef, rows = tabs.coef, np.ascontiguousarray(tabs.rows, dtype=np.int32)
        index, start = np.ascontiguousarray(tabs.index, dtype=np.int32), np.ascontiguousarray(tabs.start, dtype=np.int32)
        assert coef.shape == (int(rows.sum()), NCOEF)
        check(self.lib.ns2vc_sampler_load_items(self.h, int(rows.shape[0]), rows.ctypes.data, coef.ctypes.data_as(C.POINTER(C.c_float)),
                                                int(index.shape[0]), index.ctypes.data, start.ctypes.data, _stream_ptr(stream)), "sampler_load_items")
        self.tables = tabs
        self.table = None
        return tabs

    def _same_schedule(self, other: "Engine") -> bool:
        if (self.tables is None) != (other.tables is None):
            return False
        if self.tables is not None:
            a, b = self.tables, other.tables
            return np.array_equal(a.index, b.index) and np.array_equal(a.start, b.start) and np.array_equal(a.coef, b.coef)
        return self.table is not None and other.table is not None and other.table.steps == self.table.steps and \
            np.array_equal(np.asarray(self.table.coef, dtype=np.float32), np.asarray(other.table.coef, dtype=np.float32))

    @property
    def loop_steps(self) -> Optional[int]:
        """evaluations of the loaded loop: the table's rows, or the longest item's under per-item schedules"""
        return self.tables.steps if self.tables is not None else (None if self.table is None else self.table.steps)

    def sample(self, x_inout, use_graph: bool = True, stream=None, tail: Optional["Engine"] = None, tail_steps: int = 0) -> None:
        """x_inout (B,100,T): x_T in, sample out (in place).  NFE == steps of the loaded table.

        ``tail`` / ``tail_steps``: mixed precision -- this engine runs the first ``steps - tail_steps`` evaluations, then the
        solver state is handed to ``tail`` (normally an fp32 engine prepared for the same shape, condition and table),
        which runs the last ``tail_steps``.  The error of a sampled latent is dominated by the last evaluations
        (DPM-Solver++(2M)'s final second-order update extrapolates over a large log-SNR step, dpm_solver.py:796-831):
        two fp32 evaluations at the end take a 50-step fp16 loop from 1.7e-3 to ~2e-4 of the reference."""
        if tail is None or tail_steps <= 0:
            check(self.lib.ns2vc_sampler_run(self.h, _ptr(x_inout), int(use_graph), _stream_ptr(stream)), "sampler_run")
            return
        if not self._same_schedule(tail):
            raise Ns2vcError("mixed-precision sampling: both engines need the SAME solver table loaded (solver, steps, order, betas; "
                             "under per-item schedules the same schedules)")
        n, k = self.loop_steps, min(int(tail_steps), self.loop_steps)
        sp = _stream_ptr(stream)
        check(self.lib.ns2vc_sampler_begin(self.h, _ptr(x_inout), sp), "sampler_begin")
        check(self.lib.ns2vc_sampler_steps(self.h, n - k, int(use_graph), sp), "sampler_steps")
        check(self.lib.ns2vc_sampler_handoff(tail.h, self.h, sp), "sampler_handoff")
        tail.guidance = None if self.guidance is None else self.guidance.copy()      # (the hand-off carries the guidance over)
        tail.x0_correction = self.x0_correction                                        # (... and the x0 correction)
        tail.x0_corrections = self.x0_corrections                                      # (... in either form)
        check(self.lib.ns2vc_sampler_steps(tail.h, k, int(use_graph), sp), "sampler_steps(tail)")
        check(self.lib.ns2vc_sampler_end(tail.h, _ptr(x_inout), sp), "sampler_end")

    # the loop in parts (what ``sample(tail=...)`` is made of), for callers that look at the state in mid-loop
    def sample_begin(self, x_T, stream=None) -> None:
        check(self.lib.ns2vc_sampler_begin(self.h, _ptr(x_T), _stream_ptr(stream)), "sampler_begin")

    def sample_steps(self, n: int, use_graph: bool = True, stream=None) -> None:
        check(self.lib.ns2vc_sampler_steps(self.h, int(n), int(use_graph), _stream_ptr(stream)), "sampler_steps")

    def sample_peek(self, x_out, stream=None) -> None:
        """x_e of the loop in progress (the point the NEXT evaluation is taken at) -> x_out (B,100,T); the loop goes on"""
        check(self.lib.ns2vc_sampler_peek(self.h, _ptr(x_out), _stream_ptr(stream)), "sampler_peek")

    def sample_end(self, x_out, stream=None) -> None:
        check(self.lib.ns2vc_sampler_end(self.h, _ptr(x_out), _stream_ptr(stream)), "sampler_end")

    # -- slot loop: continuous batching (include/ns2vc_hip.h "Slot loop") ---------------------------------
    @staticmethod
    def _slot_list(slots) -> np.ndarray:
        a = np.ascontiguousarray(np.asarray(slots).reshape(-1), dtype=np.int32)
        if a.shape[0] == 0:
            raise ValueError("an empty slot list")
        return a

    def open_slots(self, history2: bool = False, noise: bool = False, stream=None, item_corrections: bool = False,
                   known_frames: bool = False) -> None:
        """Slot mode on the prepared shape: every loop item an idle slot on zero state and zero condition, the step counter running from 0.
        ``history2`` / ``noise``: order-3 / stochastic items may be admitted (fixed here: the captured step graph bakes them in, as it does
        the guidance and the x0 correction set at this moment).  ``item_corrections``: the per-item x0 correction table is on, every slot off
        until ``set_x0_correction_items`` gives it a record before its admission -- corrected and stochastic items may then share the loop;
        False switches a table left on off.  ``known_frames``: the per-slot known-frame form (``ns2vc_sampler_open_known``) -- every
        slot gets known rows and a frame mask, all clear, and the step the hold launch; ``set_known_items`` then gives idle slots their frames;
        not together with an x0 correction in either form.  Opening again starts afresh (refused while slots are busy)."""
        if known_frames and (item_corrections or self.x0_correction is not None):
            raise ValueError("known_frames and an x0 correction (set_x0_correction, item_corrections) exclude each other: it would rescale the held frames")
        if item_corrections:
            if self.x0_correction is not None:
                raise ValueError("item_corrections and the loop-wide x0 correction (set_x0_correction) exclude each other")
            items = self.shape[0] if self.guidance is None else self.guidance.shape[0]
            self.set_x0_correction_items([None] * items, stream=stream)
        elif self.x0_corrections is not None:
            self.set_x0_correction_items(None, stream=stream)
        if known_frames:
            check(self.lib.ns2vc_sampler_open_known(self.h, int(bool(history2)), int(bool(noise)), _stream_ptr(stream)), "sampler_open_known")
        else:
            check(self.lib.ns2vc_sampler_open(self.h, int(bool(history2)), int(bool(noise)), _stream_ptr(stream)), "sampler_open")
        self.table = self.tables = None

    def set_known_items(self, slots, known, mask, stream=None) -> None:
        """Known frames of the idle ``slots`` of a slot loop opened with ``known_frames=True``: ``known`` (n, latent, T) fp32 on the GPU, ``mask``
        (n, T) bool on the host (array / tensor); ``None, None`` clears the listed slots.  One launch, asynchronous on ``stream``, no recapture;
        the frames last for one request (``take`` clears them).  Call after ``set_lengths`` (a held frame lies inside its slot's length) and
        before ``admit``, whose x_T holds ``schedule.known_start`` on those frames."""
        s = self._slot_list(slots)
        if known is None and mask is None:
            check(self.lib.ns2vc_sampler_set_known_items(self.h, int(s.shape[0]), s.ctypes.data, None, None, _stream_ptr(stream)), "set_known_items")
            return
        if known is None or mask is None:
            raise ValueError("known and mask are given together (None, None clears the slots)")
        if hasattr(mask, "detach"):
            mask = mask.detach().cpu().numpy()
        m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        T = None if self.shape is None else self.shape[1]
        if m.shape != (s.shape[0], T):
            raise ValueError(f"mask must be ({s.shape[0]}, {T}) -- the listed slots and the prepared T --, got {m.shape}")
        if hasattr(known, "shape") and tuple(known.shape) != (s.shape[0], self.cfg.latent_channels, T):
            raise ValueError(f"known must be ({s.shape[0]}, {self.cfg.latent_channels}, {T}), got {tuple(known.shape)}")
        if hasattr(known, "dtype") and "float32" not in str(known.dtype):
            raise ValueError(f"known must be float32, got {known.dtype}")
        check(self.lib.ns2vc_sampler_set_known_items(self.h, int(s.shape[0]), s.ctypes.data, _ptr(known), m.ctypes.data, _stream_ptr(stream)),
              "set_known_items")

    def rebase_slots(self, stream=None) -> None:
        """the loop step of a drained slot loop (every slot idle) back to 0: the 32-bit counter does not bound a service's lifetime"""
        check(self.lib.ns2vc_sampler_rebase(self.h, _stream_ptr(stream)), "sampler_rebase")

    def write_sampler_rows(self, row0: int, coef, stream=None) -> None:
        """rows [row0, row0 + len(coef)) of the engine's 1024-row coefficient table (``schedule.TablePool`` decides where tables live)"""
        a = np.ascontiguousarray(coef, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] != NCOEF:
            raise ValueError(f"table rows must be (rows, {NCOEF}), got {a.shape}")
        check(self.lib.ns2vc_sampler_write_rows(self.h, int(row0), int(a.shape[0]), a.ctypes.data_as(C.POINTER(C.c_float)), _stream_ptr(stream)),
              "sampler_write_rows")

    def admit(self, slots, x_T, records, stream=None) -> None:
        """idle ``slots`` take ``x_T`` (n, C, T) on the GPU and ``records`` (n, 4) int32 {row0, steps, start, flags}; one launch"""
        s = self._slot_list(slots)
        r = np.ascontiguousarray(np.asarray(records), dtype=np.int32)
        if r.shape != (s.shape[0], 4):
            raise ValueError(f"records must be ({s.shape[0]}, 4) {{row0, steps, start, flags}}, got {r.shape}")
        check(self.lib.ns2vc_sampler_admit(self.h, int(s.shape[0]), s.ctypes.data, _ptr(x_T), r.ctypes.data, _stream_ptr(stream)), "sampler_admit")

    def take(self, slots, out, stream=None) -> None:
        """x_e of the finished ``slots`` -> ``out`` (n, C, T) on the GPU; the slots become idle; one launch"""
        s = self._slot_list(slots)
        check(self.lib.ns2vc_sampler_take(self.h, int(s.shape[0]), s.ctypes.data, _ptr(out), _stream_ptr(stream)), "sampler_take")

    def state_shape(self) -> Tuple[int, int, int]:
        """(planes, T, ld) of one slot's solver state in the open slot loop: xe, xbar, d1, mprev (+ mprev2 with history 2), fp32 rows"""
        p, t, ld = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.ns2vc_sampler_state_shape(self.h, C.byref(p), C.byref(t), C.byref(ld)), "sampler_state_shape")
        return int(p.value), int(t.value), int(ld.value)

    def suspend(self, slots, state, stream=None) -> List[int]:
        """the solver state of the running ``slots`` -> ``state`` (n, planes, T, ld) fp32 on the GPU, bit for bit; the slots become idle (in a
        loop with known frames their frames are cleared); returns each slot's ``done`` = rows of its table already run.  One launch, no
        recapture, no wait."""
        s = self._slot_list(slots)
        done = np.zeros((s.shape[0],), dtype=np.int32)
        check(self.lib.ns2vc_sampler_suspend(self.h, int(s.shape[0]), s.ctypes.data, _ptr(state), done.ctypes.data, _stream_ptr(stream)),
              "sampler_suspend")
        return [int(d) for d in done]

    def resume(self, slots, state, records, stream=None) -> None:
        """idle ``slots`` take ``state`` (n, planes, T, ld) fp32 on the GPU and ``records`` (n, 4) int32 {row0, steps, done, flags}: each
        continues at row ``done`` of its table with the next step.  Set the slots' lengths, condition, seed, scale, correction and known
        frames first, as for ``admit``.  One launch."""
        s = self._slot_list(slots)
        r = np.ascontiguousarray(np.asarray(records), dtype=np.int32)
        if r.shape != (s.shape[0], 4):
            raise ValueError(f"records must be ({s.shape[0]}, 4) {{row0, steps, done, flags}}, got {r.shape}")
        check(self.lib.ns2vc_sampler_resume(self.h, int(s.shape[0]), s.ctypes.data, _ptr(state), r.ctypes.data, _stream_ptr(stream)), "sampler_resume")

    def slot_step(self) -> int:
        """the loop step the next ``sample_steps`` of a slot loop starts at (-1: no slot loop)"""
        n = C.c_int()
        check(self.lib.ns2vc_sampler_slot_step(self.h, C.byref(n)), "sampler_slot_step")
        return int(n.value)

    def set_condition_items(self, slots, content, prompt, mask=None, stream=None) -> None:
        """content (n, 256, T), prompt (n, Lp, 256), mask (n, Lp) or None on the GPU -> the items ``slots`` of the prepared batch; the other
        items' hoisted tensors keep their bits.  Set the items' lengths / prompt lengths first."""
        s = self._slot_list(slots)
        check(self.lib.ns2vc_unet_set_condition_items(self.h, int(s.shape[0]), s.ctypes.data, _ptr(content), _ptr(prompt), _ptr(mask), _stream_ptr(stream)),
              "set_condition_items")

    def attn_fallbacks(self, reset: bool = True, stream=None) -> int:
        """attention workgroups whose optimistic pass (no per-tile maximum) had to be repeated by the exact pass since the last
        reset: each paid its kernel twice (scores rising > ~18 log2 units above their first 64 keys).  Waits for ``stream``."""
        n = C.c_ulonglong()
        check(self.lib.ns2vc_unet_attn_fallbacks(self.h, C.byref(n), int(reset), _stream_ptr(stream)), "attn_fallbacks")
        return int(n.value)

    def gn_coop_alone(self, reset: bool = True, stream=None) -> int:
        """workgroups of the cooperative GroupNorm prologue that waited in vain for a sibling and built every row themselves since
        the last reset (a performance counter: the values are the same either way).  Waits for ``stream``."""
        n = C.c_ulonglong()
        check(self.lib.ns2vc_unet_gn_coop_alone(self.h, C.byref(n), int(reset), _stream_ptr(stream)), "gn_coop_alone")
        return int(n.value)

    def graph_captures(self) -> int:
        """step graphs captured since the engine was created: a loop that replays a still-valid graph leaves the count alone"""
        n = C.c_ulonglong()
        check(self.lib.ns2vc_unet_graph_captures(self.h, C.byref(n)), "graph_captures")
        return int(n.value)

    # -- profiling --------------------------------------------------------------------
    def op_info(self, which: int = 0) -> List[Tuple[str, int, float, float]]:
        """[(name, kind, algorithmic flops, algorithmic bytes)] of the per-step (0) / condition (1) plan."""
        nf, nc = self.launches()
        out = []
        name = C.create_string_buffer(256)
        kind, fl, by = C.c_int(), C.c_double(), C.c_double()
        for i in range(nc if which else nf):
            check(self.lib.ns2vc_unet_op_info(self.h, which, i, name, 256, C.byref(kind), C.byref(fl), C.byref(by)), "op_info")
            out.append((name.value.decode(), int(kind.value), float(fl.value), float(by.value)))
        return out

    def temb_fork(self) -> Dict[str, int]:
        """Where the per-step plan's timestep-embedding branch sits (option fork_temb): its launches [begin, end), the launch a captured
        step joins it in front of, the first of the `readers` launches that read its scale / shift rows, and whether a captured step forks."""
        out = {}
        name = C.create_string_buffer(32)
        v, fl, by = C.c_int(), C.c_double(), C.c_double()
        for i in range(6):
            check(self.lib.ns2vc_unet_op_info(self.h, 2, i, name, 32, C.byref(v), C.byref(fl), C.byref(by)), "op_info(2)")
            out[name.value.decode()] = int(v.value)
        return out

    def profile_forward(self, reps: int = 5, stream=None) -> np.ndarray:
        """Per-launch HIP-event timing of the per-step plan (average ms per launch over `reps` back-to-back launches)."""
        nf, _ = self.launches()
        ms = (C.c_float * nf)()
        check(self.lib.ns2vc_unet_profile_forward(self.h, ms, nf, int(reps), _stream_ptr(stream)), "profile_forward")
        return np.array(list(ms), dtype=np.float64)

    # -- debug taps -----------------------------------------------------------------
    def taps(self) -> Dict[str, np.ndarray]:
        out: Dict[str, np.ndarray] = {}
        n = self.lib.ns2vc_unet_num_taps(self.h)
        name = C.create_string_buffer(256)
        rows, cols = C.c_int(), C.c_int()
        for i in range(n):
            check(self.lib.ns2vc_unet_tap_info(self.h, i, name, 256, C.byref(rows), C.byref(cols)), "tap_info")
            a = np.empty((rows.value, cols.value), dtype=np.float32)
            check(self.lib.ns2vc_unet_tap_read(self.h, i, a.ctypes.data), "tap_read")
            out[name.value.decode()] = a
        return out

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.ns2vc_unet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sync() -> None:
    check(_lib.load().ns2vc_dev_sync(), "dev_sync")
