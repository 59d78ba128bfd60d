"""A complete stand-in for ``ns2vc_amd.engine.Engine`` on the host: every method ``ns2vc_amd/pipeline.py`` and ``ns2vc_amd/slots.py`` call -- the
slot loop's known frames (``set_known_items``, ``open_slots(known_frames=)``) and its ``state_shape`` / ``suspend`` / ``resume`` included, so one
request can be held and suspended at once --, the attributes ``guidance``, ``x0_correction``, ``x0_corrections``, ``hold``, ``table`` and
``tables`` kept as ``Engine`` keeps them, and one shared list of what would have reached the device.  ``install(monkeypatch, rec)`` puts it in place of ``pipeline.Engine`` so that tests run the real ``Denoiser.__init__``:

    rec = Recording()
    install(monkeypatch, rec)
    d = Denoiser({}, precision="fp16")
    d.sample(...)
    rec.calls            # [(role, method, arguments)], role "head" | "tail" (the later instance, built with precision="fp32")

Streams are dropped from the arguments; a tensor or array becomes (dtype, shape, sha256 of its bytes)."""
import hashlib

import numpy as np
import torch

from ns2vc_amd import schedule as S


def digest(v):
    """an argument as plain data: tensors and arrays -> [dtype, shape, sha256], containers element-wise, numpy scalars -> Python's"""
    if isinstance(v, RecordingEngine):
        return v.role
    if isinstance(v, S.ItemTables):
        return ["ItemTables", [digest(k) for k in v.keys], digest(np.asarray(v.index)), digest(np.asarray(v.start)), digest(np.asarray(v.coef))]
    if torch.is_tensor(v):
        v = v.detach().cpu().contiguous().numpy()
    if isinstance(v, np.ndarray):
        a = np.ascontiguousarray(v)
        return [str(a.dtype), list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()]
    if isinstance(v, (list, tuple)):
        return [digest(e) for e in v]
    if isinstance(v, dict):
        return {str(k): digest(e) for k, e in sorted(v.items())}
    if isinstance(v, np.generic):
        return v.item()
    if callable(v):
        return "<callable>"
    return v


class Recording:
    """the shared call list of one ``Denoiser``'s engines, and what their read-outs answer"""

    def __init__(self):
        self.calls = []
        self.engines = []                 # in order of construction: the head, then the fp32 engine(s) of the tail / self-check
        self.ln_ratio = 1.0               # what ``ln_ratio`` answers (above ``Denoiser.ln_guard``: the guard's redo)
        self.ln_ratio_poll = 1.0          # what ``ln_ratio_poll`` answers (None: the read-out has not completed)
        self.attn_fallbacks = 0
        self.forward_error = 0.0          # relative error of a 16-bit engine's ``forward`` against the fp32 engine's (``_self_check``)

    def engine(self, cfg=None, precision="fp16"):
        e = RecordingEngine(self, cfg, precision, "head" if not self.engines else "tail")
        self.engines.append(e)
        return e

    def names(self, role=None):
        return [c[1] for c in self.calls if role is None or c[0] == role]

    def of(self, method, role=None):
        """the argument dicts of every recorded ``method`` call"""
        return [c[2] for c in self.calls if c[1] == method and (role is None or c[0] == role)]


def install(monkeypatch, rec, device_calls=True):
    """``rec.engine`` in place of ``pipeline.Engine``; the three torch.cuda calls of the host path answer without a device"""
    import ns2vc_amd.pipeline as P
    monkeypatch.setattr(P, "Engine", rec.engine)
    if device_calls:
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: None)
        monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    return rec


def denoiser(monkeypatch, precision="fp32", **kw):
    """The real ``Denoiser`` constructor on a fresh recording -> (denoiser, recording), the calls of the constructor dropped; ``denoiser.rec`` is
    the recording too.  The LayerNorm guard, the precision self-check and the attention read-out are off unless ``kw`` says otherwise."""
    from ns2vc_amd.pipeline import Denoiser
    rec = install(monkeypatch, Recording())
    d = Denoiser({}, precision=precision, **dict(dict(ln_guard=None, precision_check=None, attn_fallback_limit=None), **kw))
    rec.calls.clear()
    d.rec = rec
    return d, rec


class RecordingEngine:
    def __init__(self, rec, cfg, precision, role):
        from ns2vc_amd.spec import UNetConfig
        self.rec, self.cfg, self.precision, self.role = rec, cfg if cfg is not None else UNetConfig(), precision, role
        assert role == "head" or precision == "fp32"
        self.shape = self.lengths = self.prompt_lengths = self.guidance = None
        self.x0_correction = self.x0_corrections = self.hold = self.table = self.tables = None
        self.options = {}
        self._x = None                    # the state of a loop in parts
        self._slot_step = -1
        self._planes, self._starts = 4, {}      # of a slot loop: the planes of one item's solver state; slot -> the loop step of its request's row 0
        self._note("__init__", precision=precision)

    def _note(self, method, **args):
        args.pop("stream", None)
        self.rec.calls.append((self.role, method, {k: digest(v) for k, v in args.items()}))

    def _items(self):
        return None if self.shape is None else (self.shape[0] if self.guidance is None else self.guidance.shape[0])

    # -- weights, plan, read-outs ---------------------------------------------------------------------------------------
    def load_state_dict(self, state, strict=True):
        self._note("load_state_dict")
        self.shape = None

    def set_option(self, name, value):
        self._note("set_option", name=name, value=bool(value))
        self.options[name] = bool(value)
        self.shape = None

    def prepare(self, B, T, Lp):
        self._note("prepare", B=B, T=T, Lp=Lp)
        self.shape = (B, T, Lp)
        self.lengths = self.prompt_lengths = self.guidance = self.hold = None

    def ln_ratio(self, stream=None):
        self._note("ln_ratio")
        return float(self.rec.ln_ratio)

    def ln_ratio_post(self, stream=None):
        self._note("ln_ratio_post")

    def ln_ratio_poll(self):
        self._note("ln_ratio_poll")
        return self.rec.ln_ratio_poll

    def attn_fallbacks(self, reset=True, stream=None):
        self._note("attn_fallbacks", reset=reset)
        return int(self.rec.attn_fallbacks)

    def graph_captures(self):
        return 0

    # -- condition ------------------------------------------------------------------------------------------------------
    def set_condition(self, content, prompt, mask=None, stream=None):
        assert self.shape is not None and content.shape[0] == self.shape[0] and tuple(prompt.shape[:2]) == (self.shape[0], self.shape[2])
        self._note("set_condition", content=content, prompt=prompt, mask=mask)

    def set_condition_items(self, slots, content, prompt, mask=None, stream=None):
        self._note("set_condition_items", slots=list(slots), content=content, prompt=prompt, mask=mask)

    def _ints(self, v, what):
        if hasattr(v, "detach"):
            v = v.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(v).reshape(-1), dtype=np.int32)
        if self.shape is None or a.shape[0] != self.shape[0]:
            raise ValueError(f"{what} has {a.shape[0]} entries, the prepared batch {None if self.shape is None else self.shape[0]}")
        return a

    def set_lengths(self, lengths=None, stream=None):
        self.lengths = None if lengths is None else self._ints(lengths, "lengths")
        self._note("set_lengths", lengths=None if lengths is None else self.lengths.tolist())

    def set_prompt_lengths(self, prompt_lengths=None, stream=None):
        self.prompt_lengths = None if prompt_lengths is None else self._ints(prompt_lengths, "prompt_lengths")
        self._note("set_prompt_lengths", prompt_lengths=None if prompt_lengths is None else self.prompt_lengths.tolist())

    # -- sampler state ----------------------------------------------------------------------------------------------------
    def set_seeds(self, seeds, stream=None):
        if hasattr(seeds, "detach"):
            seeds = seeds.detach().cpu().numpy()
        a = np.asarray(seeds).reshape(-1).astype(np.uint64)
        if a.shape[0] != self._items():
            raise ValueError(f"seeds has {a.shape[0]} entries, the prepared batch {self._items()}")
        self._note("set_seeds", seeds=a.tolist())

    def set_guidance(self, scales=None, stream=None):
        if scales is None:
            self._note("set_guidance", scales=None)
            if self.guidance is not None:
                self.hold = None
            self.guidance = None
            return
        if hasattr(scales, "detach"):
            scales = scales.detach().cpu().numpy()
        a = np.ascontiguousarray(np.asarray(scales).reshape(-1), dtype=np.float32)
        if self.shape is None or 2 * a.shape[0] != self.shape[0]:
            raise ValueError(f"guidance for {a.shape[0]} items needs an engine prepared with B = {2 * a.shape[0]}, "
                             f"not {None if self.shape is None else self.shape[0]}")
        self._note("set_guidance", scales=a.tolist())
        if self.guidance is None:
            self.hold = None
        self.guidance = a.copy()

    def set_x0_correction(self, mode=None, ratio=0.995, max_val=1.0):
        m = S.check_x0_correction(mode, ratio, max_val)
        if m != 0 and self.hold is not None:      # (what ns2vc_sampler_set_x0_correction says while a hold is on)
            raise RuntimeError("known frames are held (ns2vc_sampler_set_known): they do not run with an x0 correction")
        if m != 0 and self.x0_corrections is not None:
            raise RuntimeError("the per-item x0 correction table is on: it excludes the loop-wide setting")
        self._note("set_x0_correction", mode=mode, ratio=float(ratio), max_val=float(max_val))
        self.x0_correction = None if m == 0 else (m, float(np.float32(ratio)), float(np.float32(max_val)))

    def set_x0_correction_items(self, modes=None, ratios=None, max_vals=None, stream=None):
        if modes is None:
            self._note("set_x0_correction_items", modes=None)
            self.x0_corrections = None
            return
        modes = list(modes)
        n = len(modes)
        ratios = [0.995] * n if ratios is None else list(ratios)
        max_vals = [1.0] * n if max_vals is None else list(max_vals)
        if len(ratios) != n or len(max_vals) != n:
            raise ValueError(f"{n} modes, {len(ratios)} ratios and {len(max_vals)} max_vals: one of each per loop item")
        m = np.asarray([S.check_x0_correction(modes[b], ratios[b], max_vals[b]) for b in range(n)], dtype=np.int32)
        if self.hold is not None:
            raise RuntimeError("known frames are held (ns2vc_sampler_set_known): they do not run with an x0 correction")
        if self.x0_correction is not None:
            raise RuntimeError("the loop-wide x0 correction is on: it excludes the per-item table")
        if self._slot_step < 0 and n != self._items():
            raise RuntimeError(f"{n} correction records for {self._items()} loop items")
        self._note("set_x0_correction_items", modes=modes, ratios=[float(v) for v in ratios], max_vals=[float(v) for v in max_vals])
        self.x0_corrections = (m, np.asarray(ratios, dtype=np.float32), np.asarray(max_vals, dtype=np.float32))

    def set_known(self, known=None, mask=None, stream=None):
        if known is None and mask is None:
            self._note("set_known", known=None, mask=None)
            self.hold = None
            return
        if known is None or mask is None:
            raise ValueError("known and mask are given together (None, None switches the hold off)")
        if hasattr(mask, "detach"):
            mask = mask.detach().cpu().numpy()
        m = np.ascontiguousarray(np.asarray(mask) != 0)
        if self.shape is None or m.shape != (self._items(), self.shape[1]):
            raise ValueError(f"mask must be ({self._items()}, {None if self.shape is None else self.shape[1]}), got {m.shape}")
        if tuple(known.shape) != (self._items(), self.cfg.latent_channels, self.shape[1]) or "float32" not in str(known.dtype):
            raise ValueError(f"known must be float32 ({self._items()}, {self.cfg.latent_channels}, {self.shape[1]}), got {known.dtype} {tuple(known.shape)}")
        if self.x0_correction is not None or self.x0_corrections is not None:
            raise RuntimeError("an x0 correction is on: known frames do not run with it")
        if self.lengths is not None:
            for b in range(m.shape[0]):
                assert not m[b, int(self.lengths[b]):].any(), "a held frame lies inside its item: set_lengths first"
        self._note("set_known", known=known, mask=m)
        self.hold = m.copy()

    def load_sampler(self, solver, steps, betas=None, order=2, eta=0.0, **options):
        table = S.build_table(solver, steps, betas, order, eta, **options)
        if self.x0_correction is not None and solver in S.DISCRETE_SOLVERS:
            raise RuntimeError(f"the x0 correction is on: not with a {solver} table")
        self._note("load_sampler", solver=solver, steps=steps, betas=betas, order=order, eta=float(eta), options=options)
        self.table, self.tables = table, None
        return table

    def load_samplers(self, specs, betas=None, discrete_betas=None, stream=None, starts=None):
        tabs = specs if isinstance(specs, S.ItemTables) else S.build_tables(specs, betas, discrete_betas, starts=starts)
        if len(tabs.index) != self._items():
            raise RuntimeError(f"{len(tabs.index)} item records for {self._items()} loop items (set the guidance first)")
        self._note("load_samplers", tables=tabs)
        self.tables, self.table = tabs, None
        return tabs

    @property
    def loop_steps(self):
        return self.tables.steps if self.tables is not None else (None if self.table is None else self.table.steps)

    # -- evaluations and loops: deterministic functions of their inputs -----------------------------------------------------------
    def forward(self, x, t, out, stream=None):
        self._note("forward", x=x, t=t)
        y = 0.5 * torch.tanh(x.float()) + 1e-4 * t.float().view(-1, 1, 1)
        if self.precision != "fp32":
            y = y * (1.0 + float(self.rec.forward_error))
        out.copy_(y)

    def sample(self, x_inout, use_graph=True, stream=None, tail=None, tail_steps=0):
        assert self.loop_steps is not None and x_inout.shape[0] == self._items()
        self._note("sample", x=x_inout, use_graph=bool(use_graph), tail=tail, tail_steps=int(tail_steps))
        if tail is not None and tail_steps > 0:
            assert tail.loop_steps == self.loop_steps and tail.shape == self.shape
            assert (tail.hold is None) == (self.hold is None) and (tail.lengths is None) == (self.lengths is None)
            tail.guidance = None if self.guidance is None else self.guidance.copy()      # (the hand-off carries these over)
            tail.x0_correction, tail.x0_corrections = self.x0_correction, self.x0_corrections
        x_inout.mul_(0.5)

    def sample_begin(self, x_T, stream=None):
        self._note("sample_begin", x=x_T)
        self._x = x_T.clone()

    def sample_steps(self, n, use_graph=True, stream=None):
        self._note("sample_steps", n=int(n), use_graph=bool(use_graph))
        if self._slot_step >= 0:
            self._slot_step += int(n)
        elif self._x is not None:
            self._x.mul_(1.0 - 0.01 * int(n))

    def sample_peek(self, x_out, stream=None):
        self._note("sample_peek")
        x_out.copy_(self._x)

    def sample_end(self, x_out, stream=None):
        self._note("sample_end")
        if self._x is not None and tuple(self._x.shape) == tuple(x_out.shape):
            x_out.copy_(self._x)
        self._x, self._slot_step = None, -1

    # -- slot loop --------------------------------------------------------------------------------------------------------
    def open_slots(self, history2=False, noise=False, stream=None, item_corrections=False, **kw):
        assert set(kw) <= {"known_frames"}
        if self.hold is not None:      # (what ns2vc_sampler_open says while a hold is on)
            raise RuntimeError("known frames are held (ns2vc_sampler_set_known): a slot loop does not run with them")
        if item_corrections and self.x0_correction is not None:
            raise ValueError("item_corrections and the loop-wide x0 correction (set_x0_correction) exclude each other")
        if kw.get("known_frames") and (item_corrections or self.x0_correction is not None):
            raise ValueError("known_frames and an x0 correction exclude each other")
        self._note("open_slots", history2=bool(history2), noise=bool(noise), item_corrections=bool(item_corrections), **kw)      # (the keyword only when passed)
        self._planes, self._starts = 5 if history2 else 4, {}
        n = self._items()
        self.x0_corrections = (np.zeros(n, np.int32), np.full(n, 0.995, np.float32), np.ones(n, np.float32)) if item_corrections else None
        self.table = self.tables = None
        self._slot_step = 0

    def rebase_slots(self, stream=None):
        self._note("rebase_slots")
        self._slot_step = 0

    def write_sampler_rows(self, row0, coef, stream=None):
        self._note("write_sampler_rows", row0=int(row0), coef=np.asarray(coef, dtype=np.float32))

    def admit(self, slots, x_T, records, stream=None):
        self._note("admit", slots=list(slots), x=x_T, records=np.asarray(records, dtype=np.int32))
        for b, r in zip(slots, np.asarray(records)):
            self._starts[b] = int(r[2])

    def set_known_items(self, slots, known, mask, stream=None):
        self._note("set_known_items", slots=list(slots), known=known, mask=mask)

    def state_shape(self):
        return (self._planes, self.shape[1], 128)

    def suspend(self, slots, state, stream=None):
        self._note("suspend", slots=list(slots), state_shape=list(state.shape))
        state.fill_(1.5)
        return [self._slot_step - self._starts[b] for b in slots]

    def resume(self, slots, state, records, stream=None):
        self._note("resume", slots=list(slots), state=state, records=np.asarray(records, dtype=np.int32))
        for b, r in zip(slots, np.asarray(records)):
            self._starts[b] = self._slot_step - int(r[2])

    def take(self, slots, out, stream=None):
        self._note("take", slots=list(slots))
        out.zero_()

    def slot_step(self):
        return self._slot_step

    def close(self):
        pass


def check_masked_option(monkeypatch, name):
    """What ``Denoiser`` does with one of ``pipeline.MASKED_OPTIONS``: the constructor passes it to the head and to the tail engine once that
    exists, ``Denoiser.set_option`` (and ``GroupedConverter`` through it) reaches both and makes the tail prepare and load its table again, and
    the default reaches neither engine."""
    from ns2vc_amd.pipeline import MASKED_OPTIONS, Denoiser
    from ns2vc_amd.service import GroupedConverter
    assert name in MASKED_OPTIONS
    g = torch.Generator().manual_seed(0)
    c, p, n = torch.randn((2, 256, 16), generator=g), torch.randn((2, 8, 256), generator=g), torch.randn((2, 100, 16), generator=g)
    with_tail = dict(solver="dpmsolver++", steps=6)
    rec = install(monkeypatch, Recording())
    d = Denoiser({}, precision="fp16", precision_check=None, **{name: True})
    assert rec.of("set_option") == [dict(name=name, value=True)] and getattr(d, name) is True and len(rec.engines) == 1
    d.sample(c, p, None, n, **with_tail)
    assert rec.of("set_option", "tail") == [dict(name=name, value=True)] and len(rec.of("set_option", "head")) == 1
    assert rec.names("tail").index("set_option") < rec.names("tail").index("prepare")
    k = len(rec.calls)
    d.set_option(name, False)
    assert [(r, m, a) for r, m, a in rec.calls[k:]] == [(r, "set_option", dict(name=name, value=False)) for r in ("head", "tail")]
    assert getattr(d, name) is False
    k = len(rec.calls)
    d.sample(c, p, None, n, **with_tail)
    for role in ("head", "tail"):      # the plan and the table of both engines are built again
        names = [m for r, m, _ in rec.calls[k:] if r == role]
        assert names[0] == "prepare" and "load_sampler" in names, (role, names)
    k = len(rec.calls)
    GroupedConverter(None, d, **{name: False})
    GroupedConverter(None, d)
    assert rec.calls[k:] == []                                   # (the denoiser's setting already; None leaves it alone)
    GroupedConverter(None, d, **{name: True})
    assert [(r, a) for r, _, a in rec.calls[k:]] == [(r, dict(name=name, value=True)) for r in ("head", "tail")] and getattr(d, name) is True
    rec = install(monkeypatch, Recording())
    d = Denoiser({}, precision="fp16", precision_check=None)
    d.sample(c, p, None, n, **with_tail)
    assert len(rec.engines) == 2 and rec.of("set_option") == [] and getattr(d, name) is False
