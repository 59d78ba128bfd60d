"""Characterisation cases of the three host loops of ``ns2vc_amd/schedule.py`` -- ``run_table_numpy``, ``run_tables_numpy``, ``run_slots_numpy`` --
which the GPU tests trust as the statement of the sampler.  tools/record_host_loops.py writes what a PARENT checkout computes on them into
tests/golden/host_loops_v1.json; tests/test_host_loops_cpu.py holds the tree to that record.

CASES is the ordered list of case ids; run_case(id) -> one record:
    {"result": digest | [[digest per item] per slot], "trace": [digest], "x0_calls": [digest], "noise_calls": [digest]}      or      {"error": text}
``x0_calls`` holds one digest of the pair (x, t) per ``x0_fn`` call in call order, ``noise_calls`` one of the arguments per ``noise_fn`` call; a
digest is the first 16 hex digits of the SHA-256 of an array's dtype, shape and bytes.  A refusal (ValueError) is recorded by its text alone.

Nothing here may depend on the libm or the numpy version of the machine that replays the record: inputs, "normals" and the stand-in denoiser are
integer hashes and ``+ - * / abs`` in float32 (every one correctly rounded by IEEE 754), no tanh, cos or random generator.  The loops do not
care how their normals are distributed.  Shapes: B = 3, C = 5, T = 12 with lengths [12, 7, 1]; ddpm (1000 steps) B = 1, C = 2, T = 4."""
import functools
import hashlib

import numpy as np

from ns2vc_amd import schedule as S

f32 = np.float32
B, C, T = 3, 5, 12
LENGTHS = [12, 7, 1]
SHAPE = (B, C, T)
DDPM_SHAPE = (1, 2, 4)
BETAS64 = S.linear_betas(1000, np.float64)
DYN = dict(mode="dynamic_thresholding", ratio=0.9, max_val=0.5)
CLAMP = dict(mode="clamp", max_val=0.7)
SCALES = [2.5, 1.0, 3.0]
_M32 = np.uint64(0xFFFFFFFF)


def hash_array(seed, shape, scale=3.0):
    """float32 values in [-scale, scale) from a multiplicative integer hash of (seed, flat index): the top 24 bits of a 32-bit hash are exact in
    float32, and so are the division by 2^23 and the subtraction of 1; the product with ``scale`` is rounded once"""
    n = int(np.prod(shape, dtype=np.int64))
    h = (np.arange(n, dtype=np.uint64) + np.uint64(int(seed) * 7919 + 1)) & _M32
    for mul, sh in ((2654435761, 15), (2246822519, 13), (3266489917, 16)):
        h = (h * np.uint64(mul)) & _M32
        h = h ^ (h >> np.uint64(sh))
    v = (h >> np.uint64(8)).astype(f32)
    return ((v / f32(2 ** 23) - f32(1)) * f32(scale)).reshape(shape)


def stand_in(x, t, cond=None):
    """the stand-in denoiser: 0.9 xx / (1 + |xx|) + 0.05 t / (1 + t) in float32, xx = x (+ cond); items independent"""
    x = np.asarray(x, dtype=f32)
    tt = np.asarray(t, dtype=f32).reshape((-1,) + (1,) * (x.ndim - 1))
    xx = x if cond is None else x + cond
    return f32(0.9) * xx / (f32(1) + np.abs(xx)) + f32(0.05) * tt / (f32(1) + tt)


def digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()[:16]


class Recorder:
    """the ``x0_fn`` and ``noise_fn`` of one case: they note what they are called with.  ``guided``: a call on 2n items is cat([unconditional,
    conditional]) and each half has its own condition; ``noise_shape``: what one ``noise_fn`` call returns"""

    def __init__(self, noise_shape, guided=False):
        self.x0_calls, self.noise_calls, self.noise_shape, self.guided = [], [], tuple(noise_shape), guided

    def x0(self, x, t):
        self.x0_calls.append(hashlib.sha256((digest(x) + digest(t)).encode()).hexdigest()[:16])
        cond = None
        if self.guided:
            n = np.asarray(x).shape[0] // 2
            cond = np.concatenate([hash_array(31, (n,) + np.asarray(x).shape[1:], 0.5), hash_array(32, (n,) + np.asarray(x).shape[1:], 0.5)], axis=0)
        return stand_in(x, t, cond)

    def noise(self, *args):
        self.noise_calls.append(digest(np.array([int(a) for a in args], dtype=np.int64)))
        return hash_array(5000 + sum(int(a) * 1009 ** i for i, a in enumerate(args)), self.noise_shape)


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------
def x_T(seed=1, shape=SHAPE):
    return hash_array(seed, shape)


def hold_of(shape=SHAPE, seed=2):
    """(known, mask): frames inside every item's length ([12, 7, 1] at B = 3)"""
    mask = np.zeros((shape[0], shape[-1]), dtype=bool)
    mask[0, :3] = True
    if shape[0] > 1:
        mask[1, 5:7] = True
        mask[shape[0] - 1, 0] = True
    return hash_array(seed, shape, 1.5), mask


@functools.lru_cache(maxsize=None)
def tables():
    t = dict(unipc2=S.build_table("unipc", 6), unipc3_logsnr=S.build_table("unipc", 6, order=3, skip_type="logSNR"),
             dpmpp3=S.build_table("dpmsolver++", 6, order=3), unipc2_dtz=S.build_table("unipc", 5, denoise_to_zero=True),
             ddim_eta0=S.build_table("ddim", 5, BETAS64, eta=0.0), ddim_eta1=S.build_table("ddim", 5, BETAS64, eta=1.0),
             ddpm=S.build_table("ddpm", 1000, BETAS64))
    assert [S.has_history2(t[k]) for k in t] == [False, True, True, False, False, False, False]
    assert not (t["ddim_eta0"].coef[:, 9] != 0).any() and (t["ddim_eta1"].coef[:, 9] != 0).any() and (t["ddpm"].coef[:, 9] != 0).any()
    return t


DETERMINISTIC = ("unipc2", "unipc3_logsnr", "dpmpp3", "unipc2_dtz")
STOCHASTIC = ("ddim_eta0", "ddim_eta1", "ddpm")
MIXED = [dict(solver="unipc", steps=6), dict(solver="dpmsolver++", steps=5, order=3), dict(solver="ddim", steps=4, eta=1.0)]
DET3 = [dict(solver="unipc", steps=6), dict(solver="dpmsolver++", steps=5, order=3), dict(solver="unipc", steps=4, order=3, skip_type="logSNR")]
STARTS = [1, 0, 3]


def item_tables(specs=MIXED, starts=None):
    return S.build_tables(specs, discrete_betas=BETAS64, starts=starts)


@functools.lru_cache(maxsize=None)
def slot_tables():
    return dict(u2=S.build_table("unipc", 4), d3=S.build_table("dpmsolver++", 5, order=3), u3=S.build_table("unipc", 5, order=3),
                ddim=S.build_table("ddim", 4, BETAS64, eta=1.0))


KEEP = "keep"      # (an entry of ``timeline(hold=)``: leave that item's tuple as it is)


def timeline(kind="mixed", own=None, hold=None):
    """slot 0: two consecutive items with a gap (loop steps 0-3 and 6-10); slot 1: no item; slot 2: one item that starts late (3).  "mixed": the
    second item of slot 0 is order 3 and runs beside slot 2's ddim item; "det": no stochastic item.  ``own`` / ``hold``: per item, in the order
    (slot 0 item 0, slot 0 item 1, slot 2 item 0), a fourth / fifth tuple element"""
    t = slot_tables()
    items = [(t["u2"], 0, x_T(11, SHAPE[1:])), (t["d3"] if kind == "mixed" else t["u3"], 6, x_T(12, SHAPE[1:])),
             (t["ddim"] if kind == "mixed" else t["d3"], 3, x_T(13, SHAPE[1:]))]
    if own is not None:
        items = [it + (o,) for it, o in zip(items, own)]
    if hold is not None:
        items = [it if isinstance(h, str) and h == KEEP else it + (None,) * (4 - len(it)) + (h,) for it, h in zip(items, hold)]
    return [[items[0], items[1]], [], [items[2]]]


def slot_hold(seed=21, frames=slice(2, 6)):
    m = np.zeros((T,), dtype=bool)
    m[frames] = True
    return hash_array(seed, SHAPE[1:], 1.5), m


# ---- the cases: name -> fn(trace) -> (recorder, result) --------------------------------------------------------------------------------------
def _table_case(name, how="plain", noise=True, **kw):
    def run(trace):
        tab = tables()[name]
        shape = DDPM_SHAPE if name == "ddpm" else SHAPE
        rec = Recorder(shape)
        x, k = x_T(1, shape), dict(kw)
        if how == "dyn":
            k["correct_x0"] = dict(DYN, lengths=LENGTHS)
        elif how == "clamp":
            k["correct_x0"] = dict(CLAMP)
        elif how == "hold":
            k["hold"] = hold_of(shape)
            x = S.known_start(x, *k["hold"], tab.coef[0])
        return rec, S.run_table_numpy(tab, rec.x0, x, trace, rec.noise if noise else None, **k)
    return run


def _tables_case(specs=MIXED, starts=None, scales=None, hold=False, noise=True, **kw):
    def run(trace):
        tabs = item_tables(specs, starts)
        rec = Recorder(SHAPE[1:], guided=scales is not None)
        x, k = x_T(3), dict(kw)
        if scales is not None:
            k["guided_x0"] = np.asarray(scales, dtype=f32)
        if hold:
            k["hold"] = hold_of()
            x = S.known_start(x, *k["hold"], np.stack([tabs.table_of(b).coef[0] for b in range(len(specs))]))
        return rec, S.run_tables_numpy(tabs, rec.x0, x, trace, rec.noise if noise else None, **k)
    return run


def _slots_case(make_timeline, noise=True, shape=SHAPE, **kw):
    def run(trace):
        rec = Recorder(SHAPE[1:])
        return rec, S.run_slots_numpy(make_timeline(), rec.x0, shape, trace, rec.noise if noise else None, **kw)
    return run


def _cases():
    c = {}
    for name in DETERMINISTIC:
        for how in ("plain", "dyn", "clamp", "hold"):
            c[f"table/{name}/{how}"] = _table_case(name, how)
    for name in STOCHASTIC:
        for how in ("plain", "hold"):
            c[f"table/{name}/{how}"] = _table_case(name, how)
    c["tables/mixed/right_aligned"] = _tables_case()
    c["tables/mixed/starts"] = _tables_case(starts=STARTS)
    c["tables/mixed/guided"] = _tables_case(scales=SCALES)
    c["tables/mixed/guided_starts"] = _tables_case(starts=STARTS, scales=SCALES)
    c["tables/det/correct_dict_dyn"] = _tables_case(DET3, correct_x0=dict(DYN, lengths=LENGTHS))
    c["tables/det/correct_dict_clamp_no_lengths"] = _tables_case(DET3, correct_x0=dict(CLAMP))
    c["tables/det/correct_dict_mode_none"] = _tables_case(DET3, correct_x0=dict(mode=None))
    c["tables/mixed/correct_list"] = _tables_case(correct_x0=[dict(DYN, lengths=12), dict(CLAMP), None])
    c["tables/mixed/correct_list_starts_off_entry"] = _tables_case(starts=STARTS, correct_x0=[dict(mode=None), dict(DYN, lengths=[7]), None])
    c["tables/mixed/hold"] = _tables_case(hold=True)
    c["tables/mixed/hold_starts"] = _tables_case(starts=STARTS, hold=True)
    c["slots/mixed/len3"] = _slots_case(timeline)
    c["slots/det/len3"] = _slots_case(lambda: timeline("det"), noise=False)
    c["slots/det/correct_all_dyn"] = _slots_case(lambda: timeline("det"), correct_x0=dict(DYN, lengths=LENGTHS))
    c["slots/det/correct_all_clamp_no_lengths"] = _slots_case(lambda: timeline("det"), correct_x0=dict(CLAMP))
    c["slots/mixed/len4_own"] = _slots_case(lambda: timeline(own=[dict(DYN, lengths=7), dict(CLAMP), None]))
    c["slots/mixed/len4_own_off_entries"] = _slots_case(lambda: timeline(own=[None, dict(DYN, lengths=[12]), dict(mode=None)]))
    c["slots/mixed/len5_held_then_unheld"] = _slots_case(lambda: timeline(hold=[slot_hold(), None, KEEP]))      # (slot 2 stays a 3-tuple)
    c["slots/mixed/len5_all_held"] = _slots_case(lambda: timeline(hold=[slot_hold(21), slot_hold(22, slice(0, 3)), slot_hold(23, slice(9, 12))]))
    c["slots/mixed/len5_own_and_hold"] = _slots_case(lambda: timeline(own=[dict(CLAMP), None, None], hold=[None, slot_hold(), None]))
    c["slots/empty"] = _slots_case(lambda: [[], [], []])
    # ---- every ValueError of the three functions
    rt = _table_case
    known, mask = hold_of()
    c["refuse/table/hold_not_a_pair"] = rt("unipc2", hold=(known, None))
    c["refuse/table/hold_with_correction"] = rt("unipc2", hold=(known, mask), correct_x0=dict(CLAMP))
    c["refuse/table/hold_known_shape"] = rt("unipc2", hold=(known[:, :, :-1], mask))
    c["refuse/table/hold_mask_dtype"] = rt("unipc2", hold=(known, mask.astype(np.uint8)))
    c["refuse/table/hold_mask_shape"] = rt("unipc2", hold=(known, mask[:, :-1]))
    c["refuse/table/correction_mode"] = rt("unipc2", correct_x0=dict(mode="bogus"))
    c["refuse/table/correction_ratio"] = rt("unipc2", correct_x0=dict(DYN, ratio=1.5))
    c["refuse/table/correction_max_val"] = rt("unipc2", correct_x0=dict(CLAMP, max_val=0.0))
    c["refuse/table/correction_on_stochastic"] = rt("ddim_eta1", correct_x0=dict(CLAMP))
    c["refuse/table/no_noise_fn"] = rt("ddim_eta1", noise=False)
    c["refuse/tables/hold_with_correction"] = _tables_case(DET3, hold=True, correct_x0=dict(CLAMP))
    c["refuse/tables/hold_with_correction_list"] = _tables_case(hold=True, correct_x0=[None, None, None])
    c["refuse/tables/batch_size"] = _tables_case(MIXED[:2])
    c["refuse/tables/correction_mode"] = _tables_case(DET3, correct_x0=dict(mode="bogus"))
    c["refuse/tables/correct_dict_stochastic_item"] = _tables_case(correct_x0=dict(CLAMP))
    c["refuse/tables/correct_list_length"] = _tables_case(correct_x0=[None, None])
    c["refuse/tables/correct_list_not_a_dict"] = _tables_case(correct_x0=[None, "clamp", None])
    c["refuse/tables/correct_list_unknown_key"] = _tables_case(correct_x0=[dict(CLAMP, quantile=0.9), None, None])
    c["refuse/tables/correct_list_stochastic_item"] = _tables_case(correct_x0=[None, None, dict(CLAMP)])
    c["refuse/tables/correct_list_lengths"] = _tables_case(correct_x0=[dict(DYN, lengths=LENGTHS), None, None])
    c["refuse/tables/no_noise_fn"] = _tables_case(noise=False)
    c["refuse/tables/guided_scales_shape"] = _tables_case(scales=[2.5, 1.0])
    c["refuse/slots/timelines"] = _slots_case(lambda: timeline()[:2])
    c["refuse/slots/busy"] = _slots_case(lambda: [[(slot_tables()["u2"], 0, x_T(11, SHAPE[1:])), (slot_tables()["d3"], 3, x_T(12, SHAPE[1:]))], [], []])
    c["refuse/slots/own_on_stochastic"] = _slots_case(lambda: timeline(own=[None, None, dict(CLAMP)]))
    c["refuse/slots/own_not_a_dict"] = _slots_case(lambda: timeline(own=["clamp", None, None]))
    c["refuse/slots/own_and_correct_x0"] = _slots_case(lambda: timeline("det", own=[None, None, None]), correct_x0=dict(CLAMP))
    c["refuse/slots/correction_mode"] = _slots_case(lambda: timeline("det"), correct_x0=dict(mode="bogus"))
    c["refuse/slots/hold_with_own_correction"] = _slots_case(lambda: timeline(own=[dict(CLAMP), None, None], hold=[slot_hold(), None, None]))
    c["refuse/slots/hold_not_a_pair"] = _slots_case(lambda: timeline(hold=[(slot_hold()[0], None), None, None]))
    c["refuse/slots/hold_known_shape"] = _slots_case(lambda: timeline(hold=[(slot_hold()[0][:, :-1], slot_hold()[1]), None, None]))
    c["refuse/slots/hold_mask_dtype"] = _slots_case(lambda: timeline(hold=[(slot_hold()[0], slot_hold()[1].astype(np.int32)), None, None]))
    c["refuse/slots/no_noise_fn"] = _slots_case(timeline, noise=False)
    return c


_CASES = _cases()
CASES = list(_CASES)


def run_case(name):
    trace = []
    try:
        rec, y = _CASES[name](trace)
    except ValueError as e:
        return {"error": str(e)}
    result = [[digest(v) for v in slot] for slot in y] if isinstance(y, list) else digest(y)
    return {"result": result, "trace": [digest(v) for v in trace], "x0_calls": rec.x0_calls, "noise_calls": rec.noise_calls}
