"""Characterisation cases of the solver-update and quantile kernels (misc.hip): inputs from fixed numpy seeds, driven through the kernel hooks
ns2vc_k_solver_update, _guided, _corrected, _items, _items_corrected and ns2vc_k_abs_quantile of whichever library is handed in, every output array returned.
tools/record_solver_bits.py hashes the arrays a PARENT library gives into tests/golden/solver_bits_v2.json; tests/test_solver_bits_gpu.py compares
the built library against that record.  Nothing here depends on the code under test but the hooks' signatures.

CASES is the ordered list of case ids (no GPU needed to build it); run_case(lib, id) -> {array name: numpy array}."""
import ctypes as C
import zlib

import numpy as np

NCOEF = 12
PRECS = {"f32": 0, "bf16": 1, "f16": 2}
NI, T, LD, NC = 4, 7, 24, 22                 # the base shape: the last live quad of a row is partial (columns 20, 21 of 20 .. 23)
LENS = np.array([7, 3, 1, 0], np.int32)
SCALES = np.array([2.5, 1.0, 0.5, 0.0], np.float32)      # (1.0 selects the conditional half)
SEEDS = np.array([0x9E3779B97F4A7C15, 1, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF], np.uint64)
STATE = ("xe", "xe_op", "xbar", "d1", "mprev", "mprev2", "thr")


class _Dev:
    """device copies of host arrays through the library's own allocator (the recorder loads a library of another tree)"""

    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.lib.ns2vc_dev_malloc(C.byref(p), max(a.nbytes, 16)) == 0, self.lib.ns2vc_last_error()
        self.ptrs.append(p.value)
        assert self.lib.ns2vc_memcpy_h2d(p.value, a.ctypes.data, a.nbytes) == 0, self.lib.ns2vc_last_error()
        return p.value

    def get(self, ptr, like):
        out = np.empty(like.shape, like.dtype)
        assert self.lib.ns2vc_memcpy_d2h(out.ctypes.data, ptr, out.nbytes) == 0, self.lib.ns2vc_last_error()
        return out

    def free(self):
        for p in self.ptrs:
            self.lib.ns2vc_dev_free(p)
        self.ptrs = []


def _rng(case):
    return np.random.default_rng(zlib.crc32(case.encode()))


def _table(rng, rows, hist2=(), noise=()):
    """rows of plausible coefficients: alpha, sigma away from zero; columns 9 (noise) and 10, 11 (history 2) only on the rows named"""
    c = (0.5 * rng.standard_normal((rows, NCOEF))).astype(np.float32)
    c[:, 0] = np.linspace(900.0, 20.0, rows)
    c[:, 1] = rng.uniform(0.3, 1.0, rows)
    c[:, 2] = rng.uniform(0.1, 0.9, rows)
    c[:, 9:] = 0.0
    for r in hist2:
        c[r, 10:12] = rng.uniform(0.1, 0.6, 2) * (1, -1)
    for r in noise:
        c[r, 9] = rng.uniform(0.2, 0.7)
    return c


def _state(rng, n, guided):
    st = {k: rng.standard_normal(n).astype(np.float32) for k in ("xbar", "d1", "mprev", "mprev2")}
    st["x0"] = rng.standard_normal(2 * n if guided else n).astype(np.float32)
    xe = rng.standard_normal(n).astype(np.float32)
    st["xe"] = np.concatenate([xe, xe]) if guided else xe      # (a guided loop holds the same point in both halves)
    st["xe_op"] = np.full(4 * st["xe"].size, 0x5A, np.uint8)   # fp32 rows, or the 16-bit hi + lo pair: four bytes per element either way
    return st


def _run(lib, st, thr0, call):
    """upload st and thr0, run call(pointers), download every output array"""
    dev = _Dev(lib)
    try:
        host = dict(st, thr=np.asarray(thr0, np.float32))
        p = {k: dev.put(v) for k, v in host.items()}
        rc = call(dev, p)
        assert rc == 0, lib.ns2vc_last_error()
        assert lib.ns2vc_dev_sync() == 0, lib.ns2vc_last_error()
        return {k: dev.get(p[k], host[k]) for k in STATE}
    finally:
        dev.free()


# ---- shared table ------------------------------------------------------------------------------------------------------------------------
def _shared(lib, case, prec, h2, gd, mode, noisy=False, shape=(NI, T, LD), lens=LENS, step=1):
    rng = _rng(case)
    ni, t, ld = shape
    n = ni * t * ld
    coef = _table(rng, 3, hist2=(step,) if h2 else (), noise=(step,) if noisy else ())
    st = _state(rng, n, gd)
    scales = np.resize(SCALES, ni)

    def call(dev, p):
        cf, sp = dev.put(coef), dev.put(np.array([step, 0, 0, 0], np.int32))
        m2 = p["mprev2"] if h2 else None
        sc = dev.put(scales) if gd else None
        ln = dev.put(lens) if lens is not None else None
        if mode:
            return lib.ns2vc_k_solver_update_corrected(cf, sp, p["x0"], p["xe"], p["xe_op"], PRECS[prec], p["xbar"], p["d1"], p["mprev"], m2, n, ld, t, sc, ln, NC,
                                                       mode, 0.9, 0.5 if mode == 1 else 0.8, p["thr"], None)
        if gd:
            return lib.ns2vc_k_solver_update_guided(cf, sp, p["x0"], p["xe"], p["xe_op"], PRECS[prec], p["xbar"], p["d1"], p["mprev"], m2, n, ld, sc, t,
                                                    dev.put(SEEDS) if noisy else None, ln if noisy else None, NC, None)
        assert not noisy, "the hooks give the unguided update no seeds"
        return lib.ns2vc_k_solver_update(cf, sp, p["x0"], p["xe"], p["xe_op"], PRECS[prec], p["xbar"], p["d1"], p["mprev"], m2, n, ld, None)
    return _run(lib, st, np.full(ni, 0.25, np.float32), call)


# ---- per-item schedules ------------------------------------------------------------------------------------------------------------------
ITEM_STEP = 4
# rows 0 .. 5: no history 2; rows 6 .. 15: history 2 on every row; rows 16 .. 19: a noise column
# (row0, steps, start, flags) at loop step 4: active without history 2 (row 2; with mode 0 the noisy table, row 17); held, not yet started;
# held, finished; active with history 2 (row 10) -- and by LENS the first item is whole while the last active one has no elements
ITEMS = np.array([[0, 6, 2, 0], [0, 6, 5, 0], [6, 4, 0, 1], [6, 10, 0, 1]], np.int32)
ITEMS_NOISY = np.array([[16, 4, 3, 2], [0, 6, 5, 0], [6, 4, 0, 1], [6, 10, 0, 1]], np.int32)


def _items(lib, case, prec, gd, mode, shape=(NI, T, LD), lens=LENS, items=None, ratio=0.9):
    rng = _rng(case)
    ni, t, ld = shape
    n = ni * t * ld
    coef = _table(rng, 20, hist2=range(6, 16), noise=range(16, 20))
    st = _state(rng, n, gd)
    if items is None:
        items = ITEMS if mode else ITEMS_NOISY
    items = np.ascontiguousarray(items, np.int32)
    noisy = bool((items[:, 3] & 2).any())
    scales = np.resize(SCALES, ni)

    def call(dev, p):
        cf, sp = dev.put(coef), dev.put(np.array([ITEM_STEP, 0, 0, 0], np.int32))
        return lib.ns2vc_k_solver_update_items(cf, coef.shape[0], sp, items.ctypes.data, ni, p["x0"], p["xe"], p["xe_op"], PRECS[prec], p["xbar"], p["d1"],
                                               p["mprev"], p["mprev2"], n, ld, t, dev.put(scales) if gd else None, dev.put(np.resize(SEEDS, ni)) if noisy else None,
                                               dev.put(lens) if lens is not None else None, NC, mode, ratio, 0.5 if mode == 1 else 0.8, p["thr"], None)
    return _run(lib, st, np.full(ni, 0.25, np.float32), call)


# ---- per-item x0 correction --------------------------------------------------------------------------------------------------------------
# Per family member: the SolverItem records, the lengths, and per item (mode, ratio, max_val); loop step 4, the table of _items.  Across the three
# every (history 2, mode) form has an active item with live elements:
#   a: (H2 0, mode 1) | (H2 1, mode 2) | HELD in mode 1: thr keeps its 0.25 | (H2 1, mode 1) active with no elements: thr 0
#   b: (H2 0, mode 2) | (H2 1, mode 1) | stochastic (row 17) in mode 0 beside the corrected ones | (H2 1, mode 0)
#   c: (H2 0, mode 0) | (H2 1, mode 2) | (H2 0, mode 2) at row 0 | held, finished -- no record in mode 1: no quantile launch, thr untouched
ITEM_CORRECT = {
    "a": (np.array([[0, 6, 2, 0], [6, 10, 0, 1], [0, 6, 5, 0], [6, 10, 0, 1]], np.int32), LENS,
          ((1, 0.9, 0.5), (2, 0.37, 0.8), (1, 0.5, 0.3), (1, 0.995, 1.0))),
    "b": (np.array([[0, 6, 2, 0], [6, 10, 0, 1], [16, 4, 3, 2], [6, 10, 0, 1]], np.int32), np.array([7, 3, 2, 5], np.int32),
          ((2, 0.9, 0.5), (1, 0.37, 0.8), (0, 0.5, 0.3), (0, 0.995, 1.0))),
    "c": (np.array([[0, 6, 2, 0], [6, 10, 0, 1], [0, 6, 4, 0], [6, 4, 0, 1]], np.int32), LENS,
          ((0, 0.9, 0.5), (2, 0.37, 0.8), (2, 0.5, 0.3), (0, 0.995, 1.0))),
}


def _items_corrected(lib, case, prec, gd, which):
    rng = _rng(case)
    n = NI * T * LD
    coef = _table(rng, 20, hist2=range(6, 16), noise=range(16, 20))
    st = _state(rng, n, gd)
    items, lens, rec = ITEM_CORRECT[which]
    noisy = bool((items[:, 3] & 2).any())
    mode = np.array([r[0] for r in rec], np.int32)
    ratio = np.array([r[1] for r in rec], np.float32)
    max_val = np.array([r[2] for r in rec], np.float32)

    def call(dev, p):
        cf, sp = dev.put(coef), dev.put(np.array([ITEM_STEP, 0, 0, 0], np.int32))
        return lib.ns2vc_k_solver_update_items_corrected(cf, coef.shape[0], sp, items.ctypes.data, NI, p["x0"], p["xe"], p["xe_op"], PRECS[prec], p["xbar"],
                                                         p["d1"], p["mprev"], p["mprev2"], n, LD, T, dev.put(SCALES) if gd else None,
                                                         dev.put(SEEDS) if noisy else None, dev.put(lens), NC, mode.ctypes.data, ratio.ctypes.data,
                                                         max_val.ctypes.data, p["thr"], None)
    return _run(lib, st, np.full(NI, 0.25, np.float32), call)


# ---- quantile ----------------------------------------------------------------------------------------------------------------------------
def _quant_values(rng):
    """four items of T x LD whose live elements (NC columns) make each branch of the select decide: 0 random normals (neighbours in rank differ in
    a high digit: v_hi only by the extra sweep); 1 consecutive floats above 1.0 (v_hi in the last histogram); 2 three values many times
    (v_lo duplicated: v_hi == v_lo); 3 random, the padding columns holding large values that must not count"""
    v = rng.standard_normal((NI, T, LD)).astype(np.float32)
    k = rng.permutation(T * NC).astype(np.uint32)
    v[1, :, :NC] = (np.float32(1.0).view(np.uint32) + k).view(np.float32).reshape(T, NC) * rng.choice(np.float32([-1, 1]), (T, NC))
    v[2, :, :NC] = rng.choice(np.float32([0.5, -1.0, 1.5]), (T, NC))
    v[3, :, NC:] = 1e30
    return v


def _quantile(lib, case, p, lens=None, shape=(NI, T, LD), crafted=True):
    rng = _rng(case)
    ni, t, ld = shape
    v = _quant_values(rng) if crafted else rng.standard_normal(shape).astype(np.float32)
    dev = _Dev(lib)
    try:
        thr0 = np.full(ni, 0.25, np.float32)
        pv, pt = dev.put(v), dev.put(thr0)
        rc = lib.ns2vc_k_abs_quantile(pv, ni, t, ld, NC, dev.put(lens) if lens is not None else None, p, pt, None)
        assert rc == 0, lib.ns2vc_last_error()
        assert lib.ns2vc_dev_sync() == 0, lib.ns2vc_last_error()
        return {"thr": dev.get(pt, thr0)}
    finally:
        dev.free()


def _formed_state(rng, n_half, per, gd):
    """state for the quantile of a FORMED m (SRC 1 | 2): item 1 holds three x0 values against one x_e, so its m has duplicates"""
    st = _state(rng, n_half, gd)
    for h in range(2 if gd else 1):
        st["x0"][h * n_half + per: h * n_half + 2 * per] = rng.choice(np.float32([0.5, -1.0, 1.5]), per)
        st["xe"][h * n_half + per: h * n_half + 2 * per] = 0.3
    return st


T_LONG = 200                                  # 200 x 6 = 1200 quads: the 1024-thread sweep of an item strides
LENS_LONG = np.array([200, 200, 150], np.int32)


def _formed(lib, case, gd, items):
    """mode 1 at T = 200 through the corrected hook (abs_quantile_kernel<1 | 2>) or the items hook (abs_quantile_items_kernel<1 | 2>), p = 0.37"""
    rng = _rng(case)
    ni, t, ld = 3, T_LONG, LD
    n = ni * t * ld
    coef = _table(rng, 20, hist2=range(6, 16))
    st = _formed_state(rng, n, t * ld, gd)
    rec = np.array([[0, 6, 2, 0], [6, 10, 0, 1], [0, 6, 4, 0]], np.int32)      # all active: rows 2, 10, 0

    def call(dev, p):
        sp = dev.put(np.array([ITEM_STEP, 0, 0, 0], np.int32))
        sc, ln = dev.put(SCALES[:ni]) if gd else None, dev.put(LENS_LONG)
        if items:
            return lib.ns2vc_k_solver_update_items(dev.put(coef), coef.shape[0], sp, rec.ctypes.data, ni, p["x0"], p["xe"], p["xe_op"], 0, p["xbar"], p["d1"],
                                                   p["mprev"], p["mprev2"], n, ld, t, sc, None, ln, NC, 1, 0.37, 0.5, p["thr"], None)
        return lib.ns2vc_k_solver_update_corrected(dev.put(coef), sp, p["x0"], p["xe"], p["xe_op"], 0, p["xbar"], p["d1"], p["mprev"], None, n, ld, t, sc, ln, NC,
                                                   1, 0.37, 0.5, p["thr"], None)
    return _run(lib, st, np.full(ni, 0.25, np.float32), call)


# ---- grid stride: more than 2048 x 256 quads, so the update's loop takes a second trip ---------------------------------------------------
BIG = (36, 938, 64)
# per item, in turn: active without history 2, active with it, held before its start, held after its end
BIG_ITEMS = np.array([[[0, 6, 2, 0], [6, 10, 0, 1], [0, 6, 5, 0], [6, 4, 0, 1]][b % 4] for b in range(BIG[0])], np.int32)


def _build():
    cases = {}
    for prec in PRECS:
        for h2 in (0, 1):
            for gd in (0, 1):
                for mode in (0, 1, 2):
                    cases[f"shared-{prec}-h2{h2}-gd{gd}-th{mode}"] = lambda lib, c, a=(prec, h2, gd, mode): _shared(lib, c, *a)
        # the noisy form: the hooks hand seeds to the guided update only (ns2vc_k_solver_update takes none), so GD = 0 with noise is reached
        # through the items form below and not here
        cases[f"shared-{prec}-h20-gd1-th0-noisy"] = lambda lib, c, prec=prec: _shared(lib, c, prec, 0, 1, 0, noisy=True)
        for gd in (0, 1):
            for mode in (0, 1, 2):
                cases[f"items-{prec}-gd{gd}-th{mode}"] = lambda lib, c, a=(prec, gd, mode): _items(lib, c, *a)
    for name, p, lens in (("p0", 0.0, None), ("p1", 1.0, None), ("p037", 0.37, None), ("p05", 0.5, None), ("p0995-lens", 0.995, LENS)):
        cases[f"quantile-{name}"] = lambda lib, c, p=p, lens=lens: _quantile(lib, c, p, lens)
    cases["quantile-long"] = lambda lib, c: _quantile(lib, c, 0.37, LENS_LONG, (3, T_LONG, LD), crafted=False)
    for gd in (0, 1):
        cases[f"formed-shared-gd{gd}"] = lambda lib, c, gd=gd: _formed(lib, c, gd, False)
        cases[f"formed-items-gd{gd}"] = lambda lib, c, gd=gd: _formed(lib, c, gd, True)
    cases["stride-shared-f32"] = lambda lib, c: _shared(lib, c, "f32", 0, 0, 0, shape=BIG, lens=None)
    cases["stride-items-f32"] = lambda lib, c: _items(lib, c, "f32", 0, 0, shape=BIG, lens=None, items=BIG_ITEMS)
    for prec in PRECS:
        for gd in (0, 1):
            for which in ITEM_CORRECT:
                cases[f"itemcorr-{prec}-gd{gd}-{which}"] = lambda lib, c, a=(prec, gd, which): _items_corrected(lib, c, *a)
    return cases


_CASES = _build()
CASES = list(_CASES)


def run_case(lib, case):
    return _CASES[case](lib, case)


def digest(arrays):
    """what the fixture keeps of a case: per array its shape, dtype and the SHA-256 of its bytes"""
    import hashlib
    return {k: {"shape": list(a.shape), "dtype": str(a.dtype), "sha256": hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()} for k, a in arrays.items()}
