"""Item-end matrix of the length-masked row-chain, feed-forward and GEGLU kernels: the length vectors, their census and the one contract checker
(plain numpy, no GPU; a module like epilogue_ref.py: no fixtures).

The three kernels decide by hand, per lane, which item a token row belongs to (b = m / T), whether the row lies in front of the item's end
(t = m - b T < clamp(lens[b], 0, T)) and whether a whole block may return early.  What can go wrong there depends on WHERE in a block of W token rows
(W = 64: row chain, feed-forward; W = 128: row chain with two tokens per lane, GEGLU) an item starts and ends, so the vectors below are chosen by
census: `census(T, lens, W)` says which block positions and which kinds of block a vector produces, `REQUIRED` is what the vectors a kernel takes must
produce together, and tests/test_masked_matrix_cpu.py holds the shipped vectors to it.

Vectors (fixed lists, no RNG):
  V65     T = 65, B = 257, L_b = 65 - (7 b mod 33).  65 is odd, so item starts -- and the first dead rows of the items with L >= 33 -- fall on every
          position of a 64-row and of a 128-row block; M = 16705 = 261 * 64 + 1: the last block holds one row inside M.
  VDEAD   T = 257, lens = [1, 257, 129, 1]: seven full 64-row blocks and two full 128-row blocks wholly dead, a block whose only live row is its
          first, two blocks with a dead first row and live rows later.
  VSHORT  T = 19, B = 64, L_b = 1 + (7 b mod 19) (every value 1 .. 19): 4 - 5 items per 64-row block, 7 - 8 per 128-row block.  For the kernels that
          take T < 64 (plain row chain, GEGLU).
  VCLAMP  V65's first 16 items with item 5 -> T + 9, item 6 -> -7, item 11 -> 0: the headers' kernel-level contract clamp(lens[b], 0, T), which the
          engine never sends.  The count above T stands directly in front of the negative one: a kernel that forms an item's end as b T + lens[b]
          without the clamp lets it reach nine rows into an item that has none.
  VLONG   (this file's own, for W = 128) T = 66, B = 128, L_b = 64 for b < 64 and 65 after: 66 b mod 128 takes every even value, so the first dead
          rows of items with L >= W / 2 = 64 fall on all 128 positions of a 128-row block -- V65 has eight such items, VDEAD one.
  VLAST   (this file's own, for both widths) T = 255, lens = [128, 1, 255]: item 1 starts on the LAST row of a 64-row and of a 128-row block whose
          other rows are dead rows of item 0 -- the block kind "only live row is the last", which needs T >= W and which no other vector has --,
          item 0 ends on a block's last row, and the last item is full in front of a partial last block (a row at or past M whose clamped frame
          T - 1 is valid by the item's count).
(The issue asked for one vector of this file's own; the two properties pull T apart -- 128 long items want a small T, an only-live-last block
wants T >= 128 -- and one vector with both would have 16 512 rows or more, so they are two: 8448 and 765 rows.)"""
from __future__ import annotations

import numpy as np

from epilogue_ref import HALF_Q, SQ_SCALE, SUM_SCALE
from util import TOL_STATS

WIDTHS = (64, 128)


def _v65(B):
    return [65 - (7 * b) % 33 for b in range(B)]


def _vclamp():
    lens = _v65(16)
    lens[5], lens[6], lens[11] = 65 + 9, -7, 0
    return lens


VECTORS = {
    "V65": (65, _v65(257)),
    "VDEAD": (257, [1, 257, 129, 1]),
    "VSHORT": (19, [1 + (7 * b) % 19 for b in range(64)]),
    "VCLAMP": (65, _vclamp()),
    "VLONG": (66, [64] * 64 + [65] * 64),
    "VLAST": (255, [128, 1, 255]),
}
# what tests/test_masked_rows_gpu.py / test_masked_ffn_gpu.py and tests/test_masked_geglu_gpu.py run (restated: importing them needs the library)
TODAY_ROWS = {"T0_LENS0": (130, [130, 129, 65, 64, 63, 1])}
TODAY_GEGLU = {"A": (200, [200, 129, 33, 1, 72]), "B": (5, [5, 4, 3, 2, 1] * 12)}
# the vectors a kernel takes and the block widths it runs at
KERNEL_VECTORS = {
    "rowchain": (("V65", "VDEAD", "VSHORT", "VCLAMP", "VLONG", "VLAST"), (64, 128)),
    "ffn": (("V65", "VDEAD", "VCLAMP", "VLONG", "VLAST"), (64,)),                 # T >= 64 only: at most two items per block
    "geglu": (("V65", "VDEAD", "VSHORT", "VCLAMP", "VLONG", "VLAST"), (128,)),
}
# the GroupNorm-prologue row chain (T >= 64; one reference launch per item): a 24-item prefix of V65, VDEAD and -- the prologue forms no address from
# a count either (rowchain.hip: the count is clamped where it is read, the table index is clamped, the divisor is max(L, 1)) -- VCLAMP
GN_VECTORS = {"V65x24": (65, _v65(24)), "VDEAD": VECTORS["VDEAD"], "VCLAMP": VECTORS["VCLAMP"]}


def clamped(T, lens):
    return [min(max(int(L), 0), T) for L in lens]


def live_rows(T, lens):
    """bool (B * T,): row m = b T + t takes part iff t < clamp(lens[b], 0, T)"""
    lc = np.asarray(clamped(T, lens))
    return (np.arange(T)[None, :] < lc[:, None]).reshape(-1)


def census(T, lens, W):
    """what the vector produces in blocks of W rows, as data"""
    B, M, lc = len(lens), len(lens) * T, clamped(T, lens)
    live = live_rows(T, lens)
    item = np.arange(M) // T
    out = dict(starts=sorted({(b * T) % W for b in range(B)}),
               first_dead=sorted({(b * T + L) % W for b, L in enumerate(lc) if L < T}),
               first_dead_long=sorted({(b * T + L) % W for b, L in enumerate(lc) if W // 2 <= L < T}),
               dead_full_blocks=0, only_first_live=[], only_last_live=[], dead_first_live_later=[], three_items=[], last_partial=M % W != 0)
    for k in range((M + W - 1) // W):
        lv = live[k * W:(k + 1) * W]
        full = (k + 1) * W <= M
        if full and not lv.any():
            out["dead_full_blocks"] += 1
        if lv.sum() == 1 and lv[0]:
            out["only_first_live"].append(k)
        if full and lv.sum() == 1 and lv[-1]:
            out["only_last_live"].append(k)
        if not lv[0] and lv.any():
            out["dead_first_live_later"].append(k)
        if len(set(item[k * W:(k + 1) * W].tolist())) >= 3:
            out["three_items"].append(k)
    return out


REQUIRED = dict(starts="every position", first_dead="every position", first_dead_long="every position", dead_full_blocks=">= 1",
                only_first_live=">= 1", only_last_live=">= 1", dead_first_live_later=">= 1", three_items=">= 1 (not the feed-forward: T >= 64)",
                last_partial="once")


def missing(vectors, W, three_items=True):
    """what REQUIRED asks of `vectors` = {name: (T, lens)} at width W and they do not produce: a list of strings, empty = complete"""
    cs = [census(T, lens, W) for T, lens in vectors.values()]
    out = []
    for key in ("starts", "first_dead", "first_dead_long"):
        gone = sorted(set(range(W)) - set().union(*(c[key] for c in cs)))
        if gone:
            out.append(f"W={W} {key}: positions {gone} never occur")
    if not sum(c["dead_full_blocks"] for c in cs):
        out.append(f"W={W}: no full block is wholly dead")
    for key in ("only_first_live", "only_last_live", "dead_first_live_later") + (("three_items",) if three_items else ()):
        if not any(c[key] for c in cs):
            out.append(f"W={W}: no block of kind {key}")
    if not any(c["last_partial"] for c in cs):
        out.append(f"W={W}: no partial last block")
    return out


def seam_change(T, lens, W=64):
    """(b, L') for check 7: the first item with an ordinary count 2 <= L < T whose first dead row is a block's FIRST row (its last live row is the last
    row of the block in front) grows by one row, across the seam; a vector without one: the first item with 2 <= L < T loses its last row"""
    for b, L in enumerate(lens):
        if 2 <= L < T and (b * T + L) % W == 0:
            return b, L + 1
    for b, L in enumerate(lens):
        if 2 <= L < T:
            return b, L - 1
    raise ValueError("no item with an ordinary count")


def compact(a, T, lens):
    """the live rows of all items, concatenated: the rows of the dense twin"""
    return np.ascontiguousarray(a[live_rows(T, lens)])


def blocks_of_item(T, L, b, W=64):
    """number of W-row blocks that hold a live row of item b"""
    return 0 if L <= 0 else (b * T + L - 1) // W - (b * T) // W + 1


def _row_report(rec, tag, vec, what, b, L, m, T, W, count, extra=""):
    rec.append(dict(check=what[0], out=what[1], item=int(b), row=int(m), pos=int(m % W), count=int(count),
                    text=f"{tag} [{vec}] check {what[0]} {what[1]}: item {b} (count {L}) row {m} (frame {m - b * T}, position {m % W} of a {W}-row block): "
                         f"{count} word(s) {extra}"))


def check_launch(tag, vec, T, lens, masked, ref, *, out_fill, W=64, changed=None, stats_from=None, changed_item_rows=True):
    """The contract the three masked kernels share, held against one (kernel case, vector).

    masked   {fill: run}, fill in ("nan", "inf"): the launch under `lens` with that pattern in the dead rows of every input and around every tensor.
             run = dict(status, outs={name: storage words (M, n)}, viol=[guard violations], health=float or None, stats=int64 (B, nblk, 2) or None)
    ref      dict(outs={name: words (sum of clamped counts, n)}, health): the compacted dense twin -- one dense launch over the live rows of all
             items concatenated (or the per-item references concatenated in item order)
    out_fill {name: the storage word every element of that output held before the launch, or its (M, n) words where it held a tensor}
    changed  (b, L', run) or None: the launch with lens[b] -> L' and nothing else changed (check 7)
    stats_from  name of the fp32 output whose live rows `stats` sums (check 6)
    -> list of violation records dict(check, out, item, row, pos, count, text); empty = the launch keeps the contract.  Checks:
      1 status 0, no guard-band violation        2 live rows bit for bit the reference's        3 dead rows inside M all-zero words
      4 the two fills give identical words and statistics        5 ln_health == the reference's, exactly
      6 |stats - fp64 sums over the live rows of the launch's own fp32 result| <= TOL_STATS max|want| + n_b HALF_Q[k], n_b = 64-row blocks with a
        live row of item b (one commit per block and moment); an item clamped to 0 has all-zero statistics
      7 one count changed: every other item's words and statistics are identical -- and, a lane owning one token, the rows the changed item keeps;
        changed_item_rows=False where the item's rows depend on its count (the GroupNorm prologue divides by it)"""
    B, M, lc = len(lens), len(lens) * T, clamped(T, lens)
    off = np.concatenate([[0], np.cumsum(lc)])
    rec = []
    first = next(iter(masked))
    for fill, run in masked.items():
        if run["status"] != 0:
            rec.append(dict(check=1, out="status", item=-1, row=-1, pos=-1, count=0, text=f"{tag} [{vec}] fill={fill}: status {run['status']}"))
            continue
        for v in run["viol"]:
            rec.append(dict(check=1, out="guard", item=B - 1, row=M, pos=M % W, count=1, text=f"{tag} [{vec}] fill={fill}: guard band: {v}"))
        for name, words in run["outs"].items():
            assert words.shape[0] == M and ref["outs"][name].shape[0] == off[-1], (tag, vec, name, words.shape, ref["outs"][name].shape)
            for b, L in enumerate(lc):
                got, want = words[b * T:b * T + L], ref["outs"][name][off[b]:off[b + 1]]
                bad = np.flatnonzero((got != want).any(axis=1))
                if len(bad):
                    _row_report(rec, f"{tag} fill={fill}", vec, (2, name), b, lens[b], b * T + bad[0], T, W, (got != want).sum(),
                                f"differ from the reference in {len(bad)} live row(s)")
                dead = words[b * T + L:(b + 1) * T]
                bad = np.flatnonzero(dead.any(axis=1))
                if len(bad):
                    pre = out_fill[name][b * T + L:(b + 1) * T][bad] if np.ndim(out_fill[name]) == 2 else out_fill[name]
                    kept = int((dead[bad] == pre).all(axis=1).sum())
                    _row_report(rec, f"{tag} fill={fill}", vec, (3, name), b, lens[b], b * T + L + bad[0], T, W, (dead != 0).sum(),
                                f"non-zero in {len(bad)} dead row(s)" + (f", {kept} of them left unstored (the pre-launch fill survives)" if kept else ""))
        if ref.get("health") is not None and run["health"] != ref["health"]:
            rec.append(dict(check=5, out="ln_health", item=-1, row=-1, pos=-1, count=1,
                            text=f"{tag} [{vec}] fill={fill} check 5: ln_health {run['health']!r}, the reference's {ref['health']!r}"))
        if run.get("stats") is not None:
            rec += _check_stats(f"{tag} fill={fill}", vec, T, lens, run, stats_from, W)
    runs = list(masked.items())
    for fill, run in runs[1:]:
        if run["status"] != 0 or runs[0][1]["status"] != 0:
            continue
        for name, words in run["outs"].items():
            d = np.flatnonzero((words != runs[0][1]["outs"][name]).any(axis=1))
            if len(d):
                _row_report(rec, tag, vec, (4, name), d[0] // T, lens[d[0] // T], d[0], T, W, (words != runs[0][1]["outs"][name]).sum(),
                            f"differ between fill {first} and fill {fill} in {len(d)} row(s)")
        if run.get("stats") is not None:
            d = np.argwhere(run["stats"] != runs[0][1]["stats"])
            if len(d):
                b = int(d[0][0])
                rec.append(dict(check=4, out="stats", item=b, row=b * T + lc[b], pos=(b * T + lc[b]) % W, count=len(d),
                                text=f"{tag} [{vec}] check 4 stats: {len(d)} integer(s) differ between fill {first} and fill {fill}, first (item, block, "
                                     f"moment) {d[0].tolist()}; item {b} (count {lens[b]}) ends in front of row {b * T + lc[b]}, position {(b * T + lc[b]) % W}"))
    if changed is not None and masked[first]["status"] == 0:
        cb, cL, run2 = changed
        base = masked[first]
        if run2["status"] != 0:
            rec.append(dict(check=7, out="status", item=cb, row=-1, pos=-1, count=0, text=f"{tag} [{vec}] check 7: status {run2['status']} with lens[{cb}] -> {cL}"))
        else:
            keep = np.ones(M, dtype=bool)
            keep[cb * T + (min(lc[cb], min(max(cL, 0), T)) if changed_item_rows else 0):(cb + 1) * T] = False
            for name, words in run2["outs"].items():
                d = np.flatnonzero((words != base["outs"][name]).any(axis=1) & keep)
                if len(d):
                    _row_report(rec, tag, vec, (7, name), d[0] // T, lens[d[0] // T], d[0], T, W, (words != base["outs"][name])[keep].sum(),
                                f"changed in {len(d)} row(s) when lens[{cb}] went {lens[cb]} -> {cL}")
            if run2.get("stats") is not None:
                others = np.arange(B) != cb
                d = np.argwhere((run2["stats"] != base["stats"]) & others[:, None, None])
                if len(d):
                    b = int(d[0][0])
                    rec.append(dict(check=7, out="stats", item=b, row=b * T, pos=(b * T) % W, count=len(d),
                                    text=f"{tag} [{vec}] check 7 stats: {len(d)} integer(s) of other items changed when lens[{cb}] went {lens[cb]} -> {cL}, "
                                         f"first (item, block, moment) {d[0].tolist()}"))
    return rec


def _check_stats(tag, vec, T, lens, run, stats_from, W):
    B, lc = len(lens), clamped(T, lens)
    out = run["outs"][stats_from].view(np.float32).astype(np.float64)
    n = out.shape[1]
    got = np.stack([run["stats"][..., 0] / SUM_SCALE, run["stats"][..., 1] / SQ_SCALE], axis=-1)
    rec = []
    for b, L in enumerate(lc):
        rows = out[b * T:b * T + L].reshape(L, n // 16, 16)
        want = np.stack([rows.sum(axis=(0, 2)), (rows ** 2).sum(axis=(0, 2))], axis=-1)
        if L == 0 and run["stats"][b].any():
            rec.append(dict(check=6, out="stats", item=b, row=b * T, pos=(b * T) % W, count=int((run["stats"][b] != 0).sum()),
                            text=f"{tag} [{vec}] check 6: item {b} (count {lens[b]}, no live row; starts at row {b * T}, position {(b * T) % W}) has non-zero statistics"))
            continue
        nb = blocks_of_item(T, L, b, 64)
        for k in range(2):
            lim = TOL_STATS * np.abs(want[:, k]).max() + nb * HALF_Q[k]
            err = np.abs(got[b, :, k] - want[:, k])
            if not (err <= lim).all():
                j = int(err.argmax())
                rec.append(dict(check=6, out="stats", item=b, row=b * T + L, pos=(b * T + L) % W, count=int((err > lim).sum()),
                                text=f"{tag} [{vec}] check 6: item {b} (count {lens[b]}, rows {b * T} .. {b * T + L - 1}, first dead row at position "
                                     f"{(b * T + L) % W}) moment {k}: {int((err > lim).sum())} channel block(s) off, worst block {j}: {got[b, j, k]!r} vs "
                                     f"{want[j, k]!r} (off by {err[j]:.3e}, limit {lim:.3e} over {nb} block commits)"))
    return rec


def stats_figures(T, lens, run, stats_from):
    """the largest (error / limit) of check 6 per moment, for the diagnostics"""
    lc = clamped(T, lens)
    out = run["outs"][stats_from].view(np.float32).astype(np.float64)
    n = out.shape[1]
    got = np.stack([run["stats"][..., 0] / SUM_SCALE, run["stats"][..., 1] / SQ_SCALE], axis=-1)
    worst = [0.0, 0.0]
    for b, L in enumerate(lc):
        if L == 0:
            continue
        rows = out[b * T:b * T + L].reshape(L, n // 16, 16)
        want = np.stack([rows.sum(axis=(0, 2)), (rows ** 2).sum(axis=(0, 2))], axis=-1)
        for k in range(2):
            lim = TOL_STATS * np.abs(want[:, k]).max() + blocks_of_item(T, L, b, 64) * HALF_Q[k]
            worst[k] = max(worst[k], float((np.abs(got[b, :, k] - want[:, k]) / lim).max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# a numpy model of a masked launch, right or wrong in one of ten ways (tests/test_masked_matrix_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "a": "live iff t <= L",
    "b": "b taken from the block's first row for all its rows",
    "c": "block skipped (zeros stored) when its first row is dead",
    "d": "a wholly dead block is skipped without storing: the pre-launch fill survives",
    "e": "only the first two items of a block are considered",
    "f": "rows at or past M in the last block are live when the item's count says so",
    "g": "count not clamped: an item's end is b T + lens[b]",
    "h": "statistics include the first dead row of each item",
    "i": "statistics of a seam block's live rows all go to the block's first item",
    "j": "ln_health takes dead tokens",
}
MODEL_C = 16                 # channels of the model's tensors: one 16-channel statistics block
MODEL_FILL = np.float32(3.25)


def model_inputs(M):
    """finite input rows (M + a block of rows behind M that stand for the back guard, whose pattern the launch's fill decides)"""
    m = np.arange(M, dtype=np.uint32)[:, None] * np.uint32(MODEL_C) + np.arange(MODEL_C, dtype=np.uint32)[None, :]
    return ((m * np.uint32(2654435761) >> np.uint32(9)).astype(np.float32) / np.float32(2 ** 23) - np.float32(0.5))


def _row_function(x):
    """the "kernel": per row, an fp32 result, 16-bit words and a health value that depend on nothing but the row's input bits"""
    h = x.view(np.uint32).astype(np.uint64)
    h = (h * np.uint64(0x9E3779B1) + np.roll(h, 1, axis=1) * np.uint64(0x85EBCA77) + np.uint64(0x1234567)) & np.uint64(0xFFFFFFFF)
    f = ((h >> np.uint64(8)) & np.uint64(0xFFFF)).astype(np.float32) / np.float32(65536) - np.float32(0.5)
    w = ((h >> np.uint64(4)) & np.uint64(0xFFFF)).astype(np.uint16) | np.uint16(1)
    health = ((h[:, 0] >> np.uint64(3)) & np.uint64(0xFFFFF)).astype(np.float32) / np.float32(2 ** 20)
    health = np.where(np.isfinite(x).all(axis=1), health, np.float32(2))         # (a NaN / Inf row would raise the read-out above every real one)
    return f, w, health


def model_launch(T, lens, W, *, mutant=None, fill="nan", dense=False, x=None):
    """A masked launch over M = B T rows in blocks of W (dense: all M rows live, T = M).  Dead input rows and the rows behind M hold the fill.
    -> run as check_launch takes it: outs {out_f32: uint32 words, out_op: uint16 words}, stats int64 (B, 1, 2), health, viol"""
    B, M = len(lens), len(lens) * T
    bad = np.float32(np.nan) if fill == "nan" else np.float32(np.inf)
    nblk = (M + W - 1) // W
    xin = np.full((nblk * W, MODEL_C), bad, dtype=np.float32)
    src = model_inputs(M) if x is None else x
    lv_true = np.ones(M, dtype=bool) if dense else live_rows(T, lens)
    xin[:M][lv_true] = src[:M][lv_true]
    f, w, hv = _row_function(xin)
    of = np.full((nblk * W, MODEL_C), MODEL_FILL, dtype=np.float32)
    oo = np.full((nblk * W, MODEL_C), np.float32(MODEL_FILL).astype(np.float16).view(np.uint16), dtype=np.uint16)
    stats = np.zeros((B, 1, 2), dtype=np.int64)
    health = np.float32(0)
    lc = lens if mutant == "g" else clamped(T, lens)
    for k in range(nblk):
        m0 = k * W
        rows = np.arange(m0, m0 + W)
        inside = rows < M
        mc = np.minimum(rows, M - 1)
        b = np.minimum(mc // T, B - 1)
        if mutant == "b":
            b = np.full(W, min(m0 // T, B - 1))
        t = mc - b * T
        cnt = np.asarray(lc)[b]
        live = (t <= cnt) if mutant == "a" else (t < cnt)
        if mutant == "b":
            live &= t < T
        if mutant == "g":            # the previous item's unclamped end reaches into this one
            prev = np.maximum(b - 1, 0)
            live |= (b > 0) & (mc < prev * T + np.asarray(lc)[prev])
        if dense:
            live = np.ones(W, dtype=bool)
        if mutant == "e":
            first_two = np.unique(b)[:2]
            live &= np.isin(b, first_two)
        if mutant != "f":
            live &= inside
        if mutant == "c" and not live[0]:
            live[:] = False
        if mutant == "d" and not live.any():
            continue
        st = rows[inside | live]                     # a live row is stored wherever it lies; a dead one only inside M
        of[st] = np.where(live[:, None], f[rows], np.float32(0))[inside | live]
        oo[st] = np.where(live[:, None], w[rows], np.uint16(0))[inside | live]
        counted = live | (inside & (t == cnt) & (t < T)) if mutant == "h" else live
        sv = np.where(counted[:, None], f[rows], np.float32(0)).astype(np.float64)
        hl = inside if mutant == "j" else live
        if hl.any():
            health = max(health, hv[rows][hl].max())
        true_b = np.minimum(mc // T, B - 1)          # one commit per (block, item in it, moment)
        for bb in np.unique(true_b[inside]):
            if mutant == "i":
                if bb != true_b[0]:
                    continue
                s = sv
            else:
                s = sv[true_b == bb]
            stats[bb, 0, 0] += int(np.rint(np.float32(s.sum()).astype(np.float64) * SUM_SCALE))
            stats[bb, 0, 1] += int(np.rint(np.float32((s ** 2).sum()).astype(np.float64) * SQ_SCALE))
    viol = []
    for name, arr, fillw in (("out_f32", of, MODEL_FILL), ("out_op", oo, MODEL_FILL.astype(np.float16).view(np.uint16))):
        touched = np.flatnonzero((arr[M:] != fillw).any(axis=1))
        if len(touched):
            viol.append(f"{name}: back (row {M + int(touched[0])}, {len(touched)} row(s) behind the tensor written)")
    return dict(status=0, outs=dict(out_f32=np.ascontiguousarray(of[:M]).view(np.uint32), out_op=np.ascontiguousarray(oo[:M])), stats=stats,
                health=float(health), viol=viol)


MODEL_OUT_FILL = dict(out_f32=np.float32(MODEL_FILL).view(np.uint32), out_op=np.float32(MODEL_FILL).astype(np.float16).view(np.uint16))


def model_case(T, lens, W, mutant=None):
    """the whole of one (kernel case, vector) on the model: both fills, the compacted dense twin (always the right model), the seam change
    -> the arguments of check_launch"""
    M = len(lens) * T
    x = model_inputs(M)
    masked = {fill: model_launch(T, lens, W, mutant=mutant, fill=fill) for fill in ("nan", "inf")}
    xc = compact(x, T, lens)
    d = model_launch(len(xc), [len(xc)], W, dense=True, x=xc)
    ref = dict(outs=d["outs"], health=d["health"])
    cb, cL = seam_change(T, lens, W)
    lens2 = list(lens)
    lens2[cb] = cL
    changed = (cb, cL, model_launch(T, lens2, W, mutant=mutant, fill="nan"))
    return masked, ref, changed


def model_affected(T, lens, W, mutant):
    """(items, rows) that the mutant truly gets wrong on this vector: rows whose words differ from the right model's under either fill, items
    whose statistics differ, and -- for a write behind the tensor -- the last item and row M"""
    items, rows = set(), set()
    for fill in ("nan", "inf"):
        good, bad = model_launch(T, lens, W, fill=fill), model_launch(T, lens, W, mutant=mutant, fill=fill)
        for name in good["outs"]:
            r = np.flatnonzero((good["outs"][name] != bad["outs"][name]).any(axis=1))
            rows |= set(r.tolist())
            items |= set((r // T).tolist())
        items |= set(np.flatnonzero((good["stats"] != bad["stats"]).any(axis=(1, 2))).tolist())
        if bad["viol"]:
            items.add(len(lens) - 1)
            rows.add(len(lens) * T)
        if good["health"] != bad["health"]:
            items.add(-1)
    return items, rows
