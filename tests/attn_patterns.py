"""Attention inputs whose OUTPUT says which keys went into each row and with what weight (test-side code, pure numpy, no GPU).

A whole-tensor tolerance cannot see one key of n counted twice, dropped or taken from a neighbour: with unit-normal data one key carries about
1/n of a row, which is at or below every 16-bit bound of the suite.  The tensors built here turn such a defect into a decoded INTEGER.

COUNT   q = 0, so every valid key weighs exactly 1/n.  V[j, h*hd + d] = 1 iff j is the d-th seam position of head h.  Row (b, q, h) must give
        out[d] * n_b == 1 for a seam key that is valid for item b and exactly 0 for a seam position that is not (at or past k_lens[b], or masked
        by the bias).  A key counted twice reads 2n / (n + 1), a dropped one 0.
ROUTE   seam keys carry rows 1..15 of the 16 x 16 Hadamard matrix (times an amplitude a) in the first 16 dims of their head, every other valid
        key -a' times row 0, query i the code of ITS seam key plus a' times row 0.  In log2 units the scores are `gap` for the match, exactly 0 for
        the other seam keys (the rows stay orthogonal under any elementwise rounding of the two query values) and about -6 for the background.
        V[j] holds, as 0 / 1 values, the binary digits of j (10 dims), of h (3) and of b (2) and a presence one: thresholding a row at 0.5 gives
        (key, head, item).
DECOY   every row of K and V that item b must not read (past k_lens[b], or masked by a -10000 bias) is a key with twice the match score and an
        all-ones V code.  In dense launches there is no such row.

Every value that must survive rounding is 0, +-1 or one amplitude per tensor, so the fp8 V path sees exact values too.

Seam positions: the first key, n - 2, n - 1, every multiple of 32 (hence of 64 and 128) below n with +-1, and `edge - 1, edge, edge + 1` for the
key count (or bias prefix) of EVERY item of the launch.  Heads carry different subsets; together they cover all of them (asserted).

The seam list of (b, h) is stored rotated so that query i of head h of item b carries S[(i + h + b) mod |S|] and that key is C[i mod |S|] of a
canonical order C in which the slots 0 and 128 mod |S| (the only live row of a workgroup when q_lens is 1 or 129) and then every other slot hold
a key behind the first key tile: at least half of the rows (where the item has that many later seams) match in a later tile -- the rows whose
optimistic pass must be rejected at a high gap -- and the rest in the first."""
from __future__ import annotations

import numpy as np

from util import bf16_round, f16_round

LOG2E = 1.4426950408889634
BACKGROUND = 6.0                       # background keys sit this far (log2 units) below the other seam keys
JBITS, HBITS, BBITS = 10, 3, 2         # V code: digits of the key, the head and the item, then one presence dim
CODE = 16
NEG = -10000.0                         # the mask bias of the reference ((1 - m) * -10000)

HAD = np.array([[1.0]])
while HAD.shape[0] < CODE:
    HAD = np.block([[HAD, HAD], [HAD, -HAD]])

MUTANTS = ("tail_twice", "seam_drop", "pad_admit", "bias_shift", "row_rotate", "head_swap", "item_next")


def round_op(a, prec):
    a = np.asarray(a, dtype=np.float32)
    return (bf16_round(a) if prec == 1 else f16_round(a) if prec == 2 else a).astype(np.float64)


def e4m3_round(x):
    """round-to-nearest-even of non-negative values to OCP e4m3 (3 mantissa bits, subnormals of 2^-9, saturating at 448)"""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(x)
    q = np.exp2(np.maximum(e - 1, -6) - 3.0)
    return np.minimum(np.rint(x / q) * q, 448.0)


class Case:
    """one launch: B items of H heads, Lq query rows and Lk key rows each; q_lens / k_lens per item or None; plen = valid bias prefix per item or None"""

    def __init__(self, B, H, Lq, Lk, q_lens=None, k_lens=None, plen=None, tile=64):
        self.B, self.H, self.Lq, self.Lk, self.tile = B, H, Lq, Lk, tile
        self.q_lens = list(q_lens) if q_lens is not None else None
        self.k_lens = list(k_lens) if k_lens is not None else None
        self.plen = list(plen) if plen is not None else None
        assert not (k_lens is not None and plen is not None)

    def key(self):
        return (self.B, self.H, self.Lq, self.Lk, tuple(self.q_lens or ()), tuple(self.k_lens or ()), tuple(self.plen or ()), self.tile)

    def nq(self, b):
        return self.q_lens[b] if self.q_lens is not None else self.Lq

    def nk(self, b):
        """number of keys that take part for item b (always a prefix of its rows)"""
        return self.k_lens[b] if self.k_lens is not None else self.plen[b] if self.plen is not None else self.Lk

    def edges(self):
        return sorted(set(self.k_lens or self.plen or ()))

    def bias(self):
        if self.plen is None:
            return None
        return np.where(np.arange(self.Lk)[None, :] < np.array(self.plen)[:, None], 0.0, NEG).astype(np.float32)

    def live_workgroups(self):
        return self.H * sum((self.nq(b) + 127) // 128 for b in range(self.B))


def seam_positions(Lk, n, edges=()):
    s = {0, n - 2, n - 1}
    for m in range(32, n, 32):
        s |= {m - 1, m, m + 1}
    for e in edges:
        s |= {e - 1, e, e + 1}
    return sorted(x for x in s if 0 <= x < Lk)


def _spread(lst, h, H, c):
    """c distinct entries of lst for head h: its residue class first (so that H heads with c >= ceil(len / H) cover lst), then the next ones"""
    n = len(lst)
    out = []
    for j in list(range(h, n, H)) + [(h + 1 + j) % n for j in range(n)]:
        if lst[j] not in out and len(out) < c:
            out.append(lst[j])
    return out


def count_sets(case, hd):
    """[b][h] -> up to hd seam positions (valid and not); all heads of an item together cover every seam position"""
    sets = []
    for b in range(case.B):
        allp = seam_positions(case.Lk, case.nk(b), case.edges())
        assert len(allp) <= case.H * hd, (len(allp), case.H, hd)
        per = [_spread(allp, h, case.H, hd) for h in range(case.H)]
        assert set().union(*per) == set(allp)
        sets.append(per)
    return sets


def route_sets(case):
    """[b][h] -> the canonical order C (see the module docstring) of up to 15 VALID seam keys; all heads of an item together cover every valid seam"""
    sets = []
    cap = CODE - 1
    for b in range(case.B):
        n = case.nk(b)
        allp = [x for x in seam_positions(case.Lk, n, case.edges()) if x < n]
        F, L = [x for x in allp if x < case.tile], [x for x in allp if x >= case.tile]
        assert len(allp) <= case.H * cap and F and F[0] == 0
        per = []
        for h in range(case.H):
            pl = _spread(L, h, case.H, min(len(L), max(-(-len(L) // case.H), 8)))
            cf = min(len(F), cap - len(pl), max(-(-len(F) // case.H), min(7, len(pl)))) if pl else min(len(F), cap)
            assert cf >= 1                           # a seam key in the first tile: its maximum is then 0 (or the match), never the background
            pf = _spread(F, h, case.H, cf)
            m = len(pl) + len(pf)
            special = list(dict.fromkeys([0, 128 % m]))
            order = special + [t for t in range(0, m, 2) if t not in special] + [t for t in range(1, m, 2) if t not in special]
            slots = [None] * m
            for t, j in zip(order, pl + pf):         # the later-tile keys fill the special and the even slots first
                slots[t] = j
            assert None not in slots and len(set(slots)) == m
            per.append(slots)
        assert set().union(*(set(p) for p in per)) == set(allp), (b, sorted(set(allp) - set().union(*(set(p) for p in per))))
        sets.append(per)
    return sets


def amplitudes(gap, hd):
    s = LOG2E / np.sqrt(hd) * CODE
    return float(np.sqrt(gap / s)), float(np.sqrt(BACKGROUND / s))


def _codes(n, h, b):
    """(n, 16) V codes of keys 0..n-1 of head h of item b"""
    assert n <= 1 << JBITS and h < 1 << HBITS and b < 1 << BBITS
    c = np.ones((n, CODE))
    c[:, :JBITS] = (np.arange(n)[:, None] >> np.arange(JBITS)) & 1
    c[:, JBITS:JBITS + HBITS] = (h >> np.arange(HBITS)) & 1
    c[:, JBITS + HBITS:JBITS + HBITS + BBITS] = (b >> np.arange(BBITS)) & 1
    return c


def build_count(case, hd, vamp=1.0):
    """-> q, k, v (float32; q rows past q_lens NaN), sets.  K is +-1 (q = 0: it must not matter)."""
    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    D = H * hd
    sets = count_sets(case, hd)
    q = np.zeros((B, Lq, D), np.float32)
    jj, dd = np.meshgrid(np.arange(Lk), np.arange(D), indexing="ij")
    k = np.broadcast_to(np.where((jj * 7 + dd * 3 + (jj * dd) // 5) % 3 == 0, -1.0, 1.0), (B, Lk, D)).astype(np.float32).copy()
    v = np.zeros((B, Lk, D), np.float32)
    for b in range(B):
        for h in range(H):
            for d, j in enumerate(sets[b][h]):
                v[b, j, h * hd + d] = vamp
        v[b, case.nk(b):] = vamp                  # decoys: all ones
        k[b, case.nk(b):] *= 2.0
        q[b, case.nq(b):] = np.nan
    return q, k, v, sets


def check_count(out, case, hd, sets, vamp=1.0, tol=None):
    """out (B, Lq, D) float64 -> (worst |out * n / vamp - 1| over valid seam dims, number of excluded elements that are not exactly 0, first offenders,
    worst error / tol(n) over the items)"""
    worst, nonzero, bad, ratio = 0.0, 0, [], 0.0
    for b in range(case.B):
        n, nq = case.nk(b), case.nq(b)
        for h in range(case.H):
            S = sets[b][h]
            o = out[b, :nq, h * hd:(h + 1) * hd]
            want = np.zeros(hd)
            want[:len(S)] = [1.0 if j < n else 0.0 for j in S]
            on = want > 0
            if on.any():
                e = np.abs(o[:, on] * n / vamp - 1.0)
                e = np.where(np.isfinite(e), e, np.inf)
                if tol is not None:
                    ratio = max(ratio, float(e.max()) / tol(n))
                if e.max() > worst:
                    worst = float(e.max())
                    i, c = np.unravel_index(int(e.argmax()), e.shape)
                    bad.insert(0, ("weight", b, int(i), h, int(S[int(np.flatnonzero(on)[c])]), float(o[i, np.flatnonzero(on)[c]] * n / vamp)))
            z = o[:, ~on] != 0.0
            if z.any():
                nonzero += int(z.sum())
                i, c = np.argwhere(z)[0]
                dcol = int(np.flatnonzero(~on)[c])
                bad.append(("not zero", b, int(i), h, int(S[dcol]) if dcol < len(S) else None, float(o[i, dcol])))
    return worst, nonzero, bad[:6], ratio


def build_route(case, hd, gap, prec):
    """-> q, k, v (float32, values exact in the operand type of `prec` after its rounding), sets, want (B, Lq, H, 3) = (key, head, item) per row"""
    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    D = H * hd
    a, a1 = amplitudes(gap, hd)
    sets = route_sets(case)
    q = np.zeros((B, Lq, D), np.float32)
    k = np.zeros((B, Lk, D), np.float32)
    v = np.zeros((B, Lk, D), np.float32)
    want = np.full((B, Lq, H, 3), -1, dtype=np.int64)
    for b in range(B):
        n, nq = case.nk(b), case.nq(b)
        for h in range(H):
            C_ = sets[b][h]
            m = len(C_)
            c0 = h * hd
            k[b, :n, c0:c0 + CODE] = -a1 * HAD[0]
            v[b, :n, c0:c0 + CODE] = _codes(n, h, b)
            for t, j in enumerate(C_):
                k[b, j, c0:c0 + CODE] = a * HAD[1 + (t + h + b) % m]          # S[(t + h + b) mod m] = C[t] carries code 1 + its index in S
            k[b, n:, c0:c0 + CODE] = 2.0 * a * HAD[1 + np.arange(n, Lk) % m]  # decoys: twice the match score of one of the queries, all-ones code
            v[b, n:, c0:c0 + hd] = 1.0
            i = np.arange(nq)
            q[b, :nq, c0:c0 + CODE] = a * HAD[1 + (i + h + b) % m] + a1 * HAD[0]
            want[b, :nq, h, 0] = np.array(C_)[i % m]
            want[b, :nq, h, 1] = h
            want[b, :nq, h, 2] = b
        q[b, nq:] = np.nan
    return q, k, v, sets, want


def decode_route(out, case, hd):
    """out (B, Lq, D) -> (got (B, Lq, H, 3), dev (B, Lq, H) = largest distance of an element from its 0 / 1 code; rows past q_lens: -1 / 0)"""
    B, H, Lq = case.B, case.H, case.Lq
    o = out.reshape(B, Lq, H, hd)
    bits = o[..., :CODE] > 0.5
    dev = np.abs(o[..., :CODE] - bits).max(-1)
    if hd > CODE:
        dev = np.maximum(dev, np.abs(o[..., CODE:]).max(-1))
    w = bits.astype(np.int64)
    got = np.stack([(w[..., :JBITS] << np.arange(JBITS)).sum(-1), (w[..., JBITS:JBITS + HBITS] << np.arange(HBITS)).sum(-1),
                    (w[..., JBITS + HBITS:JBITS + HBITS + BBITS] << np.arange(BBITS)).sum(-1)], axis=-1)
    got = np.where(bits[..., CODE - 1:CODE], got, -2)          # no presence bit: nothing decodes
    for b in range(B):
        got[b, case.nq(b):] = -1
        dev[b, case.nq(b):] = 0.0
    return got, np.where(np.isfinite(dev), dev, np.inf)


def check_route(out, case, hd, want):
    """-> (number of rows (b, q, h) that decode wrongly, worst distance from the code, first offenders)"""
    got, dev = decode_route(out, case, hd)
    wrong = (got != want).any(-1)
    bad = [(int(b), int(i), int(h), got[b, i, h].tolist(), want[b, i, h].tolist()) for b, i, h in np.argwhere(wrong)[:6]]
    return int(wrong.sum()), float(dev.max()), bad


def realised_gaps(qr, kr, case, hd, sets):
    """from the ROUNDED operands, log2 units: (smallest, largest match score, largest other-seam score, largest background score), each relative to 0"""
    lo, hi, other, back = np.inf, -np.inf, -np.inf, -np.inf
    sc = LOG2E / np.sqrt(hd)
    for b in range(case.B):
        n, nq = case.nk(b), case.nq(b)
        for h in range(case.H):
            C_ = np.array(sets[b][h])
            s = np.einsum("id,jd->ij", qr[b, :nq, h * hd:(h + 1) * hd], kr[b, :n, h * hd:(h + 1) * hd]) * sc
            i = np.arange(nq)
            mt = s[i, C_[i % len(C_)]]
            lo, hi = min(lo, mt.min()), max(hi, mt.max())
            s2 = s.copy()
            s2[i, C_[i % len(C_)]] = -np.inf
            if len(C_) > 1:
                other = max(other, s2[:, C_].max())
            s2[:, C_] = -np.inf
            if n > len(C_):
                back = max(back, s2.max())
    return float(lo), float(hi), float(other), float(back)


def attend(q, k, v, case, hd, p_round=None, mutant=None):
    """fp64 softmax attention of a case's items over the keys that take part (log2 arithmetic, probabilities relative to the row maximum, optionally
    rounded by p_round), exact zeros past q_lens.  `mutant` applies one of MUTANTS to THIS reference: what a subtly wrong kernel would compute."""
    B, H, Lq, Lk = case.B, case.H, case.Lq, case.Lk
    q, k, v = (np.asarray(t, dtype=np.float64) for t in (q, k, v))
    out = np.zeros((B, Lq, H * hd))
    sc = LOG2E / np.sqrt(hd)
    for b in range(B):
        src = (b + 1) % B if mutant == "item_next" else b
        n, nq = case.nk(b), case.nq(b)
        keys = np.arange(n)
        if mutant == "tail_twice":
            keys = np.append(keys, n - 1)
        elif mutant == "seam_drop" and n >= case.tile:
            keys = keys[keys != case.tile - 1]
        elif mutant == "pad_admit" and n < Lk:
            keys = np.append(keys, n)
        elif mutant == "bias_shift" and case.plen is not None and n > 1:
            keys = keys[:-1]
        for h in range(H):
            sl = slice(h * hd, (h + 1) * hd)
            s = np.einsum("id,jd->ij", q[b, :nq, sl], k[src, keys, sl]) * sc          # (einsum: no BLAS thread pool for these small products)
            p = np.exp2(s - s.max(-1, keepdims=True))
            if p_round is not None:
                p = p_round(p)
            out[b, :nq, sl] = (p @ v[src, keys, sl]) / p.sum(-1, keepdims=True)
        if mutant == "row_rotate":
            for r0 in range(0, nq, 128):
                r1 = min(r0 + 128, nq)
                out[b, r0:r1] = np.roll(out[b, r0:r1], -1, axis=0)
    if mutant == "head_swap":
        out[:, :, :2 * hd] = np.concatenate([out[:, :, hd:2 * hd], out[:, :, :hd]], axis=-1)
    return out


def mutant_applies(case, mutant):
    """does the mutant change what some item reads at this shape?  (no padding key exists in a dense launch, no bias row without a bias, ...)"""
    if mutant == "tail_twice":                       # (the only key counted twice is still the only key)
        return any(case.nk(b) > 1 for b in range(case.B))
    if mutant == "seam_drop":
        return any(case.nk(b) >= case.tile for b in range(case.B))
    if mutant == "pad_admit":
        return any(case.nk(b) < case.Lk for b in range(case.B))
    if mutant == "bias_shift":
        return case.plen is not None and any(n > 1 for n in case.plen)
    if mutant == "row_rotate":
        return any(case.nq(b) > 1 and case.nk(b) > 1 for b in range(case.B))      # (over one key every row of an item is the same row)
    if mutant == "item_next":
        return case.B > 1
    return True


# ---- the attention table (csrc/attn.hip attn_rows), written the way the table writes itself: fp32 at four head widths on 64-key tiles, dense and
# masked; per 16-bit type the same plus 128-key tiles at hd 16 / 32 and the fp8 PV form (dense only) at every head width
def attn_table_rows():
    """[(prec, hd, keys, fp8, masked)]: one entry per row of the table"""
    rows = []

    def row2(prec, hd, keys):
        rows.extend([(prec, hd, keys, 0, 0), (prec, hd, keys, 0, 1)])

    for hd in (16, 32, 48, 64):
        row2(0, hd, 64)
    for prec in (1, 2):
        for hd in (16, 32, 48, 64):
            row2(prec, hd, 64)
            if hd <= 32:
                row2(prec, hd, 128)
            rows.append((prec, hd, 64, 1, 0))
    return rows


# ---- the shapes of tests/test_attn_positions_gpu.py (and of its CPU twin, which validates the patterns and the mutants at every one of them)
B_ATT, H_ATT, LQ_ATT = 3, 5, 200       # 30 workgroups: the XCD remap takes its remainder branch; two query blocks with a tail
Q_LENS = [200, 129, 1]
PLEN_CROSS = [469, 257, 193]           # bias prefixes of the Lk = 469 cross case: full, one past a 128-key edge, one past a 64-key edge
# k_lens {200, 129, 128, 127, 65, 64, 1}: seven values do not fit two launches of three items, so three; kR is the launch of the optimistic passes
# (every item keeps a seam key behind the first 128-key tile, so every live workgroup can be made to reject; the one-row item is the one with a
# single such key, so that half of the launch's rows can match behind the first tile under either tile width)
K_LENS = {"kA": [200, 129, 128], "kB": [127, 65, 64], "kC": [1, 200, 129], "kR": [200, 200, 129]}


def attn_cases(masked, tile):
    """{name: Case} of one table row kind (dense / masked instantiation) and key tile"""
    mk = dict(tile=tile, q_lens=Q_LENS) if masked else dict(tile=tile)
    c = {"Lk65": Case(B_ATT, H_ATT, LQ_ATT, 65, **mk), "Lk200": Case(B_ATT, H_ATT, LQ_ATT, 200, **mk),
         "cross469": Case(B_ATT, H_ATT, LQ_ATT, 469, plen=PLEN_CROSS, **mk)}
    if masked:
        for name, kl in K_LENS.items():
            c[name] = Case(B_ATT, H_ATT, LQ_ATT, 200, k_lens=kl, **mk)
    return c


REJECT_CASES = {0: ("Lk200", "cross469"), 1: ("cross469", "kR")}      # [masked] -> the cases of passes (b) and (c)

B_FFN, H_FFN, T_FFN = 2, 8, 70
LK_FFN = (1, 31, 32, 33, 69)
PLEN_FFN = {1: [1, 1], 31: [31, 17], 32: [32, 31], 33: [33, 32], 69: [69, 33]}


def ffn_cases():
    """{(Lk, masked): Case} of the in-kernel cross-attention of ffn_kernel (32-key tiles)"""
    return {(Lk, mk): Case(B_FFN, H_FFN, T_FFN, Lk, plen=PLEN_FFN[Lk] if mk else None, tile=32) for Lk in LK_FFN for mk in (0, 1)}


def later_tile_workgroups(case, sets):
    """workgroups (b, h, 128-query block) that hold a valid row whose ROUTE match lies behind the first key tile"""
    n = 0
    for b in range(case.B):
        for h in range(case.H):
            C_ = np.array(sets[b][h])
            for r0 in range(0, case.nq(b), 128):
                i = np.arange(r0, min(r0 + 128, case.nq(b)))
                n += bool((C_[i % len(C_)] >= case.tile).any())
    return n


def later_tile_fraction(case, sets):
    rows = later = 0
    for b in range(case.B):
        for h in range(case.H):
            C_ = np.array(sets[b][h])
            i = np.arange(case.nq(b))
            rows += len(i)
            later += int((C_[i % len(C_)] >= case.tile).sum())
    return later / rows
