"""Guarded tensors for the kernel bounds tests (test-side code, not product; a plain module like util.py: no fixtures).

A `Guarded` tensor is ONE block

    [ front guard | rows at pitch ld, the logical tensor `col0` columns into each row | back guard ]

whose whole byte image is built on the host with numpy and uploaded raw, so the bit pattern of every element a kernel could
reach by overshooting is the test's choice.  `violations()` compares the BYTES of everything that is not the logical tensor
(both guards and the gap columns of every row) with what was uploaded.  The block lives on the device (ns2vc_dev_malloc /
ns2vc_memcpy_h2d / _d2h) or, for the self-test of this module, in a host array that numpy "kernels" index like device memory.

Guard size.  A kernel that overshoots does so by at most one row tile plus the halo of a k = 3 convolution:
  128 rows = the largest row tile of any kernel (gemm.hip gemm4_kernel BM = 128 and the `(128, 128, 13 | 23)` tiles; convts.hip
             TS_BM = 128, of which TS_BMO = 126 are stored; attn.hip 128-key tiles; geglu.hip / rowchain.hip 128-token workgroups),
    2 rows = convts.hip "reads two rows past the panel" (one halo row either side for the other kernels).
So each guard holds at least (128 + 2) * ld elements, rounded up to 4 KB: every such access lands in memory the test owns.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from util import bf16_round

TILE_ROWS, HALO_ROWS = 128, 2          # see the module docstring
GUARD_ROUND = 4096                     # bytes
ALIGN = 16                             # bytes: pointers and row pitches the header asks for
LINE = 128                             # bytes: what gnp_sync asks of a0

FILLS = ("nan", "inf", "zero")
# kind -> (storage dtype, {fill: bit pattern}); 16-bit and fp32: the quiet NaN / +Inf of the type; 32-bit integers get the fp32 patterns
# (they sit next to fp32 tensors in the arena); 64-bit statistics neighbours: two NaN / Inf floats side by side
KINDS = {
    "f32": (np.uint32, {"nan": 0x7FC00000, "inf": 0x7F800000, "zero": 0}),
    "bf16": (np.uint16, {"nan": 0x7FC0, "inf": 0x7F80, "zero": 0}),
    "f16": (np.uint16, {"nan": 0x7E00, "inf": 0x7C00, "zero": 0}),
    "i32": (np.uint32, {"nan": 0x7FC00000, "inf": 0x7F800000, "zero": 0}),
    "u32": (np.uint32, {"nan": 0x7FC00000, "inf": 0x7F800000, "zero": 0}),
    "i64": (np.uint64, {"nan": 0x7FF800007FF80000, "inf": 0x7F8000007F800000, "zero": 0}),
    "u64": (np.uint64, {"nan": 0x7FF800007FF80000, "inf": 0x7F8000007F800000, "zero": 0}),
}
OP_KIND = {0: "f32", 1: "bf16", 2: "f16"}      # NS2VC_PREC_* -> kind of an operand-typed tensor


def encode(a, kind: str) -> np.ndarray:
    """values -> the storage words of `kind` (fp16 through np.float16, bf16 = the upper 16 bits after round-to-nearest-even)"""
    if kind == "f32":
        return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    if kind == "bf16":
        return (bf16_round(np.asarray(a, dtype=np.float32)).view(np.uint32) >> 16).astype(np.uint16)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(np.asarray(a, dtype=np.float32).astype(np.float16)).view(np.uint16)
    sdt = KINDS[kind][0]
    return np.ascontiguousarray(a).astype({"i32": np.int32, "u32": np.uint32, "i64": np.int64, "u64": np.uint64}[kind]).view(sdt)


def decode(w: np.ndarray, kind: str) -> np.ndarray:
    if kind == "f32":
        return w.view(np.float32)
    if kind == "bf16":
        return (w.astype(np.uint32) << 16).view(np.float32)
    if kind == "f16":
        return w.view(np.float16).astype(np.float32)
    return w.view({"i32": np.int32, "u32": np.uint32, "i64": np.int64, "u64": np.uint64}[kind])


class HostBackend:
    """the "device" is a host byte array; numpy kernels address it through Guarded.mem / .base"""

    def malloc(self, nbytes):
        raw = np.zeros(nbytes + LINE, dtype=np.uint8)
        off = -raw.ctypes.data % LINE                  # (a view that starts on a 128-byte line, as the device allocator's blocks do)
        return raw[off:off + nbytes]

    def upload(self, handle, image_u8):
        handle[:] = image_u8

    def download(self, handle, nbytes):
        return handle[:nbytes].copy()

    def address(self, handle):
        return handle.ctypes.data

    def free(self, handle):
        pass


class DeviceBackend:
    def __init__(self):
        from ns2vc_amd import _lib
        self.lib, self.check = _lib.load(), _lib.check

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.check(self.lib.ns2vc_dev_malloc(C.byref(p), nbytes), "dev_malloc")
        return p.value

    def upload(self, handle, image_u8):
        self.check(self.lib.ns2vc_memcpy_h2d(handle, image_u8.ctypes.data, image_u8.nbytes), "memcpy_h2d")

    def download(self, handle, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        self.check(self.lib.ns2vc_dev_sync(), "dev_sync")
        self.check(self.lib.ns2vc_memcpy_d2h(out.ctypes.data, handle, nbytes), "memcpy_d2h")
        return out

    def address(self, handle):
        return handle

    def free(self, handle):
        self.lib.ns2vc_dev_free(handle)


def guard_elems(ld: int, esz: int) -> int:
    """(largest row tile + halo) rows of pitch ld, rounded up to 4 KB, in elements"""
    nbytes = (TILE_ROWS + HALO_ROWS) * max(ld, 1) * esz
    return (nbytes + GUARD_ROUND - 1) // GUARD_ROUND * GUARD_ROUND // esz


class Guarded:
    """rows x width elements of `kind` at pitch ld >= col0 + width inside one guarded block.

    data: the logical values ((rows, width)-shaped, or anything that reshapes to it); None = the NaN pattern of the kind (an output that
          must be written).  fill: what the guards and the gap columns hold.  skew: 1 = the block starts 16 bytes past a 128-byte
          boundary (a base that is 16-byte but not 128-byte aligned); 0 = `.ptr` of a col0 = 0 tensor is 128-byte aligned.
    ptr   address of logical element (0, 0);   base  its element index in `mem` (host back end);   ld  pitch in elements."""

    def __init__(self, backend, rows: int, width: int, kind: str, *, ld: int | None = None, col0: int = 0, fill: str = "nan",
                 data=None, skew: int = 0, name: str = ""):
        sdt, pats = KINDS[kind]
        self.kind, self.sdt, self.esz = kind, sdt, np.dtype(sdt).itemsize
        self.rows, self.width, self.col0, self.name, self.fill = rows, width, col0, name or kind, fill
        self.ld = ld = (col0 + width) if ld is None else ld
        per = ALIGN // self.esz if self.esz < ALIGN else 1
        assert rows >= 1 and width >= 1 and ld >= col0 + width, (rows, width, ld, col0)
        # (one contiguous row -- a vector, an NCT tensor -- has no pitch to align)
        assert (rows == 1 or ld % per == 0) and col0 % per == 0, f"{self.name}: pitch and column offset keep 16-byte alignment ({ld}, {col0})"
        g = guard_elems(ld, self.esz)
        self.front = g + (ALIGN // self.esz if skew else 0)
        self.back = g
        self.total = self.front + rows * ld + self.back
        self.base = self.front + col0
        img = np.full(self.total, pats[fill], dtype=sdt)
        body = img[self.front:self.front + rows * ld].reshape(rows, ld)
        if data is None:
            body[:, col0:col0 + width] = pats["nan"]
        else:
            body[:, col0:col0 + width] = encode(data, kind).reshape(rows, width)
        self.logical = np.zeros(self.total, dtype=bool)
        self.logical[self.front:self.front + rows * ld].reshape(rows, ld)[:, col0:col0 + width] = True
        self.image = img
        self.backend = backend
        self.handle = backend.malloc(self.total * self.esz)
        addr = backend.address(self.handle)
        assert addr % LINE == 0, "the allocator returns whole 128-byte lines"
        backend.upload(self.handle, img.view(np.uint8))
        self.ptr = addr + self.base * self.esz
        assert self.ptr % ALIGN == 0

    # host back end only: the whole block as the numpy "kernels" see device memory
    @property
    def mem(self) -> np.ndarray:
        return self.handle.view(self.sdt)

    def _download(self) -> np.ndarray:
        return self.backend.download(self.handle, self.total * self.esz).view(self.sdt)

    def read_bits(self) -> np.ndarray:
        """storage words of the logical region, (rows, width)"""
        return self._download()[self.logical].reshape(self.rows, self.width).copy()

    def read(self) -> np.ndarray:
        return decode(self.read_bits(), self.kind)

    def violations(self, limit: int = 24) -> list:
        """guard / gap elements whose bytes differ from what was uploaded, named by region; at most `limit` entries + a count of the rest"""
        now = self._download()
        bad = np.flatnonzero((now != self.image) & ~self.logical)
        out = []
        for i in bad[:limit]:
            i = int(i)
            if i < self.front:
                where = f"front (element {i - self.front}, {(self.front - i + self.ld - 1) // self.ld} row(s) before row 0)"
            elif i >= self.front + self.rows * self.ld:
                j = i - self.front - self.rows * self.ld
                where = f"back (element +{j}, row {self.rows + j // self.ld} col {j % self.ld - self.col0})"
            else:
                r, c = divmod(i - self.front, self.ld)
                where = f"gap row {r} col {c - self.col0}"
            out.append(f"{self.name}: {where}: {int(self.image[i]):#x} -> {int(now[i]):#x}")
        if len(bad) > limit:
            out.append(f"{self.name}: ... and {len(bad) - limit} more")
        return out

    def free(self):
        if self.handle is not None:
            self.backend.free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pattern_mismatches(runs: dict) -> list:
    """P2.  runs = {fill: {output name: Guarded or (bits, kind)}} of the same launch on the same logical data.  The logical outputs must be
    finite (floating kinds) and BITWISE equal across the fills: anything else means bytes outside a tensor took part in a result."""
    out = []
    got = {}
    for fill, outs in runs.items():
        for name, g in outs.items():
            bits, kind = (g.read_bits(), g.kind) if isinstance(g, Guarded) else g
            got[(fill, name)] = bits
            if kind in ("f32", "bf16", "f16"):
                v = decode(bits, kind)
                nf = np.argwhere(~np.isfinite(v))
                if len(nf):
                    out.append(f"{name} [{fill}]: {len(nf)} non-finite logical elements, first (row, col) {nf[:4].tolist()}")
    fills = list(runs)
    for name in runs[fills[0]]:
        for f in fills[1:]:
            a, b = got[(fills[0], name)], got[(f, name)]
            if a.shape != b.shape or not np.array_equal(a, b):
                d = np.argwhere(a != b) if a.shape == b.shape else []
                out.append(f"{name}: fill {fills[0]} vs {f}: {len(d)} logical elements differ, first (row, col) {d[:4].tolist() if len(d) else '-'}")
    return out
