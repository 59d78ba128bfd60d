"""One ns2vc_k_attention launch on guarded tensors and the fp64 reference of one item (test-side code, not product; a plain module like util.py).
Shared by tests/test_masked_attn_gpu.py and tests/test_attn_positions_gpu.py."""
import ctypes as C

import numpy as np

import guard as G

PREC_IDS = {0: "fp32", 1: "bf16", 2: "fp16"}
H0 = 2                                             # heads of a launch unless the caller says otherwise
OUT_FILL = 3.25                                    # what `out` holds before a launch (non-zero, exact in every operand type)


def _lib():
    from ns2vc_amd import _lib as L
    return L, L.load()


def _dev_i32(v):
    from ns2vc_amd.engine import DevBuf
    return DevBuf.from_numpy(np.ascontiguousarray(v, dtype=np.int32))


def _rounded(a, prec):
    kind = G.OP_KIND[prec]
    return G.decode(G.encode(a, kind), kind).astype(np.float64)


def _ref_item(q, k, v, bias, H, hd):
    """fp64 softmax attention of one item: q (Lq, D), k / v (Lk, D), bias (Lk) or None -> (Lq, D)"""
    Lq, Lk = q.shape[0], k.shape[0]
    qh, kh, vh = (t.reshape(-1, H, hd).transpose(1, 0, 2) for t in (q, k, v))
    s = qh @ kh.transpose(0, 2, 1) / np.sqrt(hd)
    if bias is not None:
        s = s + bias[None, None, :]
    s = s - s.max(-1, keepdims=True)
    p = np.exp(s)
    o = (p / p.sum(-1, keepdims=True)) @ vh
    assert o.shape == (H, Lq, hd) and Lk == v.shape[0]
    return o.transpose(1, 0, 2).reshape(Lq, H * hd)


def _launch(prec, hd, q, k, v, H=H0, bias=None, q_lens=None, k_lens=None, keys=0, optimistic=1, fill="nan", count=False, pv_fp8=0, exact_only=0):
    """one ns2vc_k_attention launch on guarded tensors.  q (B, Lq, D), k / v (B, Lk, D) float32 (NaN / Inf allowed) -> (status, storage words of
    `out` (B, Lq, D), guard violations, fallback workgroups or None)"""
    from ns2vc_amd.engine import DevBuf
    L, lib = _lib()
    bk = G.DeviceBackend()
    kind = G.OP_KIND[prec]
    B, Lq, D = q.shape
    Lk = k.shape[1]
    gs = [G.Guarded(bk, B * Lq, D, kind, data=q.reshape(B * Lq, D), fill=fill, name="q"),
          G.Guarded(bk, B * Lk, D, kind, data=k.reshape(B * Lk, D), fill=fill, name="k"),
          G.Guarded(bk, B * Lk, D, kind, data=v.reshape(B * Lk, D), fill=fill, name="v"),
          G.Guarded(bk, B * Lq, D, kind, data=np.full((B * Lq, D), OUT_FILL, np.float32), fill=fill, name="out")]
    keep = [_dev_i32(t) if t is not None else None for t in (q_lens, k_lens)]
    d_bias = DevBuf.from_numpy(np.ascontiguousarray(bias, dtype=np.float32)) if bias is not None else None
    d_cnt = DevBuf.from_numpy(np.zeros(4, dtype=np.uint32)) if count else None
    a = L.AttnArgs()
    a.q, a.k, a.v, a.out = gs[0].ptr, gs[1].ptr, gs[2].ptr, gs[3].ptr
    a.ldq = a.ldk = a.ldv = a.ldo = D
    a.B, a.H, a.Lq, a.Lk = B, H, Lq, Lk
    a.scale = 1.0 / np.sqrt(hd)
    a.pv_fp8 = pv_fp8
    a.exact_only = exact_only
    if d_bias is not None:
        a.bias = d_bias.ptr
    if keep[0] is not None:
        a.q_lens = keep[0].ptr
    if keep[1] is not None:
        a.k_lens = keep[1].ptr
    if d_cnt is not None:
        a.fallbacks = d_cnt.ptr
    L.check(lib.ns2vc_debug_set_attn_keys(keys), "set_attn_keys")
    L.check(lib.ns2vc_debug_set_attn_optimistic(optimistic), "set_attn_optimistic")
    try:
        rc = lib.ns2vc_k_attention(C.byref(a), hd, prec, None)
        L.check(lib.ns2vc_dev_sync(), "sync")
    finally:
        lib.ns2vc_debug_set_attn_keys(0)
        lib.ns2vc_debug_set_attn_optimistic(1)
    bits = gs[3].read_bits().reshape(B, Lq, D)
    viol = sum((g.violations() for g in gs), [])
    nfb = int(d_cnt.to_numpy((4,)).view(np.uint32)[0]) if d_cnt is not None else None
    for g in gs:
        g.free()
    return rc, bits, viol, nfb


def _vals(bits, prec):
    return G.decode(bits.reshape(-1), G.OP_KIND[prec]).reshape(bits.shape).astype(np.float64)
