// Epilogue building blocks shared by the implicit-GEMM kernels (gemm2_kernel, gemm4_kernel in gemm.hip, conv3ts_kernel in convts.hip), gfx950.
//
// C layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5), i.e. a lane owns ONE column: direct stores would be
// 4-byte (fp32) / 2-byte (16-bit) scalars.  Instead the waves transpose their tiles through the (then idle) LDS rings and move whole rows:
// 16-B loads of bias / residual, 16-B fp32 and 8-B 16-bit stores, fully coalesced.  A row is held by LPR lanes (a column quad each),
// a wave emits 64 / LPR rows per pass.
//
// What differs between the kernels stays with them and comes in as two callables:
//   ld(row, col)  -> float4   the staged partial sums of slab row `row`, floats col .. col+3 (the caller adds its K halves, 0 + 1 in that order)
//   rowof(row)    -> EpiRow   the result row that slab row becomes (gemm: m = m0 + ..; conv: padded q -> (b, t) -> real row)
// and so do the slab loop, its barriers (LDS-only, lds_barrier(): the stores of the previous slab are in flight and nobody waits for them)
// and the trace stamps.
#pragma once
#include "common.h"
#include "mma.h"

namespace ns2vc {

// ---------------------------------------------------------------------------
// LayerNorm by linearity.  LayerNorm(x) W^T = rstd * (x W^T - mean * rowsum(W)), so a GEMM whose input is a LayerNorm
// reads the RAW x (the operand copy its producer writes anyway) and fixes the result up in the epilogue; the
// producer's epilogue leaves (sum, sum of squares) per row and 64-column slice as plain fp32 stores (one writer per
// slot: deterministic, nothing to zero).  No normalisation pass over HBM.
// ---------------------------------------------------------------------------
// consumer, part 1 (top of the kernel, so the cold-load latency hides under the K loop): this lane's row pairs, raw
struct LnRaw { float4 v[4]; };                      // up to 8 slices of 64 channels = ln_dim 512
__device__ __forceinline__ void ln_row_load(const GemmArgs& g, int m, bool valid, LnRaw& r) {
  const int n4 = g.ln_stats ? (g.ln_dim >> 7) : 0;  // float4 = two (sum, sumsq) pairs = 128 channels
  const float4* p = reinterpret_cast<const float4*>(g.ln_stats + (size_t)min(m, g.M - 1) * (g.ln_dim >> 6) * 2);
#pragma unroll
  for (int i = 0; i < 4; ++i) r.v[i] = (valid && i < n4) ? p[i] : make_float4(0.f, 0.f, 0.f, 0.f);
}
// consumer, part 2 (epilogue): mean / rstd of the row
__device__ __forceinline__ void ln_row_finish(const GemmArgs& g, const LnRaw& r, float& mean_f, float& rstd_f, int n0) {
  float s = 0.f, q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) { s += r.v[i].x + r.v[i].z; q += r.v[i].y + r.v[i].w; }
  const float inv = 1.0f / (float)max(g.ln_dim, 1);
  const float mean = s * inv;
  double var = (double)q * (double)inv - (double)mean * (double)mean;     // the one cancellation-prone step
  if (var < 0.0) var = 0.0;
  mean_f = mean;
  rstd_f = 1.0f / sqrtf((float)var + g.ln_eps);
  // health of the linearity trick: the 16-bit modes round the raw row BEFORE centring, so the error on a row grows with
  // |mean| / std.  The first column workgroup of every row panel reports the largest ratio it sees (a plain read first:
  // the atomic is issued only by a wave that raises the maximum, i.e. a handful of times per forward).
  if (g.ln_health && n0 == 0) {
    float ratio = fabsf(mean) * rstd_f;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ratio = fmaxf(ratio, __shfl_xor(ratio, o));
    if ((threadIdx.x & 63) == 0 && ratio > __uint_as_float(__hip_atomic_load(g.ln_health, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)))
      atomicMax(g.ln_health, __float_as_uint(ratio));
  }
}
// consumer, part 3: the fix-up of one column quad; ws = rowsum(W) of its columns
__device__ __forceinline__ void ln_fix(float4& a, float mu, float rs, const float4& ws) {
  a.x = rs * (a.x - mu * ws.x); a.y = rs * (a.y - mu * ws.y); a.z = rs * (a.z - mu * ws.z); a.w = rs * (a.w - mu * ws.w);
}
// sum over the 16 lanes (one DPP row) that hold one 64-column slice of a result row; no LDS traffic, all 16 get the total
__device__ __forceinline__ float sum16_dpp(float x) {
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xB1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4E, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xf, 0xf, false));   // row_ror:4
  x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, false));   // row_ror:8
  return x;
}
// producer (64-column wave tiles only): (sum, sumsq) of row m's 64-column slice -> rowstats[m][ncol/64]
// (plain store by the slice's first lane: every slot has exactly one writer)
__device__ __forceinline__ void ln_row_store(const GemmArgs& g, int m, int ncol, const float2& sq) {
  *reinterpret_cast<float2*>(g.rowstats + ((size_t)m * (g.N >> 6) + (ncol >> 6)) * 2) = sq;
}

// ---------------------------------------------------------------------------
// fragment -> LDS slab: one 32-row block of a wave tile (NT 32x32 fragments side by side), rows of EP floats (EP = columns + 4: 16-B aligned
// rows, conflict-free column writes)
// ---------------------------------------------------------------------------
template <int NT, int EP>
__device__ __forceinline__ void epi_stage(float* et, const f32x16_t (&acc)[NT], int lane) {
  // element r of fragment j -> row 8*(r>>2) + 4*hi + (r&3), column j*32 + l31 (hi = lane>>5, l31 = lane&31).  The lane's part sits in the
  // pointer, so the 16 * NT stores differ by immediate offsets only and pair up (ds_write2_b32)
  float* const p = et + (4 * (lane >> 5)) * EP + (lane & 31);
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) p[(8 * (r >> 2) + (r & 3)) * EP + j * 32] = acc[j][r];
}

// slab row that pass k of a wave moves out: LPR lanes hold a row, so a pass covers 64 / LPR rows
template <int LPR> __device__ __forceinline__ int epi_slab_row(int lane, int k) { return k * (64 / LPR) + lane / LPR; }

// LayerNorm consumers: lane l holds mean / rstd of the wave's l-th row (ln_row_finish); slab row 0 is the wave's row `base`.  Others pass LnRow{}.
struct LnRow { float mean = 0.f, rstd = 1.f; int base = 0; };

// One result row as its kernel's row map sees it.  `m`: its row in the output tensors (meaningful where it is stored; gemm leaves it linear in the
// slab row, so that the store addresses of a pass differ by scalars).  `mres`: the row its residual is read from: m, clamped into the tensor
// where the row is not stored (so that loads need no per-lane condition).  `stored`: the row exists (gemm: m < M; conv: no pad row, not past
// the tile's own rows).
// `live`: it takes part in the result.  Per-item valid lengths (MASKED kernels, GemmArgs.lens): a row (b, t) with t >= lens[b] is stored but not
// live -- exact zeros (no bias, no residual, whatever the accumulator holds), and outside the GroupNorm statistics.  Dense kernels pass
// live = stored and carry nothing of it.  `first`: it belongs to the first of the (at most two) batch items the wave's rows touch.
struct EpiRow { int m, mres; bool stored, live, first; };

// ---------------------------------------------------------------------------
// GroupNorm statistics of the result: per lane (sum, sum of squares) of its column quads, split between item b0 and item b0 + 1
// ---------------------------------------------------------------------------
struct GnStats {
  float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;
  __device__ __forceinline__ void add(bool first, float ps, float pq) {
    if (first) { s0 += ps; q0 += pq; } else { s1 += ps; q1 += pq; }
  }
  // fixed shuffle tree over the lanes that share a 16-channel block (4 column quads x all row lanes), then ONE int64 fixed-point atomic
  // per (batch item, block, moment): integer adds are order-independent => deterministic whatever order the workgroups arrive in.
  // `any`: the wave has rows at all; `second`: item b0 + 1 exists and starts inside the wave's rows
  template <int LPR>
  __device__ __forceinline__ void commit(const GemmArgs& g, int lane, int b0, int ncol, bool any, bool second) const {
    if (!g.stats) return;
    double d0 = s0, d1 = q0, d2 = s1, d3 = q1;
#pragma unroll
    for (int o = 1; o <= 2; o <<= 1) {                       // the 4 column quads of a 16-channel block
      d0 += __shfl_xor(d0, o); d1 += __shfl_xor(d1, o); d2 += __shfl_xor(d2, o); d3 += __shfl_xor(d3, o);
    }
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) {                     // the row lanes
      d0 += __shfl_xor(d0, o); d1 += __shfl_xor(d1, o); d2 += __shfl_xor(d2, o); d3 += __shfl_xor(d3, o);
    }
    if (lane / LPR == 0 && ((lane % LPR) & 3) == 0 && any) {
      const int blk = ncol >> 4, nblk = g.N >> 4;
      unsigned long long* st = reinterpret_cast<unsigned long long*>(g.stats) + ((size_t)b0 * nblk + blk) * 2;
      atomicAdd(st, (unsigned long long)llrint(d0 * GN_SUM_SCALE));
      atomicAdd(st + 1, (unsigned long long)llrint(d1 * GN_SQ_SCALE));
      if (second) {
        atomicAdd(st + 2 * nblk, (unsigned long long)llrint(d2 * GN_SUM_SCALE));
        atomicAdd(st + 2 * nblk + 1, (unsigned long long)llrint(d3 * GN_SQ_SCALE));
      }
    }
  }
};

// ---------------------------------------------------------------------------
// linear rows: v = a + bias + res, fp32 and / or operand-typed stores, GroupNorm / LayerNorm partial statistics of v
// ---------------------------------------------------------------------------
// a lane's column quad: first column, bias, (LayerNorm consumers) rowsum(W).  col0 = first column of the wave tile
template <int LPR, bool LNC> struct LinearCols {
  int ncol;
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f), ws = bv;
  __device__ __forceinline__ LinearCols(int lane, int col0) : ncol(col0 + (lane % LPR) * 4) {}
  __device__ __forceinline__ void load(const GemmArgs& g) {
    if (g.bias) bv = *reinterpret_cast<const float4*>(g.bias + ncol);
    if constexpr (LNC) ws = *reinterpret_cast<const float4*>(g.ln_wsum + ncol);
  }
};
template <int NIT> struct LinearRows {
  float4 v[NIT];
  float2 sq[NIT];                                              // (sum, sumsq) of the row's 64-column slice, for rowstats
};
// Two passes: FIRST every value of the slab is computed into its own registers (this consumes all residual rows and
// LDS reads), THEN all stores are issued back to back.  Interleaved, the compiler had to wait for stores to complete
// (s_waitcnt vmcnt) before it could reuse a store's data registers for the next row pass, and with loads and stores
// both pending it can only wait with vmcnt(0): every pass sat through the write latency of the previous one.
//
// Pass 1.  Slab rows k * (64 / LPR) + lane / LPR, k < NIT.  LNC: lane l holds mean / rstd of the wave's l-th row, see LnRow.
// RS: the kernel can produce rowstats (64-column wave tiles).
template <int LPR, int NIT, bool LNC, bool RS, typename Ld, typename RowOf>
__device__ __forceinline__ void epi_linear_values(const GemmArgs& g, int lane, const LinearCols<LPR, LNC>& c, const LnRow& ln,
                                                  GnStats& gn, LinearRows<NIT>& e, Ld ld, RowOf rowof) {
  const int cq = lane % LPR;
  EpiRow rw[NIT];
#pragma unroll
  for (int k = 0; k < NIT; ++k) rw[k] = rowof(epi_slab_row<LPR>(lane, k));
  float4 rr[NIT];                               // every residual row before the first store: res may alias out_f32 element-for-element
  if (g.res) {                                  // (uniform branch, clamped rows that are never stored: straight-line loads -- per-lane
#pragma unroll                                  //  conditional loads were compiled with a wait after each)
    for (int k = 0; k < NIT; ++k) rr[k] = *reinterpret_cast<const float4*>(g.res + (size_t)rw[k].mres * g.ldres + c.ncol);
  } else {
#pragma unroll
    for (int k = 0; k < NIT; ++k) rr[k] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const int row = epi_slab_row<LPR>(lane, k);
    float4 a = ld(row, cq * 4);
    if constexpr (LNC) ln_fix(a, __shfl(ln.mean, ln.base + row), __shfl(ln.rstd, ln.base + row), c.ws);
    float ps = 0.f, pq = 0.f;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rw[k].live) {
      v.x = a.x + c.bv.x + rr[k].x; v.y = a.y + c.bv.y + rr[k].y; v.z = a.z + c.bv.z + rr[k].z; v.w = a.w + c.bv.w + rr[k].w;
      ps = (v.x + v.y) + (v.z + v.w); pq = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
      gn.add(rw[k].first, ps, pq);
    }
    e.v[k] = v;
    if constexpr (RS) {
      e.sq[k] = make_float2(0.f, 0.f);
      if (g.rowstats) e.sq[k] = make_float2(sum16_dpp(ps), sum16_dpp(pq));
    }
  }
}
// Pass 2
template <typename TM, int LPR, int NIT, bool RS, typename RowOf>
__device__ __forceinline__ void epi_linear_store(const GemmArgs& g, int lane, int ncol, const LinearRows<NIT>& e, RowOf rowof) {
  float* of = g.out_f32;
  TM* oo = reinterpret_cast<TM*>(g.out_op);
#pragma unroll
  for (int k = 0; k < NIT; ++k) {
    const EpiRow rw = rowof(epi_slab_row<LPR>(lane, k));
    if (rw.stored) {
      const int m = rw.m;
      if (of) out_f4(of + (size_t)m * g.ldo_f32 + ncol, e.v[k].x, e.v[k].y, e.v[k].z, e.v[k].w);
      if (oo) out_op4<TM>(oo + (size_t)m * g.ldo_op + ncol, e.v[k].x, e.v[k].y, e.v[k].z, e.v[k].w);
      if constexpr (RS) { if (g.rowstats && lane % LPR == 0) ln_row_store(g, m, ncol, e.sq[k]); }
    }
  }
}

// ---------------------------------------------------------------------------
// GEGLU rows (64-column wave tiles of the packed [value 32 | gate 32] column order): out = (value + bv) * gelu_erf(gate + bg) + res;
// 32 output columns per row = 8 lanes x 4, 8 rows per pass
// ---------------------------------------------------------------------------
template <bool LNC> struct GegluCols {
  int pcol, ocol;                                              // packed column of the value quad (gate quad = +32); output column
  float4 bv = make_float4(0.f, 0.f, 0.f, 0.f), bg = bv, wsv = bv, wsg = bv;
  __device__ __forceinline__ GegluCols(int lane, int col0) : pcol(col0 + (lane & 7) * 4), ocol((col0 >> 1) + (lane & 7) * 4) {}
  __device__ __forceinline__ void load(const GemmArgs& g) {
    if (g.bias) { bv = *reinterpret_cast<const float4*>(g.bias + pcol); bg = *reinterpret_cast<const float4*>(g.bias + pcol + 32); }
    if constexpr (LNC) { wsv = *reinterpret_cast<const float4*>(g.ln_wsum + pcol); wsg = *reinterpret_cast<const float4*>(g.ln_wsum + pcol + 32); }
  }
};
template <typename TM, int NIT, bool LNC, typename Ld, typename RowOf>
__device__ __forceinline__ void epi_geglu_rows(const GemmArgs& g, int lane, const GegluCols<LNC>& c, const LnRow& ln, Ld ld, RowOf rowof) {
  float* of = g.out_f32;
  TM* oo = reinterpret_cast<TM*>(g.out_op);
  const int rsub = lane >> 3, cq = lane & 7;
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int row = it * 8 + rsub;
    const EpiRow rw = rowof(row);
    float4 a = ld(row, cq * 4);
    float4 t = ld(row, 32 + cq * 4);
    if constexpr (LNC) {
      const float mu = __shfl(ln.mean, ln.base + row), rs = __shfl(ln.rstd, ln.base + row);
      ln_fix(a, mu, rs, c.wsv);
      ln_fix(t, mu, rs, c.wsg);
    }
    if (rw.stored) {
      float4 v;
      v.x = (a.x + c.bv.x) * gelu_erf_f(t.x + c.bg.x); v.y = (a.y + c.bv.y) * gelu_erf_f(t.y + c.bg.y);
      v.z = (a.z + c.bv.z) * gelu_erf_f(t.z + c.bg.z); v.w = (a.w + c.bv.w) * gelu_erf_f(t.w + c.bg.w);
      if (g.res) {
        const float4 rr = *reinterpret_cast<const float4*>(g.res + (size_t)rw.mres * g.ldres + c.ocol);
        v.x += rr.x; v.y += rr.y; v.z += rr.z; v.w += rr.w;
      }
      if (!rw.live) v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (of) out_f4(of + (size_t)rw.m * g.ldo_f32 + c.ocol, v.x, v.y, v.z, v.w);
      if (oo) out_op4<TM>(oo + (size_t)rw.m * g.ldo_op + c.ocol, v.x, v.y, v.z, v.w);
    }
  }
}

}  // namespace ns2vc
