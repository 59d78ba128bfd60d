// Memory-bound helper kernels of the NS2VC denoiser engine (gfx950): GroupNorm /
// LayerNorm statistics, the timestep-embedding MLP, prompt attention pooling,
// layout changes at the API boundary, the fused solver update and the per-item |x0| quantile of its corrected form.  All fp32,
// wave64, vectorised 16-B accesses on the channels-last activation layout.
#include "common.h"
#include <cmath>
#include <type_traits>
#include <vector>

namespace ns2vc {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// ---------------------------------------------------------------------------
// GroupNorm over a (possibly concatenated) channels-last fp32 tensor, in two launches.
// Reference: nn.GroupNorm at resnet.py:536,557 / transformer_1d.py:134 /
// unet_1d_condition.py:546; concat at unet_1d_blocks.py:2085,2187 (groups may
// straddle the seam between the two sources).
//
// 1) gn_partial: grid (nchunk, B); a half-wave (32 lanes) per group reduces `rows`
//    frames of one batch item and writes (sum, sumsq) in double.  Deterministic
//    (fixed shuffle tree), fp32 only inside a lane's <=128-element partial.
// 2) gn_apply: every block re-derives mean/rstd of its batch item from the
//    partials (G*nchunk doubles), folds gamma/beta and the resnet's time
//    scale/shift (resnet.py:625-629) into a per-channel affine and writes
//    act(x*scale+shift) as an OPERAND tensor [B*T][c0+c1] — the skip concat is
//    materialised here, in the operand type, as a side effect; optionally also the
//    raw concat for the resnet's 1x1 shortcut conv.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gn_partial_kernel(const float* __restrict__ a0, int lda0, int c0,
                                                         const float* __restrict__ a1, int lda1, int c1, int T, int G,
                                                         double* __restrict__ partial, int rows) {
  const int tid = threadIdx.x, b = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x;
  const int g = tid >> 5, i = tid & 31;
  const int C = c0 + c1, Cg = C / G, qpg = Cg >> 2;       // float4 quads per group (<= 32)
  const int rl = 32 / qpg;                                  // row lanes per half-wave
  const int quad = i % qpg, rlane = i / qpg;
  float sum = 0.f, sq = 0.f;
  const int r0 = chunk * rows, r1 = min(T, r0 + rows);
  if (g < G && rlane < rl) {
    const int c = g * Cg + quad * 4;
    const float* src; int ld, cs;
    if (c < c0) { src = a0; ld = lda0; cs = c; } else { src = a1; ld = lda1; cs = c - c0; }
    const float* p = src + ((size_t)b * T) * ld + cs;
    int r = r0 + rlane;
    for (; r + 3 * rl < r1; r += 4 * rl) {                  // 4 independent loads in flight
      const float4 v0 = *reinterpret_cast<const float4*>(p + (size_t)r * ld);
      const float4 v1 = *reinterpret_cast<const float4*>(p + (size_t)(r + rl) * ld);
      const float4 v2 = *reinterpret_cast<const float4*>(p + (size_t)(r + 2 * rl) * ld);
      const float4 v3 = *reinterpret_cast<const float4*>(p + (size_t)(r + 3 * rl) * ld);
      sum += ((v0.x + v0.y) + (v0.z + v0.w)) + ((v1.x + v1.y) + (v1.z + v1.w)) + ((v2.x + v2.y) + (v2.z + v2.w)) + ((v3.x + v3.y) + (v3.z + v3.w));
      sq += ((v0.x * v0.x + v0.y * v0.y) + (v0.z * v0.z + v0.w * v0.w)) + ((v1.x * v1.x + v1.y * v1.y) + (v1.z * v1.z + v1.w * v1.w)) +
            ((v2.x * v2.x + v2.y * v2.y) + (v2.z * v2.z + v2.w * v2.w)) + ((v3.x * v3.x + v3.y * v3.y) + (v3.z * v3.z + v3.w * v3.w));
    }
    for (; r < r1; r += rl) {
      const float4 v = *reinterpret_cast<const float4*>(p + (size_t)r * ld);
      sum += (v.x + v.y) + (v.z + v.w);
      sq += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
  }
  double ds = (double)sum, dq = (double)sq;
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) { ds += __shfl_xor(ds, o); dq += __shfl_xor(dq, o); }   // stays inside the half-wave
  if (i == 0 && g < G) {
    double* p = partial + ((size_t)(b * nchunk + chunk) * G + g) * 2;
    p[0] = ds; p[1] = dq;
  }
}

// MASK (per-item valid lengths, ns2vc_unet_set_lengths): statistics over the lens[b] valid rows of item b, and exact zeros written
// for rows >= lens[b] (what an unpadded run's conv zero padding reads there; GN(0) != 0).  The dense instantiation is the one above it.
template <typename TM, bool MASK = false>
__global__ __launch_bounds__(256) void gn_apply_kernel(const float* __restrict__ a0, int lda0, int c0, const float* __restrict__ a1,
                                                       int lda1, int c1, int T, int G, float eps, const double* __restrict__ partial,
                                                       int nchunk, const long long* __restrict__ st0, const long long* __restrict__ st1,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ temb, int ldtemb, int temb_off, int silu,
                                                       TM* __restrict__ out, TM* __restrict__ raw, int rows, int pair,
                                                       const int* __restrict__ lens) {
  op_mode_init<TM>();
  __shared__ float s_mean[8], s_rstd[8];
  const int tid = threadIdx.x, b = blockIdx.y, lane = tid & 63, wave = tid >> 6;
  const int nv = MASK ? lens[b] : T;            // valid rows of this item
  const int C = c0 + c1, nq = C >> 2, Cg = C / G;
  // streaming coordinates first: the activation loads do not depend on the statistics, so the first batch is in
  // flight while the block finalises mean / rstd (a chain of dependent global loads, shuffles and a double sqrt)
  const int rl = max(1, 256 / nq);
  const int quad = tid % nq, rlane = tid / nq;
  const bool active = rlane < rl;
  const int c = quad * 4;
  const float* src; int ld, cs;
  if (c < c0) { src = a0; ld = lda0; cs = c; } else { src = a1; ld = lda1; cs = c - c0; }
  const int r0 = blockIdx.x * rows, r1 = min(T, r0 + rows);
  float4 v[4];
  auto fetch = [&](int rb) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = rb + k * rl;
      v[k] = (active && r < r1) ? *reinterpret_cast<const float4*>(src + ((size_t)b * T + r) * ld + cs) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  fetch(r0 + rlane);
  // ... and so are the affine / time-conditioning vectors
  float4 ga = make_float4(0.f, 0.f, 0.f, 0.f), be = ga, t1 = ga, t2 = ga;
  if (active) {
    ga = *reinterpret_cast<const float4*>(gamma + c);
    be = *reinterpret_cast<const float4*>(beta + c);
    if (temb) {
      const float* tp = temb + (size_t)b * ldtemb + temb_off + c;
      if ((((size_t)b * ldtemb + temb_off) & 3) == 0) {
        t1 = *reinterpret_cast<const float4*>(tp);
        t2 = *reinterpret_cast<const float4*>(tp + C);
      } else {
        t1 = make_float4(tp[0], tp[1], tp[2], tp[3]);
        t2 = make_float4(tp[C], tp[C + 1], tp[C + 2], tp[C + 3]);
      }
    }
  }

  for (int g = wave; g < G; g += 4) {          // finalise the statistics of this batch item (every block, cheap)
    double ds = 0.0, dq = 0.0;
    if (st0) {                                 // fixed-point statistics left by the producing GEMMs' epilogues
      const int nb = Cg >> 4, nblk0 = c0 >> 4, nblk1 = c1 >> 4;
      if (lane < nb) {
        const int blk = g * nb + lane;         // 16-channel block of the (concatenated) input
        const long long* p = blk < nblk0 ? st0 + ((size_t)b * nblk0 + blk) * 2 : st1 + ((size_t)b * nblk1 + (blk - nblk0)) * 2;
        ds = (double)p[0] * (1.0 / GN_SUM_SCALE);
        dq = (double)p[1] * (1.0 / GN_SQ_SCALE);
      }
    } else {
      for (int k = lane; k < nchunk; k += 64) {
        const double* p = partial + ((size_t)(b * nchunk + k) * G + g) * 2;
        ds += p[0]; dq += p[1];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { ds += __shfl_xor(ds, o); dq += __shfl_xor(dq, o); }
    if (lane == 0) {
      // double only where it matters (E[x^2] - mean^2 cancels); reciprocal and rsqrt in fp32 (+1 Newton step): a double
      // divide / sqrt is a ~300-cycle software sequence and every workgroup sits on this chain before it can store
      const float inv_nf = 1.0f / ((float)nv * (float)Cg);
      const double inv_n = (double)inv_nf * (2.0 - (double)inv_nf * ((double)nv * (double)Cg));   // refine to ~double accuracy
      const double mean = ds * inv_n;
      double var = dq * inv_n - mean * mean;
      if (var < 0.0) var = 0.0;
      const float ve = (float)var + eps;
      float r = rsqrtf(ve);
      r = r * (1.5f - 0.5f * ve * r * r);
      s_mean[g] = (float)mean;
      s_rstd[g] = r;
    }
  }
  __syncthreads();
  if (!active) return;
  float sc[4], sh[4];
  {
    const int g = c / Cg;
    const float gam[4] = {ga.x, ga.y, ga.z, ga.w}, bet[4] = {be.x, be.y, be.z, be.w};
    const float ts[4] = {t1.x, t1.y, t1.z, t1.w}, tf[4] = {t2.x, t2.y, t2.z, t2.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      sc[e] = s_rstd[g] * gam[e];
      sh[e] = bet[e] - s_mean[g] * sc[e];
      if (temb) {
        const float s1 = 1.0f + ts[e];
        sc[e] *= s1;
        sh[e] = sh[e] * s1 + tf[e];
      }
    }
  }
  for (int rb = r0 + rlane; rb < r1; rb += 4 * rl) {     // 4 independent 16-B loads in flight per thread
    float4 w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = v[k];
    if (rb + 4 * rl < r1) fetch(rb + 4 * rl);            // next batch before this one is stored
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = rb + k * rl;
      if (r < r1) {
        const size_t row = (size_t)b * T + r;
        float y0 = w[k].x * sc[0] + sh[0], y1 = w[k].y * sc[1] + sh[1], y2 = w[k].z * sc[2] + sh[2], y3 = w[k].w * sc[3] + sh[3];
        if (silu) { y0 = silu_f(y0); y1 = silu_f(y1); y2 = silu_f(y2); y3 = silu_f(y3); }
        if (MASK && r >= nv) { y0 = y1 = y2 = y3 = 0.f; w[k] = make_float4(0.f, 0.f, 0.f, 0.f); }
        if (pair) {                                         // hi + lo operand pair (GemmArgs.gnp_pair writes the same): rows of 2 C columns
          out_op4<TM>(out + row * 2 * C + c, y0, y1, y2, y3);
          out_op4<TM>(out + row * 2 * C + C + c, op_rest<TM>(y0), op_rest<TM>(y1), op_rest<TM>(y2), op_rest<TM>(y3));
        } else {
          out_op4<TM>(out + row * C + c, y0, y1, y2, y3);
        }
        if (raw) out_op4<TM>(raw + row * C + c, w[k].x, w[k].y, w[k].z, w[k].w);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// LayerNorm (attention.py:83,102,118) without the affine part (gamma/beta are folded into the
// consumer GEMM's weights at pack time): one wave per fp32 row -> operand row.  C % 128 == 0.
// ---------------------------------------------------------------------------
template <typename TM, int NP>      // NP = float2 pairs per lane = C / 128
__global__ __launch_bounds__(256) void ln_apply_op_kernel(const float* __restrict__ x, int ldx, int M, int C, float eps,
                                                          TM* __restrict__ out) {
  op_mode_init<TM>();
  constexpr int R = 4;                          // rows per wave: 4 independent load streams / reduction chains
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
  if (row0 >= M) return;
  float2 v[R][NP];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const float* p = x + (size_t)min(row0 + r, M - 1) * ldx;
#pragma unroll
    for (int i = 0; i < NP; ++i) v[r][i] = *reinterpret_cast<const float2*>(p + 2 * (lane + 64 * i));
  }
  float s[R], q[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) s[r] += v[r][i].x + v[r][i].y;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] += __shfl_xor(s[r], o);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    s[r] /= (float)C;                           // mean
    q[r] = 0.f;
#pragma unroll
    for (int i = 0; i < NP; ++i) { const float d0 = v[r][i].x - s[r], d1 = v[r][i].y - s[r]; q[r] += d0 * d0 + d1 * d1; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int r = 0; r < R; ++r) q[r] += __shfl_xor(q[r], o);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (row0 + r < M) {
      const float rstd = 1.0f / sqrtf(q[r] / (float)C + eps);
      TM* o = out + (size_t)(row0 + r) * C;
#pragma unroll
      for (int i = 0; i < NP; ++i) store_op2<TM>(o + 2 * (lane + 64 * i), (v[r][i].x - s[r]) * rstd, (v[r][i].y - s[r]) * rstd);
    }
  }
}

template <typename TM>
__global__ __launch_bounds__(256) void cast_op_kernel(const float* __restrict__ x, size_t n4, TM* __restrict__ out, int split) {
  op_mode_init<TM>();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    if (split) {                                            // hi + lo operand pair: rows of 2 * split columns (see solver_update_kernel)
      TM* const q = out + 4 * i + ((4 * i) / (size_t)split) * (size_t)split;
      store_op4<TM>(q, v.x, v.y, v.z, v.w);
      store_op4<TM>(q + split, op_rest<TM>(v.x), op_rest<TM>(v.y), op_rest<TM>(v.z), op_rest<TM>(v.w));
    } else {
      store_op4<TM>(out + 4 * i, v.x, v.y, v.z, v.w);
    }
  }
}

// Full LayerNorm apply (used once per utterance for the prompt pooling path,
// embeddings.py:430).  Output row r of batch b goes to row b*(L+1)+1+t of `out`
// (row 0 of each item is reserved for the class token).
__global__ __launch_bounds__(256) void ln_apply_kernel(const float* __restrict__ x, int M, int C, float eps,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       float* __restrict__ out, int L) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const float* p = x + (size_t)row * C;
  float v[16];
  float s = 0.f;
  const int n = C >> 6;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    v[i] = (i < n) ? p[lane + 64 * i] : 0.f;
    s += v[i];
  }
  const float mean = wave_sum(s) / (float)C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const float d = (i < n) ? v[i] - mean : 0.f;
    q += d * d;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
  const int b = row / L, t = row - b * L;
  float* o = out + ((size_t)b * (L + 1) + 1 + t) * C;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    if (i < n) o[lane + 64 * i] = (v[i] - mean) * rstd * gamma[lane + 64 * i] + beta[lane + 64 * i];
}

// class token = mean_t(LN(prompt)) + positional_embedding  (embeddings.py:524).  grid (B, C/64): 64 channels x 4 time slices
// per block, the slices meet in LDS in a fixed order (was: one block per batch item walking all L rows serially, 109 us).
// P = frames summed (and the divisor), L = frames per item of `seq` (the row stride): P == L in the dense form
__device__ __forceinline__ void pool_cls_body(float* __restrict__ seq, int L, int P, int C, const float* __restrict__ pos) {
  __shared__ float part[4][64];
  const int b = blockIdx.x, c = blockIdx.y * 64 + (threadIdx.x & 63), sl = threadIdx.x >> 6;
  float s = 0.f;
  if (c < C) {
    const float* p = seq + ((size_t)b * (L + 1) + 1) * C + c;
    for (int t = sl; t < P; t += 4) s += p[(size_t)t * C];
  }
  part[sl][threadIdx.x & 63] = s;
  __syncthreads();
  if (sl == 0 && c < C) {
    const int i = threadIdx.x & 63;
    seq[(size_t)b * (L + 1) * C + c] = ((part[0][i] + part[1][i]) + (part[2][i] + part[3][i])) / (float)P + pos[c];
  }
}
__global__ __launch_bounds__(256) void pool_cls_kernel(float* __restrict__ seq, int L, int C, const float* __restrict__ pos) {
  pool_cls_body(seq, L, L, C, pos);
}
// per-item prompt lengths (ns2vc_unet_set_prompt_lengths): item b sums its frames t < plens[b] in the same slice order and divides by plens[b] --
// what the dense form does for that item alone at L = plens[b]; the rows past them are never read
__global__ __launch_bounds__(256) void pool_cls_lens_kernel(float* __restrict__ seq, int L, int C, const float* __restrict__ pos,
                                                            const int* __restrict__ plens) {
  pool_cls_body(seq, L, min(max(plens[blockIdx.x], 1), L), C, pos);
}

// AttentionPooling (embeddings.py:499-546): one query (the class token) per
// (batch, head); keys/values = [cls ; LN(prompt)].  qkv rows hold (q|k|v), each
// C wide.  One wave per head (grid (B, heads/4): was one block per batch item looping over 16 heads per wave, 188 us),
// lanes stride over keys.  dph = C/heads <= 8.
// L1 = rows per item of `qkv` (the row stride, and the stride of the waves' score rows), n = keys taken: n == L1 in the dense form
__device__ __forceinline__ void pool_attn_body(const float* __restrict__ qkv, int L1, int n, int C, int heads, float* __restrict__ pooled) {
  extern __shared__ float s_sc[];           // 4 waves x L1 scores
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int dph = C / heads;
  const float inv = 1.0f / sqrtf((float)dph);   // (q*s).(k*s), s = dph^-1/4
  float* sc = s_sc + wave * L1;
  const float* base = qkv + (size_t)b * L1 * 3 * C;
  {
    const int h = blockIdx.y * 4 + wave;
    if (h >= heads) return;
    float qv[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) qv[c] = (c < dph) ? base[h * dph + c] : 0.f;      // row 0 = class token
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) {
      const float* kp = base + (size_t)j * 3 * C + C + h * dph;
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < 8; ++c) if (c < dph) s += qv[c] * kp[c];
      s *= inv;
      sc[j] = s;
      mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    float den = 0.f;
    for (int j = lane; j < n; j += 64) {
      const float w = __expf(sc[j] - mx);
      den += w;
      const float* vp = base + (size_t)j * 3 * C + 2 * C + h * dph;
#pragma unroll
      for (int c = 0; c < 8; ++c) if (c < dph) acc[c] += w * vp[c];
    }
    den = wave_sum(den);
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const float a = wave_sum(acc[c]);
      if (lane == 0 && c < dph) pooled[(size_t)b * C + h * dph + c] = a / den;
    }
  }
}
__global__ __launch_bounds__(256) void pool_attn_kernel(const float* __restrict__ qkv, int L1, int C, int heads,
                                                        float* __restrict__ pooled) {
  pool_attn_body(qkv, L1, L1, C, heads, pooled);
}
// per-item prompt lengths: item b's keys are [0, plens[b] + 1) -- the class token and its own frames, in the order of the dense form at
// L1 = plens[b] + 1; the rows past them are never read
__global__ __launch_bounds__(256) void pool_attn_lens_kernel(const float* __restrict__ qkv, int L1, int C, int heads, float* __restrict__ pooled,
                                                             const int* __restrict__ plens) {
  pool_attn_body(qkv, L1, min(max(plens[blockIdx.x], 1), L1 - 1) + 1, C, heads, pooled);
}

// proj (Linear C->E) + LayerNorm(E)  (embeddings.py:431-433) -> aug_emb [B][E]
__global__ __launch_bounds__(256) void pool_proj_kernel(const float* __restrict__ pooled, int C, const float* __restrict__ wt,
                                                        const float* __restrict__ bias, int E, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps, float* __restrict__ out) {
  extern __shared__ float s_buf[];          // C inputs + E outputs + 8 scratch
  float* s_in = s_buf;
  float* s_y = s_buf + C;
  float* s_red = s_y + E;
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < C; i += 256) s_in[i] = pooled[(size_t)b * C + i];
  __syncthreads();
  float lsum = 0.f;
  for (int o = tid; o < E; o += 256) {
    float y = bias[o];
    for (int i = 0; i < C; ++i) y += wt[(size_t)i * E + o] * s_in[i];
    s_y[o] = y;
    lsum += y;
  }
  lsum = wave_sum(lsum);
  if ((tid & 63) == 0) s_red[tid >> 6] = lsum;
  __syncthreads();
  const float mean = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) / (float)E;
  float lq = 0.f;
  for (int o = tid; o < E; o += 256) { const float d = s_y[o] - mean; lq += d * d; }
  lq = wave_sum(lq);
  if ((tid & 63) == 0) s_red[4 + (tid >> 6)] = lq;
  __syncthreads();
  const float rstd = 1.0f / sqrtf((s_red[4] + s_red[5] + s_red[6] + s_red[7]) / (float)E + eps);
  for (int o = tid; o < E; o += 256) out[(size_t)b * E + o] = (s_y[o] - mean) * rstd * gamma[o] + beta[o];
}

// ---------------------------------------------------------------------------
// Timestep path: sinusoid -> Linear -> SiLU -> Linear, + aug_emb; also emits
// SiLU(emb), the input of every resnet's time_emb_proj.
// Reference: embeddings.py:24-64 (flip_sin_to_cos=True, freq_shift=0), :157-201,
// unet_1d_condition.py:841-848,918.  The timestep is fractional float32.
// ---------------------------------------------------------------------------
template <typename TM>
__global__ __launch_bounds__(256) void time_embed_kernel(const float* __restrict__ t_ptr, int t_stride, const int* __restrict__ step_ptr,
                                                         int coef_stride, const float* __restrict__ w1t, const float* __restrict__ b1,
                                                         const float* __restrict__ w2t, const float* __restrict__ b2,
                                                         const float* __restrict__ aug, float* __restrict__ emb,
                                                         TM* __restrict__ emb_act, int tdim, int edim) {
  op_mode_init<TM>();
  // grid (B, edim/64): every block recomputes the (cheap) hidden layer and produces 64 outputs of the second
  // Linear with 4 k-slices per output, so the 1 MB second weight matrix is spread over 8x more CUs.
  extern __shared__ float s_te[];           // tdim sinusoid + edim hidden + 256 partials
  float* s_sin = s_te;
  float* s_h = s_te + tdim;
  float* s_part = s_h + edim;
  const int b = blockIdx.x, oc = blockIdx.y, tid = threadIdx.x;
  const float t = step_ptr ? t_ptr[(size_t)(*step_ptr) * coef_stride] : t_ptr[(size_t)b * t_stride];
  const int half = tdim >> 1;
  for (int i = tid; i < half; i += 256) {
    const float expo = (-9.210340371976184f * (float)i) / (float)half;
    const float f = (float)exp((double)expo);          // (double: the reference's torch.exp of a float32 tensor is correctly rounded)
    const float ang = t * f;
    s_sin[i] = cosf(ang);
    s_sin[half + i] = sinf(ang);
  }
  __syncthreads();
  for (int o = tid; o < edim; o += 256) {
    float y0 = b1[o], y1 = 0.f, y2 = 0.f, y3 = 0.f;
#pragma unroll 8                                          // 32 independent weight loads in flight: the loop was one L2 round trip per 4 MACs
    for (int i = 0; i < tdim; i += 4) {
      y0 += w1t[(size_t)i * edim + o] * s_sin[i];
      y1 += w1t[(size_t)(i + 1) * edim + o] * s_sin[i + 1];
      y2 += w1t[(size_t)(i + 2) * edim + o] * s_sin[i + 2];
      y3 += w1t[(size_t)(i + 3) * edim + o] * s_sin[i + 3];
    }
    const float y = (y0 + y1) + (y2 + y3);
    s_h[o] = y / (1.0f + expf(-y));
  }
  __syncthreads();
  {
    const int o = oc * 64 + (tid & 63), ks = tid >> 6, kn = edim >> 2;     // k-slice [ks*kn, (ks+1)*kn)
    float y0 = 0.f, y1 = 0.f, y2 = 0.f, y3 = 0.f;
    const float* wp = w2t + (size_t)(ks * kn) * edim + o;
    const float* hp = s_h + ks * kn;
#pragma unroll 8
    for (int i = 0; i < kn; i += 4) {
      y0 += wp[(size_t)i * edim] * hp[i];
      y1 += wp[(size_t)(i + 1) * edim] * hp[i + 1];
      y2 += wp[(size_t)(i + 2) * edim] * hp[i + 2];
      y3 += wp[(size_t)(i + 3) * edim] * hp[i + 3];
    }
    s_part[tid] = (y0 + y1) + (y2 + y3);
  }
  __syncthreads();
  if (tid < 64) {
    const int o = oc * 64 + tid;
    float y = b2[o] + ((s_part[tid] + s_part[64 + tid]) + (s_part[128 + tid] + s_part[192 + tid]));
    if (aug) y += aug[(size_t)b * edim + o];
    emb[(size_t)b * edim + o] = y;
    if (emb_act) store_op<TM>(emb_act + (size_t)b * edim + o, y / (1.0f + expf(-y)));
  }
}
// Sampling loop: every batch item shares the step's timestep and the timesteps of all steps are known when the solver
// table is loaded, so the timestep MLP is evaluated ONCE per table (time_embed_kernel over the table's rows, aug = NULL)
// and a step only adds the prompt embedding: emb[b] = table[step] + aug[b] -- the same two fp32 additions in the same
// order as the direct kernel, hence bit-identical to it.
template <typename TM>
__global__ __launch_bounds__(256) void emb_from_table_kernel(const float* __restrict__ table, const int* __restrict__ step_ptr,
                                                             const float* __restrict__ aug, float* __restrict__ emb,
                                                             TM* __restrict__ emb_act, int edim, int n) {
  op_mode_init<TM>();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int o = i % edim;
  float y = table[(size_t)(*step_ptr) * edim + o];
  if (aug) y += aug[i];
  emb[i] = y;
  store_op<TM>(emb_act + i, y / (1.0f + expf(-y)));
}
// Per-item schedules (ns2vc_sampler_load_items): the table holds the timestep MLP of the rows of ALL distinct solver tables and item b reads
// the row of its own table at this loop step (common.h solver_item_row; a held item the clamped row -- its evaluation runs, its result is
// ignored).  emb[b] = table[row(b, step)] + aug[b]: the same two fp32 additions in the same order.  The records cover nitems loop items; a
// guided engine's 2 * nitems rows read them twice (both halves evaluate at the same timestep).
template <typename TM>
__global__ __launch_bounds__(256) void emb_items_from_table_kernel(const float* __restrict__ table, const int* __restrict__ step_ptr,
                                                                   const SolverItem* __restrict__ items, int nitems,
                                                                   const float* __restrict__ aug, float* __restrict__ emb,
                                                                   TM* __restrict__ emb_act, int edim, int n) {
  op_mode_init<TM>();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int b = i / edim, o = i - b * edim;
  bool active;
  const int row = solver_item_row(items[b % nitems], *step_ptr, active);
  float y = table[(size_t)row * edim + o];
  if (aug) y += aug[i];
  emb[i] = y;
  store_op<TM>(emb_act + i, y / (1.0f + expf(-y)));
}

// ---------------------------------------------------------------------------
// API-boundary layout changes: reference tensors are NCT (B,C,T); the engine is
// channels-last (B,T,Cpad).  32x32 LDS tile transpose, both directions coalesced.
// ---------------------------------------------------------------------------
template <typename TM>
__global__ __launch_bounds__(256) void nct_to_btc_kernel(const float* __restrict__ src, int C, int T, float* __restrict__ dst,
                                                         TM* __restrict__ dst_op, int ldd, int cpad, int ldd_op, int split) {
  op_mode_init<TM>();
  __shared__ float tile[32][33];
  const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < C && t < T) ? src[((size_t)b * C + c) * T + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (t < T && c < cpad) {
      if (dst) dst[((size_t)b * T + t) * ldd + c] = tile[tx][i];
      if (dst_op) {                                         // (split > 0: a hi + lo operand pair, the lo plane `split` columns further)
        TM* const q = dst_op + ((size_t)b * T + t) * ldd_op + c;
        store_op<TM>(q, tile[tx][i]);
        if (split) store_op<TM>(q + split, op_rest<TM>(tile[tx][i]));
      }
    }
  }
}
__global__ __launch_bounds__(256) void btc_to_nct_kernel(const float* __restrict__ src, int lds_, int C, int T, float* __restrict__ dst) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    tile[i][tx] = (t < T && c < C) ? src[((size_t)b * T + t) * lds_ + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c < C && t < T) dst[((size_t)b * C + c) * T + t] = tile[tx][i];
  }
}

// encoder_attention_mask (bool, True = keep) -> additive bias (unet_1d_condition.py:816-818)
__global__ void mask_bias_kernel(const uint8_t* __restrict__ mask, int n, float* __restrict__ bias) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) bias[i] = (1.0f - (mask[i] ? 1.0f : 0.0f)) * -10000.0f;
}
// the same row under per-item prompt lengths: the keys at or past plens[b] get the value a dropped key gets above, the keys below it the
// mask's value (mask == NULL: 0)
__global__ void prompt_bias_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ plens, int B, int Lp, float* __restrict__ bias) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * Lp) return;
  const int b = i / Lp, j = i - b * Lp;
  const bool keep = j < plens[b] && (!mask || mask[i]);
  bias[i] = (1.0f - (keep ? 1.0f : 0.0f)) * -10000.0f;
}

// ---------------------------------------------------------------------------
// Fused solver update (ns2vc_amd/schedule.py documents the recurrence and cites sampler/dpm_solver.py + sampler/uni_pc.py).  Scalars come from a
// row of the device-resident coefficient table chosen by *step_ptr, so the same captured graph serves every step.  The state is handled in quads
// of four floats (ld % 4 == 0: a quad lies in one row, so in one item of T rows of ld columns), and ONE function, solver_quad, is the update of a
// quad in every form: it loads the five state quads, guides x0, runs the element (common.h solver_elem), adds the noise and stores x_e', its operand
// copy and the state.  The forms, all compile time:
//   H2: the history-2 form of order-3 tables (a nonzero column 10 or 11), which also reads m_{i-2} from mprev2 and writes m_{i-1} there; H2 = false
//       is the order <= 2 update (mprev2 unused).
//   GD: classifier-free guidance on an engine of 2n items, rows [0, n*T) unconditional and [n*T, 2n*T) conditional.  n4 counts the quads of ONE
//       half; quad i combines x0[i] and x0[i + n4] by its item's scale (common.h guided_x0), updates the first half's state and writes xe / xe_op
//       to both halves, so the next evaluation is an ordinary 2n-item forward.  xbar, d1, mprev, mprev2 live in the first half only.
//   TH: the x0 correction (ns2vc_sampler_set_x0_correction; common.h solver_correct).  0 = none; 1 = by the item's threshold max(cx.thr[b],
//       cx.max_val), which the quantile kernel left there in the launch before; 2 = by cx.max_val alone.
//   noise (run time, only with H2 = false and TH = 0 -- launch_solver_step refuses the other pairs): a row with a nonzero column 9 adds knz * z to xbar'
//       on the live elements, z = Philox normals keyed by the item's seed and (frame, channel quad, jrow).  knz == 0 is no term at all (adding 0 * z
//       would turn -0 into +0), so every noise-free table keeps its bits.
// The host states a step once, as a SolverStep (common.h), and launch_solver_step picks the kernel: solver_update_kernel (TH = 0) and
// solver_update_th_kernel (TH = 1 | 2) on the row `step` of a table all items share, solver_update_items_kernel on every item's own row,
// solver_update_mixed_kernel on every item's own row and correction record.
// Every form's quad is a straight line from its loads to its stores, and a kernel that runs two forms (the items kernel: H2 is a property of the
// item) sweeps the quads once per form.  One sweep that branched per quad and joined the two forms' results in front of common stores was one ulp
// off on x_e' (seen on the device): the optimiser moves the last subtraction of the two forms into the block where they join, away from its
// products, and the fused multiply-adds of the straight-line form are lost.  For the same reason x_e' is formed once, behind the noise branch
// (common.h solver_xe), not in the element and again in the branch.  tests/test_solver_bits_gpu.py holds every form to recorded bits.
// ---------------------------------------------------------------------------
// the scalars of one table row: the element's coefficients, the noise coefficient (0 without seeds), the history-2 pair
struct SolverRow { SolverCoef k; float knz, d2c, pe; };
template <bool H2>
__device__ __forceinline__ SolverRow solver_row(const float* __restrict__ crow, bool noisy) {
  return SolverRow{solver_coef(crow), (!H2 && noisy) ? crow[9] : 0.f, H2 ? crow[10] : 0.f, H2 ? crow[11] : 0.f};
}
// the new x_e of quad i and its operand copy: fp32 rows, or for 16-bit types the hi + lo pair in rows of 2 * split columns, the lo plane `split` columns further
template <typename TM>
__device__ __forceinline__ void solver_store_xe(float* __restrict__ xe, TM* __restrict__ xe_op, size_t i, int split, const float4& oxe) {
  out_f4(xe + 4 * i, oxe.x, oxe.y, oxe.z, oxe.w);
  if (split) {
    const size_t r = (4 * i) / (size_t)split;
    TM* const q = xe_op + 4 * i + r * (size_t)split;
    out_op4<TM>(q, oxe.x, oxe.y, oxe.z, oxe.w);
    out_op4<TM>(q + split, op_rest<TM>(oxe.x), op_rest<TM>(oxe.y), op_rest<TM>(oxe.z), op_rest<TM>(oxe.w));
  } else {
    out_op4<TM>(xe_op + 4 * i, oxe.x, oxe.y, oxe.z, oxe.w);
  }
}
// RECORDED BEHAVIOUR, kept bit for bit (tests/test_solver_bits_gpu.py): under per-item schedules (own_rows) the x_e' of a quad that TOOK noise is
// the difference of xbar' and the ROUNDED product pc * d1' -- one rounding more than solver_xe's multiply-add, which every other quad and the
// shared-table kernels have.  The kernel this body replaced came out that way by code motion; a change that may move bits should drop it.
__device__ __forceinline__ float solver_xe_rounded(const SolverCoef& k, float oxb, float od1) {
#pragma clang fp contract(off)
  const float p = k.pc * od1;
  return oxb - p;
}
// quad i with the scalars kr of its row; jrow = the Philox "table row" word; T, ld = the item shape (read only where an item index is needed)
template <typename TM, bool H2, bool GD, int TH>
__device__ __forceinline__ void solver_quad(const SolverRow& kr, int jrow, size_t i, const float* __restrict__ x0, float* __restrict__ xe,
                                            TM* __restrict__ xe_op, float* __restrict__ xbar, float* __restrict__ d1, float* __restrict__ mprev,
                                            float* __restrict__ mprev2, size_t n4, int split, const SolverNoise& nz, const SolverGuide& gd,
                                            const SolverCorrect& cx, int T, int ld, bool own_rows) {
  static_assert(TH >= 0 && TH <= 2, "0 = uncorrected, 1 = dynamic thresholding, 2 = clamp");
  const SolverCoef& k = kr.k;
  const auto item = [&] { return (int)(((4 * i) / (size_t)ld) / (size_t)T); };
  float4 vx0 = reinterpret_cast<const float4*>(x0)[i];
  if constexpr (GD) {
    const float4 vxc = reinterpret_cast<const float4*>(x0)[i + n4];
    const float sc = gd.scale[item()];
    vx0 = make_float4(guided_x0(vx0.x, vxc.x, sc), guided_x0(vx0.y, vxc.y, sc), guided_x0(vx0.z, vxc.z, sc), guided_x0(vx0.w, vxc.w, sc));
  }
  const float4 vxe = reinterpret_cast<const float4*>(xe)[i];
  const float4 vxb = reinterpret_cast<const float4*>(xbar)[i];
  const float4 vd1 = reinterpret_cast<const float4*>(d1)[i];
  const float4 vmp = reinterpret_cast<const float4*>(mprev)[i];
  float sb = 0.f;
  if constexpr (TH != 0) sb = TH == 1 ? fmaxf(cx.thr[item()], cx.max_val) : cx.max_val;
  float4 vm2 = make_float4(0.f, 0.f, 0.f, 0.f);
  if constexpr (H2) vm2 = reinterpret_cast<const float4*>(mprev2)[i];
  float4 oxb, od1, om;
  solver_elem<H2, TH>(k, sb, kr.d2c, vx0.x, vxe.x, vxb.x, vd1.x, vmp.x, vm2.x, oxb.x, od1.x, om.x);
  solver_elem<H2, TH>(k, sb, kr.d2c, vx0.y, vxe.y, vxb.y, vd1.y, vmp.y, vm2.y, oxb.y, od1.y, om.y);
  solver_elem<H2, TH>(k, sb, kr.d2c, vx0.z, vxe.z, vxb.z, vd1.z, vmp.z, vm2.z, oxb.z, od1.z, om.z);
  solver_elem<H2, TH>(k, sb, kr.d2c, vx0.w, vxe.w, vxb.w, vd1.w, vmp.w, vm2.w, oxb.w, od1.w, om.w);
  if constexpr (H2) out_f4(mprev2 + 4 * i, vmp.x, vmp.y, vmp.z, vmp.w);
  bool noised = false;
  float4 oxe_rounded;
  if constexpr (!H2 && TH == 0) {
    if (kr.knz != 0.f) {      // xbar' += noise * z on the live elements (the state is zero elsewhere and stays so)
      const size_t e = 4 * i, r = e / (size_t)ld;
      const int c = (int)(e - r * (size_t)ld), b = (int)(r / (size_t)T), t = (int)(r - (size_t)b * T);
      if (c < nz.nc && (!nz.lens || t < nz.lens[b])) {
        const float4 z = philox_gauss4(nz.seeds[b], (uint32_t)t, (uint32_t)(c >> 2), (uint32_t)jrow);
        oxb.x += kr.knz * z.x;
        if (c + 1 < nz.nc) oxb.y += kr.knz * z.y;
        if (c + 2 < nz.nc) oxb.z += kr.knz * z.z;
        if (c + 3 < nz.nc) oxb.w += kr.knz * z.w;
        if (own_rows) {
          noised = true;
          oxe_rounded = make_float4(solver_xe_rounded(k, oxb.x, od1.x), solver_xe_rounded(k, oxb.y, od1.y), solver_xe_rounded(k, oxb.z, od1.z),
                                    solver_xe_rounded(k, oxb.w, od1.w));
        }
      }
    }
  }
  float4 oxe = make_float4(solver_xe<H2>(k, kr.pe, oxb.x, od1.x, om.x, vm2.x), solver_xe<H2>(k, kr.pe, oxb.y, od1.y, om.y, vm2.y),
                           solver_xe<H2>(k, kr.pe, oxb.z, od1.z, om.z, vm2.z), solver_xe<H2>(k, kr.pe, oxb.w, od1.w, om.w, vm2.w));
  if (noised) oxe = oxe_rounded;
  solver_store_xe<TM>(xe, xe_op, i, split, oxe);
  if constexpr (GD) solver_store_xe<TM>(xe, xe_op, i + n4, split, oxe);      // the conditional half evaluates at the same point (pair row r + n*T)
  out_f4(xbar + 4 * i, oxb.x, oxb.y, oxb.z, oxb.w);
  out_f4(d1 + 4 * i, od1.x, od1.y, od1.z, od1.w);
  out_f4(mprev + 4 * i, om.x, om.y, om.z, om.w);
}
template <typename TM, bool H2, bool GD>
__global__ __launch_bounds__(256) void solver_update_kernel(const float* __restrict__ coef, const int* __restrict__ step_ptr, int ncoef,
                                                            const float* __restrict__ x0, float* __restrict__ xe, TM* __restrict__ xe_op,
                                                            float* __restrict__ xbar, float* __restrict__ d1,
                                                            float* __restrict__ mprev, size_t n4, int split, SolverNoise nz,
                                                            float* __restrict__ mprev2, SolverGuide gd) {
  op_mode_init<TM>();
  const int step = *step_ptr;
  const SolverRow kr = solver_row<H2>(coef + (size_t)step * ncoef, nz.seeds != nullptr);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
    solver_quad<TM, H2, GD, 0>(kr, step, i, x0, xe, xe_op, xbar, d1, mprev, mprev2, n4, split, nz, gd, SolverCorrect(), GD ? gd.T : nz.T,
                               GD ? gd.ld : nz.ld, false);
}
// the corrected update: no noise term (the reference's discrete samplers have no correction, launch_solver_step refuses the pair); items are cx.T rows
// of cx.ld columns, under GD those of ONE half
template <typename TM, bool H2, bool GD, int TH>
__global__ __launch_bounds__(256) void solver_update_th_kernel(const float* __restrict__ coef, const int* __restrict__ step_ptr, int ncoef,
                                                               const float* __restrict__ x0, float* __restrict__ xe, TM* __restrict__ xe_op,
                                                               float* __restrict__ xbar, float* __restrict__ d1,
                                                               float* __restrict__ mprev, size_t n4, int split,
                                                               float* __restrict__ mprev2, SolverGuide gd, SolverCorrect cx) {
  static_assert(TH == 1 || TH == 2, "the uncorrected update is solver_update_kernel");
  op_mode_init<TM>();
  const int step = *step_ptr;
  const SolverRow kr = solver_row<H2>(coef + (size_t)step * ncoef, false);
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256)
    solver_quad<TM, H2, GD, TH>(kr, step, i, x0, xe, xe_op, xbar, d1, mprev, mprev2, n4, split, SolverNoise(), gd, cx, cx.T, cx.ld, false);
}
// The update under per-item schedules (ns2vc_sampler_load_items): every loop item walks a solver table of its own.  Quad i belongs to item
// b = (4 i / ld) / T; its record (common.h SolverItem) says where the item's rows sit in the coefficient table, how many there are, at which loop
// step it starts and which form it runs.  At loop step r = *step_ptr item b is ACTIVE when 0 <= r - start < steps and then uses row r - start of
// its table; otherwise it is HELD and nothing of it is loaded or stored: xe, both planes of xe_op, xbar, d1, mprev and mprev2 keep their bits.
// Flag SOLVER_ITEM_HIST2 -> H2 on every row of the item; flag SOLVER_ITEM_NOISE -> the noise term, its Philox "table row" word the item's LOCAL
// row, so the stream is what the item has alone.  n4 counts the quads of one half, the records cover the n loop items.  Two sweeps: the items
// without history 2, then (only with an mprev2 buffer) those with it.
template <typename TM, bool GD, int TH>
__global__ __launch_bounds__(256) void solver_update_items_kernel(const float* __restrict__ coef, const int* __restrict__ step_ptr, int ncoef,
                                                                  SolverItems si, const float* __restrict__ x0, float* __restrict__ xe,
                                                                  TM* __restrict__ xe_op, float* __restrict__ xbar, float* __restrict__ d1,
                                                                  float* __restrict__ mprev, size_t n4, int split, SolverNoise nz,
                                                                  float* __restrict__ mprev2, SolverGuide gd, SolverCorrect cx) {
  op_mode_init<TM>();
  const int step = *step_ptr;
  const auto sweep = [&](auto h2) {
    constexpr bool H2 = decltype(h2)::value;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
      const SolverItem it = si.rec[((4 * i) / (size_t)si.ld) / (size_t)si.T];
      bool active;
      const int row = solver_item_row(it, step, active);
      if (!active || ((it.flags & SOLVER_ITEM_HIST2) != 0) != H2) continue;      // held: nothing of this item is touched; the other form: the other sweep
      const SolverRow kr = solver_row<H2>(coef + (size_t)row * ncoef, TH == 0 && (it.flags & SOLVER_ITEM_NOISE) != 0);
      solver_quad<TM, H2, GD, TH>(kr, row - it.row0, i, x0, xe, xe_op, xbar, d1, mprev, mprev2, n4, split, nz, gd, cx, si.T, si.ld, true);
    }
  };
  sweep(std::false_type{});
  if (mprev2) sweep(std::true_type{});                                            // (without the buffer no item of the batch has history 2)
}
// The same under a per-item x0 correction (ns2vc_sampler_set_x0_correction_items): item b also has a record cr[b] (common.h ItemCorrect) whose mode
// is the TH of its quads, whose max_val is its cx.max_val and whose threshold is thr[b], left by abs_quantile_mixed_kernel in the launch before.
// The form of a quad is now (H2, TH), both properties of its item, and every form keeps its straight line (the comment above solver_quad): one sweep
// per form, six with an mprev2 buffer and three without, each a solver_quad of the items kernel's with a SolverCorrect filled from the record.  A
// stochastic item has mode 0 (the host refuses every other pair), so the noise term stays in the form it has, H2 = false and TH = 0.
template <typename TM, bool GD>
__global__ __launch_bounds__(256) void solver_update_mixed_kernel(const float* __restrict__ coef, const int* __restrict__ step_ptr, int ncoef,
                                                                  SolverItems si, const ItemCorrect* __restrict__ cr, const float* __restrict__ thr,
                                                                  const float* __restrict__ x0, float* __restrict__ xe, TM* __restrict__ xe_op,
                                                                  float* __restrict__ xbar, float* __restrict__ d1, float* __restrict__ mprev,
                                                                  size_t n4, int split, SolverNoise nz, float* __restrict__ mprev2, SolverGuide gd) {
  op_mode_init<TM>();
  const int step = *step_ptr;
  const auto sweep = [&](auto h2, auto th) {
    constexpr bool H2 = decltype(h2)::value;
    constexpr int TH = decltype(th)::value;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
      const int b = (int)(((4 * i) / (size_t)si.ld) / (size_t)si.T);
      const SolverItem it = si.rec[b];
      const ItemCorrect c = cr[b];
      bool active;
      const int row = solver_item_row(it, step, active);
      if (!active || ((it.flags & SOLVER_ITEM_HIST2) != 0) != H2 || c.mode != TH) continue;      // held, or another sweep's form
      const SolverRow kr = solver_row<H2>(coef + (size_t)row * ncoef, TH == 0 && (it.flags & SOLVER_ITEM_NOISE) != 0);
      SolverCorrect cx;
      cx.mode = TH; cx.thr = thr; cx.max_val = c.max_val; cx.T = si.T; cx.ld = si.ld;
      solver_quad<TM, H2, GD, TH>(kr, row - it.row0, i, x0, xe, xe_op, xbar, d1, mprev, mprev2, n4, split, nz, gd, cx, si.T, si.ld, true);
    }
  };
  sweep(std::false_type{}, std::integral_constant<int, 0>{});
  sweep(std::false_type{}, std::integral_constant<int, 1>{});
  sweep(std::false_type{}, std::integral_constant<int, 2>{});
  if (mprev2) {                                                                   // (without the buffer no item of the batch has history 2)
    sweep(std::true_type{}, std::integral_constant<int, 0>{});
    sweep(std::true_type{}, std::integral_constant<int, 1>{});
    sweep(std::true_type{}, std::integral_constant<int, 2>{});
  }
}
// ---------------------------------------------------------------------------
// Per-item quantile of |m| for the dynamic thresholding of the predicted x0 (sampler/dpm_solver.py:416-425, sampler/uni_pc.py:268-277:
// torch.quantile(|x0|.reshape(B, -1), p, dim=1)).  EXACT: a radix select over the IEEE bit pattern of |m| (for non-negative floats the unsigned
// order of the 31 low bits is the value order; a NaN sorts above every finite key), three digit passes of 11 + 10 + 10 bits, each a sweep of the
// item that counts the keys matching the prefix chosen so far into a 32-bit LDS histogram, then a block scan that picks the bin holding rank lo.
// The last pass leaves v_lo; v_hi == v_lo when at least two keys of that value remain at or above rank lo, else it is the next occupied bin
// of the last histogram, else (none: the next key differs in a higher digit) the minimum of the keys above v_lo by one more sweep.  Only integer
// counts and minima decide, so the result does not depend on scheduling.  thr[b] = torch's lerp of (v_lo, v_hi) at w = pos - lo,
// pos = p * (n - 1) in float32 (ns2vc_amd.schedule.abs_quantile is the host statement).
// One workgroup of 1024 threads per item and no communication between workgroups; every loop bound is a function of T, ld and the block size
// (lens is clamped to [0, T]).  An item's elements are rows t < lens[b] (NULL: T) and columns c < nc of its T rows of ld columns.
// SRC (compile time): 0 = the rows hold ready values; 1 = m is formed from x0, xe and the table row as the update forms it (solver_m); 2 = the same
// on guided_x0 of the two halves of x0 (q.half elements apart).  An item without elements gives 0.
// ---------------------------------------------------------------------------
template <int SRC>
__device__ __forceinline__ void quant_keys(const QuantArgs& q, const SolverCoef& k, float sc, size_t base, int quad, int ldq, unsigned key[4], int& nk) {
  const int t = quad / ldq, c = (quad - t * ldq) * 4;
  nk = min(4, q.nc - c);                       // (<= 0: a quad of padding columns)
  if (nk <= 0) return;
  const size_t e = base + (size_t)t * q.ld + c;
  float4 v = *reinterpret_cast<const float4*>(q.v + e);
  if constexpr (SRC != 0) {
    if constexpr (SRC == 2) {
      const float4 vc = *reinterpret_cast<const float4*>(q.v + q.half + e);
      v = make_float4(guided_x0(v.x, vc.x, sc), guided_x0(v.y, vc.y, sc), guided_x0(v.z, vc.z, sc), guided_x0(v.w, vc.w, sc));
    }
    const float4 x = *reinterpret_cast<const float4*>(q.xe + e);
    v = make_float4(solver_m(k, v.x, x.x), solver_m(k, v.y, x.y), solver_m(k, v.z, x.z), solver_m(k, v.w, x.w));
  }
  key[0] = __float_as_uint(v.x) & 0x7FFFFFFFu; key[1] = __float_as_uint(v.y) & 0x7FFFFFFFu;
  key[2] = __float_as_uint(v.z) & 0x7FFFFFFFu; key[3] = __float_as_uint(v.w) & 0x7FFFFFFFu;
}
// the select over the nquad quads of item b (n > 0 live elements), m formed with the table row k and the guidance scale sc; writes thr[b]
template <int SRC>
__device__ __forceinline__ void quant_select(const QuantArgs& q, const SolverCoef& k, float sc, int b, int nquad, unsigned n, float* __restrict__ thr) {
  constexpr int NT = 1024, NBIN = 2048;
  __shared__ unsigned s_hist[NBIN];
  __shared__ unsigned s_wave[16];
  __shared__ unsigned s_sel[4];                // chosen bin, keys below it, its count, minimum above
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ldq = q.ld >> 2;
  const size_t base = (size_t)b * q.T * q.ld;
  const float pos = q.p * (float)(n - 1);
  const unsigned lo = min((unsigned)floorf(pos), n - 1), hi = min((unsigned)ceilf(pos), n - 1);
  const float w = pos - (float)lo;
  unsigned prefix = 0, pmask = 0, rank = lo, eq = 0;
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
    const unsigned dmask = pass == 0 ? 0x7FFu : 0x3FFu;
    for (int i = tid; i < NBIN; i += NT) s_hist[i] = 0;      // (the last reads of the pass before lie in front of its second barrier)
    if (pass == 0 && tid < 4) s_sel[tid] = tid == 3 ? 0xFFFFFFFFu : 0u;
    __syncthreads();
    for (int quad = tid; quad < nquad; quad += NT) {
      unsigned key[4]; int nk;
      quant_keys<SRC>(q, k, sc, base, quad, ldq, key, nk);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < nk && (key[j] & pmask) == prefix) atomicAdd(&s_hist[(key[j] >> shift) & dmask], 1u);
    }
    __syncthreads();
    // block scan of the bins (two per thread, in bin order); the thread whose bins hold rank `rank` records the choice
    const unsigned h0 = s_hist[2 * tid], h1 = s_hist[2 * tid + 1];
    unsigned incl = h0 + h1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned u = __shfl_up(incl, o); if (lane >= o) incl += u; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    unsigned before = 0;
    for (int v = 0; v < wave; ++v) before += s_wave[v];
    const unsigned excl = before + incl - (h0 + h1);
    if (rank >= excl && rank < excl + h0) { s_sel[0] = 2 * tid; s_sel[1] = excl; s_sel[2] = h0; }
    else if (rank >= excl + h0 && rank < excl + h0 + h1) { s_sel[0] = 2 * tid + 1; s_sel[1] = excl + h0; s_sel[2] = h1; }
    __syncthreads();
    const unsigned d = s_sel[0];
    prefix |= d << shift;
    pmask |= dmask << shift;
    rank -= s_sel[1];
    eq = s_sel[2];
  }
  // v_lo = prefix; `eq` keys hold that value and `rank` of them lie below rank lo
  unsigned vhi = prefix;
  if (hi != lo && rank + 2 > eq) {             // (block-uniform) the key of rank lo + 1 is the smallest one above v_lo
    const unsigned d = prefix & 0x3FFu;
    const unsigned c0 = 2 * tid, c1 = 2 * tid + 1;
    unsigned cand = 0xFFFFFFFFu;
    if (c1 < 1024u && c1 > d && s_hist[c1]) cand = c1;
    if (c0 < 1024u && c0 > d && s_hist[c0]) cand = c0;
    if (cand != 0xFFFFFFFFu) atomicMin(&s_sel[3], (prefix & ~0x3FFu) | cand);
    __syncthreads();
    const unsigned next_bin = s_sel[3];
    __syncthreads();                           // (every thread has read it before anyone lowers it again)
    if (next_bin == 0xFFFFFFFFu) {             // (block-uniform) no occupied bin above: sweep for the minimum of the keys above v_lo
      unsigned mn = 0xFFFFFFFFu;
      for (int quad = tid; quad < nquad; quad += NT) {
        unsigned key[4]; int nk;
        quant_keys<SRC>(q, k, sc, base, quad, ldq, key, nk);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < nk && key[j] > prefix) mn = min(mn, key[j]);
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mn = min(mn, (unsigned)__shfl_xor(mn, o));
      if (lane == 0 && mn != 0xFFFFFFFFu) atomicMin(&s_sel[3], mn);
      __syncthreads();
    }
    vhi = s_sel[3] == 0xFFFFFFFFu ? prefix : s_sel[3];
  }
  if (tid == 0) {
    const float a = __uint_as_float(prefix), e = __uint_as_float(vhi), dlt = e - a;
    thr[b] = w < 0.5f ? fmaf(w, dlt, a) : fmaf(-dlt, 1.0f - w, e);     // torch's lerp
  }
}
// what the two kernels do after they have the item's table row: an item without elements gives 0 (block-uniform), every other one the select
template <int SRC>
__device__ __forceinline__ void quant_item(const QuantArgs& q, const SolverCoef& k, int b, float* __restrict__ thr) {
  const int len = q.lens ? min(max(q.lens[b], 0), q.T) : q.T;
  const unsigned n = (unsigned)len * (unsigned)q.nc;
  if (n == 0) {
    if (threadIdx.x == 0) thr[b] = 0.f;
    return;
  }
  quant_select<SRC>(q, k, SRC == 2 ? q.scale[b] : 1.f, b, len * (q.ld >> 2), n, thr);
}
template <int SRC>
__global__ __launch_bounds__(1024) void abs_quantile_kernel(QuantArgs q, float* __restrict__ thr) {
  SolverCoef k{};
  if constexpr (SRC != 0) k = solver_coef(q.coef + (size_t)(*q.step_ptr) * q.ncoef);
  quant_item<SRC>(q, k, blockIdx.x, thr);
}
// The same under per-item schedules (ns2vc_sampler_load_items; SRC 1 | 2: m is always formed there): item b's m comes from the row of its OWN
// table at this loop step (common.h solver_item_row), and the workgroup of a held item returns at once and leaves thr[b] alone.
template <int SRC>
__global__ __launch_bounds__(1024) void abs_quantile_items_kernel(QuantArgs q, float* __restrict__ thr, const SolverItem* __restrict__ items) {
  static_assert(SRC == 1 || SRC == 2, "ready values have no table row");
  bool active;
  const int row = solver_item_row(items[blockIdx.x], *q.step_ptr, active);
  if (!active) return;                         // (block-uniform) a held item: nothing at all, thr[b] keeps its value
  quant_item<SRC>(q, solver_coef(q.coef + (size_t)row * q.ncoef), blockIdx.x, thr);
}
// The same under a per-item x0 correction (common.h ItemCorrect): only an active item in mode 1 needs a threshold, at its OWN ratio (q.p is not
// read); the workgroup of every other item returns at once and leaves thr[b] alone.
template <int SRC>
__global__ __launch_bounds__(1024) void abs_quantile_mixed_kernel(QuantArgs q, float* __restrict__ thr, const SolverItem* __restrict__ items,
                                                                  const ItemCorrect* __restrict__ cr) {
  static_assert(SRC == 1 || SRC == 2, "ready values have no table row");
  bool active;
  const int row = solver_item_row(items[blockIdx.x], *q.step_ptr, active);
  const ItemCorrect c = cr[blockIdx.x];
  if (!active || c.mode != 1) return;          // (block-uniform) held, uncorrected or clamped: nothing at all, thr[b] keeps its value
  q.p = c.ratio;
  quant_item<SRC>(q, solver_coef(q.coef + (size_t)row * q.ncoef), blockIdx.x, thr);
}
// the normals of ns2vc_k_noise: one thread per (row, channel quad), the same philox_gauss4 the update adds
__global__ __launch_bounds__(256) void noise_kernel(const unsigned long long* __restrict__ seeds, int B, int nc, int T, int ld, int step,
                                                    const int* __restrict__ lens, float* __restrict__ out) {
  const int nq = ld >> 2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)B * T * nq) return;
  const size_t r = i / nq;
  const int c = (int)(i - r * nq) * 4, b = (int)(r / T), t = (int)(r - (size_t)b * T);
  float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < nc && (!lens || t < lens[b])) {
    z = philox_gauss4(seeds[b], (uint32_t)t, (uint32_t)(c >> 2), (uint32_t)step);
    if (c + 1 >= nc) z.y = 0.f;
    if (c + 2 >= nc) z.z = 0.f;
    if (c + 3 >= nc) z.w = 0.f;
  }
  reinterpret_cast<float4*>(out)[i] = z;
}
__global__ void fill_i32_kernel(int* p, int v) { if (threadIdx.x == 0 && blockIdx.x == 0) *p = v; }
// read-and-reset of a device maximum (LayerNorm health, ns2vc_unet_ln_ratio*): stream-ordered with the launches that raise it
__global__ void snapshot_u32_kernel(unsigned* src, unsigned* dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = atomicExch(src, 0u); }

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_gn_partial(const float* a0, int lda0, int c0, const float* a1, int lda1, int c1, int B, int T, int G,
                             double* partial, int nchunk, int rows_per_chunk, hipStream_t s) {
  const int C = c0 + c1;
  if (C > 1024 || (C & 3) || (c0 & 3) || G > 8 || C % G || (C / G) % 4 || (C / G) > 128) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gn_partial_kernel, dim3(nchunk, B), dim3(256), 0, s, a0, lda0, c0, a1, lda1, c1, T, G, partial, rows_per_chunk);
  return hipGetLastError();
}
// precision dispatch of a templated kernel launch: TMX is bound to the operand storage type
#define NS2VC_BY_PREC(prec, ...)                                              \
  switch (prec) {                                                             \
    case PREC_BF16: { using TMX = bf16_t; __VA_ARGS__; break; }               \
    case PREC_F16: { using TMX = f16_t; __VA_ARGS__; break; }                 \
    case PREC_F32: { using TMX = float; __VA_ARGS__; break; }                 \
    default: return hipErrorInvalidValue;                                     \
  }

hipError_t launch_gn_apply(const float* a0, int lda0, int c0, const float* a1, int lda1, int c1, int B, int T, int G, float eps,
                           const double* partial, int nchunk, const long long* st0, const long long* st1, const float* gamma,
                           const float* beta, const float* temb, int ldtemb, int temb_off, int silu, void* out_op, void* raw_op,
                           int prec, hipStream_t s, int pair, const int* lens) {
  const int C = c0 + c1;
  if (C > 1024 || (C & 3) || (c0 & 3) || G > 8 || (pair && prec == PREC_F32)) return hipErrorInvalidValue;
  if (st0 && (((C / G) & 15) || (c0 & 15) || (c1 && !st1))) return hipErrorInvalidValue;
  // rows per block: at least one full batch of loads per thread (4 * rl), at most 32, sized so that the grid has >= ~1500
  // blocks -- at the coarse levels (T = 118 / 235) 32-row blocks left most of the chip without a wave to hide latency
  const int rl = 256 / (C >> 2) > 0 ? 256 / (C >> 2) : 1;
  int rows = 32;
  while (rows > 4 * rl && (long)((T + rows - 1) / rows) * B < 1500) rows >>= 1;
  if (rows < 4 * rl) rows = 4 * rl;
  dim3 grid((T + rows - 1) / rows, B);
  if (lens) {
    NS2VC_BY_PREC(prec, hipLaunchKernelGGL((gn_apply_kernel<TMX, true>), grid, dim3(256), 0, s, a0, lda0, c0, a1, lda1, c1, T, G, eps, partial, nchunk,
                                           st0, st1, gamma, beta, temb, ldtemb, temb_off, silu, (TMX*)out_op, (TMX*)raw_op, rows, pair, lens));
  } else {
    NS2VC_BY_PREC(prec, hipLaunchKernelGGL((gn_apply_kernel<TMX, false>), grid, dim3(256), 0, s, a0, lda0, c0, a1, lda1, c1, T, G, eps, partial, nchunk,
                                           st0, st1, gamma, beta, temb, ldtemb, temb_off, silu, (TMX*)out_op, (TMX*)raw_op, rows, pair, lens));
  }
  return hipGetLastError();
}
template <typename TM> static hipError_t launch_ln_t(const float* x, int ldx, int M, int C, float eps, TM* out, hipStream_t s) {
  dim3 grid((M + 15) / 16);
  switch (C / 128) {
    case 1: hipLaunchKernelGGL((ln_apply_op_kernel<TM, 1>), grid, dim3(256), 0, s, x, ldx, M, C, eps, out); break;
    case 2: hipLaunchKernelGGL((ln_apply_op_kernel<TM, 2>), grid, dim3(256), 0, s, x, ldx, M, C, eps, out); break;
    case 3: hipLaunchKernelGGL((ln_apply_op_kernel<TM, 3>), grid, dim3(256), 0, s, x, ldx, M, C, eps, out); break;
    case 4: hipLaunchKernelGGL((ln_apply_op_kernel<TM, 4>), grid, dim3(256), 0, s, x, ldx, M, C, eps, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}
hipError_t launch_ln_apply_op(const float* x, int ldx, int M, int C, float eps, void* out_op, int prec, hipStream_t s) {
  if (C % 128 || C > 512) return hipErrorInvalidValue;
  NS2VC_BY_PREC(prec, return launch_ln_t<TMX>(x, ldx, M, C, eps, (TMX*)out_op, s));
  return hipSuccess;
}
hipError_t launch_cast_op(const float* x, size_t n, void* out_op, int prec, hipStream_t s, int split) {
  if ((n & 3) || (split && (prec == PREC_F32 || (split & 3) || n % (size_t)split))) return hipErrorInvalidValue;
  const size_t n4 = n >> 2;
  const int blocks = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
  NS2VC_BY_PREC(prec, hipLaunchKernelGGL(cast_op_kernel<TMX>, dim3(blocks), dim3(256), 0, s, x, n4, (TMX*)out_op, split));
  return hipGetLastError();
}
hipError_t launch_ln_apply(const float* x, int M, int C, float eps, const float* gamma, const float* beta, float* out, int L,
                           int, hipStream_t s) {
  if (C % 64 || C > 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ln_apply_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, M, C, eps, gamma, beta, out, L);
  return hipGetLastError();
}
hipError_t launch_pool_cls(float* seq, int B, int L, int C, const float* pos, hipStream_t s, const int* plens) {
  if (plens) hipLaunchKernelGGL(pool_cls_lens_kernel, dim3(B, (C + 63) / 64), dim3(256), 0, s, seq, L, C, pos, plens);
  else hipLaunchKernelGGL(pool_cls_kernel, dim3(B, (C + 63) / 64), dim3(256), 0, s, seq, L, C, pos);
  return hipGetLastError();
}
hipError_t launch_pool_attn(const float* qkv, int B, int L1, int C, int heads, float* pooled, hipStream_t s, const int* plens) {
  if (C % heads || C / heads > 8 || (plens && L1 < 2)) return hipErrorInvalidValue;
  const size_t lds = 4 * (size_t)L1 * sizeof(float);
  if (plens) hipLaunchKernelGGL(pool_attn_lens_kernel, dim3(B, (heads + 3) / 4), dim3(256), lds, s, qkv, L1, C, heads, pooled, plens);
  else hipLaunchKernelGGL(pool_attn_kernel, dim3(B, (heads + 3) / 4), dim3(256), lds, s, qkv, L1, C, heads, pooled);
  return hipGetLastError();
}
hipError_t launch_pool_proj(const float* pooled, int B, int C, const float* wt, const float* b, int E, const float* gamma,
                            const float* beta, float eps, float* out, hipStream_t s) {
  hipLaunchKernelGGL(pool_proj_kernel, dim3(B), dim3(256), (size_t)(C + E + 8) * sizeof(float), s, pooled, C, wt, b, E, gamma, beta, eps, out);
  return hipGetLastError();
}
hipError_t launch_time_embed(const float* t_ptr, int t_stride, const int* step_ptr, int coef_stride, const float* w1t,
                             const float* b1, const float* w2t, const float* b2, const float* aug, float* emb, void* emb_act_op,
                             int prec, int B, int tdim, int edim, hipStream_t s) {
  const size_t lds = (size_t)(tdim + edim + 256) * sizeof(float);
  if ((edim & 63) || (tdim & 3) || (edim & 15)) return hipErrorInvalidValue;
  NS2VC_BY_PREC(prec, hipLaunchKernelGGL(time_embed_kernel<TMX>, dim3(B, edim / 64), dim3(256), lds, s, t_ptr, t_stride, step_ptr, coef_stride,
                                         w1t, b1, w2t, b2, aug, emb, (TMX*)emb_act_op, tdim, edim));
  return hipGetLastError();
}
// ---------------------------------------------------------------------------
// Test tool: leave a bit pattern in the LDS of every CU (and in a slab of vector registers of the waves that ran),
// as a foreign kernel (rocBLAS, MIOpen, flash attention ...) scheduled before ours would.  The GPU clears neither
// between kernels, so a kernel that reads LDS / registers it has not written gives results that depend on whatever ran
// before it; the parity tests run with this poison in front of the launches under test.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void poison_kernel(unsigned pattern, int lds_words, unsigned* __restrict__ sink) {
  extern __shared__ unsigned s_poison[];
  for (int i = threadIdx.x; i < lds_words; i += 256) s_poison[i] = pattern;
  __syncthreads();
  // hold the CU for a while so that the grid spreads over all CUs instead of cycling through a few
  unsigned acc = 0;
  for (int rep = 0; rep < 64; ++rep)
    for (int i = threadIdx.x; i < lds_words; i += 256 * 64) acc += s_poison[(i + rep) % lds_words];
  unsigned v[96];
#pragma unroll
  for (int i = 0; i < 96; ++i) { v[i] = pattern; asm volatile("" : "+v"(v[i])); }
  unsigned fold = 0;
#pragma unroll
  for (int i = 0; i < 96; ++i) fold ^= v[i];
  if (acc == 0x12345u && fold == 0x54321u) sink[0] = acc;      // never true for the patterns used; keeps everything live
}
hipError_t launch_poison(unsigned pattern, int lds_bytes, unsigned* sink, hipStream_t s) {
  static bool attr = false;
  if (!attr) {
    hipError_t e = hipFuncSetAttribute((const void*)poison_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    attr = true;
  }
  hipLaunchKernelGGL(poison_kernel, dim3(2048), dim3(256), (size_t)lds_bytes, s, pattern, lds_bytes / 4, sink);
  return hipGetLastError();
}
hipError_t launch_emb_from_table(const float* table, const int* step_ptr, const float* aug, float* emb, void* emb_act_op, int prec, int B,
                                 int edim, hipStream_t s) {
  const int n = B * edim;
  NS2VC_BY_PREC(prec, hipLaunchKernelGGL(emb_from_table_kernel<TMX>, dim3((n + 255) / 256), dim3(256), 0, s, table, step_ptr, aug, emb,
                                         (TMX*)emb_act_op, edim, n));
  return hipGetLastError();
}
hipError_t launch_nct_to_btc(const float* src, int C, int T, int B, float* dst_f32, void* dst_op, int prec, int ldd, int cpad, hipStream_t s, int ldd_op, int split) {
  dim3 grid((T + 31) / 32, (cpad + 31) / 32, B);
  if (ldd_op <= 0) ldd_op = ldd;
  if (split && (prec == PREC_F32 || split < cpad || ldd_op < split + cpad)) return hipErrorInvalidValue;
  NS2VC_BY_PREC(prec, hipLaunchKernelGGL(nct_to_btc_kernel<TMX>, grid, dim3(256), 0, s, src, C, T, dst_f32, (TMX*)dst_op, ldd, cpad, ldd_op, split));
  return hipGetLastError();
}
hipError_t launch_btc_to_nct(const float* src, int lds_, int C, int T, int B, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(btc_to_nct_kernel, dim3((T + 31) / 32, (C + 31) / 32, B), dim3(256), 0, s, src, lds_, C, T, dst);
  return hipGetLastError();
}
hipError_t launch_mask_bias(const uint8_t* mask, int n, float* bias, hipStream_t s) {
  hipLaunchKernelGGL(mask_bias_kernel, dim3((n + 255) / 256), dim3(256), 0, s, mask, n, bias);
  return hipGetLastError();
}
hipError_t launch_prompt_bias(const uint8_t* mask, const int* plens, int B, int Lp, float* bias, hipStream_t s) {
  if (!plens || !bias || B <= 0 || Lp <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(prompt_bias_kernel, dim3((B * Lp + 255) / 256), dim3(256), 0, s, mask, plens, B, Lp, bias);
  return hipGetLastError();
}
// run-time flags -> template arguments of a launch: f gets std::true_type / std::false_type, or std::integral_constant<int, v> for v in LO .. HI
// (the caller has checked the range), and names the kernel once with decltype(flag)::value; its hipError_t comes back
template <typename F> static hipError_t with_flag(bool v, F&& f) { return v ? f(std::true_type{}) : f(std::false_type{}); }
template <int LO, int HI, typename F> static hipError_t with_int(int v, F&& f) {
  if constexpr (LO < HI) { if (v != LO) return with_int<LO + 1, HI>(v, f); }
  return f(std::integral_constant<int, LO>{});
}
hipError_t launch_abs_quantile(const QuantArgs& q, int n_items, float* thr, hipStream_t s, const SolverItem* items, const ItemCorrect* item_correct) {
  const bool formed = q.xe != nullptr;
  if (!q.v || !thr || n_items <= 0 || q.T <= 0 || q.ld <= 0 || (q.ld & 3) || q.nc <= 0 || q.nc > q.ld || (size_t)q.T * (size_t)q.ld > 0x7FFFFFFFull ||
      (((uintptr_t)q.v | (uintptr_t)q.xe) & 15) || (!item_correct && !(q.p >= 0.f && q.p <= 1.f)))
    return hipErrorInvalidValue;
  if (formed && (!q.coef || !q.step_ptr || q.ncoef < 9)) return hipErrorInvalidValue;
  if (q.scale && (!formed || q.half == 0 || (q.half & 3))) return hipErrorInvalidValue;
  if ((items && !formed) || (item_correct && !items)) return hipErrorInvalidValue;      // (ready values have no table row; records go with rows)
  if (!items)
    return with_int<0, 2>(q.scale ? 2 : (formed ? 1 : 0), [&](auto src) {
      hipLaunchKernelGGL(abs_quantile_kernel<decltype(src)::value>, dim3(n_items), dim3(1024), 0, s, q, thr);
      return hipGetLastError();
    });
  return with_int<1, 2>(q.scale ? 2 : 1, [&](auto src) {
    if (item_correct) hipLaunchKernelGGL(abs_quantile_mixed_kernel<decltype(src)::value>, dim3(n_items), dim3(1024), 0, s, q, thr, items, item_correct);
    else hipLaunchKernelGGL(abs_quantile_items_kernel<decltype(src)::value>, dim3(n_items), dim3(1024), 0, s, q, thr, items);
    return hipGetLastError();
  });
}
hipError_t launch_solver_step(const SolverStep& st, hipStream_t s) {
  const size_t n = st.n;
  const int T = st.T, ld = st.ld, mode = st.mode;
  if (!st.coef || !st.step_ptr || st.ncoef < 12 || !st.x0 || !st.xe || !st.xe_op || !st.xbar || !st.d1 || !st.mprev) return hipErrorInvalidValue;
  if ((n & 3) || (st.split && (st.prec == PREC_F32 || (st.split & 3) || n % (size_t)st.split))) return hipErrorInvalidValue;
  // a part that asks for a quad's item: whole items of T rows of ld columns, the operand pair split at ld
  if ((st.scale || st.seeds || mode || st.items) && (T <= 0 || ld <= 0 || (ld & 3) || n == 0 || n % ((size_t)T * ld) || (st.split && st.split != ld)))
    return hipErrorInvalidValue;
  if (st.seeds && (st.nc > ld || mode || (!st.items && st.mprev2))) return hipErrorInvalidValue;
  if (mode && (mode < 0 || mode > 2 || st.item_correct || (mode == 1 && !st.thr) || !(st.max_val > 0.f) || !std::isfinite(st.max_val)))
    return hipErrorInvalidValue;
  if (st.items && n != (size_t)st.n_items * T * ld) return hipErrorInvalidValue;      // (records for every item of the launch)
  if (st.item_correct && (!st.items || !st.thr)) return hipErrorInvalidValue;
  // the kernels' arguments, from the one geometry; a part that is off keeps its empty struct
  SolverNoise nz;
  if (st.seeds) { nz.seeds = st.seeds; nz.lens = st.lens; nz.T = T; nz.ld = ld; nz.nc = st.nc; }
  SolverGuide gd;
  if (st.scale) { gd.scale = st.scale; gd.T = T; gd.ld = ld; }
  SolverCorrect cx;
  if (mode) { cx.mode = mode; cx.max_val = st.max_val; cx.T = T; cx.ld = ld; cx.thr = mode == 1 ? st.thr : nullptr; }
  SolverItems si;
  si.rec = st.items; si.T = T; si.ld = ld;
  if (st.item_correct ? st.quant : mode == 1) {      // the item's |m| quantile over its valid frames and real channels, from the update's own operands
    QuantArgs q;
    q.v = st.x0; q.xe = st.xe; q.coef = st.coef; q.step_ptr = st.step_ptr; q.ncoef = st.ncoef; q.scale = st.scale; q.half = st.scale ? n : 0;
    q.lens = st.lens; q.T = T; q.ld = ld; q.nc = st.nc;
    if (!st.item_correct) q.p = st.ratio;
    const hipError_t e = launch_abs_quantile(q, st.items ? st.n_items : (int)(n / ((size_t)T * ld)), st.thr, s, st.items, st.item_correct);
    if (e != hipSuccess) return e;
  }
  const size_t n4 = n >> 2;
  const dim3 grid((unsigned)((n4 + 255) / 256 < 2048 ? (n4 + 255) / 256 : 2048)), block(256);
  return with_flag(st.scale != nullptr, [&](auto gdf) {
    constexpr bool GD = decltype(gdf)::value;
    if (st.item_correct) {
      NS2VC_BY_PREC(st.prec, hipLaunchKernelGGL((solver_update_mixed_kernel<TMX, GD>), grid, block, 0, s, st.coef, st.step_ptr, st.ncoef, si, st.item_correct,
                                                st.thr, st.x0, st.xe, (TMX*)st.xe_op, st.xbar, st.d1, st.mprev, n4, st.split, nz, st.mprev2, gd));
      return hipGetLastError();
    }
    if (st.items)
      return with_int<0, 2>(mode, [&](auto th) {
        NS2VC_BY_PREC(st.prec, hipLaunchKernelGGL((solver_update_items_kernel<TMX, GD, decltype(th)::value>), grid, block, 0, s, st.coef, st.step_ptr, st.ncoef,
                                                  si, st.x0, st.xe, (TMX*)st.xe_op, st.xbar, st.d1, st.mprev, n4, st.split, nz, st.mprev2, gd, cx));
        return hipGetLastError();
      });
    return with_flag(st.mprev2 != nullptr, [&](auto h2f) {
      constexpr bool H2 = decltype(h2f)::value;
      if (mode)
        return with_int<1, 2>(mode, [&](auto th) {
          NS2VC_BY_PREC(st.prec, hipLaunchKernelGGL((solver_update_th_kernel<TMX, H2, GD, decltype(th)::value>), grid, block, 0, s, st.coef, st.step_ptr,
                                                    st.ncoef, st.x0, st.xe, (TMX*)st.xe_op, st.xbar, st.d1, st.mprev, n4, st.split, st.mprev2, gd, cx));
          return hipGetLastError();
        });
      NS2VC_BY_PREC(st.prec, hipLaunchKernelGGL((solver_update_kernel<TMX, H2, GD>), grid, block, 0, s, st.coef, st.step_ptr, st.ncoef, st.x0, st.xe,
                                                (TMX*)st.xe_op, st.xbar, st.d1, st.mprev, n4, st.split, nz, st.mprev2, gd));
      return hipGetLastError();
    });
  });
}
hipError_t launch_emb_items_from_table(const float* table, const int* step_ptr, const SolverItem* items, int n_items, const float* aug, float* emb,
                                       void* emb_act_op, int prec, int B, int edim, hipStream_t s) {
  if (!items || n_items <= 0 || B % n_items) return hipErrorInvalidValue;
  const int n = B * edim;
  NS2VC_BY_PREC(prec, hipLaunchKernelGGL(emb_items_from_table_kernel<TMX>, dim3((n + 255) / 256), dim3(256), 0, s, table, step_ptr, items, n_items, aug,
                                         emb, (TMX*)emb_act_op, edim, n));
  return hipGetLastError();
}
hipError_t launch_noise(const unsigned long long* seeds, int B, int nc, int T, int ld, int step, const int* lens, float* out, hipStream_t s) {
  if (!seeds || !out || B <= 0 || T <= 0 || ld <= 0 || (ld & 3) || nc < 0 || nc > ld || step < 0) return hipErrorInvalidValue;
  const size_t nth = (size_t)B * T * (ld >> 2);
  hipLaunchKernelGGL(noise_kernel, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, s, seeds, B, nc, T, ld, step, lens, out);
  return hipGetLastError();
}
// Plain kernels for clearing / copying workspace buffers.  The step loop is replayed from a captured hipGraph; memset /
// memcpy NODES in that graph (what hipMemsetAsync / hipMemcpyAsync become under capture) were seen to make replays of the
// 32 x 938 plan return garbage depending on what ran before (tools/order_probe.py), kernel nodes never -- so everything
// inside and next to the captured loop is a kernel.
// `counter` (optional): the sampling loop's step counter, advanced by the FIRST launch of every step (nobody else is running
// then: every other launch of the step only reads it) -- one launch less than a separate one-thread kernel at the step's end
__global__ __launch_bounds__(256) void zero_kernel(uint4* __restrict__ p, size_t n16, unsigned char* __restrict__ tail, int ntail,
                                                   int* __restrict__ counter) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0 && (int)threadIdx.x < ntail) tail[threadIdx.x] = 0;
  if (counter && blockIdx.x == 0 && threadIdx.x == 0) *counter += 1;
}
__global__ __launch_bounds__(256) void copy_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
// Per-item valid lengths (ns2vc_unet_set_lengths): rows t >= lens[b] of item b of a [B*T] row tensor become exact zeros, so that every
// convolution halo, GroupNorm sum and attention key past an item's end reads what an unpadded run of that item reads.  One wave per
// row, 16-byte stores.  With `src` set the kernel instead COPIES row (b, t) from src row (b, t >> up) -- the nearest upsampling
// (upsamplers.0, resnet.py Upsample1D) materialised with its padded rows zeroed: the fused stride-1/2 upsampling conv would read
// source row L >> 1 (a valid row for odd L) as the halo of output row L - 1.
__global__ __launch_bounds__(256) void mask_rows_kernel(uint4* __restrict__ dst, size_t ldd16, const uint4* __restrict__ src, size_t lds16, int row16,
                                                        int B, int T, int Tsrc, int up, const int* __restrict__ lens) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= B * T) return;
  const int b = row / T, t = row - b * T;
  const bool valid = t < lens[b];
  if (valid && !src) return;
  uint4* d = dst + (size_t)row * ldd16;
  if (valid) {
    const uint4* sp = src + ((size_t)b * Tsrc + (t >> up)) * lds16;
    for (int i = lane; i < row16; i += 64) d[i] = sp[i];
  } else {
    for (int i = lane; i < row16; i += 64) d[i] = make_uint4(0u, 0u, 0u, 0u);
  }
}
hipError_t launch_mask_rows(void* dst, size_t ldd_bytes, size_t row_bytes, int B, int T, const int* lens, hipStream_t s, const void* src,
                            size_t lds_bytes, int Tsrc, int up) {
  if (!dst || !lens || B <= 0 || T <= 0 || ((uintptr_t)dst & 15) || (ldd_bytes & 15) || (row_bytes & 15) || row_bytes > ldd_bytes) return hipErrorInvalidValue;
  if (src && (((uintptr_t)src & 15) || (lds_bytes & 15) || row_bytes > lds_bytes || Tsrc <= 0 || up < 0 || up > 1 || ((T - 1) >> up) >= Tsrc)) return hipErrorInvalidValue;
  const int rows = B * T;
  hipLaunchKernelGGL(mask_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, (uint4*)dst, ldd_bytes / 16, (const uint4*)src, lds_bytes / 16,
                     (int)(row_bytes / 16), B, T, Tsrc, up, lens);
  return hipGetLastError();
}
hipError_t launch_zero(void* p, size_t bytes, hipStream_t s, int* counter) {
  if (((uintptr_t)p & 15) != 0) return hipErrorInvalidValue;
  const size_t n16 = bytes / 16;
  const int blocks = (int)std::min<size_t>(2048, std::max<size_t>(1, (n16 + 255) / 256));
  hipLaunchKernelGGL(zero_kernel, dim3(blocks), dim3(256), 0, s, (uint4*)p, n16, (unsigned char*)p + n16 * 16, (int)(bytes & 15), counter);
  return hipGetLastError();
}
hipError_t launch_copy16(const void* src, void* dst, size_t bytes, hipStream_t s) {
  if ((((uintptr_t)src | (uintptr_t)dst) & 15) != 0 || (bytes & 15) != 0) return hipErrorInvalidValue;
  const size_t n16 = bytes / 16;
  const int blocks = (int)std::min<size_t>(2048, std::max<size_t>(1, (n16 + 255) / 256));
  hipLaunchKernelGGL(copy_kernel, dim3(blocks), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, n16);
  return hipGetLastError();
}
// ---------------------------------------------------------------------------
// Placement probe.  The cooperative GroupNorm prologue (gemm.hip, GemmArgs.gnp_sync) lets workgroups whose ids differ by a multiple
// of 8 exchange rows through "the L2 they share": that is the dispatcher's round robin over the XCDs (workgroup id i -> XCD i mod
// #XCDs; one XCD per partition in CPX mode), and it is a matter of CORRECTNESS there, not only of speed as for the tile orders.  So it
// is checked once per device: every workgroup of a 2048-block launch reports HW_REG_XCC_ID, and ids 8 apart must agree.
// ---------------------------------------------------------------------------
__global__ void xcc_probe_kernel(unsigned* out) {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  if (threadIdx.x == 0) out[blockIdx.x] = v & 15u;
}
int probe_xcd_round_robin(unsigned* map8) {   // 1 = ids 8 apart share an XCD, 0 = they do not, -1 = the probe could not run; map8[i] = XCC id of ids = i mod 8
  constexpr int N = 2048;
  unsigned* d = nullptr;
  if (hipMalloc((void**)&d, N * sizeof(unsigned)) != hipSuccess) return -1;
  int ok = -1;
  std::vector<unsigned> h(N, 0xFFu);
  if (hipMemset(d, 0xFF, N * sizeof(unsigned)) == hipSuccess) {
    hipLaunchKernelGGL(xcc_probe_kernel, dim3(N), dim3(64), 0, 0, d);
    if (hipGetLastError() == hipSuccess && hipMemcpy(h.data(), d, N * sizeof(unsigned), hipMemcpyDeviceToHost) == hipSuccess) {
      ok = 1;
      for (int i = 0; i < N; ++i)
        if (h[i] > 15u || h[i] != h[i & 7]) { ok = 0; break; }
      if (ok == 1 && map8)
        for (int i = 0; i < 8; ++i) map8[i] = h[i];
    }
  }
  (void)hipFree(d);
  return ok;
}

// where the blocks of a launch on `s` run: out[2 i] = XCC id, out[2 i + 1] = HW_REG_HW_ID of block i (CU / SE / SH fields) -- for the CU-mask
// partition experiments (tools/overlap_partition.py) and the placement tests
__global__ void placement_kernel(unsigned* out, int spin) {
  unsigned x, h;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(h));
  for (int i = 0; i < spin; ++i) __builtin_amdgcn_s_sleep(8);        // (keeps the block resident so that the grid spreads over the CUs)
  if (threadIdx.x == 0) { out[2 * blockIdx.x] = x & 15u; out[2 * blockIdx.x + 1] = h; }
}
hipError_t launch_placement(unsigned* dev_out, int n_blocks, int spin, hipStream_t s) {
  hipLaunchKernelGGL(placement_kernel, dim3(n_blocks), dim3(256), 0, s, dev_out, spin);
  return hipGetLastError();
}

hipError_t launch_fill_i32(int* p, int v, hipStream_t s) {
  hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(64), 0, s, p, v);
  return hipGetLastError();
}
hipError_t launch_snapshot_u32(unsigned* src, unsigned* dst, hipStream_t s) {
  hipLaunchKernelGGL(snapshot_u32_kernel, dim3(1), dim3(64), 0, s, src, dst);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Slot loop (ns2vc_sampler_open): the B items of a running loop are filled, run and emptied independently.  Three kernels, each ONE
// launch for a list of slots read from device memory (`slots` [n]; entry k of the caller's tensors goes to / comes from item slots[k]); an entry
// outside [0, nslots) is skipped, never used as an index.  They sit behind everything else in this file: every earlier kernel keeps its code.
// ---------------------------------------------------------------------------
// x_T [n][C][T] -> the solver state of the listed slots, exactly what ns2vc_sampler_begin leaves for those items (nct_to_btc + mask_rows + copy16 +
// zero): xe fp32 rows with the pad channels and the rows t >= lens[slot] zero, xe_op the same values in the operand type (16-bit: the [hi | lo] pair,
// `split` columns apart), xbar = xe, d1 = mprev = mprev2 = 0, and the slot's record.  half > 0 (guided engine of 2 * half items): xe / xe_op also go
// to item slot + half, whose xbar, d1, mprev, mprev2 rows are zero.  Nothing of any other item is touched.
template <typename TM>
__global__ __launch_bounds__(256) void sampler_admit_kernel(const float* __restrict__ src, int C, int T, const int* __restrict__ slots, int nslots,
                                                            const SolverItem* __restrict__ rec_in, SolverItem* __restrict__ rec,
                                                            float* __restrict__ xe, TM* __restrict__ xe_op, float* __restrict__ xbar,
                                                            float* __restrict__ d1, float* __restrict__ mprev, float* __restrict__ mprev2, int ld,
                                                            int split, const int* __restrict__ lens, int half) {
  op_mode_init<TM>();
  __shared__ float tile[32][33];
  const int k = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int slot = slots[k];
  if (slot < 0 || slot >= nslots) return;                    // (uniform per block: in front of the barrier)
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;    // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < C && t < T) ? src[((size_t)k * C + c) * T + t] : 0.f;
  }
  __syncthreads();
  const int L = lens ? lens[slot] : T;
  const int ldo = split ? 2 * split : ld;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (t >= T || c >= ld) continue;
    const float v = t < L ? tile[tx][i] : 0.f;
    const size_t r = (size_t)slot * T + t, e = r * ld + c;
    xe[e] = v; xbar[e] = v; d1[e] = 0.f; mprev[e] = 0.f;
    if (mprev2) mprev2[e] = 0.f;
    TM* q = xe_op + r * ldo + c;
    store_op<TM>(q, v);
    if (split) store_op<TM>(q + split, op_rest<TM>(v));
    if (half > 0) {
      const size_t r2 = (size_t)(slot + half) * T + t, e2 = r2 * ld + c;
      xe[e2] = v; xbar[e2] = 0.f; d1[e2] = 0.f; mprev[e2] = 0.f;
      if (mprev2) mprev2[e2] = 0.f;
      q = xe_op + r2 * ldo + c;
      store_op<TM>(q, v);
      if (split) store_op<TM>(q + split, op_rest<TM>(v));
    }
  }
  if (rec && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) rec[slot] = rec_in[k];
}
// xe of the listed slots -> dst [n][C][T] (btc_to_nct_kernel's rows of those items), and the slots' records -> idle (common.h solver_item_idle)
__global__ __launch_bounds__(256) void sampler_take_kernel(const float* __restrict__ src, int lds_, int C, int T, const int* __restrict__ slots,
                                                           int nslots, float* __restrict__ dst, SolverItem* __restrict__ rec) {
  __shared__ float tile[32][33];
  const int k = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int slot = slots[k];
  if (slot < 0 || slot >= nslots) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    tile[i][tx] = (t < T && c < C) ? src[((size_t)slot * T + t) * lds_ + c] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    if (c < C && t < T) dst[((size_t)k * C + c) * T + t] = tile[tx][i];
  }
  if (rec && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) rec[slot] = solver_item_idle();
}
// The condition of the listed slots: content [n][Cc][T] -> the slot's rows of the content operand copy (and of its fp32 copy, where the engine
// keeps one) as ns2vc_unet_set_content writes them -- channels-last, 16-bit: the [hi | lo] pair, rows t >= lens[slot] zero --, and prompt
// [n][Lp][Cx] (Cx % 4 == 0) -> the slot's rows of the fp32 prompt copy; mask_dst set: mask [n][Lp] (NULL: all ones) -> the slot's keep-mask row.
// Blocks x < ceil(T / 32) transpose a content tile; the blocks behind them (y = 0 only) copy the prompt.
template <typename TM>
__global__ __launch_bounds__(256) void condition_items_kernel(const float* __restrict__ content, int Cc, int T, const float* __restrict__ prompt,
                                                              int Lp, int Cx, const uint8_t* __restrict__ mask, const int* __restrict__ slots,
                                                              int nslots, TM* __restrict__ content_op, int split, float* __restrict__ content_f32,
                                                              const int* __restrict__ lens, float* __restrict__ prompt_dst,
                                                              uint8_t* __restrict__ mask_dst) {
  op_mode_init<TM>();
  __shared__ float tile[32][33];
  const int k = blockIdx.z;
  const int slot = slots[k];
  if (slot < 0 || slot >= nslots) return;
  const int tb = (T + 31) / 32;
  if ((int)blockIdx.x >= tb) {
    if (blockIdx.y != 0) return;
    const int pb = blockIdx.x - tb, npb = gridDim.x - tb;
    const size_t n4 = (size_t)Lp * Cx / 4;
    const float4* ps = reinterpret_cast<const float4*>(prompt + (size_t)k * Lp * Cx);
    float4* pd = reinterpret_cast<float4*>(prompt_dst + (size_t)slot * Lp * Cx);
    for (size_t i = (size_t)pb * 256 + threadIdx.x; i < n4; i += (size_t)npb * 256) pd[i] = ps[i];
    if (mask_dst && pb == 0)
      for (int j = threadIdx.x; j < Lp; j += 256) mask_dst[(size_t)slot * Lp + j] = mask ? mask[(size_t)k * Lp + j] : (uint8_t)1;
    return;
  }
  const int t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < Cc && t < T) ? content[((size_t)k * Cc + c) * T + t] : 0.f;
  }
  __syncthreads();
  const int L = lens ? lens[slot] : T;
  const int ldo = split ? 2 * split : Cc;
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (t >= T || c >= Cc) continue;
    const float v = t < L ? tile[tx][i] : 0.f;
    const size_t r = (size_t)slot * T + t;
    if (content_f32) content_f32[r * Cc + c] = v;
    TM* const q = content_op + r * ldo + c;
    store_op<TM>(q, v);
    if (split) store_op<TM>(q + split, op_rest<TM>(v));
  }
}
hipError_t launch_sampler_admit(const float* x_T, int C, int T, int n, const int* slots, int nslots, const SolverItem* rec_in, SolverItem* rec, float* xe,
                                void* xe_op, int prec, float* xbar, float* d1, float* mprev, float* mprev2, int ld, int split, const int* lens, int half,
                                hipStream_t s) {
  if (!x_T || !slots || !xe || !xe_op || !xbar || !d1 || !mprev || n <= 0 || nslots <= 0 || C <= 0 || C > ld || T <= 0 || ld <= 0 || half < 0 ||
      (rec && !rec_in) || (split && (prec == PREC_F32 || split != ld)))
    return hipErrorInvalidValue;
  const dim3 grid((T + 31) / 32, (ld + 31) / 32, n);
  NS2VC_BY_PREC(prec, hipLaunchKernelGGL(sampler_admit_kernel<TMX>, grid, dim3(256), 0, s, x_T, C, T, slots, nslots, rec_in, rec, xe, (TMX*)xe_op, xbar,
                                         d1, mprev, mprev2, ld, split, lens, half));
  return hipGetLastError();
}
hipError_t launch_sampler_take(const float* xe, int ld, int C, int T, int n, const int* slots, int nslots, float* dst, SolverItem* rec, hipStream_t s) {
  if (!xe || !slots || !dst || n <= 0 || nslots <= 0 || C <= 0 || C > ld || T <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sampler_take_kernel, dim3((T + 31) / 32, (C + 31) / 32, n), dim3(256), 0, s, xe, ld, C, T, slots, nslots, dst, rec);
  return hipGetLastError();
}
hipError_t launch_condition_items(const float* content, int Cc, int T, const float* prompt, int Lp, int Cx, const uint8_t* mask, int n, const int* slots,
                                  int nslots, void* content_op, int prec, int split, float* content_f32, const int* lens, float* prompt_dst,
                                  uint8_t* mask_dst, hipStream_t s) {
  if (!content || !prompt || !slots || !content_op || !prompt_dst || n <= 0 || nslots <= 0 || Cc <= 0 || T <= 0 || Lp <= 0 || Cx <= 0 || (Cx & 3) ||
      (((uintptr_t)prompt | (uintptr_t)prompt_dst) & 15) || (split && (prec == PREC_F32 || split != Cc)))
    return hipErrorInvalidValue;
  const int pblocks = (int)std::min<size_t>(8, std::max<size_t>(1, ((size_t)Lp * Cx / 4 + 255) / 256));
  const dim3 grid((T + 31) / 32 + pblocks, (Cc + 31) / 32, n);
  NS2VC_BY_PREC(prec, hipLaunchKernelGGL(condition_items_kernel<TMX>, grid, dim3(256), 0, s, content, Cc, T, prompt, Lp, Cx, mask, slots, nslots,
                                         (TMX*)content_op, split, content_f32, lens, prompt_dst, mask_dst));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Known frames (ns2vc_sampler_set_known): common.h launch_hold_x0 states the rule.  One thread per channel quad of a held row; fp32 in,
// fp32 out whatever the engine's precision, so it is no template.  A step without held rows costs the launch and one scalar load per workgroup.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hold_x0_kernel(float* __restrict__ x0, const float* __restrict__ known, const int* __restrict__ list, int rows,
                                                      int ld, int nc, int halves) {
  const int nq = ld >> 2;
  const int count = min(max(list[0], 0), rows);
  const size_t total = (size_t)count * nq;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t k = i / nq;
    const int c = (int)(i - k * nq) * 4;
    const int r = list[HOLD_LIST_HEAD + k];
    if (r < 0 || r >= rows) continue;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c < nc) {
      v = *reinterpret_cast<const float4*>(known + (size_t)r * ld + c);
      if (c + 1 >= nc) v.y = 0.f;
      if (c + 2 >= nc) v.z = 0.f;
      if (c + 3 >= nc) v.w = 0.f;
    }
    *reinterpret_cast<float4*>(x0 + (size_t)r * ld + c) = v;
    if (halves == 2) *reinterpret_cast<float4*>(x0 + ((size_t)rows + r) * ld + c) = v;
  }
}
hipError_t launch_hold_x0(float* x0, const float* known, const int* list, int rows, int ld, int nc, int halves, hipStream_t s) {
  if (!x0 || !known || !list || rows <= 0 || ld <= 0 || (ld & 3) || nc <= 0 || nc > ld || (halves != 1 && halves != 2) ||
      (((uintptr_t)x0 | (uintptr_t)known) & 15))
    return hipErrorInvalidValue;
  const size_t nth = (size_t)rows * (ld >> 2);
  const unsigned blocks = (unsigned)std::min<size_t>((nth + 255) / 256, 512);
  hipLaunchKernelGGL(hold_x0_kernel, dim3(blocks), dim3(256), 0, s, x0, known, list, rows, ld, nc, halves);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Known frames of a slot loop (ns2vc_sampler_open_known): common.h launch_hold_slots / launch_known_items state the rules.
// hold_slots_kernel: one wave per 64 consecutive rows b * T + t; a lane reads one mask byte, the ballot is the wave's set of held rows, an empty set
// ends the wave.  Otherwise the wave walks the set bits, min(ld / 4, 64) lanes per row (ld = 128: two rows per pass), one float4 per lane and
// quad.  A row index comes from a bit position alone -- never from memory -- and a bit is set only for a row < rows.  fp32 in and out: no template.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void hold_slots_kernel(float* __restrict__ x0, const float* __restrict__ known, const uint8_t* __restrict__ mask,
                                                         int rows, int ld, int nc, int halves) {
  const int lane = threadIdx.x & 63;
  const size_t base = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
  const size_t mine = base + lane;
  unsigned long long set = __ballot(mine < (size_t)rows && mask[mine] != 0);
  if (!set) return;
  const int nq = ld >> 2;
  const int lpr = min(nq, 64), rpp = 64 / lpr;      // lanes per row, rows per pass
  const int j = lane / lpr, q0 = lane - j * lpr;
  while (set) {
    int bit = -1;
    for (int i = 0; i < rpp && set; ++i) {          // (uniform: `set` is the same in every lane)
      const int f = __ffsll(set) - 1;
      set &= set - 1;
      if (i == j) bit = f;
    }
    if (bit < 0) continue;
    const size_t r = base + bit;
    for (int q = q0; q < nq; q += lpr) {
      const int c = q * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < nc) {
        v = *reinterpret_cast<const float4*>(known + r * ld + c);
        if (c + 1 >= nc) v.y = 0.f;
        if (c + 2 >= nc) v.z = 0.f;
        if (c + 3 >= nc) v.w = 0.f;
      }
      *reinterpret_cast<float4*>(x0 + r * ld + c) = v;
      if (halves == 2) *reinterpret_cast<float4*>(x0 + ((size_t)rows + r) * ld + c) = v;
    }
  }
}
hipError_t launch_hold_slots(float* x0, const float* known, const uint8_t* mask, int rows, int ld, int nc, int halves, hipStream_t s) {
  if (!x0 || !known || !mask || rows <= 0 || ld <= 0 || (ld & 3) || nc <= 0 || nc > ld || (halves != 1 && halves != 2) ||
      (((uintptr_t)x0 | (uintptr_t)known) & 15))
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)(((size_t)rows + 255) / 256);      // four waves of 64 rows
  hipLaunchKernelGGL(hold_slots_kernel, dim3(blocks), dim3(256), 0, s, x0, known, mask, rows, ld, nc, halves);
  return hipGetLastError();
}
// known [n][C][T] -> the listed slots' known rows (channels-last, pad channels zero: sampler_admit_kernel's 32 x 33 tile) and mask [n][T] -> their
// mask bytes (0 | 1), written by the blocks y = 0; known == NULL (the clear form, grid y = 1): the listed slots' mask bytes become zero, nothing else
// is written.  An entry outside [0, nslots) is skipped, never used as an index.
__global__ __launch_bounds__(256) void known_items_kernel(const float* __restrict__ known, const uint8_t* __restrict__ mask, int C, int T,
                                                          const int* __restrict__ slots, int nslots, float* __restrict__ known_rows,
                                                          uint8_t* __restrict__ mask_dst, int ld) {
  __shared__ float tile[32][33];
  const int k = blockIdx.z, t0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const int slot = slots[k];
  if (slot < 0 || slot >= nslots) return;                    // (uniform per block: in front of the barrier)
  if (blockIdx.y == 0 && threadIdx.x < 32 && t0 + (int)threadIdx.x < T) {
    const int t = t0 + threadIdx.x;
    mask_dst[(size_t)slot * T + t] = (known && mask[(size_t)k * T + t]) ? (uint8_t)1 : (uint8_t)0;
  }
  if (!known) return;                                        // (uniform: a launch argument)
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;    // 32 x 8
  for (int i = ty; i < 32; i += 8) {
    const int c = c0 + i, t = t0 + tx;
    tile[i][tx] = (c < C && t < T) ? known[((size_t)k * C + c) * T + t] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int t = t0 + i, c = c0 + tx;
    if (t < T && c < ld) known_rows[((size_t)slot * T + t) * ld + c] = tile[tx][i];
  }
}
hipError_t launch_known_items(const float* known, const uint8_t* mask, int C, int T, int n, const int* slots, int nslots, float* known_rows,
                              uint8_t* mask_dst, int ld, hipStream_t s) {
  if (!slots || !mask_dst || (known != nullptr) != (mask != nullptr) || (known && !known_rows) || n <= 0 || nslots <= 0 || T <= 0 || C <= 0 || ld <= 0 ||
      C > ld)
    return hipErrorInvalidValue;
  const dim3 grid((T + 31) / 32, known ? (ld + 31) / 32 : 1, n);
  hipLaunchKernelGGL(known_items_kernel, grid, dim3(256), 0, s, known, mask, C, T, slots, nslots, known_rows, mask_dst, ld);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Suspend / resume of a slot's request (ns2vc_sampler_suspend / _resume): the solver state of the listed slots as P = 4 planes
// (xe, xbar, d1, mprev) or 5 (+ mprev2, a loop opened with history 2) of T rows of ld fp32 columns each, [n][P][T][ld] in the caller's buffer.  Both
// kernels move float4 quads bit for bit -- pad columns, rows past the length and the sign of a zero included -- one launch per slot list, an entry
// outside [0, nslots) skipped and never used as an index.  They sit behind the slot kernels: every earlier kernel keeps its code.
// ---------------------------------------------------------------------------
// the planes of the listed slots -> dst, and the slots' records -> idle.  Grid (x, plane, k).
__global__ __launch_bounds__(256) void sampler_suspend_kernel(const float4* __restrict__ xe, const float4* __restrict__ xbar, const float4* __restrict__ d1,
                                                              const float4* __restrict__ mprev, const float4* __restrict__ mprev2, int q4,
                                                              const int* __restrict__ slots, int nslots, float4* __restrict__ dst,
                                                              SolverItem* __restrict__ rec) {
  const int k = blockIdx.z, p = blockIdx.y;
  const int slot = slots[k];
  if (slot < 0 || slot >= nslots) return;
  const float4* const plane = p == 0 ? xe : p == 1 ? xbar : p == 2 ? d1 : p == 3 ? mprev : mprev2;
  const float4* const src = plane + (size_t)slot * q4;
  float4* const d = dst + ((size_t)k * gridDim.y + p) * q4;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < q4; i += gridDim.x * 256) d[i] = src[i];
  if (rec && blockIdx.x == 0 && p == 0 && threadIdx.x == 0) rec[slot] = solver_item_idle();
}
// src [n][P][T][ld] -> the listed slots' state: xe with its operand copy as the update writes it (solver_store_xe: 16-bit types the [hi | lo] pair),
// xbar, d1, mprev and (P = 5) mprev2, and the slot's record.  half > 0 (guided engine of 2 * half items): xe / xe_op also go to item slot + half,
// whose xbar, d1, mprev, mprev2 rows become zero, as sampler_admit_kernel leaves them.  Grid (x, k).
template <typename TM>
__global__ __launch_bounds__(256) void sampler_resume_kernel(const float4* __restrict__ src, int q4, const int* __restrict__ slots, int nslots,
                                                             const SolverItem* __restrict__ rec_in, SolverItem* __restrict__ rec,
                                                             float* __restrict__ xe, TM* __restrict__ xe_op, float* __restrict__ xbar,
                                                             float* __restrict__ d1, float* __restrict__ mprev, float* __restrict__ mprev2, int split,
                                                             int half) {
  op_mode_init<TM>();
  const int k = blockIdx.y;
  const int slot = slots[k];
  if (slot < 0 || slot >= nslots) return;
  const size_t P = mprev2 ? 5 : 4;
  const float4* const s = src + (size_t)k * P * q4;
  const size_t base = (size_t)slot * q4, base2 = (size_t)(slot + half) * q4;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < q4; i += gridDim.x * 256) {
    const float4 vxe = s[i], vxb = s[(size_t)q4 + i], vd1 = s[2 * (size_t)q4 + i], vmp = s[3 * (size_t)q4 + i];
    const size_t e = base + i;
    solver_store_xe<TM>(xe, xe_op, e, split, vxe);
    out_f4(xbar + 4 * e, vxb.x, vxb.y, vxb.z, vxb.w);
    out_f4(d1 + 4 * e, vd1.x, vd1.y, vd1.z, vd1.w);
    out_f4(mprev + 4 * e, vmp.x, vmp.y, vmp.z, vmp.w);
    if (mprev2) {
      const float4 vm2 = s[4 * (size_t)q4 + i];
      out_f4(mprev2 + 4 * e, vm2.x, vm2.y, vm2.z, vm2.w);
    }
    if (half > 0) {
      const size_t e2 = base2 + i;
      solver_store_xe<TM>(xe, xe_op, e2, split, vxe);
      out_f4(xbar + 4 * e2, 0.f, 0.f, 0.f, 0.f);
      out_f4(d1 + 4 * e2, 0.f, 0.f, 0.f, 0.f);
      out_f4(mprev + 4 * e2, 0.f, 0.f, 0.f, 0.f);
      if (mprev2) out_f4(mprev2 + 4 * e2, 0.f, 0.f, 0.f, 0.f);
    }
  }
  if (rec && blockIdx.x == 0 && threadIdx.x == 0) rec[slot] = rec_in[k];
}
static bool slot_state_fits(int T, int ld, int n, int nslots) {
  return n > 0 && nslots > 0 && T > 0 && ld > 0 && !(ld & 3) && (size_t)T * ld / 4 <= (size_t)0x7fffffff / 8;
}
hipError_t launch_sampler_suspend(const float* xe, const float* xbar, const float* d1, const float* mprev, const float* mprev2, int T, int ld, int n,
                                  const int* slots, int nslots, float* dst, SolverItem* rec, hipStream_t s) {
  if (!xe || !xbar || !d1 || !mprev || !slots || !dst || !slot_state_fits(T, ld, n, nslots) ||
      (((uintptr_t)xe | (uintptr_t)xbar | (uintptr_t)d1 | (uintptr_t)mprev | (uintptr_t)mprev2 | (uintptr_t)dst) & 15))
    return hipErrorInvalidValue;
  const int q4 = T * ld / 4;
  const dim3 grid((unsigned)std::min(64, (q4 + 255) / 256), mprev2 ? 5 : 4, n);
  hipLaunchKernelGGL(sampler_suspend_kernel, grid, dim3(256), 0, s, (const float4*)xe, (const float4*)xbar, (const float4*)d1, (const float4*)mprev,
                     (const float4*)mprev2, q4, slots, nslots, (float4*)dst, rec);
  return hipGetLastError();
}
hipError_t launch_sampler_resume(const float* src, int T, int ld, int n, const int* slots, int nslots, const SolverItem* rec_in, SolverItem* rec, float* xe,
                                 void* xe_op, int prec, float* xbar, float* d1, float* mprev, float* mprev2, int split, int half, hipStream_t s) {
  if (!src || !slots || !xe || !xe_op || !xbar || !d1 || !mprev || !slot_state_fits(T, ld, n, nslots) || half < 0 || (rec && !rec_in) ||
      (split && (prec == PREC_F32 || split != ld)) ||
      (((uintptr_t)src | (uintptr_t)xe | (uintptr_t)xe_op | (uintptr_t)xbar | (uintptr_t)d1 | (uintptr_t)mprev | (uintptr_t)mprev2) & 15))
    return hipErrorInvalidValue;
  const int q4 = T * ld / 4;
  const dim3 grid((unsigned)std::min(128, (q4 + 255) / 256), n);
  NS2VC_BY_PREC(prec, hipLaunchKernelGGL(sampler_resume_kernel<TMX>, grid, dim3(256), 0, s, (const float4*)src, q4, slots, nslots, rec_in, rec, xe,
                                         (TMX*)xe_op, xbar, d1, mprev, mprev2, split, half));
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The flat solver step (ns2vc_k_solver_step_flat; the device path of the top-level sampler/ package): one table row on n elements of
// the five fp32 state planes xe, xbar, d1, mprev, mprev2, with no layout at all -- no rows, no items, no operand copy -- so the planes may be torch
// tensors of any shape, views and slices included.  It sits behind the suspend / resume kernels: every earlier kernel keeps its code.
//   KIND (compile time): what `out`, the model's output at xe, is.  m, the predicted x0 the recurrence runs on, is
//     0 x_start  solver_m(out, xe): the float32 round trip of the model wrapper, the bits of solver_update_kernel
//     1 noise    (xe - sigma * out) / alpha
//     2 v        eps = alpha * out + sigma * xe, then as noise          (sampler/dpm_solver.py:305-308)
//     3 score    eps = -sigma * out, then as noise                      (sampler/dpm_solver.py:309-311)
//     4 data     out itself (an m that was corrected on the way: FORM, torch, then this)
//   H2: the history-2 form (mprev2 read and rotated), as in solver_quad.
//   FORM: m goes to m_out and NO state plane is read but xe or written at all.
// Behind m the element is common.h solver_elem_m + solver_xe, the functions solver_quad runs.  Alignment: the pointers need 4 bytes only.  The n
// elements are cut into SLOTS of up to four: where all planes of the launch share one 16-byte phase, a head slot of 0..3 elements that brings them
// to a 16-byte boundary, nq full quads loaded and stored as float4, and a tail slot; planes on different phases have no common quad, and every slot
// (ceil(n / 4) of them) is loaded and stored element by element.  ONE loop body serves every slot -- loads (float4 or per element, absent lanes 0),
// the four elements in a straight line, stores (float4 or per element) -- because two bodies did not give the same bits: a scalar loop beside the
// float4 loop was one ulp off on x_e' in some elements (seen on the device; the compiler contracts multiply-adds per body, the comment above
// solver_quad has the same finding), and an element's bits must not depend on the path that handled it.  The loop is grid-stride over size_t slot
// indices.  Seven streams of 4 bytes per element and a dozen flops: bandwidth.
// ---------------------------------------------------------------------------
template <int KIND>
__device__ __forceinline__ float flat_m(const SolverCoef& k, float out, float vxe) {
  static_assert(KIND >= 0 && KIND <= 4, "0 x_start, 1 noise, 2 v, 3 score, 4 data");
  if constexpr (KIND == 0) return solver_m(k, out, vxe);
  if constexpr (KIND == 4) return out;
  float eps = out;
  if constexpr (KIND == 2) eps = k.alpha * out + k.sigma * vxe;
  if constexpr (KIND == 3) eps = -k.sigma * out;
  return (vxe - k.sigma * eps) / k.alpha;
}
template <int KIND, bool H2>
__device__ __forceinline__ void flat_elem(const SolverRow& kr, float out, float vxe, float vxb, float vd1, float vmp, float vm2, float& oxe, float& oxb,
                                          float& od1, float& om) {
  solver_elem_m<H2>(kr.k, kr.d2c, flat_m<KIND>(kr.k, out, vxe), vxb, vd1, vmp, vm2, oxb, od1, om);
  oxe = solver_xe<H2>(kr.k, kr.pe, oxb, od1, om, vm2);
}
// up to four elements from e0 on: one float4 (vec: the slot is full and 16-byte aligned) or cnt single loads, the absent lanes 0
__device__ __forceinline__ float4 flat_load(const float* p, size_t e0, int cnt, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p + e0);
  float4 v = make_float4(p[e0], 0.f, 0.f, 0.f);
  if (cnt > 1) v.y = p[e0 + 1];
  if (cnt > 2) v.z = p[e0 + 2];
  if (cnt > 3) v.w = p[e0 + 3];
  return v;
}
__device__ __forceinline__ void flat_store(float* p, size_t e0, int cnt, bool vec, const float4& v) {
  if (vec) { out_f4(p + e0, v.x, v.y, v.z, v.w); return; }
  p[e0] = v.x;
  if (cnt > 1) p[e0 + 1] = v.y;
  if (cnt > 2) p[e0 + 2] = v.z;
  if (cnt > 3) p[e0 + 3] = v.w;
}
// Slot j of the launch: j < hs = the head slot ([0, head)), then nq quads from `head` on, then the tail slot.  vec: the quads are 16-byte aligned in
// every plane.  (No __restrict__ on the planes: a model may hand back a view of the state it was given; a slot is loaded in full before it is stored.)
template <int KIND, bool H2, bool FORM>
__global__ __launch_bounds__(256) void solver_step_flat_kernel(const float* __restrict__ crow, const float* out, float* xe, float* xbar, float* d1,
                                                               float* mprev, float* mprev2, float* m_out, size_t n, size_t head, size_t nq, int vec) {
  const SolverRow kr = solver_row<H2>(crow, false);
  const size_t hs = head ? 1 : 0, tail0 = head + 4 * nq, nslots = hs + nq + (tail0 < n ? 1 : 0);
  for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < nslots; j += (size_t)gridDim.x * 256) {
    size_t e0 = head + 4 * (j - hs);
    int cnt = 4;
    bool v4 = vec != 0;
    if (j < hs) { e0 = 0; cnt = (int)head; v4 = false; }
    else if (j >= hs + nq) { e0 = tail0; cnt = (int)(n - tail0); v4 = false; }
    const float4 vo = flat_load(out, e0, cnt, v4);
    float4 vxe = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (KIND != 4 || !FORM) vxe = flat_load(xe, e0, cnt, v4);
    if constexpr (FORM) {
      flat_store(m_out, e0, cnt, v4, make_float4(flat_m<KIND>(kr.k, vo.x, vxe.x), flat_m<KIND>(kr.k, vo.y, vxe.y), flat_m<KIND>(kr.k, vo.z, vxe.z),
                                                 flat_m<KIND>(kr.k, vo.w, vxe.w)));
    } else {
      const float4 vxb = flat_load(xbar, e0, cnt, v4), vd1 = flat_load(d1, e0, cnt, v4), vmp = flat_load(mprev, e0, cnt, v4);
      float4 vm2 = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (H2) vm2 = flat_load(mprev2, e0, cnt, v4);
      float4 oxe, oxb, od1, om;
      flat_elem<KIND, H2>(kr, vo.x, vxe.x, vxb.x, vd1.x, vmp.x, vm2.x, oxe.x, oxb.x, od1.x, om.x);
      flat_elem<KIND, H2>(kr, vo.y, vxe.y, vxb.y, vd1.y, vmp.y, vm2.y, oxe.y, oxb.y, od1.y, om.y);
      flat_elem<KIND, H2>(kr, vo.z, vxe.z, vxb.z, vd1.z, vmp.z, vm2.z, oxe.z, oxb.z, od1.z, om.z);
      flat_elem<KIND, H2>(kr, vo.w, vxe.w, vxb.w, vd1.w, vmp.w, vm2.w, oxe.w, oxb.w, od1.w, om.w);
      if constexpr (H2) flat_store(mprev2, e0, cnt, v4, vmp);
      flat_store(xe, e0, cnt, v4, oxe);
      flat_store(xbar, e0, cnt, v4, oxb);
      flat_store(d1, e0, cnt, v4, od1);
      flat_store(mprev, e0, cnt, v4, om);
    }
  }
}
template <int KIND>
static void launch_flat_kind(dim3 grid, hipStream_t s, const float* crow, const float* out, float* xe, float* xbar, float* d1, float* mprev, float* mprev2,
                             float* m_out, size_t n, size_t head, size_t nq, int vec) {
  if (m_out)
    hipLaunchKernelGGL((solver_step_flat_kernel<KIND, false, true>), grid, dim3(256), 0, s, crow, out, xe, xbar, d1, mprev, mprev2, m_out, n, head, nq, vec);
  else if (mprev2)
    hipLaunchKernelGGL((solver_step_flat_kernel<KIND, true, false>), grid, dim3(256), 0, s, crow, out, xe, xbar, d1, mprev, mprev2, m_out, n, head, nq, vec);
  else
    hipLaunchKernelGGL((solver_step_flat_kernel<KIND, false, false>), grid, dim3(256), 0, s, crow, out, xe, xbar, d1, mprev, mprev2, m_out, n, head, nq, vec);
}
hipError_t launch_solver_step_flat(const float* crow, int kind, const float* out, float* xe, float* xbar, float* d1, float* mprev, float* mprev2,
                                   float* m_out, size_t n, hipStream_t s) {
  if (!crow || !out || !xe || !xbar || !d1 || !mprev || n == 0 || kind < 0 || kind > 4) return hipErrorInvalidValue;
  // the planes this launch touches: FORM reads out (and xe, unless m is out itself) and writes m_out alone
  const uintptr_t form[3] = {(uintptr_t)out, (uintptr_t)m_out, kind == 4 ? (uintptr_t)out : (uintptr_t)xe};
  const uintptr_t upd[6] = {(uintptr_t)out, (uintptr_t)xe, (uintptr_t)xbar, (uintptr_t)d1, (uintptr_t)mprev, mprev2 ? (uintptr_t)mprev2 : (uintptr_t)out};
  const uintptr_t* const p = m_out ? form : upd;
  const int np = m_out ? 3 : 6;
  bool one_phase = true;
  for (int i = 0; i < np; ++i) {
    if (p[i] & 3) return hipErrorInvalidValue;
    one_phase = one_phase && (p[i] & 15) == (p[0] & 15);
  }
  // one phase: a head slot up to the 16-byte boundary, float4 quads, a tail slot; otherwise quads from element 0 on, loaded element by element
  const size_t head = one_phase ? std::min<size_t>(n, ((16 - (p[0] & 15)) & 15) / 4) : 0;
  const size_t nq = (n - head) / 4;
  const int vec = one_phase ? 1 : 0;
  const size_t nslots = (head ? 1 : 0) + nq + (head + 4 * nq < n ? 1 : 0);
  const dim3 grid((unsigned)std::min<size_t>(FLAT_MAX_BLOCKS, (nslots + 255) / 256));
  switch (kind) {
    case 0: launch_flat_kind<0>(grid, s, crow, out, xe, xbar, d1, mprev, mprev2, m_out, n, head, nq, vec); break;
    case 1: launch_flat_kind<1>(grid, s, crow, out, xe, xbar, d1, mprev, mprev2, m_out, n, head, nq, vec); break;
    case 2: launch_flat_kind<2>(grid, s, crow, out, xe, xbar, d1, mprev, mprev2, m_out, n, head, nq, vec); break;
    case 3: launch_flat_kind<3>(grid, s, crow, out, xe, xbar, d1, mprev, mprev2, m_out, n, head, nq, vec); break;
    default: launch_flat_kind<4>(grid, s, crow, out, xe, xbar, d1, mprev, mprev2, m_out, n, head, nq, vec); break;
  }
  return hipGetLastError();
}

}  // namespace ns2vc
