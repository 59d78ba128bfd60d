// Shared device/host definitions for the NS2VC denoiser engine (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../include/ns2vc_hip.h"

namespace ns2vc {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4_t;

// 2-byte storage types of the 16-bit operand precisions (activations / weights as the MFMA reads them)
struct bf16_t { uint16_t v; };
struct f16_t { uint16_t v; };

__host__ __device__ inline uint16_t f32_to_bf16_bits(float f) {
  union { float f; uint32_t u; } x;
  x.f = f;
  uint32_t u = x.u;
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // quiet NaN
  u += 0x7fffu + ((u >> 16) & 1u);                                            // round to nearest even
  return (uint16_t)(u >> 16);
}
__host__ __device__ inline float bf16_bits_to_f32(uint16_t h) {
  union { float f; uint32_t u; } x;
  x.u = (uint32_t)h << 16;
  return x.f;
}

// IEEE binary16, round to nearest even; overflow -> inf, subnormals kept (host side: weight packing, test helpers)
__host__ __device__ inline uint16_t f32_to_f16_bits(float f) {
  union { float f; uint32_t u; } x;
  x.f = f;
  const uint32_t sign = (x.u >> 16) & 0x8000u;
  uint32_t a = x.u & 0x7fffffffu;
  if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);             // NaN
  if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);            // >= 65520 rounds to inf
  if (a < 0x38800000u) {                                              // below the smallest normal (2^-14): subnormal / zero
    if (a < 0x33000000u) return (uint16_t)sign;                       // < 2^-25 -> 0
    const int e = (int)(a >> 23);                                     // biased fp32 exponent, 102..112
    const uint32_t m = (a & 0x7fffffu) | 0x800000u;                   // 24-bit significand
    const int shift = 126 - e;                                        // 14..24: bits dropped
    uint32_t r = m >> shift;
    const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    if (rem > half || (rem == half && (r & 1u))) ++r;
    return (uint16_t)(sign | r);
  }
  a += 0xc8000000u;                                                   // rebias exponent 127 -> 15 (subtract 112 << 23)
  a += 0xfffu + ((a >> 13) & 1u);                                     // round to nearest even on the 13 dropped bits
  return (uint16_t)(sign | (a >> 13));
}
__host__ __device__ inline float f16_bits_to_f32(uint16_t h) {
  union { float f; uint32_t u; } x;
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  if (e == 0) {
    if (m == 0) { x.u = sign; return x.f; }
    x.f = (float)m * 5.9604644775390625e-8f;                          // m * 2^-24
    x.u |= sign;
    return x.f;
  }
  if (e == 31) { x.u = sign | 0x7f800000u | (m << 13); return x.f; }
  x.u = sign | ((e + 112u) << 23) | (m << 13);
  return x.f;
}

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
// hardware round-to-nearest-even pack (v_cvt_pk_bf16_f32): lo -> bits [15:0], hi -> bits [31:16]
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  f32x2_t v = {lo, hi};
  union { bf16x2_t b; uint32_t u; } r;
  r.b = __builtin_convertvector(v, bf16x2_t);
  return r.u;
}
__device__ __forceinline__ float bf16_lo(uint32_t u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(uint32_t u) { return __uint_as_float(u & 0xffff0000u); }
// fp16 (IEEE binary16, round to nearest even; v_cvt_pk_f16_f32 on gfx950).  Overflow: every kernel that produces fp16
// operands starts with op_mode_init<f16_t>(), which sets MODE.FP16_OVFL -- finite values beyond +-65504 then convert to
// +-65504 instead of +-inf (an activation outlier saturates instead of turning whole rows into inf/NaN downstream), while
// +-inf inputs stay inf (the attention mask's -inf for tail keys relies on that).  Checked on MI355X by
// tools/fp16_ovfl_probe.hip; costs nothing per element (an explicit v_med3 clamp cost 1.7 % of the step).
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ uint32_t pack_f16x2(float lo, float hi) {
  f32x2_t v = {lo, hi};
  union { f16x2_t h; uint32_t u; } r;
  r.h = __builtin_convertvector(v, f16x2_t);
  return r.u;
}
__device__ __forceinline__ float f16_lo(uint32_t u) { union { uint32_t u; f16x2_t h; } r; r.u = u; return (float)r.h[0]; }
__device__ __forceinline__ float f16_hi(uint32_t u) { union { uint32_t u; f16x2_t h; } r; r.u = u; return (float)r.h[1]; }

// one interface over the two 16-bit operand types (TM = bf16_t | f16_t): two floats <-> one packed dword
template <typename TM> struct Op16;
template <> struct Op16<bf16_t> {
  __device__ static __forceinline__ uint32_t pack(float lo, float hi) { return pack_bf16x2(lo, hi); }
  __device__ static __forceinline__ float lo(uint32_t u) { return bf16_lo(u); }
  __device__ static __forceinline__ float hi(uint32_t u) { return bf16_hi(u); }
};
template <> struct Op16<f16_t> {
  __device__ static __forceinline__ uint32_t pack(float lo, float hi) { return pack_f16x2(lo, hi); }
  __device__ static __forceinline__ float lo(uint32_t u) { return f16_lo(u); }
  __device__ static __forceinline__ float hi(uint32_t u) { return f16_hi(u); }
};
// per-kernel setup of the operand type: fp16 -> MODE.FP16_OVFL = 1 (hwreg(HW_REG_MODE, offset 23, size 1)), see above
template <typename TM> __device__ __forceinline__ void op_mode_init() {}
template <> __device__ __forceinline__ void op_mode_init<f16_t>() { __builtin_amdgcn_s_setreg(1 | (23 << 6) | (0 << 11), 1); }

// operand-typed scalar / 4-vector stores and loads (TM = float or bf16_t)
template <typename TM> __device__ __forceinline__ void store_op(TM* p, float v);
template <> __device__ __forceinline__ void store_op<float>(float* p, float v) { *p = v; }
template <> __device__ __forceinline__ void store_op<bf16_t>(bf16_t* p, float v) { p->v = (uint16_t)pack_bf16x2(v, 0.f); }
template <> __device__ __forceinline__ void store_op<f16_t>(f16_t* p, float v) { p->v = (uint16_t)pack_f16x2(v, 0.f); }
// Workgroup barrier that orders LDS traffic only.  __syncthreads() carries a workgroup-scope memory fence: once a kernel has
// issued global stores the compiler puts `s_waitcnt vmcnt(0)` in front of the barrier, i.e. every wave sits through the
// write latency of everything stored so far (1-2 us per barrier in the epilogues, found in the ISA).  Where the barrier only
// protects an LDS staging buffer this is all that is needed.
__device__ __forceinline__ void lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}
// what the operand type drops of v: v - float(TM(v)) -- the `lo` plane of a hi + lo operand pair (r6 split_io: conv_in / conv_out with
// x*w ~= hi(x)*hi(w) + lo(x)*hi(w) + hi(x)*lo(w) on the 16-bit MFMA, 2^-22-ish relative instead of 2^-11)
template <typename TM> __device__ __forceinline__ float op_rest(float v) { return v - Op16<TM>::lo(Op16<TM>::pack(v, 0.f)); }
template <> __device__ __forceinline__ float op_rest<float>(float) { return 0.f; }
template <typename TM> __device__ __forceinline__ void store_op4(TM* p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void store_op4<float>(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
template <> __device__ __forceinline__ void store_op4<bf16_t>(bf16_t* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
}
template <> __device__ __forceinline__ void store_op4<f16_t>(f16_t* p, float a, float b, float c, float d) {
  *reinterpret_cast<uint2*>(p) = make_uint2(pack_f16x2(a, b), pack_f16x2(c, d));
}
// Result stores of the big producers (GEMM epilogues, norm outputs).  NS2VC_WT_STORES=1 (default) issues them
// write-through (sc1): the bytes leave during the kernel instead of as an L2 write-back at the kernel boundary
// (every kernel used to leave 8-30 MB dirty).  Same-box A/B: 4.65 -> 4.45 ms/step; the attention output is better
// left to plain stores (+5 % attention time with sc1), so attn.hip does not use these.
#ifndef NS2VC_WT_STORES
#define NS2VC_WT_STORES 1
#endif
#ifndef NS2VC_WT_MODE
#define NS2VC_WT_MODE 1
#endif
#ifndef NS2VC_WT_MOD            // cache-policy bits of those stores; NS2VC_WT_MODE selects one for A/B builds (1 = shipped).  r4, same box, ms/step:
                                // sc1 3.709 | sc1 nt 3.827 | nt 3.808 | sc0 sc1 3.704 (profiles/r04_ab_store_policy.txt)
#if NS2VC_WT_MODE == 2
#define NS2VC_WT_MOD "sc1 nt"
#elif NS2VC_WT_MODE == 3
#define NS2VC_WT_MOD "nt"
#elif NS2VC_WT_MODE == 4
#define NS2VC_WT_MOD "sc0 sc1"
#else
#define NS2VC_WT_MOD "sc1"
#endif
#endif
__device__ __forceinline__ void out_store16(void* p, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
#if NS2VC_WT_STORES
  const u32x4_t v = {a, b, c, d};
  asm volatile("global_store_dwordx4 %0, %1, off " NS2VC_WT_MOD "\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
#else
  *reinterpret_cast<uint4*>(p) = make_uint4(a, b, c, d);
#endif
}
__device__ __forceinline__ void out_store8(void* p, uint32_t a, uint32_t b) {
#if NS2VC_WT_STORES
  typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
  const u32x2_t v = {a, b};
  asm volatile("global_store_dwordx2 %0, %1, off " NS2VC_WT_MOD "\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
#else
  *reinterpret_cast<uint2*>(p) = make_uint2(a, b);
#endif
}
__device__ __forceinline__ void out_f4(float* p, float a, float b, float c, float d) {
  out_store16(p, __float_as_uint(a), __float_as_uint(b), __float_as_uint(c), __float_as_uint(d));
}
template <typename TM> __device__ __forceinline__ void out_op4(TM* p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void out_op4<float>(float* p, float a, float b, float c, float d) { out_f4(p, a, b, c, d); }
template <> __device__ __forceinline__ void out_op4<bf16_t>(bf16_t* p, float a, float b, float c, float d) { out_store8(p, pack_bf16x2(a, b), pack_bf16x2(c, d)); }
template <> __device__ __forceinline__ void out_op4<f16_t>(f16_t* p, float a, float b, float c, float d) { out_store8(p, pack_f16x2(a, b), pack_f16x2(c, d)); }
template <typename TM> __device__ __forceinline__ void store_op2(TM* p, float a, float b);
template <> __device__ __forceinline__ void store_op2<float>(float* p, float a, float b) { *reinterpret_cast<float2*>(p) = make_float2(a, b); }
template <> __device__ __forceinline__ void store_op2<bf16_t>(bf16_t* p, float a, float b) { *reinterpret_cast<uint32_t*>(p) = pack_bf16x2(a, b); }
template <> __device__ __forceinline__ void store_op2<f16_t>(f16_t* p, float a, float b) { *reinterpret_cast<uint32_t*>(p) = pack_f16x2(a, b); }
#endif

__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float silu_f(float v) { return v * fast_rcp(1.0f + __expf(-v)); }
// erf via Abramowitz-Stegun 7.1.26 (|abs err| <= 1.5e-7, branch-free): the exact-GELU of the reference
// (attention.py:295, F.gelu default) to ~1e-7, far inside the 1e-3 parity budget, at ~15 VALU ops.
__device__ __forceinline__ float erf_as(float x) {
  const float ax = fabsf(x);
  const float t = fast_rcp(1.0f + 0.3275911f * ax);
  float p = 1.061405429f;
  p = fmaf(p, t, -1.453152027f);
  p = fmaf(p, t, 1.421413741f);
  p = fmaf(p, t, -0.284496736f);
  p = fmaf(p, t, 0.254829592f);
  const float e = 1.0f - p * t * __expf(-ax * ax);
  return copysignf(e, x);
}
__device__ __forceinline__ float gelu_erf_f(float v) { return 0.5f * v * (1.0f + erf_as(v * 0.70710678118654752440f)); }

// ---------------------------------------------------------------------------
// implicit-GEMM (conv1d k3/k1, linear) arguments
// rows   m = b*Tout + t          (activations, channels-last [B][T][C])
// K idx  k = tap*(c0+c1) + c     (c < c0 -> source 0, else source 1: no-copy concat)
// out[m][n] = epi( sum_k pro(A[m,k]) * W[n][k] )
// ---------------------------------------------------------------------------
enum { TMODE_SAME = 0, TMODE_DOWN2 = 1, TMODE_UP2 = 2 };
enum { PRO_NONE = 0, PRO_BC = 1, PRO_ROW = 2 };

typedef ::ns2vc_gemm_args GemmArgs;   // public POD, include/ns2vc_hip.h
typedef ::ns2vc_attn_args AttnArgs;

enum Precision { PREC_F32 = 0, PREC_BF16 = 1, PREC_F16 = 2 };
inline size_t operand_bytes(int prec) { return prec == PREC_F32 ? 4 : 2; }
// host-side rounding of a value to the operand type (weight packing, row sums of the rounded weights)
inline uint16_t f32_to_op16_bits(float v, int prec) { return prec == PREC_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v); }
inline float op16_bits_to_f32(uint16_t b, int prec) { return prec == PREC_BF16 ? bf16_bits_to_f32(b) : f16_bits_to_f32(b); }
// fixed-point scales of the epilogue GroupNorm statistics (order-independent int64 atomics => deterministic)
// One element of the fused solver update (ns2vc_amd/schedule.py documents the recurrence; sampler/dpm_solver.py:433-442, 547-580, sampler/uni_pc.py:471-588):
// the x0 -> eps -> x0 round trip of the reference's model wrapper, literally (solver_m; the quantile kernel forms the same m), then the unified
// multistep update.  ONE definition, solver_elem, used by the update kernels (misc.hip solver_quad) and, as solver_upd, by the conv_out epilogue of
// conv3ts_kernel (convts.hip): all forms give the same bits.
//   H2 (compile time): the second history term of order-3 rows (columns 10-11 of the table: d2c, pe; vmp2 = m_{i-2}).  Only tables with a nonzero
//     column 10 or 11 run it; every other table keeps the arithmetic of H2 = false (d2c, pe, vmp2 unused).
//   TH (compile time): the reference's correction of the predicted x0 (correcting_x0_fn: sampler/dpm_solver.py:416-425, :433-442,
//     sampler/uni_pc.py:268-294), applied to m in front of everything that uses it.  0 = none (s unused); 1 = dynamic thresholding,
//     clamp(m, -s, s) / s with s = max(the item's |m| quantile, max_val); 2 = the static clamp(m, -s, s), s = max_val.
//     ns2vc_amd.schedule.correct_x0 is the host statement.
struct SolverCoef { float alpha, sigma, g0, g1, A, Bc, d1c, pc; };
__device__ __forceinline__ SolverCoef solver_coef(const float* __restrict__ c) { return SolverCoef{c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]}; }
__device__ __forceinline__ float solver_m(const SolverCoef& k, float vx0, float vxe) {
  const float eps = (vxe - k.alpha * vx0) / k.sigma;
  return (vxe - k.sigma * eps) / k.alpha;
}
template <int TH> __device__ __forceinline__ float solver_correct(float m, float s) {
  const float c = fminf(fmaxf(m, -s), s);
  return TH == 1 ? c / s : c;
}
// In two steps, because the stochastic samplers add their noise to xbar' in between (misc.hip solver_quad): solver_elem gives the new state
// (xbar', d1', m), solver_xe the next evaluation point x_e' from it.  x_e' is formed ONCE, from the final state and next to its products: a second
// statement of it inside a noise branch left the choice of fusing the multiply-adds to where the optimiser moved the subtraction.
template <bool H2, int TH>
__device__ __forceinline__ void solver_elem(const SolverCoef& k, float s, float d2c, float vx0, float vxe, float vxb, float vd1, float vmp, float vmp2,
                                            float& oxb, float& od1, float& om) {
  float m = solver_m(k, vx0, vxe);
  if constexpr (TH != 0) m = solver_correct<TH>(m, s);
  const float x = vxb - k.g0 * vd1 - k.g1 * (m - vmp);
  oxb = k.A * x - k.Bc * m;
  od1 = H2 ? k.d1c * (vmp - m) + d2c * (vmp2 - m) : k.d1c * (vmp - m);
  om = m;
}
// The element behind the formation of m, for the flat step (misc.hip solver_step_flat_kernel), which enters with an m it formed from a noise / v /
// score output or was handed: the three lines of solver_elem, character for character.  (solver_elem calling this function instead of stating them
// gave the dynamic-thresholding kernels other code (tools/kernel_code_diff.py), and every earlier kernel keeps its code; with
// m = solver_m(vx0, vxe) the two give the same bits, which tests/test_sampler_pkg_gpu.py holds the flat kernel to.)
template <bool H2>
__device__ __forceinline__ void solver_elem_m(const SolverCoef& k, float d2c, float m, float vxb, float vd1, float vmp, float vmp2, float& oxb, float& od1,
                                              float& om) {
  const float x = vxb - k.g0 * vd1 - k.g1 * (m - vmp);
  oxb = k.A * x - k.Bc * m;
  od1 = H2 ? k.d1c * (vmp - m) + d2c * (vmp2 - m) : k.d1c * (vmp - m);
  om = m;
}
template <bool H2>
__device__ __forceinline__ float solver_xe(const SolverCoef& k, float pe, float oxb, float od1, float om, float vmp2) {
  return H2 ? oxb - k.pc * od1 - pe * (vmp2 - om) : oxb - k.pc * od1;
}
__device__ __forceinline__ void solver_upd(const SolverCoef& k, float vx0, float vxe, float vxb, float vd1, float vmp, float& oxe, float& oxb, float& od1, float& om) {
  solver_elem<false, 0>(k, 0.f, 0.f, vx0, vxe, vxb, vd1, vmp, 0.f, oxb, od1, om);
  oxe = solver_xe<false>(k, 0.f, oxb, od1, om, 0.f);
}

// Classifier-free guidance (sampler/uni_pc.py:225-229, sampler/dpm_solver.py:327-331 combine in noise space; eps is affine in x0 with the same
// x, alpha, sigma in both halves, so this is the same point): x0_g = x0_u + s * (x0_c - x0_u).  s == 1 SELECTS x0_c -- such an item follows its
// unguided trajectory from the conditional values with no rounding added (and takes nothing from x0_u, NaN included).
// ns2vc_amd.schedule.guided_x0 is the host statement.
__device__ __forceinline__ float guided_x0(float x0u, float x0c, float s) { return s == 1.0f ? x0c : x0u + s * (x0c - x0u); }

// Device noise of the stochastic samplers (DDPM, DDIM with eta > 0; ns2vc_amd/noise.py is the host statement of the stream):
// Philox4x32-10 (Salmon et al., SC 2011) keyed by the item's 64-bit seed, counter (t, c / 4, step, 0) -> the four normals of
// channels 4q..4q+3 at frame t by two Box-Muller pairs.  Precise logf / sincosf (not the __ intrinsics): the host agrees to ulps.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
    const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
    const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
  }
  return c;
}
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = ((float)a + 1.0f) * 0x1p-32f;       // (0, 1]: r stays finite
  const float u2 = (float)b * 0x1p-32f;
  const float r = sqrtf(-2.0f * logf(u1));
  float sn, cs;
  sincosf(u2 * 6.2831853071795864769f, &sn, &cs);
  z0 = r * cs; z1 = r * sn;
}
__device__ __forceinline__ float4 philox_gauss4(unsigned long long seed, uint32_t t, uint32_t q, uint32_t step) {
  const uint4 x = philox4x32_10(make_uint4(t, q, step, 0u), (uint32_t)seed, (uint32_t)(seed >> 32));
  float4 z;
  box_muller(x.x, x.y, z.x, z.y);
  box_muller(x.z, x.w, z.z, z.w);
  return z;
}

// Per-item solver schedules (ns2vc_sampler_load_items): loop item b walks rows [row0, row0 + steps) of the coefficient table, which holds the
// rows of all distinct tables of the batch, beginning at loop step `start`.  At loop step r the item is ACTIVE when 0 <= r - start < steps and
// uses row row0 + (r - start); otherwise it is HELD: its evaluation runs at the clamped row's timestep and nothing of its state is touched.
// ns2vc_amd.schedule.run_tables_numpy is the host statement.
struct SolverItem { int row0, steps, start, flags; };
constexpr int SOLVER_ITEM_HIST2 = 1;      // the item's table has a nonzero column 10 or 11: the history-2 element on all its rows, m_prev2 rolled
constexpr int SOLVER_ITEM_NOISE = 2;      // ... a nonzero column 9: the noise term, Philox "table row" word = the item's local row
__device__ __forceinline__ int solver_item_row(const SolverItem& it, int r, bool& active) {
  const int j = r - it.start;
  active = j >= 0 && j < it.steps;
  return it.row0 + min(max(j, 0), it.steps - 1);
}

// the record of an IDLE slot of a slot loop (ns2vc_sampler_open): never active at any loop step r >= 0 (r - start < 0 without overflow), evaluated
// at row 0 of the table
constexpr int SOLVER_ITEM_NEVER = 0x7fffffff;
__host__ __device__ __forceinline__ SolverItem solver_item_idle() { return SolverItem{0, 1, SOLVER_ITEM_NEVER, 0}; }

constexpr double GN_SUM_SCALE = 268435456.0;   // 2^28
constexpr double GN_SQ_SCALE = 65536.0;        // 2^16

// launchers (defined in the .hip files); return hipError_t
hipError_t launch_gemm(const GemmArgs& g, int prec, hipStream_t s);
size_t xattn_pack_bytes(int B, int Lk, int hd);                            // ffn.hip: the k | v fragment image of the in-kernel cross-attention
hipError_t launch_xattn_pack(const void* k, int ldk, const void* v, int ldv, int B, int Lk, int hd, void* out, int prec, hipStream_t s);
bool gemm_masks_rows(const GemmArgs& g, int prec);                        // ... on a kernel with a masked epilogue (GemmArgs.lens), were lens set?
bool gemm_uses_convts(const GemmArgs& g, int prec);                        // would launch_gemm run this launch on the tap-sharing conv kernel (convts.hip)?
int last_gemm_refusal_line();                                               // gemm.hip line of the argument check that refused the last launch on this thread (0: none), cleared by the call
// resident: the plan option attn_resident; resident_lens: masked_attn_resident (asked for launches under q_lens / k_lens only, and only with `resident`)
hipError_t launch_attention(const AttnArgs& a, int head_dim, int prec, hipStream_t s, bool resident = true, bool resident_lens = true);
// K/V-resident attention (attn_resident.hip): dense 16-bit launches at hd 16 / 32 whose key tiles all fit the LDS
bool attention_resident_eligible(const AttnArgs& a, int head_dim, int prec, bool allow);      // consulted by launch_attention only
hipError_t launch_attention_resident(const AttnArgs& a, int head_dim, int prec, hipStream_t s);
hipError_t init_attnres_attributes();
void set_attn_resident_mode(int mode);          // test / tuning hook: -1 = the rule (B*H >= CUs), 0 = never, 1 = whenever the launch fits
unsigned long long attn_resident_launches();   // launches issued (or captured) on the resident kernel so far in this process
void set_attnres_optimistic(int on);            // (set_attn_optimistic forwards to it)
// ... under per-item length tables (attnres_lens_kernel): a predicate, a hook and a counter of their own
bool attention_resident_lens_eligible(const AttnArgs& a, int head_dim, int prec, bool allow);      // consulted by launch_attention only, for masked launches
hipError_t launch_attention_resident_lens(const AttnArgs& a, int head_dim, int prec, hipStream_t s);
void set_attn_resident_lens_mode(int mode);     // test / tuning hook: -1 = the rule (B*H >= CUs), 0 = never, 1 = whenever the launch fits
unsigned long long attn_resident_lens_launches();
bool attention_masks_rows(const AttnArgs& a, int head_dim, int prec);      // ... on a masked instantiation (AttnArgs.q_lens / k_lens), were they set?
hipError_t init_gemm_attributes();
// tap-sharing k = 3 conv kernel (convts.hip)
bool convts_eligible(const GemmArgs& g, int prec);
int convts_default_bn(const GemmArgs& g);                                  // g.conv_bn if set, else the heuristic with the process default (debug hooks)
int convts_bn_for(const GemmArgs& g, int bn128_min);                       // the heuristic: 128-column tiles while they still give bn128_min workgroups
void set_convts_bn128_min(int wgs);
int convts_row_blocks(const GemmArgs& g);
hipError_t launch_convts(const GemmArgs& g, int prec, int bn, int nl, int ks, hipStream_t s);
hipError_t init_convts_attributes();
hipError_t pack_conv3_tiled(const float* rows, int N, int ctot, int c2, int prec, std::vector<unsigned char>& out);   // tile-major k = 3 conv weights (convts.hip)
void set_forced_gemm_tile(int bm, int bn, int stages);
void set_gemm_trace(unsigned long long* p);
hipError_t init_attn_attributes();
void set_forced_attn_keys(int keys);            // test hook: 0 = heuristic, 64 / 128 = K/V tile size where the kernel exists
// fused feed-forward + proj_out (ffn.hip), 16-bit operand types only
hipError_t launch_ffn(const ::ns2vc_ffn_args& a, int prec, hipStream_t s);
bool ffn_eligible(int dim, int T, int prec);
bool ffn_masks_rows(const ::ns2vc_ffn_args& a, int prec);                                      // ... on a masked instantiation (ns2vc_ffn_args.lens), were it set?
hipError_t init_ffn_attributes();
hipError_t pack_ffn_stream(const float* w1p, const float* w2f, const float* w0, int dim, int prec, std::vector<unsigned short>& out);
void set_ffn_trace(unsigned long long* p);
// token-stationary GEGLU projection (geglu.hip), 16-bit operand types, dim 384
bool geglu_eligible(int dim, int T, int prec);
hipError_t pack_geglu_stream(const float* w1p, const float* bias1p, int dim, int prec, std::vector<unsigned short>& stream, std::vector<float>& consts);
hipError_t launch_geglu(const ::ns2vc_geglu_args& a, int prec, hipStream_t s);
bool geglu_masks_rows(const ::ns2vc_geglu_args& a, int prec);                                  // ... on a masked instantiation (ns2vc_geglu_args.lens, T), were it set?
hipError_t init_geglu_attributes();
void set_gg_trace(unsigned long long* p);
void set_ts_trace(unsigned long long* p);       // convts.hip
void set_attn_optimistic(int on);               // attn.hip

// misc kernels (misc.hip).  "op" buffers are operand-typed (bf16 / fp16 / fp32 by `prec`)
hipError_t launch_gn_partial(const float* a0, int lda0, int c0, const float* a1, int lda1, int c1,
                             int B, int T, int G, double* partial, int nchunk, int rows_per_chunk, hipStream_t s);
hipError_t launch_gn_apply(const float* a0, int lda0, int c0, const float* a1, int lda1, int c1, int B, int T, int G, float eps,
                           const double* partial, int nchunk, const long long* st0, const long long* st1, const float* gamma,
                           const float* beta, const float* temb, int ldtemb, int temb_off, int silu, void* out_op, void* raw_op,
                           int prec, hipStream_t s, int pair = 0,       // pair (16-bit): out_op rows are [hi(C) | lo(C)] (op_rest)
                           const int* lens = nullptr);                  // per-item valid rows [B] (device) or NULL = all T
// per-item valid lengths: zero rows t >= lens[b] of a [B*T] row tensor in place, or (src set) copy row (b, t) from src row (b, t >> up) and
// zero the rest; pointers, strides and row_bytes 16-byte multiples
hipError_t launch_mask_rows(void* dst, size_t ldd_bytes, size_t row_bytes, int B, int T, const int* lens, hipStream_t s, const void* src = nullptr,
                            size_t lds_bytes = 0, int Tsrc = 0, int up = 0);
hipError_t launch_ln_apply_op(const float* x, int ldx, int M, int C, float eps, void* out_op, int prec, hipStream_t s);
hipError_t launch_cast_op(const float* x, size_t n, void* out_op, int prec, hipStream_t s, int split = 0);   // split: as SolverStep.split
hipError_t launch_time_embed(const float* t_ptr, int t_stride, const int* step_ptr, int coef_stride,
                             const float* w1t, const float* b1, const float* w2t, const float* b2,
                             const float* aug, float* emb, void* emb_act_op, int prec, int B, int tdim, int edim, hipStream_t s);
hipError_t launch_rowchain(const ::ns2vc_rowchain_args& a, int prec, hipStream_t s);            // rowchain.hip
bool rowchain_eligible(int dim, int n2, int T, int prec);
bool rowchain_masks_rows(const ::ns2vc_rowchain_args& a, int prec);                            // ... on a masked instantiation (ns2vc_rowchain_args.lens), were it set?
hipError_t init_rowchain_attributes();
hipError_t pack_rowchain_stream(const float* w1, const float* w2, int dim, int n2, int prec, std::vector<unsigned short>& out, int slices = 1);
int rowchain_slice_blocks(int n2, int slices);
void set_rc_trace(unsigned long long* p);
void set_forced_rowchain_tokens(int nt);        // test hook: 0 = heuristic, 1 = 64-token blocks, 2 = 128-token blocks (dim 128 only)
hipError_t launch_emb_from_table(const float* table, const int* step_ptr, const float* aug, float* emb, void* emb_act_op, int prec, int B,
                                 int edim, hipStream_t s);
int probe_xcd_round_robin(unsigned* map8 = nullptr);
//                                             // misc.hip: 1 = workgroup ids 8 apart share an XCD (what gnp_sync relies on), 0 = not, -1 = probe failed
hipError_t launch_zero(void* p, size_t bytes, hipStream_t s, int* counter = nullptr);                                  // bytes: any; p 16-byte aligned
hipError_t launch_copy16(const void* src, void* dst, size_t bytes, hipStream_t s);           // bytes % 16 == 0
hipError_t launch_poison(unsigned pattern, int lds_bytes, unsigned* sink, hipStream_t s);
hipError_t launch_nct_to_btc(const float* src, int C, int T, int B, float* dst_f32, void* dst_op, int prec, int ldd, int cpad, hipStream_t s,
                             int ldd_op = 0, int split = 0);   // split > 0 (16-bit): dst_op rows of ldd_op columns hold a hi + lo pair, lo at column split + c
hipError_t launch_btc_to_nct(const float* src, int lds, int C, int T, int B, float* dst, hipStream_t s);
hipError_t launch_mask_bias(const uint8_t* mask, int n, float* bias, hipStream_t s);
// the bias row under per-item prompt lengths (plens = DEVICE [B]): -10000 for the keys at or past plens[b], the mask's value below (mask may be NULL)
hipError_t launch_prompt_bias(const uint8_t* mask, const int* plens, int B, int Lp, float* bias, hipStream_t s);
hipError_t launch_ln_apply(const float* x, int M, int C, float eps, const float* gamma, const float* beta,
                           float* out, int L, int Lout_stride_rows, hipStream_t s);
// plens (DEVICE [B] or NULL): per-item prompt lengths -- the kernels' own forms, which pool over frames [0, plens[b]) of item b only
hipError_t launch_pool_cls(float* seq, int B, int L, int C, const float* pos, hipStream_t s, const int* plens = nullptr);
hipError_t launch_pool_attn(const float* qkv, int B, int L1, int C, int heads, float* pooled, hipStream_t s, const int* plens = nullptr);
hipError_t launch_pool_proj(const float* pooled, int B, int C, const float* wt, const float* b, int E,
                            const float* gamma, const float* beta, float eps, float* out, hipStream_t s);
// ---- the solver step (misc.hip) ----
// The kernels' argument structs, passed by value; launch_solver_step builds them from the one geometry of a SolverStep (below).
// noise: column 9 of the table row; where it is nonzero, state element (b, t, c) of rows of `ld` columns gains noise * z with
// z = philox_gauss4(seeds[b], t, c / 4, step), for c < nc and t < lens[b] (lens NULL: every t < T) -- the other elements get nothing
struct SolverNoise { const unsigned long long* seeds = nullptr; const int* lens = nullptr; int T = 0, ld = 0, nc = 0; };
// guidance: scale = DEVICE [n] per-item scales of a guided engine of 2n items of T rows of ld columns
struct SolverGuide { const float* scale = nullptr; int T = 0, ld = 0; };
// x0 correction (common.h solver_correct): mode 1 = dynamic thresholding by max(thr[b], max_val), thr = DEVICE [items] left by the quantile
// launch; mode 2 = clamp by max_val
struct SolverCorrect { int mode = 0; const float* thr = nullptr; float max_val = 1.0f; int T = 0, ld = 0; };
// per-item rows: rec = DEVICE [items] records (SolverItem above)
struct SolverItems { const SolverItem* rec = nullptr; int T = 0, ld = 0; };
// per-item x0 correction (ns2vc_sampler_set_x0_correction_items): DEVICE [items] records beside the SolverItem records, validated by the host
// (solver_items_fit: mode 0 = off, 1 = dynamic thresholding at the item's own ratio, 2 = clamp; max_val finite and > 0; mode 0 on a stochastic item)
struct ItemCorrect { int mode; float ratio, max_val; int reserved; };
// thr[b] = the p-quantile (torch.quantile's float32 rule) of |m| over rows t < lens[b] (NULL: T) and columns c < nc of item b's T rows of ld columns.
// xe == NULL: `v` holds the values themselves.  Otherwise v = x0 and m is formed as the update forms it from row *step_ptr of the table; with
// `scale` (DEVICE [items]) on guided_x0 of v and v + half (half = the elements of one half).  One workgroup per item, nothing shared between them
struct QuantArgs {
  const float* v = nullptr; const float* xe = nullptr; const float* coef = nullptr; const int* step_ptr = nullptr; int ncoef = 0;
  const float* scale = nullptr; size_t half = 0; const int* lens = nullptr; int T = 0, ld = 0, nc = 0; float p = 0.995f;
};
// items (DEVICE [n_items] records): every item's m from the row of its own table, thr[b] of a held item keeps its value; with item_correct
// (DEVICE [n_items]) only the active items in mode 1 get a threshold, at their own ratio (q.p is not read)
hipError_t launch_abs_quantile(const QuantArgs& q, int n_items, float* thr, hipStream_t s, const SolverItem* items = nullptr,
                               const ItemCorrect* item_correct = nullptr);
// What one solver step is, every fact once.  All pointers DEVICE; the optional parts are off when NULL / 0.
struct SolverStep {
  const float* coef = nullptr; const int* step_ptr = nullptr; int ncoef = 0;      // the table, its row (shared) or loop step (items) read from *step_ptr
  const float* x0 = nullptr; float* xe = nullptr; void* xe_op = nullptr; int prec = PREC_F32;      // the state; xe_op operand-typed by prec
  float *xbar = nullptr, *d1 = nullptr, *mprev = nullptr;
  float* mprev2 = nullptr;                 // the history-2 update (order-3 tables; m_{i-2} in, m_{i-1} out); under `items`, the buffer of the items that run it
  // the geometry: n elements (guided: of ONE half -- x0, xe and xe_op cover both, unconditional rows first, the histories the first) in whole
  // items of T rows of ld columns, nc of them real, lens[b] rows of item b valid (NULL: T).  T may stay 0 where no part below asks for items
  size_t n = 0; int T = 0, ld = 0, nc = 0; const int* lens = nullptr;
  int split = 0;                           // (16-bit) xe_op rows are the pair [hi(split) | lo(split)] of state rows of `split` columns
  const float* scale = nullptr;            // guidance: [items] per-item scales
  const unsigned long long* seeds = nullptr;      // noise: [items] seeds; no correction and (shared table) no history 2 with it
  const SolverItem* items = nullptr; int n_items = 0;      // per-item rows: n covers exactly these items; a held item is left alone
  int mode = 0; float ratio = 0.995f, max_val = 1.0f;      // loop-wide x0 correction, or ...
  const ItemCorrect* item_correct = nullptr; bool quant = false;      // ... per-item records (with `items`); quant: a record in mode 1 may exist
  float* thr = nullptr;                    // [items] thresholds: written by the quantile launch of mode 1 / quant, read by the update
};
// validates, issues the quantile launch where the form has one, then the update -- refused rather than run unguided, uncorrected or on the shared row
hipError_t launch_solver_step(const SolverStep& st, hipStream_t s);
// Known frames (ns2vc_sampler_set_known): the rows of x0 the caller holds get the caller's latent in front of the solver step.
// x0 = fp32 rows [halves * rows][ld], known = fp32 rows [rows][ld]; list = DEVICE ints, list[0] = the number of held rows and list[HOLD_LIST_HEAD + k]
// the k-th of them, a row of ONE half in [0, rows).  Held row r: x0[r][c] = known[r][c] for c < nc and 0 for nc <= c < ld, in both halves where
// halves == 2 (row r + rows); every other row keeps every bit.  The grid is sized by `rows`, the work by the count read on the device, so a captured
// launch serves every later list; a count above `rows` is clamped and an entry outside [0, rows) skipped, never used as an index.
constexpr int HOLD_LIST_HEAD = 4;
hipError_t launch_hold_x0(float* x0, const float* known, const int* list, int rows, int ld, int nc, int halves, hipStream_t s);
// Known frames of a slot loop (ns2vc_sampler_open_known): the same rule with the held rows given by a DEVICE byte mask [rows] (nonzero =
// held) instead of a list, so a slot's frames change without touching its neighbours' bytes.  The grid is sized by `rows` (one wave per 64 rows);
// a wave whose 64 bytes are all clear returns at once; a row index is a bit position of the wave's ballot, never a value read from memory.
hipError_t launch_hold_slots(float* x0, const float* known, const uint8_t* mask, int rows, int ld, int nc, int halves, hipStream_t s);
// known [n][C][T] fp32 and mask [n][T] bytes (both DEVICE) -> rows [slots[k] * T, + T) of known_rows [nslots * T][ld] (channels-last, columns C .. ld
// zero) and of mask_dst [nslots * T] (0 | 1), one launch for the DEVICE list `slots` [n]; known == mask == NULL: the listed slots' mask bytes
// become zero and nothing else is written.  An entry outside [0, nslots) is skipped, never used as an index.
hipError_t launch_known_items(const float* known, const uint8_t* mask, int C, int T, int n, const int* slots, int nslots, float* known_rows,
                              uint8_t* mask_dst, int ld, hipStream_t s);
// the time embedding under per-item rows: a held item is evaluated at its clamped row; B engine rows read the n_items records B / n_items times
hipError_t launch_emb_items_from_table(const float* table, const int* step_ptr, const SolverItem* items, int n_items, const float* aug, float* emb,
                                       void* emb_act_op, int prec, int B, int edim, hipStream_t s);
// slot loop (misc.hip, the last section): one launch per list of n slots read from device memory; nslots = the loop items an entry may name
hipError_t launch_sampler_admit(const float* x_T, int C, int T, int n, const int* slots, int nslots, const SolverItem* rec_in, SolverItem* rec, float* xe,
                                void* xe_op, int prec, float* xbar, float* d1, float* mprev, float* mprev2, int ld, int split, const int* lens, int half,
                                hipStream_t s);
hipError_t launch_sampler_take(const float* xe, int ld, int C, int T, int n, const int* slots, int nslots, float* dst, SolverItem* rec, hipStream_t s);
hipError_t launch_condition_items(const float* content, int Cc, int T, const float* prompt, int Lp, int Cx, const uint8_t* mask, int n, const int* slots,
                                  int nslots, void* content_op, int prec, int split, float* content_f32, const int* lens, float* prompt_dst,
                                  uint8_t* mask_dst, hipStream_t s);
// Suspend / resume of a slot's request: the state of the listed slots as P planes of T rows of ld fp32 columns, [n][P][T][ld] -- xe,
// xbar, d1, mprev and, with an mprev2 buffer, mprev2 (P = 5) -- copied bit for bit in float4 quads (every pointer 16-byte aligned, ld % 4 == 0).
// Suspend also writes the slots' idle records; resume rebuilds xe_op from xe as the solver update stores it, writes xe / xe_op to item slot + half of
// a guided engine as well and zeroes that item's histories, and installs rec_in[k] as the slot's record.
hipError_t launch_sampler_suspend(const float* xe, const float* xbar, const float* d1, const float* mprev, const float* mprev2, int T, int ld, int n,
                                  const int* slots, int nslots, float* dst, SolverItem* rec, hipStream_t s);
hipError_t launch_sampler_resume(const float* src, int T, int ld, int n, const int* slots, int nslots, const SolverItem* rec_in, SolverItem* rec, float* xe,
                                 void* xe_op, int prec, float* xbar, float* d1, float* mprev, float* mprev2, int split, int half, hipStream_t s);
// The flat solver step (ns2vc_k_solver_step_flat; the top-level sampler/ package's device path): row `crow` (NCOEF floats, DEVICE) on n elements of
// five state planes of any 4-byte alignment.  kind 0 x_start | 1 noise | 2 v | 3 score | 4 data says what `out` holds; mprev2 NULL = history 1;
// m_out non-NULL = FORM (m is written there, no state plane is touched).  FLAT_MAX_BLOCKS 256-thread blocks at most: one trip of the grid covers
// FLAT_MAX_BLOCKS * 1024 elements, the rest comes in further trips of the grid-stride loop.
constexpr unsigned FLAT_MAX_BLOCKS = 1024;
hipError_t launch_solver_step_flat(const float* crow, int kind, const float* out, float* xe, float* xbar, float* d1, float* mprev, float* mprev2,
                                   float* m_out, size_t n, hipStream_t s);
// the normals a stochastic update adds at table row `step` (ns2vc_k_noise): out rows [B*T][ld] fp32, zeros where no noise goes
hipError_t launch_noise(const unsigned long long* seeds, int B, int nc, int T, int ld, int step, const int* lens, float* out, hipStream_t s);
hipError_t launch_fill_i32(int* p, int v, hipStream_t s);
hipError_t launch_placement(unsigned* dev_out, int n_blocks, int spin, hipStream_t s);
hipError_t launch_snapshot_u32(unsigned* src, unsigned* dst, hipStream_t s);   // *dst = atomicExch(src, 0)

}  // namespace ns2vc
