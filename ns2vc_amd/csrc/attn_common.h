// What the attention kernels share (attn.hip: K/V streamed through a two-stage LDS ring; attn_resident.hip: a head's K/V staged once): the MFMA
// wrappers, the operand-type helpers, the geometry of one K / V^T stage in LDS and the arithmetic of one key tile.  One definition of each: the
// resident kernel must return the tiled kernel's bits.
#pragma once
#include "common.h"
#include "mma.h"

namespace ns2vc {

template <typename T> struct AMma;
template <> struct AMma<float> {
  static constexpr int SZ = 4;
  __device__ static __forceinline__ void mma(f32x16_t& acc, const u32x4_t& a, const u32x4_t& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  }
  __device__ static __forceinline__ f32x16_t mma0(const u32x4_t& a, const u32x4_t& b) {   // acc = a*b (srcC = inline 0)
    f32x16_t acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), f32x16_t{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
    return acc;
  }
  // position (in elements) of key `key` (0..31) inside a 32-key V^T sub-row
  __device__ static __forceinline__ int vpos(int key) { return key; }
};
template <typename TM> struct AMma16 {     // bf16_t / f16_t: one v_mfma_f32_32x32x16_{bf16,f16} per 32-B k-slab
  static constexpr int SZ = 2;
  __device__ static __forceinline__ void mma(f32x16_t& acc, const u32x4_t& a, const u32x4_t& b) { MmaT<TM>::mma(acc, a, b); }
  __device__ static __forceinline__ f32x16_t mma0(const u32x4_t& a, const u32x4_t& b) {   // acc = a*b (srcC = inline 0)
    f32x16_t acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    MmaT<TM>::mma(acc, a, b);
    return acc;
  }
  // swap key bits 2 and 3 so that the 8 keys one lane-half contributes to a
  // 16-key MFMA k-slab are contiguous (see header comment of attn_kernel)
  __device__ static __forceinline__ int vpos(int key) { return (key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1); }
};
template <> struct AMma<bf16_t> : AMma16<bf16_t> {};
template <> struct AMma<f16_t> : AMma16<f16_t> {};

// scatter the EPC elements of one 16-B piece (one key, EPC consecutive d) down a V^T column
template <typename TM> __device__ __forceinline__ void vt_scatter(char* vp, int rowb, const u32x4_t& v);
template <> __device__ __forceinline__ void vt_scatter<float>(char* vp, int rowb, const u32x4_t& v) {
  *reinterpret_cast<uint32_t*>(vp) = v.x;
  *reinterpret_cast<uint32_t*>(vp + rowb) = v.y;
  *reinterpret_cast<uint32_t*>(vp + 2 * rowb) = v.z;
  *reinterpret_cast<uint32_t*>(vp + 3 * rowb) = v.w;
}
__device__ __forceinline__ void vt_scatter16(char* vp, int rowb, const u32x4_t& v) {
  *reinterpret_cast<uint16_t*>(vp) = (uint16_t)v.x;
  *reinterpret_cast<uint16_t*>(vp + rowb) = (uint16_t)(v.x >> 16);
  *reinterpret_cast<uint16_t*>(vp + 2 * rowb) = (uint16_t)v.y;
  *reinterpret_cast<uint16_t*>(vp + 3 * rowb) = (uint16_t)(v.y >> 16);
  *reinterpret_cast<uint16_t*>(vp + 4 * rowb) = (uint16_t)v.z;
  *reinterpret_cast<uint16_t*>(vp + 5 * rowb) = (uint16_t)(v.z >> 16);
  *reinterpret_cast<uint16_t*>(vp + 6 * rowb) = (uint16_t)v.w;
  *reinterpret_cast<uint16_t*>(vp + 7 * rowb) = (uint16_t)(v.w >> 16);
}
template <> __device__ __forceinline__ void vt_scatter<bf16_t>(char* vp, int rowb, const u32x4_t& v) { vt_scatter16(vp, rowb, v); }
template <> __device__ __forceinline__ void vt_scatter<f16_t>(char* vp, int rowb, const u32x4_t& v) { vt_scatter16(vp, rowb, v); }

// combine a value with its partner lane (lane ^ 32) without an LDS round trip: v_permlane32_swap puts the lower
// half's values in one result and the upper half's in the other, for every lane
__device__ __forceinline__ float half_max(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
__device__ __forceinline__ float half_sum(float v) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// operand-type helpers of the softmax reference shift
template <typename TM> __device__ __forceinline__ float round_op(float x);
template <> __device__ __forceinline__ float round_op<float>(float x) { return x; }
template <> __device__ __forceinline__ float round_op<bf16_t>(float x) { return __uint_as_float(pack_bf16x2(0.f, x) & 0xffff0000u); }
template <> __device__ __forceinline__ float round_op<f16_t>(float x) { return f16_lo(pack_f16x2(x, 0.f)); }
// first 16-B chunk of a K/Q "aux" k-slab: {e0, e1, 0, ...}
template <typename TM> __device__ __forceinline__ u32x4_t aux_chunk(float e0, float e1);
template <> __device__ __forceinline__ u32x4_t aux_chunk<float>(float e0, float e1) { return u32x4_t{__float_as_uint(e0), __float_as_uint(e1), 0u, 0u}; }
template <> __device__ __forceinline__ u32x4_t aux_chunk<bf16_t>(float e0, float e1) { return u32x4_t{pack_bf16x2(e0, e1), 0u, 0u, 0u}; }
template <> __device__ __forceinline__ u32x4_t aux_chunk<f16_t>(float e0, float e1) { return u32x4_t{pack_f16x2(e0, e1), 0u, 0u, 0u}; }
template <typename TM> __device__ __forceinline__ TM op_from_float(float x);
template <> __device__ __forceinline__ float op_from_float<float>(float x) { return x; }
template <> __device__ __forceinline__ bf16_t op_from_float<bf16_t>(float x) { bf16_t r; r.v = (uint16_t)pack_bf16x2(x, 0.f); return r; }
template <> __device__ __forceinline__ f16_t op_from_float<f16_t>(float x) { f16_t r; r.v = (uint16_t)pack_f16x2(x, 0.f); return r; }   // (-inf passes)

// The attention kernels are bound by instruction issue on MI355X (every score used to cost a scale-fma, a max, a subtract,
// an exp, a sum-add and half a convert), while the MFMA pipe idles.  v_exp_f32 itself issues in 9.75 cycles with one wave per
// SIMD and 6.8 SIMD-cycles with two (profiles/vexp_probe_r02.txt) -- not the 16 of a quarter-rate unit that earlier notes
// assumed: the exponentials of a level-0 self-attention are 10-12 us, about a third of the tiled hd-16 launch, not its floor.
// So everything except max / exp / convert is pushed INTO the MFMAs:
//   * the softmax scale (in log2 units) is folded into Q once, at load;
//   * every K row carries an extra "aux" k-slab {1, bias(key), 0...} and every Q fragment the matching {-m_ref, 1, 0...}:
//     the score MFMA returns  s*scale*log2e + bias - m_ref  directly (mask bias and tail-key -inf included);
//   * m_ref is a per-query REFERENCE, not the running maximum: probabilities are exp2(score - m_ref) for a whole run of
//     tiles and only when some score exceeds m_ref by 2^12 are accumulators and reference moved (softmax is
//     shift-invariant, so any common reference is exact; it is kept representable in the operand type so the shift done
//     by the MFMA is exact too);
//   * V^T carries a row of ones, so the PV MFMA also accumulates the denominator (of the SAME rounded probabilities
//     that build the numerator): no per-score add, no separate running sum.
// P8 (16-bit operand types only; BASELINE config 5's "fp8 MFMA attention path"): the PV product runs on the fp8-RATE matrix
// instruction of gfx950, v_mfma_scale_f32_32x32x64_f8f6f4 (K = 64 = one whole key tile per instruction, OCP e4m3 operands, unit
// E8M0 scales; twice the bf16 rate -- the non-scaled v_mfma_f32_32x32x16_fp8_fp8 of round 2 runs at the bf16 rate,
// MI355X_MICROARCH.md "Matrix cores").  V^T is staged in LDS as fp8 (converted while staging), the probabilities are packed to
// fp8 instead of the 16-bit type; QK^T (K = head dim: 16..64), the softmax state and all accumulators are unchanged.
// Operand slots: the instruction contracts over 64 k-slots, lane half `hi` supplying slots 32*hi .. 32*hi+31 of its A row / B
// column (8 VGPRs, 4 slots each).  The contraction index is a dummy, so the keys are PERMUTED to where the score MFMA left
// them: after S^T = K Q^T lane (q, hi) holds the keys  k2*32 + 8*g + 4*hi + i  (k2 = 32-key sub-tile, g = 0..3, i = 0..3) in
// s[k2][4*g + i]; key -> slot 32*hi + (16*k2 + 4*g + i), i.e. P's register v = 4*k2 + g is pack(s[k2][4g .. 4g+3]) with no
// data movement at all, and V^T rows are stored with the same key -> slot map (vpos8).  See DESIGN section 4 for why it stays an
// option (the kernel is VALU-bound, fp8 shortens only the matrix time; 3 mantissa bits in P cost the parity bar).
__device__ __forceinline__ uint32_t pack_fp8x4(float a, float b, float c, float d) {
  int v = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  v = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, v, true);
  return (uint32_t)v;
}
typedef int i32x8_t __attribute__((ext_vector_type(8)));
#ifndef NS2VC_ATTN_OPT
#define NS2VC_ATTN_OPT 1
#endif
template <bool B> struct OptTag { static constexpr bool value = B; };
// slot of key (0..63) inside a 64-slot V^T row of the fp8 path
__device__ __forceinline__ int vpos8(int key) { return ((key & 4) << 3) | ((key & 32) >> 1) | ((key & 24) >> 1) | (key & 3); }

// One K / V^T stage in LDS and one key tile's arithmetic on it, for one wave's 32 queries.  The stage is KEYS rows of K (HD elements, a 32-B "aux"
// k-slab {1, bias(key), 0 ...}, a 16-B pad nobody reads) followed by HDX rows of V^T (KEYS keys in vpos order, a 16-B pad): HD value rows, the ones row
// (row HD), zero rows up to the next multiple of 32.
template <typename TM, int HD, int KEYS, bool P8> struct AttnTile {
  static constexpr int NSUB = KEYS / 32;         // 32-key sub-tiles per K/V tile (2 or 4): per-tile bookkeeping, barrier and waits amortise over them
  static constexpr int SZ = AMma<TM>::SZ;
  static constexpr int EPC = 16 / SZ;            // elements per 16-B fragment chunk
  static constexpr int NS = HD * SZ / 32;        // 32-B d-slabs per key row (QK^T k-steps), + 1 aux slab
  static constexpr int KROWB = HD * SZ + 48;     // K tile row bytes: HD elements, 32-B aux slab, pad (stride = 4*odd dwords)
  static constexpr int VSZ = P8 ? 1 : SZ;        // bytes per V^T / P element
  static constexpr int VROWB = KEYS * VSZ + 16;  // V^T tile row bytes (KEYS keys)
  static constexpr int HDX = (HD + 1 + 31) / 32 * 32;   // V^T rows: HD value rows + the ones row (row HD), padded to 32
  static constexpr int DT = HDX / 32;
  static constexpr int NSL = SZ;                 // 32-B key-slabs per 32-key sub-tile (f32: 4x8 keys, bf16: 2x16 keys)
  static constexpr int KBYTES = KEYS * KROWB, VBYTES = HDX * VROWB;
  static constexpr int STAGE = KBYTES + VBYTES;
  static constexpr int PPR = HD * SZ / 16;       // 16-B pieces per key row
  static constexpr int NPIECE = KEYS * PPR;      // pieces per K (or V) tile
  static constexpr float THRESH = P8 ? 8.0f : 12.0f;   // move the reference when a score exceeds it by more than this (log2 units; fp8: p <= 2^8 < 448)
  static constexpr float OPT_MARGIN = 4.0f;
  // r6, hd 16 without a mask bias (the level-0 self-attention: a quarter of this kernel's MFMAs is the aux slab, which then only carries -m_ref): the
  // reference enters as the score MFMA's C operand instead -- sixteen registers that hold -m_ref, rewritten when the reference moves (once per pass in the
  // optimistic form) -- and the aux slab, its LDS read and its MFMA are left to the one tile that needs the tail keys' -inf.  Same sum in the same order:
  // the aux product was the first addend of every score already.  (hd 32: the sixteen registers would cost a wave per SIMD; with a bias the C operand
  // would have to be rebuilt per tile, 16 VALU adds against one MFMA.)
  static constexpr bool CINIT = HD == 16 && SZ == 2 && !P8;
  // the accumulator row of the denominator: block HD/32, register ((HD%32)/8)*4, lane half 0
  static constexpr int LB = HD / 32, LR = ((HD % 32) / 8) * 4;
  static_assert(HD % 32 == 0 || HD % 32 == 16, "ones row must sit at row 0 or 16 of its 32-row block");

  // piece u (0 .. NPIECE-1) of a tile: K pieces run row-major (coalesced along d), V pieces key-fastest (the transposed LDS write is then conflict-free)
  __device__ static __forceinline__ void store_k_piece(char* Ks, int u, const u32x4_t& raw) {
    const int key = u / PPR, pc = u - key * PPR;
    *reinterpret_cast<u32x4_t*>(Ks + key * KROWB + pc * 16) = raw;
  }
  __device__ static __forceinline__ void store_v_piece(char* Vs, int u, const u32x4_t& w) {
    const int key = u % KEYS, pc = u / KEYS;
    if constexpr (P8) {       // eight 16-bit values of one key -> eight fp8 bytes down the V^T column, at the key's k-slot
      const uint32_t b0 = pack_fp8x4(Op16<TM>::lo(w.x), Op16<TM>::hi(w.x), Op16<TM>::lo(w.y), Op16<TM>::hi(w.y));
      const uint32_t b1 = pack_fp8x4(Op16<TM>::lo(w.z), Op16<TM>::hi(w.z), Op16<TM>::lo(w.w), Op16<TM>::hi(w.w));
      uint8_t* vp = reinterpret_cast<uint8_t*>(Vs + (pc * EPC) * VROWB + vpos8(key));
#pragma unroll
      for (int j = 0; j < 4; ++j) { vp[j * VROWB] = (uint8_t)(b0 >> (8 * j)); vp[(4 + j) * VROWB] = (uint8_t)(b1 >> (8 * j)); }
    } else {
      const int pos = (key & ~31) + AMma<TM>::vpos(key & 31);
      vt_scatter<TM>(Vs + (pc * EPC) * VROWB + pos * SZ, VROWB, w);
    }
  }

  // one key tile for this wave's 32 queries: scores, reference check, probabilities, PV.  O: the optimistic pass (reference from tile 0 alone);
  // cform (wave-uniform, CINIT kernels only): the reference through the C operand, no aux slab
  template <bool O>
  __device__ static __forceinline__ void step(const char* Ks, const char* Vs, const int t, const bool cform, const u32x4_t (&qf)[NS], u32x4_t& qaux,
                                              f32x16_t& cinit, float& m_ref, f32x16_t (&o)[DT], const int l31, const int hi) {
    // ---- S'^T[key][q] = sum_d K[key][d] * (Q[q][d]*scale*log2e) + 1*(-m_ref[q]) + bias[key]*1   (two 32-key sub-tiles)
    f32x16_t s[NSUB];
    if (CINIT && cform) {
#pragma unroll
      for (int k2 = 0; k2 < NSUB; ++k2) {
        const char* kr = Ks + (k2 * 32 + l31) * KROWB + hi * 16;
        s[k2] = cinit;
#pragma unroll
        for (int sl = 0; sl < NS; ++sl) AMma<TM>::mma(s[k2], *reinterpret_cast<const u32x4_t*>(kr + sl * 32), qf[sl]);
      }
    } else {
#pragma unroll
    for (int k2 = 0; k2 < NSUB; ++k2) {
      const char* kr = Ks + (k2 * 32 + l31) * KROWB + hi * 16;
      s[k2] = AMma<TM>::mma0(*reinterpret_cast<const u32x4_t*>(kr + NS * 32), qaux);      // aux slab first: no zero-init movs
#pragma unroll
      for (int sl = 0; sl < NS; ++sl) AMma<TM>::mma(s[k2], *reinterpret_cast<const u32x4_t*>(kr + sl * 32), qf[sl]);
    }
    }
    // ---- reference check (per query = per lane; both lane halves agree): lane's keys are k2*32 + 8*g + 4*hi + i
    if (!O || t == 0) {
      float mx = s[0][0];
#pragma unroll
      for (int k2 = 0; k2 < NSUB; ++k2)
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[k2][r]);
      mx = half_max(mx);
      if (t == 0 || __any(mx > THRESH)) {                 // wave-uniform; after the first tile this is rare
        float target = t == 0 ? mx : fmaxf(mx, 0.f);
        if (!(target > -INFINITY)) target = 0.f;          // nothing but masked keys so far
        if (O) target += OPT_MARGIN;
        const float m_new = round_op<TM>(m_ref + target);
        const float dsh = m_new - m_ref;
        if (t > 0) {
          const float alpha = __builtin_amdgcn_exp2f(-dsh);    // dsh >= 0
#pragma unroll
          for (int d = 0; d < DT; ++d)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
        }
#pragma unroll
        for (int k2 = 0; k2 < NSUB; ++k2)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[k2][r] -= dsh;
        m_ref = m_new;
        if (hi == 0) qaux = aux_chunk<TM>(-m_ref, 1.0f);
        if constexpr (CINIT) {
#pragma unroll
          for (int r = 0; r < 16; ++r) cinit[r] = -m_ref;
        }
      }
    }
#pragma unroll
    for (int k2 = 0; k2 < NSUB; ++k2)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[k2][r] = __builtin_amdgcn_exp2f(s[k2][r]);

    // ---- [O^T ; l][d][q] += sum_key [V^T ; 1][d][key] * P^T[key][q]
    if constexpr (P8) {
      // the lane's 32 probabilities of this tile = its 32 k-slots, already in slot order: register v = 4*k2 + g
      i32x8_t pf;
#pragma unroll
      for (int v = 0; v < 8; ++v)
        pf[v] = (int)pack_fp8x4(s[v >> 2][4 * (v & 3) + 0], s[v >> 2][4 * (v & 3) + 1], s[v >> 2][4 * (v & 3) + 2], s[v >> 2][4 * (v & 3) + 3]);
#pragma unroll
      for (int d = 0; d < DT; ++d) {
        const char* vr = Vs + (d * 32 + l31) * VROWB + hi * 32;
        const u32x4_t v0 = *reinterpret_cast<const u32x4_t*>(vr), v1 = *reinterpret_cast<const u32x4_t*>(vr + 16);
        const i32x8_t vf = {(int)v0.x, (int)v0.y, (int)v0.z, (int)v0.w, (int)v1.x, (int)v1.y, (int)v1.z, (int)v1.w};
        // cbsz = blgp = 0: both operands OCP e4m3; scales 0x7f = 2^0 in every E8M0 byte
        o[d] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(vf, pf, o[d], 0, 0, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
      }
    } else {
#pragma unroll
    for (int k2 = 0; k2 < NSUB; ++k2) {
#pragma unroll
      for (int sl = 0; sl < NSL; ++sl) {
        u32x4_t pf;
        if constexpr (SZ == 4) {
          pf = u32x4_t{__float_as_uint(s[k2][4 * sl + 0]), __float_as_uint(s[k2][4 * sl + 1]),
                       __float_as_uint(s[k2][4 * sl + 2]), __float_as_uint(s[k2][4 * sl + 3])};
        } else {
          pf = u32x4_t{Op16<TM>::pack(s[k2][8 * sl + 0], s[k2][8 * sl + 1]), Op16<TM>::pack(s[k2][8 * sl + 2], s[k2][8 * sl + 3]),
                       Op16<TM>::pack(s[k2][8 * sl + 4], s[k2][8 * sl + 5]), Op16<TM>::pack(s[k2][8 * sl + 6], s[k2][8 * sl + 7])};
        }
#pragma unroll
        for (int d = 0; d < DT; ++d) {
          const u32x4_t vf = *reinterpret_cast<const u32x4_t*>(Vs + (d * 32 + l31) * VROWB + k2 * 32 * SZ + sl * 32 + hi * 16);
          AMma<TM>::mma(o[d], vf, pf);
        }
      }
    }
    }
  }

  // Q fragments of query row qp (B operand of S^T = K Q^T), pre-multiplied by scale*log2e: lane (q, hi) holds d = s*2*EPC + hi*EPC .. +EPC; a row that
  // does not exist (`dead`) enters as zeros
  __device__ static __forceinline__ void load_q(u32x4_t (&qf)[NS], const TM* qp, const float sc2, const int hi, const bool dead) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const u32x4_t raw = *reinterpret_cast<const u32x4_t*>(qp + s * 2 * EPC + hi * EPC);
      if constexpr (SZ == 4) {
        qf[s] = u32x4_t{__float_as_uint(__uint_as_float(raw.x) * sc2), __float_as_uint(__uint_as_float(raw.y) * sc2),
                        __float_as_uint(__uint_as_float(raw.z) * sc2), __float_as_uint(__uint_as_float(raw.w) * sc2)};
      } else {
        auto sc = [&](uint32_t w) __attribute__((always_inline)) { return Op16<TM>::pack(Op16<TM>::lo(w) * sc2, Op16<TM>::hi(w) * sc2); };
        qf[s] = u32x4_t{sc(raw.x), sc(raw.y), sc(raw.z), sc(raw.w)};
      }
      if (dead) qf[s] = u32x4_t{0, 0, 0, 0};
    }
  }

  // normalise and store O[q][h*HD + d] (op = the row's first element of this head); lane holds d = dt*32 + 8*g + 4*hi + i.  The denominator is row HD of
  // the accumulator, lane half 0 -> broadcast to both halves.  `live`: the row exists in out; `padded`: it is stored as exact zeros
  __device__ static __forceinline__ void store_out(const f32x16_t (&o)[DT], TM* op, const int hi, const bool live, const bool padded) {
    const auto lsw = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[LB][LR]), __float_as_uint(o[LB][LR]), false, false);
    const float l_tot = __uint_as_float(lsw[0]);
    const float inv = 1.0f / l_tot;
    if constexpr (SZ == 2) {
      // 16-bit results: the two lane halves of a query trade 4-element groups so that every lane stores 8 consecutive d (16 B) -- half the store
      // instructions of the 8-byte form, and the output of a workgroup is nothing but row-per-lane pieces whose issue sets its tail (r5: without
      // any output store the step ran 2.2 % faster)
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int gp = 0; gp < 2; ++gp) {
          if (d * 32 + 16 * gp < HD) {
            const uint32_t a0 = Op16<TM>::pack(o[d][8 * gp] * inv, o[d][8 * gp + 1] * inv), a1 = Op16<TM>::pack(o[d][8 * gp + 2] * inv, o[d][8 * gp + 3] * inv);
            const uint32_t b0 = Op16<TM>::pack(o[d][8 * gp + 4] * inv, o[d][8 * gp + 5] * inv), b1 = Op16<TM>::pack(o[d][8 * gp + 6] * inv, o[d][8 * gp + 7] * inv);
            const auto x0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);      // lower half: group 2 gp of both halves; upper half: group 2 gp + 1
            const auto x1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
#if defined(NS2VC_ATTN_ABLATE_STORE)      // diagnostic build (wrong results, timing only): no output stores
            asm volatile("" :: "v"(x0[0]), "v"(x1[0]), "v"(x0[1]), "v"(x1[1]));
#else
            if (live) *reinterpret_cast<u32x4_t*>(op + d * 32 + 8 * (2 * gp + hi)) = padded ? u32x4_t{0, 0, 0, 0} : u32x4_t{x0[0], x1[0], x0[1], x1[1]};
#endif
          }
        }
    } else if (live) {
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const int d0 = d * 32 + 8 * gq + 4 * hi;
          if (d0 < HD) store_op4<TM>(op + d0, padded ? 0.f : o[d][4 * gq] * inv, padded ? 0.f : o[d][4 * gq + 1] * inv, padded ? 0.f : o[d][4 * gq + 2] * inv,
                                     padded ? 0.f : o[d][4 * gq + 3] * inv);
        }
    }
  }
};

}  // namespace ns2vc
