// Flash-style multi-head attention for the NS2VC denoiser on CDNA4 (gfx950).
//
// Replaces F.scaled_dot_product_attention at reference
// unet1d/attention_processor.py:1032 (self-attention, Lq = Lk = T_l, no mask; and
// prompt cross-attention, Lk = Lp, additive mask bias (1-m)*-10000 built at
// unet1d/unet_1d_condition.py:816-818 and broadcast over heads :1003-1007).
//
// One workgroup = 4 waves = 128 queries of one (batch, head); each wave owns 32
// queries.  K/V stream through LDS in 64-key tiles (register prefetch of tile
// t+1 under the MFMAs of tile t, one barrier per tile).  The score tile is
// computed TRANSPOSED, S^T = K * Q^T, so that after the 32x32 MFMA each lane
// holds 16 keys of ONE query (col = lane&31): the online-softmax row reduction is
// lane-local plus one exchange with lane^32, and the probabilities feed the PV
// MFMA's B operand straight from registers.  O^T = V^T * P^T needs V^T tiles,
// which are written transposed into LDS at staging time.
//   bf16: v_mfma_f32_32x32x16_bf16, P rounded to bf16, fp32 softmax state / accumulators
//   f32 : v_mfma_f32_32x32x2_f32 (exact fp32, parity mode)
// head_dim in {16,32,48,64} (NS2VC: C_l/8 for C_l in {128,256,384,512}).
// Every workgroup of a head stages all of the head's K/V tiles: at Lq = Lk = 938 that is eight times per launch, and about half of
// the instructions a wave issues per tile are staging.  Dense 16-bit launches at hd 16 / 32 whose key tiles all fit the LDS
// (<= 1024 / 640 keys) and whose grid fills the chip (B*H >= the CUs) therefore run on attnres_kernel (attn_resident.hip: one
// 16-wave workgroup per head, K/V staged once, no barrier in the loop), chosen by launch_attention through
// attention_resident_eligible; the tile arithmetic both kernels execute is AttnTile (attn_common.h), and their results are
// bit-identical.  This kernel keeps fp32, the fp8 PV form, masked launches, hd 48 / 64, longer key rows and small grids.  (Masked launches of the
// same shapes move to attnres_lens_kernel where the plan has the option masked_attn_resident on as well: attention_resident_lens_eligible.)
// q/k/v/out are operand-typed tensors (bf16, or fp32 in parity mode): no conversions while staging.
#include "attn_common.h"
#include "kernel_table.h"
#include <cstdlib>

namespace ns2vc {

// test hook (ns2vc_debug_set_attn_optimistic): 1 = every workgroup takes the exact pass only
__device__ int g_attn_exact_only = 0;
// MASKED: per-item query and key counts (AttnArgs.q_lens / k_lens; option masked_attn).  Its own instantiations: the dense ones keep their instructions.
// The item's key count Lkb stands wherever the dense kernel uses Lk -- the clamp of the row fetch, the tail keys' -inf, the tile count and the C-operand
// condition -- so item b walks exactly the tiles the dense kernel walks for it alone at Lk = Lkb (the row stride between items stays Lk).  The item's query
// count Lqb does the same for Lq (rows past it are fetched from the last valid row, enter as zeros and never decide a repeat of the optimistic pass), except
// that those rows exist in `out`: they are stored as exact zeros, and a query tile wholly past Lqb stores them before it touches K, V or the LDS.
template <typename TM, int HD, int KEYS, bool P8, bool MASKED = false>
__global__ __launch_bounds__(256) void attn_kernel(const AttnArgs a) {
  op_mode_init<TM>();
  static_assert(!P8 || (sizeof(TM) == 2 && KEYS == 64), "the fp8 PV path: 16-bit operand types, one 64-key tile per f8f6f4 MFMA");
  using G = AttnTile<TM, HD, KEYS, P8>;      // stage geometry and tile arithmetic (attn_common.h)
  constexpr int SZ = G::SZ, EPC = G::EPC, NS = G::NS, KROWB = G::KROWB, VROWB = G::VROWB, DT = G::DT, KBYTES = G::KBYTES, STAGE = G::STAGE, PPR = G::PPR,
                NPIECE = G::NPIECE;
  constexpr int UPT = (NPIECE + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  // XCD-aware mapping: consecutive workgroup ids round-robin over the 8 XCDs (each with a private L2), so the ids are
  // remapped to give every XCD a contiguous run of (batch item, head, query block): all heads and query blocks of one
  // batch item share K/V rows (a head is a 32..128-B column slice of them) and now hit the same L2.  Measured before
  // the remap (rocprofv3 FETCH_SIZE): 77-132 MB fetched per launch for ~28 MB of Q/K/V, L2 hit rate 24-29 %.
  const int nqb = (a.Lq + 127) >> 7;
  int b, h, qb;
  {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int qn = nwg >> 3, rn = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    const int swz = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + idx;
    b = swz / (a.H * nqb);
    const int rem = swz - b * (a.H * nqb);
    h = rem / nqb;
    qb = rem - h * nqb;
  }
  const int q = qb * 128 + wave * 32 + l31;
  int Lqb = a.Lq, Lkb = a.Lk;             // this item's query / key counts (workgroup-uniform; clamped to the tensor: a bad table cannot send a fetch outside it)
  if constexpr (MASKED) {
    if (a.q_lens) Lqb = min(max(a.q_lens[b], 0), a.Lq);
    if (a.k_lens) Lkb = min(max(a.k_lens[b], 1), a.Lk);
    if (qb * 128 >= Lqb) {                // nothing but padded queries: their zeros, and no K / V tile, no MFMA
      if (q < a.Lq) {
        char* zp = reinterpret_cast<char*>(a.out) + ((size_t)(b * a.Lq + q) * a.ldo + h * HD) * SZ;
#pragma unroll
        for (int pc = hi; pc < PPR; pc += 2) *reinterpret_cast<u32x4_t*>(zp + pc * 16) = u32x4_t{0, 0, 0, 0};
      }
      return;
    }
  }
  const float LOG2E = 1.4426950408889634f;
  const float sc2 = a.scale * LOG2E;      // scores are kept in log2 units

  // zero both stages once (V^T pad rows and the aux slabs' tails must read as 0), then the constants
  for (int i = tid * 16; i < 2 * STAGE; i += 256 * 16) *reinterpret_cast<u32x4_t*>(smem + i) = u32x4_t{0, 0, 0, 0};
  __syncthreads();
  for (int i = tid; i < 2 * KEYS; i += 256) {      // K aux element 0 = 1 for every key row, V^T row HD = ones, both stages
    const int st = i / KEYS, key = i - st * KEYS;
    *reinterpret_cast<TM*>(smem + st * STAGE + key * KROWB + HD * SZ) = op_from_float<TM>(1.0f);
    if constexpr (P8) *reinterpret_cast<uint8_t*>(smem + st * STAGE + KBYTES + HD * VROWB + key) = (uint8_t)0x38;     // e4m3 1.0; all 64 slots of the row
    else *reinterpret_cast<TM*>(smem + st * STAGE + KBYTES + HD * VROWB + key * SZ) = op_from_float<TM>(1.0f);
  }

  u32x4_t qf[NS];
  G::load_q(qf, reinterpret_cast<const TM*>(a.q) + ((size_t)(b * a.Lq + min(q, Lqb - 1)) * a.ldq + h * HD), sc2, hi, q >= Lqb);
  float m_ref = 0.f;                       // softmax reference of this lane's query (operand-representable)
  u32x4_t qaux = hi == 0 ? aux_chunk<TM>(-m_ref, 1.0f) : u32x4_t{0, 0, 0, 0};
  constexpr bool CINIT = G::CINIT;         // the reference through the score MFMA's C operand (AttnTile)
  f32x16_t cinit;
#pragma unroll
  for (int r = 0; r < 16; ++r) cinit[r] = 0.f;

  const TM* kbase = reinterpret_cast<const TM*>(a.k) + (size_t)b * a.Lk * a.ldk + h * HD;
  const TM* vbase = reinterpret_cast<const TM*>(a.v) + (size_t)b * a.Lk * a.ldv + h * HD;
  const float* bias = a.bias ? a.bias + (size_t)b * a.Lk : nullptr;

  u32x4_t kraw[UPT], vraw[UPT];
  float braw = 0.f;
  // Rows past Lk are fetched from the LAST valid row instead of being replaced by zeros: their scores carry the -inf of the
  // aux slab whatever K holds (finite), and their probabilities are exactly 0 against any finite V -- so the loads need no
  // per-lane select / zero-fill and no divergent branch.  The mask bias is kept RAW here and scaled in store_tile: scaling it
  // at load time made the compiler wait for this tile's whole prefetch (s_waitcnt vmcnt(0)) in front of the MFMAs.
  auto load_tile = [&](int t) __attribute__((always_inline)) {
    const int key0 = t * KEYS;
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int u = tid + 256 * i;
      if (u < NPIECE) {
        {  // K: row-major pieces, coalesced along d
          const int key = u / PPR, pc = u - key * PPR;
          const int kk = min(key0 + key, Lkb - 1);
          kraw[i] = *reinterpret_cast<const u32x4_t*>(kbase + (size_t)kk * a.ldk + pc * EPC);
        }
        {  // V: key-fastest pieces (the transposed LDS write is then conflict-free)
          const int key = u % KEYS, pc = u / KEYS;
          const int kk = min(key0 + key, Lkb - 1);
          vraw[i] = *reinterpret_cast<const u32x4_t*>(vbase + (size_t)kk * a.ldv + pc * EPC);
        }
      }
    }
    if (tid < KEYS && bias) braw = bias[min(key0 + tid, Lkb - 1)];
  };
  auto store_tile = [&](int stage, int key0s) __attribute__((always_inline)) {
    char* Ks = smem + stage * STAGE;
    char* Vs = Ks + KBYTES;
#pragma unroll
    for (int i = 0; i < UPT; ++i) {
      const int u = tid + 256 * i;
      if (u < NPIECE) {
        G::store_k_piece(Ks, u, kraw[i]);
        G::store_v_piece(Vs, u, vraw[i]);
      }
    }
    if (tid < KEYS) {                                 // K aux element 1 = bias(key) in log2 units; -inf for the keys past Lk
      const float bl = (key0s + tid < Lkb) ? (bias ? braw * LOG2E : 0.f) : -INFINITY;
      *reinterpret_cast<TM*>(Ks + tid * KROWB + HD * SZ + SZ) = op_from_float<TM>(bl);
    }
  };

  f32x16_t o[DT];
  const int ntile = (Lkb + KEYS - 1) / KEYS;
  // OPT (r3, 16-bit operand types without the fp8 PV): the per-tile maximum (16 v_max3 + a lane exchange + a vote per tile, ~15 %
  // of the loop's VALU work) only guards the 16-bit range of the probabilities.  The optimistic
  // pass takes the reference from the FIRST tile alone (its maximum + OPT_MARGIN: later scores may exceed the first tile's by
  // 2^(14 + margin) before the check at the end sends the row to the exact pass) and checks nothing afterwards; an overflow (or a
  // row whose probabilities all flushed to zero behind a fully masked first tile) shows up in the denominator, which the PV MFMA
  // accumulates anyway, and sends the whole workgroup through the exact pass below.  Softmax is shift-invariant: both passes are
  // exact up to the rounding of the probabilities.
  constexpr bool OPT = NS2VC_ATTN_OPT && !P8 && sizeof(TM) == 2;
#if defined(NS2VC_ATTN_ABLATE_RESIDENT)     // diagnostic build (wrong results, timing only): every tile reads stage 0 as staged for tile 0 -- no fetch, no LDS
  constexpr bool ABL_RES = HD <= 32 && sizeof(TM) == 2 && !P8 && !MASKED;      // write and no barrier in the loop: the bound of a K/V-resident kernel (hd 16 / 32)
#else
  constexpr bool ABL_RES = false;
#endif
  // `compute` (wave-uniform): false = this wave keeps the accumulators it has and only helps staging the K / V tiles (r4: the exact pass of
  // a workgroup is computed by the waves that hold a failing row; the others would only burn the VALU slots that bound this kernel)
  auto run = [&](auto optimistic, const bool compute) __attribute__((always_inline)) {
  constexpr bool O = decltype(optimistic)::value;
  if (compute) {
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
    m_ref = 0.f;
    qaux = hi == 0 ? aux_chunk<TM>(-m_ref, 1.0f) : u32x4_t{0, 0, 0, 0};
    if constexpr (CINIT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) cinit[r] = 0.f;
    }
  }
  load_tile(0);
  __syncthreads();          // constants written (first pass) / everybody is done with the stages (second pass)
  store_tile(0, 0);
  __syncthreads();

  for (int t = 0; t < ntile; ++t) {
    if (!ABL_RES && t + 1 < ntile) load_tile(t + 1);
    const char* Ks = smem + (ABL_RES ? 0 : (t & 1)) * STAGE;
    const char* Vs = Ks + KBYTES;
    if (compute)      // (the C-operand form: every tile but the one that needs the tail keys' -inf)
      G::template step<O>(Ks, Vs, t, CINIT && !bias && (t + 1 < ntile || Lkb % KEYS == 0), qf, qaux, cinit, m_ref, o, l31, hi);
    if constexpr (!ABL_RES) {
      if (t + 1 < ntile) store_tile((t + 1) & 1, (t + 1) * KEYS);
      __syncthreads();
    }
  }
  };

  constexpr int LB = G::LB, LR = G::LR;
  if (OPT && !g_attn_exact_only && !a.exact_only) {
    run(OptTag<true>{}, true);
    // the denominator of this lane's query (lane half 0 holds it) bounds every probability of the row: below 2^14 none of them
    // reached the fp16 range (the converts SATURATE under MODE.FP16_OVFL, so an overflow would not show up as inf), and it is
    // positive unless every probability flushed to zero -- otherwise the exact pass decides
    const float lq = o[LB][LR];
    const int bad = (hi == 0 && q < Lqb && !(lq > 0.f && lq < 16384.f)) ? 1 : 0;
    const bool wave_bad = __any(bad) != 0;
    if (__syncthreads_or(bad)) {
      if (a.fallbacks && threadIdx.x == 0) atomicAdd(a.fallbacks, 1u);      // (this workgroup stages its tiles twice: counted, ns2vc_unet_attn_fallbacks)
      run(OptTag<false>{}, wave_bad);
    }
  } else {
    run(OptTag<false>{}, true);
  }

  TM* op = reinterpret_cast<TM*>(a.out) + ((size_t)(b * a.Lq + min(q, a.Lq - 1)) * a.ldo + h * HD);
  G::store_out(o, op, hi, q < a.Lq, MASKED && q >= Lqb);      // a row past the item's end (both lane halves agree): exact zeros, whatever its accumulators hold
}

template <typename TM, int HD, int KEYS> static constexpr size_t attn_lds() { return 2 * (size_t)AttnTile<TM, HD, KEYS, false>::STAGE; }

// The compiled set, one row per instantiation: every operand type and head width with 64-key tiles, dense and masked; for the 16-bit
// types the fp8 PV form (dense only) and, at hd 16 / 32, the 128-key tiles.
// 64-key tiles everywhere.  128-key tiles (half the per-tile bookkeeping, barriers and waits; round-1 review item) exist for
// the narrow heads of the 16-bit precisions (hd 16 / 32) behind the tuning hook, and LOSE: same-box 3.93 (64) vs 3.98 ms/step
// (128), attention 0.68 vs 0.73 ms -- 64 more score registers and twice the LDS per workgroup cost more occupancy than the
// bookkeeping saves in a VALU-bound loop.
// (the fp8 variant needs less than attn_lds: its V^T rows are half as long)
#define NS2VC_ATTN_ROW(TM, PREC, HD, KEYS, FP8, MK) \
  {kernel_key(PREC, HD, KEYS, FP8, MK), reinterpret_cast<const void*>(attn_kernel<TM, HD, KEYS, FP8, MK>), (uint32_t)attn_lds<TM, HD, KEYS>(), 256}
#define NS2VC_ATTN_ROW2(TM, PREC, HD, KEYS) NS2VC_ATTN_ROW(TM, PREC, HD, KEYS, false, false), NS2VC_ATTN_ROW(TM, PREC, HD, KEYS, false, true)
#define NS2VC_ATTN_ROWS16(TM, PREC)                                                                                            \
  NS2VC_ATTN_ROW2(TM, PREC, 16, 64), NS2VC_ATTN_ROW2(TM, PREC, 16, 128), NS2VC_ATTN_ROW(TM, PREC, 16, 64, true, false),         \
  NS2VC_ATTN_ROW2(TM, PREC, 32, 64), NS2VC_ATTN_ROW2(TM, PREC, 32, 128), NS2VC_ATTN_ROW(TM, PREC, 32, 64, true, false),         \
  NS2VC_ATTN_ROW2(TM, PREC, 48, 64), NS2VC_ATTN_ROW(TM, PREC, 48, 64, true, false),                                             \
  NS2VC_ATTN_ROW2(TM, PREC, 64, 64), NS2VC_ATTN_ROW(TM, PREC, 64, 64, true, false)
static const KernelRow attn_rows[] = {
  NS2VC_ATTN_ROW2(float, PREC_F32, 16, 64), NS2VC_ATTN_ROW2(float, PREC_F32, 32, 64), NS2VC_ATTN_ROW2(float, PREC_F32, 48, 64), NS2VC_ATTN_ROW2(float, PREC_F32, 64, 64),
  NS2VC_ATTN_ROWS16(bf16_t, PREC_BF16),
  NS2VC_ATTN_ROWS16(f16_t, PREC_F16),
};
#undef NS2VC_ATTN_ROWS16
#undef NS2VC_ATTN_ROW2
#undef NS2VC_ATTN_ROW
static const KernelTable k_attn_table(attn_rows);      // (static: host data, no copy in the code object)
const KernelTable& attn_kernel_table() { return k_attn_table; }

static int g_force_keys = 0;   // test / tuning hook (ns2vc_debug_set_attn_keys): 128 selects the 128-key kernels
void set_forced_attn_keys(int keys) { g_force_keys = keys; }
void set_attn_optimistic(int on) {
  const int v = on ? 0 : 1;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_attn_exact_only), &v, sizeof(v));
  set_attnres_optimistic(on);      // (attn_resident.hip keeps its own copy of the switch: device symbols are per file)
}

hipError_t init_attn_attributes() { return set_lds_all(k_attn_table); }

// would launch_attention run this launch on a masked instantiation, were AttnArgs.q_lens / k_lens set?  (every operand type, head width and key tile;
// not the fp8 PV form: the table says)  The planner asks per launch: an attention refused here keeps its key-bias row and its mask_rows launch.
bool attention_masks_rows(const AttnArgs& a, int head_dim, int prec) {
  return find(k_attn_table, kernel_key(prec, head_dim, 64, a.pv_fp8 != 0, true)) != nullptr;
}

hipError_t launch_attention(const AttnArgs& a, int head_dim, int prec, hipStream_t s, bool resident, bool resident_lens) {
  const int al = prec == PREC_F32 ? 3 : 7;       // rows must start 16-B aligned
  if (!a.q || !a.k || !a.v || !a.out) return hipErrorInvalidValue;
  const bool masked = a.q_lens || a.k_lens, fp8 = a.pv_fp8 != 0;
  if (masked && !attention_masks_rows(a, head_dim, prec)) return hipErrorInvalidValue;     // refused, never run unmasked
  if (a.Lq <= 0 || a.Lk <= 0 || (a.ldq & al) || (a.ldk & al) || (a.ldv & al) || (a.ldo & al)) return hipErrorInvalidValue;
  if (reinterpret_cast<uintptr_t>(a.out) & 15) return hipErrorInvalidValue;      // (results leave in 16-byte pieces)
  if (attention_resident_eligible(a, head_dim, prec, resident)) return launch_attention_resident(a, head_dim, prec, s);      // a head's K/V staged once
  if (masked && attention_resident_lens_eligible(a, head_dim, prec, resident && resident_lens))                               // ... under length tables
    return launch_attention_resident_lens(a, head_dim, prec, s);
  const int keys = !fp8 && g_force_keys == 128 && find(k_attn_table, kernel_key(prec, head_dim, 128, false, masked)) ? 128 : 64;
  const KernelRow* row = find(k_attn_table, kernel_key(prec, head_dim, keys, fp8, masked));      // (no row: fp8 PV at fp32, or masked)
  if (!row) return hipErrorInvalidValue;
  return launch(*row, dim3(((a.Lq + 127) / 128) * a.H * a.B), s, a);      // (const AttnArgs)
}

}  // namespace ns2vc
