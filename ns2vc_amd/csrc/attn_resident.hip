// K/V-resident attention for the narrow heads (hd 16 / 32, fp16 / bf16, dense): one workgroup = 16 waves = one (item, head).
//
// attn_kernel (attn.hip) gives 128 queries of a head to a 4-wave workgroup that streams ALL the head's K/V tiles through a two-stage LDS ring: at the
// level-0 self-attention (Lq = Lk = 938) eight workgroups fetch, transpose and write every tile of their head, and per wave-tile about half of the
// instructions issued are staging (fetch, V transpose, LDS writes, waits, one barrier).  Here the head's K and V^T are staged ONCE, into ntile stages of
// exactly attn_kernel's stage layout, and after one barrier every wave walks query tiles w, w+16, w+32, ... (32 queries each) over all key tiles with the
// shared tile arithmetic of attn_common.h -- no fetch, no LDS write, no barrier in the loop.  Same operands in the same order: the results are
// attn_kernel's, bit for bit, in the accepted and in the rejected optimistic case (a wave whose rows fail the denominator check repeats its own query
// tile with the exact pass: nothing is restaged, so no other wave takes part).
// Capacity follows from the layout and the 160 KB of LDS: hd 16 -> 16 tiles (1024 keys, 152 KiB), hd 32 -> 10 tiles (640 keys, 160 KiB).
// Everything else (fp32, the fp8 PV form, masked launches, hd 48 / 64, more keys, small grids) keeps attn_kernel: attention_resident_eligible.
// Launches under per-item length tables (AttnArgs.q_lens / k_lens) have the same kernel body with the item's own counts, attnres_lens_kernel, behind a plan
// option of its own (masked_attn_resident, default 0) and its own predicate, attention_resident_lens_eligible: the bits and the fallback count are the
// masked attn_kernel's.  Measured: profiles/r22_masked_attn_resident.txt, DESIGN.md 4.7.
#include "attn_common.h"
#include "kernel_table.h"
#include <atomic>

namespace ns2vc {

// test hook (ns2vc_debug_set_attn_optimistic; attn.hip forwards it): 1 = the exact pass only
__device__ int g_attnres_exact_only = 0;

constexpr int ATTNRES_LDS = 160 * 1024;
constexpr int ATTNRES_WAVES = 16;
constexpr int ATTNRES_MAX_QBLOCKS = 256;       // fallback flags live in the 64 x 16 B of row pads of stage 0's K rows: one word per 128-query block

template <typename TM, int HD> struct AttnResGeom {
  using G = AttnTile<TM, HD, 64, false>;
  static constexpr int MAXT = ATTNRES_LDS / G::STAGE;             // stages that fit
  static constexpr int TPP = 1024 / G::NPIECE;                    // tiles one pass of the 1024 threads fetches (a K and a V piece per thread)
  static constexpr int NPASS = (MAXT + TPP - 1) / TPP;
  static_assert(1024 % G::NPIECE == 0 && MAXT * 64 <= 1024, "one thread per staged key row");
};

// the count of item b from a length table of the masked form, clamped to [lo, hi]; hi without a table and in the dense form
template <bool MASKED> __device__ __forceinline__ int attnres_count(const int32_t* lens, int b, int lo, int hi) {
  if constexpr (MASKED) {
    if (lens) return min(max(lens[b], lo), hi);
  }
  return hi;
}
// exact zeros into rows row0 .. Lq-1 of head h of item b of `out` (16-B pieces, the whole workgroup): the rows behind an item's live query tiles (the
// partial tile's own rows past the item's end leave through store_out)
template <typename TM, int HD> __device__ __forceinline__ void attnres_zero_rows(const AttnArgs& a, int b, int h, int row0, int tid) {
  constexpr int SZ = sizeof(TM), PPR = HD * SZ / 16;
  char* zp = reinterpret_cast<char*>(a.out) + ((size_t)b * a.Lq * a.ldo + h * HD) * SZ;
  for (int i = tid; i < (a.Lq - row0) * PPR; i += 1024) {
    const int row = row0 + i / PPR, pc = i % PPR;
    *reinterpret_cast<u32x4_t*>(zp + (size_t)row * a.ldo * SZ + pc * 16) = u32x4_t{0, 0, 0, 0};
  }
}

// The body of both kernels.  MASKED: per-item query and key counts (AttnArgs.q_lens / k_lens), the rule of attn_kernel<..., MASKED>: the item's counts
// Lqb / Lkb (workgroup-uniform, clamped to the tensor) stand wherever the dense form uses Lq / Lk, the row stride between items stays Lq / Lk.  Key side:
// only the ceil(Lkb / 64) tiles the item has are staged, nothing of k / v at or past row Lkb is read.  Query side: only the ceil(Lqb / 32) live query
// tiles are walked; the rows of the partial tile past Lqb enter as zeros, decide no repeat and leave as exact zeros, and every other row of [Lqb, Lq) is
// stored as zeros by the whole workgroup without a fetch or an MFMA (an item with no query at all does that and returns before it stages anything).
template <typename TM, int HD, bool MASKED>
__device__ __forceinline__ void attnres_body(const AttnArgs& a) {
  op_mode_init<TM>();
  using R = AttnResGeom<TM, HD>;
  using G = typename R::G;
  constexpr int KEYS = 64, SZ = G::SZ, EPC = G::EPC, NS = G::NS, KROWB = G::KROWB, VROWB = G::VROWB, DT = G::DT, KBYTES = G::KBYTES, STAGE = G::STAGE,
                PPR = G::PPR, NPIECE = G::NPIECE, HDX = G::HDX;
  constexpr int TPP = R::TPP, NPASS = R::NPASS;
  static_assert(SZ == 2, "16-bit operand types");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  // XCD-aware mapping (as attn_kernel): every XCD gets a contiguous run of (item, head), so the heads of an item, which share K/V rows, share an L2
  int b, h;
  {
    const int nwg = gridDim.x, bid = blockIdx.x;
    const int qn = nwg >> 3, rn = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    const int swz = (xcd < rn ? xcd * (qn + 1) : rn * (qn + 1) + (xcd - rn) * qn) + idx;
    b = swz / a.H;
    h = swz - b * a.H;
  }
  const int Lq = a.Lq, Lk = a.Lk;
  // this item's query / key counts (clamped to the tensor: a bad table cannot send a fetch or a store outside it)
  const int Lqb = attnres_count<MASKED>(a.q_lens, b, 0, Lq), Lkb = attnres_count<MASKED>(a.k_lens, b, 1, Lk);
  if constexpr (MASKED) {
    if (Lqb == 0) {                                   // nothing but padded queries: their zeros, and no K / V tile, no MFMA
      attnres_zero_rows<TM, HD>(a, b, h, 0, tid);
      return;
    }
  }
  const int ntile = (Lkb + KEYS - 1) / KEYS;          // <= MAXT (attention_resident_eligible / attention_resident_lens_eligible)
  const float LOG2E = 1.4426950408889634f;
  const float sc2 = a.scale * LOG2E;                  // scores are kept in log2 units

  // ---- stage the whole head.  Every byte a fragment read touches is written exactly once, by one thread, so one barrier closes the prologue:
  //   K rows: HD elements by the K pieces; the aux slab {1, bias(key) | -inf, 0 ...} and the pad by the key's thread
  //   V^T:    rows 0 .. HD-1 by the V pieces (all 64 key slots: rows past the item's Lkb are fetched from its last valid row, as in attn_kernel), the ones row by the
  //           key's thread, rows HD+1 .. HDX-1 zeroed here (the row pads are never read)
  {
    const TM* kbase = reinterpret_cast<const TM*>(a.k) + (size_t)b * Lk * a.ldk + h * HD;
    const TM* vbase = reinterpret_cast<const TM*>(a.v) + (size_t)b * Lk * a.ldv + h * HD;
    const float* bias = a.bias ? a.bias + (size_t)b * Lk : nullptr;
    const int u = tid % NPIECE, tsub = tid / NPIECE;
    u32x4_t kraw[NPASS], vraw[NPASS];
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {                 // the loads of all passes in flight before the first store
      const int t = tsub + i * TPP;
      if (t < ntile) {
        {
          const int key = u / PPR, pc = u - key * PPR;
          const int kk = min(t * KEYS + key, Lkb - 1);
          kraw[i] = *reinterpret_cast<const u32x4_t*>(kbase + (size_t)kk * a.ldk + pc * EPC);
        }
        {
          const int key = u % KEYS, pc = u / KEYS;
          const int kk = min(t * KEYS + key, Lkb - 1);
          vraw[i] = *reinterpret_cast<const u32x4_t*>(vbase + (size_t)kk * a.ldv + pc * EPC);
        }
      }
    }
    float braw = 0.f;
    const bool keyrow = tid < ntile * KEYS;           // thread tid owns key row tid of the head (stage tid / 64, row tid % 64)
    if (keyrow && bias) braw = bias[min(tid, Lkb - 1)];
    constexpr int NZC = (HDX - HD - 1) * (KEYS * SZ / 16);        // 16-B chunks of one stage's V^T zero rows
    for (int i = tid; i < ntile * NZC; i += 1024) {
      const int t = i / NZC, r = i - t * NZC;
      *reinterpret_cast<u32x4_t*>(smem + t * STAGE + KBYTES + (HD + 1 + r / 8) * VROWB + (r & 7) * 16) = u32x4_t{0, 0, 0, 0};
    }
    if (keyrow) {
      const int st = tid / KEYS, key = tid - st * KEYS;
      const float bl = tid < Lkb ? (bias ? braw * LOG2E : 0.f) : -INFINITY;      // bias(key) in log2 units; -inf for the keys past the item's Lkb
      char* aux = smem + st * STAGE + key * KROWB + HD * SZ;
      *reinterpret_cast<u32x4_t*>(aux) = aux_chunk<TM>(1.0f, bl);
      *reinterpret_cast<u32x4_t*>(aux + 16) = u32x4_t{0, 0, 0, 0};
      *reinterpret_cast<u32x4_t*>(aux + 32) = u32x4_t{0, 0, 0, 0};               // (the pad: stage 0's holds the fallback flags)
      *reinterpret_cast<TM*>(smem + st * STAGE + KBYTES + HD * VROWB + key * SZ) = op_from_float<TM>(1.0f);
    }
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
      const int t = tsub + i * TPP;
      if (t < ntile) {
        G::store_k_piece(smem + t * STAGE, u, kraw[i]);
        G::store_v_piece(smem + t * STAGE + KBYTES, u, vraw[i]);
      }
    }
  }
  __syncthreads();

  const bool cform_all = G::CINIT && !a.bias;
  const bool exact_only = !NS2VC_ATTN_OPT || g_attnres_exact_only || a.exact_only;
  const int nqt = (Lqb + 31) >> 5;                               // the live query tiles
  for (int qt = wave; qt < nqt; qt += ATTNRES_WAVES) {          // a wave with no live query tile goes straight to the final barrier
    const int q = qt * 32 + l31;
    u32x4_t qf[NS];
    // (fetching the first tile's rows in front of the staging loads, and a round's rows under the loop of the round before, was measured and lost
    //  0.45 % of the step: profiles/r21_attn_resident.txt)
    G::load_q(qf, reinterpret_cast<const TM*>(a.q) + ((size_t)(b * Lq + min(q, Lqb - 1)) * a.ldq + h * HD), sc2, hi, q >= Lqb);
    float m_ref;
    u32x4_t qaux;
    f32x16_t cinit, o[DT];
    auto run = [&](auto optimistic) __attribute__((always_inline)) {
      constexpr bool O = decltype(optimistic)::value;
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
      m_ref = 0.f;
      qaux = hi == 0 ? aux_chunk<TM>(-m_ref, 1.0f) : u32x4_t{0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < 16; ++r) cinit[r] = 0.f;
      for (int t = 0; t < ntile; ++t) {
        const char* Ks = smem + t * STAGE;
        G::template step<O>(Ks, Ks + KBYTES, t, cform_all && (t + 1 < ntile || Lkb % KEYS == 0), qf, qaux, cinit, m_ref, o, l31, hi);
      }
    };
    if (!exact_only) {
      run(OptTag<true>{});
      // the denominator check of attn_kernel, decided per wave: a failing row sends this wave's 32 queries through the exact pass
      const float lq = o[G::LB][G::LR];
      const int bad = (hi == 0 && q < Lqb && !(lq > 0.f && lq < 16384.f)) ? 1 : 0;
      if (__any(bad)) {
        if (lane == 0) *reinterpret_cast<uint32_t*>(smem + (qt >> 4) * KROWB + HD * SZ + 32 + ((qt >> 2) & 3) * 4) = 1u;      // block qt / 4: row blk / 4, word blk % 4
        run(OptTag<false>{});
      }
    } else {
      run(OptTag<false>{});
    }
    TM* op = reinterpret_cast<TM*>(a.out) + ((size_t)(b * Lq + min(q, Lq - 1)) * a.ldo + h * HD);
    G::store_out(o, op, hi, q < Lq, MASKED && q >= Lqb);      // a row past the item's end (both lane halves agree): exact zeros
  }
  if constexpr (MASKED) attnres_zero_rows<TM, HD>(a, b, h, nqt * 32, tid);      // (a wave with no live query tile begins here while the others compute)

  // ---- fallbacks: + 1 per 128-query block (query tiles 4j .. 4j+3) in which a row took the exact pass -- attn_kernel's unit, one workgroup there
  if (a.fallbacks && !exact_only) {         // (workgroup-uniform)
    __syncthreads();
    if (tid == 0) {
      unsigned n = 0;
      const int nqb = (Lqb + 127) >> 7;                        // the live 128-query blocks
      for (int j = 0; j < nqb; ++j) n += *reinterpret_cast<const uint32_t*>(smem + (j >> 2) * KROWB + HD * SZ + 32 + (j & 3) * 4);
      if (n) atomicAdd(a.fallbacks, n);
    }
  }
}

template <typename TM, int HD>
__global__ __launch_bounds__(1024) void attnres_kernel(const AttnArgs a) { attnres_body<TM, HD, false>(a); }
// the same under per-item counts (options masked_attn + masked_attn_resident).  Its own template: the dense instantiations keep their instructions
template <typename TM, int HD>
__global__ __launch_bounds__(1024) void attnres_lens_kernel(const AttnArgs a) { attnres_body<TM, HD, true>(a); }

#define NS2VC_ATTNRES_ROW(TM, PREC, HD) {kernel_key(PREC, HD), reinterpret_cast<const void*>(attnres_kernel<TM, HD>), (uint32_t)ATTNRES_LDS, 1024}
static const KernelRow attnres_rows[] = {
  NS2VC_ATTNRES_ROW(bf16_t, PREC_BF16, 16), NS2VC_ATTNRES_ROW(bf16_t, PREC_BF16, 32),
  NS2VC_ATTNRES_ROW(f16_t, PREC_F16, 16), NS2VC_ATTNRES_ROW(f16_t, PREC_F16, 32),
};
#undef NS2VC_ATTNRES_ROW
static const KernelTable k_attnres_table(attnres_rows);
const KernelTable& attnres_kernel_table() { return k_attnres_table; }
#define NS2VC_ATTNRES_LENS_ROW(TM, PREC, HD) \
  {kernel_key(PREC, HD), reinterpret_cast<const void*>(attnres_lens_kernel<TM, HD>), (uint32_t)ATTNRES_LDS, 1024}
static const KernelRow attnres_lens_rows[] = {
  NS2VC_ATTNRES_LENS_ROW(bf16_t, PREC_BF16, 16), NS2VC_ATTNRES_LENS_ROW(bf16_t, PREC_BF16, 32),
  NS2VC_ATTNRES_LENS_ROW(f16_t, PREC_F16, 16), NS2VC_ATTNRES_LENS_ROW(f16_t, PREC_F16, 32),
};
#undef NS2VC_ATTNRES_LENS_ROW
static const KernelTable k_attnres_lens_table(attnres_lens_rows);
const KernelTable& attnres_lens_kernel_table() { return k_attnres_lens_table; }
static int g_min_grid = 256;          // the rule's threshold: one workgroup per CU of the device (init_attnres_attributes)
hipError_t init_attnres_attributes() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) g_min_grid = cus;
  const hipError_t e = set_lds_all(k_attnres_table);
  return e != hipSuccess ? e : set_lds_all(k_attnres_lens_table);
}

void set_attnres_optimistic(int on) { const int v = on ? 0 : 1; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_attnres_exact_only), &v, sizeof(v)); }

static int g_resident_mode = -1;      // test / tuning hook (ns2vc_debug_set_attn_resident): -1 = the rule, 0 = never, 1 = whenever the launch fits
void set_attn_resident_mode(int mode) { g_resident_mode = mode; }

static int resident_max_tiles(int head_dim, int prec) {
  if (prec == PREC_BF16) return head_dim == 16 ? AttnResGeom<bf16_t, 16>::MAXT : head_dim == 32 ? AttnResGeom<bf16_t, 32>::MAXT : 0;
  if (prec == PREC_F16) return head_dim == 16 ? AttnResGeom<f16_t, 16>::MAXT : head_dim == 32 ? AttnResGeom<f16_t, 32>::MAXT : 0;
  return 0;
}
// does this launch run on attnres_kernel?  dense 16-bit, hd 16 / 32, every key tile of the head resident in LDS, at most ATTNRES_MAX_QBLOCKS query
// blocks (the fallback flags), and -- under the rule -- a grid of at least one workgroup per CU: below it attn_kernel's 4-wave workgroups (eight per head
// at level 0) fill the chip better than B*H workgroups of 16 waves.  `allow` is the plan's option attn_resident.
bool attention_resident_eligible(const AttnArgs& a, int head_dim, int prec, bool allow) {
  if (!allow || g_resident_mode == 0) return false;
  if (a.q_lens || a.k_lens || a.pv_fp8) return false;
  if (!find(k_attnres_table, kernel_key(prec, head_dim))) return false;
  if ((a.Lk + 63) / 64 > resident_max_tiles(head_dim, prec) || (a.Lq + 127) / 128 > ATTNRES_MAX_QBLOCKS) return false;
  if (g_resident_mode == 1) return true;
  return (long long)a.B * a.H >= g_min_grid;
}

static int g_resident_lens_mode = -1; // ns2vc_debug_set_attn_resident_lens: the same three modes for the launches under length tables
void set_attn_resident_lens_mode(int mode) { g_resident_lens_mode = mode; }
// does this launch run on attnres_lens_kernel?  A launch under q_lens / k_lens that attention_resident_eligible would take without them.  The capacity is
// asked of the PADDED Lk (the tables live on the device: the host does not know the counts), and the rule is the dense one.  With B*H workgroups in one
// round the launch lasts as long as its longest item; at lengths of 470 .. 938 frames it was still the faster kernel (profiles/r22_masked_attn_resident.txt),
// a batch of a few long and many very short items was not measured.  `allow`: the plan has both attn_resident and masked_attn_resident on.
bool attention_resident_lens_eligible(const AttnArgs& a, int head_dim, int prec, bool allow) {
  if (!allow || g_resident_lens_mode == 0) return false;
  if (!(a.q_lens || a.k_lens) || a.pv_fp8) return false;
  if (!find(k_attnres_lens_table, kernel_key(prec, head_dim))) return false;
  if ((a.Lk + 63) / 64 > resident_max_tiles(head_dim, prec) || (a.Lq + 127) / 128 > ATTNRES_MAX_QBLOCKS) return false;
  if (g_resident_lens_mode == 1) return true;
  return (long long)a.B * a.H >= g_min_grid;
}

static std::atomic<unsigned long long> g_resident_launches{0};      // launches issued (or captured) on attnres_kernel: what tests read to see the selection
unsigned long long attn_resident_launches() { return g_resident_launches.load(); }

hipError_t launch_attention_resident(const AttnArgs& a, int head_dim, int prec, hipStream_t s) {
  const KernelRow* row = find(k_attnres_table, kernel_key(prec, head_dim));
  if (!row) return hipErrorInvalidValue;
  ++g_resident_launches;
  return launch(*row, dim3(a.B * a.H), s, a);      // (const AttnArgs)
}

static std::atomic<unsigned long long> g_resident_lens_launches{0}; // ... on attnres_lens_kernel: a counter of its own, the dense one keeps its meaning
unsigned long long attn_resident_lens_launches() { return g_resident_lens_launches.load(); }

hipError_t launch_attention_resident_lens(const AttnArgs& a, int head_dim, int prec, hipStream_t s) {
  const KernelRow* row = find(k_attnres_lens_table, kernel_key(prec, head_dim));
  if (!row) return hipErrorInvalidValue;
  ++g_resident_lens_launches;
  return launch(*row, dim3(a.B * a.H), s, a);      // (const AttnArgs)
}

}  // namespace ns2vc
