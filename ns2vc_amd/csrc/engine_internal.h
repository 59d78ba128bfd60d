// What the host units of libns2vc_hip.so share: the engine state behind the opaque ns2vc_unet handle, the error string of the C ABI, and
// the few functions the units call in one another.  pack.cpp packs weights, plan.cpp builds the launch plan, sampler.cpp runs the captured
// sampling loop, engine.cpp is the engine's own C ABI, abi_kernels.cpp the entry points that take no engine handle.
#pragma once
#include "common.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

namespace ns2vc {

inline thread_local std::string g_err;      // ns2vc_last_error()

inline int fail(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return 1;
}
#define HIPCHK(expr)                                                                                       \
  do {                                                                                                     \
    hipError_t _e = (expr);                                                                                \
    if (_e != hipSuccess) return ns2vc::fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
  } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The form of a solver table, from its rows: SOLVER_ITEM_NOISE with a nonzero column 9, SOLVER_ITEM_HIST2 with a nonzero column 10 or 11.
// No update runs both (SOLVER_ITEM_BOTH): every caller refuses such a table in its own words.
constexpr int SOLVER_ITEM_BOTH = SOLVER_ITEM_NOISE | SOLVER_ITEM_HIST2;
inline int solver_table_form(const float* rows, int n) {
  int flags = 0;
  for (int i = 0; i < n; ++i) {
    const float* r = rows + (size_t)i * NS2VC_NCOEF;
    if (r[9] != 0.f) flags |= SOLVER_ITEM_NOISE;
    if (r[10] != 0.f || r[11] != 0.f) flags |= SOLVER_ITEM_HIST2;
  }
  return flags;
}

// "These SolverItem records are fit to launch" -- the one statement of what the step's kernels trust about them.  Record k is named `who`
// index[k] (NULL: k) in the messages, and that is also its place in `correct`.  rows inside [0, n_rows) and a start >= 0; flags one form; with the
// host's copy of the table (`table`, else NULL) flags = the form of the item's rows; history 2 needs the m_prev2 buffer and noise the seeds --
// no_mprev2 / no_seeds are NULL when the buffer is there, else the caller's words for why it is not; a stochastic item takes no correction,
// neither the loop-wide `mode` nor its own record in `correct` (NULL: none).
inline int solver_items_fit(const char* who, const SolverItem* rec, const int32_t* index, int n, int n_rows, const float* table, const char* no_mprev2,
                            const char* no_seeds, int mode, const ItemCorrect* correct) {
  for (int k = 0; k < n; ++k) {
    const SolverItem& r = rec[k];
    const int b = index ? index[k] : k;
    if (r.row0 < 0 || r.steps <= 0 || r.start < 0 || r.row0 > n_rows - r.steps)
      return fail("%s %d: rows %d + %d outside the table of %d rows, or start %d < 0", who, b, r.row0, r.steps, n_rows, r.start);
    if ((r.flags & ~SOLVER_ITEM_BOTH) || r.flags == SOLVER_ITEM_BOTH)
      return fail("%s %d: flags %d (1 = history 2, 2 = noise; a table with both is not supported)", who, b, r.flags);
    if (table && solver_table_form(table + (size_t)r.row0 * NS2VC_NCOEF, r.steps) != r.flags)
      return fail("%s %d: flags %d, its rows %d .. %d have the form %d (1 = history 2, 2 = noise)", who, b, r.flags, r.row0, r.row0 + r.steps - 1,
                  solver_table_form(table + (size_t)r.row0 * NS2VC_NCOEF, r.steps));
    if ((r.flags & SOLVER_ITEM_HIST2) && no_mprev2) return fail("%s %d runs history 2: %s", who, b, no_mprev2);
    if (!(r.flags & SOLVER_ITEM_NOISE)) continue;
    if (no_seeds) return fail("%s %d is stochastic: %s", who, b, no_seeds);
    const int m = correct ? correct[b].mode : mode;
    if (m != 0)
      return fail("%s %d is stochastic and its x0 correction has mode %d: ddim / ddpm have no correction (set the %s's mode to 0)", who, b, m, who);
  }
  return 0;
}
// the per-item x0 correction records from the ABI's three host arrays, every value checked; dyn: a record in mode 1 exists
inline int item_corrections_from(const int32_t* mode, const float* ratio, const float* max_val, int n, std::vector<ItemCorrect>& rec, bool& dyn) {
  rec.resize((size_t)n);
  dyn = false;
  for (int b = 0; b < n; ++b) {
    if (mode[b] < 0 || mode[b] > 2) return fail("item %d: x0 correction mode %d: 0 (off), 1 (dynamic thresholding) or 2 (clamp)", b, (int)mode[b]);
    if (!(ratio[b] >= 0.f && ratio[b] <= 1.f)) return fail("item %d: dynamic thresholding ratio %g outside [0, 1]", b, (double)ratio[b]);
    if (!(std::isfinite(max_val[b]) && max_val[b] > 0.f)) return fail("item %d: thresholding max_val %g must be finite and > 0", b, (double)max_val[b]);
    rec[(size_t)b] = ItemCorrect{(int)mode[b], ratio[b], max_val[b], 0};
    dyn |= mode[b] == 1;
  }
  return 0;
}

// The held-row list of launch_hold_x0 from a HOST frame mask [n][T] (nonzero = held): list[0] = the count, the rows b * T + t behind the head in
// ascending order; last[b] = item b's last held frame (-1: none).  lens (HOST [n], or NULL = all T): a held frame at or past lens[b] is refused.
inline int hold_list_from_mask(const uint8_t* mask, int n, int T, const int32_t* lens, std::vector<int>& list, std::vector<int32_t>& last) {
  list.assign((size_t)HOLD_LIST_HEAD, 0);
  last.assign((size_t)n, -1);
  for (int b = 0; b < n; ++b)
    for (int t = 0; t < T; ++t) {
      if (!mask[(size_t)b * T + t]) continue;
      if (lens && t >= lens[b]) return fail("known frame %d of item %d lies at or past its length %d", t, b, (int)lens[b]);
      list.push_back(b * T + t);
      last[(size_t)b] = t;
    }
  list[0] = (int)list.size() - HOLD_LIST_HEAD;
  return 0;
}

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
  size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};

struct PackedW {     // device-resident packed GEMM weight
  void* w = nullptr;
  void* wt = nullptr;      // k = 3 convs: the same weights tile-major for conv3ts_kernel (pack_conv3_tiled)
  float* bias = nullptr;
  float* wsum = nullptr;   // [N] row sums of the packed (rounded) weights: LayerNorm-by-linearity consumers only
  int N = 0, K = 0;
};

struct ResnetW {
  std::string prefix;
  int cin = 0, cout = 0, temb_off = 0;
  bool shortcut = false;
  float *n1g = nullptr, *n1b = nullptr, *n2g = nullptr, *n2b = nullptr;
  PackedW conv1, conv2, sc;
};
struct AttnW {
  std::string prefix;
  int dim = 0, kv_off = 0;
  float *ng = nullptr, *nb = nullptr;
  PackedW proj_in, qkv, o1, q2, o2, ff1, ff2, proj_out;
  PackedW ffpo;    // ff.net.2 folded into proj_out: [W_po W_2 | W_po], K = 4*dim + dim (see pack_all)
  void* ffn_pre_stream = nullptr; // the same stream with attn2.to_out in front (pre-stage of the fused kernel)
  void* ffn_stream = nullptr;     // fused feed-forward + proj_out (ffn.hip): weight tile stream ...
  float* ffn_consts = nullptr;    // ... and (rowsum, bias) per packed ff.net.0 row; 16-bit precisions, dim <= 256 only
  void* geglu_stream = nullptr;   // token-stationary GEGLU projection (geglu.hip): weight tile stream and constants; 16-bit precisions, dim 384
  float* geglu_consts = nullptr;
  // token-local chains (rowchain.hip; 16-bit precisions, dim <= 256): proj_in -> norm1 -> q|k|v and attn1.to_out -> norm2 -> attn2.to_q
  void *chain_in = nullptr, *chain_mid = nullptr;          // weight tile streams
  void* chain_in_s2 = nullptr;                              // ... of the first chain packed for two N-slices (dim 384, r4)
  float *chain_in_consts = nullptr, *chain_mid_consts = nullptr;   // (rowsum, bias) per LayerNorm-folded stage-2 row
};
struct BlockW {
  std::string kind;   // down | mid | up
  int index = 0, level = 0, channels = 0;
  std::vector<ResnetW> res;
  std::vector<AttnW> attn;
  int sampler = 0;    // 0 none, 1 down, 2 up
  PackedW samp;
};

struct Op {
  std::string name;
  std::function<hipError_t(hipStream_t)> fn;
  int kind = 0;          // 0 other, 1 implicit GEMM, 2 attention, 3 norm statistics, 4 copy
  double flops = 0.0;    // algorithmic FLOPs (2*MAC) of this launch
  double bytes = 0.0;    // algorithmic (compulsory) HBM bytes: operands read once + result written once
  // what the forward's one clear launch does for THIS op (zero the arrival words of a cooperative GroupNorm prologue): only
  // ns2vc_unet_profile_forward needs it, because it repeats an op without the rest of the forward in between
  std::function<hipError_t(hipStream_t)> rearm;
};
struct Tap {
  std::string name;
  float* copy = nullptr;
  int rows = 0, cols = 0;
};

// Pinned staging for host-to-device copies that must be truly asynchronous: the caller's data is copied into the buffer, the copies out of
// it go on the caller's stream, and an event marks the last of them.  The host waits only for the PREVIOUS call's copy out of the buffer
// (enqueued in front of whatever the caller launched since, so normally long done) -- never for the stream's work behind it.
struct Staged {
  void* buf = nullptr;
  size_t cap = 0;
  hipEvent_t event = nullptr;
  bool pending = false;
  // waits for the previous copy out of the buffer and makes room for `bytes`
  int reserve(size_t bytes) {
    if (!event) HIPCHK(hipEventCreateWithFlags(&event, hipEventDisableTiming));
    if (pending) { HIPCHK(hipEventSynchronize(event)); pending = false; }
    if (cap < bytes) {
      if (buf) HIPCHK(hipHostFree(buf));
      buf = nullptr; cap = 0;
      HIPCHK(hipHostMalloc(&buf, bytes, hipHostMallocDefault));
      cap = bytes;
    }
    return 0;
  }
  // after the copies out of the buffer have been issued on `s`
  int record(hipStream_t s) {
    HIPCHK(hipEventRecord(event, s));
    pending = true;
    return 0;
  }
  ~Staged() {
    if (pending) (void)hipEventSynchronize(event);
    if (event) (void)hipEventDestroy(event);
    if (buf) (void)hipHostFree(buf);
  }
};


void drop_step_graph(::ns2vc_unet* h);      // plan.cpp

// A device table of the sampling loop that lives outside the plan arena and grows on demand: the seeds, the guidance scales, the thresholds, the
// per-item records, the m_{i-2} buffer.  The captured step graph holds its pointer, so a NEW buffer drops the graph; new values in the same buffer
// are a copy from pinned staging on the caller's stream and replay it.  cap is kept a 16-byte multiple (launch_copy16 moves whole tables).
template <typename T> struct StepTable {
  T* dev = nullptr;
  size_t cap = 0;      // elements
  Staged stage;
  static size_t rounded(size_t n) { return sizeof(T) >= 16 ? n : (n + 16 / sizeof(T) - 1) / (16 / sizeof(T)) * (16 / sizeof(T)); }
  // room for n elements: nothing when they fit; else the step graph goes, the device drains, and a new buffer (zeroed with `clear`) replaces the old
  int reserve(::ns2vc_unet* h, size_t n, bool clear) {
    if (dev && cap >= n) return 0;
    drop_step_graph(h);
    if (dev) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(dev)); dev = nullptr; cap = 0; }
    const size_t c = rounded(n);
    HIPCHK(hipMalloc((void**)&dev, c * sizeof(T)));
    if (clear) HIPCHK(hipMemset(dev, 0, c * sizeof(T)));
    cap = c;
    return 0;
  }
  // these n host values into the buffer (room made before), asynchronously on s
  int send(const T* host, size_t n, hipStream_t s) {
    const size_t nb = n * sizeof(T);
    if (stage.reserve(nb)) return 1;
    memcpy(stage.buf, host, nb);
    HIPCHK(hipMemcpyAsync(dev, stage.buf, nb, hipMemcpyHostToDevice, s));
    return stage.record(s);
  }
  ~StepTable() { if (dev) (void)hipFree(dev); }
};

}  // namespace ns2vc

struct ns2vc_unet {
  ns2vc_unet_cfg cfg{};
  std::map<std::string, ns2vc::HostTensor> raw;
  std::vector<std::pair<std::string, std::vector<int64_t>>> expected;
  int prec = -1;
  bool finalized = false;
  std::vector<void*> weight_allocs;

  // packed weights
  std::vector<ns2vc::BlockW> blocks;
  ns2vc::PackedW conv_in_x, conv_in_c, conv_out, temb_all, kv_all, pool_qkv;
  ns2vc::PackedW conv_in_xp, conv_in_cp, conv_outp;                     // r6, 16-bit engines: the first three against hi + lo operand pairs (option split_io; K = 3 x)
  ns2vc::PackedW conv_in_x32, conv_in_c32, conv_out32, temb_all32;      // r6, 16-bit engines: the same four in fp32 (option exact_io)
  float *t_w1t = nullptr, *t_b1 = nullptr, *t_w2t = nullptr, *t_b2 = nullptr;
  float *p_n1g = nullptr, *p_n1b = nullptr, *p_pos = nullptr, *p_projT = nullptr, *p_projb = nullptr, *p_n2g = nullptr, *p_n2b = nullptr;
  float *out_ng = nullptr, *out_nb = nullptr;
  int n_temb = 0, n_kv = 0;
  int CP = 128;       // padded latent channels in the engine's channels-last x buffers

  // workspace / plan
  int B = 0, T = 0, Lp = 0;
  void* arena = nullptr;
  size_t arena_bytes = 0, arena_used = 0;
  std::vector<ns2vc::Op> cond_ops, fwd_ops;
  size_t cond_split = 0;      // cond_ops[0 .. cond_split) depend on the content only, the rest on the prompt (+ mask) only
  bool debug = false;
  int device = 0;             // HIP device the engine (weights, arena, graph) lives on; every entry point binds to it
  // LayerNorm by linearity (csrc/gemm.hip): no normalisation pass; NS2VC_LN_LINEAR=0 (or ns2vc_unet_set_option) restores
  // the ln_apply kernels.  The consumers record max |mean| * rstd over all LayerNorm rows in `ln_health`: the 16-bit
  // modes round the RAW x before centring, so their error on a row grows with that ratio (ns2vc_unet_ln_ratio).
  bool ln_linear = true;
  // ff.net.2 folded into proj_out at pack time (one GEMM with a second K segment instead of two launches; the
  // post-feed-forward stream tensor is never materialised).  NS2VC_FOLD_FF=0 restores the two launches.
  bool fold_ff = true;
  // GEGLU feed-forward + ff.net.2 + proj_out in ONE launch per transformer block (csrc/ffn.hip) where eligible
  // (16-bit precisions, dim 128 / 256, LayerNorm by linearity and the fold on).  NS2VC_FUSE_FFN=0 restores the two GEMMs.
  bool fuse_ffn = true;
  bool fuse_rows = true;     // proj_in+q|k|v and attn1.to_out+attn2.to_q as one launch each (rowchain.hip)
  bool attn_fp8 = false;     // PV product of every attention on the fp8 MFMA (16-bit precisions; BASELINE config 5's fp8 path; costs parity)
  bool fuse_ffn_pre = true;  // attn2.to_out + residual computed inside the fused feed-forward kernel
  bool fuse_geglu = true;    // r5: token-stationary GEGLU projection (csrc/geglu.hip) where the fused feed-forward does not apply (dim 384)
  bool fuse_rows_gn = true;  // ... and the transformer's GroupNorm computed in the prologue of the first of them
  // GroupNorm-apply as the prologue of the GEMM that consumes it (gemm.hip gn_prologue, ns2vc_gemm_args.gnp_*) wherever the norm has
  // one source, one consumer and epilogue statistics: resnet norm2 -> conv2, norm1 -> conv1 of the resnets without a
  // shortcut, the transformer norm in front of a plain proj_in, conv_norm_out -> conv_out.  Bit-identical to the gn_apply
  // launches it removes (210 -> 174 launches at the bench shape).  NS2VC_FUSE_GN_GEMM=0 restores them.  (r3 had this off: not
  // run-to-run deterministic; root cause and fix in r4, profiles/r04_gn_prologue_rootcause.txt.)
  bool fuse_gn_gemm = true;
  bool fuse_gn_cat = true;                // ... also where the norm's input is a concat of two tensors and / or a raw operand copy is wanted (first resnet of a level, up blocks)
  bool gn_coop = true;                    // the column tiles of one row block split the GroupNorm prologue's rows between them (ns2vc_gemm_args.gnp_sync)
  bool conv_ts = true;         // k = 3 convolutions on the tap-sharing kernel (convts.hip, r5)
  bool conv_wtiled = true;     // ... reading tile-major weights (PackedW.wt)
  bool split_io = true;       // r6 (16-bit engines): conv_in and conv_out -- 23 % of the forward error's energy in two launches (profiles/r06_error_budget.txt) -- on hi + lo operand
                              //   pairs: x * w ~= hi(x) hi(w) + lo(x) hi(w) + hi(x) lo(w), three times the K of two small convolutions instead of their fp32 MFMA rate (exact_io)
                              //   ON: forward error 8.08e-4 -> 7.10e-4 at the bench shape for +0.3 % of the step (profiles/r06_ab_split_io.txt)
  bool exact_io = false;       // r6 (16-bit engines): conv_in, conv_out and the time_emb_proj GEMM -- three single launches that carry 23 + 6 % of the forward error's energy
                               // (profiles/r06_error_budget.txt) -- with fp32 operands on the fp32 MFMA: a precision-for-time knob
  float* content_f32 = nullptr;      // ... their fp32 inputs: the content rows, SiLU(emb)
  float* emb_act_f32 = nullptr;
  int conv_out_prec = -1;
  bool fork_temb = false;      // (measured: +3 % -- a graph with a parallel branch replays SLOWER than the linear chain, 3.696 vs 3.587 ms/step, profiles/r06_ab_fork_temb.txt; off)
                               // r6: inside the captured step graph the timestep-embedding branch (time_embed + time_emb_proj.all: two small launches that depend on the step
                               // counter only) runs BESIDE conv_in and the first resnet's conv1 on a forked stream and joins in front of the first consumer of the scale / shift rows
  struct TembFork {
    int begin = -1, end = -1, join = -1;     // ... their places in fwd_ops (build_plan)
    int first = -1, readers = 0;             // the first launch that reads the scale / shift rows (fused GEMM prologue OR stand-alone gn_apply) and how many do
    bool ok = false;                         // plan-build invariant: no reader sits in front of `join` (otherwise the fork is refused; ns2vc_unet_op_info which = 2)
    int join_skip = 0;                       // tests (set_option "temb_join_skip"): readers passed over when the join is recorded -- forces the refusal
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  } tfork;
  bool fuse_xattn = false;     // the prompt cross-attention of attn2 runs inside the fused feed-forward kernel (ffn.hip ATT, r6): no attn2.sdpa launch at dim 128 / 256.
                               // Correct (kernel + engine tests), 10 launches fewer, measured SLOWER (3.53 vs 3.39 ms/step; profiles/r06_ab_fuse_xattn.txt): with 8 waves per workgroup
                               // (2 per SIMD, 212-252 VGPRs) the attention phase runs 2-3x off its VALU bound -- a tested option, off
  bool fuse_solver = false;    // the sampling loop's solver update runs in conv_out's epilogue (GemmArgs.sol_*, r6) instead of as its own launch: bit-identical,
                               // one launch and 88 MB of HBM traffic less per step, but 0.1-0.4 % SLOWER in three same-box A/Bs (profiles/r06_ab_fuse_solver.txt) -- a tested option, off
  ns2vc::GemmArgs conv_out_g;         // ... conv_out's launch arguments and its place in fwd_ops, kept by build_plan for that
  int conv_out_idx = -1;
  bool warned_wtiled = false;
  int bn128_min = 160;         // workgroups a 128-column tap-sharing tiling must still give on THIS engine's device (5/8 of its CUs); per engine, not process-global
  bool gn_inloop = false;      // ... normalising inside its K loop (gnpro.h GnInloop, r6) instead of materialising the rows in a prologue (GemmArgs.algo 0 vs 2).
                               // Bit-identical results, measured SLOWER (profiles/r06_ab_gn_inloop.txt: 3.85 vs 3.61 ms/step; SiLU of a 128 x 64 chunk is 1.7 k VALU cycles per SIMD,
                               // more than the consumers need for the chunk, and every column tile repeats it): a tested option, off
  int gn_coop_min = 2;         // fewest column tiles of a row block for which the cooperative prologue is used (tuning: NS2VC_GN_COOP_MIN under NS2VC_DEBUG_ENV)
  int cus = 256;               // compute units of this device (hipDeviceProp_t.multiProcessorCount): the "one round of workgroups" heuristics scale with it
  int xcd_probe = -1;          // misc.hip's placement probe of this device: 1 = workgroup ids 8 apart share an XCD
  bool slice_rows = true;      // first row chain of a dim-384 block as two N-slices per token block (r4; see Planner::transformer)
  unsigned* ln_health = nullptr;
  bool attn_optimistic = true;   // attention without the per-tile maximum + exact fallback (attn.hip OPT); 0 = exact pass only, on every device
  bool attn_resident = true;     // dense 16-bit attention at hd 16 / 32 on the K/V-resident kernel where launch_attention's rule selects it (attn_resident.hip); 0 = attn_kernel everywhere
  unsigned* attn_fallbacks = nullptr;     // device counter: workgroups that needed the fallback (ns2vc_unet_attn_fallbacks)
  unsigned long long coef_hash = 0;       // FNV-1a of the loaded solver table (handoff compares)
  std::vector<ns2vc::Tap> taps;
  bool has_mask = false;
  // Option masked_fuse (off): a plan built under per-item lengths keeps the dense plan's fused launches wherever the kernel has a masked form
  // (GemmArgs.lens: the tap-sharing conv kernel with its GroupNorm prologue, the 8-wave GEMM kernel's epilogue) -- those launches keep the
  // rows past an item's end zero and out of the epilogue statistics themselves, so their gn_partial / mask_rows launches go away.  What
  // has no masked form yet keeps today's unfused launches: the transformer's token-local kernels (row chains, fused feed-forward / GEGLU,
  // LayerNorm by linearity), the attention's result rows, GEMMs on the 4-wave kernel, the nearest upsampling.  Dense plans ignore it.
  bool masked_fuse = false;
  // Option masked_attn (off): under per-item lengths the attention launches get the level's length table (AttnArgs.q_lens, and k_lens for the
  // self-attention) instead of the key-bias row and the mask_rows launch behind them: the keys, key tiles and query tiles past an item's end are
  // skipped, not computed and thrown away.  Asked per launch (attention_masks_rows): the fp8 PV form keeps the bias row and its sweeper.
  // Independent of masked_fuse; dense plans ignore it.  Under per-item PROMPT lengths (plens below) it also hands attn2 the prompt table as k_lens
  // instead of the bias row.
  bool masked_attn = false;
  // Option masked_rows (off): under per-item lengths a transformer block keeps its two row-chain launches (rowchain.hip), which get the level's
  // length table (ns2vc_rowchain_args.lens): a lane of that kernel owns one token, so the rows past an item's end are zero rows by a per-lane
  // predicate and the LayerNorm statistics that forbid LayerNorm by linearity under lengths never leave the kernel.  Replaces the GroupNorm apply
  // (with masked_fuse, where the producer's statistics survive), proj_in, norm1, attn1.qkv, attn1.to_out, norm2, attn2.to_q and their mask_rows
  // launches; norm3 and everything behind it stay as they are.  Asked per launch (rowchain_masks_rows).  Independent of masked_fuse and
  // masked_attn; dense plans ignore it.
  bool masked_rows = false;
  // Option masked_ffn (off): under per-item lengths a transformer block of dim 128 / 256 keeps the pre-stage launch of the fused feed-forward
  // (ffn.hip), which gets the level's length table (ns2vc_ffn_args.lens).  In that form the kernel computes the LayerNorm sums of norm3 itself, so it
  // needs no LayerNorm-by-linearity producer, and a lane owns one token: a row past an item's end is a zero row by a per-lane predicate, stored as
  // exact zeros, left out of the GroupNorm statistics of the result.  Replaces attn2.to_out, norm3, ff.geglu, ff.out+proj_out and their mask_rows
  // launches; the plain form (whose ln_stats would need a masked producer), dim 384 / 512 and levels under 64 frames stay as they are.  Asked per
  // launch (ffn_masks_rows).  Independent of masked_fuse, masked_attn and masked_rows; dense plans and the fp32 engine ignore it.
  bool masked_ffn = false;
  // Option masked_geglu (off): under per-item lengths a dim-384 transformer block on a level of at least g_geglu_min_rows rows keeps the
  // token-stationary GEGLU launch (geglu.hip), which gets the level's length table (ns2vc_geglu_args.T, lens) and no ln_stats: its masked
  // instantiation takes the LayerNorm sums of norm3 from the operand rows it holds in registers, so it needs no LayerNorm-by-linearity producer, and
  // stores the rows past an item's end as exact zeros.  Replaces norm3 and the plain GEGLU GEMM with its mask_rows launch; attn2.to_out (raw operand
  // copy to qb) and ff.out+proj_out stay as they are.  Asked per launch (geglu_masks_rows).  Independent of the four options above; dense plans and
  // the fp32 engine ignore it.
  bool masked_geglu = false;
  // Option masked_attn_resident (off): the attention launches that masked_attn has given a length table run on the K/V-resident kernel's masked form
  // (attnres_lens_kernel) where launch_attention's rule selects it (attention_resident_lens_eligible: hd 16 / 32, 16-bit, the padded key rows fit the
  // LDS, B * heads >= the CUs) and attn_resident is on.  Same bits, same launches.  On its own (masked_attn or attn_resident off, a dense plan) it does nothing.
  bool masked_attn_resident = false;
  // Per-item valid lengths (ns2vc_unet_set_lengths).  `masked`: the plan was built for them -- GroupNorm statistics by their own pass over
  // rows whose padding is zero (no epilogue sums, so no fused GroupNorm prologue, row chain or LayerNorm by linearity), every activation's
  // rows past an item's end zeroed after the launch that writes them, the self-attention keys there masked by an additive bias row, the
  // nearest upsampling materialised.  The tables live in the arena at a place that does not depend on the plan, so new lengths for the same
  // padded shape are a copy on the caller's stream: a captured step graph stays valid.
  struct Lengths {
    bool masked = false;
    int* dev = nullptr;                    // [n_levels][B] valid frames per level and item
    size_t off = 0;                        // arena offset of the two tables
    float* selfbias = nullptr;             // per level l: [B][T_l] additive self-attention key bias (0 | -10000), levels back to back
    std::vector<int32_t> applied;          // the lengths the tables hold (a repeat of them copies nothing)
    ns2vc::Staged stage;                   // pinned staging of both tables for the asynchronous copies
  } lens;
  // Per-item prompt lengths (ns2vc_unet_set_prompt_lengths).  `on`: the plan was built for them -- the prompt copy zeroed past an item's frames on
  // entry, both attention poolings of add_embedding over the item's own frames, and attn2 of every block reading either the table (k_lens, option
  // masked_attn) or the bias row h->maskbias, which then also drops the keys past an item's frames.  The table sits behind the length tables above,
  // at a place that does not depend on the plan: new lengths for the same shape are a copy and the bias-row launch, a captured graph stays valid.
  struct PromptLengths {
    bool on = false;
    int* dev = nullptr;                    // [B] prompt frames per item
    std::vector<int32_t> applied;          // the lengths the table holds (a repeat of them copies nothing)
    ns2vc::Staged stage;
  } plens;
  // Per-item noise seeds of the stochastic samplers (ns2vc_sampler_set_seeds): a buffer of its own (the captured step graph reads it, so new
  // seeds are a copy into it), pinned staging as for the lengths.
  struct Seeds : ns2vc::StepTable<unsigned long long> {
    bool set = false;                      // set since the last prepare
  } seeds;
  bool stochastic = false;                 // the loaded table has a nonzero noise column
  // Classifier-free guidance (ns2vc_sampler_set_guidance): the engine is prepared for B = 2n items, rows [0, n*T) the unconditional half and
  // [n*T, 2n*T) the conditional one; the loop's entry points take and give n items and the update combines the halves by the per-item scales.
  // The scales live in a buffer of their own as the seeds do (new values are a copy, the captured step graph stays valid).
  struct Guidance : ns2vc::StepTable<float> {
    bool on = false;
    int n = 0;
  } guide;
  int loop_items() const { return guide.on ? guide.n : B; }      // items the sampling loop's entry points take and give
  // History 2 (order-3 tables: a nonzero column 10 or 11, detected by ns2vc_sampler_load): the update also keeps m_{i-2}, in a buffer
  // of its own outside the plan arena, allocated on the first loop that needs it -- the dense plan's layout and launches do not change.
  struct History2 : ns2vc::StepTable<float> {      // dev = m_{i-2}, B * T * CP floats
    bool on = false;
  } hist2;
  // Per-item schedules (ns2vc_sampler_load_items): every loop item walks a solver table of its own (common.h SolverItem).  coef_dev then holds the
  // `rows` rows of the distinct tables, `steps` the loop's length S = max(start + steps), `stochastic` / `hist2.on` the UNION over the items (what
  // begin allocates and requires).  The records live in a buffer of their own outside the plan arena, filled from pinned staging (new schedules of
  // the same form are a copy: the captured step graph stays valid); on / off, and a change of either union flag, recapture.
  struct ItemSchedules : ns2vc::StepTable<ns2vc::SolverItem> {
    bool on = false;
    int n = 0, rows = 0;                   // loop items the records cover; rows of coef_dev in use
    std::vector<ns2vc::SolverItem> host;   // the records ns2vc_sampler_load_items sent (a slot loop's live in slots.rec)
  } items;
  // Slot loop (ns2vc_sampler_open): the per-item form with the loop items as SLOTS that are admitted and taken independently while the step
  // counter keeps running.  `rec` / `busy` are the host's mirror of the device records (busy = admitted and not yet taken); the forms the
  // captured step graph bakes in (hist2.on, stochastic) are fixed at open.  Slot lists and records travel through a ring of pinned staging
  // buffers (a call waits only for the copy made `kRing` calls earlier) into `list_dev`, which the kernels read: [cap] slots, then [cap] records.
  struct SlotLoop {
    static constexpr int kRing = 8;
    bool on = false;
    std::vector<ns2vc::SolverItem> rec;
    std::vector<char> busy;
    std::vector<float> coef;                 // host mirror of the coefficient table (ns2vc_sampler_write_rows): admit derives an item's form from its rows
    int* list_dev = nullptr;
    int cap = 0;
    ns2vc::Staged ring[kRing];
    int ring_next = 0;
    ns2vc::Staged coef_ring[kRing];
    int coef_next = 0;
    bool any_busy() const { for (char b : busy) if (b) return true; return false; }
  } slots;
  bool in_slot_loop() const { return slots.on && next_step >= 0; }
  // Correction of the predicted x0 (ns2vc_sampler_set_x0_correction): mode 1 = dynamic thresholding, 2 = clamp.  The ratio and max_val are
  // arguments of the step's launches, so a change of the mode or of a value the active mode passes drops the captured step graph.  The per-item thresholds of mode 1 live in a
  // buffer of their own outside the plan arena (one float per batch item), allocated when the correction is switched on.
  struct X0Correction {
    int mode = 0;
    float ratio = 0.995f, max_val = 1.0f;
    ns2vc::StepTable<float> thr;
    // The per-item form (ns2vc_sampler_set_x0_correction_items; not together with mode != 0 above): one record per loop item in a buffer of its
    // own, filled from pinned staging like the seeds and the scales, so new values replay the captured step graph.  What the graph bakes in: the
    // table being on, the two pointers, and whether the quantile launch is there (`quant`: a record in mode 1 exists, or a slot loop, whose
    // admissions the host cannot foresee).  `host` mirrors the records for the per-item refusals (a corrected stochastic item).
    struct Items : ns2vc::StepTable<ns2vc::ItemCorrect> {
      bool on = false;
      bool quant = false;
      int n = 0;
      std::vector<ns2vc::ItemCorrect> host;
    } items;
  } x0c;

  // Known frames (ns2vc_sampler_set_known): the rows of x0 that every step overwrites with the caller's latent in front of the
  // solver update (launch_hold_x0).  The known rows, channels-last like x0, and the held-row list with its count live in buffers of their own
  // outside the plan arena, allocated on first use for the whole prepared shape: new values and new masks are copies on the caller's stream and
  // replay the captured step graph, on / off recaptures.  `last` mirrors each item's last held frame for the length check of ns2vc_sampler_begin.
  struct Hold {
    bool on = false;
    int n = 0;                             // loop items the mask covered
    ns2vc::StepTable<float> known;         // [n * T][CP]
    ns2vc::StepTable<int> rows;            // [HOLD_LIST_HEAD + n * T]: the count, then the held rows of one half
    std::vector<int32_t> last;
  } hold;
  // Known frames of a slot loop (ns2vc_sampler_open_known): per SLOT state for the whole prepared shape, allocated at open outside the
  // plan arena -- the known rows channels-last like x0, one mask byte per frame (all clear at open) that launch_hold_slots reads at every step,
  // and the device landing place of a call's host mask.  `on` is the form the captured step graph bakes in (the launch is there or not); an
  // admission's frames are copies and one launch_known_items, a take clears its slots: neither recaptures.  `last` mirrors each slot's last held
  // frame (-1: none) for the length check of ns2vc_sampler_admit.
  struct SlotHold {
    bool on = false;
    ns2vc::StepTable<float> known;         // [loop_items * T][CP]
    ns2vc::StepTable<uint8_t> mask;        // [loop_items * T]
    ns2vc::StepTable<uint8_t> mask_in;     // [loop_items * T]: a call's mask [n][T] on its way to launch_known_items
    std::vector<int32_t> last;
    void drop(::ns2vc_unet* h) {           // the form goes (the loop ended, the shape or the item count changed): the next loop captures without it
      if (on) ns2vc::drop_step_graph(h);
      on = false;
      last.clear();
    }
  } shold;

  // named persistent buffers
  float *xe = nullptr, *xbar = nullptr, *d1 = nullptr, *mprev = nullptr, *x0 = nullptr;
  float *content_conv = nullptr, *prompt = nullptr, *maskbias = nullptr;
  float *aug = nullptr, *emb = nullptr, *temb = nullptr;
  float *seq = nullptr, *pool_qkv_buf = nullptr, *pooled = nullptr;
  void *xe_op = nullptr, *content_op = nullptr, *prompt_op = nullptr, *emb_act_op = nullptr, *kv = nullptr, *seq_op = nullptr;   // operand-typed
  float *t_dev = nullptr;
  uint8_t* mask_dev = nullptr;
  int* step_dev = nullptr;
  size_t stats_bytes = 8;
  float* coef_dev = nullptr;
  float* temb_table = nullptr;   // [kMaxSteps][time_embed_dim]: the timestep MLP of every row of the solver table (sampling loop only)
  bool temb_table_valid = false;
  int steps = 0;
  int next_step = -1;            // sampling loop position (host mirror of step_dev + 1); -1 = no loop begun
  bool use_step_table = false;
  // LayerNorm-health read-out (ns2vc_unet_ln_ratio*): snapshot slot in the arena, pinned host mailbox, completion event
  struct LnReadout {
    unsigned* mail = nullptr;
    hipEvent_t event = nullptr;
    bool posted = false;
  } ln_out;

  hipStream_t cap_stream = nullptr;
  hipGraphExec_t step_graph = nullptr;
  unsigned long long graph_captures = 0;      // step graphs instantiated over the engine's life (ns2vc_unet_graph_captures)

  // 16-bit engines keep the solver state's operand copy as a hi + lo pair, rows [hi(CP) | lo(CP)] (common.h op_rest): its row width and where lo starts
  int pair_width() const { return prec != ns2vc::PREC_F32 ? 2 * CP : CP; }
  int pair_off() const { return prec != ns2vc::PREC_F32 ? CP : 0; }

  ~ns2vc_unet() {      // (the step tables and the pinned staging release themselves after this: ns2vc::StepTable, ns2vc::Staged)
    if (slots.list_dev) (void)hipFree(slots.list_dev);
    if (step_graph) (void)hipGraphExecDestroy(step_graph);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    if (tfork.side_stream) (void)hipStreamDestroy(tfork.side_stream);
    if (tfork.ev_fork) (void)hipEventDestroy(tfork.ev_fork);
    if (tfork.ev_join) (void)hipEventDestroy(tfork.ev_join);
    if (ln_out.event) (void)hipEventDestroy(ln_out.event);
    if (ln_out.mail) (void)hipHostFree(ln_out.mail);
    if (arena) (void)hipFree(arena);
    if (coef_dev) (void)hipFree(coef_dev);
    if (temb_table) (void)hipFree(temb_table);
    for (void* p : weight_allocs) (void)hipFree(p);
  }
};

namespace ns2vc {

// pack.cpp
std::vector<BlockW> make_topology(const ns2vc_unet_cfg& c);
void build_expected(ns2vc_unet* h);
std::vector<float> rounded_rowsum(const float* rows, int N, int K, int Np, int prec);
int pack_all(ns2vc_unet* h);
// plan.cpp
extern int g_geglu_min_rows;
std::vector<int> level_lengths(int T, int n_levels);
int build_plan(ns2vc_unet* h, bool sizing);
int run_ops(const std::vector<Op>& ops, hipStream_t s, size_t first = 0, size_t last = (size_t)-1);
bool temb_forks(const ns2vc_unet* h, size_t last);
void drop_plan(ns2vc_unet* h);
// engine.cpp
int check_ready(ns2vc_unet* h, bool need_plan);
int load_state(ns2vc_unet* h, const float* x_bct, hipStream_t s, int items = 0);   // items: the first `items` of the batch (0 = all B)
// sampler.cpp
bool solver_in_conv_out(ns2vc_unet* h, GemmArgs& g);
// a host list of n slots in [0, nslots) (no repeats) -> the engine's device list, asynchronously on `s`; with `rec` their n records behind it.
// *slots_dev / *rec_dev point into h->slots.list_dev.  Fails on a bad list.  extra: `extra_bytes` more host bytes that travel in the same staging
// buffer to `extra_dev` (a known-frame mask).
int stage_slot_list(ns2vc_unet* h, int n, const int32_t* slots, int nslots, const SolverItem* rec, hipStream_t s, const int** slots_dev,
                    const SolverItem** rec_dev, const void* extra = nullptr, size_t extra_bytes = 0, void* extra_dev = nullptr);
// abi_kernels.cpp
hipError_t init_all_attributes();
int xcd_round_robin_of_current_device();

}  // namespace ns2vc
