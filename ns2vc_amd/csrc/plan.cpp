// The launch planner: restates the op sequence of the reference forward
// (unet1d/unet_1d_condition.py:743-1037; blocks unet1d/unet_1d_blocks.py:949-1016,
// 1071-1097, 602-623, 2070-2131, 2182-2207; resnet.py:591-641; transformer_1d.py:256-295;
// attention.py:130-203) as a flat list of kernel launches on channels-last tensors carved from one arena.
#include "engine_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ns2vc {

int g_geglu_min_rows = 4608;   // rows from which the token-stationary GEGLU kernel replaces the GEMM (tests: ns2vc_debug_set_geglu_min_rows)

// frames per level: every stride-2 downsampling halves, rounding up
std::vector<int> level_lengths(int T, int n_levels) {
  std::vector<int> Ts(n_levels);
  Ts[0] = T;
  for (int l = 1; l < n_levels; ++l) Ts[l] = (Ts[l - 1] + 1) / 2;
  return Ts;
}

namespace {

// ------------------------------------------------------------------------------------
// plan building.  Two kinds of activation tensors:
//   fp32  "stream" tensors : residual stream, skips, GroupNorm inputs (statistics stay fp32)
//   "op"  operand tensors  : what GEMMs / attention read — bf16 (perf) or fp32 (parity)
// ------------------------------------------------------------------------------------
struct Planner {
  ns2vc_unet* h;
  std::vector<Op>* ops;
  bool sizing = false;       // first pass: only measure the arena
  size_t off = 0;
  int B, T, Lp, G, prec;
  size_t opsz = 2;
  // scratch shared by all layers (stream-ordered)
  double* gn_partial = nullptr;
  void *xn = nullptr, *xr = nullptr;     // GroupNorm-applied / raw operand copies of a resnet input
  float *rs1 = nullptr, *rs2 = nullptr, *rs3 = nullptr;   // LayerNorm-by-linearity row statistics [M][C/64][2] (norm1/2/3)
  int gn_rows = 64;
  // per-item valid lengths (h->lens.masked): level lengths of the plan, and the zeroing of padded rows after every launch that writes a frame tensor
  bool masked = false;
  // option masked_fuse: the launches whose kernel masks its own rows (gemm_masks_rows) get the length table instead of a mask_rows launch, keep their epilogue
  // statistics, and a k = 3 conv on the tap-sharing kernel keeps its GroupNorm prologue
  bool fused = false;
  std::vector<int> Ts;
  int level_of(int Tl) const {
    for (size_t l = 0; l < Ts.size(); ++l) if (Ts[l] == Tl) return (int)l;
    return -1;
  }
  const int* lens_of(int Tl) const {
    const int l = level_of(Tl);
    return (masked && l >= 0 && !sizing) ? h->lens.dev + (size_t)l * B : nullptr;
  }
  const float* selfbias_of(int Tl) const {
    const int l = level_of(Tl);
    if (!masked || l < 0) return nullptr;
    size_t o = 0;
    for (int k = 0; k < l; ++k) o += (size_t)B * Ts[k];
    return sizing ? nullptr : h->lens.selfbias + o;
  }
  // rows t >= lens[b] of a frame tensor [B*Tl][ld] (elements of `esz` bytes, the first `cols` of each row) -> 0 after the launch planned last
  void mask(const std::string& name, void* p, int ld, int cols, size_t esz, int Tl) {
    if (!masked || !p || ops != &h->fwd_ops || level_of(Tl) < 0) return;
    const int* lens = lens_of(Tl);
    const int Bq = B;
    const size_t ldb = (size_t)ld * esz, rb = (size_t)cols * esz;
    add(name + ".mask", [=](hipStream_t s) { return launch_mask_rows(p, ldb, rb, Bq, Tl, lens, s); }, 4, 0.0, 0.0);
  }
  // GroupNorm statistics accumulated by the producing GEMM's epilogue (int64 fixed point, [B][C/16][2]);
  // one zeroed slab per produced tensor, all carved from stats_pool (cleared by one memset per forward)
  long long* stats_pool = nullptr;
  size_t stats_cap = 0, stats_used = 0;
  std::map<const void*, long long*> stats_of;
  long long* new_stats(const float* tensor, int Tl, int C) {
    // (masked: the epilogue would also sum the padded rows it has not zeroed yet -- the statistics come from gn_partial over the masked rows)
    // (masked_fuse: the producer's masked epilogue leaves the padded rows out; Planner::gemm takes the slab back where the producer has no such epilogue)
    if (Tl < 64 || (C & 15) || (masked && !fused)) { stats_of.erase(tensor); return nullptr; }
    const size_t n = (size_t)B * (C / 16) * 2;
    if (stats_used + n > stats_cap) { stats_of.erase(tensor); return nullptr; }
    long long* p = stats_pool ? stats_pool + stats_used : reinterpret_cast<long long*>(sizeof(long long) * (stats_used + 1));  // sizing pass: non-null token
    stats_used += n;
    stats_of[tensor] = p;
    return p;
  }
  unsigned* new_sync(size_t nblocks) {       // 64-bit arrival words of a cooperative GroupNorm prologue, one per row block
    nblocks = (nblocks + 1) & ~(size_t)1;     // (whole 16-byte units, 16-byte aligned: Op::rearm zeroes them with 16-byte stores)
    stats_used = (stats_used + 1) & ~(size_t)1;
    if (stats_used + nblocks > stats_cap) return nullptr;
    long long* p = stats_pool ? stats_pool + stats_used : reinterpret_cast<long long*>(sizeof(long long) * (stats_used + 1));
    stats_used += nblocks;
    return reinterpret_cast<unsigned*>(p);
  }
  long long* find_stats(const float* tensor) const {
    auto it = stats_of.find(tensor);
    return it == stats_of.end() ? nullptr : it->second;
  }

  char* alloc_bytes(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    char* p = sizing ? nullptr : reinterpret_cast<char*>(h->arena) + off;
    off += bytes;
    return p;
  }
  template <typename Tp> Tp* alloc(size_t count) { return reinterpret_cast<Tp*>(alloc_bytes(count * sizeof(Tp))); }
  void* alloc_op(size_t count) { return alloc_bytes(count * opsz); }
  void* op_off(void* p, size_t elems) const { return p ? static_cast<void*>(static_cast<char*>(p) + elems * opsz) : nullptr; }

  void add(const std::string& name, std::function<hipError_t(hipStream_t)> fn, int kind = 0, double flops = 0.0, double bytes = 0.0) {
    if (sizing) return;
    Op op;
    op.name = name; op.fn = std::move(fn); op.kind = kind; op.flops = flops; op.bytes = bytes;
    ops->push_back(std::move(op));
  }
  // every launch that reads the time scale / shift rows (h->temb) -- a GEMM with a GroupNorm prologue or a stand-alone gn_apply -- is planned
  // through here: the captured step's side branch that computes them (fork_temb) joins in front of the FIRST of them
  void temb_reader() {
    if (sizing || ops != &h->fwd_ops) return;
    const int idx = (int)ops->size();
    if (h->tfork.first < 0) h->tfork.first = idx;
    if (h->tfork.join < 0 && h->tfork.readers >= h->tfork.join_skip) h->tfork.join = idx;
    ++h->tfork.readers;
  }
  void tap(const std::string& name, const float* src, int rows, int cols) {
    if (!h->debug) return;
    float* cp = alloc<float>((size_t)rows * cols);
    if (sizing) return;
    h->taps.push_back({name, cp, rows, cols});
    const size_t bytes = (size_t)rows * cols * sizeof(float);
    add("tap:" + name, [=](hipStream_t s) { return hipMemcpyAsync(cp, src, bytes, hipMemcpyDeviceToDevice, s); }, 4, 0.0, 2.0 * bytes);
  }

  void gemm(const std::string& name, GemmArgs g, int pr_override = -1) {
    const int pr = pr_override >= 0 ? pr_override : prec;
    const double osz = (double)opsz;
    const double nout = g.geglu ? g.N / 2 : g.N;
    // the ALGORITHMIC figures of the op (what the roofline fractions are priced on): a launch on hi + lo operand pairs (split_io: [hi | lo] + hi again against
    // (hi(w) | hi(w) | lo(w)), three times the K) counts as the plain convolution it computes, not as the MFMA work and bytes it spends on it
    const bool pair = g.c1 && g.a1 == g.a0 && g.c0 == 2 * g.c1 && g.c2 == 0;
    const double Kalg = pair ? g.K / 3.0 : (double)g.K, cin = pair ? g.c1 : g.c0 + g.c1 + g.c2, cgn = pair ? g.c1 : g.c0;
    const double flops = 2.0 * g.M * (double)g.N * Kalg;
    const double in_rows = (double)g.B * g.Tin;
    const double bytes = in_rows * cin * osz + (double)g.N * Kalg * osz + (g.out_f32 ? g.M * nout * 4.0 : 0.0) +
                         (g.out_op ? g.M * nout * osz : 0.0) + (g.res ? g.M * nout * 4.0 : 0.0);
    // (a GroupNorm prologue reads the fp32 rows and writes + re-reads the operand rows it builds)
    const double pro = g.gnp_x ? in_rows * cgn * (4.0 + osz * (g.gnp_raw ? 2.0 : 1.0)) : 0.0;
    if (g.taps == 3 && g.tmode == TMODE_SAME && !g.conv_bn) g.conv_bn = convts_bn_for(g, h->bn128_min);     // the column tile is a PLAN decision (this engine's device)
    // masked_fuse: the kernel zeroes the rows past an item's end itself where it can; elsewhere the mask_rows launches below and no epilogue statistics
    const bool self_mask = fused && ops == &h->fwd_ops && g.Tout > 1 && level_of(g.Tout) >= 0 && gemm_masks_rows(g, pr);
    if (self_mask) {
      g.lens = lens_of(g.Tout);
      if (g.gnp_x && g.algo == 0) g.algo = 2;                    // (the masked prologue is the materialising one)
    } else if (masked && g.stats) { stats_of.erase(g.out_f32); g.stats = nullptr; }
    if (g.gnp_temb) temb_reader();
    add(g.gnp_x ? name + "[+norm]" : name, [=](hipStream_t s) { return launch_gemm(g, pr, s); }, 1, flops, bytes + pro);
    if (!sizing && g.gnp_x && g.gnp_sync) {
      unsigned* words = g.gnp_sync;
      const size_t nbytes = (((size_t)g.B * g.Tin + 63) / 64) * 8;
      ops->back().rearm = [=](hipStream_t s) { return launch_zero(words, (nbytes + 15) & ~(size_t)15, s); };
    }
    if (g.Tout > 1 && !self_mask) {
      const int nc = g.geglu ? g.N / 2 : g.N;
      mask(name, g.out_f32, g.ldo_f32, nc, 4, g.Tout);
      mask(name, g.out_op, g.ldo_op, nc, operand_bytes(pr), g.Tout);
    }
  }
  // A = operand tensor [B*Tin][c0]; results to out_f32 and/or out_op (row stride = logical width)
  GemmArgs base(const void* a0, int lda0, int c0, int Tin, int Tout, const PackedW& w, float* out_f32, void* out_op, int ldo) {
    GemmArgs g;
    memset(&g, 0, sizeof(g));
    g.a0 = a0; g.lda0 = lda0; g.c0 = c0;
    g.B = B; g.Tin = Tin; g.Tout = Tout; g.M = B * Tout;
    g.taps = 1; g.tmode = TMODE_SAME;
    g.w = w.w; g.K = w.K; g.N = w.N; g.bias = w.bias;
    g.w_tiled = h->conv_wtiled ? w.wt : nullptr;     // (only the k = 3 / stride-1 launches of the tap-sharing kernel look at it)
    g.out_f32 = out_f32; g.ldo_f32 = ldo;
    g.out_op = out_op; g.ldo_op = ldo;
    g.algo = h->conv_ts ? (h->gn_inloop ? 0 : 2) : 1;
    return g;
  }
  // GroupNorm of a (possibly concatenated) fp32 input: statistics -> per-(b,c) affine -> operand tensor `dst`
  // (= act(GN(x)) with the concat materialised), optionally also the raw concat `raw` for a 1x1 shortcut.
  // `consumer_n` > 0: `dst` has exactly one reader, a GEMM with that many output columns that is planned next -- where the
  // norm qualifies (see fuse_gn_gemm) no launch is added and the returned GnPro is handed to that GEMM with gn_fuse().
  struct GnPro { const float* x = nullptr; int ldx = 0; const long long* st = nullptr; const float* gamma = nullptr; const float* beta = nullptr;
                 const float* temb = nullptr; int ldtemb = 0; float eps = 0.f; int G = 0, silu = 0; unsigned* sync = nullptr; unsigned* alone = nullptr;
                 const float* x1 = nullptr; int ldx1 = 0, c1 = 0; const long long* st1 = nullptr; void* raw = nullptr; };
  static void gn_fuse(GemmArgs& g, const GnPro& p) {
    if (!p.x) return;
    g.gnp_x = p.x; g.gnp_ldx = p.ldx; g.gnp_stats = p.st; g.gnp_gamma = p.gamma; g.gnp_beta = p.beta;
    g.gnp_temb = p.temb; g.gnp_ldtemb = p.ldtemb; g.gnp_eps = p.eps; g.gnp_G = p.G; g.gnp_silu = p.silu;
    g.gnp_sync = p.sync; g.gnp_alone = p.alone;
    g.gnp_x1 = p.x1; g.gnp_ldx1 = p.ldx1; g.gnp_c1 = p.c1; g.gnp_stats1 = p.st1; g.gnp_raw = p.raw;
  }
  GnPro groupnorm(const std::string& name, const float* a0, int lda0, int c0, const float* a1, int lda1, int c1, int Tl, float eps,
                  const float* gamma, const float* beta, const float* temb, int temb_off, int cout, int silu, void* dst, void* raw,
                  int consumer_n = 0, int consumer_taps = 1, int pair = 0) {
    (void)cout;
    const int nchunk = (Tl + gn_rows - 1) / gn_rows, rows = gn_rows, Bq = B, Gq = G, ldt = h->temb_all.N, pr = prec;
    double* part = gn_partial;
    const double n = (double)Bq * Tl * (c0 + c1);
    const long long* st0 = find_stats(a0);
    const long long* st1 = a1 ? find_stats(a1) : nullptr;
    const bool epi = st0 && (!a1 || st1) && (((c0 + c1) / Gq) % 16 == 0) && (c0 % 16 == 0);
    // masked: a prologue only under masked_fuse and only in front of a conv the tap-sharing kernel takes (the one kernel with a masked prologue)
    bool pro_ok = !masked;
    if (masked && fused && consumer_taps == 3 && consumer_n > 0) {
      GemmArgs t;
      memset(&t, 0, sizeof(t));
      t.taps = 3; t.tmode = TMODE_SAME; t.B = Bq; t.Tin = t.Tout = Tl; t.M = Bq * Tl; t.N = consumer_n;
      t.c0 = pair ? 2 * (c0 + c1) : c0 + c1; t.c1 = pair ? c0 + c1 : 0;
      t.algo = h->conv_ts ? 2 : 1;
      pro_ok = gemm_uses_convts(t, prec);
    }
    // (pair: the prologue that writes hi + lo pairs exists in the tap-sharing conv kernel only)
    if (epi && pro_ok && h->fuse_gn_gemm && consumer_n > 0 && (consumer_n % 128) == 0 && (h->fuse_gn_cat || (!a1 && !raw)) && Tl >= 66 && c0 + c1 <= 1024 &&
        (!pair || (h->conv_ts && consumer_taps == 3 && ((c0 + c1) % 64) == 0)) &&
        ((c0 + c1) % Gq) == 0 && Gq <= 8 && (lda0 & 3) == 0 && (!a1 || ((lda1 & 3) == 0 && (c1 & 15) == 0))) {
      GnPro p;
      p.x = a0; p.ldx = lda0; p.st = st0;
      if (a1) { p.x1 = a1; p.ldx1 = lda1; p.c1 = c1; p.st1 = st1; }      // a concat of two sources (up blocks), normalised as one tensor
      p.raw = raw;                                                         // ... and the un-normalised operand copy for the 1x1 shortcut
      p.gamma = gamma; p.beta = beta; p.temb = temb ? temb + temb_off : nullptr; p.ldtemb = ldt;
      p.eps = eps; p.G = Gq; p.silu = silu;
      // wider than one column tile: the column tiles of a row block share the prologue's rows (one 64-bit count per 64-row block, zeroed with the arena)
      // (r5: the counts live in the statistics pool, so the forward's one clear launch also zeroes them: a launch that was cut short cannot
      //  leave a remainder behind for the next forward)
      int nshare = consumer_n / 128;           // column tiles of a row block: N / 128 in gemm4_kernel, N / BN in the tap-sharing conv kernel
      if (consumer_taps == 3 && h->conv_ts && Tl >= 66) {
        GemmArgs t;
        memset(&t, 0, sizeof(t));
        t.B = Bq; t.Tin = t.Tout = Tl; t.N = consumer_n;
        nshare = consumer_n / convts_bn_for(t, h->bn128_min);
      }
      if (h->gn_coop && nshare >= std::max(2, h->gn_coop_min)) { p.sync = new_sync(((size_t)Bq * Tl + 63) / 64); p.alone = (p.sync && h->ln_health) ? h->ln_health + 48 : nullptr; }
      return p;
    }
    if (!epi) {
      st0 = st1 = nullptr;
      add(name + ".gn_stats", [=](hipStream_t s) { return launch_gn_partial(a0, lda0, c0, a1, lda1, c1, Bq, Tl, Gq, part, nchunk, rows, s); },
          3, 3.0 * n, 4.0 * n);
    }
    if (temb) temb_reader();
    const int* lens = masked ? lens_of(Tl) : nullptr;             // (masked: statistics over the valid rows, zero rows past them)
    add(name + ".gn_apply", [=](hipStream_t s) {
      return launch_gn_apply(a0, lda0, c0, a1, lda1, c1, Bq, Tl, Gq, eps, part, nchunk, st0, st1, gamma, beta, temb, ldt, temb_off, silu, dst,
                             raw, pr, s, pair, lens);            // (pair: the rows as a hi + lo operand pair, split_io's conv_out)
    }, 3, 4.0 * n, n * (4.0 + opsz * (raw ? 2.0 : 1.0) + opsz * (pair ? 1.0 : 0.0)));
    return GnPro();
  }

  // ResnetBlock2D (resnet.py:591-641).  out (fp32) [+ out_op operand copy when a conv consumes it next]
  void resnet(const ResnetW& r, const float* a0, int lda0, int c0, const float* a1, int lda1, int c1, int Tl, float* h1, void* hn,
              float* out, void* out_op) {
    const int cin = c0 + c1;
    // ---- conv1(act(norm1(x)))
    const GnPro p1 = groupnorm(r.prefix + ".norm1", a0, lda0, c0, a1, lda1, c1, Tl, 1e-5f, r.n1g, r.n1b, nullptr, 0, 0, 1, xn,
                               r.shortcut ? xr : nullptr, r.conv1.N, 3);
    GemmArgs g = base(xn, cin, cin, Tl, Tl, r.conv1, h1, nullptr, r.cout);
    g.taps = 3;
    gn_fuse(g, p1);
    g.stats = new_stats(h1, Tl, r.cout);
    gemm(r.prefix + ".conv1", g);
    // ---- conv2(act(norm2(h) * (1 + scale) + shift)) + shortcut
    const GnPro p2 = groupnorm(r.prefix + ".norm2", h1, r.cout, r.cout, nullptr, 0, 0, Tl, 1e-5f, r.n2g, r.n2b, h->temb, r.temb_off, r.cout, 1, hn,
                               nullptr, r.conv2.N, 3);
    GemmArgs g2 = base(hn, r.cout, r.cout, Tl, Tl, r.conv2, out, out_op, r.cout);
    g2.taps = 3;
    gn_fuse(g2, p2);
    if (r.shortcut) {      // out = conv2(hn) + conv_shortcut(x): the 1x1 conv rides along as a second K segment
      g2.a2 = xr; g2.lda2 = cin; g2.c2 = cin;
    } else {
      g2.res = a0; g2.ldres = lda0;
    }
    g2.stats = new_stats(out, Tl, r.cout);
    gemm(r.prefix + ".conv2", g2);
  }

  // `self`: Lk is a frame count like Lq (attn1); its keys past an item's end are masked by the level's key-bias row, or -- option masked_attn --
  // left out by the kernel itself (AttnArgs.k_lens), which then also stores the result rows past the end as zeros (q_lens): no mask_rows launch
  // `cross_lens`: the per-item prompt lengths (attn2 under ns2vc_unet_set_prompt_lengths; `bias` is then the row that also drops the keys past an
  // item's frames).  With masked_attn the kernel takes the table as k_lens -- the key tiles past an item's frames are skipped -- and the bias only
  // where a mask was given; otherwise (option off, the fp8 PV form) the launch reads the bias row.  (With a mask the launch keeps the COMBINED row
  // beside k_lens: its tail repeats what k_lens already drops, but its entries below P_b are the mask's holes, which k_lens cannot express.)
  void attention(const std::string& name, const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int Lq, int Lk,
                 const float* bias, int hd, void* out, int ldo, bool self = false, const int* cross_lens = nullptr) {
    AttnArgs a;
    memset(&a, 0, sizeof(a));
    a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
    a.B = B; a.H = h->cfg.heads; a.Lq = Lq; a.Lk = Lk; a.bias = bias;
    a.scale = 1.0f / std::sqrt((float)hd);
    a.out = out; a.ldo = ldo;
    a.pv_fp8 = (h->attn_fp8 && prec != PREC_F32) ? 1 : 0;
    a.exact_only = h->attn_optimistic ? 0 : 1;
    a.fallbacks = h->attn_fallbacks;
    const int pr = prec;
    const bool self_mask = masked && h->masked_attn && ops == &h->fwd_ops && level_of(Lq) >= 0 && attention_masks_rows(a, hd, pr);
    if (self_mask) {
      a.q_lens = lens_of(Lq);
      if (self) a.k_lens = lens_of(Lk);
    } else if (self) a.bias = selfbias_of(Lk);
    if (cross_lens && (self_mask || (h->masked_attn && ops == &h->fwd_ops && attention_masks_rows(a, hd, pr)))) {
      a.k_lens = cross_lens;
      if (!h->has_mask) a.bias = nullptr;
    }
    const bool resident = h->attn_resident, resident_lens = h->masked_attn_resident;      // (the second: launches under q_lens / k_lens only)
    add(name, [=](hipStream_t s) { return launch_attention(a, hd, pr, s, resident, resident_lens); }, 2, 4.0 * B * a.H * (double)Lq * Lk * hd,
        (double)opsz * B * a.H * hd * (2.0 * Lq + 2.0 * Lk));
    if (!self_mask) mask(name, out, ldo, a.H * hd, opsz, Lq);
  }

  // r6: does this block run its prompt cross-attention inside the fused feed-forward kernel?  (the plan of the pre-stage form, 8 heads of 16 / 32 channels)
  std::map<std::string, void*> xattn_vt;      // per transformer block: the k | v fragment image of its hoisted rows (built by the condition plan)
  bool xattn_fused(const AttnW& a, int Tl) const {
    const int d = a.dim;
    const bool lin = h->ln_linear && (d % 128 == 0) && d <= 512 && !masked;
    return h->fuse_xattn && lin && h->fold_ff && h->fuse_ffn && a.ffn_stream && ffn_eligible(d, Tl, prec) && h->fuse_ffn_pre && a.ffn_pre_stream &&
           h->cfg.heads == 8 && (d == 128 || d == 256);
  }
  // Transformer2DModel + BasicTransformerBlock (transformer_1d.py:256-295, attention.py:130-203)
  void transformer(const AttnW& a, const float* x, int Tl, float* y, void* yn, void* qkv, void* ao, void* qb, void* ffh, float* out,
                   void* out_op) {
    const int d = a.dim, M = B * Tl, hd = d / h->cfg.heads, pr = prec;
    const std::string t = a.prefix + ".transformer_blocks.0";
    GemmArgs g;
    auto layernorm = [&](const std::string& nm) {
      add(nm, [=](hipStream_t s) { return launch_ln_apply_op(y, d, M, d, 1e-5f, yn, pr, s); }, 3, 8.0 * M * d, (4.0 + opsz) * M * d);
    };
    // LayerNorm by linearity (h->ln_linear): the producer of every LayerNorm input also writes the raw operand copy
    // `yn` and per-row statistics; the consumer GEMM reads yn and normalises in its epilogue -- no ln_apply pass
    // (masked: the row statistics of LayerNorm by linearity come from epilogues that see the padded rows before they are zeroed, and its health
    //  guard would count them: the explicit normalisation pass over the zeroed rows instead -- LayerNorm of a zero row is zero)
    const bool lin_dense = h->ln_linear && (d % 128 == 0) && d <= 512;
    const bool lin = lin_dense && !masked;
    // option masked_rows: the row chains keep their LayerNorm sums inside the kernel (neither rs1 nor rs2 exists for them) and a lane owns one token,
    // so under lengths they run on their masked instantiations with the level's length table -- everything else of `lin` stays off
    const bool lens_rows = masked && h->masked_rows && ops == &h->fwd_ops && level_of(Tl) >= 0;
    auto consume = [&](GemmArgs& gg, float* rs, const PackedW& w) {
      if (rs) { gg.ln_stats = rs; gg.ln_wsum = w.wsum; gg.ln_eps = 1e-5f; gg.ln_dim = d; gg.ln_health = h->ln_health; }
    };
    float* r1 = lin ? rs1 : nullptr;
    // token-local chains in one launch each (rowchain.hip): same arithmetic and rounding points as the two GEMMs they replace
    auto rowchain = [&](const std::string& nm, const void* a_op, const long long* gn_st, void* stream, const float* bias1, const float* consts2,
                        const float* res, void* z_op, int n2) {
      ns2vc_rowchain_args c;
      memset(&c, 0, sizeof(c));
      c.a_op = a_op; c.lda = d; c.wstream = stream; c.bias1 = bias1; c.consts2 = consts2;
      c.res = res; c.ldres = d; c.out1_f32 = y; c.ldo1 = d; c.out2_op = z_op; c.ldo2 = n2;
      c.ln_eps = 1e-5f; c.M = M; c.dim = d; c.n2 = n2; c.ln_health = h->ln_health;
      if (gn_st) {       // A = GroupNorm(x) built in the kernel's prologue from the producer's epilogue statistics
        c.a_op = nullptr; c.gn_x = x; c.ldx = d; c.gn_stats = gn_st; c.gn_gamma = a.ng; c.gn_beta = a.nb; c.gn_eps = 1e-6f; c.T = Tl; c.G = G;
      }
      // r4: two N-slices per token block where that still is one round of workgroups (dim 384 at the bench batch: 118 blocks on 256 CUs);
      // only for the chain without a residual (the second chain reads and rewrites y in place: two slices would race on it)
      if (!res && stream == a.chain_in && a.chain_in_s2 && h->slice_rows && 2 * ((M + 63) / 64) <= h->cus + 8) { c.wstream = a.chain_in_s2; c.slices = 2; }   // (one round of workgroups on this device's CUs)
      if (lens_rows) { c.lens = lens_of(Tl); c.T = Tl; }            // (the kernel zeroes the rows past an item's end itself: no mask() behind it)
      add(c.slices == 2 ? nm + "[2 slices]" : nm, [=](hipStream_t s) { return launch_rowchain(c, pr, s); }, 1, 2.0 * M * (double)d * (d + n2),
          (double)M * (d * ((gn_st ? 4.0 : opsz) + 4.0 + (res ? 4.0 : 0.0)) + n2 * opsz) + (double)(d + n2) * d * opsz);
    };
    // (masked: asked per launch, rowchain_masks_rows, for the shapes of both chains with and without the GroupNorm prologue)
    auto chains_mask_rows = [&]() {
      ns2vc_rowchain_args c;
      memset(&c, 0, sizeof(c));
      c.M = M; c.dim = d; c.T = Tl;
      c.n2 = 3 * d;
      const bool in_ok = rowchain_masks_rows(c, pr);
      c.n2 = d;
      return in_ok && rowchain_masks_rows(c, pr);
    };
    const bool rows_ok = (masked ? lin_dense && lens_rows && chains_mask_rows() : lin) && h->fuse_rows && a.chain_in && a.chain_mid &&
                         rowchain_eligible(d, d, Tl, pr);
    // (masked: the producer's statistics survive under lengths only where its masked epilogue left the padded rows out -- masked_fuse; new_stats /
    //  Planner::gemm drop the slab everywhere else, and the chain then reads xn from the masked gn_apply)
    const long long* xst = (rows_ok && h->fuse_rows_gn && Tl >= 64 && (d % G) == 0 && ((d / G) % 16) == 0) ? find_stats(x) : nullptr;
    GnPro pn;
    if (!xst) pn = groupnorm(a.prefix + ".norm", x, d, d, nullptr, 0, 0, Tl, 1e-6f, a.ng, a.nb, nullptr, 0, 0, 0, xn, nullptr, rows_ok ? 0 : a.proj_in.N);
    if (rows_ok) {
      rowchain(a.prefix + (xst ? ".rows[norm+proj_in+qkv]" : ".rows[proj_in+qkv]"), xn, xst, a.chain_in, a.proj_in.bias, a.chain_in_consts, nullptr, qkv,
               3 * d);
    } else {
      g = base(xn, d, d, Tl, Tl, a.proj_in, y, r1 ? yn : nullptr, d);
      gn_fuse(g, pn);
      g.rowstats = r1;
      gemm(a.prefix + ".proj_in", g);
      // self attention
      if (!r1) layernorm(t + ".norm1");
      g = base(yn, d, d, Tl, Tl, a.qkv, nullptr, qkv, 3 * d);
      consume(g, r1, a.qkv);
      gemm(t + ".attn1.qkv", g);
    }
    attention(t + ".attn1.sdpa", qkv, 3 * d, op_off(qkv, d), 3 * d, op_off(qkv, 2 * d), 3 * d, Tl, Tl, nullptr, hd, ao, d, true);
    float* r2 = lin ? rs2 : nullptr;
    if (rows_ok) {
      rowchain(t + ".rows[attn1.to_out+attn2.to_q]", ao, nullptr, a.chain_mid, a.o1.bias, a.chain_mid_consts, y, qb, d);
    } else {
      g = base(ao, d, d, Tl, Tl, a.o1, y, r2 ? yn : nullptr, d);
      g.res = y; g.ldres = d;
      g.rowstats = r2;
      gemm(t + ".attn1.to_out", g);
      if (!r2) layernorm(t + ".norm2");
      g = base(yn, d, d, Tl, Tl, a.q2, nullptr, qb, d);
      consume(g, r2, a.q2);
      gemm(t + ".attn2.to_q", g);
    }
    // cross attention (k|v hoisted into h->kv by set_condition)
    const int nkv = h->kv_all.N;
    const bool xatt = xattn_fused(a, Tl) && xattn_vt.count(a.prefix);
    if (!xatt)
      attention(t + ".attn2.sdpa", qb, d, op_off(h->kv, a.kv_off), nkv, op_off(h->kv, a.kv_off + d), nkv, Tl, Lp,
                (h->has_mask || h->plens.on) ? h->maskbias : nullptr, hd, ao, d, false, h->plens.on ? h->plens.dev : nullptr);
    float* r3 = lin ? rs3 : nullptr;
    // With the feed-forward output folded into proj_out, proj_out reads the RAW operand copy of y next to the GEGLU
    // output.  LayerNorm by linearity writes that copy anyway (yn); the explicit-LayerNorm plan overwrites yn with the
    // normalised rows, so there the raw copy goes to qb (the cross-attention query buffer, free by now).
    const bool fold = h->fold_ff;
    void* yraw = r3 ? yn : (fold ? qb : nullptr);
    // option masked_ffn: in its pre-stage form the fused feed-forward computes the LayerNorm sums of norm3 itself (no r3) and a lane owns one token, so
    // under lengths it runs on its masked instantiations with the level's length table; the plain form, which reads r3, is not planned under lengths
    auto ffn_masks = [&]() {
      ns2vc_ffn_args f;
      memset(&f, 0, sizeof(f));
      f.B = B; f.T = Tl; f.M = M; f.dim = d;
      return ffn_masks_rows(f, pr);
    };
    // (every condition of the kept launch in one place, as lens_rows / rows_ok above: the option, the forward plan, a level with a length row, the
    //  dense conditions of the pre-stage form and a masked kernel for the launch)
    const bool lens_ffn = masked && h->masked_ffn && ops == &h->fwd_ops && level_of(Tl) >= 0 && lin_dense && fold && h->fuse_ffn && a.ffn_stream &&
                          h->fuse_ffn_pre && a.ffn_pre_stream && ffn_eligible(d, Tl, pr) && ffn_masks();
    const bool ffn_ok = lens_ffn || (fold && r3 && h->fuse_ffn && a.ffn_stream && ffn_eligible(d, Tl, pr));
    // attn2.to_out + residual as the pre-stage of the fused feed-forward kernel: y after the cross-attention is never stored
    const bool ffn_pre = ffn_ok && h->fuse_ffn_pre && a.ffn_pre_stream;
    if (!ffn_pre) {
      g = base(ao, d, d, Tl, Tl, a.o2, y, yraw, d);
      g.res = y; g.ldres = d;
      g.rowstats = r3;
      gemm(t + ".attn2.to_out", g);
    }
    // feed-forward (GEGLU)
    if (ffn_ok) {
      // LayerNorm(norm3) -> GEGLU -> ff.net.2 -> + y -> proj_out -> + x in ONE launch: the hidden tensor never exists
      ns2vc_ffn_args f;
      memset(&f, 0, sizeof(f));
      f.yn = yn; f.ldy = d; f.ln_stats = r3; f.ln_eps = 1e-5f;
      f.wstream = a.ffn_stream; f.consts = a.ffn_consts; f.bias2 = a.ffpo.bias;
      if (ffn_pre) {
        f.yn = nullptr; f.ln_stats = nullptr; f.wstream = a.ffn_pre_stream;
        f.pre_a = ao; f.pre_lda = d; f.pre_bias = a.o2.bias; f.pre_res = y; f.pre_ldres = d;
      }
      if (xatt) {         // (implies ffn_pre) the cross-attention's output never exists: the kernel builds its token panel from q, the hoisted k rows and V^T
        f.pre_a = nullptr;
        f.att_q = qb; f.att_ldq = d; f.att_kv = xattn_vt[a.prefix];
        f.att_bias = (h->has_mask || h->plens.on) ? h->maskbias : nullptr; f.att_scale = 1.0f / std::sqrt((float)hd); f.att_Lk = Lp;
      }
      f.res = x; f.ldres = d;
      f.out_f32 = out; f.ldo_f32 = d; f.out_op = out_op; f.ldo_op = d;
      f.stats = new_stats(out, Tl, d);
      f.B = B; f.T = Tl; f.M = M; f.dim = d; f.ln_health = h->ln_health;
      if (lens_ffn) f.lens = lens_of(Tl);           // (the kernel zeroes the rows past an item's end itself: no mask() behind it)
      const double fl = 2.0 * M * (double)d * ((ffn_pre ? 14.0 : 13.0) * d) + (xatt ? 4.0 * B * h->cfg.heads * (double)Tl * Lp * hd : 0.0);
      add(a.prefix + (xatt ? ".ffn[attn2.sdpa+to_out+geglu+ff.out+proj_out]" : ffn_pre ? ".ffn[attn2.to_out+geglu+ff.out+proj_out]" : ".ffn[geglu+ff.out+proj_out]"),
          [=](hipStream_t s) { return launch_ffn(f, pr, s); }, 1, fl,
          (double)M * d * (opsz + 8.0 + (ffn_pre ? 4.0 : 0.0) + (out_op ? opsz : 0.0)) + (ffn_pre ? 14.0 : 13.0) * d * d * opsz +
              (xatt ? (double)opsz * B * d * 2.0 * Lp : 0.0));
      return;
    }
    // option masked_geglu: under lengths the token-stationary kernel takes the LayerNorm sums of norm3 from the raw operand rows it holds (qb, which
    // attn2.to_out has just written and ff.out+proj_out reads again) and masks its own rows -- no norm3 pass, no r3, no mask() behind it.  (Every
    // condition of the kept launch in one place: the option, the forward plan, a level with a length row, the dense conditions of the launch
    // with its crossover and a masked kernel for it; the fused feed-forward above did not apply.)
    auto geglu_masks = [&]() {
      ns2vc_geglu_args f;
      memset(&f, 0, sizeof(f));
      f.M = M; f.dim = d; f.T = Tl;
      return geglu_masks_rows(f, pr);
    };
    const bool lens_geglu = masked && h->masked_geglu && ops == &h->fwd_ops && level_of(Tl) >= 0 && lin_dense && fold && h->fuse_geglu &&
                            a.geglu_stream && geglu_eligible(d, Tl, pr) && M >= g_geglu_min_rows && geglu_masks();
    if (!r3 && !lens_geglu) layernorm(t + ".norm3");
    // (a workgroup of that kernel sweeps a quarter of the hidden units for its 128 tokens -- 36 dependent tile steps: worth it once the token blocks
    //  fill the chip; below ~144 workgroups the GEMM's 24 column tiles per row block finish sooner.  r5 batch sweep: batch 1-4 +0.1 ms/step without this; crossover between 3760 and 5640 rows)
    if (lens_geglu || (r3 && h->fuse_geglu && a.geglu_stream && geglu_eligible(d, Tl, pr) && M >= g_geglu_min_rows)) {
      // the token rows stay in LDS, only weights stream (csrc/geglu.hip): half the L2 -> LDS bytes of the GEMM below
      ns2vc_geglu_args f;
      memset(&f, 0, sizeof(f));
      f.yn = yn; f.ldy = d; f.ln_stats = r3; f.ln_eps = 1e-5f;
      if (lens_geglu) { f.yn = qb; f.ln_stats = nullptr; f.T = Tl; f.lens = lens_of(Tl); }
      f.wstream = a.geglu_stream; f.consts = a.geglu_consts;
      f.out_op = ffh; f.ldo = 4 * d; f.M = M; f.dim = d; f.ln_health = h->ln_health;
      add(t + ".ff.geglu[token-stationary]", [=](hipStream_t s) { return launch_geglu(f, pr, s); }, 1, 2.0 * M * (double)d * 8.0 * d,
          (double)M * d * opsz * 5.0 + (double)M * (d / 64) * 8.0 + 8.0 * d * d * opsz);
    } else {
      g = base(yn, d, d, Tl, Tl, a.ff1, nullptr, ffh, 4 * d);
      g.geglu = 1;
      consume(g, r3, a.ff1);
      gemm(t + ".ff.geglu", g);
    }
    if (fold) {
      // out = [Wpo W2 | Wpo] [ffh | yn] + (Wpo b2 + bpo) + x : ff.net.2 and proj_out in one launch
      g = base(ffh, 4 * d, 4 * d, Tl, Tl, a.ffpo, out, out_op, d);
      g.a2 = yraw; g.lda2 = d; g.c2 = d;
      g.res = x; g.ldres = d;
      g.stats = new_stats(out, Tl, d);
      gemm(a.prefix + ".ff.out+proj_out", g);
    } else {
      g = base(ffh, 4 * d, 4 * d, Tl, Tl, a.ff2, nullptr, yn, d);     // y_final = y + ff(...) is only consumed by proj_out: operand copy only
      g.res = y; g.ldres = d;
      gemm(t + ".ff.out", g);
      g = base(yn, d, d, Tl, Tl, a.proj_out, out, out_op, d);
      g.res = x; g.ldres = d;
      g.stats = new_stats(out, Tl, d);
      gemm(a.prefix + ".proj_out", g);
    }
  }
};
}  // namespace

int build_plan(ns2vc_unet* h, bool sizing) {
  const auto& c = h->cfg;
  const int B = h->B, T = h->T, Lp = h->Lp, nl = c.n_levels;
  const int c0 = c.block_out_channels[0], E = 4 * c0, cross = c.cross_attention_dim, CP = h->CP;
  const std::vector<int> Ts = level_lengths(T, nl);

  Planner P;
  P.h = h; P.sizing = sizing; P.B = B; P.T = T; P.Lp = Lp; P.G = c.norm_num_groups; P.prec = h->prec;
  P.opsz = operand_bytes(h->prec);
  const int prec = h->prec;
  if (!sizing) { h->cond_ops.clear(); h->fwd_ops.clear(); h->taps.clear(); }

  size_t maxMC = 0, maxIn = 0;   // max over levels of B*Tl*C (outputs) / over resnets of B*Tl*Cin (concat inputs)
  int maxC = 0;
  for (int l = 0; l < nl; ++l) {
    // an upsampler writes the COARSER level's channel count at this level's length
    const int cmax = std::max(c.block_out_channels[l], c.block_out_channels[std::min(l + 1, nl - 1)]);
    maxMC = std::max(maxMC, (size_t)B * Ts[l] * cmax);
    maxC = std::max(maxC, c.block_out_channels[l]);
  }
  for (const auto& b : h->blocks)
    for (const auto& r : b.res) maxIn = std::max(maxIn, (size_t)B * Ts[b.level] * r.cin);
  maxIn = std::max(maxIn, maxMC);
  // ---- persistent state
  h->xe = P.alloc<float>((size_t)B * T * CP); h->xbar = P.alloc<float>((size_t)B * T * CP);
  h->d1 = P.alloc<float>((size_t)B * T * CP); h->mprev = P.alloc<float>((size_t)B * T * CP);
  h->x0 = P.alloc<float>((size_t)B * T * CP);
  // 16-bit engines keep the two inputs of conv_in as hi + lo operand pairs, rows [hi(C) | lo(C)] (common.h op_rest): the lo planes are read with split_io only
  const int pw = prec != PREC_F32 ? 2 : 1;
  h->xe_op = P.alloc_op((size_t)B * T * CP * pw);
  h->content_op = P.alloc_op((size_t)B * T * c.content_channels * pw);
  const bool pio = h->split_io && prec != PREC_F32 && !h->exact_io;
  const bool xio = h->exact_io && prec != PREC_F32;            // conv_in / conv_out / time_emb_proj with fp32 operands inside a 16-bit engine
  h->content_f32 = xio ? P.alloc<float>((size_t)B * T * c.content_channels) : nullptr;
  h->emb_act_f32 = xio ? P.alloc<float>((size_t)B * E) : nullptr;
  h->content_conv = P.alloc<float>((size_t)B * T * c0);
  h->prompt = P.alloc<float>((size_t)B * Lp * cross);
  h->prompt_op = P.alloc_op((size_t)B * Lp * cross);
  h->maskbias = P.alloc<float>((size_t)B * Lp);
  h->mask_dev = P.alloc<uint8_t>((size_t)B * Lp);
  h->aug = P.alloc<float>((size_t)B * E); h->emb = P.alloc<float>((size_t)B * E);
  h->emb_act_op = P.alloc_op((size_t)B * E);
  h->temb = P.alloc<float>((size_t)B * h->temb_all.N);
  h->kv = P.alloc_op((size_t)B * Lp * h->kv_all.N);
  h->seq = P.alloc<float>((size_t)B * (Lp + 1) * cross);
  h->seq_op = P.alloc_op((size_t)B * (Lp + 1) * cross);
  h->pool_qkv_buf = P.alloc<float>((size_t)B * (Lp + 1) * h->pool_qkv.N);
  h->pooled = P.alloc<float>((size_t)B * cross);
  h->t_dev = P.alloc<float>((size_t)B);
  h->step_dev = P.alloc<int>(64);
  h->ln_health = P.alloc<unsigned>(64);
  h->attn_fallbacks = h->ln_health + 32;          // (same zero-initialised block; the LayerNorm read-out uses words 0 and 16, the cooperative GroupNorm prologue's counter word 48)
  // per-item valid lengths: the two tables sit BEHIND everything the dense plan of this shape carves (h->lens.off, measured by prepare's sizing
  // pass), so the dense plan's layout is the one it had without them, and a masked rebuild (which carves no more) finds them where they were
  size_t lens_bytes = 0;
  {
    size_t nb = 0;
    for (int l = 0; l < nl; ++l) nb += (size_t)B * Ts[l];
    const size_t lb = (((size_t)nl * B * sizeof(int)) + 255) & ~(size_t)255;
    lens_bytes = lb + ((nb * sizeof(float) + 255) & ~(size_t)255);
    h->lens.dev = sizing ? nullptr : reinterpret_cast<int*>(static_cast<char*>(h->arena) + h->lens.off);
    h->lens.selfbias = sizing ? nullptr : reinterpret_cast<float*>(static_cast<char*>(h->arena) + h->lens.off + lb);
    // ... and the per-item prompt lengths [B] behind both (ns2vc_unet_set_prompt_lengths)
    h->plens.dev = sizing ? nullptr : reinterpret_cast<int*>(static_cast<char*>(h->arena) + h->lens.off + lens_bytes);
    lens_bytes += ((size_t)B * sizeof(int) + 255) & ~(size_t)255;
  }
  const int* plens = h->plens.on ? h->plens.dev : nullptr;
  P.masked = h->lens.masked;
  P.fused = h->lens.masked && h->masked_fuse;
  P.Ts = Ts;
  // ---- shared scratch
  P.gn_rows = 32;
  P.gn_partial = P.alloc<double>((size_t)B * ((T + P.gn_rows - 1) / P.gn_rows) * c.norm_num_groups * 2);
  P.xn = P.alloc_op(maxIn); P.xr = P.alloc_op(maxIn);
  P.rs1 = P.alloc<float>(maxMC / 32); P.rs2 = P.alloc<float>(maxMC / 32); P.rs3 = P.alloc<float>(maxMC / 32);
  float* h1 = P.alloc<float>(maxMC);
  void* hn = P.alloc_op(maxMC);
  float* y = P.alloc<float>(maxMC);
  void* yn = P.alloc_op(maxMC);
  void* qkv = P.alloc_op(3 * maxMC);
  void* ao = P.alloc_op(maxMC);
  void* qb = P.alloc_op(maxMC);
  void* ffh = P.alloc_op(4 * maxMC);
  void* samp_in = P.alloc_op(maxMC);        // operand copy of a block output that a down/up-sampling conv reads
  float* ua = P.alloc<float>(maxMC);
  float* ub = P.alloc<float>(maxMC);
  float* uc = P.alloc<float>(maxMC);

  // ================= condition plan (once per utterance batch) =================
  P.ops = &h->cond_ops;
  {
    float *prompt = h->prompt, *seq = h->seq, *pq = h->pool_qkv_buf, *pooled = h->pooled, *aug = h->aug;
    void *prompt_op = h->prompt_op, *seq_op = h->seq_op;
    // content half of conv_in (+ conv_in bias)
    const int cc = c.content_channels;
    GemmArgs g = xio ? P.base(h->content_f32, cc, cc, T, T, h->conv_in_c32, h->content_conv, nullptr, c0)
               : pio ? P.base(h->content_op, 2 * cc, 2 * cc, T, T, h->conv_in_cp, h->content_conv, nullptr, c0)
                     : P.base(h->content_op, pw * cc, cc, T, T, h->conv_in_c, h->content_conv, nullptr, c0);
    if (pio) { g.a1 = h->content_op; g.lda1 = 2 * cc; g.c1 = cc; }       // [hi | lo] then hi once more, against (hi(w) | hi(w) | lo(w))
    g.taps = 3;
    P.gemm("cond.conv_in.content", g, xio ? PREC_F32 : -1);
    if (!sizing) h->cond_split = h->cond_ops.size();
    // all cross-attention k|v projections in one GEMM: prompt [B*Lp][cross] x [n_kv][cross]^T -> operand tensor
    const size_t np = (size_t)B * Lp * cross;
    // per-item prompt lengths: the prompt copy's rows past an item's frames -> 0, so that every row-wise launch below sees finite rows whatever the
    // caller's padding holds
    if (plens) P.add("cond.prompt.mask", [=](hipStream_t s) { return launch_mask_rows(prompt, (size_t)cross * 4, (size_t)cross * 4, B, Lp, plens, s); }, 4);
    P.add("cond.prompt.cast", [=](hipStream_t s) { return launch_cast_op(prompt, np, prompt_op, prec, s); });
    g = P.base(prompt_op, cross, cross, Lp, Lp, h->kv_all, nullptr, h->kv, h->kv_all.N);
    P.gemm("cond.cross_kv", g);
    // r6: the V^T images of the blocks whose cross-attention runs inside the fused feed-forward kernel (ffn.hip ATT): one small launch each, once per utterance
    for (const auto& b : h->blocks)
      for (const auto& at : b.attn)
        if (P.xattn_fused(at, Ts[b.level])) {
          const int ldv = h->kv_all.N, hdv = at.dim / 8, Bq = B, Lq = Lp;
          void* vt = P.alloc_op(xattn_pack_bytes(B, Lp, hdv) / 2);
          P.xattn_vt[at.prefix] = vt;
          const void* ksrc = P.op_off(h->kv, (size_t)at.kv_off);
          const void* vsrc = P.op_off(h->kv, (size_t)(at.kv_off + at.dim));
          P.add("cond.cross_kv_image." + at.prefix, [=](hipStream_t s) { return launch_xattn_pack(ksrc, ldv, vsrc, ldv, Bq, Lq, hdv, vt, prec, s); }, 4);
        }
    // add_embedding = TextTimeEmbedding(prompt)
    const float *n1g = h->p_n1g, *n1b = h->p_n1b, *pos = h->p_pos, *projT = h->p_projT, *projb = h->p_projb, *n2g = h->p_n2g, *n2b = h->p_n2b;
    const int ph_ = c.pool_heads;
    const size_t ns = (size_t)B * (Lp + 1) * cross;
    P.add("cond.pool.ln1", [=](hipStream_t s) { return launch_ln_apply(prompt, B * Lp, cross, 1e-5f, n1g, n1b, seq, Lp, 0, s); });
    P.add("cond.pool.cls", [=](hipStream_t s) { return launch_pool_cls(seq, B, Lp, cross, pos, s, plens); });
    P.add("cond.pool.cast", [=](hipStream_t s) { return launch_cast_op(seq, ns, seq_op, prec, s); });
    g = P.base(seq_op, cross, cross, Lp + 1, Lp + 1, h->pool_qkv, pq, nullptr, h->pool_qkv.N);
    P.gemm("cond.pool.qkv", g);
    const int ldq = h->pool_qkv.N;
    if (ldq != 3 * cross) return fail("pool qkv width %d must equal 3*cross=%d (cross must be a multiple of 128)", ldq, 3 * cross);
    if ((ns & 3) || (np & 3)) return fail("internal: cast sizes must be multiples of 4");
    P.add("cond.pool.attn", [=](hipStream_t s) { return launch_pool_attn(pq, B, Lp + 1, cross, ph_, pooled, s, plens); });
    P.add("cond.pool.proj", [=](hipStream_t s) { return launch_pool_proj(pooled, B, cross, projT, projb, E, n2g, n2b, 1e-5f, aug, s); });
    P.tap("aug", aug, B, E);
  }

  // ================= per-step forward plan =================
  P.ops = &h->fwd_ops;
  {
    const size_t cap = (size_t)1 << 20;                 // 8 MB of int64 statistics slots
    P.stats_pool = P.alloc<long long>(cap);
    P.stats_cap = cap; P.stats_used = 0;
    long long* pool = P.stats_pool;
    ns2vc_unet* hq = h;
    // first launch of every forward: clears the statistics pool and, in the sampling loop, advances the step counter
    // (ns2vc_sampler_run starts it at -1; a plain forward does not read it)
    P.add("gn_stats.clear", [=](hipStream_t s) { return launch_zero(pool, hq->stats_bytes, s, hq->step_dev); }, 4);
  }
  {
    ns2vc_unet* hh = h;
    const float *w1t = h->t_w1t, *b1 = h->t_b1, *w2t = h->t_w2t, *b2 = h->t_b2, *aug = h->aug;
    float *emb = h->emb, *tdev = h->t_dev;
    void* emb_act = xio ? (void*)h->emb_act_f32 : h->emb_act_op;
    const int eprec = xio ? PREC_F32 : prec;                    // type SiLU(emb) is written in
    const int tdim = c0;
    if (!sizing) { h->tfork.begin = (int)h->fwd_ops.size(); h->tfork.join = h->tfork.first = -1; h->tfork.readers = 0; }
    P.add("time_embed", [=](hipStream_t s) {
      // sampling loop: the MLP of every step's timestep was evaluated once for the table (ns2vc_sampler_run), a step adds aug
      // (per-item schedules: every item the row of its own table -- chosen at launch time like the table itself, the plan does not change)
      if (hh->use_step_table && hh->items.on)
        return launch_emb_items_from_table(hh->temb_table, hh->step_dev, hh->items.dev, hh->items.n, aug, emb, emb_act, eprec, B, E, s);
      if (hh->use_step_table) return launch_emb_from_table(hh->temb_table, hh->step_dev, aug, emb, emb_act, eprec, B, E, s);
      return launch_time_embed(tdev, 1, nullptr, 0, w1t, b1, w2t, b2, aug, emb, emb_act, eprec, B, tdim, E, s);
    });
    P.tap("emb", emb, B, E);
    // every resnet's time_emb_proj(SiLU(emb)) in one GEMM (M = B)
    GemmArgs g = P.base(emb_act, E, E, 1, 1, xio ? h->temb_all32 : h->temb_all, h->temb, nullptr, h->temb_all.N);
    P.gemm("time_emb_proj.all", g, xio ? PREC_F32 : -1);
    if (!sizing) h->tfork.end = (int)h->fwd_ops.size();
  }
  // skip stack
  struct Skip { float* p; int C; int l; };
  std::vector<Skip> skips;
  auto new_skip = [&](int l) { float* p = P.alloc<float>((size_t)B * Ts[l] * c.block_out_channels[l]); skips.push_back({p, c.block_out_channels[l], l}); return p; };
  {
    float* s0 = new_skip(0);
    GemmArgs g = xio ? P.base(h->xe, CP, CP, T, T, h->conv_in_x32, s0, nullptr, c0)          // (the fp32 solver state IS the fp32 operand: no copy involved)
               : pio ? P.base(h->xe_op, 2 * CP, 2 * CP, T, T, h->conv_in_xp, s0, nullptr, c0)
                     : P.base(h->xe_op, pw * CP, CP, T, T, h->conv_in_x, s0, nullptr, c0);
    if (pio) { g.a1 = h->xe_op; g.lda1 = 2 * CP; g.c1 = CP; }
    g.taps = 3; g.res = h->content_conv; g.ldres = c0;
    g.stats = P.new_stats(s0, T, c0);
    P.gemm("conv_in", g, xio ? PREC_F32 : -1);
    P.tap("conv_in", s0, B * T, c0);
  }
  const float* cur = skips.back().p;
  int curC = c0;
  for (const auto& b : h->blocks) {
    const int l = b.level, Tl = Ts[l];
    const std::string tag = b.kind == "mid" ? "mid" : b.kind + std::to_string(b.index);
    if (b.kind == "down") {
      for (size_t j = 0; j < b.res.size(); ++j) {
        const bool has_attn = !b.attn.empty();
        const bool last = (j + 1 == b.res.size());
        float* rout = has_attn ? ua : new_skip(l);
        P.resnet(b.res[j], cur, curC, curC, nullptr, 0, 0, Tl, h1, hn, rout, (!has_attn && last && b.sampler) ? samp_in : nullptr);
        P.tap(tag + ".res" + std::to_string(j), rout, B * Tl, b.channels);
        cur = rout; curC = b.channels;
        if (has_attn) {
          float* aout = new_skip(l);
          P.transformer(b.attn[j], cur, Tl, y, yn, qkv, ao, qb, ffh, aout, (last && b.sampler) ? samp_in : nullptr);
          P.tap(tag + ".attn" + std::to_string(j), aout, B * Tl, b.channels);
          cur = aout;
        }
      }
      if (b.sampler == 1) {
        float* ds = new_skip(l + 1);
        skips.back().C = b.channels;     // this block's channels at the next level's length
        GemmArgs g = P.base(samp_in, curC, curC, Tl, Ts[l + 1], b.samp, ds, nullptr, b.channels);
        g.taps = 3; g.tmode = TMODE_DOWN2;
        g.stats = P.new_stats(ds, Ts[l + 1], b.channels);
        P.gemm(tag + ".downsample", g);
        P.tap(tag + ".ds", ds, B * Ts[l + 1], b.channels);
        cur = ds;
      }
    } else if (b.kind == "mid") {
      P.resnet(b.res[0], cur, curC, curC, nullptr, 0, 0, Tl, h1, hn, ua, nullptr);
      P.tap("mid.res0", ua, B * Tl, b.channels);
      P.transformer(b.attn[0], ua, Tl, y, yn, qkv, ao, qb, ffh, ub, nullptr);
      P.tap("mid.attn0", ub, B * Tl, b.channels);
      P.resnet(b.res[1], ub, b.channels, b.channels, nullptr, 0, 0, Tl, h1, hn, uc, nullptr);
      P.tap("mid.res1", uc, B * Tl, b.channels);
      cur = uc; curC = b.channels;
    } else {
      for (size_t j = 0; j < b.res.size(); ++j) {
        const Skip sk = skips.back();
        skips.pop_back();
        const bool last = (j + 1 == b.res.size());
        const bool has_attn = !b.attn.empty();
        if (sk.l != l) return fail("internal: skip level mismatch at %s", b.res[j].prefix.c_str());
        if (curC + sk.C != b.res[j].cin) return fail("internal: concat width %d+%d != %d at %s", curC, sk.C, b.res[j].cin, b.res[j].prefix.c_str());
        float* rout = (cur == ua) ? ub : ua;
        if (rout == cur) rout = uc;
        P.resnet(b.res[j], cur, curC, curC, sk.p, sk.C, sk.C, Tl, h1, hn, rout, (!has_attn && last && b.sampler) ? samp_in : nullptr);
        P.tap(tag + ".res" + std::to_string(j), rout, B * Tl, b.channels);
        cur = rout; curC = b.channels;
        if (has_attn) {
          float* aout = (cur == ua) ? ub : ua;
          P.transformer(b.attn[j], cur, Tl, y, yn, qkv, ao, qb, ffh, aout, (last && b.sampler) ? samp_in : nullptr);
          P.tap(tag + ".attn" + std::to_string(j), aout, B * Tl, b.channels);
          cur = aout;
        }
      }
      if (b.sampler == 2) {
        float* us = (cur == uc) ? ua : uc;
        GemmArgs g = P.base(samp_in, curC, curC, Tl, Ts[l - 1], b.samp, us, nullptr, b.channels);
        g.taps = 3; g.tmode = TMODE_UP2;
        if (P.masked) {
          // (the fused form would read source row L >> 1 -- a valid row when the finer level's length L is odd -- as the halo of output row L - 1:
          //  the upsampled rows are materialised in P.xn, zero past every item's end, and convolved like any stride-1 input)
          const int Td = Ts[l - 1], Bq = B;
          const size_t rb = (size_t)curC * P.opsz;
          void* dst = P.xn;
          const void* src = samp_in;
          const int* lens = P.lens_of(Td);
          P.add(tag + ".upsample.nearest", [=](hipStream_t s) { return launch_mask_rows(dst, rb, rb, Bq, Td, lens, s, src, rb, Tl, 1); }, 4, 0.0, 3.0 * Bq * Td * rb);
          g = P.base(P.xn, curC, curC, Td, Td, b.samp, us, nullptr, b.channels);
          g.taps = 3;
        }
        g.stats = P.new_stats(us, Ts[l - 1], b.channels);
        P.gemm(tag + ".upsample", g);
        P.tap(tag + ".us", us, B * Ts[l - 1], b.channels);
        cur = us;
      }
    }
  }
  if (!skips.empty()) return fail("internal: %zu skips left over", skips.size());
  {
    // split_io: conv_out reads a hi + lo operand pair -- written by its fused GroupNorm prologue (gnp_pair) or by the gn_apply launch, the same bytes either way
    const bool po = pio && 2 * curC <= 3 * c0 && h->conv_outp.w;
    const auto pno = P.groupnorm("conv_norm_out", cur, curC, curC, nullptr, 0, 0, T, 1e-5f, h->out_ng, h->out_nb, nullptr, 0, 0, 1, P.xn, nullptr, h->conv_out.N, 3, po ? 1 : 0);
    // exact_io: only where the norm is the conv's prologue (it then writes fp32 operand rows: xn holds 2-byte elements of up to 3 x 128 channels per row, i.e. room for 128 fp32)
    const bool xo = xio && pno.x != nullptr && (size_t)curC * 4 <= (size_t)3 * c0 * P.opsz;
    GemmArgs g = po ? P.base(P.xn, 2 * curC, 2 * curC, T, T, h->conv_outp, h->x0, nullptr, CP)
                    : P.base(P.xn, curC, curC, T, T, xo ? h->conv_out32 : h->conv_out, h->x0, nullptr, CP);
    if (po) { g.a1 = P.xn; g.lda1 = 2 * curC; g.c1 = curC; g.gnp_pair = pno.x ? 1 : 0; }       // [hi | lo] then hi once more (3 x 128 columns: what a row of xn holds)
    g.taps = 3;
    P.gn_fuse(g, pno);
    if (h->conv_out.N != CP) return fail("internal: conv_out padded width %d != %d", h->conv_out.N, CP);
    const int conv_out_at = (int)h->fwd_ops.size();      // (the conv_out launch itself: a masked plan appends the zeroing of x0's padded rows behind it)
    P.gemm("conv_out", g, xo ? PREC_F32 : -1);
    if (!sizing) { h->conv_out_g = g; h->conv_out_idx = conv_out_at; h->conv_out_prec = xo ? PREC_F32 : prec; }
    P.tap("out", h->x0, B * T, CP);
  }
  if (sizing) { h->lens.off = P.off; P.off += lens_bytes; }
  else if (P.off > h->lens.off) {       // (the tables' place: a rebuild must carve no more than the plan that measured it)
    h->cond_ops.clear(); h->fwd_ops.clear(); h->taps.clear();
    return fail("internal: plan needs %zu bytes in front of the length tables at %zu (re-run ns2vc_unet_prepare)", P.off, h->lens.off);
  } else P.off = h->lens.off + lens_bytes;
  if (sizing) h->arena_bytes = P.off;
  else if (P.off > h->arena_bytes) {    // a rebuild must never carve past the allocation the sizing pass measured
    h->cond_ops.clear(); h->fwd_ops.clear(); h->taps.clear();
    return fail("internal: plan needs %zu bytes but the arena holds %zu (re-run ns2vc_unet_prepare)", P.off, h->arena_bytes);
  }
  h->arena_used = P.off;
  h->stats_bytes = std::max<size_t>(P.stats_used, 1) * sizeof(long long);
  // the fork of the timestep-embedding branch is only correct if every reader of its result is at or after the join
  h->tfork.ok = !sizing && h->tfork.begin > 0 && h->tfork.end > h->tfork.begin && h->tfork.join >= h->tfork.end && h->tfork.first >= h->tfork.join;
  if (!sizing && h->fork_temb && !h->tfork.ok)
    fprintf(stderr, "ns2vc: fork_temb refused for this plan (join at launch %d, first reader of the time scale / shift rows at %d): the step graph stays linear\n",
            h->tfork.join, h->tfork.first);
  return 0;
}

// does a captured step run the timestep-embedding branch on a forked stream (fork_temb)?  `last`: end of the fwd_ops range the step launches
bool temb_forks(const ns2vc_unet* h, size_t last) {
  return h->fork_temb && !h->debug && h->tfork.ok && (size_t)h->tfork.join <= last;
}

int run_ops(const std::vector<Op>& ops, hipStream_t s, size_t first, size_t last) {
  for (size_t i = first; i < std::min(last, ops.size()); ++i) {
    hipError_t e = ops[i].fn(s);
    if (e != hipSuccess) {
      const int line = last_gemm_refusal_line();
      if (line) return fail("launch of '%s' failed: %s (refused by the argument check at gemm.hip:%d)", ops[i].name.c_str(), hipGetErrorString(e), line);
      return fail("launch of '%s' failed: %s", ops[i].name.c_str(), hipGetErrorString(e));
    }
  }
  return 0;
}

// the captured step graph bakes in the plan's launches and pointers: whatever changes either drops it, and the next captured loop records it again
void drop_step_graph(ns2vc_unet* h) {
  if (h->step_graph) { (void)hipGraphExecDestroy(h->step_graph); h->step_graph = nullptr; }
}
void drop_plan(ns2vc_unet* h) {
  drop_step_graph(h);
  if (h->arena) { (void)hipDeviceSynchronize(); (void)hipFree(h->arena); h->arena = nullptr; }
  h->cond_ops.clear(); h->fwd_ops.clear(); h->taps.clear();
  h->arena_bytes = h->arena_used = 0;
  h->next_step = -1;           // the solver state lived in the arena
  h->slots.on = false;         // (... and so did a slot loop's)
  h->ln_out.posted = false;
  h->attn_fallbacks = nullptr; // (the counters lived in the arena too)
  h->tfork.ok = false;
  h->ln_health = nullptr;
}

}  // namespace ns2vc
