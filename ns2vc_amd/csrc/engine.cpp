// The engine's own part of the C ABI declared in include/ns2vc_hip.h: create / destroy, weights, options, prepare, condition, lengths,
// forward, and the read-outs (LayerNorm ratio, taps, op list, per-launch profile, counters).  Weight packing is pack.cpp, the launch
// plan plan.cpp, the sampling loop sampler.cpp; the entry points that take no engine handle are abi_kernels.cpp.
#include "engine_internal.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

using namespace ns2vc;

// Every entry point that touches the device binds the calling thread to the engine's device first: weights, arena and
// the captured graph live there, and launches go to the CURRENT device (a model on cuda:1 called while cuda:0 is
// current would otherwise launch on the wrong GPU with cross-device pointers).
static int bind_device(ns2vc_unet* h) {
  int cur = -1;
  HIPCHK(hipGetDevice(&cur));
  if (cur != h->device) HIPCHK(hipSetDevice(h->device));
  return 0;
}
int ns2vc::check_ready(ns2vc_unet* h, bool need_plan) {
  if (!h) return fail("null engine handle");
  if (bind_device(h)) return 1;
  if (!h->finalized) return fail("weights not finalized (call ns2vc_unet_finalize_weights)");
  if (need_plan && !h->arena) return fail("engine not prepared (call ns2vc_unet_prepare)");
  return 0;
}

// x [B][C][T] -> the solver state, channels-last: the fp32 rows and their operand copy (16-bit: the hi + lo pair);
// masked plans: the rows past every item's end of both -> 0
int ns2vc::load_state(ns2vc_unet* h, const float* x_bct, hipStream_t s, int items) {
  const int B = items > 0 ? items : h->B;
  HIPCHK(launch_nct_to_btc(x_bct, h->cfg.latent_channels, h->T, B, h->xe, h->xe_op, h->prec, h->CP, h->CP, s, h->pair_width(), h->pair_off()));
  if (!h->lens.masked) return 0;
  const size_t ob = (size_t)h->pair_width() * operand_bytes(h->prec);
  HIPCHK(launch_mask_rows(h->xe, (size_t)h->CP * 4, (size_t)h->CP * 4, B, h->T, h->lens.dev, s));
  HIPCHK(launch_mask_rows(h->xe_op, ob, ob, B, h->T, h->lens.dev, s));
  return 0;
}

// every plan option: its name for ns2vc_unet_set_option, its switch in the environment (honoured under NS2VC_DEBUG_ENV=1 only) and the
// engine field, whose initialiser is the default
static const struct { const char* name; const char* env; bool ns2vc_unet::* member; } kOptions[] = {
  {"ln_linear", "NS2VC_LN_LINEAR", &ns2vc_unet::ln_linear}, {"fold_ff", "NS2VC_FOLD_FF", &ns2vc_unet::fold_ff},
  {"fuse_ffn", "NS2VC_FUSE_FFN", &ns2vc_unet::fuse_ffn}, {"fuse_ffn_pre", "NS2VC_FUSE_FFN_PRE", &ns2vc_unet::fuse_ffn_pre},
  {"fuse_geglu", "NS2VC_FUSE_GEGLU", &ns2vc_unet::fuse_geglu}, {"fuse_rows", "NS2VC_FUSE_ROWS", &ns2vc_unet::fuse_rows},
  {"fuse_rows_gn", "NS2VC_FUSE_ROWS_GN", &ns2vc_unet::fuse_rows_gn}, {"fuse_gn_gemm", "NS2VC_FUSE_GN_GEMM", &ns2vc_unet::fuse_gn_gemm},
  {"fuse_gn_cat", "NS2VC_FUSE_GN_CAT", &ns2vc_unet::fuse_gn_cat}, {"gn_coop", "NS2VC_GN_COOP", &ns2vc_unet::gn_coop},
  {"slice_rows", "NS2VC_SLICE_ROWS", &ns2vc_unet::slice_rows}, {"attn_fp8", "NS2VC_ATTN_FP8", &ns2vc_unet::attn_fp8},
  {"attn_optimistic", "NS2VC_ATTN_OPTIMISTIC", &ns2vc_unet::attn_optimistic}, {"conv_ts", "NS2VC_CONV_TS", &ns2vc_unet::conv_ts},
  {"conv_wtiled", "NS2VC_CONV_WTILED", &ns2vc_unet::conv_wtiled}, {"gn_inloop", "NS2VC_GN_INLOOP", &ns2vc_unet::gn_inloop},
  {"fuse_solver", "NS2VC_FUSE_SOLVER", &ns2vc_unet::fuse_solver}, {"fuse_xattn", "NS2VC_FUSE_XATTN", &ns2vc_unet::fuse_xattn},
  {"fork_temb", "NS2VC_FORK_TEMB", &ns2vc_unet::fork_temb}, {"exact_io", "NS2VC_EXACT_IO", &ns2vc_unet::exact_io},
  {"split_io", "NS2VC_SPLIT_IO", &ns2vc_unet::split_io}, {"masked_fuse", "NS2VC_MASKED_FUSE", &ns2vc_unet::masked_fuse},
  {"masked_attn", "NS2VC_MASKED_ATTN", &ns2vc_unet::masked_attn}, {"masked_rows", "NS2VC_MASKED_ROWS", &ns2vc_unet::masked_rows},
  {"masked_ffn", "NS2VC_MASKED_FFN", &ns2vc_unet::masked_ffn}, {"masked_geglu", "NS2VC_MASKED_GEGLU", &ns2vc_unet::masked_geglu},
  {"attn_resident", "NS2VC_ATTN_RESIDENT", &ns2vc_unet::attn_resident},
  {"masked_attn_resident", "NS2VC_MASKED_ATTN_RESIDENT", &ns2vc_unet::masked_attn_resident}};
static bool* option_ptr(ns2vc_unet* h, const char* name) {
  for (const auto& o : kOptions)
    if (!strcmp(name, o.name)) return &(h->*o.member);
  return nullptr;
}

extern "C" {

int ns2vc_unet_create(const ns2vc_unet_cfg* cfg, ns2vc_unet** out) {
  if (!cfg || !out) return fail("null argument");
  // every message names the offending field (ns2vc_amd.spec.engine_supports states the same predicate); the divisors are range-checked
  // before they divide
  if (cfg->n_levels < 2 || cfg->n_levels > NS2VC_MAX_LEVELS) return fail("n_levels=%d out of range (2..%d)", cfg->n_levels, NS2VC_MAX_LEVELS);
  if (cfg->latent_channels <= 0 || cfg->latent_channels > 128) return fail("latent_channels=%d must be in 1..128", cfg->latent_channels);
  if (cfg->content_channels <= 0 || cfg->content_channels % 64)
    return fail("content_channels=%d must be a positive multiple of 64", cfg->content_channels);
  if (cfg->cross_attention_dim <= 0 || cfg->cross_attention_dim % 128)
    return fail("cross_attention_dim=%d must be a positive multiple of 128", cfg->cross_attention_dim);
  if (cfg->heads < 1) return fail("heads=%d must be >= 1", cfg->heads);
  if (cfg->norm_num_groups < 1 || cfg->norm_num_groups > 8) return fail("norm_num_groups=%d unsupported (1..8)", cfg->norm_num_groups);
  if (cfg->layers_per_block < 1) return fail("layers_per_block=%d must be >= 1", cfg->layers_per_block);
  if (cfg->pool_heads < 1 || cfg->cross_attention_dim % cfg->pool_heads || cfg->cross_attention_dim / cfg->pool_heads > 8)
    return fail("cross_attention_dim=%d over pool_heads=%d: the pool head width must be a whole number <= 8", cfg->cross_attention_dim, cfg->pool_heads);
  if (cfg->block_out_channels[0] != 128) return fail("block_out_channels[0]=%d must be 128 (padded latent width)", cfg->block_out_channels[0]);
  for (int l = 0; l < cfg->n_levels; ++l) {
    const int c = cfg->block_out_channels[l];
    // (a multiple of 128: the transformer's LayerNorm -- by linearity or explicit, ln_apply_op -- takes rows of 128k <= 512 channels)
    if (c <= 0 || c % 128 || c > 512) return fail("block_out_channels[%d]=%d must be a multiple of 128 in 128..512", l, c);
    if (c % cfg->heads) return fail("block_out_channels[%d]=%d not divisible by heads=%d", l, c, cfg->heads);
    const int hd = c / cfg->heads;
    if (hd != 16 && hd != 32 && hd != 48 && hd != 64)
      return fail("heads=%d gives head width %d at block_out_channels[%d]=%d (16/32/48/64 supported)", cfg->heads, hd, l, c);
    if (c % cfg->norm_num_groups || (c / cfg->norm_num_groups) % 4)
      return fail("block_out_channels[%d]=%d incompatible with norm_num_groups=%d (group width must be a multiple of 4)", l, c, cfg->norm_num_groups);
  }
  // the GroupNorm kernels take groups of at most 128 channels: the widest GroupNorm input is an up block's concat [h ; skip]
  for (const BlockW& b : make_topology(*cfg))
    for (const ResnetW& r : b.res)
      if (r.cin / cfg->norm_num_groups > 128)
        return fail("norm_num_groups=%d: the GroupNorm over the %d input channels of %s has groups of %d channels (<= 128 supported)",
                    cfg->norm_num_groups, r.cin, r.prefix.c_str(), r.cin / cfg->norm_num_groups);
  const hipError_t e = init_all_attributes();
  if (e != hipSuccess) return fail("kernel attribute setup failed: %s (is a gfx950 GPU visible?)", hipGetErrorString(e));
  auto* h = new ns2vc_unet();
  h->cfg = *cfg;
  if (hipGetDevice(&h->device) != hipSuccess) { delete h; return fail("hipGetDevice failed"); }
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0) h->cus = prop.multiProcessorCount;
    h->bn128_min = h->cus * 5 / 8;             // 128-column tap-sharing tiles while they still give 5/8 of the CUs a workgroup (160 of 256)
  }
  // rows shared between workgroups through an XCD's L2 only where the placement probe has SEEN ids 8 apart on one XCD (and even then
  // every workgroup checks its own placement, gnpro.h)
  h->xcd_probe = xcd_round_robin_of_current_device();
  h->gn_coop = h->xcd_probe == 1;
  // plan switches from the environment: tuning / A-B runs only (tools/ab_libs.sh), honoured when NS2VC_DEBUG_ENV=1 -- a served engine's
  // launch plan is set through ns2vc_unet_set_option and never changes behind the caller's back
  if (const char* dbg = getenv("NS2VC_DEBUG_ENV"); dbg && atoi(dbg) != 0) {
    for (const auto& o : kOptions)
      if (const char* v = getenv(o.env)) h->*o.member = atoi(v) != 0;
    if (h->xcd_probe != 1) h->gn_coop = false;
    {   // loader waves (4 | 8) and consumer layout (NS2VC_TS_KS = 1: K-split, 0: plain) of the tap-sharing conv kernel, process-wide
      const char* nl = getenv("NS2VC_TS_NL");
      const char* ks = getenv("NS2VC_TS_KS");
      if (nl || ks) set_forced_gemm_tile(-4, ks ? (atoi(ks) ? 1 : 2) : 0, nl ? atoi(nl) : 0);
    }
    if (const char* v = getenv("NS2VC_GN_COOP_MIN")) h->gn_coop_min = atoi(v);
    if (const char* v = getenv("NS2VC_TS_BN128_MIN")) h->bn128_min = atoi(v) > 0 ? atoi(v) : h->bn128_min;        // workgroups a 128-column tiling must still give to be chosen
  }
  h->blocks = make_topology(*cfg);
  build_expected(h);
  *out = h;
  return 0;
}

int ns2vc_unet_destroy(ns2vc_unet* h) {
  if (h) (void)bind_device(h);
  delete h;
  return 0;
}

int ns2vc_unet_load_weight(ns2vc_unet* h, const char* key, const void* data, const int64_t* shape, int ndim) {
  if (!h || !key || !data) return fail("null argument");
  if (bind_device(h)) return 1;
  std::string k(key);
  const std::vector<int64_t>* want = nullptr;
  for (const auto& e : h->expected) if (e.first == k) { want = &e.second; break; }
  if (!want) return fail("unexpected weight key '%s'", key);
  if ((int)want->size() != ndim) return fail("%s: ndim %d != expected %zu", key, ndim, want->size());
  for (int i = 0; i < ndim; ++i) if (shape[i] != (*want)[i]) return fail("%s: shape[%d]=%lld != expected %lld", key, i, (long long)shape[i], (long long)(*want)[i]);
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  t.data.resize(t.numel());
  HIPCHK(hipMemcpy(t.data.data(), data, t.numel() * sizeof(float), hipMemcpyDefault));
  h->raw[k] = std::move(t);
  h->finalized = false;
  return 0;
}

int ns2vc_unet_num_missing_weights(ns2vc_unet* h, char* first_missing, int buflen) {
  int n = 0;
  for (const auto& e : h->expected)
    if (!h->raw.count(e.first)) {
      if (n == 0 && first_missing && buflen > 0) snprintf(first_missing, buflen, "%s", e.first.c_str());
      ++n;
    }
  return n;
}

int ns2vc_unet_finalize_weights(ns2vc_unet* h, int precision) {
  if (!h) return fail("null engine handle");
  if (bind_device(h)) return 1;
  if (precision != NS2VC_PREC_F32 && precision != NS2VC_PREC_BF16 && precision != NS2VC_PREC_F16) return fail("unknown precision %d", precision);
  char first[256] = {0};
  const int miss = ns2vc_unet_num_missing_weights(h, first, sizeof(first));
  if (miss) return fail("%d weights missing, first: %s", miss, first);
  for (void* p : h->weight_allocs) (void)hipFree(p);
  h->weight_allocs.clear();
  h->prec = precision;
  if (pack_all(h)) return 1;
  h->finalized = true;
  h->temb_table_valid = false;
  drop_plan(h);       // a plan built for other weights holds stale pointers
  return 0;
}

int ns2vc_unet_set_debug(ns2vc_unet* h, int enable) {
  if (!h) return fail("null engine handle");
  if (bind_device(h)) return 1;
  if (h->debug != (enable != 0)) {
    h->debug = enable != 0;
    drop_plan(h);     // the tap copies change the arena size: a later rebuild must not carve a stale allocation
  }
  return 0;
}

int ns2vc_unet_set_option(ns2vc_unet* h, const char* name, int value) {
  if (!h || !name) return fail("null argument");
  if (bind_device(h)) return 1;
  if (!strcmp(name, "temb_join_skip")) {      // (a test knob, not a plan option: see ns2vc_unet_op_info which = 2)
    if (h->tfork.join_skip != std::max(value, 0)) { h->tfork.join_skip = std::max(value, 0); drop_plan(h); }
    return 0;
  }
  bool* opt = option_ptr(h, name);
  if (!opt) {
    std::string names;
    for (const auto& o : kOptions) names += (names.empty() ? "" : ", ") + std::string(o.name);
    return fail("unknown option '%s' (%s)", name, names.c_str());
  }
  // the cooperative GroupNorm prologue only where the placement probe of this device came back positive (r5)
  if (opt == &h->gn_coop && value != 0 && h->xcd_probe != 1) return fail("gn_coop needs workgroup ids 8 apart on one XCD; the placement probe of this device returned %d", h->xcd_probe);
  if (*opt != (value != 0)) { *opt = value != 0; drop_plan(h); }
  return 0;
}

// The maximum lives in the arena and is raised by the consumers' atomicMax on whatever stream the forward runs on, so the
// read-and-reset is a kernel + an async copy ON THAT STREAM (a host-side memset on the legacy stream raced with the
// non-blocking streams the engine is driven on, and a device-wide synchronize stalled the overlapped pipeline).
int ns2vc_unet_ln_ratio_post(ns2vc_unet* h, void* stream) {
  if (check_ready(h, true)) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (!h->ln_out.mail) {
    HIPCHK(hipHostMalloc((void**)&h->ln_out.mail, 64, hipHostMallocDefault));
    h->ln_out.mail[0] = 0;
  }
  if (!h->ln_out.event) HIPCHK(hipEventCreateWithFlags(&h->ln_out.event, hipEventDisableTiming));
  HIPCHK(launch_snapshot_u32(h->ln_health, h->ln_health + 16, s));
  HIPCHK(hipMemcpyAsync(h->ln_out.mail, h->ln_health + 16, sizeof(unsigned), hipMemcpyDeviceToHost, s));
  HIPCHK(hipEventRecord(h->ln_out.event, s));
  h->ln_out.posted = true;
  return 0;
}

int ns2vc_unet_ln_ratio_poll(ns2vc_unet* h, float* out_ratio, int* out_ready) {
  if (!h || !out_ratio || !out_ready) return fail("null argument");
  *out_ready = 0;
  *out_ratio = 0.f;
  if (!h->ln_out.posted) return 0;
  if (bind_device(h)) return 1;
  const hipError_t q = hipEventQuery(h->ln_out.event);
  if (q == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
  if (q != hipSuccess) return fail("hipEventQuery failed: %s", hipGetErrorString(q));
  memcpy(out_ratio, h->ln_out.mail, sizeof(float));
  *out_ready = 1;
  h->ln_out.posted = false;
  return 0;
}

int ns2vc_unet_ln_ratio(ns2vc_unet* h, float* out_ratio, void* stream) {
  if (!out_ratio) return fail("null argument");
  if (ns2vc_unet_ln_ratio_post(h, stream)) return 1;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  memcpy(out_ratio, h->ln_out.mail, sizeof(float));
  h->ln_out.posted = false;
  return 0;
}

int ns2vc_unet_prepare(ns2vc_unet* h, int B, int T, int Lp) {
  if (check_ready(h, false)) return 1;
  if (B <= 0 || T <= 0 || Lp <= 0) return fail("B, T, Lp must be positive");
  const int min_t = 1 << (h->cfg.n_levels - 1);
  if (T < min_t) return fail("T=%d too short for %d levels", T, h->cfg.n_levels);
  drop_plan(h);
  h->B = B; h->T = T; h->Lp = Lp;
  h->has_mask = false;
  h->lens.masked = false;         // a new shape starts dense (ns2vc_unet_set_lengths)
  h->lens.applied.clear();
  h->seeds.set = false;      // ... and without noise seeds (ns2vc_sampler_set_seeds)
  h->guide.on = false;       // ... and unguided (ns2vc_sampler_set_guidance)
  h->guide.n = 0;
  h->hold.on = false;        // ... and without known frames (ns2vc_sampler_set_known)
  h->hold.n = 0;
  h->hold.last.clear();
  h->shold.drop(h);          // ... a slot loop's too (ns2vc_sampler_open_known)
  h->plens.on = false;       // ... and with whole prompts (ns2vc_unet_set_prompt_lengths)
  h->plens.applied.clear();
  if (build_plan(h, true)) return 1;
  HIPCHK(hipMalloc(&h->arena, h->arena_bytes));
  HIPCHK(hipMemset(h->arena, 0, h->arena_bytes));
  if (build_plan(h, false)) return 1;
  return 0;
}

int ns2vc_unet_workspace_bytes(ns2vc_unet* h, size_t* out) {
  if (!h || !out) return fail("null argument");
  *out = h->arena_bytes;
  return 0;
}

int ns2vc_unet_set_content(ns2vc_unet* h, const float* content_bct, void* stream) {
  if (check_ready(h, true)) return 1;
  if (!content_bct) return fail("null condition tensor");
  hipStream_t s = (hipStream_t)stream;
  const auto& c = h->cfg;
  { const int pw = h->prec != PREC_F32 ? 2 : 1;      // (16-bit: the hi + lo pair, see prepare)
    HIPCHK(launch_nct_to_btc(content_bct, c.content_channels, h->T, h->B, h->content_f32, h->content_op, h->prec, c.content_channels, c.content_channels, s,
                             pw * c.content_channels, pw == 2 ? c.content_channels : 0));
    if (h->lens.masked) {    // content frames past an item's end read as the zero padding of an unpadded run (conv_in's halo)
      const size_t ob = (size_t)pw * c.content_channels * operand_bytes(h->prec);
      HIPCHK(launch_mask_rows(h->content_op, ob, ob, h->B, h->T, h->lens.dev, s));
      if (h->content_f32) HIPCHK(launch_mask_rows(h->content_f32, c.content_channels * 4, c.content_channels * 4, h->B, h->T, h->lens.dev, s));
    } }
  return run_ops(h->cond_ops, s, 0, h->cond_split);
}

int ns2vc_unet_set_mask(ns2vc_unet* h, const uint8_t* mask_bl, void* stream) {
  if (check_ready(h, true)) return 1;
  hipStream_t s = (hipStream_t)stream;
  const bool want_mask = mask_bl != nullptr;
  if (want_mask != h->has_mask) {
    // the cross-attention launches bake in whether a bias is read: rebuild the (cheap) plan; workspace offsets do not
    // depend on it, so everything already hoisted stays valid
    h->has_mask = want_mask;
    drop_step_graph(h);
    if (build_plan(h, false)) return 1;
  }
  if (want_mask) HIPCHK(hipMemcpyAsync(h->mask_dev, mask_bl, (size_t)h->B * h->Lp, hipMemcpyDeviceToDevice, s));
  // per-item prompt lengths: the row also drops the keys past an item's frames, with or without a mask
  if (h->plens.on) HIPCHK(launch_prompt_bias(want_mask ? h->mask_dev : nullptr, h->plens.dev, h->B, h->Lp, h->maskbias, s));
  else if (want_mask) HIPCHK(launch_mask_bias(h->mask_dev, h->B * h->Lp, h->maskbias, s));
  return 0;
}

int ns2vc_unet_set_prompt(ns2vc_unet* h, const float* prompt_blc, const uint8_t* mask_bl, void* stream) {
  if (!prompt_blc) return fail("null condition tensor");
  if (ns2vc_unet_set_mask(h, mask_bl, stream)) return 1;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(h->prompt, prompt_blc, (size_t)h->B * h->Lp * h->cfg.cross_attention_dim * sizeof(float), hipMemcpyDeviceToDevice, s));
  return run_ops(h->cond_ops, s, h->cond_split);
}

int ns2vc_unet_set_condition(ns2vc_unet* h, const float* content_bct, const float* prompt_blc, const uint8_t* mask_bl, void* stream) {
  if (!content_bct || !prompt_blc) return fail("null condition tensor");
  if (ns2vc_unet_set_prompt(h, prompt_blc, mask_bl, stream)) return 1;      // (first: it may rebuild the plan)
  return ns2vc_unet_set_content(h, content_bct, stream);
}

// The condition of the listed items only (a slot loop's admissions): one scatter launch writes what set_content / set_prompt write for
// those items, then the WHOLE condition plan runs again -- every launch of it works item by item, so the other items' hoisted tensors come out
// with the bits they had.  A mask where the plan has none (or none where it has one, NULL = all keys kept) would rebuild the plan: refused.
int ns2vc_unet_set_condition_items(ns2vc_unet* h, int n, const int32_t* slots, const float* content_nct, const float* prompt_nlc, const uint8_t* mask_nl,
                                   void* stream) {
  if (check_ready(h, true)) return 1;
  if (!content_nct || !prompt_nlc) return fail("null condition tensor");
  if (mask_nl && !h->has_mask)
    return fail("the plan was built without a prompt mask: set one for the whole batch first (ns2vc_unet_set_mask) -- a per-item call does not rebuild the plan");
  hipStream_t s = (hipStream_t)stream;
  const auto& c = h->cfg;
  const int* slots_dev = nullptr;
  if (stage_slot_list(h, n, slots, h->B, nullptr, s, &slots_dev, nullptr)) return 1;
  HIPCHK(launch_condition_items(content_nct, c.content_channels, h->T, prompt_nlc, h->Lp, c.cross_attention_dim, mask_nl, n, slots_dev, h->B, h->content_op,
                                h->prec, h->prec != PREC_F32 ? c.content_channels : 0, h->content_f32, h->lens.masked ? h->lens.dev : nullptr, h->prompt,
                                h->has_mask ? h->mask_dev : nullptr, s));
  if (h->has_mask) {
    if (h->plens.on) HIPCHK(launch_prompt_bias(h->mask_dev, h->plens.dev, h->B, h->Lp, h->maskbias, s));
    else HIPCHK(launch_mask_bias(h->mask_dev, h->B * h->Lp, h->maskbias, s));
  }
  return run_ops(h->cond_ops, s);
}

// the plan for the current shape again, dense or masked (h->lens.masked), in the arena it already has: the persistent state (condition, solver
// state, the length tables) sits at the same offsets in both, so nothing but the launch list and the captured step graph changes
static int rebuild_plan(ns2vc_unet* h) {
  drop_step_graph(h);
  return build_plan(h, false);
}

int ns2vc_unet_set_lengths(ns2vc_unet* h, const int32_t* lengths_b, void* stream) {
  if (check_ready(h, true)) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (!lengths_b) {
    if (!h->lens.masked) return 0;
    h->lens.masked = false;
    h->lens.applied.clear();
    return rebuild_plan(h);
  }
  const int nl = h->cfg.n_levels, B = h->B;
  for (int b = 0; b < B; ++b)
    if (lengths_b[b] < 1 || lengths_b[b] > h->T) return fail("lengths[%d] = %d outside [1, T = %d]", b, (int)lengths_b[b], h->T);
  if (h->lens.masked && h->lens.applied.size() == (size_t)B && std::equal(lengths_b, lengths_b + B, h->lens.applied.begin())) return 0;   // (tables already hold them)
  const std::vector<int> Ts = level_lengths(h->T, nl);
  std::vector<int32_t> lens((size_t)nl * B);
  size_t nb = 0;
  for (int l = 0; l < nl; ++l) nb += (size_t)B * Ts[l];
  std::vector<float> bias(nb, 0.f);
  size_t o = 0;
  for (int l = 0; l < nl; ++l) {
    for (int b = 0; b < B; ++b) {
      const int L = l == 0 ? lengths_b[b] : (lens[(size_t)(l - 1) * B + b] + 1) / 2;      // spec.level_lengths: ceil(L / 2) per stride-2 level
      lens[(size_t)l * B + b] = L;
      for (int t = L; t < Ts[l]; ++t) bias[o + (size_t)b * Ts[l] + t] = -10000.f;   // (the cross-attention mask's value: its exp is 0 in fp32)
    }
    o += (size_t)B * Ts[l];
  }
  if (!h->lens.masked) {
    h->lens.masked = true;
    if (rebuild_plan(h)) { h->lens.masked = false; (void)rebuild_plan(h); return 1; }
  }
  const size_t lb = lens.size() * sizeof(int32_t), bb = bias.size() * sizeof(float);
  Staged& stage = h->lens.stage;
  if (stage.reserve(lb + bb)) return 1;
  char* st = static_cast<char*>(stage.buf);
  memcpy(st, lens.data(), lb);
  memcpy(st + lb, bias.data(), bb);
  HIPCHK(hipMemcpyAsync(h->lens.dev, st, lb, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(h->lens.selfbias, st + lb, bb, hipMemcpyHostToDevice, s));
  if (stage.record(s)) return 1;
  h->lens.applied.assign(lengths_b, lengths_b + B);
  return 0;
}

int ns2vc_unet_set_prompt_lengths(ns2vc_unet* h, const int32_t* plens_b, void* stream) {
  if (check_ready(h, true)) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (!plens_b) {
    if (!h->plens.on) return 0;
    h->plens.on = false;
    h->plens.applied.clear();
    if (rebuild_plan(h)) return 1;
    if (h->has_mask) HIPCHK(launch_mask_bias(h->mask_dev, h->B * h->Lp, h->maskbias, s));     // (the row of the mask alone again)
    return 0;
  }
  const int B = h->B;
  for (int b = 0; b < B; ++b)
    if (plens_b[b] < 1 || plens_b[b] > h->Lp) return fail("prompt_lengths[%d] = %d outside [1, Lp = %d]", b, (int)plens_b[b], h->Lp);
  if (h->plens.on && h->plens.applied.size() == (size_t)B && std::equal(plens_b, plens_b + B, h->plens.applied.begin())) return 0;   // (the table already holds them)
  if (!h->plens.on) {
    // the condition plan and the cross-attention launches bake in whether the table is read: rebuild the (cheap) plan, as set_mask does when a
    // bias appears; the arena's layout does not depend on it
    h->plens.on = true;
    if (rebuild_plan(h)) { h->plens.on = false; (void)rebuild_plan(h); return 1; }
  }
  const size_t lb = (size_t)B * sizeof(int32_t);
  Staged& stage = h->plens.stage;
  if (stage.reserve(lb)) return 1;
  memcpy(stage.buf, plens_b, lb);
  HIPCHK(hipMemcpyAsync(h->plens.dev, stage.buf, lb, hipMemcpyHostToDevice, s));
  if (stage.record(s)) return 1;
  HIPCHK(launch_prompt_bias(h->has_mask ? h->mask_dev : nullptr, h->plens.dev, B, h->Lp, h->maskbias, s));
  h->plens.applied.assign(plens_b, plens_b + B);
  return 0;
}

int ns2vc_unet_forward(ns2vc_unet* h, const float* x_bct, const float* t_b, float* out_bct, void* stream) {
  if (check_ready(h, true)) return 1;
  if (!x_bct || !t_b || !out_bct) return fail("null tensor");
  hipStream_t s = (hipStream_t)stream;
  h->use_step_table = false;
  if (load_state(h, x_bct, s)) return 1;
  HIPCHK(hipMemcpyAsync(h->t_dev, t_b, (size_t)h->B * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (run_ops(h->fwd_ops, s)) return 1;
  HIPCHK(launch_btc_to_nct(h->x0, h->CP, h->cfg.latent_channels, h->T, h->B, out_bct, s));
  return 0;
}

// a device counter of the plan's zero-initialised block (null: no plan yet) -> host, optionally cleared
static int read_counter(unsigned* counter, unsigned long long* count, int reset, hipStream_t s) {
  if (!count) return fail("null argument");
  *count = 0;
  if (!counter) return 0;
  unsigned v = 0;
  HIPCHK(hipMemcpyAsync(&v, counter, sizeof(v), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *count = v;
  if (reset) HIPCHK(launch_zero(counter, 16, s));
  return 0;
}
int ns2vc_unet_attn_fallbacks(ns2vc_unet* h, unsigned long long* count, int reset, void* stream) {
  if (!h) return fail("null argument");
  return read_counter(h->attn_fallbacks, count, reset, (hipStream_t)stream);
}
int ns2vc_unet_gn_coop_alone(ns2vc_unet* h, unsigned long long* count, int reset, void* stream) {
  if (!h) return fail("null argument");
  return read_counter(h->ln_health ? h->ln_health + 48 : nullptr, count, reset, (hipStream_t)stream);
}

int ns2vc_unet_graph_captures(ns2vc_unet* h, unsigned long long* count) {
  if (!h || !count) return fail("null argument");
  *count = h->graph_captures;
  return 0;
}

int ns2vc_unet_num_taps(ns2vc_unet* h) { return h ? (int)h->taps.size() : 0; }
int ns2vc_unet_tap_info(ns2vc_unet* h, int idx, char* name, int buflen, int* rows, int* cols) {
  if (!h || idx < 0 || idx >= (int)h->taps.size()) return fail("tap index out of range");
  snprintf(name, buflen, "%s", h->taps[idx].name.c_str());
  *rows = h->taps[idx].rows; *cols = h->taps[idx].cols;
  return 0;
}
int ns2vc_unet_tap_read(ns2vc_unet* h, int idx, float* host_dst) {
  if (!h || idx < 0 || idx >= (int)h->taps.size()) return fail("tap index out of range");
  HIPCHK(hipDeviceSynchronize());
  const Tap& t = h->taps[idx];
  HIPCHK(hipMemcpy(host_dst, t.copy, (size_t)t.rows * t.cols * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}
int ns2vc_unet_num_launches(ns2vc_unet* h, int* per_forward, int* per_condition) {
  if (!h) return fail("null engine handle");
  if (per_forward) *per_forward = (int)h->fwd_ops.size();
  if (per_condition) *per_condition = (int)h->cond_ops.size();
  return 0;
}

int ns2vc_unet_op_info(ns2vc_unet* h, int which, int idx, char* name, int buflen, int* kind, double* flops, double* bytes) {
  if (!h) return fail("null engine handle");
  if (which == 2) {      // the record of the timestep-embedding branch (fork_temb): field `idx` -> its name and, in *kind, its value
    static const char* const field[6] = {"begin", "end", "join", "first_reader", "readers", "forks"};
    if (!h->arena) return fail("engine not prepared (call ns2vc_unet_prepare)");
    if (idx < 0 || idx >= 6) return fail("op index out of range");
    GemmArgs g;
    const int v[6] = {h->tfork.begin, h->tfork.end, h->tfork.join, h->tfork.first, h->tfork.readers,
                      temb_forks(h, solver_in_conv_out(h, g) ? (size_t)h->conv_out_idx : h->fwd_ops.size()) ? 1 : 0};
    snprintf(name, buflen, "%s", field[idx]);
    *kind = v[idx]; *flops = 0.0; *bytes = 0.0;
    return 0;
  }
  const std::vector<Op>& ops = which ? h->cond_ops : h->fwd_ops;
  if (idx < 0 || idx >= (int)ops.size()) return fail("op index out of range");
  snprintf(name, buflen, "%s", ops[idx].name.c_str());
  *kind = ops[idx].kind; *flops = ops[idx].flops; *bytes = ops[idx].bytes;
  return 0;
}

// Times every launch of the per-step forward plan on `stream`: each op is launched `reps` times back to back
// between one hipEvent pair (so the event/launch overhead is amortised and the figure approaches the kernel's
// own duration, comparable with rocprofv3's kernel trace).  ms[i] = average milliseconds of launch i.
// The tensors hold garbage afterwards (in-place ops were repeated).  Synchronous.
int ns2vc_unet_profile_forward(ns2vc_unet* h, float* ms, int n_ms, int reps, void* stream) {
  if (check_ready(h, true)) return 1;
  const size_t n = h->fwd_ops.size();
  if ((size_t)n_ms < n) return fail("ms buffer too small: need %zu", n);
  if (reps < 1) reps = 1;
  hipStream_t s = (hipStream_t)stream;
  h->use_step_table = false;      // time with the (B,) timestep buffer of the plain forward
  std::vector<hipEvent_t> ev(2 * n);
  for (auto& e : ev) HIPCHK(hipEventCreate(&e));
  int rc = 0;
  // An op with a cooperative GroupNorm prologue starts from zeroed arrival words (the forward's clear launch): repeated here, it gets
  // its own small clear in front of every repetition, and the time of `reps` such clears alone (measured once, below) is taken off.
  hipEvent_t rz0 = nullptr, rz1 = nullptr;
  const Op* rz_op = nullptr;
  for (size_t i = 0; i < n && !rc; ++i) {
    const Op& op = h->fwd_ops[i];
    if (op.rearm && !rz_op) rz_op = &op;
    if (hipEventRecord(ev[2 * i], s) != hipSuccess) rc = fail("hipEventRecord failed");
    for (int r = 0; r < reps && !rc; ++r) {
      hipError_t e = op.rearm ? op.rearm(s) : hipSuccess;
      if (e == hipSuccess) e = op.fn(s);
      if (e != hipSuccess) rc = fail("launch of '%s' failed: %s", op.name.c_str(), hipGetErrorString(e));
    }
    if (!rc && hipEventRecord(ev[2 * i + 1], s) != hipSuccess) rc = fail("hipEventRecord failed");
  }
  if (!rc && rz_op) {
    if (hipEventCreate(&rz0) != hipSuccess || hipEventCreate(&rz1) != hipSuccess) rc = fail("hipEventCreate failed");
    if (!rc) (void)hipEventRecord(rz0, s);
    for (int r = 0; r < reps && !rc; ++r)
      if (rz_op->rearm(s) != hipSuccess) rc = fail("clear launch failed");
    if (!rc) (void)hipEventRecord(rz1, s);
  }
  if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = fail("stream sync failed: %s", hipGetErrorString(hipGetLastError()));
  float rz_ms = 0.f;
  if (!rc && rz_op && hipEventElapsedTime(&rz_ms, rz0, rz1) != hipSuccess) rc = fail("hipEventElapsedTime failed");
  for (size_t i = 0; i < n && !rc; ++i) {
    if (hipEventElapsedTime(&ms[i], ev[2 * i], ev[2 * i + 1]) != hipSuccess) rc = fail("hipEventElapsedTime failed");
    if (h->fwd_ops[i].rearm) ms[i] = std::max(ms[i] - rz_ms, 0.f);
    ms[i] /= (float)reps;
  }
  if (rz0) (void)hipEventDestroy(rz0);
  if (rz1) (void)hipEventDestroy(rz1);
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

}  // extern "C"
