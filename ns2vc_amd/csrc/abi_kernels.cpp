// The part of the C ABI that takes no engine handle: device, stream, event and memcpy helpers, the ns2vc_pack_* weight packers, the
// single-kernel launchers ns2vc_k_*, the ns2vc_debug_* hooks and the operand conversions (kernel tests and tools/ drive the kernels through these).
#include "engine_internal.h"
#include "kernel_table.h"

#include <algorithm>
#include <cstring>
#include <mutex>

using namespace ns2vc;

hipError_t ns2vc::init_all_attributes() {
  hipError_t e = init_gemm_attributes();
  if (e == hipSuccess) e = init_convts_attributes();
  if (e == hipSuccess) e = init_attn_attributes();
  if (e == hipSuccess) e = init_attnres_attributes();
  if (e == hipSuccess) e = init_ffn_attributes();
  if (e == hipSuccess) e = init_geglu_attributes();
  if (e == hipSuccess) e = init_rowchain_attributes();
  return e;
}
// the attribute setup of one kernel family in front of its packer; `once`: skipped after the first success
static int init_attributes(hipError_t (*init)(), bool* once = nullptr) {
  if (once && *once) return 0;
  const hipError_t e = init();
  if (e != hipSuccess) return fail("kernel attribute setup failed: %s", hipGetErrorString(e));
  if (once) *once = true;
  return 0;
}
// a packed host image -> a device allocation of its own, handed to the caller (who frees it with ns2vc_dev_free)
static int upload(const void* src, size_t bytes, void** out_dev) {
  void* d = nullptr;
  HIPCHK(hipMalloc(&d, std::max<size_t>(bytes, 1)));
  HIPCHK(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice));
  *out_dev = d;
  return 0;
}
// the status of a kernel launch as the ABI reports it
static int launched(hipError_t e, const char* what) { return e == hipSuccess ? 0 : fail("%s: %s", what, hipGetErrorString(e)); }
static int upload_u16(const std::vector<unsigned short>& v, void** out_dev) { return upload(v.data(), v.size() * 2, out_dev); }

// per device (the process may serve several): the result of misc.hip's placement probe, taken at the first engine of a device
int ns2vc::xcd_round_robin_of_current_device() {
  static std::mutex mu;
  static std::map<int, int> seen;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  std::lock_guard<std::mutex> lock(mu);
  auto it = seen.find(dev);
  if (it != seen.end()) return it->second;
  const int r = probe_xcd_round_robin();
  seen[dev] = r;
  return r;
}

extern "C" {

int ns2vc_abi_version(void) { return NS2VC_ABI_VERSION; }
int ns2vc_sizeof_gemm_args(void) { return (int)sizeof(ns2vc_gemm_args); }
int ns2vc_sizeof_attn_args(void) { return (int)sizeof(ns2vc_attn_args); }
int ns2vc_sizeof_rowchain_args(void) { return (int)sizeof(ns2vc_rowchain_args); }
int ns2vc_sizeof_ffn_args(void) { return (int)sizeof(ns2vc_ffn_args); }
int ns2vc_sizeof_geglu_args(void) { return (int)sizeof(ns2vc_geglu_args); }
const char* ns2vc_last_error(void) { return g_err.c_str(); }

int ns2vc_device_count(int* out_count) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *out_count = 0; return fail("hipGetDeviceCount: %s", hipGetErrorString(e)); }
  *out_count = n;
  return 0;
}
int ns2vc_set_device(int device) { HIPCHK(hipSetDevice(device)); return 0; }
int ns2vc_device_name(char* buf, int buflen) {
  hipDeviceProp_t p;
  int dev = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipGetDeviceProperties(&p, dev));
  snprintf(buf, buflen, "%s|%s|CUs=%d|clock_khz=%d|mem_gb=%.1f", p.name, p.gcnArchName, p.multiProcessorCount, p.clockRate,
           (double)p.totalGlobalMem / 1e9);
  return 0;
}

int ns2vc_device_xcd_round_robin(int* out) {
  if (!out) return fail("null argument");
  *out = xcd_round_robin_of_current_device();
  return 0;
}

// ---- raw helpers ----------------------------------------------------------------------
int ns2vc_dev_malloc(void** out, size_t bytes) { HIPCHK(hipMalloc(out, bytes ? bytes : 1)); return 0; }
int ns2vc_dev_free(void* p) { HIPCHK(hipFree(p)); return 0; }
int ns2vc_memcpy_h2d(void* dst, const void* src, size_t bytes) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice)); return 0; }
int ns2vc_memcpy_d2h(void* dst, const void* src, size_t bytes) { HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost)); return 0; }
int ns2vc_dev_sync(void) { HIPCHK(hipDeviceSynchronize()); return 0; }
int ns2vc_stream_create(void** out) { hipStream_t s; HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)); *out = s; return 0; }
// NOTE: hipExtStreamCreateWithCUMask makes a DEFAULT (blocking) stream: it synchronises implicitly with the legacy null stream, so work
// queued on the null stream serialises with it (keep PyTorch work on explicit streams when overlapping stages).  The mask is validated against the
// device: at least one bit set, and no bit at or beyond the CU count.
int ns2vc_stream_create_cu_mask(void** out, const uint32_t* mask_words, int n_words) {
  if (!out || !mask_words || n_words <= 0) return fail("null argument");
  int dev = 0, cus = 0;
  HIPCHK(hipGetDevice(&dev));
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  if (n_words > (cus + 31) / 32) return fail("CU mask of %d words for a device with %d CUs (at most %d words)", n_words, cus, (cus + 31) / 32);
  bool any = false;
  for (int w = 0; w < n_words; ++w)
    for (int b = 0; b < 32; ++b)
      if (mask_words[w] >> b & 1u) {
        if (w * 32 + b >= cus) return fail("CU mask bit %d set, the device has %d CUs", w * 32 + b, cus);
        any = true;
      }
  if (!any) return fail("empty CU mask");
  hipStream_t s;
  HIPCHK(hipExtStreamCreateWithCUMask(&s, (uint32_t)n_words, mask_words));
  *out = s;
  return 0;
}
int ns2vc_stream_destroy(void* s) { HIPCHK(hipStreamDestroy((hipStream_t)s)); return 0; }
int ns2vc_stream_sync(void* s) { HIPCHK(hipStreamSynchronize((hipStream_t)s)); return 0; }
int ns2vc_event_create(void** out) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); *out = e; return 0; }
int ns2vc_event_destroy(void* e) { HIPCHK(hipEventDestroy((hipEvent_t)e)); return 0; }
int ns2vc_event_record(void* e, void* s) { HIPCHK(hipEventRecord((hipEvent_t)e, (hipStream_t)s)); return 0; }
int ns2vc_event_elapsed_ms(void* a, void* b, float* ms) {
  HIPCHK(hipEventSynchronize((hipEvent_t)b));
  HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)a, (hipEvent_t)b));
  return 0;
}

// ---- kernel-level entry points -----------------------------------------------------------
int ns2vc_pack_weight(const float* rows_host, int N, int K, int precision, void** out_dev) {
  if (!rows_host || !out_dev || N <= 0 || K <= 0) return fail("bad argument");
  static bool inited = false;
  if (init_attributes(init_all_attributes, &inited)) return 1;
  return ns2vc_to_operand(rows_host, (size_t)N * K, precision, out_dev);
}
int ns2vc_pack_conv3_tiled(const float* rows_host, int N, int ctot, int c2, int precision, void** out_dev) {
  if (!rows_host || !out_dev || N <= 0) return fail("bad argument");
  std::vector<unsigned char> img;
  if (pack_conv3_tiled(rows_host, N, ctot, c2, precision, img) != hipSuccess) return fail("pack_conv3_tiled: ctot / c2 must be multiples of the chunk (64 elements; 32 for fp32)");
  return upload(img.data(), img.size(), out_dev);
}
int ns2vc_weight_rowsum(const float* rows_host, int N, int K, int precision, float** out_dev) {
  if (!rows_host || !out_dev || N <= 0 || K <= 0) return fail("bad argument");
  const std::vector<float> ws = rounded_rowsum(rows_host, N, K, N, precision);
  return upload(ws.data(), ws.size() * sizeof(float), (void**)out_dev);
}
int ns2vc_debug_set_attn_optimistic(int on) {
  set_attn_optimistic(on);
  return 0;
}
int ns2vc_debug_set_gemm_trace(void* dev_u64_blocks_x8) {
  set_gemm_trace((unsigned long long*)dev_u64_blocks_x8);
  set_ffn_trace((unsigned long long*)dev_u64_blocks_x8);
  set_rc_trace((unsigned long long*)dev_u64_blocks_x8);
  set_ts_trace((unsigned long long*)dev_u64_blocks_x8);     // (convts.hip and geglu.hip write 16 words per block)
  set_gg_trace((unsigned long long*)dev_u64_blocks_x8);
  return 0;
}
int ns2vc_debug_poison(unsigned pattern, int lds_bytes, void* stream) {
  static unsigned* sink = nullptr;
  if (lds_bytes < 4 || lds_bytes > 160 * 1024) return fail("poison: LDS bytes out of range");
  if (!sink) HIPCHK(hipMalloc((void**)&sink, 64));
  return launched(launch_poison(pattern, lds_bytes & ~3, sink, (hipStream_t)stream), "launch_poison");
}
int ns2vc_debug_placement(void* stream, int n_blocks, int spin, uint32_t* out_host) {
  if (!out_host || n_blocks <= 0 || n_blocks > (1 << 20)) return fail("bad argument");
  unsigned* d = nullptr;
  HIPCHK(hipMalloc((void**)&d, (size_t)n_blocks * 2 * sizeof(unsigned)));
  hipError_t e = launch_placement(d, n_blocks, spin, (hipStream_t)stream);
  if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
  if (e == hipSuccess) e = hipMemcpy(out_host, d, (size_t)n_blocks * 2 * sizeof(unsigned), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  if (e != hipSuccess) return fail("placement probe: %s", hipGetErrorString(e));
  return 0;
}
int ns2vc_debug_set_gemm_tile(int bm, int bn, int stages) { set_forced_gemm_tile(bm, bn, stages); return 0; }
int ns2vc_debug_kernel_table(int family, int* rows, int* unready) {
  static const struct { const KernelTable& (*table)(); hipError_t (*init)(); } fam[] = {
      {gemm2_kernel_table, init_gemm_attributes}, {gemm4_kernel_table, init_gemm_attributes}, {conv3ts_kernel_table, init_convts_attributes},
      {attn_kernel_table, init_attn_attributes},  {ffn_kernel_table, init_ffn_attributes},    {geglu_kernel_table, init_geglu_attributes},
      {rowchain_kernel_table, init_rowchain_attributes}};
  constexpr int NF = (int)(sizeof(fam) / sizeof(fam[0]));
  if (family < 0 || family >= NF || !rows) return fail("kernel table: family 0 .. %d, rows not NULL", NF - 1);
  const KernelTable& t = fam[family].table();
  *rows = t.n;
  if (!unready) return 0;
  if (init_attributes(fam[family].init)) return 1;
  *unready = 0;
  for (int i = 0; i < t.n; ++i) {
    hipFuncAttributes fa;
    HIPCHK(hipFuncGetAttributes(&fa, t.rows[i].fn));
    if (fa.maxDynamicSharedSizeBytes < (int)t.rows[i].lds || t.rows[i].lds > 160 * 1024) ++*unready;
  }
  return 0;
}
int ns2vc_k_gemm(const ns2vc_gemm_args* a, int precision, void* stream) {
  if (!a) return fail("null args");
  hipError_t e = launch_gemm(*a, precision, (hipStream_t)stream);
  if (e != hipSuccess) {
    const int line = last_gemm_refusal_line();
    if (line) return fail("launch_gemm: %s (refused by the argument check at gemm.hip:%d)", hipGetErrorString(e), line);
    return fail("launch_gemm: %s", hipGetErrorString(e));
  }
  return 0;
}
int ns2vc_pack_ffn(const float* w1_packed_host, const float* w2f_host, int dim, int precision, void** out_stream_dev) {
  if (!w1_packed_host || !w2f_host || !out_stream_dev) return fail("null argument");
  static bool inited = false;
  if (init_attributes(init_ffn_attributes, &inited)) return 1;
  std::vector<unsigned short> st;
  if (pack_ffn_stream(w1_packed_host, w2f_host, nullptr, dim, precision, st) != hipSuccess) return fail("ffn: dim must be 128 or 256 and the precision 16-bit");
  return upload_u16(st, out_stream_dev);
}
int ns2vc_pack_ffn_pre(const float* w1_packed_host, const float* w2f_host, const float* w0_host, int dim, int precision, void** out_stream_dev) {
  if (!w1_packed_host || !w2f_host || !w0_host || !out_stream_dev) return fail("null argument");
  if (init_attributes(init_ffn_attributes)) return 1;
  std::vector<unsigned short> st;
  if (pack_ffn_stream(w1_packed_host, w2f_host, w0_host, dim, precision, st) != hipSuccess) return fail("ffn: dim must be 128 or 256 and the precision 16-bit");
  return upload_u16(st, out_stream_dev);
}
int ns2vc_pack_rowchain(const float* w1_host, const float* w2_host, int dim, int n2, int precision, void** out_stream_dev) {
  if (!w1_host || !w2_host || !out_stream_dev) return fail("null argument");
  static bool inited = false;
  if (init_attributes(init_rowchain_attributes, &inited)) return 1;
  std::vector<unsigned short> st;
  if (pack_rowchain_stream(w1_host, w2_host, dim, n2, precision, st) != hipSuccess)
    return fail("rowchain: dim must be 128, 256 or 384, n2 = dim or 3 dim, and the precision 16-bit");
  return upload_u16(st, out_stream_dev);
}
int ns2vc_pack_rowchain_sliced(const float* w1_host, const float* w2_host, int dim, int n2, int slices, int precision, void** out_stream_dev) {
  if (!w1_host || !w2_host || !out_stream_dev) return fail("null argument");
  static bool inited = false;
  if (init_attributes(init_rowchain_attributes, &inited)) return 1;
  std::vector<unsigned short> st;
  if (pack_rowchain_stream(w1_host, w2_host, dim, n2, precision, st, slices) != hipSuccess)
    return fail("rowchain (sliced): dim 384, n2 = dim or 3 dim, 2 slices, 16-bit precision");
  return upload_u16(st, out_stream_dev);
}
int ns2vc_debug_set_attn_keys(int keys) {
  if (keys != 0 && keys != 64 && keys != 128) return fail("attention K/V tile: 0 (heuristic), 64 or 128 keys");
  set_forced_attn_keys(keys);
  return 0;
}
int ns2vc_debug_set_attn_resident(int mode) {
  if (mode < -1 || mode > 1) return fail("resident attention: -1 (the rule), 0 (never) or 1 (whenever the launch fits)");
  set_attn_resident_mode(mode);
  return 0;
}
unsigned long long ns2vc_debug_attn_resident_launches(void) { return attn_resident_launches(); }
int ns2vc_debug_attnres_table(int* rows) {
  if (!rows) return fail("attnres table: rows not NULL");
  *rows = attnres_kernel_table().n;
  return 0;
}
int ns2vc_debug_set_attn_resident_lens(int mode) {
  if (mode < -1 || mode > 1) return fail("resident attention under lengths: -1 (the rule), 0 (never) or 1 (whenever the launch fits)");
  set_attn_resident_lens_mode(mode);
  return 0;
}
unsigned long long ns2vc_debug_attn_resident_lens_launches(void) { return attn_resident_lens_launches(); }
int ns2vc_debug_attnres_lens_table(int* rows) {
  if (!rows) return fail("attnres lens table: rows not NULL");
  *rows = attnres_lens_kernel_table().n;
  return 0;
}
int ns2vc_debug_set_rowchain_tokens(int nt) {
  if (nt < 0 || nt > 2) return fail("rowchain tokens: 0 (heuristic), 1 (64-token blocks) or 2 (128-token blocks)");
  set_forced_rowchain_tokens(nt);
  return 0;
}
int ns2vc_k_rowchain(const ns2vc_rowchain_args* a, int precision, void* stream) {
  if (!a) return fail("null args");
  return launched(launch_rowchain(*a, precision, (hipStream_t)stream), "launch_rowchain");
}
size_t ns2vc_xattn_pack_bytes(int B, int Lk, int hd) { return xattn_pack_bytes(B, Lk, hd); }
int ns2vc_k_xattn_pack(const void* k, int ldk, const void* v, int ldv, int B, int Lk, int hd, void* out, int precision, void* stream) {
  hipError_t e = launch_xattn_pack(k, ldk, v, ldv, B, Lk, hd, out, precision, (hipStream_t)stream);
  if (e != hipSuccess) return fail("xattn_pack: %s (16-bit precisions, head dim 16 | 32, 8 heads, 16-byte aligned k rows)", hipGetErrorString(e));
  return 0;
}
int ns2vc_k_ffn(const ns2vc_ffn_args* a, int precision, void* stream) {
  if (!a) return fail("null args");
  return launched(launch_ffn(*a, precision, (hipStream_t)stream), "launch_ffn");
}
int ns2vc_pack_geglu(const float* w1_packed_host, const float* bias1_packed_host, int dim, int precision, void** out_stream_dev, float** out_consts_dev) {
  if (!w1_packed_host || !out_stream_dev || !out_consts_dev) return fail("null argument");
  if (init_attributes(init_geglu_attributes)) return 1;
  std::vector<unsigned short> st;
  std::vector<float> cs;
  if (pack_geglu_stream(w1_packed_host, bias1_packed_host, dim, precision, st, cs) != hipSuccess) return fail("geglu: dim must be 384 and the precision 16-bit");
  if (upload_u16(st, out_stream_dev)) return 1;
  return upload(cs.data(), cs.size() * 4, (void**)out_consts_dev);
}
int ns2vc_debug_set_geglu_min_rows(int rows) { g_geglu_min_rows = rows < 0 ? 4608 : rows; return 0; }
int ns2vc_pack_geglu_host(const float* w1_packed_host, const float* bias1_packed_host, int dim, int precision, uint16_t* stream_out, float* consts_out) {
  if (!w1_packed_host || !stream_out || !consts_out) return fail("null argument");
  std::vector<unsigned short> st;
  std::vector<float> cs;
  if (pack_geglu_stream(w1_packed_host, bias1_packed_host, dim, precision, st, cs) != hipSuccess) return fail("geglu: dim must be 384 and the precision 16-bit");
  memcpy(stream_out, st.data(), st.size() * 2);
  memcpy(consts_out, cs.data(), cs.size() * 4);
  return 0;
}
int ns2vc_k_geglu(const ns2vc_geglu_args* a, int precision, void* stream) {
  if (!a) return fail("null args");
  return launched(launch_geglu(*a, precision, (hipStream_t)stream), "launch_geglu");
}
int ns2vc_k_attention(const ns2vc_attn_args* a, int head_dim, int precision, void* stream) {
  if (!a) return fail("null args");
  // per-item counts: this entry (tests, tools) reads the tables back and refuses a count outside its range; the engine's tables are checked on the
  // host by ns2vc_unet_set_lengths, and the kernel clamps what it reads either way
  if (a->q_lens || a->k_lens) {
    if (a->B <= 0) return fail("attention: B=%d", a->B);
    std::vector<int32_t> host((size_t)a->B);
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    const struct { const int32_t* dev; int max; const char* name; } tabs[2] = {{a->q_lens, a->Lq, "q_lens"}, {a->k_lens, a->Lk, "k_lens"}};
    for (const auto& t : tabs) {
      if (!t.dev) continue;
      HIPCHK(hipMemcpy(host.data(), t.dev, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      for (int b = 0; b < a->B; ++b)
        if (host[b] < 1 || host[b] > t.max) return fail("attention: %s[%d]=%d outside 1..%d", t.name, b, host[b], t.max);
    }
  }
  return launched(launch_attention(*a, head_dim, precision, (hipStream_t)stream, true, true), "launch_attention");      // (the hooks decide)
}
int ns2vc_k_groupnorm(const float* a0, int lda0, int c0, const float* a1, int lda1, int c1, int B, int T, int G, float eps,
                      const float* gamma, const float* beta, const float* temb, int ldtemb, int temb_off, int silu, void* out_op,
                      void* raw_op, int precision, void* stream) {
  const int rows = 32, nchunk = (T + rows - 1) / rows;
  double* part = nullptr;
  HIPCHK(hipMalloc((void**)&part, (size_t)B * nchunk * G * 2 * sizeof(double)));
  hipError_t e = launch_gn_partial(a0, lda0, c0, a1, lda1, c1, B, T, G, part, nchunk, rows, (hipStream_t)stream);
  if (e == hipSuccess)
    e = launch_gn_apply(a0, lda0, c0, a1, lda1, c1, B, T, G, eps, part, nchunk, nullptr, nullptr, gamma, beta, temb, ldtemb, temb_off, silu,
                        out_op, raw_op, precision, (hipStream_t)stream);
  hipError_t e2 = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(part);
  if (e != hipSuccess) return fail("groupnorm launch: %s", hipGetErrorString(e));
  if (e2 != hipSuccess) return fail("groupnorm sync: %s", hipGetErrorString(e2));
  return 0;
}
int ns2vc_k_groupnorm_stats(const float* a0, int lda0, int c0, const long long* stats0, int B, int T, int G, float eps, const float* gamma,
                            const float* beta, const float* temb, int ldtemb, int temb_off, int silu, void* out_op, int precision, void* stream) {
  if (!stats0 || (c0 % G) || ((c0 / G) & 15)) return fail("groupnorm_stats: needs the int64 epilogue statistics and groups of whole 16-channel blocks");
  return launched(launch_gn_apply(a0, lda0, c0, nullptr, 0, 0, B, T, G, eps, nullptr, 0, stats0, nullptr, gamma, beta, temb, ldtemb, temb_off, silu,
                                 out_op, nullptr, precision, (hipStream_t)stream), "groupnorm_stats launch");
}
int ns2vc_k_groupnorm_stats2(const float* a0, int lda0, int c0, const long long* stats0, const float* a1, int lda1, int c1, const long long* stats1,
                             int B, int T, int G, float eps, const float* gamma, const float* beta, const float* temb, int ldtemb, int temb_off,
                             int silu, void* out_op, void* raw_op, int precision, void* stream) {
  if (!stats0 || !a1 || !stats1 || (c0 & 15) || (c1 & 15) || ((c0 + c1) % G) || (((c0 + c1) / G) & 15))
    return fail("groupnorm_stats2: needs both sources' int64 epilogue statistics, whole 16-channel blocks per source and per group");
  return launched(launch_gn_apply(a0, lda0, c0, a1, lda1, c1, B, T, G, eps, nullptr, 0, stats0, stats1, gamma, beta, temb, ldtemb, temb_off, silu,
                                 out_op, raw_op, precision, (hipStream_t)stream), "groupnorm_stats2 launch");
}
int ns2vc_k_layernorm_apply(const float* x, int ldx, int M, int C, float eps, void* out_op, int precision, void* stream) {
  return launched(launch_ln_apply_op(x, ldx, M, C, eps, out_op, precision, (hipStream_t)stream), "ln_apply launch");
}
int ns2vc_to_operand(const float* host, size_t n, int precision, void** out_dev) {
  if (!host || !out_dev) return fail("null argument");
  if (precision == NS2VC_PREC_F32) return upload(host, n * 4, out_dev);
  std::vector<uint16_t> q(n);
  for (size_t i = 0; i < n; ++i) q[i] = f32_to_op16_bits(host[i], precision);
  return upload(q.data(), n * 2, out_dev);
}
int ns2vc_round_to_operand(const float* host_in, size_t n, int precision, float* host_out) {
  if (!host_in || !host_out) return fail("null argument");
  if (precision != NS2VC_PREC_F32 && precision != NS2VC_PREC_BF16 && precision != NS2VC_PREC_F16) return fail("unknown precision %d", precision);
  for (size_t i = 0; i < n; ++i)
    host_out[i] = precision == NS2VC_PREC_F32 ? host_in[i] : op16_bits_to_f32(f32_to_op16_bits(host_in[i], precision), precision);
  return 0;
}
int ns2vc_from_operand(const void* dev, size_t n, int precision, float* host) {
  if (!dev || !host) return fail("null argument");
  HIPCHK(hipDeviceSynchronize());
  if (precision != NS2VC_PREC_F32) {
    std::vector<uint16_t> q(n);
    HIPCHK(hipMemcpy(q.data(), dev, n * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; ++i) host[i] = op16_bits_to_f32(q[i], precision);
  } else {
    HIPCHK(hipMemcpy(host, dev, n * 4, hipMemcpyDeviceToHost));
  }
  return 0;
}
int ns2vc_k_nct_to_btc(const float* src, int C, int T, int B, float* dst, int ldd, int cpad, void* stream) {
  return launched(launch_nct_to_btc(src, C, T, B, dst, nullptr, PREC_F32, ldd, cpad, (hipStream_t)stream), "nct_to_btc launch");
}
int ns2vc_k_btc_to_nct(const float* src, int lds, int C, int T, int B, float* dst, void* stream) {
  return launched(launch_btc_to_nct(src, lds, C, T, B, dst, (hipStream_t)stream), "btc_to_nct launch");
}
// The solver hooks: check the pointers, state the step (common.h SolverStep), launch.  hook_step fills what they all give
static SolverStep hook_step(const float* coef_dev, const int32_t* step_dev, const float* x0, float* xe, void* xe_op, int precision, float* xbar, float* d1,
                            float* mprev, float* mprev2, size_t n, int ld) {
  SolverStep st;
  st.coef = coef_dev; st.step_ptr = step_dev; st.ncoef = NS2VC_NCOEF;
  st.x0 = x0; st.xe = xe; st.xe_op = xe_op; st.prec = precision; st.xbar = xbar; st.d1 = d1; st.mprev = mprev; st.mprev2 = mprev2;
  st.n = n; st.ld = ld; st.split = precision != PREC_F32 ? ld : 0;
  return st;
}
int ns2vc_k_solver_update(const float* coef_dev, const int32_t* step_dev, const float* x0, float* xe, void* xe_op, int precision, float* xbar,
                          float* d1, float* mprev, float* mprev2, size_t n, int ld, void* stream) {
  if (!coef_dev || !step_dev || !x0 || !xe || !xe_op || !xbar || !d1 || !mprev) return fail("null argument");
  if (ld <= 0 || (ld & 3) || n % (size_t)ld) return fail("n (%zu) must be a multiple of ld (%d), ld a multiple of 4", n, ld);
  return launched(launch_solver_step(hook_step(coef_dev, step_dev, x0, xe, xe_op, precision, xbar, d1, mprev, mprev2, n, ld), (hipStream_t)stream),
                  "solver_update launch");
}
int ns2vc_k_solver_step_flat(const float* coef_dev, int n_rows, int row, int kind, const float* model_out, float* xe, float* xbar, float* d1,
                             float* mprev, float* mprev2, float* m_out, size_t n, void* stream) {
  if (!coef_dev || !model_out || !xe || !xbar || !d1 || !mprev) return fail("null argument");
  if (n == 0) return fail("flat solver step: n must be at least 1");
  if (kind < 0 || kind > 4) return fail("flat solver step: kind %d must be 0 (x_start), 1 (noise), 2 (v), 3 (score) or 4 (data)", kind);
  if (n_rows <= 0 || row < 0 || row >= n_rows) return fail("flat solver step: row %d outside the table of %d rows", row, n_rows);
  const uintptr_t bits = (uintptr_t)coef_dev | (uintptr_t)model_out | (uintptr_t)xe | (uintptr_t)xbar | (uintptr_t)d1 | (uintptr_t)mprev |
                         (uintptr_t)mprev2 | (uintptr_t)m_out;
  if (bits & 3) return fail("flat solver step: every pointer must be 4-byte aligned");
  return launched(launch_solver_step_flat(coef_dev + (size_t)row * NS2VC_NCOEF, kind, model_out, xe, xbar, d1, mprev, mprev2, m_out, n,
                                          (hipStream_t)stream),
                  "solver_step_flat launch");
}
int ns2vc_k_solver_update_guided(const float* coef_dev, const int32_t* step_dev, const float* x0, float* xe, void* xe_op, int precision, float* xbar,
                                 float* d1, float* mprev, float* mprev2, size_t n_half, int ld, const float* scale_dev, int T, const uint64_t* seeds_dev,
                                 const int32_t* lens_dev, int nc, void* stream) {
  if (!coef_dev || !step_dev || !x0 || !xe || !xe_op || !xbar || !d1 || !mprev || !scale_dev) return fail("null argument");
  if (ld <= 0) return fail("ld (%d) must be positive", ld);
  SolverStep st = hook_step(coef_dev, step_dev, x0, xe, xe_op, precision, xbar, d1, mprev, mprev2, n_half, ld);
  st.T = T; st.nc = nc; st.lens = lens_dev; st.scale = scale_dev; st.seeds = reinterpret_cast<const unsigned long long*>(seeds_dev);
  return launched(launch_solver_step(st, (hipStream_t)stream), "guided solver_update launch");
}
int ns2vc_k_abs_quantile(const float* values, int n_items, int T, int ld, int nc, const int32_t* lens_dev, float p, float* thr, void* stream) {
  if (!values || !thr) return fail("null argument");
  QuantArgs q;
  q.v = values; q.lens = lens_dev; q.T = T; q.ld = ld; q.nc = nc; q.p = p;
  return launched(launch_abs_quantile(q, n_items, thr, (hipStream_t)stream), "abs_quantile launch");
}
int ns2vc_k_solver_update_corrected(const float* coef_dev, const int32_t* step_dev, const float* x0, float* xe, void* xe_op, int precision, float* xbar,
                                    float* d1, float* mprev, float* mprev2, size_t n, int ld, int T, const float* scale_dev, const int32_t* lens_dev,
                                    int nc, int mode, float ratio, float max_val, float* thr_dev, void* stream) {
  if (!coef_dev || !step_dev || !x0 || !xe || !xe_op || !xbar || !d1 || !mprev) return fail("null argument");
  if (mode != 1 && mode != 2) return fail("corrected update: mode %d must be 1 (dynamic thresholding) or 2 (clamp)", mode);
  if (mode == 1 && !thr_dev) return fail("dynamic thresholding needs thr_dev");
  if (ld <= 0 || (ld & 3) || T <= 0 || n == 0 || n % ((size_t)T * ld)) return fail("n (%zu) must hold whole items of T (%d) rows of ld (%d) columns, ld a multiple of 4", n, T, ld);
  if (!(ratio >= 0.f && ratio <= 1.f) || !(max_val > 0.f)) return fail("ratio %g must be in [0, 1] and max_val %g > 0", (double)ratio, (double)max_val);
  SolverStep st = hook_step(coef_dev, step_dev, x0, xe, xe_op, precision, xbar, d1, mprev, mprev2, n, ld);
  st.T = T; st.nc = nc; st.lens = lens_dev; st.scale = scale_dev; st.mode = mode; st.ratio = ratio; st.max_val = max_val; st.thr = thr_dev;
  return launched(launch_solver_step(st, (hipStream_t)stream), "corrected solver_update launch");
}
// The two hooks with records: the n_items SolverItem records (and, with `cr`, as many ItemCorrect records behind them) go to the device for the
// one call, the step runs on them, and the call returns when it is done
static int run_items_step(SolverStep st, const int32_t* items_host, int n_items, const ItemCorrect* cr, hipStream_t s) {
  static_assert(sizeof(SolverItem) == 4 * sizeof(int32_t) && sizeof(ItemCorrect) == sizeof(SolverItem), "records are four 32-bit words");
  const size_t rb = (size_t)n_items * sizeof(SolverItem);
  char* dev = nullptr;
  HIPCHK(hipMalloc((void**)&dev, cr ? 2 * rb : rb));
  int rc;
  if (hipMemcpy(dev, items_host, rb, hipMemcpyHostToDevice) != hipSuccess || (cr && hipMemcpy(dev + rb, cr, rb, hipMemcpyHostToDevice) != hipSuccess)) {
    rc = fail("items solver_update: copy of the records failed");
  } else {
    st.items = reinterpret_cast<const SolverItem*>(dev); st.n_items = n_items;
    if (cr) st.item_correct = reinterpret_cast<const ItemCorrect*>(dev + rb);
    rc = launched(launch_solver_step(st, s), "items solver_update launch");
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail("items solver_update: stream synchronize failed");
  }
  (void)hipFree(dev);
  return rc;
}
int ns2vc_k_solver_update_items(const float* coef_dev, int n_rows, const int32_t* step_dev, const int32_t* items_host, int n_items, const float* x0, float* xe,
                                void* xe_op, int precision, float* xbar, float* d1, float* mprev, float* mprev2, size_t n, int ld, int T,
                                const float* scale_dev, const uint64_t* seeds_dev, const int32_t* lens_dev, int nc, int mode, float ratio, float max_val,
                                float* thr_dev, void* stream) {
  if (!coef_dev || !step_dev || !items_host || !x0 || !xe || !xe_op || !xbar || !d1 || !mprev) return fail("null argument");
  if (mode < 0 || mode > 2) return fail("items update: mode %d must be 0 (off), 1 (dynamic thresholding) or 2 (clamp)", mode);
  if (mode == 1 && !thr_dev) return fail("dynamic thresholding needs thr_dev");
  if (ld <= 0 || (ld & 3) || T <= 0 || n_items <= 0 || n != (size_t)n_items * T * ld)
    return fail("n (%zu) must hold the %d items of T (%d) rows of ld (%d) columns, ld a multiple of 4", n, n_items, T, ld);
  if (mode && (!(ratio >= 0.f && ratio <= 1.f) || !(max_val > 0.f))) return fail("ratio %g must be in [0, 1] and max_val %g > 0", (double)ratio, (double)max_val);
  if (solver_items_fit("item", reinterpret_cast<const SolverItem*>(items_host), nullptr, n_items, n_rows, nullptr, mprev2 ? nullptr : "mprev2 is needed",
                       seeds_dev ? nullptr : "seeds_dev is needed", mode, nullptr))
    return 1;
  SolverStep st = hook_step(coef_dev, step_dev, x0, xe, xe_op, precision, xbar, d1, mprev, mprev2, n, ld);
  st.T = T; st.nc = nc; st.lens = lens_dev; st.scale = scale_dev; st.seeds = reinterpret_cast<const unsigned long long*>(seeds_dev);
  if (mode) { st.mode = mode; st.ratio = ratio; st.max_val = max_val; }
  st.thr = thr_dev;
  return run_items_step(st, items_host, n_items, nullptr, (hipStream_t)stream);
}
// the same step under a per-item x0 correction: HOST arrays [n_items] of mode, ratio and max_val in place of the three scalars; the two launches the
// loop makes (the quantile only when a record has mode 1)
int ns2vc_k_solver_update_items_corrected(const float* coef_dev, int n_rows, const int32_t* step_dev, const int32_t* items_host, int n_items, const float* x0,
                                          float* xe, void* xe_op, int precision, float* xbar, float* d1, float* mprev, float* mprev2, size_t n, int ld, int T,
                                          const float* scale_dev, const uint64_t* seeds_dev, const int32_t* lens_dev, int nc, const int32_t* mode_host,
                                          const float* ratio_host, const float* max_val_host, float* thr_dev, void* stream) {
  if (!coef_dev || !step_dev || !items_host || !x0 || !xe || !xe_op || !xbar || !d1 || !mprev) return fail("null argument");
  if (!mode_host || !ratio_host || !max_val_host) return fail("items corrected update: the record table (mode, ratio, max_val) is needed");
  if (!thr_dev) return fail("items corrected update: thr_dev is needed");
  if (ld <= 0 || (ld & 3) || T <= 0 || n_items <= 0 || n != (size_t)n_items * T * ld)
    return fail("n (%zu) must hold the %d items of T (%d) rows of ld (%d) columns, ld a multiple of 4", n, n_items, T, ld);
  std::vector<ItemCorrect> cr;
  SolverStep st = hook_step(coef_dev, step_dev, x0, xe, xe_op, precision, xbar, d1, mprev, mprev2, n, ld);
  if (item_corrections_from(mode_host, ratio_host, max_val_host, n_items, cr, st.quant) ||
      solver_items_fit("item", reinterpret_cast<const SolverItem*>(items_host), nullptr, n_items, n_rows, nullptr, mprev2 ? nullptr : "mprev2 is needed",
                       seeds_dev ? nullptr : "seeds_dev is needed", 0, cr.data()))
    return 1;
  st.T = T; st.nc = nc; st.lens = lens_dev; st.scale = scale_dev; st.seeds = reinterpret_cast<const unsigned long long*>(seeds_dev); st.thr = thr_dev;
  return run_items_step(st, items_host, n_items, cr.data(), (hipStream_t)stream);
}
// a host slot list, checked (entries in [0, n_items), none twice), on the device for one hook call
static int upload_slots(const int32_t* slots_host, int n, int n_items, int** out_dev) {
  if (!slots_host || n <= 0 || n_items <= 0 || n > n_items) return fail("a slot list needs 1 .. %d entries, got %d", n_items, n);
  std::vector<char> seen((size_t)n_items, 0);
  for (int k = 0; k < n; ++k) {
    if (slots_host[k] < 0 || slots_host[k] >= n_items) return fail("slots[%d] = %d outside [0, %d)", k, (int)slots_host[k], n_items);
    if (seen[slots_host[k]]) return fail("slot %d is listed twice", (int)slots_host[k]);
    seen[slots_host[k]] = 1;
  }
  HIPCHK(hipMalloc((void**)out_dev, (size_t)n * sizeof(int)));
  if (hipMemcpy(*out_dev, slots_host, (size_t)n * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(*out_dev);
    *out_dev = nullptr;
    return fail("copy of the slot list failed");
  }
  return 0;
}
int ns2vc_k_sampler_admit(const float* x_T, int C, int T, int n, const int32_t* slots_host, int n_items, float* xe, void* xe_op, int precision, float* xbar,
                          float* d1, float* mprev, float* mprev2, int ld, const int32_t* lens_dev, int guided, void* stream) {
  if (!x_T || !xe || !xe_op || !xbar || !d1 || !mprev) return fail("null argument");
  if (C <= 0 || ld <= 0 || (ld & 3) || C > ld || T <= 0) return fail("C (%d) must be in 1 .. ld (%d), ld a multiple of 4, T (%d) positive", C, ld, T);
  int* sd = nullptr;
  if (upload_slots(slots_host, n, n_items, &sd)) return 1;
  hipStream_t s = (hipStream_t)stream;
  int rc = launched(launch_sampler_admit(x_T, C, T, n, sd, n_items, nullptr, nullptr, xe, xe_op, precision, xbar, d1, mprev, mprev2, ld,
                                         precision != PREC_F32 ? ld : 0, lens_dev, guided ? n_items : 0, s), "sampler_admit launch");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail("sampler_admit: stream synchronize failed");
  (void)hipFree(sd);
  return rc;
}
int ns2vc_k_sampler_take(const float* xe, int ld, int C, int T, int n, const int32_t* slots_host, int n_items, float* out, void* stream) {
  if (!xe || !out) return fail("null argument");
  if (C <= 0 || ld <= 0 || C > ld || T <= 0) return fail("C (%d) must be in 1 .. ld (%d), T (%d) positive", C, ld, T);
  int* sd = nullptr;
  if (upload_slots(slots_host, n, n_items, &sd)) return 1;
  hipStream_t s = (hipStream_t)stream;
  int rc = launched(launch_sampler_take(xe, ld, C, T, n, sd, n_items, out, nullptr, s), "sampler_take launch");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail("sampler_take: stream synchronize failed");
  (void)hipFree(sd);
  return rc;
}
int ns2vc_k_noise(const uint64_t* seeds_dev, int B, int C, int T, int ld, int step, const int32_t* lens_dev, float* out, void* stream) {
  return launched(launch_noise(reinterpret_cast<const unsigned long long*>(seeds_dev), B, C, T, ld, step, lens_dev, out, (hipStream_t)stream), "noise launch");
}
// the hold launch of the loop on its own: the held-row list is built from the host mask as ns2vc_sampler_set_known builds it, lives on the device
// for the one call, and the call returns when the launch is done
int ns2vc_k_hold_x0(float* x0, const float* known_rows, const uint8_t* mask_host, int n, int T, int ld, int nc, int halves, void* stream) {
  if (!x0 || !known_rows || !mask_host) return fail("null argument");
  if (n <= 0 || T <= 0 || ld <= 0 || (ld & 3) || nc <= 0 || nc > ld || (halves != 1 && halves != 2) || (size_t)n * T > (size_t)0x7fffffff - HOLD_LIST_HEAD)
    return fail("hold_x0: n (%d) and T (%d) positive, nc (%d) in 1 .. ld (%d), ld a multiple of 4, halves (%d) 1 or 2", n, T, nc, ld, halves);
  std::vector<int> list;
  std::vector<int32_t> last;
  if (hold_list_from_mask(mask_host, n, T, nullptr, list, last)) return 1;
  int* dev = nullptr;
  const size_t nb = ((size_t)HOLD_LIST_HEAD + (size_t)n * T) * sizeof(int);
  HIPCHK(hipMalloc((void**)&dev, nb));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (hipMemset(dev, 0, nb) != hipSuccess || hipMemcpy(dev, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
    rc = fail("hold_x0: copy of the row list failed");
  } else {
    rc = launched(launch_hold_x0(x0, known_rows, dev, n * T, ld, nc, halves, s), "hold_x0 launch");
    if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail("hold_x0: stream synchronize failed");
  }
  (void)hipFree(dev);
  return rc;
}
// host bytes on the device for one hook call
static int upload_bytes(const void* host, size_t nb, void** out_dev, const char* what) {
  HIPCHK(hipMalloc(out_dev, nb));
  if (hipMemcpy(*out_dev, host, nb, hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(*out_dev);
    *out_dev = nullptr;
    return fail("%s: copy to the device failed", what);
  }
  return 0;
}
// the hold launch of a slot loop on its own: the host mask lives on the device for the one call
int ns2vc_k_hold_slots(float* x0, const float* known_rows, const uint8_t* mask_host, int n, int T, int ld, int nc, int halves, void* stream) {
  if (!x0 || !known_rows || !mask_host) return fail("null argument");
  if (n <= 0 || T <= 0 || ld <= 0 || (ld & 3) || nc <= 0 || nc > ld || (halves != 1 && halves != 2) || (size_t)n * T > (size_t)0x7fffffff)
    return fail("hold_slots: n (%d) and T (%d) positive, nc (%d) in 1 .. ld (%d), ld a multiple of 4, halves (%d) 1 or 2", n, T, nc, ld, halves);
  void* md = nullptr;
  if (upload_bytes(mask_host, (size_t)n * T, &md, "hold_slots")) return 1;
  hipStream_t s = (hipStream_t)stream;
  int rc = launched(launch_hold_slots(x0, known_rows, static_cast<const uint8_t*>(md), n * T, ld, nc, halves, s), "hold_slots launch");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail("hold_slots: stream synchronize failed");
  (void)hipFree(md);
  return rc;
}
// the known-frame scatter of a slot loop on its own; the slot list goes to the device AS GIVEN (the kernel skips an entry outside [0, nslots))
int ns2vc_k_known_items(const float* known_nct, const uint8_t* mask_host, int C, int T, int n, const int32_t* slots_host, int nslots, float* known_rows,
                        uint8_t* mask_dev, int ld, void* stream) {
  if (!slots_host || !mask_dev || !known_rows) return fail("null argument");
  if ((known_nct != nullptr) != (mask_host != nullptr)) return fail("known_items: the latent and the mask are given together (both NULL = clear)");
  if (C <= 0 || ld <= 0 || C > ld || T <= 0 || n <= 0 || nslots <= 0 || (size_t)nslots * T > (size_t)0x7fffffff)
    return fail("known_items: C (%d) in 1 .. ld (%d), T (%d), n (%d) and nslots (%d) positive", C, ld, T, n, nslots);
  void *sd = nullptr, *md = nullptr;
  if (upload_bytes(slots_host, (size_t)n * sizeof(int), &sd, "known_items")) return 1;
  if (mask_host && upload_bytes(mask_host, (size_t)n * T, &md, "known_items")) { (void)hipFree(sd); return 1; }
  hipStream_t s = (hipStream_t)stream;
  int rc = launched(launch_known_items(known_nct, static_cast<const uint8_t*>(md), C, T, n, static_cast<const int*>(sd), nslots, known_rows, mask_dev, ld, s),
                    "known_items launch");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail("known_items: stream synchronize failed");
  (void)hipFree(sd);
  if (md) (void)hipFree(md);
  return rc;
}

// the suspend / resume launches on their own; the slot list goes to the device AS GIVEN (the kernels skip an entry outside [0, n_items)),
// rec_dev (DEVICE [n_items][4], or NULL) is the record table the launches write
int ns2vc_k_sampler_suspend(const float* xe, const float* xbar, const float* d1, const float* mprev, const float* mprev2, int T, int ld, int n,
                            const int32_t* slots_host, int n_items, float* state_out, int32_t* rec_dev, void* stream) {
  if (!xe || !xbar || !d1 || !mprev || !slots_host || !state_out) return fail("null argument");
  if (T <= 0 || ld <= 0 || (ld & 3) || n <= 0 || n_items <= 0) return fail("sampler_suspend: T (%d), n (%d) and n_items (%d) positive, ld (%d) a positive multiple of 4", T, n, n_items, ld);
  void* sd = nullptr;
  if (upload_bytes(slots_host, (size_t)n * sizeof(int), &sd, "sampler_suspend")) return 1;
  hipStream_t s = (hipStream_t)stream;
  int rc = launched(launch_sampler_suspend(xe, xbar, d1, mprev, mprev2, T, ld, n, static_cast<const int*>(sd), n_items, state_out,
                                           reinterpret_cast<SolverItem*>(rec_dev), s), "sampler_suspend launch");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail("sampler_suspend: stream synchronize failed");
  (void)hipFree(sd);
  return rc;
}
int ns2vc_k_sampler_resume(const float* state_in, int T, int ld, int n, const int32_t* slots_host, int n_items, const int32_t* records_host, int32_t* rec_dev,
                           float* xe, void* xe_op, int precision, float* xbar, float* d1, float* mprev, float* mprev2, int guided, void* stream) {
  if (!state_in || !slots_host || !xe || !xe_op || !xbar || !d1 || !mprev) return fail("null argument");
  if (T <= 0 || ld <= 0 || (ld & 3) || n <= 0 || n_items <= 0) return fail("sampler_resume: T (%d), n (%d) and n_items (%d) positive, ld (%d) a positive multiple of 4", T, n, n_items, ld);
  if ((rec_dev != nullptr) != (records_host != nullptr)) return fail("sampler_resume: the records and their device table are given together (both NULL = none)");
  void *sd = nullptr, *rd = nullptr;
  if (upload_bytes(slots_host, (size_t)n * sizeof(int), &sd, "sampler_resume")) return 1;
  if (records_host && upload_bytes(records_host, (size_t)n * sizeof(SolverItem), &rd, "sampler_resume")) { (void)hipFree(sd); return 1; }
  hipStream_t s = (hipStream_t)stream;
  int rc = launched(launch_sampler_resume(state_in, T, ld, n, static_cast<const int*>(sd), n_items, static_cast<const SolverItem*>(rd),
                                          reinterpret_cast<SolverItem*>(rec_dev), xe, xe_op, precision, xbar, d1, mprev, mprev2,
                                          precision != PREC_F32 ? ld : 0, guided ? n_items : 0, s), "sampler_resume launch");
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = fail("sampler_resume: stream synchronize failed");
  (void)hipFree(sd);
  if (rd) (void)hipFree(rd);
  return rc;
}

}  // extern "C"
