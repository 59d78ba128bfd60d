// Weights of the engine: the UNet topology, the table of expected state-dict entries, and the packing of the loaded fp32 tensors into the
// device-resident forms the kernels read (rows padded to 128, LayerNorm folds, fused / tile-major / streamed layouts).
#include "engine_internal.h"

#include <algorithm>
#include <cstring>

namespace ns2vc {

// ------------------------------------------------------------------------------------
// topology (same rules as ns2vc_amd/spec.py::topology)
// ------------------------------------------------------------------------------------
std::vector<BlockW> make_topology(const ns2vc_unet_cfg& c) {
  std::vector<BlockW> out;
  const int n = c.n_levels;
  int out_c = c.block_out_channels[0];
  for (int i = 0; i < n; ++i) {
    const int in_c = out_c;
    out_c = c.block_out_channels[i];
    BlockW b;
    b.kind = "down"; b.index = i; b.level = i; b.channels = out_c;
    const bool cross = (i != n - 1);      // ("CrossAttnDownBlock2D",)*3 + ("DownBlock2D",)
    for (int j = 0; j < c.layers_per_block; ++j) {
      ResnetW r;
      r.prefix = "down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
      r.cin = j == 0 ? in_c : out_c; r.cout = out_c; r.shortcut = r.cin != r.cout;
      b.res.push_back(r);
      if (cross) {
        AttnW a;
        a.prefix = "down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j);
        a.dim = out_c;
        b.attn.push_back(a);
      }
    }
    b.sampler = (i != n - 1) ? 1 : 0;
    out.push_back(b);
  }
  {
    BlockW m;
    const int mc = c.block_out_channels[n - 1];
    m.kind = "mid"; m.index = 0; m.level = n - 1; m.channels = mc;
    for (int j = 0; j < 2; ++j) {
      ResnetW r;
      r.prefix = "mid_block.resnets." + std::to_string(j);
      r.cin = r.cout = mc; r.shortcut = false;
      m.res.push_back(r);
    }
    AttnW a;
    a.prefix = "mid_block.attentions.0"; a.dim = mc;
    m.attn.push_back(a);
    out.push_back(m);
  }
  out_c = c.block_out_channels[n - 1];
  for (int i = 0; i < n; ++i) {
    const int prev_c = out_c;
    out_c = c.block_out_channels[n - 1 - i];
    const int in_c = c.block_out_channels[std::max(n - 2 - i, 0)];
    BlockW b;
    b.kind = "up"; b.index = i; b.level = n - 1 - i; b.channels = out_c;
    const bool cross = (i != 0);          // ("UpBlock2D",) + ("CrossAttnUpBlock2D",)*3
    const int nl = c.layers_per_block + 1;
    for (int j = 0; j < nl; ++j) {
      ResnetW r;
      r.prefix = "up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j);
      const int skip_c = (j == nl - 1) ? in_c : out_c;
      r.cin = (j == 0 ? prev_c : out_c) + skip_c; r.cout = out_c; r.shortcut = true;
      b.res.push_back(r);
      if (cross) {
        AttnW a;
        a.prefix = "up_blocks." + std::to_string(i) + ".attentions." + std::to_string(j);
        a.dim = out_c;
        b.attn.push_back(a);
      }
    }
    b.sampler = (i != n - 1) ? 2 : 0;
    out.push_back(b);
  }
  return out;
}

static void expect(ns2vc_unet* h, const std::string& k, std::vector<int64_t> shape) { h->expected.emplace_back(k, std::move(shape)); }

void build_expected(ns2vc_unet* h) {
  const auto& c = h->cfg;
  const int64_t c0 = c.block_out_channels[0], temb = 4 * c0, cross = c.cross_attention_dim;
  const int64_t cin = c.latent_channels + c.content_channels;
  expect(h, "conv_in.weight", {c0, cin, 3}); expect(h, "conv_in.bias", {c0});
  expect(h, "time_embedding.linear_1.weight", {temb, c0}); expect(h, "time_embedding.linear_1.bias", {temb});
  expect(h, "time_embedding.linear_2.weight", {temb, temb}); expect(h, "time_embedding.linear_2.bias", {temb});
  expect(h, "add_embedding.norm1.weight", {cross}); expect(h, "add_embedding.norm1.bias", {cross});
  expect(h, "add_embedding.pool.positional_embedding", {1, cross});
  for (const char* p : {"k_proj", "q_proj", "v_proj"}) {
    expect(h, std::string("add_embedding.pool.") + p + ".weight", {cross, cross});
    expect(h, std::string("add_embedding.pool.") + p + ".bias", {cross});
  }
  expect(h, "add_embedding.proj.weight", {temb, cross}); expect(h, "add_embedding.proj.bias", {temb});
  expect(h, "add_embedding.norm2.weight", {temb}); expect(h, "add_embedding.norm2.bias", {temb});
  for (const auto& b : h->blocks) {
    for (const auto& a : b.attn) {
      const int64_t d = a.dim;
      const std::string t = a.prefix + ".transformer_blocks.0";
      expect(h, a.prefix + ".norm.weight", {d}); expect(h, a.prefix + ".norm.bias", {d});
      expect(h, a.prefix + ".proj_in.weight", {d, d, 1}); expect(h, a.prefix + ".proj_in.bias", {d});
      for (const char* nn : {"norm1", "norm2", "norm3"}) { expect(h, t + "." + nn + ".weight", {d}); expect(h, t + "." + nn + ".bias", {d}); }
      expect(h, t + ".attn1.to_q.weight", {d, d}); expect(h, t + ".attn1.to_k.weight", {d, d}); expect(h, t + ".attn1.to_v.weight", {d, d});
      expect(h, t + ".attn1.to_out.0.weight", {d, d}); expect(h, t + ".attn1.to_out.0.bias", {d});
      expect(h, t + ".attn2.to_q.weight", {d, d}); expect(h, t + ".attn2.to_k.weight", {d, cross}); expect(h, t + ".attn2.to_v.weight", {d, cross});
      expect(h, t + ".attn2.to_out.0.weight", {d, d}); expect(h, t + ".attn2.to_out.0.bias", {d});
      expect(h, t + ".ff.net.0.proj.weight", {8 * d, d}); expect(h, t + ".ff.net.0.proj.bias", {8 * d});
      expect(h, t + ".ff.net.2.weight", {d, 4 * d}); expect(h, t + ".ff.net.2.bias", {d});
      expect(h, a.prefix + ".proj_out.weight", {d, d, 1}); expect(h, a.prefix + ".proj_out.bias", {d});
    }
    for (const auto& r : b.res) {
      expect(h, r.prefix + ".norm1.weight", {r.cin}); expect(h, r.prefix + ".norm1.bias", {r.cin});
      expect(h, r.prefix + ".conv1.weight", {r.cout, r.cin, 3}); expect(h, r.prefix + ".conv1.bias", {r.cout});
      expect(h, r.prefix + ".time_emb_proj.weight", {2 * r.cout, temb}); expect(h, r.prefix + ".time_emb_proj.bias", {2 * r.cout});
      expect(h, r.prefix + ".norm2.weight", {r.cout}); expect(h, r.prefix + ".norm2.bias", {r.cout});
      expect(h, r.prefix + ".conv2.weight", {r.cout, r.cout, 3}); expect(h, r.prefix + ".conv2.bias", {r.cout});
      if (r.shortcut) { expect(h, r.prefix + ".conv_shortcut.weight", {r.cout, r.cin, 1}); expect(h, r.prefix + ".conv_shortcut.bias", {r.cout}); }
    }
    if (b.sampler) {
      const std::string p = b.kind == "down" ? "down_blocks." + std::to_string(b.index) + ".downsamplers.0.conv"
                                             : "up_blocks." + std::to_string(b.index) + ".upsamplers.0.conv";
      expect(h, p + ".weight", {b.channels, b.channels, 3}); expect(h, p + ".bias", {b.channels});
    }
  }
  expect(h, "conv_norm_out.weight", {c0}); expect(h, "conv_norm_out.bias", {c0});
  expect(h, "conv_out.weight", {c.latent_channels, c0, 3}); expect(h, "conv_out.bias", {c.latent_channels});
}

// ------------------------------------------------------------------------------------
// weight packing (host, fp32/double) -> device
// ------------------------------------------------------------------------------------
// sum_k of the operand-rounded weight row (what the MFMA will actually multiply), accumulated in double
std::vector<float> rounded_rowsum(const float* rows, int N, int K, int Np, int prec) {
  std::vector<float> ws(Np, 0.f);
  for (int n = 0; n < N; ++n) {
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      float v = rows[(size_t)n * K + k];
      if (prec != PREC_F32) v = op16_bits_to_f32(f32_to_op16_bits(v, prec), prec);
      acc += (double)v;
    }
    ws[n] = (float)acc;
  }
  return ws;
}

namespace {
struct Packer {
  ns2vc_unet* h;
  int err = 0;

  const HostTensor& T(const std::string& k) {
    auto it = h->raw.find(k);
    if (it == h->raw.end()) { err = fail("weight %s missing", k.c_str()); static HostTensor empty; return empty; }
    return it->second;
  }
  // a device copy of `bytes` host bytes that lives as long as the engine's weights; on failure `err` is set and the result is null
  void* upload(const void* src, size_t bytes, const char* what = "weights") {
    void* d = nullptr;
    if (hipMalloc(&d, std::max<size_t>(bytes, 1)) != hipSuccess) { err = fail("hipMalloc failed (%s)", what); return nullptr; }
    h->weight_allocs.push_back(d);
    if (hipMemcpy(d, src, bytes, hipMemcpyHostToDevice) != hipSuccess) err = fail("hipMemcpy failed (weights)");
    return d;
  }
  float* upload_f32(const std::vector<float>& v) { return (float*)upload(v.data(), v.size() * sizeof(float)); }
  void* upload_u16(const std::vector<unsigned short>& v) { return upload(v.data(), v.size() * 2); }
  float* vec(const std::string& k) { return upload_f32(T(k).data); }
  // rows: [N][K] fp32, bias: [N] or empty.  Pads N to a multiple of 128 with zero rows.
  // tile3_ctot > 0: a k = 3 conv weight (K = 3 * tile3_ctot + tile3_c2): also packed tile-major for the tap-sharing kernel
  int prec_override = -1;      // pack the next weights in this precision instead of the engine's (exact_io: fp32 copies of four weights of a 16-bit engine)
  PackedW pack(const std::vector<float>& rows, int N, int K, const std::vector<float>& bias, bool want_wsum = false, int tile3_ctot = 0, int tile3_c2 = 0) {
    const int wprec = prec_override >= 0 ? prec_override : h->prec;
    PackedW p;
    const int Np = round_up(N, 128);
    p.N = Np; p.K = K;
    // (the second, tile-major copy only when the tap-sharing kernel will read it; when the layout cannot be built the kernel falls back to the
    //  [N][K] rows and the engine says so once)
    if (tile3_ctot > 0 && K == 3 * tile3_ctot + tile3_c2 && h->conv_ts && h->conv_wtiled) {
      std::vector<unsigned char> img;
      if (pack_conv3_tiled(rows.data(), N, tile3_ctot, tile3_c2, wprec, img) != hipSuccess) {
        if (!h->warned_wtiled) { fprintf(stderr, "ns2vc: tile-major conv weights unavailable for a %d x %d weight (channels not a multiple of the chunk): row-major fallback\n", N, K); h->warned_wtiled = true; }
      } else {
        p.wt = upload(img.data(), img.size(), "tile-major weights");
        if (!p.wt) return p;
      }
    }
    if (want_wsum) p.wsum = upload_f32(rounded_rowsum(rows.data(), N, K, Np, wprec));
    if (wprec != PREC_F32) {
      std::vector<uint16_t> q((size_t)Np * K, 0);
      for (size_t i = 0; i < (size_t)N * K; ++i) q[i] = f32_to_op16_bits(rows[i], wprec);
      p.w = upload(q.data(), q.size() * 2);
    } else {
      std::vector<float> q((size_t)Np * K, 0.f);
      memcpy(q.data(), rows.data(), (size_t)N * K * sizeof(float));
      p.w = upload(q.data(), q.size() * 4);
    }
    if (!p.w) return p;
    if (!bias.empty()) {
      std::vector<float> bb(Np, 0.f);
      memcpy(bb.data(), bias.data(), (size_t)N * sizeof(float));
      p.bias = upload_f32(bb);
    }
    return p;
  }

  // conv weight (Cout, Cin, taps) -> rows [Cout][tap*CinP + c'], channels [c_lo, c_hi) of the input, padded to CinP
  std::vector<float> conv_rows(const HostTensor& w, int c_lo, int c_hi, int CinP) {
    const int Cout = (int)w.shape[0], Cin = (int)w.shape[1], taps = (int)w.shape[2];
    std::vector<float> rows((size_t)Cout * taps * CinP, 0.f);
    for (int n = 0; n < Cout; ++n)
      for (int c = c_lo; c < c_hi; ++c)
        for (int t = 0; t < taps; ++t) rows[((size_t)n * taps + t) * CinP + (c - c_lo)] = w.data[((size_t)n * Cin + c) * taps + t];
    return rows;
  }
  // rows [N][taps][C] -> [N][taps][3 C] for activations laid out [hi(x) | lo(x) | hi(x)]: (w, w, w - round(w)); pack() then rounds each -> (hi(w), hi(w), lo(w))
  std::vector<float> pair_rows(const std::vector<float>& rows, int N, int taps, int C) {
    std::vector<float> out((size_t)N * taps * 3 * C);
    for (size_t nt = 0; nt < (size_t)N * taps; ++nt)
      for (int c = 0; c < C; ++c) {
        const float w = rows[nt * C + c];
        out[nt * 3 * C + c] = out[nt * 3 * C + C + c] = w;
        out[nt * 3 * C + 2 * C + c] = w - op16_bits_to_f32(f32_to_op16_bits(w, h->prec), h->prec);
      }
    return out;
  }
  PackedW conv(const std::string& prefix, bool tile3 = false) {
    const HostTensor& w = T(prefix + ".weight");
    if (err) return {};
    const int Cout = (int)w.shape[0], Cin = (int)w.shape[1], taps = (int)w.shape[2];
    return pack(conv_rows(w, 0, Cin, Cin), Cout, taps * Cin, T(prefix + ".bias").data, false, (tile3 && taps == 3) ? Cin : 0, 0);
  }
  // Linear whose input is LayerNorm(x): fold gamma into W and beta into the bias.
  void ln_fold(const HostTensor& w, const HostTensor* b, const HostTensor& g, const HostTensor& be, std::vector<float>& rows,
               std::vector<float>& bias) {
    const int N = (int)w.shape[0], K = (int)w.shape[1];
    const size_t r0 = rows.size(), b0 = bias.size();
    rows.resize(r0 + (size_t)N * K);
    bias.resize(b0 + N);
    for (int n = 0; n < N; ++n) {
      double acc = b ? (double)b->data[n] : 0.0;
      for (int k = 0; k < K; ++k) {
        const float wv = w.data[(size_t)n * K + k];
        rows[r0 + (size_t)n * K + k] = wv * g.data[k];
        acc += (double)wv * (double)be.data[k];
      }
      bias[b0 + n] = (float)acc;
    }
  }
};

// weight stream + stage-2 constants of one token-local chain (rowchain.hip): w1 [d][d] plain, w2 [n2][d] LayerNorm-folded
// with its folded bias; only for the shapes / precisions the kernel serves, otherwise both outputs stay null
static int chain_stream(Packer& P, const std::vector<float>& w1, const std::vector<float>& w2, const std::vector<float>& b2, int d, int n2,
                        void*& stream_dev, float*& consts_dev, void** sliced_dev = nullptr) {
  ns2vc_unet* h = P.h;
  stream_dev = nullptr; consts_dev = nullptr;
  if (P.err) return 1;
  if (!rowchain_eligible(d, n2, 64, h->prec)) return 0;
  std::vector<unsigned short> st;
  if (pack_rowchain_stream(w1.data(), w2.data(), d, n2, h->prec, st) != hipSuccess) return fail("row-chain stream packing failed");
  void* dev = P.upload_u16(st);
  if (P.err) return 1;
  if (sliced_dev && d == 384) {     // the same chain packed for two N-slices (planner: where 64-token blocks fill less than half of the chip)
    *sliced_dev = nullptr;
    if (pack_rowchain_stream(w1.data(), w2.data(), d, n2, h->prec, st, 2) != hipSuccess) return fail("row-chain stream packing failed (sliced)");
    *sliced_dev = P.upload_u16(st);
    if (P.err) return 1;
  }
  const std::vector<float> ws = rounded_rowsum(w2.data(), n2, d, n2, h->prec);
  std::vector<float> cs((size_t)n2 * 2);
  for (int r = 0; r < n2; ++r) { cs[2 * r] = ws[r]; cs[2 * r + 1] = b2[r]; }
  stream_dev = dev;
  consts_dev = P.upload_f32(cs);
  return P.err;
}
}  // namespace

int pack_all(ns2vc_unet* h) {
  Packer P{h};
  const auto& c = h->cfg;
  const int c0 = c.block_out_channels[0], temb = 4 * c0, cross = c.cross_attention_dim;
  const int lat = c.latent_channels, CP = h->CP;
  // conv_in split: x part (latent channels, padded to CP) per step, content part hoisted
  {
    const HostTensor& w = P.T("conv_in.weight");
    if (P.err) return 1;
    h->conv_in_x = P.pack(P.conv_rows(w, 0, lat, CP), c0, 3 * CP, {}, false, CP, 0);
    h->conv_in_c = P.pack(P.conv_rows(w, lat, lat + c.content_channels, c.content_channels), c0, 3 * c.content_channels, P.T("conv_in.bias").data);
    if (h->prec != PREC_F32) {
      const int cc = c.content_channels;
      h->conv_in_xp = P.pack(P.pair_rows(P.conv_rows(w, 0, lat, CP), c0, 3, CP), c0, 9 * CP, {}, false, 3 * CP, 0);
      h->conv_in_cp = P.pack(P.pair_rows(P.conv_rows(w, lat, lat + cc, cc), c0, 3, cc), c0, 9 * cc, P.T("conv_in.bias").data, false, 3 * cc, 0);
    }
    if (h->prec != PREC_F32) {
      P.prec_override = PREC_F32;
      h->conv_in_x32 = P.pack(P.conv_rows(w, 0, lat, CP), c0, 3 * CP, {}, false, CP, 0);
      h->conv_in_c32 = P.pack(P.conv_rows(w, lat, lat + c.content_channels, c.content_channels), c0, 3 * c.content_channels, P.T("conv_in.bias").data);
      P.prec_override = -1;
    }
  }
  // time MLP, transposed to [in][out] for coalesced GEMV reads
  auto transpose = [&](const HostTensor& w) {
    const int N = (int)w.shape[0], K = (int)w.shape[1];
    std::vector<float> t((size_t)N * K);
    for (int n = 0; n < N; ++n) for (int k = 0; k < K; ++k) t[(size_t)k * N + n] = w.data[(size_t)n * K + k];
    return t;
  };
  h->t_w1t = P.upload_f32(transpose(P.T("time_embedding.linear_1.weight"))); h->t_b1 = P.vec("time_embedding.linear_1.bias");
  h->t_w2t = P.upload_f32(transpose(P.T("time_embedding.linear_2.weight"))); h->t_b2 = P.vec("time_embedding.linear_2.bias");
  // add_embedding
  h->p_n1g = P.vec("add_embedding.norm1.weight"); h->p_n1b = P.vec("add_embedding.norm1.bias");
  h->p_pos = P.vec("add_embedding.pool.positional_embedding");
  {
    std::vector<float> rows, bias;
    for (const char* p : {"q_proj", "k_proj", "v_proj"}) {
      const HostTensor& w = P.T(std::string("add_embedding.pool.") + p + ".weight");
      const HostTensor& b = P.T(std::string("add_embedding.pool.") + p + ".bias");
      if (P.err) return 1;
      rows.insert(rows.end(), w.data.begin(), w.data.end());
      bias.insert(bias.end(), b.data.begin(), b.data.end());
    }
    h->pool_qkv = P.pack(rows, 3 * cross, cross, bias);
  }
  h->p_projT = P.upload_f32(transpose(P.T("add_embedding.proj.weight"))); h->p_projb = P.vec("add_embedding.proj.bias");
  h->p_n2g = P.vec("add_embedding.norm2.weight"); h->p_n2b = P.vec("add_embedding.norm2.bias");
  if (P.err) return 1;

  std::vector<float> temb_rows, temb_bias, kv_rows;
  int temb_off = 0, kv_off = 0;
  for (auto& b : h->blocks) {
    for (auto& r : b.res) {
      r.n1g = P.vec(r.prefix + ".norm1.weight"); r.n1b = P.vec(r.prefix + ".norm1.bias");
      r.n2g = P.vec(r.prefix + ".norm2.weight"); r.n2b = P.vec(r.prefix + ".norm2.bias");
      r.conv1 = P.conv(r.prefix + ".conv1", true);
      if (r.shortcut) {   // conv2 and the 1x1 shortcut share one GEMM: K = 3*cout + cin, biases summed
        const HostTensor& w2 = P.T(r.prefix + ".conv2.weight");
        const HostTensor& ws = P.T(r.prefix + ".conv_shortcut.weight");
        const HostTensor& b2 = P.T(r.prefix + ".conv2.bias");
        const HostTensor& bs = P.T(r.prefix + ".conv_shortcut.bias");
        if (P.err) return 1;
        const std::vector<float> r2 = P.conv_rows(w2, 0, r.cout, r.cout);
        const int K1 = 3 * r.cout, K2 = r.cin;
        std::vector<float> rows((size_t)r.cout * (K1 + K2)), bias(r.cout);
        for (int n = 0; n < r.cout; ++n) {
          memcpy(&rows[(size_t)n * (K1 + K2)], &r2[(size_t)n * K1], K1 * sizeof(float));
          memcpy(&rows[(size_t)n * (K1 + K2) + K1], &ws.data[(size_t)n * K2], K2 * sizeof(float));
          bias[n] = b2.data[n] + bs.data[n];
        }
        r.conv2 = P.pack(rows, r.cout, K1 + K2, bias, false, r.cout, K2);
      } else {
        r.conv2 = P.conv(r.prefix + ".conv2", true);
      }
      const HostTensor& tw = P.T(r.prefix + ".time_emb_proj.weight");
      const HostTensor& tb = P.T(r.prefix + ".time_emb_proj.bias");
      if (P.err) return 1;
      r.temb_off = temb_off;
      temb_rows.insert(temb_rows.end(), tw.data.begin(), tw.data.end());
      temb_bias.insert(temb_bias.end(), tb.data.begin(), tb.data.end());
      temb_off += 2 * r.cout;
    }
    for (auto& a : b.attn) {
      const std::string t = a.prefix + ".transformer_blocks.0";
      const int d = a.dim;
      a.ng = P.vec(a.prefix + ".norm.weight"); a.nb = P.vec(a.prefix + ".norm.bias");
      a.proj_in = P.conv(a.prefix + ".proj_in");
      a.proj_out = P.conv(a.prefix + ".proj_out");
      {  // fused q|k|v of the self-attention, LayerNorm(norm1) folded in
        std::vector<float> rows, bias;
        for (const char* nm : {"to_q", "to_k", "to_v"}) P.ln_fold(P.T(t + ".attn1." + nm + ".weight"), nullptr, P.T(t + ".norm1.weight"), P.T(t + ".norm1.bias"), rows, bias);
        if (P.err) return 1;
        a.qkv = P.pack(rows, 3 * d, d, bias, true);
        if (chain_stream(P, P.T(a.prefix + ".proj_in.weight").data, rows, bias, d, 3 * d, a.chain_in, a.chain_in_consts, &a.chain_in_s2)) return 1;
      }
      a.o1 = P.pack(P.T(t + ".attn1.to_out.0.weight").data, d, d, P.T(t + ".attn1.to_out.0.bias").data);
      {
        std::vector<float> rows, bias;
        P.ln_fold(P.T(t + ".attn2.to_q.weight"), nullptr, P.T(t + ".norm2.weight"), P.T(t + ".norm2.bias"), rows, bias);
        if (P.err) return 1;
        a.q2 = P.pack(rows, d, d, bias, true);
        if (chain_stream(P, P.T(t + ".attn1.to_out.0.weight").data, rows, bias, d, d, a.chain_mid, a.chain_mid_consts)) return 1;
      }
      a.o2 = P.pack(P.T(t + ".attn2.to_out.0.weight").data, d, d, P.T(t + ".attn2.to_out.0.bias").data);
      std::vector<float> ff1_rows, ff1_bias;     // packed ff.net.0 (kept for the fused feed-forward stream below)
      {  // GEGLU projection: LayerNorm(norm3) folded, rows interleaved in (32 value | 32 gate) groups
        std::vector<float> rows, bias;
        P.ln_fold(P.T(t + ".ff.net.0.proj.weight"), &P.T(t + ".ff.net.0.proj.bias"), P.T(t + ".norm3.weight"), P.T(t + ".norm3.bias"), rows, bias);
        if (P.err) return 1;
        const int inner = 4 * d;
        std::vector<float> rows2((size_t)8 * d * d), bias2(8 * d);
        for (int gidx = 0; gidx < inner / 32; ++gidx)
          for (int i = 0; i < 32; ++i) {
            const int v_src = 32 * gidx + i, g_src = inner + 32 * gidx + i;
            const int v_dst = 64 * gidx + i, g_dst = 64 * gidx + 32 + i;
            memcpy(&rows2[(size_t)v_dst * d], &rows[(size_t)v_src * d], d * sizeof(float));
            memcpy(&rows2[(size_t)g_dst * d], &rows[(size_t)g_src * d], d * sizeof(float));
            bias2[v_dst] = bias[v_src];
            bias2[g_dst] = bias[g_src];
          }
        a.ff1 = P.pack(rows2, 8 * d, d, bias2, true);
        ff1_rows.swap(rows2); ff1_bias.swap(bias2);
      }
      a.ff2 = P.pack(P.T(t + ".ff.net.2.weight").data, d, 4 * d, P.T(t + ".ff.net.2.bias").data);
      {  // ff.net.2 folded into proj_out (attention.py:178-203 + transformer_1d.py:287-295):
         //   proj_out(y + W2 g + b2) + x = [Wpo W2 | Wpo] [g | y] + (Wpo b2 + bpo) + x
         // one GEMM, K = 4d (GEGLU output) + d (second K segment: the operand copy of y).  Products in double.
        const HostTensor& w2 = P.T(t + ".ff.net.2.weight");      // [d][4d]
        const HostTensor& b2 = P.T(t + ".ff.net.2.bias");
        const HostTensor& wp = P.T(a.prefix + ".proj_out.weight"); // [d][d][1]
        const HostTensor& bp = P.T(a.prefix + ".proj_out.bias");
        if (P.err) return 1;
        const int K1 = 4 * d, K2 = d;
        std::vector<float> rows((size_t)d * (K1 + K2)), bias(d);
        std::vector<double> acc(K1);
        for (int n = 0; n < d; ++n) {
          std::fill(acc.begin(), acc.end(), 0.0);
          double bacc = (double)bp.data[n];
          for (int j = 0; j < d; ++j) {
            const double wpj = (double)wp.data[(size_t)n * d + j];
            const float* w2r = &w2.data[(size_t)j * K1];
            for (int k = 0; k < K1; ++k) acc[k] += wpj * (double)w2r[k];
            bacc += wpj * (double)b2.data[j];
          }
          float* r = &rows[(size_t)n * (K1 + K2)];
          for (int k = 0; k < K1; ++k) r[k] = (float)acc[k];
          memcpy(r + K1, &wp.data[(size_t)n * d], (size_t)K2 * sizeof(float));
          bias[n] = (float)bacc;
        }
        a.ffpo = P.pack(rows, d, K1 + K2, bias);
        if (h->prec != PREC_F32 && (d == 128 || d == 256)) {   // fused feed-forward + proj_out (csrc/ffn.hip)
          std::vector<unsigned short> st;
          for (int pre = 0; pre < 2; ++pre) {
            const float* w0 = pre ? P.T(t + ".attn2.to_out.0.weight").data.data() : nullptr;
            if (P.err) return 1;
            if (pack_ffn_stream(ff1_rows.data(), rows.data(), w0, d, h->prec, st) != hipSuccess) return fail("ffn stream packing failed");
            (pre ? a.ffn_pre_stream : a.ffn_stream) = P.upload_u16(st);
            if (P.err) return 1;
          }
          const std::vector<float> ws = rounded_rowsum(ff1_rows.data(), 8 * d, d, 8 * d, h->prec);
          std::vector<float> cs((size_t)8 * d * 2);
          for (int r = 0; r < 8 * d; ++r) { cs[2 * r] = ws[r]; cs[2 * r + 1] = ff1_bias[r]; }
          a.ffn_consts = P.upload_f32(cs);
        } else {
          a.ffn_stream = nullptr; a.ffn_pre_stream = nullptr; a.ffn_consts = nullptr;
        }
        if (geglu_eligible(d, 1, h->prec)) {                   // token-stationary GEGLU projection (csrc/geglu.hip)
          std::vector<unsigned short> st;
          std::vector<float> cs;
          if (pack_geglu_stream(ff1_rows.data(), ff1_bias.data(), d, h->prec, st, cs) != hipSuccess) return fail("geglu stream packing failed");
          a.geglu_stream = P.upload_u16(st);
          if (P.err) return 1;
          a.geglu_consts = P.upload_f32(cs);
        }
      }
      {  // cross-attention k|v of this block into the hoisted all-blocks projection
        const HostTensor& wk = P.T(t + ".attn2.to_k.weight");
        const HostTensor& wv = P.T(t + ".attn2.to_v.weight");
        if (P.err) return 1;
        a.kv_off = kv_off;
        kv_rows.insert(kv_rows.end(), wk.data.begin(), wk.data.end());
        kv_rows.insert(kv_rows.end(), wv.data.begin(), wv.data.end());
        kv_off += 2 * d;
      }
    }
    if (b.sampler) {
      const std::string p = b.kind == "down" ? "down_blocks." + std::to_string(b.index) + ".downsamplers.0.conv"
                                             : "up_blocks." + std::to_string(b.index) + ".upsamplers.0.conv";
      b.samp = P.conv(p);
    }
    if (P.err) return 1;
  }
  h->n_temb = temb_off;
  h->temb_all = P.pack(temb_rows, temb_off, temb, temb_bias);
  if (h->prec != PREC_F32) { P.prec_override = PREC_F32; h->temb_all32 = P.pack(temb_rows, temb_off, temb, temb_bias); P.prec_override = -1; }
  h->n_kv = kv_off;
  h->kv_all = P.pack(kv_rows, kv_off, cross, {});
  h->out_ng = P.vec("conv_norm_out.weight"); h->out_nb = P.vec("conv_norm_out.bias");
  {
    const HostTensor& w = P.T("conv_out.weight");
    if (P.err) return 1;
    h->conv_out = P.pack(P.conv_rows(w, 0, c0, c0), lat, 3 * c0, P.T("conv_out.bias").data, false, c0, 0);
    if (h->prec != PREC_F32) h->conv_outp = P.pack(P.pair_rows(P.conv_rows(w, 0, c0, c0), lat, 3, c0), lat, 9 * c0, P.T("conv_out.bias").data, false, 3 * c0, 0);
    if (h->prec != PREC_F32) { P.prec_override = PREC_F32; h->conv_out32 = P.pack(P.conv_rows(w, 0, c0, c0), lat, 3 * c0, P.T("conv_out.bias").data, false, c0, 0); P.prec_override = -1; }
  }
  return P.err;
}

}  // namespace ns2vc
