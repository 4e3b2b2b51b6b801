// Model weight intake: the strict state-dict contract, BN folding, repacking and the uploads (see model.h).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <set>

#include "arch.h"
#include "gemm.h"
#include "model.h"

namespace roma {

int Model::set_tensor(const char* name, int ndim, const int64_t* shape, const void* data, int is_int64) {
  ROMA_REQUIRE(!finalized,"roma_set_tensor: model already finalized");
  ROMA_REQUIRE(name && data && ndim >= 0 && ndim <= 8, "roma_set_tensor: bad arguments");
  HostTensor t;
  t.shape.assign(shape, shape + ndim);
  const long n = t.numel();
  t.data.resize((size_t)n);
  if (is_int64) {
    const int64_t* s = static_cast<const int64_t*>(data);
    for (long i = 0; i < n; ++i) t.data[(size_t)i] = (float)s[i];
  } else {
    memcpy(t.data.data(), data, (size_t)n * sizeof(float));
  }
  host[name] = std::move(t);
  return 0;
}

// ---------------------------------------------------------------- strict state-dict contract
static void expect(std::vector<std::pair<std::string, std::vector<int64_t>>>& v, const std::string& k,
                   std::vector<int64_t> s) {
  v.emplace_back(k, std::move(s));
}
static void expect_bn(std::vector<std::pair<std::string, std::vector<int64_t>>>& v, const std::string& p, int c) {
  expect(v, p + ".weight", {c});
  expect(v, p + ".bias", {c});
  expect(v, p + ".running_mean", {c});
  expect(v, p + ".running_var", {c});
  expect(v, p + ".num_batches_tracked", {});
}

int Model::check_contract() {
  std::vector<std::pair<std::string, std::vector<int64_t>>> e;
  int cin = 3;
  for (int i = 0; i < 12; ++i) {
    const std::string p = "encoder.cnn.layers." + std::to_string(VGG_IDX[i]);
    expect(e, p + ".weight", {VGG_CH[i], cin, 3, 3});
    expect(e, p + ".bias", {VGG_CH[i]});
    expect_bn(e, "encoder.cnn.layers." + std::to_string(VGG_IDX[i] + 1), VGG_CH[i]);
    cin = VGG_CH[i];
  }
  auto vit = [&](const std::string& p, bool qkv_bias, bool ls) {
    expect(e, p + ".norm1.weight", {1024});
    expect(e, p + ".norm1.bias", {1024});
    expect(e, p + ".attn.qkv.weight", {3072, 1024});
    if (qkv_bias) expect(e, p + ".attn.qkv.bias", {3072});
    expect(e, p + ".attn.proj.weight", {1024, 1024});
    expect(e, p + ".attn.proj.bias", {1024});
    if (ls) expect(e, p + ".ls1.gamma", {1024});
    expect(e, p + ".norm2.weight", {1024});
    expect(e, p + ".norm2.bias", {1024});
    expect(e, p + ".mlp.fc1.weight", {4096, 1024});
    expect(e, p + ".mlp.fc1.bias", {4096});
    expect(e, p + ".mlp.fc2.weight", {1024, 4096});
    expect(e, p + ".mlp.fc2.bias", {1024});
    if (ls) expect(e, p + ".ls2.gamma", {1024});
  };
  for (int i = 0; i < 5; ++i) vit("decoder.embedding_decoder.blocks." + std::to_string(i), false, false);
  expect(e, "decoder.embedding_decoder.to_out.weight", {4097, 1024});
  expect(e, "decoder.embedding_decoder.to_out.bias", {4097});
  expect(e, "decoder.gps.16.pos_conv.weight", {512, 2, 1, 1});
  expect(e, "decoder.gps.16.pos_conv.bias", {512});
  for (int s = 0; s < 5; ++s) {
    const std::string p = std::string("decoder.proj.") + SCALES[s];
    expect(e, p + ".0.weight", {PROJ_COUT[s], PROJ_CIN[s], 1, 1});
    expect(e, p + ".0.bias", {PROJ_COUT[s]});
    expect_bn(e, p + ".1", PROJ_COUT[s]);
  }
  for (int s = 0; s < 5; ++s) {
    const int K = REF_RAD[s] ? (2 * REF_RAD[s] + 1) * (2 * REF_RAD[s] + 1) : 0;
    const int C = 2 * PROJ_COUT[s] + REF_EMB[s] + K;
    const std::string p = std::string("decoder.conv_refiner.") + SCALES[s];
    for (int b = 0; b < 9; ++b) {
      const std::string bp = b == 0 ? p + ".block1" : p + ".hidden_blocks." + std::to_string(b - 1);
      expect(e, bp + ".0.weight", {C, 1, 5, 5});
      expect(e, bp + ".0.bias", {C});
      expect_bn(e, bp + ".1", C);
      expect(e, bp + ".3.weight", {C, C, 1, 1});
      expect(e, bp + ".3.bias", {C});
    }
    expect(e, p + ".out_conv.weight", {3, C, 1, 1});
    expect(e, p + ".out_conv.bias", {3});
    expect(e, p + ".disp_emb.weight", {REF_EMB[s], 2, 1, 1});
    expect(e, p + ".disp_emb.bias", {REF_EMB[s]});
  }
  // DINOv2 dict under the "dinov2." prefix
  expect(e, "dinov2.cls_token", {1, 1, 1024});
  expect(e, "dinov2.pos_embed", {1, 1370, 1024});
  expect(e, "dinov2.mask_token", {1, 1024});
  expect(e, "dinov2.patch_embed.proj.weight", {1024, 3, 14, 14});
  expect(e, "dinov2.patch_embed.proj.bias", {1024});
  for (int i = 0; i < 24; ++i) vit("dinov2.blocks." + std::to_string(i), true, true);
  expect(e, "dinov2.norm.weight", {1024});
  expect(e, "dinov2.norm.bias", {1024});

  std::set<std::string> seen;
  for (auto& kv : e) {
    auto it = host.find(kv.first);
    if (it == host.end()) {
      set_error("roma_finalize: missing key in state_dict: " + kv.first);
      return ROMA_ERR_STATE;
    }
    if (it->second.shape != kv.second) {
      set_error("roma_finalize: size mismatch for " + kv.first);
      return ROMA_ERR_STATE;
    }
    seen.insert(kv.first);
  }
  for (auto& kv : host)
    if (!seen.count(kv.first)) {
      set_error("roma_finalize: unexpected key in state_dict: " + kv.first);
      return ROMA_ERR_STATE;
    }
  return 0;
}

// ---------------------------------------------------------------- uploads
template <typename F>
int Model::upload_f32(const std::vector<float>& v, F** out) {
  void* p = nullptr;
  ROMA_CHECK_HIP(hipMalloc(&p, std::max<size_t>(v.size(), 4) * sizeof(float)));
  owned.push_back(p);
  ROMA_CHECK_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  *out = static_cast<F*>(p);
  return 0;
}

int Model::upload_act(const std::vector<float>& v, void** out) {
  if (act_dt == DT_F32) {
    float* p = nullptr;
    if (int rc = upload_f32(v, &p)) return rc;
    *out = p;
    return 0;
  }
  std::vector<bf16_t> h(v.size());
  if (pack_as_bf16) {
    for (size_t i = 0; i < v.size(); ++i) h[i] = f32_to_bfloat16_bits(v[i]);  // ROMA_MIXED: the DINOv2 weights of the bf16 library
  } else {
    for (size_t i = 0; i < v.size(); ++i) h[i] = f32_to_bf16(v[i]);
  }
  void* p = nullptr;
  ROMA_CHECK_HIP(hipMalloc(&p, std::max<size_t>(h.size(), 8) * sizeof(bf16_t)));
  owned.push_back(p);
  ROMA_CHECK_HIP(hipMemcpy(p, h.data(), h.size() * sizeof(bf16_t), hipMemcpyHostToDevice));
  *out = p;
  return 0;
}

// w: [N][K] row-major; pads K to a multiple of 8
int Model::make_lin(const std::vector<float>& w, const std::vector<float>* b, int N, int K, Lin* out) {
  const int ldw = (int)round_up(K, 8);
  std::vector<float> wp((size_t)N * ldw, 0.f);
  for (int n = 0; n < N; ++n) memcpy(&wp[(size_t)n * ldw], &w[(size_t)n * K], (size_t)K * sizeof(float));
  out->N = N;
  out->K = ldw;
  out->ldw = ldw;
  if (int rc = upload_act(wp, &out->w)) return rc;
  out->b = nullptr;
  if (b)
    if (int rc = upload_f32(*b, &out->b)) return rc;
  return 0;
}

static void bn_fold(const std::map<std::string, HostTensor>& h, const std::string& p, std::vector<float>& s,
                    std::vector<float>& t) {
  const auto& g = h.at(p + ".weight").data;
  const auto& be = h.at(p + ".bias").data;
  const auto& mu = h.at(p + ".running_mean").data;
  const auto& var = h.at(p + ".running_var").data;
  s.resize(g.size());
  t.resize(g.size());
  for (size_t i = 0; i < g.size(); ++i) {
    s[i] = g[i] / sqrtf(var[i] + 1e-5f);
    t[i] = be[i] - mu[i] * s[i];
  }
}

static inline float cubic1(float x) { const float A = -0.75f; return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
static inline float cubic2(float x) { const float A = -0.75f; return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }

// DINOv2 interpolate_pos_encoding (romatch/models/transformer/dinov2.py:166-190): bicubic, A=-0.75, with the
// scale_factor=(h0+0.1)/37 quirk (coordinates map with 37/(h0+0.1), not 37/h0).
static std::vector<float> resize_pos_embed(const std::vector<float>& pos, int th, int tw) {
  const int M = 37, D = 1024;
  std::vector<float> out((size_t)(1 + th * tw) * D);
  memcpy(out.data(), pos.data(), D * sizeof(float));
  if (th == M && tw == M) {
    memcpy(out.data(), pos.data(), out.size() * sizeof(float));
    return out;
  }
  const float sh = (float)(1.0 / ((th + 0.1) / 37.0)), sw = (float)(1.0 / ((tw + 0.1) / 37.0));
  std::vector<int> iy(th * 4), ix(tw * 4);
  std::vector<float> wy(th * 4), wx(tw * 4);
  auto prep = [&](int n, float scale, std::vector<int>& idx, std::vector<float>& wgt) {
    for (int o = 0; o < n; ++o) {
      const float src = scale * ((float)o + 0.5f) - 0.5f;
      const float fl = floorf(src);
      float t = src - fl;
      t = std::min(std::max(t, 0.f), 1.f);
      const int i0 = (int)fl;
      const float c[4] = {cubic2(t + 1.f), cubic1(t), cubic1(1.f - t), cubic2(2.f - t)};
      for (int j = 0; j < 4; ++j) {
        idx[o * 4 + j] = std::max(std::min(i0 - 1 + j, M - 1), 0);
        wgt[o * 4 + j] = c[j];
      }
    }
  };
  prep(th, sh, iy, wy);
  prep(tw, sw, ix, wx);
  const float* pp = pos.data() + D;  // patch part [37*37][D]
  for (int y = 0; y < th; ++y)
    for (int x = 0; x < tw; ++x) {
      float* o = &out[(size_t)(1 + y * tw + x) * D];
      for (int d = 0; d < D; ++d) o[d] = 0.f;
      for (int a = 0; a < 4; ++a) {
        for (int b = 0; b < 4; ++b) {
          const float w = wy[y * 4 + a] * wx[x * 4 + b];
          const float* src = pp + (size_t)(iy[y * 4 + a] * M + ix[x * 4 + b]) * D;
          for (int d = 0; d < D; ++d) o[d] += w * src[d];
        }
      }
    }
  return out;
}

int Model::pack_weights() {
  auto H = [&](const std::string& k) -> const std::vector<float>& { return host.at(k).data; };
  // ---- VGG19-BN: fold BN, repack to [cout][(ky*3+kx)*cin + ci]
  int cin = 3;
  for (int i = 0; i < 12; ++i) {
    const int cout = VGG_CH[i];
    const std::string p = "encoder.cnn.layers." + std::to_string(VGG_IDX[i]);
    std::vector<float> s, t;
    bn_fold(host, "encoder.cnn.layers." + std::to_string(VGG_IDX[i] + 1), s, t);
    const auto& w = H(p + ".weight");
    const auto& b = H(p + ".bias");
    std::vector<float> bf(cout);
    for (int o = 0; o < cout; ++o) bf[o] = b[o] * s[o] + t[o];
    if (i == 0) {
      // MFMA form of the first layer: [64][32] with k = ci*9 + ky*3 + kx (27 real taps, zero padded to 32)
      std::vector<float> wg(64 * 27);
      for (int o = 0; o < 64; ++o)
        for (int k = 0; k < 27; ++k) wg[o * 27 + k] = w[o * 27 + k] * s[o];
      if (int rc = make_lin(wg, &bf, 64, 27, &vgg[0])) return rc;
    } else {
      std::vector<float> wp((size_t)cout * 9 * cin);
      vgg_korder[i] = (vgg_slab_major && act_dt != DT_F32 && cout >= 256 && cin % 64 == 0) ? 1 : 0;
      for (int o = 0; o < cout; ++o)
        for (int ci = 0; ci < cin; ++ci)
          for (int k = 0; k < 9; ++k) {
            const size_t kk = vgg_korder[i] ? ((size_t)(ci / 64) * 9 + k) * 64 + ci % 64 : (size_t)k * cin + ci;
            wp[(size_t)o * 9 * cin + kk] = w[((size_t)o * cin + ci) * 9 + k] * s[o];
          }
      if (int rc = make_lin(wp, &bf, cout, 9 * cin, &vgg[i])) return rc;
    }
    vgg_cin[i] = cin;
    vgg_cout[i] = cout;
    cin = cout;
  }
  // ---- ViT blocks
  auto pack_vit = [&](const std::string& p, bool qkv_bias, bool ls, VitBlockW& o) -> int {
    if (int rc = upload_f32(H(p + ".norm1.weight"), &o.ln1w)) return rc;
    if (int rc = upload_f32(H(p + ".norm1.bias"), &o.ln1b)) return rc;
    if (int rc = upload_f32(H(p + ".norm2.weight"), &o.ln2w)) return rc;
    if (int rc = upload_f32(H(p + ".norm2.bias"), &o.ln2b)) return rc;
    if (int rc = make_lin(H(p + ".attn.qkv.weight"), qkv_bias ? &H(p + ".attn.qkv.bias") : nullptr, 3072, 1024, &o.qkv)) return rc;
    if (int rc = make_lin(H(p + ".mlp.fc1.weight"), &H(p + ".mlp.fc1.bias"), 4096, 1024, &o.fc1)) return rc;
    if (ls && act_dt == DT_BF16) {
      // LayerScale (layers/layer_scale.py:27-28) folded into the branch's last linear: x += g * (W a + b) = (g W) a + g b.
      // In the throughput mode the product g W is rounded to bf16 once at pack time instead of the branch output being
      // scaled in f32 before its bf16 rounding - the same 2^-9 class of rounding - and the GEMM epilogue needs no
      // per-column scale vector (32 registers it does not have next to 128 accumulators).  The exact-f32 mode keeps the
      // reference's order of operations.
      auto fold = [&](const std::vector<float>& w, const std::vector<float>& b, const std::vector<float>& g, int N, int K,
                      Lin* out) -> int {
        std::vector<float> wf(w), bf(b);
        for (int n = 0; n < N; ++n) {
          for (int k = 0; k < K; ++k) wf[(size_t)n * K + k] *= g[n];
          bf[n] *= g[n];
        }
        return make_lin(wf, &bf, N, K, out);
      };
      if (int rc = fold(H(p + ".attn.proj.weight"), H(p + ".attn.proj.bias"), H(p + ".ls1.gamma"), 1024, 1024, &o.proj)) return rc;
      if (int rc = fold(H(p + ".mlp.fc2.weight"), H(p + ".mlp.fc2.bias"), H(p + ".ls2.gamma"), 1024, 4096, &o.fc2)) return rc;
      return 0;
    }
    if (ls) {
      if (int rc = upload_f32(H(p + ".ls1.gamma"), &o.ls1)) return rc;
      if (int rc = upload_f32(H(p + ".ls2.gamma"), &o.ls2)) return rc;
    }
    if (int rc = make_lin(H(p + ".attn.proj.weight"), &H(p + ".attn.proj.bias"), 1024, 1024, &o.proj)) return rc;
    if (int rc = make_lin(H(p + ".mlp.fc2.weight"), &H(p + ".mlp.fc2.bias"), 1024, 4096, &o.fc2)) return rc;
    return 0;
  };
  pack_as_bf16 = mixed;  // ROMA_MIXED: DINOv2's GEMM operands are bfloat16 (it runs in the bf16 library)
  for (int i = 0; i < 24; ++i)
    if (int rc = pack_vit("dinov2.blocks." + std::to_string(i), true, true, dino[i])) return rc;
  if (int rc = make_lin(H("dinov2.patch_embed.proj.weight"), &H("dinov2.patch_embed.proj.bias"), 1024, 588, &patch)) return rc;
  pack_as_bf16 = false;
  for (int i = 0; i < 5; ++i)
    if (int rc = pack_vit("decoder.embedding_decoder.blocks." + std::to_string(i), false, false, tdec[i])) return rc;
  {
    std::vector<float> cls(H("dinov2.cls_token"));
    if (int rc = upload_f32(cls, &cls_tok)) return rc;
    std::vector<float> pe = resize_pos_embed(H("dinov2.pos_embed"), cfg.coarse_h / 14, cfg.coarse_w / 14);
    if (int rc = upload_f32(pe, &pos_emb)) return rc;
  }
  if (int rc = upload_f32(H("dinov2.norm.weight"), &dino_nw)) return rc;
  if (int rc = upload_f32(H("dinov2.norm.bias"), &dino_nb)) return rc;
  {
    // 4097 = 64 * 64 anchors + 1 is not a multiple of 4, which keeps the f32 row writers of the 8-phase kernels away (the launch
    // fell to the classic 128 x 128 kernel: 4 launches of 183 us per step at 0.4 PFLOP/s).  Three zero rows (weights and bias)
    // make it 4100: logits columns 4097 .. 4099 come out 0 and nobody reads them (ldl = 4104 below; cls_to_flow takes 4097).
    const auto& w0 = H("decoder.embedding_decoder.to_out.weight");
    const auto& b0 = H("decoder.embedding_decoder.to_out.bias");
    std::vector<float> wpad((size_t)4100 * 1024, 0.f), bpad(4100, 0.f);
    memcpy(wpad.data(), w0.data(), (size_t)4097 * 1024 * sizeof(float));
    memcpy(bpad.data(), b0.data(), (size_t)4097 * sizeof(float));
    if (int rc = make_lin(wpad, &bpad, 4100, 1024, &to_out)) return rc;
  }
  if (int rc = upload_f32(H("decoder.gps.16.pos_conv.weight"), &gp_w)) return rc;
  if (int rc = upload_f32(H("decoder.gps.16.pos_conv.bias"), &gp_b)) return rc;
  // ---- proj heads (conv1x1 + BN folded)
  for (int s = 0; s < 5; ++s) {
    const std::string p = std::string("decoder.proj.") + SCALES[s];
    std::vector<float> sc, sh;
    bn_fold(host, p + ".1", sc, sh);
    const int co = PROJ_COUT[s], ci = PROJ_CIN[s];
    std::vector<float> w(H(p + ".0.weight")), b(co);
    for (int o = 0; o < co; ++o) {
      for (int c = 0; c < ci; ++c) w[(size_t)o * ci + c] *= sc[o];
      b[o] = H(p + ".0.bias")[o] * sc[o] + sh[o];
    }
    if (int rc = make_lin(w, &b, co, ci, &proj[s])) return rc;
  }
  // ---- ConvRefiners
  for (int s = 0; s < 5; ++s) {
    RefinerW& r = ref[s];
    r.Cf = PROJ_COUT[s];
    r.E = REF_EMB[s];
    r.radius = REF_RAD[s];
    r.K = r.radius ? (2 * r.radius + 1) * (2 * r.radius + 1) : 0;
    r.C = 2 * r.Cf + r.E + r.K;
    // channel padding: whole 128-byte rows for the wide (MFMA-bound) refiners so every GEMM slab row is one aligned
    // cache line; 16-byte granularity for the narrow HBM-bound ones (144, 24 channels)
    r.Cp = (int)(r.C >= 256 ? round_up(r.C, 64) : round_up(r.C, 8));
    const std::string p = std::string("decoder.conv_refiner.") + SCALES[s];
    if (int rc = upload_f32(H(p + ".disp_emb.weight"), &r.emb_w)) return rc;
    if (int rc = upload_f32(H(p + ".disp_emb.bias"), &r.emb_b)) return rc;
    for (int b = 0; b < 9; ++b) {
      const std::string bp = b == 0 ? p + ".block1" : p + ".hidden_blocks." + std::to_string(b - 1);
      std::vector<float> sc, sh;
      bn_fold(host, bp + ".1", sc, sh);
      const auto& w = H(bp + ".0.weight");
      const auto& bb = H(bp + ".0.bias");
      std::vector<float> dw((size_t)25 * r.Cp, 0.f), db((size_t)r.Cp, 0.f);
      for (int c = 0; c < r.C; ++c) {
        for (int t = 0; t < 25; ++t) dw[(size_t)t * r.Cp + c] = w[(size_t)c * 25 + t] * sc[c];
        db[c] = bb[c] * sc[c] + sh[c];
      }
      if (int rc = upload_f32(dw, &r.dw_w[b])) return rc;
      if (int rc = upload_f32(db, &r.dw_b[b])) return rc;
      const auto& pw = H(bp + ".3.weight");
      std::vector<float> pwp((size_t)r.Cp * r.Cp, 0.f), pb((size_t)r.Cp, 0.f);
      for (int o = 0; o < r.C; ++o) {
        memcpy(&pwp[(size_t)o * r.Cp], &pw[(size_t)o * r.C], (size_t)r.C * sizeof(float));
        pb[o] = H(bp + ".3.bias")[o];
      }
      if (int rc = make_lin(pwp, &pb, r.Cp, r.Cp, &r.pw[b])) return rc;
    }
    std::vector<float> ow((size_t)3 * r.Cp, 0.f);
    for (int o = 0; o < 3; ++o)
      memcpy(&ow[(size_t)o * r.Cp], &H(p + ".out_conv.weight")[(size_t)o * r.C], (size_t)r.C * sizeof(float));
    if (int rc = upload_f32(ow, &r.out_w)) return rc;
    if (int rc = upload_f32(H(p + ".out_conv.bias"), &r.out_b)) return rc;
    {  // out_conv o (last block's 1x1): d -> out_w (pw8 d + b8) + out_b = (out_w pw8) d + (out_w b8 + out_b), accumulated in f64.
      // pw8 enters as the kernels would see it (rounded to the 16-bit storage format in those modes, like autocast's weight cast)
      const std::string bp = p + ".hidden_blocks.7";
      const auto& pw8 = H(bp + ".3.weight");
      const auto& pb8 = H(bp + ".3.bias");
      const auto& ob = H(p + ".out_conv.bias");
      std::vector<float> cw((size_t)3 * r.Cp, 0.f), cb(4, 0.f);
      for (int o = 0; o < 3; ++o) {
        for (int k = 0; k < r.C; ++k) {
          double acc = 0.0;
          for (int n = 0; n < r.C; ++n) {
            float wv = pw8[(size_t)n * r.C + k];
            if (act_dt != DT_F32) wv = bf16_to_f32(f32_to_bf16(wv));
            acc += (double)ow[(size_t)o * r.Cp + n] * (double)wv;
          }
          cw[(size_t)o * r.Cp + k] = (float)acc;
        }
        double accb = (double)ob[o];
        for (int n = 0; n < r.C; ++n) accb += (double)ow[(size_t)o * r.Cp + n] * (double)pb8[n];
        cb[o] = (float)accb;
      }
      if (int rc = upload_f32(cw, &r.oc_w)) return rc;
      if (int rc = upload_f32(cb, &r.oc_b)) return rc;
      if (act_dt != DT_F32) {  // head + remainder split for the MFMA of the FINAL fused blocks
        std::vector<float> hl((size_t)8 * r.Cp, 0.f), fb((size_t)r.Cp, 0.f);
        for (int o = 0; o < 3; ++o) {
          for (int k = 0; k < r.Cp; ++k) {
            const float wv = cw[(size_t)o * r.Cp + k];
            const float hi = bf16_to_f32(f32_to_bf16(wv));
            hl[(size_t)o * r.Cp + k] = hi;
            hl[(size_t)(4 + o) * r.Cp + k] = wv - hi;  // (rounded to 16 bits by upload_act)
          }
          fb[o] = cb[o];
        }
        if (int rc = upload_act(hl, &r.ocf_w)) return rc;
        if (int rc = upload_f32(fb, &r.ocf_b)) return rc;
      }
    }
  }
  return 0;
}
}  // namespace roma
