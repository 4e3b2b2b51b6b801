// extern "C" boundary of libroma_hip (declarations + reference citations: include/roma_hip.h)
#include <algorithm>
#include <mutex>
#include <map>
#include <vector>
#include <dlfcn.h>
#include <string.h>

#include "../../include/roma_hip.h"
#include "attention.h"
#include "conv64.h"
#include "conv_patch.h"
#include "elementwise.h"
#include "gemm.h"
#include "local_corr.h"
#include "pool_proj.h"
#include "gp.h"
#include "model.h"
#include "refiner_block.h"
#include "kde.h"
#include "keypoints.h"
#include "keypoints_batched.h"
#include "tiny.h"
#include "tuning.h"
#include "vit.h"
#include "sampling.h"
#include "sample_batched.h"
#include "absolute_pose.h"
#include "bundle.h"
#include "essential.h"
#include "model_refine.h"
#include "pose_refine.h"
#include "geometry.h"
#include "triangulate.h"
#include "depth_fusion.h"
#include "point_render.h"
#include "tracks.h"
#include "set_keypoints.h"
#include "gt_warp.h"
#include "metrics.h"
#include "morph.h"
#include "preprocess.h"

namespace roma {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace roma

namespace roma {
struct ProfRec { std::string name, unit; double work; hipEvent_t e0, e1; };
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
bool prof_enabled() { return g_prof_on; }
void prof_begin(const char* kernel, double work, const char* unit, hipStream_t s) {
  ProfRec r;
  r.name = kernel; r.unit = unit; r.work = work;
  (void)hipEventCreate(&r.e0);
  (void)hipEventCreate(&r.e1);
  (void)hipEventRecord(r.e0, s);
  g_prof.push_back(r);
}
void prof_end(hipStream_t s) { (void)hipEventRecord(g_prof.back().e1, s); }
}  // namespace roma

struct roma_model {
  roma::Model m;
};

namespace roma {
// ROMA_MIXED: the sibling bfloat16 library (once a mixed handle has loaded it) keeps its own switches and its own launch
// profile; tuning calls and the profile of THIS library are forwarded / merged so that callers see one library.
void* g_peer_lib = nullptr;  // set by Model::load_peer (model.hip)
int g_mixed_handles = 0;      // live ROMA_MIXED handles (model.hip): the sibling follows roma_tuning / roma_profile_* only while > 0
template <typename F> static F peer_sym(const char* name) {
  return g_peer_lib ? reinterpret_cast<F>(dlsym(g_peer_lib, name)) : nullptr;
}
}  // namespace roma

using namespace roma;

static inline hipStream_t S(void* s) { return static_cast<hipStream_t>(s); }
// public dtype code -> internal one.  The 16-bit storage format is a property of the BUILD (common.h): this library accepts
// ROMA_F32 and its own 16-bit code only; the other one fails loudly instead of reinterpreting the bits.
#ifdef ROMA_H16_F16
static constexpr int ROMA_H16_CODE = ROMA_F16, ROMA_OTHER16_CODE = ROMA_BF16;
#else
static constexpr int ROMA_H16_CODE = ROMA_BF16, ROMA_OTHER16_CODE = ROMA_F16;
#endif
static inline int dt_code(int dt) {
  if (dt == ROMA_F32) return DT_F32;
  if (dt == ROMA_H16_CODE) return DT_BF16;
  set_error(dt == ROMA_OTHER16_CODE
                ? std::string("this library stores ") + ROMA_H16_NAME + ": load " +
                      (ROMA_H16_CODE == ROMA_BF16 ? "libroma_hip_f16.so for ROMA_F16" : "libroma_hip.so for ROMA_BF16")
                : std::string("bad dtype code"));
  return -1;
}
#define DT(dt)                           \
  ({                                     \
    const int _d = dt_code(dt);          \
    if (_d < 0) return ROMA_ERR_ARG;     \
    _d;                                  \
  })

extern "C" {

const char* roma_last_error(void) { return g_err.c_str(); }
const char* roma_version(void) { return "roma_hip 0.3 (gfx950, 16-bit storage = " ROMA_H16_NAME ")"; }
int roma_h16_format(void) { return ROMA_H16_CODE; }
int roma_abi_stamp(void) { return ROMA_ABI_VERSION * 100000 + (int)sizeof(roma_vit_args_t); }
// roma::internal_h16_code lives in ANOTHER translation unit (vit.hip) on purpose: a call inside one TU binds locally under
// clang's default -fno-semantic-interposition, a cross-TU call goes through the PLT unless the library is linked -Bsymbolic
int roma_self_check(void) { return roma::internal_h16_code(); }

int roma_create(const roma_config_t* cfg, roma_handle_t* out) {
  ROMA_REQUIRE(cfg && out, "roma_create: null argument");
  ROMA_REQUIRE(cfg->coarse_h > 0 && cfg->coarse_w > 0 && cfg->coarse_h % 14 == 0 && cfg->coarse_w % 14 == 0,
               "Needs to be multiple of 14 for backbone");  // roma_models.py:58-59
  // no multiple-of-8 requirement (the reference has none either, e.g. 518 / 574 / 602): the VGG pyramid takes the
  // floor-divided sizes of its 2x2 max-pools and every decoder resize goes to those sizes (model.hip)
  ROMA_REQUIRE(cfg->coarse_h >= 16 && cfg->coarse_w >= 16, "roma_create: coarse resolution too small for the stride-16 pyramid");
  ROMA_REQUIRE(cfg->upsample_h >= 0 && cfg->upsample_w >= 0 && (cfg->upsample_h == 0 || (cfg->upsample_h >= 16 && cfg->upsample_w >= 16)),
               "roma_create: bad upsample resolution");
  ROMA_REQUIRE(cfg->max_batch >= 1, "roma_create: max_batch must be >= 1");
  if (cfg->precision == ROMA_MIXED) {  // bf16 DINOv2 (sibling library) + binary16 elsewhere: a mode of the binary16 build
    ROMA_REQUIRE(ROMA_H16_CODE == ROMA_F16, "ROMA_MIXED: load libroma_hip_f16.so (it runs DINOv2 through libroma_hip.so)");
  } else if (dt_code(cfg->precision) < 0) {
    return ROMA_ERR_ARG;  // ROMA_F32 or this build's 16-bit format
  }
  int ndev = 0;
  ROMA_CHECK_HIP(hipGetDeviceCount(&ndev));
  ROMA_REQUIRE(cfg->device >= 0 && cfg->device < ndev, "roma_create: no such HIP device (the HIP path has no CPU fallback)");
  roma_model* h = new roma_model();
  h->m.cfg = *cfg;
  *out = h;
  return 0;
}

int roma_set_tensor(roma_handle_t h, const char* name, int ndim, const int64_t* shape, const void* data, int is_int64) {
  ROMA_REQUIRE(h, "roma_set_tensor: null handle");
  return h->m.set_tensor(name, ndim, shape, data, is_int64);
}

int roma_finalize(roma_handle_t h) {
  ROMA_REQUIRE(h, "roma_finalize: null handle");
  return h->m.finalize();
}

int roma_set_option(roma_handle_t h, const char* key, int value) {
  ROMA_REQUIRE(h && key, "roma_set_option: null argument");
  const std::string k(key);
  if (k == "symmetric") h->m.cfg.symmetric = value ? 1 : 0;
  else if (k == "upsample_preds") {
    ROMA_REQUIRE(!value || h->m.cfg.upsample_h > 0, "roma_set_option: handle was created without an upsample resolution");
    h->m.cfg.upsample_preds = value ? 1 : 0;
  } else if (k == "attenuate_cert") h->m.cfg.attenuate_cert = value ? 1 : 0;
  else if (k == "debug") h->m.debug = value != 0;
  else if (k == "fuse_refiner_blocks") h->m.fuse_refiner_blocks = value != 0;
  else if (k == "compose_out_conv") h->m.compose_out_conv = value != 0;
  else if (k == "vit_bf16_residual") h->m.vit_bf16_residual = value != 0;
  else if (k == "dual_stream") h->m.n_streams = value != 0 ? 2 : 1;
  else if (k == "trace") h->m.trace_on = value != 0;
  else if (k == "streams") {
    ROMA_REQUIRE(value >= 1 && value <= Model::MAX_STREAMS, "roma_set_option: streams must be 1..4");
    h->m.n_streams = value;
  }
  else {
    set_error("roma_set_option: unknown key " + k);
    return ROMA_ERR_ARG;
  }
  return 0;
}

int roma_set_option_f(roma_handle_t h, const char* key, double value) {
  ROMA_REQUIRE(h && key, "roma_set_option_f: null argument");
  const std::string k(key);
  if (k == "coarse_scale_factor") {
    ROMA_REQUIRE(value >= 0.0, "roma_set_option_f: coarse_scale_factor must be >= 0 (0 = derive from the handle's resolution)");
    h->m.coarse_scale_factor = value;
  } else {
    set_error("roma_set_option_f: unknown key " + k);
    return ROMA_ERR_ARG;
  }
  return 0;
}

int roma_match(roma_handle_t h, int B, const float* im_a, const float* im_b, const float* im_a_hr, const float* im_b_hr,
               float* warp_out, float* cert_out, void* stream) {
  ROMA_REQUIRE(h, "roma_match: null handle");
  return h->m.match(B, im_a, im_b, im_a_hr, im_b_hr, warp_out, cert_out, S(stream));
}

long roma_encoded_bytes(roma_handle_t h) {
  if (!h || !h->m.finalized) {
    set_error("roma_encoded_bytes: null handle or roma_finalize not called yet");
    return -1;
  }
  return h->m.pack.total;
}

int roma_encode(roma_handle_t h, int N, const float* images, const float* images_hr, void* feats, long feats_bytes, void* stream) {
  ROMA_REQUIRE(h, "roma_encode: null handle");
  return h->m.encode(N, images, images_hr, feats, feats_bytes, S(stream));
}

int roma_match_encoded(roma_handle_t h, int P, const void* feats, long feats_bytes, int N, const int* idx_a_host,
                       const int* idx_b_host, float* warp_out, float* cert_out, void* stream) {
  ROMA_REQUIRE(h, "roma_match_encoded: null handle");
  return h->m.match_encoded(P, feats, feats_bytes, N, idx_a_host, idx_b_host, warp_out, cert_out, S(stream));
}

int roma_forward(roma_handle_t h, int B, const float* im_a, const float* im_b, const roma_forward_args_t* a, void* stream) {
  ROMA_REQUIRE(h, "roma_forward: null handle");
  return h->m.forward(B, im_a, im_b, a, S(stream));
}

long roma_debug_fetch(roma_handle_t h, const char* name, void* dst_host, long nbytes) {
  if (!h || !name) return ROMA_ERR_ARG;
  auto it = h->m.dbg.find(name);
  if (it == h->m.dbg.end()) {
    set_error(std::string("roma_debug_fetch: no such stage: ") + name);
    return ROMA_ERR_ARG;
  }
  if (!dst_host) return (long)it->second.second;
  if ((size_t)nbytes < it->second.second) {
    set_error("roma_debug_fetch: destination too small");
    return ROMA_ERR_ARG;
  }
  if (hipSetDevice(h->m.cfg.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ROMA_ERR_HIP;
  if (hipMemcpy(dst_host, it->second.first, it->second.second, hipMemcpyDeviceToHost) != hipSuccess) return ROMA_ERR_HIP;
  return (long)it->second.second;
}

int roma_debug_inject(roma_handle_t h, const char* name, const void* src_host, long nbytes) {
  ROMA_REQUIRE(h, "roma_debug_inject: null handle");
  return h->m.debug_inject(name, src_host, nbytes > 0 ? (size_t)nbytes : 0);
}

long roma_debug_trace(roma_handle_t h, int slot, unsigned long long* sums_host, long max_entries, char* names_host,
                      long names_bytes) {
  if (!h || slot < 0 || slot >= Model::MAX_STREAMS_DECL) return ROMA_ERR_ARG;
  const long n = h->m.trace_n[slot];
  if (!sums_host) return n;
  if (max_entries < n || !h->m.trace_dev[slot]) {
    set_error("roma_debug_trace: destination too small or tracing was never enabled");
    return ROMA_ERR_ARG;
  }
  if (hipSetDevice(h->m.cfg.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ROMA_ERR_HIP;
  if (hipMemcpy(sums_host, h->m.trace_dev[slot], (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess)
    return ROMA_ERR_HIP;
  if (names_host && names_bytes > 0) {
    std::string all;
    for (long i = 0; i < n; ++i) all += h->m.trace_names[slot][(size_t)i] + "\n";
    const size_t c = std::min<size_t>(all.size(), (size_t)names_bytes - 1);
    memcpy(names_host, all.data(), c);
    names_host[c] = 0;
  }
  return n;
}

int roma_destroy(roma_handle_t h) {
  delete h;
  return 0;
}

int roma_tuning(const char* key, int value) {
  ROMA_REQUIRE(key, "roma_tuning: null key");
  // ROMA_MIXED handles run DINOv2 in the bfloat16 sibling, so its switches follow - but only while such a handle is alive:
  // the sibling is the same process-wide instance a pure-bf16 matcher uses (roma_amd loads it too), and a tuning call on
  // the binary16 library must not silently retune an unrelated bf16 matcher once the last mixed handle is gone.
  if (g_mixed_handles > 0)
    if (auto f = peer_sym<int (*)(const char*, int)>("roma_tuning"))
      if (int rc = f(key, value)) {
        set_error(std::string("roma_tuning: the bfloat16 sibling library refused key ") + key);
        return rc;
      }
  return tuning_set(key, value);
}

long roma_tuning_describe(char* buf, long nbytes) {
  const std::string js = tuning_describe();
  if (!buf) return (long)js.size() + 1;
  if (nbytes < (long)js.size() + 1) return ROMA_ERR_ARG;
  memcpy(buf, js.c_str(), js.size() + 1);
  return (long)js.size() + 1;
}

int roma_vit_forward(const roma_vit_args_t* a, void* stream) {
  ROMA_REQUIRE(a, "roma_vit_forward: null argument");
  ROMA_REQUIRE(a->act == ROMA_F32 || a->act == ROMA_H16_CODE, "roma_vit_forward: act must be ROMA_F32 or this library's 16-bit code");
  return vit_forward(*a, S(stream));
}

int roma_op_convert_from_bf16(const void* in_bf16, void* out_h16, long n, void* stream) {
  ROMA_REQUIRE(in_bf16 && out_h16, "roma_op_convert_from_bf16: null pointer");
  return convert_from_bf16_launch(in_bf16, out_h16, n, S(stream));
}

long roma_debug_gemm_trace(unsigned int* dst_host, long nbytes) {
  ROMA_REQUIRE(dst_host && nbytes > 0, "roma_debug_gemm_trace: null destination");
  if (hipDeviceSynchronize() != hipSuccess) return ROMA_ERR_HIP;
  const int rc = gemm8p_trace_read(dst_host, nbytes);
  return rc < 0 ? rc : std::min<long>(nbytes, (long)sizeof(unsigned) * 16 * 2 * 256 * 4);
}

int roma_profile_enable(int on) {
  if (g_mixed_handles > 0)  // see roma_tuning
    if (auto f = peer_sym<int (*)(int)>("roma_profile_enable"))
      if (int rc = f(on)) return rc;
  for (auto& r : g_prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  g_prof.clear();
  g_prof_on = on != 0;
  return 0;
}

long roma_profile_report(char* buf, long nbytes) {
  if (hipDeviceSynchronize() != hipSuccess) return ROMA_ERR_HIP;
  struct Agg { long calls = 0; double ms = 0, work = 0; std::string unit; };
  std::map<std::string, Agg> agg;
  for (auto& r : g_prof) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) continue;
    Agg& a = agg[r.name];
    a.calls++; a.ms += ms; a.work += r.work; a.unit = r.unit;
  }
  std::string js = "{";
  bool first = true;
  for (auto& kv : agg) {
    char tmp[512];
    snprintf(tmp, sizeof tmp, "%s\"%s\": {\"calls\": %ld, \"total_ms\": %.6f, \"work\": %.6e, \"unit\": \"%s\"}", first ? "" : ", ",
             kv.first.c_str(), kv.second.calls, kv.second.ms, kv.second.work, kv.second.unit.c_str());
    js += tmp;
    first = false;
  }
  if (auto f = peer_sym<long (*)(char*, long)>("roma_profile_report")) {  // the sibling library's launches (DINOv2 of a mixed handle)
    const long n = f(nullptr, 0);
    if (n > 3) {
      std::string peer((size_t)n, '\0');
      if (f(&peer[0], n) > 0) {
        peer.resize(strlen(peer.c_str()));
        if (peer.size() > 2) js += (first ? "" : ", ") + peer.substr(1, peer.size() - 2);
      }
    }
  }
  js += "}";
  if (!buf) return (long)js.size() + 1;
  if (nbytes < (long)js.size() + 1) return ROMA_ERR_ARG;
  memcpy(buf, js.c_str(), js.size() + 1);
  return (long)js.size() + 1;
}

// ------------------------------------------------------------------------------------ operators
int roma_op_local_corr(const void* feature0, const void* feature1, const float* warp, void* out, int B, int H, int W,
                       int C, int K, int nearest, int dt_in, int dt_out, void* stream) {
  LocalCorrArgs a;
  a.nearest = nearest ? 1 : 0;
  a.f0 = feature0; a.f1 = feature1; a.warp = warp; a.out = out; a.B = B; a.H = H; a.W = W; a.C = C; a.K = K;
  a.ld0 = C; a.ld1 = C; a.ldo = K; a.nimg = B; a.f1_shift = 0; a.scale = 1.f; a.in_dt = DT(dt_in); a.out_dt = DT(dt_out);
  return local_corr_general_launch(a, S(stream));
}

int roma_op_local_corr_window(const void* feature0, const void* feature1, const float* warp, void* out, int B, int H,
                              int W, int C, int radius, float scale, long ldo, int dt_in, int dt_out, void* stream) {
  LocalCorrArgs a;
  a.f0 = feature0; a.f1 = feature1; a.warp = warp; a.out = out; a.B = B; a.H = H; a.W = W; a.C = C; a.radius = radius;
  a.ld0 = C; a.ld1 = C; a.ldo = ldo; a.nimg = B; a.f1_shift = 0; a.scale = scale; a.in_dt = DT(dt_in); a.out_dt = DT(dt_out);
  ROMA_REQUIRE(ldo >= (2 * radius + 1) * (2 * radius + 1), "local_corr_window: ldo < K");
  return local_corr_window_launch(a, S(stream));
}

long roma_op_local_corr_window_workspace(int B, int H, int W, int radius) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return local_corr_ws_ints(B, H, W, radius) * (long)sizeof(int);
}

int roma_op_local_corr_window_ws(const void* feature0, const void* feature1, const float* warp, void* out, int B, int H,
                                 int W, int C, int radius, float scale, long ldo, int dt_in, int dt_out, void* ws,
                                 long ws_bytes, void* stream) {
  LocalCorrArgs a;
  a.f0 = feature0; a.f1 = feature1; a.warp = warp; a.out = out; a.B = B; a.H = H; a.W = W; a.C = C; a.radius = radius;
  a.ld0 = C; a.ld1 = C; a.ldo = ldo; a.nimg = B; a.f1_shift = 0; a.scale = scale; a.in_dt = DT(dt_in); a.out_dt = DT(dt_out);
  a.ws = static_cast<int*>(ws); a.ws_bytes = ws_bytes;
  ROMA_REQUIRE(ldo >= (2 * radius + 1) * (2 * radius + 1), "local_corr_window: ldo < K");
  if (roma_op_local_corr_window_workspace(B, H, W, radius) == 0) {  // a radius that needs no scratch: ws may be NULL
    a.ws = nullptr; a.ws_bytes = 0;
  } else {
    ROMA_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 3) == 0, "local_corr_window_ws: ws must be a 4-byte aligned device pointer");
  }
  return local_corr_window_launch(a, S(stream));
}

int roma_op_gemm(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, int batch,
                 long sA, long sW, long sC, const float* bias, const float* scale, const float* res, long ldr, int act,
                 float alpha, int dt_in, int dt_out, void* stream) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K; g.batch = batch;
  g.sA = sA; g.sW = sW; g.sC = sC; g.bias = bias; g.scale = scale; g.res = res; g.ldr = ldr; g.sR = sC; g.act = act;
  g.alpha = alpha; g.in_dt = DT(dt_in); g.out_dt = DT(dt_out);
  return gemm_launch(g, S(stream));
}

int roma_op_conv3x3(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                    int relu, int dt, void* stream) {
  GemmArgs g;
  g.A = in; g.W = w; g.ldw = 9 * Cin; g.C = out; g.ldc = Cout; g.M = B * H * W; g.N = Cout; g.K = 9 * Cin;
  g.in_dt = DT(dt); g.out_dt = DT(dt); g.bias = bias; g.act = relu ? ACT_RELU : ACT_NONE;
  g.conv_h = H; g.conv_w = W; g.conv_c = Cin;
  return gemm_launch(g, S(stream));
}

int roma_op_conv3x3_slab(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                         int relu, int dt, void* stream) {
  GemmArgs g;
  g.A = in; g.W = w; g.ldw = 9 * Cin; g.C = out; g.ldc = Cout; g.M = B * H * W; g.N = Cout; g.K = 9 * Cin;
  g.in_dt = DT(dt); g.out_dt = DT(dt); g.bias = bias; g.act = relu ? ACT_RELU : ACT_NONE;
  g.conv_h = H; g.conv_w = W; g.conv_c = Cin; g.conv_korder = 1;
  return gemm_launch(g, S(stream));
}

int roma_op_attention(const void* q, const void* k, const void* vt, void* out, int B, int heads, int N, int npad, int hd,
                      int dt_in, int dt_out, void* stream) {
  AttnArgs a;
  a.q = q; a.k = k; a.vt = vt; a.out = out; a.B = B; a.heads = heads; a.N = N; a.npad = npad; a.hd = hd;
  a.ldo = (long)heads * hd; a.in_dt = DT(dt_in); a.out_dt = DT(dt_out);
  return attention_launch(a, S(stream));
}

int roma_op_qkv_scatter_gemm(const void* A, const void* W, const float* bias, void* q, void* k, void* vt, int B, int N,
                             int npad, int heads, int hd, int K, int dt_in, int dt_out, void* stream) {
  GemmArgs g;
  g.A = A; g.lda = K; g.W = W; g.ldw = K; g.M = B * N; g.N = 3 * heads * hd; g.K = K; g.in_dt = DT(dt_in);
  g.out_dt = DT(dt_out); g.bias = bias; g.mode = EPI_QKV; g.q = q; g.k = k; g.vt = vt; g.heads = heads; g.hd = hd;
  g.ntok = N; g.npad = npad; g.qscale = 1.0f / sqrtf((float)hd);
  return gemm_launch(g, S(stream));
}

int roma_op_layernorm(const float* x, const float* w, const float* b, void* out, long M, int D, float eps, int dt_out,
                      void* stream) {
  return layernorm_launch(x, w, b, out, M, D, eps, DT(dt_out), S(stream));
}

int roma_op_layernorm_dt(const void* x, int dt_in, const float* w, const float* b, void* out, long M, int D, float eps,
                         int dt_out, void* stream) {
  return layernorm_launch_dt(x, DT(dt_in), w, b, out, M, D, eps, DT(dt_out), S(stream));
}

int roma_op_gemm_res_bf16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K,
                          const float* bias, const float* scale, const void* res, long ldr, void* stream) {
  GemmArgs g;
  g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
  g.bias = bias; g.scale = scale; g.res_bf16 = res; g.ldr = ldr; g.in_dt = DT_BF16; g.out_dt = DT_BF16;
  return gemm_launch(g, S(stream));
}

int roma_op_cholesky_solve_t(float* A, float* Ft, float* LT, float* Linv, float* LinvT, int n, int d, int batch,
                             void* stream) {
  // Ft == A + n * n with batch > 1 cannot be the dense [batch, n, n] + [batch, d, n] layout (Ft would overlap the second
  // matrix): it is the augmented layout of the GP - one (n + d) x n matrix per item, items (n + d) * n floats apart
  if (batch > 1 && Ft == A + (long)n * n)
    return cholesky_solve_t(A, Ft, LT, Linv, LinvT, n, d, batch, S(stream), (long)(n + d) * n, (long)(n + d) * n);
  return cholesky_solve_t(A, Ft, LT, Linv, LinvT, n, d, batch, S(stream));
}

int roma_op_gp(const void* x, const void* y, const float* pos_w, const float* pos_b, float* mu, int b, int h, int w, int dt,
               void* stream) {
  ROMA_REQUIRE(x && y && pos_w && pos_b && mu && b > 0 && h > 0 && w > 0, "roma_op_gp: bad arguments");
  hipStream_t st = S(stream);
  const int n = h * w;
  const size_t esz = DT(dt) == DT_F32 ? 4 : 2;
  // one feature buffer [2b, n, 512]: images [0, b) = x (queries), [b, 2b) = y (supports); non-symmetric pairing
  Arena plan;
  plan.alloc((size_t)2 * b * n * 512 * esz);
  if (int rc = gp_posterior(nullptr, 512, DT(dt), b, false, h, w, pos_w, pos_b, mu, 512, plan, st, true)) return rc;
  Arena ar;
  ar.cap = plan.peak + 4096;
  ar.dry = false;
  ROMA_CHECK_HIP(hipMallocAsync(reinterpret_cast<void**>(&ar.base), ar.cap, st));
  char* pf = static_cast<char*>(ar.alloc((size_t)2 * b * n * 512 * esz));
  int rc = 0;
  if (hipMemcpyAsync(pf, x, (size_t)b * n * 512 * esz, hipMemcpyDeviceToDevice, st) != hipSuccess ||
      hipMemcpyAsync(pf + (size_t)b * n * 512 * esz, y, (size_t)b * n * 512 * esz, hipMemcpyDeviceToDevice, st) != hipSuccess) {
    set_error("roma_op_gp: device copy failed");
    rc = ROMA_ERR_HIP;
  }
  if (!rc) rc = gp_posterior(pf, 512, DT(dt), b, false, h, w, pos_w, pos_b, mu, 512, ar, st, false);
  (void)hipFreeAsync(ar.base, st);
  return rc;
}

int roma_op_cls_to_flow(const float* logits, long ld, float* flow, float* cert, long M, void* stream) {
  return cls_to_flow_launch(logits, ld, flow, cert, M, S(stream));
}

int roma_op_resize_bilinear(const float* in, float* out, int B, int Hin, int Win, int Hout, int Wout, int nc,
                            void* stream) {
  return resize_bilinear_launch(in, out, B, Hin, Win, Hout, Wout, nc, S(stream));
}

int roma_op_refiner_input(const void* feat, long ldf, const float* flow, void* d, long ldd, const float* emb_w,
                          const float* emb_b, int B, int H, int W, int C, int E, int Kcorr, int nimg, int shift,
                          float disp_scale, int dt, void* stream) {
  RefinerInputArgs a;
  a.feat = feat; a.ldf = ldf; a.flow = flow; a.d = d; a.ldd = ldd; a.emb_w = emb_w; a.emb_b = emb_b;
  a.B = B; a.H = H; a.W = W; a.C = C; a.E = E; a.Kcorr = Kcorr; a.nimg = nimg; a.shift = shift;
  a.disp_scale = disp_scale; a.dt = DT(dt);
  ROMA_REQUIRE(feat && flow && d && B > 0 && H > 0 && W > 0 && C > 0 && nimg > 0, "roma_op_refiner_input: bad arguments");
  ROMA_REQUIRE(ldd >= 2 * C + E + Kcorr && ldf >= C, "roma_op_refiner_input: row strides too small");
  return refiner_input_launch(a, S(stream));
}

int roma_op_dwconv5x5(const void* in, void* out, const float* w, const float* bias, int B, int H, int W, int Cp, int dt,
                      void* stream) {
  return dwconv5x5_launch(in, out, w, bias, B, H, W, Cp, DT(dt), S(stream));
}

int roma_op_refiner_block(const void* in, void* out, const float* dw_w, const float* dw_b, const void* pw,
                          const float* pw_b, int B, int H, int W, int Cp, int dt, void* stream) {
  return refiner_block_launch(in, out, dw_w, dw_b, pw, Cp, pw_b, B, H, W, Cp, DT(dt), S(stream));
}

int roma_op_refiner_block_final(const void* in, float* delta, const float* dw_w, const float* dw_b, const void* pw_final,
                                const float* bias_final, int B, int H, int W, int Cp, int dt, void* stream) {
  ROMA_REQUIRE(in && delta && dw_w && dw_b && pw_final && bias_final, "roma_op_refiner_block_final: null pointer");
  return refiner_block_final_launch(in, delta, dw_w, dw_b, pw_final, Cp, bias_final, B, H, W, Cp, DT(dt), S(stream));
}

int roma_op_refiner_apply_delta(const float* delta, float* flow, float* cert, long M, float sx, float sy, void* stream) {
  ROMA_REQUIRE(delta && flow && cert && M >= 0, "roma_op_refiner_apply_delta: null pointer");
  return refiner_apply_delta_launch(delta, flow, cert, M, sx, sy, S(stream));
}

int roma_op_kde(const float* x, long n, int down, float std, int half_inputs, float* density, void* stream) {
  return kde_launch(x, n, down, std, half_inputs, density, S(stream));
}

int roma_op_sample_warp_at(const float* warp, const float* cert, int H, int W, const float* xa, long n, float* xa_to_b,
                           float* cert_a, void* stream) {
  return sample_warp_at_launch(warp, cert, H, W, xa, n, xa_to_b, cert_a, S(stream));
}

int roma_op_mutual_nn(const float* a, long na, const float* b, long nb, const float* cert_a, float cert_th, float max_dist,
                      int* match_b, void* ws_a, void* ws_b, void* stream) {
  return mutual_nn_launch(a, na, b, nb, cert_a, cert_th, max_dist, match_b, static_cast<unsigned long long*>(ws_a),
                          static_cast<unsigned long long*>(ws_b), S(stream));
}

int roma_op_mutual_nn_count(const float* a, long na, const float* b, long nb, const float* cert_a, float cert_th, float max_dist,
                            void* ws_a, void* ws_b, long long* offsets, void* stream) {
  return mutual_nn_count_launch(a, na, b, nb, cert_a, cert_th, max_dist, static_cast<unsigned long long*>(ws_a),
                                static_cast<unsigned long long*>(ws_b), offsets, S(stream));
}
int roma_op_mutual_nn_fill(const float* a, long na, const float* b, long nb, const float* cert_a, float cert_th, float max_dist,
                           const void* ws_a, const void* ws_b, long long* offsets, long long* pairs, void* stream) {
  return mutual_nn_fill_launch(a, na, b, nb, cert_a, cert_th, max_dist, static_cast<const unsigned long long*>(ws_a),
                               static_cast<const unsigned long long*>(ws_b), offsets, pairs, S(stream));
}

long roma_op_multinomial_workspace(long n, long k) { return (long)multinomial_workspace_bytes(n, k); }
int roma_op_multinomial(const float* weights, long n, long k, unsigned long long seed, long long* out_indices, void* workspace,
                        long workspace_bytes, void* stream) {
  return multinomial_launch(weights, n, k, seed, out_indices, workspace, (size_t)workspace_bytes, S(stream));
}
// ---- RegressionMatcher.sample for a batch of pairs (sample_batched.hip)
long roma_op_sample_matches_workspace(int B, long n, long num, int balanced) {
  return (long)sample_matches_workspace_bytes(B, n, num, balanced);
}
int roma_op_sample_matches(const float* matches, const float* certainty, const unsigned long long* seeds, int B, long n, long num,
                           int threshold, float thresh, int balanced, float* out_matches, float* out_certainty, int* out_counts,
                           long long* out_idx, long long* out_first_idx, float* out_density, void* workspace, long workspace_bytes,
                           void* stream) {
  return sample_matches_launch(matches, certainty, seeds, B, n, num, threshold, thresh, balanced, out_matches, out_certainty, out_counts,
                               out_idx, out_first_idx, out_density, workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0),
                               S(stream));
}
// ---- batched RANSAC (geometry.hip)
long roma_op_ransac_workspace(int B, int N) { return (long)ransac_workspace_bytes(B, N); }
int roma_op_ransac(int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, int B,
                   int N, float threshold, double confidence, int max_iters, int refine, double* out_model, unsigned char* out_mask,
                   unsigned char* out_ok, int* out_info, void* workspace, long workspace_bytes, void* stream) {
  return ransac_launch(model, kpts_a, kpts_b, counts, seeds, B, N, threshold, confidence, max_iters, refine, out_model, out_mask,
                       out_ok, out_info, workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
long roma_op_magsac_workspace(int B, int N) { return (long)magsac_workspace_bytes(B, N); }
int roma_op_magsac(int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, int B,
                   int N, float threshold, double confidence, int max_iters, int lo_iters, double* out_model, unsigned char* out_mask,
                   unsigned char* out_ok, int* out_info, double* out_score, void* workspace, long workspace_bytes, void* stream) {
  return magsac_launch(model, kpts_a, kpts_b, counts, seeds, B, N, threshold, confidence, max_iters, lo_iters, out_model, out_mask,
                       out_ok, out_info, out_score, workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
// ---- essential matrix and recoverPose (essential.hip)
long roma_op_essential_workspace(int B, int N) { return (long)essential_workspace_bytes(B, N); }
int roma_op_essential(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
                      const double* camera_matrix, int B, int N, float threshold, double prob, int max_iters, double* out_e,
                      unsigned char* out_mask, unsigned char* out_ok, int* out_info, void* workspace, long workspace_bytes,
                      void* stream) {
  return essential_launch(kpts_a, kpts_b, counts, seeds, camera_matrix, B, N, threshold, prob, max_iters, out_e, out_mask, out_ok,
                          out_info, workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
long roma_op_essential_magsac_workspace(int B, int N) { return (long)essential_magsac_workspace_bytes(B, N); }
int roma_op_essential_magsac(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
                             const double* camera_matrix, int B, int N, float threshold, double prob, int max_iters, int lo_iters,
                             double* out_e, unsigned char* out_mask, unsigned char* out_ok, int* out_info, double* out_score,
                             void* workspace, long workspace_bytes, void* stream) {
  return essential_magsac_launch(kpts_a, kpts_b, counts, seeds, camera_matrix, B, N, threshold, prob, max_iters, lo_iters, out_e,
                                 out_mask, out_ok, out_info, out_score, workspace,
                                 (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
int roma_op_essential_minimal(const double* x0, const double* x1, int S_, double* out_e, int* out_n, void* stream) {
  return essential_minimal_launch(x0, x1, S_, out_e, out_n, S(stream));
}
long roma_op_recover_pose_workspace(int B, int N) { return (long)recover_pose_workspace_bytes(B, N); }
int roma_op_recover_pose(const double* E, const float* kpts_a, const float* kpts_b, const unsigned char* mask, const int* counts,
                         const double* camera_matrix, int B, int N, double distance_thresh, int* out_n_good, double* out_r,
                         double* out_t, unsigned char* out_mask, void* workspace, long workspace_bytes, void* stream) {
  return recover_pose_launch(E, kpts_a, kpts_b, mask, counts, camera_matrix, B, N, distance_thresh, out_n_good, out_r, out_t,
                             out_mask, workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
// ---- relative-pose refinement (pose_refine.hip)
long roma_op_refine_pose_workspace(int B, int N) { return (long)refine_pose_workspace_bytes(B, N); }
int roma_op_refine_pose(const double* R, const double* t, const float* kpts_a, const float* kpts_b, const int* counts,
                        const unsigned char* valid, int B, int N, double thr, int max_steps, double* out_r, double* out_t,
                        unsigned char* out_mask, int* out_info, void* workspace, long workspace_bytes, void* stream) {
  return refine_pose_launch(R, t, kpts_a, kpts_b, counts, valid, B, N, thr, max_steps, out_r, out_t, out_mask, out_info, workspace,
                            (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
// ---- absolute pose: P3P RANSAC, refinement, lifting (absolute_pose.hip)
long roma_op_absolute_pose_workspace(int B, int N) { return (long)absolute_pose_workspace_bytes(B, N); }
int roma_op_absolute_pose(const float* points3d, const float* kpts, const int* counts, const unsigned long long* seeds,
                          const double* camera_matrix, int B, int N, float threshold, double conf, int max_iters, double* out_r,
                          double* out_t, unsigned char* out_mask, unsigned char* out_ok, int* out_info, void* workspace,
                          long workspace_bytes, void* stream) {
  return absolute_pose_launch(points3d, kpts, counts, seeds, camera_matrix, B, N, threshold, conf, max_iters, out_r, out_t, out_mask,
                              out_ok, out_info, workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
int roma_op_absolute_pose_minimal(const double* X, const double* x, int S_, double* out_r, double* out_t, int* out_n, void* stream) {
  return absolute_pose_minimal_launch(X, x, S_, out_r, out_t, out_n, S(stream));
}
int roma_op_refine_absolute_pose(const double* R, const double* t, const float* points3d, const float* kpts, const int* counts,
                                 const unsigned char* valid, const double* camera_matrix, int B, int N, double thr, int max_steps,
                                 double* out_r, double* out_t, unsigned char* out_mask, int* out_info, void* stream) {
  return refine_absolute_pose_launch(R, t, points3d, kpts, counts, valid, camera_matrix, B, N, thr, max_steps, out_r, out_t, out_mask,
                                     out_info, S(stream));
}
int roma_op_lift_matches(const float* matches, const float* depth_a, const double* camera_a, int B, int N, int H, int W, int H_b,
                         int W_b, float* out_points, float* out_kpts_b, void* stream) {
  return lift_matches_launch(matches, depth_a, camera_a, B, N, H, W, H_b, W_b, out_points, out_kpts_b, S(stream));
}
// ---- bundle adjustment: cameras and points together, Schur-complement LM (bundle.hip)
long roma_op_bundle_adjust_workspace(int B, int V, int N) { return (long)bundle_adjust_workspace_bytes(B, V, N); }
int roma_op_bundle_adjust(const double* points, const float* kpts, const double* camera_matrices, const double* R, const double* t,
                          const unsigned char* hold, const int* counts, const unsigned char* valid, int B, int V, int N,
                          double reproj_thresh, int max_steps, double* out_points, double* out_r, double* out_t, unsigned char* out_mask,
                          int* out_info, double* out_cost, void* workspace, long workspace_bytes, void* stream) {
  return bundle_adjust_launch(points, kpts, camera_matrices, R, t, hold, counts, valid, B, V, N, reproj_thresh, max_steps, out_points,
                              out_r, out_t, out_mask, out_info, out_cost, workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0),
                              S(stream));
}
// ---- multi-view tracks from pairwise index matches (tracks.hip) and their N-view triangulation (triangulate_views.hip)
long roma_op_build_tracks_workspace(int B, int V, int K, int P, int M) { return (long)build_tracks_workspace_bytes(B, V, K, P, M); }
int roma_op_build_tracks(const int* inds, const int* pair_views, const int* match_counts, const int* num_kpts, const float* x, int B,
                         int V, int K, int P, int M, int max_tracks, int min_views, int* out_tracks, float* out_kpts, int* out_counts,
                         int* out_total, int* out_info, void* workspace, long workspace_bytes, void* stream) {
  return build_tracks_launch(inds, pair_views, match_counts, num_kpts, x, B, V, K, P, M, max_tracks, min_views, out_tracks, out_kpts,
                             out_counts, out_total, out_info, workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
// ---- detector-free keypoints: the dense matches of an image set to per-view keypoints and index matches (set_keypoints.hip)
long roma_op_keypoints_from_matches_workspace(int B, int V, int P, int N, long G_total, int K) {
  return (long)keypoints_from_matches_workspace_bytes(B, V, P, N, G_total, K);
}
int roma_op_keypoints_from_matches(const float* matches, const float* certainty, const int* counts, const int* pair_views,
                                   const int* sizes, int B, int V, int P, int N, int cell, float radius, int max_kpts, int one_to_one,
                                   float* out_kpts, float* out_score, int* out_num_kpts, int* out_total, int* out_inds, int* out_kept,
                                   int* out_info, void* workspace, long workspace_bytes, void* stream) {
  return keypoints_from_matches_launch(matches, certainty, counts, pair_views, sizes, B, V, P, N, cell, radius, max_kpts, one_to_one,
                                       out_kpts, out_score, out_num_kpts, out_total, out_inds, out_kept, out_info, workspace,
                                       (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
int roma_op_triangulate_views(const float* kpts, const double* camera_matrices, const double* R, const double* t,
                              const unsigned char* view_valid, const int* counts, const unsigned char* valid, int B, int V, int N,
                              double max_reproj, double min_parallax, double max_depth, int min_views, int gn_steps, int trim,
                              double* out_points, float* out_reproj, unsigned char* out_used, float* out_parallax,
                              unsigned char* out_flags, int* out_stats, void* stream) {
  return triangulate_views_launch(kpts, camera_matrices, R, t, view_valid, counts, valid, B, V, N, max_reproj, min_parallax, max_depth,
                                  min_views, gn_steps, trim, out_points, out_reproj, out_used, out_parallax, out_flags, out_stats,
                                  S(stream));
}
// ---- homography / fundamental-matrix refinement (model_refine.hip)
long roma_op_refine_model_workspace(int B, int N) { return (long)refine_model_workspace_bytes(B, N); }
int roma_op_refine_model(int model, const double* M, const float* kpts_a, const float* kpts_b, const int* counts,
                         const unsigned char* valid, int B, int N, double thr, int max_steps, double* out_m, unsigned char* out_mask,
                         int* out_info, double* out_cost, void* workspace, long workspace_bytes, void* stream) {
  return refine_model_launch(model, M, kpts_a, kpts_b, counts, valid, B, N, thr, max_steps, out_m, out_mask, out_info, out_cost,
                             workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
// ---- triangulation and depth consistency (triangulate.hip)
int roma_op_triangulate(const float* matches, const float* certainty, const int* counts, const unsigned char* valid, const double* R,
                        const double* t, const double* K_a, const double* K_b, int B, long n, int coords, int W_a, int H_a, int W_b,
                        int H_b, int sym_w, double max_depth, double max_reproj, double min_parallax, double min_certainty,
                        float* out_points, float* out_depth_other, float* out_reproj, float* out_parallax, unsigned char* out_flags,
                        int* out_stats, void* stream) {
  return triangulate_launch(matches, certainty, counts, valid, R, t, K_a, K_b, B, n, coords, W_a, H_a, W_b, H_b, sym_w, max_depth,
                            max_reproj, min_parallax, min_certainty, out_points, out_depth_other, out_reproj, out_parallax, out_flags,
                            out_stats, S(stream));
}
int roma_op_depth_consistency(const float* points, const unsigned char* flags, const double* R, const double* t, const double* K_a,
                              const double* K_b, int W_a, int H_a, int W_b, int H_b, int B, int H, int W, double rel_thresh,
                              unsigned char* out_consistent, float* out_err, void* stream) {
  return depth_consistency_launch(points, flags, R, t, K_a, K_b, W_a, H_a, W_b, H_b, B, H, W, rel_thresh, out_consistent, out_err,
                                  S(stream));
}
// ---- dense multi-view depth fusion and the relative poses of the pairs of a set of views (depth_fusion.hip)
long roma_op_fuse_depth_maps_workspace(int B, int V, int H, int W) { return (long)fuse_depth_maps_workspace_bytes(B, V, H, W); }
int roma_op_fuse_depth_maps(const float* points, const unsigned char* flags, const float* certainty, const int* pair_views,
                            const double* cameras, const double* R, const double* t, const unsigned char* view_valid,
                            const unsigned char* valid, const unsigned char* images, const long long* image_offsets,
                            const int* image_sizes, int B, int V, int P, int H, int W, int symmetric, double rel_thresh,
                            int min_support, int min_consistent, int max_violations, int dedupe, int max_points, float* out_depth,
                            float* out_weight, unsigned char* out_support, unsigned char* out_seen, unsigned char* out_violated,
                            unsigned char* out_state, float* out_points, unsigned char* out_colors, float* out_cloud_weight,
                            int* out_source, int* out_counts, int* out_total, int* out_stats, void* workspace, long workspace_bytes,
                            void* stream) {
  return fuse_depth_maps_launch(points, flags, certainty, pair_views, cameras, R, t, view_valid, valid, images, image_offsets,
                                image_sizes, B, V, P, H, W, symmetric, rel_thresh, min_support, min_consistent, max_violations, dedupe,
                                max_points, out_depth, out_weight, out_support, out_seen, out_violated, out_state, out_points,
                                out_colors, out_cloud_weight, out_source, out_counts, out_total, out_stats, workspace,
                                (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
int roma_op_relative_poses(const double* R, const double* t, const int* pair_views, int B, int V, int P, double* out_R, double* out_t,
                           void* stream) {
  return relative_poses_launch(R, t, pair_views, B, V, P, out_R, out_t, S(stream));
}
// ---- point-cloud rendering: z-buffered splat, occlusion filter, hole fill (point_render.hip)
long roma_op_render_points_workspace(int B, int C, int H, int W) { return (long)render_points_workspace_bytes(B, C, H, W); }
int roma_op_render_points(const float* points, const unsigned char* colors, const int* counts, const unsigned char* valid,
                          const double* cameras, const double* R, const double* t, int B, int N, int C, int H, int W, int radius,
                          double near, double far, int occlusion_radius, double occlusion_rel, int occlusion_count, int fill_radius,
                          int fill_min, int background, unsigned char* out_color, float* out_depth, int* out_index,
                          unsigned char* out_mask, int* out_stats, void* workspace, long workspace_bytes, void* stream) {
  return render_points_launch(points, colors, counts, valid, cameras, R, t, B, N, C, H, W, radius, near, far, occlusion_radius,
                              occlusion_rel, occlusion_count, fill_radius, fill_min, background, out_color, out_depth, out_index,
                              out_mask, out_stats, workspace, (size_t)(workspace_bytes > 0 ? workspace_bytes : 0), S(stream));
}
// ---- ground-truth warp from depth and dense EPE / PCK metrics (gt_warp.hip)
int roma_op_warp_kpts(const void* kpts, int kpts_f64, int grid_h, int grid_w, const float* depth0, const float* depth1, const double* T,
                      int t_rows, const double* K0, const double* K1, int B, long L, int H0, int W0, int H1, int W1, double rel_thresh,
                      unsigned char* out_valid, float* out_prob, double* out_rel, double* out_warped, void* stream) {
  return warp_kpts_launch(kpts, kpts_f64, grid_h, grid_w, depth0, depth1, T, t_rows, K0, K1, B, L, H0, W0, H1, W1, rel_thresh, out_valid,
                          out_prob, out_rel, out_warped, S(stream));
}
long roma_op_dense_metrics_workspace(int B, int h, int w) { return dense_metrics_workspace_bytes(B, h, w); }
int roma_op_dense_metrics(const float* matches, long batch_stride, long row_stride, const float* depth1, const float* depth2,
                          const double* T, int t_rows, const double* K1, const double* K2, int B, int h, int w, int H1, int W1, int H2,
                          int W2, double rel_thresh, double thr0, double thr1, double thr2, long long* out_n_valid,
                          long long* out_n_below, double* out_gd_sum, double* out_epe, double* out_pck, float* out_prob, double* out_gd,
                          void* workspace, long workspace_bytes, void* stream) {
  return dense_metrics_launch(matches, batch_stride, row_stride, depth1, depth2, T, t_rows, K1, K2, B, h, w, H1, W1, H2, W2, rel_thresh,
                              thr0, thr1, thr2, out_n_valid, out_n_below, out_gd_sum, out_epe, out_pck, out_prob, out_gd, workspace,
                              workspace_bytes, S(stream));
}
// ---- pose / homography benchmark scoring: errors, the error log, accuracy and AUC (metrics.hip)
int roma_op_pose_error(const double* R, const double* t, const unsigned char* ok, const double* T_gt, int t_rows, int B, double* out_err,
                       double* log, long capacity, long long* state, void* stream) {
  return pose_error_launch(R, t, ok, T_gt, t_rows, B, out_err, log, capacity, state, S(stream));
}
int roma_op_corner_error(const double* H_pred, const unsigned char* ok, const double* H_gt, const double* sizes, int B, double* out_err,
                         double* log, long capacity, long long* state, void* stream) {
  return corner_error_launch(H_pred, ok, H_gt, sizes, B, out_err, log, capacity, state, S(stream));
}
int roma_op_error_log_append(const double* values, int B, double* log, long capacity, long long* state, void* stream) {
  return error_log_append_launch(values, B, log, capacity, state, S(stream));
}
int roma_op_error_summary(const double* errors, long n, const long long* state, long capacity, const double* thresholds, int T,
                          long long* out_n, long long* out_below, double* out_acc, double* out_auc, void* stream) {
  return error_summary_launch(errors, n, state, capacity, thresholds, T, out_n, out_below, out_acc, out_auc, S(stream));
}
// ---- warp morph rendering: the frames of a parallax animation in one enqueue (morph.hip)
int roma_op_render_morph_frame_chunk(void) { return render_morph_frame_chunk(); }
long roma_op_render_morph_workspace(int B, int im_h, int im_w, long T) { return render_morph_workspace_bytes(B, im_h, im_w, T); }
int roma_op_render_morph(const float* warp, long warp_batch_stride, long warp_row_stride, const void* image, int image_u8, const double* ts,
                         const float* certainty, long cert_batch_stride, long cert_row_stride, float background, int B, long T, int H,
                         int W, int im_h, int im_w, void* out, int out_f32, void* workspace, long workspace_bytes, void* stream) {
  return render_morph_launch(warp, warp_batch_stride, warp_row_stride, image, image_u8, ts, certainty, cert_batch_stride, cert_row_stride,
                             background, B, T, H, W, im_h, im_w, out, out_f32, workspace, workspace_bytes, S(stream));
}
// ---- match_keypoints for a batch of warps: padded, counted, no host read (keypoints_batched.hip)
long roma_op_match_keypoints_workspace(int B, long NA, long NB) { return match_keypoints_workspace_bytes(B, NA, NB); }
int roma_op_match_keypoints(const float* x_a, const float* x_b, const int* counts_a, const int* counts_b, const float* warp,
                            long warp_batch_stride, long warp_row_stride, const float* certainty, long cert_batch_stride,
                            long cert_row_stride, const float* sizes, long sizes_batch_stride, int B, long NA, long NB, int H, int W,
                            float max_dist, float cert_th, long M, int* inds, float* kpts_a, float* kpts_b, int* counts,
                            long long* total, void* workspace, long workspace_bytes, void* stream) {
  return match_keypoints_launch(x_a, x_b, counts_a, counts_b, warp, warp_batch_stride, warp_row_stride, certainty, cert_batch_stride,
                                cert_row_stride, sizes, sizes_batch_stride, B, NA, NB, H, W, max_dist, cert_th, M, inds, kpts_a, kpts_b,
                                counts, total, workspace, workspace_bytes, S(stream));
}
// ---- image preprocessing: Pillow-exact bicubic resize + normalisation (preprocess.hip)
long roma_op_preprocess_workspace(const long long* desc_host, int n_images, const int* targets_hw, int n_targets) {
  return preprocess_workspace_bytes(desc_host, n_images, targets_hw, n_targets);
}
int roma_op_preprocess(const unsigned char* src, long long src_bytes, const long long* desc_host, const long long* desc_dev,
                       int n_images, const int* targets_hw, int n_targets, int normalize, float* out0, float* out1, void* workspace,
                       void* stream) {
  return preprocess_launch(src, src_bytes, desc_host, desc_dev, n_images, targets_hw, n_targets, normalize, out0, out1, workspace,
                           S(stream));
}
// ---- Tiny RoMa matcher side (tiny.hip)
int roma_op_nchw_to_nhwc(const float* in, float* out, int B, int C, int H, int W, void* stream) {
  return nchw_to_nhwc_launch(in, out, B, C, H, W, S(stream));
}
int roma_op_tiny_pos_embed(const float* corr_volume, float* out, int B, int H1, int W1, int H0, int W0, int exact_softmax,
                           void* stream) {
  return tiny_pos_embed_launch(corr_volume, out, B, H1, W1, H0, W0, exact_softmax, S(stream));
}
int roma_op_gray_instnorm(const float* in, float* out, int B, int H, int W, int C, float eps, void* stream) {
  return gray_instnorm_launch(in, out, B, H, W, C, eps, S(stream));
}
int roma_op_conv2d_nhwc(const float* in, const float* w, const float* bias, const float* res, float* out, int B, int H, int W,
                        int Cin, int Cout, int K, int stride, int pad, int relu, void* stream) {
  return conv2d_nhwc_launch(in, w, bias, res, out, B, H, W, Cin, Cout, K, stride, pad, relu, S(stream));
}
int roma_op_avgpool_nhwc(const float* in, float* out, int B, int H, int W, int C, int k, void* stream) {
  return avgpool_nhwc_launch(in, out, B, H, W, C, k, S(stream));
}
int roma_op_add3(const float* a, const float* b, const float* c, float* out, long n, void* stream) {
  return add3_launch(a, b, c, out, n, S(stream));
}
int roma_op_tiny_matcher_input(const float* f0, const float* f1, const float* warp, int warp_channels, float* d, int B, int H,
                               int W, int H1, int W1, int C, int Cp, void* stream) {
  return tiny_matcher_input_launch(f0, f1, warp, warp_channels, d, B, H, W, H1, W1, C, Cp, S(stream));
}
int roma_op_tiny_update(const float* base, int base_channels, const float* delta, long ldd, float sx, float sy, float* out,
                        long npix, void* stream) {
  return tiny_update_launch(base, base_channels, delta, ldd, sx, sy, out, npix, S(stream));
}
int roma_op_tiny_final(const float* matches, float* warp, float* certainty, int B, int H, int W, void* stream) {
  return tiny_final_launch(matches, warp, certainty, B, H, W, S(stream));
}
int roma_op_visualize_warp(const float* warp, const float* certainty, const float* im_a, const float* im_b, int H, int W,
                           int symmetric, int im_h, int im_w, float* out, void* stream) {
  return visualize_warp_launch(warp, certainty, im_a, im_b, H, W, symmetric, im_h, im_w, out, S(stream));
}
int roma_op_fb_consistency(const float* flow_fwd, const float* flow_bwd, int B, int H, int W, float th_n, float* out,
                           void* stream) {
  return fb_consistency_launch(flow_fwd, flow_bwd, B, H, W, th_n, out, S(stream));
}

int roma_op_maxpool2x2(const void* in, void* out, int B, int H, int W, int C, int dt, void* stream) {
  return maxpool2x2_launch(in, out, B, H, W, C, DT(dt), S(stream));
}

int roma_op_pool_proj(const void* in, void* pooled, void* pf, const void* pw, long ldw, const float* pb, int N, int ldf, int B, int H,
                      int W, int C, int dt, void* stream) {
  return pool_proj_launch(in, pooled, pf, pw, ldw, pb, N, ldf, B, H, W, C, DT(dt), S(stream));
}

int roma_op_refiner_out(const void* d, long ldd, int dt, const float* w, const float* b, float* flow, float* cert, long M,
                        int Cp, float sx, float sy, void* stream) {
  ROMA_REQUIRE(d && w && b && flow && cert && M > 0 && Cp > 0 && ldd >= Cp, "roma_op_refiner_out: bad arguments");
  return refiner_out_launch(d, ldd, DT(dt), w, b, flow, cert, M, Cp, sx, sy, S(stream));
}

int roma_op_conv3x3_c3_bf16(const float* img, const void* w, const float* bias, void* out, int B, int H, int W, void* stream) {
  return conv3x3_c3_bf16_launch(img, w, bias, out, B, H, W, S(stream));
}

int roma_op_conv3x3_c3(const float* img, const float* w, const float* bias, void* out, int B, int H, int W, int dt_out,
                       void* stream) {
  return conv3x3_c3_launch(img, w, bias, out, B, H, W, DT(dt_out), S(stream));
}

}  // extern "C"
