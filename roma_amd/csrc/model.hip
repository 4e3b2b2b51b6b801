// Model object: handle plumbing and the match() kernel schedule (see model.h).  Weight intake is model_weights.hip, the GP
// of the stride-16 scale gp.hip.
#include "model.h"

#include <dlfcn.h>
#include <math.h>
#include <stdlib.h>

#include <algorithm>

#include "arch.h"
#include "attention.h"
#include "conv64.h"
#include "dry_run.h"
#include "pool_proj.h"
#include "elementwise.h"
#include "gemm.h"
#include "gp.h"
#include "local_corr.h"
#include "refiner_block.h"
#include "vit.h"

namespace roma {

std::mutex g_peer_mutex;
extern void* g_peer_lib;  // api.hip: roma_tuning / roma_profile_* forward to the sibling library while a mixed handle lives
extern int g_mixed_handles;

Model::~Model() {
  for (int i = 0; i < MAX_STREAMS - 1; ++i) {
    if (side[i]) (void)hipStreamDestroy(side[i]);
    if (ev_join[i]) (void)hipEventDestroy(ev_join[i]);
  }
  if (ev_fork) (void)hipEventDestroy(ev_fork);
  for (void* p : owned) (void)hipFree(p);
  for (auto& kv : dbg) (void)hipFree(kv.second.first);
  for (auto& kv : inject) (void)hipFree(kv.second.first);
  if (peer_lib) {
    std::lock_guard<std::mutex> lk(g_peer_mutex);
    --g_mixed_handles;
  }
}


// ROMA_MIXED: the bfloat16 build of this library (libroma_hip.so, next to this shared object) runs DINOv2.  Loaded once per
// process with RTLD_LOCAL: both libraries export the same C ABI, each keeps its own symbols.
int Model::load_peer() {
  static void* lib = nullptr;
  static int (*fwd)(const roma_vit_args_t*, void*) = nullptr;
  std::lock_guard<std::mutex> lk(g_peer_mutex);  // handles may be created from several threads
  if (!lib) {
    ROMA_REQUIRE(roma_h16_format() == ROMA_F16, "ROMA_MIXED is a mode of the binary16 build (libroma_hip_f16.so)");
    Dl_info info;
    ROMA_REQUIRE(dladdr(reinterpret_cast<void*>(&roma_vit_forward), &info) && info.dli_fname, "ROMA_MIXED: cannot locate this library");
    std::string path(info.dli_fname);
    const size_t slash = path.find_last_of('/');
    path = (slash == std::string::npos ? std::string("") : path.substr(0, slash + 1)) + "libroma_hip.so";
    // RTLD_LOCAL: its C ABI must not shadow ours; RTLD_DEEPBIND on top of the link-time -Bsymbolic (csrc/Makefile): the
    // sibling's own definitions win over anything in the global scope - this library, when a C program linked it directly
    void* l = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL | RTLD_DEEPBIND);
    if (!l) {
      set_error("ROMA_MIXED: cannot load the bfloat16 library " + path + ": " + (dlerror() ? dlerror() : "?"));
      return ROMA_ERR_STATE;
    }
    auto fmt = reinterpret_cast<int (*)(void)>(dlsym(l, "roma_h16_format"));
    auto self = reinterpret_cast<int (*)(void)>(dlsym(l, "roma_self_check"));
    auto abi = reinterpret_cast<int (*)(void)>(dlsym(l, "roma_abi_stamp"));
    auto f = reinterpret_cast<int (*)(const roma_vit_args_t*, void*)>(dlsym(l, "roma_vit_forward"));
    std::string why;
    if (!fmt || !f || !self || !abi) why = "it does not export roma_h16_format / roma_self_check / roma_abi_stamp / roma_vit_forward (an older build)";
    else if (fmt() != ROMA_BF16) why = "it is not the bfloat16 build";
    else if (abi() != roma_abi_stamp()) why = "its ABI stamp " + std::to_string(abi()) + " differs from this library's " + std::to_string(roma_abi_stamp()) + " (stale build: roma_vit_args_t would be misread)";
    else if (self() != ROMA_BF16) why = "its internal calls resolve into another library (symbol interposition: link both builds with -Wl,-Bsymbolic)";
    if (!why.empty()) {
      dlclose(l);
      set_error("ROMA_MIXED: " + path + " cannot serve as the bfloat16 sibling: " + why);
      return ROMA_ERR_STATE;
    }
    lib = l;
    fwd = f;
    g_peer_lib = l;
  }
  if (!peer_lib) ++g_mixed_handles;
  peer_lib = lib;
  peer_vit_forward = fwd;
  return 0;
}

int Model::debug_inject(const char* name, const void* host, size_t bytes) {
  ROMA_REQUIRE(name, "roma_debug_inject: null name");
  const std::string k(name);
  ROMA_REQUIRE(k == "gm_flow16" || k == "gm_cert16", "roma_debug_inject: unknown stage (gm_flow16, gm_cert16)");
  ROMA_CHECK_HIP(hipSetDevice(cfg.device));
  auto it = inject.find(k);
  if (it != inject.end()) {
    ROMA_CHECK_HIP(hipDeviceSynchronize());
    (void)hipFree(it->second.first);
    inject.erase(it);
  }
  if (!host || bytes == 0) return 0;
  void* p = nullptr;
  ROMA_CHECK_HIP(hipMalloc(&p, bytes));
  ROMA_CHECK_HIP(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
  inject[k] = {p, bytes};
  return 0;
}

int Model::finalize() {
  ROMA_REQUIRE(!finalized, "roma_finalize: already finalized");
  ROMA_CHECK_HIP(hipSetDevice(cfg.device));
  if (int rc = check_contract()) return rc;
  act_dt = cfg.precision == ROMA_F32 ? DT_F32 : DT_BF16;  // roma_create admitted only this build's 16-bit code (+ ROMA_MIXED)
  mixed = cfg.precision == ROMA_MIXED;
  if (mixed)
    if (int rc = load_peer()) return rc;
  if (int rc = pack_weights()) return rc;
  host.clear();
  // plan the workspace with a dry run at the largest configuration
  arena.dry = persist.dry = true;
  arena.peak = persist.peak = 0;
  const int keep_sym = cfg.symmetric, keep_up = cfg.upsample_preds;
  cfg.symmetric = 1;
  cfg.upsample_preds = cfg.upsample_h > 0 ? 1 : 0;
  int rc = match_impl(cfg.max_batch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, arena, persist);
  // cached features (encoded.h): the layout of a pack, and the two schedules that use it - roma_match_encoded of max_batch
  // pairs and roma_encode of a chunk of 2 * max_batch images - walk the same arenas; the peaks keep the maximum
  int cf[5];
  for (int i = 0; i < 5; ++i) cf[i] = ref[i].Cf;
  pack = pack_layout(cfg.coarse_h, cfg.coarse_w, cfg.upsample_h, cfg.upsample_w, cf, act_dt == DT_F32 ? 4 : 2);
  const EncodedIn plan_enc;
  if (!rc) rc = match_impl(cfg.max_batch, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, arena, persist, nullptr, &plan_enc);
  if (!rc) rc = encode_impl(2 * cfg.max_batch, nullptr, nullptr, nullptr, nullptr, true, cfg.upsample_h > 0, arena, persist);
  // side streams (model.h): every side sub-batch is at most floor(max_batch / 2) pairs; only the sizes are planned here
  Arena plan, plan_p;
  if (!rc && cfg.max_batch >= 2)
    rc = match_impl(cfg.max_batch / 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, plan, plan_p);
  if (!rc && cfg.max_batch >= 2)
    rc = match_impl(cfg.max_batch / 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, true, plan, plan_p, nullptr, &plan_enc);
  cfg.symmetric = keep_sym;
  cfg.upsample_preds = keep_up;
  if (rc) return rc;
  side_arena_bytes = plan.peak + 4096;
  side_persist_bytes = plan_p.peak + 4096;
  arena.cap = arena.peak + 4096;
  persist.cap = persist.peak + 4096;
  ROMA_CHECK_HIP(hipMalloc((void**)&arena.base, arena.cap));
  owned.push_back(arena.base);
  ROMA_CHECK_HIP(hipMalloc((void**)&persist.base, persist.cap));
  owned.push_back(persist.base);
  ROMA_CHECK_HIP(hipMemset(persist.base, 0, persist.cap));
  ROMA_CHECK_HIP(hipMemset(arena.base, 0, arena.cap));
  arena.dry = persist.dry = false;
  finalized = true;
  return 0;
}

// Side arenas, streams and events for `n` sub-batch streams, created on first use (a few GB of hipMalloc: first call only).
int Model::ensure_side_streams(int n) {
  for (int i = streams_ready - 1; i + 1 < n; ++i) {
    Arena &a = side_arena[i], &p = side_persist[i];
    a.cap = side_arena_bytes;
    p.cap = side_persist_bytes;
    ROMA_CHECK_HIP(hipMalloc((void**)&a.base, a.cap));
    owned.push_back(a.base);
    ROMA_CHECK_HIP(hipMalloc((void**)&p.base, p.cap));
    owned.push_back(p.base);
    ROMA_CHECK_HIP(hipMemset(p.base, 0, p.cap));
    ROMA_CHECK_HIP(hipMemset(a.base, 0, a.cap));
    ROMA_CHECK_HIP(hipDeviceSynchronize());
    a.dry = p.dry = false;
    ROMA_CHECK_HIP(hipStreamCreateWithFlags(&side[i], hipStreamNonBlocking));
    ROMA_CHECK_HIP(hipEventCreateWithFlags(&ev_join[i], hipEventDisableTiming));
    if (!ev_fork) ROMA_CHECK_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    streams_ready = i + 2;
  }
  return 0;
}

// diagnostics (tools/repro_mixed.py): ROMA_DEBUG_DUAL_SLOT = k keeps the sub-batch stream split on in debug mode and lets only
// sub-batch k capture its stages (the capture table is per handle, not per stream)
static int dbg_dual_slot() { return tuning(SW_DEBUG_DUAL_SLOT); }

int Model::dbg_save(const char* name, const void* p, size_t bytes, hipStream_t st) {
  if (!debug) return 0;
  if (dbg_dual_slot() >= 0) {  // only the stages named in ROMA_DEBUG_ONLY (comma separated), only for the chosen sub-batch
    static const std::string only = std::string(",") + (getenv("ROMA_DEBUG_ONLY") ? getenv("ROMA_DEBUG_ONLY") : "") + ",";
    if (dbg_cur_slot != dbg_dual_slot() || only.find(std::string(",") + name + ",") == std::string::npos) return 0;
  }
  auto it = dbg.find(name);
  if (it == dbg.end() || it->second.second != bytes) {
    if (it != dbg.end()) (void)hipFree(it->second.first);
    void* q = nullptr;
    ROMA_CHECK_HIP(hipMalloc(&q, bytes));
    dbg[name] = {q, bytes};
    it = dbg.find(name);
  }
  ROMA_CHECK_HIP(hipMemcpyAsync(it->second.first, p, bytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

int Model::match(int B, const float* ima, const float* imb, const float* ima_hr, const float* imb_hr, float* warp,
                 float* cert, hipStream_t st) {
  ROMA_REQUIRE(finalized, "roma_match: call roma_finalize first");
  ROMA_REQUIRE(B >= 1 && B <= cfg.max_batch, "roma_match: batch size out of range (max_batch)");
  ROMA_REQUIRE(ima && imb && warp && cert, "roma_match: null image / output pointer");
  if (cfg.upsample_preds) {
    ROMA_REQUIRE(cfg.upsample_h > 0, "roma_match: upsample_preds set but the handle has no upsample resolution");
    ROMA_REQUIRE(ima_hr && imb_hr, "roma_match: upsample_preds requires im_A_high_res and im_B_high_res");
  }
  ROMA_CHECK_HIP(hipSetDevice(cfg.device));
  return match_streams(B, ima, imb, ima_hr, imb_hr, warp, cert, st);
}

int Model::forward(int B, const float* ima, const float* imb, const roma_forward_args_t* fw, hipStream_t st) {
  ROMA_REQUIRE(finalized, "roma_forward: call roma_finalize first");
  ROMA_REQUIRE(B >= 1 && B <= cfg.max_batch, "roma_forward: batch size out of range (max_batch)");
  ROMA_REQUIRE(ima && imb && fw, "roma_forward: null image / argument pointer");
  if (fw->upsample) {
    ROMA_REQUIRE(cfg.upsample_h > 0, "roma_forward: upsample pass on a handle without an upsample resolution");
    ROMA_REQUIRE(fw->seed_flow && fw->seed_cert && fw->seed_h > 0 && fw->seed_w > 0,
                 "roma_forward: the upsample pass needs batch[\"corresps\"] (seed_flow / seed_cert)");
  }
  ROMA_CHECK_HIP(hipSetDevice(cfg.device));
  return match_impl(B, ima, imb, nullptr, nullptr, nullptr, nullptr, st, false, arena, persist, fw);
}

// Encoders and proj heads once per image.  Chunks of 2 * max_batch images: the image count the workspace was planned for.
int Model::encode(int N, const float* images, const float* images_hr, void* feats, long feats_bytes, hipStream_t st) {
  ROMA_REQUIRE(finalized, "roma_encode: call roma_finalize first");
  ROMA_REQUIRE(N >= 1 && images && feats, "roma_encode: N < 1 or null image / feature pointer");
  ROMA_REQUIRE(!images_hr || cfg.upsample_h > 0, "roma_encode: high-resolution images on a handle without an upsample resolution");
  ROMA_REQUIRE(feats_bytes == (long)N * pack.total, "roma_encode: feats_bytes must be N * roma_encoded_bytes() = " +
                                                        std::to_string((long)N * pack.total) + " (got " + std::to_string(feats_bytes) + ")");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(feats) & 15) == 0, "roma_encode: the feature buffer must be 16-byte aligned");
  ROMA_CHECK_HIP(hipSetDevice(cfg.device));
  const size_t im_lo = (size_t)3 * cfg.coarse_h * cfg.coarse_w, im_hi = (size_t)3 * cfg.upsample_h * cfg.upsample_w;
  const int chunk = 2 * cfg.max_batch;
  for (int i0 = 0; i0 < N; i0 += chunk)
    if (int rc = encode_impl(std::min(chunk, N - i0), images + i0 * im_lo, images_hr ? images_hr + i0 * im_hi : nullptr,
                             static_cast<char*>(feats) + (long)i0 * pack.total, st, false, images_hr != nullptr, arena, persist))
      return rc;
  return 0;
}

// match() on pairs of cached images: every index is checked here, on the host, before anything is enqueued
int Model::match_encoded(int P, const void* feats, long feats_bytes, int N, const int* idx_a, const int* idx_b, float* warp, float* cert,
                         hipStream_t st) {
  ROMA_REQUIRE(finalized, "roma_match_encoded: call roma_finalize first");
  ROMA_REQUIRE(P >= 1 && P <= cfg.max_batch, "roma_match_encoded: number of pairs out of range (max_batch)");
  ROMA_REQUIRE(feats && idx_a && idx_b && warp && cert && N >= 1, "roma_match_encoded: null pointer or N < 1");
  ROMA_REQUIRE(feats_bytes == (long)N * pack.total, "roma_match_encoded: feats_bytes must be N * roma_encoded_bytes() = " +
                                                        std::to_string((long)N * pack.total) + " (got " + std::to_string(feats_bytes) + ")");
  ROMA_REQUIRE((reinterpret_cast<uintptr_t>(feats) & 15) == 0, "roma_match_encoded: the feature buffer must be 16-byte aligned");
  for (int i = 0; i < P; ++i)
    ROMA_REQUIRE(idx_a[i] >= 0 && idx_a[i] < N && idx_b[i] >= 0 && idx_b[i] < N,
                 "roma_match_encoded: pair " + std::to_string(i) + " = (" + std::to_string(idx_a[i]) + ", " + std::to_string(idx_b[i]) +
                     ") names an image outside [0, " + std::to_string(N) + ")");
  if (cfg.upsample_preds)
    ROMA_REQUIRE(cfg.upsample_h > 0, "roma_match_encoded: upsample_preds set but the handle has no upsample resolution");
  ROMA_CHECK_HIP(hipSetDevice(cfg.device));
  const EncodedIn enc{static_cast<const char*>(feats), idx_a, idx_b};
  return match_streams(P, nullptr, nullptr, nullptr, nullptr, warp, cert, st, &enc);
}

int Model::match_streams(int B, const float* ima, const float* imb, const float* ima_hr, const float* imb_hr, float* warp,
                         float* cert, hipStream_t st, const EncodedIn* enc) {
  const int env_streams = tuning(SW_STREAMS);
  const bool serial_env = tuning(SW_STREAMS_SERIAL) != 0;
  const int ns = (debug && dbg_dual_slot() < 0) ? 1 : std::min(std::min(env_streams > 0 ? env_streams : n_streams, (int)MAX_STREAMS), B);
  if (ns <= 1) return match_impl(B, ima, imb, ima_hr, imb_hr, warp, cert, st, false, arena, persist, nullptr, enc);
  if (int rc = ensure_side_streams(ns)) return rc;
  // fork: the side streams start after everything already queued on the caller's stream (inputs); join at the end
  const size_t im_lo = (size_t)3 * cfg.coarse_h * cfg.coarse_w, im_hi = (size_t)3 * cfg.upsample_h * cfg.upsample_w;
  const int Ho = cfg.upsample_preds ? cfg.upsample_h : cfg.coarse_h, Wo = cfg.upsample_preds ? cfg.upsample_w : cfg.coarse_w;
  const size_t px = (size_t)Ho * Wo * (cfg.symmetric ? 2 : 1);
  ROMA_CHECK_HIP(hipEventRecord(ev_fork, st));
  int rc = 0, b0 = 0;
  for (int i = 0; i < ns; ++i) {  // balanced contiguous split; part 0 (the largest) stays on the caller's stream
    const int bi = B / ns + (i < B % ns ? 1 : 0);
    hipStream_t si = i == 0 ? st : side[i - 1];
    if (i > 0) ROMA_CHECK_HIP(hipStreamWaitEvent(si, ev_fork, 0));
    if (i > 0 && serial_env) {  // diagnostic: same streams and arenas, but no overlap - sub-batch i starts after i - 1 ended
      hipStream_t sp = i == 1 ? st : side[i - 2];
      ROMA_CHECK_HIP(hipEventRecord(ev_join[i - 1], sp));
      ROMA_CHECK_HIP(hipStreamWaitEvent(si, ev_join[i - 1], 0));
    }
    EncodedIn sub;  // cached features: this sub-batch's slice of the pair list
    if (enc) sub = EncodedIn{enc->feats, enc->idx_a + b0, enc->idx_b + b0};
    if (!rc)
      rc = match_impl(bi, ima ? ima + b0 * im_lo : nullptr, imb ? imb + b0 * im_lo : nullptr, ima_hr ? ima_hr + b0 * im_hi : nullptr,
                      imb_hr ? imb_hr + b0 * im_hi : nullptr, warp + b0 * px * 4, cert + b0 * px, si, false,
                      i == 0 ? arena : side_arena[i - 1], i == 0 ? persist : side_persist[i - 1], nullptr, enc ? &sub : nullptr);
    b0 += bi;
  }
  // always join, also on error: the caller's stream must not run ahead of work already queued on a side stream
  for (int i = 1; i < ns; ++i) {
    (void)hipEventRecord(ev_join[i - 1], side[i - 1]);
    (void)hipStreamWaitEvent(st, ev_join[i - 1], 0);
  }
  return rc;
}

// ---------------------------------------------------------------- the match() schedule: contexts
struct Model::Call {
  Arena &arena, &persist;
  int B = 0, nimg = 0, ndp = 0;
  int shift = 0;  // support image of directed pair i = (i + shift) % nimg
  bool sym = false;
  size_t esz = 4;  // bytes of an activation element
  hipStream_t st = nullptr;
  bool dry = false;
  int tslot = 0;  // sub-batch stream of this call: row of the trace table, slot of the debug capture
  bool tracing = false;
  const roma_forward_args_t* fw = nullptr;
  int th = 0, tw = 0, T = 0;                                 // coarse token grid
  int Npd = 0, Npt = 0;                                      // padded attention rows of DINOv2 (T + 1) / the decoder (T)
  void *qbuf = nullptr, *kbuf = nullptr, *vtbuf = nullptr;   // persistent, zero-initialised (pads must stay finite)
  void *ln = nullptr, *ao = nullptr, *hid = nullptr;         // shared transformer scratch (DINOv2 rows >= decoder rows)
  Call(Arena& a, Arena& p) : arena(a), persist(p) {}
  void* alloc(size_t elems, size_t es) const { return arena.alloc(elems * es); }
  void* at(void* p, long elems) const { return static_cast<char*>(p) + elems * (long)esz; }
};

struct Model::Pass {
  bool up = false;
  int H = 0, W = 0;
  const float *imA = nullptr, *imB = nullptr;
  void* feat[5] = {nullptr};  // index by log2(stride): 0 -> stride 1 ... 3 -> stride 8 ; [4] = stride 16 (DINOv2)
  // Round 6 (pool_proj.hip): at strides 1 and 2 the max-pool and the proj head of the level read the un-pooled map in ONE
  // pass (16-bit modes); the projected maps are then ready when the decoder reaches those scales.  pf_pre[l]: stride 2^l.
  void* pf_pre[2] = {nullptr, nullptr};
  bool pp_on[2] = {false, false};
  double scale_factor = 1.0;
  float *flow = nullptr, *cert = nullptr, *flow_alt = nullptr, *cert_alt = nullptr;  // current maps and their ping-pong alternates
  const char* tag() const { return up ? "p2" : "p1"; }
};

struct Model::Scale {
  int si, ins, hs, ws;
  int lvl;  // log2(ins): index into Pass::feat
  long hw, M;  // pixels of one map; rows of the refiner's buffers (ndp * hw)
  const RefinerW& r;
  int ldf;
  float sx, sy;    // flow delta -> normalised coordinates
  std::string tp;  // trace prefix "p<pass>_s<stride>"
  size_t pf_bytes, d_bytes, flow_bytes, cert_bytes;
  void* pf = nullptr;                  // projected features [nimg, hw, ldf]
  void *d0 = nullptr, *d1 = nullptr;   // ConvRefiner ping-pong [M, Cp]
  Scale(const Call& c, const Pass& p, int si_, const RefinerW& r_)
      : si(si_), ins(SCALE_INT[si_]), hs(ins == 16 ? c.th : p.H / ins), ws(ins == 16 ? c.tw : p.W / ins),
        lvl(ins == 16 ? 4 : (ins == 8 ? 3 : (ins == 4 ? 2 : (ins == 2 ? 1 : 0)))), hw((long)hs * ws), M((long)c.ndp * hw), r(r_),
        ldf((int)round_up(r_.Cf, 8)), sx((float)ins / (4.0f * (float)p.W)), sy((float)ins / (4.0f * (float)p.H)),
        tp(std::string(p.tag()) + "_s" + SCALES[si_]), pf_bytes((size_t)c.nimg * hw * ldf * c.esz),
        d_bytes((size_t)M * r_.Cp * c.esz), flow_bytes((size_t)M * 2 * 4), cert_bytes((size_t)M * 4) {}
};

// A live call whose allocations no longer fit the plan returns here, before the launches that would have used them.
int Model::fits(const Call& c) {
  if (c.dry || !(c.arena.overflow || c.persist.overflow)) return 0;
  c.arena.overflow = c.persist.overflow = false;
  set_error("roma_match / roma_forward: the workspace planned by roma_finalize is too small for this call (an option that "
            "changes the buffer plan was switched after roma_finalize); the results of this call are invalid");
  return -5;
}

// The one observation point of the schedule.  trace_name: the determinism trace XORs a checksum of the buffer (of columns
// [c0, c1) of its `rows` rows of `ld` elements when c1 > c0) into the next entry of this sub-batch stream's table.
// dbg_name: the debug capture keeps a copy.  An empty name switches that half off.
int Model::observe(const Call& c, const std::string& trace_name, const std::string& dbg_name, const void* p, size_t bytes,
                   long rows, int ld, int c0, int c1) {
  // table full: later stages are not traced (roma_debug_trace sees <= TRACE_MAX)
  if (c.tracing && !trace_name.empty() && trace_n[c.tslot] < TRACE_MAX) {
    const int k = trace_n[c.tslot]++;
    if ((int)trace_names[c.tslot].size() <= k) trace_names[c.tslot].push_back(trace_name);
    else trace_names[c.tslot][k] = trace_name;
    unsigned long long* out = trace_dev[c.tslot] + k;
    if (int rc = c1 > c0 ? checksum_cols_launch(p, rows, ld, c0, c1, out, c.st) : checksum_launch(p, bytes, out, c.st)) return rc;
  }
  if (debug && !c.dry && !dbg_name.empty()) return dbg_save(dbg_name.c_str(), p, bytes, c.st);
  return 0;
}

// ---------------------------------------------------------------- stages
// encoder: VGG19-BN pyramid (encoders.py:17-27) -> feat[0..3], and the projected maps of strides 1 / 2 where they are fused
int Model::encode_vgg(const Call& c, Pass& p) {
  const bool dry = c.dry; hipStream_t st = c.st;
  const int H = p.H, W = p.W, nimg = c.nimg, B = c.B;  // B images at imA and B at imB; roma_encode: imB == nullptr, B == nimg
  const size_t esz = c.esz;
  const int fh[4] = {H, H / 2, H / 4, H / 8}, fw_[4] = {W, W / 2, W / 4, W / 8};
  const int fc[4] = {64, 128, 256, 512};
  size_t fbytes[4];
  for (int l = 0; l < 4; ++l) {
    fbytes[l] = (size_t)nimg * fh[l] * fw_[l] * fc[l] * esz;
    p.feat[l] = c.arena.alloc(fbytes[l]);
  }
  const int pp_si[2] = {4, 3};  // index of stride 1 / 2 in SCALES
  for (int l = 0; l < 2; ++l) {
    const RefinerW& rr = ref[pp_si[l]];
    const int ldf_l = (int)round_up(rr.Cf, 8);
    p.pp_on[l] = tuning(SW_POOL_PROJ) != 0 && fh[l] >= 2 && fw_[l] >= 2 &&
                 pool_proj_supported(fc[l], rr.Cf, ldf_l, act_dt) && proj[pp_si[l]].b != nullptr;
    if (p.pp_on[l] || dry) p.pf_pre[l] = c.alloc((size_t)nimg * fh[l] * fw_[l] * ldf_l, esz);  // (planned whatever the switch says now)
    if (!p.pp_on[l] && !dry) p.pf_pre[l] = nullptr;
  }
  const size_t enc_mark = c.arena.mark();
  void* t0 = c.alloc((size_t)nimg * H * W * 64, esz);
  void* t1 = c.alloc((size_t)nimg * (H / 2) * (W / 2) * 64, esz);
  void* col1 = c.alloc((size_t)nimg * H * W * 32, esz);  // (planned whichever form runs: the switch may change between calls)
  if (int rc = fits(c)) return rc;
  if (act_dt == DT_BF16 && (tuning(SW_CONV64) & 4) && (long)3 * H * W < (1l << 23)) {  // (its packed tap offsets)
    // first layer (Cin = 3), bf16: fused kernel straight from the f32 image (conv64.hip)
    RUN(conv3x3_c3_bf16_launch(p.imA, vgg[0].w, vgg[0].b, t0, B, H, W, st));
    if (p.imB) RUN(conv3x3_c3_bf16_launch(p.imB, vgg[0].w, vgg[0].b, c.at(t0, (long)B * H * W * 64), B, H, W, st));
  } else {  // im2col to K = 32, then the same MFMA GEMM as every other layer
    RUN(im2col3x3_c3_launch(p.imA, col1, B, H, W, act_dt, st));
    if (p.imB) RUN(im2col3x3_c3_launch(p.imB, c.at(col1, (long)B * H * W * 32), B, H, W, act_dt, st));
    GemmArgs g;
    g.A = col1; g.lda = 32; g.W = vgg[0].w; g.ldw = vgg[0].ldw; g.C = t0; g.ldc = 64;
    g.M = nimg * H * W; g.N = 64; g.K = 32; g.k_alg = 27; g.in_dt = act_dt; g.out_dt = act_dt; g.bias = vgg[0].b; g.act = ACT_RELU;
    RUN(gemm_launch(g, st));
  }
  auto conv = [&](int li, const void* in, void* out, int h, int w) -> int {
    GemmArgs g;
    g.A = in; g.W = vgg[li].w; g.ldw = vgg[li].ldw; g.C = out; g.ldc = vgg_cout[li];
    g.M = nimg * h * w; g.N = vgg_cout[li]; g.K = 9 * vgg_cin[li];
    g.in_dt = act_dt; g.out_dt = act_dt; g.bias = vgg[li].b; g.act = ACT_RELU;
    g.conv_h = h; g.conv_w = w; g.conv_c = vgg_cin[li]; g.conv_korder = vgg_korder[li];
    RUN(gemm_launch(g, st));
    return 0;
  };
  auto pool = [&](int l, const void* in, void* out) -> int {
    if (p.pp_on[l]) {
      const int si_ = pp_si[l];
      RUN(pool_proj_launch(in, out, p.pf_pre[l], proj[si_].w, proj[si_].ldw, proj[si_].b, ref[si_].Cf, (int)round_up(ref[si_].Cf, 8),
                           nimg, fh[l], fw_[l], fc[l], act_dt, st));
    } else {
      RUN(maxpool2x2_launch(in, out, nimg, fh[l], fw_[l], fc[l], act_dt, st));
    }
    return 0;
  };
  if (int rc = conv(1, t0, p.feat[0], H, W)) return rc;
  if (int rc = pool(0, p.feat[0], t1)) return rc;
  if (int rc = conv(2, t1, t0, H / 2, W / 2)) return rc;
  if (int rc = conv(3, t0, p.feat[1], H / 2, W / 2)) return rc;
  if (int rc = pool(1, p.feat[1], t1)) return rc;
  if (int rc = conv(4, t1, t0, H / 4, W / 4)) return rc;
  if (int rc = conv(5, t0, t1, H / 4, W / 4)) return rc;
  if (int rc = conv(6, t1, t0, H / 4, W / 4)) return rc;
  if (int rc = conv(7, t0, p.feat[2], H / 4, W / 4)) return rc;
  RUN(maxpool2x2_launch(p.feat[2], t1, nimg, H / 4, W / 4, 256, act_dt, st));
  if (int rc = conv(8, t1, t0, H / 8, W / 8)) return rc;
  if (int rc = conv(9, t0, t1, H / 8, W / 8)) return rc;
  if (int rc = conv(10, t1, t0, H / 8, W / 8)) return rc;
  if (int rc = conv(11, t0, p.feat[3], H / 8, W / 8)) return rc;
  c.arena.release(enc_mark);
  static const char* const dbg_names[4] = {"feat1", "feat2", "feat4", "feat8"};
  for (int l = 0; l < 4; ++l)
    if (int rc = observe(c, std::string(p.tag()) + "_" + dbg_names[l], p.up ? "" : dbg_names[l], p.feat[l], fbytes[l])) return rc;
  if (c.fw && !dry)  // extract_backbone_features (matcher.py:585-596): fw->feat[] is ordered 16, 8, 4, 2, 1
    for (int l = 0; l < 4; ++l)
      if (c.fw->feat[4 - l]) ROMA_CHECK_HIP(hipMemcpyAsync(c.fw->feat[4 - l], p.feat[l], fbytes[l], hipMemcpyDeviceToDevice, st));
  return 0;
}

// encoder: DINOv2 ViT-L/14 (dinov2.py:192-237) -> feat[4]; also allocates the transformer scratch it shares with the decoder
int Model::encode_dino(Call& c, Pass& p) {
  const bool dry = c.dry; hipStream_t st = c.st;
  const int nimg = c.nimg, T = c.T;
  const size_t esz = c.esz;
  const long rows_d = (long)nimg * (T + 1), rows_t = (long)c.ndp * T;
  const size_t fbytes = (size_t)nimg * T * 1024 * esz;
  p.feat[4] = c.arena.alloc(fbytes);
  const long rmax = std::max(rows_d, rows_t);
  c.ln = c.alloc((size_t)rmax * 1024, esz);
  c.ao = c.alloc((size_t)rmax * 1024, esz);
  c.hid = c.alloc((size_t)rmax * 4096, esz);
  const size_t dmark = c.arena.mark();
  void* col = c.alloc((size_t)nimg * T * patch.ldw, esz);
  float* pt = (float*)c.alloc((size_t)nimg * T * 1024, 4);
  float* x = (float*)c.alloc((size_t)rows_d * 1024, 4);
  const bool res_f32_env = tuning(SW_VIT_RES_F32) != 0;
  void* xs = nullptr;
  if (act_dt == DT_BF16) xs = c.alloc((size_t)rows_d * 1024, 2);  // 16-bit residual stream: always planned, the option may flip later
  void* feat_vit = p.feat[4];
  if (mixed) feat_vit = c.alloc((size_t)nimg * T * 1024, 2);       // bfloat16 patch tokens of the sibling library
  if (int rc = fits(c)) return rc;
  if (!dry) {
    roma_vit_block_t blk[24];
    for (int i = 0; i < 24; ++i) blk[i] = dino[i].pub();
    roma_vit_args_t va{};
    va.B = c.B; va.H = p.H; va.W = p.W;
    va.act = act_dt == DT_F32 ? ROMA_F32 : (mixed ? ROMA_BF16 : roma_h16_format());
    va.bf16_residual = act_dt == DT_BF16 && vit_bf16_residual && !res_f32_env;
    va.im_a = p.imA; va.im_b = p.imB;
    va.patch_w = patch.w; va.patch_b = patch.b; va.patch_ldw = patch.ldw;
    va.cls_tok = cls_tok; va.pos_emb = pos_emb;
    va.blocks = blk; va.nblocks = 24;
    va.norm_w = dino_nw; va.norm_b = dino_nb;
    va.col = col; va.pt = pt; va.x = x; va.xs = xs; va.ln = c.ln; va.ao = c.ao; va.hid = c.hid;
    va.q = c.qbuf; va.k = c.kbuf; va.vt = c.vtbuf;
    va.feat_out = feat_vit;
    if (mixed) {
      // DINOv2 in bfloat16 (the reference's amp_dtype reaches only it, roma_models.py:183-188) in the bf16 build of this
      // library, on this sub-batch's stream; autocast then casts its features to binary16 for the proj head
      if (int rc = peer_vit_forward(&va, st)) {
        set_error("ROMA_MIXED: roma_vit_forward of the bfloat16 library failed");
        return rc;
      }
      RUN(convert_from_bf16_launch(feat_vit, p.feat[4], (long)nimg * T * 1024, st));
    } else {
      RUN(vit_forward(va, st));
    }
  }
  c.arena.release(dmark);
  if (int rc = observe(c, "feat16", "feat16", p.feat[4], fbytes)) return rc;
  if (c.fw && !dry && c.fw->feat[0]) ROMA_CHECK_HIP(hipMemcpyAsync(c.fw->feat[0], p.feat[4], fbytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

// The upsample pass starts from the finest correspondences of the coarse pass, or from the caller's (roma_forward)
int Model::seed_upsample_pass(const Call& c, const Pass& p, const float* flow_p1, const float* cert_p1) {
  const bool dry = c.dry;
  const roma_forward_args_t* fw = c.fw;  // batch["corresps"] of the caller, any resolution (matcher.py:423-435)
  const int sh = fw ? fw->seed_h : cfg.coarse_h, sw = fw ? fw->seed_w : cfg.coarse_w;
  RUN(resize_bilinear_launch(fw ? fw->seed_flow : flow_p1, p.flow, c.ndp, sh, sw, p.H / 8, p.W / 8, 2, c.st));
  RUN(resize_bilinear_launch(fw ? fw->seed_cert : cert_p1, p.cert, c.ndp, sh, sw, p.H / 8, p.W / 8, 1, c.st));
  return 0;
}

// proj head of a scale, once per image (proj(f_s) == swap(proj(f_q)) since it is per-image)
int Model::proj_head(const Call& c, const Pass& p, Scale& s) {
  const bool dry = c.dry;
  const bool pf_ready = s.lvl < 2 && p.pp_on[s.lvl];  // projected with the max-pool of the level (pool_proj.hip)
  s.pf = pf_ready ? p.pf_pre[s.lvl] : c.arena.alloc(s.pf_bytes);
  if (int rc = fits(c)) return rc;
  if (!pf_ready) {
    GemmArgs g;
    g.A = p.feat[s.lvl]; g.lda = PROJ_CIN[s.si]; g.W = proj[s.si].w; g.ldw = proj[s.si].ldw; g.C = s.pf; g.ldc = s.ldf;
    g.M = (int)(c.nimg * s.hw); g.N = s.r.Cf; g.K = PROJ_CIN[s.si]; g.in_dt = act_dt; g.out_dt = act_dt; g.bias = proj[s.si].b;
    RUN(gemm_launch(g, c.st));
  }
  return observe(c, s.tp + "_proj", s.ins == 16 ? "proj16" : "", s.pf, s.pf_bytes);
}

// coarse match at stride 16: GP match encoder (matcher.py:291-323, f32), coordinate decoder (transformer/__init__.py:30-46),
// to_out and the classification -> flow / certainty conversion into p.flow / p.cert
int Model::coarse_match(const Call& c, const Pass& p, const Scale& s) {
  const bool dry = c.dry; hipStream_t st = c.st;
  const long rows_t = s.M;
  float* tokens = (float*)c.alloc((size_t)rows_t * 1024, 4);
  const size_t gp_mark = c.arena.mark();
  if (int rc = gp_posterior(s.pf, s.ldf, act_dt, c.B, c.sym, c.th, c.tw, gp_w, gp_b, tokens, 1024, c.arena, st, dry))
    return c.arena.overflow ? fits(c) : rc;
  c.arena.release(gp_mark);
  const int ldl = 4104;
  float* logits = (float*)c.alloc((size_t)rows_t * ldl, 4);
  if (int rc = fits(c)) return rc;
  RUN(copy2d_launch(s.pf, s.ldf, act_dt, tokens + 512, 1024, DT_F32, rows_t, 512, st));
  if (int rc = observe(c, "", "tokens16", tokens, (size_t)rows_t * 1024 * 4)) return rc;
  // the shared ViT block (vit.hip) on an f32 residual stream; DINOv2 goes through vit_forward / roma_vit_forward
  VitScratch sc;
  sc.ln = c.ln; sc.ao = c.ao; sc.hid = c.hid; sc.q = c.qbuf; sc.k = c.kbuf; sc.vt = c.vtbuf;
  for (int i = 0; i < 5; ++i) RUN(vit_block_run(tdec[i].pub(), tokens, DT_F32, rows_t, c.ndp, c.T, c.Npt, 8, 128, 1e-5f, act_dt, sc, st));
  const void* zin = tokens;
  if (act_dt != DT_F32) {
    RUN(copy2d_launch(tokens, 1024, DT_F32, c.ln, 1024, act_dt, rows_t, 1024, st));
    zin = c.ln;
  }
  GemmArgs g;
  g.A = zin; g.lda = 1024; g.W = to_out.w; g.ldw = to_out.ldw; g.C = logits; g.ldc = ldl;
  g.M = (int)rows_t; g.N = to_out.N; g.K = 1024; g.in_dt = act_dt; g.out_dt = DT_F32; g.bias = to_out.b;  // 4100: 4097 + 3 zero rows
  RUN(gemm_launch(g, st));
  if (int rc = observe(c, s.tp + "_tokens_gp", "", tokens, (size_t)rows_t * 1024 * 4)) return rc;
  if (int rc = observe(c, s.tp + "_logits", "logits16", logits, (size_t)rows_t * ldl * 4)) return rc;
  RUN(cls_to_flow_launch(logits, ldl, p.flow, p.cert, rows_t, st));
  // tests: the computed coarse match first (so the flips can be counted), then the override (roma_debug_inject)
  if (int rc = observe(c, s.tp + "_gm_flow", "gm_flow16_own", p.flow, s.flow_bytes)) return rc;
  if (!debug || dry) return 0;
  auto inj = [&](const char* nm, float* dst, size_t bytes) -> int {
    auto it = inject.find(nm);
    if (it == inject.end()) return 0;
    ROMA_REQUIRE(it->second.second == bytes, "roma_debug_inject: injected stage has the wrong size for this batch");
    ROMA_CHECK_HIP(hipMemcpyAsync(dst, it->second.first, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
  };
  if (int rc = inj("gm_flow16", p.flow, s.flow_bytes)) return rc;
  if (int rc = inj("gm_cert16", p.cert, s.cert_bytes)) return rc;
  if (int rc = observe(c, "", "gm_flow16", p.flow, s.flow_bytes)) return rc;
  return observe(c, "", "gm_cert16", p.cert, s.cert_bytes);
}

// ConvRefiner input (matcher.py:124-160): [x | x_hat | displacement embedding | local correlation] -> s.d0
int Model::refiner_input(const Call& c, const Pass& p, Scale& s) {
  const bool dry = c.dry; hipStream_t st = c.st;
  const RefinerW& r = s.r;
  s.d0 = c.arena.alloc(s.d_bytes);
  s.d1 = c.arena.alloc(s.d_bytes);
  LocalCorrArgs lc;
  if (r.radius) {
    const long lc_ints = local_corr_ws_ints(c.ndp, s.hs, s.ws, r.radius);  // tile work lists + bin tables + sorted query list (local_corr.h)
    lc.ws = (int*)c.alloc((size_t)lc_ints, 4); lc.ws_bytes = lc_ints * 4;
  }
  if (int rc = fits(c)) return rc;
  if (int rc = observe(c, s.tp + "_flow_before", "", p.flow, s.flow_bytes)) return rc;
  RefinerInputArgs ia;
  ia.feat = s.pf; ia.ldf = s.ldf; ia.flow = p.flow; ia.d = s.d0; ia.ldd = r.Cp; ia.emb_w = r.emb_w; ia.emb_b = r.emb_b;
  ia.B = c.ndp; ia.H = s.hs; ia.W = s.ws; ia.C = r.Cf; ia.E = r.E; ia.Kcorr = r.K; ia.nimg = c.nimg; ia.shift = c.shift;
  ia.disp_scale = (float)(40.0 / 32.0 * p.scale_factor); ia.dt = act_dt;
  RUN(refiner_input_launch(ia, st));
  if (r.radius) {
    lc.f0 = s.pf; lc.f1 = s.pf; lc.warp = p.flow; lc.out = c.at(s.d0, 2 * r.Cf + r.E);
    lc.B = c.ndp; lc.H = s.hs; lc.W = s.ws; lc.C = r.Cf; lc.radius = r.radius; lc.ld0 = s.ldf; lc.ld1 = s.ldf; lc.ldo = r.Cp;
    lc.nimg = c.nimg; lc.f1_shift = c.shift; lc.scale = 1.0f / sqrtf((float)r.Cf); lc.in_dt = act_dt; lc.out_dt = act_dt;
    RUN(local_corr_window_launch(lc, st));
  }
  const bool dual = dbg_dual_slot() >= 0;
  const bool din_small = s.d_bytes <= ((size_t)(dual ? 512 : 64) << 20);  // the debug capture keeps the small scales only
  if (int rc = observe(c, s.tp + "_din", din_small ? std::string(p.tag()) + "_din" + SCALES[s.si] : "", s.d0, s.d_bytes)) return rc;
  if (dual && s.ins == 1)
    if (int rc = observe(c, "", std::string(p.tag()) + "_flowin1", p.flow, s.flow_bytes)) return rc;
  if (!c.tracing) return 0;
  // diagnostic re-reads: are the inputs of the stage still what they were, is d0 stable?
  if (int rc = observe(c, s.tp + "_proj_again", "", s.pf, s.pf_bytes)) return rc;
  if (int rc = observe(c, s.tp + "_flow_again", "", p.flow, s.flow_bytes)) return rc;
  if (int rc = observe(c, s.tp + "_din_again", "", s.d0, s.d_bytes)) return rc;
  if (c.esz != 2 || r.E <= 0) return 0;
  // which part of d deviates: x | x_hat | displacement embedding | rest; which directed pair
  const int cols[5] = {0, r.Cf, 2 * r.Cf, 2 * r.Cf + r.E, r.Cp};
  static const char* const part[4] = {"_din_x", "_din_xhat", "_din_emb", "_din_rest"};
  for (int i = 0; i < 4; ++i)
    if (int rc = observe(c, s.tp + part[i], "", s.d0, 0, s.M, r.Cp, cols[i], cols[i + 1])) return rc;
  for (int b = 0; b < c.ndp; ++b)
    if (int rc = observe(c, s.tp + "_din_pair" + std::to_string(b), "", c.at(s.d0, (long)b * s.hw * r.Cp), 0, s.hw, r.Cp, 0, r.Cp)) return rc;
  return 0;
}

// The nine depthwise 5x5 + 1x1 blocks of a ConvRefiner (matcher.py:92-122).  Block 8 has four forms: narrow scales run the
// fused kernel (refiner_block.hip) and wide ones depthwise + GEMM, each either whole or, with "compose_out_conv", without its
// 1x1, which then lives in the composed out_conv.  *d_last: the buffer out_conv reads; nullptr when the FINAL fused block has
// already added its deltas to p.flow / p.cert.
// (Running the chain over GROUPS of pairs whose ping-pong buffers fit the 256 MiB Infinity Cache was measured in round 3 and is
// slower: 97.4 ms/step whole batch, 98.6 / 99.3 / 101.3 with 400 / 200 / 100 MiB groups - the smaller launches lose more than
// the cache hits win, profiles/r03_v1_ab_attn_map_refiner_groups.log.)
int Model::refiner_chain(const Call& c, const Pass& p, const Scale& s, const void** d_last, bool* composed) {
  const bool dry = c.dry; hipStream_t st = c.st;
  const RefinerW& r = s.r;
  const bool fused = fuse_refiner_blocks && refiner_block_supported(r.Cp, act_dt);
  // the FINAL block's delta buffer is planned whatever "compose_out_conv" is now: the option may change later
  float* delta = fused && (dry || compose_out_conv) ? (float*)c.alloc((size_t)s.M * 4, 4) : nullptr;
  if (int rc = fits(c)) return rc;
  void *dcur = s.d0, *dalt = s.d1;
  *composed = compose_out_conv;
  for (int b = 0; b < 9; ++b) {
    const bool last = b == 8 && compose_out_conv;
    if (last && fused) {
      // depthwise + the composed C -> 3 map on the MFMA, 16 bytes of deltas per pixel instead of a block output, then one
      // small pass that adds them to flow / certainty
      RUN(refiner_block_final_launch(dcur, delta, r.dw_w[b], r.dw_b[b], r.ocf_w, r.Cp, r.ocf_b, c.ndp, s.hs, s.ws, r.Cp, act_dt, st));
      RUN(refiner_apply_delta_launch(delta, p.flow, p.cert, s.M, s.sx, s.sy, st));
      *d_last = nullptr;
      return 0;
    }
    if (fused) {  // dw5x5 + 1x1 in one pass over HBM
      RUN(refiner_block_launch(dcur, dalt, r.dw_w[b], r.dw_b[b], r.pw[b].w, r.pw[b].ldw, r.pw[b].b, c.ndp, s.hs, s.ws, r.Cp, act_dt, st));
      std::swap(dcur, dalt);
      if (int rc = observe(c, s.tp + "_blk" + std::to_string(b), "", dcur, s.d_bytes)) return rc;
      continue;
    }
    RUN(dwconv5x5_launch(dcur, dalt, r.dw_w[b], r.dw_b[b], c.ndp, s.hs, s.ws, r.Cp, act_dt, st));
    if (int rc = observe(c, s.tp + "_dw" + std::to_string(b), "", dalt, s.d_bytes)) return rc;
    if (last) {  // depthwise + BN + ReLU only: its 1x1 lives inside the composed out_conv (RefinerW::oc_w)
      std::swap(dcur, dalt);
      break;
    }
    GemmArgs g;
    g.A = dalt; g.lda = r.Cp; g.W = r.pw[b].w; g.ldw = r.pw[b].ldw; g.C = dcur; g.ldc = r.Cp;
    g.M = (int)s.M; g.N = r.Cp; g.K = r.Cp; g.in_dt = act_dt; g.out_dt = act_dt; g.bias = r.pw[b].b;
    g.n_alg = g.k_alg = r.C;  // FLOPs of the reference's C x C convolution, not of the padded one
    RUN(gemm_launch(g, st));
    if (int rc = observe(c, s.tp + "_blk" + std::to_string(b), "", dcur, s.d_bytes)) return rc;
  }
  *d_last = dcur;
  return 0;
}

// out_conv fused with the flow / certainty update (matcher.py:177-178, 496-506), then the scale's results go out
int Model::refiner_out(const Call& c, const Pass& p, const Scale& s, const void* d_last, bool composed) {
  const bool dry = c.dry; hipStream_t st = c.st;
  const RefinerW& r = s.r;
  if (d_last)
    RUN(refiner_out_launch(d_last, r.Cp, act_dt, composed ? r.oc_w : r.out_w, composed ? r.oc_b : r.out_b, p.flow, p.cert, s.M, r.Cp,
                           s.sx, s.sy, st));
  if (int rc = observe(c, s.tp + "_flow", std::string(p.tag()) + "_flow" + SCALES[s.si], p.flow, s.flow_bytes)) return rc;
  if (int rc = observe(c, s.tp + "_cert", std::string(p.tag()) + "_cert" + SCALES[s.si], p.cert, s.cert_bytes)) return rc;
  if (c.fw && !dry) {  // corresps[ins] = {"flow", "certainty"} (matcher.py:496-512), before the resize to the next scale
    if (c.fw->flow[s.si]) ROMA_CHECK_HIP(hipMemcpyAsync(c.fw->flow[s.si], p.flow, s.flow_bytes, hipMemcpyDeviceToDevice, st));
    if (c.fw->cert[s.si]) ROMA_CHECK_HIP(hipMemcpyAsync(c.fw->cert[s.si], p.cert, s.cert_bytes, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

// Keeps the stride-16 certainty for the epilogue and resizes flow / certainty to the next finer scale (into the alternates)
int Model::next_scale(const Call& c, Pass& p, const Scale& s, float* cert16_keep) {
  const bool dry = c.dry; hipStream_t st = c.st;
  if (s.ins == 16) {  // (one of our own kernels rather than a runtime copy node on the stream)
    if (s.M % 4 == 0) {
      RUN(copy2d_launch(p.cert, s.M, DT_F32, cert16_keep, s.M, DT_F32, 1, (int)s.M, st));
    } else if (!dry) {
      ROMA_CHECK_HIP(hipMemcpyAsync(cert16_keep, p.cert, s.cert_bytes, hipMemcpyDeviceToDevice, st));
    }
  }
  if (s.ins == 1) return 0;
  const int nh = p.H / (s.ins / 2), nw = p.W / (s.ins / 2);
  RUN(resize_bilinear_launch(p.flow, p.flow_alt, c.ndp, s.hs, s.ws, nh, nw, 2, st));
  RUN(resize_bilinear_launch(p.cert, p.cert_alt, c.ndp, s.hs, s.ws, nh, nw, 1, st));
  std::swap(p.flow, p.flow_alt);
  std::swap(p.cert, p.cert_alt);
  return observe(c, s.tp + "_flow_up", "", p.flow, (size_t)c.ndp * nh * nw * 2 * 4);
}

// epilogue (matcher.py:839-850, 891-929): certainty attenuation, warp assembly, symmetric concatenation
int Model::epilogue(const Call& c, const float* flow, const float* cert, const float* cert16_keep, float* warp_out, float* cert_out) {
  const bool dry = c.dry;
  const int Hfin = cfg.upsample_preds ? cfg.upsample_h : cfg.coarse_h, Wfin = cfg.upsample_preds ? cfg.upsample_w : cfg.coarse_w;
  FinalArgs fa;
  fa.flow = flow;
  fa.cert = cert;
  fa.cert16 = cfg.attenuate_cert ? cert16_keep : nullptr;
  fa.warp = warp_out; fa.certainty = cert_out;
  fa.B = c.B; fa.H = Hfin; fa.W = Wfin; fa.h16 = c.th; fa.w16 = c.tw; fa.symmetric = cfg.symmetric;
  RUN(final_epilogue_launch(fa, c.st));
  const size_t px = (size_t)c.B * Hfin * Wfin * (cfg.symmetric ? 2 : 1);
  if (int rc = observe(c, "final_warp", "", warp_out, px * 4 * 4)) return rc;
  return observe(c, "final_cert", "", cert_out, px * 4);
}

// ---------------------------------------------------------------- cached per-image features (encoded.h)
// coarse token grid and the persistent attention buffers: the first allocations of every schedule
void Model::token_grid(Call& c) {
  c.th = cfg.coarse_h / 14; c.tw = cfg.coarse_w / 14; c.T = c.th * c.tw;
  c.Npd = (int)round_up(c.T + 1, 128); c.Npt = (int)round_up(c.T, 128);
  const size_t qkv_elems = std::max((size_t)c.nimg * 16 * c.Npd * 64, (size_t)c.ndp * 8 * c.Npt * 128);
  c.qbuf = c.persist.alloc(qkv_elems * c.esz);
  c.kbuf = c.persist.alloc(qkv_elems * c.esz);
  c.vtbuf = c.persist.alloc(qkv_elems * c.esz);
}

// the transformer scratch of the coordinate decoder, where encode_dino would have allocated it
int Model::decoder_scratch(Call& c) {
  const long rows_t = (long)c.ndp * c.T;
  c.ln = c.alloc((size_t)rows_t * 1024, c.esz);
  c.ao = c.alloc((size_t)rows_t * 1024, c.esz);
  c.hid = c.alloc((size_t)rows_t * 4096, c.esz);
  return fits(c);
}

// In place of proj_head: s.pf [nimg, hw, ldf] = the maps of the B query images, then of the B support images, copied out of
// their packs (the kernels behind read images i and i + shift of ONE buffer; teaching them an index table instead of copying
// is a possible follow-up).  The indices were range-checked by match_encoded.
int Model::gather_head(const Call& c, const Pass& p, Scale& s, const EncodedIn& enc) {
  const bool dry = c.dry;
  s.pf = c.arena.alloc(s.pf_bytes);
  if (int rc = fits(c)) return rc;
  const long seg = pack.off[p.up ? 1 : 0][s.si], slab = pack.bytes[p.up ? 1 : 0][s.si];
  ROMA_REQUIRE(seg >= 0 && (size_t)slab * c.nimg == s.pf_bytes, "roma_match_encoded: the pack layout does not hold this scale");
  for (int i0 = 0; i0 < c.nimg && !dry; i0 += SLAB_MAX) {
    SlabTable t;
    t.n = std::min((int)SLAB_MAX, c.nimg - i0);
    for (int k = 0; k < t.n; ++k) {
      const int i = i0 + k;
      t.src_idx[k] = i < c.B ? enc.idx_a[i] : enc.idx_b[i - c.B];
      t.dst_idx[k] = i;
    }
    RUN(slab_copy_launch(enc.feats + seg, pack.total, s.pf, slab, slab, t, c.st));
  }
  return observe(c, s.tp + "_proj", s.ins == 16 ? "proj16" : "", s.pf, s.pf_bytes);
}

// roma_encode: the projected maps of this chunk's images go to their packs
int Model::scatter_head(const Call& c, const Pass& p, const Scale& s, char* feats) {
  const bool dry = c.dry;
  const long seg = pack.off[p.up ? 1 : 0][s.si], slab = pack.bytes[p.up ? 1 : 0][s.si];
  ROMA_REQUIRE(seg >= 0 && (size_t)slab * c.nimg == s.pf_bytes, "roma_encode: the pack layout does not hold this scale");
  for (int i0 = 0; i0 < c.nimg && !dry; i0 += SLAB_MAX) {
    SlabTable t;
    t.n = std::min((int)SLAB_MAX, c.nimg - i0);
    for (int k = 0; k < t.n; ++k) t.src_idx[k] = t.dst_idx[k] = i0 + k;
    RUN(slab_copy_launch(s.pf, slab, feats + seg, pack.total, slab, t, c.st));
  }
  return 0;
}

// n images through the encoders and the proj heads of one pass (coarse) or both; no decoder.  The images are one array: the
// encoders run with imB == nullptr (B = nimg = n)
int Model::encode_impl(int n, const float* im, const float* im_hr, char* feats, hipStream_t st, bool dry, bool with_up, Arena& arena,
                       Arena& persist) {
  Call c(arena, persist);
  c.B = n; c.nimg = n; c.shift = 0; c.sym = false; c.ndp = 0;
  c.esz = act_dt == DT_F32 ? 4 : 2;
  c.st = st; c.dry = dry;
  arena.reset();
  persist.reset();
  dbg_cur_slot = 0;
  token_grid(c);
  if (int rc = fits(c)) return rc;
  for (int pass = 0; pass < (with_up ? 2 : 1); ++pass) {
    Pass p;
    p.up = pass == 1;
    p.H = p.up ? cfg.upsample_h : cfg.coarse_h; p.W = p.up ? cfg.upsample_w : cfg.coarse_w;
    p.imA = p.up ? im_hr : im;
    const size_t pass_mark = arena.mark();
    if (int rc = encode_vgg(c, p)) return rc;
    if (!p.up)
      if (int rc = encode_dino(c, p)) return rc;
    for (int si = p.up ? 1 : 0; si < 5; ++si) {
      Scale s(c, p, si, ref[si]);
      const size_t scale_mark = arena.mark();
      if (int rc = proj_head(c, p, s)) return rc;
      if (int rc = scatter_head(c, p, s, feats)) return rc;
      arena.release(scale_mark);
    }
    arena.release(pass_mark);
  }
  return 0;
}

// ---------------------------------------------------------------- the driver: passes x scales.  The order of the arena's
// alloc / mark / release calls defines the workspace that roma_finalize plans with a dry run of this same code.
int Model::match_impl(int B, const float* ima, const float* imb, const float* ima_hr, const float* imb_hr,
                      float* warp_out, float* cert_out, hipStream_t st, bool dry, Arena& arena, Arena& persist,
                      const roma_forward_args_t* fw, const EncodedIn* enc) {
  Call c(arena, persist);
  c.B = B; c.nimg = 2 * B; c.shift = B;
  c.sym = fw ? fw->symmetric != 0 : cfg.symmetric != 0;
  c.ndp = c.sym ? 2 * B : B;
  c.esz = act_dt == DT_F32 ? 4 : 2;
  c.st = st; c.dry = dry; c.fw = fw;
  arena.reset();
  persist.reset();
  // determinism trace: checksum of a stage's output, XORed into this sub-batch stream's table
  c.tslot = (&arena == &this->arena) ? 0 : (int)(&arena - side_arena) + 1;
  dbg_cur_slot = c.tslot;  // (per handle: two handles may be in match() from two threads)
  c.tracing = trace_on && !dry;
  if (c.tracing) {
    if (!trace_dev[c.tslot]) {
      ROMA_CHECK_HIP(hipMalloc((void**)&trace_dev[c.tslot], TRACE_MAX * sizeof(unsigned long long)));
      owned.push_back(trace_dev[c.tslot]);
    }
    ROMA_CHECK_HIP(hipMemsetAsync(trace_dev[c.tslot], 0, TRACE_MAX * sizeof(unsigned long long), st));
    trace_n[c.tslot] = 0;
  }
  token_grid(c);

  // ---- results that live across the two passes
  float* cert16_keep = (float*)c.alloc((size_t)c.ndp * c.T, 4);
  // The flow / certainty ping-pong buffers of BOTH passes live outside the per-pass scratch: the coarse pass's finest
  // correspondences seed the upsample pass and the last pass's feed the epilogue where they are - round 5: no device-to-device
  // copies at the end of a pass (2 x 72 MB + 2 x 30 MB per sub-batch and call before).
  float *pp_flow[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}, *pp_cert[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  for (int ps = 0; ps < ((cfg.upsample_preds || (fw && fw->upsample)) ? 2 : 1); ++ps) {
    const size_t px = (size_t)c.ndp * (ps ? cfg.upsample_h : cfg.coarse_h) * (ps ? cfg.upsample_w : cfg.coarse_w);
    for (int i = 0; i < 2; ++i) {
      pp_flow[ps][i] = (float*)c.alloc(px * 2, 4);
      pp_cert[ps][i] = (float*)c.alloc(px, 4);
    }
  }
  if (int rc = fits(c)) return rc;
  float *flow_p1 = nullptr, *cert_p1 = nullptr;    // finest correspondences of the coarse pass (wherever the ping-pong ended)
  float *flow_fin = nullptr, *cert_fin = nullptr;  // ... of the last pass

  const int pass0 = fw ? (fw->upsample ? 1 : 0) : 0, pass1 = fw ? pass0 + 1 : (cfg.upsample_preds ? 2 : 1);
  for (int pass = pass0; pass < pass1; ++pass) {
    Pass p;
    p.up = pass == 1;
    p.H = p.up ? cfg.upsample_h : cfg.coarse_h; p.W = p.up ? cfg.upsample_w : cfg.coarse_w;
    p.imA = (p.up && !fw) ? ima_hr : ima;  // roma_forward hands the pass's own images over as im_a / im_b
    p.imB = (p.up && !fw) ? imb_hr : imb;
    p.scale_factor = sqrt((double)p.H * (double)p.W / (560.0 * 560.0));  // matcher.py:805, 877-881
    if (!p.up && coarse_scale_factor > 0.0) p.scale_factor = coarse_scale_factor;
    if (fw && fw->scale_factor > 0.0) p.scale_factor = fw->scale_factor;
    p.flow = pp_flow[pass][0]; p.cert = pp_cert[pass][0]; p.flow_alt = pp_flow[pass][1]; p.cert_alt = pp_cert[pass][1];

    const size_t pass_mark = arena.mark();
    if (enc) {  // cached features: no encoders; the coarse pass still needs the decoder's transformer scratch
      if (!p.up)
        if (int rc = decoder_scratch(c)) return rc;
    } else {
      if (int rc = encode_vgg(c, p)) return rc;
      if (!p.up)
        if (int rc = encode_dino(c, p)) return rc;
    }
    if (p.up)
      if (int rc = seed_upsample_pass(c, p, flow_p1, cert_p1)) return rc;
    // decoder (matcher.py:395-527)
    for (int si = p.up ? 1 : 0; si < 5; ++si) {
      Scale s(c, p, si, ref[si]);
      const size_t scale_mark = arena.mark();
      if (int rc = enc ? gather_head(c, p, s, *enc) : proj_head(c, p, s)) return rc;
      if (s.ins == 16) {
        const size_t coarse_mark = arena.mark();  // behind s.pf, which the refiner below still reads
        if (int rc = coarse_match(c, p, s)) return rc;
        arena.release(coarse_mark);
      }
      // ConvRefiner (matcher.py:124-179)
      const void* d_last = nullptr;
      bool composed = false;
      if (int rc = refiner_input(c, p, s)) return rc;
      if (int rc = refiner_chain(c, p, s, &d_last, &composed)) return rc;
      if (int rc = refiner_out(c, p, s, d_last, composed)) return rc;
      arena.release(scale_mark);
      if (int rc = next_scale(c, p, s, cert16_keep)) return rc;
    }
    // the finest flow / certainty of this pass stay where they are
    flow_fin = p.flow; cert_fin = p.cert;
    if (!p.up) { flow_p1 = p.flow; cert_p1 = p.cert; }
    arena.release(pass_mark);
  }
  if (fw) return 0;
  return epilogue(c, flow_fin, cert_fin, cert16_keep, warp_out, cert_out);
}

}  // namespace roma
