// Host-side model object behind the C ABI: state-dict intake, BN folding / repacking, device
// workspace (bump arena, planned by a dry run - no allocation inside roma_match) and the
// kernel schedule of RegressionMatcher.match() (romatch/models/matcher.py:779-934).
#pragma once
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/roma_hip.h"
#include "arena.h"
#include "common.h"
#include "encoded.h"
#include "tuning.h"

namespace roma {

extern std::mutex g_peer_mutex;  // guards the one-time load of the sibling library and the mixed-handle count (model.hip)

struct HostTensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  long numel() const {
    long n = 1;
    for (auto d : shape) n *= d;
    return n;
  }
};

struct Lin {  // y = x W^T + b ; W in activation dtype [N][ldw]
  void* w = nullptr;
  float* b = nullptr;
  int N = 0, K = 0, ldw = 0;
};

struct VitBlockW {
  float *ln1w = nullptr, *ln1b = nullptr, *ln2w = nullptr, *ln2b = nullptr, *ls1 = nullptr, *ls2 = nullptr;
  Lin qkv, proj, fc1, fc2;
  roma_vit_block_t pub() const {  // the plain-pointer form vit.h / roma_vit_forward take
    roma_vit_block_t b{};
    b.ln1_w = ln1w; b.ln1_b = ln1b; b.ln2_w = ln2w; b.ln2_b = ln2b; b.ls1 = ls1; b.ls2 = ls2;
    b.qkv_w = qkv.w; b.proj_w = proj.w; b.fc1_w = fc1.w; b.fc2_w = fc2.w;
    b.qkv_b = qkv.b; b.proj_b = proj.b; b.fc1_b = fc1.b; b.fc2_b = fc2.b;
    b.qkv_ldw = qkv.ldw; b.proj_ldw = proj.ldw; b.fc1_ldw = fc1.ldw; b.fc2_ldw = fc2.ldw;
    return b;
  }
};

struct RefinerW {
  int Cf = 0, E = 0, radius = 0, K = 0, C = 0, Cp = 0;
  float *emb_w = nullptr, *emb_b = nullptr;
  float* dw_w[9] = {nullptr};  // [25][Cp], BN folded
  float* dw_b[9] = {nullptr};
  Lin pw[9];
  float *out_w = nullptr, *out_b = nullptr;  // [3][Cp], [3]
  // out_conv composed with the LAST block's 1x1 (two linear maps with nothing in between, matcher.py:92-122, 175-178):
  // oc_w = out_w . pw[8] ([3][Cp], f32), oc_b = out_w . pw[8].b + out_b - the last block then needs no C x C GEMM at all
  float *oc_w = nullptr, *oc_b = nullptr;
  // the same for the FINAL form of the fused narrow blocks (refiner_block.h): 16-bit [8][Cp], rows 0-2 head / 4-6 remainder of
  // oc_w, and the composed bias zero-padded to [Cp]
  void* ocf_w = nullptr;
  float* ocf_b = nullptr;
};

class Model {
 public:
  static constexpr int MAX_STREAMS_DECL = 4;
  roma_config_t cfg{};
  int act_dt = 0;  // DT_F32 / DT_BF16
  // ROMA_MIXED (binary16 build only): DINOv2 runs in bfloat16 in the sibling library (its weights are packed as bfloat16
  // bits here, its patch tokens converted to binary16 behind it), everything else in this build's binary16.
  bool mixed = false;
  bool pack_as_bf16 = false;                                   // upload_act: write bfloat16 bits whatever the build
  void* peer_lib = nullptr;                                    // dlopen handle of libroma_hip.so
  int (*peer_vit_forward)(const roma_vit_args_t*, void*) = nullptr;
  bool finalized = false;
  bool debug = false;
  // The last ConvRefiner block's 1x1 convolution and out_conv are composed into ONE C -> 3 map at pack time (option
  // "compose_out_conv", default 1): 1/9 of the refiners' 1x1 GEMM work and one pass over the block output disappear; the
  // result differs from the two-step evaluation only by rounding (the 16-bit modes no longer round the dropped intermediate)
  bool compose_out_conv = tuning(SW_COMPOSE_OUT) != 0;  // env: A/B runs
  // VGG layers with Cout >= 256 in the 16-bit modes: weight rows in slab-major K order (gemm.h, GemmArgs::conv_korder) - the nine
  // taps of a 64-channel slab back to back, an L2-sized working set per workgroup.  Measured in round 5: L2-miss traffic of the
  // conv GEMM 477 -> 143 MB raw FETCH_SIZE per launch, and the kernel 1.6 % SLOWER (9.31 against 9.15 ms per step, three
  // alternations on one box: profiles/r05_v15_conv_k_order_ab.log) - the misses were Infinity-Cache hits and the tap-major walk
  // reads each pixel's channels as one contiguous run.  OFF by default; ROMA_CONV_KORDER=1 selects it (read before the weights
  // are packed; it changes only the summation order of the K loop).
  // Round 6: ON by default - it is the K order of the patch-resident kernel (conv_patch.hip), which keeps the activation patch of a
  // slab in LDS across the nine taps.  ROMA_CONV_KORDER=0 (or ROMA_CONV_PATCH=0) restores tap-major rows on the implicit GEMM.
  // (The environment half of conv_patch alone: roma_tuning("conv_patch", v) switches kernels, never the weight layout.)
  bool vgg_slab_major = tuning(SW_CONV_KORDER) != 0 && tuning_env(SW_CONV_PATCH) != 0;
  int vgg_korder[12] = {0};
  bool fuse_refiner_blocks = true;  // bf16 mode: fused dw5x5+1x1 kernel at the narrow scales (option "fuse_refiner_blocks")
  // bf16 mode: DINOv2's residual stream in bf16, like the reference's bf16 backbone (encoders.py: dinov2 weights and
  // input are cast to amp_dtype); the decoder transformer keeps f32 (autocast leaves its residual f32).  Option
  // "vit_bf16_residual"; env ROMA_VIT_RES_F32=1 forces the f32 stream for A/B runs.
  bool vit_bf16_residual = true;
  // option "trace": every stage of match() XORs a checksum of its output into a per-stream table (roma_debug_trace)
  bool trace_on = false;
  static constexpr int TRACE_MAX = 1024;
  unsigned long long* trace_dev[MAX_STREAMS_DECL] = {nullptr};
  std::vector<std::string> trace_names[MAX_STREAMS_DECL];
  int trace_n[MAX_STREAMS_DECL] = {0};
  double coarse_scale_factor = 0.0;  // roma_set_option_f; 0 = sqrt(coarse_h * coarse_w / 560^2)
  std::map<std::string, HostTensor> host;

  // packed weights (device)
  Lin vgg[12];  // [0]: first layer as a [64][32] GEMM (27 taps, zero padded); [1..11]: implicit-GEMM convs
  int vgg_cin[12] = {0}, vgg_cout[12] = {0};
  Lin patch;
  float *cls_tok = nullptr, *pos_emb = nullptr;  // pos-embed already resized to the coarse token grid
  VitBlockW dino[24];
  float *dino_nw = nullptr, *dino_nb = nullptr;
  VitBlockW tdec[5];
  Lin to_out;
  float *gp_w = nullptr, *gp_b = nullptr;
  Lin proj[5];  // scales 16,8,4,2,1
  RefinerW ref[5];

  Arena arena;        // per-call scratch
  Arena persist;      // zero-initialised, never aliased (attention q/k/v^T pads, GP basis)
  // Sub-batches on several HIP streams (option "streams" 1..4, "dual_stream" = 2 / 1; env ROMA_STREAMS overrides):
  // pairs are independent, so sub-batch i > 0 runs the same schedule out of its own arenas on side stream i and the
  // partially filled last rounds of one sub-batch's kernels (e.g. 404 GEMM tiles on 256 CUs) are filled by the
  // others' work: +5 % at batch 8 with 2 streams (profiles/r02_final_bench_bf16.json vs r02_final_bench_bf16_1stream.json).
  // ON by default (2 streams) since round 2: results are bit-identical to the single-stream schedule (2 000 / 2 000 bf16
  // stress runs in the GPU suite; the 1-5 % one-ulp deviations of round 1 went away with the GEMM epilogue rewrite,
  // while the library of the commit before it still shows them on the same box - DESIGN.md section 4).
  // Side arenas / streams are created on first use from the sizes planned at roma_finalize.
  static constexpr int MAX_STREAMS = 4;
  int n_streams = 2, streams_ready = 1;
  size_t side_arena_bytes = 0, side_persist_bytes = 0;
  Arena side_arena[MAX_STREAMS - 1], side_persist[MAX_STREAMS - 1];
  hipStream_t side[MAX_STREAMS - 1] = {nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[MAX_STREAMS - 1] = {nullptr};
  std::vector<void*> owned;  // device allocations to free
  std::map<std::string, std::pair<void*, size_t>> dbg;
  int dbg_cur_slot = 0;  // sub-batch slot match_impl is currently enqueueing (ROMA_DEBUG_DUAL_SLOT diagnostics)
  // debug mode only (roma_debug_inject): device buffers that REPLACE a named intermediate of the next match() calls.
  // "gm_flow16" [ndp, T, 2] / "gm_cert16" [ndp, T] f32 overwrite the output of cls_to_flow_refine, so a parity test can
  // pin the (discontinuous) coarse arg-max to the oracle's and hold everything downstream to a continuous bound.
  std::map<std::string, std::pair<void*, size_t>> inject;
  int debug_inject(const char* name, const void* host, size_t bytes);

  ~Model();
  int set_tensor(const char* name, int ndim, const int64_t* shape, const void* data, int is_int64);
  int finalize();
  int match(int B, const float* ima, const float* imb, const float* ima_hr, const float* imb_hr, float* warp,
            float* cert, hipStream_t st);
  int forward(int B, const float* ima, const float* imb, const roma_forward_args_t* fw, hipStream_t st);
  // ---- cached per-image features (encoded.h): encoders + proj heads once per image, then match() on pairs of cached images
  PackLayout pack;  // fixed at finalize
  int encode(int N, const float* images, const float* images_hr, void* feats, long feats_bytes, hipStream_t st);
  int match_encoded(int P, const void* feats, long feats_bytes, int N, const int* idx_a, const int* idx_b, float* warp, float* cert,
                    hipStream_t st);

 private:
  // the cache a match() schedule reads its projected features from: query image of pair i = idx_a[i], support = idx_b[i] (HOST
  // arrays, range-checked by match_encoded)
  struct EncodedIn {
    const char* feats = nullptr;
    const int *idx_a = nullptr, *idx_b = nullptr;
  };
  int ensure_side_streams(int n);
  int match_streams(int B, const float* ima, const float* imb, const float* ima_hr, const float* imb_hr, float* warp,
                    float* cert, hipStream_t st, const EncodedIn* enc = nullptr);
  int check_contract();
  int pack_weights();
  int load_peer();
  int dbg_save(const char* name, const void* p, size_t bytes, hipStream_t st);
  template <typename F> int upload_f32(const std::vector<float>& v, F** out);
  int upload_act(const std::vector<float>& v, void** out);
  int make_lin(const std::vector<float>& w, const std::vector<float>* b, int N, int K, Lin* out);

  // ---- the match() schedule (model.hip): a driver over the passes and scales, and its stages
  struct Call;   // what one call shares: sizes, stream, arenas, trace slot, token grid, transformer scratch
  struct Pass;   // one pass (coarse / upsample): resolution, images, feature pyramid, current flow / certainty
  struct Scale;  // one decoder scale of a pass: geometry, refiner weights, projected features, refiner buffers
  // fw != nullptr: ONE pass (roma_forward) - per-scale outputs copied out, no epilogue
  // enc != nullptr: no encoders and no proj heads - every scale's projected features are gathered from the cache
  int match_impl(int B, const float* ima, const float* imb, const float* ima_hr, const float* imb_hr, float* warp,
                 float* cert, hipStream_t st, bool dry, Arena& arena, Arena& persist, const roma_forward_args_t* fw = nullptr,
                 const EncodedIn* enc = nullptr);
  // encoders + proj heads of n images (both passes with `with_up`), scattered into the packs starting at `feats`
  int encode_impl(int n, const float* im, const float* im_hr, char* feats, hipStream_t st, bool dry, bool with_up, Arena& arena,
                  Arena& persist);
  void token_grid(Call& c);
  int decoder_scratch(Call& c);
  int gather_head(const Call& c, const Pass& p, Scale& s, const EncodedIn& enc);
  int scatter_head(const Call& c, const Pass& p, const Scale& s, char* feats);
  int fits(const Call& c);
  int observe(const Call& c, const std::string& trace_name, const std::string& dbg_name, const void* p, size_t bytes,
              long rows = 0, int ld = 0, int c0 = 0, int c1 = 0);
  int encode_vgg(const Call& c, Pass& p);
  int encode_dino(Call& c, Pass& p);
  int seed_upsample_pass(const Call& c, const Pass& p, const float* flow_p1, const float* cert_p1);
  int proj_head(const Call& c, const Pass& p, Scale& s);
  int coarse_match(const Call& c, const Pass& p, const Scale& s);
  int refiner_input(const Call& c, const Pass& p, Scale& s);
  int refiner_chain(const Call& c, const Pass& p, const Scale& s, const void** d_last, bool* composed);
  int refiner_out(const Call& c, const Pass& p, const Scale& s, const void* d_last, bool composed);
  int next_scale(const Call& c, Pass& p, const Scale& s, float* cert16_keep);
  int epilogue(const Call& c, const float* flow, const float* cert, const float* cert16_keep, float* warp_out, float* cert_out);
};

}  // namespace roma
