/* libroma_hip - C ABI of the MI355X-native RoMa dense-matching path.
 *
 * The reference (Parskatt/RoMa) is pure Python; the interfaces this library replaces are
 *   - romatch/models/model_zoo/__init__.py:31-93  roma_outdoor / roma_indoor factories
 *                                                 -> roma_create / roma_set_tensor / roma_finalize
 *   - romatch/models/model_zoo/roma_models.py:204 strict load_state_dict       -> roma_set_tensor + roma_finalize
 *   - romatch/models/matcher.py:779-934           RegressionMatcher.match()    -> roma_match
 *   - romatch/models/matcher.py:585-596, 631-670  forward / forward_symmetric / extract_backbone_features -> roma_forward
 *   - romatch/utils/local_correlation.py:22-35    local_corr.local_corr(...) (external fused-local-corr wheel)
 *                                                 -> roma_op_local_corr (plugin signature),
 *                                                    roma_op_local_corr_window (what local_correlation():77-143 needs)
 * plus per-operator entry points so that every kernel can be parity-tested alone.
 *
 * Conventions: plain pointers and sizes only; all tensor pointers are DEVICE pointers unless
 * stated otherwise; `stream` is a hipStream_t passed as void* (NULL = default stream); calls are
 * asynchronous on that stream; return 0 on success, negative on error (text: roma_last_error()).
 * One handle per device, one in-flight roma_match per handle (the reference's single-caller model).
 */
#ifndef ROMA_HIP_H
#define ROMA_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct roma_model* roma_handle_t;

/* arithmetic / storage type of activations.  The 16-bit format is a property of the library BUILD: libroma_hip.so stores
 * bfloat16 and accepts ROMA_F32 / ROMA_BF16; libroma_hip_f16.so (same sources, -DROMA_H16_F16) stores IEEE binary16 - the
 * reference's default amp_dtype (model_zoo/__init__.py:37) - and accepts ROMA_F32 / ROMA_F16.  The other code is an error
 * (ROMA_ERR_ARG), never a reinterpretation.  roma_h16_format() returns the code of the loaded library. */
enum { ROMA_F32 = 0, ROMA_BF16 = 1, ROMA_F16 = 2,
       /* the precision policy the reference's own timing script runs (tests/test_roma_upsample_inference_time.py:36-45):
        * amp_dtype = bfloat16 reaches DINOv2 only (model_zoo/roma_models.py:183-188); the VGG pyramid, the decoder and the
        * refiners keep binary16 (encoders.py:7, matcher.py:46,341).  Accepted by libroma_hip_f16.so, which loads
        * libroma_hip.so from its own directory and runs DINOv2 there through roma_vit_forward. */
       ROMA_MIXED = 3 };
int roma_h16_format(void);
enum { ROMA_ERR_ARG = -1, ROMA_ERR_HIP = -2, ROMA_ERR_STATE = -3 };

typedef struct {
  int coarse_h, coarse_w;     /* multiples of 14 (DINOv2 patch; roma_models.py:58-59), e.g. 560, 518, 672 */
  int upsample_h, upsample_w; /* any size >= 16 (0 = no upsample pass); used when upsample_preds != 0 */
  int symmetric;              /* matcher.py:801   */
  int upsample_preds;         /* matcher.py:836   */
  int attenuate_cert;         /* matcher.py:839   */
  int precision;              /* ROMA_F32 (exact f32 MFMA; CPU-oracle parity), the library's 16-bit code, or - binary16 build
                                 only - ROMA_MIXED: DINOv2 in bfloat16, everything else in binary16 (the policy of
                                 tests/test_roma_upsample_inference_time.py:36-45 + roma_models.py:183-188) */
  int max_batch;              /* largest number of image pairs per roma_match call                 */
  int device;                 /* HIP device ordinal                                                */
} roma_config_t;

const char* roma_last_error(void);
const char* roma_version(void);
/* ABI stamp of the structures that cross the library boundary BETWEEN the two builds (roma_vit_args_t, roma_vit_block_t:
 * a ROMA_MIXED handle of libroma_hip_f16.so calls roma_vit_forward of libroma_hip.so): ROMA_ABI_VERSION * 100000 +
 * sizeof(roma_vit_args_t).  The sibling is refused unless the stamps are equal. */
#define ROMA_ABI_VERSION 6
int roma_abi_stamp(void);
/* the 16-bit format as THIS library's own internal calls see it (== roma_h16_format() unless another library's symbols
 * interpose: the sibling check of ROMA_MIXED and tests/test_cpu_oracle.py use it) */
int roma_self_check(void);

/* ---- DINOv2 ViT-L/14 as a stand-alone entry (dinov2.py:192-237: patch embed, cls + position embedding, 24 pre-norm
 * blocks, final LayerNorm, patch tokens).  Everything is a DEVICE pointer prepared by the caller: weights in THIS
 * library's 16-bit format (w) or f32 (everything else; LayerScale already folded into proj / fc2), workspace of the
 * sizes given below.  act = ROMA_F32 or this library's 16-bit code.  Used by ROMA_MIXED handles of the other build. */
typedef struct {
  const float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
  const float *ls1, *ls2;                    /* per-channel LayerScale applied in the epilogue, or NULL when folded */
  const void *qkv_w, *proj_w, *fc1_w, *fc2_w; /* [N][ldw], K-contiguous */
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;
  int qkv_ldw, proj_ldw, fc1_ldw, fc2_ldw;
} roma_vit_block_t;

typedef struct {
  int B, H, W;                      /* B pairs = 2B images: im_a[B,3,H,W], im_b[B,3,H,W] f32 (H, W multiples of 14); im_b == NULL
                                       (ABI 6): B images, all at im_a - read "B" for "2B" below */
  int act;                          /* ROMA_F32 or the library's 16-bit code */
  int bf16_residual;                /* 16-bit mode: residual stream in 16 bits (the reference's bf16 backbone) */
  const float *im_a, *im_b;
  const void* patch_w;              /* [1024][patch_ldw], k = c*196 + ky*14 + kx, zero padded */
  const float* patch_b;
  int patch_ldw;
  const float *cls_tok, *pos_emb;   /* [1024], [1 + T][1024] (already resized to the token grid) */
  const roma_vit_block_t* blocks;   /* HOST array */
  int nblocks;
  const float *norm_w, *norm_b;
  /* workspace, T = (H/14)(W/14), rows = 2B (T + 1), Npad = T + 1 rounded up to 128, e = bytes per activation element:
   * col [2B T patch_ldw] e | pt [2B T 1024] f32 | x [rows 1024] f32 | xs [rows 1024] 2 B (16-bit residual only) |
   * ln, ao [rows 1024] e | hid [rows 4096] e | q, k, vt [2B 16 Npad 64] e, zero-initialised once and never written by
   * anyone else (the padding rows must stay zero) */
  void *col, *pt, *x, *xs, *ln, *ao, *hid, *q, *k, *vt;
  void* feat_out;                   /* [2B, T, 1024] patch tokens (x_norm_patchtokens), activation dtype */
} roma_vit_args_t;
int roma_vit_forward(const roma_vit_args_t* a, void* stream);
/* bfloat16 bits -> this library's 16-bit format (the hand-over of a ROMA_MIXED handle), n elements */
int roma_op_convert_from_bf16(const void* in_bf16, void* out_h16, long n, void* stream);

int roma_create(const roma_config_t* cfg, roma_handle_t* out);
/* name: a key of the reference's matcher state-dict, or "dinov2." + a key of the DINOv2 dict.
 * data: HOST pointer to float32 (int64 for num_batches_tracked, ignored). The library copies. */
int roma_set_tensor(roma_handle_t h, const char* name, int ndim, const int64_t* shape, const void* data, int is_int64);
/* strict key/shape check (as load_state_dict strict=True), BN folding, repacking, upload. */
int roma_finalize(roma_handle_t h);
/* mutable attributes of RegressionMatcher (README.md:82-90): "symmetric", "upsample_preds", "attenuate_cert", "debug";
 * tuning: "fuse_refiner_blocks" (default 1; 0 = separate dwconv + GEMM kernels at every scale),
 *         "compose_out_conv" (default 1: the last ConvRefiner block's 1x1 convolution and out_conv - two linear maps with
 *         nothing in between, matcher.py:92-122, 175-178 - are evaluated as the ONE C -> 3 map composed at roma_finalize;
 *         0 = the reference's two steps.  The results differ by rounding only),
 *         "vit_bf16_residual" (bf16 mode only, default 1: DINOv2 residual stream in bf16 like the reference's bf16
 *         backbone, encoders.py; 0 = keep it in f32),
 *         "streams" (1..4, default 2) / "dual_stream" (1 = 2 streams, 0 = 1): run a batch of >= 2 pairs as sub-batches on
 *         several HIP streams (+5 % at batch 8 with 2; side workspaces are allocated on first use; results are
 *         bit-identical to the single-stream schedule - DESIGN.md section 4) */
int roma_set_option(roma_handle_t h, const char* key, int value);
/* "coarse_scale_factor": the displacement-embedding scale of the COARSE pass, sqrt(h_resized * w_resized / 560^2) of the
 * matcher's configured resolution (matcher.py:805) - it differs from the handle's own resolution only when the caller
 * feeds tensors of another size than the matcher was configured for (matcher.py:822-826).  0 = derive from the handle. */
int roma_set_option_f(roma_handle_t h, const char* key, double value);
/* im_*: [B,3,H,W] float32 normalised images (already on the device). *_hr may be NULL when
 * upsample_preds == 0.  warp_out: [B,Ho,2*Wo,4] (symmetric) or [B,Ho,Wo,4]; cert_out: [B,Ho,2*Wo] / [B,Ho,Wo]. */
int roma_match(roma_handle_t h, int B, const float* im_a, const float* im_b, const float* im_a_hr,
               const float* im_b_hr, float* warp_out, float* cert_out, void* stream);
/* ---- cached per-image features for image sets: encode every image ONCE, then match any pairs of the encoded images.
 * Everything the decoder reads of an image is its projected feature maps (the proj heads of scales 16, 8, 4, 2, 1 of the coarse
 * pass and of 8, 4, 2, 1 of the upsample pass), so one image's "pack" holds exactly those: per pass and scale [h_s * w_s, ldf] in
 * the handle's activation type, ldf = C_s rounded up to 8 with C = 512, 512, 256, 64, 9, every segment on a 256-byte boundary
 * (coarse 16, 8, 4, 2, 1, then upsample 8, 4, 2, 1 when the handle has an upsample resolution).  The layout is fixed at
 * roma_finalize; roma_amd/encoded.py::pack_layout restates it.  About 120 MB per image in the 16-bit modes at 560 -> 864 and 240 MB
 * in f32.  The raw VGG / DINOv2 pyramids are NOT cached (roma_forward's feat[] still computes them per call).
 * The caller owns the feature buffer: N packs back to back, 16-byte aligned device memory.
 *
 * roma_encoded_bytes: bytes of one pack for this handle; -1 before roma_finalize. */
long roma_encoded_bytes(roma_handle_t h);
/* images [N,3,coarse_h,coarse_w] f32; images_hr [N,3,upsample_h,upsample_w] f32 or NULL (then only the coarse part of every pack
 * is written and the packs serve upsample_preds == 0 only - the caller keeps track).  Runs the VGG19-BN pyramid, DINOv2 and the
 * proj heads of the coarse pass, and with images_hr the pyramid and the proj heads of the upsample pass.  Any N >= 1; images are
 * processed in chunks of 2 * max_batch out of the workspace planned at roma_finalize, on the caller's stream.  feats_bytes must
 * be N * roma_encoded_bytes(h). */
int roma_encode(roma_handle_t h, int N, const float* images, const float* images_hr, void* feats, long feats_bytes, void* stream);
/* roma_match for the P pairs (idx_a_host[i], idx_b_host[i]) of the N encoded images in feats: the same schedule with the encoders
 * and the proj heads left out - one gather kernel per scale copies the 2P projected maps (the P query images, then the P support
 * images) to where the proj head would have written them, everything behind it runs unchanged.  Same options ("symmetric",
 * "upsample_preds", "attenuate_cert", "compose_out_conv", "dual_stream" / "streams"), same output layout and - for packs written by
 * roma_encode of the same handle configuration - the same bits as roma_match on those images.  P <= max_batch.  The indices are
 * HOST arrays, range-checked against N before anything is enqueued: a bad index, a feats_bytes other than
 * N * roma_encoded_bytes(h) or P > max_batch return an error with nothing launched. */
int roma_match_encoded(roma_handle_t h, int P, const void* feats, long feats_bytes, int N, const int* idx_a_host,
                       const int* idx_b_host, float* warp_out, float* cert_out, void* stream);
/* ONE decoder pass with its per-scale correspondences exposed: RegressionMatcher.forward / forward_symmetric in eval mode
 * (matcher.py:631-670 -> Decoder.forward, matcher.py:395-527: corresps[s] = {"flow", "certainty"} for s = 16, 8, 4, 2, 1) and
 * extract_backbone_features (matcher.py:585-596).  upsample = 0: the coarse pass over images at the handle's coarse resolution
 * (scales 16 .. 1); upsample = 1: the upsample pass (matcher.py:870-889: scales 8 .. 1, no DINOv2 / GP) over images at the
 * handle's upsample resolution, seeded with batch["corresps"] = (seed_flow, seed_cert) of ANY resolution, which Decoder.forward
 * resizes bilinearly to the stride-8 grid (matcher.py:423-435).  symmetric selects forward_symmetric (decoder batch Bd = 2B:
 * A->B then B->A) or forward (Bd = B).  Outputs are channels-last f32, the caller permutes: flow[i] [Bd, h_s, w_s, 2] (x, y),
 * cert[i] [Bd, h_s, w_s] logits, i = 0 .. 4 for s = 16, 8, 4, 2, 1 (h_16 = H / 14, h_s = H / s otherwise); any pointer may be
 * NULL (that output is skipped; index 0 is ignored in an upsample pass).  feat[i]: the two images' feature pyramid
 * [2B, h_s, w_s, C_s] (C = 1024, 512, 256, 128, 64) in the handle's activation type (f32, or the library's 16-bit format).
 * Runs on the caller's stream, one sub-batch (no stream split); B <= max_batch. */
typedef struct {
  int upsample;
  int symmetric;
  double scale_factor;      /* ConvRefiner displacement scale (matcher.py:805, 877-881); forward()'s default is 1 */
  const float* seed_flow;   /* upsample pass only: [Bd, seed_h, seed_w, 2] f32 */
  const float* seed_cert;   /* [Bd, seed_h, seed_w] f32 logits */
  int seed_h, seed_w;
  float* flow[5];
  float* cert[5];
  void* feat[5];
} roma_forward_args_t;
int roma_forward(roma_handle_t h, int B, const float* im_a, const float* im_b, const roma_forward_args_t* a, void* stream);
/* debug stage capture (enabled by roma_set_option(h,"debug",1)): copies a named intermediate to HOST memory.
 * Returns the number of bytes available when dst == NULL. */
long roma_debug_fetch(roma_handle_t h, const char* name, void* dst_host, long nbytes);
/* debug mode only: replace a named intermediate of the following roma_match calls by the HOST buffer given here
 * (copied; src_host == NULL removes the override).  Stages: "gm_flow16" [b, h16*w16, 2] and "gm_cert16" [b, h16*w16]
 * f32, b = decoder batch - the output of cls_to_flow_refine (utils/utils.py:300-322), whose arg-max is discontinuous:
 * parity tests of the reduced-precision mode inject the oracle's coarse match and bound everything downstream. */
int roma_debug_inject(roma_handle_t h, const char* name, const void* src_host, long nbytes);
/* determinism trace (roma_set_option(h, "trace", 1)): every stage of the following roma_match calls XORs an
 * order-independent 64-bit checksum of its output into a table, one table per sub-batch stream (slot 0 = the caller's
 * stream).  Returns the number of entries of the last call (sums_host == NULL: count only); names_host receives the stage
 * names, newline separated.  tools/stress_streams.py --trace uses it to name the FIRST stage that differs between runs. */
long roma_debug_trace(roma_handle_t h, int slot, unsigned long long* sums_host, long max_entries, char* names_host,
                      long names_bytes);
int roma_destroy(roma_handle_t h);
/* Per-launch HIP-event timing of the dominant kernels (bench.py roofline pass). roma_profile_report writes a JSON
 * object {kernel: {calls,total_ms,work,unit}} (work = algorithmic FLOPs or bytes); returns bytes needed when buf==NULL. */
/* process-wide kernel-selection switches for A/B measurements and tests (not needed for normal use).  The one list of keys,
 * environment variables, defaults and meanings is the table in roma_amd/csrc/tuning.hip, printed in INTEGRATION.md section 2
 * and by roma_tuning_describe.  A value below the key's lowest override value (-1 for every key) clears the override: the
 * environment variable of the row, else its default, holds again.  Every alternative computes the same values - the stencil /
 * block kernels, "gemm8p_sched", "ws1x1", "conv_patch" and "gp_col_leader" (also the time-out path of its hand-off) bit for bit,
 * "gp_col" to f32 rounding, "gemm8p_walk" and "gemm8p_maxwg" change only the order and number of workgroups - except that
 * "attn_exp2" assumes q pre-scaled by log2 e and the "gemm_dbg" experiment bits produce wrong outputs by design. */
int roma_tuning(const char* key, int value);
/* The switch table as a JSON array, one object per row in table order: {"key": str | null, "env": str | null, "default": n,
 * "override": n | null, "value": n, "doc": str}; "value" is what a launch would see now.  Size query
 * as roma_profile_report (buf == NULL: bytes needed).  Touches no device; each library describes its own table. */
long roma_tuning_describe(char* buf, long nbytes);
/* measuring tool (tools/bench_gemm_ablation.py): after a GEMM launched with the "gemm_dbg" trace bit (32768), copies the
 * phase time stamps [workgroup < 16][wave group][K tile < 256][phase] (low 32 bits of s_memtime at each phase's first
 * barrier release) to the host; returns the number of bytes written. */
long roma_debug_gemm_trace(unsigned int* dst_host, long nbytes);
int roma_profile_enable(int on);
long roma_profile_report(char* buf, long nbytes);

/* ---- operator entry points (dt: ROMA_F32 or the library's 16-bit code, ROMA_BF16 / ROMA_F16) ------------ */

/* Drop-in for local_corr.local_corr(feature0[B,HW,C], feature1[B,H,W,C], warp[B,HW,K,2], mode, normalized_coords=True)
 * -> out[B,HW,K]   (local_correlation.py:26-32).  feature0 is expected pre-scaled.  nearest = 0: mode "bilinear"; 1: mode
 * "nearest" (the sample_mode the reference threads through local_correlation.py:19,30,85: the pixel at nearbyint of the
 * un-normalised coordinate, zero outside the image - F.grid_sample(mode="nearest", align_corners=False)). */
int roma_op_local_corr(const void* feature0, const void* feature1, const float* warp, void* out, int B, int H, int W,
                       int C, int K, int nearest, int dt_in, int dt_out, void* stream);
/* Window form: warp is the centre coordinate [B,HW,2]; taps = (2r+1)^2 one-pixel steps; scale multiplies the
 * result (1/sqrt(C) when feature0 is not pre-scaled); out row stride ldo >= K. */
int roma_op_local_corr_window(const void* feature0, const void* feature1, const float* warp, void* out, int B, int H,
                              int W, int C, int radius, float scale, long ldo, int dt_in, int dt_out, void* stream);
/* The same operator on caller-owned device scratch (the plain entry allocates stream-ordered scratch per call): ws holds at
 * least roma_op_local_corr_window_workspace(B, H, W, radius) bytes - 0 for the radii that need none: ws may then be
 * NULL - and needs no initialisation: the call writes every word it reads. */
long roma_op_local_corr_window_workspace(int B, int H, int W, int radius);
int roma_op_local_corr_window_ws(const void* feature0, const void* feature1, const float* warp, void* out, int B, int H,
                                 int W, int C, int radius, float scale, long ldo, int dt_in, int dt_out, void* ws,
                                 long ws_bytes, void* stream);

/* C[M,N] = act(A[M,K] W[N,K]^T + bias) * scale + res   (batched with element strides; any pointer may be NULL) */
int roma_op_gemm(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, int batch,
                 long sA, long sW, long sC, const float* bias, const float* scale, const float* res, long ldr,
                 int act, float alpha, int dt_in, int dt_out, void* stream);
/* 3x3 conv (pad 1) as implicit GEMM on NHWC input: out[B,H,W,Cout] = relu?(conv(in[B,H,W,Cin], w[Cout][9*Cin]) + bias) */
int roma_op_conv3x3(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                    int relu, int dt, void* stream);
/* The same convolution with the weight rows in SLAB-MAJOR K order, w[Cout][k], k = ((ci / 64) * 9 + ky * 3 + kx) * 64 + ci % 64
 * (Cin % 64 == 0) - how the model packs the VGG layers with Cout >= 256 in the 16-bit modes.  Those run on the patch-resident
 * kernel (conv_patch.hip: the activation patch + halo of a 64-channel slab stays in LDS for all nine taps, only the weights
 * stream; roma_tuning("conv_patch", 0) selects the plain implicit GEMM instead - bit-identical results). */
int roma_op_conv3x3_slab(const void* in, const void* w, const float* bias, void* out, int B, int H, int W, int Cin, int Cout,
                         int relu, int dt, void* stream);
/* Multi-head attention from a packed qkv activation [B*N, 3*heads*hd] (f32): out[B*N, heads*hd].
 * Workspace q,k,vt must hold B*heads*Npad*hd elements each, Npad = roundup(N,128), zero-initialised.
 * roma_op_qkv_scatter_gemm writes the N tokens of every image only: the rows N .. Npad of q / k and the columns N .. Npad of
 * V^T keep their zeros (roma_op_attention itself does not read them into a result). */
int roma_op_attention(const void* q, const void* k, const void* vt, void* out, int B, int heads, int N, int npad, int hd,
                      int dt_in, int dt_out, void* stream);
int roma_op_qkv_scatter_gemm(const void* A, const void* W, const float* bias, void* q, void* k, void* vt, int B, int N,
                             int npad, int heads, int hd, int K, int dt_in, int dt_out, void* stream);
int roma_op_layernorm(const float* x, const float* w, const float* b, void* out, long M, int D, float eps, int dt_out,
                      void* stream);
/* LayerNorm with a typed input (dt_in 0 = f32, 1 = bf16; bf16 input implies bf16 output) - the bf16 residual stream of
 * the DINOv2 blocks in bf16 mode (reference: encoders.py casts the backbone and its input to amp_dtype). */
int roma_op_layernorm_dt(const void* x, int dt_in, const float* w, const float* b, void* out, long M, int D, float eps,
                         int dt_out, void* stream);
/* bf16 GEMM with a bf16 residual: C = bf16( res + scale * (A W^T + bias) ), C may alias res (the in-place residual
 * update x += ls * linear(y) of a transformer block, dinov2.py NestedTensorBlock).  N, ldc, ldr multiples of 8. */
int roma_op_gemm_res_bf16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K,
                          const float* bias, const float* scale, const void* res, long ldr, void* stream);
/* Batched SPD solve  (A + 0 ) X = F  via blocked Cholesky: A [batch,n,n] f32 (destroyed), Ft [batch, d, n] = F^T,
 * overwritten by X^T.  Workspaces: LT [batch,n,n], Linv/LinvT [batch, n/64, 64, 64].  n multiple of 64.
 * Augmented layout (what the GP uses): Ft == A + n * n, i.e. ONE (n + d) x n matrix per item with the right-hand sides right
 * behind A (items (n + d) * n floats apart when batch > 1) - the forward substitution then runs inside the factorisation,
 * one launch per 64-column block (chol_col.hip; roma_tuning("gp_col", 0) selects the right-looking launch chain instead). */
int roma_op_cholesky_solve_t(float* A, float* Ft, float* LT, float* Linv, float* LinvT, int n, int d, int batch,
                             void* stream);
/* GP.forward (matcher.py:291-323) with the cosine kernel (matcher.py:191-200, T = 0.2) and sigma_noise = 0.1:
 *   mu[i] = K(x_i, y_i) (K(y_i, y_i) + 0.1 I)^-1 cos(8 pi (pos_w . grid + pos_b))
 * x, y: [b, h*w, 512] channels-last stride-16 features (dt), pos_w [512,2], pos_b [512] f32 (decoder.gps.16.pos_conv),
 * mu: [b, h*w, 512] f32.  Always evaluated in f32 (Gram matrices via exact-f32 MFMA when dt = ROMA_F32, blocked
 * Cholesky, two triangular solves); scratch is stream-ordered. */
int roma_op_gp(const void* x, const void* y, const float* pos_w, const float* pos_b, float* mu, int b, int h, int w, int dt,
               void* stream);
int roma_op_cls_to_flow(const float* logits, long ld, float* flow, float* cert, long M, void* stream);
int roma_op_resize_bilinear(const float* in, float* out, int B, int Hin, int Win, int Hout, int Wout, int nc,
                            void* stream);
/* The ConvRefiner input writer = F.grid_sample warp + concat (matcher.py:132-148, 166), one pass:
 *   d[b,p,:] = [ x[b,p,0:C] | bilinear_zeropad(y[(b+shift) % nimg], flow[b,p]) (align_corners=False) |
 *                emb_w . (disp_scale * (flow[b,p] - grid[p])) + emb_b (E values) | Kcorr columns left untouched (local
 *                correlation writes them) | zeros up to ldd ]
 * feat: projected features of all nimg images [nimg, H*W, ldf] (x = image b, y = image (b+shift) % nimg), flow [B,H*W,2]
 * f32 normalised (x,y), emb_w [E,2], emb_b [E] f32, disp_scale = 40/32 * scale_factor. */
int roma_op_refiner_input(const void* feat, long ldf, const float* flow, void* d, long ldd, const float* emb_w,
                          const float* emb_b, int B, int H, int W, int C, int E, int Kcorr, int nimg, int shift,
                          float disp_scale, int dt, void* stream);
int roma_op_dwconv5x5(const void* in, void* out, const float* w, const float* bias, int B, int H, int W, int Cp, int dt,
                      void* stream);
/* One fused ConvRefiner block (matcher.py:88-117 create_block): out = conv1x1(relu(bn(dwconv5x5(in)))), BN folded into
 * dw_w/dw_b.  bf16 only, Cp in {24, 144} (the narrow scales); in/out [B,H,W,Cp] must not alias; pw bf16 [Cp][Cp],
 * pw_b f32 [Cp]. */
int roma_op_refiner_block(const void* in, void* out, const float* dw_w, const float* dw_b, const void* pw,
                          const float* pw_b, int B, int H, int W, int Cp, int dt, void* stream);
/* The LAST block of a narrow ConvRefiner with its 1x1 composed with out_conv (two linear maps back to back, matcher.py:92-122,
 * 175-178; "compose_out_conv"): delta[pixel] = {d flow x, d flow y, d certainty, 0} (f32 [B*H*W][4]) instead of a block output.
 * pw_final: 16-bit [8][Cp], rows 0-2 = 16-bit head and rows 4-6 = 16-bit remainder of the composed [3][Cp] weights (rows 3, 7
 * zero); bias_final f32 [Cp] (composed bias in [0, 3), zeros behind).  bf16 / f16 only, Cp in {24, 144}. */
int roma_op_refiner_block_final(const void* in, float* delta, const float* dw_w, const float* dw_b, const void* pw_final,
                                const float* bias_final, int B, int H, int W, int Cp, int dt, void* stream);
/* flow[i] += (sx, sy) * delta[i].xy, cert[i] += delta[i].z (the deltas above; flow [M][2], cert [M], f32) */
int roma_op_refiner_apply_delta(const float* delta, float* flow, float* cert, long M, float sx, float sy, void* stream);
/* Gaussian KDE of sampled matches (romatch/utils/kde.py:4-12; RegressionMatcher.sample, matcher.py:598-629):
 * density[i] = sum_j exp(-|x_i - x_{j*down}|^2 / (2 std^2)), x: DEVICE [n,4] f32.  half_inputs != 0 rounds the
 * coordinates to fp16 first (the reference's x.half()); accumulation is f32. */
int roma_op_kde(const float* x, long n, int down, float std, int half_inputs, float* density, void* stream);
/* RegressionMatcher.match_keypoints (matcher.py:732-773), all pointers DEVICE:
 * sample_warp_at: xa_to_b[i] = bilinear(warp[..., 2:4], xa[i]), cert_a[i] = bilinear(cert, xa[i])  (zeros padding,
 *   align_corners=False); warp [H,W,4] f32, cert [H,W] f32, xa [n,2] normalised (x,y).
 * mutual_nn: match_b[i] = j if b[j] is the nearest neighbour of a[i], a[i] is at the column-minimum distance of
 *   b[j], cert_a[i] > cert_th (cert_a may be NULL) and |a[i]-b[j]| < max_dist; else -1.  Row ties resolve to the
 *   lowest j.  ws_a / ws_b: 8*na / 8*nb byte workspaces.
 * mutual_nn_count / mutual_nn_fill: the tie-complete form, i.e. torch.nonzero of the reference's mask
 *   (D == row min) * (D == column min) * (cert > th) * (D < max_dist) (matcher.py:756-762) with EVERY tied pair (duplicate
 *   keypoints), row-major.  count runs the two nearest-neighbour passes and writes offsets[0..na] (int64): the exclusive
 *   prefix sums of the per-row match counts, offsets[na] = number of pairs; the caller reads that one value, allocates
 *   pairs[n][2] (int64: index into a, index into b) and calls fill with the same arguments and workspaces. */
int roma_op_sample_warp_at(const float* warp, const float* cert, int H, int W, const float* xa, long n, float* xa_to_b,
                           float* cert_a, void* stream);
int roma_op_mutual_nn(const float* a, long na, const float* b, long nb, const float* cert_a, float cert_th, float max_dist,
                      int* match_b, void* ws_a, void* ws_b, void* stream);
int roma_op_mutual_nn_count(const float* a, long na, const float* b, long nb, const float* cert_a, float cert_th, float max_dist,
                            void* ws_a, void* ws_b, long long* offsets, void* stream);
int roma_op_mutual_nn_fill(const float* a, long na, const float* b, long nb, const float* cert_a, float cert_th, float max_dist,
                           const void* ws_a, const void* ws_b, long long* offsets, long long* pairs, void* stream);
/* torch.multinomial(weights, k, replacement=False) of RegressionMatcher.sample (matcher.py:615-627): k distinct int64
 * indices, drawn with probability proportional to the non-negative f32 weights [n] (exponential race + radix select, no
 * sort; reproducible from `seed`), returned in DRAW order (ascending race key) like torch.multinomial, so a prefix of the
 * result is itself a valid smaller sample.  If fewer than k weights are positive, zero-weight entries complete the sample
 * (last), as on torch's GPU path.  workspace: device memory of roma_op_multinomial_workspace(n, k) bytes. */
long roma_op_multinomial_workspace(long n, long k);
int roma_op_multinomial(const float* weights, long n, long k, unsigned long long seed, long long* out_indices, void* workspace,
                        long workspace_bytes, void* stream);
/* RegressionMatcher.sample (matcher.py:598-629) applied to each of B pairs separately, in one enqueue of a fixed number of
 * launches (24 in the balanced modes, 12 otherwise, whatever B is) with no host read.  matches [B, n, 4] and certainty [B, n] are
 * f32; pair b draws from seeds[b].  threshold != 0 (the "threshold" sample modes): a certainty above `thresh` counts as 1, in
 * the weights and in out_certainty.  With k = min(4 num, n) if balanced != 0 (the "balanced" modes), min(num, n) otherwise, and
 * m = min(num, k), per pair:
 *   first draw: k of the n rows without replacement, weight = the (thresholded) certainty, by roma_op_multinomial's exponential
 *     race on seed seeds[b] (row i: u from mix64 of (seed, i), key = min(-log(u) / w, 3e38), +inf for w <= 0; the k smallest keys,
 *     in ascending (key, index) order = draw order).  Entries that share the k-th key are taken by ascending index, so a pair
 *     with fewer than k positive weights is completed by its LOWEST zero-weight rows, behind every real row.
 *   balanced == 0: the first draw is the result (k = m).
 *   balanced != 0: density[j] = sum over the k drawn rows of exp(-|x_j - x_i|^2 / (2 0.1^2)) as roma_op_kde(half_inputs = 1)
 *     evaluates it (coordinates rounded to fp16, f32 sum), summed in a fixed order that depends on k alone;
 *     p[j] = 1 / (density[j] + 1), 1e-7 where density[j] < 10, and - the one extension of the reference - 0 for a drawn row whose
 *     certainty is not positive (a filler row).  Second draw: m of the k rows with weight p, the same race over j = 0 .. k - 1
 *     on seed seeds[b] ^ 0x5851f42d4c957f2d, again in draw order, filler rows last.
 * out_matches [B, m, 4] and out_certainty [B, m] are the drawn rows and their (thresholded) certainties.  Nullable outputs:
 * out_counts [B] = min(m, positive weights of the pair), the number of leading rows that are real matches (the `counts` of
 * roma_op_ransac and its neighbours); out_idx [B, m] the drawn rows' indices into the pair's n rows; out_first_idx [B, k] the
 * first draw's; out_density [B, k] the density of the first draw's rows (balanced modes only, otherwise not written).
 * Every output is a function of the pair's inputs and its seed alone: bit-identical from run to run, for every B and for every
 * position of the pair in the batch (ties are broken by index, the density adds its partial sums in a fixed order, no float is
 * added atomically).  The stream of random numbers is not torch's: parity with the reference is distributional.
 * k > 65536 (num > 16384 in the balanced modes) is refused: the order of larger samples (roma_op_multinomial's bitonic
 * network) is not batched.  Also refused, before anything is enqueued: null required pointers, n >= 2^31, B > 65535, a
 * workspace below roma_op_sample_matches_workspace(B, n, num, balanced) bytes (0 for B <= 0, n <= 0 or num <= 0, where the call
 * does nothing), matches / out_matches / workspace not 16-byte aligned.  Restated in numpy float64 by tools/sample_ref.py. */
long roma_op_sample_matches_workspace(int B, long n, long num, int balanced);
int roma_op_sample_matches(const float* matches, const float* certainty, const unsigned long long* seeds, int B, long n, long num,
                           int threshold, float thresh, int balanced, float* out_matches, float* out_certainty, int* out_counts,
                           long long* out_idx, long long* out_first_idx, float* out_density, void* workspace, long workspace_bytes,
                           void* stream);
/* Batched RANSAC - the robust estimation the reference's demos run on sample() output through OpenCV:
 * cv2.findHomography(A, B, RANSAC) (model 0: 4-point DLT, one-sided reprojection error in image B) and
 * cv2.findFundamentalMat(A, B, FM_RANSAC) (model 1: 7-point solver, up to 3 models per sample, max of the two point-to-epipolar-line
 * distances).  Plain RANSAC in rounds of 256 hypotheses per pair with OpenCV's adaptive iteration count, optionally followed by
 * up to 3 least-squares refits on the inliers (refine != 0); the algorithm is restated in tools/geometry_ref.py.
 * kpts_a, kpts_b DEVICE f32 [B, N, 2] pixel coordinates; counts DEVICE int32 [B] rows per pair (NULL: N; rows at or beyond
 * counts[b] are never read); seeds DEVICE u64 [B] (the samples of pair b depend on seeds[b] only).  Outputs, all DEVICE:
 * model f64 [B, 3, 3] mapping A to B (x_B ~ H x_A, x_B^T F x_A = 0; [2][2] = 1, or unit Frobenius norm where |[2][2]| < 1e-12
 * of it; zeros where no model), mask u8 [B, N] inliers of the returned model, ok u8 [B], info int32 [B, 6] = {rounds run,
 * winning hypothesis, its root, its inlier count, final inlier count, pair valid}.  No host synchronisation.
 * workspace: device memory of roma_op_ransac_workspace(B, N) bytes. */
long roma_op_ransac_workspace(int B, int N);
int roma_op_ransac(int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, int B,
                   int N, float threshold, double confidence, int max_iters, int refine, double* out_model, unsigned char* out_mask,
                   unsigned char* out_ok, int* out_info, void* workspace, long workspace_bytes, void* stream);
/* The same batched RANSAC with MAGSAC++ scoring (Barath et al., CVPR 2020; nu = 4), restated in tools/magsac_ref.py - what
 * demo_fundamental asks OpenCV for with USAC_MAGSAC, defined as there (not OpenCV's implementation).  threshold tau is the largest
 * residual that counts as an inlier; a model's score is the sum over the pair's rows of the MAGSAC++ loss of its pixel residual
 * (model 0: reprojection error in image B; model 1: Sampson distance), lower is better; then up to lo_iters (0 .. 64) IRLS steps
 * with the MAGSAC++ weights, each kept only if the score drops.  Inputs as for roma_op_ransac.  Outputs, all DEVICE: model, mask
 * (residual < threshold under the returned model), ok as for roma_op_ransac; info int32 [B, 7] = {rounds run, winning hypothesis,
 * its root, inliers of the winning minimal model, final inliers, pair valid, LO steps accepted}; score f64 [B, 2] = {sum of the
 * loss of the winning minimal model, final sum: that less the accepted LO steps' gains} (0 where no model).  No host
 * synchronisation.
 * workspace: device memory of roma_op_magsac_workspace(B, N) bytes. */
long roma_op_magsac_workspace(int B, int N);
int roma_op_magsac(int model, const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds, int B,
                   int N, float threshold, double confidence, int max_iters, int lo_iters, double* out_model, unsigned char* out_mask,
                   unsigned char* out_ok, int* out_info, double* out_score, void* workspace, long workspace_bytes, void* stream);
/* Essential matrix and relative pose - the tail of the reference's pose benchmarks (romatch/utils/utils.py estimate_pose):
 * cv2.findEssentialMat(A, B, K, RANSAC, prob, threshold, maxIters) and cv2.recoverPose.  Algorithm restated in
 * tools/essential_ref.py.  roma_op_essential: Nister's five-point solver (up to 10 models per sample, real roots by Sturm
 * bisection), Sampson test (x_B^T E x_A)^2 < thr^2 (|E x_A|_{1,2}^2 + |E^T x_B|_{1,2}^2), plain RANSAC in rounds of 256
 * hypotheses per pair with OpenCV's adaptive iteration count, no refinement.  kpts_a, kpts_b DEVICE f32 [B, N, 2]; counts,
 * seeds as for roma_op_ransac; camera_matrix DEVICE f64 [B, 3, 3] or NULL (identity: the points are normalised already),
 * applied as OpenCV does: x_n = ((x - cx) / fx, (y - cy) / fy), threshold / ((fx + fy) / 2).  Outputs, all DEVICE: E f64
 * [B, 3, 3] on normalised points (unit Frobenius norm, largest-magnitude entry positive; zeros where no model), mask u8 [B, N],
 * ok u8 [B], info int32 [B, 5] = {rounds run, winning hypothesis, its root, inlier count, pair valid}.  No host
 * synchronisation.  workspace: device memory of roma_op_essential_workspace(B, N) bytes. */
long roma_op_essential_workspace(int B, int N);
int roma_op_essential(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
                      const double* camera_matrix, int B, int N, float threshold, double prob, int max_iters, double* out_e,
                      unsigned char* out_mask, unsigned char* out_ok, int* out_info, void* workspace, long workspace_bytes,
                      void* stream);
/* roma_op_essential with MAGSAC++ scoring and local optimisation (Barath et al., CVPR 2020; nu = 4, k^2 = 13.2767), restated in
 * tools/essential_magsac_ref.py.  Sampling, five-point solver, slots and adaptive iteration count are roma_op_essential's; a
 * model's score is the sum over the pair's rows of the MAGSAC++ loss of its Sampson distance in normalised camera coordinates,
 * (x_B^T E x_A)^2 / (|E x_A|_{1,2}^2 + |E^T x_B|_{1,2}^2), with tau = threshold / ((fx + fy) / 2) the largest residual that counts
 * as an inlier; lower is better.  Then up to lo_iters (0 .. 64) IRLS steps: the MAGSAC++ weights of the current model, over the
 * rows of positive weight (at least 8) the weighted eight-point system on Hartley-normalised coordinates, the eigenvectors of its
 * four smallest eigenvalues as the basis of the five-point solver's cubic constraints (Nister's form for more than five points),
 * the solution of the smallest score projected onto the essential manifold; a step is kept only if the score drops, so a model
 * is never lost and lo_iters = 0 returns the winning five-point model untouched.  Inputs as for roma_op_essential.  Outputs, all
 * DEVICE: E, ok as for roma_op_essential; mask u8 [B, N] (residual < tau under the returned E: roma_op_essential's inlier rule up
 * to the rounding of one f32 division); info int32 [B, 7] = {rounds run, winning hypothesis, its root, inliers of the winning
 * minimal model, final inliers, pair valid, LO steps accepted}; score f64 [B, 2] = {sum of the loss of the winning minimal
 * model, final sum: that less the accepted LO steps' gains} (0 where no model).  No host synchronisation; bit-identical from run
 * to run and independent of B.  workspace: device memory of roma_op_essential_magsac_workspace(B, N) bytes. */
long roma_op_essential_magsac_workspace(int B, int N);
int roma_op_essential_magsac(const float* kpts_a, const float* kpts_b, const int* counts, const unsigned long long* seeds,
                             const double* camera_matrix, int B, int N, float threshold, double prob, int max_iters, int lo_iters,
                             double* out_e, unsigned char* out_mask, unsigned char* out_ok, int* out_info, double* out_score,
                             void* workspace, long workspace_bytes, void* stream);
/* The five-point solver alone: x0, x1 DEVICE f64 [S, 5, 2] (x1^T E x0 = 0) -> E DEVICE f64 [S, 10, 3, 3] (solutions in ascending
 * order of Nister's z, unused slots 0), n DEVICE int32 [S]. */
int roma_op_essential_minimal(const double* x0, const double* x1, int S, double* out_e, int* out_n, void* stream);
/* cv2.recoverPose(E, A, B, K, distance_thresh, mask): the four decompositions (R1, t), (R2, t), (R1, -t), (R2, -t) of E (SVD with
 * OpenCV's det(U), det(V^T) > 0 fix-up, t = U[:, 2]), linear triangulation of the masked rows, a row counts for a candidate if
 * its depth is positive and below distance_thresh in both cameras; the candidate with the most rows wins (ties: the earlier).
 * E DEVICE f64 [B, 3, 3]; kpts as above; mask DEVICE u8 [B, N] or NULL (every row); counts, camera_matrix as above.
 * Outputs, all DEVICE: n_good int32 [B], R f64 [B, 3, 3], t f64 [B, 3], mask_good u8 [B, N].  workspace: device memory of
 * roma_op_recover_pose_workspace(B, N) bytes. */
long roma_op_recover_pose_workspace(int B, int N);
int roma_op_recover_pose(const double* E, const float* kpts_a, const float* kpts_b, const unsigned char* mask, const int* counts,
                         const double* camera_matrix, int B, int N, double distance_thresh, int* out_n_good, double* out_r,
                         double* out_t, unsigned char* out_mask, void* workspace, long workspace_bytes, void* stream);
/* Nonlinear refinement of a relative pose: a Levenberg-Marquardt fit of (R, t) to the Sampson error of E = [t]x R under a
 * hard-truncated loss sum min(r^2, thr^2) - what the final refinement of PoseLib's estimate_relative_pose is (the reference's
 * megadepth_pose_estimation_benchmark_poselib.py); it follows roma_op_essential + roma_op_recover_pose, whose pose is the winning
 * five-point sample's.  Algorithm restated in tools/pose_refine_ref.py: five parameters (R <- exp([w]x) R, t on the unit sphere),
 * analytic Jacobian over the active rows (r^2 < thr^2), (H + lambda diag H) delta = -g by Cholesky, lambda from 1e-3, a step is
 * kept only if it lowers the truncated cost (else lambda x 10, at most 10 retries).  It stops after max_steps accepted steps, on a
 * step shorter than 1e-10, with fewer than 5 active rows or when H + lambda diag H is not positive definite; the pose so far is
 * returned, so the cost never rises and a pose is never lost.  R DEVICE f64 [B, 3, 3], t DEVICE f64 [B, 3]; kpts_a, kpts_b
 * DEVICE f32 [B, N, 2] NORMALISED points; counts as for roma_op_ransac; valid DEVICE u8 [B] or NULL (every pair): pairs to fit,
 * the others are copied through; thr in normalised units.  Outputs, all DEVICE: R f64 [B, 3, 3], t f64 [B, 3] (the input bits
 * when no step was accepted), mask u8 [B, N] (r^2 < thr^2 under the returned pose and positive depth in both cameras by
 * recoverPose's triangulation; zeros for a pair that is not fitted), info int32 [B, 4] = {accepted steps, cost evaluations,
 * active rows at the end, pair fitted (valid, at least 5 rows, finite pose)}.  One workgroup per pair runs the whole loop in
 * one launch: no host synchronisation, bit-identical from run to run and independent of B.  workspace: device memory of
 * roma_op_refine_pose_workspace(B, N) bytes. */
long roma_op_refine_pose_workspace(int B, int N);
int roma_op_refine_pose(const double* R, const double* t, const float* kpts_a, const float* kpts_b, const int* counts,
                        const unsigned char* valid, int B, int N, double thr, int max_steps, double* out_r, double* out_t,
                        unsigned char* out_mask, int* out_info, void* workspace, long workspace_bytes, void* stream);
/* Absolute pose: the camera pose (R, t), x_cam = R X + t, from rows of a 3-D point X and its image x - P3P RANSAC.  Restated in
 * tools/absolute_pose_ref.py.  points3d DEVICE f32 [B, N, 3]; kpts DEVICE f32 [B, N, 2]; counts, seeds as for roma_op_ransac;
 * camera_matrix DEVICE f64 [B, 3, 3] or NULL (kpts are normalised image coordinates): x_n = ((u - cx) / fx, (v - cy) / fy) and
 * the threshold is divided by (fx + fy) / 2, as in roma_op_essential.  The 3-D rows are centred on the centroid of the finite
 * rows and scaled to mean distance 1 first, so the f32 scoring is independent of the world origin.  Hypotheses: samples of 3
 * rows, up to 4 poses each (every real solution with three positive depths, ascending in the solver's root; collinear samples
 * give none).  A row is an inlier when its depth is positive and its reprojection error is below the threshold; a row with a
 * non-finite entry never is; rounds, selection and the adaptive iteration count are roma_op_ransac's.  A model needs 4 inliers
 * (the rows of its own sample always fit).  Outputs, all DEVICE: R f64 [B, 3, 3], t f64 [B, 3] (0 where no model), mask u8
 * [B, N], ok u8 [B], info int32 [B, 5] = {rounds run, winning hypothesis, its slot, its inlier count, pair valid (at least 4
 * finite rows that are not all one point)}.  No host synchronisation; bit-identical from run to run and independent of B.
 * workspace: device memory of roma_op_absolute_pose_workspace(B, N) bytes. */
long roma_op_absolute_pose_workspace(int B, int N);
int roma_op_absolute_pose(const float* points3d, const float* kpts, const int* counts, const unsigned long long* seeds,
                          const double* camera_matrix, int B, int N, float threshold, double conf, int max_iters, double* out_r,
                          double* out_t, unsigned char* out_mask, unsigned char* out_ok, int* out_info, void* workspace,
                          long workspace_bytes, void* stream);
/* The P3P solver alone: X DEVICE f64 [S, 3, 3] points, x DEVICE f64 [S, 3, 2] normalised image points -> R DEVICE f64
 * [S, 4, 3, 3], t DEVICE f64 [S, 4, 3] (solutions in ascending order of the solver's root, unused slots 0), n DEVICE int32 [S]. */
int roma_op_absolute_pose_minimal(const double* X, const double* x, int S, double* out_r, double* out_t, int* out_n, void* stream);
/* Nonlinear refinement of an absolute pose: a Levenberg-Marquardt fit of (R, t) to the reprojection error in normalised image
 * coordinates under the hard-truncated loss sum min(|r|^2, thr^2); the loop (lambda, retries, stopping rules) is
 * roma_op_refine_pose's, with six parameters (R <- exp([w]x) R, t <- t + dt), two residuals per row and at least 3 active rows; a
 * row whose depth is not positive is not active.  It runs on the normalised problem of roma_op_absolute_pose.  R DEVICE f64
 * [B, 3, 3], t DEVICE f64 [B, 3]; points3d, kpts, counts, camera_matrix as for roma_op_absolute_pose; valid DEVICE u8 [B] or NULL
 * (every pair): pairs to fit, the others are copied through; thr in pixels of camera_matrix (normalised units without one).
 * Outputs, all DEVICE: R, t (the input bits when no step was accepted), mask u8 [B, N] (active under the returned pose; zeros
 * for a pair that is not fitted), info int32 [B, 4] = {accepted steps, cost evaluations, active rows at the end, pair fitted}.
 * One workgroup per pair runs the whole loop in one launch; bit-identical from run to run and independent of B. */
int roma_op_refine_absolute_pose(const double* R, const double* t, const float* points3d, const float* kpts, const int* counts,
                                 const unsigned char* valid, const double* camera_matrix, int B, int N, double thr, int max_steps,
                                 double* out_r, double* out_t, unsigned char* out_mask, int* out_info, void* stream);
/* Matches to rows of roma_op_absolute_pose through a depth map of image A: matches DEVICE f32 [B, N, 4] in normalised
 * coordinates (columns 0:2 in A, 2:4 in B), depth_a DEVICE f32 [B, H, W], camera_a DEVICE f64 [B, 3, 3] at the depth map's size
 * -> points DEVICE f32 [B, N, 3] in camera A's frame, kpts_b DEVICE f32 [B, N, 2] pixels of an (H_b, W_b) image.  Depth is
 * bilinear (align_corners = False) from four neighbours that are all finite and positive (roma_op_depth_consistency's rule);
 * otherwise the point is NaN, which the pose kernels ignore. */
int roma_op_lift_matches(const float* matches, const float* depth_a, const double* camera_a, int B, int N, int H, int W, int H_b,
                         int W_b, float* out_points, float* out_kpts_b, void* stream);
/* Bundle adjustment: B independent problems of V views (1 <= V <= 8) and N points, the cameras and the points refined together
 * on the reprojection error by Levenberg-Marquardt with the Schur complement, under the hard-truncated loss
 * sum min(|r|^2, thr_i^2) over the observations; lambda, retries and stopping rules are roma_op_refine_pose's.  points DEVICE
 * f64 [B, N, 3]; kpts DEVICE f32 [B, V, N, 2] in pixels of their view, a non-finite entry: not observed; camera_matrices DEVICE
 * f64 [B, V, 3, 3] or NULL (kpts are normalised image coordinates, and so is reproj_thresh); R DEVICE f64 [B, V, 3, 3], t DEVICE
 * f64 [B, V, 3] with x_cam = R X + t; hold DEVICE u8 [B, V, 6] or NULL (nothing held): the camera parameters (three of the
 * rotation update R <- exp([w]x) R, three of t) that stay - hold at least seven, or the gauge is left to the damping; counts
 * DEVICE int32 [B] or NULL (N points each; later points are copied through); valid DEVICE u8 [B] or NULL (every problem);
 * reproj_thresh in pixels of each view (divided by (fx + fy) / 2), +inf: plain least squares.  A point beyond counts[b], with a
 * non-finite start or with fewer than two observations is not part of the problem.  Outputs, all DEVICE: points f64 [B, N, 3], R,
 * t (the input bits when no step was accepted, and always for a point outside the problem), mask u8 [B, V, N] (active under
 * the returned state; zeros for a problem that is not fitted), info int32 [B, 6] = {accepted steps, cost evaluations, active
 * rows at the end, points adjusted, free camera parameters, problem fitted}, cost f64 [B, 2] = {start, end} (NaN for a problem
 * that is not evaluated).  The workspace (roma_op_bundle_adjust_workspace bytes, N <= 2^27, B V N < 2^31) holds the current and
 * the trial points.  One workgroup per problem runs the whole loop in one launch; bit-identical from run to run and independent
 * of B. */
long roma_op_bundle_adjust_workspace(int B, int V, int N);
int roma_op_bundle_adjust(const double* points, const float* kpts, const double* camera_matrices, const double* R, const double* t,
                          const unsigned char* hold, const int* counts, const unsigned char* valid, int B, int V, int N,
                          double reproj_thresh, int max_steps, double* out_points, double* out_r, double* out_t, unsigned char* out_mask,
                          int* out_info, double* out_cost, void* workspace, long workspace_bytes, void* stream);
/* Multi-view tracks from pairwise index matches: what joins roma_op_match_keypoints over the pairs of V images (2 <= V <= 8) into
 * the [V, N] observation table roma_op_triangulate_views and roma_op_bundle_adjust read.  Restated by tools/tracks_ref.py.
 * inds DEVICE int32 [B, P, M, 2], 8-byte aligned: row (i, j) of pair p joins keypoint i of view pair_views[p][0] to keypoint j of
 * view pair_views[p][1]; pair_views HOST int32 [P, 2], shared by all problems, P <= 64 (it is checked before any device work and
 * travels in the kernel's arguments): both views in [0, V) and different, the same pair of views may occur more than once;
 * match_counts DEVICE int32 [B, P] or NULL (M each): the rows of each pair that are read, later rows never are; num_kpts DEVICE
 * int32 [B, V] or NULL (K each): a row with an index outside [0, num_kpts[v]) on either side - the -1 padding of
 * roma_op_match_keypoints - is ignored and counted; x DEVICE f32 [B, V, K, 2] or NULL, with out_kpts: the keypoints themselves.
 * Nodes are (v, i) with id v K + i, edges the rows that were used.  A connected component is a track when it has at least
 * min_views (>= 2) nodes and no view twice; a component that holds two keypoints of one view is dropped whole and counted
 * (OpenMVG's rule).  Tracks are numbered in ascending order of their smallest node id: the whole result depends on the edge set
 * alone, not on the order of rows or pairs, on duplicate rows or on the thread schedule.
 * Outputs, all DEVICE: tracks int32 [B, V, T], T = max_tracks: the keypoint index, -1 where the view is not in the track and for
 * tracks at or beyond counts[b]; kpts f32 [B, V, T, 2] (NULL with x NULL): the keypoint's bits, NaN elsewhere - what
 * roma_op_bundle_adjust and roma_op_triangulate_views read as "not observed"; counts int32 [B] = min(total, T); total int32 [B];
 * info int32 [B, 4] = {rows used, rows ignored, components of >= 2 nodes, components dropped}.
 * One workgroup per problem runs everything in one launch and never waits on another: labels by min-label hooking (atomicMin,
 * the kernel's only atomic) and pointer jumping between workgroup barriers, until a round changes nothing (fewer than V K
 * rounds: each one that changes anything removes a root); then conflicts, counting and a prefix sum over the roots in id order.
 * Limits: K <= 65536 keypoints per view (2^19 nodes, four int32 each in the workspace of roma_op_build_tracks_workspace bytes),
 * P <= 64, B <= 65535, B P M < 2^30, B V T < 2^30.  Every argument is checked before anything is enqueued; B == 0 launches
 * nothing; bit-identical from run to run and independent of B. */
long roma_op_build_tracks_workspace(int B, int V, int K, int P, int M);
int roma_op_build_tracks(const int* inds, const int* pair_views, const int* match_counts, const int* num_kpts, const float* x, int B,
                         int V, int K, int P, int M, int max_tracks, int min_views, int* out_tracks, float* out_kpts, int* out_counts,
                         int* out_total, int* out_info, void* workspace, long workspace_bytes, void* stream);
/* Detector-free keypoints: the dense matches of an image set to per-view keypoints and index matches - what stands between
 * roma_op_sample_matches over the P pairs of V images (2 <= V <= 8) and roma_op_build_tracks when no detector supplies
 * keypoints.  The endpoints of all pairs that touch a view are quantised to a pixel grid, one keypoint per occupied cell stays,
 * close keypoints of neighbouring cells are merged, and the rows are re-indexed.  Restated by tools/set_keypoints_ref.py.
 * matches DEVICE f32 [B, P, N, 4], 16-byte aligned: rows (xA, yA, xB, yB) in normalised coordinates, A in view pair_views[p][0],
 * B in view pair_views[p][1]; certainty DEVICE f32 [B, P, N]; counts DEVICE int32 [B, P] or NULL (N each): later rows are
 * never read; pair_views HOST int32 [P, 2] as for roma_op_build_tracks; sizes HOST int32 [V, 2] = (H_v, W_v), each in
 * [1, 65535]: the image sizes the caller's intrinsics refer to; cell in [1, 64] pixels; 0 <= radius <= cell pixels;
 * 1 <= max_kpts = K <= 65536; one_to_one 0 or 1.
 *   1. pixels: x_px = fl32(W_v / 2) * fl32(x + 1), y_px = fl32(H_v / 2) * fl32(y + 1): a product of a rounded sum, nothing fused.
 *   2. an endpoint is valid when both are finite, 0 <= x_px < W_v and 0 <= y_px < H_v; a row is valid when n < counts, its
 *      certainty c is finite and > 0 and both endpoints are valid.  An invalid row gets inds (-1, -1) and is counted.
 *   3. cells: Gw_v = ceil(W_v / cell), Gh_v = ceil(H_v / cell); the cell of an endpoint is (int(floor(y_px)) / cell,
 *      int(floor(x_px)) / cell) in integer division, its id g = cy Gw_v + cx.
 *   4. key: the ordinal of an endpoint is o = (p N + n) 2 + side (A 0, B 1), its 64-bit key (bits of c) << 32 | (0xFFFFFFFF - o):
 *      the certainty decides, then the earlier row.  The candidate of a (view, cell) is the valid endpoint in it with the largest
 *      key; its float32 pixel position and its c are the position and the score of the cell.
 *   5. suppression (radius > 0): a candidate survives unless one of the 8 neighbouring cells holds a candidate with a larger key
 *      at squared distance d2 <= fl32(radius * radius), d2 = fmaf(dy, dy, fl32(dx * dx)) in float32.  One pass, a local-maximum
 *      test: a suppressed candidate still suppresses.  radius == 0: every candidate survives.
 *   6. cut: of more than K survivors of a view the K with the largest keys stay; total[b, v] counts them before the cut.
 *   7. numbering: the keypoints of a view are its kept survivors in ascending cell id; num_kpts[b, v] = min(total, K).
 *   8. assignment: with radius > 0 a valid endpoint takes the nearest kept keypoint among the 3 x 3 cells around its own with
 *      d2 <= fl32(radius * radius), the larger key on a tie; with radius == 0 its own cell's keypoint if kept.  A row with an
 *      endpoint that gets none has inds (-1, -1) and is counted.
 *   9. one_to_one: within a pair, among the rows that still have indices, with the row key (bits of c) << 32 | (0xFFFFFFFF - n)
 *      a row stays only if it has the largest row key among the rows with its A keypoint and among the rows with its B
 *      keypoint - one pass, not iterated; the others become (-1, -1) and are counted.  (Two rows of a pair that share a
 *      keypoint would put a view twice into a component, which roma_op_build_tracks drops whole.)
 * Outputs, all DEVICE: kpts f32 [B, V, K, 2], 8-byte aligned, pixels, NaN at and beyond num_kpts - what roma_op_build_tracks and
 * everything after it read as "not observed"; score f32 [B, V, K], 0 beyond num_kpts; num_kpts int32 [B, V]; total int32 [B, V];
 * inds int32 [B, P, N, 2], 8-byte aligned: rows stay where they are ((-1, -1) for every row without indices, rows at and beyond
 * counts included), so counts serves as roma_op_build_tracks' match_counts; kept int32 [B, P]: the rows of the pair with
 * indices; info int32 [B, 6] = {rows read, rows invalid, rows without a keypoint, rows dropped by one_to_one, rows kept,
 * candidates suppressed}.
 * Everything is integer or max-selection logic: bit-identical from run to run and independent of B.  Seven kernels on the
 * stream (clear, scatter by 64-bit atomicMax, suppress, a per-view scan of block counts with a radix select where a view
 * exceeds K, number, assign, finish), every phase closed by a kernel boundary; no host synchronisation, no allocation.  The
 * workspace (roma_op_keypoints_from_matches_workspace bytes for G_total = sum_v Gw_v Gh_v; 0 for an empty or refused problem)
 * holds 12 bytes per cell, every view's grid padded to 1024 cells, and 16 bytes per (pair, keypoint); it need not be zero on
 * entry.  Limits: Gw_v Gh_v <= 2^22 per view, B (G_total + 1024 V) <= 2^28, 2 P N < 2^32, B P N < 2^30, P <= 64, B <= 65535.
 * Every argument is checked before anything is enqueued; B == 0 launches nothing. */
long roma_op_keypoints_from_matches_workspace(int B, int V, int P, int N, long G_total, int K);
int roma_op_keypoints_from_matches(const float* matches, const float* certainty, const int* counts, const int* pair_views,
                                   const int* sizes, int B, int V, int P, int N, int cell, float radius, int max_kpts, int one_to_one,
                                   float* out_kpts, float* out_score, int* out_num_kpts, int* out_total, int* out_inds, int* out_kept,
                                   int* out_info, void* workspace, long workspace_bytes, void* stream);
/* N-view triangulation: the 3-D point of every track from all the views that observe it, the poses given (x_cam = R X + t) -
 * the point half of roma_op_bundle_adjust.  Float64 with fp contraction off; restated operation by operation by
 * tools/triangulate_views_ref.py.  kpts DEVICE f32 [B, V, N, 2], 8-byte aligned, pixels of their view, a non-finite entry: the
 * view does not observe the point; camera_matrices DEVICE f64 [B, V, 3, 3] or NULL (observations and thresholds are normalised);
 * R DEVICE f64 [B, V, 3, 3], t DEVICE f64 [B, V, 3]; view_valid DEVICE u8 [B, V] or NULL: a view that is not valid (or whose pose or
 * camera is not finite) contributes no observation - how an unregistered view is passed; counts DEVICE int32 [B] or NULL (N);
 * valid DEVICE u8 [B] or NULL (every problem).  Per point, x_n = ((u - cx) / fx, (v - cy) / fy):
 *   1. the observations in use: finite, of a valid view, not trimmed; fewer than min_views (>= 2) of them: DEGENERATE;
 *   2. unit ray d_v = R_v^T (x_n, 1) / |.| from the centre c_v = -R_v^T t_v;
 *   3. midpoint (sum (I - d d^T)) X = sum (I - d d^T) c by a 3 x 3 Cholesky factor; a pivot that is not finite or not above 1e-14 x
 *      the largest diagonal entry (parallel rays): DEGENERATE;
 *   4. up to gn_steps (0 .. 10) Gauss-Newton steps on sum |p_xy / z - x_n|^2, p = R_v X + t_v, over the observations in use:
 *      analytic Jacobian, normal equations by the same factor; a step is kept only if its cost is finite and strictly lower, the
 *      first rejected or failed step ends the loop - the cost never rises above the midpoint's;
 *   5. trim = 1: e_v = |error| / thr_v with thr_v = max_reproj / ((fx_v + fy_v) / 2) (roma_op_bundle_adjust's rule; +inf switches the
 *      test off); while the largest e_v exceeds 1 and at least 3 observations are in use, the worst one (the lowest view of a
 *      tie) leaves the set and the point is computed again from 2 - at most V - 2 times.
 * Outputs, all DEVICE: points f64 [B, N, 3], NaN where bit 1 or 2 is set, so the array feeds roma_op_bundle_adjust unchanged;
 * reproj f32 [B, V, N]: the error in pixels of every finite observation of a valid view, trimmed ones included, NaN elsewhere;
 * used u8 [B, V, N]: the observations of the final fit; parallax f32 [B, N]: the largest angle between two rays in use (the pair
 * with the smallest dot product), degrees; flags u8 [B, N], roma_op_triangulate's bits: 1 skipped, 2 degenerate, 4 not
 * 0 < depth < max_depth in a view in use, 8 an observation in use above max_reproj, 16 not parallax >= min_parallax; stats int32
 * [B, 8] = {points considered, valid, degenerate, cheirality, reproj, parallax, observations trimmed, 0}, cleared on the stream by
 * the same call.  One thread per point, the views staged once per workgroup; no workspace, no host read; bit-identical from
 * run to run and independent of B.  Refused before anything is enqueued: a null required pointer, V outside [2, 8], B > 65535,
 * B V N >= 2^31, a negative (or NaN) threshold, min_views outside [2, V], gn_steps outside [0, 10], trim not 0 or 1, kpts not
 * 8-byte aligned.  B = 0 or N = 0 launches nothing. */
int roma_op_triangulate_views(const float* kpts, const double* camera_matrices, const double* R, const double* t,
                              const unsigned char* view_valid, const int* counts, const unsigned char* valid, int B, int V, int N,
                              double max_reproj, double min_parallax, double max_depth, int min_views, int gn_steps, int trim,
                              double* out_points, float* out_reproj, unsigned char* out_used, float* out_parallax,
                              unsigned char* out_flags, int* out_stats, void* stream);
/* Nonlinear refinement of a homography (model 0) or a fundamental matrix (model 1): a Levenberg-Marquardt fit under the
 * hard-truncated loss sum min(|r|^2, thr^2) of the forward reprojection error in image B (H: what cv2.findHomography(..., RANSAC)
 * ends with) or of the Sampson distance (F: what PoseLib's estimate_fundamental ends with); it follows roma_op_ransac /
 * roma_op_magsac, whose last step is an algebraic least-squares refit.  Algorithm restated in tools/model_refine_ref.py: the fit
 * runs in the Hartley-normalised coordinates of the pair's finite rows with residuals in pixels; H keeps its largest entry fixed
 * and updates the other eight, F = U diag(1, sigma, 0) V^T is updated on (U, V, sigma) and has rank 2 at every iterate; the loop
 * (lambda, retries, stopping rules) is roma_op_refine_pose's, with at least 4 (H) or 7 (F) active rows.  The active set is
 * re-evaluated with every cost, not frozen to a RANSAC mask.  M DEVICE f64 [B, 3, 3] in pixel coordinates (x_B ~ H x_A,
 * x_B^T F x_A = 0); kpts_a, kpts_b DEVICE f32 [B, N, 2] pixels; counts as for roma_op_ransac; valid DEVICE u8 [B] or NULL (every
 * pair): pairs to fit, the others are copied through; thr > 0 in pixels (inf: plain least squares over the finite rows).
 * Outputs, all DEVICE: M f64 [B, 3, 3] (scaled like roma_op_ransac's; the input bits when no step was accepted), mask u8 [B, N]
 * (|r|^2 < thr^2 under the returned model; zeros for a pair that is not fitted), info int32 [B, 4] = {accepted steps, cost
 * evaluations, active rows at the end, pair fitted}, cost f64 [B, 2] = {truncated cost at the start, at the end} in px^2 (NaN
 * for a pair that is not fitted).  One workgroup per pair runs the whole loop in one launch: no host synchronisation,
 * bit-identical from run to run and independent of B.  B == 0 launches nothing.  workspace: device memory of
 * roma_op_refine_model_workspace(B, N) bytes. */
long roma_op_refine_model_workspace(int B, int N);
int roma_op_refine_model(int model, const double* M, const float* kpts_a, const float* kpts_b, const int* counts,
                         const unsigned char* valid, int B, int N, double thr, int max_steps, double* out_m, unsigned char* out_mask,
                         int* out_info, double* out_cost, void* workspace, long workspace_bytes, void* stream);
/* Triangulation under a known relative pose: the depth of every match and its 3-D point - what follows roma_op_recover_pose /
 * roma_op_refine_pose when the user wants a depth map or a point cloud from a dense warp (or from sample() output).  Restated
 * operation by operation in numpy float64 by tools/triangulate_ref.py; evaluated in float64 with fp contraction off.
 * The error model is one-sided, as a dense matcher's is: the pixel on the grid of the REFERENCE image is exact, the predicted
 * coordinate in the OTHER image carries the error, so the point lies on the reference pixel's ray at the depth whose projection
 * into the other image is closest to the prediction.  Reference pixel (u, v) with camera K_r, observation (u', v') with camera
 * K_o, (R, t) mapping reference-frame points to the other frame, cameras applied by fx, fy, cx, cy only:
 *   x = ((u - cx_r) / fx_r, (v - cy_r) / fy_r, 1), r = R x, A = K_o r (image of the ray's point at infinity), Bv = K_o t (epipole);
 *   l = A x Bv (epipolar line), n2 = l0^2 + l1^2, s = l0 u' + l1 v' + l2; signed residual d = s / sqrt(n2) in pixels of the other
 *   image; foot point p = (u', v') - s (l0, l1) / n2;
 *   a = (p_x A2 - A0, p_y A2 - A1), b = (Bv0 - p_x Bv2, Bv1 - p_y Bv2), z_ref = a.b / a.a, X = z_ref x, z_other = z_ref r2 + t2;
 *   xh = ((p_x - cx_o) / fx_o, (p_y - cy_o) / fy_o, 1), parallax = atan2(|r x xh|, r . xh) in degrees.
 * matches DEVICE f32 [B, n, 4], 16-byte aligned: columns 0:2 in image A, 2:4 in image B; coords 0: pixels, 1: normalised [-1, 1]
 * with pixel = (x + 1) * W / 2 of the image sizes W_a, H_a, W_b, H_b (not read for coords 0).  sym_w 0: every point is
 * A-reference (columns 0:2 exact, K_r = K_a, K_o = K_b, pose (R, t)).  sym_w = W: the rows are those of a symmetric warp on an
 * [H, 2W] grid, n a multiple of 2W, and point i is B-reference when i mod 2W >= W: columns 2:4 are the exact grid of image B,
 * the roles of the cameras swap and the pose is (R^T, -R^T t), formed in the kernel; its X is in camera B's frame.
 * certainty DEVICE f32 [B, n] or NULL; counts DEVICE int32 [B] or NULL (n); valid DEVICE u8 [B] or NULL (every pair); R DEVICE
 * f64 [B, 3, 3], t DEVICE f64 [B, 3] (A to B); K_a, K_b DEVICE f64 [B, 3, 3] or NULL (identity).
 * Outputs, all DEVICE: points f32 [B, n, 3] in the reference camera's frame (points[..., 2] is the depth map); nullable
 * depth_other, reproj (signed), parallax (degrees) f32 [B, n]; flags u8 [B, n], a point is valid when its byte is 0:
 *    1 skipped: the row lies at or beyond counts[b], or valid[b] == 0 (inputs of such rows are never read);
 *    2 degenerate: a non-finite coordinate, pose or camera entry (fx, fy, cx, cy), or not n2 > 0 (the reference pixel is at the
 *      epipole, or t = 0);
 *    4 cheirality: not 0 < z_ref < max_depth or not 0 < z_other < max_depth (NaN and a.a = 0 fail by this wording);
 *    8 not |d| <= max_reproj;   16 not parallax >= min_parallax;   32 certainty given and not certainty >= min_certainty.
 * A row with bit 1 or 2 carries no other bit and its float outputs are NaN; every other row gets all of its bits and its computed
 * values.  Nullable stats int32 [B, 2, 8] = {rows considered, valid rows, degenerate, cheirality, reproj, parallax, certainty,
 * 0} for the A-reference and the B-reference rows (second row zero when sym_w = 0): integer atomics, cleared on the stream by
 * the same call.  One launch (plus the clear) for the whole batch, no workspace, no host read; bit-identical from run to run and
 * independent of B and of the order of the pairs.  Refused before anything is enqueued: a null required pointer, B < 0 or
 * B > 65535, n < 0, B * n >= 2^31, matches not 16-byte aligned, sym_w < 0 or n not a multiple of 2 sym_w, coords = 1 with a
 * size that is not positive, a negative threshold.  B = 0 or n = 0 returns 0 and launches nothing. */
int roma_op_triangulate(const float* matches, const float* certainty, const int* counts, const unsigned char* valid, const double* R,
                        const double* t, const double* K_a, const double* K_b, int B, long n, int coords, int W_a, int H_a, int W_b,
                        int H_b, int sym_w, double max_depth, double max_reproj, double min_parallax, double min_certainty,
                        float* out_points, float* out_depth_other, float* out_reproj, float* out_parallax, unsigned char* out_flags,
                        int* out_stats, void* stream);
/* Depth consistency of the two halves of a symmetric warp, which triangulate the same surface from both sides - the rule of the
 * reference's warp_kpts (romatch/utils/utils.py: relative_depth_error_threshold) with triangulated depth in place of sensor
 * depth.  points, flags: the outputs of a roma_op_triangulate call with sym_w = W on an [H, 2W] grid.  For a valid point with
 * position X in its own frame: X' = R X + t (A half) or R^T (X - t) (B half); p = (fx X'_x / X'_z + cx, fy X'_y / X'_z + cy) with
 * the other camera; the other half's grid position by the align_corners=False rule, gx = p_x / W_other * W - 0.5,
 * gy = p_y / H_other * H - 0.5, x0 = floor(gx), y0 = floor(gy); the point has support only if 0 <= x0, x0 + 1 <= W - 1, 0 <= y0,
 * y0 + 1 <= H - 1 and its four neighbours in the other half are valid (stricter than zero padding, on purpose); v = the bilinear
 * interpolation of their z_ref (f32 depths, f64 arithmetic: (d00 (1 - fx) + d01 fx) (1 - fy) + (d10 (1 - fx) + d11 fx) fy);
 * err = |v - X'_z| / v.  consistent DEVICE u8 [B, H, 2W]: 1 err < rel_thresh, 0 otherwise, 2 no support or the point itself is not
 * valid; nullable err DEVICE f32 [B, H, 2W], NaN where there is no support.  R, t, K_a, K_b as for roma_op_triangulate.  One
 * launch, no workspace, no host read.  Refused before anything is enqueued: a null required pointer, B < 0 or B > 65535, negative
 * H or W, B * H * 2W >= 2^31, an image size that is not positive, a negative rel_thresh.  B, H or W = 0 launches nothing. */
int roma_op_depth_consistency(const float* points, const unsigned char* flags, const double* R, const double* t, const double* K_a,
                              const double* K_b, int W_a, int H_a, int W_b, int H_b, int B, int H, int W, double rel_thresh,
                              unsigned char* out_consistent, float* out_err, void* stream);
/* Dense multi-view depth fusion: the depth maps of the pairs of an image set to one depth map per view and one point cloud - what
 * joins the poses of roma_op_bundle_adjust to the dense product of a dense matcher.  B problems of V views (2 <= V <= 8) and P
 * pairs (1 <= P <= 64) on a grid H x W.  Restated operation by operation in numpy float64 by tools/depth_fusion_ref.py.  All
 * arithmetic is float64 in the order written, with fp contraction off; depths are read and stored as float32.
 * points DEVICE f32 [B, P, H, Wd, 3], flags DEVICE u8 [B, P, H, Wd], certainty DEVICE f32 [B, P, H, Wd] or NULL (every weight 1): the
 * outputs of ONE roma_op_triangulate call over the pairs (sym_w = W or 0) and the certainty it read, read in place; only
 * points[..., 2], the depth, is read.  symmetric 1: Wd = 2W, the left half of pair p lies on the grid of view pair_views[p][0], the
 * right half on the grid of view pair_views[p][1]; symmetric 0: Wd = W, only the first.  pair_views HOST int32 [P, 2]: both views in
 * [0, V) and different, no ORDERED pair twice ((i, j) and (j, i) may both occur: a view has at most 2 (V - 1) = 14 hypotheses).
 * cameras DEVICE f64 [B, V, 3, 3] IN GRID UNITS, applied by fx, fy, cx, cy: the image intrinsics scaled by W / W_img and H / H_img; the
 * centre of grid cell (r, c) is (c + 0.5, r + 0.5).  R DEVICE f64 [B, V, 3, 3], t DEVICE f64 [B, V, 3], x_cam = R X + t, as
 * roma_op_triangulate_views takes them.  view_valid DEVICE u8 [B, V] or NULL, valid DEVICE u8 [B] or NULL: a view that is not valid
 * (every view of a problem that is not) has no depth, supports nothing, and the slots of its pairs are not usable in either view.
 * Colour source, all three or none: images DEVICE u8, packed [H_img, W_img, 3] images; image_offsets HOST int64 [B, V] byte offsets
 * into it; image_sizes HOST int32 [B, V, 2] = (H_img, W_img).  They travel in a kernel's arguments: B V <= 128 with out_colors.
 *   1. hypotheses of pixel q of view v: its slots are the halves on v's grid, in ascending p (of one pair in both orders: the
 *      order of the rows of pair_views).  A slot is usable when its flag byte is 0, its depth z is finite and > 0 and its weight
 *      w (the certainty, or 1) is finite and > 0.
 *   2. support: slot l supports slot k when both are usable and |z_l - z_k| <= rel_thresh * min(z_l, z_k) (one product); a slot
 *      supports itself.  n_k = the supporters of k, s_k = the sum of their w and m_k = the sum of their w z (each product rounded),
 *      both added in slot order starting from 0.
 *   3. select: the usable slot with the largest n_k, then the largest s_k, then the lowest slot.  n < min_support (in [1, 14]):
 *      depth NaN, weight 0, support = the best n (0 without a usable slot).  Otherwise depth = fl32(m_k / s_k), weight = fl32(s_k),
 *      support = n.
 *   4. cross-view check, on the maps of step 3, after a kernel boundary.  A pixel (r, c) of view v with depth z:
 *      x = (((c + 0.5) - cx) / fx, ((r + 0.5) - cy) / fy), d = (z x0 - t0, z x1 - t1, z - t2), X_w = R_v^T d with
 *      X_w[i] = (R[0][i] d0 + R[1][i] d1) + R[2][i] d2.  For every other valid view u: X' = R_u X_w + t_u with
 *      X'[i] = ((R[i][0] X0 + R[i][1] X1) + R[i][2] X2) + t[i]; not X'_z > 0: no support.  g = (fx (X'_x / X'_z) + cx - 0.5,
 *      fy (X'_y / X'_z) + cy - 0.5) is its position on u's grid (align_corners = False); x0 = floor(g_x), y0 = floor(g_y); support
 *      only if 0 <= x0, x0 + 1 <= W - 1, 0 <= y0, y0 + 1 <= H - 1 and the four neighbours all have a depth; dd = the bilinear
 *      expression of roma_op_depth_consistency on them; e = (X'_z - dd) / dd.  |e| <= rel_thresh sets bit u of seen; e < -rel_thresh
 *      sets bit u of violated (the point floats in front of the surface u sees); e > rel_thresh sets neither (occluded in u).
 *      keep = popcount(seen) >= min_consistent and popcount(violated) <= max_violations.
 *   5. duplicates (dedupe = 1), after another kernel boundary, from step 4's keep alone: a kept pixel of view v is a duplicate
 *      when for some u < v bit u of its seen is set and the pixel (floor(g_y + 0.5), floor(g_x + 0.5)) of u lies inside the grid and
 *      is kept.
 *   6. emission: the pixels that are kept and no duplicates are numbered in the order (view ascending, row-major pixel) by block
 *      counts, one workgroup per problem for their exclusive prefix, and ballot ranks - independent of the schedule.  The first
 *      max_points are written, total reports all of them.  The colour of a point is the image pixel that holds the centre of
 *      its cell: (((2 r + 1) H_img) / (2 H), ((2 c + 1) W_img) / (2 W)) in integer division.
 * Outputs, all DEVICE.  Per view: depth f32 [B, V, H, W] (NaN where none), weight f32, support u8, seen u8, violated u8 (bit masks
 * over views), state u8 (bit 0 kept, bit 1 duplicate).  Cloud: points f32 [B, max_points, 3] = fl32(X_w), NaN padding; colors u8
 * [B, max_points, 3] or NULL, 0 padding; cloud_weight f32 [B, max_points] (the pixel's weight), 0 padding; source int32
 * [B, max_points, 2] = (view, r W + c), -1 padding; counts int32 [B] = min(total, max_points); total int32 [B]; stats int32 [B, 8] =
 * {pixels with a usable slot, fused, kept, duplicates, emitted, pixels with a violation, 0, 0}: integer atomics, one per workgroup
 * that has something to count, cleared on the stream by the same call.  Every element of every output is written.
 * Five kernels on the stream (select, check, dedupe, scan, emit), one thread per pixel, the cameras and poses of the views staged
 * once per workgroup; no host read; the workspace (roma_op_fuse_depth_maps_workspace bytes, 0 for an empty or refused problem:
 * one byte per pixel and one int32 per block of 256 pixels) need not be cleared.  Bit-identical from run to run and independent
 * of B.  Refused before anything is enqueued: a null required pointer, V outside [2, 8], P outside [1, 64], B > 65535, H or W
 * below 1, symmetric or dedupe not 0 or 1, a negative (or NaN) rel_thresh, min_support outside [1, 14], min_consistent outside
 * [0, 7], negative max_violations or max_points, a pair_views entry out of range, a pair of a view with itself, an ordered pair
 * twice, a partial colour source or out_colors without one, B P H Wd, B V H W or 3 B max_points >= 2^31, a workspace that is too
 * small.  B = 0 launches nothing. */
long roma_op_fuse_depth_maps_workspace(int B, int V, int H, int W);
int roma_op_fuse_depth_maps(const float* points, const unsigned char* flags, const float* certainty, const int* pair_views,
                            const double* cameras, const double* R, const double* t, const unsigned char* view_valid,
                            const unsigned char* valid, const unsigned char* images, const long long* image_offsets,
                            const int* image_sizes, int B, int V, int P, int H, int W, int symmetric, double rel_thresh,
                            int min_support, int min_consistent, int max_violations, int dedupe, int max_points, float* out_depth,
                            float* out_weight, unsigned char* out_support, unsigned char* out_seen, unsigned char* out_violated,
                            unsigned char* out_state, float* out_points, unsigned char* out_colors, float* out_cloud_weight,
                            int* out_source, int* out_counts, int* out_total, int* out_stats, void* workspace, long workspace_bytes,
                            void* stream);
/* The pose of every pair from the poses of the views, x_cam = R X + t: R_ij = R_j R_i^T with R_ij[a][c] = (R_j[a][0] R_i[c][0] +
 * R_j[a][1] R_i[c][1]) + R_j[a][2] R_i[c][2], t_ij[a] = t_j[a] - ((R_ij[a][0] t_i[0] + R_ij[a][1] t_i[1]) + R_ij[a][2] t_i[2]) - the
 * (A to B) pose roma_op_triangulate takes for pair (i, j).  R DEVICE f64 [B, V, 3, 3], t DEVICE f64 [B, V, 3], pair_views HOST int32
 * [P, 2] (1 <= P <= 64, both views in [0, V) and different); out_R DEVICE f64 [B, P, 3, 3], out_t DEVICE f64 [B, P, 3].  One launch,
 * float64 with fp contraction off; restated by tools/depth_fusion_ref.py. */
int roma_op_relative_poses(const double* R, const double* t, const int* pair_views, int B, int V, int P, double* out_R, double* out_t,
                           void* stream);
/* Point-cloud rendering: the N rows of a world-space point cloud splatted into C cameras per problem with a z-buffer, then an
 * occlusion filter and a hole fill - depth, row index, colour and a mask per pixel of every frame.  What a dense reconstruction is
 * looked at with (a turntable of novel views), localised against (the depth map of the whole cloud in a registered camera) and
 * checked with (its depth in a camera that has sensor depth, or in one of its own).  Restated operation by operation in numpy
 * float64 by tools/point_render_ref.py.  All arithmetic is float64 in the order written, with fp contraction off; depths are
 * stored as float32.
 * points DEVICE f32 [B, N, 3] world points, the cloud of roma_op_fuse_depth_maps with its NaN padding taken as it is; colors DEVICE
 * u8 [B, N, 3] or NULL; counts DEVICE int32 [B] or NULL: rows n >= min(max(counts[b], 0), N) are ignored; valid DEVICE u8 [B] or
 * NULL: a problem that is not valid renders empty.  cameras DEVICE f64 [B, C, 3, 3], applied by fx, fy, cx, cy, in units of the
 * output pixel: the centre of pixel (r, c) is (c + 0.5, r + 0.5), the convention of roma_op_fuse_depth_maps.  R DEVICE f64
 * [B, C, 3, 3], t DEVICE f64 [B, C, 3], x_cam = R X + t.  H, W: the size of every frame.  background = r | g << 8 | b << 16, the
 * colour of a pixel without a point.
 *   1. splat.  Row n of problem b is usable for camera k when its three coordinates are finite; near <= X'_z <= far with
 *      X'[i] = ((R[i][0] X0 + R[i][1] X1) + R[i][2] X2) + t[i], X widened from float32; zf = fl32(X'_z) is finite and > 0;
 *      u = fx (X'_x / X'_z) + cx and v = fy (X'_y / X'_z) + cy are finite; and -radius <= floor(u) < W + radius, -radius <=
 *      floor(v) < H + radius, decided in double before any conversion to an integer.  With c0 = floor(u), r0 = floor(v) it offers
 *      the key (bits(zf) << 32) | n to every pixel (r, c) of the image with |r - r0| <= radius and |c - c0| <= radius.  A pixel
 *      holds the minimum of the keys offered to it - the nearest depth, then the lowest row; all ones means empty.  Integer minima
 *      do not depend on the order of arrival.
 *   2. occlusion filter (occlusion_radius o > 0), after a kernel boundary, on the raw buffer of step 1 only: a hit pixel of depth z
 *      is removed when at least occlusion_count hit pixels q of its (2 o + 1)^2 window, clipped to the image, are nearer by more
 *      than occlusion_rel: (double)z > (double)z_q * (1.0 + occlusion_rel), one product.  These are the points of a back surface
 *      that show through the gaps of a nearer one.  o = 0 removes nothing.
 *   3. fill (fill_radius f > 0), after another kernel boundary, from step 2's decisions alone: a pixel that is empty or removed
 *      counts the surviving pixels (hit and not removed) of its clipped (2 f + 1)^2 window and with at least fill_min of them takes
 *      the smallest of their keys.  f = 0 fills nothing.  Known: at a depth edge the nearer surface grows by up to o + f pixels -
 *      the filter removes the far pixels next to the edge and the fill closes them with the near key.
 *   4. resolve, per pixel from its final key or none.
 * Outputs, all DEVICE, [B, C, H, W]: out_depth f32 = zf, NaN if empty; out_index int32 = the row, -1 if empty; out_color u8
 * [B, C, H, W, 3] = the row's colour, background if empty, NULL exactly when colors is; out_mask u8: bit 0 hit in step 1, bit 1
 * removed, bit 2 filled; out_stats int32 [B, C, 4] = {usable rows with (r0, c0) inside the image, pixels hit, pixels removed, pixels
 * filled}: integer atomics, one per workgroup that has something to count, cleared on the stream by the same call.  Every element
 * of every output is written.
 * A clear (two memsets) and three kernels on the stream: splat with grid (blocks of 256 rows, camera, problem), the camera staged
 * once per workgroup, 64-bit atomicMin behind a plain load of the current key (a key only ever decreases, so the load is exact: it
 * can only skip an atomic that would change nothing); filter and fill with one thread per pixel.  No host read.  The workspace
 * (roma_op_render_points_workspace bytes, 0 for an empty or refused problem: 8 bytes per pixel for the keys and one for step 2's
 * decision) need not be cleared: the call initialises whatever it reads.  Bit-identical from run to run, independent of B and of C:
 * a frame rendered alone equals the same frame in a batch.  Refused before anything is enqueued: a null required pointer, colors
 * without out_color or the reverse, C < 1, B < 0 or B C > 65535, H or W below 1, N < 0 (N = 0 renders empty), radius,
 * occlusion_radius or fill_radius outside [0, 4], occlusion_count or fill_min below 1, a negative (or NaN) occlusion_rel, near not
 * > 0, far < near (or NaN; +inf is allowed), a background outside [0, 0xFFFFFF], 3 B C H W >= 2^31, a workspace that is too small.
 * B = 0 launches nothing. */
long roma_op_render_points_workspace(int B, int C, int H, int W);
int roma_op_render_points(const float* points, const unsigned char* colors, const int* counts, const unsigned char* valid,
                          const double* cameras, const double* R, const double* t, int B, int N, int C, int H, int W, int radius,
                          double near, double far, int occlusion_radius, double occlusion_rel, int occlusion_count, int fill_radius,
                          int fill_min, int background, unsigned char* out_color, float* out_depth, int* out_index,
                          unsigned char* out_mask, int* out_stats, void* workspace, long workspace_bytes, void* stream);
/* Ground-truth warp from SENSOR depth - the reference's warp_kpts / get_gt_warp (romatch/utils/utils.py) - and the dense EPE / PCK
 * metrics of a warp against it - MegadepthDenseBenchmark.geometric_dist in one pass.  The sensor-depth twin of
 * roma_op_depth_consistency.  Restated operation by operation in numpy float64 by tools/gt_warp_ref.py.  All arithmetic is float64
 * in the order written, with fp contraction off, except the one float32 line marked below; depth and key points are widened exactly.
 *   sample(D [Hs, Ws], x, y), torch grid_sample bilinear, align_corners=False, zeros padding:
 *     ix = ((x + 1) Ws - 1) / 2, iy likewise; x0 = floor(ix), y0 = floor(iy); weights w_nw = (x0+1-ix)(y0+1-iy),
 *     w_ne = (ix-x0)(y0+1-iy), w_sw = (x0+1-ix)(iy-y0), w_se = (ix-x0)(iy-y0); result = v_nw w_nw + v_ne w_ne + v_sw w_sw + v_se w_se
 *     added left to right, where a tap outside the map contributes 0 (not 0 times its weight).  In and out of range is decided in
 *     float64 (0 <= x0 <= Ws - 1 and so on; NaN fails) before any conversion to an integer: a coordinate of 1e7 pixels or a
 *     non-finite one samples 0 and forms no address.
 *   key point (x, y) normalised in image 0:  px = W0 (x + 1) / 2, py = H0 (y + 1) / 2, d0 = sample(depth0, x, y), nonzero = d0 != 0
 *   K0inv = adjugate / determinant of the general 3 x 3 K0 = [a b c; d e f; g h i]:  cofactors c00 = e i - f h, c01 = c h - b i,
 *     c02 = b f - c e, c10 = f g - d i, c11 = a i - c g, c12 = c d - a f, c20 = d h - e g, c21 = b g - a h, c22 = a e - b d,
 *     det = (a c00 + b c10) + c c20, K0inv[r][q] = c_rq / det; formed once per workgroup, not per thread
 *   X = K0inv (px d0, py d0, d0), Y = R X + t, zc = Y_z, P = K1 Y: each row is (m0 v0 + m1 v1) + m2 v2 (then + t_r for Y)
 *   u = P_x / (P_z + 1e-4), v = P_y / (P_z + 1e-4); covisible = u > 0 && u < W1 - 1 && v > 0 && v < H1 - 1
 *   warped = (2 u / W1 - 1, 2 v / H1 - 1), written for every row, valid or not
 *   d1 = sample(depth1, warped), rel = |(d1 - zc) / d1| (+-inf for a zero d1, NaN for 0 / 0); consistent = rel < rel_thresh (false
 *   for NaN); valid = nonzero && covisible && consistent.
 * roma_op_warp_kpts: kpts DEVICE [B, L, 2], float32 (kpts_f64 = 0) or float64 (1), or NULL: the key points are then the pixel
 * centres of a grid_h x grid_w grid (L = grid_h grid_w, row-major), value j of n being float32((2 j + 1) / n - 1) formed in float64,
 * rounded once to float32 and widened again - no grid tensor exists.  depth0 DEVICE f32 [B, H0, W0], depth1 f32 [B, H1, W1];
 * T DEVICE f64 [B, t_rows, 4], t_rows 3 or 4 (rows 0..2 = [R | t], camera 0 to camera 1); K0, K1 DEVICE f64 [B, 3, 3].  Outputs,
 * DEVICE, the first three nullable: valid u8 [B, L] (0 / 1), prob f32 [B, L] (0.0 / 1.0, get_gt_warp's form), rel f64 [B, L],
 * warped f64 [B, L, 2].  One launch, no workspace, no host read; every bit is independent of B, of the order of the pairs and of
 * the run.  Refused before anything is enqueued: a null required pointer, B < 0 or > 65535, L < 0, B L >= 2^31, t_rows not 3 or
 * 4, kpts_f64 not 0 or 1, a depth size outside [1, 32768], kpts NULL with a grid outside [1, 32768]^2 or grid_h grid_w != L, kpts
 * not aligned to its type, a negative (or NaN) rel_thresh.  B = 0 or L = 0 launches nothing.
 * roma_op_dense_metrics: matches DEVICE f32, 16-byte aligned, pixel (b, r, c) at matches + b batch_stride + r row_stride + 4 c
 * (strides in floats, multiples of 4: a contiguous [B, h, w, 4] warp has row_stride = 4 w, the left half of a symmetric
 * [B, h, 2w, 4] warp row_stride = 8 w, read in place).  Columns 0:2 are the key points in image 1 (camera K1, depth1 [B, H1, W1]),
 * columns 2:4 the prediction in image 2 (K2, depth2 [B, H2, W2]); the chain above gives valid and warped per pixel.  The pixel
 * scale is the warp grid's (h, w), not depth2's size (the reference's convention):
 *   prediction, in FLOAT32 as the reference forms it, then widened:  xh = float32(float32(w * float32(x^ + 1)) / 2), yh with h
 *   truth in float64: tx = w (warped_x + 1) / 2, ty = h (warped_y + 1) / 2;  gd = sqrt(dx dx + dy dy), dx = xh - tx, dy = yh - ty
 * Outputs, DEVICE: n_valid int64 [B]; n_below int64 [B, 3], valid pixels with gd < thr0, thr1, thr2; gd_sum f64 [B] over the valid
 * pixels - each thread sums its pixels in ascending index, then a fixed tree over the wave, the waves in order, and the
 * per-workgroup partials in index order by a finishing kernel; no float is added atomically; the workgroups of a pair do not
 * depend on B, so the per-pair outputs are bit-identical for any batch and pair order.  epe f64 [1] = sum_b gd_sum / sum_b
 * n_valid and pck f64 [3] = sum_b n_below / sum_b n_valid, the sums in pair order (NaN when no pixel of the batch is valid:
 * the mean of an empty selection).  Nullable maps prob f32 [B, h, w] and gd f64 [B, h, w], NaN where prob == 0.  workspace:
 * DEVICE, 8-byte aligned, roma_op_dense_metrics_workspace(B, h, w) bytes (-1 for sizes that are refused).  Two launches, no host
 * read.  Refused before anything is enqueued: a null required pointer, B < 1 or > 65535, h or w outside [1, 32768], B h w >=
 * 2^31, t_rows not 3 or 4, a depth size outside [1, 32768], strides that are not multiples of 4 or let rows overlap, matches or
 * workspace not aligned as stated, a negative (or NaN) threshold, a workspace that is too small. */
int roma_op_warp_kpts(const void* kpts, int kpts_f64, int grid_h, int grid_w, const float* depth0, const float* depth1, const double* T,
                      int t_rows, const double* K0, const double* K1, int B, long L, int H0, int W0, int H1, int W1, double rel_thresh,
                      unsigned char* out_valid, float* out_prob, double* out_rel, double* out_warped, void* stream);
long roma_op_dense_metrics_workspace(int B, int h, int w);
int roma_op_dense_metrics(const float* matches, long batch_stride, long row_stride, const float* depth1, const float* depth2,
                          const double* T, int t_rows, const double* K1, const double* K2, int B, int h, int w, int H1, int W1, int H2,
                          int W2, double rel_thresh, double thr0, double thr1, double thr2, long long* out_n_valid,
                          long long* out_n_below, double* out_gd_sum, double* out_epe, double* out_pck, float* out_prob, double* out_gd,
                          void* workspace, long workspace_bytes, void* stream);
/* Scoring of the pose and homography benchmarks - the reference's compute_pose_error and pose_auc (romatch/utils/utils.py:115-147),
 * the accuracy / mAP lines of its MegaDepth and ScanNet pose benchmarks and the corner distance of its HPatches benchmark
 * (hpatches_sequences_homog_benchmark.py:89-104) - so that a loop of roma_op_essential / roma_op_recover_pose or roma_op_ransac
 * calls is scored with no host read before the final summary.  Restated operation by operation in numpy float64 by
 * tools/metrics_ref.py.  All arithmetic is float64 in the order written, with fp contraction off; clip(c) = c < -1 ? -1 : (c > 1 ?
 * 1 : c) keeps a NaN; DEG = 180.0 / pi as a double (numpy's rad2deg factor).  Every kernel is one workgroup; every output is
 * bit-identical from run to run.
 * The ERROR LOG is device memory: double log[capacity] and long long state[2] = {count, dropped}, both zero at first.  The three
 * entries that take (log, capacity, state) append their B values in the launch that computes them: the launch reads count, writes
 * value i to log[count + i] where count + i < capacity, then stores count + B and adds the number of values that did not fit to
 * dropped (count keeps counting them).  No host value takes part; successive appends are ordered by the stream.  log and state NULL:
 * no log.
 * roma_op_pose_error: R DEVICE f64 [B, 3, 3], t f64 [B, 3], ok u8 [B] or NULL (all ok), T_gt f64 [B, t_rows, 4], t_rows 3 or 4
 * (rows 0..2 = [R_gt | t_gt]).  out_err f64 [B, 3] = (e_t, e_R, e_pose) in degrees:
 *   n = sqrt((t0 t0 + t1 t1) + t2 t2) sqrt((g0 g0 + g1 g1) + g2 g2), a = acos(clip(((t0 g0 + t1 g1) + t2 g2) / n)) DEG,
 *   e_t = (180 - a) < a ? 180 - a : a   (NaN for a t or t_gt of zero norm, as np.minimum keeps it)
 *   tr = the nine products R[r][q] R_gt[r][q] added in row-major order (the trace of R^T R_gt), e_R = |acos(clip((tr - 1) / 2))| DEG
 *   e_pose = e_R > e_t ? e_R : e_t   (Python's max(e_t, e_R): a NaN e_t stays)
 *   a pair with ok == 0 gets (90, 90, 90) whatever R and t hold - the except branch of the benchmarks.
 * e_pose is what goes to the log.
 * roma_op_corner_error: H_pred DEVICE f64 [B, 3, 3], ok u8 [B] or NULL, H_gt f64 [B, 3, 3], sizes f64 [B, 4] = (w1, h1, w2, h2).
 * out_err f64 [B]: for the corners (x, y) = (0, 0), (0, h1 - 1), (w1 - 1, 0), (w1 - 1, h1 - 1), in this order, and either matrix
 *   X = (H00 x + H01 y) + H02, Y and Z likewise, p = (X / Z, Y / Z); d = sqrt(dx dx + dy dy) with dx = p_gt.x - p_pred.x;
 *   out = ((((0 + d0) + d1) + d2) + d3) / 4 / (min(w2, h2) / 480), min(w2, h2) = w2 < h2 ? w2 : h2.
 * ok == 0 replaces H_pred by [[0, 0, 0], [0, 0, 0], [0, 0, 1]] (the reference's stand-in); inf and NaN of a zero Z propagate.
 * roma_op_error_log_append: values DEVICE f64 [B], already computed, appended as above.
 * roma_op_error_summary: errors DEVICE f64, not negative (NaN and +inf allowed).  Their number N is n (state NULL, 0 <= n <= 65536)
 * or min(state[0], capacity), read on the device (state the log's, errors its rows, capacity <= 65536).  thresholds HOST f64 [T],
 * 1 <= T <= 16, positive and finite; they travel in the kernel arguments.  One launch.  Per threshold thr: L = the number of errors
 * < thr (strictly, as searchsorted on the left and the benchmarks' `<`; NaN and +inf are never below), S their sum, M their
 * maximum (0 for L = 0) - per thread (256) over its errors in ascending index, a shuffle tree over the wave (offsets 32 .. 1), the
 * four waves in order; no float atomics.  out_n i64 [1] = N, out_below i64 [T] = L, out_acc f64 [T] = L / N, out_auc f64 [T] =
 * (((L thr) - S) + M / 2) / (N thr): the trapezoid under the recall curve from 0 to thr that pose_auc sorts for, telescoped.
 * N = 0 gives NaN in acc and auc (0 / 0).
 * Refused before anything is enqueued: a null required pointer, B < 0 or > 65535, t_rows not 3 or 4, an array that is not 8-byte
 * aligned, a log without its state or the reverse, capacity < 1, more than 65536 errors, T outside [1, 16], a threshold that is
 * not positive and finite.  B = 0 launches nothing. */
int roma_op_pose_error(const double* R, const double* t, const unsigned char* ok, const double* T_gt, int t_rows, int B, double* out_err,
                       double* log, long capacity, long long* state, void* stream);
int roma_op_corner_error(const double* H_pred, const unsigned char* ok, const double* H_gt, const double* sizes, int B, double* out_err,
                         double* log, long capacity, long long* state, void* stream);
int roma_op_error_log_append(const double* values, int B, double* log, long capacity, long long* state, void* stream);
int roma_op_error_summary(const double* errors, long n, const long long* state, long capacity, const double* thresholds, int T,
                          long long* out_n, long long* out_below, double* out_acc, double* out_auc, void* stream);
/* Warp morph rendering - the frames of the reference's demo/demo_3D_effect.py, F.grid_sample(image B, (1 - t) warp[..., :2] +
 * t warp[..., 2:]) through tensor_to_pil for every t of a schedule - in one enqueue.  Restated operation by operation in numpy
 * float32 by tools/morph_ref.py.  Per frame t and pixel, every step in float32 in the order written, one rounding per operation,
 * fp contraction off:
 *   weights     w0 = float32(1.0 - t), w1 = float32(t), formed in float64 and rounded once (what the reference's Python scalars become
 *               when they multiply a float32 tensor); any real t, also outside [0, 1]
 *   coordinate  gx = w0 ax + w1 bx, gy = w0 ay + w1 by for the warp row (ax, ay, bx, by): two rounded products, a rounded sum
 *   unnormalise ix = ((gx + 1) w - 1) 0.5 clamped to +-1e6 as min(max(ix, -1e6), 1e6) (a NaN becomes -1e6), iy with h - as
 *               visualize_warp_kernel
 *   sample      x0 = floor(ix), y0 = floor(iy), tx = ix - x0, ty = iy - y0; taps (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1) with
 *               weights (1-tx)(1-ty), tx (1-ty), (1-tx) ty, tx ty; per channel v = 0, then v = v + weight * value tap by tap in that
 *               order, a tap outside the image having the value 0 (zeros padding; no texel it does not cover is read)
 *   blend       with certainty c: v = c v + (1 - c) background (visualize_warp's blend over white, for background = 1)
 *   uint8       (unsigned char)(min(max(v, 0), 1) * 255.f): truncation, as numpy_to_pil; NaN -> 0
 * warp DEVICE f32, 16-byte aligned, pixel (b, r, c) at warp + b warp_batch_stride + r warp_row_stride + 4 c (strides in floats,
 * multiples of 4, as roma_op_dense_metrics takes them: the left half of a symmetric [H, 2W, 4] warp is read in place).  image
 * DEVICE, contiguous: f32 [B, 3, im_h, im_w] (image_u8 = 0) or uint8 [B, im_h, im_w, 3] (image_u8 = 1), used as float(u) / 255.f
 * with a correctly rounded division - the same bits as the f32 form of the same picture; (im_h, im_w) is independent of (H, W).
 * ts DEVICE f64 [T].  certainty: NULL, or DEVICE f32 with pixel (b, r, c) at certainty + b cert_batch_stride + r cert_row_stride +
 * c.  out DEVICE: uint8 [B, T, H, W, 3] (out_f32 = 0) or f32 [B, T, 3, H, W] (out_f32 = 1, the frames before the uint8 step).
 * workspace DEVICE, 16-byte aligned, roma_op_render_morph_workspace(B, im_h, im_w, T) bytes (-1 for sizes that are refused): a
 * first kernel packs the picture into 16-byte (r, g, b, 0) texels there, so that a tap is one load, and the T weight pairs; the
 * second renders, a wave taking 256 consecutive pixels of the flattened frame (four per lane, 64 apart), which load their warp
 * rows once and loop over roma_op_render_morph_frame_chunk() frames - frame chunks and B are the other grid axes.  A wave's 768
 * bytes of a uint8 frame leave as three coalesced dwords per lane where the frame's first byte is dword aligned (always when H W
 * is a multiple of 4) and the wave is full, and byte by byte elsewhere.  Two
 * launches on the caller's stream, no host read, no allocation; every bit is independent of B, of the pair's place and of the run.
 * Refused before anything is enqueued: a null required pointer, B outside [1, 65535], T < 1 or > 65535 frame chunks, H, W, im_h or
 * im_w outside [1, 32768], image_u8 or out_f32 not 0 or 1, B T H W 3 beyond 9e15, strides that are not multiples of 4 (warp) or
 * let rows overlap, a pointer not aligned as stated, a NaN background, a workspace that is too small, out or workspace sharing a
 * byte with an input or with each other. */
int roma_op_render_morph_frame_chunk(void);
long roma_op_render_morph_workspace(int B, int im_h, int im_w, long T);
int roma_op_render_morph(const float* warp, long warp_batch_stride, long warp_row_stride, const void* image, int image_u8, const double* ts,
                         const float* certainty, long cert_batch_stride, long cert_row_stride, float background, int B, long T, int H,
                         int W, int im_h, int im_w, void* out, int out_f32, void* workspace, long workspace_bytes, void* stream);
/* RegressionMatcher.match_keypoints (matcher.py:732-773) for B pairs in one enqueue: five launches whatever B is, no host read, no
 * allocation, the result padded and counted so that it feeds roma_op_ransac and its neighbours through `counts`.  Restated in numpy
 * float32 by tools/keypoints_ref.py.  For pair b let na = min(max(counts_a[b], 0), NA) and nb likewise (NULL counts: NA / NB); the
 * definition is the reference's on the pair's first na rows of x_a [B, NA, 2] and nb rows of x_b [B, NB, 2] (normalised (x, y)):
 *   sample    p_i = bilinear(warp[b][..., 2:4], x_a[b, i]), c_i = bilinear(certainty[b], x_a[b, i]): zeros padding,
 *             align_corners = False, the tap rule, the +-1e6 clamp and the float32 expression of roma_op_sample_warp_at (same bits)
 *   distance  d2(i, j) = fmaf(dy, dy, dx * dx) in float32 with (dx, dy) = p_i - x_b[b, j], the expression of roma_op_mutual_nn
 *   pairs     (i, j) is returned iff d2(i, j) equals the minimum of row i over j < nb AND the minimum of column j over i < na AND
 *             c_i > cert_th AND d2(i, j) < max_dist * max_dist - EVERY tied pair, as the reference's torch.nonzero returns them, in
 *             row-major order (i ascending, then j ascending).  A NaN distance is never a minimum.
 *   counts    total[b] (int64) = the number of such pairs; counts[b] (int32) = min(total[b], M); only the first M pairs in that order
 *             are written.  Duplicate keypoints tie, so total[b] can exceed na: M is the caller's choice.
 *   outputs   inds [B, M, 2] int32 (index into A, index into B); kpts_a, kpts_b [B, M, 2] f32 = the caller's own rows x_a[b, i] and
 *             x_b[b, j] (not p_i); rows at or beyond counts[b] hold -1 in inds and 0 in both kpts.
 *   sizes     NULL, or DEVICE f32 (H_A, W_A, H_B, W_B) of pair b at sizes + b sizes_batch_stride (stride 0: one row for all): kpts
 *             then come out in pixels, (W * 0.5f) * (x + 1.0f) and (H * 0.5f) * (y + 1.0f) in float32 - to_pixel_coordinates' bits.
 * All pointers DEVICE.  warp f32, 16-byte aligned, pixel (b, r, c) at warp + b warp_batch_stride + r warp_row_stride + 4 c (strides
 * in floats, multiples of 4, as roma_op_render_morph takes them: the A -> B half of a symmetric [B, H, 2W, 4] warp is read in place);
 * certainty f32, pixel (b, r, c) at certainty + b cert_batch_stride + r cert_row_stride + c.  Rows of x_a / x_b at or beyond the
 * counts are never read.  workspace: 16-byte aligned, roma_op_match_keypoints_workspace(B, NA, NB) bytes (-1 for sizes that are
 * refused); it starts with p [B, NA, 2] f32 and, at the next multiple of 16 bytes, c [B, NA] f32 (rows below na written), then
 * holds the bits of the row and column minima and the int64 positions.
 * A pair's outputs are a function of that pair's rows alone: bit-identical from run to run, for every B, every place in the batch
 * and every padding width NA / NB.  No output position comes from an atomic; slices of a row's or column's candidates are merged
 * by an integer minimum on the bits of d2 >= 0, which is the same in any order.
 * Refused before anything is enqueued: a null pointer (x_a may be NULL where NA = 0, x_b where NB = 0; counts_a, counts_b and
 * sizes are optional), B outside [1, 65535], NA or NB outside [0, 2^20], M outside [1, 2^31 - 1], H or W outside [1, 32768], warp
 * strides that are not multiples of 4 or let rows overlap, certainty strides that let rows overlap, a sizes stride in (0, 4), warp
 * or workspace not 16-byte aligned, another pointer not aligned to its type, a NaN max_dist or cert_th, a workspace that is too
 * small.  NA = 0 or NB = 0 is valid and gives zero counts. */
long roma_op_match_keypoints_workspace(int B, long NA, long NB);
int roma_op_match_keypoints(const float* x_a, const float* x_b, const int* counts_a, const int* counts_b, const float* warp,
                            long warp_batch_stride, long warp_row_stride, const float* certainty, long cert_batch_stride,
                            long cert_row_stride, const float* sizes, long sizes_batch_stride, int B, long NA, long NB, int H, int W,
                            float max_dist, float cert_th, long M, int* inds, float* kpts_a, float* kpts_b, int* counts,
                            long long* total, void* workspace, long workspace_bytes, void* stream);
/* Image preprocessing: Pillow's 8-bit bicubic resize (Image.resize((w, h), Image.BICUBIC) on a mode-RGB image, which is what
 * transforms.Resize(size, BICUBIC) does to a PIL image) of a batch of packed RGB images of mixed sizes to one or two target sizes,
 * then / 255 and the ImageNet mean / std of the matcher's host path - bit-identical to that path (roma_amd/matcher.py:
 * _pil_to_normalised), restated in numpy by tools/pil_resample_ref.py.  The output is what roma_match takes: float32 NCHW.
 * Pillow resamples in fixed point in TWO PASSES, HORIZONTAL FIRST, THEN VERTICAL, and the intermediate image is rounded and clamped
 * to uint8 between the passes (so no float bicubic can match it, and the order matters):
 *   PRECISION_BITS = 22
 *   bicubic(x), a = -0.5:  x = |x|;  x < 1: ((a+2)x - (a+3)) x x + 1;   x < 2: (((x-5)x + 8)x - 4) a;   else 0
 *   coefficients of one axis, in -> out, all in float64, no contraction, sums in index order:
 *     scale = in / out;  fs = max(scale, 1);  support = 2 fs;  ss = 1 / fs
 *     for each output xx:  center = (xx + 0.5) scale
 *         xmin = max(0, (int)(center - support + 0.5));  xmax = min(in, (int)(center + support + 0.5));  n = xmax - xmin
 *         k[i] = bicubic((i + xmin - center + 0.5) ss), i < n;   ww = sum k[i];   if ww != 0: k[i] /= ww
 *         K[i] = (int)(k[i] * 2^22 + 0.5) if k[i] >= 0 else (int)(k[i] * 2^22 - 0.5)        ((int) truncates toward zero)
 *   one pass, per channel:  s = 2^21 + sum_i pixel[xmin + i] * K[i]  (int32);   out = clamp(s >> 22, 0, 255)   (arithmetic shift)
 *   an axis whose size does not change is skipped (the pass is not run); both unchanged = a copy
 * then, all in float32, out = (float32(u) / float32(255) - mean_c) / std_c with mean = (0.485, 0.456, 0.406), std = (0.229, 0.224,
 * 0.225); normalize = 0 stops after the / 255 (what visualize_warp feeds on).  Evaluated through a table of 3 x 256 entries.
 * src DEVICE u8, 4-byte aligned, src_bytes long: the images, each contiguous [H, W, 3]; desc = {byte offset into src, H, W} per
 * image (int64 x 3, any offset alignment), once on the HOST (it sizes the grid and the workspace and is validated) and once on the
 * DEVICE (what the kernels read; 8-byte aligned).  An image whose device descriptor exceeds the largest H or W of the host copy, or
 * src_bytes, is skipped by the kernels: its output is left unwritten, nothing is read or written out of bounds.  targets_hw HOST
 * int32 [n_targets, 2] = (h, w), n_targets 1 or 2 (the coarse and the upsample resolution of one matcher from one upload); out0
 * (and out1 for the second target, NULL when there is one) DEVICE f32 [n_images, 3, h_t, w_t].  workspace: DEVICE, 16-byte aligned,
 * roma_op_preprocess_workspace(desc_host, n_images, targets_hw, n_targets) bytes (-1 for arguments that are refused): the
 * normalisation table, the coefficient tables and the uint8 [H, w_t, 3] intermediates (rows padded to whole dwords), in equal
 * slots sized by the largest image.  Three kernels in one enqueue on `stream` (coefficient and normalisation tables, in float64
 * with contraction off; horizontal pass; vertical pass + table lookup), no host read, no synchronisation; every output bit is
 * independent of the batch, of the order of the images and of the run.
 * Refused on the host before anything is enqueued (nonzero, text in roma_last_error): a null pointer; n_targets not 1 or 2;
 * n_images < 1 or > 65535; a target below 1 or above 32768; an image with H or W below 1 or above 32768, a negative offset, or
 * offset + 3 H W > src_bytes; src, desc_dev or workspace not aligned as stated. */
long roma_op_preprocess_workspace(const long long* desc_host, int n_images, const int* targets_hw, int n_targets);
int roma_op_preprocess(const unsigned char* src, long long src_bytes, const long long* desc_host, const long long* desc_dev,
                       int n_images, const int* targets_hw, int n_targets, int normalize, float* out0, float* out1, void* workspace,
                       void* stream);
/* ---- Tiny RoMa (romatch/models/tiny.py), matcher side; the XFeat backbone is the caller's (model_zoo/__init__.py:24-27).
 * All tensors f32, channels-last unless noted.  corr_volume (tiny.py:182-196) = roma_op_gemm with A = feats of image B
 * [H1*W1, C], W = feats of image A [H0*W0, C], alpha = 1/sqrt(C), batch = pairs: cv [B, H1*W1, H0*W0]. */
int roma_op_nchw_to_nhwc(const float* in, float* out, int B, int C, int H, int W, void* stream);
/* pos_embed (tiny.py:114-142): out [B, H0*W0, 2].  exact_softmax = 0: the inference path, soft arg-max over the
 * 4x-subsampled correlation column plus the arg-max position (H1, W1 multiples of 4); 1: the exact_softmax=True branch
 * (tiny.py:139-141), the softmax over all H1 x W1 positions. */
int roma_op_tiny_pos_embed(const float* corr_volume, float* out, int B, int H1, int W1, int H0, int W0, int exact_softmax,
                           void* stream);
/* TinyRoMa.forward_single (tiny.py:81-99) - the caller's XFeat network, replayed layer by layer, channels-last f32:
 * gray_instnorm: out [B,H,W,1] = InstanceNorm2d(1)(mean over the C channels of in [B,H,W,C]) (no affine, biased variance);
 * conv2d_nhwc: out [B,Ho,Wo,Cout] = act(conv(in [B,H,W,Cin], w [K*K*Cin][Cout] (tap-major, BatchNorm folded)) + bias) + res;
 *   K 1 or 3, stride 1 or 2, padding 0 or 1, Cout % 4 == 0; bias, res may be NULL;  avgpool_nhwc: AvgPool2d(k, k);
 * add3: out = a + b (+ c, may be NULL).  The bilinear resizes are roma_op_resize_bilinear. */
int roma_op_gray_instnorm(const float* in, float* out, int B, int H, int W, int C, float eps, void* stream);
int roma_op_conv2d_nhwc(const float* in, const float* w, const float* bias, const float* res, float* out, int B, int H, int W,
                        int Cin, int Cout, int K, int stride, int pad, int relu, void* stream);
int roma_op_avgpool_nhwc(const float* in, float* out, int B, int H, int W, int C, int k, void* stream);
int roma_op_add3(const float* a, const float* b, const float* c, float* out, long n, void* stream);
/* d[B,H,W,Cp] = cat(f0 [B,H,W,C], grid_sample(f1 [B,H1,W1,C], warp[..., 0:2]), warp[..., 0:2], zero pad)  (tiny.py:290-291,
 * 298-299; bilinear, zeros padding, align_corners=False); warp has warp_channels >= 2 channels per pixel. */
int roma_op_tiny_matcher_input(const float* f0, const float* f1, const float* warp, int warp_channels, float* d, int B, int H,
                               int W, int H1, int W1, int C, int Cp, void* stream);
/* out[p, 0:3] = base[p, 0:base_channels] (third channel 0 when base has 2) + delta[p, 0:3] * (sx, sy, 1)  (tiny.py:289-300) */
int roma_op_tiny_update(const float* base, int base_channels, const float* delta, long ldd, float sx, float sy, float* out,
                        long npix, void* stream);
/* warp [B,H,W,4] = (grid, matches[..., 0:2]), certainty [B,H,W] = sigmoid(matches[..., 2])  (tiny.py:226-238) */
int roma_op_tiny_final(const float* matches, float* warp, float* certainty, int B, int H, int W, void* stream);
/* RegressionMatcher.visualize_warp (matcher.py:936-986): out[c,y,x] = certainty * grid_sample(image, warp) + (1 - certainty)
 * (bilinear, zeros padding, align_corners=False; white background).  warp [H, W2, 4] f32 with W2 = 2W (symmetric: left
 * half samples im_b at warp[..., 2:4], right half samples im_a at warp[..., 0:2], matcher.py:967-975) or W2 = W (im_a may
 * be NULL); certainty [H, W2]; images [3, im_h, im_w] f32; out [3, H, W2] f32. */
int roma_op_visualize_warp(const float* warp, const float* certainty, const float* im_a, const float* im_b, int H, int W,
                           int symmetric, int im_h, int im_w, float* out, void* stream);
/* conf_from_fb_consistency (matcher.py:672-699): out[b,y,x] = 1 if the backward flow sampled (bilinear, zeros padding,
 * align_corners=False) at the forward flow's target returns to within th_n of pixel (x,y)'s own normalised
 * coordinate, else 0.  flows DEVICE [B,H,W,2] f32, out [B,H,W] f32; th_n = 2*th / max(H,W). */
int roma_op_fb_consistency(const float* flow_fwd, const float* flow_bwd, int B, int H, int W, float th_n, float* out,
                           void* stream);
int roma_op_maxpool2x2(const void* in, void* out, int B, int H, int W, int C, int dt, void* stream);
/* MaxPool2d(2) + the proj head of a VGG pyramid level in one pass over the un-pooled map (encoders.py:17-27,
 * roma_models.py:156-160): in [B,H,W,C] 16-bit, C = 64 (N <= 32) or 128 (N <= 64) -> pooled [B,H/2,W/2,C] and
 * pf [B,H*W,ldf] = in . pw^T + pb (pw [N][ldw] 16-bit, pb f32 [N], columns N .. ldf zero; ldf any multiple of 8 from N up to
 * 32 / 64, and nothing is written outside a pixel's ldf columns).  Bit-identical to
 * roma_op_maxpool2x2 + roma_op_gemm; roma_tuning("pool_proj", 0) makes the model use those two instead. */
int roma_op_pool_proj(const void* in, void* pooled, void* pf, const void* pw, long ldw, const float* pb, int N, int ldf, int B, int H,
                      int W, int C, int dt, void* stream);
/* ConvRefiner out_conv fused with the flow / certainty update (matcher.py:177-178, 496-506):
 *   o = d[m, 0:Cp] . w[0:3, 0:Cp]^T + b;  flow[m] += (sx * o0, sy * o1);  cert[m] += o2        (f32 accumulate)
 * d DEVICE [M, ldd] in dt (f32 / bf16; channels Cp..ldd ignored), w DEVICE f32 [3][Cp], b f32 [3], flow f32 [M,2], cert f32 [M]. */
int roma_op_refiner_out(const void* d, long ldd, int dt, const float* w, const float* b, float* flow, float* cert, long M,
                        int Cp, float sx, float sy, void* stream);
int roma_op_conv3x3_c3(const float* img, const float* w, const float* bias, void* out, int B, int H, int W, int dt_out,
                       void* stream);
/* First VGG19-BN layer of the bf16 path (encoders.py:17-27, features[0..2] with the BatchNorm folded): img DEVICE f32
 * [B,3,H,W] -> out DEVICE bf16 [B,H,W,64] = ReLU(conv3x3(bf16(img), w, pad 1) + bias), products exact, f32 accumulate.
 * w DEVICE bf16 [64][32] with column k = ci*9 + ky*3 + kx (columns 27..31 zero), bias DEVICE f32 [64]. */
int roma_op_conv3x3_c3_bf16(const float* img, const void* w, const float* bias, void* out, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif
