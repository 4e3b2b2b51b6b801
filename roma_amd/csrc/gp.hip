// GP match encoder of the stride-16 scale and its blocked Cholesky solve (see gp.h).  Host side only: the kernels live in
// chol_col.hip, chol_diag.h, elementwise.hip and the GEMM family.
#include "gp.h"

#include <atomic>

#include "dry_run.h"
#include "elementwise.h"
#include "gemm.h"
#include "tuning.h"

namespace roma {

// ---------------------------------------------------------------- blocked Cholesky solve (transposed RHS)
// Solves A X = F for SPD A (n x n, n % 64 == 0) with Rt = F^T [d x n] overwritten by X^T.
// Right-looking 64-wide blocked factorisation; diagonal blocks are factorised and explicitly inverted by one
// workgroup (chol_diag), everything else is the MFMA GEMM with alpha = -1 accumulate:
//   panel  L[i,k]  = A[i,k] Linv_kk^T ; trailing A[i,j] -= L[i,k] L[j,k]^T (lower tiles only)
//   fwd    Yt[:,k] = Rt[:,k] Linv_kk^T ; Rt[:,i>k] -= Yt[:,k] L[i,k]^T
//   bwd    Xt[:,k] = Rt[:,k] Linv_kk   ; Rt[:,j<k] -= Xt[:,k] L[k,j]      (via LT = L^T)
// Round 4 - the augmented form.  The forward substitution does to the d rows of Rt exactly what the factorisation does to the
// rows of A below the diagonal block: multiply the column block k by Linv_kk^T, then subtract its product with L[j,k]^T from the
// column blocks j > k.  When the caller stores Rt right behind A (one (n + d) x n matrix per item), the panel and the trailing
// GEMM of step k simply run over mrem + d rows and the 2 * nblk - 1 launches of the forward loop disappear from the GP's
// launch-latency-bound chain (~0.75 ms of 10 .. 25 us launches at n = 1600); same operations on every element in the same
// order, so the result is bit-identical to the separate loop.
int cholesky_solve_t(float* A, float* Rt, float* LT, float* Linv, float* LinvT, int n, int d, int batch, hipStream_t st,
                     long strideA, long strideR) {
  ROMA_REQUIRE(n % 64 == 0 && n > 0 && d % 4 == 0, "cholesky_solve: n must be a multiple of 64, d of 4");
  const int nblk = n / 64;
  const long sA = strideA > 0 ? strideA : (long)n * n, sR = strideR > 0 ? strideR : (long)d * n, sL = (long)nblk * 4096;
  const long sLT = (long)n * n;  // LT is always dense
  const bool aug_env = tuning(SW_GP_AUG) != 0;  // A/B: 0 = always the separate forward loop
  const bool aug = aug_env && Rt == A + (long)n * n && (batch == 1 || (sA == sR && sA >= (long)(n + d) * n));
  const int extra = aug ? d : 0;
  // Round 6: the augmented system left-looking, ONE launch per block column (chol_col.hip) instead of chol_diag + panel +
  // trailing update; L^T is written by the same launches.  roma_tuning("gp_col", 0) / ROMA_GP_COL=0: the right-looking chain.
  const bool col = aug && tuning(SW_GP_COL) != 0 && d >= 64 && d % 64 == 0;
  static std::atomic<unsigned> solve_epoch{0};  // tags the in-launch hand-off flags of this solve (chol_col.hip)
  const unsigned epoch = col ? ++solve_epoch : 0u;
  const int col_leader = col ? (int)tuning(SW_GP_COL_LEADER) : 0;  // once per solve: the columns hand work to each other
  for (int k = 0; k < nblk && col; ++k)
    if (int rc = chol_col_launch(A, n, sA, LT, sLT, n, d, Linv, LinvT, k, nblk, batch, epoch, col_leader, st)) return rc;
  if (col)
    if (int rc = chol_col_restore_launch(A, n, sA, LT, sLT, n, batch, st)) return rc;
  for (int k = 0; k < nblk && !col; ++k) {
    if (int rc = chol_diag_launch(A, n, sA, Linv, LinvT, k, nblk, batch, st)) return rc;
    const int mrem = n - (k + 1) * 64;
    if (mrem + extra <= 0) break;
    GemmArgs g;
    g.A = A + (long)(k + 1) * 64 * n + k * 64; g.lda = n; g.sA = sA;
    g.W = Linv + (long)k * 4096; g.ldw = 64; g.sW = sL;
    g.C = const_cast<float*>(static_cast<const float*>(g.A)); g.ldc = n; g.sC = sA;
    g.M = mrem + extra; g.N = 64; g.K = 64; g.batch = batch;
    if (int rc = gemm_launch(g, st)) return rc;
    if (mrem <= 0) break;
    GemmArgs t;
    t.A = g.A; t.lda = n; t.sA = sA;
    t.W = g.A; t.ldw = n; t.sW = sA;
    float* Ct = A + (long)(k + 1) * 64 * n + (k + 1) * 64;
    t.C = Ct; t.ldc = n; t.sC = sA;
    t.res = Ct; t.ldr = n; t.sR = sA;
    t.alpha = -1.f; t.lower_only = 1;
    t.M = mrem + extra; t.N = mrem; t.K = 64; t.batch = batch;
    if (int rc = gemm_launch(t, st)) return rc;
  }
  if (!col)
    if (int rc = transpose_launch(A, LT, n, n, batch, st, sA, sLT)) return rc;
  for (int k = 0; k < nblk && !aug; ++k) {  // forward (separate right-hand sides only)
    GemmArgs g;
    g.A = Rt + k * 64; g.lda = n; g.sA = sR;
    g.W = Linv + (long)k * 4096; g.ldw = 64; g.sW = sL;
    g.C = Rt + k * 64; g.ldc = n; g.sC = sR;
    g.M = d; g.N = 64; g.K = 64; g.batch = batch;
    if (int rc = gemm_launch(g, st)) return rc;
    const int mrem = n - (k + 1) * 64;
    if (mrem <= 0) break;
    GemmArgs u;
    u.A = Rt + k * 64; u.lda = n; u.sA = sR;
    u.W = A + (long)(k + 1) * 64 * n + k * 64; u.ldw = n; u.sW = sA;
    u.C = Rt + (k + 1) * 64; u.ldc = n; u.sC = sR;
    u.res = Rt + (k + 1) * 64; u.ldr = n; u.sR = sR;
    u.alpha = -1.f;
    u.M = d; u.N = mrem; u.K = 64; u.batch = batch;
    if (int rc = gemm_launch(u, st)) return rc;
  }
  const bool bwd_env = tuning(SW_GP_BWD2) != 0;  // A/B: 0 = two launches per backward step
  if (bwd_env && nblk > 1) {
    // Backward substitution with ONE launch per step.  X_k = R_k Linv_kk and R_j -= X_k L[k,j] (j < k) re-associate to
    // R_j -= R_k (Linv_kk L[k,j]): the products M_k = Linv_kk L[k, :k] do not depend on the right-hand sides, so they are formed
    // for all k at once (in place over L^T: LT[:, block k] <- LT[:, block k] LinvT_kk, one launch with the second batch
    // level over k), the chain is the nblk - 1 update GEMMs on the not-yet-scaled R_k, and all X_k = R_k Linv_kk follow in one
    // launch at the end.  2 + nblk - 1 launches instead of 2 nblk - 1 on the GP's launch-latency-bound chain.
    GemmArgs m;
    m.A = LT; m.lda = n; m.sA = sLT; m.sA2 = 64;
    m.W = Linv; m.ldw = 64; m.sW = sL; m.sW2 = 4096;
    m.C = LT; m.ldc = n; m.sC = sLT; m.sC2 = 64;
    m.M = n; m.N = 64; m.K = 64; m.batch = batch; m.batch2 = nblk;
    if (int rc = gemm_launch(m, st)) return rc;
    for (int k = nblk - 1; k >= 1; --k) {
      GemmArgs u;
      u.A = Rt + k * 64; u.lda = n; u.sA = sR;
      u.W = LT + k * 64; u.ldw = n; u.sW = sLT;
      u.C = Rt; u.ldc = n; u.sC = sR;
      u.res = Rt; u.ldr = n; u.sR = sR;
      u.alpha = -1.f;
      u.M = d; u.N = k * 64; u.K = 64; u.batch = batch;
      if (int rc = gemm_launch(u, st)) return rc;
    }
    GemmArgs x;
    x.A = Rt; x.lda = n; x.sA = sR; x.sA2 = 64;
    x.W = LinvT; x.ldw = 64; x.sW = sL; x.sW2 = 4096;
    x.C = Rt; x.ldc = n; x.sC = sR; x.sC2 = 64;
    x.M = d; x.N = 64; x.K = 64; x.batch = batch; x.batch2 = nblk;
    return gemm_launch(x, st);
  }
  for (int k = nblk - 1; k >= 0; --k) {  // backward
    GemmArgs g;
    g.A = Rt + k * 64; g.lda = n; g.sA = sR;
    g.W = LinvT + (long)k * 4096; g.ldw = 64; g.sW = sL;
    g.C = Rt + k * 64; g.ldc = n; g.sC = sR;
    g.M = d; g.N = 64; g.K = 64; g.batch = batch;
    if (int rc = gemm_launch(g, st)) return rc;
    if (k == 0) break;
    GemmArgs u;
    u.A = Rt + k * 64; u.lda = n; u.sA = sR;
    u.W = LT + k * 64; u.ldw = n; u.sW = sLT;
    u.C = Rt; u.ldc = n; u.sC = sR;
    u.res = Rt; u.ldr = n; u.sR = sR;
    u.alpha = -1.f;
    u.M = d; u.N = k * 64; u.K = 64; u.batch = batch;
    if (int rc = gemm_launch(u, st)) return rc;
  }
  return 0;
}

// ---------------------------------------------------------------- GP match encoder (matcher.py:291-323, 191-200, 274-289)
// pf: projected stride-16 features of the 2B images [2B, n, ldf] (n = th * tw tokens, 512 channels; images [0, B) = A,
// [B, 2B) = B).  Directed pair i (i < B, or i < 2B when symmetric) has query image i and support image (i + B) % 2B.
// mu[i, :, 0:512] = K_xy (K_yy + 0.1 I)^-1 cos(8 pi (W_pos grid + b_pos)), written with row stride ld_mu (f32).
// K_yy, its Cholesky factor and alpha depend only on the SUPPORT image, so they are computed once per image.
int gp_posterior(const void* pf, long ldf, int act_dt, int B, bool symmetric, int th, int tw, const float* gp_w,
                 const float* gp_b, float* mu, long ld_mu, Arena& arena, hipStream_t st, bool dry) {
  const size_t esz = act_dt == DT_F32 ? 4 : 2;
  const int nimg = 2 * B, ndp = symmetric ? 2 * B : B, shift = B;
  const int n = th * tw, npad = (int)round_up(n, 64), nblk = npad / 64;
  auto AL = [&](size_t elems, size_t es) { return arena.alloc(elems * es); };
  auto off = [&](const void* p, long elems) -> const void* { return static_cast<const char*>(p) + elems * (long)esz; };
  float* norms = (float*)AL((size_t)nimg * n, 4);
  // K_yy and the right-hand sides F^T of an image in ONE (npad + 512) x npad matrix: cholesky_solve_t then runs the forward
  // substitution inside the factorisation loop
  const long saug = (long)(npad + 512) * npad;
  float* Kyy = (float*)AL((size_t)nimg * saug, 4);
  float* Rt = Kyy + (long)npad * npad;  // image j: Kyy + j * saug, Rt + j * saug
  float* LT = (float*)AL((size_t)nimg * npad * npad, 4);
  float* Kxy = (float*)AL((size_t)ndp * n * npad, 4);
  float* Linv = (float*)AL((size_t)nimg * nblk * 4096, 4);
  float* LinvT = (float*)AL((size_t)nimg * nblk * 4096, 4);
  if (!dry && arena.overflow) return -5;  // nothing launched on an aliased buffer; the caller words the error
  RUN(rownorm_launch(pf, ldf, act_dt, norms, (long)nimg * n, 512, st));
  // support images actually needed: symmetric -> all, else images [B, 2B)
  const int j0 = symmetric ? 0 : B, nj = symmetric ? nimg : B;
  {
    GemmArgs g;  // K_yy + sigma^2 I  (cosine kernel, CosKernel matcher.py:191-200)
    g.A = off(pf, (long)j0 * n * ldf); g.lda = ldf; g.sA = (long)n * ldf;
    g.W = g.A; g.ldw = ldf; g.sW = g.sA;
    g.C = Kyy + (long)j0 * saug; g.ldc = npad; g.sC = saug;
    g.M = n; g.N = n; g.K = 512; g.batch = nj; g.in_dt = act_dt; g.out_dt = DT_F32; g.mode = EPI_COSK;
    g.nx = norms + (long)j0 * n; g.ny = g.nx; g.sNx = n; g.sNy = n; g.inv_t = 1.0f / 0.2f; g.diag_add = 0.1f;
    RUN(gemm_launch(g, st));
  }
  RUN(pad_identity_launch(Kyy + (long)j0 * saug, npad, saug, n, npad, nj, st));
  if (!dry && npad != n) ROMA_CHECK_HIP(hipMemsetAsync(Kxy, 0, (size_t)ndp * n * npad * 4, st));  // (pad columns only: the GEMM writes the rest)
  for (int half = 0; half < (symmetric ? 2 : 1); ++half) {
    GemmArgs g;  // K_xy for directed pairs [half*B, half*B + B): x = image i, y = image (i + B) % nimg
    const int i0 = half * B, s0 = (i0 + shift) % nimg;
    g.A = off(pf, (long)i0 * n * ldf); g.lda = ldf; g.sA = (long)n * ldf;
    g.W = off(pf, (long)s0 * n * ldf); g.ldw = ldf; g.sW = (long)n * ldf;
    g.C = Kxy + (long)i0 * n * npad; g.ldc = npad; g.sC = (long)n * npad;
    g.M = n; g.N = n; g.K = 512; g.batch = B; g.in_dt = act_dt; g.out_dt = DT_F32; g.mode = EPI_COSK;
    g.nx = norms + (long)i0 * n; g.ny = norms + (long)s0 * n; g.sNx = n; g.sNy = n; g.inv_t = 1.0f / 0.2f;
    RUN(gemm_launch(g, st));
  }
  RUN(gp_basis_launch(gp_w, gp_b, Rt + (long)j0 * saug, 512, th, tw, npad, st, nj, saug));  // F^T behind every image's K_yy
  RUN(cholesky_solve_t(Kyy + (long)j0 * saug, Rt + (long)j0 * saug, LT + (long)j0 * npad * npad,
                          Linv + (long)j0 * nblk * 4096, LinvT + (long)j0 * nblk * 4096, npad, 512, nj, st, saug, saug));
  for (int half = 0; half < (symmetric ? 2 : 1); ++half) {
    GemmArgs g;  // mu = K_xy alpha
    const int i0 = half * B, s0 = (i0 + shift) % nimg;
    g.A = Kxy + (long)i0 * n * npad; g.lda = npad; g.sA = (long)n * npad;
    g.W = Rt + (long)s0 * saug; g.ldw = npad; g.sW = saug;
    g.C = mu + (long)i0 * n * ld_mu; g.ldc = ld_mu; g.sC = (long)n * ld_mu;
    g.M = n; g.N = 512; g.K = npad; g.batch = B;
    RUN(gemm_launch(g, st));
  }
  return 0;
}
}  // namespace roma
