// GP match encoder and the batched Cholesky solve behind it (gp.hip): called by the match() schedule (model.hip) and by
// roma_op_gp / roma_op_cholesky_solve_t (api.hip).
#pragma once
#include "arena.h"
#include "common.h"

namespace roma {

// GP match encoder for all directed pairs of a call; scratch comes from `arena` (dry = plan sizes only).  A live call whose
// scratch does not fit the arena launches nothing and returns -5 with Arena::overflow set.
int gp_posterior(const void* pf, long ldf, int act_dt, int B, bool symmetric, int th, int tw, const float* gp_w,
                 const float* gp_b, float* mu, long ld_mu, Arena& arena, hipStream_t st, bool dry);

// Batched SPD solve via blocked Cholesky (see include/roma_hip.h roma_op_cholesky_solve_t)
// strideA / strideR: batch strides of A and Rt in floats (0 = dense: n * n and d * n).  When Rt is stored right behind A
// (Rt == A + n * n, strideA == strideR: one (n + d) x n matrix per item) the forward substitution is folded into the
// factorisation loop - see cholesky_solve_t.
int cholesky_solve_t(float* A, float* Rt, float* LT, float* Linv, float* LinvT, int n, int d, int batch, hipStream_t st,
                     long strideA = 0, long strideR = 0);

}  // namespace roma
