// The linear triangulation and cheirality rule of recoverPose (essential.hip) and of the pose refinement's mask
// (pose_refine.hip).  ransac.h first: its fp-contract setting holds here as well.
#pragma once
#include "ransac.h"

namespace roma {
namespace {

// linear triangulation with P0 = [I | 0], P1 = [R | t] and the point on the ray of camera 0, X = (lam x0, w): (lam, w) is the
// smallest eigenvector of M^T M for the two equations of camera 1, M = [[u R3.x0 - R1.x0, u t3 - t1], [v R3.x0 - R2.x0, v t3 - t2]].
// OpenCV's cheirality rule: Q2 Q3 = lam w > 0, then depth lam / w and depth (R X)_3 / w in camera 1 both in (0, dist).
__device__ __forceinline__ bool cheiral(const double* c, double x, double y, double u, double v, double dist) {
  const double r1 = (c[0] * x + c[1] * y) + c[2], r2 = (c[3] * x + c[4] * y) + c[5], r3 = (c[6] * x + c[7] * y) + c[8];
  const double a1 = u * r3 - r1, b1 = u * c[11] - c[9];
  const double a2 = v * r3 - r2, b2 = v * c[11] - c[10];
  const double p = a1 * a1 + a2 * a2, q = a1 * b1 + a2 * b2, r = b1 * b1 + b2 * b2;
  const double hd = (p - r) * 0.5;
  const double mu = (p + r) * 0.5 - sqrt(hd * hd + q * q);
  const double lam = p >= r ? q : mu - r;
  const double w = p >= r ? mu - p : q;
  if (!(lam * w > 0)) return false;
  const double z0 = lam / w, z1 = (lam * r3 + w * c[11]) / w;
  return z0 < dist && z1 > 0 && z1 < dist;
}

}  // namespace
}  // namespace roma
