// The counter-based generator shared by the multinomial race keys (sampling.hip, sample_batched.hip) and RANSAC's samples (ransac.h).
#pragma once
#include <algorithm>

#include "common.h"

namespace roma {
// splitmix64 finaliser
__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
}  // namespace roma
