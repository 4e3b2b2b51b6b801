// RegressionMatcher.sample (romatch/models/matcher.py:598-629) for a whole batch of pairs in one enqueue: see
// sample_batched.hip and roma_op_sample_matches in include/roma_hip.h.
#pragma once
#include "common.h"

namespace roma {
// the second draw of pair b runs on seeds[b] ^ SAMPLE_SECOND_DRAW_SEED (the multiplier of Knuth's MMIX generator)
constexpr unsigned long long SAMPLE_SECOND_DRAW_SEED = 0x5851f42d4c957f2dull;
// largest first-draw size: the all-pairs order of sampling.hip (ORDER_ALLPAIRS_MAX); its bitonic path is not batched
constexpr long SAMPLE_BATCHED_MAX_K = 65536;

size_t sample_matches_workspace_bytes(int B, long n, long num, int balanced);
int sample_matches_launch(const float* matches, const float* certainty, const unsigned long long* seeds, int B, long n, long num,
                          int threshold, float thresh, int balanced, float* out_matches, float* out_certainty, int* out_counts,
                          long long* out_idx, long long* out_first_idx, float* out_density, void* ws, size_t ws_bytes, hipStream_t s);
}  // namespace roma
