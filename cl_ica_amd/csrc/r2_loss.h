// (Negative) R2 score per latent column (reference losses.py:480-503): launch geometry, workspace layout and the moment
// partials that the forward kernel (r2_loss.hip) leaves per wave and its last wave merges.
#pragma once
#include "common.h"

namespace clica {
namespace r2 {

// workspace: [0, 256) the arrival counter (int, zero between launches), then four planes [kind][wave slot][column] of floats:
// kind 0 the rows the wave saw, 1 their mean of t = y - y[0] (the first row as pivot), 2 their M2 = sum (t - mean)^2, 3 their sum (y_pred - y)^2
constexpr size_t kHeaderBytes = 256;
constexpr int kThreads = 256;                 // forward and backward: workgroup size
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 32;                // forward grid cap: at most 128 partials per column for the last wave to merge
constexpr int kGroupsPerWave = 8;             // row groups a wave is sized for before the grid cap
constexpr int kMaxN = 256;
constexpr int kBwdMaxBlocks = 1024;
constexpr int kBwdElemsPerThread = 4;

// A wave covers R = 64 / P rows at once, P = the column count rounded up to a power of two (64 from n = 33 on; beyond 64 columns the
// wave walks its rows once per 64-column chunk): lane = r * P + c, so the lanes of a row read consecutive addresses.
static inline int log2_cols(int32_t n) {
  int l = 0;
  while ((1 << l) < n && l < 6) ++l;
  return l;
}
static inline int64_t fwd_blocks(int64_t M, int32_t n) {
  const int64_t groups = ceil_div(M, (int64_t)(64 >> log2_cols(n)));
  const int64_t b = ceil_div(ceil_div(groups, (int64_t)kGroupsPerWave), (int64_t)kWaves);
  return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b);
}
static inline size_t workspace_bytes(int64_t M, int32_t n) {
  return kHeaderBytes + (size_t)4 * (size_t)(fwd_blocks(M, n) * kWaves) * (size_t)n * sizeof(float);
}
static inline int64_t bwd_blocks(int64_t M, int32_t n) {
  const int64_t b = ceil_div(M * (int64_t)n, (int64_t)kThreads * kBwdElemsPerThread);
  return b < 1 ? 1 : (b > kBwdMaxBlocks ? kBwdMaxBlocks : b);
}

// Moments of one column over a set of rows.  Two sets combine by Chan's formula (Chan, Golub, LeVeque 1979): the variance never
// appears as a difference of two sums that each carry the squared mean, so it stays at fp32 grade when |mean| >> std.
struct Stat { float cnt, mean, m2, sse; };

__device__ __forceinline__ void stat_add(Stat& a, float y, float d) {        // Welford's update by one row
  a.cnt += 1.f;
  const float delta = y - a.mean;
  a.mean += delta / a.cnt;
  a.m2 = fmaf(delta, y - a.mean, a.m2);
  a.sse = fmaf(d, d, a.sse);
}

__device__ __forceinline__ void stat_merge(Stat& a, const Stat& b) {         // an empty b (a wave or a lane without rows) changes nothing
  if (b.cnt > 0.f) {
    const float tot = a.cnt + b.cnt, delta = b.mean - a.mean, f = b.cnt / tot;
    a.mean = fmaf(delta, f, a.mean);
    a.m2 += b.m2 + delta * delta * (a.cnt * f);
    a.cnt = tot;
  }
  a.sse += b.sse;
}

}  // namespace r2
}  // namespace clica
