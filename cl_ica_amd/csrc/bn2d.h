// BatchNorm2d fused with the residual add and the (leaky) ReLU behind it on contiguous fp32 NCHW x[N, C, HW] (bn2d.hip): launch
// geometry and workspace layout.  The rules of norm.h hold: every reduction is a fixed tree -- per-lane accumulation over a fixed
// element sequence, the lanes of a wave by shuffles in lane order, the waves of a workgroup through LDS in wave order, the split
// partials of the workspace in split order by the LATER launch.  Phases are ordered by the stream only (no counters, no atomics).
//
// Two geometries, chosen from HW alone (never from the pointers, so an unaligned call reduces in the same order as an aligned one):
//   plane  one workgroup = (channel, image split).  Its 256 threads sweep the split's planes of that channel, 4 consecutive pixels
//          ("quad", one 16-byte load when the pointers are aligned) or, when HW % 4 != 0, single pixels per thread and step; a wave
//          reads 1 KB rows of a plane (HW >= 256) or whole planes of consecutive images (HW = 64: four 256-byte planes).
//   small  HW = 4, 8, 16: one image's C * HW values are contiguous and a channel's plane is only 16 .. 64 bytes, so a LANE owns a
//          (channel, quad) "piece" and walks over the images; a wave reads 1 KB of consecutive channels of one image, the four waves
//          of a workgroup take images n0 + w, n0 + w + 4, ...  One workgroup = (64 pieces, image split).
#pragma once
#include "common.h"
#include "r2_loss.h"      // r2::Stat / stat_add / stat_merge: Welford's update and Chan's merge

namespace clica {
namespace bn2d {

constexpr int kThreads = 256;                 // every kernel: 4 waves
constexpr int kWaves = kThreads / 64;
constexpr int kMaxC = 1 << 20;
constexpr int kMaxSplits = 32;                // S: partials per channel that every apply workgroup merges again
constexpr int64_t kPlaneSplitElems = 16384;   // plane: values of one channel a split is sized for before the cap on S (64 per thread)
constexpr int64_t kSmallSplitImages = 16;     // small: images a split is sized for before the cap on S (4 per wave)

static inline bool small_hw(int32_t HW) { return HW == 4 || HW == 8 || HW == 16; }

struct Geometry {
  int S;                // image splits = partials per channel
  int64_t per;          // images per split (the last one may hold fewer)
};

static inline Geometry geometry(int64_t N, int32_t HW) {
  int64_t s = small_hw(HW) ? ceil_div(N, kSmallSplitImages) : ceil_div(N * (int64_t)HW, kPlaneSplitElems);
  if (s > kMaxSplits) s = kMaxSplits;
  if (s > N) s = N;
  if (s < 1) s = 1;
  Geometry g;
  g.per = ceil_div(N, s);
  g.S = (int)ceil_div(N, g.per);             // no empty split
  return g;
}

// workgroups along x: channels (plane) or 64-piece chunks (small)
static inline unsigned grid_x(int32_t C, int32_t HW) { return small_hw(HW) ? (unsigned)ceil_div((int64_t)C * (HW / 4), 64) : (unsigned)C; }

// forward: three planes [S][C] (count, mean, M2 of x - x[0, c, 0]); backward: two (sum dz, sum dz xhat) in the same buffer
static inline size_t workspace_bytes(int64_t N, int32_t C, int32_t HW) {
  return align_up((size_t)3 * (size_t)geometry(N, HW).S * (size_t)C * sizeof(float), 16);
}

}  // namespace bn2d
}  // namespace clica
