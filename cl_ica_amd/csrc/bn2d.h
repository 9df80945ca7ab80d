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
#include "bn_core.h"      // the batch-normalisation family's shared device code; kThreads, kWaves, aligned16

namespace clica {
namespace bn2d {

using bn::kThreads;                           // every kernel: 4 waves
using bn::kWaves;
using bn::aligned16;
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

// ------------------------------------------------------------------------------------------------ stem unit with the max-pool (pool2d.hip)
// P = maxpool 3x3 / stride 2 / pad 1 of lrelu(gamma xhat + beta), floor mode.  The plane decomposition above: one workgroup =
// (channel, image split); it sweeps its split's planes in batches of as many whole planes as fit kPoolLdsFloats: a batch's planes
// [H][W] sit in LDS back to back, in the backward followed by the batch's gated window gradients [Ho][Wo] and a nibble per window (the
// position of its first maximum).  Hence the limit on a plane: pool_lds_floats(H, W) = H W + Ho Wo + ceil(Ho Wo / 8) <= kPoolLdsFloats
// (112 x 112 with its 56 x 56 windows fits exactly: 64288 of the 65536 bytes of static LDS).
// Planes with pool_lds_floats <= kPoolLdsSmall (the 32 x 32 stem planes of 64 x 64 images among them) run instances with 16 KB of LDS, so
// that eight workgroups share a CU.  Which instance runs depends on H and W alone: the reduction order of a shape is fixed.
constexpr int kPoolLdsFloats = 112 * 112 + 56 * 56 + 56 * 56 / 8;
constexpr int kPoolLdsSmall = 4096;

static inline int pool_out(int32_t n) { return (n - 1) / 2 + 1; }
static inline int64_t pool_lds_floats(int32_t H, int32_t W) {
  const int64_t hw = (int64_t)H * W, howo = (int64_t)pool_out(H) * pool_out(W);
  return hw + howo + (howo + 7) / 8;
}
static inline bool pool_fits(int32_t H, int32_t W) { return H >= 1 && W >= 1 && pool_lds_floats(H, W) <= kPoolLdsFloats; }
static inline bool pool_small(int32_t H, int32_t W) { return pool_lds_floats(H, W) <= kPoolLdsSmall; }

// the statistics launch of clica_bn2d_act_fwd_train (bn2d.hip): partials [3][S][C] of geometry(N, HW) into `part`
void launch_stats(hipStream_t st, const float* X, int64_t N, int32_t C, int32_t HW, float* part);

#ifdef __HIPCC__
// VEC consecutive values; AL: one 16-byte access (the pointer is aligned), else scalar accesses of the same values
template <int VEC, bool AL>
__device__ __forceinline__ void load(const float* __restrict__ p, float* v) {
  if (VEC == 4 && AL) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = p[k];
  }
}
template <int VEC, bool AL>
__device__ __forceinline__ void store(float* __restrict__ p, const float* v) {
  if (VEC == 4 && AL) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) p[k] = v[k];
  }
}

// the lanes of a wave, then the waves of the workgroup in wave order: thread 0 ends with the workgroup's sums
__device__ __forceinline__ void block_sum2(float& a, float& b, float* sh /*[kWaves * 2]*/) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sh[2 * w] = a; sh[2 * w + 1] = b; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < kWaves; ++i) { a += sh[2 * i]; b += sh[2 * i + 1]; }
}

// The units (VEC values each, U = HW / VEC per plane) of channel c over the images n0 .. of a split form one sequence (image-major);
// thread t takes units t, t + 256, ...  next() gives the element offset of the thread's current unit and steps on, without a division.
struct Walk {
  int64_t n, stride_n;      // image; C * HW
  int q, dn, dq, U;
  int64_t base;             // c * HW
  __device__ Walk(int64_t n0, int U_, int C, int c, int HW) : U(U_) {
    n = n0 + (int)threadIdx.x / U_;
    q = (int)threadIdx.x % U_;
    dn = kThreads / U_;
    dq = kThreads % U_;
    stride_n = (int64_t)C * HW;
    base = (int64_t)c * HW;
  }
  template <int VEC>
  __device__ __forceinline__ int64_t next() {
    const int64_t off = n * stride_n + base + (int64_t)q * VEC;
    q += dq;
    n += dn;
    if (q >= U) { q -= U; ++n; }
    return off;
  }
};
#endif  // __HIPCC__

}  // namespace bn2d
}  // namespace clica
