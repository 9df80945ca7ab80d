// What the batch-normalisation kernels of norm.hip (BatchNorm1d), bn2d.hip (BatchNorm2d + shortcut add + ReLU) and pool2d.hip (the stem
// unit with its max-pool) share -- the single source of each piece, so that two kernels that promise the same bits run the same code:
//   the channel finish    merged statistic (or running statistics) -> mean, invstd; the designated writer stores save_mean / save_invstd
//                         and the momentum update of the running statistics (unbiased variance)
//   the element functions xhat, y = lrelu(gamma xhat + beta (+ r), slope); dz = dy gate(y), the sums (sum dz, sum dz xhat) and
//                         dx = gamma invstd (dz - sum dz / M - xhat sum(dz xhat) / M)
//   the merges            of the S split partials of the workspace in split order, and of the waves of a workgroup whose lanes are columns
//   the workspace check   of the entry points
// The library is built with -ffp-contract=fast: the compiler decides per inlined copy and per loop version (main / remainder) whether
// a product that feeds a sum becomes a fused multiply-add.  Only a spelled fmaf is fused everywhere; where the expression is left to the
// compiler below, it is the expression all its users had, and tools/norm_digest.py is the check that their bits did not move.
#pragma once
#include "common.h"
#include "r2_loss.h"      // r2::Stat / stat_add / stat_merge: Welford's update and Chan's merge

namespace clica {
namespace bn {

constexpr int kThreads = 256;                 // every kernel of the family: 4 waves
constexpr int kWaves = kThreads / 64;

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

#ifdef __HIPCC__
using r2::Stat;
using r2::stat_merge;

__device__ __forceinline__ float lrelu(float z, float slope) { return z > 0.f ? z : slope * z; }
__device__ __forceinline__ float gate(float y, float slope) { return y > 0.f ? 1.f : slope; }

// ------------------------------------------------------------------------------------------------ channel finish
struct Norm { float mean, invstd; };

// training: t = the merged statistic of x - pivot over the M = Mf values of channel c
__device__ __forceinline__ Norm finish_train(const Stat& t, float pivot, float Mf, float eps, float momentum, int c, bool writer,
                                             float* __restrict__ save_mean, float* __restrict__ save_invstd, float* running_mean,
                                             float* running_var) {
  const float mean = pivot + t.mean;
  const float invstd = 1.f / sqrtf(t.m2 / Mf + eps);
  if (writer) {
    save_mean[c] = mean;
    save_invstd[c] = invstd;
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
    if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (t.m2 / (Mf - 1.f));      // unbiased
  }
  return Norm{mean, invstd};
}

// inference: the running statistics
__device__ __forceinline__ Norm finish_eval(const float* running_mean, const float* running_var, int c, float eps) {
  return Norm{running_mean[c], 1.f / sqrtf(running_var[c] + eps)};
}

// ------------------------------------------------------------------------------------------------ element functions
__device__ __forceinline__ float xhat(float x, const Norm& n) { return (x - n.mean) * n.invstd; }
__device__ __forceinline__ float affine(float xh, float g, float b) { return fmaf(g, xh, b); }       // z without a residual
__device__ __forceinline__ float fwd_xhat(float xh, float g, float b, float slope) { return lrelu(affine(xh, g, b), slope); }
__device__ __forceinline__ float fwd(float x, const Norm& n, float g, float b, float slope) { return fwd_xhat(xhat(x, n), g, b, slope); }
// (with a residual: lrelu(affine(xhat(x, n), g, b) + r, slope))

__device__ __forceinline__ float bwd_dz(float dy, float y, float slope) { return dy * gate(y, slope); }
__device__ __forceinline__ void bwd_sums(float& s1, float& s2, float dz, float xh) {
  s1 += dz;
  s2 = fmaf(dz, xh, s2);
}
struct Bwd { float k, m1, m2; };              // gamma invstd, sum dz / M, sum(dz xhat) / M
__device__ __forceinline__ Bwd bwd_coeffs(float gamma, float invstd, float s1, float s2, float Mf) { return Bwd{gamma * invstd, s1 / Mf, s2 / Mf}; }
__device__ __forceinline__ float bwd_dx(float dz, float xh, const Bwd& w) { return w.k * (dz - w.m1 - xh * w.m2); }

// ------------------------------------------------------------------------------------------------ the S partials of channel c, split order
// Partials [planes][S][C].  The loads of eight partials are in flight before their merges; the index is clamped, so no address past
// the buffer is formed.  Every caller of a channel: the same bits.  An empty Welford partial merges as nothing; a sum pair past S is
// added as +0 rather than skipped: the guarded form makes the compiler pair (s1, s2) differently, and the remainder iterations of the
// backward sweeps behind it then lose the contraction of dz - m1 that their main loops have.
__device__ __forceinline__ Stat merge_stats(const float* __restrict__ part, int S, int C, int c) {
  const size_t plane = (size_t)S * C;
  Stat t{0.f, 0.f, 0.f, 0.f};
  for (int i0 = 0; i0 < S; i0 += 8) {
    float a[8], m[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float* p = part + (size_t)(i0 + j < S ? i0 + j : S - 1) * C + c;
      a[j] = p[0]; m[j] = p[plane]; q[j] = p[2 * plane];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i0 + j < S) stat_merge(t, Stat{a[j], m[j], q[j], 0.f});
  }
  return t;
}

__device__ __forceinline__ void merge_sums(const float* __restrict__ part, int S, int C, int c, float& s1, float& s2) {
  const size_t plane = (size_t)S * C;
  s1 = 0.f; s2 = 0.f;
  for (int i0 = 0; i0 < S; i0 += 8) {
    float a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = i0 + j < S;
      const float* p = part + (size_t)(in ? i0 + j : S - 1) * C + c;
      a[j] = in ? p[0] : 0.f; b[j] = in ? p[plane] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1 += a[j]; s2 += b[j]; }      // (a sum that starts at +0 never becomes -0: adding +0 changes no bit)
  }
}

// The splits [s0, s1) of the S alone, in split order: what one of several threads that share a channel's merge takes (bn2d_nhwc.hip).
// Siblings rather than the general case of the two above, whose code -- and with it the contraction choices behind them -- stays as it is.
__device__ __forceinline__ Stat merge_stats_range(const float* __restrict__ part, int S, int C, int c, int s0, int s1) {
  const size_t plane = (size_t)S * C;
  Stat t{0.f, 0.f, 0.f, 0.f};
  for (int i0 = s0; i0 < s1; i0 += 8) {
    float a[8], m[8], q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float* p = part + (size_t)(i0 + j < s1 ? i0 + j : s1 - 1) * C + c;
      a[j] = p[0]; m[j] = p[plane]; q[j] = p[2 * plane];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i0 + j < s1) stat_merge(t, Stat{a[j], m[j], q[j], 0.f});
  }
  return t;
}

__device__ __forceinline__ void merge_sums_range(const float* __restrict__ part, int S, int C, int c, int s0, int s1, float& s1_, float& s2_) {
  const size_t plane = (size_t)S * C;
  s1_ = 0.f; s2_ = 0.f;
  for (int i0 = s0; i0 < s1; i0 += 8) {
    float a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool in = i0 + j < s1;
      const float* p = part + (size_t)(in ? i0 + j : s1 - 1) * C + c;
      a[j] = in ? p[0] : 0.f; b[j] = in ? p[plane] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) { s1_ += a[j]; s2_ += b[j]; }
  }
}

// ------------------------------------------------------------------------------------------------ lane = column: the waves of a workgroup
// Every wave holds a value per lane (column); the lanes of wave 0 whose column is `active` end with the workgroup's, merged in wave
// order.  All threads call (a barrier).
constexpr int kColumnStatLds = (kWaves - 1) * 3 * 64;
constexpr int kColumnSumsLds = (kWaves - 1) * 2 * 64;

__device__ __forceinline__ void column_merge(Stat& s, float* sh /*[kColumnStatLds]*/, bool active = true) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (w > 0) {
    float* p = sh + (w - 1) * 3 * 64 + lane;
    p[0] = s.cnt; p[64] = s.mean; p[128] = s.m2;
  }
  __syncthreads();
  if (w == 0 && active) {
    for (int i = 0; i < kWaves - 1; ++i) {
      const float* p = sh + i * 3 * 64 + lane;
      stat_merge(s, Stat{p[0], p[64], p[128], 0.f});
    }
  }
}

__device__ __forceinline__ void column_sums(float& s1, float& s2, float* sh /*[kColumnSumsLds]*/, bool active = true) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (w > 0) {
    float* p = sh + (w - 1) * 2 * 64 + lane;
    p[0] = s1; p[64] = s2;
  }
  __syncthreads();
  if (w == 0 && active) {
    for (int i = 0; i < kWaves - 1; ++i) {
      const float* p = sh + i * 2 * 64 + lane;
      s1 += p[0]; s2 += p[64];
    }
  }
}
#endif  // __HIPCC__

}  // namespace bn
}  // namespace clica

// The partial workspace of an entry point `fn` (its arguments workspace / workspace_bytes): 16-byte aligned, or CLICA_E_INVALID; of at
// least `need` bytes -- what `size_fn` reports --, or `short_code`.
#define CLICA_BN_WORKSPACE(fn, need, size_fn, short_code)                                                              \
  do {                                                                                                                 \
    CLICA_CHECK_ARG(::clica::bn::aligned16(workspace), fn ": workspace must be 16-byte aligned");                      \
    const size_t need_ = (need);                                                                                       \
    if (workspace_bytes < need_) {                                                                                     \
      ::clica::set_error(fn ": workspace of %zu bytes, %zu needed (" size_fn ")", workspace_bytes, need_);             \
      return short_code;                                                                                               \
    }                                                                                                                  \
  } while (0)
