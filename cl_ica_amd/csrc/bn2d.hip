// BatchNorm2d of ResNet-18 fused with the shortcut add and the ReLU behind it, fp32, contiguous NCHW x[N, C, HW]:
//   z = gamma[c] (x - mean[c]) invstd[c] + beta[c] (+ r),   y = z > 0 ? z : slope z      (slope = 0: ReLU, slope = 1: none)
// Statistics over the N * HW values of a channel.  The backward takes the gate from the saved output (y > 0 -> 1, else slope), as
// norm.hip does; z is never recomputed:  dz = dy gate(y),  dr = dz,  dx = gamma invstd (dz - sum dz / M - xhat sum(dz xhat) / M).
//
// Training forward: *_stats_k leaves Welford / Chan partials (count, mean, M2 of x - x[0, c, 0]: the channel's first value as pivot)
// per (image split, channel); *_apply_k -- the next launch on the stream -- merges the S partials of its channel in split order in
// EVERY workgroup (the same bits everywhere, no hand-off between workgroups), normalises its own split, and split 0 writes save_mean /
// save_invstd and the running statistics.  The backward is the same pair: *_sums_k, *_bwd_apply_k.  Inference: *_apply_k<.., false> on
// the running statistics, one launch.  Geometries "plane" and "small": bn2d.h.  A thread folds 4 or 16 values at a time into its
// statistic: their mean and M2 two-pass in registers, then one Chan merge (one division per block, not per value).
// No floating-point atomics, no arrival counters, nothing that waits inside a kernel: phases are ordered by the stream.
#include "bn2d.h"

namespace clica {
namespace bn2d {

using r2::Stat;
using r2::stat_add;
using r2::stat_merge;

// K values (already minus the pivot) into a: their own mean and M2, then Chan's merge
template <int K>
__device__ __forceinline__ void stat_block(Stat& a, const float* d) {
  if (K == 1) {
    stat_add(a, d[0], 0.f);
    return;
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) s += d[k];
  const float m = s * (1.f / K);
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float e = d[k] - m;
    q = fmaf(e, e, q);
  }
  stat_merge(a, Stat{(float)K, m, q, 0.f});
}

__device__ __forceinline__ Stat shfl_down_stat(const Stat& s, int off) {
  return Stat{__shfl_down(s.cnt, off, 64), __shfl_down(s.mean, off, 64), __shfl_down(s.m2, off, 64), 0.f};
}

// the lanes of a wave, then the waves of the workgroup in wave order: thread 0 ends with the workgroup's statistic
__device__ __forceinline__ void block_merge(Stat& s, float* sh /*[kWaves * 3]*/) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) stat_merge(s, shfl_down_stat(s, off));      // lane l < off takes lane l + off
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) { sh[3 * w] = s.cnt; sh[3 * w + 1] = s.mean; sh[3 * w + 2] = s.m2; }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int i = 1; i < kWaves; ++i) stat_merge(s, Stat{sh[3 * i], sh[3 * i + 1], sh[3 * i + 2], 0.f});
}

// S partials of channel c in split order (every caller: the same bits)
__device__ __forceinline__ Stat merge_partials(const float* __restrict__ part, int S, int C, int c) {
  const size_t plane = (size_t)S * C;
  Stat t{0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < S; ++i) {
    const float* p = part + (size_t)i * C + c;
    stat_merge(t, Stat{p[0], p[plane], p[2 * plane], 0.f});
  }
  return t;
}
// ------------------------------------------------------------------------------------------------ plane geometry
// grid (C, S)
template <int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void plane_stats_k(const float* __restrict__ x, int64_t N, int C, int HW, int64_t per,
                                                         float* __restrict__ part) {
  __shared__ float sh[kWaves * 3];
  const int c = (int)blockIdx.x, split = (int)blockIdx.y, S = (int)gridDim.y;
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int U = HW / VEC;
  const int64_t T = (n1 - n0) * U;
  const float pivot = x[(int64_t)c * HW];      // moments of x - x[0, c, 0]: at the scale of the deviation, whatever the channel's offset
  Walk wk(n0, U, C, c, HW);
  Stat s{0.f, 0.f, 0.f, 0.f};
  int64_t i = threadIdx.x;
  for (; i + 3 * kThreads < T; i += 4 * kThreads) {       // four loads in flight, then one block of 4 VEC values
    float d[4 * VEC];
#pragma unroll
    for (int j = 0; j < 4; ++j) load<VEC, AL>(x + wk.next<VEC>(), d + j * VEC);
#pragma unroll
    for (int k = 0; k < 4 * VEC; ++k) d[k] -= pivot;
    stat_block<4 * VEC>(s, d);
  }
  for (; i < T; i += kThreads) {
    float d[VEC];
    load<VEC, AL>(x + wk.next<VEC>(), d);
#pragma unroll
    for (int k = 0; k < VEC; ++k) d[k] -= pivot;
    stat_block<VEC>(s, d);
  }
  block_merge(s, sh);
  if (threadIdx.x == 0) {
    const size_t plane = (size_t)S * C;
    float* q = part + (size_t)split * C + c;
    q[0] = s.cnt; q[plane] = s.mean; q[2 * plane] = s.m2;
  }
}

// grid (C, S).  TRAIN: batch statistics from the partials; otherwise the running statistics (inference).  No barrier.
template <int VEC, bool AL, bool TRAIN>
__global__ __launch_bounds__(kThreads) void plane_apply_k(const float* __restrict__ x, const float* __restrict__ r,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, int64_t N, int C,
                                                         int HW, int64_t per, float Mf, float eps, float momentum, float slope,
                                                         const float* __restrict__ part, float* __restrict__ y, float* __restrict__ save_mean,
                                                         float* __restrict__ save_invstd, float* running_mean, float* running_var) {
  const int c = (int)blockIdx.x, split = (int)blockIdx.y, S = (int)gridDim.y;
  float mean, invstd;
  if (TRAIN) {
    const Stat t = merge_partials(part, S, C, c);
    mean = x[(int64_t)c * HW] + t.mean;
    invstd = 1.f / sqrtf(t.m2 / Mf + eps);
    if (split == 0 && threadIdx.x == 0) {
      save_mean[c] = mean;
      save_invstd[c] = invstd;
      if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
      if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (t.m2 / (Mf - 1.f));      // unbiased
    }
  } else {
    mean = running_mean[c];
    invstd = 1.f / sqrtf(running_var[c] + eps);
  }
  const float g = gamma[c], b = beta[c];
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int U = HW / VEC;
  const int64_t T = (n1 - n0) * U;
  Walk wk(n0, U, C, c, HW);
#pragma unroll 2
  for (int64_t i = threadIdx.x; i < T; i += kThreads) {
    const int64_t e = wk.next<VEC>();
    float v[VEC], rr[VEC];
    load<VEC, AL>(x + e, v);
    if (r) load<VEC, AL>(r + e, rr);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float z = fmaf(g, (v[k] - mean) * invstd, b);
      if (r) z += rr[k];
      v[k] = lrelu(z, slope);
    }
    store<VEC, AL>(y + e, v);
  }
}

// grid (C, S): sum dz and sum dz xhat per (split, channel)
template <int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void plane_sums_k(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ dy, const float* __restrict__ save_mean,
                                                        const float* __restrict__ save_invstd, int64_t N, int C, int HW, int64_t per,
                                                        float slope, float* __restrict__ part) {
  __shared__ float sh[kWaves * 2];
  const int c = (int)blockIdx.x, split = (int)blockIdx.y, S = (int)gridDim.y;
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int U = HW / VEC;
  const int64_t T = (n1 - n0) * U;
  const float mean = save_mean[c], invstd = save_invstd[c];
  Walk wk(n0, U, C, c, HW);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll 2
  for (int64_t i = threadIdx.x; i < T; i += kThreads) {
    const int64_t e = wk.next<VEC>();
    float xv[VEC], yv[VEC], gv[VEC];
    load<VEC, AL>(x + e, xv); load<VEC, AL>(y + e, yv); load<VEC, AL>(dy + e, gv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float dz = gv[k] * gate(yv[k], slope);
      s1 += dz;
      s2 = fmaf(dz, (xv[k] - mean) * invstd, s2);
    }
  }
  block_sum2(s1, s2, sh);
  if (threadIdx.x == 0) {
    float* q = part + (size_t)split * C + c;
    q[0] = s1; q[(size_t)S * C] = s2;
  }
}

// grid (C, S).  No barrier.
template <int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void plane_bwd_apply_k(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dy, const float* __restrict__ gamma,
                                                             const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
                                                             int64_t N, int C, int HW, int64_t per, float Mf, float slope,
                                                             const float* __restrict__ part, float* __restrict__ dx, float* __restrict__ dr,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = (int)blockIdx.x, split = (int)blockIdx.y, S = (int)gridDim.y;
  float s1, s2;
  sum_partials(part, S, C, c, s1, s2);
  if (split == 0 && threadIdx.x == 0) {
    dgamma[c] = s2;
    dbeta[c] = s1;
  }
  const float mean = save_mean[c], invstd = save_invstd[c];
  const float kk = gamma[c] * invstd, m1 = s1 / Mf, m2 = s2 / Mf;
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int U = HW / VEC;
  const int64_t T = (n1 - n0) * U;
  Walk wk(n0, U, C, c, HW);
#pragma unroll 2
  for (int64_t i = threadIdx.x; i < T; i += kThreads) {
    const int64_t e = wk.next<VEC>();
    float xv[VEC], yv[VEC], gv[VEC];
    load<VEC, AL>(x + e, xv); load<VEC, AL>(y + e, yv); load<VEC, AL>(dy + e, gv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float dz = gv[k] * gate(yv[k], slope);
      gv[k] = dz;
      xv[k] = kk * (dz - m1 - (xv[k] - mean) * invstd * m2);
    }
    store<VEC, AL>(dx + e, xv);
    if (dr) store<VEC, AL>(dr + e, gv);
  }
}

// ------------------------------------------------------------------------------------------------ small geometry (HW = 4 Q, Q = 1, 2, 4)
// grid (64-piece chunks, S).  Piece p = (channel p / Q, quad p % Q); 64 % Q == 0, so a channel's pieces are neighbouring lanes of one wave.
template <bool AL>
__global__ __launch_bounds__(kThreads) void small_stats_k(const float* __restrict__ x, int64_t N, int C, int Q, int64_t per,
                                                         float* __restrict__ part) {
  __shared__ float sh[(kWaves - 1) * 3 * 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = (int)blockIdx.x * 64 + lane, P = C * Q;
  const int split = (int)blockIdx.y, S = (int)gridDim.y;
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int64_t row = (int64_t)P * 4;           // values of one image
  const int c = p / Q;
  Stat s{0.f, 0.f, 0.f, 0.f};
  if (p < P) {
    const float pivot = x[(int64_t)c * Q * 4];
    const float* xp = x + (int64_t)p * 4;
    int64_t n = n0 + w;
    for (; n + 3 * kWaves < n1; n += 4 * kWaves) {        // four images' loads in flight, then one block of 16 values
      float d[16];
#pragma unroll
      for (int j = 0; j < 4; ++j) load<4, AL>(xp + (n + j * kWaves) * row, d + 4 * j);
#pragma unroll
      for (int k = 0; k < 16; ++k) d[k] -= pivot;
      stat_block<16>(s, d);
    }
    for (; n < n1; n += kWaves) {
      float d[4];
      load<4, AL>(xp + n * row, d);
#pragma unroll
      for (int k = 0; k < 4; ++k) d[k] -= pivot;
      stat_block<4>(s, d);
    }
  }
  if (w > 0) {
    float* q = sh + (w - 1) * 3 * 64 + lane;
    q[0] = s.cnt; q[64] = s.mean; q[128] = s.m2;
  }
  __syncthreads();
  if (w == 0) {
    for (int i = 0; i < kWaves - 1; ++i) {                // the workgroup's waves in wave order
      const float* q = sh + i * 3 * 64 + lane;
      stat_merge(s, Stat{q[0], q[64], q[128], 0.f});
    }
    const Stat own = s;
    for (int j = 1; j < Q; ++j) {                         // the channel's quads in quad order, into its first lane
      const Stat o{__shfl(own.cnt, lane + j, 64), __shfl(own.mean, lane + j, 64), __shfl(own.m2, lane + j, 64), 0.f};
      if (p % Q == 0) stat_merge(s, o);
    }
    if (p < P && p % Q == 0) {
      const size_t plane = (size_t)S * C;
      float* q = part + (size_t)split * C + c;
      q[0] = s.cnt; q[plane] = s.mean; q[2 * plane] = s.m2;
    }
  }
}

// grid (64-piece chunks, S).  No barrier: a lane beyond C Q leaves at once.
template <bool AL, bool TRAIN>
__global__ __launch_bounds__(kThreads) void small_apply_k(const float* __restrict__ x, const float* __restrict__ r,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, int64_t N, int C,
                                                         int Q, int64_t per, float Mf, float eps, float momentum, float slope,
                                                         const float* __restrict__ part, float* __restrict__ y, float* __restrict__ save_mean,
                                                         float* __restrict__ save_invstd, float* running_mean, float* running_var) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = (int)blockIdx.x * 64 + lane, P = C * Q;
  if (p >= P) return;
  const int split = (int)blockIdx.y, S = (int)gridDim.y;
  const int c = p / Q;
  float mean, invstd;
  if (TRAIN) {
    const Stat t = merge_partials(part, S, C, c);
    mean = x[(int64_t)c * Q * 4] + t.mean;
    invstd = 1.f / sqrtf(t.m2 / Mf + eps);
    if (split == 0 && w == 0 && p % Q == 0) {
      save_mean[c] = mean;
      save_invstd[c] = invstd;
      if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
      if (running_var) running_var[c] = (1.f - momentum) * running_var[c] + momentum * (t.m2 / (Mf - 1.f));      // unbiased
    }
  } else {
    mean = running_mean[c];
    invstd = 1.f / sqrtf(running_var[c] + eps);
  }
  const float g = gamma[c], b = beta[c];
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int64_t row = (int64_t)P * 4;
#pragma unroll 2
  for (int64_t n = n0 + w; n < n1; n += kWaves) {
    const int64_t e = n * row + (int64_t)p * 4;
    float v[4], rr[4];
    load<4, AL>(x + e, v);
    if (r) load<4, AL>(r + e, rr);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float z = fmaf(g, (v[k] - mean) * invstd, b);
      if (r) z += rr[k];
      v[k] = lrelu(z, slope);
    }
    store<4, AL>(y + e, v);
  }
}

template <bool AL>
__global__ __launch_bounds__(kThreads) void small_sums_k(const float* __restrict__ x, const float* __restrict__ y,
                                                        const float* __restrict__ dy, const float* __restrict__ save_mean,
                                                        const float* __restrict__ save_invstd, int64_t N, int C, int Q, int64_t per,
                                                        float slope, float* __restrict__ part) {
  __shared__ float sh[(kWaves - 1) * 2 * 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = (int)blockIdx.x * 64 + lane, P = C * Q;
  const int split = (int)blockIdx.y, S = (int)gridDim.y;
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int64_t row = (int64_t)P * 4;
  const int c = p / Q;
  float s1 = 0.f, s2 = 0.f;
  if (p < P) {
    const float mean = save_mean[c], invstd = save_invstd[c];
#pragma unroll 2
    for (int64_t n = n0 + w; n < n1; n += kWaves) {
      const int64_t e = n * row + (int64_t)p * 4;
      float xv[4], yv[4], gv[4];
      load<4, AL>(x + e, xv); load<4, AL>(y + e, yv); load<4, AL>(dy + e, gv);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float dz = gv[k] * gate(yv[k], slope);
        s1 += dz;
        s2 = fmaf(dz, (xv[k] - mean) * invstd, s2);
      }
    }
  }
  if (w > 0) {
    float* q = sh + (w - 1) * 2 * 64 + lane;
    q[0] = s1; q[64] = s2;
  }
  __syncthreads();
  if (w == 0) {
    for (int i = 0; i < kWaves - 1; ++i) {
      const float* q = sh + i * 2 * 64 + lane;
      s1 += q[0]; s2 += q[64];
    }
    const float o1 = s1, o2 = s2;
    for (int j = 1; j < Q; ++j) {
      const float a = __shfl(o1, lane + j, 64), b = __shfl(o2, lane + j, 64);
      if (p % Q == 0) { s1 += a; s2 += b; }
    }
    if (p < P && p % Q == 0) {
      float* q = part + (size_t)split * C + c;
      q[0] = s1; q[(size_t)S * C] = s2;
    }
  }
}

template <bool AL>
__global__ __launch_bounds__(kThreads) void small_bwd_apply_k(const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ dy, const float* __restrict__ gamma,
                                                             const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
                                                             int64_t N, int C, int Q, int64_t per, float Mf, float slope,
                                                             const float* __restrict__ part, float* __restrict__ dx, float* __restrict__ dr,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int p = (int)blockIdx.x * 64 + lane, P = C * Q;
  if (p >= P) return;
  const int split = (int)blockIdx.y, S = (int)gridDim.y;
  const int c = p / Q;
  float s1, s2;
  sum_partials(part, S, C, c, s1, s2);
  if (split == 0 && w == 0 && p % Q == 0) {
    dgamma[c] = s2;
    dbeta[c] = s1;
  }
  const float mean = save_mean[c], invstd = save_invstd[c];
  const float kk = gamma[c] * invstd, m1 = s1 / Mf, m2 = s2 / Mf;
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int64_t row = (int64_t)P * 4;
#pragma unroll 2
  for (int64_t n = n0 + w; n < n1; n += kWaves) {
    const int64_t e = n * row + (int64_t)p * 4;
    float xv[4], yv[4], gv[4];
    load<4, AL>(x + e, xv); load<4, AL>(y + e, yv); load<4, AL>(dy + e, gv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float dz = gv[k] * gate(yv[k], slope);
      gv[k] = dz;
      xv[k] = kk * (dz - m1 - (xv[k] - mean) * invstd * m2);
    }
    store<4, AL>(dx + e, xv);
    if (dr) store<4, AL>(dr + e, gv);
  }
}

// ------------------------------------------------------------------------------------------------ launches
template <bool TRAIN>
static void launch_apply(dim3 grid, hipStream_t st, bool small, bool quad, bool al, const float* x, const float* r, const float* gamma,
                         const float* beta, int64_t N, int C, int HW, int64_t per, float Mf, float eps, float momentum, float slope,
                         const float* part, float* y, float* save_mean, float* save_invstd, float* rm, float* rv) {
  const dim3 block(kThreads);
#define CLICA_BN2D_APPLY(K, D) \
  hipLaunchKernelGGL(K, grid, block, 0, st, x, r, gamma, beta, N, C, D, per, Mf, eps, momentum, slope, part, y, save_mean, save_invstd, rm, rv)
  if (small) {
    if (al) CLICA_BN2D_APPLY((small_apply_k<true, TRAIN>), HW / 4);
    else CLICA_BN2D_APPLY((small_apply_k<false, TRAIN>), HW / 4);
  } else if (quad) {
    if (al) CLICA_BN2D_APPLY((plane_apply_k<4, true, TRAIN>), HW);
    else CLICA_BN2D_APPLY((plane_apply_k<4, false, TRAIN>), HW);
  } else {
    CLICA_BN2D_APPLY((plane_apply_k<1, false, TRAIN>), HW);
  }
#undef CLICA_BN2D_APPLY
}

// launch 1 of the training forward (also of pool2d.hip's): 16-byte loads when X allows them -- the same bits either way
void launch_stats(hipStream_t st, const float* X, int64_t N, int32_t C, int32_t HW, float* part) {
  const Geometry geo = geometry(N, HW);
  const bool al = HW % 4 == 0 && aligned16(X);
  const dim3 grid(grid_x(C, HW), (unsigned)geo.S), block(kThreads);
  if (small_hw(HW)) {
    if (al) hipLaunchKernelGGL(small_stats_k<true>, grid, block, 0, st, X, N, (int)C, (int)(HW / 4), geo.per, part);
    else hipLaunchKernelGGL(small_stats_k<false>, grid, block, 0, st, X, N, (int)C, (int)(HW / 4), geo.per, part);
  } else if (HW % 4 == 0) {
    if (al) hipLaunchKernelGGL((plane_stats_k<4, true>), grid, block, 0, st, X, N, (int)C, (int)HW, geo.per, part);
    else hipLaunchKernelGGL((plane_stats_k<4, false>), grid, block, 0, st, X, N, (int)C, (int)HW, geo.per, part);
  } else {
    hipLaunchKernelGGL((plane_stats_k<1, false>), grid, block, 0, st, X, N, (int)C, (int)HW, geo.per, part);
  }
}

}  // namespace bn2d
}  // namespace clica

using namespace clica;

#define CLICA_BN2D_SHAPE(fn, min_M)                                                                                                  \
  CLICA_CHECK_ARG(N >= 1 && N <= INT32_MAX && C >= 1 && C <= bn2d::kMaxC && HW >= 1 && N * (int64_t)HW >= (min_M) &&                  \
                      (double)N * (double)HW * (double)C < 1e18,                                                                      \
                  fn ": N=%lld C=%d HW=%d (N >= 1, 1 <= C <= %d, HW >= 1, N HW >= %d)", (long long)N, C, HW, bn2d::kMaxC, (min_M))

#define CLICA_BN2D_SLOPE(fn) \
  CLICA_CHECK_ARG(slope >= 0.f, fn ": slope=%g must be >= 0 (the backward recovers the gate from the output)", slope)

extern "C" int clica_bn2d_workspace_bytes(int64_t N, int32_t C, int32_t HW, size_t* bytes) {
  CLICA_CHECK_ARG(bytes != nullptr, "clica_bn2d_workspace_bytes: bytes is NULL");
  CLICA_BN2D_SHAPE("clica_bn2d_workspace_bytes", 2);
  *bytes = bn2d::workspace_bytes(N, C, HW);
  return CLICA_OK;
}

extern "C" int clica_bn2d_act_fwd_train(const float* X, const float* R, const float* gamma, const float* beta, int64_t N, int32_t C,
                                        int32_t HW, float eps, float momentum, float slope, float* Y, float* save_mean,
                                        float* save_invstd, float* running_mean, float* running_var, void* workspace,
                                        size_t workspace_bytes, clica_stream_t stream) {
  CLICA_BN2D_SHAPE("clica_bn2d_act_fwd_train", 2);
  CLICA_BN2D_SLOPE("clica_bn2d_act_fwd_train");
  CLICA_CHECK_ARG(X && gamma && beta && Y && save_mean && save_invstd && workspace, "clica_bn2d_act_fwd_train: NULL pointer");
  CLICA_CHECK_ARG(bn2d::aligned16(workspace), "clica_bn2d_act_fwd_train: workspace must be 16-byte aligned");
  const size_t need = bn2d::workspace_bytes(N, C, HW);
  CLICA_CHECK_ARG(workspace_bytes >= need, "clica_bn2d_act_fwd_train: workspace of %zu bytes, %zu needed (clica_bn2d_workspace_bytes)",
                  workspace_bytes, need);
  const bn2d::Geometry geo = bn2d::geometry(N, HW);
  const bool small = bn2d::small_hw(HW), quad = HW % 4 == 0;
  const bool al = quad && bn2d::aligned16(X) && bn2d::aligned16(Y) && (!R || bn2d::aligned16(R));
  const dim3 grid(bn2d::grid_x(C, HW), (unsigned)geo.S);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  bn2d::launch_stats(st, X, N, C, HW, part);
  bn2d::launch_apply<true>(grid, st, small, quad, al, X, R, gamma, beta, N, (int)C, (int)HW, geo.per, (float)(N * (int64_t)HW), eps,
                           momentum, slope, part, Y, save_mean, save_invstd, running_mean, running_var);
  return launch_status("clica_bn2d_act_fwd_train");
}

extern "C" int clica_bn2d_act_fwd_eval(const float* X, const float* R, const float* gamma, const float* beta, const float* running_mean,
                                       const float* running_var, int64_t N, int32_t C, int32_t HW, float eps, float slope, float* Y,
                                       clica_stream_t stream) {
  CLICA_BN2D_SHAPE("clica_bn2d_act_fwd_eval", 1);
  CLICA_BN2D_SLOPE("clica_bn2d_act_fwd_eval");
  CLICA_CHECK_ARG(X && gamma && beta && running_mean && running_var && Y, "clica_bn2d_act_fwd_eval: NULL pointer");
  const bn2d::Geometry geo = bn2d::geometry(N, HW);
  const bool small = bn2d::small_hw(HW), quad = HW % 4 == 0;
  const bool al = quad && bn2d::aligned16(X) && bn2d::aligned16(Y) && (!R || bn2d::aligned16(R));
  const dim3 grid(bn2d::grid_x(C, HW), (unsigned)geo.S);
  // (the inference instance only reads the running statistics)
  bn2d::launch_apply<false>(grid, as_stream(stream), small, quad, al, X, R, gamma, beta, N, (int)C, (int)HW, geo.per, 0.f, eps, 0.f, slope,
                            nullptr, Y, nullptr, nullptr, const_cast<float*>(running_mean), const_cast<float*>(running_var));
  return launch_status("clica_bn2d_act_fwd_eval");
}

extern "C" int clica_bn2d_act_bwd(const float* X, const float* Y, const float* dY, const float* gamma, const float* save_mean,
                                  const float* save_invstd, int64_t N, int32_t C, int32_t HW, float slope, float* dX, float* dR,
                                  float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  CLICA_BN2D_SHAPE("clica_bn2d_act_bwd", 2);
  CLICA_BN2D_SLOPE("clica_bn2d_act_bwd");
  CLICA_CHECK_ARG(X && Y && dY && gamma && save_mean && save_invstd && dX && dgamma && dbeta && workspace, "clica_bn2d_act_bwd: NULL pointer");
  CLICA_CHECK_ARG(bn2d::aligned16(workspace), "clica_bn2d_act_bwd: workspace must be 16-byte aligned");
  const size_t need = bn2d::workspace_bytes(N, C, HW);
  CLICA_CHECK_ARG(workspace_bytes >= need, "clica_bn2d_act_bwd: workspace of %zu bytes, %zu needed (clica_bn2d_workspace_bytes)",
                  workspace_bytes, need);
  const bn2d::Geometry geo = bn2d::geometry(N, HW);
  const bool small = bn2d::small_hw(HW), quad = HW % 4 == 0;
  const bool al = quad && bn2d::aligned16(X) && bn2d::aligned16(Y) && bn2d::aligned16(dY) && bn2d::aligned16(dX) && (!dR || bn2d::aligned16(dR));
  const dim3 grid(bn2d::grid_x(C, HW), (unsigned)geo.S), block(bn2d::kThreads);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const float Mf = (float)(N * (int64_t)HW);
#define CLICA_BN2D_BWD(SUMS, APPLY, D)                                                                                              \
  do {                                                                                                                              \
    hipLaunchKernelGGL(SUMS, grid, block, 0, st, X, Y, dY, save_mean, save_invstd, N, (int)C, (int)(D), geo.per, slope, part);      \
    hipLaunchKernelGGL(APPLY, grid, block, 0, st, X, Y, dY, gamma, save_mean, save_invstd, N, (int)C, (int)(D), geo.per, Mf, slope, \
                       part, dX, dR, dgamma, dbeta);                                                                                \
  } while (0)
  if (small) {
    if (al) CLICA_BN2D_BWD(bn2d::small_sums_k<true>, bn2d::small_bwd_apply_k<true>, HW / 4);
    else CLICA_BN2D_BWD(bn2d::small_sums_k<false>, bn2d::small_bwd_apply_k<false>, HW / 4);
  } else if (quad) {
    if (al) CLICA_BN2D_BWD((bn2d::plane_sums_k<4, true>), (bn2d::plane_bwd_apply_k<4, true>), HW);
    else CLICA_BN2D_BWD((bn2d::plane_sums_k<4, false>), (bn2d::plane_bwd_apply_k<4, false>), HW);
  } else {
    CLICA_BN2D_BWD((bn2d::plane_sums_k<1, false>), (bn2d::plane_bwd_apply_k<1, false>), HW);
  }
#undef CLICA_BN2D_BWD
  return launch_status("clica_bn2d_act_bwd");
}
