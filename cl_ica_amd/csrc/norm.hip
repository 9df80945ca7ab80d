// BatchNorm1d and GroupNorm(1, C) fused with the LeakyReLU behind them, the hidden-layer normalisations of
// get_mlp(layer_normalization = "bn" | "gn"):  y = lrelu(z, slope),  z = gamma xhat + beta  (slope = 1: no activation, slope = 0: ReLU).
// fp32, row-major contiguous [M, C].  The backward takes the gate from the saved output (y > 0 -> 1, else slope), as
// clica_leaky_relu_bwd does; z is never recomputed.
//
// BatchNorm, training (column statistics): bn_stats_k leaves Welford / Chan partials (count, mean, M2 of x - x[0, c]: the first row
// as pivot, as r2_loss.hip) per (row split, column); bn_apply_k -- the next launch on the stream -- merges the S partials of its 64
// columns in split order in EVERY workgroup (the same bits everywhere, no hand-off between workgroups), normalises its row tile, and
// row tile 0 writes save_mean / save_invstd and the running statistics.  The backward is the same pair: bn_bwd_sums_k (sum dz,
// sum dz xhat per split), bn_bwd_apply_k.  Inference: bn_apply_k<false> on the running statistics, one element-wise launch.
// The channel finish, the element functions and the merges are bn_core.h's, shared with bn2d.hip and pool2d.hip.
// GroupNorm(1, C) (row statistics): gn_fwd_k, one wave per row, true two-pass (mean, then sum (x - mean)^2), the row in registers up
// to 1024 columns; gn_bwd_k the same layout, each lane keeping d gamma / d beta partials of its own columns over the rows of its
// wave slot; gn_param_reduce_k sums the slots in slot order.
// No floating-point atomics, no arrival counters, nothing that waits inside a kernel: phases are ordered by the stream.
#include "norm.h"

namespace clica {
namespace norm {

using r2::Stat;
using r2::stat_add;
using bn::lrelu;
using bn::gate;

__device__ __forceinline__ float wave_sum(float v) {       // butterfly: every lane ends with the same bits
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------ BatchNorm1d
// grid (64-column chunks, S row splits).  Lane = column (256 contiguous bytes per row and wave), wave w takes rows r0 + w, r0 + w + 4, ...
__global__ __launch_bounds__(kThreads) void bn_stats_k(const float* __restrict__ x, int64_t M, int C, int64_t split_rows,
                                                      float* __restrict__ part) {
  __shared__ float sh[bn::kColumnStatLds];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = (int)blockIdx.x * 64 + lane;
  const int split = (int)blockIdx.y, S = (int)gridDim.y;
  const int64_t r0 = (int64_t)split * split_rows;
  const int64_t r1 = r0 + split_rows < M ? r0 + split_rows : M;
  Stat s{0.f, 0.f, 0.f, 0.f};
  if (col < C) {
    const float pivot = x[col];        // moments of x - x[0, c]: at the scale of the deviation, whatever the column's offset
    int64_t r = r0 + w;
    for (; r + 3 * kWaves < r1; r += 4 * kWaves) {       // four loads in flight, then the four updates in row order
      const float a = x[r * C + col], b = x[(r + kWaves) * C + col], c = x[(r + 2 * kWaves) * C + col], d = x[(r + 3 * kWaves) * C + col];
      stat_add(s, a - pivot, 0.f); stat_add(s, b - pivot, 0.f); stat_add(s, c - pivot, 0.f); stat_add(s, d - pivot, 0.f);
    }
    for (; r < r1; r += kWaves) stat_add(s, x[r * C + col] - pivot, 0.f);
  }
  bn::column_merge(s, sh, col < C);
  if (w == 0 && col < C) {
    const size_t plane = (size_t)S * C;
    float* q = part + (size_t)split * C + col;
    q[0] = s.cnt; q[plane] = s.mean; q[2 * plane] = s.m2;
  }
}

// grid (row tiles, 64-column chunks).  TRAIN: batch statistics from the partials, row tile 0 is the writer; otherwise the running
// statistics (inference).  No barrier: a lane beyond C leaves at once.
template <bool TRAIN>
__global__ __launch_bounds__(kThreads) void bn_apply_k(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, int64_t M, int C, int S, float Mf, float eps,
                                                      float momentum, float slope, const float* __restrict__ part, float* __restrict__ y,
                                                      float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                      float* running_mean, float* running_var) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = (int)blockIdx.y * 64 + lane;
  if (col >= C) return;
  const bn::Norm nm = TRAIN ? bn::finish_train(bn::merge_stats(part, S, C, col), x[col], Mf, eps, momentum, col, blockIdx.x == 0 && w == 0,
                                               save_mean, save_invstd, running_mean, running_var)
                            : bn::finish_eval(running_mean, running_var, col, eps);
  const float g = gamma[col], b = beta[col];
  const int64_t row0 = (int64_t)blockIdx.x * kBnTileRows;
  const int64_t row1 = row0 + kBnTileRows < M ? row0 + kBnTileRows : M;
#pragma unroll 4
  for (int64_t r = row0 + w; r < row1; r += kWaves) y[r * C + col] = bn::fwd(x[r * C + col], nm, g, b, slope);
}

// the geometry of bn_stats_k: sum dz and sum dz xhat per (split, column), dz = dy gate(y), xhat = (x - save_mean) save_invstd
__global__ __launch_bounds__(kThreads) void bn_bwd_sums_k(const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ dy, const float* __restrict__ save_mean,
                                                         const float* __restrict__ save_invstd, int64_t M, int C, int64_t split_rows,
                                                         float slope, float* __restrict__ part) {
  __shared__ float sh[bn::kColumnSumsLds];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = (int)blockIdx.x * 64 + lane;
  const int split = (int)blockIdx.y, S = (int)gridDim.y;
  const int64_t r0 = (int64_t)split * split_rows;
  const int64_t r1 = r0 + split_rows < M ? r0 + split_rows : M;
  float s1 = 0.f, s2 = 0.f;
  if (col < C) {
    const bn::Norm nm{save_mean[col], save_invstd[col]};
#pragma unroll 4
    for (int64_t r = r0 + w; r < r1; r += kWaves) {
      const int64_t e = r * C + col;
      bn::bwd_sums(s1, s2, bn::bwd_dz(dy[e], y[e], slope), bn::xhat(x[e], nm));
    }
  }
  bn::column_sums(s1, s2, sh, col < C);
  if (w == 0 && col < C) {
    float* q = part + (size_t)split * C + col;
    q[0] = s1; q[(size_t)S * C] = s2;
  }
}

__global__ __launch_bounds__(kThreads) void bn_bwd_apply_k(const float* __restrict__ x, const float* __restrict__ y,
                                                          const float* __restrict__ dy, const float* __restrict__ gamma,
                                                          const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
                                                          int64_t M, int C, int S, float Mf, float slope, const float* __restrict__ part,
                                                          float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int col = (int)blockIdx.y * 64 + lane;
  if (col >= C) return;
  float s1, s2;
  bn::merge_sums(part, S, C, col, s1, s2);
  if (blockIdx.x == 0 && w == 0) {
    dgamma[col] = s2;
    dbeta[col] = s1;
  }
  const bn::Norm nm{save_mean[col], save_invstd[col]};
  const bn::Bwd bw = bn::bwd_coeffs(gamma[col], nm.invstd, s1, s2, Mf);
  const int64_t row0 = (int64_t)blockIdx.x * kBnTileRows;
  const int64_t row1 = row0 + kBnTileRows < M ? row0 + kBnTileRows : M;
#pragma unroll 4
  for (int64_t r = row0 + w; r < row1; r += kWaves) {
    const int64_t e = r * C + col;
    const float dz = bn::bwd_dz(dy[e], y[e], slope);
    dx[e] = bn::bwd_dx(dz, bn::xhat(x[e], nm), bw);
  }
}

// ------------------------------------------------------------------------------------------------ GroupNorm(1, C)
// REG: the row (C <= kGnRegCols) stays in registers between the passes; otherwise it is read again.
template <bool REG>
__global__ __launch_bounds__(kThreads) void gn_fwd_k(const float* __restrict__ x, const float* __restrict__ gamma,
                                                    const float* __restrict__ beta, int64_t M, int C, float eps, float slope,
                                                    float* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  const int lane = threadIdx.x & 63;
  const int64_t W = (int64_t)gridDim.x * kWaves, slot = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const float Cf = (float)C;
  for (int64_t row = slot; row < M; row += W) {
    const float* xr = x + row * C;
    float* yr = y + row * C;
    float v[kGnRegs];
    float s = 0.f;
    if (REG) {
#pragma unroll
      for (int i = 0; i < kGnRegs; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < C ? xr[c] : 0.f;
        s += v[i];
      }
    } else {
      for (int c = lane; c < C; c += 64) s += xr[c];
    }
    const float mean = wave_sum(s) / Cf;
    float q = 0.f;
    if (REG) {
#pragma unroll
      for (int i = 0; i < kGnRegs; ++i) {
        const float d = lane + 64 * i < C ? v[i] - mean : 0.f;
        q = fmaf(d, d, q);
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        const float d = xr[c] - mean;
        q = fmaf(d, d, q);
      }
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / Cf + eps);
    if (REG) {
#pragma unroll
      for (int i = 0; i < kGnRegs; ++i) {
        const int c = lane + 64 * i;
        if (c < C) yr[c] = lrelu(fmaf(gamma[c], (v[i] - mean) * rstd, beta[c]), slope);
      }
    } else {
      for (int c = lane; c < C; c += 64) yr[c] = lrelu(fmaf(gamma[c], (xr[c] - mean) * rstd, beta[c]), slope);
    }
    if (lane == 0) {
      mean_out[row] = mean;
      rstd_out[row] = rstd;
    }
  }
}

// part: two planes [slots][C] (d gamma, d beta); a wave slot writes its own row of each, every column, rows or not
template <bool REG>
__global__ __launch_bounds__(kThreads) void gn_bwd_k(const float* __restrict__ x, const float* __restrict__ y,
                                                    const float* __restrict__ dy, const float* __restrict__ gamma,
                                                    const float* __restrict__ mean_in, const float* __restrict__ rstd_in, int64_t M, int C,
                                                    float slope, float* __restrict__ dx, float* part) {
  const int lane = threadIdx.x & 63;
  const int64_t W = (int64_t)gridDim.x * kWaves, slot = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const float Cf = (float)C;
  float* pg = part + (size_t)slot * C;
  float* pb = part + (size_t)(W + slot) * C;
  float ag[kGnRegs], ab[kGnRegs];
  if (REG) {
#pragma unroll
    for (int i = 0; i < kGnRegs; ++i) ag[i] = ab[i] = 0.f;
  } else {
    for (int c = lane; c < C; c += 64) pg[c] = pb[c] = 0.f;        // (a lane only ever touches its own columns of its own slot)
  }
  for (int64_t row = slot; row < M; row += W) {
    const int64_t base = row * C;
    const float mu = mean_in[row], rs = rstd_in[row];
    float G[kGnRegs], XH[kGnRegs];
    float s1 = 0.f, s2 = 0.f;
    if (REG) {
#pragma unroll
      for (int i = 0; i < kGnRegs; ++i) {
        const int c = lane + 64 * i;
        float g = 0.f, xh = 0.f;
        if (c < C) {
          const float dz = dy[base + c] * gate(y[base + c], slope);
          xh = (x[base + c] - mu) * rs;
          g = dz * gamma[c];
          ag[i] = fmaf(dz, xh, ag[i]);
          ab[i] += dz;
        }
        G[i] = g; XH[i] = xh;
        s1 += g;
        s2 = fmaf(g, xh, s2);
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        const float dz = dy[base + c] * gate(y[base + c], slope);
        const float xh = (x[base + c] - mu) * rs;
        const float g = dz * gamma[c];
        pg[c] = fmaf(dz, xh, pg[c]);
        pb[c] += dz;
        s1 += g;
        s2 = fmaf(g, xh, s2);
      }
    }
    const float m1 = wave_sum(s1) / Cf, m2 = wave_sum(s2) / Cf;
    if (REG) {
#pragma unroll
      for (int i = 0; i < kGnRegs; ++i) {
        const int c = lane + 64 * i;
        if (c < C) dx[base + c] = rs * (G[i] - m1 - XH[i] * m2);
      }
    } else {
      for (int c = lane; c < C; c += 64) {
        const float dz = dy[base + c] * gate(y[base + c], slope);
        const float xh = (x[base + c] - mu) * rs;
        dx[base + c] = rs * (dz * gamma[c] - m1 - xh * m2);
      }
    }
  }
  if (REG) {
#pragma unroll
    for (int i = 0; i < kGnRegs; ++i) {
      const int c = lane + 64 * i;
      if (c < C) { pg[c] = ag[i]; pb[c] = ab[i]; }
    }
  }
}

__global__ __launch_bounds__(kThreads) void gn_param_reduce_k(const float* __restrict__ part, int slots, int C, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta) {
  const int c = (int)blockIdx.x * kThreads + (int)threadIdx.x;
  if (c >= C) return;
  const size_t plane = (size_t)slots * C;
  float sg = 0.f, sb = 0.f;
#pragma unroll 8
  for (int i = 0; i < slots; ++i) {                      // slot order
    sg += part[(size_t)i * C + c];
    sb += part[plane + (size_t)i * C + c];
  }
  dgamma[c] = sg;
  dbeta[c] = sb;
}

}  // namespace norm
}  // namespace clica

using namespace clica;

#define CLICA_NORM_SHAPE(fn, min_M)                                                                                               \
  CLICA_CHECK_ARG(M >= (min_M) && C >= 1 && C <= norm::kMaxC, fn ": M=%lld C=%d (M >= %d, 1 <= C <= %d)", (long long)M, C, (min_M), \
                  norm::kMaxC);                                                                                                   \
  CLICA_CHECK_ARG(slope >= 0.f, fn ": slope=%g must be >= 0 (the backward recovers the gate from the output)", slope)

extern "C" int clica_norm_workspace_bytes(int32_t kind, int64_t M, int32_t C, float slope, size_t* bytes) {
  CLICA_CHECK_ARG(bytes != nullptr, "clica_norm_workspace_bytes: bytes is NULL");
  CLICA_CHECK_ARG(kind == CLICA_NORM_BATCH || kind == CLICA_NORM_GROUP, "clica_norm_workspace_bytes: kind=%d (CLICA_NORM_*)", kind);
  CLICA_NORM_SHAPE("clica_norm_workspace_bytes", kind == CLICA_NORM_BATCH ? 2 : 1);
  *bytes = kind == CLICA_NORM_BATCH ? norm::bn_workspace_bytes(M, C) : norm::gn_workspace_bytes(M, C);
  return CLICA_OK;
}

extern "C" int clica_bn_lrelu_fwd_train(const float* X, const float* gamma, const float* beta, int64_t M, int32_t C, float eps,
                                        float momentum, float slope, float* Y, float* save_mean, float* save_invstd, float* running_mean,
                                        float* running_var, void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  CLICA_NORM_SHAPE("clica_bn_lrelu_fwd_train", 2);
  CLICA_CHECK_ARG(X && gamma && beta && Y && save_mean && save_invstd && workspace, "clica_bn_lrelu_fwd_train: NULL pointer");
  CLICA_BN_WORKSPACE("clica_bn_lrelu_fwd_train", norm::bn_workspace_bytes(M, C), "clica_norm_workspace_bytes", CLICA_E_INVALID);
  const int S = norm::bn_splits(M), chunks = norm::bn_chunks(C);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(norm::bn_stats_k, dim3((unsigned)chunks, (unsigned)S), dim3(norm::kThreads), 0, as_stream(stream), X, M, (int)C,
                     norm::bn_split_rows(M), part);
  hipLaunchKernelGGL(norm::bn_apply_k<true>, dim3((unsigned)norm::bn_tiles(M), (unsigned)chunks), dim3(norm::kThreads), 0, as_stream(stream), X,
                     gamma, beta, M, (int)C, S, (float)M, eps, momentum, slope, part, Y, save_mean, save_invstd, running_mean, running_var);
  return launch_status("clica_bn_lrelu_fwd_train");
}

extern "C" int clica_bn_lrelu_fwd_eval(const float* X, const float* gamma, const float* beta, const float* running_mean,
                                       const float* running_var, int64_t M, int32_t C, float eps, float slope, float* Y,
                                       clica_stream_t stream) {
  CLICA_NORM_SHAPE("clica_bn_lrelu_fwd_eval", 1);
  CLICA_CHECK_ARG(X && gamma && beta && running_mean && running_var && Y, "clica_bn_lrelu_fwd_eval: NULL pointer");
  // (the inference instance only reads the running statistics)
  hipLaunchKernelGGL(norm::bn_apply_k<false>, dim3((unsigned)norm::bn_tiles(M), (unsigned)norm::bn_chunks(C)), dim3(norm::kThreads), 0,
                     as_stream(stream), X, gamma, beta, M, (int)C, 0, 0.f, eps, 0.f, slope, nullptr, Y, nullptr, nullptr,
                     const_cast<float*>(running_mean), const_cast<float*>(running_var));
  return launch_status("clica_bn_lrelu_fwd_eval");
}

extern "C" int clica_bn_lrelu_bwd(const float* X, const float* Y, const float* dY, const float* gamma, const float* save_mean,
                                  const float* save_invstd, int64_t M, int32_t C, float slope, float* dX, float* dgamma, float* dbeta,
                                  void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  CLICA_NORM_SHAPE("clica_bn_lrelu_bwd", 2);
  CLICA_CHECK_ARG(X && Y && dY && gamma && save_mean && save_invstd && dX && dgamma && dbeta && workspace, "clica_bn_lrelu_bwd: NULL pointer");
  CLICA_BN_WORKSPACE("clica_bn_lrelu_bwd", norm::bn_workspace_bytes(M, C), "clica_norm_workspace_bytes", CLICA_E_INVALID);
  const int S = norm::bn_splits(M), chunks = norm::bn_chunks(C);
  float* part = static_cast<float*>(workspace);
  hipLaunchKernelGGL(norm::bn_bwd_sums_k, dim3((unsigned)chunks, (unsigned)S), dim3(norm::kThreads), 0, as_stream(stream), X, Y, dY,
                     save_mean, save_invstd, M, (int)C, norm::bn_split_rows(M), slope, part);
  hipLaunchKernelGGL(norm::bn_bwd_apply_k, dim3((unsigned)norm::bn_tiles(M), (unsigned)chunks), dim3(norm::kThreads), 0, as_stream(stream),
                     X, Y, dY, gamma, save_mean, save_invstd, M, (int)C, S, (float)M, slope, part, dX, dgamma, dbeta);
  return launch_status("clica_bn_lrelu_bwd");
}

extern "C" int clica_gn_lrelu_fwd(const float* X, const float* gamma, const float* beta, int64_t M, int32_t C, float eps, float slope,
                                  float* Y, float* mean, float* rstd, clica_stream_t stream) {
  CLICA_NORM_SHAPE("clica_gn_lrelu_fwd", 1);
  CLICA_CHECK_ARG(X && gamma && beta && Y && mean && rstd, "clica_gn_lrelu_fwd: NULL pointer");
  const dim3 grid((unsigned)norm::gn_fwd_blocks(M)), block(norm::kThreads);
  if (C <= norm::kGnRegCols)
    hipLaunchKernelGGL(norm::gn_fwd_k<true>, grid, block, 0, as_stream(stream), X, gamma, beta, M, (int)C, eps, slope, Y, mean, rstd);
  else
    hipLaunchKernelGGL(norm::gn_fwd_k<false>, grid, block, 0, as_stream(stream), X, gamma, beta, M, (int)C, eps, slope, Y, mean, rstd);
  return launch_status("clica_gn_lrelu_fwd");
}

extern "C" int clica_gn_lrelu_bwd(const float* X, const float* Y, const float* dY, const float* gamma, const float* mean, const float* rstd,
                                  int64_t M, int32_t C, float slope, float* dX, float* dgamma, float* dbeta, void* workspace,
                                  size_t workspace_bytes, clica_stream_t stream) {
  CLICA_NORM_SHAPE("clica_gn_lrelu_bwd", 1);
  CLICA_CHECK_ARG(X && Y && dY && gamma && mean && rstd && dX && dgamma && dbeta && workspace, "clica_gn_lrelu_bwd: NULL pointer");
  CLICA_BN_WORKSPACE("clica_gn_lrelu_bwd", norm::gn_workspace_bytes(M, C), "clica_norm_workspace_bytes", CLICA_E_INVALID);
  const dim3 grid((unsigned)norm::gn_bwd_blocks(M)), block(norm::kThreads);
  float* part = static_cast<float*>(workspace);
  if (C <= norm::kGnRegCols)
    hipLaunchKernelGGL(norm::gn_bwd_k<true>, grid, block, 0, as_stream(stream), X, Y, dY, gamma, mean, rstd, M, (int)C, slope, dX, part);
  else
    hipLaunchKernelGGL(norm::gn_bwd_k<false>, grid, block, 0, as_stream(stream), X, Y, dY, gamma, mean, rstd, M, (int)C, slope, dX, part);
  hipLaunchKernelGGL(norm::gn_param_reduce_k, dim3((unsigned)ceil_div(C, norm::kThreads)), block, 0, as_stream(stream), part,
                     norm::gn_slots(M), (int)C, dgamma, dbeta);
  return launch_status("clica_gn_lrelu_bwd");
}
