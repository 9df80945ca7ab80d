// (Negative) R2 score per latent column, the supervised 3DIdent objective (losses.R2Loss, reference losses.py:480-503, built by
// main_3dident.py:575 with reduction = "mean", mode = "negative_r2"):
//   var_j = mean_i (y_ij - mean_i y_ij)^2,  mse_j = mean_i (y_pred_ij - y_ij)^2,  r2_j = 1 - mse_j / var_j,  out = s reduce(r2)
//   dY_pred_ij = g_j s w (-2 / M) (y_pred_ij - y_ij) / var_j
// Forward: ONE launch.  Every wave walks its rows with the columns across its lanes (coalesced on a skinny matrix), keeps Welford
// moments per lane (of the target minus its first row: the pivot note below), combines the lanes of a column by a shuffle tree and
// leaves one partial per column; the last wave to arrive (the pattern of mse.h::wave_arrive) merges the partials in slot order -- the same bits whoever arrives last, eager or replayed -- writes
// r2_cols, inv_var and the reduced, signed result, and leaves the arrival counter at zero.  Backward: one element-wise launch.
// A column without variance (constant, or M = 1) gets what IEEE division gives, as in the reference; no other column sees it.
#include "r2_loss.h"

namespace clica {
namespace r2 {

__global__ __launch_bounds__(kThreads) void r2_fwd_k(const float* __restrict__ yp, int64_t ldp, const float* __restrict__ y, int64_t ldy,
                                                    int64_t M, int n, int log2p, float inv_M, int reduction, float sign, float weight,
                                                    float* __restrict__ out, float* __restrict__ r2_cols, float* __restrict__ inv_var,
                                                    float* part, int* arrive) {
  const int lane = threadIdx.x & 63;
  const int W = (int)gridDim.x * kWaves, w = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
  const int P = 1 << log2p, R = 64 >> log2p;
  const int r = lane >> log2p, c = lane & (P - 1);
  const int64_t groups = (M + R - 1) >> (6 - log2p);
  const size_t plane = (size_t)W * n;
  for (int c0 = 0; c0 < n; c0 += 64) {       // (one pass up to 64 columns)
    const int col = c0 + c;
    Stat s{0.f, 0.f, 0.f, 0.f};
    if (col < n) {
      // moments of y - y[0][col]: the column's first row as pivot, subtracted before anything is summed.  A mean kept in fp32 next to an
      // offset of 30 is only good to 2e-6 absolute -- 4e-5 of a standard deviation of 0.05 -- and Chan's delta^2 term would carry that
      // (7e-6 on the variance in the offset goldens); the shifted values are at the scale of the deviation itself.
      const float pivot = y[col];
      for (int64_t g = w; g < groups; g += W) {
        const int64_t row = g * R + r;
        if (row < M) {
          const float t = y[row * ldy + col];
          stat_add(s, t - pivot, yp[row * ldp + col] - t);
        }
      }
    }
    // the R lanes of a column: a tree over the row index, the same for every launch of this shape
    for (int off = 32; off >= P; off >>= 1) {
      Stat o;
      o.cnt = __shfl_down(s.cnt, off, 64); o.mean = __shfl_down(s.mean, off, 64);
      o.m2 = __shfl_down(s.m2, off, 64); o.sse = __shfl_down(s.sse, off, 64);
      stat_merge(s, o);
    }
    if (r == 0 && col < n) {
      float* p = part + (size_t)w * n + col;
      __hip_atomic_store(p, s.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p + plane, s.mean, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p + 2 * plane, s.m2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(p + 3 * plane, s.sse, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // agent-scope stores, acknowledged for the whole wave before its lane 0 arrives (mse.h: no release fence)
  __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0)
  asm volatile("" ::: "memory");
  int last = 0;
  if (lane == 0) {
    const int prev = __hip_atomic_fetch_add(arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == W - 1;
    if (last) __hip_atomic_store(arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // every arrival of this launch is in
  }
  last = __shfl(last, 0, 64);
  if (!last) return;
  float acc = 0.f;
  for (int c0 = 0; c0 < n; c0 += 64) {
    const int col = c0 + lane;
    float v = 0.f;
    if (col < n) {
      Stat t{0.f, 0.f, 0.f, 0.f};
      for (int i = 0; i < W; ++i) {
        const float* p = part + (size_t)i * n + col;
        Stat o;
        o.cnt = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        o.mean = __hip_atomic_load(p + plane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        o.m2 = __hip_atomic_load(p + 2 * plane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        o.sse = __hip_atomic_load(p + 3 * plane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        stat_merge(t, o);
      }
      const float var = t.m2 * inv_M, mse = t.sse * inv_M;
      v = 1.f - mse / var;
      r2_cols[col] = v;
      inv_var[col] = 1.f / var;
      if (reduction == CLICA_R2_REDUCE_NONE) out[col] = sign * v;
    }
    acc += v;
  }
  if (reduction == CLICA_R2_REDUCE_NONE) return;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) out[0] = sign * (acc * weight);
}

__global__ __launch_bounds__(kThreads) void r2_bwd_k(const float* __restrict__ yp, int64_t ldp, const float* __restrict__ y, int64_t ldy,
                                                    int64_t M, int n, const float* __restrict__ inv_var, const float* __restrict__ g,
                                                    int g_per_column, float coef, float* __restrict__ dy, int64_t lddy) {
  const int64_t total = M * (int64_t)n;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int64_t row = e / n;
    const int k = (int)(e - row * n);
    const float d = yp[row * ldp + k] - y[row * ldy + k];
    dy[row * lddy + k] = (g[g_per_column ? k : 0] * coef) * (d * inv_var[k]);
  }
}

static bool known(int32_t reduction, int32_t mode) {
  return (reduction == CLICA_R2_REDUCE_NONE || reduction == CLICA_R2_REDUCE_MEAN || reduction == CLICA_R2_REDUCE_SUM) &&
         (mode == CLICA_R2_MODE_R2 || mode == CLICA_R2_MODE_NEGATIVE_R2);
}

}  // namespace r2
}  // namespace clica

using namespace clica;

extern "C" int clica_r2_loss_workspace_bytes(int64_t M, int32_t n, size_t* bytes) {
  CLICA_CHECK_ARG(bytes != nullptr, "clica_r2_loss_workspace_bytes: bytes is NULL");
  CLICA_CHECK_ARG(M >= 1 && n >= 1 && n <= r2::kMaxN, "clica_r2_loss_workspace_bytes: M=%lld n=%d (M >= 1, 1 <= n <= %d)", (long long)M, n,
                  r2::kMaxN);
  *bytes = r2::workspace_bytes(M, n);
  return CLICA_OK;
}

extern "C" int clica_r2_loss_fwd(const float* y_pred, int64_t ldp, const float* y, int64_t ldy, int64_t M, int32_t n, int32_t reduction,
                                 int32_t mode, float* out, float* r2_cols, float* inv_var, void* workspace, size_t workspace_bytes,
                                 clica_stream_t stream) {
  CLICA_CHECK_ARG(y_pred && y && out && r2_cols && inv_var && workspace, "clica_r2_loss_fwd: NULL pointer");
  CLICA_CHECK_ARG(M >= 1 && n >= 1 && n <= r2::kMaxN, "clica_r2_loss_fwd: M=%lld n=%d (M >= 1, 1 <= n <= %d)", (long long)M, n, r2::kMaxN);
  CLICA_CHECK_ARG(ldp >= n && ldy >= n, "clica_r2_loss_fwd: leading dimension below n=%d (ldp=%lld ldy=%lld)", n, (long long)ldp,
                  (long long)ldy);
  CLICA_CHECK_ARG(r2::known(reduction, mode), "clica_r2_loss_fwd: reduction=%d mode=%d (CLICA_R2_REDUCE_*, CLICA_R2_MODE_*)", reduction, mode);
  CLICA_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "clica_r2_loss_fwd: workspace must be 16-byte aligned");
  const size_t need = r2::workspace_bytes(M, n);
  CLICA_CHECK_ARG(workspace_bytes >= need, "clica_r2_loss_fwd: workspace of %zu bytes, %zu needed (clica_r2_loss_workspace_bytes)",
                  workspace_bytes, need);
  char* ws = static_cast<char*>(workspace);
  hipLaunchKernelGGL(r2::r2_fwd_k, dim3((unsigned)r2::fwd_blocks(M, n)), dim3(r2::kThreads), 0, as_stream(stream), y_pred, ldp, y, ldy, M,
                     (int)n, r2::log2_cols(n), (float)(1.0 / (double)M), (int)reduction, mode == CLICA_R2_MODE_R2 ? 1.f : -1.f,
                     reduction == CLICA_R2_REDUCE_MEAN ? (float)(1.0 / (double)n) : 1.f, out, r2_cols, inv_var,
                     reinterpret_cast<float*>(ws + r2::kHeaderBytes), reinterpret_cast<int*>(ws));
  return launch_status("clica_r2_loss_fwd");
}

extern "C" int clica_r2_loss_bwd(const float* y_pred, int64_t ldp, const float* y, int64_t ldy, int64_t M, int32_t n, int32_t reduction,
                                 int32_t mode, const float* inv_var, const float* g, float* dY, int64_t lddy, clica_stream_t stream) {
  CLICA_CHECK_ARG(y_pred && y && inv_var && g && dY, "clica_r2_loss_bwd: NULL pointer");
  CLICA_CHECK_ARG(M >= 1 && n >= 1 && n <= r2::kMaxN, "clica_r2_loss_bwd: M=%lld n=%d (M >= 1, 1 <= n <= %d)", (long long)M, n, r2::kMaxN);
  CLICA_CHECK_ARG(ldp >= n && ldy >= n && lddy >= n, "clica_r2_loss_bwd: leading dimension below n=%d (ldp=%lld ldy=%lld lddy=%lld)", n,
                  (long long)ldp, (long long)ldy, (long long)lddy);
  CLICA_CHECK_ARG(r2::known(reduction, mode), "clica_r2_loss_bwd: reduction=%d mode=%d (CLICA_R2_REDUCE_*, CLICA_R2_MODE_*)", reduction, mode);
  const double s = mode == CLICA_R2_MODE_R2 ? 1.0 : -1.0, w = reduction == CLICA_R2_REDUCE_MEAN ? 1.0 / (double)n : 1.0;
  hipLaunchKernelGGL(r2::r2_bwd_k, dim3((unsigned)r2::bwd_blocks(M, n)), dim3(r2::kThreads), 0, as_stream(stream), y_pred, ldp, y, ldy, M,
                     (int)n, inv_var, g, reduction == CLICA_R2_REDUCE_NONE ? 1 : 0, (float)(s * w * -2.0 / (double)M), dY, lddy);
  return launch_status("clica_r2_loss_bwd");
}
