// Mean-squared-error objective, forward and backward in one launch: loss = mean((y - t)^2) over all M x n elements and
// dY = 2 (y - t) / (M n) -- F.mse_loss(z1_rec, z1) of the supervised phase (/root/reference/main_mlp.py:274-276) and its gradient.
// The training engine folds the same objective into the backward chain's prologue where that chain runs (clica_mse_target); this
// launch serves every other configuration (an output head, native fp32, the per-layer wide path).
#include "mse.h"

namespace clica {
namespace mse {

__global__ __launch_bounds__(kThreads) void mse_fwd_bwd_k(const float* __restrict__ y, int64_t ldy, const float* __restrict__ t, int64_t ldt,
                                                         int64_t M, int n, float* __restrict__ dy, int64_t lddy, float scale, float inv_count,
                                                         float* loss_out, int* tick, float* part, int* arrive) {
  const int64_t total = M * (int64_t)n;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  float s = 0.f;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += stride) {
    const int64_t r = e / n;
    const int k = (int)(e - r * n);
    const float d = y[r * ldy + k] - t[r * ldt + k];
    s = fmaf(d, d, s);
    dy[r * lddy + k] = d * scale;
  }
  wave_arrive(s, part, (int)blockIdx.x * (kThreads / 64) + (int)(threadIdx.x >> 6), (int)gridDim.x * (kThreads / 64), arrive, loss_out,
              inv_count, tick);
}

}  // namespace mse
}  // namespace clica

using namespace clica;

extern "C" int clica_mse_loss_workspace_bytes(int64_t M, int32_t n, size_t* bytes) {
  CLICA_CHECK_ARG(bytes != nullptr, "clica_mse_loss_workspace_bytes: bytes is NULL");
  CLICA_CHECK_ARG(M >= 1 && n >= 1 && n <= 4096, "clica_mse_loss_workspace_bytes: M=%lld n=%d (M >= 1, 1 <= n <= 4096)", (long long)M, n);
  *bytes = mse::workspace_bytes(M, n);
  return CLICA_OK;
}

extern "C" int clica_mse_loss_fwd_bwd(const float* y, int64_t ldy, const float* target, int64_t ldt, int64_t M, int32_t n,
                                      float* dY, int64_t lddy, float* loss_out, int32_t* tick_counter, void* workspace,
                                      size_t workspace_bytes, clica_stream_t stream) {
  CLICA_CHECK_ARG(y && target && dY && loss_out && workspace, "clica_mse_loss_fwd_bwd: NULL pointer");
  CLICA_CHECK_ARG(M >= 1 && n >= 1 && n <= 4096, "clica_mse_loss_fwd_bwd: M=%lld n=%d (M >= 1, 1 <= n <= 4096)", (long long)M, n);
  CLICA_CHECK_ARG(ldy >= n && ldt >= n && lddy >= n, "clica_mse_loss_fwd_bwd: leading dimension below n=%d (ldy=%lld ldt=%lld lddy=%lld)", n,
                  (long long)ldy, (long long)ldt, (long long)lddy);
  CLICA_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "clica_mse_loss_fwd_bwd: workspace must be 16-byte aligned");
  const size_t need = mse::workspace_bytes(M, n);
  CLICA_CHECK_ARG(workspace_bytes >= need, "clica_mse_loss_fwd_bwd: workspace of %zu bytes, %zu needed (clica_mse_loss_workspace_bytes)",
                  workspace_bytes, need);
  const double count = (double)M * (double)n;
  char* ws = static_cast<char*>(workspace);
  hipLaunchKernelGGL(mse::mse_fwd_bwd_k, dim3((unsigned)mse::standalone_blocks(M, n)), dim3(mse::kThreads), 0, as_stream(stream), y, ldy,
                     target, ldt, M, (int)n, dY, lddy, (float)(2.0 / count), (float)(1.0 / count), loss_out, tick_counter,
                     reinterpret_cast<float*>(ws + mse::kHeaderBytes), reinterpret_cast<int*>(ws));
  return launch_status("clica_mse_loss_fwd_bwd");
}
