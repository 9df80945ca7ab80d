// Mean-squared-error objective (F.mse_loss(z1_rec, z1), the supervised phase of /root/reference/main_mlp.py:274-276): the
// deterministic reduction that the stand-alone kernel (mse_loss.hip) and the backward chain's prologue (fused_mlp.hip, clica_mse_target)
// share, and the workspace layout both use.
#pragma once
#include "common.h"

namespace clica {
namespace mse {

// workspace: [0, 256) the arrival counter (int, zero between launches), then one float partial per arriving wave
constexpr size_t kHeaderBytes = 256;
constexpr int kThreads = 256;                 // stand-alone kernel: workgroup size ...
constexpr int kMaxBlocks = 512;               // ... and grid cap (the partials stay few)
constexpr int kElemsPerThread = 4;
constexpr int kFoldRows = 48;                 // backward chain: rows per workgroup (fmlp::ROWS) ...
constexpr int kFoldWaves = 16;                // ... and an upper bound of its waves per workgroup (fmlp::WAVES)

static inline int64_t standalone_blocks(int64_t M, int32_t n) {
  const int64_t b = ceil_div(M * (int64_t)n, (int64_t)kThreads * kElemsPerThread);
  return b < 1 ? 1 : (b > kMaxBlocks ? kMaxBlocks : b);
}
static inline size_t workspace_bytes(int64_t M, int32_t n) {
  const int64_t slots_a = standalone_blocks(M, n) * (kThreads / 64);
  const int64_t slots_b = ceil_div(M, (int64_t)kFoldRows) * kFoldWaves;
  return kHeaderBytes + (size_t)(slots_a > slots_b ? slots_a : slots_b) * sizeof(float);
}

// Called by EVERY wave of the launch (all 64 lanes active) with its lanes' sums of squares.  The wave's total goes to partial slot
// `slot` (an agent-scope store, acknowledged before the wave arrives -- the pattern of lp_finalize.h: no release fence); the LAST of
// the `nslots` waves to arrive adds the partials in slot order (lane l takes slots l, l + 64, ..., then the shuffle tree: the same
// bits whoever arrives last), writes mean = sum * inv_count, advances `tick` by one if given, and puts the counter back to zero.
__device__ __forceinline__ void wave_arrive(float s, float* part, int slot, int nslots, int* arrive, float* loss_out, float inv_count,
                                            int* tick) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  int last = 0;
  if (lane == 0) {
    __hip_atomic_store(&part[slot], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): the partial's store has been acknowledged
    const int prev = __hip_atomic_fetch_add(arrive, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == nslots - 1;
    if (last) __hip_atomic_store(arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // every arrival of this launch is in
  }
  last = __shfl(last, 0, 64);
  if (!last) return;
  float v = 0.f;
  for (int i = lane; i < nslots; i += 64) v += __hip_atomic_load(&part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if (lane == 0) {
    loss_out[0] = v * inv_count;
    if (tick) tick[0] += 1;
  }
}

}  // namespace mse
}  // namespace clica
