// BatchNorm1d / GroupNorm(1, C) fused with LeakyReLU on row-major contiguous fp32 [M, C] (norm.hip): launch geometry and workspace
// layout.  Every reduction is a fixed tree: per-lane accumulation over a fixed row range, the waves of a workgroup through LDS in wave
// order, the (split | slot) partials of a workspace in index order by a LATER launch.  Phases are ordered by the stream only -- no
// arrival counter, no atomics --, so eager launches and graph replays give the same bits.
#pragma once
#include "bn_core.h"      // the batch-normalisation family's shared device code; kThreads, kWaves

namespace clica {
namespace norm {

using bn::kThreads;                           // every kernel: 4 waves
using bn::kWaves;
constexpr int kMaxC = 1 << 20;

// ---- BatchNorm: columns across the lanes of a wave, 64 per workgroup; rows across waves, workgroups (row tiles) and row splits
constexpr int kBnMaxSplits = 64;              // S: partials per column that every apply workgroup merges again
constexpr int kBnRowsPerSplit = 64;           // rows a split is sized for before the cap on S (16 per wave)
constexpr int kBnTileRows = 64;               // rows of one apply workgroup

static inline int bn_chunks(int32_t C) { return (int)ceil_div(C, 64); }
static inline int bn_splits(int64_t M) {
  const int64_t s = ceil_div(M, (int64_t)kBnRowsPerSplit);
  return (int)(s < 1 ? 1 : (s > kBnMaxSplits ? kBnMaxSplits : s));
}
static inline int64_t bn_split_rows(int64_t M) { return ceil_div(M, (int64_t)bn_splits(M)); }
static inline int64_t bn_tiles(int64_t M) { return ceil_div(M, (int64_t)kBnTileRows); }
// forward: three planes [S][C] (count, mean, M2 of x - x[0, c]); backward: two (sum dz, sum dz xhat) in the same buffer
static inline size_t bn_workspace_bytes(int64_t M, int32_t C) { return (size_t)3 * (size_t)bn_splits(M) * (size_t)C * sizeof(float); }

// ---- GroupNorm(1, C): one wave per row at a time, lane l owns columns l, l + 64, ...; a row of up to kGnRegCols stays in registers
constexpr int kGnRegCols = 1024;
constexpr int kGnRegs = kGnRegCols / 64;
constexpr int kGnFwdMaxBlocks = 4096;
// backward: 4 wave slots per workgroup, one partial row of d gamma / d beta per slot.  A trade-off, recorded and not tuned: every slot is
// a row that gn_param_reduce_k reads again, one after the other, so 128 workgroups (512 slots) bound the reduction and the workspace,
// and leave about half of the 256 CUs without a workgroup at M = 6144 (gn_bwd_k 44 us, gn_param_reduce_k 25 us there: DESIGN 4.8)
constexpr int kGnBwdMaxBlocks = 128;
constexpr int kGnBwdRowsPerWave = 2;

static inline int gn_fwd_blocks(int64_t M) {
  const int64_t b = ceil_div(M, (int64_t)kWaves);
  return (int)(b < 1 ? 1 : (b > kGnFwdMaxBlocks ? kGnFwdMaxBlocks : b));
}
static inline int gn_bwd_blocks(int64_t M) {
  const int64_t b = ceil_div(M, (int64_t)kWaves * kGnBwdRowsPerWave);
  return (int)(b < 1 ? 1 : (b > kGnBwdMaxBlocks ? kGnBwdMaxBlocks : b));
}
static inline int gn_slots(int64_t M) { return gn_bwd_blocks(M) * kWaves; }
// two planes [slots][C]: d gamma, d beta partials
static inline size_t gn_workspace_bytes(int64_t M, int32_t C) { return (size_t)2 * (size_t)gn_slots(M) * (size_t)C * sizeof(float); }

}  // namespace norm
}  // namespace clica
