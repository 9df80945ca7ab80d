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

// ------------------------------------------------------------------------------------------------ channels-last (bn2d_nhwc.hip)
// Dense NHWC activations are the row-major matrix x[M = N H W, C], row = pixel.  "rows" geometry, from (M, C) alone:
//   a lane owns `vec` consecutive channels of a row (4 when C % 4 == 0: one 16-byte access when the pointers are aligned; else 1) and
//   walks down the rows; `lpr` lanes (a power of two <= 64) cover a row or a 64-lane chunk of it, so a wave covers 64 / lpr consecutive
//   rows -- at C = 64 one contiguous KB -- and the 4 waves of a workgroup `rps` = 256 / lpr rows per step.  grid.x = chunks of lpr lanes.
//   statistics / sums launches: grid.y = S row splits of `per` rows, sized for kRowsSplitSteps steps of a workgroup.  Every apply
//     workgroup merges the S partials of its lpr * vec channels again, `mg` = 256 / (lpr vec) threads per channel, each the `ms` splits
//     of its range in split order, then the ranges in range order through LDS: S <= kRowsMergeLoads * mg (<= kRowsMaxSplits) keeps that
//     at kRowsMergeLoads / 8 rounds of loads whatever C is, and lets C = 64 -- where one chunk is the whole row -- have 256 splits.
//     The T workgroups of an apply launch read T S C 12 bytes of partials between them, from L2: with S <= 512 and 2048 tiles that was
//     0.8 GB at ResNet-18's C = 64 layers and cost more than the statistics launch gained (profiles/c4_nhwc_summary.md), hence these caps.
//   apply / backward-apply launches: grid.y = T row tiles of `tile` rows, as many as fill the part (kRowsMaxTiles workgroups), at least
//     kRowsTileSteps steps each so that the merge is paid for; the tiles are element-wise work and shape no reduction.
constexpr int kRowsMaxSplits = 256;
constexpr int kRowsMergeLoads = 64;           // partials per channel one thread of an apply workgroup merges, at most
constexpr int kRowsSplitSteps = 32;           // rows a lane takes in a split before the cap on S
constexpr int kRowsTileSteps = 8;             // rows a lane takes in a tile, at least
constexpr int kRowsMaxTiles = 1024;           // apply workgroups: 256 CUs x 4

struct Rows {
  int vec, lpr, rps, chunks;      // channels per lane; lanes per row (chunk); rows per workgroup step; grid.x
  int mg, ms;                     // merge: threads per channel, splits per thread
  int S;                          // row splits = partials per channel
  int64_t per;                    // rows per split (the last one may hold fewer)
  int T;                          // row tiles of the apply launches
  int64_t tile;                   // rows per tile, a multiple of rps
};

static inline Rows rows_geometry(int64_t M, int32_t C) {
  Rows g;
  g.vec = C % 4 == 0 ? 4 : 1;
  const int U = C / g.vec;
  g.lpr = 1;
  while (g.lpr < U && g.lpr < 64) g.lpr *= 2;
  g.rps = kThreads / g.lpr;
  g.chunks = (int)ceil_div((int64_t)U, (int64_t)g.lpr);
  g.mg = kThreads / (g.lpr * g.vec);        // (lpr = 64, vec = 4: a thread per channel)
  int64_t cap = (int64_t)kRowsMergeLoads * g.mg;
  if (cap > kRowsMaxSplits) cap = kRowsMaxSplits;
  int64_t s = ceil_div(M, (int64_t)kRowsSplitSteps * g.rps);
  if (s > cap) s = cap;
  if (s < 1) s = 1;
  g.per = ceil_div(M, s);
  g.S = (int)ceil_div(M, g.per);            // no empty split
  g.ms = (int)ceil_div((int64_t)g.S, (int64_t)g.mg);
  int64_t tiles = kRowsMaxTiles / g.chunks;
  if (tiles < 1) tiles = 1;
  int64_t t = ceil_div(M, tiles);
  if (t < (int64_t)kRowsTileSteps * g.rps) t = (int64_t)kRowsTileSteps * g.rps;
  g.tile = ceil_div(t, (int64_t)g.rps) * g.rps;
  g.T = (int)ceil_div(M, g.tile);
  return g;
}

// forward: three planes [S][C] (count, mean, M2 of x - x[0, c]); backward: two (sum dz, sum dz xhat) in the same buffer
static inline size_t rows_workspace_bytes(int64_t M, int32_t C) {
  return align_up((size_t)3 * (size_t)rows_geometry(M, C).S * (size_t)C * sizeof(float), 16);
}

// ------------------------------------------------------------------------------------------------ channels-last stem unit with the max-pool
// P = maxpool 3x3 / stride 2 / pad 1 of lrelu(gamma xhat + beta), floor mode, on x[N, H, W, C] (bn2d_nhwc.hip).  The lanes are those of
// the "rows" geometry (`vec` channels per lane, `lpr` lanes along C, rps = 256 / lpr pixel slots per workgroup, grid.x = chunks), the
// statistics launch and the merge of its S partials are the unit's own (rows_geometry(N H W, C)).
//   forward: a slot owns an output pixel (n, ho, wo) and reads its <= 9 inputs itself; the N Ho Wo output pixels are cut into `Tf`
//     runs of `tile_f` (as the apply launches above).  No LDS beyond the merge.
//   backward sums: a slot owns a window as in the forward -- a window's gradient lands on one pixel, its first maximum, so the sums over
//     pixels are sums over windows --; the N Ho Wo windows are cut into `Sb` runs of `per_b`, one workgroup and one partial per run and
//     channel, Sb sized and capped as S is.  No LDS beyond the wave merge.
//   backward apply: one TILE = (image, band of BH output rows, band of BW output columns) for a chunk of lpr vec channels.  A workgroup
//     first leaves, for each of the tile's (BH + 1) x (BW + 1) windows -- its own and the row below / column right of them, which share pixels
//     with it --, dP gate(y) (a float) and the position of the window's first maximum (a byte) per channel in LDS, then a slot owns an
//     input pixel of rows 2 ho0 .. 2 (ho0 + BH) - 1, columns 2 wo0 .. 2 (wo0 + BW) - 1 and gathers its <= 4 windows.  LDS per workgroup:
//     (BH + 1)(BW + 1) lpr vec <= kPoolRowsLdsFloats entries of 5 bytes (30 KB), whatever the plane: BW <= 8 columns, then as many rows
//     as fit, both evened out over the plane (C = 64: 8 x 8 windows = 16 x 16 pixels per tile; a chunk of 256 channels: 3 x 4).
//     The N nbh nbw tiles in (image, row band, column band) order are cut into `Ta` runs of `per_a` tiles, each workgroup merging the Sb
//     partials (`msb` per merging thread) as the unit's backward apply does.
// Everything is a function of (N, H, W, C) alone; the only limit on a plane is H, W <= kPoolRowsMaxSide (int arithmetic inside a tile).
constexpr int kPoolRowsLdsFloats = 6144;
constexpr int kPoolRowsMaxSide = 1 << 15;
constexpr int kPoolRowsMaxBand = 8;

struct PoolRows {
  Rows rows;                      // lanes; the statistics launch and the merge of its partials
  int Ho, Wo, BH, BW, nbh, nbw;   // output plane; output rows / columns per tile; bands per plane
  int Sb, msb;                    // backward sums: runs of windows = partials per channel; per merging thread
  int64_t per_b;
  int64_t tiles;                  // backward apply: N nbh nbw tiles
  int Ta;                         //   in runs of per_a
  int64_t per_a;
  int Tf;                         // forward: runs of output pixels
  int64_t tile_f;                 // a multiple of rps
};

static inline bool pool_rows_fits(int32_t H, int32_t W, int32_t C) {
  return H >= 1 && W >= 1 && H <= kPoolRowsMaxSide && W <= kPoolRowsMaxSide && C >= 1 && C <= kMaxC;
}

static inline PoolRows pool_rows_geometry(int64_t N, int32_t C, int32_t H, int32_t W) {
  PoolRows g;
  g.rows = rows_geometry(N * (int64_t)H * W, C);
  const Rows& r = g.rows;
  g.Ho = pool_out(H); g.Wo = pool_out(W);
  static_assert(kPoolRowsLdsFloats / kThreads >= 2 * (kPoolRowsMaxBand + 1), "a tile holds at least one row of windows and the row below");
  const int nwin = kPoolRowsLdsFloats / (r.lpr * r.vec);      // (lpr vec <= 256: >= 24 windows)
  g.nbw = (int)ceil_div((int64_t)g.Wo, (int64_t)kPoolRowsMaxBand);
  g.BW = (int)ceil_div((int64_t)g.Wo, (int64_t)g.nbw);
  int bh = nwin / (g.BW + 1) - 1;
  if (bh > g.Ho) bh = g.Ho;
  g.nbh = (int)ceil_div((int64_t)g.Ho, (int64_t)bh);
  g.BH = (int)ceil_div((int64_t)g.Ho, (int64_t)g.nbh);        // <= bh: (BH + 1)(BW + 1) <= nwin
  g.tiles = N * g.nbh * g.nbw;
  const int64_t Mo = N * g.Ho * g.Wo;
  int64_t cap = (int64_t)kRowsMergeLoads * r.mg;
  if (cap > kRowsMaxSplits) cap = kRowsMaxSplits;
  int64_t s = ceil_div(Mo, (int64_t)kRowsSplitSteps * r.rps);
  if (s > cap) s = cap;
  g.per_b = ceil_div(Mo, s);
  g.Sb = (int)ceil_div(Mo, g.per_b);
  g.msb = (int)ceil_div((int64_t)g.Sb, (int64_t)r.mg);
  int64_t fill = kRowsMaxTiles / r.chunks;                    // workgroups along y that fill the part
  if (fill < 1) fill = 1;
  g.per_a = ceil_div(g.tiles, fill < g.tiles ? fill : g.tiles);
  g.Ta = (int)ceil_div(g.tiles, g.per_a);
  int64_t f = ceil_div(Mo, fill);
  if (f < (int64_t)kRowsTileSteps * r.rps) f = (int64_t)kRowsTileSteps * r.rps;
  g.tile_f = ceil_div(f, (int64_t)r.rps) * r.rps;
  g.Tf = (int)ceil_div(Mo, g.tile_f);
  return g;
}

// forward: the unit's three planes [S][C]; backward: two planes [Sb][C] in the same buffer
static inline size_t pool_rows_workspace_bytes(int64_t N, int32_t C, int32_t H, int32_t W) {
  const PoolRows g = pool_rows_geometry(N, C, H, W);
  const size_t s = (size_t)(g.rows.S > g.Sb ? g.rows.S : g.Sb);
  return align_up((size_t)3 * s * (size_t)C * sizeof(float), 16);
}

// the statistics launch of clica_bn2d_act_fwd_train (bn2d.hip): partials [3][S][C] of geometry(N, HW) into `part`
void launch_stats(hipStream_t st, const float* X, int64_t N, int32_t C, int32_t HW, float* part);

#ifdef __HIPCC__
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

// bf16 activations, carried as their 16 bits.  bf16 -> fp32 is the shift (exact); fp32 -> bf16 rounds to nearest, ties to even, as
// Tensor.to(torch.bfloat16) does (a NaN becomes the quiet NaN 0x7fc0 with the sign dropped, c10's rule).  Every kernel computes in fp32
// on the widened values, so a bf16 instance has the bits of the fp32 one on the upcast input, rounded once at the store.
using bf16_t = uint16_t;
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(bf16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ bf16_t bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)0x7fc0u;
  return (bf16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ void from_f32(float* p, float v) { *p = v; }
__device__ __forceinline__ void from_f32(bf16_t* p, float v) { *p = bf16_rne(v); }

// the same lanes and values on bf16: AL is one 8-byte access (the pointer is 8-byte aligned), else scalar 2-byte accesses
template <int VEC, bool AL>
__device__ __forceinline__ void load(const bf16_t* __restrict__ p, float* v) {
  if (VEC == 4 && AL) {
    const uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = to_f32(p[k]);
  }
}
template <int VEC, bool AL>
__device__ __forceinline__ void store(bf16_t* __restrict__ p, const float* v) {
  if (VEC == 4 && AL) {
    *reinterpret_cast<uint2*>(p) = make_uint2((uint32_t)bf16_rne(v[0]) | (uint32_t)bf16_rne(v[1]) << 16,
                                              (uint32_t)bf16_rne(v[2]) | (uint32_t)bf16_rne(v[3]) << 16);
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) p[k] = bf16_rne(v[k]);
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
