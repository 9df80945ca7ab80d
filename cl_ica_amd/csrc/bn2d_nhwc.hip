// The BatchNorm2d unit of bn2d.hip -- z = gamma xhat + beta (+ r), y = lrelu(z, slope), and its backward from the saved output -- and the
// global average pool on DENSE CHANNELS-LAST fp32 activations: an NHWC tensor is the row-major matrix x[M = N H W, C], row = pixel.
// Every kernel takes the activations' element type T: float, or bf16 as its 16 bits (bn2d.h: widened exactly on load, rounded to nearest
// even on store).  Statistics, parameters, partials, LDS and every accumulation are fp32 in both, and the geometry does not know T: a
// bf16 instance computes what the fp32 one computes on the upcast input.
//
// Geometry "rows" (bn2d.h, rows_geometry): a lane owns VEC consecutive channels (4 when C % 4 == 0, else 1) and walks down the rows; lpr
// lanes cover a row (or a 64-lane chunk of it: grid.x), a wave 64 / lpr consecutive rows, the workgroup rps = 256 / lpr rows per step.
// With four channels per lane the kernels of bn2d.hip do not fit (one Norm, one pair of sums per thread there), so these are their
// siblings: the same element functions, channel finish and merges of bn_core.h, per lane VEC times.
//
// Training forward: rows_stats_k leaves Welford / Chan partials of x - x[0, c] per (row split, channel); rows_apply_k, the next launch
// on the stream, runs over row TILES (as many workgroups as fill the part, whatever S is): each workgroup merges the S partials of its
// lpr VEC channels -- mg threads per channel, each its range of ms splits in split order, thread 0 of the channel the ranges in range
// order through LDS -- finishes the channel (tile 0 writes save_mean / save_invstd and the running statistics) and normalises its rows.
// Backward: rows_sums_k and rows_bwd_apply_k, the same pair.  Inference: rows_apply_k<.., false>, one launch.
// The reduction tree of a channel: per lane over its rows m0 + row, m0 + row + rps, ... (blocks of four rows two-pass in registers, as
// bn2d.hip), the lanes of a wave that hold the channel by shuffles (lane l takes lane l + off, off = 32 .. lpr), the waves through LDS
// in wave order, the splits as above.  It depends on (M, C) alone; AL only picks one access per lane (16 bytes of fp32, 8 of bf16).
// The stem unit with its max-pool, P = maxpool 3 x 3 / 2 / 1 of y, on the same lanes (bn2d.h, PoolRows): rows_stats_k, then
// pool_rows_fwd_k, which merges and finishes as rows_apply_k and writes each output pixel's first maximum; inference: one launch;
// backward: pool_rows_sums_k (a slot per window: the sums need no pixels) and pool_rows_bwd_apply_k, which recomputes y per tile of
// windows and gathers dz per pixel.
// No floating-point atomics, no arrival counters, nothing that waits inside a kernel: phases are ordered by the stream.
#include "bn2d.h"

namespace clica {
namespace bn2d {
namespace nhwc {

// the thread's place: channels c0 .. c0 + VEC - 1 (in: the lane has channels), row `row` of every workgroup step of `rps` rows
template <int VEC>
struct Lane {
  int c0, row, rps, ci0;      // ci0: c0 within the workgroup's chunk of channels
  bool in;
  __device__ Lane(int C, int lpr) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, rpw = 64 / lpr;
    ci0 = (lane & (lpr - 1)) * VEC;
    c0 = (int)blockIdx.x * lpr * VEC + ci0;
    in = c0 < C;              // (C % VEC == 0: all of the lane's channels or none)
    row = w * rpw + lane / lpr;
    rps = kWaves * rpw;
  }
};

// ------------------------------------------------------------------------------------------------ statistics: grid (chunks, S)
template <class T, int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void rows_stats_k(const T* __restrict__ x, int64_t M, int C, int lpr, int64_t per,
                                                        float* __restrict__ part) {
  __shared__ float sh[VEC * bn::kColumnStatLds];
  const Lane<VEC> ln(C, lpr);
  const int split = (int)blockIdx.y, S = (int)gridDim.y;
  const int64_t m0 = (int64_t)split * per;
  const int64_t m1 = m0 + per < M ? m0 + per : M;
  Stat s[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) s[k] = Stat{0.f, 0.f, 0.f, 0.f};
  if (ln.in) {
    float pivot[VEC];                                      // moments of x - x[0, c]
    load<VEC, AL>(x + ln.c0, pivot);
    const T* xp = x + ln.c0;
    const int64_t step = ln.rps;
    int64_t m = m0 + ln.row;
    for (; m + 3 * step < m1; m += 4 * step) {             // four rows' loads in flight, then one block of 4 values per channel
      float d[4][VEC];
#pragma unroll
      for (int j = 0; j < 4; ++j) load<VEC, AL>(xp + (m + j * step) * C, d[j]);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float e[4] = {d[0][k] - pivot[k], d[1][k] - pivot[k], d[2][k] - pivot[k], d[3][k] - pivot[k]};
        stat_block<4>(s[k], e);
      }
    }
    for (; m < m1; m += step) {
      float d[VEC];
      load<VEC, AL>(xp + m * C, d);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        const float e = d[k] - pivot[k];
        stat_block<1>(s[k], &e);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    for (int off = 32; off >= lpr; off >>= 1) stat_merge(s[k], shfl_down_stat(s[k], off));      // lane l < off takes lane l + off
    bn::column_merge(s[k], sh + k * bn::kColumnStatLds);
  }
  if ((int)threadIdx.x < lpr && ln.in) {                   // wave 0, the first of the lanes that hold the channels
    const size_t plane = (size_t)S * C;
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float* q = part + (size_t)split * C + ln.c0 + k;
      q[0] = s[k].cnt; q[plane] = s[k].mean; q[2 * plane] = s[k].m2;
    }
  }
}

// ------------------------------------------------------------------------------------------------ the S partials of a workgroup's channels
// Thread t: channel t % CH of the chunk's CH = lpr VEC, range t / CH of the mg = 256 / CH ranges of ms splits.  All threads call (two
// barriers); thread 0 of a channel (range 0) ends with its value.
constexpr int kMergeLds = 3 * kThreads;

struct Merger {
  int ci, g, c, CH;
  bool in;
  __device__ Merger(int C, int lpr, int vec) {
    CH = lpr * vec;
    ci = (int)threadIdx.x & (CH - 1);
    g = (int)threadIdx.x / CH;
    c = (int)blockIdx.x * CH + ci;
    in = c < C;
  }
  __device__ __forceinline__ bool first() const { return in && g == 0; }
};

__device__ __forceinline__ Stat merged_stat(const Merger& mr, const float* __restrict__ part, int S, int C, int mg, int ms, float* sh /*[kMergeLds]*/) {
  Stat t{0.f, 0.f, 0.f, 0.f};
  const int s0 = mr.g * ms, s1 = s0 + ms < S ? s0 + ms : S;
  if (mr.in) t = bn::merge_stats_range(part, S, C, mr.c, s0, s1);
  const int i = (int)threadIdx.x;
  sh[i] = t.cnt; sh[kThreads + i] = t.mean; sh[2 * kThreads + i] = t.m2;
  __syncthreads();
  if (mr.first())
    for (int j = 1; j < mg; ++j) {
      const int o = j * mr.CH + mr.ci;
      stat_merge(t, Stat{sh[o], sh[kThreads + o], sh[2 * kThreads + o], 0.f});
    }
  __syncthreads();
  return t;
}

__device__ __forceinline__ void merged_sums(const Merger& mr, const float* __restrict__ part, int S, int C, int mg, int ms, float* sh /*[kMergeLds]*/,
                                            float& a, float& b) {
  a = 0.f; b = 0.f;
  const int s0 = mr.g * ms, s1 = s0 + ms < S ? s0 + ms : S;
  if (mr.in) bn::merge_sums_range(part, S, C, mr.c, s0, s1, a, b);
  const int i = (int)threadIdx.x;
  sh[i] = a; sh[kThreads + i] = b;
  __syncthreads();
  if (mr.first())
    for (int j = 1; j < mg; ++j) {
      const int o = j * mr.CH + mr.ci;
      a += sh[o]; b += sh[kThreads + o];
    }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------ apply: grid (chunks, T)
// TRAIN: batch statistics from the partials, tile 0 holds the writers; otherwise the running statistics (inference, no LDS, no barrier).
template <class T, int VEC, bool AL, bool TRAIN>
__global__ __launch_bounds__(kThreads) void rows_apply_k(const T* __restrict__ x, const T* __restrict__ r, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int64_t M, int C, int lpr, int mg, int ms, int S,
                                                        int64_t tile, float Mf, float eps, float momentum, float slope,
                                                        const float* __restrict__ part, T* __restrict__ y, float* __restrict__ save_mean,
                                                        float* __restrict__ save_invstd, float* running_mean, float* running_var) {
  __shared__ float sh[TRAIN ? kMergeLds : 1];
  __shared__ float shn[TRAIN ? 2 * kThreads : 1];          // mean, invstd of the chunk's channels
  const Lane<VEC> ln(C, lpr);
  bn::Norm nm[VEC];
  if (TRAIN) {
    const Merger mr(C, lpr, VEC);
    const Stat t = merged_stat(mr, part, S, C, mg, ms, sh);
    if (mr.first()) {
      const bn::Norm n = bn::finish_train(t, to_f32(x[mr.c]), Mf, eps, momentum, mr.c, blockIdx.y == 0, save_mean, save_invstd, running_mean,
                                          running_var);
      shn[mr.ci] = n.mean; shn[kThreads + mr.ci] = n.invstd;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < VEC; ++k) nm[k] = bn::Norm{shn[ln.ci0 + k], shn[kThreads + ln.ci0 + k]};
  }
  if (!ln.in) return;
  float g[VEC], b[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    if (!TRAIN) nm[k] = bn::finish_eval(running_mean, running_var, ln.c0 + k, eps);
    g[k] = gamma[ln.c0 + k]; b[k] = beta[ln.c0 + k];
  }
  const int64_t r0 = (int64_t)blockIdx.y * tile;
  const int64_t r1 = r0 + tile < M ? r0 + tile : M;
#pragma unroll 2
  for (int64_t m = r0 + ln.row; m < r1; m += ln.rps) {
    const int64_t e = m * C + ln.c0;
    float v[VEC], rr[VEC];
    load<VEC, AL>(x + e, v);
    if (r) load<VEC, AL>(r + e, rr);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float z = bn::affine(bn::xhat(v[k], nm[k]), g[k], b[k]);
      if (r) z += rr[k];
      v[k] = bn::lrelu(z, slope);
    }
    store<VEC, AL>(y + e, v);
  }
}

// ------------------------------------------------------------------------------------------------ backward sums: grid (chunks, S)
template <class T, int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void rows_sums_k(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ dy,
                                                       const float* __restrict__ save_mean, const float* __restrict__ save_invstd, int64_t M,
                                                       int C, int lpr, int64_t per, float slope, float* __restrict__ part) {
  __shared__ float sh[VEC * bn::kColumnSumsLds];
  const Lane<VEC> ln(C, lpr);
  const int split = (int)blockIdx.y, S = (int)gridDim.y;
  const int64_t m0 = (int64_t)split * per;
  const int64_t m1 = m0 + per < M ? m0 + per : M;
  float s1[VEC], s2[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) { s1[k] = 0.f; s2[k] = 0.f; }
  if (ln.in) {
    bn::Norm nm[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) nm[k] = bn::Norm{save_mean[ln.c0 + k], save_invstd[ln.c0 + k]};
#pragma unroll 2
    for (int64_t m = m0 + ln.row; m < m1; m += ln.rps) {
      const int64_t e = m * C + ln.c0;
      float xv[VEC], yv[VEC], gv[VEC];
      load<VEC, AL>(x + e, xv); load<VEC, AL>(y + e, yv); load<VEC, AL>(dy + e, gv);
#pragma unroll
      for (int k = 0; k < VEC; ++k) bn::bwd_sums(s1[k], s2[k], bn::bwd_dz(gv[k], yv[k], slope), bn::xhat(xv[k], nm[k]));
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    for (int off = 32; off >= lpr; off >>= 1) { s1[k] += __shfl_down(s1[k], off, 64); s2[k] += __shfl_down(s2[k], off, 64); }
    bn::column_sums(s1[k], s2[k], sh + k * bn::kColumnSumsLds);
  }
  if ((int)threadIdx.x < lpr && ln.in) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float* q = part + (size_t)split * C + ln.c0 + k;
      q[0] = s1[k]; q[(size_t)S * C] = s2[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------ backward apply: grid (chunks, T)
template <class T, int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void rows_bwd_apply_k(const T* __restrict__ x, const T* __restrict__ y, const T* __restrict__ dy,
                                                            const float* __restrict__ gamma, const float* __restrict__ save_mean,
                                                            const float* __restrict__ save_invstd, int64_t M, int C, int lpr, int mg, int ms,
                                                            int S, int64_t tile, float Mf, float slope, const float* __restrict__ part,
                                                            T* __restrict__ dx, T* __restrict__ dr, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta) {
  __shared__ float sh[kMergeLds];
  __shared__ float shs[2 * kThreads];                      // sum dz, sum dz xhat of the chunk's channels
  const Lane<VEC> ln(C, lpr);
  {
    const Merger mr(C, lpr, VEC);
    float a, b;
    merged_sums(mr, part, S, C, mg, ms, sh, a, b);
    if (mr.first()) {
      if (blockIdx.y == 0) {
        dgamma[mr.c] = b;
        dbeta[mr.c] = a;
      }
      shs[mr.ci] = a; shs[kThreads + mr.ci] = b;
    }
    __syncthreads();
  }
  if (!ln.in) return;
  bn::Norm nm[VEC];
  bn::Bwd bw[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    nm[k] = bn::Norm{save_mean[ln.c0 + k], save_invstd[ln.c0 + k]};
    bw[k] = bn::bwd_coeffs(gamma[ln.c0 + k], nm[k].invstd, shs[ln.ci0 + k], shs[kThreads + ln.ci0 + k], Mf);
  }
  const int64_t r0 = (int64_t)blockIdx.y * tile;
  const int64_t r1 = r0 + tile < M ? r0 + tile : M;
#pragma unroll 2
  for (int64_t m = r0 + ln.row; m < r1; m += ln.rps) {
    const int64_t e = m * C + ln.c0;
    float xv[VEC], yv[VEC], gv[VEC];
    load<VEC, AL>(x + e, xv); load<VEC, AL>(y + e, yv); load<VEC, AL>(dy + e, gv);
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      gv[k] = bn::bwd_dz(gv[k], yv[k], slope);
      xv[k] = bn::bwd_dx(gv[k], bn::xhat(xv[k], nm[k]), bw[k]);
    }
    store<VEC, AL>(dx + e, xv);
    if (dr) store<VEC, AL>(dr + e, gv);
  }
}

// ------------------------------------------------------------------------------------------------ launches
template <int VEC_, bool AL_>
struct Tag {
  static constexpr int VEC = VEC_;
  static constexpr bool AL = AL_;
};

// f(Tag<VEC, AL>): C alone picks VEC (the reduction order); `al` only picks one access per lane: 16 bytes of fp32, 8 bytes of bf16
template <class T>
static inline bool lane_aligned(const T* p) { return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0; }

template <class F>
static void with_lane(int vec, bool al, F&& f) {
  if (vec == 4) {
    if (al) f(Tag<4, true>{});
    else f(Tag<4, false>{});
  } else {
    f(Tag<1, false>{});
  }
}

template <bool TRAIN, class T>
static void launch_apply(hipStream_t st, const T* x, const T* r, const float* gamma, const float* beta, int64_t M, int C, float eps,
                         float momentum, float slope, const float* part, T* y, float* save_mean, float* save_invstd, float* rm,
                         float* rv) {
  const Rows geo = rows_geometry(M, C);
  const dim3 grid((unsigned)geo.chunks, (unsigned)geo.T), block(kThreads);
  const bool al = lane_aligned(x) && lane_aligned(y) && (!r || lane_aligned(r));
  with_lane(geo.vec, al, [&](auto tag) {
    using L = decltype(tag);
    hipLaunchKernelGGL((rows_apply_k<T, L::VEC, L::AL, TRAIN>), grid, block, 0, st, x, r, gamma, beta, M, C, geo.lpr, geo.mg, geo.ms, geo.S,
                       geo.tile, (float)M, eps, momentum, slope, part, y, save_mean, save_invstd, rm, rv);
  });
}

// ------------------------------------------------------------------------------------------------ global average pool, x[N, HW, C]
// thread = (n, c), lanes along C: the HW values of a channel in pixel order
template <class T>
__global__ __launch_bounds__(kThreads) void avgpool_fwd_k(const T* __restrict__ x, int64_t NC, int HW, int C, float inv,
                                                         float* __restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= NC) return;
  const int64_t n = t / C;
  const T* p = x + n * HW * C + (t - n * C);
  float s = 0.f;
#pragma unroll 4
  for (int k = 0; k < HW; ++k) s += to_f32(p[(int64_t)k * C]);
  y[t] = s * inv;
}

// thread = element (n, k, c)
template <class T>
__global__ __launch_bounds__(kThreads) void avgpool_bwd_k(const float* __restrict__ dy, int64_t total, int HW, int C, float inv,
                                                         T* __restrict__ dx) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int64_t nk = t / C;
  from_f32(dx + t, dy[(nk / HW) * C + (t - nk * C)] * inv);
}

// ------------------------------------------------------------------------------------------------ the stem unit with its max-pool
// P = maxpool 3 x 3 / stride 2 / padding 1 of y = lrelu(gamma xhat + beta, slope), on x[N, H, W, C]; geometry: bn2d.h, PoolRows.
//
// The window (ho, wo) of the image at xn (= x + n H W C + c0), per channel of the lane: y of its pixels inside the plane in scan order
// (rows, then columns), its maximum and the position 0 .. 8 of the maximum's first occurrence -- strict >, torch's rule and window_max's
// of pool2d.hip, so the bits of that first maximum, signed zeros included -- and xhat of that pixel in xm.  The nine loads are issued
// before the first comparison; a position outside the plane loads the window's centre, which is always inside, and never wins.
template <int VEC, bool AL, class T>
__device__ __forceinline__ void window_first_max(const T* __restrict__ xn, int ho, int wo, int H, int W, int C, const bn::Norm* nm,
                                                 const float* g, const float* b, float slope, float* m, int* code, float* xm) {
  float v[9][VEC];
  bool ok[9];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int hh = 2 * ho - 1 + dy;
    const bool vr = hh >= 0 && hh < H;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int ww = 2 * wo - 1 + dx;
      const bool vc = ww >= 0 && ww < W;
      ok[dy * 3 + dx] = vr && vc;
      load<VEC, AL>(xn + ((int64_t)(vr ? hh : 2 * ho) * W + (vc ? ww : 2 * wo)) * C, v[dy * 3 + dx]);
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) { m[k] = -INFINITY; code[k] = 4; xm[k] = 0.f; }
#pragma unroll
  for (int p = 0; p < 9; ++p) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float xh = bn::xhat(v[p][k], nm[k]);
      const float y = bn::fwd_xhat(xh, g[k], b[k], slope);      // (= bn::fwd: the unit's y)
      if (ok[p] && y > m[k]) { m[k] = y; code[k] = p; xm[k] = xh; }
    }
  }
}

// forward: grid (chunks, Tf); a slot (Lane::row) owns an output pixel o = (n, ho, wo) of its run of `tile`.  TRAIN as rows_apply_k.
template <class T, int VEC, bool AL, bool TRAIN>
__global__ __launch_bounds__(kThreads) void pool_rows_fwd_k(const T* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int64_t Mo, int C, int H, int W, int Ho, int Wo,
                                                           int lpr, int mg, int ms, int S, int64_t tile, float Mf, float eps, float momentum,
                                                           float slope, const float* __restrict__ part, T* __restrict__ P,
                                                           float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                           float* running_mean, float* running_var) {
  __shared__ float sh[TRAIN ? kMergeLds : 1];
  __shared__ float shn[TRAIN ? 2 * kThreads : 1];          // mean, invstd of the chunk's channels
  const Lane<VEC> ln(C, lpr);
  bn::Norm nm[VEC];
  if (TRAIN) {
    const Merger mr(C, lpr, VEC);
    const Stat t = merged_stat(mr, part, S, C, mg, ms, sh);
    if (mr.first()) {
      const bn::Norm n = bn::finish_train(t, to_f32(x[mr.c]), Mf, eps, momentum, mr.c, blockIdx.y == 0, save_mean, save_invstd, running_mean,
                                          running_var);
      shn[mr.ci] = n.mean; shn[kThreads + mr.ci] = n.invstd;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < VEC; ++k) nm[k] = bn::Norm{shn[ln.ci0 + k], shn[kThreads + ln.ci0 + k]};
  }
  if (!ln.in) return;
  float g[VEC], b[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    if (!TRAIN) nm[k] = bn::finish_eval(running_mean, running_var, ln.c0 + k, eps);
    g[k] = gamma[ln.c0 + k]; b[k] = beta[ln.c0 + k];
  }
  const int HoWo = Ho * Wo;
  const int64_t o0 = (int64_t)blockIdx.y * tile;
  const int64_t o1 = o0 + tile < Mo ? o0 + tile : Mo;
  for (int64_t o = o0 + ln.row; o < o1; o += ln.rps) {
    const int64_t n = o / HoWo;
    const int r = (int)(o - n * HoWo), ho = r / Wo, wo = r - ho * Wo;
    float m[VEC], xm[VEC];
    int code[VEC];
    window_first_max<VEC, AL>(x + n * H * W * C + ln.c0, ho, wo, H, W, C, nm, g, b, slope, m, code, xm);
    store<VEC, AL>(P + o * C + ln.c0, m);
  }
}

// backward sums: grid (chunks, Sb) over runs of `per` output pixels, a slot per window as pool_rows_fwd_k.  A window's gated gradient
// d = dP gate(y_max) lands on exactly one pixel, its first maximum, so over a channel
//   sum over pixels of dz = sum over windows of d,      sum over pixels of dz xhat = sum over windows of d xhat(first maximum):
// the sums need the windows, not the pixels -- no LDS staging, no halo.  The partial's tree: per lane over its windows in order, then
// lanes and waves as rows_sums_k.
template <class T, int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void pool_rows_sums_k(const T* __restrict__ x, const T* __restrict__ dP,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
                                                            int64_t Mo, int C, int H, int W, int Ho, int Wo, int lpr, int64_t per,
                                                            float slope, float* __restrict__ part) {
  __shared__ float sh[VEC * bn::kColumnSumsLds];
  const Lane<VEC> ln(C, lpr);
  const int split = (int)blockIdx.y, S = (int)gridDim.y;
  float s1[VEC], s2[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) { s1[k] = 0.f; s2[k] = 0.f; }
  if (ln.in) {
    bn::Norm nm[VEC];
    float g[VEC], b[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      nm[k] = bn::Norm{save_mean[ln.c0 + k], save_invstd[ln.c0 + k]};
      g[k] = gamma[ln.c0 + k]; b[k] = beta[ln.c0 + k];
    }
    const int HoWo = Ho * Wo;
    const int64_t o0 = (int64_t)split * per;
    const int64_t o1 = o0 + per < Mo ? o0 + per : Mo;
    for (int64_t o = o0 + ln.row; o < o1; o += ln.rps) {
      const int64_t n = o / HoWo;
      const int r = (int)(o - n * HoWo), ho = r / Wo, wo = r - ho * Wo;
      float m[VEC], xm[VEC], d[VEC];
      int code[VEC];
      load<VEC, AL>(dP + o * C + ln.c0, d);
      window_first_max<VEC, AL>(x + n * H * W * C + ln.c0, ho, wo, H, W, C, nm, g, b, slope, m, code, xm);
#pragma unroll
      for (int k = 0; k < VEC; ++k) bn::bwd_sums(s1[k], s2[k], bn::bwd_dz(d[k], m[k], slope), xm[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    for (int off = 32; off >= lpr; off >>= 1) { s1[k] += __shfl_down(s1[k], off, 64); s2[k] += __shfl_down(s2[k], off, 64); }
    bn::column_sums(s1[k], s2[k], sh + k * bn::kColumnSumsLds);
  }
  if ((int)threadIdx.x < lpr && ln.in) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      float* q = part + (size_t)split * C + ln.c0 + k;
      q[0] = s1[k]; q[(size_t)S * C] = s2[k];
    }
  }
}

struct PoolPlane { int H, W, C, Ho, Wo, BH, BW, nbh, nbw; };

// The positions of the first maxima of a lane's VEC channels, a byte each: one 4-byte LDS access when VEC = 4 (entries of 4 channels
// start at multiples of 4).
template <int VEC>
__device__ __forceinline__ void codes_store(unsigned char* p, const int* code) {
  if (VEC == 4) *reinterpret_cast<uint32_t*>(p) = (uint32_t)code[0] | (uint32_t)code[1] << 8 | (uint32_t)code[2] << 16 | (uint32_t)code[3] << 24;
  else p[0] = (unsigned char)code[0];
}
template <int VEC>
__device__ __forceinline__ void codes_load(const unsigned char* p, int* code) {
  if (VEC == 4) {
    const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) code[k] = (int)(u >> (8 * k) & 255u);
  } else {
    code[0] = p[0];
  }
}
template <int VEC>
__device__ __forceinline__ void lds_store(float* p, const float* v) {
  if (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else p[0] = v[0];
}
template <int VEC>
__device__ __forceinline__ void lds_load(const float* p, float* v) {
  if (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}

// dz of the tile's pixel (lh, lw) -- row 2 ho0 + lh, column 2 wo0 + lw of the plane -- for the lane's channels (entry ci0 of the chunk):
// the gated gradients of the <= 4 windows that contain the pixel and whose first maximum it is, added in window order (ho, then wo), as
// pool_dz of pool2d.hip.  hb / wb: the pixel is also row 0 of the window below / column 0 of the window to the right.
template <int VEC>
__device__ __forceinline__ void pool_rows_dz(const float* sd, const unsigned char* sc, int lh, int lw, bool hb, bool wb, int stride, int CH,
                                             int ci0, float* dz) {
  const int ha = lh >> 1, wa = lw >> 1, ph = (lh & 1) + 1, pw = (lw & 1) + 1;            // position (ph, pw) in window (ha, wa)
  const int h2 = hb ? ha + 1 : ha, w2 = wb ? wa + 1 : wa;
  const int o[4] = {(ha * stride + wa) * CH + ci0, (ha * stride + w2) * CH + ci0, (h2 * stride + wa) * CH + ci0,
                    (h2 * stride + w2) * CH + ci0};
  float d[4][VEC];
  int c[4][VEC];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lds_load<VEC>(sd + o[j], d[j]);
    codes_load<VEC>(sc + o[j], c[j]);
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    float acc = c[0][k] == ph * 3 + pw ? d[0][k] : 0.f;
    acc += wb && c[1][k] == ph * 3 ? d[1][k] : 0.f;
    acc += hb && c[2][k] == pw ? d[2][k] : 0.f;
    acc += hb && wb && c[3][k] == 0 ? d[3][k] : 0.f;
    dz[k] = acc;
  }
}

// backward apply: grid (chunks, Ta), a workgroup per run of `per` tiles; run 0 writes dgamma and dbeta.  Per tile every slot takes
// windows i = row, row + rps, ... of the tile's staged (BH + 1) x (BW + 1) (the part inside the output plane) and leaves dP gate(y_max)
// in sd and the position of the first maximum in sc, entry (window, channel of the chunk); after a barrier it takes pixels i = row,
// row + rps, ... of the tile's own (row-major), gathers dz and writes dx.  Lanes without channels only keep the barriers company.
template <class T, int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void pool_rows_bwd_apply_k(const T* __restrict__ x, const T* __restrict__ dP,
                                                                 const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
                                                                 PoolPlane g, int lpr, int mg, int ms, int S, int64_t tiles, int64_t per,
                                                                 float Mf, float slope, const float* __restrict__ part,
                                                                 T* __restrict__ dx, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta) {
  __shared__ float sh[kMergeLds];
  __shared__ float shs[2 * kThreads];                      // sum dz, sum dz xhat of the chunk's channels
  __shared__ __attribute__((aligned(16))) float sd[kPoolRowsLdsFloats];
  __shared__ __attribute__((aligned(16))) unsigned char sc[kPoolRowsLdsFloats];
  const Lane<VEC> ln(g.C, lpr);
  {
    const Merger mr(g.C, lpr, VEC);
    float a, b;
    merged_sums(mr, part, S, g.C, mg, ms, sh, a, b);
    if (mr.first()) {
      if (blockIdx.y == 0) {
        dgamma[mr.c] = b;
        dbeta[mr.c] = a;
      }
      shs[mr.ci] = a; shs[kThreads + mr.ci] = b;
    }
    __syncthreads();
  }
  bn::Norm nm[VEC];
  bn::Bwd bw[VEC];
  float gm[VEC], bt[VEC];
  if (ln.in) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      nm[k] = bn::Norm{save_mean[ln.c0 + k], save_invstd[ln.c0 + k]};
      gm[k] = gamma[ln.c0 + k]; bt[k] = beta[ln.c0 + k];
      bw[k] = bn::bwd_coeffs(gm[k], nm[k].invstd, shs[ln.ci0 + k], shs[kThreads + ln.ci0 + k], Mf);
    }
  }
  const int CH = lpr * VEC, per_image = g.nbh * g.nbw, stride = g.BW + 1;
  const int64_t t0 = (int64_t)blockIdx.y * per;
  const int64_t t1 = t0 + per < tiles ? t0 + per : tiles;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t n = t / per_image;
    const int r = (int)(t - n * per_image), bh = r / g.nbw, bwi = r - bh * g.nbw;
    const int ho0 = bh * g.BH, wo0 = bwi * g.BW;
    const int nh = g.BH < g.Ho - ho0 ? g.BH : g.Ho - ho0, nw = g.BW < g.Wo - wo0 ? g.BW : g.Wo - wo0;      // the tile's own windows
    const int wh = nh + 1 < g.Ho - ho0 ? nh + 1 : g.Ho - ho0, ww = nw + 1 < g.Wo - wo0 ? nw + 1 : g.Wo - wo0;      // staged
    const int ph = 2 * nh < g.H - 2 * ho0 ? 2 * nh : g.H - 2 * ho0, pw = 2 * nw < g.W - 2 * wo0 ? 2 * nw : g.W - 2 * wo0;      // own pixels
    if (ln.in) {
      const T* xn = x + n * g.H * g.W * g.C + ln.c0;
      const T* dpn = dP + n * g.Ho * g.Wo * g.C + ln.c0;
      for (int i = ln.row; i < wh * ww; i += ln.rps) {
        const int lh = i / ww, lw = i - lh * ww, ho = ho0 + lh, wo = wo0 + lw;
        float m[VEC], xm[VEC], d[VEC];
        int code[VEC];
        load<VEC, AL>(dpn + ((int64_t)ho * g.Wo + wo) * g.C, d);
        window_first_max<VEC, AL>(xn, ho, wo, g.H, g.W, g.C, nm, gm, bt, slope, m, code, xm);
#pragma unroll
        for (int k = 0; k < VEC; ++k) d[k] = bn::bwd_dz(d[k], m[k], slope);
        const int e = (lh * stride + lw) * CH + ln.ci0;
        lds_store<VEC>(sd + e, d);
        codes_store<VEC>(sc + e, code);
      }
    }
    __syncthreads();
    if (ln.in) {
      const int64_t base = n * g.H * g.W * g.C + ln.c0;
#pragma unroll 2
      for (int i = ln.row; i < ph * pw; i += ln.rps) {
        const int lh = i / pw, lw = i - lh * pw;
        const bool hb = (lh & 1) && ho0 + (lh >> 1) + 1 < g.Ho, wb = (lw & 1) && wo0 + (lw >> 1) + 1 < g.Wo;
        const int64_t e = base + ((int64_t)(2 * ho0 + lh) * g.W + (2 * wo0 + lw)) * g.C;
        float v[VEC], dz[VEC];
        load<VEC, AL>(x + e, v);
        pool_rows_dz<VEC>(sd, sc, lh, lw, hb, wb, stride, CH, ln.ci0, dz);
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = bn::bwd_dx(dz[k], bn::xhat(v[k], nm[k]), bw[k]);
        store<VEC, AL>(dx + e, v);
      }
    }
    __syncthreads();
  }
}

template <bool TRAIN, class T>
static void launch_pool_fwd(hipStream_t st, const T* x, const float* gamma, const float* beta, int64_t N, int C, int H, int W, float eps,
                            float momentum, float slope, const float* part, T* P, float* save_mean, float* save_invstd, float* rm,
                            float* rv) {
  const PoolRows geo = pool_rows_geometry(N, C, H, W);
  const Rows& r = geo.rows;
  const dim3 grid((unsigned)r.chunks, (unsigned)geo.Tf), block(kThreads);
  with_lane(r.vec, lane_aligned(x) && lane_aligned(P), [&](auto tag) {
    using L = decltype(tag);
    hipLaunchKernelGGL((pool_rows_fwd_k<T, L::VEC, L::AL, TRAIN>), grid, block, 0, st, x, gamma, beta, N * geo.Ho * geo.Wo, C, H, W, geo.Ho,
                       geo.Wo, r.lpr, r.mg, r.ms, r.S, geo.tile_f, (float)(N * H * W), eps, momentum, slope, part, P, save_mean, save_invstd,
                       rm, rv);
  });
}

}  // namespace nhwc
}  // namespace bn2d
}  // namespace clica

using namespace clica;
using bn2d::nhwc::with_lane;
using bn2d::nhwc::lane_aligned;

// The entry points come in pairs, fp32 and bf16 activations, on one body each: `fn` is the entry point's name, T the activations'
// element (float, or bf16 as its 16 bits).  Checks, geometry, workspace and return codes do not depend on T.
#define CLICA_BN2D_NHWC_SHAPE(fn, min_M)                                                                                       \
  CLICA_CHECK_ARG(M >= (min_M) && C >= 1 && C <= bn2d::kMaxC && (double)M * (double)C < 1e18,                                  \
                  "%s: M=%lld C=%d (M = N H W >= %d, 1 <= C <= %d)", fn, (long long)M, C, (min_M), bn2d::kMaxC)

#define CLICA_BN2D_NHWC_SLOPE(fn) \
  CLICA_CHECK_ARG(slope >= 0.f, "%s: slope=%g must be >= 0 (the backward recovers the gate from the output)", fn, slope)

// CLICA_BN_WORKSPACE (bn_core.h) with the entry point's name at run time
#define CLICA_BN2D_NHWC_WORKSPACE(fn, need, size_fn, short_code)                                                       \
  do {                                                                                                                 \
    CLICA_CHECK_ARG(bn2d::aligned16(workspace), "%s: workspace must be 16-byte aligned", fn);                          \
    const size_t need_ = (need);                                                                                       \
    if (workspace_bytes < need_) {                                                                                     \
      ::clica::set_error("%s: workspace of %zu bytes, %zu needed (" size_fn ")", fn, workspace_bytes, need_);          \
      return short_code;                                                                                               \
    }                                                                                                                  \
  } while (0)

extern "C" int clica_bn2d_nhwc_workspace_bytes(int64_t M, int32_t C, size_t* bytes) {
  CLICA_CHECK_ARG(bytes != nullptr, "clica_bn2d_nhwc_workspace_bytes: bytes is NULL");
  CLICA_BN2D_NHWC_SHAPE("clica_bn2d_nhwc_workspace_bytes", 1);
  *bytes = bn2d::rows_workspace_bytes(M, C);
  return CLICA_OK;
}

namespace {

template <class T>
int act_fwd_train(const char* fn, const T* X, const T* R, const float* gamma, const float* beta, int64_t M, int32_t C, float eps,
                  float momentum, float slope, T* Y, float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                  void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  CLICA_BN2D_NHWC_SHAPE(fn, 2);
  CLICA_BN2D_NHWC_SLOPE(fn);
  CLICA_CHECK_ARG(X && gamma && beta && Y && save_mean && save_invstd && workspace, "%s: NULL pointer", fn);
  CLICA_BN2D_NHWC_WORKSPACE(fn, bn2d::rows_workspace_bytes(M, C), "clica_bn2d_nhwc_workspace_bytes", CLICA_E_INVALID);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const bn2d::Rows geo = bn2d::rows_geometry(M, C);
  const dim3 grid((unsigned)geo.chunks, (unsigned)geo.S), block(bn2d::kThreads);
  with_lane(geo.vec, lane_aligned(X), [&](auto tag) {
    using L = decltype(tag);
    hipLaunchKernelGGL((bn2d::nhwc::rows_stats_k<T, L::VEC, L::AL>), grid, block, 0, st, X, M, (int)C, geo.lpr, geo.per, part);
  });
  bn2d::nhwc::launch_apply<true>(st, X, R, gamma, beta, M, (int)C, eps, momentum, slope, part, Y, save_mean, save_invstd, running_mean,
                                 running_var);
  return launch_status(fn);
}

template <class T>
int act_fwd_eval(const char* fn, const T* X, const T* R, const float* gamma, const float* beta, const float* running_mean,
                 const float* running_var, int64_t M, int32_t C, float eps, float slope, T* Y, clica_stream_t stream) {
  CLICA_BN2D_NHWC_SHAPE(fn, 1);
  CLICA_BN2D_NHWC_SLOPE(fn);
  CLICA_CHECK_ARG(X && gamma && beta && running_mean && running_var && Y, "%s: NULL pointer", fn);
  // (the inference instance only reads the running statistics)
  bn2d::nhwc::launch_apply<false>(as_stream(stream), X, R, gamma, beta, M, (int)C, eps, 0.f, slope, static_cast<const float*>(nullptr), Y,
                                  static_cast<float*>(nullptr), static_cast<float*>(nullptr), const_cast<float*>(running_mean),
                                  const_cast<float*>(running_var));
  return launch_status(fn);
}

template <class T>
int act_bwd(const char* fn, const T* X, const T* Y, const T* dY, const float* gamma, const float* save_mean, const float* save_invstd,
            int64_t M, int32_t C, float slope, T* dX, T* dR, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes,
            clica_stream_t stream) {
  CLICA_BN2D_NHWC_SHAPE(fn, 2);
  CLICA_BN2D_NHWC_SLOPE(fn);
  CLICA_CHECK_ARG(X && Y && dY && gamma && save_mean && save_invstd && dX && dgamma && dbeta && workspace, "%s: NULL pointer", fn);
  CLICA_BN2D_NHWC_WORKSPACE(fn, bn2d::rows_workspace_bytes(M, C), "clica_bn2d_nhwc_workspace_bytes", CLICA_E_INVALID);
  const bn2d::Rows geo = bn2d::rows_geometry(M, C);
  const dim3 sgrid((unsigned)geo.chunks, (unsigned)geo.S), agrid((unsigned)geo.chunks, (unsigned)geo.T), block(bn2d::kThreads);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const bool al = lane_aligned(X) && lane_aligned(Y) && lane_aligned(dY) && lane_aligned(dX) && (!dR || lane_aligned(dR));
  with_lane(geo.vec, al, [&](auto tag) {
    using L = decltype(tag);
    hipLaunchKernelGGL((bn2d::nhwc::rows_sums_k<T, L::VEC, L::AL>), sgrid, block, 0, st, X, Y, dY, save_mean, save_invstd, M, (int)C,
                       geo.lpr, geo.per, slope, part);
    hipLaunchKernelGGL((bn2d::nhwc::rows_bwd_apply_k<T, L::VEC, L::AL>), agrid, block, 0, st, X, Y, dY, gamma, save_mean, save_invstd, M,
                       (int)C, geo.lpr, geo.mg, geo.ms, geo.S, geo.tile, (float)M, slope, part, dX, dR, dgamma, dbeta);
  });
  return launch_status(fn);
}

}  // namespace

extern "C" int clica_bn2d_nhwc_act_fwd_train(const float* X, const float* R, const float* gamma, const float* beta, int64_t M, int32_t C,
                                             float eps, float momentum, float slope, float* Y, float* save_mean, float* save_invstd,
                                             float* running_mean, float* running_var, void* workspace, size_t workspace_bytes,
                                             clica_stream_t stream) {
  return act_fwd_train("clica_bn2d_nhwc_act_fwd_train", X, R, gamma, beta, M, C, eps, momentum, slope, Y, save_mean, save_invstd,
                       running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int clica_bn2d_nhwc_act_fwd_train_bf16(const uint16_t* X, const uint16_t* R, const float* gamma, const float* beta, int64_t M,
                                                  int32_t C, float eps, float momentum, float slope, uint16_t* Y, float* save_mean,
                                                  float* save_invstd, float* running_mean, float* running_var, void* workspace,
                                                  size_t workspace_bytes, clica_stream_t stream) {
  return act_fwd_train("clica_bn2d_nhwc_act_fwd_train_bf16", X, R, gamma, beta, M, C, eps, momentum, slope, Y, save_mean, save_invstd,
                       running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int clica_bn2d_nhwc_act_fwd_eval(const float* X, const float* R, const float* gamma, const float* beta, const float* running_mean,
                                            const float* running_var, int64_t M, int32_t C, float eps, float slope, float* Y,
                                            clica_stream_t stream) {
  return act_fwd_eval("clica_bn2d_nhwc_act_fwd_eval", X, R, gamma, beta, running_mean, running_var, M, C, eps, slope, Y, stream);
}

extern "C" int clica_bn2d_nhwc_act_fwd_eval_bf16(const uint16_t* X, const uint16_t* R, const float* gamma, const float* beta,
                                                 const float* running_mean, const float* running_var, int64_t M, int32_t C, float eps,
                                                 float slope, uint16_t* Y, clica_stream_t stream) {
  return act_fwd_eval("clica_bn2d_nhwc_act_fwd_eval_bf16", X, R, gamma, beta, running_mean, running_var, M, C, eps, slope, Y, stream);
}

extern "C" int clica_bn2d_nhwc_act_bwd(const float* X, const float* Y, const float* dY, const float* gamma, const float* save_mean,
                                       const float* save_invstd, int64_t M, int32_t C, float slope, float* dX, float* dR, float* dgamma,
                                       float* dbeta, void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  return act_bwd("clica_bn2d_nhwc_act_bwd", X, Y, dY, gamma, save_mean, save_invstd, M, C, slope, dX, dR, dgamma, dbeta, workspace,
                 workspace_bytes, stream);
}

extern "C" int clica_bn2d_nhwc_act_bwd_bf16(const uint16_t* X, const uint16_t* Y, const uint16_t* dY, const float* gamma,
                                            const float* save_mean, const float* save_invstd, int64_t M, int32_t C, float slope,
                                            uint16_t* dX, uint16_t* dR, float* dgamma, float* dbeta, void* workspace,
                                            size_t workspace_bytes, clica_stream_t stream) {
  return act_bwd("clica_bn2d_nhwc_act_bwd_bf16", X, Y, dY, gamma, save_mean, save_invstd, M, C, slope, dX, dR, dgamma, dbeta, workspace,
                 workspace_bytes, stream);
}

#define CLICA_POOL_NHWC_SHAPE(fn, min_M)                                                                                                  \
  CLICA_CHECK_ARG(N >= 1 && N <= INT32_MAX && bn2d::pool_rows_fits(H, W, C) && (double)N * H * W >= (min_M) &&                            \
                      (double)N * (double)H * (double)W * (double)C < 1e18,                                                               \
                  "%s: N=%lld C=%d H=%d W=%d (N >= 1, 1 <= C <= %d, 1 <= H, W <= %d, N H W >= %d)", fn, (long long)N, C, H, W,            \
                  bn2d::kMaxC, bn2d::kPoolRowsMaxSide, (min_M))

// (as pool2d.hip's: the pool's argmax is taken after the activation)
#define CLICA_POOL_NHWC_SLOPE(fn) CLICA_CHECK_ARG(slope >= 0.f && slope <= 1.f, "%s: slope=%g must be in [0, 1]", fn, slope)

#define CLICA_POOL_NHWC_WORKSPACE(fn) \
  CLICA_BN2D_NHWC_WORKSPACE(fn, bn2d::pool_rows_workspace_bytes(N, C, H, W), "clica_bn2d_nhwc_maxpool_workspace_bytes", CLICA_E_WORKSPACE)

extern "C" int clica_bn2d_nhwc_maxpool_workspace_bytes(int64_t N, int32_t C, int32_t H, int32_t W, size_t* bytes) {
  CLICA_CHECK_ARG(bytes != nullptr, "clica_bn2d_nhwc_maxpool_workspace_bytes: bytes is NULL");
  CLICA_POOL_NHWC_SHAPE("clica_bn2d_nhwc_maxpool_workspace_bytes", 2);
  *bytes = bn2d::pool_rows_workspace_bytes(N, C, H, W);
  return CLICA_OK;
}

namespace {

template <class T>
int act_maxpool_fwd_train(const char* fn, const T* X, const float* gamma, const float* beta, int64_t N, int32_t C, int32_t H, int32_t W,
                          float eps, float momentum, float slope, T* P, float* save_mean, float* save_invstd, float* running_mean,
                          float* running_var, void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  CLICA_POOL_NHWC_SHAPE(fn, 2);
  CLICA_POOL_NHWC_SLOPE(fn);
  CLICA_CHECK_ARG(X && gamma && beta && P && save_mean && save_invstd && workspace, "%s: NULL pointer", fn);
  CLICA_POOL_NHWC_WORKSPACE(fn);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const int64_t M = N * H * W;
  const bn2d::Rows geo = bn2d::rows_geometry(M, C);          // the unit's statistics launch: its partials, its bits
  const dim3 grid((unsigned)geo.chunks, (unsigned)geo.S), block(bn2d::kThreads);
  with_lane(geo.vec, lane_aligned(X), [&](auto tag) {
    using L = decltype(tag);
    hipLaunchKernelGGL((bn2d::nhwc::rows_stats_k<T, L::VEC, L::AL>), grid, block, 0, st, X, M, (int)C, geo.lpr, geo.per, part);
  });
  bn2d::nhwc::launch_pool_fwd<true>(st, X, gamma, beta, N, (int)C, (int)H, (int)W, eps, momentum, slope, part, P, save_mean, save_invstd,
                                    running_mean, running_var);
  return launch_status(fn);
}

template <class T>
int act_maxpool_fwd_eval(const char* fn, const T* X, const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, int64_t N, int32_t C, int32_t H, int32_t W, float eps, float slope, T* P,
                         clica_stream_t stream) {
  CLICA_POOL_NHWC_SHAPE(fn, 1);
  CLICA_POOL_NHWC_SLOPE(fn);
  CLICA_CHECK_ARG(X && gamma && beta && running_mean && running_var && P, "%s: NULL pointer", fn);
  // (the inference instance only reads the running statistics)
  bn2d::nhwc::launch_pool_fwd<false>(as_stream(stream), X, gamma, beta, N, (int)C, (int)H, (int)W, eps, 0.f, slope,
                                     static_cast<const float*>(nullptr), P, static_cast<float*>(nullptr), static_cast<float*>(nullptr),
                                     const_cast<float*>(running_mean), const_cast<float*>(running_var));
  return launch_status(fn);
}

template <class T>
int act_maxpool_bwd(const char* fn, const T* X, const T* dP, const float* gamma, const float* beta, const float* save_mean,
                    const float* save_invstd, int64_t N, int32_t C, int32_t H, int32_t W, float slope, T* dX, float* dgamma, float* dbeta,
                    void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  CLICA_POOL_NHWC_SHAPE(fn, 2);
  CLICA_POOL_NHWC_SLOPE(fn);
  CLICA_CHECK_ARG(X && dP && gamma && beta && save_mean && save_invstd && dX && dgamma && dbeta && workspace, "%s: NULL pointer", fn);
  CLICA_POOL_NHWC_WORKSPACE(fn);
  const bn2d::PoolRows geo = bn2d::pool_rows_geometry(N, C, H, W);
  const bn2d::Rows& r = geo.rows;
  const bn2d::nhwc::PoolPlane plane{(int)H, (int)W, (int)C, geo.Ho, geo.Wo, geo.BH, geo.BW, geo.nbh, geo.nbw};
  const dim3 sgrid((unsigned)r.chunks, (unsigned)geo.Sb), agrid((unsigned)r.chunks, (unsigned)geo.Ta), block(bn2d::kThreads);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const bool al = lane_aligned(X) && lane_aligned(dP) && lane_aligned(dX);
  with_lane(r.vec, al, [&](auto tag) {
    using L = decltype(tag);
    hipLaunchKernelGGL((bn2d::nhwc::pool_rows_sums_k<T, L::VEC, L::AL>), sgrid, block, 0, st, X, dP, gamma, beta, save_mean, save_invstd,
                       N * geo.Ho * geo.Wo, (int)C, (int)H, (int)W, geo.Ho, geo.Wo, r.lpr, geo.per_b, slope, part);
    hipLaunchKernelGGL((bn2d::nhwc::pool_rows_bwd_apply_k<T, L::VEC, L::AL>), agrid, block, 0, st, X, dP, gamma, beta, save_mean,
                       save_invstd, plane, r.lpr, r.mg, geo.msb, geo.Sb, geo.tiles, geo.per_a, (float)(N * H * W), slope, part, dX, dgamma,
                       dbeta);
  });
  return launch_status(fn);
}

}  // namespace

extern "C" int clica_bn2d_nhwc_act_maxpool_fwd_train(const float* X, const float* gamma, const float* beta, int64_t N, int32_t C, int32_t H,
                                                     int32_t W, float eps, float momentum, float slope, float* P, float* save_mean,
                                                     float* save_invstd, float* running_mean, float* running_var, void* workspace,
                                                     size_t workspace_bytes, clica_stream_t stream) {
  return act_maxpool_fwd_train("clica_bn2d_nhwc_act_maxpool_fwd_train", X, gamma, beta, N, C, H, W, eps, momentum, slope, P, save_mean,
                               save_invstd, running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int clica_bn2d_nhwc_act_maxpool_fwd_train_bf16(const uint16_t* X, const float* gamma, const float* beta, int64_t N, int32_t C,
                                                          int32_t H, int32_t W, float eps, float momentum, float slope, uint16_t* P,
                                                          float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                                                          void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  return act_maxpool_fwd_train("clica_bn2d_nhwc_act_maxpool_fwd_train_bf16", X, gamma, beta, N, C, H, W, eps, momentum, slope, P, save_mean,
                               save_invstd, running_mean, running_var, workspace, workspace_bytes, stream);
}

extern "C" int clica_bn2d_nhwc_act_maxpool_fwd_eval(const float* X, const float* gamma, const float* beta, const float* running_mean,
                                                    const float* running_var, int64_t N, int32_t C, int32_t H, int32_t W, float eps,
                                                    float slope, float* P, clica_stream_t stream) {
  return act_maxpool_fwd_eval("clica_bn2d_nhwc_act_maxpool_fwd_eval", X, gamma, beta, running_mean, running_var, N, C, H, W, eps, slope, P,
                              stream);
}

extern "C" int clica_bn2d_nhwc_act_maxpool_fwd_eval_bf16(const uint16_t* X, const float* gamma, const float* beta, const float* running_mean,
                                                         const float* running_var, int64_t N, int32_t C, int32_t H, int32_t W, float eps,
                                                         float slope, uint16_t* P, clica_stream_t stream) {
  return act_maxpool_fwd_eval("clica_bn2d_nhwc_act_maxpool_fwd_eval_bf16", X, gamma, beta, running_mean, running_var, N, C, H, W, eps,
                              slope, P, stream);
}

extern "C" int clica_bn2d_nhwc_act_maxpool_bwd(const float* X, const float* dP, const float* gamma, const float* beta, const float* save_mean,
                                               const float* save_invstd, int64_t N, int32_t C, int32_t H, int32_t W, float slope, float* dX,
                                               float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  return act_maxpool_bwd("clica_bn2d_nhwc_act_maxpool_bwd", X, dP, gamma, beta, save_mean, save_invstd, N, C, H, W, slope, dX, dgamma,
                         dbeta, workspace, workspace_bytes, stream);
}

extern "C" int clica_bn2d_nhwc_act_maxpool_bwd_bf16(const uint16_t* X, const uint16_t* dP, const float* gamma, const float* beta,
                                                    const float* save_mean, const float* save_invstd, int64_t N, int32_t C, int32_t H,
                                                    int32_t W, float slope, uint16_t* dX, float* dgamma, float* dbeta, void* workspace,
                                                    size_t workspace_bytes, clica_stream_t stream) {
  return act_maxpool_bwd("clica_bn2d_nhwc_act_maxpool_bwd_bf16", X, dP, gamma, beta, save_mean, save_invstd, N, C, H, W, slope, dX, dgamma,
                         dbeta, workspace, workspace_bytes, stream);
}

// (the limits of clica_avgpool2d_global_*: pool2d.hip)
#define CLICA_AVGPOOL_NHWC_SHAPE(fn)                                                                                                  \
  CLICA_CHECK_ARG(N >= 1 && HW >= 1 && HW <= (1 << 14) && C >= 1 && C <= bn2d::kMaxC && N * (int64_t)C <= ((int64_t)1 << 31) &&      \
                      (double)N * (double)HW * (double)C <= 274877906944.0,                                                          \
                  "%s: N=%lld HW=%d C=%d (N >= 1, 1 <= HW <= 16384, 1 <= C <= %d, N C <= 2^31, N HW C <= 2^38)", fn, (long long)N, HW, \
                  C, bn2d::kMaxC)

namespace {

template <class T>
int avgpool_fwd(const char* fn, const T* X, int64_t N, int32_t HW, int32_t C, float* Y, clica_stream_t stream) {
  CLICA_AVGPOOL_NHWC_SHAPE(fn);
  CLICA_CHECK_ARG(X && Y, "%s: NULL pointer", fn);
  const int64_t NC = N * C;
  const dim3 grid((unsigned)ceil_div(NC, bn2d::kThreads)), block(bn2d::kThreads);
  hipLaunchKernelGGL(bn2d::nhwc::avgpool_fwd_k<T>, grid, block, 0, as_stream(stream), X, NC, (int)HW, (int)C, 1.f / (float)HW, Y);
  return launch_status(fn);
}

template <class T>
int avgpool_bwd(const char* fn, const float* dY, int64_t N, int32_t HW, int32_t C, T* dX, clica_stream_t stream) {
  CLICA_AVGPOOL_NHWC_SHAPE(fn);
  CLICA_CHECK_ARG(dY && dX, "%s: NULL pointer", fn);
  const int64_t total = N * HW * C;
  const dim3 grid((unsigned)ceil_div(total, bn2d::kThreads)), block(bn2d::kThreads);
  hipLaunchKernelGGL(bn2d::nhwc::avgpool_bwd_k<T>, grid, block, 0, as_stream(stream), dY, total, (int)HW, (int)C, 1.f / (float)HW, dX);
  return launch_status(fn);
}

}  // namespace

extern "C" int clica_avgpool2d_global_nhwc_fwd(const float* X, int64_t N, int32_t HW, int32_t C, float* Y, clica_stream_t stream) {
  return avgpool_fwd("clica_avgpool2d_global_nhwc_fwd", X, N, HW, C, Y, stream);
}

extern "C" int clica_avgpool2d_global_nhwc_fwd_bf16(const uint16_t* X, int64_t N, int32_t HW, int32_t C, float* Y, clica_stream_t stream) {
  return avgpool_fwd("clica_avgpool2d_global_nhwc_fwd_bf16", X, N, HW, C, Y, stream);
}

extern "C" int clica_avgpool2d_global_nhwc_bwd(const float* dY, int64_t N, int32_t HW, int32_t C, float* dX, clica_stream_t stream) {
  return avgpool_bwd("clica_avgpool2d_global_nhwc_bwd", dY, N, HW, C, dX, stream);
}

extern "C" int clica_avgpool2d_global_nhwc_bwd_bf16(const float* dY, int64_t N, int32_t HW, int32_t C, uint16_t* dX, clica_stream_t stream) {
  return avgpool_bwd("clica_avgpool2d_global_nhwc_bwd_bf16", dY, N, HW, C, dX, stream);
}
