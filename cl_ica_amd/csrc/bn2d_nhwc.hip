// The BatchNorm2d unit of bn2d.hip -- z = gamma xhat + beta (+ r), y = lrelu(z, slope), and its backward from the saved output -- and the
// global average pool on DENSE CHANNELS-LAST fp32 activations: an NHWC tensor is the row-major matrix x[M = N H W, C], row = pixel.
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
// in wave order, the splits as above.  It depends on (M, C) alone; AL only picks 16-byte accesses.
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
template <int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void rows_stats_k(const float* __restrict__ x, int64_t M, int C, int lpr, int64_t per,
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
    const float* xp = x + ln.c0;
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
template <int VEC, bool AL, bool TRAIN>
__global__ __launch_bounds__(kThreads) void rows_apply_k(const float* __restrict__ x, const float* __restrict__ r, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, int64_t M, int C, int lpr, int mg, int ms, int S,
                                                        int64_t tile, float Mf, float eps, float momentum, float slope,
                                                        const float* __restrict__ part, float* __restrict__ y, float* __restrict__ save_mean,
                                                        float* __restrict__ save_invstd, float* running_mean, float* running_var) {
  __shared__ float sh[TRAIN ? kMergeLds : 1];
  __shared__ float shn[TRAIN ? 2 * kThreads : 1];          // mean, invstd of the chunk's channels
  const Lane<VEC> ln(C, lpr);
  bn::Norm nm[VEC];
  if (TRAIN) {
    const Merger mr(C, lpr, VEC);
    const Stat t = merged_stat(mr, part, S, C, mg, ms, sh);
    if (mr.first()) {
      const bn::Norm n = bn::finish_train(t, x[mr.c], Mf, eps, momentum, mr.c, blockIdx.y == 0, save_mean, save_invstd, running_mean,
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
template <int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void rows_sums_k(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
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
template <int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void rows_bwd_apply_k(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                            const float* __restrict__ gamma, const float* __restrict__ save_mean,
                                                            const float* __restrict__ save_invstd, int64_t M, int C, int lpr, int mg, int ms,
                                                            int S, int64_t tile, float Mf, float slope, const float* __restrict__ part,
                                                            float* __restrict__ dx, float* __restrict__ dr, float* __restrict__ dgamma,
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

// f(Tag<VEC, AL>): C alone picks VEC (the reduction order); `al` only picks 16-byte accesses
template <class F>
static void with_lane(int vec, bool al, F&& f) {
  if (vec == 4) {
    if (al) f(Tag<4, true>{});
    else f(Tag<4, false>{});
  } else {
    f(Tag<1, false>{});
  }
}

template <bool TRAIN>
static void launch_apply(hipStream_t st, const float* x, const float* r, const float* gamma, const float* beta, int64_t M, int C, float eps,
                         float momentum, float slope, const float* part, float* y, float* save_mean, float* save_invstd, float* rm,
                         float* rv) {
  const Rows geo = rows_geometry(M, C);
  const dim3 grid((unsigned)geo.chunks, (unsigned)geo.T), block(kThreads);
  const bool al = aligned16(x) && aligned16(y) && (!r || aligned16(r));
  with_lane(geo.vec, al, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((rows_apply_k<T::VEC, T::AL, TRAIN>), grid, block, 0, st, x, r, gamma, beta, M, C, geo.lpr, geo.mg, geo.ms, geo.S,
                       geo.tile, (float)M, eps, momentum, slope, part, y, save_mean, save_invstd, rm, rv);
  });
}

// ------------------------------------------------------------------------------------------------ global average pool, x[N, HW, C]
// thread = (n, c), lanes along C: the HW values of a channel in pixel order
__global__ __launch_bounds__(kThreads) void avgpool_fwd_k(const float* __restrict__ x, int64_t NC, int HW, int C, float inv,
                                                         float* __restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= NC) return;
  const int64_t n = t / C;
  const float* p = x + n * HW * C + (t - n * C);
  float s = 0.f;
#pragma unroll 4
  for (int k = 0; k < HW; ++k) s += p[(int64_t)k * C];
  y[t] = s * inv;
}

// thread = element (n, k, c)
__global__ __launch_bounds__(kThreads) void avgpool_bwd_k(const float* __restrict__ dy, int64_t total, int HW, int C, float inv,
                                                         float* __restrict__ dx) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (t >= total) return;
  const int64_t nk = t / C;
  dx[t] = dy[(nk / HW) * C + (t - nk * C)] * inv;
}

}  // namespace nhwc
}  // namespace bn2d
}  // namespace clica

using namespace clica;
using bn2d::nhwc::with_lane;

#define CLICA_BN2D_NHWC_SHAPE(fn, min_M)                                                                                       \
  CLICA_CHECK_ARG(M >= (min_M) && C >= 1 && C <= bn2d::kMaxC && (double)M * (double)C < 1e18,                                  \
                  fn ": M=%lld C=%d (M = N H W >= %d, 1 <= C <= %d)", (long long)M, C, (min_M), bn2d::kMaxC)

#define CLICA_BN2D_NHWC_SLOPE(fn) \
  CLICA_CHECK_ARG(slope >= 0.f, fn ": slope=%g must be >= 0 (the backward recovers the gate from the output)", slope)

extern "C" int clica_bn2d_nhwc_workspace_bytes(int64_t M, int32_t C, size_t* bytes) {
  CLICA_CHECK_ARG(bytes != nullptr, "clica_bn2d_nhwc_workspace_bytes: bytes is NULL");
  CLICA_BN2D_NHWC_SHAPE("clica_bn2d_nhwc_workspace_bytes", 1);
  *bytes = bn2d::rows_workspace_bytes(M, C);
  return CLICA_OK;
}

extern "C" int clica_bn2d_nhwc_act_fwd_train(const float* X, const float* R, const float* gamma, const float* beta, int64_t M, int32_t C,
                                             float eps, float momentum, float slope, float* Y, float* save_mean, float* save_invstd,
                                             float* running_mean, float* running_var, void* workspace, size_t workspace_bytes,
                                             clica_stream_t stream) {
  CLICA_BN2D_NHWC_SHAPE("clica_bn2d_nhwc_act_fwd_train", 2);
  CLICA_BN2D_NHWC_SLOPE("clica_bn2d_nhwc_act_fwd_train");
  CLICA_CHECK_ARG(X && gamma && beta && Y && save_mean && save_invstd && workspace, "clica_bn2d_nhwc_act_fwd_train: NULL pointer");
  CLICA_BN_WORKSPACE("clica_bn2d_nhwc_act_fwd_train", bn2d::rows_workspace_bytes(M, C), "clica_bn2d_nhwc_workspace_bytes", CLICA_E_INVALID);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const bn2d::Rows geo = bn2d::rows_geometry(M, C);
  const dim3 grid((unsigned)geo.chunks, (unsigned)geo.S), block(bn2d::kThreads);
  with_lane(geo.vec, bn2d::aligned16(X), [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((bn2d::nhwc::rows_stats_k<T::VEC, T::AL>), grid, block, 0, st, X, M, (int)C, geo.lpr, geo.per, part);
  });
  bn2d::nhwc::launch_apply<true>(st, X, R, gamma, beta, M, (int)C, eps, momentum, slope, part, Y, save_mean, save_invstd, running_mean,
                                 running_var);
  return launch_status("clica_bn2d_nhwc_act_fwd_train");
}

extern "C" int clica_bn2d_nhwc_act_fwd_eval(const float* X, const float* R, const float* gamma, const float* beta, const float* running_mean,
                                            const float* running_var, int64_t M, int32_t C, float eps, float slope, float* Y,
                                            clica_stream_t stream) {
  CLICA_BN2D_NHWC_SHAPE("clica_bn2d_nhwc_act_fwd_eval", 1);
  CLICA_BN2D_NHWC_SLOPE("clica_bn2d_nhwc_act_fwd_eval");
  CLICA_CHECK_ARG(X && gamma && beta && running_mean && running_var && Y, "clica_bn2d_nhwc_act_fwd_eval: NULL pointer");
  // (the inference instance only reads the running statistics)
  bn2d::nhwc::launch_apply<false>(as_stream(stream), X, R, gamma, beta, M, (int)C, eps, 0.f, slope, nullptr, Y, nullptr, nullptr,
                                  const_cast<float*>(running_mean), const_cast<float*>(running_var));
  return launch_status("clica_bn2d_nhwc_act_fwd_eval");
}

extern "C" int clica_bn2d_nhwc_act_bwd(const float* X, const float* Y, const float* dY, const float* gamma, const float* save_mean,
                                       const float* save_invstd, int64_t M, int32_t C, float slope, float* dX, float* dR, float* dgamma,
                                       float* dbeta, void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  CLICA_BN2D_NHWC_SHAPE("clica_bn2d_nhwc_act_bwd", 2);
  CLICA_BN2D_NHWC_SLOPE("clica_bn2d_nhwc_act_bwd");
  CLICA_CHECK_ARG(X && Y && dY && gamma && save_mean && save_invstd && dX && dgamma && dbeta && workspace,
                  "clica_bn2d_nhwc_act_bwd: NULL pointer");
  CLICA_BN_WORKSPACE("clica_bn2d_nhwc_act_bwd", bn2d::rows_workspace_bytes(M, C), "clica_bn2d_nhwc_workspace_bytes", CLICA_E_INVALID);
  const bn2d::Rows geo = bn2d::rows_geometry(M, C);
  const dim3 sgrid((unsigned)geo.chunks, (unsigned)geo.S), agrid((unsigned)geo.chunks, (unsigned)geo.T), block(bn2d::kThreads);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const bool al = bn2d::aligned16(X) && bn2d::aligned16(Y) && bn2d::aligned16(dY) && bn2d::aligned16(dX) && (!dR || bn2d::aligned16(dR));
  with_lane(geo.vec, al, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((bn2d::nhwc::rows_sums_k<T::VEC, T::AL>), sgrid, block, 0, st, X, Y, dY, save_mean, save_invstd, M, (int)C, geo.lpr,
                       geo.per, slope, part);
    hipLaunchKernelGGL((bn2d::nhwc::rows_bwd_apply_k<T::VEC, T::AL>), agrid, block, 0, st, X, Y, dY, gamma, save_mean, save_invstd, M,
                       (int)C, geo.lpr, geo.mg, geo.ms, geo.S, geo.tile, (float)M, slope, part, dX, dR, dgamma, dbeta);
  });
  return launch_status("clica_bn2d_nhwc_act_bwd");
}

// (the limits of clica_avgpool2d_global_*: pool2d.hip)
#define CLICA_AVGPOOL_NHWC_SHAPE(fn)                                                                                                  \
  CLICA_CHECK_ARG(N >= 1 && HW >= 1 && HW <= (1 << 14) && C >= 1 && C <= bn2d::kMaxC && N * (int64_t)C <= ((int64_t)1 << 31) &&      \
                      (double)N * (double)HW * (double)C <= 274877906944.0,                                                          \
                  fn ": N=%lld HW=%d C=%d (N >= 1, 1 <= HW <= 16384, 1 <= C <= %d, N C <= 2^31, N HW C <= 2^38)", (long long)N, HW, C, \
                  bn2d::kMaxC)

extern "C" int clica_avgpool2d_global_nhwc_fwd(const float* X, int64_t N, int32_t HW, int32_t C, float* Y, clica_stream_t stream) {
  CLICA_AVGPOOL_NHWC_SHAPE("clica_avgpool2d_global_nhwc_fwd");
  CLICA_CHECK_ARG(X && Y, "clica_avgpool2d_global_nhwc_fwd: NULL pointer");
  const int64_t NC = N * C;
  const dim3 grid((unsigned)ceil_div(NC, bn2d::kThreads)), block(bn2d::kThreads);
  hipLaunchKernelGGL(bn2d::nhwc::avgpool_fwd_k, grid, block, 0, as_stream(stream), X, NC, (int)HW, (int)C, 1.f / (float)HW, Y);
  return launch_status("clica_avgpool2d_global_nhwc_fwd");
}

extern "C" int clica_avgpool2d_global_nhwc_bwd(const float* dY, int64_t N, int32_t HW, int32_t C, float* dX, clica_stream_t stream) {
  CLICA_AVGPOOL_NHWC_SHAPE("clica_avgpool2d_global_nhwc_bwd");
  CLICA_CHECK_ARG(dY && dX, "clica_avgpool2d_global_nhwc_bwd: NULL pointer");
  const int64_t total = N * HW * C;
  const dim3 grid((unsigned)ceil_div(total, bn2d::kThreads)), block(bn2d::kThreads);
  hipLaunchKernelGGL(bn2d::nhwc::avgpool_bwd_k, grid, block, 0, as_stream(stream), dY, total, (int)HW, (int)C, 1.f / (float)HW, dX);
  return launch_status("clica_avgpool2d_global_nhwc_bwd");
}
