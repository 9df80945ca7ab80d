// BatchNorm2d of ResNet-18 fused with the shortcut add and the ReLU behind it, fp32, contiguous NCHW x[N, C, HW]:
//   z = gamma[c] (x - mean[c]) invstd[c] + beta[c] (+ r),   y = z > 0 ? z : slope z      (slope = 0: ReLU, slope = 1: none)
// Statistics over the N * HW values of a channel.  The backward takes the gate from the saved output (y > 0 -> 1, else slope), as
// norm.hip does; z is never recomputed:  dz = dy gate(y),  dr = dz,  dx = gamma invstd (dz - sum dz / M - xhat sum(dz xhat) / M).
//
// Training forward: plane_stats_k / small_stats_k leaves Welford / Chan partials (count, mean, M2 of x - x[0, c, 0]: the channel's first
// value as pivot) per (image split, channel); apply_k -- the next launch on the stream -- merges the S partials of its channel in split
// order in EVERY workgroup (the same bits everywhere, no hand-off between workgroups), normalises its own split, and split 0 writes
// save_mean / save_invstd and the running statistics.  The backward is the same pair: sums_k, bwd_apply_k.  Inference: apply_k<.., false>
// on the running statistics, one launch.  Geometries "plane" and "small" (bn2d.h): the statistics kernels are written per geometry
// (their four-loads-in-flight loops are the geometry), the other three are one template over the geometry types Plane / Small below.
// A thread folds 4 or 16 values at a time into its statistic: their mean and M2 two-pass in registers, then one Chan merge (one
// division per block, not per value).  The channel finish, the element functions and the merges of partials are bn_core.h's.
// No floating-point atomics, no arrival counters, nothing that waits inside a kernel: phases are ordered by the stream.
#include "bn2d.h"

namespace clica {
namespace bn2d {

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

// ------------------------------------------------------------------------------------------------ statistics, plane geometry
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

// ------------------------------------------------------------------------------------------------ statistics, small geometry (HW = 4 Q, Q = 1, 2, 4)
// grid (64-piece chunks, S).  Piece p = (channel p / Q, quad p % Q); 64 % Q == 0, so a channel's pieces are neighbouring lanes of one wave.
template <bool AL>
__global__ __launch_bounds__(kThreads) void small_stats_k(const float* __restrict__ x, int64_t N, int C, int Q, int64_t per,
                                                         float* __restrict__ part) {
  __shared__ float sh[bn::kColumnStatLds];
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
  bn::column_merge(s, sh);
  if (w == 0) {
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

// ------------------------------------------------------------------------------------------------ the two geometries (bn2d.h)
// What differs between them in the apply, sums and backward-apply kernels below, and nothing else: the channel of a thread and whether
// the lane has work; the thread's element offsets -- for (i = first; i < end; i += kStep) offset(i), VEC values each, in that order --;
// the workgroup's reduction of a pair of sums, with its LDS; the thread that writes a (split, channel) result.
template <int VEC_, bool AL_>
struct Plane {                      // grid (C, S): workgroup = (channel, image split); thread t takes units t, t + 256, ... of its Walk
  static constexpr int VEC = VEC_, kStep = kThreads, kSumsLds = kWaves * 2;
  static constexpr bool AL = AL_;
  int c;
  int64_t first, end;
  Walk wk;
  __device__ Plane(int64_t N, int C, int HW, int64_t per)
      : c((int)blockIdx.x), first(threadIdx.x), wk((int64_t)blockIdx.y * per, HW / VEC_, C, (int)blockIdx.x, HW) {
    const int64_t n0 = (int64_t)blockIdx.y * per, n1 = n0 + per < N ? n0 + per : N;
    end = (n1 - n0) * (HW / VEC_);
  }
  __device__ __forceinline__ bool active() const { return true; }
  __device__ __forceinline__ int64_t offset(int64_t) { return wk.next<VEC_>(); }
  __device__ __forceinline__ bool writer() const { return threadIdx.x == 0; }
  // the lanes of a wave, then the waves in wave order; true in the thread that holds the workgroup's sums
  __device__ __forceinline__ bool reduce(float& a, float& b, float* sh) {
    block_sum2(a, b, sh);
    return threadIdx.x == 0;
  }
};

template <bool AL_>
struct Small {                      // grid (64-piece chunks, S): lane = piece (channel p / Q, quad p % Q), wave w takes images n0 + w, n0 + w + 4, ...
  static constexpr int VEC = 4, kStep = kWaves, kSumsLds = bn::kColumnSumsLds;
  static constexpr bool AL = AL_;
  int c, p, Q;
  bool in;
  int64_t first, end, row;          // row: values of one image
  __device__ Small(int64_t N, int C, int HW, int64_t per) {
    Q = HW / 4;
    p = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63);
    in = p < C * Q;
    c = p / Q;
    const int64_t n0 = (int64_t)blockIdx.y * per;
    first = n0 + (threadIdx.x >> 6);
    end = n0 + per < N ? n0 + per : N;
    row = (int64_t)C * Q * 4;
  }
  __device__ __forceinline__ bool active() const { return in; }
  __device__ __forceinline__ int64_t offset(int64_t n) const { return n * row + (int64_t)p * 4; }
  __device__ __forceinline__ bool writer() const { return threadIdx.x < 64 && p % Q == 0; }      // (of an active lane)
  // the waves in wave order, then the channel's quads in quad order into its first lane (64 % Q == 0: neighbouring lanes of wave 0)
  __device__ __forceinline__ bool reduce(float& a, float& b, float* sh) {
    bn::column_sums(a, b, sh);
    if (threadIdx.x >= 64) return false;
    const int lane = threadIdx.x & 63;
    const float o1 = a, o2 = b;
    for (int j = 1; j < Q; ++j) {
      const float u = __shfl(o1, lane + j, 64), v = __shfl(o2, lane + j, 64);
      if (p % Q == 0) { a += u; b += v; }
    }
    return in && p % Q == 0;
  }
};

// ------------------------------------------------------------------------------------------------ apply, sums, backward apply
// TRAIN: batch statistics from the partials, split 0 holds the writers; otherwise the running statistics (inference).  No barrier: a
// lane without work leaves at once.
template <class G, bool TRAIN>
__global__ __launch_bounds__(kThreads) void apply_k(const float* __restrict__ x, const float* __restrict__ r, const float* __restrict__ gamma,
                                                   const float* __restrict__ beta, int64_t N, int C, int HW, int64_t per, float Mf, float eps,
                                                   float momentum, float slope, const float* __restrict__ part, float* __restrict__ y,
                                                   float* __restrict__ save_mean, float* __restrict__ save_invstd, float* running_mean,
                                                   float* running_var) {
  G geo(N, C, HW, per);
  if (!geo.active()) return;
  const int c = geo.c;
  const bn::Norm nm = TRAIN ? bn::finish_train(bn::merge_stats(part, (int)gridDim.y, C, c), x[(int64_t)c * HW], Mf, eps, momentum, c,
                                               blockIdx.y == 0 && geo.writer(), save_mean, save_invstd, running_mean, running_var)
                            : bn::finish_eval(running_mean, running_var, c, eps);
  const float g = gamma[c], b = beta[c];
#pragma unroll 2
  for (int64_t i = geo.first; i < geo.end; i += G::kStep) {
    const int64_t e = geo.offset(i);
    float v[G::VEC], rr[G::VEC];
    load<G::VEC, G::AL>(x + e, v);
    if (r) load<G::VEC, G::AL>(r + e, rr);
#pragma unroll
    for (int k = 0; k < G::VEC; ++k) {
      float z = bn::affine(bn::xhat(v[k], nm), g, b);
      if (r) z += rr[k];
      v[k] = bn::lrelu(z, slope);
    }
    store<G::VEC, G::AL>(y + e, v);
  }
}

// sum dz and sum dz xhat per (split, channel)
template <class G>
__global__ __launch_bounds__(kThreads) void sums_k(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                  const float* __restrict__ save_mean, const float* __restrict__ save_invstd, int64_t N, int C,
                                                  int HW, int64_t per, float slope, float* __restrict__ part) {
  __shared__ float sh[G::kSumsLds];
  G geo(N, C, HW, per);
  const int c = geo.c;
  float s1 = 0.f, s2 = 0.f;
  if (geo.active()) {
    const bn::Norm nm{save_mean[c], save_invstd[c]};
#pragma unroll 2
    for (int64_t i = geo.first; i < geo.end; i += G::kStep) {
      const int64_t e = geo.offset(i);
      float xv[G::VEC], yv[G::VEC], gv[G::VEC];
      load<G::VEC, G::AL>(x + e, xv); load<G::VEC, G::AL>(y + e, yv); load<G::VEC, G::AL>(dy + e, gv);
#pragma unroll
      for (int k = 0; k < G::VEC; ++k) bn::bwd_sums(s1, s2, bn::bwd_dz(gv[k], yv[k], slope), bn::xhat(xv[k], nm));
    }
  }
  if (geo.reduce(s1, s2, sh)) {
    float* q = part + (size_t)blockIdx.y * C + c;
    q[0] = s1; q[(size_t)gridDim.y * C] = s2;
  }
}

// No barrier.
template <class G>
__global__ __launch_bounds__(kThreads) void bwd_apply_k(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ dy,
                                                       const float* __restrict__ gamma, const float* __restrict__ save_mean,
                                                       const float* __restrict__ save_invstd, int64_t N, int C, int HW, int64_t per, float Mf,
                                                       float slope, const float* __restrict__ part, float* __restrict__ dx,
                                                       float* __restrict__ dr, float* __restrict__ dgamma, float* __restrict__ dbeta) {
  G geo(N, C, HW, per);
  if (!geo.active()) return;
  const int c = geo.c;
  float s1, s2;
  bn::merge_sums(part, (int)gridDim.y, C, c, s1, s2);
  if (blockIdx.y == 0 && geo.writer()) {
    dgamma[c] = s2;
    dbeta[c] = s1;
  }
  const bn::Norm nm{save_mean[c], save_invstd[c]};
  const bn::Bwd bw = bn::bwd_coeffs(gamma[c], nm.invstd, s1, s2, Mf);
#pragma unroll 2
  for (int64_t i = geo.first; i < geo.end; i += G::kStep) {
    const int64_t e = geo.offset(i);
    float xv[G::VEC], yv[G::VEC], gv[G::VEC];
    load<G::VEC, G::AL>(x + e, xv); load<G::VEC, G::AL>(y + e, yv); load<G::VEC, G::AL>(dy + e, gv);
#pragma unroll
    for (int k = 0; k < G::VEC; ++k) {
      gv[k] = bn::bwd_dz(gv[k], yv[k], slope);
      xv[k] = bn::bwd_dx(gv[k], bn::xhat(xv[k], nm), bw);
    }
    store<G::VEC, G::AL>(dx + e, xv);
    if (dr) store<G::VEC, G::AL>(dr + e, gv);
  }
}

// ------------------------------------------------------------------------------------------------ launches
template <class G>
struct Tag { using type = G; };

// f(Tag<geometry>): HW alone picks plane / small and quads / single pixels (the reduction order); `al` only picks 16-byte accesses
template <class F>
static void with_geometry(int32_t HW, bool al, F&& f) {
  if (small_hw(HW)) {
    if (al) f(Tag<Small<true>>{});
    else f(Tag<Small<false>>{});
  } else if (HW % 4 == 0) {
    if (al) f(Tag<Plane<4, true>>{});
    else f(Tag<Plane<4, false>>{});
  } else {
    f(Tag<Plane<1, false>>{});
  }
}

template <bool TRAIN>
static void launch_apply(hipStream_t st, const float* x, const float* r, const float* gamma, const float* beta, int64_t N, int C, int HW,
                         float eps, float momentum, float slope, const float* part, float* y, float* save_mean, float* save_invstd,
                         float* rm, float* rv) {
  const Geometry geo = geometry(N, HW);
  const dim3 grid(grid_x(C, HW), (unsigned)geo.S), block(kThreads);
  const float Mf = (float)(N * (int64_t)HW);
  const bool al = HW % 4 == 0 && aligned16(x) && aligned16(y) && (!r || aligned16(r));
  with_geometry(HW, al, [&](auto tag) {
    using G = typename decltype(tag)::type;
    hipLaunchKernelGGL((apply_k<G, TRAIN>), grid, block, 0, st, x, r, gamma, beta, N, C, HW, geo.per, Mf, eps, momentum, slope, part, y,
                       save_mean, save_invstd, rm, rv);
  });
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
  CLICA_BN_WORKSPACE("clica_bn2d_act_fwd_train", bn2d::workspace_bytes(N, C, HW), "clica_bn2d_workspace_bytes", CLICA_E_INVALID);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  bn2d::launch_stats(st, X, N, C, HW, part);
  bn2d::launch_apply<true>(st, X, R, gamma, beta, N, (int)C, (int)HW, eps, momentum, slope, part, Y, save_mean, save_invstd, running_mean,
                           running_var);
  return launch_status("clica_bn2d_act_fwd_train");
}

extern "C" int clica_bn2d_act_fwd_eval(const float* X, const float* R, const float* gamma, const float* beta, const float* running_mean,
                                       const float* running_var, int64_t N, int32_t C, int32_t HW, float eps, float slope, float* Y,
                                       clica_stream_t stream) {
  CLICA_BN2D_SHAPE("clica_bn2d_act_fwd_eval", 1);
  CLICA_BN2D_SLOPE("clica_bn2d_act_fwd_eval");
  CLICA_CHECK_ARG(X && gamma && beta && running_mean && running_var && Y, "clica_bn2d_act_fwd_eval: NULL pointer");
  // (the inference instance only reads the running statistics)
  bn2d::launch_apply<false>(as_stream(stream), X, R, gamma, beta, N, (int)C, (int)HW, eps, 0.f, slope, nullptr, Y, nullptr, nullptr,
                            const_cast<float*>(running_mean), const_cast<float*>(running_var));
  return launch_status("clica_bn2d_act_fwd_eval");
}

extern "C" int clica_bn2d_act_bwd(const float* X, const float* Y, const float* dY, const float* gamma, const float* save_mean,
                                  const float* save_invstd, int64_t N, int32_t C, int32_t HW, float slope, float* dX, float* dR,
                                  float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  CLICA_BN2D_SHAPE("clica_bn2d_act_bwd", 2);
  CLICA_BN2D_SLOPE("clica_bn2d_act_bwd");
  CLICA_CHECK_ARG(X && Y && dY && gamma && save_mean && save_invstd && dX && dgamma && dbeta && workspace, "clica_bn2d_act_bwd: NULL pointer");
  CLICA_BN_WORKSPACE("clica_bn2d_act_bwd", bn2d::workspace_bytes(N, C, HW), "clica_bn2d_workspace_bytes", CLICA_E_INVALID);
  const bn2d::Geometry geo = bn2d::geometry(N, HW);
  const dim3 grid(bn2d::grid_x(C, HW), (unsigned)geo.S), block(bn2d::kThreads);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const float Mf = (float)(N * (int64_t)HW);
  const bool al = HW % 4 == 0 && bn2d::aligned16(X) && bn2d::aligned16(Y) && bn2d::aligned16(dY) && bn2d::aligned16(dX) && (!dR || bn2d::aligned16(dR));
  bn2d::with_geometry(HW, al, [&](auto tag) {
    using G = typename decltype(tag)::type;
    hipLaunchKernelGGL(bn2d::sums_k<G>, grid, block, 0, st, X, Y, dY, save_mean, save_invstd, N, (int)C, (int)HW, geo.per, slope, part);
    hipLaunchKernelGGL(bn2d::bwd_apply_k<G>, grid, block, 0, st, X, Y, dY, gamma, save_mean, save_invstd, N, (int)C, (int)HW, geo.per, Mf, slope,
                       part, dX, dR, dgamma, dbeta);
  });
  return launch_status("clica_bn2d_act_bwd");
}
