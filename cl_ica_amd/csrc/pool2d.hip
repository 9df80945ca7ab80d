// The two pools of ResNet-18 on contiguous fp32 NCHW tensors.
//
// 1. The stem unit: BatchNorm2d + (leaky) ReLU of bn2d.hip with the 3x3 / stride 2 / pad 1 max-pool behind it (floor mode),
//      y = lrelu(gamma xhat + beta, slope),   P[n, c, ho, wo] = max of y over rows 2 ho - 1 .. 2 ho + 1, columns 2 wo - 1 .. 2 wo + 1
//    (the part inside the plane: padding never wins).  y, pooling indices and the sparse gradient dy never reach memory.
//    Training forward: bn2d.hip's statistics launch (the same partials, hence the bits of the unfused unit in save_mean, save_invstd
//    and the running statistics), then pool_fwd_k: every workgroup merges the partials of its channel (bn_core.h's merge and channel
//    finish, as bn2d.hip's apply_k), forms y for a batch of whole planes in LDS with bn_core.h's forward element function -- the
//    unfused unit's, hence the same bits -- and writes the maxima.  Inference: pool_fwd_k<.., false> on the running statistics, one launch.
//    Backward from x, dP, gamma, beta and the saved statistics: a batch's xhat planes go to LDS; a thread per window forms y from xhat,
//    finds the window's FIRST maximum in scan order (rows, then columns: torch's rule) and leaves its position (a nibble) and
//    dP gate(y) in LDS; then a pixel GATHERS  dz = the sum over the <= 4 windows that contain it and whose first maximum it is.
//    pool_sums_k reduces sum dz and sum dz xhat into [S][C] partials, pool_bwd_apply_k (the next launch) sums them in split order
//    and writes dx = gamma invstd (dz - sum dz / M - xhat sum(dz xhat) / M).
//    Workgroup = (channel, image split) as in bn2d.h's plane geometry; limit on a plane and LDS layout: bn2d.h.
// 2. The global average pool Y[r] = mean of X[r, 0 .. HW) over the rows r = (n, c), and its backward dX[r, k] = dY[r] / HW.
//    L = the largest power of two <= min(HW, 64) neighbouring lanes own a row: lane l adds elements l, l + L, ... in that order, then
//    the lanes are added as a tree of shuffles with offsets 1, 2, 4, ... (pairs of neighbours first).
// No floating-point atomics, no counters, nothing that waits inside a kernel: eager launches and graph replays give the same bits.
#include "bn2d.h"

namespace clica {
namespace bn2d {

template <int VEC>
__device__ __forceinline__ void lds_store(float* p, const float* v) {
  if (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);      // (i * 4 floats off a 16-byte aligned array)
  } else {
#pragma unroll
    for (int k = 0; k < VEC; ++k) p[k] = v[k];
  }
}

// The window (ho, wo) of plane pl [H][W] in scan order (rows, then columns), the part inside the plane.  XHAT: pl holds xhat and
// y = lrelu(g xhat + b) is formed here.  Returns the maximum and the position 0 .. 8 of its first occurrence (strict >: torch's rule;
// the bits of that first maximum, signed zeros included).
template <bool XHAT>
__device__ __forceinline__ float window_max(const float* pl, int ho, int wo, int H, int W, float g, float b, float slope, int& code) {
  float m = -INFINITY;
  code = 4;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy) {
    const int hh = 2 * ho - 1 + dy;
    const bool vr = hh >= 0 && hh < H;
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int ww = 2 * wo - 1 + dx;
      const bool vc = ww >= 0 && ww < W;
      float v = pl[(vr ? hh : 2 * ho) * W + (vc ? ww : 2 * wo)];      // (the centre is always inside)
      if (XHAT) v = bn::fwd_xhat(v, g, b, slope);
      if (vr && vc && v > m) { m = v; code = dy * 3 + dx; }
    }
  }
  return m;
}

// grid (C, S).  TRAIN: batch statistics from the partials; otherwise the running statistics.  VEC = 4: W % 4 == 0.
template <int LDSF, int VEC, bool AL, bool TRAIN>
__global__ __launch_bounds__(kThreads) void pool_fwd_k(const float* __restrict__ x, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, int64_t N, int C, int H, int W, int64_t per, float Mf,
                                                      float eps, float momentum, float slope, const float* __restrict__ part,
                                                      float* __restrict__ P, float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                                      float* running_mean, float* running_var) {
  __shared__ __attribute__((aligned(16))) float sy[LDSF];
  const int c = (int)blockIdx.x, split = (int)blockIdx.y, S = (int)gridDim.y;
  const int HW = H * W, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, HoWo = Ho * Wo;
  const bn::Norm nm = TRAIN ? bn::finish_train(bn::merge_stats(part, S, C, c), x[(int64_t)c * HW], Mf, eps, momentum, c,
                                               split == 0 && threadIdx.x == 0, save_mean, save_invstd, running_mean, running_var)
                            : bn::finish_eval(running_mean, running_var, c, eps);
  const float g = gamma[c], b = beta[c];
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int U = HW / VEC;
  const int G = LDSF / HW;                                // whole planes per batch
  for (int64_t nb = n0; nb < n1; nb += G) {
    const int cnt = n1 - nb < G ? (int)(n1 - nb) : G;
    const int T = cnt * U;
    Walk wk(nb, U, C, c, HW);
#pragma unroll 4
    for (int i = threadIdx.x; i < T; i += kThreads) {
      float v[VEC];
      load<VEC, AL>(x + wk.next<VEC>(), v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = bn::fwd(v[k], nm, g, b, slope);
      lds_store<VEC>(sy + i * VEC, v);
    }
    __syncthreads();
    const int TO = cnt * HoWo;
    for (int o = threadIdx.x; o < TO; o += kThreads) {
      const int gi = o / HoWo, r = o - gi * HoWo, ho = r / Wo, wo = r - ho * Wo;
      int code;
      const float m = window_max<false>(sy + gi * HW, ho, wo, H, W, g, b, slope, code);
      P[((nb + gi) * C + c) * HoWo + r] = m;
    }
    __syncthreads();
  }
}

// a batch's xhat planes to sl[0 .. cnt HW)
template <int VEC, bool AL>
__device__ __forceinline__ void pool_bwd_stage(float* sl, const float* __restrict__ x, int64_t nb, int cnt, int C, int c, int HW,
                                               const bn::Norm& nm) {
  const int U = HW / VEC, T = cnt * U;
  Walk wk(nb, U, C, c, HW);
#pragma unroll 4
  for (int i = threadIdx.x; i < T; i += kThreads) {
    float v[VEC];
    load<VEC, AL>(x + wk.next<VEC>(), v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) v[k] = bn::xhat(v[k], nm);
    lds_store<VEC>(sl + i * VEC, v);
  }
}

// Every window o of the batch (batch-linear: plane, ho, wo): sd[o] = dP gate(its maximum), and the position 0 .. 8 of its first maximum
// in scan order as nibble o of sc.  A thread takes two neighbouring windows: one byte.
__device__ __forceinline__ void pool_bwd_windows(const float* sl, float* sd, unsigned char* sc, const float* __restrict__ dP, int64_t nb,
                                                 int cnt, int C, int c, int H, int W, int Ho, int Wo, float g, float b, float slope) {
  const int HW = H * W, HoWo = Ho * Wo, TO = cnt * HoWo;
  for (int o2 = threadIdx.x; 2 * o2 < TO; o2 += kThreads) {
    unsigned byte = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int o = 2 * o2 + j;
      if (o < TO) {
        const int gi = o / HoWo, r = o - gi * HoWo, ho = r / Wo, wo = r - ho * Wo;
        const float d = dP[((nb + gi) * C + c) * HoWo + r];
        int code;
        const float m = window_max<true>(sl + gi * HW, ho, wo, H, W, g, b, slope, code);
        sd[o] = bn::bwd_dz(d, m, slope);
        byte |= (unsigned)code << (4 * j);
      }
    }
    sc[o2] = (unsigned char)byte;
  }
}

// dz of pixel (h, w) of the plane whose windows start at `base`: the gated gradients of the <= 4 windows that contain the pixel and
// whose first maximum it is, added in window order (ho, then wo)
__device__ __forceinline__ float pool_dz(const float* sd, const unsigned char* sc, int base, int h, int w, int Ho, int Wo) {
  const int ha = h >> 1, wa = w >> 1, ph = (h & 1) + 1, pw = (w & 1) + 1;            // position (ph, pw) in window (ha, wa)
  const bool hb = (h & 1) && ha + 1 < Ho, wb = (w & 1) && wa + 1 < Wo;                // also row 0 of window ha + 1 / column 0 of wa + 1
  const int h2 = hb ? ha + 1 : ha, w2 = wb ? wa + 1 : wa;
  const int o0 = base + ha * Wo + wa, o1 = base + ha * Wo + w2, o2 = base + h2 * Wo + wa, o3 = base + h2 * Wo + w2;
  const int c0 = (sc[o0 >> 1] >> (4 * (o0 & 1))) & 15, c1 = (sc[o1 >> 1] >> (4 * (o1 & 1))) & 15;
  const int c2 = (sc[o2 >> 1] >> (4 * (o2 & 1))) & 15, c3 = (sc[o3 >> 1] >> (4 * (o3 & 1))) & 15;
  const float d0 = sd[o0], d1 = sd[o1], d2 = sd[o2], d3 = sd[o3];
  float acc = c0 == ph * 3 + pw ? d0 : 0.f;
  acc += wb && c1 == ph * 3 ? d1 : 0.f;
  acc += hb && c2 == pw ? d2 : 0.f;
  acc += hb && wb && c3 == 0 ? d3 : 0.f;
  return acc;
}

// grid (C, S): sum dz and sum dz xhat per (split, channel).  VEC = 4: W % 4 == 0 (a thread's pixel sequence depends on W alone, not on AL).
template <int LDSF, int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void pool_sums_k(const float* __restrict__ x, const float* __restrict__ dP,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ save_mean, const float* __restrict__ save_invstd, int64_t N,
                                                       int C, int H, int W, int64_t per, float slope, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float sl[LDSF];
  __shared__ float sh[kWaves * 2];
  const int c = (int)blockIdx.x, split = (int)blockIdx.y, S = (int)gridDim.y;
  const int HW = H * W, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, HoWo = Ho * Wo;
  const bn::Norm nm{save_mean[c], save_invstd[c]};
  const float g = gamma[c], b = beta[c];
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int G = LDSF / (HW + HoWo + (HoWo + 7) / 8);
  const int U = HW / VEC;
  float s1 = 0.f, s2 = 0.f;
  for (int64_t nb = n0; nb < n1; nb += G) {
    const int cnt = n1 - nb < G ? (int)(n1 - nb) : G;
    float* sd = sl + cnt * HW;
    unsigned char* sc = reinterpret_cast<unsigned char*>(sd + cnt * HoWo);
    pool_bwd_stage<VEC, AL>(sl, x, nb, cnt, C, c, HW, nm);
    __syncthreads();
    pool_bwd_windows(sl, sd, sc, dP, nb, cnt, C, c, H, W, Ho, Wo, g, b, slope);
    __syncthreads();
    const int T = cnt * U;
    for (int i = threadIdx.x; i < T; i += kThreads) {
      const int gi = i / U, rem = (i - gi * U) * VEC, h = rem / W, w = rem - h * W;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        bn::bwd_sums(s1, s2, pool_dz(sd, sc, gi * HoWo, h, w + k, Ho, Wo), sl[i * VEC + k]);
      }
    }
    __syncthreads();
  }
  block_sum2(s1, s2, sh);
  if (threadIdx.x == 0) {
    float* q = part + (size_t)split * C + c;
    q[0] = s1; q[(size_t)S * C] = s2;
  }
}

// grid (C, S).  VEC = 4: W % 4 == 0, so a thread's four pixels lie in one row.
template <int LDSF, int VEC, bool AL>
__global__ __launch_bounds__(kThreads) void pool_bwd_apply_k(const float* __restrict__ x, const float* __restrict__ dP,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* __restrict__ save_mean, const float* __restrict__ save_invstd,
                                                            int64_t N, int C, int H, int W, int64_t per, float Mf, float slope,
                                                            const float* __restrict__ part, float* __restrict__ dx,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
  __shared__ __attribute__((aligned(16))) float sl[LDSF];
  const int c = (int)blockIdx.x, split = (int)blockIdx.y, S = (int)gridDim.y;
  const int HW = H * W, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1, HoWo = Ho * Wo;
  float s1, s2;
  bn::merge_sums(part, S, C, c, s1, s2);
  if (split == 0 && threadIdx.x == 0) {
    dgamma[c] = s2;
    dbeta[c] = s1;
  }
  const bn::Norm nm{save_mean[c], save_invstd[c]};
  const float g = gamma[c], b = beta[c];
  const bn::Bwd bw = bn::bwd_coeffs(g, nm.invstd, s1, s2, Mf);
  const int64_t n0 = (int64_t)split * per;
  const int64_t n1 = n0 + per < N ? n0 + per : N;
  const int G = LDSF / (HW + HoWo + (HoWo + 7) / 8);
  const int U = HW / VEC;
  for (int64_t nb = n0; nb < n1; nb += G) {
    const int cnt = n1 - nb < G ? (int)(n1 - nb) : G;
    float* sd = sl + cnt * HW;
    unsigned char* sc = reinterpret_cast<unsigned char*>(sd + cnt * HoWo);
    pool_bwd_stage<VEC, AL>(sl, x, nb, cnt, C, c, HW, nm);
    __syncthreads();
    pool_bwd_windows(sl, sd, sc, dP, nb, cnt, C, c, H, W, Ho, Wo, g, b, slope);
    __syncthreads();
    const int T = cnt * U;
    for (int i = threadIdx.x; i < T; i += kThreads) {
      const int gi = i / U, rem = (i - gi * U) * VEC, h = rem / W, w = rem - h * W;
      float v[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = bn::bwd_dx(pool_dz(sd, sc, gi * HoWo, h, w + k, Ho, Wo), sl[i * VEC + k], bw);
      store<VEC, AL>(dx + ((nb + gi) * C + c) * HW + rem, v);
    }
    __syncthreads();
  }
}

// f(instance): the LDS size from H and W, quads from W alone (the reduction order); `al` only picks 16-byte accesses
template <int LDSF_, int VEC_, bool AL_>
struct PoolInstance { static constexpr int LDSF = LDSF_, VEC = VEC_; static constexpr bool AL = AL_; };

template <class F>
static void with_pool_instance(int H, int W, bool al, F&& f) {
  const bool quad = W % 4 == 0;
  if (pool_small(H, W)) {
    if (!quad) f(PoolInstance<kPoolLdsSmall, 1, false>{});
    else if (al) f(PoolInstance<kPoolLdsSmall, 4, true>{});
    else f(PoolInstance<kPoolLdsSmall, 4, false>{});
  } else {
    if (!quad) f(PoolInstance<kPoolLdsFloats, 1, false>{});
    else if (al) f(PoolInstance<kPoolLdsFloats, 4, true>{});
    else f(PoolInstance<kPoolLdsFloats, 4, false>{});
  }
}

template <bool TRAIN>
static void launch_pool_fwd(hipStream_t st, const float* x, const float* gamma, const float* beta, int64_t N, int C, int H, int W, float eps,
                            float momentum, float slope, const float* part, float* P, float* save_mean, float* save_invstd, float* rm,
                            float* rv) {
  const Geometry geo = geometry(N, H * W);
  const dim3 grid((unsigned)C, (unsigned)geo.S), block(kThreads);
  const float Mf = (float)(N * (int64_t)H * W);
  with_pool_instance(H, W, W % 4 == 0 && aligned16(x), [&](auto i) {
    hipLaunchKernelGGL((pool_fwd_k<i.LDSF, i.VEC, i.AL, TRAIN>), grid, block, 0, st, x, gamma, beta, N, C, H, W, geo.per, Mf, eps, momentum, slope,
                       part, P, save_mean, save_invstd, rm, rv);
  });
}

}  // namespace bn2d

namespace avgpool {

constexpr int kThreads = 256;
constexpr int kMaxHW = 1 << 14;

static inline int lanes_per_row(int32_t HW) {
  int L = 1;
  while (2 * L <= HW && 2 * L <= 64) L *= 2;
  return L;
}

// grid: ceil(rows L / 256); thread = (row, lane l of the row's L)
__global__ __launch_bounds__(kThreads) void global_fwd_k(const float* __restrict__ x, int64_t rows, int HW, int L, float inv,
                                                        float* __restrict__ y) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t row = t / L;
  const int l = (int)(t - row * L);
  float s = 0.f;
  if (row < rows) {
    const float* p = x + row * HW;
    for (int k = l; k < HW; k += L) s += p[k];
  }
  for (int off = 1; off < L; off <<= 1) s += __shfl_down(s, off, 64);       // (a row's lanes are neighbours in one wave: 64 % L == 0)
  if (row < rows && l == 0) y[row] = s * inv;
}

__global__ __launch_bounds__(kThreads) void global_bwd_k(const float* __restrict__ dy, int64_t rows, int HW, int L, float inv,
                                                        float* __restrict__ dx) {
  const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t row = t / L;
  const int l = (int)(t - row * L);
  if (row >= rows) return;
  const float v = dy[row] * inv;
  float* p = dx + row * HW;
  for (int k = l; k < HW; k += L) p[k] = v;
}

}  // namespace avgpool
}  // namespace clica

using namespace clica;

#define CLICA_POOL_SHAPE(fn, min_M)                                                                                                      \
  CLICA_CHECK_ARG(N >= 1 && N <= INT32_MAX && C >= 1 && C <= bn2d::kMaxC && H >= 1 && W >= 1 && (double)N * H * W >= (min_M) &&          \
                      (double)N * (double)H * (double)W * (double)C < 1e18,                                                              \
                  fn ": N=%lld C=%d H=%d W=%d (N >= 1, 1 <= C <= %d, H, W >= 1, N H W >= %d)", (long long)N, C, H, W, bn2d::kMaxC,       \
                  (min_M));                                                                                                              \
  CLICA_CHECK_ARG(bn2d::pool_fits(H, W), fn ": plane H=%d W=%d over the limit H W + Ho Wo + ceil(Ho Wo / 8) <= %d floats of LDS (112 x 112 fits)", H, W,   \
                  bn2d::kPoolLdsFloats)

#define CLICA_POOL_SLOPE(fn) \
  CLICA_CHECK_ARG(slope >= 0.f && slope <= 1.f, fn ": slope=%g must be in [0, 1] (the pool's argmax is taken after the activation)", slope)

#define CLICA_POOL_WORKSPACE(fn) \
  CLICA_BN_WORKSPACE(fn, bn2d::workspace_bytes(N, C, H * W), "clica_bn2d_maxpool_workspace_bytes", CLICA_E_WORKSPACE)

extern "C" int clica_bn2d_maxpool_workspace_bytes(int64_t N, int32_t C, int32_t H, int32_t W, size_t* bytes) {
  CLICA_CHECK_ARG(bytes != nullptr, "clica_bn2d_maxpool_workspace_bytes: bytes is NULL");
  CLICA_POOL_SHAPE("clica_bn2d_maxpool_workspace_bytes", 2);
  *bytes = bn2d::workspace_bytes(N, C, H * W);
  return CLICA_OK;
}

extern "C" int clica_bn2d_act_maxpool_fwd_train(const float* X, const float* gamma, const float* beta, int64_t N, int32_t C, int32_t H,
                                                int32_t W, float eps, float momentum, float slope, float* P, float* save_mean,
                                                float* save_invstd, float* running_mean, float* running_var, void* workspace,
                                                size_t workspace_bytes, clica_stream_t stream) {
  CLICA_POOL_SHAPE("clica_bn2d_act_maxpool_fwd_train", 2);
  CLICA_POOL_SLOPE("clica_bn2d_act_maxpool_fwd_train");
  CLICA_CHECK_ARG(X && gamma && beta && P && save_mean && save_invstd && workspace, "clica_bn2d_act_maxpool_fwd_train: NULL pointer");
  CLICA_POOL_WORKSPACE("clica_bn2d_act_maxpool_fwd_train");
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  bn2d::launch_stats(st, X, N, C, H * W, part);
  bn2d::launch_pool_fwd<true>(st, X, gamma, beta, N, (int)C, (int)H, (int)W, eps, momentum, slope, part, P, save_mean, save_invstd,
                              running_mean, running_var);
  return launch_status("clica_bn2d_act_maxpool_fwd_train");
}

extern "C" int clica_bn2d_act_maxpool_fwd_eval(const float* X, const float* gamma, const float* beta, const float* running_mean,
                                               const float* running_var, int64_t N, int32_t C, int32_t H, int32_t W, float eps, float slope,
                                               float* P, clica_stream_t stream) {
  CLICA_POOL_SHAPE("clica_bn2d_act_maxpool_fwd_eval", 1);
  CLICA_POOL_SLOPE("clica_bn2d_act_maxpool_fwd_eval");
  CLICA_CHECK_ARG(X && gamma && beta && running_mean && running_var && P, "clica_bn2d_act_maxpool_fwd_eval: NULL pointer");
  // (the inference instance only reads the running statistics)
  bn2d::launch_pool_fwd<false>(as_stream(stream), X, gamma, beta, N, (int)C, (int)H, (int)W, eps, 0.f, slope, nullptr, P, nullptr, nullptr,
                               const_cast<float*>(running_mean), const_cast<float*>(running_var));
  return launch_status("clica_bn2d_act_maxpool_fwd_eval");
}

extern "C" int clica_bn2d_act_maxpool_bwd(const float* X, const float* dP, const float* gamma, const float* beta, const float* save_mean,
                                          const float* save_invstd, int64_t N, int32_t C, int32_t H, int32_t W, float slope, float* dX,
                                          float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  CLICA_POOL_SHAPE("clica_bn2d_act_maxpool_bwd", 2);
  CLICA_POOL_SLOPE("clica_bn2d_act_maxpool_bwd");
  CLICA_CHECK_ARG(X && dP && gamma && beta && save_mean && save_invstd && dX && dgamma && dbeta && workspace,
                  "clica_bn2d_act_maxpool_bwd: NULL pointer");
  CLICA_POOL_WORKSPACE("clica_bn2d_act_maxpool_bwd");
  const bn2d::Geometry geo = bn2d::geometry(N, H * W);
  const dim3 grid((unsigned)C, (unsigned)geo.S), block(bn2d::kThreads);
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const float Mf = (float)(N * (int64_t)H * W);
  bn2d::with_pool_instance(H, W, W % 4 == 0 && bn2d::aligned16(X) && bn2d::aligned16(dX), [&](auto i) {
    hipLaunchKernelGGL((bn2d::pool_sums_k<i.LDSF, i.VEC, i.AL>), grid, block, 0, st, X, dP, gamma, beta, save_mean, save_invstd, N, (int)C, (int)H,
                       (int)W, geo.per, slope, part);
    hipLaunchKernelGGL((bn2d::pool_bwd_apply_k<i.LDSF, i.VEC, i.AL>), grid, block, 0, st, X, dP, gamma, beta, save_mean, save_invstd, N, (int)C,
                       (int)H, (int)W, geo.per, Mf, slope, part, dX, dgamma, dbeta);
  });
  return launch_status("clica_bn2d_act_maxpool_bwd");
}

#define CLICA_AVGPOOL_SHAPE(fn)                                                                                                     \
  CLICA_CHECK_ARG(rows >= 1 && HW >= 1 && HW <= avgpool::kMaxHW && rows <= ((int64_t)1 << 31),                                       \
                  fn ": rows=%lld HW=%d (1 <= rows = N C <= 2^31, 1 <= HW <= %d)", (long long)rows, HW, avgpool::kMaxHW)

extern "C" int clica_avgpool2d_global_fwd(const float* X, int64_t rows, int32_t HW, float* Y, clica_stream_t stream) {
  CLICA_AVGPOOL_SHAPE("clica_avgpool2d_global_fwd");
  CLICA_CHECK_ARG(X && Y, "clica_avgpool2d_global_fwd: NULL pointer");
  const int L = avgpool::lanes_per_row(HW);
  const dim3 grid((unsigned)ceil_div(rows * L, avgpool::kThreads)), block(avgpool::kThreads);
  hipLaunchKernelGGL(avgpool::global_fwd_k, grid, block, 0, as_stream(stream), X, rows, (int)HW, L, 1.f / (float)HW, Y);
  return launch_status("clica_avgpool2d_global_fwd");
}

extern "C" int clica_avgpool2d_global_bwd(const float* dY, int64_t rows, int32_t HW, float* dX, clica_stream_t stream) {
  CLICA_AVGPOOL_SHAPE("clica_avgpool2d_global_bwd");
  CLICA_CHECK_ARG(dY && dX, "clica_avgpool2d_global_bwd: NULL pointer");
  const int L = avgpool::lanes_per_row(HW);
  const dim3 grid((unsigned)ceil_div(rows * L, avgpool::kThreads)), block(avgpool::kThreads);
  hipLaunchKernelGGL(avgpool::global_bwd_k, grid, block, 0, as_stream(stream), dY, rows, (int)HW, L, 1.f / (float)HW, dX);
  return launch_status("clica_avgpool2d_global_bwd");
}
