// SGD over one flat parameter arena: torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov, maximize), the optimizer the
// reference's 3DIdent driver builds for `--optimizer sgd` (main_3dident.py:453-454, 582-583).  With t = *step_dev before the update:
//   gr = g s (negated for maximize) ; gr += wd p (wd != 0)
//   momentum != 0:  buf = gr (t == 0) | momentum buf + (1 - dampening) gr ;  d = gr + momentum buf (nesterov) | buf
//   momentum == 0:  d = gr
//   p -= lr d
// HBM-bound: 8 B read + 4 B written per parameter plain, 12 B + 8 B with a momentum buffer; one launch for all layers.
#include "common.h"

namespace clica {
namespace sgd {
constexpr int THREADS = 256;

struct Opts { float lr, momentum, one_minus_dampening, weight_decay, gscale; int nesterov, maximize; };

// Every operation one correctly rounded fp32 multiply, add or subtract, NO fused multiply-add: a NumPy fp32 restatement of this
// sequence (include/clica.h) is the kernel's exact expectation.  __fmul_rn / __fadd_rn are plain `*` / `+` to this compiler, which
// -ffp-contract=fast lets the backend fuse whatever the source says: the Makefile builds THIS unit with -ffp-contract=off.
// `first` = this is update number 0: the buffer takes the gradient as it is.
template <bool MOM>
__device__ __forceinline__ void update(float& p, float g, float& buf, const Opts& o, bool first) {
  float gr = g * o.gscale;
  if (o.maximize) gr = -gr;
  if (o.weight_decay != 0.f) { const float wp = o.weight_decay * p; gr = gr + wp; }
  float d = gr;
  if (MOM) {
    if (first) {
      buf = gr;
    } else {
      const float a = o.momentum * buf, b = o.one_minus_dampening * gr;
      buf = a + b;
    }
    if (o.nesterov) { const float c = o.momentum * buf; d = gr + c; } else { d = buf; }
  }
  const float u = o.lr * d;
  p = p - u;
}

template <bool MOM>
__global__ __launch_bounds__(THREADS) void sgd_k(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ b, int64_t count,
                                                Opts o, int32_t* __restrict__ step_dev, int32_t* __restrict__ ticket) {
  __shared__ int s_t;
  if (threadIdx.x == 0) s_t = step_dev[0];
  __syncthreads();
  const bool first = s_t == 0;
  const int64_t n4 = count / 4;
  const int64_t stride = (int64_t)gridDim.x * THREADS;
  float4* p4 = reinterpret_cast<float4*>(p); const float4* g4 = reinterpret_cast<const float4*>(g);
  float4* b4 = reinterpret_cast<float4*>(b);
  for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n4; i += stride) {
    float4 pp = p4[i], gg = g4[i], bb = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MOM && !first) bb = b4[i];
    float* pa = &pp.x; float* ga = &gg.x; float* ba = &bb.x;
#pragma unroll
    for (int u = 0; u < 4; ++u) update<MOM>(pa[u], ga[u], ba[u], o, first);
    p4[i] = pp;
    if (MOM) b4[i] = bb;
  }
  for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * THREADS + threadIdx.x; i < count; i += stride) {
    float pn = p[i], bn = 0.f;
    if (MOM && !first) bn = b[i];
    update<MOM>(pn, g[i], bn, o, first);
    if (MOM) b[i] = bn;
    p[i] = pn;
  }
  // optional fused tick, as adam_k's: every workgroup read *step_dev on entry, so the LAST one to arrive may advance it (relaxed arrival
  // counter, no fence: nothing but that read has to be ordered)
  if (ticket) {
    __syncthreads();
    if (threadIdx.x == 0) {
      if (__hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
        step_dev[0] += 1;
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}
}  // namespace sgd
}  // namespace clica

using namespace clica;

static int sgd_launch(float* param, const float* grad, float* momentum_buf, int64_t count, float lr, float momentum, float dampening,
                      float weight_decay, int32_t nesterov, int32_t maximize, float grad_scale, int32_t* step_dev, int32_t* ticket,
                      clica_stream_t stream) {
  CLICA_CHECK_ARG(param && grad && step_dev && count > 0, "clica_sgd_step: bad argument");
  CLICA_CHECK_ARG(momentum == 0.f || momentum_buf, "clica_sgd_step: momentum != 0 needs a momentum buffer");
  CLICA_CHECK_ARG(!nesterov || (momentum != 0.f && dampening == 0.f), "clica_sgd_step: nesterov needs a momentum and zero dampening");
  CLICA_CHECK_ARG(((uintptr_t)param % 16 == 0) && ((uintptr_t)grad % 16 == 0) && ((uintptr_t)momentum_buf % 16 == 0),
                  "clica_sgd_step: arenas must be 16-byte aligned");
  int64_t blocks = ceil_div(ceil_div(count, 4), sgd::THREADS);
  if (blocks > kNumCU * 8) blocks = kNumCU * 8;
  // fused tick: one workgroup per CU, as adam_launch (the arrivals on the ticket word serialise)
  if (ticket && blocks > kNumCU) blocks = kNumCU;
  if (blocks < 1) blocks = 1;
  sgd::Opts o;
  o.lr = lr; o.momentum = momentum; o.one_minus_dampening = 1.f - dampening;      // formed in fp32 from the fp32 argument
  o.weight_decay = weight_decay; o.gscale = grad_scale; o.nesterov = nesterov ? 1 : 0; o.maximize = maximize ? 1 : 0;
  if (momentum != 0.f)
    hipLaunchKernelGGL(sgd::sgd_k<true>, dim3((unsigned)blocks), dim3(sgd::THREADS), 0, as_stream(stream), param, grad, momentum_buf, count, o,
                       step_dev, ticket);
  else
    hipLaunchKernelGGL(sgd::sgd_k<false>, dim3((unsigned)blocks), dim3(sgd::THREADS), 0, as_stream(stream), param, grad, (float*)nullptr, count, o,
                       step_dev, ticket);
  return launch_status("clica_sgd_step");
}

extern "C" int clica_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t count, float lr, float momentum, float dampening,
                              float weight_decay, int32_t nesterov, int32_t maximize, float grad_scale, const int32_t* step_dev,
                              clica_stream_t stream) {
  return sgd_launch(param, grad, momentum_buf, count, lr, momentum, dampening, weight_decay, nesterov, maximize, grad_scale,
                    const_cast<int32_t*>(step_dev), nullptr, stream);
}

extern "C" int clica_sgd_step_tick(float* param, const float* grad, float* momentum_buf, int64_t count, float lr, float momentum, float dampening,
                                   float weight_decay, int32_t nesterov, int32_t maximize, float grad_scale, int32_t* step_dev, int32_t* ticket,
                                   clica_stream_t stream) {
  CLICA_CHECK_ARG(ticket != nullptr, "clica_sgd_step_tick: ticket is NULL");
  return sgd_launch(param, grad, momentum_buf, count, lr, momentum, dampening, weight_decay, nesterov, maximize, grad_scale, step_dev, ticket,
                    stream);
}
