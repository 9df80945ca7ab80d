// Image batches from a uint8 table resident in HBM  --  the image half of ThreeDIdentDataset / SequentialThreeDIdentDataset
// (reference datasets/threedident_dataset.py:120-127, 184-190) with the transform of main_3dident.py:787-796: pil_loader's RGB array
// [H][W][C] uint8 -> torchvision ToTensor (CHW, float(v) / 255) -> Normalize ((x - mean[c]) / std[c]).  The reference decodes two PNGs per
// item on DataLoader workers and copies the collated batch to the GPU every step; here every decoded image lives in HBM once
// (N x H x W x C bytes: 250 000 x 224 x 224 x 3 = 37.6 GB) and ONE launch writes the normalised float32 batch [n_index][C][H][W] for a list
// of row indices (both views of a pair batch: the 2 B concatenated indices).  Write-dominated: C bytes read, 4 C bytes written per pixel
// (2 x 1024 images of 224 x 224 x 3: 308 MB read, 1.23 GB written).
// The three operations stay three correctly rounded fp32 operations (two true divisions, one subtraction: nothing to contract, no
// reciprocal), so the batch is defined bit for bit by the transform's definition.
// clica_image_channel_stats is the data pass of tools/3dident/get_mean_std.py: exact integer sums of v and v^2 per image and channel,
// one workgroup per image, combined in a fixed order (no atomics); the fp64 finish is host code (datasets/image_table.py).
// clica_image_gather_norm_ex writes the same values in the layout and element type the backbone takes (NCHW | NHWC, fp32 | bf16): the
// value is the fp32 one above, a bf16 output is that value narrowed once at the store (bn2d.h's bf16_rne).  A channels-last image is the
// table row's own byte order: one 32-bit load, four conversions, one 16-byte (bf16: 8-byte) store per thread.
#include "common.h"
#include "bn2d.h"      // bf16_t, bf16_rne, from_f32: the repository's one fp32 -> bf16 rounding rule

namespace clica {
namespace imgtab {
constexpr int THREADS = 256;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
using bn2d::bf16_t;
using bn2d::bf16_rne;
using bn2d::from_f32;

// four consecutive outputs as ONE store: 16 bytes of fp32, 8 bytes of bf16 (dst aligned to that)
template <bool NT>
__device__ __forceinline__ void store4(float* dst, const float* v) {
  const f32x4 o = {v[0], v[1], v[2], v[3]};
  if (NT) __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(dst));
  else *reinterpret_cast<f32x4*>(dst) = o;
}
template <bool NT>
__device__ __forceinline__ void store4(bf16_t* dst, const float* v) {
  const u32x2 o = {(uint32_t)bf16_rne(v[0]) | (uint32_t)bf16_rne(v[1]) << 16, (uint32_t)bf16_rne(v[2]) | (uint32_t)bf16_rne(v[3]) << 16};
  if (NT) __builtin_nontemporal_store(o, reinterpret_cast<u32x2*>(dst));
  else *reinterpret_cast<u32x2*>(dst) = o;
}

struct Norm { float mean[4], std[4]; };      // by value: the kernels read it through scalar loads

template <bool NORM>
__device__ __forceinline__ float to_float(uint32_t v, float mean, float std) {
  const float x = (float)v / 255.0f;                          // ToTensor
  return NORM ? (x - mean) / std : x;                         // Normalize
}

// Work decomposition shared by both gather kernels.  A "unit" is what one thread handles (4 pixels on the fast path, 1 on the scalar
// path); an image has `units` of them.  One block iteration ("item") covers upb = min(units, THREADS) units of each of ipb = THREADS / upb
// images (ipb = 1 once an image has THREADS units or more, which then takes cpi = ceil(units / THREADS) items):
//   img = (item / cpi) * ipb + tid / upb,   unit = (item % cpi) * upb + tid % upb
struct Split { int64_t units, cpi, items; uint32_t upb, ipb; };

static Split make_split(int64_t units, int64_t n_index) {
  Split s;
  s.units = units;
  s.upb = (uint32_t)(units < THREADS ? units : THREADS);
  s.ipb = THREADS / s.upb;
  s.cpi = ceil_div(units, (int64_t)s.upb);
  s.items = ceil_div(n_index, (int64_t)s.ipb) * s.cpi;
  return s;
}

__device__ __forceinline__ int64_t clamp_row(int64_t r, int64_t n_images) {
  return r < 0 ? 0 : (r >= n_images ? n_images - 1 : r);     // (a bad index reads a valid row: never out of bounds)
}

// C == 3, H W % 4 == 0: every image base is 4-byte aligned; a thread takes 4 pixels = 12 bytes R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3 with
// three 32-bit loads and writes one 16-byte store (bf16: 8-byte) into each channel plane.
template <bool NORM, bool NT, typename T = float>
__global__ __launch_bounds__(THREADS) void gather_rgb_k(const uint8_t* __restrict__ table, int64_t n_images, int64_t hw,
                                                        const int64_t* __restrict__ index, int64_t n_index, Split s, Norm nm,
                                                        T* __restrict__ out) {
  const uint32_t sub = threadIdx.x / s.upb, lu = threadIdx.x - sub * s.upb;
  for (int64_t item = blockIdx.x; item < s.items; item += gridDim.x) {
    const int64_t g = item / s.cpi;
    const int64_t img = g * s.ipb + sub, q = (item - g * s.cpi) * s.upb + lu;
    if (sub >= s.ipb || img >= n_index || q >= s.units) continue;
    const int64_t row = clamp_row(index[img], n_images);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(table + row * hw * 3 + 12 * q);
    const uint32_t w0 = src[0], w1 = src[1], w2 = src[2];
    const uint32_t r[4] = {w0 & 255u, w0 >> 24, (w1 >> 16) & 255u, (w2 >> 8) & 255u};
    const uint32_t g4[4] = {(w0 >> 8) & 255u, w1 & 255u, w1 >> 24, (w2 >> 16) & 255u};
    const uint32_t b[4] = {(w0 >> 16) & 255u, (w1 >> 8) & 255u, w2 & 255u, w2 >> 24};
    float o0[4], o1[4], o2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      o0[e] = to_float<NORM>(r[e], nm.mean[0], nm.std[0]);
      o1[e] = to_float<NORM>(g4[e], nm.mean[1], nm.std[1]);
      o2[e] = to_float<NORM>(b[e], nm.mean[2], nm.std[2]);
    }
    T* dst = out + img * 3 * hw + 4 * q;
    store4<NT>(dst, o0);
    store4<NT>(dst + hw, o1);
    store4<NT>(dst + 2 * hw, o2);
  }
}

// Every other shape: one pixel per thread, C byte loads, C 4-byte (bf16: 2-byte) stores (coalesced within each plane).
template <int C, bool NORM, typename T = float>
__global__ __launch_bounds__(THREADS) void gather_any_k(const uint8_t* __restrict__ table, int64_t n_images, int64_t hw,
                                                        const int64_t* __restrict__ index, int64_t n_index, Split s, Norm nm,
                                                        T* __restrict__ out) {
  const uint32_t sub = threadIdx.x / s.upb, lu = threadIdx.x - sub * s.upb;
  for (int64_t item = blockIdx.x; item < s.items; item += gridDim.x) {
    const int64_t g = item / s.cpi;
    const int64_t img = g * s.ipb + sub, p = (item - g * s.cpi) * s.upb + lu;
    if (sub >= s.ipb || img >= n_index || p >= s.units) continue;
    const int64_t row = clamp_row(index[img], n_images);
    const uint8_t* src = table + (row * hw + p) * C;
    T* dst = out + img * C * hw + p;
#pragma unroll
    for (int c = 0; c < C; ++c) from_f32(dst + c * hw, to_float<NORM>(src[c], nm.mean[c], nm.std[c]));
  }
}

// Channels-last output [n_index][H][W][C]: image `img` of the batch is row index[img] of the table, element for element
// (elems = H W C of them); the channel of element e is e % C.  A unit is 4 consecutive elements (VEC: elems % 4 == 0, so every image
// base is 4-byte aligned in the table and 4-element aligned in `out`: one 32-bit load, one store4) or one element.
template <int C>
__device__ __forceinline__ float pick(const float* a, uint32_t c) {
  float r = a[0];
#pragma unroll
  for (int k = 1; k < C; ++k) r = c == (uint32_t)k ? a[k] : r;
  return r;
}

template <int C, typename T, bool VEC, bool NORM, bool NT>
__global__ __launch_bounds__(THREADS) void gather_nhwc_k(const uint8_t* __restrict__ table, int64_t n_images, int64_t elems,
                                                         const int64_t* __restrict__ index, int64_t n_index, Split s, Norm nm,
                                                         T* __restrict__ out) {
  const uint32_t sub = threadIdx.x / s.upb, lu = threadIdx.x - sub * s.upb;
  for (int64_t item = blockIdx.x; item < s.items; item += gridDim.x) {
    const int64_t g = item / s.cpi;
    const int64_t img = g * s.ipb + sub, u = (item - g * s.cpi) * s.upb + lu;
    if (sub >= s.ipb || img >= n_index || u >= s.units) continue;
    const int64_t row = clamp_row(index[img], n_images);
    if (VEC) {
      const uint32_t w = *reinterpret_cast<const uint32_t*>(table + row * elems + 4 * u);
      uint32_t c = (uint32_t)((4 * u) % C);
      float v[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        v[k] = to_float<NORM>((w >> (8 * k)) & 255u, pick<C>(nm.mean, c), pick<C>(nm.std, c));
        c = c + 1 == (uint32_t)C ? 0u : c + 1;
      }
      store4<NT>(out + img * elems + 4 * u, v);
    } else {
      const uint32_t c = (uint32_t)(u % C);
      from_f32(out + img * elems + u, to_float<NORM>(table[row * elems + u], pick<C>(nm.mean, c), pick<C>(nm.std, c)));
    }
  }
}

// ---- channel statistics: one workgroup per image, thread-local integer sums, waves by shuffle, the four waves through LDS in order
template <int C>
__global__ __launch_bounds__(THREADS) void channel_stats_k(const uint8_t* __restrict__ table, int64_t hw, int quad_path,
                                                           unsigned long long* __restrict__ sums) {
  const uint8_t* img = table + (int64_t)blockIdx.x * hw * C;
  unsigned long long s1[C], s2[C];
#pragma unroll
  for (int c = 0; c < C; ++c) s1[c] = s2[c] = 0;
  if (C == 3 && quad_path) {      // H W % 4 == 0: the image base is 4-byte aligned, 4 pixels per three 32-bit loads
    for (int64_t q = threadIdx.x; q < hw / 4; q += THREADS) {
      const uint32_t* src = reinterpret_cast<const uint32_t*>(img + 12 * q);
      const uint32_t w[3] = {src[0], src[1], src[2]};
      uint32_t a1[3] = {0, 0, 0}, a2[3] = {0, 0, 0};          // 4 bytes per channel: at most 4 x 65025
#pragma unroll
      for (int k = 0; k < 12; ++k) {
        const uint32_t v = (w[k / 4] >> (8 * (k % 4))) & 255u;
        a1[k % 3] += v; a2[k % 3] += v * v;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) { s1[c % C] += a1[c]; s2[c % C] += a2[c]; }
    }
  } else {
    for (int64_t p = threadIdx.x; p < hw; p += THREADS) {
#pragma unroll
      for (int c = 0; c < C; ++c) { const uint32_t v = img[p * C + c]; s1[c] += v; s2[c] += v * v; }
    }
  }
  __shared__ unsigned long long part[THREADS / 64][2 * C];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { s1[c] += __shfl_down(s1[c], off, 64); s2[c] += __shfl_down(s2[c], off, 64); }
    if (lane == 0) { part[wave][2 * c] = s1[c]; part[wave][2 * c + 1] = s2[c]; }
  }
  __syncthreads();
  if (threadIdx.x < 2 * C) {
    unsigned long long t = 0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) t += part[w][threadIdx.x];
    sums[(int64_t)blockIdx.x * 2 * C + threadIdx.x] = t;
  }
}

// The RGB path writes its planes with non-temporal stores: measured 1 - 4 % (224 x 224) and 1 - 7 % (64 x 64) faster than plain stores at
// 2 x 1024 images on two boxes, same bits.  clica_set_tuning("image_nt_stores", 0): plain stores (A/B hook).
static bool g_nt_stores = true;
void set_nt_stores(int on) { g_nt_stores = on != 0; }

template <int C, typename T>
static void launch_any(bool norm, unsigned blocks, hipStream_t st, const uint8_t* table, int64_t n_images, int64_t hw, const int64_t* index,
                       int64_t n_index, const Split& s, const Norm& nm, T* out) {
  if (norm) hipLaunchKernelGGL((gather_any_k<C, true, T>), dim3(blocks), dim3(THREADS), 0, st, table, n_images, hw, index, n_index, s, nm, out);
  else hipLaunchKernelGGL((gather_any_k<C, false, T>), dim3(blocks), dim3(THREADS), 0, st, table, n_images, hw, index, n_index, s, nm, out);
}

// The NCHW batch: `fast` (decided by the caller from C, H W and the pointers' alignment) is the RGB quad path, else a pixel per thread.
template <typename T>
static void launch_nchw(bool fast, bool norm, hipStream_t st, const uint8_t* table, int64_t n_images, int64_t hw, int32_t C,
                        const int64_t* index, int64_t n_index, const Norm& nm, T* out) {
  const Split s = make_split(fast ? hw / 4 : hw, n_index);
  const unsigned blocks = (unsigned)(s.items < 8 * kNumCU ? s.items : 8 * kNumCU);
  if (fast) {
    const bool nt = g_nt_stores;
#define CLICA_IMG_RGB(NORM, NT) \
  hipLaunchKernelGGL((gather_rgb_k<NORM, NT, T>), dim3(blocks), dim3(THREADS), 0, st, table, n_images, hw, index, n_index, s, nm, out)
    if (norm) { if (nt) CLICA_IMG_RGB(true, true); else CLICA_IMG_RGB(true, false); }
    else { if (nt) CLICA_IMG_RGB(false, true); else CLICA_IMG_RGB(false, false); }
#undef CLICA_IMG_RGB
  } else if (C == 1) launch_any<1, T>(norm, blocks, st, table, n_images, hw, index, n_index, s, nm, out);
  else if (C == 2) launch_any<2, T>(norm, blocks, st, table, n_images, hw, index, n_index, s, nm, out);
  else if (C == 3) launch_any<3, T>(norm, blocks, st, table, n_images, hw, index, n_index, s, nm, out);
  else launch_any<4, T>(norm, blocks, st, table, n_images, hw, index, n_index, s, nm, out);
}

// The NHWC batch: `vec` (elems % 4 == 0, table 4-byte and out 4-element aligned) is the 4-elements-per-thread path.
template <int C, typename T>
static void launch_nhwc_c(bool vec, bool norm, hipStream_t st, const uint8_t* table, int64_t n_images, int64_t elems, const int64_t* index,
                          int64_t n_index, const Norm& nm, T* out) {
  const Split s = make_split(vec ? elems / 4 : elems, n_index);
  const unsigned blocks = (unsigned)(s.items < 8 * kNumCU ? s.items : 8 * kNumCU);
#define CLICA_IMG_NHWC(VEC, NORM, NT) \
  hipLaunchKernelGGL((gather_nhwc_k<C, T, VEC, NORM, NT>), dim3(blocks), dim3(THREADS), 0, st, table, n_images, elems, index, n_index, s, nm, out)
  if (vec) {
    const bool nt = g_nt_stores;
    if (norm) { if (nt) CLICA_IMG_NHWC(true, true, true); else CLICA_IMG_NHWC(true, true, false); }
    else { if (nt) CLICA_IMG_NHWC(true, false, true); else CLICA_IMG_NHWC(true, false, false); }
  } else {
    if (norm) CLICA_IMG_NHWC(false, true, false); else CLICA_IMG_NHWC(false, false, false);
  }
#undef CLICA_IMG_NHWC
}

template <typename T>
static void launch_nhwc(bool vec, bool norm, hipStream_t st, const uint8_t* table, int64_t n_images, int64_t elems, int32_t C,
                        const int64_t* index, int64_t n_index, const Norm& nm, T* out) {
  if (C == 1) launch_nhwc_c<1, T>(vec, norm, st, table, n_images, elems, index, n_index, nm, out);
  else if (C == 2) launch_nhwc_c<2, T>(vec, norm, st, table, n_images, elems, index, n_index, nm, out);
  else if (C == 3) launch_nhwc_c<3, T>(vec, norm, st, table, n_images, elems, index, n_index, nm, out);
  else launch_nhwc_c<4, T>(vec, norm, st, table, n_images, elems, index, n_index, nm, out);
}
}  // namespace imgtab
}  // namespace clica

using namespace clica;

extern "C" int clica_image_gather_norm(const uint8_t* table, int64_t n_images, int32_t H, int32_t W, int32_t C, const int64_t* index,
                                       int64_t n_index, const float* mean, const float* std, float* out, clica_stream_t stream) {
  CLICA_CHECK_ARG(table && index && out && n_images > 0 && n_index > 0, "clica_image_gather_norm: NULL pointer / empty table or batch");
  CLICA_CHECK_ARG(H > 0 && W > 0, "clica_image_gather_norm: image size %d x %d", (int)H, (int)W);
  CLICA_CHECK_ARG(C >= 1 && C <= 4, "clica_image_gather_norm: C=%d channels (1..4 supported)", (int)C);
  CLICA_CHECK_ARG((mean == nullptr) == (std == nullptr), "clica_image_gather_norm: mean and std must be given together");
  const int64_t hw = (int64_t)H * W;
  const bool fast = C == 3 && hw % 4 == 0;
  CLICA_CHECK_ARG((reinterpret_cast<uintptr_t>(out) & (fast ? 15 : 3)) == 0 && (!fast || (reinterpret_cast<uintptr_t>(table) & 3) == 0),
                  "clica_image_gather_norm: out must be %d-byte aligned%s", fast ? 16 : 4, fast ? ", table 4-byte" : "");
  imgtab::Norm nm;
  for (int c = 0; c < 4; ++c) { nm.mean[c] = mean && c < C ? mean[c] : 0.f; nm.std[c] = std && c < C ? std[c] : 1.f; }
  imgtab::launch_nchw<float>(fast, mean != nullptr, as_stream(stream), table, n_images, hw, C, index, n_index, nm, out);
  return launch_status("clica_image_gather_norm");
}

extern "C" int clica_image_gather_norm_ex(const uint8_t* table, int64_t n_images, int32_t H, int32_t W, int32_t C, const int64_t* index,
                                          int64_t n_index, const float* mean, const float* std, void* out, int32_t layout, int32_t dtype,
                                          clica_stream_t stream) {
  CLICA_CHECK_ARG(table && index && out && n_images > 0 && n_index > 0, "clica_image_gather_norm_ex: NULL pointer / empty table or batch");
  CLICA_CHECK_ARG(H > 0 && W > 0, "clica_image_gather_norm_ex: image size %d x %d", (int)H, (int)W);
  CLICA_CHECK_ARG(C >= 1 && C <= 4, "clica_image_gather_norm_ex: C=%d channels (1..4 supported)", (int)C);
  CLICA_CHECK_ARG((mean == nullptr) == (std == nullptr), "clica_image_gather_norm_ex: mean and std must be given together");
  CLICA_CHECK_ARG(layout == CLICA_IMAGE_NCHW || layout == CLICA_IMAGE_NHWC, "clica_image_gather_norm_ex: layout %d (0: NCHW, 1: NHWC)", (int)layout);
  CLICA_CHECK_ARG(dtype == CLICA_IMAGE_F32 || dtype == CLICA_IMAGE_BF16, "clica_image_gather_norm_ex: dtype %d (0: fp32, 1: bf16)", (int)dtype);
  const uintptr_t esize = dtype == CLICA_IMAGE_BF16 ? 2 : 4, po = reinterpret_cast<uintptr_t>(out), pt = reinterpret_cast<uintptr_t>(table);
  CLICA_CHECK_ARG((po & (esize - 1)) == 0, "clica_image_gather_norm_ex: out must be %d-byte aligned", (int)esize);
  const int64_t hw = (int64_t)H * W, elems = hw * C;
  imgtab::Norm nm;
  for (int c = 0; c < 4; ++c) { nm.mean[c] = mean && c < C ? mean[c] : 0.f; nm.std[c] = std && c < C ? std[c] : 1.f; }
  const bool norm = mean != nullptr;
  // the wide path of either layout is taken only where the sizes AND both pointers allow it; everything else is the scalar path
  const bool wide_ptrs = (pt & 3) == 0 && (po & (4 * esize - 1)) == 0;
  hipStream_t st = as_stream(stream);
  if (layout == CLICA_IMAGE_NCHW) {
    const bool fast = C == 3 && hw % 4 == 0 && wide_ptrs;
    if (dtype == CLICA_IMAGE_F32) imgtab::launch_nchw<float>(fast, norm, st, table, n_images, hw, C, index, n_index, nm, static_cast<float*>(out));
    else imgtab::launch_nchw<imgtab::bf16_t>(fast, norm, st, table, n_images, hw, C, index, n_index, nm, static_cast<imgtab::bf16_t*>(out));
  } else {
    const bool vec = elems % 4 == 0 && wide_ptrs;
    if (dtype == CLICA_IMAGE_F32) imgtab::launch_nhwc<float>(vec, norm, st, table, n_images, elems, C, index, n_index, nm, static_cast<float*>(out));
    else imgtab::launch_nhwc<imgtab::bf16_t>(vec, norm, st, table, n_images, elems, C, index, n_index, nm, static_cast<imgtab::bf16_t*>(out));
  }
  return launch_status("clica_image_gather_norm_ex");
}

extern "C" int clica_image_channel_stats(const uint8_t* table, int64_t n_images, int32_t H, int32_t W, int32_t C, uint64_t* sums,
                                         clica_stream_t stream) {
  CLICA_CHECK_ARG(table && sums && n_images > 0, "clica_image_channel_stats: NULL pointer / empty table");
  CLICA_CHECK_ARG(n_images <= 0x7fffffffLL, "clica_image_channel_stats: %lld images (one workgroup each: at most 2^31 - 1)", (long long)n_images);
  CLICA_CHECK_ARG(H > 0 && W > 0, "clica_image_channel_stats: image size %d x %d", (int)H, (int)W);
  CLICA_CHECK_ARG(C >= 1 && C <= 4, "clica_image_channel_stats: C=%d channels (1..4 supported)", (int)C);
  CLICA_CHECK_ARG((reinterpret_cast<uintptr_t>(sums) & 7) == 0, "clica_image_channel_stats: sums must be 8-byte aligned");
  const int64_t hw = (int64_t)H * W;
  const int quad = C == 3 && hw % 4 == 0 && (reinterpret_cast<uintptr_t>(table) & 3) == 0;
  unsigned long long* o = reinterpret_cast<unsigned long long*>(sums);
  const dim3 grid((unsigned)n_images), block(imgtab::THREADS);
  hipStream_t st = as_stream(stream);
  if (C == 1) hipLaunchKernelGGL((imgtab::channel_stats_k<1>), grid, block, 0, st, table, hw, quad, o);
  else if (C == 2) hipLaunchKernelGGL((imgtab::channel_stats_k<2>), grid, block, 0, st, table, hw, quad, o);
  else if (C == 3) hipLaunchKernelGGL((imgtab::channel_stats_k<3>), grid, block, 0, st, table, hw, quad, o);
  else hipLaunchKernelGGL((imgtab::channel_stats_k<4>), grid, block, 0, st, table, hw, quad, o);
  return launch_status("clica_image_channel_stats");
}
