// KITTI-masks temporal pairs, gathered and interleaved on the device  --  the batch assembly of
// /root/reference/kitti_masks/dataset.py:90-131 (__getitem__: frame `start` and frame `end` of one pedestrian sequence, uint8 mask
// * 255 -> float32 / 255, channel dim added) and :134-142 (custom_collate: inputs = [first_0, second_0, first_1, second_1, ...],
// labels likewise).  The reference builds the batch on DataLoader workers from a pickled list of bool arrays and copies it to the
// GPU; here every frame of the data set lives in HBM as one uint8 tensor [F][H*W] (4 KB per 64 x 64 mask) and ONE launch writes the
// interleaved float32 batch [2B][1][H][W] and the interleaved latents [2B][3] from the two frame indices of each pair.
// HBM-bound: 2 B H W bytes read, 8 B H W bytes written (B = 1024 pairs of 64 x 64: 8.4 MB + 33.6 MB).
// Next to it: the same gather of single frames (frames_k: the evaluation's first frames), and sample_pairs_k, which also DRAWS the
// pairs -- the shuffled, drop_last stream of the reference's DataLoader walked by a device counter, so that a captured training step
// holds its own data.
#include "common.h"
#include "sampler_dev.h"

namespace clica {
namespace kitti {
constexpr int THREADS = 256;
typedef float f32x4 __attribute__((ext_vector_type(4)));

// astype(uint8) * 255 ... / 255.0 (:100-101, :128-131) of four pixels: 0 -> 0.0f, 1 -> 1.0f (255 / 255.0 is exactly 1); other byte
// values v (never produced by the bool masks) follow the same formula with uint8 wrap-around: ((v * 255) & 255) / 255
__device__ __forceinline__ f32x4 to_float4(uint32_t px) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const uint32_t v = (px >> (8 * e)) & 255u;
    o[e] = (float)((v * 255u) & 255u) / 255.0f;
  }
  return o;
}

__global__ __launch_bounds__(THREADS) void pairs_k(const uint8_t* __restrict__ frames, int64_t frame_elems, int64_t n_frames,
                                                   const int64_t* __restrict__ first, const int64_t* __restrict__ second, int64_t n_pairs,
                                                   float* __restrict__ images, const float* __restrict__ latents, int n_lat,
                                                   float* __restrict__ labels) {
  const int64_t quads = frame_elems / 4;                    // 4 pixels (one 32-bit load, one 16-byte store) per thread step
  const int64_t total = 2 * n_pairs * quads;
  for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * THREADS) {
    const int64_t img = t / quads, q = t - img * quads;     // image 2 i = first of pair i, 2 i + 1 = second
    int64_t f = (img & 1) ? second[img >> 1] : first[img >> 1];
    f = f < 0 ? 0 : (f >= n_frames ? n_frames - 1 : f);     // (indices are validated on the host; never read out of bounds)
    const uint32_t px = *reinterpret_cast<const uint32_t*>(frames + f * frame_elems + 4 * q);
    *reinterpret_cast<f32x4*>(images + img * frame_elems + 4 * q) = to_float4(px);
  }
  if (labels) {
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < 2 * n_pairs * n_lat; t += (int64_t)gridDim.x * THREADS) {
      const int64_t img = t / n_lat; const int k = (int)(t - img * n_lat);
      int64_t f = (img & 1) ? second[img >> 1] : first[img >> 1];
      f = f < 0 ? 0 : (f >= n_frames ? n_frames - 1 : f);
      labels[t] = latents[f * n_lat + k];
    }
  }
}

// Single frames (no pairing): images[j] = float(frames[ids[j]]), labels[j] = latents[ids[j]]  --  the evaluation's first frames.
__global__ __launch_bounds__(THREADS) void frames_k(const uint8_t* __restrict__ frames, int64_t frame_elems, int64_t n_frames,
                                                    const int64_t* __restrict__ ids, int64_t n, float* __restrict__ images,
                                                    const float* __restrict__ latents, int n_lat, float* __restrict__ labels) {
  const int64_t quads = frame_elems / 4;
  const int64_t total = n * quads;
  for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * THREADS) {
    const int64_t img = t / quads, q = t - img * quads;
    int64_t f = ids[img];
    f = f < 0 ? 0 : (f >= n_frames ? n_frames - 1 : f);     // (never read out of bounds: an id outside the table gives its nearest frame;
                                                            //  ops.kitti_gather_frames refuses such ids where it sees them on the host)
    *reinterpret_cast<f32x4*>(images + img * frame_elems + 4 * q) = to_float4(*reinterpret_cast<const uint32_t*>(frames + f * frame_elems + 4 * q));
  }
  if (labels) {
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < n * n_lat; t += (int64_t)gridDim.x * THREADS) {
      const int64_t img = t / n_lat; const int k = (int)(t - img * n_lat);
      int64_t f = ids[img];
      f = f < 0 ? 0 : (f >= n_frames ? n_frames - 1 : f);
      labels[t] = latents[f * n_lat + k];
    }
  }
}

// The NEXT batch of the training stream, drawn where it is gathered: the sampler of a DataLoader(shuffle=True, drop_last=True) over
// KittiMasks plus __getitem__'s index arithmetic (:91-98) plus custom_collate, one launch, nothing from the host but the launch itself.
//   c = state[0] (batches drawn so far), pair i of the batch: r = (c mod steps_per_epoch) B + i, index = order[r] (the epoch's
//   permutation, refilled by the owner between epochs), t = 1 + mulhi(philox(seed; i, c, STREAM_TIME_STEP), max_delta_t),
//   seq = #{cumlens <= index} (searchsorted side="right"), start = index - cumlens[seq - 1], end = min(start + t, seq_len - 1),
//   frames seq_start + start and seq_start + end.
// One group of four waves per pair: its lane 0 does the lookup (a chain of dependent loads: counter, order, ceil(log2(n_seq + 1)) search
// steps, three table reads), the group streams the two frames.  The last workgroup to finish advances the counter (every workgroup has read it by
// then), the pattern of adam_k / sgd_k: consecutive replays of a captured launch walk the stream.
constexpr uint32_t STREAM_TIME_STEP = 0x4B495454u;      // Philox stream id of the time-step draw ("KITT"): no other sampler uses it

struct SampleArgs {
  const uint8_t* frames; int64_t frame_elems, n_frames;
  const float* latents; int n_lat;
  const int64_t* cumlens; const int64_t* seq_start; const int64_t* seq_len; int64_t n_seq, n_items;
  const int64_t* order; int64_t B, steps_per_epoch; uint32_t max_delta_t; int search_steps; uint64_t seed;
  unsigned long long* state;       // [0] batch counter, [1] ticket word (low 32 bits)
  float* images; float* labels;
  int64_t* out_index; int64_t* out_t; int64_t* out_first; int64_t* out_second;
};

// Four pairs per workgroup, one per group of THREADS threads (4 waves): the ticket word then takes one arrival per FOUR pairs -- returning
// atomics on one word serialise.  With one arrival per pair (1024 workgroups) the launch took 21.8 us against 15.5 us in this form
// (profiles/c5_stream_summary.md); that the arrivals account for the difference is inferred from this one pair of timings, not from a
// measured atomic rate.
constexpr int SUBS = 4;

__global__ __launch_bounds__(SUBS * THREADS) void sample_pairs_k(const SampleArgs a) {
  __shared__ int64_t s_frame[SUBS][2];
  const int sub = threadIdx.x / THREADS, tid = threadIdx.x % THREADS;
  const int64_t quads = a.frame_elems / 4;
  // (the host launches ceil(B / SUBS) workgroups up to a cap: at most ceil(B / (SUBS grid)) rounds, the same for every thread)
  for (int64_t base = (int64_t)blockIdx.x * SUBS; base < a.B; base += (int64_t)gridDim.x * SUBS) {
    const int64_t i = base + sub;
    const bool active = i < a.B;
    if (active && tid == 0) {
      const uint64_t c = a.state[0];
      const int64_t r = (int64_t)(c % (uint64_t)a.steps_per_epoch) * a.B + i;      // < steps_per_epoch B <= n_items
      int64_t index = a.order[r];
      index = index < 0 ? 0 : (index >= a.n_items ? a.n_items - 1 : index);        // (order is a permutation; never read out of bounds)
      rng::Philox g(a.seed, (uint32_t)i, (uint32_t)c, STREAM_TIME_STEP, (uint32_t)(c >> 32));
      const int64_t t = 1 + (int64_t)(((uint64_t)g.next() * a.max_delta_t) >> 32);  // uniform in 1 .. max_delta_t, multiply-high
      int64_t lo = 0, hi = a.n_seq;
      for (int k = 0; k < a.search_steps; ++k) {                // 2^search_steps > n_seq: the interval is empty after that many halvings
        if (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (a.cumlens[mid] <= index) lo = mid + 1; else hi = mid;
        }
      }
      const int64_t seq = lo < a.n_seq ? lo : a.n_seq - 1;      // (index < n_items = cumlens[n_seq - 1], so lo <= n_seq - 1 already)
      const int64_t start = index - (seq > 0 ? a.cumlens[seq - 1] : 0);
      int64_t end = start + t;
      const int64_t last = a.seq_len[seq] - 1;
      end = end < last ? end : last;
      const int64_t first_frame = a.seq_start[seq];
      int64_t f0 = first_frame + start, f1 = first_frame + end;
      f0 = f0 < 0 ? 0 : (f0 >= a.n_frames ? a.n_frames - 1 : f0);
      f1 = f1 < 0 ? 0 : (f1 >= a.n_frames ? a.n_frames - 1 : f1);
      s_frame[sub][0] = f0; s_frame[sub][1] = f1;
      if (a.out_index) a.out_index[i] = index;
      if (a.out_t) a.out_t[i] = t;
      if (a.out_first) a.out_first[i] = f0;
      if (a.out_second) a.out_second[i] = f1;
    }
    __syncthreads();
    if (active) {
      const int64_t f0 = s_frame[sub][0], f1 = s_frame[sub][1];
      const uint8_t* src0 = a.frames + f0 * a.frame_elems;
      const uint8_t* src1 = a.frames + f1 * a.frame_elems;
      float* dst = a.images + 2 * i * a.frame_elems;            // image 2 i = first, 2 i + 1 = second: contiguous
      for (int64_t q = tid; q < quads; q += THREADS) {
        const uint32_t p0 = *reinterpret_cast<const uint32_t*>(src0 + 4 * q);
        const uint32_t p1 = *reinterpret_cast<const uint32_t*>(src1 + 4 * q);
        *reinterpret_cast<f32x4*>(dst + 4 * q) = to_float4(p0);
        *reinterpret_cast<f32x4*>(dst + a.frame_elems + 4 * q) = to_float4(p1);
      }
      if (a.labels && tid < 2 * a.n_lat) {
        const int half = tid >= a.n_lat, k = tid - half * a.n_lat;
        a.labels[(2 * i + half) * a.n_lat + k] = a.latents[(half ? f1 : f0) * a.n_lat + k];
      }
    }
    __syncthreads();                                            // s_frame is rewritten in the next round
  }
  // tick (relaxed ticket, no fence, as adam_k / sgd_k): the ONLY thing the increment must stay behind is every workgroup's reads of
  // state[0].  Those reads happen in the lookup branch above, whose value is consumed (it addresses order[]) before that round's first
  // __syncthreads; thread 0 arrives here after the last round's barriers, so all of its workgroup's reads are complete.  Whoever
  // restructures the loop must keep every read of state[0] in front of a barrier that thread 0 passes before this arrival.
  if (threadIdx.x == 0) {
    if (__hip_atomic_fetch_add(reinterpret_cast<int32_t*>(a.state + 1), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1) {
      a.state[0] = a.state[0] + 1;
      __hip_atomic_store(reinterpret_cast<int32_t*>(a.state + 1), 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
}  // namespace kitti
}  // namespace clica

using namespace clica;

extern "C" int clica_kitti_gather_pairs(const uint8_t* frames, int64_t frame_elems, int64_t n_frames, const int64_t* first_frame,
                                        const int64_t* second_frame, int64_t n_pairs, float* images, const float* latents, int32_t n_latents,
                                        float* labels, clica_stream_t stream) {
  CLICA_CHECK_ARG(frames && first_frame && second_frame && images && n_pairs > 0 && n_frames > 0, "clica_kitti_gather_pairs: NULL pointer / empty batch");
  CLICA_CHECK_ARG(frame_elems > 0 && frame_elems % 4 == 0, "clica_kitti_gather_pairs: %lld pixels per frame (a multiple of 4 required)", (long long)frame_elems);
  CLICA_CHECK_ARG((reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (reinterpret_cast<uintptr_t>(images) & 15) == 0,
                  "clica_kitti_gather_pairs: frames must be 4-byte, images 16-byte aligned");
  CLICA_CHECK_ARG(!labels || (latents && n_latents >= 1), "clica_kitti_gather_pairs: labels requested without a latent table");
  const int64_t work = 2 * n_pairs * (frame_elems / 4);
  const int64_t blocks = ceil_div(work, kitti::THREADS);
  hipLaunchKernelGGL(kitti::pairs_k, dim3((unsigned)(blocks < 8 * kNumCU ? blocks : 8 * kNumCU)), dim3(kitti::THREADS), 0, as_stream(stream),
                     frames, frame_elems, n_frames, first_frame, second_frame, n_pairs, images, latents, (int)n_latents, labels);
  return launch_status("clica_kitti_gather_pairs");
}

extern "C" int clica_kitti_gather_frames(const uint8_t* frames, int64_t frame_elems, int64_t n_frames, const int64_t* frame_ids, int64_t n,
                                         float* images, const float* latents, int32_t n_latents, float* labels, clica_stream_t stream) {
  CLICA_CHECK_ARG(frames && frame_ids && images && n > 0 && n_frames > 0, "clica_kitti_gather_frames: NULL pointer / empty batch");
  CLICA_CHECK_ARG(frame_elems > 0 && frame_elems % 4 == 0, "clica_kitti_gather_frames: %lld pixels per frame (a multiple of 4 required)", (long long)frame_elems);
  CLICA_CHECK_ARG((reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (reinterpret_cast<uintptr_t>(images) & 15) == 0,
                  "clica_kitti_gather_frames: frames must be 4-byte, images 16-byte aligned");
  CLICA_CHECK_ARG(!labels || (latents && n_latents >= 1), "clica_kitti_gather_frames: labels requested without a latent table");
  const int64_t blocks = ceil_div(n * (frame_elems / 4), kitti::THREADS);
  hipLaunchKernelGGL(kitti::frames_k, dim3((unsigned)(blocks < 8 * kNumCU ? blocks : 8 * kNumCU)), dim3(kitti::THREADS), 0, as_stream(stream),
                     frames, frame_elems, n_frames, frame_ids, n, images, latents, (int)n_latents, labels);
  return launch_status("clica_kitti_gather_frames");
}

extern "C" int clica_kitti_sample_pairs(const uint8_t* frames, int64_t frame_elems, int64_t n_frames, const float* latents, int32_t n_latents,
                                        const int64_t* cumlens, const int64_t* seq_start, const int64_t* seq_len, int64_t n_seq,
                                        int64_t n_items, const int64_t* order, int64_t n_pairs, int32_t max_delta_t, uint64_t seed,
                                        uint64_t* state, float* images, float* labels, int64_t* out_index, int64_t* out_t,
                                        int64_t* out_first, int64_t* out_second, clica_stream_t stream) {
  CLICA_CHECK_ARG(frames && cumlens && seq_start && seq_len && order && state && images, "clica_kitti_sample_pairs: NULL pointer");
  CLICA_CHECK_ARG(n_frames > 0 && n_seq > 0 && n_items > 0, "clica_kitti_sample_pairs: empty table");
  CLICA_CHECK_ARG(frame_elems > 0 && frame_elems % 4 == 0, "clica_kitti_sample_pairs: %lld pixels per frame (a multiple of 4 required)", (long long)frame_elems);
  CLICA_CHECK_ARG((reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (reinterpret_cast<uintptr_t>(images) & 15) == 0 &&
                      (reinterpret_cast<uintptr_t>(state) & 7) == 0,
                  "clica_kitti_sample_pairs: frames must be 4-byte, images 16-byte, state 8-byte aligned");
  CLICA_CHECK_ARG(!labels || (latents && n_latents >= 1 && 2 * n_latents <= kitti::THREADS), "clica_kitti_sample_pairs: labels need a latent table of 1..%d columns", kitti::THREADS / 2);
  CLICA_CHECK_ARG(max_delta_t >= 1, "clica_kitti_sample_pairs: max_delta_t = %d (>= 1 required)", (int)max_delta_t);
  CLICA_CHECK_ARG(n_pairs >= 1, "clica_kitti_sample_pairs: %lld pairs per batch", (long long)n_pairs);
  CLICA_CHECK_ARG(n_pairs <= n_items, "clica_kitti_sample_pairs: %lld pairs per batch from %lld items (no full batch exists)", (long long)n_pairs, (long long)n_items);
  kitti::SampleArgs a;
  a.frames = frames; a.frame_elems = frame_elems; a.n_frames = n_frames; a.latents = latents; a.n_lat = (int)n_latents;
  a.cumlens = cumlens; a.seq_start = seq_start; a.seq_len = seq_len; a.n_seq = n_seq; a.n_items = n_items;
  a.order = order; a.B = n_pairs; a.steps_per_epoch = n_items / n_pairs; a.max_delta_t = (uint32_t)max_delta_t; a.seed = seed;
  a.search_steps = 1;
  while (a.search_steps < 63 && ((int64_t)1 << a.search_steps) <= n_seq) ++a.search_steps;
  a.state = reinterpret_cast<unsigned long long*>(state); a.images = images; a.labels = labels;
  a.out_index = out_index; a.out_t = out_t; a.out_first = out_first; a.out_second = out_second;
  const int64_t blocks = ceil_div(n_pairs, kitti::SUBS);      // one workgroup (one ticket arrival) per CU at the most; beyond that, rounds
  hipLaunchKernelGGL(kitti::sample_pairs_k, dim3((unsigned)(blocks < kNumCU ? blocks : kNumCU)), dim3(kitti::SUBS * kitti::THREADS), 0,
                     as_stream(stream), a);
  return launch_status("clica_kitti_sample_pairs");
}
