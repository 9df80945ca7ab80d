// Training pair of the dot-product InfoNCE loss (SimCLRLoss.loss with normalize=False, /root/reference/losses.py:177-202) for gfx950:
// what the fused engine step calls at p = 0.  The negatives are a POOL that contains the anchors (the reference's z3_rec = roll(z1_rec),
// main_mlp.py:272; under data parallelism the all-gather of every rank's z1_rec).
//
//   s_ij = <z1_i, pool_j> / tau,  x = s log2(e) (the kernels' log2 domain),  pos_i = <z1_i, z2_i>
//   L_i  = log2 sum_j 2^x_ij + 2^(pos_i log2(e)/tau)   (lse_i as clica_dot_loss_fwd writes it: log2 units, the positive pair included)
//   loss_i = 2 (alpha (-pos_i/tau) + (1 - alpha) L_i ln 2)
//
// forward  (one launch)  grid (owner tiles of 64 rows) x (pool splits).  A workgroup keeps its 64 owner rows in registers (two per lane;
//          lanes l and l + 32 hold the same two owners and read different pool rows of the LDS tile, so one ds_read_b128 serves both
//          halves and both owners) and sweeps its pool chunk through LDS, 64 rows at a time, with a true running maximum per owner: the
//          Lp pair's shortcut (the self-pair is the row maximum) does not hold for dot products of rows of unequal norm.  Each workgroup
//          stores one (max, sum) partial per owner; the last workgroup to arrive at a tile (agent-scope arrival counter, as in
//          lp_finalize.h) merges the tile's partials in split order -- deterministic whoever arrives last -- adds the positive pair,
//          writes loss_i / pos_i / lse_i, the positive-pair part of dz1 / dz2 and the tile's sums of the three means.
// backward (two launches) one symmetric sweep: s is symmetric and every pool row is an anchor whose negatives contain this rank's
//          rows, so  dz1_k += (2 (1 - alpha) / (B tau)) sum_j (2^(x_kj - L_k) + 2^(x_kj - L_j)) pool_j  with L_j = pool_lse[j] -- no
//          column pass, no dz3 (the argument of DESIGN 4.2 for Lp).  Both exponents are <= 0 up to rounding (L_k and L_j are
//          log-sum-exps over sets that contain x_kj), so no maximum is needed.  The reduction launch sums the per-split partials in
//          split order into dz1, writes means[3] from the forward's tile sums and advances the step counter.
//
// Vector ALU only (packed v_pk_fma_f32 on coordinate pairs); rows up to 64 coordinates.
#include "common.h"

namespace clica {
namespace dot_train {

typedef float f32x2 __attribute__((ext_vector_type(2)));
constexpr int THREADS = 256;
constexpr int ROWS = 64;              // owner rows per workgroup = one finisher tile
constexpr int TS = 64;                // pool rows per LDS tile
constexpr int G = TS / 8;             // pool rows of a tile per half-wave (wave w, half h: rows [G (2w + h), G (2w + h + 1)))
constexpr int TARGET_BLOCKS = 1024;   // ~4 workgroups per CU
constexpr int kMaxN = 64;
constexpr float kNegBig = -1e30f;

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float flog2(float x) { return __builtin_amdgcn_logf(x); }

struct Plan { int64_t tiles; int nsplit; int64_t chunk; };
static Plan make_plan(int64_t B, int64_t B3) {
  Plan P;
  P.tiles = ceil_div(B, ROWS);
  int64_t want = ceil_div(TARGET_BLOCKS, P.tiles);
  if (want < 1) want = 1;
  if (want > ceil_div(B3, TS)) want = ceil_div(B3, TS);
  P.chunk = ceil_div(ceil_div(B3, want), TS) * TS;      // a multiple of the tile: only the pool's last tile is ragged
  P.nsplit = (int)ceil_div(B3, P.chunk);
  return P;
}

// workspace: arrival counters (zero before the first call, left zero by every launch), tile sums of the means, forward partials,
// backward partials
struct Ws { int* arrive; float* blocksums; float2* fpart; float* bpart; size_t bytes; };
static Ws carve(void* ws, const Plan& P, int64_t B, int n) {
  Ws w{};
  char* base = (char*)ws;
  size_t off = 0;
  auto take = [&](size_t bytes) -> void* { void* r = base ? (void*)(base + off) : nullptr; off += align_up(bytes, 256); return r; };
  w.arrive = (int*)take((size_t)P.tiles * sizeof(int));
  w.blocksums = (float*)take((size_t)P.tiles * 3 * sizeof(float));
  w.fpart = (float2*)take((size_t)P.nsplit * B * sizeof(float2));
  w.bpart = (float*)take((size_t)P.nsplit * B * n * sizeof(float));
  w.bytes = off;
  return w;
}

// (m, s) <- (m, s) (+) (m2, s2): merge of two log2-domain (max, sum) pairs (commutative bit for bit)
__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
  const float mn = fmaxf(m, m2);
  s = s * fexp2(m - mn) + s2 * fexp2(m2 - mn);
  m = mn;
}

// one owner row as coordinate pairs, zero beyond n (rows past the end: all zero)
template <int NQ>
__device__ __forceinline__ void load_owner(const float* __restrict__ z, int64_t ld, int64_t i, int64_t rows, int n, f32x2 (&o)[NQ]) {
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int k = 2 * q;
    o[q].x = (i < rows && k < n) ? z[i * ld + k] : 0.f;
    o[q].y = (i < rows && k + 1 < n) ? z[i * ld + k + 1] : 0.f;
  }
}

// the pool rows of the tile starting at jt: thread-strided elements of the [TS][NP] tile (zero outside [.., j1) and beyond n)
template <int NP, int E>
__device__ __forceinline__ void fetch_tile(float (&pre)[E], const float* __restrict__ pool, int64_t ldp, int n, int64_t jt, int64_t j1) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int idx = (int)threadIdx.x + e * THREADS;
    const int rr = idx / NP, k = idx - rr * NP;
    const int64_t j = jt + rr;
    pre[e] = (j < j1 && k < n) ? pool[j * ldp + k] : 0.f;
  }
}

// logits of the two owners against pool row `sr` of the tile (log2 domain)
template <int NQ>
__device__ __forceinline__ void dot2(const float* sr, const f32x2 (&o0)[NQ], const f32x2 (&o1)[NQ], float kscale, float& x0, float& x1) {
  f32x2 a0 = {0.f, 0.f}, a1 = {0.f, 0.f};
  const float4* s4 = reinterpret_cast<const float4*>(sr);
#pragma unroll
  for (int q4 = 0; q4 < (NQ + 1) / 2; ++q4) {
    const float4 v = s4[q4];
    const f32x2 lo = {v.x, v.y}, hi = {v.z, v.w};
    a0 = __builtin_elementwise_fma(o0[2 * q4], lo, a0);            // v_pk_fma_f32: two coordinates per issue slot
    a1 = __builtin_elementwise_fma(o1[2 * q4], lo, a1);
    if (2 * q4 + 1 < NQ) {
      a0 = __builtin_elementwise_fma(o0[2 * q4 + 1], hi, a0);
      a1 = __builtin_elementwise_fma(o1[2 * q4 + 1], hi, a1);
    }
  }
  x0 = (a0.x + a0.y) * kscale;
  x1 = (a1.x + a1.y) * kscale;
}

// running (max, sum) of one owner over a group of G logits, the first `valid` of which exist
__device__ __forceinline__ void online(float& m, float& s, const float (&x)[G], int valid) {
  float mx = kNegBig;
#pragma unroll
  for (int c = 0; c < G; ++c) mx = c < valid ? fmaxf(mx, x[c]) : mx;
  const float mn = fmaxf(m, mx);
  float add = 0.f;
#pragma unroll
  for (int c = 0; c < G; ++c) add += c < valid ? fexp2(x[c] - mn) : 0.f;
  s = s * fexp2(m - mn) + add;
  m = mn;
}

struct FwdArgs {
  const float* z1; int64_t ld1; const float* z2; int64_t ld2; const float* pool; int64_t ldp;
  int64_t B, B3; int n; int64_t chunk; float kscale, tau, alpha;
  float* loss_i; float* pos_i; float* lse_i; float* dz1; int64_t ldd1; float* dz2; int64_t ldd2;
  float2* part; float* blocksums; int* arrive;
};

template <int NP>
__global__ __launch_bounds__(THREADS) void fwd_train_k(FwdArgs a) {
  constexpr int NQ = NP / 2, E = TS * NP / THREADS;
  __shared__ __attribute__((aligned(16))) float tile[TS * NP];
  __shared__ float2 red[4][ROWS];
  __shared__ int last;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  const int r0 = lane & 31, r1 = r0 + 32;
  const int64_t row0 = (int64_t)blockIdx.x * ROWS;
  f32x2 o0[NQ], o1[NQ];
  load_owner<NQ>(a.z1, a.ld1, row0 + r0, a.B, a.n, o0);
  load_owner<NQ>(a.z1, a.ld1, row0 + r1, a.B, a.n, o1);
  const int64_t j0 = (int64_t)blockIdx.y * a.chunk, j1 = min(a.B3, j0 + a.chunk);
  const int part = 2 * wave + half;
  float m0 = kNegBig, s0 = 0.f, m1 = kNegBig, s1 = 0.f;
  float pre[E];
  fetch_tile<NP, E>(pre, a.pool, a.ldp, a.n, j0, j1);
  for (int64_t jt = j0; jt < j1; jt += TS) {
    __syncthreads();                                     // the previous tile is consumed
#pragma unroll
    for (int e = 0; e < E; ++e) tile[threadIdx.x + e * THREADS] = pre[e];
    __syncthreads();
    if (jt + TS < j1) fetch_tile<NP, E>(pre, a.pool, a.ldp, a.n, jt + TS, j1);      // next tile in flight during this one
    const int valid = (int)min((int64_t)G, j1 - jt - (int64_t)part * G);
    const float* base = tile + part * G * NP;
    float x0[G], x1[G];
#pragma unroll
    for (int c = 0; c < G; ++c) dot2<NQ>(base + c * NP, o0, o1, a.kscale, x0[c], x1[c]);
    online(m0, s0, x0, valid);
    online(m1, s1, x1, valid);
  }
  // the eight partitions of an owner: half-waves by one shuffle, waves in index order through LDS
  merge(m0, s0, __shfl_xor(m0, 32, 64), __shfl_xor(s0, 32, 64));
  merge(m1, s1, __shfl_xor(m1, 32, 64), __shfl_xor(s1, 32, 64));
  if (half == 0) { red[wave][r0] = make_float2(m0, s0); red[wave][r1] = make_float2(m1, s1); }
  __syncthreads();
  if (threadIdx.x < ROWS) {
    float m = red[0][threadIdx.x].x, s = red[0][threadIdx.x].y;
#pragma unroll
    for (int w = 1; w < 4; ++w) merge(m, s, red[w][threadIdx.x].x, red[w][threadIdx.x].y);
    const int64_t i = row0 + threadIdx.x;
    if (i < a.B)      // read by another workgroup of this launch: written through to the device's coherence point
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(a.part + (int64_t)blockIdx.y * a.B + i),
                         __builtin_bit_cast(unsigned long long, make_float2(m, s)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // hand-over as in lp_finalize.h (fwd_partial_fin_k): each storing thread waits for its store's acknowledgement, the barrier collects
  // the workgroup, then thread 0 arrives; no fences
  __builtin_amdgcn_s_waitcnt(0x0F70);                   // vmcnt(0)
  __syncthreads();
  if (threadIdx.x == 0) {
    const int prev = __hip_atomic_fetch_add(&a.arrive[blockIdx.x], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    last = prev == (int)gridDim.y - 1;
    if (last) __hip_atomic_store(&a.arrive[blockIdx.x], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // every arrival is in
  }
  __syncthreads();
  if (!last) return;

  // ---- tile finisher: four groups of 64 threads merge the splits g, g + 4, ... of each row, then group 0 merges the groups in order
  const int r = threadIdx.x & (ROWS - 1), grp = threadIdx.x / ROWS;
  const int64_t i = row0 + r;
  float m = kNegBig, s = 0.f;
  if (i < a.B) {
    for (int sp = grp; sp < (int)gridDim.y; sp += 4) {
      const float2 p = __builtin_bit_cast(float2, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(a.part + (int64_t)sp * a.B + i),
                                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      merge(m, s, p.x, p.y);
    }
  }
  red[grp][r] = make_float2(m, s);
  __syncthreads();
  if (grp != 0) return;
  float v[3] = {0.f, 0.f, 0.f};
  if (i < a.B) {
#pragma unroll
    for (int w = 1; w < 4; ++w) merge(m, s, red[w][r].x, red[w][r].y);
    const float* ra = a.z1 + i * a.ld1;
    const float* rb = a.z2 + i * a.ld2;
    float pos = 0.f;
    for (int k = 0; k < a.n; ++k) pos += ra[k] * rb[k];
    const float xp = pos * a.kscale;
    merge(m, s, xp, 1.f);                                // the positive pair joins the denominator (losses.py:190-193)
    const float L2 = m + flog2(s);
    const float lse = L2 * kLn2;
    const float lp = -pos / a.tau;                       // loss_pos (losses.py:192)
    const float li = 2.f * (a.alpha * lp + (1.f - a.alpha) * lse);
    a.loss_i[i] = li; a.pos_i[i] = lp; a.lse_i[i] = L2;
    // d mean(loss) / d pos_i = (2 / B) ((1 - alpha) w+_i - alpha) / tau,  w+_i = 2^(xp - L_i)
    const float coef = (2.f / (float)a.B) * ((1.f - a.alpha) * fexp2(xp - L2) - a.alpha) / a.tau;
    for (int k = 0; k < a.n; ++k) {
      if (a.dz1) a.dz1[i * a.ldd1 + k] = coef * rb[k];
      if (a.dz2) a.dz2[i * a.ldd2 + k] = coef * ra[k];
    }
    v[0] = li; v[1] = lp; v[2] = lse;
  }
  // the tile's sums of the three means (wave 0 holds every row): fixed shuffle tree, read by the reduction launch of the backward
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_down(v[c], off, 64);
  }
  if (threadIdx.x == 0) { a.blocksums[blockIdx.x * 3 + 0] = v[0]; a.blocksums[blockIdx.x * 3 + 1] = v[1]; a.blocksums[blockIdx.x * 3 + 2] = v[2]; }
}

struct BwdArgs {
  const float* z1; int64_t ld1; const float* pool; int64_t ldp; const float* lse_i; const float* pool_lse;
  int64_t B, B3; int n; int64_t chunk; float kscale;
  float* part;
};

template <int NP>
__global__ __launch_bounds__(THREADS) void bwd_sym_k(BwdArgs a) {
  constexpr int NQ = NP / 2, E = TS * NP / THREADS;
  __shared__ __attribute__((aligned(16))) float tile[TS * NP];     // (after the sweep: the [ROWS][NP] sum of the waves)
  __shared__ float tl[TS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5;
  const int r0 = lane & 31, r1 = r0 + 32;
  const int64_t row0 = (int64_t)blockIdx.x * ROWS;
  f32x2 o0[NQ], o1[NQ], g0[NQ], g1[NQ];
  load_owner<NQ>(a.z1, a.ld1, row0 + r0, a.B, a.n, o0);
  load_owner<NQ>(a.z1, a.ld1, row0 + r1, a.B, a.n, o1);
#pragma unroll
  for (int q = 0; q < NQ; ++q) { g0[q] = (f32x2){0.f, 0.f}; g1[q] = (f32x2){0.f, 0.f}; }
  const float L0 = row0 + r0 < a.B ? a.lse_i[row0 + r0] : 1e30f;     // (rows past the end: weight 0 from the owner side, never written)
  const float L1 = row0 + r1 < a.B ? a.lse_i[row0 + r1] : 1e30f;
  const int64_t j0 = (int64_t)blockIdx.y * a.chunk, j1 = min(a.B3, j0 + a.chunk);
  const int part = 2 * wave + half;
  float pre[E];
  float pl = 0.f;
  fetch_tile<NP, E>(pre, a.pool, a.ldp, a.n, j0, j1);
  if (threadIdx.x < TS) pl = j0 + threadIdx.x < j1 ? a.pool_lse[j0 + threadIdx.x] : 1e30f;
  for (int64_t jt = j0; jt < j1; jt += TS) {
    __syncthreads();
#pragma unroll
    for (int e = 0; e < E; ++e) tile[threadIdx.x + e * THREADS] = pre[e];
    if (threadIdx.x < TS) tl[threadIdx.x] = pl;
    __syncthreads();
    if (jt + TS < j1) {
      fetch_tile<NP, E>(pre, a.pool, a.ldp, a.n, jt + TS, j1);
      if (threadIdx.x < TS) pl = jt + TS + threadIdx.x < j1 ? a.pool_lse[jt + TS + threadIdx.x] : 1e30f;
    }
    const int valid = (int)min((int64_t)G, j1 - jt - (int64_t)part * G);
    const float* base = tile + part * G * NP;
#pragma unroll
    for (int c = 0; c < G; ++c) {
      const float* sr = base + c * NP;
      float x0, x1;
      dot2<NQ>(sr, o0, o1, a.kscale, x0, x1);
      const float Lj = tl[part * G + c];
      // (a padded pool row is zero: its logit 0 can sit far above a row's L, so it is masked, not multiplied by its zeros)
      const float w0 = c < valid ? fexp2(x0 - L0) + fexp2(x0 - Lj) : 0.f;
      const float w1 = c < valid ? fexp2(x1 - L1) + fexp2(x1 - Lj) : 0.f;
      const f32x2 w0v = {w0, w0}, w1v = {w1, w1};
      const float4* s4 = reinterpret_cast<const float4*>(sr);
#pragma unroll
      for (int q4 = 0; q4 < (NQ + 1) / 2; ++q4) {
        const float4 v = s4[q4];
        const f32x2 lo = {v.x, v.y}, hi = {v.z, v.w};
        g0[2 * q4] = __builtin_elementwise_fma(w0v, lo, g0[2 * q4]);
        g1[2 * q4] = __builtin_elementwise_fma(w1v, lo, g1[2 * q4]);
        if (2 * q4 + 1 < NQ) {
          g0[2 * q4 + 1] = __builtin_elementwise_fma(w0v, hi, g0[2 * q4 + 1]);
          g1[2 * q4 + 1] = __builtin_elementwise_fma(w1v, hi, g1[2 * q4 + 1]);
        }
      }
    }
  }
  // the eight partitions of an owner: half-waves by shuffle, then the waves added in index order into the tile buffer
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    g0[q].x += __shfl_xor(g0[q].x, 32, 64); g0[q].y += __shfl_xor(g0[q].y, 32, 64);
    g1[q].x += __shfl_xor(g1[q].x, 32, 64); g1[q].y += __shfl_xor(g1[q].y, 32, 64);
  }
  for (int w = 0; w < 4; ++w) {
    __syncthreads();
    if (wave == w && half == 0) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        float* d0 = tile + r0 * NP + 2 * q;
        float* d1 = tile + r1 * NP + 2 * q;
        d0[0] = (w ? d0[0] : 0.f) + g0[q].x; d0[1] = (w ? d0[1] : 0.f) + g0[q].y;
        d1[0] = (w ? d1[0] : 0.f) + g1[q].x; d1[1] = (w ? d1[1] : 0.f) + g1[q].y;
      }
    }
  }
  __syncthreads();
  const int64_t rows = min((int64_t)ROWS, a.B - row0);
  float* out = a.part + ((int64_t)blockIdx.y * a.B + row0) * a.n;
  for (int idx = threadIdx.x; idx < (int)rows * a.n; idx += THREADS) {
    const int rr = idx / a.n, k = idx - rr * a.n;
    out[idx] = tile[rr * NP + k];
  }
}

// dz1 += coef * (sum of the splits' partials, in split order); block 0 also writes the forward's three means (tile sums in index
// order, then a fixed shuffle tree) and advances the step counter
__global__ __launch_bounds__(THREADS) void bwd_reduce_k(const float* __restrict__ part, int nsplit, int64_t B, int n, float coef,
                                                       float* __restrict__ dz1, int64_t ldd1, const float* __restrict__ blocksums,
                                                       int nblocks, float inv_count, float* __restrict__ means, int32_t* __restrict__ tick) {
  if (blockIdx.x == 0 && threadIdx.x < 64) {
    float v[3] = {0.f, 0.f, 0.f};
    for (int b = threadIdx.x; b < nblocks; b += 64) {
      v[0] += blocksums[b * 3 + 0]; v[1] += blocksums[b * 3 + 1]; v[2] += blocksums[b * 3 + 2];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v[c] += __shfl_down(v[c], off, 64);
    }
    if (threadIdx.x == 0) {
      if (means) { means[0] = v[0] * inv_count; means[1] = v[1] * inv_count; means[2] = v[2] * inv_count; }
      if (tick) tick[0] = tick[0] + 1;
    }
  }
  const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
  if (idx >= B * n) return;
  const int64_t i = idx / n;
  const int k = (int)(idx - i * n);
  float s = 0.f;
  for (int sp = 0; sp < nsplit; ++sp) s += part[(int64_t)sp * B * n + idx];
  dz1[i * ldd1 + k] += coef * s;
}

#define DOT_TRAIN_FOR_NP(NPV, BODY)                                                   \
  switch (NPV) {                                                                       \
    case 4: { constexpr int NP = 4; BODY } break;   case 8: { constexpr int NP = 8; BODY } break;     \
    case 12: { constexpr int NP = 12; BODY } break; case 16: { constexpr int NP = 16; BODY } break;   \
    case 20: { constexpr int NP = 20; BODY } break; case 24: { constexpr int NP = 24; BODY } break;   \
    case 28: { constexpr int NP = 28; BODY } break; case 32: { constexpr int NP = 32; BODY } break;   \
    case 36: { constexpr int NP = 36; BODY } break; case 40: { constexpr int NP = 40; BODY } break;   \
    case 44: { constexpr int NP = 44; BODY } break; case 48: { constexpr int NP = 48; BODY } break;   \
    case 52: { constexpr int NP = 52; BODY } break; case 56: { constexpr int NP = 56; BODY } break;   \
    case 60: { constexpr int NP = 60; BODY } break; case 64: { constexpr int NP = 64; BODY } break;   \
    default: break;                                                                    \
  }

static int validate(const clica_dot_loss_desc* d, const char* who) {
  CLICA_CHECK_ARG(d != nullptr, "%s: desc is NULL", who);
  CLICA_CHECK_ARG(d->B > 0 && d->B3 >= d->B, "%s: B=%lld B3=%lld: need 0 < B <= B3 (the pool contains the local rows)", who,
                  (long long)d->B, (long long)d->B3);
  CLICA_CHECK_ARG(d->n >= 1 && d->n <= kMaxN, "%s: n=%d: the dot training pair covers rows of 1..%d coordinates", who, d->n, kMaxN);
  CLICA_CHECK_ARG(d->tau > 0.f, "%s: tau=%g must be > 0", who, d->tau);
  CLICA_CHECK_ARG(d->normalize == 0, "%s: normalize=1 is not supported by the training pair (use clica_dot_loss_fwd / _bwd)", who);
  return CLICA_OK;
}
static int pad_np(int n) { return (n + 3) / 4 * 4; }

}  // namespace dot_train
}  // namespace clica

using namespace clica;
using namespace clica::dot_train;

extern "C" int clica_dot_loss_train_workspace_bytes(const clica_dot_loss_desc* d, size_t* bytes) {
  int rc = validate(d, "clica_dot_loss_train_workspace_bytes");
  if (rc) return rc;
  CLICA_CHECK_ARG(bytes != nullptr, "clica_dot_loss_train_workspace_bytes: bytes is NULL");
  *bytes = carve(nullptr, make_plan(d->B, d->B3), d->B, d->n).bytes;
  return CLICA_OK;
}

extern "C" int clica_dot_loss_fwd_train(const clica_dot_loss_desc* d,
                                        const float* z1, int64_t ld1, const float* z2, int64_t ld2, const float* pool, int64_t ldp,
                                        float* loss_i, float* pos_i, float* lse_i,
                                        float* dz1, int64_t ldd1, float* dz2, int64_t ldd2,
                                        void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  int rc = validate(d, "clica_dot_loss_fwd_train");
  if (rc) return rc;
  CLICA_CHECK_ARG(z1 && z2 && pool && loss_i && pos_i && lse_i && workspace, "clica_dot_loss_fwd_train: NULL pointer");
  CLICA_CHECK_ARG(ld1 >= d->n && ld2 >= d->n && ldp >= d->n, "clica_dot_loss_fwd_train: leading dimension < n");
  CLICA_CHECK_ARG((!dz1 || ldd1 >= d->n) && (!dz2 || ldd2 >= d->n), "clica_dot_loss_fwd_train: gradient leading dimension < n");
  const Plan P = make_plan(d->B, d->B3);
  const Ws w = carve(workspace, P, d->B, d->n);
  if (w.bytes > workspace_bytes) { set_error("clica_dot_loss_fwd_train: workspace %zu < %zu", workspace_bytes, w.bytes); return CLICA_E_WORKSPACE; }
  FwdArgs a{z1, ld1, z2, ld2, pool, ldp, d->B, d->B3, d->n, P.chunk, kLog2e / d->tau, d->tau, d->alpha,
            loss_i, pos_i, lse_i, dz1, ldd1, dz2, ldd2, w.fpart, w.blocksums, w.arrive};
  dim3 grid((unsigned)P.tiles, (unsigned)P.nsplit), block(THREADS);
  hipStream_t st = as_stream(stream);
  DOT_TRAIN_FOR_NP(pad_np(d->n), { hipLaunchKernelGGL((fwd_train_k<NP>), grid, block, 0, st, a); })
  return launch_status("clica_dot_loss_fwd_train");
}

extern "C" int clica_dot_loss_bwd_sym_train(const clica_dot_loss_desc* d,
                                            const float* z1, int64_t ld1, const float* pool, int64_t ldp,
                                            const float* lse_i, const float* pool_lse,
                                            float* dz1, int64_t ldd1, float* means, int32_t* tick_counter,
                                            void* workspace, size_t workspace_bytes, clica_stream_t stream) {
  int rc = validate(d, "clica_dot_loss_bwd_sym_train");
  if (rc) return rc;
  CLICA_CHECK_ARG(z1 && pool && lse_i && pool_lse && dz1 && workspace, "clica_dot_loss_bwd_sym_train: NULL pointer");
  CLICA_CHECK_ARG(ld1 >= d->n && ldp >= d->n && ldd1 >= d->n, "clica_dot_loss_bwd_sym_train: leading dimension < n");
  const Plan P = make_plan(d->B, d->B3);
  const Ws w = carve(workspace, P, d->B, d->n);
  if (w.bytes > workspace_bytes) { set_error("clica_dot_loss_bwd_sym_train: workspace %zu < %zu", workspace_bytes, w.bytes); return CLICA_E_WORKSPACE; }
  BwdArgs a{z1, ld1, pool, ldp, lse_i, pool_lse, d->B, d->B3, d->n, P.chunk, kLog2e / d->tau, w.bpart};
  dim3 grid((unsigned)P.tiles, (unsigned)P.nsplit), block(THREADS);
  hipStream_t st = as_stream(stream);
  DOT_TRAIN_FOR_NP(pad_np(d->n), { hipLaunchKernelGGL((bwd_sym_k<NP>), grid, block, 0, st, a); })
  const float coef = 2.f * (1.f - d->alpha) / ((float)d->B * d->tau);
  const int64_t elems = d->B * d->n;
  hipLaunchKernelGGL(bwd_reduce_k, dim3((unsigned)ceil_div(elems, (int64_t)THREADS)), dim3(THREADS), 0, st,
                     (const float*)w.bpart, P.nsplit, d->B, d->n, coef, dz1, ldd1, (const float*)w.blocksums, (int)P.tiles,
                     1.f / (float)d->B, means, tick_counter);
  return launch_status("clica_dot_loss_bwd_sym_train");
}
