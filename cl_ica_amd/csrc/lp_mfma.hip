// LpSimCLRLoss with p = 2 (pow) on the bf16 matrix cores: the pair sweeps of the TRAINING entry points
// (clica_lp_loss_fwd_train / clica_lp_loss_bwd_sym_train, /root/reference/losses.py:430-477 with main_mlp.py:272's z3 = roll(z1))
// for n <= 10.
//
// Why this is matrix work.  With x' = sqrt(2 log2(e) / tau) (x - origin) the scaled logit of a pair is
//     x_ij = -log2(e)/tau |a_i - p_j|^2 = a'_i . p'_j - |a'_i|^2 / 2 - |p'_j|^2 / 2,
// i.e. ONE inner product of the augmented rows  (a', -|a'|^2/2, 1) . (p', 1, -|p'|^2/2)  -- n + 6 <= 16 feature slots with the norms in pieces, the K of a
// v_mfma_f32_32x32x16_bf16 -- and the symmetric backward is
//     dz_i = 2 sum_j 2^x_ij (u_i + u_j) (a_i - p_j) = (2 / s) [ u_i (a'_i W1_i - T1_i) + (a'_i W2_i - T2_i) ],
//     W1_i = sum_j e_ij,  T1_i = sum_j e_ij p'_j,  W2_i = sum_j e_ij u_j,  T2_i = sum_j e_ij u_j p'_j,   e_ij = 2^x_ij
// which is a second product E [P', 1, u P', u] (n + 1 feature rows and their u_j-weighted copies: 2 (n + 1) <= 32 rows of ONE MFMA operand):
// the structure of flash attention with K = V = the pool.  The VALU
// sweeps (lp_kernels.h) spend ~22 (forward) / ~26 (backward) issue slots per pair at n = 10, 10 + 10 of them on the differences and
// their squares / the gradient FMAs; here a pair costs its exponential (v_exp_f32, quarter rate), one add (forward) or the coefficient
// and a two-piece bf16 split (backward), the rest runs on the matrix pipe next to it.
//
// Arithmetic.  The three terms of the expansion are of the size of M = log2(e)/tau |x - origin|^2 each and their sum is the (possibly much
// smaller) negated scaled squared distance, and the reference's training lives at M ~ 10^3 (unnormalised encoder outputs).  The large part
// of every term is therefore computed exactly -- hi pieces on a grid common to the launch, hi x hi in an accumulator of its own, see "planes"
// below -- and the remainders' seven piece products carry terms of size M / 256; rows are shifted by an origin inside the data (the pool's
// first row; distances do not change).  The exponential e_ij enters the second product as hi + mid bf16 pieces, both rounded to nearest
// (relative error <= 2^-18 per pair, unbiased), against three exact pieces of the pool features (u_j p'_j rounded once to fp32, then split
// exactly): five products.  The W sums come out of the same product (ones / u columns), so the e_ij that weigh a'_i and p'_j are the same
// numbers and the self pair cancels exactly.  Parity is measured, not assumed: tests/test_gpu_loss.py compares these sweeps with the fp64
// oracle at the bench sizes and over spreads up to M = 15 000; CLICA_LP_MFMA=0 keeps the VALU sweeps.
//
// Layout.  A prep launch writes the planes once per step, already in MFMA operand order, so staging is a linear copy and an operand is
// one 16-byte LDS read:  row planes [tile of 32 rows][piece][k half][row] x 8 bf16 (operand of the logit product, for the anchors and
// for the pool) and the pool's feature planes [tile][piece][mfma 0/1][k half][feature slot < 32] x 8 bf16 (slots 0..n: p', 1; slots
// 16..16+n: the same times u_j -- written by the backward call, which knows u), element e = pool row
// 16 t + 8 (e / 4) + 4 h + e % 4 of the tile -- the order in which a lane of the logit block holds its 16 results, so that the
// coefficients go into the second product's B operand from the registers they were computed in (no LDS round trip, no shuffles).
// A wave owns T x 32 anchors (lane l and l + 32: the same anchor, different pool rows), a workgroup four waves, the pool is cut into
// HBM-level splits of whole stages; partial formats are those of fwd_partial_k<ZMAX> / bwd_pairs_k<FOLD>, finalize / reduce are shared.
#include "lp_mfma.h"
#include "lp_mfma_dev.h"
#include "lp_kernels.h"
#include <math.h>
#include <stdlib.h>
#include <type_traits>

namespace clica {
namespace lp2 {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256, WAVES = 4;
constexpr int STAGE_B = 2;            // pool tiles per LDS stage of the backward sweep (its stage also holds the feature planes)
static_assert(STAGE_TILES % STAGE_B == 0, "chunks are whole stages of both sweeps");

__device__ __forceinline__ float fexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// two fp32 -> packed bf16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}
#ifndef LP2_ABLATE
#define LP2_ABLATE 0      // measurement builds only (make variant EXTRA=-DLP2_ABLATE=k): 1 = no MFMAs, 2 = no vector work in the backward block
#endif
__device__ __forceinline__ f32x16 mfma(u32x4 a, u32x4 b, f32x16 c) {
#if LP2_ABLATE & 1
  c[0] += __uint_as_float((a.x ^ b.x) & 1u);
  return c;
#else
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
#endif
}
// eight piece products: hi x hi -- exact, see the planes -- in an accumulator of its own, the other seven (all but lo x lo) in a second one
__device__ __forceinline__ f32x16 logit_block(const u32x4 (&a)[3], const u32x4 (&b)[3]) {
  f32x16 acc, acch;
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc[r] = 0.f; acch[r] = 0.f; }
  acc = mfma(a[2], b[1], acc);
  acch = mfma(a[0], b[0], acch);
  acc = mfma(a[1], b[2], acc);
  acc = mfma(a[2], b[0], acc);
  acc = mfma(a[0], b[2], acc);
  acc = mfma(a[1], b[1], acc);
  acc = mfma(a[1], b[0], acc);
  acc = mfma(a[0], b[1], acc);
  return acc + acch;
}

// ---- planes ---------------------------------------------------------------------------------------------------------------------
// The expansion's enemy is the size of its terms: a'.p' and the two half norms are ~M = log2(e)/tau |x - origin|^2 each, their sum is the
// logit, and an fp32 accumulator that has held a number of size M carries 2^-24 M of rounding -- 6e-5 of relative error in the weights at
// M = 1000, which is where the reference's own training lives (unnormalised encoder outputs grow to a standard deviation of ~10 within a
// thousand steps of main_mlp.py's defaults).  So the LARGE part is made exact: the hi piece of every coordinate is a multiple of one grid
// step D = 2^e for the whole launch (|x'| / D < 256 from the step's own max |x'|, maxabs_k), its half norm Nh = sum hi^2 / 2 goes into
// three slots of the hi plane as an exact three-piece split, and the hi x hi product runs into an accumulator of its own: every partial
// sum is an integer multiple of D^2 / 2 below 2^24 of them, i.e. exact, and the result -|hi_a - hi_p|^2 / 2 is small wherever the pair
// matters.  The other SEVEN piece products (hi / mid / lo against each other except lo x lo: the remainder r = x' - hi, |r| <= D / 2, is not
// small against hi the way a plain split's second piece is, so mid x lo counts) carry terms of size M / 256 and the remainder norms
// Nr = sum (hi r + r^2 / 2) in a second accumulator; the two are added on the vector ALU.  Measured: section "spread" of the tests.
// Slots (K = 16 = n + 6, n <= 10): coordinates 0..n-1; pool rows: ones at n..n+2, own norms at n+3..n+5; anchors the other way round;
// own norm slots: hi plane = the three pieces of -Nh, mid plane = the three pieces of -Nr; rows >= `rows` of the pool: -Nr = -1e30.
constexpr int PREP_TILES = 8;                         // tiles (32 rows each) per prep workgroup: 4 waves x 2
__global__ __launch_bounds__(256) void prep_k(const float* __restrict__ Xp, int64_t ldp, int64_t rows_p, u32x4* __restrict__ RPp, int pool_blocks,
                                              int pool_tiles, const float* __restrict__ Xa, int64_t lda, int64_t rows_a, u32x4* __restrict__ RPa,
                                              int own_tiles, int n, float pre2, float* __restrict__ words) {
  // one launch for both operands: blocks [0, pool_blocks) the pool (role 0), the rest the anchors (role 1); PREP_TILES tiles per block.
  // (Round 5: 256 rows and TWO atomics per workgroup.  With one wave per workgroup and four same-line atomics each -- 768 of them at
  //  B = 6144, serialised in one L2 channel -- the launch took 17 us; the arithmetic is a few hundred instructions per row.)
  const int role = (int)blockIdx.x >= pool_blocks ? 1 : 0;
  // the grid of THIS call (measured by the previous one, lp_mfma.h) and, for the next call, the mean of the pool's first <= 64 rows --
  // computed by every workgroup the same way (one wave, fixed shuffle tree: identical everywhere), so that each can measure ITS rows
  // against the next origin
  const unsigned call = reinterpret_cast<const unsigned*>(words)[W_CALL];
  const float* __restrict__ origin = words + W_ORIGIN_CUR;
  float onext = 0.f;                                   // lane k < n: coordinate k of the next origin
  {
    // (all MAX_N loads in flight before the first shuffle: as a loop over n with a load + six shuffles per turn this was ten
    //  dependent memory round trips in front of every workgroup's real work -- 17 us for the launch, profiles/r5_summary.md)
    const int lane64 = threadIdx.x & 63;           // (every wave for itself: no barrier in front of the real work)
    const int cnt = rows_p < 64 ? (int)rows_p : 64;
    float v[MAX_N];
#pragma unroll
    for (int k = 0; k < MAX_N; ++k) v[k] = (lane64 < cnt && k < n) ? Xp[(int64_t)lane64 * ldp + k] : 0.f;
#pragma unroll
    for (int k = 0; k < MAX_N; ++k) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
      if (lane64 == k) onext = v[k] / (float)cnt;
    }
  }
  if (blockIdx.x == 0 && (int)threadIdx.x < KSLOTS) {
    words[W_ORIGIN_USED + threadIdx.x] = (int)threadIdx.x < n ? origin[threadIdx.x] : 0.f;      // (nobody reads USED before the next kernel)
    words[W_ORIGIN_NEXT + threadIdx.x] = (int)threadIdx.x < n ? onext : 0.f;
  }
  const float* __restrict__ X = role ? Xa : Xp;
  const int64_t ldx = role ? lda : ldp, rows = role ? rows_a : rows_p;
  u32x4* __restrict__ RP = role ? RPa : RPp;
  const int tile = ((int)blockIdx.x - (role ? pool_blocks : 0)) * PREP_TILES + (threadIdx.x >> 5), lane = threadIdx.x & 31;
  const bool tile_ok = tile < (role ? own_tiles : pool_tiles);
  // grid step: the power of two with max |x'| / D in [64, 128)
  const unsigned xb = __float_as_uint(words[W_MAXABS_CUR] * 1.03125f);      // (a 3 % margin: a cloud that merely breathes does not cross the power of two)
  const int ex = (int)((xb >> 23) & 0xffu) - 7;      // biased exponent of max |x'|, minus 7: max / D in [128, 256), hi = 8-bit integers x D
  const float D = __uint_as_float((unsigned)(ex < 1 ? 1 : ex) << 23), invD = 1.f / D;
  const int64_t j = (int64_t)tile * ROWS + lane;
  const bool live = tile_ok && j < rows;
  unsigned hb[KSLOTS], mb[KSLOTS], lb[KSLOTS];
  float nh = 0.f, nr = 0.f, amax = 0.f, amax_next = 0.f;
#pragma unroll
  for (int k = 0; k < MAX_N; ++k) {
    const bool ok = live && k < n;
    const float xv = X[ok ? j * ldx + k : 0];
    const float xr = pre2 * (xv - origin[k < n ? k : 0]);
    const float x = ok ? xr : 0.f;
    amax = fmaxf(amax, fabsf(x));
    amax_next = fmaxf(amax_next, ok ? fabsf(pre2 * (xv - __shfl(onext, k, 64))) : 0.f);
    const float hi = __uint_as_float(__float_as_uint(rintf(x * invD) * D) & 0xffff0000u);      // a multiple of D with <= 8 significant bits
    const float r = x - hi;
    const unsigned mbits = __float_as_uint(r) & 0xffff0000u;
    const float r2 = r - __uint_as_float(mbits);
    const unsigned lbits = __float_as_uint(r2) & 0xffff0000u;
    hb[k] = __float_as_uint(hi) >> 16; mb[k] = mbits >> 16; lb[k] = lbits >> 16;
    // the remainder as the product sees it (16 bits: what is cut off is below 2^-24 of the launch's largest coordinate); the norm must be
    // the norm of THESE numbers, or hi x (cut-off part) -- 5e-5 at M = 900 -- stays in every logit, the self pair's included
    const float r16 = __uint_as_float(mbits) + __uint_as_float(lbits);
    nh = fmaf(hi, hi, nh);
    nr += fmaf(hi, r16, 0.5f * r16 * r16);
  }
  nh *= 0.5f;
  {      // M of this call (the guard: anchors and pool rows both enter the expansion), the grid check, the next call's max |x'|
    __shared__ float red[3][4];
    float m = live ? nh + nr : 0.f;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      m = fmaxf(m, __shfl_xor(m, off, 64)); amax = fmaxf(amax, __shfl_xor(amax, off, 64)); amax_next = fmaxf(amax_next, __shfl_xor(amax_next, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = m; red[1][threadIdx.x >> 6] = amax; red[2][threadIdx.x >> 6] = amax_next; }
    __syncthreads();
    if (threadIdx.x == 0) {
      m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
      amax = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
      amax_next = fmaxf(fmaxf(red[2][0], red[2][1]), fmaxf(red[2][2], red[2][3]));
      const unsigned long long tag = (unsigned long long)call << 32;
      unsigned long long* w64 = reinterpret_cast<unsigned long long*>(words);
      // A row up to 2 x beyond the grid is still exact: its hi piece is cut to 8 significant bits, i.e. lands on the 2 D grid (sums of
      // products of integers < 512 stay below 2^24 multiples of D^2 / 2), only its remainder is up to D instead of D / 2.  Violation =
      // beyond that (the cloud more than doubled since the last call; the very first call), or non-finite rows.  (With the check at 256 a
      // 300 000-step run fell back on 8 % of its calls -- the cloud's max |x'| breathing across a power of two -- profiles/r5_long_run_*.)
      const bool viol = !(amax * invD < 512.f) || !(m <= 3.0e38f);
      atomicMax(w64 + W_M64 / 2, tag | (unsigned long long)__float_as_uint(fminf(fmaxf(m, 0.f), 3.0e38f)));      // every workgroup: the tag of W_M64 IS this call's id
      if (viol) atomicMax(w64 + W_V64 / 2, tag | 1ull);                                                            // (read against that tag: guard_falls_back)
      atomicMax(reinterpret_cast<int*>(words + W_MAXABS_NEXT), __float_as_int(fminf(amax_next, 3.0e38f)));
    }
  }
  unsigned nhp[3], nrp[3];
  split3(-nh, nhp[0], nhp[1], nhp[2]);
  split3((role == 0 && !live) ? -1e30f : -nr, nrp[0], nrp[1], nrp[2]);
  const int own0 = role == 0 ? n + 3 : n, one0 = role == 0 ? n : n + 3;
#pragma unroll
  for (int k = 0; k < KSLOTS; ++k) {
    const int o = k - own0, u = k - one0;
    if (k >= n) {
      const bool isown = o >= 0 && o < 3, isone = u >= 0 && u < 3;
      hb[k] = isown ? (o == 0 ? nhp[0] : (o == 1 ? nhp[1] : nhp[2])) : (isone ? 0x3f80u : 0u);
      mb[k] = isown ? (o == 0 ? nrp[0] : (o == 1 ? nrp[1] : nrp[2])) : 0u;
      lb[k] = 0u;
    }
  }
  if (!tile_ok) return;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    unsigned t8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t8[e] = hb[8 * h + e];
    RP[((int64_t)(tile * 3 + 0) * 2 + h) * ROWS + lane] = pack8(t8);
#pragma unroll
    for (int e = 0; e < 8; ++e) t8[e] = mb[8 * h + e];
    RP[((int64_t)(tile * 3 + 1) * 2 + h) * ROWS + lane] = pack8(t8);
#pragma unroll
    for (int e = 0; e < 8; ++e) t8[e] = lb[8 * h + e];
    RP[((int64_t)(tile * 3 + 2) * 2 + h) * ROWS + lane] = pack8(t8);
  }
}

// the pool's feature planes (operand of the gradient product): slot f < 16: y_f = (p'_0 .. p'_{n-1}, 1, 0 ..), slot 16 + f: u_j y_f
__global__ __launch_bounds__(128) void prep_feat_k(const float* __restrict__ X, int64_t ldx, int64_t rows, int n, const float* __restrict__ origin,
                                                   float pre2, const float* __restrict__ poolL, const float* __restrict__ poolC,
                                                   u32x4* __restrict__ FP) {
  const int id = threadIdx.x;
  feat_vectors((int64_t)blockIdx.x, id >> 6, (id >> 5) & 1, id & 31, rows, n, origin, pre2,
               [&](int64_t j, int f) { return X[j * ldx + f]; },
               [&](int64_t j) { return poolC[j] * fexp2(-poolL[j]); }, FP);
}

// Both sweeps are software pipelines over "blocks" (one pool tile x one anchor tile = 1024 pairs): the matrix pipe works on block q
// (and, in the backward, on the gradient product of block q - 2) while the vector ALU turns block q - 1's logits into exponentials /
// coefficient pieces.  Left to itself the compiler issues all MFMAs of a stage, then all exponentials (measured: 660 cycles per block
// and SIMD where the exponentials alone need 290).  The state that crosses a block boundary lives in registers, so the skew also
// crosses the stage barrier; before the first block it is "logits = -1e30, pieces = 0" (contributes exact zeros).
#define LP2_SCHED_PAIR(nvalu) do { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x402, nvalu, 0); } while (0)

// Workgroup -> (anchor group, pool split).  Consecutive workgroup ids go to consecutive XCDs (8 of them, each with its own 4 MB L2), and
// the planes of a 49 152-row pool are 9.4 MB: with the natural mapping every XCD walks the WHOLE pool and every stage comes from the
// Infinity Cache (~2 us; a workgroup keeps one stage in flight, so the sweep ran at 14 B/clk/CU of staging -- measured with the
// arithmetic ablated: 65 of the backward's 150 us).  Remapped, XCD x owns the logical ids [x N / 8, (x + 1) N / 8): all anchor
// groups of a FEW splits, whose chunks (432 KB each) stay in that XCD's L2 after the first workgroup touched them.
__device__ __forceinline__ void xcd_tile(const unsigned id, const unsigned gx, const unsigned gy, int& bx, int& by) {
  const unsigned n = gx * gy;
  const unsigned m = n & ~7u;                   // ids beyond the last multiple of 8 keep their place
  const unsigned logical = id < m ? (id & 7u) * (m >> 3) + (id >> 3) : id;
  by = (int)(logical / gx); bx = (int)(logical - (unsigned)by * gx);
}

// ---- forward: sum_j 2^x_ij per anchor and split -------------------------------------------------------------------------------
// The guard's fallback rides in the SAME launch (round 5; as a launch of its own behind this one it cost ~5 us per sweep even when
// it had nothing to do): a 1-D grid of max(matrix-core workgroups, difference-sweep workgroups); every workgroup reads the guard
// words and runs one sweep or the other.  The difference sweep is lp_kernels.h's fwd_partial_k / bwd_pairs_k body, instantiated
// here for the p = 2 training variants (fixed maximum / folded coefficient) of the three padded widths n <= 10 takes.
struct ValuSweep {
  const float* own; int64_t ldo, n_own; const float* str; int64_t lds, n_str; lp::Params q; int chunk, gx, gy;
  const float* ownL; const float* ownC; const float* strL; const float* strC;      // backward only
};
template <int T, int NP, int NQ>
__global__ __launch_bounds__(THREADS, 2) void fwd_k(const u32x4* __restrict__ RPa, const u32x4* __restrict__ RPp, int64_t n_own,
                                                    float2* __restrict__ part, int chunk_tiles, float* __restrict__ words, float limit,
                                                    const unsigned mgx, const unsigned mgy, const ValuSweep v) {
  constexpr int SV = STAGE_TILES * ROWVEC, PER = SV / THREADS;       // 768 vectors per stage, 3 per thread
  static_assert(SV % THREADS == 0, "stage copy");
  __shared__ u32x4 stage[2][SV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
  // The guard words come from memory another XCD wrote a moment ago (~2 us): they are requested FIRST, the matrix-core path's own first
  // loads (anchor fragments, first pool stage) go out behind them, and only then does the workgroup branch on the answer.
  const bool fall_back = guard_falls_back(words, limit);
  int bx, by;
  xcd_tile(blockIdx.x < mgx * mgy ? blockIdx.x : 0u, mgx, mgy, bx, by);
  const int64_t atile0 = ((int64_t)bx * WAVES + wave) * T;
  u32x4 b[T][3];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int p = 0; p < 3; ++p) b[t][p] = RPa[(((atile0 + t) * 3 + p) * 2 + h) * ROWS + l31];
  const u32x4* src = RPp + (int64_t)by * chunk_tiles * ROWVEC;
  u32x4 pre[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) pre[u] = src[threadIdx.x + u * THREADS];
  if (blockIdx.x == 0 && threadIdx.x < 64) {      // the planes are written: hand the next call its grid (lp_mfma.h)
    if (threadIdx.x < KSLOTS) words[W_ORIGIN_CUR + threadIdx.x] = words[W_ORIGIN_NEXT + threadIdx.x];
    if (threadIdx.x == 0) {
      words[W_MAXABS_CUR] = words[W_MAXABS_NEXT]; words[W_MAXABS_NEXT] = 0.f;
      reinterpret_cast<unsigned*>(words)[W_CALL] += 1u;
      if (!guard_violated(words)) words[W_RUN_M] = fmaxf(words[W_RUN_M], words[W_M64]);      // (a call without a grid measures M against a stale origin)
    }
  }
  if (fall_back) {                                  // the guard (lp_mfma.h): this call runs on the coordinate differences
    if (blockIdx.x < (unsigned)(v.gx * v.gy))
      lp::fwd_partial_body<NP, 2, lp::owners_fwd(NP), false, false, NQ, true>(v.own, v.ldo, v.n_own, v.str, v.lds, v.n_str, v.q, part, nullptr, v.chunk,
                                                                             (int)(blockIdx.x % (unsigned)v.gx), (int)(blockIdx.x / (unsigned)v.gx));
    return;
  }
  if (blockIdx.x >= mgx * mgy) return;
  float s[T];
#pragma unroll
  for (int t = 0; t < T; ++t) s[t] = 0.f;
  const int nst = chunk_tiles / STAGE_TILES;
#pragma unroll
  for (int u = 0; u < PER; ++u) stage[0][threadIdx.x + u * THREADS] = pre[u];
  __syncthreads();
  f32x16 accP;                      // logits of the previous block, not yet exponentiated
#pragma unroll
  for (int r = 0; r < 16; ++r) accP[r] = -1e30f;
  auto finish = [&](int t) {        // block q - 1: sixteen exponentials into its anchor tile's sum
    float add = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) add += fexp2(accP[r]);
    s[t] += add;
  };
  int cur = 0;
  for (int st = 0; st < nst; ++st, cur ^= 1) {
    const bool more = st + 1 < nst;
    if (more) {
#pragma unroll
      for (int u = 0; u < PER; ++u) pre[u] = src[(int64_t)(st + 1) * SV + threadIdx.x + u * THREADS];
    }
    u32x4 a[3];
#pragma unroll
    for (int q = 0; q < STAGE_TILES * T; ++q) {
      const int tl = q / T, t = q % T;
      if (t == 0) {
#pragma unroll
        for (int p = 0; p < 3; ++p) a[p] = stage[cur][((tl * 3 + p) * 2 + h) * ROWS + l31];
      }
      __builtin_amdgcn_sched_barrier(0);          // one scheduling region per block: the MFMAs of q with the exponentials of q - 1
      f32x16 accN = logit_block(a, b[t]);
      finish((q + T - 1) % T);
      // (pure instructions carry no order towards the region fences: tie both results to this point of the program)
      asm volatile("" : "+v"(accN), "+v"(s[(q + T - 1) % T]));
      accP = accN;
#pragma unroll
      for (int i = 0; i < 6; ++i) LP2_SCHED_PAIR(4);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (more) {
#pragma unroll
      for (int u = 0; u < PER; ++u) stage[cur ^ 1][threadIdx.x + u * THREADS] = pre[u];
    }
    __syncthreads();
  }
  finish(T - 1);
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const float so = __shfl_xor(s[t], 32, 64);
    const float tot = h ? so + s[t] : s[t] + so;
    const int64_t i = (atile0 + t) * ROWS + l31;
    if (h == 0 && i < n_own) part[(int64_t)by * n_own + i] = make_float2(0.f, tot);
  }
}

// ---- symmetric backward: (2 / s) (a'_i W_i - T_i) per anchor and split --------------------------------------------------------
template <int T, int NP, int NQ>
__global__ __launch_bounds__(THREADS, 2) void bwd_k(const u32x4* __restrict__ RPa, const u32x4* __restrict__ RPp, const u32x4* __restrict__ FPp,
                                                    const float* __restrict__ own, int64_t ldo, int64_t n_own,
                                                    const float* __restrict__ origin, int64_t n_pool, int n, int np, float pre2,
                                                    const float* __restrict__ ownL, const float* __restrict__ ownC,
                                                    float* __restrict__ part, int chunk_tiles, const float* __restrict__ words, float limit,
                                                    const unsigned mgx, const unsigned mgy, const ValuSweep v) {
  const bool fall_back = guard_falls_back(words, limit);      // requested first, consumed behind the path's own first loads (see fwd_k)
  constexpr int RV = STAGE_B * ROWVEC, FV = STAGE_B * FEATVEC, SV = RV + FV, PER = (SV + THREADS - 1) / THREADS;      // 384 + 768 vectors
  constexpr int NB = STAGE_B * T;                                                                    // blocks per stage
  static_assert(RV % 64 == 0 && SV % 64 == 0, "stage copy: whole waves on either side of the row / feature boundary");
  constexpr int LV = SV;        // LDS image of a stage: [row planes of STAGE_B tiles][feature planes of STAGE_B tiles], a linear copy
  __shared__ u32x4 stage[2][LV];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
  int bx, by;
  xcd_tile(blockIdx.x < mgx * mgy ? blockIdx.x : 0u, mgx, mgy, bx, by);
  const int64_t atile0 = ((int64_t)bx * WAVES + wave) * T;
  u32x4 b[T][3];
  float ui[T], Lrow[T], Crow[T];
  f32x16 G[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
#pragma unroll
    for (int p = 0; p < 3; ++p) b[t][p] = RPa[(((atile0 + t) * 3 + p) * 2 + h) * ROWS + l31];
    const int64_t i = (atile0 + t) * ROWS + l31;
    const bool ok = i < n_own;
    Lrow[t] = ownL[ok ? i : 0]; Crow[t] = ok ? ownC[i] : 0.f;
  }
  if (fall_back) {                                  // the guard (lp_mfma.h): this call runs on the coordinate differences
    if (blockIdx.x < (unsigned)(v.gx * v.gy))
      lp::bwd_pairs_body<NP, 2, lp::owners_bwd(NP), 3, false, NQ, true>(v.own, v.ldo, v.n_own, v.str, v.lds, v.n_str, v.q, v.ownL, v.ownC, v.strL, v.strC,
                                                                       part, v.chunk, (int)(blockIdx.x % (unsigned)v.gx), (int)(blockIdx.x / (unsigned)v.gx));
    return;
  }
  if (blockIdx.x >= mgx * mgy) return;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    ui[t] = Crow[t] * fexp2(-Lrow[t]);
#pragma unroll
    for (int r = 0; r < 16; ++r) G[t][r] = 0.f;
  }
  const int64_t tile_b = (int64_t)by * chunk_tiles;
  const u32x4* srcR = RPp + tile_b * ROWVEC;
  const u32x4* srcF = FPp + tile_b * FEATVEC;
  const int nst = chunk_tiles / STAGE_B;
  // A stage's LDS image holds the row planes of ITS tiles and the feature planes of the tiles whose gradient product runs during it --
  // the pipeline is two blocks behind, i.e. BACK tiles earlier -- so that every read of a stage goes to the buffer the barrier in front
  // of it has completed.  (The first version read those feature planes from the previous stage's buffer, which a faster wave was already
  // refilling: a race that showed as run-to-run differences of 1e-3 of the gradient scale once the waves drifted apart.)  Tile indices
  // outside the chunk (the window of the first stage, the S-less last stage) are clamped: their coefficient pieces are exact zeros.
  constexpr int BACK = T == 1 ? 2 : 1;
  auto fetch = [&](int st, u32x4 (&pre)[PER]) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = threadIdx.x + u * THREADS;
      if (idx < RV) {
        pre[u] = srcR[(int64_t)(st < nst ? st : nst - 1) * RV + idx];
      } else if (idx < SV) {
        const int fi = idx - RV, tl = fi / FEATVEC;
        int tile = st * STAGE_B - BACK + tl;
        tile = tile < 0 ? 0 : (tile > chunk_tiles - 1 ? chunk_tiles - 1 : tile);
        pre[u] = srcF[(int64_t)tile * FEATVEC + (fi - tl * FEATVEC)];
      }
    }
  };
  auto put = [&](int bsel, const u32x4 (&pre)[PER]) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int idx = threadIdx.x + u * THREADS;
      if (idx < SV) stage[bsel][idx] = pre[u];
    }
  };
  u32x4 pre[PER];
  fetch(0, pre);
  put(0, pre);
  __syncthreads();
  // pipeline state: logits of block q - 1 (awaiting the vector work), coefficient pieces of block q - 2 (awaiting the gradient product)
  f32x16 accP;
  unsigned hpP[8], mpP[8];
#pragma unroll
  for (int r = 0; r < 16; ++r) accP[r] = -1e30f;
#pragma unroll
  for (int e = 0; e < 8; ++e) { hpP[e] = 0u; mpP[e] = 0u; }
  // One block of the pipeline, issued in a fixed interleave (the wave issues in order: an MFMA behind an MFMA waits for the matrix pipe,
  // vector work behind it then waits too -- left to the scheduler the 16 MFMAs of a block go first and nothing overlaps, measured
  // 1040 cycles per block for 512 + 512).  Eight steps; step e: one MFMA, the two exponentials of coefficient pair e, a second MFMA, the
  // rest of pair e (coefficient, hi + mid bf16 pieces, both rounded to nearest, packed in B-operand order).  MFMA list: the six logit
  // products of block q (S) and the ten gradient products of block q - 2 (G), two independent accumulation chains, alternating.
  // `pin` ties a value to a point of the program (pure instructions carry no order towards the sched_barrier fences by themselves).
#define LP2_PIN1(x) asm volatile("" : "+v"(x))
#define LP2_FENCE() __builtin_amdgcn_sched_barrier(0)
  auto block = [&](const u32x4 (&a)[3], const u32x4 (&bt)[3], bool do_s, f32x16& accN,       /* S: logits of block q */
                   const f32x16& accV, unsigned (&hpN)[8], unsigned (&mpN)[8],                                /* V: block q - 1 */
                   f32x16& Gt, int bufG, int tlG, const unsigned (&hpG)[8], const unsigned (&mpG)[8]) {          /* G: block q - 2 */
    u32x4 fa[2][3];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int p = 0; p < 3; ++p) fa[tt][p] = stage[bufG][RV + (((tlG * 3 + p) * 2 + tt) * 2 + h) * 32 + l31];
    const u32x4 bh0 = {hpG[0], hpG[1], hpG[2], hpG[3]}, bm0 = {mpG[0], mpG[1], mpG[2], mpG[3]};
    const u32x4 bh1 = {hpG[4], hpG[5], hpG[6], hpG[7]}, bm1 = {mpG[4], mpG[5], mpG[6], mpG[7]};
    constexpr int NS = 8;
    constexpr int SA[NS] = {2, 0, 1, 2, 0, 1, 1, 0}, SB[NS] = {1, 0, 2, 0, 2, 1, 0, 1};        // logit piece products ((hi, hi) second: its own accumulator)
#ifndef LP2_GPROD
#define LP2_GPROD 5      // piece products of the gradient per K = 16 half: 5 = (mid, mid), (hi, mid), (lo, hi), (mid, hi), (hi, hi); 4 = without (mid, mid):
                         // measured -6 % sweep time, but the gradient at tau = 0.1 goes from 3e-6 to 1.2e-5 against the oracle -- not taken
#endif
    constexpr int NGH = LP2_GPROD, NG = 2 * NGH, NM = NGH - 3;                   // NM products take the mid piece of e
    constexpr int GA5[5] = {1, 0, 2, 1, 0}, GA4[4] = {0, 2, 1, 0};
#ifndef LP2_PRIO
#define LP2_PRIO 0       // measurement switch: 1 = s_setprio 1 around every MFMA issue (measured: 146 -> 168 us at the 49 152-row pool), 2 = around the vector work (150 -> 171 us): per-instruction priority flips cost more than the arbitration they buy
#endif
    auto gstep = [&](int i) {                                                     // i-th of the NG gradient products
      if (i >= NG) return;
      const int tt = i / NGH, k = i % NGH;
      const u32x4 bb = tt == 0 ? (k < NM ? bm0 : bh0) : (k < NM ? bm1 : bh1);
      if (LP2_PRIO) __builtin_amdgcn_s_setprio(LP2_PRIO == 1 ? 1 : 0);
      Gt = mfma(fa[tt][NGH == 5 ? GA5[k] : GA4[k]], bb, Gt);
      LP2_PIN1(Gt);
      if (LP2_PRIO) __builtin_amdgcn_s_setprio(LP2_PRIO == 1 ? 0 : 1);
    };
    f32x16 accH;                 // the exact hi x hi product of block q (see the planes), added to the other five at the end
    if (do_s) {
#pragma unroll
      for (int r = 0; r < 16; ++r) { accN[r] = 0.f; accH[r] = 0.f; }
    }
    // MFMA list of a block: S0 G0 S1 G1 .. S7 G7 G8 G9 (two independent chains alternating); step e issues entries 2e and 2e + 1, the
    // last two steps one more each
    auto sstep = [&](int i) {
      if (!do_s) return;
      if (LP2_PRIO) __builtin_amdgcn_s_setprio(LP2_PRIO == 1 ? 1 : 0);
      if (SA[i] == 0 && SB[i] == 0) { accH = mfma(a[0], bt[0], accH); LP2_PIN1(accH); }
      else { accN = mfma(a[SA[i]], bt[SB[i]], accN); LP2_PIN1(accN); }
      if (LP2_PRIO) __builtin_amdgcn_s_setprio(LP2_PRIO == 1 ? 0 : 1);
    };
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      sstep(e);
#if LP2_ABLATE & 2
      float e0 = accV[2 * e], e1 = accV[2 * e + 1];
#else
      float e0 = fexp2(accV[2 * e]), e1 = fexp2(accV[2 * e + 1]);
#endif
      LP2_PIN1(e0); LP2_PIN1(e1);
      LP2_FENCE();
      gstep(e);
      if (e >= 6) gstep(8 + (e - 6));
#if LP2_ABLATE & 2
      hpN[e] = __float_as_uint(e0);
      mpN[e] = __float_as_uint(e1);
#else
      hpN[e] = cvt_pk_bf16(e0, e1);
      const float r0 = e0 - __uint_as_float(hpN[e] << 16), r1 = e1 - __uint_as_float(hpN[e] & 0xffff0000u);
      mpN[e] = cvt_pk_bf16(r0, r1);
#endif
      LP2_PIN1(hpN[e]); LP2_PIN1(mpN[e]);
      LP2_FENCE();
    }
    if (do_s) accN = accN + accH;
  };
  int cur = 0;
  auto run_stage = [&](auto s_tag) {
    constexpr bool DO_S = decltype(s_tag)::value;
    u32x4 a[3];
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int tl = q / T, t = q % T;
      const int q2 = (q + NB - 2) % NB;          // block q - 2: its anchor tile is q2 % T, its feature planes sit at window index ...
      const int tlG = (q - 2 + BACK * T) / T;
      if (DO_S && t == 0) {
#pragma unroll
        for (int p = 0; p < 3; ++p) a[p] = stage[cur][((tl * 3 + p) * 2 + h) * ROWS + l31];
      }
      LP2_FENCE();
      f32x16 accN;
      unsigned hpN[8], mpN[8];
      block(DO_S ? a : b[t], b[t], DO_S, accN, accP, hpN, mpN, G[q2 % T], cur, tlG, hpP, mpP);
      if (!DO_S) {
#pragma unroll
        for (int r = 0; r < 16; ++r) accN[r] = -1e30f;
      }
      accP = accN;
#pragma unroll
      for (int e = 0; e < 8; ++e) { hpP[e] = hpN[e]; mpP[e] = mpN[e]; }
    }
  };
  for (int st = 0; st < nst; ++st, cur ^= 1) {
    fetch(st + 1, pre);                            // (st + 1 == nst: the feature window of the S-less last stage)
    run_stage(std::true_type{});
    put(cur ^ 1, pre);
    __syncthreads();
  }
  run_stage(std::false_type{});                    // no new logits: the pipeline's last two blocks drain
  // ---- epilogue: lane (anchor l31, half h) holds feature slots (r & 3) + 8 (r >> 2) + 4 h of G^T: r < 8 the plain sums (T1_k, W1 in slot n),
  //      r >= 8 the u_j-weighted ones (T2_k in slot 16 + k, W2 in slot 16 + n) ----
  const int hn = (n >> 2) & 1, rn = (n & 3) + 4 * (n >> 3);      // where slot n lives (slot 16 + n: the same lane, register rn + 8)
  const float scale = 2.f / pre2;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    float w1 = 0.f, w2 = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) { w1 = r == rn ? G[t][r] : w1; w2 = r == rn ? G[t][r + 8] : w2; }
    const float W1 = __shfl(w1, l31 + 32 * hn, 64), W2 = __shfl(w2, l31 + 32 * hn, 64);
    const int64_t i = (atile0 + t) * ROWS + l31;
    if (i >= n_own) continue;
    float* dst = part + ((int64_t)by * n_own + i) * np;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
      const int k0 = 8 * g + 4 * h;
      if (k0 >= np) continue;
      f32x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int k = k0 + e;
        const bool ok = k < n;
        const float xa = pre2 * (own[ok ? i * ldo + k : i * ldo] - origin[ok ? k : 0]);
        o[e] = ok ? scale * (ui[t] * (xa * W1 - G[t][4 * g + e]) + (xa * W2 - G[t][8 + 4 * g + e])) : 0.f;
      }
      *reinterpret_cast<f32x4*>(dst + k0) = o;
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }

static float g_limit = 0.f;     // <= 0: CLICA_LP_MFMA_LIMIT / the default
void set_spread_limit(float m) { g_limit = m > 0.f ? m : 0.f; }
float spread_limit() {
  static const float env_limit = [] { const char* e = getenv("CLICA_LP_MFMA_LIMIT"); const float v = e ? (float)atof(e) : 0.f; return v > 0.f ? v : kDefaultSpreadLimit; }();
  return g_limit > 0.f ? g_limit : env_limit;
}

// 0: never; 1 (the default): only where the negatives pool is at least four times the local rows (the gathered pool of a data-parallel
// job); 2: whatever the pool.  Round 6: at the reference's own spread (M ~ 511) the gradient of the matrix-core sweeps
// measures 6.4e-6 of its 1e-5 budget where the coordinate-difference sweeps hold 2.1e-6, and at a local pool (B3 = B) the trade buys 13 us
// of a 350 us step -- so a single-rank step runs the difference sweeps (which is also what north_star describes: MFMA for the GEMMs, not
// for the Lp distance); at the 49 152-row pool of the 8-rank job the sweeps are ~40 % of the step and the matrix cores stay.
static int g_enabled = -1;      // -1: take CLICA_LP_MFMA (default 1); set_enabled overrides it for the process
void set_enabled(int on) { g_enabled = on < 0 ? -1 : (on > 2 ? 2 : on); }
static int mode() {
  static const int env_on = env_int("CLICA_LP_MFMA", 1);
  return g_enabled >= 0 ? g_enabled : env_on;
}
bool applies(int n, float p, int pow) { return mode() != 0 && p == 2.f && pow != 0 && n >= 1 && n <= MAX_N; }
bool applies_to_pool(int64_t n_own, int64_t n_pool) { return mode() >= 2 || (mode() == 1 && n_pool >= 4 * n_own); }

Plan make_plan(int64_t n_own, int64_t n_pool) {
  // anchor tiles per wave: measured (3 workgroups per CU) pool 6 144: T = 1 29 + 36 us, T = 2 31 + 43; pool 49 152: T = 1 71 + 146, T = 2 67 + 142
  // -> two tiles (half the pool reads per pair) once the pool is several times the local rows
  constexpr int wg_per_cu = 3;
  Plan P;
  P.T = n_pool >= 4 * n_own ? 2 : 1;
  const int64_t per_group = (int64_t)WAVES * P.T * ROWS;
  P.groups = ceil_div(n_own > 0 ? n_own : 1, per_group);
  P.own_tiles = P.groups * WAVES * P.T;
  const int64_t tiles = ceil_div(n_pool > 0 ? n_pool : 1, (int64_t)ROWS);
  int64_t ns = ceil_div((int64_t)kNumCU * wg_per_cu, P.groups);
  const int64_t cap = ceil_div(tiles, (int64_t)STAGE_TILES);
  if (ns > cap) ns = cap;
  if (ns < 1) ns = 1;
  const int64_t chunk = ceil_div(ceil_div(tiles, ns), (int64_t)STAGE_TILES) * STAGE_TILES;
  P.chunk_tiles = (int)chunk;
  P.nsplit = (int)ceil_div(tiles, chunk);
  P.pool_tiles = (int64_t)P.nsplit * chunk;
  return P;
}

Ws carve(void* base, const Plan& P) {
  Ws w; char* p = (char*)base; size_t off = 0;
  w.spread = (float*)(p + off); off += 256;
  w.own_rows = p + off; off += align_up((size_t)P.own_tiles * ROWVEC * 16, 256);
  w.pool_rows = p + off; off += align_up((size_t)P.pool_tiles * ROWVEC * 16, 256);
  w.pool_feat = p + off; off += align_up((size_t)P.pool_tiles * FEATVEC * 16, 256);
  w.bytes = off;
  return w;
}

void launch_prep(const Plan& P, const Ws& w, const float* own, int64_t ldo, int64_t n_own, const float* pool, int64_t ldp, int64_t n_pool,
                 int n, float kscale, hipStream_t st) {
  const float pre2 = sqrtf(2.f * kscale);
  const int pb = (int)ceil_div(P.pool_tiles, (int64_t)PREP_TILES), ob = (int)ceil_div(P.own_tiles, (int64_t)PREP_TILES);
  hipLaunchKernelGGL(prep_k, dim3((unsigned)(pb + ob)), dim3(256), 0, st, pool, ldp, n_pool, (u32x4*)w.pool_rows, pb, (int)P.pool_tiles,
                     own, ldo, n_own, (u32x4*)w.own_rows, (int)P.own_tiles, n, pre2, w.spread);
}

template <int T>
static void launch_fwd_T(const Plan& P, const Ws& w, int64_t n_own, float2* part, float limit, const ValuSweep& v, hipStream_t st) {
  const unsigned mg = (unsigned)(P.groups * P.nsplit), vg = (unsigned)(v.gx * v.gy);
  dim3 grid(mg > vg ? mg : vg), block(THREADS);
#define LP2_FWD(NPV, NQV) hipLaunchKernelGGL((fwd_k<T, NPV, NQV>), grid, block, 0, st, (const u32x4*)w.own_rows, (const u32x4*)w.pool_rows, n_own, part, \
                                             P.chunk_tiles, w.spread, limit, (unsigned)P.groups, (unsigned)P.nsplit, v)
  if (v.q.n <= 4) LP2_FWD(4, 2); else if (v.q.n <= 8) LP2_FWD(8, 4); else LP2_FWD(12, 5);
#undef LP2_FWD
}
void launch_fwd(const Plan& P, const Ws& w, int64_t n_own, float2* part, float limit, const lp::Plan& PV, const float* own, int64_t ldo,
                const float* pool, int64_t ldp, int64_t n_pool, const lp::Params& q, hipStream_t st) {
  ValuSweep v{own, ldo, n_own, pool, ldp, n_pool, q, PV.chunk, (int)PV.tiles, PV.nsplit, nullptr, nullptr, nullptr, nullptr};
  if (P.T == 1) launch_fwd_T<1>(P, w, n_own, part, limit, v, st); else launch_fwd_T<2>(P, w, n_own, part, limit, v, st);
}

template <int T>
static void launch_bwd_T(const Plan& P, const Ws& w, const float* own, int64_t ldo, int64_t n_own, int64_t n_pool, int n, int np, float pre2,
                         const float* ownL, const float* ownC, float* part, float limit, const ValuSweep& v, hipStream_t st) {
  const unsigned mg = (unsigned)(P.groups * P.nsplit), vg = (unsigned)(v.gx * v.gy);
  dim3 grid(mg > vg ? mg : vg), block(THREADS);
  const float* origin = w.spread + W_ORIGIN_USED;
#define LP2_BWD(NPV, NQV) hipLaunchKernelGGL((bwd_k<T, NPV, NQV>), grid, block, 0, st, (const u32x4*)w.own_rows, (const u32x4*)w.pool_rows, \
                                             (const u32x4*)w.pool_feat, own, ldo, n_own, origin, n_pool, n, np, pre2, ownL, ownC, part, P.chunk_tiles, \
                                             (const float*)w.spread, limit, (unsigned)P.groups, (unsigned)P.nsplit, v)
  if (n <= 4) LP2_BWD(4, 2); else if (n <= 8) LP2_BWD(8, 4); else LP2_BWD(12, 5);
#undef LP2_BWD
}
void launch_bwd(const Plan& P, const Ws& w, const float* own, int64_t ldo, int64_t n_own, const float* pool, int64_t ldp, int64_t n_pool, int n,
                int np, float kscale, const float* ownL, const float* ownC, const float* poolL, const float* poolC, float* part, bool feat_ready,
                float limit, const lp::Plan& PV, const lp::Params& q, hipStream_t st) {
  const float pre2 = sqrtf(2.f * kscale);
  const float* origin = w.spread + W_ORIGIN_USED;
  if (!feat_ready)
    hipLaunchKernelGGL(prep_feat_k, dim3((unsigned)P.pool_tiles), dim3(128), 0, st, pool, ldp, n_pool, n, origin, pre2, poolL, poolC,
                       (u32x4*)w.pool_feat);
  ValuSweep v{own, ldo, n_own, pool, ldp, n_pool, q, PV.chunk, (int)PV.tiles, PV.nsplit, ownL, ownC, poolL, poolC};
  if (P.T == 1) launch_bwd_T<1>(P, w, own, ldo, n_own, n_pool, n, np, pre2, ownL, ownC, part, limit, v, st);
  else launch_bwd_T<2>(P, w, own, ldo, n_own, n_pool, n, np, pre2, ownL, ownC, part, limit, v, st);
}

}  // namespace lp2
}  // namespace clica
