// gjx_pairwise.hip — pairwise Gaussian log-sum-exp (gjx_pairwise_gauss_lse):
//   out[r] = log sum_c exp(bias[c] - 1/2 p |q_r - k_c|^2),   r < n_q, c < n_k,
// the n_q x n_k part of marginal backward smoothing (FFBSm), where both sets are a filter step's K particles.  Nothing of size
// n_q x n_k is ever stored: the pairs are made 16 x 16 at a time on the matrix cores and consumed by a streaming log-sum-exp.
//
// Score.  With tildes for values minus `centre`:  score(r, c) = -1/2 p |q~_r|^2 + [bias_c - 1/2 p |k~_c|^2] + p q~_r . k~_c.
// The first term is constant in c and is added at the very end (k_pw_merge); the bracket is a per-key number kb_c, computed when the
// key is staged; the cross term is a matrix product.  Everything inside the loop is in units of log 2 (kb and the query fragment
// are scaled by log2 e), so the exponential of a pair is one v_exp_f32 and nothing else.
//
// Matrix instruction.  v_mfma_f32_16x16x4_f32, inputs f32 (the expansion cancels: bf16 would not survive it).  d is padded with
// zeros to DC = ceil(d / 4) chunks of 4.  Keys are the A operand (lane l holds key l % 16, component 4 c + l / 16), queries the B
// operand (lane l holds query l % 16, component 4 c + l / 16), so D's rows are keys and its columns queries: lane l's four
// accumulators are keys 4 (l / 16) .. + 3 for the ONE query l % 16.  The running (max, sum) of a query is therefore lane-local for
// the whole key loop; the four lanes l % 16 + {0, 16, 32, 48} of a query are combined once, after the loop.  kb_c enters as the
// C operand of the first MFMA of a tile (a 16-byte LDS read per 16 keys), so the accumulator comes out as the score.
//
// Block.  256 threads, 4 waves.  A wave keeps 4 groups of 16 queries as B fragments in registers (4 DC VGPRs, scaled by p log2 e)
// for the whole kernel: 64 queries per wave, 256 per block, and every A fragment read from LDS feeds 4 MFMAs.  Keys are staged 64 at a
// time through LDS, double-buffered: the global loads of tile n + 1 are issued before the MFMAs of tile n and stored after them,
// one barrier per tile.  Staging: thread t takes key t / 4 and the components 4 c + t % 4 (dword loads, so no alignment is asked
// of the rows), subtracts the centre, sums the squares over its quad of lanes, and writes the centred coordinates (row stride 80
// floats: the four component rows a wave reads together fall on disjoint banks) and kb.  A dead key (bias -inf or NaN), a key past
// n_k, and a live key whose centred norm is not finite are staged as ZERO coordinates with kb = -inf (dead, tail) or NaN (the last):
// what the matrix cores see is always finite.
//
// Online rescaling, once per staged tile: the 16 scores of a (lane, group) give the tile's maximum, the running sum is rescaled by
// one exponential, the 16 pairs cost one exponential each.
//
// Grid: (query blocks) x (key splits).  The number of splits is a function of (n_q, n_k) alone: enough to offer the device about
// 1024 blocks, never less than 2 tiles per split.  Block (x, y) writes the (max, sum) of its 256 queries over its keys to
// part[y][query]; k_pw_merge, one thread per query, folds the splits in index order, adds -1/2 p |q~|^2 and writes out.  No
// atomics, no block waits for another, every sum in an order fixed by the shape: the output is bit-reproducible.
//
// gjx_pairwise_gauss_mean (k_pw_mean, k_pw_mean_merge; second half of this file) adds the softmax-weighted mean of a value matrix
// over the same scores: attention with a Gaussian kernel.  Its scheme is described there.
//
// gjx_pairwise_gauss_lse_diag (k_pw_lse_diag, k_pw_merge_diag; last part of this file) is the log-sum-exp with one diagonal precision
// per key or per query: the score becomes a bilinear form over 2 d features.  Its scheme and edge rules are described there.
//
// gjx_pairwise_gauss_mean_diag and gjx_pairwise_gauss_pick_diag (k_pw_mean_diag, k_pw_pick_diag, k_pw_pick_finish_diag; after it) are
// the mean and the pick over those scores with the precisions on the keys.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "gjx_device.h"
#include "gjx_host.h"

namespace gjx {

typedef float pw_v4f __attribute__((ext_vector_type(4)));

constexpr int kPwThreads = 256;
constexpr int kPwGroups = 4;                          // 16-query groups per wave
constexpr int kPwBlockQ = 4 * 16 * kPwGroups;         // queries per block
constexpr int kPwTile = 64;                           // keys per staged tile
constexpr int kPwLd = kPwTile + 16;                   // floats between component rows in LDS
constexpr int kPwMinTiles = 2;                        // tiles per key split at least
constexpr int kPwTargetBlocks = 1024;
constexpr float kPwLog2e = 1.44269504f, kPwLn2 = 0.693147181f;

struct PwArgs {
  const float* q;
  const float* k;
  const float* bias;       // or NULL
  const float* centre;     // or NULL
  float* out;
  float2* part;            // [n_splits][n_q] = {max, sum} in units of log 2, without the query's own term
  int64_t stride_q, stride_k;
  int32_t n_q, n_k, d;
  int32_t n_tiles, tiles_per_split, n_splits;
  float p;
};

// (m, s) <- (m, s) + (om, os) where a pair stands for s 2^m; (-inf, 0) is the empty sum
GJX_DEV void pw_fold(float& m, float& s, float om, float os) {
  const float M = fmaxf(m, om), Ms = M > -INFINITY ? M : 0.0f;
  s = s * __builtin_amdgcn_exp2f(m - Ms) + os * __builtin_amdgcn_exp2f(om - Ms);
  m = M;
}

template <int DC>
__global__ __launch_bounds__(kPwThreads) void k_pw_lse(const PwArgs a) {
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;            // the MFMA's view of the lane
  const int skey = tid >> 2, spart = tid & 3;             // the staging's view: key of the tile, components 4 c + spart

  // the wave's query fragments, for the whole kernel
  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  const float ps = a.p * kPwLog2e;
  float qf[kPwGroups][DC];
  float scen[DC];
#pragma unroll
  for (int c = 0; c < DC; ++c) {
    const int dq = 4 * c + quad, ds = 4 * c + spart;
    const float cen = (a.centre && dq < a.d) ? a.centre[dq] : 0.0f;
    scen[c] = (a.centre && ds < a.d) ? a.centre[ds] : 0.0f;
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      const int qi = q0 + 16 * g + col;
      qf[g][c] = (dq < a.d && qi < a.n_q) ? (a.q[(int64_t)dq * a.stride_q + qi] - cen) * ps : 0.0f;
    }
  }

  float v[DC], b;
  auto load = [&](int tile) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int ds = 4 * c + spart;
      v[c] = (in && ds < a.d) ? a.k[(int64_t)ds * a.stride_k + key] - scen[c] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    float k2 = 0.0f;
#pragma unroll
    for (int c = 0; c < DC; ++c) k2 = fmaf(v[c], v[c], k2);
    k2 = quad_sum(k2);
    const bool dead = !(b > -INFINITY);                   // -inf or NaN
    const bool zero = dead || !(k2 < INFINITY);
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[buf][(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : v[c];
    if (spart == 0) sb[buf][skey] = dead ? -INFINITY : (zero ? NAN : (b - 0.5f * a.p * k2) * kPwLog2e);
  };

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  float m[kPwGroups], s[kPwGroups];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) { m[g] = -INFINITY; s[g] = 0.0f; }

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    float af[4][DC];
    pw_v4f seed[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                         // the tile's four 16-key subtiles
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sb[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      pw_v4f acc[4];
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
        mn = fmaxf(fmaxf(mn, fmaxf(acc[u][0], acc[u][1])), fmaxf(acc[u][2], acc[u][3]));        // (fmaxf drops a NaN)
      }
      const float ms = mn > -INFINITY ? mn : 0.0f;
      float e = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) e += __builtin_amdgcn_exp2f(acc[u][r] - ms);
      s[g] = s[g] * __builtin_amdgcn_exp2f(m[g] - ms) + e;
      m[g] = mn;
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // the four lanes of a query, then its partial
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float om = __shfl_xor(m[g], off, 64), os = __shfl_xor(s[g], off, 64);
      pw_fold(m[g], s[g], om, os);
    }
    const int qi = q0 + 16 * g + col;
    if (quad == 0 && qi < a.n_q) a.part[(int64_t)blockIdx.y * a.n_q + qi] = make_float2(m[g], s[g]);
  }
}

// one thread per query: the splits in index order, the query's own term, the answer in natural units
__global__ __launch_bounds__(kPwThreads) void k_pw_merge(const PwArgs a) {
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q) return;
  float q2 = 0.0f;
  for (int i = 0; i < a.d; ++i) {
    const float x = a.q[(int64_t)i * a.stride_q + r] - (a.centre ? a.centre[i] : 0.0f);
    q2 = fmaf(x, x, q2);
  }
  float m = -INFINITY, s = 0.0f;
  for (int y = 0; y < a.n_splits; ++y) {
    const float2 p = a.part[(int64_t)y * a.n_q + r];
    pw_fold(m, s, p.x, p.y);
  }
  // no live key: m = -inf, s = 0 -> -inf; a poisoned key: s = NaN -> NaN
  a.out[r] = q2 < INFINITY ? (m + __builtin_amdgcn_logf(s)) * kPwLn2 - 0.5f * a.p * q2 : NAN;
}

// the split of the keys over blocks: a function of (n_q, n_k) alone.  false: a shape the call refuses
static bool pw_plan(int64_t n_q, int64_t n_k, int32_t d, PwArgs* a) {
  if (n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 || d > GJX_PAIRWISE_MAX_DIM) return false;
  const int64_t n_qb = (n_q + kPwBlockQ - 1) / kPwBlockQ;
  const int32_t n_tiles = (int32_t)((n_k + kPwTile - 1) / kPwTile);
  int64_t want = (kPwTargetBlocks + n_qb - 1) / n_qb;
  if (want > n_tiles / kPwMinTiles) want = n_tiles / kPwMinTiles;
  if (want < 1) want = 1;
  a->n_q = (int32_t)n_q; a->n_k = (int32_t)n_k; a->d = d;
  a->n_tiles = n_tiles;
  a->tiles_per_split = (int32_t)((n_tiles + want - 1) / want);
  a->n_splits = (n_tiles + a->tiles_per_split - 1) / a->tiles_per_split;
  return true;
}

template <int DC>
static void pw_launch(const PwArgs& a, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(k_pw_lse<DC>, grid, dim3(kPwThreads), 0, st, a);
}

// ---- gjx_pairwise_gauss_mean:  mean[j][r] = sum_c softmax_c(score(r, c)) v[j][c],  and the log-sum-exp as a by-product ----
//
// Scores are made exactly as in k_pw_lse (same staging, same centring, same zeroing of dead, tail and poisoned keys, kb as the C
// operand).  Second product.  Lane l's accumulators acc[u][i] are the scores of keys 16 u + 4 (l / 16) + i for the one query l % 16:
// that is the B-operand layout of a 16x16x4 product whose contraction index is l / 16.  So P = exp2(acc - max) feeds a second
// v_mfma_f32_16x16x4_f32 as B with no shuffle and no LDS round trip: MFMA (u, i) contracts the four keys 16 u + 4 quad + i, quad =
// 0 .. 3, its A fragment is V[j = l % 16][that key].  The output is O^T[j][query]: lane l holds j = 4 (l / 16) + r for query l % 16,
// so the online rescale factor of a query is lane-local.  dv is padded with zero rows to VB = ceil(dv / 16) blocks of 16: 16 VB
// MFMAs per staged tile and query group on top of the 4 DC of the scores; O^T lives in 4 VB accumulators per group for the whole loop.
//
// Shared maximum.  The second product contracts over the four lanes l % 16 + {0, 16, 32, 48} of a query, so these must agree on the
// maximum BEFORE the exponentials (k_pw_lse lets each keep its own).  Two v_permlane{16,32}_swap per tile and group exchange the
// rows of the wave in the VALU (ds_bpermute where the compiler lacks them).  The running maximum is then the same number in the four
// lanes; the running sum stays lane-local (a lane's own 16 keys per tile) and the four are added after the loop.  O^T and the sum
// are rescaled once per staged tile by one exponential.
//
// Values go through LDS with the keys, double-buffered, under the same single barrier per tile, laid out [j][key] with row stride
// 68 floats: a lane's four i are one 16-byte read at [j = col][16 u + 4 quad], and the 16 lanes of a quad-row (col = 0 .. 15) start
// 68 floats = 4 banks (mod 64) apart: 16 x 4 dwords on 64 distinct banks.  (Staging stores fall 4 spart + skey: up to 4 lanes on
// a bank, 4 VB dword stores a thread and tile, nothing next to the 16 (DC / 4 + VB) MFMAs.)  A dead or tail key's values are staged
// as zeros (they often hold NaN / inf, and 0 x NaN must not reach an accumulator); a live key's non-finite value is staged as NaN:
// the A fragment's row j is then NaN in every query's accumulator whether or not the weight underflowed.
//
// Grid and plan are k_pw_lse's.  A split leaves (max, sum) and O^T[dv] per query in the workspace ([split][j][n_q], coalesced over
// queries); k_pw_mean_merge, one thread per (query, j), folds the splits in index order, divides, and (j = 0) writes the lse.
constexpr int kPwLdV = kPwTile + 4;                   // floats between value rows in LDS

struct PwMeanArgs {
  PwArgs pw;               // pw.out: the lse, or NULL
  const float* v;
  float* mean;             // f32[dv][n_q]
  float* opart;            // [n_splits][dv][n_q], scaled by 2^-max of the split
  int64_t stride_v;
  int32_t dv;
};

// the maximum over the four lanes l % 16 + {0, 16, 32, 48}, in all four
GJX_DEV float pw_rows_max(float x) {
#if __has_builtin(__builtin_amdgcn_permlane16_swap) && __has_builtin(__builtin_amdgcn_permlane32_swap)
  unsigned u = __float_as_uint(x);
  auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);          // {r0 r0 r2 r2}, {r1 r1 r3 r3}
  x = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
  u = __float_as_uint(x);
  auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);          // {lo lo}, {hi hi}
  return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
#else
  x = fmaxf(x, __shfl_xor(x, 16, 64));
  return fmaxf(x, __shfl_xor(x, 32, 64));
#endif
}

template <int DC, int VB>
__global__ __launch_bounds__(kPwThreads) void k_pw_mean(const PwMeanArgs ma) {
  const PwArgs& a = ma.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];
  __shared__ __attribute__((aligned(16))) float sv[2][16 * VB * kPwLdV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int skey = tid >> 2, spart = tid & 3;

  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  const float ps = a.p * kPwLog2e;
  float qf[kPwGroups][DC];
  float scen[DC];
#pragma unroll
  for (int c = 0; c < DC; ++c) {
    const int dq = 4 * c + quad, ds = 4 * c + spart;
    const float cen = (a.centre && dq < a.d) ? a.centre[dq] : 0.0f;
    scen[c] = (a.centre && ds < a.d) ? a.centre[ds] : 0.0f;
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      const int qi = q0 + 16 * g + col;
      qf[g][c] = (dq < a.d && qi < a.n_q) ? (a.q[(int64_t)dq * a.stride_q + qi] - cen) * ps : 0.0f;
    }
  }

  float kv[DC], vv[4 * VB], b;
  auto load = [&](int tile) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int ds = 4 * c + spart;
      kv[c] = (in && ds < a.d) ? a.k[(int64_t)ds * a.stride_k + key] - scen[c] : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 4 * VB; ++c) {
      const int j = 4 * c + spart;
      vv[c] = (in && j < ma.dv) ? ma.v[(int64_t)j * ma.stride_v + key] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    float k2 = 0.0f;
#pragma unroll
    for (int c = 0; c < DC; ++c) k2 = fmaf(kv[c], kv[c], k2);
    k2 = quad_sum(k2);
    const bool dead = !(b > -INFINITY);                   // -inf or NaN
    const bool zero = dead || !(k2 < INFINITY);
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[buf][(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : kv[c];
#pragma unroll
    for (int c = 0; c < 4 * VB; ++c)
      sv[buf][(4 * c + spart) * kPwLdV + skey] = dead ? 0.0f : (fabsf(vv[c]) < INFINITY ? vv[c] : NAN);
    if (spart == 0) sb[buf][skey] = dead ? -INFINITY : (zero ? NAN : (b - 0.5f * a.p * k2) * kPwLog2e);
  };

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  float m[kPwGroups], s[kPwGroups];
  pw_v4f o[kPwGroups][VB];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    m[g] = -INFINITY;
    s[g] = 0.0f;
#pragma unroll
    for (int vb = 0; vb < VB; ++vb) o[g][vb] = pw_v4f{0.0f, 0.0f, 0.0f, 0.0f};
  }

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    float af[4][DC];
    pw_v4f seed[4], vf[4][VB];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sb[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
#pragma unroll
      for (int vb = 0; vb < VB; ++vb)
        vf[u][vb] = *reinterpret_cast<const pw_v4f*>(&sv[buf][(16 * vb + col) * kPwLdV + 16 * u + 4 * quad]);
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      pw_v4f acc[4];
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
        mn = fmaxf(fmaxf(mn, fmaxf(acc[u][0], acc[u][1])), fmaxf(acc[u][2], acc[u][3]));        // (fmaxf drops a NaN)
      }
      mn = pw_rows_max(mn);                               // the query's four lanes agree before the exponentials
      const float ms = mn > -INFINITY ? mn : 0.0f;
      const float f = __builtin_amdgcn_exp2f(m[g] - ms);
      float e = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[u][r] = __builtin_amdgcn_exp2f(acc[u][r] - ms);
          e += acc[u][r];
        }
      s[g] = s[g] * f + e;
      m[g] = mn;
#pragma unroll
      for (int vb = 0; vb < VB; ++vb) {
        o[g][vb] *= f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) o[g][vb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[u][vb][r], acc[u][r], o[g][vb], 0, 0, 0);
      }
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // the four lanes of a query share m; their sums are added in one fixed order.  Then the partials.
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    s[g] += __shfl_xor(s[g], 16, 64);
    s[g] += __shfl_xor(s[g], 32, 64);
    const int qi = q0 + 16 * g + col;
    if (qi >= a.n_q) continue;
    if (quad == 0) a.part[(int64_t)blockIdx.y * a.n_q + qi] = make_float2(m[g], s[g]);
#pragma unroll
    for (int vb = 0; vb < VB; ++vb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * vb + 4 * quad + r;
        if (j < ma.dv) ma.opart[((int64_t)blockIdx.y * ma.dv + j) * a.n_q + qi] = o[g][vb][r];
      }
  }
}

// one thread per (query, value row): the splits in index order, the division, and from row 0 the log-sum-exp
__global__ __launch_bounds__(kPwThreads) void k_pw_mean_merge(const PwMeanArgs ma) {
  const PwArgs& a = ma.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  const int j = (int)blockIdx.y;
  if (r >= a.n_q) return;
  float q2 = 0.0f;
  for (int i = 0; i < a.d; ++i) {
    const float x = a.q[(int64_t)i * a.stride_q + r] - (a.centre ? a.centre[i] : 0.0f);
    q2 = fmaf(x, x, q2);
  }
  float m = -INFINITY, s = 0.0f;
  for (int y = 0; y < a.n_splits; ++y) {
    const float2 p = a.part[(int64_t)y * a.n_q + r];
    pw_fold(m, s, p.x, p.y);
  }
  const float ms = m > -INFINITY ? m : 0.0f;
  float o = 0.0f;
  for (int y = 0; y < a.n_splits; ++y)
    o = fmaf(ma.opart[((int64_t)y * ma.dv + j) * a.n_q + r], __builtin_amdgcn_exp2f(a.part[(int64_t)y * a.n_q + r].x - ms), o);
  // no live key: 0 / 0 = NaN; a poisoned key: s = NaN; a live key's non-finite value: o = NaN in its row
  ma.mean[(int64_t)j * a.n_q + r] = q2 < INFINITY ? o / s : NAN;
  if (j == 0 && a.out) a.out[r] = q2 < INFINITY ? (m + __builtin_amdgcn_logf(s)) * kPwLn2 - 0.5f * a.p * q2 : NAN;
}

template <int DC>
static void pw_mean_launch(const PwMeanArgs& ma, dim3 grid, hipStream_t st) {
  if (ma.dv <= 16) hipLaunchKernelGGL((k_pw_mean<DC, 1>), grid, dim3(kPwThreads), 0, st, ma);
  else hipLaunchKernelGGL((k_pw_mean<DC, 2>), grid, dim3(kPwThreads), 0, st, ma);
}

// ---- gjx_pairwise_gauss_pick:  pick[r] = the first key c with  sum_{c' <= c} e_rc' >= u_r sum_c e_rc,  e_rc = exp(score(r, c)) ----
//
// Backward simulation (FFBSi): one categorical draw per query over the scores of k_pw_lse, by inverse CDF in key-index order with the
// caller's uniform.  Four launches, nothing of size n_q x n_k stored, no atomics, no block waits for another.
//   1. k_pw_lse as it is: part[split][query] = (max, sum).
//   2. k_pw_pick_plan, one thread per query: folds the splits in index order (as k_pw_merge) to L = max + log2(sum) in the loop's
//      units, and writes the lse if asked.  With L known the mass of split y in units of the total is sum_y 2^(max_y - L); the splits
//      are walked in index order to the first positive one whose prefix interval reaches the target.  The target is u, but +inf for
//      u >= 1 (nothing ever reaches it: every level falls back to its last positive entry) and 0 for u <= 0 (the first positive entry
//      reaches it).  That split OWNS the query; the target left inside it (`resid`) goes to the workspace.  A query without a pick
//      (no live key, a poisoned key, a non-finite query, a NaN u) is owned by nobody and gets -1 here.
//   3. k_pw_pick<DC>: grid, plan, staging and MFMAs of k_pw_lse, but exp2(acc - L) <= 1 needs no running maximum and no rescaling.
//      A CHUNK is one staged tile of 64 keys: a lane adds its 16 keys, the query's four lanes are added with two
//      v_permlane{16,32}_swap (the same bits in all four), and the running cumulative is compared with the residual target: the first
//      positive chunk that reaches it is recorded together with the cumulative before it, else the last positive chunk.  Only the
//      lanes of the owning split hold a finite L, and a 16-query group of which this split owns nobody is skipped (wave-uniform): with
//      S splits about (1 - 1/S)^16 of the matrix work goes away.  The split's maximum key contributes exp2(max_y - L), the very number
//      that was positive in launch 2, so an owned query always records a positive chunk.
//   4. k_pw_pick_finish, one thread per query: the recorded chunk's 64 scores again in plain VALU in key order (same centring, same
//      kb), the cumulative walked to the first key with positive mass that reaches resid - before; else the last key with positive
//      mass; and should the VALU scores of a chunk of vanishing mass all underflow, the chunk's largest score.  64 d multiply-adds a
//      query.
// Chunk-then-key in index order is inverse-CDF in index order.  Registers per 16-query group next to qf: L, residual, cumulative,
// recorded chunk and the cumulative before it.  LDS: k_pw_lse's.
struct PwPickArgs {
  PwArgs pw;               // pw.out: the lse, or NULL
  const float* u;
  int32_t* pick;
  float* L;                // [n_q] log2 of the total, without the query's own term
  float* resid;            // [n_q] the target inside the owning split, in units of the total
  int32_t* own;            // [n_q] the owning split; -1: no pick
  int32_t* rchunk;         // [n_q] the recorded tile, written by the owning split's block
  float* rbefore;          // [n_q] the split's cumulative before that tile
};

// the sum over the four lanes l % 16 + {0, 16, 32, 48}, the same bits in all four (a + b is b + a)
GJX_DEV float pw_rows_sum(float x) {
#if __has_builtin(__builtin_amdgcn_permlane16_swap) && __has_builtin(__builtin_amdgcn_permlane32_swap)
  unsigned u = __float_as_uint(x);
  auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);          // {r0 r0 r2 r2}, {r1 r1 r3 r3}
  x = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  u = __float_as_uint(x);
  auto b = __builtin_amdgcn_permlane32_swap(u, u, false, false);          // {lo lo}, {hi hi}
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
#else
  x += __shfl_xor(x, 16, 64);
  return x + __shfl_xor(x, 32, 64);
#endif
}

__global__ __launch_bounds__(kPwThreads) void k_pw_pick_plan(const PwPickArgs pa) {
  const PwArgs& a = pa.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q) return;
  float q2 = 0.0f;
  for (int i = 0; i < a.d; ++i) {
    const float x = a.q[(int64_t)i * a.stride_q + r] - (a.centre ? a.centre[i] : 0.0f);
    q2 = fmaf(x, x, q2);
  }
  float m = -INFINITY, s = 0.0f;
  for (int y = 0; y < a.n_splits; ++y) {
    const float2 p = a.part[(int64_t)y * a.n_q + r];
    pw_fold(m, s, p.x, p.y);
  }
  const float L = m + __builtin_amdgcn_logf(s);
  if (a.out) a.out[r] = q2 < INFINITY ? L * kPwLn2 - 0.5f * a.p * q2 : NAN;
  const float u = pa.u[r];
  int own = -1;
  float resid = 0.0f;
  if (q2 < INFINITY && m > -INFINITY && s == s && u == u) {
    const float target = u >= 1.0f ? INFINITY : fmaxf(u, 0.0f);
    float cum = 0.0f;
    for (int y = 0; y < a.n_splits; ++y) {
      const float2 p = a.part[(int64_t)y * a.n_q + r];
      const float mass = p.y * __builtin_amdgcn_exp2f(p.x - L);
      if (mass > 0.0f) {
        own = y;
        resid = target - cum;
        if (cum + mass >= target) break;
      }
      cum += mass;
    }
  }
  pa.L[r] = L;
  pa.resid[r] = resid;
  pa.own[r] = own;
  if (own < 0) pa.pick[r] = -1;
}

template <int DC>
__global__ __launch_bounds__(kPwThreads) void k_pw_pick(const PwPickArgs pa) {
  const PwArgs& a = pa.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int skey = tid >> 2, spart = tid & 3;

  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  const float ps = a.p * kPwLog2e;
  float qf[kPwGroups][DC];
  float scen[DC];
#pragma unroll
  for (int c = 0; c < DC; ++c) {
    const int dq = 4 * c + quad, ds = 4 * c + spart;
    const float cen = (a.centre && dq < a.d) ? a.centre[dq] : 0.0f;
    scen[c] = (a.centre && ds < a.d) ? a.centre[ds] : 0.0f;
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      const int qi = q0 + 16 * g + col;
      qf[g][c] = (dq < a.d && qi < a.n_q) ? (a.q[(int64_t)dq * a.stride_q + qi] - cen) * ps : 0.0f;
    }
  }

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  // per group: the query's L and residual target where this split owns it, the running cumulative, the record
  float L[kPwGroups], want[kPwGroups], cum[kPwGroups], rb[kPwGroups];
  int rt[kPwGroups];
  bool mine[kPwGroups], act[kPwGroups], done[kPwGroups];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    const int qi = q0 + 16 * g + col;
    mine[g] = qi < a.n_q && pa.own[qi] == (int)blockIdx.y;
    act[g] = __any(mine[g]) != 0;                         // wave-uniform: somebody in the group is owned here
    L[g] = mine[g] ? pa.L[qi] : INFINITY;                 // (+inf: every exponential of a query owned elsewhere is 0)
    want[g] = mine[g] ? pa.resid[qi] : INFINITY;
    cum[g] = rb[g] = 0.0f;
    rt[g] = t0;
    done[g] = false;
  }

  float v[DC], b;
  auto load = [&](int tile) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int ds = 4 * c + spart;
      v[c] = (in && ds < a.d) ? a.k[(int64_t)ds * a.stride_k + key] - scen[c] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    float k2 = 0.0f;
#pragma unroll
    for (int c = 0; c < DC; ++c) k2 = fmaf(v[c], v[c], k2);
    k2 = quad_sum(k2);
    const bool dead = !(b > -INFINITY);                   // -inf or NaN
    const bool zero = dead || !(k2 < INFINITY);
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[buf][(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : v[c];
    if (spart == 0) sb[buf][skey] = dead ? -INFINITY : (zero ? NAN : (b - 0.5f * a.p * k2) * kPwLog2e);
  };

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    float af[4][DC];
    pw_v4f seed[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sb[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      if (!act[g]) continue;
      pw_v4f acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
      }
      float e = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) e += __builtin_amdgcn_exp2f(acc[u][r] - L[g]);
      e = pw_rows_sum(e);                                 // the chunk's mass, the same bits in the query's four lanes
      if (!done[g] && e > 0.0f) {
        rt[g] = t;
        rb[g] = cum[g];
        done[g] = cum[g] + e >= want[g];
      }
      cum[g] += e;
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    const int qi = q0 + 16 * g + col;
    if (quad == 0 && mine[g]) {
      pa.rchunk[qi] = rt[g];
      pa.rbefore[qi] = rb[g];
    }
  }
}

// one thread per query: the recorded chunk key by key
__global__ __launch_bounds__(kPwThreads) void k_pw_pick_finish(const PwPickArgs pa) {
  const PwArgs& a = pa.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q || pa.own[r] < 0) return;                // (no pick: k_pw_pick_plan wrote the -1)
  const float ps = a.p * kPwLog2e;
  float qv[GJX_PAIRWISE_MAX_DIM];
#pragma unroll
  for (int i = 0; i < GJX_PAIRWISE_MAX_DIM; ++i)
    qv[i] = i < a.d ? (a.q[(int64_t)i * a.stride_q + r] - (a.centre ? a.centre[i] : 0.0f)) * ps : 0.0f;
  const float L = pa.L[r], want = pa.resid[r] - pa.rbefore[r];
  const int t = min(max(pa.rchunk[r], 0), a.n_tiles - 1);
  const int c0 = t * kPwTile, c1 = min(c0 + kPwTile, a.n_k);
  float cum = 0.0f, top = -INFINITY;
  int pick = -1, last = -1, topc = -1;
  for (int c = c0; c < c1 && pick < 0; ++c) {
    const float b = a.bias ? a.bias[c] : 0.0f;
    if (!(b > -INFINITY)) continue;                       // dead
    float k2 = 0.0f, dot = 0.0f;
#pragma unroll
    for (int i = 0; i < GJX_PAIRWISE_MAX_DIM; ++i) {
      if (i >= a.d) break;
      const float x = a.k[(int64_t)i * a.stride_k + c] - (a.centre ? a.centre[i] : 0.0f);
      k2 = fmaf(x, x, k2);
      dot = fmaf(x, qv[i], dot);
    }
    const float sc = (b - 0.5f * a.p * k2) * kPwLog2e + dot;
    if (sc > top) { top = sc; topc = c; }
    const float e = __builtin_amdgcn_exp2f(sc - L);
    if (e > 0.0f) {
      last = c;
      cum += e;
      if (cum >= want) pick = c;
    }
  }
  pa.pick[r] = pick >= 0 ? pick : (last >= 0 ? last : topc);
}

template <int DC>
static void pw_pick_launch(const PwPickArgs& pa, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(k_pw_pick<DC>, grid, dim3(kPwThreads), 0, st, pa);
}

// ---- gjx_pairwise_gauss_lse_diag:  out[r] = log sum_c exp(bias[c] - 1/2 sum_j P_j(r, c) (q[j][r] - k[j][c])^2) ----
//
// P_j(r, c) = prec[j][c] (side KEYS) or prec[j][r] (side QUERIES): the diagonal precision belongs to one of the two particles of a
// pair, so no scaling of the sets removes it.  With tildes for values minus `centre` the score is still bilinear, over 2 d FEATURES:
//   KEYS:     score = [bias_c - 1/2 sum_j p_cj k~_cj^2]  +  sum_j (p_cj k~_cj) q~_rj  +  sum_j (-1/2 p_cj) q~_rj^2
//   QUERIES:  score = bias_c  +  sum_j k~_cj (p_rj q~_rj)  +  sum_j k~_cj^2 (-1/2 p_rj)  -  1/2 sum_j p_rj q~_rj^2
//   side     A operand (key features)   B operand (query features, x log2 e)   kb (C operand)                      added by the merge
//   KEYS     p k~,  -1/2 p              q~,  q~^2                              (bias - 1/2 sum p k~^2) log2 e      nothing
//   QUERIES  k~,    k~^2                p q~, -1/2 p                           bias log2 e                         -1/2 sum p q~^2
// Feature order: f = 2 j + s, s = 0 the linear and s = 1 the quadratic feature of component j, padded with zeros to DC = ceil(2 d / 4)
// chunks of 4 (d <= GJX_PAIRWISE_DIAG_MAX_DIM = 16: DC <= 8, the register budget k_pw_lse meets at d = 32).  A staging thread (key
// t / 4, features 4 c + t % 4) and a B lane (features 4 c + l / 16) therefore turn ONE loaded coordinate, component 2 c + (t % 4) / 2,
// into one feature; an odd d leaves the last chunk half empty.
//
// Everything else is k_pw_lse's, instruction for instruction in the key loop: keys the A operand and queries the B operand of
// v_mfma_f32_16x16x4_f32 with f32 inputs, the running (max, sum) of a query lane-local, 256 threads, 4 groups of 16 queries per wave held
// as B fragments for the whole kernel, 64-key tiles through double-buffered LDS (row stride 80 floats) under one barrier per tile, one
// rescale per tile, pw_plan's grid and key splits, partials [split][n_q], a merge that folds the splits in index order.  No atomics,
// fixed orders: bit-reproducible.  The workspace is gjx_pairwise_gauss_lse's.
//
// Edge rules.  A key whose bias is -inf or NaN is DEAD whatever its coordinates and precisions hold (NaN included); a key past n_k is
// staged like a dead one: zero features, kb = -inf.  A LIVE key is POISONED (every query's output NaN) when a precision entry of its own
// (side KEYS) is not > 0 and < inf, when a centred feature or kb is not finite (side QUERIES: a non-finite k~ or k~^2), or when its
// bias is +inf: zero features, kb = NaN, so the A operand and the C operand's finite part are all the matrix cores see of a key.  A
// query with a non-finite centred coordinate or square, or (side QUERIES) a precision entry that is not > 0 and < inf, gets NaN for
// that query alone: k_pw_merge_diag decides it from q, prec and centre (a query's B fragment touches its own column only).  No live
// key: -inf.  The normaliser 1/2 sum_j log prec is NOT part of the score: the caller folds it into bias (KEYS) or adds it to out.
struct PwDiagArgs {
  PwArgs pw;               // (pw.p is not read)
  const float* prec;       // f32[d][stride_p]: a column per key (side KEYS) or per query (side QUERIES)
  int64_t stride_p;
  int32_t side;
};

GJX_DEV bool pw_prec_ok(float p) { return p > 0.0f && p < INFINITY; }

template <int DC, int SIDE>
__global__ __launch_bounds__(kPwThreads) void k_pw_lse_diag(const PwDiagArgs da) {
  const PwArgs& a = da.pw;
  constexpr bool kKeys = SIDE == GJX_PAIRWISE_PREC_KEYS;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;            // the MFMA's view of the lane: query col, features 4 c + quad
  const int skey = tid >> 2, spart = tid & 3;             // the staging's view: key of the tile, features 4 c + spart
  const bool qquad = quad & 1, squad = spart & 1;         // the lane's features are the quadratic ones

  // the wave's query features, for the whole kernel
  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  float qf[kPwGroups][DC];
  float scen[DC];
#pragma unroll
  for (int c = 0; c < DC; ++c) {
    const int jq = 2 * c + (quad >> 1), js = 2 * c + (spart >> 1);
    const float cen = (a.centre && jq < a.d) ? a.centre[jq] : 0.0f;
    scen[c] = (a.centre && js < a.d) ? a.centre[js] : 0.0f;
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      const int qi = q0 + 16 * g + col;
      float f = 0.0f;
      if (jq < a.d && qi < a.n_q) {
        const float x = a.q[(int64_t)jq * a.stride_q + qi] - cen;
        if constexpr (kKeys) {
          f = qquad ? x * x : x;
        } else {
          const float p = da.prec[(int64_t)jq * da.stride_p + qi];
          f = qquad ? -0.5f * p : p * x;
        }
      }
      qf[g][c] = f * kPwLog2e;
    }
  }

  float v[DC], pv[kKeys ? DC : 1], b;
  auto load = [&](int tile) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int js = 2 * c + (spart >> 1);
      const bool have = in && js < a.d;
      v[c] = have ? a.k[(int64_t)js * a.stride_k + key] - scen[c] : 0.0f;
      if constexpr (kKeys) pv[c] = have ? da.prec[(int64_t)js * da.stride_p + key] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    // k2: sum_j p k~^2 (KEYS) or sum_j k~^2 (QUERIES, where only its finiteness is used); NaN for a precision that is not one
    float k2 = 0.0f;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      if constexpr (kKeys) {
        const bool pad = 2 * c + (spart >> 1) >= a.d;
        const float p = pv[c], lin = p * v[c];
        k2 = (pad || pw_prec_ok(p)) ? (squad ? k2 : fmaf(lin, v[c], k2)) : NAN;
        v[c] = squad ? -0.5f * p : lin;
      } else {
        if (squad) {
          v[c] *= v[c];
          k2 += v[c];
        }
      }
    }
    k2 = quad_sum(k2);
    const bool dead = !(b > -INFINITY);                   // -inf or NaN
    const bool zero = dead || !(k2 < INFINITY) || !(b < INFINITY);
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[buf][(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : v[c];
    if (spart == 0) sb[buf][skey] = dead ? -INFINITY : (zero ? NAN : (kKeys ? b - 0.5f * k2 : b) * kPwLog2e);
  };

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  float m[kPwGroups], s[kPwGroups];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) { m[g] = -INFINITY; s[g] = 0.0f; }

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    float af[4][DC];
    pw_v4f seed[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                         // the tile's four 16-key subtiles
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sb[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      pw_v4f acc[4];
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
        mn = fmaxf(fmaxf(mn, fmaxf(acc[u][0], acc[u][1])), fmaxf(acc[u][2], acc[u][3]));        // (fmaxf drops a NaN)
      }
      const float ms = mn > -INFINITY ? mn : 0.0f;
      float e = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) e += __builtin_amdgcn_exp2f(acc[u][r] - ms);
      s[g] = s[g] * __builtin_amdgcn_exp2f(m[g] - ms) + e;
      m[g] = mn;
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // the four lanes of a query, then its partial
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float om = __shfl_xor(m[g], off, 64), os = __shfl_xor(s[g], off, 64);
      pw_fold(m[g], s[g], om, os);
    }
    const int qi = q0 + 16 * g + col;
    if (quad == 0 && qi < a.n_q) a.part[(int64_t)blockIdx.y * a.n_q + qi] = make_float2(m[g], s[g]);
  }
}

// one thread per query: the splits in index order, the query's own term and its own verdict, the answer in natural units
__global__ __launch_bounds__(kPwThreads) void k_pw_merge_diag(const PwDiagArgs da) {
  const PwArgs& a = da.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q) return;
  const bool keys = da.side == GJX_PAIRWISE_PREC_KEYS;
  float q2 = 0.0f;                                        // sum_j p q~^2; side KEYS: p = 1, and only its finiteness is used
  for (int i = 0; i < a.d; ++i) {
    const float x = a.q[(int64_t)i * a.stride_q + r] - (a.centre ? a.centre[i] : 0.0f);
    const float p = keys ? 1.0f : da.prec[(int64_t)i * da.stride_p + r];
    q2 = pw_prec_ok(p) ? fmaf(p * x, x, q2) : NAN;
  }
  float m = -INFINITY, s = 0.0f;
  for (int y = 0; y < a.n_splits; ++y) {
    const float2 p = a.part[(int64_t)y * a.n_q + r];
    pw_fold(m, s, p.x, p.y);
  }
  // no live key: m = -inf, s = 0 -> -inf; a poisoned key: s = NaN -> NaN
  a.out[r] = q2 < INFINITY ? (m + __builtin_amdgcn_logf(s)) * kPwLn2 - (keys ? 0.0f : 0.5f * q2) : NAN;
}

template <int DC>
static void pw_diag_launch(const PwDiagArgs& da, dim3 grid, hipStream_t st) {
  if (da.side == GJX_PAIRWISE_PREC_KEYS)
    hipLaunchKernelGGL((k_pw_lse_diag<DC, GJX_PAIRWISE_PREC_KEYS>), grid, dim3(kPwThreads), 0, st, da);
  else
    hipLaunchKernelGGL((k_pw_lse_diag<DC, GJX_PAIRWISE_PREC_QUERIES>), grid, dim3(kPwThreads), 0, st, da);
}

// ---- gjx_pairwise_gauss_mean_diag, gjx_pairwise_gauss_pick_diag: the mean and the pick over the scores of k_pw_lse_diag<DC, KEYS> ----
//
// Side KEYS only (the parents of both smoothers are the keys).  k_pw_mean_diag<DC, VB> and k_pw_pick_diag<DC> are k_pw_mean and k_pw_pick
// with the 2 d features in place of the d coordinates: PwDiagKeys<DC> below is the prologue, the loads and the staging of
// k_pw_lse_diag<DC, KEYS>, operation for operation (same feature order, same kb, same zeroing of dead, tail and poisoned keys, so the
// scores of the three kernels are the same bits), and everything after the scores is the isotropic kernel's.  DC = ceil(2 d / 4) <= 8.
//
// The per-query launches need no diag sibling.  Under KEYS a query adds nothing to its scores after the loop and its verdict is the
// finiteness of sum_j q~_j^2 (that is: of every q~ and q~^2), which is what k_pw_mean_merge and k_pw_pick_plan compute with pw.p = 0:
// their own term 1/2 p |q~|^2 is then exactly 0 for a finite sum, and the lse comes out as L ln 2.  Both run unchanged with p = 0.
// Only k_pw_pick_finish has a sibling, k_pw_pick_finish_diag: it makes scores itself, with the key's own precisions.
template <int DC>
struct PwDiagKeys {
  float scen[DC];          // the centre at the staging thread's components
  float v[DC], pv[DC], b;  // the staging thread's key of the tile in flight: centred coordinates (then features), precisions, bias

  // the wave's query features (q~, q~^2) log2 e, for the whole kernel
  GJX_DEV void queries(const PwArgs& a, int q0, int col, int quad, int spart, float (&qf)[kPwGroups][DC]) {
    const bool qquad = quad & 1;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int jq = 2 * c + (quad >> 1), js = 2 * c + (spart >> 1);
      const float cen = (a.centre && jq < a.d) ? a.centre[jq] : 0.0f;
      scen[c] = (a.centre && js < a.d) ? a.centre[js] : 0.0f;
#pragma unroll
      for (int g = 0; g < kPwGroups; ++g) {
        const int qi = q0 + 16 * g + col;
        float f = 0.0f;
        if (jq < a.d && qi < a.n_q) {
          const float x = a.q[(int64_t)jq * a.stride_q + qi] - cen;
          f = qquad ? x * x : x;
        }
        qf[g][c] = f * kPwLog2e;
      }
    }
  }

  GJX_DEV void load(const PwArgs& a, const float* prec, int64_t stride_p, int tile, int skey, int spart) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int js = 2 * c + (spart >> 1);
      const bool have = in && js < a.d;
      v[c] = have ? a.k[(int64_t)js * a.stride_k + key] - scen[c] : 0.0f;
      pv[c] = have ? prec[(int64_t)js * stride_p + key] : 0.0f;
    }
  }

  // the key features (p k~, -1/2 p) and kb into one LDS buffer; -> the key is dead (bias -inf or NaN, or past n_k)
  GJX_DEV bool store(const PwArgs& a, float* sk, float* sb, int skey, int spart) {
    const bool squad = spart & 1;
    float k2 = 0.0f;                                      // sum_j p k~^2; NaN for a precision that is not one
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const bool pad = 2 * c + (spart >> 1) >= a.d;
      const float p = pv[c], lin = p * v[c];
      k2 = (pad || pw_prec_ok(p)) ? (squad ? k2 : fmaf(lin, v[c], k2)) : NAN;
      v[c] = squad ? -0.5f * p : lin;
    }
    k2 = quad_sum(k2);
    const bool dead = !(b > -INFINITY);                   // -inf or NaN
    const bool zero = dead || !(k2 < INFINITY) || !(b < INFINITY);
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : v[c];
    if (spart == 0) sb[skey] = dead ? -INFINITY : (zero ? NAN : (b - 0.5f * k2) * kPwLog2e);
    return dead;
  }
};

struct PwMeanDiagArgs {
  PwMeanArgs ma;           // ma.pw.p = 0: see above
  const float* prec;       // f32[d][stride_p], a column per key
  int64_t stride_p;
};

// k_pw_mean's loop over k_pw_lse_diag's scores: the shared maximum by pw_rows_max, exp2(acc - max) as the B operand of the value
// product, values staged [j][key] with row stride 68, O^T in 4 VB accumulators per group, one rescale and one barrier per tile.
template <int DC, int VB>
__global__ __launch_bounds__(kPwThreads) void k_pw_mean_diag(const PwMeanDiagArgs mda) {
  const PwMeanArgs& ma = mda.ma;
  const PwArgs& a = ma.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];
  __shared__ __attribute__((aligned(16))) float sv[2][16 * VB * kPwLdV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;            // the MFMA's view of the lane: query col, features 4 c + quad
  const int skey = tid >> 2, spart = tid & 3;             // the staging's view: key of the tile, features 4 c + spart

  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  float qf[kPwGroups][DC];
  PwDiagKeys<DC> keys;
  keys.queries(a, q0, col, quad, spart, qf);

  float vv[4 * VB];
  auto load = [&](int tile) {
    keys.load(a, mda.prec, mda.stride_p, tile, skey, spart);
    const int key = tile * kPwTile + skey;
#pragma unroll
    for (int c = 0; c < 4 * VB; ++c) {
      const int j = 4 * c + spart;
      vv[c] = (key < a.n_k && j < ma.dv) ? ma.v[(int64_t)j * ma.stride_v + key] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    const bool dead = keys.store(a, sk[buf], sb[buf], skey, spart);
#pragma unroll
    for (int c = 0; c < 4 * VB; ++c)
      sv[buf][(4 * c + spart) * kPwLdV + skey] = dead ? 0.0f : (fabsf(vv[c]) < INFINITY ? vv[c] : NAN);
  };

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  float m[kPwGroups], s[kPwGroups];
  pw_v4f o[kPwGroups][VB];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    m[g] = -INFINITY;
    s[g] = 0.0f;
#pragma unroll
    for (int vb = 0; vb < VB; ++vb) o[g][vb] = pw_v4f{0.0f, 0.0f, 0.0f, 0.0f};
  }

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    float af[4][DC];
    pw_v4f seed[4], vf[4][VB];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                         // the tile's four 16-key subtiles
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sb[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
#pragma unroll
      for (int vb = 0; vb < VB; ++vb)
        vf[u][vb] = *reinterpret_cast<const pw_v4f*>(&sv[buf][(16 * vb + col) * kPwLdV + 16 * u + 4 * quad]);
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      pw_v4f acc[4];
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
        mn = fmaxf(fmaxf(mn, fmaxf(acc[u][0], acc[u][1])), fmaxf(acc[u][2], acc[u][3]));        // (fmaxf drops a NaN)
      }
      mn = pw_rows_max(mn);                               // the query's four lanes agree before the exponentials
      const float ms = mn > -INFINITY ? mn : 0.0f;
      const float f = __builtin_amdgcn_exp2f(m[g] - ms);
      float e = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[u][r] = __builtin_amdgcn_exp2f(acc[u][r] - ms);
          e += acc[u][r];
        }
      s[g] = s[g] * f + e;
      m[g] = mn;
#pragma unroll
      for (int vb = 0; vb < VB; ++vb) {
        o[g][vb] *= f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) o[g][vb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[u][vb][r], acc[u][r], o[g][vb], 0, 0, 0);
      }
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // the four lanes of a query share m; their sums are added in one fixed order.  Then the partials, laid out as k_pw_mean's.
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    s[g] += __shfl_xor(s[g], 16, 64);
    s[g] += __shfl_xor(s[g], 32, 64);
    const int qi = q0 + 16 * g + col;
    if (qi >= a.n_q) continue;
    if (quad == 0) a.part[(int64_t)blockIdx.y * a.n_q + qi] = make_float2(m[g], s[g]);
#pragma unroll
    for (int vb = 0; vb < VB; ++vb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * vb + 4 * quad + r;
        if (j < ma.dv) ma.opart[((int64_t)blockIdx.y * ma.dv + j) * a.n_q + qi] = o[g][vb][r];
      }
  }
}

template <int DC>
static void pw_mean_diag_launch(const PwMeanDiagArgs& mda, dim3 grid, hipStream_t st) {
  if (mda.ma.dv <= 16) hipLaunchKernelGGL((k_pw_mean_diag<DC, 1>), grid, dim3(kPwThreads), 0, st, mda);
  else hipLaunchKernelGGL((k_pw_mean_diag<DC, 2>), grid, dim3(kPwThreads), 0, st, mda);
}

struct PwPickDiagArgs {
  PwPickArgs pa;           // pa.pw.p = 0: see above
  const float* prec;       // f32[d][stride_p], a column per key
  int64_t stride_p;
};

// k_pw_pick's loop over k_pw_lse_diag's scores: exp2(acc - L) with L from the plan, 64-key chunk masses by pw_rows_sum, the crossing
// chunk recorded with the cumulative before it, groups this split does not own skipped wave-uniformly.
template <int DC>
__global__ __launch_bounds__(kPwThreads) void k_pw_pick_diag(const PwPickDiagArgs pda) {
  const PwPickArgs& pa = pda.pa;
  const PwArgs& a = pa.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int skey = tid >> 2, spart = tid & 3;

  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  float qf[kPwGroups][DC];
  PwDiagKeys<DC> keys;
  keys.queries(a, q0, col, quad, spart, qf);

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  // per group: the query's L and residual target where this split owns it, the running cumulative, the record
  float L[kPwGroups], want[kPwGroups], cum[kPwGroups], rb[kPwGroups];
  int rt[kPwGroups];
  bool mine[kPwGroups], act[kPwGroups], done[kPwGroups];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    const int qi = q0 + 16 * g + col;
    mine[g] = qi < a.n_q && pa.own[qi] == (int)blockIdx.y;
    act[g] = __any(mine[g]) != 0;                         // wave-uniform: somebody in the group is owned here
    L[g] = mine[g] ? pa.L[qi] : INFINITY;                 // (+inf: every exponential of a query owned elsewhere is 0)
    want[g] = mine[g] ? pa.resid[qi] : INFINITY;
    cum[g] = rb[g] = 0.0f;
    rt[g] = t0;
    done[g] = false;
  }

  keys.load(a, pda.prec, pda.stride_p, t0, skey, spart);
  keys.store(a, sk[0], sb[0], skey, spart);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) keys.load(a, pda.prec, pda.stride_p, t + 1, skey, spart);
    float af[4][DC];
    pw_v4f seed[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sb[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      if (!act[g]) continue;
      pw_v4f acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
      }
      float e = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) e += __builtin_amdgcn_exp2f(acc[u][r] - L[g]);
      e = pw_rows_sum(e);                                 // the chunk's mass, the same bits in the query's four lanes
      if (!done[g] && e > 0.0f) {
        rt[g] = t;
        rb[g] = cum[g];
        done[g] = cum[g] + e >= want[g];
      }
      cum[g] += e;
    }
    if (more) keys.store(a, sk[buf ^ 1], sb[buf ^ 1], skey, spart);
    __syncthreads();
  }

#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    const int qi = q0 + 16 * g + col;
    if (quad == 0 && mine[g]) {
      pa.rchunk[qi] = rt[g];
      pa.rbefore[qi] = rb[g];
    }
  }
}

// one thread per query: the recorded chunk key by key, every key scored with its own precisions:
// score = kb + sum_j (p k~)(q~ log2 e) + sum_j (-1/2 p)(q~^2 log2 e).  An owned query has no poisoned live key (k_pw_pick_plan).
__global__ __launch_bounds__(kPwThreads) void k_pw_pick_finish_diag(const PwPickDiagArgs pda) {
  const PwPickArgs& pa = pda.pa;
  const PwArgs& a = pa.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q || pa.own[r] < 0) return;                // (no pick: k_pw_pick_plan wrote the -1)
  float ql[GJX_PAIRWISE_DIAG_MAX_DIM], qq[GJX_PAIRWISE_DIAG_MAX_DIM];
#pragma unroll
  for (int i = 0; i < GJX_PAIRWISE_DIAG_MAX_DIM; ++i) {
    const float x = i < a.d ? a.q[(int64_t)i * a.stride_q + r] - (a.centre ? a.centre[i] : 0.0f) : 0.0f;
    ql[i] = x * kPwLog2e;
    qq[i] = x * x * kPwLog2e;
  }
  const float L = pa.L[r], want = pa.resid[r] - pa.rbefore[r];
  const int t = min(max(pa.rchunk[r], 0), a.n_tiles - 1);
  const int c0 = t * kPwTile, c1 = min(c0 + kPwTile, a.n_k);
  float cum = 0.0f, top = -INFINITY;
  int pick = -1, last = -1, topc = -1;
  for (int c = c0; c < c1 && pick < 0; ++c) {
    const float b = a.bias ? a.bias[c] : 0.0f;
    if (!(b > -INFINITY)) continue;                       // dead
    float k2 = 0.0f, dot = 0.0f;
#pragma unroll
    for (int i = 0; i < GJX_PAIRWISE_DIAG_MAX_DIM; ++i) {
      if (i >= a.d) break;
      const float x = a.k[(int64_t)i * a.stride_k + c] - (a.centre ? a.centre[i] : 0.0f);
      const float p = pda.prec[(int64_t)i * pda.stride_p + c], lin = p * x;
      k2 = fmaf(lin, x, k2);
      dot = fmaf(-0.5f * p, qq[i], fmaf(lin, ql[i], dot));
    }
    const float sc = (b - 0.5f * k2) * kPwLog2e + dot;
    if (sc > top) { top = sc; topc = c; }
    const float e = __builtin_amdgcn_exp2f(sc - L);
    if (e > 0.0f) {
      last = c;
      cum += e;
      if (cum >= want) pick = c;
    }
  }
  pa.pick[r] = pick >= 0 ? pick : (last >= 0 ? last : topc);
}

template <int DC>
static void pw_pick_diag_launch(const PwPickDiagArgs& pda, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(k_pw_pick_diag<DC>, grid, dim3(kPwThreads), 0, st, pda);
}

// ---- gjx_pairwise_gauss_argmax, gjx_pairwise_gauss_argmax_diag:  max[r] = max_c score(r, c),  arg[r] = the smallest c that attains it ----
//
// The max-plus twin of k_pw_lse / k_pw_lse_diag<KEYS> (the K x K part of the particle Viterbi recursion; with no bias, nearest key).
// Scores are made as there: same centring, same zeroing of dead, tail and poisoned keys, kb as the C operand, pw_plan's grid and key
// splits, 64-key tiles through double-buffered LDS under one barrier per tile; the diagonal kernel stages through PwDiagKeys<DC>.
//
// The running pair.  A lane's 16 accumulators of a tile and query group are the keys 64 t + 16 u + 4 quad + i of ONE query, so (max,
// index) is lane-local for the whole key loop and there is no exponential anywhere.  Per tile and group: the tile's maximum joined
// with the running one by 8 v_max3_f32; the index is touched only where the maximum rises STRICTLY (mn > m: an exec-masked region the
// wave skips when no lane rises): a compare/select chain over the 16 accumulators from the last to the first leaves the first one
// equal to mn.  Strictly: an equal score in a later tile never replaces an earlier key.  After the loop the four lanes of a query are
// joined by (larger max, then smaller index), the split leaves {max, index} in part[split][query] (8 bytes: the lse's workspace), and
// k_pw_argmax_merge, one thread per query, folds the splits in index order with strict >, adds the query's own term and converts
// from units of log 2.  The smallest index among bit-equal scores wins at every level.  No atomics, no block waits for another,
// nothing depends on the workspace's contents: bit-reproducible.
//
// Poison.  fmaxf drops a NaN, so the kb = NaN of a poisoned live key would vanish in the maximum where it spreads through the lse's
// sum.  It is carried outside the arithmetic: the staging thread that writes a NaN kb sets a sticky flag, one __syncthreads_or after
// the loop makes it the block's, and a poisoned block writes max = NaN into its partials.  Every block of a split stages every key
// of the split, so every query sees it; the merge answers NaN / -1.  The loop pays nothing for it.  A bias of +inf is poison too
// (the isotropic kernel's staging tests it here; PwDiagKeys already does).  A query's own verdict (non-finite centred coordinate or
// norm) is the merge's, as in k_pw_merge; a score that overflows to +inf is NaN / -1 as well.
struct PwArgmaxArgs {
  PwArgs pw;               // pw.out: the maxima, or NULL; pw.part[split][query] = {max in units of log 2, the index's bits}; diag: pw.p = 0
  int32_t* arg;
  const float* prec;       // the diagonal call: f32[d][stride_p], a column per key
  int64_t stride_p;
};

// one staged tile against the wave's four query groups; base = 64 tile + 4 quad, the lane's first key
template <int DC>
GJX_DEV void pw_argmax_tile(const float* sk, const float* sb, const float (&qf)[kPwGroups][DC], int base, int col, int quad,
                            float (&m)[kPwGroups], int (&idx)[kPwGroups]) {
  float af[4][DC];
  pw_v4f seed[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {                           // the tile's four 16-key subtiles
    seed[u] = *reinterpret_cast<const pw_v4f*>(&sb[16 * u + 4 * quad]);
#pragma unroll
    for (int c = 0; c < DC; ++c) af[u][c] = sk[(4 * c + quad) * kPwLd + 16 * u + col];
  }
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    pw_v4f acc[4];
    float mn = m[g];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[u] = seed[u];
#pragma unroll
      for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
      mn = fmaxf(fmaxf(fmaxf(fmaxf(mn, acc[u][0]), acc[u][1]), acc[u][2]), acc[u][3]);          // (fmaxf drops a NaN)
    }
    if (mn > m[g]) {                                      // some accumulator IS mn: the first of them, in key order
      int j = 0;
#pragma unroll
      for (int u = 3; u >= 0; --u)
#pragma unroll
        for (int i = 3; i >= 0; --i) j = acc[u][i] == mn ? 16 * u + i : j;
      m[g] = mn;
      idx[g] = base + j;
    }
  }
}

// the four lanes of a query, the block's poison, the partial
GJX_DEV void pw_argmax_partial(const PwArgs& a, int q0, int col, int quad, bool bad, float (&m)[kPwGroups], int (&idx)[kPwGroups]) {
  const bool poisoned = __syncthreads_or(bad) != 0;
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float om = __shfl_xor(m[g], off, 64);
      const int oi = __shfl_xor(idx[g], off, 64);
      const bool take = om > m[g] || (om == m[g] && oi < idx[g]);       // (no key yet: -inf and -1 on both sides)
      m[g] = take ? om : m[g];
      idx[g] = take ? oi : idx[g];
    }
    const int qi = q0 + 16 * g + col;
    if (quad == 0 && qi < a.n_q)
      a.part[(int64_t)blockIdx.y * a.n_q + qi] = make_float2(poisoned ? NAN : m[g], __int_as_float(idx[g]));
  }
}

template <int DC>
__global__ __launch_bounds__(kPwThreads) void k_pw_argmax(const PwArgmaxArgs aa) {
  const PwArgs& a = aa.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;            // the MFMA's view of the lane
  const int skey = tid >> 2, spart = tid & 3;             // the staging's view: key of the tile, components 4 c + spart

  // the wave's query fragments, for the whole kernel
  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  const float ps = a.p * kPwLog2e;
  float qf[kPwGroups][DC];
  float scen[DC];
#pragma unroll
  for (int c = 0; c < DC; ++c) {
    const int dq = 4 * c + quad, ds = 4 * c + spart;
    const float cen = (a.centre && dq < a.d) ? a.centre[dq] : 0.0f;
    scen[c] = (a.centre && ds < a.d) ? a.centre[ds] : 0.0f;
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      const int qi = q0 + 16 * g + col;
      qf[g][c] = (dq < a.d && qi < a.n_q) ? (a.q[(int64_t)dq * a.stride_q + qi] - cen) * ps : 0.0f;
    }
  }

  float v[DC], b;
  bool bad = false;                                       // this thread staged a poisoned key
  auto load = [&](int tile) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int ds = 4 * c + spart;
      v[c] = (in && ds < a.d) ? a.k[(int64_t)ds * a.stride_k + key] - scen[c] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    float k2 = 0.0f;
#pragma unroll
    for (int c = 0; c < DC; ++c) k2 = fmaf(v[c], v[c], k2);
    k2 = quad_sum(k2);
    const bool dead = !(b > -INFINITY);                   // -inf or NaN
    const bool zero = dead || !(k2 < INFINITY) || !(b < INFINITY);
    bad |= zero && !dead;
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[buf][(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : v[c];
    if (spart == 0) sb[buf][skey] = dead ? -INFINITY : (zero ? NAN : (b - 0.5f * a.p * k2) * kPwLog2e);
  };

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  float m[kPwGroups];
  int idx[kPwGroups];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) { m[g] = -INFINITY; idx[g] = -1; }

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    pw_argmax_tile<DC>(sk[buf], sb[buf], qf, t * kPwTile + 4 * quad, col, quad, m, idx);
    if (more) store(buf ^ 1);
    __syncthreads();
  }
  pw_argmax_partial(a, q0, col, quad, bad, m, idx);
}

// the same loop over k_pw_lse_diag<DC, KEYS>'s scores: PwDiagKeys stages the 2 d features; the poison is read off the kb it wrote
template <int DC>
__global__ __launch_bounds__(kPwThreads) void k_pw_argmax_diag(const PwArgmaxArgs aa) {
  const PwArgs& a = aa.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int skey = tid >> 2, spart = tid & 3;

  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  float qf[kPwGroups][DC];
  PwDiagKeys<DC> keys;
  keys.queries(a, q0, col, quad, spart, qf);

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  float m[kPwGroups];
  int idx[kPwGroups];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) { m[g] = -INFINITY; idx[g] = -1; }
  bool bad = false;
  auto stage = [&](int buf) {
    keys.store(a, sk[buf], sb[buf], skey, spart);
    if (spart == 0) bad |= sb[buf][skey] != sb[buf][skey];                // (its own store: a live key staged as NaN)
  };

  keys.load(a, aa.prec, aa.stride_p, t0, skey, spart);
  stage(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) keys.load(a, aa.prec, aa.stride_p, t + 1, skey, spart);
    pw_argmax_tile<DC>(sk[buf], sb[buf], qf, t * kPwTile + 4 * quad, col, quad, m, idx);
    if (more) stage(buf ^ 1);
    __syncthreads();
  }
  pw_argmax_partial(a, q0, col, quad, bad, m, idx);
}

// one thread per query: the splits in index order (strict >: the earlier split keeps a tie), the query's own term and verdict.  The
// diagonal call runs it with p = 0: under the keys side a query adds nothing and its verdict is the finiteness of sum_j q~_j^2.
__global__ __launch_bounds__(kPwThreads) void k_pw_argmax_merge(const PwArgmaxArgs aa) {
  const PwArgs& a = aa.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q) return;
  float q2 = 0.0f;
  for (int i = 0; i < a.d; ++i) {
    const float x = a.q[(int64_t)i * a.stride_q + r] - (a.centre ? a.centre[i] : 0.0f);
    q2 = fmaf(x, x, q2);
  }
  float m = -INFINITY;
  int idx = -1;
  bool bad = false;
  for (int y = 0; y < a.n_splits; ++y) {
    const float2 p = a.part[(int64_t)y * a.n_q + r];
    bad |= p.x != p.x;
    if (p.x > m) { m = p.x; idx = __float_as_int(p.y); }
  }
  // no live key: m = -inf, idx = -1
  const bool ok = q2 < INFINITY && !bad && m < INFINITY;
  aa.arg[r] = ok ? idx : -1;
  if (a.out) a.out[r] = ok ? m * kPwLn2 - 0.5f * a.p * q2 : NAN;
}

// both calls after their own checks: chunks = DC, diag picks the kernel
static int pw_argmax_launch(const char* who, const PwArgmaxArgs& aa, int chunks, bool diag, hipStream_t st) {
  const PwArgs& a = aa.pw;
  const dim3 grid((unsigned)((a.n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits), block(kPwThreads);
#define GJX_PW_ARGMAX(DC)                                                     \
  case DC:                                                                    \
    if (diag) hipLaunchKernelGGL(k_pw_argmax_diag<DC>, grid, block, 0, st, aa); \
    else hipLaunchKernelGGL(k_pw_argmax<DC>, grid, block, 0, st, aa);         \
    break;
  switch (chunks) {
    GJX_PW_ARGMAX(1) GJX_PW_ARGMAX(2) GJX_PW_ARGMAX(3) GJX_PW_ARGMAX(4) GJX_PW_ARGMAX(5) GJX_PW_ARGMAX(6) GJX_PW_ARGMAX(7)
    default: GJX_PW_ARGMAX(8)
  }
#undef GJX_PW_ARGMAX
  GJX_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(k_pw_argmax_merge, dim3((unsigned)((a.n_q + kPwThreads - 1) / kPwThreads)), block, 0, st, aa);
  GJX_CHECK_LAUNCH(who);
  return GJX_OK;
}

// ---- gjx_pairwise_t_lse, gjx_pairwise_t_mean: the log-sum-exp and the mean over Student-t scores ----
//
//   score(r, c) = bias[c] - 1/2 (nu + d) log(1 + p |q_r - k_c|^2 / nu)
// the multivariate t with nu degrees of freedom and scale matrix I / p, up to the constant that cancels: FFBSm for heavy-tailed
// transition noise.  The bias sits outside a logarithm, so the matrix product cannot make the score as it does in k_pw_lse.  It makes
// the scaled squared distance instead.  With pn = p / nu and tildes for values minus `centre`:
//   x(r, c) = pn |q~_r|^2 + pn |k~_c|^2 - 2 pn q~_r . k~_c
// The query fragment is scaled by -2 pn; kn_c = pn |k~_c|^2 is computed when the key is staged and enters as the C operand of the
// tile's first MFMA (a 16-byte LDS read per 16 keys, as kb in k_pw_lse); qn = pn |q~_r|^2 is one register per query group, lane-local
// (a lane serves one query per group), summed over the query's four lanes once before the loop.  Per pair, from the accumulator:
//   x  = max(acc + qn, 0)            v_add, v_max: the expansion cancels and a slightly negative x must not reach the logarithm
//   l  = log2(1 + x)                 v_add, v_log_f32 (base 2 already)
//   sc = b2 - a l                    v_fma, a = (nu + d) / 2, b2_c = bias_c log2 e from a second per-tile LDS array (same 16-byte read)
// sc is the score in units of log 2, held in the accumulator's registers: from there on the loop IS k_pw_lse's / k_pw_mean's (tile
// maximum, one v_exp_f32 per pair, one rescale per tile; the mean's shared maximum and second product).  Per pair one quarter-rate
// and four full-rate instructions more than the Gaussian loop.
//
// Edge rules, the family's.  A dead key (bias -inf or NaN) and a key past n_k: zero coordinates, kn = 0, b2 = -inf: x is finite, sc =
// -inf.  A live key whose scaled centred norm pn |k~|^2 is not finite, or whose bias is +inf, is POISON: zero coordinates, kn = 0, b2 =
// NaN.  The clamp would drop a NaN that came through x (fmaxf does), so the poison rides in b2: the fma hands it to the exponential
// and the exponential to every query's sum.  The matrix cores see finite numbers only, but for a bad query's own column.  A query
// whose pn |q~|^2 is not finite gets NaN from the merge (k_pw_merge_t, k_pw_mean_merge_t), for that query alone.  These merges fold
// the splits exactly as k_pw_merge / k_pw_mean_merge and add nothing: the query's term is inside the logarithm.
// Plan, grid, partials, merge order and workspace are the Gaussian calls'.  LDS: one more 64-float array per buffer.
struct PwTArgs {
  PwArgs pw;               // pw.p: the precision
  float pn, a;             // p / nu;  (nu + d) / 2
};

struct PwMeanTArgs {
  PwMeanArgs m;
  float pn, a;
};

// the t kernels' common parts.  Q: the wave's query fragments (x -2 pn) and qn; K: one key's staging
template <int DC>
struct PwT {
  // qf[g][c], qn[g] for the lane's queries q0 + 16 g + col; scen[c] the staging's centre components
  static GJX_DEV void queries(const PwArgs& a, float pn, int q0, int col, int quad, int spart, float (&qf)[kPwGroups][DC],
                              float (&qn)[kPwGroups], float (&scen)[DC]) {
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) qn[g] = 0.0f;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int dq = 4 * c + quad, ds = 4 * c + spart;
      const float cen = (a.centre && dq < a.d) ? a.centre[dq] : 0.0f;
      scen[c] = (a.centre && ds < a.d) ? a.centre[ds] : 0.0f;
#pragma unroll
      for (int g = 0; g < kPwGroups; ++g) {
        const int qi = q0 + 16 * g + col;
        const float x = (dq < a.d && qi < a.n_q) ? a.q[(int64_t)dq * a.stride_q + qi] - cen : 0.0f;
        qn[g] = fmaf(x, x, qn[g]);
        qf[g][c] = x * (-2.0f * pn);
      }
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) qn[g] = pn * pw_rows_sum(qn[g]);       // the same bits in the query's four lanes
  }

  // a staged key: k2 the quad's sum of squares -> zero coordinates?, kn, b2
  static GJX_DEV bool classify(float b, float pn, float k2, float& kn, float& b2) {
    kn = pn * k2;
    const bool dead = !(b > -INFINITY);                   // -inf or NaN
    const bool zero = dead || !(kn < INFINITY) || !(b < INFINITY);
    b2 = dead ? -INFINITY : (zero ? NAN : b * kPwLog2e);
    if (zero) kn = 0.0f;
    return zero;
  }

  // the lane's 16 accumulators of a tile and group (scaled distances without qn) -> scores in units of log 2; returns their maximum
  // joined with mn (fmaxf drops the NaN of a poisoned key: it reaches the sum through the exponential)
  static GJX_DEV float scores(pw_v4f (&acc)[4], const pw_v4f (&b2)[4], float qn, float a, float mn) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = fmaxf(acc[u][r] + qn, 0.0f);
        acc[u][r] = fmaf(-a, __builtin_amdgcn_logf(1.0f + x), b2[u][r]);
      }
      mn = fmaxf(fmaxf(mn, fmaxf(acc[u][0], acc[u][1])), fmaxf(acc[u][2], acc[u][3]));
    }
    return mn;
  }
};

template <int DC>
__global__ __launch_bounds__(kPwThreads) void k_pw_lse_t(const PwTArgs ta) {
  const PwArgs& a = ta.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sn[2][kPwTile];            // kn
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];            // b2
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;            // the MFMA's view of the lane
  const int skey = tid >> 2, spart = tid & 3;             // the staging's view: key of the tile, components 4 c + spart

  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  float qf[kPwGroups][DC], qn[kPwGroups], scen[DC];
  PwT<DC>::queries(a, ta.pn, q0, col, quad, spart, qf, qn, scen);

  float v[DC], b;
  auto load = [&](int tile) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int ds = 4 * c + spart;
      v[c] = (in && ds < a.d) ? a.k[(int64_t)ds * a.stride_k + key] - scen[c] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    float k2 = 0.0f, kn, b2;
#pragma unroll
    for (int c = 0; c < DC; ++c) k2 = fmaf(v[c], v[c], k2);
    const bool zero = PwT<DC>::classify(b, ta.pn, quad_sum(k2), kn, b2);
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[buf][(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : v[c];
    if (spart == 0) { sn[buf][skey] = kn; sb[buf][skey] = b2; }
  };

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  float m[kPwGroups], s[kPwGroups];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) { m[g] = -INFINITY; s[g] = 0.0f; }

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    float af[4][DC];
    pw_v4f seed[4], b2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                         // the tile's four 16-key subtiles
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sn[buf][16 * u + 4 * quad]);
      b2[u] = *reinterpret_cast<const pw_v4f*>(&sb[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      pw_v4f acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
      }
      const float mn = PwT<DC>::scores(acc, b2, qn[g], ta.a, m[g]);
      const float ms = mn > -INFINITY ? mn : 0.0f;
      float e = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) e += __builtin_amdgcn_exp2f(acc[u][r] - ms);
      s[g] = s[g] * __builtin_amdgcn_exp2f(m[g] - ms) + e;
      m[g] = mn;
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // the four lanes of a query, then its partial
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float om = __shfl_xor(m[g], off, 64), os = __shfl_xor(s[g], off, 64);
      pw_fold(m[g], s[g], om, os);
    }
    const int qi = q0 + 16 * g + col;
    if (quad == 0 && qi < a.n_q) a.part[(int64_t)blockIdx.y * a.n_q + qi] = make_float2(m[g], s[g]);
  }
}

// pn |q~_r|^2 of query r: only its finiteness is the merges' business
GJX_DEV float pw_t_query_norm(const PwArgs& a, float pn, int64_t r) {
  float q2 = 0.0f;
  for (int i = 0; i < a.d; ++i) {
    const float x = a.q[(int64_t)i * a.stride_q + r] - (a.centre ? a.centre[i] : 0.0f);
    q2 = fmaf(x, x, q2);
  }
  return pn * q2;
}

// k_pw_merge without the query's own term
__global__ __launch_bounds__(kPwThreads) void k_pw_merge_t(const PwTArgs ta) {
  const PwArgs& a = ta.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q) return;
  float m = -INFINITY, s = 0.0f;
  for (int y = 0; y < a.n_splits; ++y) {
    const float2 p = a.part[(int64_t)y * a.n_q + r];
    pw_fold(m, s, p.x, p.y);
  }
  // no live key: m = -inf, s = 0 -> -inf; a poisoned key: s = NaN -> NaN
  a.out[r] = pw_t_query_norm(a, ta.pn, r) < INFINITY ? (m + __builtin_amdgcn_logf(s)) * kPwLn2 : NAN;
}

template <int DC>
static void pw_t_launch(const PwTArgs& ta, dim3 grid, hipStream_t st) {
  hipLaunchKernelGGL(k_pw_lse_t<DC>, grid, dim3(kPwThreads), 0, st, ta);
}

// k_pw_mean with the t scores: staging of the values, shared maximum, second product and partials as there
template <int DC, int VB>
__global__ __launch_bounds__(kPwThreads) void k_pw_mean_t(const PwMeanTArgs mta) {
  const PwMeanArgs& ma = mta.m;
  const PwArgs& a = ma.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sn[2][kPwTile];            // kn
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];            // b2
  __shared__ __attribute__((aligned(16))) float sv[2][16 * VB * kPwLdV];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int skey = tid >> 2, spart = tid & 3;

  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  float qf[kPwGroups][DC], qn[kPwGroups], scen[DC];
  PwT<DC>::queries(a, mta.pn, q0, col, quad, spart, qf, qn, scen);

  float kv[DC], vv[4 * VB], b;
  auto load = [&](int tile) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int ds = 4 * c + spart;
      kv[c] = (in && ds < a.d) ? a.k[(int64_t)ds * a.stride_k + key] - scen[c] : 0.0f;
    }
#pragma unroll
    for (int c = 0; c < 4 * VB; ++c) {
      const int j = 4 * c + spart;
      vv[c] = (in && j < ma.dv) ? ma.v[(int64_t)j * ma.stride_v + key] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    float k2 = 0.0f, kn, b2;
#pragma unroll
    for (int c = 0; c < DC; ++c) k2 = fmaf(kv[c], kv[c], k2);
    const bool zero = PwT<DC>::classify(b, mta.pn, quad_sum(k2), kn, b2);
    const bool dead = !(b > -INFINITY);
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[buf][(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : kv[c];
#pragma unroll
    for (int c = 0; c < 4 * VB; ++c)
      sv[buf][(4 * c + spart) * kPwLdV + skey] = dead ? 0.0f : (fabsf(vv[c]) < INFINITY ? vv[c] : NAN);
    if (spart == 0) { sn[buf][skey] = kn; sb[buf][skey] = b2; }
  };

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  float m[kPwGroups], s[kPwGroups];
  pw_v4f o[kPwGroups][VB];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    m[g] = -INFINITY;
    s[g] = 0.0f;
#pragma unroll
    for (int vb = 0; vb < VB; ++vb) o[g][vb] = pw_v4f{0.0f, 0.0f, 0.0f, 0.0f};
  }

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    float af[4][DC];
    pw_v4f seed[4], b2[4], vf[4][VB];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sn[buf][16 * u + 4 * quad]);
      b2[u] = *reinterpret_cast<const pw_v4f*>(&sb[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
#pragma unroll
      for (int vb = 0; vb < VB; ++vb)
        vf[u][vb] = *reinterpret_cast<const pw_v4f*>(&sv[buf][(16 * vb + col) * kPwLdV + 16 * u + 4 * quad]);
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      pw_v4f acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
      }
      float mn = PwT<DC>::scores(acc, b2, qn[g], mta.a, m[g]);
      mn = pw_rows_max(mn);                               // the query's four lanes agree before the exponentials
      const float ms = mn > -INFINITY ? mn : 0.0f;
      const float f = __builtin_amdgcn_exp2f(m[g] - ms);
      float e = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          acc[u][r] = __builtin_amdgcn_exp2f(acc[u][r] - ms);
          e += acc[u][r];
        }
      s[g] = s[g] * f + e;
      m[g] = mn;
#pragma unroll
      for (int vb = 0; vb < VB; ++vb) {
        o[g][vb] *= f;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int r = 0; r < 4; ++r) o[g][vb] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[u][vb][r], acc[u][r], o[g][vb], 0, 0, 0);
      }
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // the four lanes of a query share m; their sums are added in one fixed order.  Then the partials.
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    s[g] += __shfl_xor(s[g], 16, 64);
    s[g] += __shfl_xor(s[g], 32, 64);
    const int qi = q0 + 16 * g + col;
    if (qi >= a.n_q) continue;
    if (quad == 0) a.part[(int64_t)blockIdx.y * a.n_q + qi] = make_float2(m[g], s[g]);
#pragma unroll
    for (int vb = 0; vb < VB; ++vb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * vb + 4 * quad + r;
        if (j < ma.dv) ma.opart[((int64_t)blockIdx.y * ma.dv + j) * a.n_q + qi] = o[g][vb][r];
      }
  }
}

// k_pw_mean_merge without the query's own term
__global__ __launch_bounds__(kPwThreads) void k_pw_mean_merge_t(const PwMeanTArgs mta) {
  const PwMeanArgs& ma = mta.m;
  const PwArgs& a = ma.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  const int j = (int)blockIdx.y;
  if (r >= a.n_q) return;
  const bool ok = pw_t_query_norm(a, mta.pn, r) < INFINITY;
  float m = -INFINITY, s = 0.0f;
  for (int y = 0; y < a.n_splits; ++y) {
    const float2 p = a.part[(int64_t)y * a.n_q + r];
    pw_fold(m, s, p.x, p.y);
  }
  const float ms = m > -INFINITY ? m : 0.0f;
  float o = 0.0f;
  for (int y = 0; y < a.n_splits; ++y)
    o = fmaf(ma.opart[((int64_t)y * ma.dv + j) * a.n_q + r], __builtin_amdgcn_exp2f(a.part[(int64_t)y * a.n_q + r].x - ms), o);
  // no live key: 0 / 0 = NaN; a poisoned key: s = NaN; a live key's non-finite value: o = NaN in its row
  ma.mean[(int64_t)j * a.n_q + r] = ok ? o / s : NAN;
  if (j == 0 && a.out) a.out[r] = ok ? (m + __builtin_amdgcn_logf(s)) * kPwLn2 : NAN;
}

template <int DC>
static void pw_mean_t_launch(const PwMeanTArgs& mta, dim3 grid, hipStream_t st) {
  if (mta.m.dv <= 16) hipLaunchKernelGGL((k_pw_mean_t<DC, 1>), grid, dim3(kPwThreads), 0, st, mta);
  else hipLaunchKernelGGL((k_pw_mean_t<DC, 2>), grid, dim3(kPwThreads), 0, st, mta);
}

// precision and dof of the t calls -> pn = p / nu and a = (nu + d) / 2 as floats; false: not positive and finite, or a quotient that is not
static bool pw_t_scalars(float precision, float dof, int32_t d, float* pn, float* a) {
  if (!(precision > 0.0f) || !(precision < INFINITY) || !(dof > 0.0f) || !(dof < INFINITY)) return false;
  *pn = (float)((double)precision / (double)dof);
  *a = (float)(0.5 * ((double)dof + (double)d));
  return *pn > 0.0f && *pn < INFINITY;
}

// ---- gjx_pairwise_t_pick: one key per query with probability proportional to exp(t score), by inverse CDF in key-index order ----
//
// gjx_pairwise_gauss_pick's four launches over the t scores.  1. k_pw_lse_t, unchanged: the partials.  2. k_pw_pick_plan_t, one thread per
// query: k_pw_pick_plan without the query's own term (the t score keeps it inside the logarithm; the query's verdict is the
// finiteness of pn |q~|^2, and the lse it writes is k_pw_merge_t's expression on the same fold: the same bits).  3. k_pw_pick_t: the
// block, staging, group skipping and chunk bookkeeping of k_pw_pick around PwT<DC>'s scores.  With the total L known there is no
// running maximum: per pair v_add, v_max, v_add, v_log_f32, v_fma (the score), v_sub, v_exp_f32, v_add (the mass).  A dead key is
// b2 = -inf -> mass 0; a poisoned key never gets here with an owner (its NaN total left own = -1 everywhere: every group is skipped).
// 4. k_pw_pick_finish_t, one thread per query: the 64 keys of the recorded chunk in the VALU, in the DIRECT form pn |q - k|^2 (no
// expansion, so no centre and no clamp), the fall-backs of k_pw_pick_finish.  Workspace: gjx_pairwise_gauss_pick's layout and size.
struct PwPickTArgs {
  PwPickArgs p;            // p.pw.p: the precision
  float pn, a;             // p / nu;  (nu + d) / 2
};

__global__ __launch_bounds__(kPwThreads) void k_pw_pick_plan_t(const PwPickTArgs pta) {
  const PwPickArgs& pa = pta.p;
  const PwArgs& a = pa.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q) return;
  const bool okq = pw_t_query_norm(a, pta.pn, r) < INFINITY;
  float m = -INFINITY, s = 0.0f;
  for (int y = 0; y < a.n_splits; ++y) {
    const float2 p = a.part[(int64_t)y * a.n_q + r];
    pw_fold(m, s, p.x, p.y);
  }
  const float L = m + __builtin_amdgcn_logf(s);
  if (a.out) a.out[r] = okq ? L * kPwLn2 : NAN;
  const float u = pa.u[r];
  int own = -1;
  float resid = 0.0f;
  if (okq && m > -INFINITY && s == s && u == u) {
    const float target = u >= 1.0f ? INFINITY : fmaxf(u, 0.0f);
    float cum = 0.0f;
    for (int y = 0; y < a.n_splits; ++y) {
      const float2 p = a.part[(int64_t)y * a.n_q + r];
      const float mass = p.y * __builtin_amdgcn_exp2f(p.x - L);
      if (mass > 0.0f) {
        own = y;
        resid = target - cum;
        if (cum + mass >= target) break;
      }
      cum += mass;
    }
  }
  pa.L[r] = L;
  pa.resid[r] = resid;
  pa.own[r] = own;
  if (own < 0) pa.pick[r] = -1;
}

template <int DC>
__global__ __launch_bounds__(kPwThreads) void k_pw_pick_t(const PwPickTArgs pta) {
  const PwPickArgs& pa = pta.p;
  const PwArgs& a = pa.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sn[2][kPwTile];            // kn
  __shared__ __attribute__((aligned(16))) float sb[2][kPwTile];            // b2
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;
  const int skey = tid >> 2, spart = tid & 3;

  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  float qf[kPwGroups][DC], qn[kPwGroups], scen[DC];
  PwT<DC>::queries(a, pta.pn, q0, col, quad, spart, qf, qn, scen);

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  // per group: the query's L and residual target where this split owns it, the running cumulative, the record
  float L[kPwGroups], want[kPwGroups], cum[kPwGroups], rb[kPwGroups];
  int rt[kPwGroups];
  bool mine[kPwGroups], act[kPwGroups], done[kPwGroups];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    const int qi = q0 + 16 * g + col;
    mine[g] = qi < a.n_q && pa.own[qi] == (int)blockIdx.y;
    act[g] = __any(mine[g]) != 0;                         // wave-uniform: somebody in the group is owned here
    L[g] = mine[g] ? pa.L[qi] : INFINITY;                 // (+inf: every exponential of a query owned elsewhere is 0)
    want[g] = mine[g] ? pa.resid[qi] : INFINITY;
    cum[g] = rb[g] = 0.0f;
    rt[g] = t0;
    done[g] = false;
  }

  float v[DC], b;
  auto load = [&](int tile) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int ds = 4 * c + spart;
      v[c] = (in && ds < a.d) ? a.k[(int64_t)ds * a.stride_k + key] - scen[c] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    float k2 = 0.0f, kn, b2;
#pragma unroll
    for (int c = 0; c < DC; ++c) k2 = fmaf(v[c], v[c], k2);
    const bool zero = PwT<DC>::classify(b, pta.pn, quad_sum(k2), kn, b2);
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[buf][(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : v[c];
    if (spart == 0) { sn[buf][skey] = kn; sb[buf][skey] = b2; }
  };

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    float af[4][DC];
    pw_v4f seed[4], b2[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sn[buf][16 * u + 4 * quad]);
      b2[u] = *reinterpret_cast<const pw_v4f*>(&sb[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      if (!act[g]) continue;
      pw_v4f acc[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
      }
      PwT<DC>::scores(acc, b2, qn[g], pta.a, -INFINITY);   // (the maximum is not used: L is known)
      float e = 0.0f;
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) e += __builtin_amdgcn_exp2f(acc[u][r] - L[g]);
      e = pw_rows_sum(e);                                 // the chunk's mass, the same bits in the query's four lanes
      if (!done[g] && e > 0.0f) {
        rt[g] = t;
        rb[g] = cum[g];
        done[g] = cum[g] + e >= want[g];
      }
      cum[g] += e;
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
    const int qi = q0 + 16 * g + col;
    if (quad == 0 && mine[g]) {
      pa.rchunk[qi] = rt[g];
      pa.rbefore[qi] = rb[g];
    }
  }
}

// one thread per query: the recorded chunk key by key, x = pn |q - k|^2 as written
__global__ __launch_bounds__(kPwThreads) void k_pw_pick_finish_t(const PwPickTArgs pta) {
  const PwPickArgs& pa = pta.p;
  const PwArgs& a = pa.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q || pa.own[r] < 0) return;                // (no pick: k_pw_pick_plan_t wrote the -1)
  float qv[GJX_PAIRWISE_MAX_DIM];
#pragma unroll
  for (int i = 0; i < GJX_PAIRWISE_MAX_DIM; ++i) qv[i] = i < a.d ? a.q[(int64_t)i * a.stride_q + r] : 0.0f;
  const float L = pa.L[r], want = pa.resid[r] - pa.rbefore[r];
  const int t = min(max(pa.rchunk[r], 0), a.n_tiles - 1);
  const int c0 = t * kPwTile, c1 = min(c0 + kPwTile, a.n_k);
  float cum = 0.0f, top = -INFINITY;
  int pick = -1, last = -1, topc = -1;
  for (int c = c0; c < c1 && pick < 0; ++c) {
    const float b = a.bias ? a.bias[c] : 0.0f;
    if (!(b > -INFINITY)) continue;                       // dead
    float r2 = 0.0f;
#pragma unroll
    for (int i = 0; i < GJX_PAIRWISE_MAX_DIM; ++i) {
      if (i >= a.d) break;
      const float x = qv[i] - a.k[(int64_t)i * a.stride_k + c];
      r2 = fmaf(x, x, r2);
    }
    const float sc = fmaf(-pta.a, __builtin_amdgcn_logf(1.0f + pta.pn * r2), b * kPwLog2e);
    if (sc > top) { top = sc; topc = c; }
    const float e = __builtin_amdgcn_exp2f(sc - L);
    if (e > 0.0f) {
      last = c;
      cum += e;
      if (cum >= want) pick = c;
    }
  }
  pa.pick[r] = pick >= 0 ? pick : (last >= 0 ? last : topc);
}

// ---- gjx_pairwise_t_argmax:  max[r] = max_c score(r, c),  arg[r] = the smallest c that attains it, under the t score ----
//
// The product form: no transcendental per pair.  With a = (nu + d) / 2, x = pn |q - k|^2 and B the largest live bias,
//   argmax_c [bias_c - a ln(1 + x_c)]  =  argmin_c (1 + x_c) w_c,     w_c = exp((B - bias_c) / a) >= 1,
// and max = B - a ln(min).  w_c is computed ONCE per staged key (one v_exp_f32 by the staging thread) and lies in LDS where the lse keeps
// b2; the matrix cores make x as in k_pw_lse_t (query fragment x -2 pn, kn the C operand, qn + 1 in a register).  Per pair:
//   v = max(acc + (qn + 1), 1) w         v_add, v_max, v_mul
// then k_pw_argmax's lane-local tracking with min for max: 8 v_min3_f32 per tile and group, and only where the minimum falls
// STRICTLY the compare/select chain that finds the first accumulator equal to it.  The four lanes of a query are joined by (smaller
// value, then smaller index), a split leaves {min, index} in part[split][query], and k_pw_argmax_merge_t, one thread per query, folds
// the splits in index order with strict <, and takes the one logarithm: max = B - a ln 2 log2(min).
// B is ONE number per call (k_pw_bias_max, a one-block launch in front, writes it behind the partials): w, and so v, of a key are then
// the same bits in whatever tile, split or block the key is staged, and bit-equal copies of a key tie exactly: the smallest index wins
// at every level.  A dead key, a key past n_k and a poisoned key are staged as zero coordinates, kn = 0, w = +inf: v = +inf never
// falls below anything.  A w that overflows to +inf belongs to a key that cannot win (1 + x is a finite float).  The poison is
// k_pw_argmax's sticky flag (PwT::classify's NaN b2), joined by __syncthreads_or, written as NaN into the block's partials.  A bad
// query's NaN accumulators are clamped to 1 by the v_max: what it tracks is discarded by the merge's own verdict on pn |q~|^2.
// Accuracy: w carries a relative error of about 2^-24 (1 + |B - bias_c| / a), i.e. |B - bias_c| 2^-24 in the score; the winner has
// |B - bias_c| <= a ln(1 + x_B) <= a x_B with x_B the scaled distance to the key that carries B, which the lse's bound already allows.
struct PwArgmaxTArgs {
  PwArgmaxArgs aa;         // aa.pw.out: the maxima, or NULL; aa.pw.part[split][query] = {min of (1 + x) w, the index's bits}
  float* top;              // [1] B, the largest bias (0 without a bias, -inf where nobody lives), written by k_pw_bias_max
  float pn, a;             // p / nu;  (nu + d) / 2
};

// one block: B.  fmaxf drops the NaN of a dead key; -inf is the neutral element; +inf stays (the staging calls that key poison)
__global__ __launch_bounds__(kPwThreads) void k_pw_bias_max(const PwArgmaxTArgs ata) {
  __shared__ float sm[kPwThreads / 64];
  const PwArgs& a = ata.aa.pw;
  float m = a.bias ? -INFINITY : 0.0f;
  if (a.bias)
    for (int c = threadIdx.x; c < a.n_k; c += kPwThreads) m = fmaxf(m, a.bias[c]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) *ata.top = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

template <int DC>
__global__ __launch_bounds__(kPwThreads) void k_pw_argmax_t(const PwArgmaxTArgs ata) {
  const PwArgs& a = ata.aa.pw;
  __shared__ float sk[2][4 * DC * kPwLd];
  __shared__ __attribute__((aligned(16))) float sn[2][kPwTile];            // kn
  __shared__ __attribute__((aligned(16))) float sw[2][kPwTile];            // w
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, quad = lane >> 4;            // the MFMA's view of the lane
  const int skey = tid >> 2, spart = tid & 3;             // the staging's view: key of the tile, components 4 c + spart

  const int q0 = (int)blockIdx.x * kPwBlockQ + wave * 16 * kPwGroups;
  float qf[kPwGroups][DC], qn[kPwGroups], scen[DC];
  PwT<DC>::queries(a, ata.pn, q0, col, quad, spart, qf, qn, scen);
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) qn[g] += 1.0f;      // 1 + x = acc + (qn + 1)
  const float B = *ata.top, ia = kPwLog2e / ata.a;

  float v[DC], b;
  bool bad = false;                                       // this thread staged a poisoned key
  auto load = [&](int tile) {
    const int key = tile * kPwTile + skey;
    const bool in = key < a.n_k;
    b = in ? (a.bias ? a.bias[key] : 0.0f) : -INFINITY;
#pragma unroll
    for (int c = 0; c < DC; ++c) {
      const int ds = 4 * c + spart;
      v[c] = (in && ds < a.d) ? a.k[(int64_t)ds * a.stride_k + key] - scen[c] : 0.0f;
    }
  };
  auto store = [&](int buf) {
    float k2 = 0.0f, kn, b2;
#pragma unroll
    for (int c = 0; c < DC; ++c) k2 = fmaf(v[c], v[c], k2);
    const bool zero = PwT<DC>::classify(b, ata.pn, quad_sum(k2), kn, b2);
    bad |= b2 != b2;
#pragma unroll
    for (int c = 0; c < DC; ++c) sk[buf][(4 * c + spart) * kPwLd + skey] = zero ? 0.0f : v[c];
    if (spart == 0) { sn[buf][skey] = kn; sw[buf][skey] = zero ? INFINITY : __builtin_amdgcn_exp2f((B - b) * ia); }
  };

  const int t0 = (int)blockIdx.y * a.tiles_per_split;
  const int t1 = min(t0 + a.tiles_per_split, a.n_tiles);
  float m[kPwGroups];
  int idx[kPwGroups];
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) { m[g] = INFINITY; idx[g] = -1; }

  load(t0);
  store(0);
  __syncthreads();
  for (int t = t0; t < t1; ++t) {
    const int buf = (t - t0) & 1;
    const bool more = t + 1 < t1;                         // block-uniform
    if (more) load(t + 1);
    float af[4][DC];
    pw_v4f seed[4], w[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {                         // the tile's four 16-key subtiles
      seed[u] = *reinterpret_cast<const pw_v4f*>(&sn[buf][16 * u + 4 * quad]);
      w[u] = *reinterpret_cast<const pw_v4f*>(&sw[buf][16 * u + 4 * quad]);
#pragma unroll
      for (int c = 0; c < DC; ++c) af[u][c] = sk[buf][(4 * c + quad) * kPwLd + 16 * u + col];
    }
#pragma unroll
    for (int g = 0; g < kPwGroups; ++g) {
      pw_v4f acc[4];
      float mn = m[g];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        acc[u] = seed[u];
#pragma unroll
        for (int c = 0; c < DC; ++c) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][c], qf[g][c], acc[u], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[u][i] = fmaxf(acc[u][i] + qn[g], 1.0f) * w[u][i];      // (fmaxf drops a bad query's NaN)
        mn = fminf(fminf(fminf(fminf(mn, acc[u][0]), acc[u][1]), acc[u][2]), acc[u][3]);
      }
      if (mn < m[g]) {                                    // some accumulator IS mn: the first of them, in key order
        int j = 0;
#pragma unroll
        for (int u = 3; u >= 0; --u)
#pragma unroll
          for (int i = 3; i >= 0; --i) j = acc[u][i] == mn ? 16 * u + i : j;
        m[g] = mn;
        idx[g] = t * kPwTile + 4 * quad + j;
      }
    }
    if (more) store(buf ^ 1);
    __syncthreads();
  }

  // the four lanes of a query, the block's poison, the partial
  const bool poisoned = __syncthreads_or(bad) != 0;
#pragma unroll
  for (int g = 0; g < kPwGroups; ++g) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const float om = __shfl_xor(m[g], off, 64);
      const int oi = __shfl_xor(idx[g], off, 64);
      const bool take = om < m[g] || (om == m[g] && oi < idx[g]);       // (no key yet: +inf and -1 on both sides)
      m[g] = take ? om : m[g];
      idx[g] = take ? oi : idx[g];
    }
    const int qi = q0 + 16 * g + col;
    if (quad == 0 && qi < a.n_q)
      a.part[(int64_t)blockIdx.y * a.n_q + qi] = make_float2(poisoned ? NAN : m[g], __int_as_float(idx[g]));
  }
}

// one thread per query: the splits in index order (strict <: the earlier split keeps a tie), the query's verdict, the one logarithm
__global__ __launch_bounds__(kPwThreads) void k_pw_argmax_merge_t(const PwArgmaxTArgs ata) {
  const PwArgs& a = ata.aa.pw;
  const int64_t r = (int64_t)blockIdx.x * kPwThreads + threadIdx.x;
  if (r >= a.n_q) return;
  float m = INFINITY;
  int idx = -1;
  bool bad = false;
  for (int y = 0; y < a.n_splits; ++y) {
    const float2 p = a.part[(int64_t)y * a.n_q + r];
    bad |= p.x != p.x;
    if (p.x < m) { m = p.x; idx = __float_as_int(p.y); }
  }
  // no live key, or every 1 + x overflowed: m = +inf, idx = -1, max = -inf
  const bool ok = pw_t_query_norm(a, ata.pn, r) < INFINITY && !bad;
  ata.aa.arg[r] = ok ? idx : -1;
  if (a.out) a.out[r] = ok ? fmaf(-ata.a * kPwLn2, __builtin_amdgcn_logf(m), *ata.top) : NAN;
}

// the instance for DC = ceil(d / 4) chunks of a kernel template over one argument struct
#define GJX_PW_T_DISPATCH(KERNEL, d, grid, st, args)                                                    \
  switch (((d) + 3) / 4) {                                                                              \
    case 1: hipLaunchKernelGGL(KERNEL<1>, grid, dim3(kPwThreads), 0, st, args); break;                  \
    case 2: hipLaunchKernelGGL(KERNEL<2>, grid, dim3(kPwThreads), 0, st, args); break;                  \
    case 3: hipLaunchKernelGGL(KERNEL<3>, grid, dim3(kPwThreads), 0, st, args); break;                  \
    case 4: hipLaunchKernelGGL(KERNEL<4>, grid, dim3(kPwThreads), 0, st, args); break;                  \
    case 5: hipLaunchKernelGGL(KERNEL<5>, grid, dim3(kPwThreads), 0, st, args); break;                  \
    case 6: hipLaunchKernelGGL(KERNEL<6>, grid, dim3(kPwThreads), 0, st, args); break;                  \
    case 7: hipLaunchKernelGGL(KERNEL<7>, grid, dim3(kPwThreads), 0, st, args); break;                  \
    default: hipLaunchKernelGGL(KERNEL<8>, grid, dim3(kPwThreads), 0, st, args); break;                 \
  }

}  // namespace gjx

extern "C" size_t gjx_pairwise_gauss_lse_workspace_bytes(int64_t n_q, int64_t n_k, int32_t d) {
  gjx::PwArgs a;
  if (!gjx::pw_plan(n_q, n_k, d, &a)) return 0;
  return 8 + sizeof(float2) * (size_t)a.n_splits * (size_t)n_q;          // (8: the alignment of any pointer)
}

extern "C" int gjx_pairwise_gauss_lse(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k,
                                      int32_t d, const float* bias, float precision, const float* centre, float* out, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  using namespace gjx;
  if (!q || !k || !out || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      stride_q < n_q || stride_k < n_k || !(precision > 0.0f) || !(precision < INFINITY))
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_gauss_lse: bad argument");
  if (d > GJX_PAIRWISE_MAX_DIM) return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_gauss_lse: more than GJX_PAIRWISE_MAX_DIM components");
  PwArgs a;
  memset(&a, 0, sizeof(a));
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_lse_workspace_bytes(n_q, n_k, d))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_gauss_lse: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = out;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = precision;
  const dim3 grid((unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits);
  switch ((d + 3) / 4) {
    case 1: pw_launch<1>(a, grid, st); break;
    case 2: pw_launch<2>(a, grid, st); break;
    case 3: pw_launch<3>(a, grid, st); break;
    case 4: pw_launch<4>(a, grid, st); break;
    case 5: pw_launch<5>(a, grid, st); break;
    case 6: pw_launch<6>(a, grid, st); break;
    case 7: pw_launch<7>(a, grid, st); break;
    default: pw_launch<8>(a, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_lse(lse)");
  hipLaunchKernelGGL(k_pw_merge, dim3((unsigned)((n_q + kPwThreads - 1) / kPwThreads)), dim3(kPwThreads), 0, st, a);
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_lse(merge)");
  return GJX_OK;
}

extern "C" size_t gjx_pairwise_gauss_mean_workspace_bytes(int64_t n_q, int64_t n_k, int32_t d, int32_t dv) {
  gjx::PwArgs a;
  if (dv <= 0 || dv > GJX_PAIRWISE_MAX_DIM || !gjx::pw_plan(n_q, n_k, d, &a)) return 0;
  return 8 + (sizeof(float2) + sizeof(float) * (size_t)dv) * (size_t)a.n_splits * (size_t)n_q;
}

extern "C" int gjx_pairwise_gauss_mean(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k,
                                       int32_t d, const float* v, int64_t stride_v, int32_t dv, const float* bias, float precision,
                                       const float* centre, float* mean, float* lse, void* workspace, size_t workspace_bytes,
                                       void* stream) {
  using namespace gjx;
  if (!q || !k || !v || !mean || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      dv <= 0 || stride_q < n_q || stride_k < n_k || stride_v < n_k || !(precision > 0.0f) || !(precision < INFINITY))
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_gauss_mean: bad argument");
  if (d > GJX_PAIRWISE_MAX_DIM || dv > GJX_PAIRWISE_MAX_DIM)
    return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_gauss_mean: more than GJX_PAIRWISE_MAX_DIM components");
  PwMeanArgs ma;
  memset(&ma, 0, sizeof(ma));
  PwArgs& a = ma.pw;
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_mean_workspace_bytes(n_q, n_k, d, dv))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_gauss_mean: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = lse;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = precision;
  ma.v = v; ma.mean = mean; ma.stride_v = stride_v; ma.dv = dv;
  ma.opart = (float*)(a.part + (size_t)a.n_splits * (size_t)n_q);
  const unsigned n_qb = (unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ);
  const dim3 grid(n_qb, (unsigned)a.n_splits);
  switch ((d + 3) / 4) {
    case 1: pw_mean_launch<1>(ma, grid, st); break;
    case 2: pw_mean_launch<2>(ma, grid, st); break;
    case 3: pw_mean_launch<3>(ma, grid, st); break;
    case 4: pw_mean_launch<4>(ma, grid, st); break;
    case 5: pw_mean_launch<5>(ma, grid, st); break;
    case 6: pw_mean_launch<6>(ma, grid, st); break;
    case 7: pw_mean_launch<7>(ma, grid, st); break;
    default: pw_mean_launch<8>(ma, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_mean(mean)");
  hipLaunchKernelGGL(k_pw_mean_merge, dim3((unsigned)((n_q + kPwThreads - 1) / kPwThreads), (unsigned)dv), dim3(kPwThreads), 0, st, ma);
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_mean(merge)");
  return GJX_OK;
}

extern "C" size_t gjx_pairwise_gauss_pick_workspace_bytes(int64_t n_q, int64_t n_k, int32_t d) {
  gjx::PwArgs a;
  if (!gjx::pw_plan(n_q, n_k, d, &a)) return 0;
  return 8 + (sizeof(float2) * (size_t)a.n_splits + 5 * sizeof(float)) * (size_t)n_q;
}

extern "C" int gjx_pairwise_gauss_pick(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k,
                                       int32_t d, const float* bias, float precision, const float* centre, const float* u, int32_t* pick,
                                       float* lse, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  if (!q || !k || !u || !pick || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      stride_q < n_q || stride_k < n_k || !(precision > 0.0f) || !(precision < INFINITY))
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_gauss_pick: bad argument");
  if (d > GJX_PAIRWISE_MAX_DIM) return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_gauss_pick: more than GJX_PAIRWISE_MAX_DIM components");
  PwPickArgs pa;
  memset(&pa, 0, sizeof(pa));
  PwArgs& a = pa.pw;
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_pick_workspace_bytes(n_q, n_k, d))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_gauss_pick: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = lse;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = precision;
  pa.u = u; pa.pick = pick;
  pa.L = (float*)(a.part + (size_t)a.n_splits * (size_t)n_q);
  pa.resid = pa.L + n_q;
  pa.rbefore = pa.resid + n_q;
  pa.own = (int32_t*)(pa.rbefore + n_q);
  pa.rchunk = pa.own + n_q;
  const dim3 grid((unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits);
  const dim3 per_query((unsigned)((n_q + kPwThreads - 1) / kPwThreads));
  switch ((d + 3) / 4) {
    case 1: pw_launch<1>(a, grid, st); break;
    case 2: pw_launch<2>(a, grid, st); break;
    case 3: pw_launch<3>(a, grid, st); break;
    case 4: pw_launch<4>(a, grid, st); break;
    case 5: pw_launch<5>(a, grid, st); break;
    case 6: pw_launch<6>(a, grid, st); break;
    case 7: pw_launch<7>(a, grid, st); break;
    default: pw_launch<8>(a, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_pick(lse)");
  hipLaunchKernelGGL(k_pw_pick_plan, per_query, dim3(kPwThreads), 0, st, pa);
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_pick(plan)");
  switch ((d + 3) / 4) {
    case 1: pw_pick_launch<1>(pa, grid, st); break;
    case 2: pw_pick_launch<2>(pa, grid, st); break;
    case 3: pw_pick_launch<3>(pa, grid, st); break;
    case 4: pw_pick_launch<4>(pa, grid, st); break;
    case 5: pw_pick_launch<5>(pa, grid, st); break;
    case 6: pw_pick_launch<6>(pa, grid, st); break;
    case 7: pw_pick_launch<7>(pa, grid, st); break;
    default: pw_pick_launch<8>(pa, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_pick(pick)");
  hipLaunchKernelGGL(k_pw_pick_finish, per_query, dim3(kPwThreads), 0, st, pa);
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_pick(finish)");
  return GJX_OK;
}

extern "C" size_t gjx_pairwise_gauss_lse_diag_workspace_bytes(int64_t n_q, int64_t n_k, int32_t d) {
  if (d > GJX_PAIRWISE_DIAG_MAX_DIM) return 0;
  return gjx_pairwise_gauss_lse_workspace_bytes(n_q, n_k, d);
}

extern "C" int gjx_pairwise_gauss_lse_diag(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k,
                                           int32_t d, const float* bias, const float* prec, int64_t stride_p, int32_t prec_side,
                                           const float* centre, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  const bool keys = prec_side == GJX_PAIRWISE_PREC_KEYS;
  if (!q || !k || !prec || !out || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      stride_q < n_q || stride_k < n_k || (!keys && prec_side != GJX_PAIRWISE_PREC_QUERIES) || stride_p < (keys ? n_k : n_q))
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_gauss_lse_diag: bad argument");
  if (d > GJX_PAIRWISE_DIAG_MAX_DIM)
    return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_gauss_lse_diag: more than GJX_PAIRWISE_DIAG_MAX_DIM components");
  PwDiagArgs da;
  memset(&da, 0, sizeof(da));
  PwArgs& a = da.pw;
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_lse_diag_workspace_bytes(n_q, n_k, d))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_gauss_lse_diag: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = out;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k;
  da.prec = prec; da.stride_p = stride_p; da.side = prec_side;
  const dim3 grid((unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits);
  switch ((2 * d + 3) / 4) {                              // chunks of 4 features
    case 1: pw_diag_launch<1>(da, grid, st); break;
    case 2: pw_diag_launch<2>(da, grid, st); break;
    case 3: pw_diag_launch<3>(da, grid, st); break;
    case 4: pw_diag_launch<4>(da, grid, st); break;
    case 5: pw_diag_launch<5>(da, grid, st); break;
    case 6: pw_diag_launch<6>(da, grid, st); break;
    case 7: pw_diag_launch<7>(da, grid, st); break;
    default: pw_diag_launch<8>(da, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_lse_diag(lse)");
  hipLaunchKernelGGL(k_pw_merge_diag, dim3((unsigned)((n_q + kPwThreads - 1) / kPwThreads)), dim3(kPwThreads), 0, st, da);
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_lse_diag(merge)");
  return GJX_OK;
}

// what the two KEYS-only diag calls refuse beyond their isotropic siblings' own checks; GJX_OK: go on
static int pw_diag_keys_only(const char* who, const float* prec, int64_t stride_p, int64_t n_k, int32_t prec_side, int32_t d) {
  const bool queries = prec_side == GJX_PAIRWISE_PREC_QUERIES;
  const bool bad = !queries && (!prec || prec_side != GJX_PAIRWISE_PREC_KEYS || stride_p < n_k);
  if (!queries && !bad && d <= GJX_PAIRWISE_DIAG_MAX_DIM) return GJX_OK;
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", who, queries ? "GJX_PAIRWISE_PREC_QUERIES is not served, only GJX_PAIRWISE_PREC_KEYS"
                                            : bad   ? "bad argument" : "more than GJX_PAIRWISE_DIAG_MAX_DIM components");
  return gjx_fail(bad ? GJX_EINVAL : GJX_EUNSUPPORTED, msg);
}

extern "C" size_t gjx_pairwise_gauss_mean_diag_workspace_bytes(int64_t n_q, int64_t n_k, int32_t d, int32_t dv) {
  if (d > GJX_PAIRWISE_DIAG_MAX_DIM) return 0;
  return gjx_pairwise_gauss_mean_workspace_bytes(n_q, n_k, d, dv);
}

extern "C" int gjx_pairwise_gauss_mean_diag(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k,
                                            int32_t d, const float* v, int64_t stride_v, int32_t dv, const float* bias, const float* prec,
                                            int64_t stride_p, int32_t prec_side, const float* centre, float* mean, float* lse,
                                            void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  if (!q || !k || !v || !mean || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      dv <= 0 || stride_q < n_q || stride_k < n_k || stride_v < n_k)
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_gauss_mean_diag: bad argument");
  if (const int rc = pw_diag_keys_only("gjx_pairwise_gauss_mean_diag", prec, stride_p, n_k, prec_side, d)) return rc;
  if (dv > GJX_PAIRWISE_MAX_DIM)
    return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_gauss_mean_diag: more than GJX_PAIRWISE_MAX_DIM value components");
  PwMeanDiagArgs mda;
  memset(&mda, 0, sizeof(mda));
  PwMeanArgs& ma = mda.ma;
  PwArgs& a = ma.pw;
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_mean_diag_workspace_bytes(n_q, n_k, d, dv))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_gauss_mean_diag: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = lse;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = 0.0f;             // (0: k_pw_mean_merge then adds no query term)
  ma.v = v; ma.mean = mean; ma.stride_v = stride_v; ma.dv = dv;
  ma.opart = (float*)(a.part + (size_t)a.n_splits * (size_t)n_q);
  mda.prec = prec; mda.stride_p = stride_p;
  const dim3 grid((unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits);
  switch ((2 * d + 3) / 4) {                              // chunks of 4 features
    case 1: pw_mean_diag_launch<1>(mda, grid, st); break;
    case 2: pw_mean_diag_launch<2>(mda, grid, st); break;
    case 3: pw_mean_diag_launch<3>(mda, grid, st); break;
    case 4: pw_mean_diag_launch<4>(mda, grid, st); break;
    case 5: pw_mean_diag_launch<5>(mda, grid, st); break;
    case 6: pw_mean_diag_launch<6>(mda, grid, st); break;
    case 7: pw_mean_diag_launch<7>(mda, grid, st); break;
    default: pw_mean_diag_launch<8>(mda, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_mean_diag(mean)");
  hipLaunchKernelGGL(k_pw_mean_merge, dim3((unsigned)((n_q + kPwThreads - 1) / kPwThreads), (unsigned)dv), dim3(kPwThreads), 0, st, ma);
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_mean_diag(merge)");
  return GJX_OK;
}

extern "C" size_t gjx_pairwise_gauss_pick_diag_workspace_bytes(int64_t n_q, int64_t n_k, int32_t d) {
  if (d > GJX_PAIRWISE_DIAG_MAX_DIM) return 0;
  return gjx_pairwise_gauss_pick_workspace_bytes(n_q, n_k, d);
}

extern "C" int gjx_pairwise_gauss_pick_diag(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k,
                                            int32_t d, const float* bias, const float* prec, int64_t stride_p, int32_t prec_side,
                                            const float* centre, const float* u, int32_t* pick, float* lse, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  using namespace gjx;
  if (!q || !k || !u || !pick || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      stride_q < n_q || stride_k < n_k)
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_gauss_pick_diag: bad argument");
  if (const int rc = pw_diag_keys_only("gjx_pairwise_gauss_pick_diag", prec, stride_p, n_k, prec_side, d)) return rc;
  PwPickDiagArgs pda;
  memset(&pda, 0, sizeof(pda));
  PwPickArgs& pa = pda.pa;
  PwArgs& a = pa.pw;
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_pick_diag_workspace_bytes(n_q, n_k, d))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_gauss_pick_diag: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = lse;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = 0.0f;             // (0: k_pw_pick_plan then adds no query term)
  pa.u = u; pa.pick = pick;
  pa.L = (float*)(a.part + (size_t)a.n_splits * (size_t)n_q);
  pa.resid = pa.L + n_q;
  pa.rbefore = pa.resid + n_q;
  pa.own = (int32_t*)(pa.rbefore + n_q);
  pa.rchunk = pa.own + n_q;
  pda.prec = prec; pda.stride_p = stride_p;
  PwDiagArgs da;
  memset(&da, 0, sizeof(da));
  da.pw = a; da.prec = prec; da.stride_p = stride_p; da.side = GJX_PAIRWISE_PREC_KEYS;
  const dim3 grid((unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits);
  const dim3 per_query((unsigned)((n_q + kPwThreads - 1) / kPwThreads));
  switch ((2 * d + 3) / 4) {
    case 1: pw_diag_launch<1>(da, grid, st); break;
    case 2: pw_diag_launch<2>(da, grid, st); break;
    case 3: pw_diag_launch<3>(da, grid, st); break;
    case 4: pw_diag_launch<4>(da, grid, st); break;
    case 5: pw_diag_launch<5>(da, grid, st); break;
    case 6: pw_diag_launch<6>(da, grid, st); break;
    case 7: pw_diag_launch<7>(da, grid, st); break;
    default: pw_diag_launch<8>(da, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_pick_diag(lse)");
  hipLaunchKernelGGL(k_pw_pick_plan, per_query, dim3(kPwThreads), 0, st, pa);
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_pick_diag(plan)");
  switch ((2 * d + 3) / 4) {
    case 1: pw_pick_diag_launch<1>(pda, grid, st); break;
    case 2: pw_pick_diag_launch<2>(pda, grid, st); break;
    case 3: pw_pick_diag_launch<3>(pda, grid, st); break;
    case 4: pw_pick_diag_launch<4>(pda, grid, st); break;
    case 5: pw_pick_diag_launch<5>(pda, grid, st); break;
    case 6: pw_pick_diag_launch<6>(pda, grid, st); break;
    case 7: pw_pick_diag_launch<7>(pda, grid, st); break;
    default: pw_pick_diag_launch<8>(pda, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_pick_diag(pick)");
  hipLaunchKernelGGL(k_pw_pick_finish_diag, per_query, dim3(kPwThreads), 0, st, pda);
  GJX_CHECK_LAUNCH("gjx_pairwise_gauss_pick_diag(finish)");
  return GJX_OK;
}

extern "C" size_t gjx_pairwise_gauss_argmax_workspace_bytes(int64_t n_q, int64_t n_k, int32_t d) {
  return gjx_pairwise_gauss_lse_workspace_bytes(n_q, n_k, d);             // {max, index} per (query, split)
}

extern "C" int gjx_pairwise_gauss_argmax(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k,
                                         int32_t d, const float* bias, float precision, const float* centre, int32_t* arg, float* max,
                                         void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  if (!q || !k || !arg || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      stride_q < n_q || stride_k < n_k || !(precision > 0.0f) || !(precision < INFINITY))
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_gauss_argmax: bad argument");
  if (d > GJX_PAIRWISE_MAX_DIM)
    return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_gauss_argmax: more than GJX_PAIRWISE_MAX_DIM components");
  PwArgmaxArgs aa;
  memset(&aa, 0, sizeof(aa));
  PwArgs& a = aa.pw;
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_argmax_workspace_bytes(n_q, n_k, d))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_gauss_argmax: workspace too small");
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = max;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = precision;
  aa.arg = arg;
  return pw_argmax_launch("gjx_pairwise_gauss_argmax", aa, (d + 3) / 4, false, (hipStream_t)stream);
}

extern "C" size_t gjx_pairwise_gauss_argmax_diag_workspace_bytes(int64_t n_q, int64_t n_k, int32_t d) {
  if (d > GJX_PAIRWISE_DIAG_MAX_DIM) return 0;
  return gjx_pairwise_gauss_lse_workspace_bytes(n_q, n_k, d);
}

extern "C" int gjx_pairwise_gauss_argmax_diag(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k,
                                              int32_t d, const float* bias, const float* prec, int64_t stride_p, int32_t prec_side,
                                              const float* centre, int32_t* arg, float* max, void* workspace, size_t workspace_bytes,
                                              void* stream) {
  using namespace gjx;
  if (!q || !k || !arg || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      stride_q < n_q || stride_k < n_k)
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_gauss_argmax_diag: bad argument");
  if (const int rc = pw_diag_keys_only("gjx_pairwise_gauss_argmax_diag", prec, stride_p, n_k, prec_side, d)) return rc;
  PwArgmaxArgs aa;
  memset(&aa, 0, sizeof(aa));
  PwArgs& a = aa.pw;
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_argmax_diag_workspace_bytes(n_q, n_k, d))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_gauss_argmax_diag: workspace too small");
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = max;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = 0.0f;             // (0: k_pw_argmax_merge then adds no query term)
  aa.arg = arg; aa.prec = prec; aa.stride_p = stride_p;
  return pw_argmax_launch("gjx_pairwise_gauss_argmax_diag", aa, (2 * d + 3) / 4, true, (hipStream_t)stream);   // chunks of 4 features
}

extern "C" int gjx_pairwise_t_lse(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k, int32_t d,
                                  const float* bias, float precision, float dof, const float* centre, float* out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
  using namespace gjx;
  PwTArgs ta;
  memset(&ta, 0, sizeof(ta));
  PwArgs& a = ta.pw;
  if (!q || !k || !out || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      stride_q < n_q || stride_k < n_k || !pw_t_scalars(precision, dof, d, &ta.pn, &ta.a))
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_t_lse: bad argument");
  if (d > GJX_PAIRWISE_MAX_DIM) return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_t_lse: more than GJX_PAIRWISE_MAX_DIM components");
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_lse_workspace_bytes(n_q, n_k, d))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_t_lse: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = out;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = precision;
  const dim3 grid((unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits);
  switch ((d + 3) / 4) {
    case 1: pw_t_launch<1>(ta, grid, st); break;
    case 2: pw_t_launch<2>(ta, grid, st); break;
    case 3: pw_t_launch<3>(ta, grid, st); break;
    case 4: pw_t_launch<4>(ta, grid, st); break;
    case 5: pw_t_launch<5>(ta, grid, st); break;
    case 6: pw_t_launch<6>(ta, grid, st); break;
    case 7: pw_t_launch<7>(ta, grid, st); break;
    default: pw_t_launch<8>(ta, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_t_lse(lse)");
  hipLaunchKernelGGL(k_pw_merge_t, dim3((unsigned)((n_q + kPwThreads - 1) / kPwThreads)), dim3(kPwThreads), 0, st, ta);
  GJX_CHECK_LAUNCH("gjx_pairwise_t_lse(merge)");
  return GJX_OK;
}

extern "C" int gjx_pairwise_t_mean(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k, int32_t d,
                                   const float* v, int64_t stride_v, int32_t dv, const float* bias, float precision, float dof,
                                   const float* centre, float* mean, float* lse, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  PwMeanTArgs mta;
  memset(&mta, 0, sizeof(mta));
  PwMeanArgs& ma = mta.m;
  PwArgs& a = ma.pw;
  if (!q || !k || !v || !mean || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      dv <= 0 || stride_q < n_q || stride_k < n_k || stride_v < n_k || !pw_t_scalars(precision, dof, d, &mta.pn, &mta.a))
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_t_mean: bad argument");
  if (d > GJX_PAIRWISE_MAX_DIM || dv > GJX_PAIRWISE_MAX_DIM)
    return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_t_mean: more than GJX_PAIRWISE_MAX_DIM components");
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_mean_workspace_bytes(n_q, n_k, d, dv))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_t_mean: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = lse;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = precision;
  ma.v = v; ma.mean = mean; ma.stride_v = stride_v; ma.dv = dv;
  ma.opart = (float*)(a.part + (size_t)a.n_splits * (size_t)n_q);
  const dim3 grid((unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits);
  switch ((d + 3) / 4) {
    case 1: pw_mean_t_launch<1>(mta, grid, st); break;
    case 2: pw_mean_t_launch<2>(mta, grid, st); break;
    case 3: pw_mean_t_launch<3>(mta, grid, st); break;
    case 4: pw_mean_t_launch<4>(mta, grid, st); break;
    case 5: pw_mean_t_launch<5>(mta, grid, st); break;
    case 6: pw_mean_t_launch<6>(mta, grid, st); break;
    case 7: pw_mean_t_launch<7>(mta, grid, st); break;
    default: pw_mean_t_launch<8>(mta, grid, st); break;
  }
  GJX_CHECK_LAUNCH("gjx_pairwise_t_mean(mean)");
  hipLaunchKernelGGL(k_pw_mean_merge_t, dim3((unsigned)((n_q + kPwThreads - 1) / kPwThreads), (unsigned)dv), dim3(kPwThreads), 0, st, mta);
  GJX_CHECK_LAUNCH("gjx_pairwise_t_mean(merge)");
  return GJX_OK;
}

extern "C" int gjx_pairwise_t_pick(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k, int32_t d,
                                   const float* bias, float precision, float dof, const float* centre, const float* u, int32_t* pick,
                                   float* lse, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  PwPickTArgs pta;
  memset(&pta, 0, sizeof(pta));
  PwPickArgs& pa = pta.p;
  PwArgs& a = pa.pw;
  if (!q || !k || !u || !pick || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      stride_q < n_q || stride_k < n_k || !pw_t_scalars(precision, dof, d, &pta.pn, &pta.a))
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_t_pick: bad argument");
  if (d > GJX_PAIRWISE_MAX_DIM) return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_t_pick: more than GJX_PAIRWISE_MAX_DIM components");
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_gauss_pick_workspace_bytes(n_q, n_k, d))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_t_pick: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = lse;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = precision;
  pa.u = u; pa.pick = pick;
  pa.L = (float*)(a.part + (size_t)a.n_splits * (size_t)n_q);
  pa.resid = pa.L + n_q;
  pa.rbefore = pa.resid + n_q;
  pa.own = (int32_t*)(pa.rbefore + n_q);
  pa.rchunk = pa.own + n_q;
  PwTArgs ta;                                                               // the partials: gjx_pairwise_t_lse's first launch
  ta.pw = a; ta.pn = pta.pn; ta.a = pta.a;
  const dim3 grid((unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits);
  const dim3 per_query((unsigned)((n_q + kPwThreads - 1) / kPwThreads));
  GJX_PW_T_DISPATCH(k_pw_lse_t, d, grid, st, ta)
  GJX_CHECK_LAUNCH("gjx_pairwise_t_pick(lse)");
  hipLaunchKernelGGL(k_pw_pick_plan_t, per_query, dim3(kPwThreads), 0, st, pta);
  GJX_CHECK_LAUNCH("gjx_pairwise_t_pick(plan)");
  GJX_PW_T_DISPATCH(k_pw_pick_t, d, grid, st, pta)
  GJX_CHECK_LAUNCH("gjx_pairwise_t_pick(pick)");
  hipLaunchKernelGGL(k_pw_pick_finish_t, per_query, dim3(kPwThreads), 0, st, pta);
  GJX_CHECK_LAUNCH("gjx_pairwise_t_pick(finish)");
  return GJX_OK;
}

extern "C" size_t gjx_pairwise_t_argmax_workspace_bytes(int64_t n_q, int64_t n_k, int32_t d) {
  const size_t part = gjx_pairwise_gauss_lse_workspace_bytes(n_q, n_k, d);  // {min, index} per (query, split)
  return part ? part + 8 : 0;                                               // and B behind them
}

extern "C" int gjx_pairwise_t_argmax(const float* q, int64_t stride_q, int64_t n_q, const float* k, int64_t stride_k, int64_t n_k, int32_t d,
                                     const float* bias, float precision, float dof, const float* centre, int32_t* arg, float* max,
                                     void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  PwArgmaxTArgs ata;
  memset(&ata, 0, sizeof(ata));
  PwArgs& a = ata.aa.pw;
  if (!q || !k || !arg || !workspace || n_q <= 0 || n_k <= 0 || n_q > INT32_MAX || n_k > INT32_MAX - kPwTile || d <= 0 ||
      stride_q < n_q || stride_k < n_k || !pw_t_scalars(precision, dof, d, &ata.pn, &ata.a))
    return gjx_fail(GJX_EINVAL, "gjx_pairwise_t_argmax: bad argument");
  if (d > GJX_PAIRWISE_MAX_DIM) return gjx_fail(GJX_EUNSUPPORTED, "gjx_pairwise_t_argmax: more than GJX_PAIRWISE_MAX_DIM components");
  pw_plan(n_q, n_k, d, &a);
  if (workspace_bytes < gjx_pairwise_t_argmax_workspace_bytes(n_q, n_k, d))
    return gjx_fail(GJX_EWORKSPACE, "gjx_pairwise_t_argmax: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  a.q = q; a.k = k; a.bias = bias; a.centre = centre; a.out = max;
  a.part = (float2*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  a.stride_q = stride_q; a.stride_k = stride_k; a.p = precision;
  ata.aa.arg = arg;
  ata.top = (float*)(a.part + (size_t)a.n_splits * (size_t)n_q);
  const dim3 grid((unsigned)((n_q + kPwBlockQ - 1) / kPwBlockQ), (unsigned)a.n_splits);
  hipLaunchKernelGGL(k_pw_bias_max, dim3(1), dim3(kPwThreads), 0, st, ata);
  GJX_CHECK_LAUNCH("gjx_pairwise_t_argmax(bias)");
  GJX_PW_T_DISPATCH(k_pw_argmax_t, d, grid, st, ata)
  GJX_CHECK_LAUNCH("gjx_pairwise_t_argmax(argmax)");
  hipLaunchKernelGGL(k_pw_argmax_merge_t, dim3((unsigned)((n_q + kPwThreads - 1) / kPwThreads)), dim3(kPwThreads), 0, st, ata);
  GJX_CHECK_LAUNCH("gjx_pairwise_t_argmax(merge)");
  return GJX_OK;
}
