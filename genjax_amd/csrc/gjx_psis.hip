// gjx_psis.hip — Pareto-smoothed importance weights and the k-hat diagnostic (gjx_pareto_smooth): per segment, a generalised Pareto
// distribution is fitted to the M largest weights (Zhang & Stephens 2009 with the priors of Vehtari et al.), its shape is reported
// and those M weights are replaced by the fitted quantiles.  The definition is in include/gjx.h.
//
// The hot path is finding M of n particles, without a sort: a most-significant-digit radix SELECT on the composite
// (key << ib) | index — key the order-preserving 32-bit key of the log-weight as in gjx_quantiles.hip (0 for a dead particle), ib
// the bits of n - 1 — finds the (M + 1)-th largest composite: the tail and the particle just below it (the cutoff).  Composites are
// distinct, so the threshold is unique and exactly M + 1 particles are at or above it.  11 bits per pass; counts are integers (LDS
// histogram, then the block's non-zero bins into the workspace with integer atomics): no order of arrival to depend on.
//
// Launches (plain launches on the stream, nothing read back, no block waits for another):
//   memset of the states and histograms;
//   per pass p = 0 .. P-1 (P = ceil((32 + ib) / 11) <= 5):
//     k_p_bins: a block takes 1..4 tiles of 1024 particles of one segment and counts digit p of the composites that carry the
//       prefix chosen so far; pass 0 also copies logw to logw_out;
//     k_p_select: one block per segment walks the histogram from the top for the digit in which the running count reaches what is
//       left of M + 1, records prefix and remainder and zeroes the histogram.  When the chosen bin is taken whole the threshold is
//       known: the segment is done and the later passes return at once (the usual case after the key's bits: no tie at the cutoff);
//   k_p_compact: the M + 1 composites at or above the threshold into the workspace, slots from one counter per segment (one atomic
//     per block that has any); slot order is free;
//   k_p_sort: one block per segment sorts them in LDS (a bitonic network, comparators past the end left out), decides "no estimate",
//     writes the sorted composites and x_i (double) back;
//   k_p_cand: one block per (segment, candidate j), one wave where M <= 256: b_j and the profile likelihood L_j, the sum over the
//     tail in a fixed order;
//   k_p_finish: one block per segment: the softmax over the candidates, k-hat and sigma;
//   k_p_smooth: the M smoothed values, 256 ranks per block, scattered to logw_out.
// Every floating-point sum is taken in an order that depends on M alone: the outputs are bit-reproducible, and a segment's outputs
// are those of a call on that segment alone.  A tail index is the low ib bits of a composite that k_p_compact made from the index
// of a particle it read: in range by construction.
#include <math.h>
#include <string.h>

#include "gjx_device.h"
#include "gjx_host.h"

namespace gjx {

constexpr int kPTile = 1024;                          // particles per tile: 256 lanes x 4
constexpr int kPMaxTiles = 4;                         // tiles per block at most (a lane holds them all in registers)
constexpr int kPBits = 11, kPDigits = 1 << kPBits;
constexpr int64_t kPMaxSeg = (int64_t)1 << 22;        // particles per segment at most: the filter kernels' own limit on K
constexpr int kPMaxTail = 6144;                       // M at n = 2^22
constexpr int kPMaxCand = 30 + 78;                    // 30 + floor(sqrt(6144))

typedef unsigned long long u64;

struct PState {
  u64 prefix;              // the digits chosen so far, right-aligned
  u64 threshold;           // the (M + 1)-th largest composite, once done
  uint32_t remaining;      // what the count inside the prefix, from the top, has to reach
  uint32_t done;
  uint32_t slots;          // k_p_compact's slot counter
  uint32_t noest;          // k_p_sort: no estimate for this segment
  float mx, c;             // the largest log-weight, the cutoff
  double ecut;             // exp(c - mx)
  double khat, sigma;      // k_p_finish, for k_p_smooth
};

struct PArgs {
  const float* logw;
  float* out;
  float* fit;
  int64_t n;               // particles per segment
  int64_t S;
  int M, mc, ib, P, pass;
  int tiles_per_block, nc_seg;
  PState* state;           // [S]
  uint32_t* hist;          // u32[S][kPDigits]
  u64* comp;               // u64[S][M + 1]
  double* xs;              // f64[S][max(M, 1)]
  double* cand;            // f64[S][2][mc]: b_j, L_j
};

GJX_DEV uint32_t p_ordered_key(uint32_t bits) { return bits ^ ((bits & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u); }
GJX_DEV uint32_t p_ordered_bits(uint32_t key) { return key ^ ((key & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu); }
GJX_DEV float p_key_value(uint32_t key) { return __uint_as_float(p_ordered_bits(key)); }
// (key << ib) | index: the key of gjx_quantiles.hip's value_key (-0.0 folded onto +0.0), 0 for a dead particle (-inf, NaN): below the
// smallest live key, 0x00800000 of -FLT_MAX
GJX_DEV u64 p_composite(float lw, int64_t idx, int ib) {
  const uint32_t b = __float_as_uint(lw);
  const bool dead = (b & 0x7FFFFFFFu) > 0x7F800000u || b == 0xFF800000u;
  const uint32_t key = dead ? 0u : p_ordered_key(b == 0x80000000u ? 0u : b);
  return ((u64)key << ib) | (u64)idx;
}

// the lane's four consecutive values, nv of them inside the segment: one 16-byte access where the address allows
GJX_DEV void p_load4(const float* p, int nv, float (&x)[4]) {
  if (nv == 4 && ((uintptr_t)p & 15) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = k < nv ? p[k] : 0.0f;
  }
}
GJX_DEV void p_store4(float* p, int nv, const float (&x)[4]) {
  if (nv == 4 && ((uintptr_t)p & 15) == 0) {
    *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < nv) p[k] = x[k];
  }
}

// h[d] += 1 for the active lanes; called by whole waves.  The lanes that share the first active lane's digit add once (equal
// weights: every lane of every wave on one bin); the others on their own.
GJX_DEV void p_count(uint32_t* h, int d, bool active) {
  const u64 act = __ballot(active);
  if (act == 0) return;
  const int first = __ffsll((long long)act) - 1;
  const int d0 = __builtin_amdgcn_readlane(d, first);
  const u64 same = __ballot(active && d == d0);
  if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[d0], (uint32_t)__popcll(same));
  if (active && d != d0) atomicAdd(&h[d], 1u);
}

// the particles of (tile t of the block, lane): first index inside the segment and how many of the four are inside it
GJX_DEV int p_lane_span(const PArgs& a, int64_t p0, int t, int64_t* i0) {
  *i0 = p0 + (int64_t)t * kPTile + threadIdx.x * 4;
  const int64_t left = a.n - *i0;
  return left >= 4 ? 4 : (left > 0 ? (int)left : 0);
}

// every tile of the block, loaded before any is used: the loads are in flight together
GJX_DEV void p_load_tiles(const PArgs& a, const float* w, int64_t p0, float (&x)[kPMaxTiles][4], int (&nv)[kPMaxTiles]) {
#pragma unroll
  for (int t = 0; t < kPMaxTiles; ++t) {
    int64_t i0;
    nv[t] = t < a.tiles_per_block ? p_lane_span(a, p0, t, &i0) : 0;
    x[t][0] = x[t][1] = x[t][2] = x[t][3] = 0.0f;
    if (nv[t] > 0) p_load4(w + i0, nv[t], x[t]);
  }
}

__global__ __launch_bounds__(256) void k_p_bins(const PArgs a) {
  __shared__ uint32_t h[kPDigits];
  const int64_t seg = blockIdx.x / a.nc_seg;
  const int64_t c = blockIdx.x - seg * a.nc_seg;
  const PState* s = a.state + seg;
  u64 prefix = 0;
  if (a.pass > 0) {
    if (s->done) return;                                   // block-uniform
    prefix = s->prefix;
  }
  for (int i = threadIdx.x; i < kPDigits; i += 256) h[i] = 0;
  __syncthreads();
  const int lo_shift = kPBits * (a.P - 1 - a.pass), hi_shift = lo_shift + kPBits;     // (hi_shift <= 55; pass 0: nothing above it)
  const bool copy = a.pass == 0 && a.out != a.logw;
  const int64_t p0 = c * a.tiles_per_block * kPTile;
  const float* w = a.logw + seg * a.n;
  float* o = a.out + seg * a.n;
  float x[kPMaxTiles][4];
  int nv[kPMaxTiles];
  p_load_tiles(a, w, p0, x, nv);
#pragma unroll
  for (int t = 0; t < kPMaxTiles; ++t) {
    if (t >= a.tiles_per_block || p0 + (int64_t)t * kPTile >= a.n) break;     // block-uniform
    const int64_t i0 = p0 + (int64_t)t * kPTile + threadIdx.x * 4;
    if (copy && nv[t] > 0) p_store4(o + i0, nv[t], x[t]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u64 cmp = p_composite(x[t][k], i0 + k, a.ib);
      const bool active = k < nv[t] && (cmp >> hi_shift) == prefix;
      p_count(h, (int)((cmp >> lo_shift) & (kPDigits - 1)), active);
    }
  }
  __syncthreads();
  uint32_t* gh = a.hist + seg * kPDigits;
  for (int i = threadIdx.x; i < kPDigits; i += 256) {
    const uint32_t v = h[i];
    if (v) atomicAdd(&gh[i], v);
  }
}

// One block per segment; thread t holds bins 8t .. 8t + 7.  The digit d with  count(bins above d) < r <= count(bins from d up).
__global__ __launch_bounds__(256) void k_p_select(const PArgs a) {
  __shared__ uint32_t wsum[4];
  PState* s = a.state + blockIdx.x;
  if (a.pass > 0 && s->done) return;                       // block-uniform; the histogram is clean
  uint32_t* gh = a.hist + (int64_t)blockIdx.x * kPDigits + 8 * threadIdx.x;
  const uint32_t r = a.pass == 0 ? (uint32_t)a.M + 1u : s->remaining;
  const u64 prefix = a.pass == 0 ? 0 : s->prefix;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t b[8], tot = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) { b[k] = gh[k]; tot += b[k]; }
  uint32_t incl = tot;                                     // inclusive suffix sum: this thread's bins and every bin above them
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_down(incl, d, 64);
    if (lane + d < 64) incl += o;
  }
  if (lane == 0) wsum[wave] = incl;
  __syncthreads();                                         // (also: every read of the old state is done)
  for (int w = wave + 1; w < 4; ++w) incl += wsum[w];
  uint32_t above = incl - tot;
  if (incl >= r && above < r) {                            // one thread
    int dsel = -1;
    uint32_t cnt = 0;
#pragma unroll
    for (int k = 7; k >= 0; --k) {
      if (dsel < 0) {
        if (above + b[k] >= r) { dsel = k; cnt = b[k]; } else { above += b[k]; }
      }
    }
    const u64 np = (prefix << kPBits) | (u64)(8 * threadIdx.x + dsel);
    const uint32_t rem = r - above;
    const bool last = a.pass == a.P - 1;
    s->prefix = np;
    s->remaining = rem;
    if (last || cnt == rem) {                              // the bin is taken whole: everything at or above its lowest composite
      s->threshold = np << (kPBits * (a.P - 1 - a.pass));
      s->done = 1u;
    }
  }
  if (a.pass < a.P - 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (b[k]) gh[k] = 0;                                 // read and done: clean for the next pass
  }
}

// Two sweeps over the block's tiles (held in registers): count what is at or above the threshold, take the block's run of slots with ONE atomic, write.
__global__ __launch_bounds__(256) void k_p_compact(const PArgs a) {
  __shared__ uint32_t wtot[4];
  __shared__ uint32_t bbase;
  const int64_t seg = blockIdx.x / a.nc_seg;
  const int64_t c = blockIdx.x - seg * a.nc_seg;
  PState* s = a.state + seg;
  const u64 T = s->threshold;
  const uint32_t cap = (uint32_t)a.M + 1u;
  u64* comp = a.comp + seg * (int64_t)cap;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p0 = c * a.tiles_per_block * kPTile;
  const float* w = a.logw + seg * a.n;
  float x[kPMaxTiles][4];
  int nv[kPMaxTiles];
  p_load_tiles(a, w, p0, x, nv);
  uint32_t cnt = 0;
#pragma unroll
  for (int t = 0; t < kPMaxTiles; ++t) {
    const int64_t i0 = p0 + (int64_t)t * kPTile + threadIdx.x * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt += (k < nv[t] && p_composite(x[t][k], i0 + k, a.ib) >= T) ? 1u : 0u;
  }
  uint32_t incl = cnt;                                     // inclusive prefix over the wave
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(incl, d, 64);
    if (lane >= d) incl += o;
  }
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t tot = wtot[0] + wtot[1] + wtot[2] + wtot[3];
    bbase = tot ? atomicAdd(&s->slots, tot) : 0u;
  }
  __syncthreads();
  if (wtot[0] + wtot[1] + wtot[2] + wtot[3] == 0u) return; // block-uniform
  uint32_t slot = bbase + incl - cnt;
  for (int v = 0; v < wave; ++v) slot += wtot[v];
  if (cnt == 0u) return;
#pragma unroll
  for (int t = 0; t < kPMaxTiles; ++t) {
    const int64_t i0 = p0 + (int64_t)t * kPTile + threadIdx.x * 4;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const u64 cmp = p_composite(x[t][k], i0 + k, a.ib);
      if (k < nv[t] && cmp >= T) {
        if (slot < cap) comp[slot] = cmp;                  // (exactly cap composites pass: the compare only states it)
        ++slot;
      }
    }
  }
}

// One step of the sorting network: comparator t orders the pair (i, i ^ (2 d - 1)) (mirror: the first step of a merge) or
// (i, i | d), i the lower; a comparator that reaches past N - 1 is left out
GJX_DEV void p_sort_step(u64* v, int N, int half, int d, bool mirror, int tid, int nt) {
  for (int t = tid; t < half; t += nt) {
    const int lo = ((t & ~(d - 1)) << 1) | (t & (d - 1));
    const int hi = mirror ? lo ^ (2 * d - 1) : lo | d;
    if (hi < N) {
      const u64 x = v[lo], y = v[hi];
      if (x > y) { v[lo] = y; v[hi] = x; }
    }
  }
}

// sum of v over the block in an order that depends on blockDim alone, the same double in every thread
GJX_DEV double p_block_sum(double v, double* red) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  const int nw = blockDim.x >> 6;
  if (nw == 1) return v;
  __syncthreads();                                         // (red may still be read from the sum before)
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = red[0];
  for (int w = 1; w < nw; ++w) s += red[w];                // red: one double per wave, 16 at most
  return s;
}

// One block per segment: the M + 1 composites ascending; sorted[0] is the cutoff particle, sorted[1 + i] the tail particle of rank i.
__global__ __launch_bounds__(1024) void k_p_sort(const PArgs a) {
  extern __shared__ u64 v[];                               // u64[M + 1]
  const int64_t seg = blockIdx.x;
  const int N = a.M + 1, nt = blockDim.x, tid = threadIdx.x;
  u64* comp = a.comp + seg * (int64_t)N;
  for (int i = tid; i < N; i += nt) v[i] = comp[i];
  __syncthreads();
  // bitonic network with every comparator ascending (the first step of a merge against the mirrored partner); a comparator that
  // reaches past N - 1 would meet the +inf of a padded array and change nothing: it is left out
  int half = 1;
  while (2 * half < N) half <<= 1;                         // comparators per step of the padded network
  if (N == 1) half = 0;
  // Comparators 64 w .. 64 w + 63 of a step of distance <= 64 touch elements 128 w .. 128 w + 127 only, and a wave runs the same
  // comparators in every such step: between two of them the wave waits for its own LDS accesses, not for the block.
  for (int k = 2; (k >> 1) < N; k <<= 1) {
    const int hk = k >> 1;
    p_sort_step(v, N, half, hk, true, tid, nt);
    if (hk > 64 || hk == 1) __syncthreads(); else __threadfence_block();     // (hk > 64: the steps below leave the wave's elements)
    for (int j = hk >> 1; j > 0; j >>= 1) {
      p_sort_step(v, N, half, j, false, tid, nt);
      if (j > 64 || j == 1) __syncthreads(); else __threadfence_block();     // (j == 1: the next stage's first step may)
    }
  }
  __syncthreads();
  const uint32_t key0 = (uint32_t)(v[0] >> a.ib), keyM = (uint32_t)(v[a.M] >> a.ib);
  const float c = key0 ? p_key_value(key0) : NAN;          // a dead particle just below the tail: no more than M live ones
  const float mx = p_key_value(keyM);
  const double ecut = exp((double)c - (double)mx);
  bool noest = a.M < 5 || key0 == 0u;
  if (!noest) {
    const int q = (a.M + 2) / 4 - 1;                       // floor(M / 4 + 0.5) - 1
    const double xq = exp((double)p_key_value((uint32_t)(v[1 + q] >> a.ib)) - (double)mx) - ecut;
    noest = !(xq > 0.0);
  }
  PState* s = a.state + seg;
  if (noest) {                                             // (uniform over the block)
    if (tid == 0) {
      float* f = a.fit + 4 * seg;
      f[0] = NAN; f[1] = NAN; f[2] = c; f[3] = (float)a.M;
      s->noest = 1u;
    }
    return;
  }
  double* xs = a.xs + seg * (int64_t)a.M;
  for (int i = tid; i < N; i += nt) {
    comp[i] = v[i];
    if (i > 0) xs[i - 1] = exp((double)p_key_value((uint32_t)(v[i] >> a.ib)) - (double)mx) - ecut;
  }
  if (tid == 0) { s->mx = mx; s->c = c; s->ecut = ecut; }
}

// b_j and L_j = M (log(-b_j / k_j) - k_j - 1), k_j = mean log1p(-b_j x_i), of candidate j = 1 .. mc.  A tail of more than 256: one block
// per (segment, candidate); a shorter one: one WAVE per candidate, four candidates per block.  (M decides: the order of the sum is
// a function of M alone.)
__global__ __launch_bounds__(256) void k_p_cand(const PArgs a) {
  __shared__ double red[4];
  const bool per_wave = a.M <= 256;
  const int bps = per_wave ? (a.mc + 3) / 4 : a.mc;        // blocks per segment
  const int64_t seg = blockIdx.x / bps;
  const int r = (int)(blockIdx.x - seg * bps);
  if (a.state[seg].noest) return;                          // block-uniform
  const int lane = threadIdx.x & 63;
  const int j = per_wave ? 4 * r + (int)(threadIdx.x >> 6) + 1 : r + 1;
  if (j > a.mc) return;                                    // (whole waves of the last block of a short tail: no barrier follows)
  const double* xs = a.xs + seg * (int64_t)a.M;
  const double xq = xs[(a.M + 2) / 4 - 1], xmax = xs[a.M - 1];
  const double b = (1.0 - sqrt((double)a.mc / ((double)j - 0.5))) / (3.0 * xq) + 1.0 / xmax;
  double acc = 0.0;
  for (int i = per_wave ? lane : (int)threadIdx.x; i < a.M; i += per_wave ? 64 : 256) acc += log1p(-b * xs[i]);
  double sum;
  if (per_wave) {
    sum = acc;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) sum += __shfl_xor(sum, d, 64);
  } else {
    sum = p_block_sum(acc, red);
  }
  const double k = sum / (double)a.M;
  if ((per_wave ? lane : (int)threadIdx.x) == 0) {
    double* cd = a.cand + seg * 2 * (int64_t)a.mc;
    cd[j - 1] = b;
    cd[a.mc + j - 1] = (double)a.M * (log(-b / k) - k - 1.0);
  }
}

// One block per segment: b-hat from the softmax over the candidates, k-hat and sigma-hat
__global__ __launch_bounds__(1024) void k_p_finish(const PArgs a) {
  __shared__ double red[16];
  __shared__ double wgt[kPMaxCand], cb[kPMaxCand];
  const int64_t seg = blockIdx.x;
  PState* s = a.state + seg;
  if (s->noest) return;                                    // block-uniform
  const double* cd = a.cand + seg * 2 * (int64_t)a.mc;
  for (int j = threadIdx.x; j < a.mc; j += blockDim.x) { cb[j] = cd[j]; wgt[j] = cd[a.mc + j]; }
  __syncthreads();
  double lmax = -INFINITY;
  for (int j = 0; j < a.mc; ++j) {
    const double L = wgt[j];
    if (isfinite(L) && L > lmax) lmax = L;
  }
  __syncthreads();
  for (int j = threadIdx.x; j < a.mc; j += blockDim.x) {
    const double L = wgt[j];
    wgt[j] = isfinite(L) ? exp(L - lmax) : 0.0;
  }
  __syncthreads();
  double sw = 0.0, bhat = 0.0;
  for (int j = 0; j < a.mc; ++j) sw += wgt[j];
  for (int j = threadIdx.x; j < a.mc; j += blockDim.x) cb[j] = (wgt[j] / sw) * cb[j];
  __syncthreads();
  for (int j = 0; j < a.mc; ++j) bhat += cb[j];
  const double* xs = a.xs + seg * (int64_t)a.M;
  double acc = 0.0;
  for (int i = threadIdx.x; i < a.M; i += blockDim.x) acc += log1p(-bhat * xs[i]);
  const double k0 = p_block_sum(acc, red) / (double)a.M;
  const double sigma = -k0 / bhat;
  const double khat = ((double)a.M * k0 + 5.0) / ((double)a.M + 10.0);
  if (threadIdx.x == 0) {
    float* f = a.fit + 4 * seg;
    f[0] = (float)khat; f[1] = (float)sigma; f[2] = s->c; f[3] = (float)a.M;
    s->khat = khat; s->sigma = sigma;
  }
}

// The M smoothed log-weights, 256 ranks of one segment per block, scattered to the particles they belong to
__global__ __launch_bounds__(256) void k_p_smooth(const PArgs a) {
  const int bps = (a.M + 255) / 256;
  const int64_t seg = blockIdx.x / bps;
  const PState* s = a.state + seg;
  if (s->noest) return;                                    // block-uniform
  const double khat = s->khat, sigma = s->sigma, mx = (double)s->mx, ecut = s->ecut;
  const u64* comp = a.comp + seg * ((int64_t)a.M + 1) + 1;
  const u64 imask = ((u64)1 << a.ib) - 1;
  float* o = a.out + seg * a.n;
  const int i = (int)(blockIdx.x - seg * bps) * 256 + (int)threadIdx.x;
  if (i < a.M) {
    const double l1 = log1p(-((double)i + 0.5) / (double)a.M);
    const double q = khat == 0.0 ? -sigma * l1 : sigma * expm1(-khat * l1) / khat;
    double val = log(q + ecut);
    val = val > 0.0 ? 0.0 : val;                           // never above the largest raw weight (a NaN stays)
    const int64_t idx = (int64_t)(comp[i] & imask);
    if (idx < a.n) o[idx] = (float)(val + mx);             // (in range by construction: the compare only states it)
  }
}

// ceil(3 sqrt(n)) = ceil(sqrt(9 n)) in integers
static int64_t p_ceil3sqrt(int64_t n) {
  const int64_t v = 9 * n;
  int64_t r = (int64_t)sqrt((double)v);
  while (r * r >= v) --r;
  while ((r + 1) * (r + 1) < v) ++r;                       // r = floor(sqrt(v - 1))
  return r + 1;
}
static int p_isqrt(int v) {
  int r = (int)sqrt((double)v);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// the shape of a call; 0: accepted, else the status of the refusal
static int p_shape(int64_t K, int64_t S, PArgs* a) {
  if (K <= 0 || S <= 0 || K % S != 0) return GJX_EINVAL;
  const int64_t n = K / S;
  if (n > kPMaxSeg) return GJX_EUNSUPPORTED;
  const int64_t M5 = n / 5, M3 = p_ceil3sqrt(n);
  const int M = (int)(M5 < M3 ? M5 : M3);
  int ib = 0;
  while (((int64_t)1 << ib) < n) ++ib;
  const int64_t nt_seg = (n + kPTile - 1) / kPTile;
  // enough blocks to fill the device, few enough that a block's LDS histogram is worth its zeroing and its flush
  // (a block ends in atomics on its segment's few hot bins and on its slot counter: a few hundred blocks per segment at most)
  int64_t tpb = nt_seg * S / 4096;
  if (tpb < (nt_seg + 255) / 256) tpb = (nt_seg + 255) / 256;
  tpb = tpb < 1 ? 1 : (tpb > kPMaxTiles ? kPMaxTiles : tpb);
  const int64_t nc_seg = (nt_seg + tpb - 1) / tpb;
  const int mc = 30 + p_isqrt(M);
  if (S > INT32_MAX / nc_seg || S > INT32_MAX / mc) return GJX_EINVAL;      // grid sizes ((M + 255) / 256 <= mc)
  a->n = n; a->S = S; a->M = M; a->mc = mc; a->ib = ib; a->P = (32 + ib + kPBits - 1) / kPBits;
  a->tiles_per_block = (int)tpb; a->nc_seg = (int)nc_seg;
  return GJX_OK;
}

// workspace: [state PState[S]] [hist u32[S][2048]] [comp u64[S][M + 1]] [xs f64[S][max(M, 1)]] [cand f64[S][2][mc]]; the first two
// are zeroed by the call
static size_t p_layout(PArgs* a, void* workspace, size_t* zero_bytes) {
  const size_t S = (size_t)a->S, M = (size_t)a->M;
  const size_t o_hist = S * sizeof(PState), o_comp = o_hist + S * 4 * kPDigits, o_xs = o_comp + S * 8 * (M + 1);
  const size_t o_cand = o_xs + S * 8 * (M ? M : 1), end = o_cand + S * 16 * (size_t)a->mc;
  if (workspace) {
    char* base = (char*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
    a->state = (PState*)base;
    a->hist = (uint32_t*)(base + o_hist);
    a->comp = (u64*)(base + o_comp);
    a->xs = (double*)(base + o_xs);
    a->cand = (double*)(base + o_cand);
  }
  *zero_bytes = o_comp;
  return 8 + end;                                          // (8: the alignment of any pointer)
}

}  // namespace gjx

extern "C" size_t gjx_pareto_smooth_workspace_bytes(int64_t K, int64_t n_segments) {
  gjx::PArgs a;
  size_t zero;
  if (gjx::p_shape(K, n_segments, &a) != GJX_OK) return 0;
  return gjx::p_layout(&a, nullptr, &zero);
}

extern "C" int gjx_pareto_smooth(const float* logw, int64_t K, int64_t n_segments, float* logw_out, float* fit, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  using namespace gjx;
  static_assert(sizeof(PState) == 64, "a state is one 64-byte block");
  static_assert(8 * (kPMaxTail + 1) <= 65536, "the tail and the cutoff of the largest segment are sorted in one block's LDS");
  PArgs a;
  memset(&a, 0, sizeof(a));
  const int rc = p_shape(K, n_segments, &a);
  if (!logw || !logw_out || !fit || !workspace || rc == GJX_EINVAL) return gjx_fail(GJX_EINVAL, "gjx_pareto_smooth: bad argument");
  if (rc != GJX_OK) return gjx_fail(rc, "gjx_pareto_smooth: a segment takes at most 2^22 particles");
  size_t zero;
  if (workspace_bytes < p_layout(&a, workspace, &zero)) return gjx_fail(GJX_EWORKSPACE, "gjx_pareto_smooth: workspace too small");
  a.logw = logw; a.out = logw_out; a.fit = fit;
  const hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(a.state, 0, zero, st);
  if (e != hipSuccess) return gjx_fail_hip(e, "gjx_pareto_smooth(memset)");
  const dim3 chunks((unsigned)(a.S * a.nc_seg)), segs((unsigned)a.S);
  for (a.pass = 0; a.pass < a.P; ++a.pass) {
    hipLaunchKernelGGL(k_p_bins, chunks, dim3(256), 0, st, a);
    GJX_CHECK_LAUNCH("gjx_pareto_smooth(bins)");
    hipLaunchKernelGGL(k_p_select, segs, dim3(256), 0, st, a);
    GJX_CHECK_LAUNCH("gjx_pareto_smooth(select)");
  }
  hipLaunchKernelGGL(k_p_compact, chunks, dim3(256), 0, st, a);
  GJX_CHECK_LAUNCH("gjx_pareto_smooth(compact)");
  int nt = 64;
  while (nt < a.M + 1 && nt < 1024) nt <<= 1;
  hipLaunchKernelGGL(k_p_sort, segs, dim3(nt), 8 * ((size_t)a.M + 1), st, a);          // (at most 49160 bytes of LDS)
  GJX_CHECK_LAUNCH("gjx_pareto_smooth(sort)");
  if (a.M >= 5) {                                          // (below: every segment is "no estimate", written by the sort)
    hipLaunchKernelGGL(k_p_cand, dim3((unsigned)(a.S * (a.M <= 256 ? (a.mc + 3) / 4 : a.mc))), dim3(256), 0, st, a);
    GJX_CHECK_LAUNCH("gjx_pareto_smooth(candidates)");
    int nf = 64;
    while (nf < a.M && nf < 1024) nf <<= 1;
    hipLaunchKernelGGL(k_p_finish, segs, dim3(nf), 0, st, a);
    GJX_CHECK_LAUNCH("gjx_pareto_smooth(finish)");
    hipLaunchKernelGGL(k_p_smooth, dim3((unsigned)(a.S * ((a.M + 255) / 256))), dim3(256), 0, st, a);
    GJX_CHECK_LAUNCH("gjx_pareto_smooth(smooth)");
  }
  return GJX_OK;
}
