// gjx_resample.hip — 1-of-K categorical pick (Gumbel-max argmax reduce), fixed-point weight
// prefix sums, systematic / multinomial ancestor search, SoA row gather.
//
// All index work is integer: weights become q_i = (uint64)(w_i * 2^30), prefix sums are exact
// uint64 adds (associative, so the block decomposition cannot change a single bit), comb
// thresholds are one IEEE double multiply + truncation per output slot.  HBM traffic per
// particle: pick 4 B read; cumsum 2x4 B read + 8 B write; search 4 B write (+ L2-resident
// binary-search probes); gather 4 B read + 4 B write per row.
#include <limits.h>
#include <math.h>
#include <string.h>

#include "gjx_device.h"
#include "gjx_host.h"
#include "gjx_scan.h"
#include "gjx_tile.h"

namespace gjx {

struct PickPair {
  float v;
  int32_t i;
};

GJX_DEV void pick_better(float& v, int32_t& i, float ov, int32_t oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

template <int RNG>
__global__ __launch_bounds__(256) void k_pick_partial(const float* logw, int64_t K, int64_t offset, const float* lse,
                                                     key2 key, PickPair* partials) {
  __shared__ float rv[4];
  __shared__ int32_t ri[4];
  const float l = lse[2];
  float bv = -INFINITY;
  int32_t bi = 0x7FFFFFFF;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < K; i += (int64_t)gridDim.x * 256) {
    const uint64_t gi = (uint64_t)(offset + i);
    uint32_t bits;
    if (RNG == GJX_RNG_JAX32) {
      const key2 h = fold_in64(key, gi);
      bits = h.a ^ h.b;
    } else {
      const key2 h = fold_in64(key, gi >> 1);
      bits = (gi & 1u) ? h.b : h.a;
    }
    const float v = (logw[i] - l) + gumbel_from_bits(bits);
    pick_better(bv, bi, v, (int32_t)gi);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int32_t oi = __shfl_xor(bi, o, 64);
    pick_better(bv, bi, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = bv; ri[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) pick_better(bv, bi, rv[w], ri[w]);
    partials[blockIdx.x] = PickPair{bv, bi};
  }
}

__global__ __launch_bounds__(256) void k_pick_finish(const PickPair* partials, int n, PickPair* out) {
  __shared__ float rv[4];
  __shared__ int32_t ri[4];
  float bv = -INFINITY;
  int32_t bi = 0x7FFFFFFF;
  for (int t = threadIdx.x; t < n; t += 256) pick_better(bv, bi, partials[t].v, partials[t].i);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int32_t oi = __shfl_xor(bi, o, 64);
    pick_better(bv, bi, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = bv; ri[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) pick_better(bv, bi, rv[w], ri[w]);
    *out = PickPair{bv, bi};
  }
}

// Independent trials (jax.vmap(alg.run_smc)(split(key, n)), README.md:110-113): trial t owns particles [t K, (t + 1) K) of one
// n K-particle run.  One block per trial: its LSE record {max, sumexp, lse, lse - log K} and, if asked, its 1-of-K draw
// argmax_i (logw_i - lse_t) + Gumbel(bits(key, global index)) — the same rule as k_pick_partial with particle_offset = t K.
template <int RNG>
__global__ __launch_bounds__(256) void k_trials_lse_pick(const float* logw, int64_t K, int64_t offset, key2 key, int want_pick, float log_k,
                                                        float* lse_out, int32_t* pick_out) {
  __shared__ float red[8];
  __shared__ float rv[4];
  __shared__ int32_t ri[4];
  const int64_t t = blockIdx.x;
  const float* lw = logw + t * K;
  float m = -INFINITY;
  for (int64_t i = threadIdx.x; i < K; i += 256) m = fmaxf(m, lw[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  const float bm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sm = 0.0f;
  if (bm > -INFINITY)
    for (int64_t i = threadIdx.x; i < K; i += 256) sm += fast_exp(lw[i] - bm);
  sm = wave_sum(sm);
  if ((threadIdx.x & 63) == 0) red[4 + (threadIdx.x >> 6)] = sm;
  __syncthreads();
  const float bs = (red[4] + red[5]) + (red[6] + red[7]);
  const float l = bm > -INFINITY ? bm + fast_log(bs) : -INFINITY;
  if (threadIdx.x == 0) {
    float* o = lse_out + 4 * t;
    o[0] = bm; o[1] = bs; o[2] = l; o[3] = l - log_k;
  }
  if (!want_pick) return;
  float bv = -INFINITY;
  int32_t bi = 0x7FFFFFFF;
  for (int64_t i = threadIdx.x; i < K; i += 256) {
    const uint64_t gi = (uint64_t)(offset + t * K + i);
    uint32_t bits;
    if (RNG == GJX_RNG_JAX32) {
      const key2 h = fold_in64(key, gi);
      bits = h.a ^ h.b;
    } else {
      const key2 h = fold_in64(key, gi >> 1);
      bits = (gi & 1u) ? h.b : h.a;
    }
    pick_better(bv, bi, (lw[i] - l) + gumbel_from_bits(bits), (int32_t)gi);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int32_t oi = __shfl_xor(bi, o, 64);
    pick_better(bv, bi, ov, oi);
  }
  if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = bv; ri[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) pick_better(bv, bi, rv[w], ri[w]);
    pick_out[t] = bi == 0x7FFFFFFF ? (int32_t)(offset + t * K) : bi;   // a dead trial (all weights zero, lse = -inf): its first particle
  }
}

__global__ __launch_bounds__(256) void k_wsum_blocks(const float* x, int64_t K, int is_log, const float* lse,
                                                    int n_partials, float* lse_out, float log_k_total,
                                                    uint64_t* block_sums) {
  __shared__ uint64_t red[4];
  __shared__ float fred[8];
  float sm;
  const float mx = block_ref_max(is_log, lse, n_partials, fred, &sm);
  if (is_log == 2 && lse_out && blockIdx.x == 0 && threadIdx.x == 0) {
    const float l = mx > -INFINITY ? mx + logf(sm) : -INFINITY;
    lse_out[0] = mx; lse_out[1] = sm; lse_out[2] = l; lse_out[3] = l - log_k_total;
  }
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k)
    if (base + k < K) s += weight_q(x, base + k, is_log, mx);
  s = wave_sum_u64(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) block_sums[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// Second (final) pass: every block sums the totals of the blocks before it (nblocks u64 values, L2-resident:
// K/2048 of them) instead of waiting for a separate single-block scan kernel, then scans its own tile.
// The last block also publishes base_total = {0, sum of all weights}.
__global__ __launch_bounds__(256) void k_wscan_write(const float* x, int64_t K, int is_log, const float* lse,
                                                    int n_partials, const uint64_t* block_sums, uint64_t* cum,
                                                    uint64_t* base_total) {
  __shared__ uint64_t wsum[4];
  __shared__ uint64_t red[4];
  __shared__ float fred[8];
  const float mx = block_ref_max(is_log, lse, n_partials, fred, nullptr);
  const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  // offset of this block = sum of block_sums[0 .. blockIdx.x)
  uint64_t pre = 0;
  for (int t = threadIdx.x; t < (int)blockIdx.x; t += 256) pre += block_sums[t];
  pre = wave_sum_u64(pre);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = pre;
  uint64_t q[kScanItems];
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    q[k] = (base + k < K) ? weight_q(x, base + k, is_log, mx) : 0;
    s += q[k];
    q[k] = s;  // thread-local inclusive
  }
  uint64_t inc = wave_scan_u64(s);
  if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = inc;
  __syncthreads();
  uint64_t off = red[0] + red[1] + red[2] + red[3] + inc - s;
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) off += wsum[w];
#pragma unroll
  for (int k = 0; k < kScanItems; ++k)
    if (base + k < K) cum[base + k] = off + q[k];
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) {
    base_total[0] = 0;
    base_total[1] = off + s;
  }
}

// first i in [0, K) with cum[i] > t   (requires t < cum[K-1])
GJX_DEV int64_t upper_search(const uint64_t* __restrict__ cum, int64_t K, uint64_t t) {
  int64_t lo = 0, hi = K - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cum[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// first i in [lo, hi] with cum[i] > t   (requires cum[hi] > t)
GJX_DEV int64_t upper_search_in(const uint64_t* __restrict__ cum, int64_t lo, int64_t hi, uint64_t t) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cum[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// Systematic resampling, particle-oriented ("expand"): particle i owns the output slots
// [J(base + cum[i-1]), J(base + cum[i])) — a few consecutive slots, usually 0..3 — so one lane per particle
// reads two prefix sums (coalesced), computes its slot range in O(1), and writes its index (and, with
// GATHER, its SoA rows) to those slots.  Consecutive particles own consecutive slot runs, so the writes
// coalesce; particles without offspring read nothing.  Particles with many offspring (degenerate weights)
// are filled cooperatively by the whole block.  No binary search, no dependent-load chain.
template <bool GATHER>
__global__ __launch_bounds__(256) void k_systematic_expand(const uint64_t* __restrict__ cum, int64_t K,
                                                          const uint64_t* base_total, double u, int64_t N_total,
                                                          int64_t out_begin, int64_t n_out, int32_t* ancestors,
                                                          const float* __restrict__ src, int64_t src_stride, int rows,
                                                          float* __restrict__ dst, int64_t dst_stride,
                                                          const int64_t* range_dev = nullptr) {
  constexpr int kOwn = 8;  // offspring a lane writes by itself
  if (range_dev) {         // sharded plan: {first slot, slot count} of this rank's run live on the device
    out_begin = range_dev[0];
    const int64_t n = range_dev[1];
    n_out = n < n_out ? n : n_out;   // n_out carries the capacity of ancestors[]
  }
  __shared__ int n_heavy;
  __shared__ int32_t h_i[256];
  __shared__ int64_t h_lo[256], h_hi[256];
  if (threadIdx.x == 0) n_heavy = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t base = base_total[0], total = base_total[1];
  const double step = (double)total / (double)N_total;
  const double inv_step = (double)N_total / (double)total;
  // J(base + cum[i]) once per lane; the lower end of a particle's run is its left neighbour's upper end
  const bool in = i < K && total > 0;
  const uint64_t c_cur = in ? base + cum[i] : 0;
  const int64_t j_cur = in ? slots_below(c_cur, u, step, inv_step, total, N_total) : 0;
  int64_t j_prev = __shfl_up((long long)j_cur, 1, 64);
  uint64_t c_prev = __shfl_up((unsigned long long)c_cur, 1, 64);
  if ((threadIdx.x & 63) == 0) {
    c_prev = base + ((in && i > 0) ? cum[i - 1] : 0);
    j_prev = in ? slots_below(c_prev, u, step, inv_step, total, N_total) : 0;
  }
  if (in) {
    if (c_cur > c_prev) {
      int64_t lo = j_prev - out_begin;
      int64_t hi = j_cur - out_begin;
      lo = lo < 0 ? 0 : lo;
      hi = hi > n_out ? n_out : hi;
      if (hi - lo > kOwn) {
        const int h = atomicAdd(&n_heavy, 1);
        h_i[h] = (int32_t)i; h_lo[h] = lo; h_hi[h] = hi;
      } else if (hi > lo) {
        if (ancestors) for (int64_t j = lo; j < hi; ++j) ancestors[j] = (int32_t)i;
        if (GATHER) {
          for (int r = 0; r < rows; ++r) {
            const float v = src[(int64_t)r * src_stride + i];
            for (int64_t j = lo; j < hi; ++j) dst[(int64_t)r * dst_stride + j] = v;
          }
        }
      }
    }
  }
  __syncthreads();
  const int nh = n_heavy;
  for (int h = 0; h < nh; ++h) {
    const int32_t pi = h_i[h];
    const int64_t lo = h_lo[h], hi = h_hi[h];
    if (ancestors) for (int64_t j = lo + threadIdx.x; j < hi; j += 256) ancestors[j] = pi;
    if (GATHER) {
      for (int r = 0; r < rows; ++r) {
        const float v = src[(int64_t)r * src_stride + pi];
        for (int64_t j = lo + threadIdx.x; j < hi; j += 256) dst[(int64_t)r * dst_stride + j] = v;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// One-launch resampling indices for a single GPU: fixed-point weights, their prefix sums and the systematic
// ancestor expansion in ONE kernel (gjx_scan.h: tile_scan_expand).  Each block scans its tile in registers, publishes
// the tile total as one tagged 8-byte agent-scope granule, and then reads EVERY block's granule to get both its own
// offset and the grand total — an all-gather of <= 1024 words instead of two kernel boundaries and a 16 MB round trip
// of the prefix-sum array.  Requires all blocks co-resident: the launcher sizes the grid with the occupancy query.
// ------------------------------------------------------------------------------------------
template <int ITEMS>
__global__ __launch_bounds__(256) void k_resample_fused(const float* __restrict__ x, int64_t K, int mode,
                                                       const float* lse, int n_partials, float* lse_out,
                                                       float log_k_total, double u, int64_t N, int32_t* ancestors,
                                                       uint64_t* cum_out, uint64_t* base_total_out,
                                                       unsigned long long* agg, unsigned* ctrl) {
  __shared__ float fred[8];
  __shared__ ScanSmem sm;
  unsigned epoch;
  const unsigned long long tag = grid_tag(ctrl, &epoch);
  // the weights are requested before the reference maximum is reduced: their latency overlaps the reduction
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * ITEMS;
  float xv[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) xv[k] = (i0 + k < K) ? x[i0 + k] : 0.0f;
  float sm_sum;
  const float mx = block_ref_max(mode, lse, n_partials, fred, &sm_sum);
  if (mode == 2 && lse_out && blockIdx.x == 0 && threadIdx.x == 0) {
    const float l = mx > -INFINITY ? mx + logf(sm_sum) : -INFINITY;
    lse_out[0] = mx; lse_out[1] = sm_sum; lse_out[2] = l; lse_out[3] = l - log_k_total;
  }
  tile_scan_expand<ITEMS, false>(xv, mode, mx, i0, K, u, N, ancestors, cum_out, base_total_out, agg, tag, ctrl, epoch, true, sm);
}

// ------------------------------------------------------------------------------------------
// One-launch resampling + gather for a single GPU (N = K): weights -> systematic ancestors -> rows of the children,
// the ancestors never written to memory unless asked for.  Block b scans its own tile of 256 ITEMS fixed-point weights,
// the tile totals are all-gathered (the one rendezvous, as in k_resample_fused), and then the block is the CONSUMER of
// the output slots [b TILE, (b+1) TILE): each lane takes ITEMS consecutive slots, computes their comb thresholds T_j,
// and finds the source tile of each among the eight tiles around its own, whose boundaries are the weight below them (summed
// while the totals are gathered) plus a serial prefix of eight totals; the cumulative weights of tiles b - 1 .. b + 1 are in
// LDS by then, and a lane searches its first slot and counts the others off in a short window (rank_in_tiles_sorted).  Only a
// block whose slots leave those windows (collapsed or drifting weights) makes the full prefix of the totals, descends in it,
// and re-scans the few distinct source tiles its thresholds fall into (log-weights from L2, the next tile's loads in flight
// while the current one is searched); ancestor = first particle of the tile with inclusive cumulative weight > T_j.  Same ancestors as
// the slot-run expansion: particle i owns slot j  <=>  cum_excl(i) <= T_j < cum_incl(i).  Then the rows are copied,
// ITEMS slots per lane (16-byte stores at ITEMS = 4).  Balanced whatever the weights are; a window that touches many
// source tiles (collapsed weights) just loops longer.
// ------------------------------------------------------------------------------------------
constexpr int kGatherMaxTiles = 1024;

template <int ITEMS>
__global__ __launch_bounds__(256) void k_resample_gather(const float* __restrict__ x, int64_t K, int mode,
                                                        const float* lse, int n_partials, float* lse_out,
                                                        float log_k_total, double u, const float* __restrict__ src,
                                                        int64_t src_stride, int rows, float* __restrict__ dst,
                                                        int64_t dst_stride, int32_t* ancestors,
                                                        unsigned long long* agg, unsigned* ctrl,
                                                        unsigned long long* timeline) {
#define GJX_STAMP(n) do { if (timeline && threadIdx.x == 0) timeline[blockIdx.x * 8 + (n)] = __builtin_amdgcn_s_memrealtime(); } while (0)
  GJX_STAMP(0);
  constexpr int TILE = 256 * ITEMS;
  __shared__ float fred[8];
  __shared__ uint64_t wsum[4];
  __shared__ uint64_t s_sums[8];                // wave sums of the totals: below the window [4], all [4]
  __shared__ uint64_t P[kGatherMaxTiles + 1];   // P[b + 1] = total of tile b; on the re-scan branch their prefix: P[t] = total weight of tiles < t
  constexpr int CH = 3;                          // source tiles re-scanned per round
  __shared__ __align__(16) uint64_t cumL[CH * TILE];   // inclusive cumulative weights of the tiles being searched, relative to each tile's start (16-byte reads)
  __shared__ uint64_t s_wtot[CH][4];
  __shared__ int s_range[2];                    // first and last source tile of this block's slots
  unsigned epoch;
  const unsigned long long tag = grid_tag(ctrl, &epoch);
  const int nb = (int)gridDim.x;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * ITEMS;   // first particle this lane scans
  auto load_tile = [&](int64_t p0, float (&v)[ITEMS]) {
    if (ITEMS == 4 && p0 + 4 <= K) {
      const float4 q4 = *(const float4*)(x + p0);
      v[0] = q4.x; v[1] = q4.y; v[2] = q4.z; v[3] = q4.w;
    } else {
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) v[k] = (p0 + k < K) ? x[p0 + k] : 0.0f;
    }
  };
  // the block's own tile and its two neighbours: with weights that are not collapsed the slots of block b draw from
  // tiles b - 1 .. b + 1, so their cumulative weights are laid out in LDS while the tile totals travel (below)
  const int w0 = (int)blockIdx.x - 1;            // first tile of the prefetched window
  float xv[ITEMS], xn[2][ITEMS];
  load_tile(i0, xv);
  float sm_sum;
  const float mx = block_ref_max(mode, lse, n_partials, fred, &sm_sum);
  if (mode == 2 && lse_out && blockIdx.x == 0 && threadIdx.x == 0) {
    const float l = mx > -INFINITY ? mx + logf(sm_sum) : -INFINITY;
    lse_out[0] = mx; lse_out[1] = sm_sum; lse_out[2] = l; lse_out[3] = l - log_k_total;
  }
  // ---- own tile total -> all-gather ----
  uint64_t qown[ITEMS], sown = 0, incown;
  {
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { sown += (i0 + k < K) ? weight_q(xv, k, mode, mx) : 0; qown[k] = sown; }
    incown = wave_scan_u64(sown);
    if (lane == 63) { wsum[wid] = incown; s_wtot[1][wid] = incown; }
    __syncthreads();
    if (threadIdx.x == 0) grid_publish(agg, tag, wsum[0] + wsum[1] + wsum[2] + wsum[3]);
  }
  GJX_STAMP(1);
  // ---- while the totals are in flight: cumulative weights of tiles b - 1, b, b + 1 RELATIVE to each tile's start.  Written out, not a
  //      rescan_round: the own tile's scan above is reused (scanning it again measured 0.3 us per step at K = 2^20)
  //      (the neighbours' log-weights are requested only now: nothing may delay the publication above, every block waits
  //      for the last one) ----
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int tc = w0 + 2 * c;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) xn[c][k] = 0.0f;
    if (tc >= 0 && tc < nb) load_tile((int64_t)tc * TILE + (int64_t)threadIdx.x * ITEMS, xn[c]);
  }
  {
    uint64_t qn[2][ITEMS], sn[2], incn[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int tc = w0 + 2 * c;
      const bool on = tc >= 0 && tc < nb;
      const int64_t p0 = (int64_t)tc * TILE + (int64_t)threadIdx.x * ITEMS;
      sn[c] = 0;
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) { sn[c] += (on && p0 + k < K) ? weight_q(xn[c], k, mode, mx) : 0; qn[c][k] = sn[c]; }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) incn[c] = wave_scan_u64(sn[c]);
    if (lane == 63) { s_wtot[0][wid] = incn[0]; s_wtot[2][wid] = incn[1]; }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint64_t base = c == 1 ? incown - sown : incn[c >> 1] - sn[c >> 1];
      for (int w = 0; w < wid; ++w) base += s_wtot[c][w];
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) cumL[c * TILE + threadIdx.x * ITEMS + k] = base + (c == 1 ? qown[k] : qn[c >> 1][k]);
    }
  }
  // the totals land in P[1 .. nb] as they are; what the usual case needs of their prefix — the grand total and the weight below the
  // nine-boundary window of source_tiles — is summed on the way (u64 adds: the same bits in any order).  The prefix itself is
  // made only by a block whose slots leave that window (below)
  const int wlo = source_window_start(nb, (int)blockIdx.x);
  uint64_t below = 0, total = 0;
  grid_gather(agg, tag, ctrl, [&](int b, unsigned long long val) {
    P[b + 1] = val;
    total += val;
    below += b < wlo ? val : 0;
  });
  below = wave_sum_u64(below);
  total = wave_sum_u64(total);
  if (lane == 0) { s_sums[wid] = below; s_sums[4 + wid] = total; }
  if (threadIdx.x == 0) P[0] = 0;
  __syncthreads();
  below = sum_partials<4>(s_sums);
  total = sum_partials<4>(s_sums + 4);
  GJX_STAMP(2);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    __hip_atomic_store(&ctrl[0], epoch + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (total == 0) __hip_atomic_fetch_or(&ctrl[2], kStatusZeroTotal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // ---- ancestors of slots i0 .. i0 + ITEMS - 1 (consecutive slots per lane: 16-byte row stores at ITEMS = 4; the
  //      striped assignment, 64 consecutive slots per wave instruction, measured 1.3 us slower at K = 2^20) ----
  int32_t anc[ITEMS];
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) anc[k] = (int32_t)((i0 + k < K) ? i0 + k : 0);   // dead collection: identity (flagged)
  if (total > 0) {   // block-uniform
    const double step = (double)total / (double)K;
    uint64_t T[ITEMS];
    int tile[ITEMS], kpos[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int64_t j = (i0 + k < K) ? i0 + k : K - 1;
      T[k] = comb_threshold(j, u, step, total);
    }
    // the nine boundaries of the window around the own tile: the weight below it plus a serial prefix of eight totals (the same
    // addresses in every lane), and the tile and residual of every slot counted off against them — what source_tiles does on a
    // finished prefix.  Thresholds do not decrease with the slot index, so the block's slots all lie inside the window if its
    // first and its last one do; the tile index does not decrease either, so the block's source tiles are the range between the
    // first and the last slot's tile — no list to build, the two ends (or "outside") travel through LDS behind one barrier
    uint64_t Tr[ITEMS];                             // residual of every slot in its source tile
    uint64_t Pw[9];
    Pw[0] = below;
#pragma unroll
    for (int w = 1; w < 9; ++w) Pw[w] = Pw[w - 1] + (wlo + w <= nb ? P[wlo + w] : 0);
    GJX_STAMP(6);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      tile[k] = wlo;
      uint64_t lo = Pw[0];
#pragma unroll
      for (int w = 1; w < 8; ++w) {
        const bool past = Pw[w] <= T[k];
        tile[k] += past ? 1 : 0;
        lo = past ? Pw[w] : lo;
      }
      Tr[k] = T[k] - lo;
    }
    if (timeline) { asm volatile("" :: "v"(tile[0]), "v"(tile[ITEMS - 1])); GJX_STAMP(7); }
    if (threadIdx.x == 0) s_range[0] = T[0] >= Pw[0] ? tile[0] : INT_MIN;
    if (threadIdx.x == 255) s_range[1] = T[ITEMS - 1] < Pw[8] ? tile[ITEMS - 1] : INT_MAX;
    __syncthreads();
    int tmin = s_range[0], tmax = s_range[1];
    const bool windowed = tmin >= w0 && tmax <= w0 + 2;   // block-uniform: every source tile is in the prefetched window (w0 >= -1)
    int pos[ITEMS];
    const uint64_t* cm[ITEMS];
    if (windowed) {
      GJX_STAMP(3);
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) cm[k] = cumL + (tile[k] - w0) * TILE;
      if constexpr (ITEMS > 1) rank_in_tiles_sorted<TILE, ITEMS>(cm, Tr, pos);
      else rank_in_tiles<TILE, ITEMS>(cm, Tr, pos);
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) anc[k] = (int32_t)((int64_t)tile[k] * TILE + pos[k]);
    } else {
    // collapsed or strongly drifting weights: the full prefix of the totals, the source tiles by descent, and the re-scan.  A round
    // starts at a tile that has weight (block-uniform skip; the range's last tile always has), so collapsed weights far
    // apart cost as many rounds as there are live tiles
    prefix_in_place<256>(P, nb, wsum, NoShift{});   // (every lane read s_range before the barrier inside; the publish read wsum long ago)
    source_tiles<ITEMS>(P, nb, (int)blockIdx.x, T, tile);
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) Tr[k] = T[k] - P[tile[k]];
    if (threadIdx.x == 0) s_range[0] = tile[0];
    if (threadIdx.x == 255) s_range[1] = tile[ITEMS - 1];
    __syncthreads();
    tmin = s_range[0]; tmax = s_range[1];
    const int ntiles = tmax - tmin + 1;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) kpos[k] = tile[k] - tmin;
    auto next_live = [&](int at) { while (at < ntiles && P[tmin + at + 1] == P[tmin + at]) ++at; return at; };
    GJX_STAMP(3);
    // re-scan the source tiles, CH at a time (a window of TILE slots rarely touches more than 3)
    float nv[CH][ITEMS];
#pragma unroll
    for (int c = 0; c < CH; ++c)
      if (c < ntiles) load_tile((int64_t)(tmin + c) * TILE + (int64_t)threadIdx.x * ITEMS, nv[c]);
    for (int idx = 0; idx < ntiles;) {
      const int nidx = next_live(idx + CH);
      // (the barrier inside the round: every lane is done searching the previous round's cumL)
      rescan_round<256, TILE, ITEMS, CH>(cumL, &s_wtot[0][0], [&](int c, int o, uint64_t (&q)[ITEMS]) {
        const bool on = idx + c < ntiles;
        const int64_t p0 = (int64_t)(tmin + idx + c) * TILE + o;
        if (on) {
#pragma unroll
          for (int k = 0; k < ITEMS; ++k) q[k] = (p0 + k < K) ? weight_q(nv[c], k, mode, mx) : 0;
        }
        if (nidx + c < ntiles) load_tile((int64_t)(tmin + nidx + c) * TILE + o, nv[c]);   // next round, in flight
        return on;
      }, [] {});
      // first particle p of the slot's tile with cum_incl(p) > T (a slot of another round is left out; with one slot per lane it
      // searches the round's first tile for nothing)
      bool mine[ITEMS];
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) {
        mine[k] = kpos[k] >= idx && kpos[k] < idx + CH;
        cm[k] = cumL + (mine[k] ? (kpos[k] - idx) * TILE : 0);
      }
      if constexpr (ITEMS > 1) rank_in_tiles_sorted<TILE, ITEMS>(cm, Tr, mine, pos);
      else rank_in_tiles<TILE, ITEMS>(cm, Tr, pos);
#pragma unroll
      for (int k = 0; k < ITEMS; ++k)
        if (mine[k]) anc[k] = (int32_t)((int64_t)tile[k] * TILE + pos[k]);
      idx = nidx;
    }
    }
  }
  GJX_STAMP(4);
  // if a rendezvous timed out (grid not co-resident) the totals are partial and the ancestors undefined (the caller
  // repeats the call): keep them inside the rows whatever happened — one v_med3_i32 per slot
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) anc[k] = max(0, min(anc[k], (int32_t)(K - 1)));
  // ---- children: rows of the ancestors, ITEMS consecutive slots per lane ----
  const bool whole = i0 + ITEMS <= K;
  if (ancestors) {
    if (ITEMS == 4 && whole) *(int4*)(ancestors + i0) = make_int4(anc[0], anc[1], anc[2], anc[3]);
    else {
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) if (i0 + k < K) ancestors[i0 + k] = anc[k];
    }
  }
  const bool vec = ITEMS == 4 && whole && (dst_stride & 3) == 0 && (((uintptr_t)dst) & 15) == 0;
  if (vec) {
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
      const float* sr = src + (int64_t)r * src_stride;
      float4 v;
      v.x = sr[anc[0]]; v.y = sr[anc[ITEMS > 1 ? 1 : 0]]; v.z = sr[anc[ITEMS > 2 ? 2 : 0]]; v.w = sr[anc[ITEMS > 3 ? 3 : 0]];
      *(float4*)(dst + (int64_t)r * dst_stride + i0) = v;
    }
  } else {
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
      const float* sr = src + (int64_t)r * src_stride;
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) if (i0 + k < K) dst[(int64_t)r * dst_stride + i0 + k] = sr[anc[k]];
    }
  }
  GJX_STAMP(5);
#undef GJX_STAMP
}

// ------------------------------------------------------------------------------------------
// Resampling + gather under the TILE-SCALED scheme (GJX_WEIGHTS_TILE_SCALED, include/gjx.h), N = K: a PLAIN kernel — no
// rendezvous, no co-resident grid, any K up to kGatherTiledMaxTiles tiles.  The {e_b, S_b} of every 1024-particle tile
// exist before the launch: the propagate kernel leaves them beside its LSE partials when a block of it covers whole
// tiles (gjx_run_program, k_run_gmm_flat<.., TILES>), otherwise k_tile_totals computes them (one small launch).  Every
// block reads all of them (12 B per tile), takes the maximum exponent, shifts, prefixes, and is the consumer of the
// output slots [b 1024, (b+1) 1024) exactly as k_resample_gather: thresholds, source tile in a window of the prefix,
// cumulative q of tiles b-1 .. b+1 laid out in LDS from the log-weights (quantised against each tile's OWN exponent),
// 4-ary search of the residual, rows copied.  Every load the head needs is issued at the top: the head is one memory
// latency plus LDS work instead of two fabric round trips.  Ancestors are those of gjx_resample_indices_tiled bit for bit.
// ------------------------------------------------------------------------------------------
constexpr int kGatherTiledMaxTiles = 65536;

// {S_b, E_b} of every tile from the log-weights (what k_tiled_quantise computes, without the cumulative array)
// GATED (the adaptive filter, gjx_scan_filter_adaptive): *gate == 0 means "this step does not resample" — nothing is written
template <bool GATED>
__global__ __launch_bounds__(kTileQ) void k_tile_totals(const float* __restrict__ logw, int64_t K, uint64_t* S, int32_t* E, const int32_t* gate) {
  constexpr int NW = kTileQ / 64;
  if (GATED && *gate == 0) return;
  __shared__ float fred[NW];
  __shared__ uint64_t wsum[NW];
  const int64_t i = (int64_t)blockIdx.x * kTileQ + threadIdx.x;
  const float lw[1] = {i < K ? logw[i] : -INFINITY};
  uint64_t q[1], inc;
  const int e = tile_quantise<kTileQ, 1>(lw, fred, wsum, q, inc);
  if (threadIdx.x == 0) {
    const uint64_t tot = sum_partials<NW>(wsum);
    S[blockIdx.x] = tot;
    E[blockIdx.x] = tot ? e : kTileDead;
  }
}

// PLANNED (more than 1024 tiles): the maximum exponent, the shifts and the prefix were computed ONCE by k_tiled_plan (one
// small launch) and are read from memory — a block touches the nine prefix entries around its own index — instead of
// every block reducing all nt granules again (O(nt^2) reads and 72 KB of LDS at nt = 4096).
// GATED: *gate == 0 -> identity ancestors (the rows, if any, are copied as they are); tile totals, plan and status word are not read
template <int ITEMS, bool PLANNED, bool GATED>
__global__ __launch_bounds__(256) void k_resample_gather_tiled(const float* __restrict__ x, int64_t K, const uint64_t* __restrict__ S,
                                                              const int32_t* __restrict__ E, const uint64_t* __restrict__ Pg,
                                                              const int32_t* __restrict__ shg, int lse_mode, const float* lse,
                                                              int n_partials, float* lse_out, float log_k_total, double u,
                                                              const float* __restrict__ src, int64_t src_stride, int rows,
                                                              float* __restrict__ dst, int64_t dst_stride, int32_t* ancestors,
                                                              unsigned* ctrl, unsigned long long* timeline, const int32_t* gate) {
#define GJX_STAMP(n) do { if (timeline && threadIdx.x == 0) timeline[blockIdx.x * 8 + (n)] = __builtin_amdgcn_s_memrealtime(); } while (0)
  GJX_STAMP(0);
  static_assert(ITEMS == 4, "a block consumes one quantisation tile: 256 lanes x 4 slots");
  extern __shared__ __align__(16) unsigned char gt_dyn[];
  const int nt = (int)gridDim.x;
  uint64_t* const Pl = (uint64_t*)gt_dyn;                      // [nt + 1] prefix of the shifted tile totals (!PLANNED)
  int32_t* const Ebl = (int32_t*)(Pl + ((nt + 2) & ~1));       // [nt] tile exponents (!PLANNED)
  __shared__ TiledSearchShared sh;
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * ITEMS;
  int32_t anc[ITEMS];
  if (GATED && *gate == 0) {     // grid-uniform
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) anc[k] = (int32_t)((i0 + k < K) ? i0 + k : K - 1);
  } else
  tiled_search_tile<PLANNED>(x, K, S, E, Pg, shg, nt, (int)blockIdx.x, Pl, Ebl, sh, lse_mode, lse, n_partials, lse_out, log_k_total, u, ctrl, timeline, anc);
  GJX_STAMP(4);
  // ---- children: rows of the ancestors, ITEMS consecutive slots per lane ----
  const bool whole = i0 + ITEMS <= K;
  if (ancestors) {
    if (whole) *(int4*)(ancestors + i0) = make_int4(anc[0], anc[1], anc[2], anc[3]);
    else {
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) if (i0 + k < K) ancestors[i0 + k] = anc[k];
    }
  }
  const bool vec = whole && (dst_stride & 3) == 0 && (((uintptr_t)dst) & 15) == 0;
  if (vec) {
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
      const float* sr = src + (int64_t)r * src_stride;
      float4 v;
      v.x = sr[anc[0]]; v.y = sr[anc[1]]; v.z = sr[anc[2]]; v.w = sr[anc[3]];
      *(float4*)(dst + (int64_t)r * dst_stride + i0) = v;
    }
  } else {
#pragma unroll 4
    for (int r = 0; r < rows; ++r) {
      const float* sr = src + (int64_t)r * src_stride;
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) if (i0 + k < K) dst[(int64_t)r * dst_stride + i0 + k] = sr[anc[k]];
    }
  }
  GJX_STAMP(5);
#undef GJX_STAMP
}

__global__ __launch_bounds__(256) void k_multinomial(const uint64_t* cum, int64_t K, const uint64_t* base_total,
                                                    key2 key, int64_t out_begin, int64_t n_out, int32_t* ancestors) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_out) return;
  const uint64_t base = base_total[0], total = base_total[1];
  const key2 h = fold_in64(key, (uint64_t)(out_begin + j));
  const uint64_t r = (((uint64_t)h.a << 32) | h.b) >> 11;
  const double uj = (double)r * (1.0 / 9007199254740992.0);
  const uint64_t T = (uint64_t)(uj * (double)total);
  int32_t a = -1;
  if (K > 0) {
    const uint64_t local = cum[K - 1];
    if (T >= base && T < base + local) a = (int32_t)upper_search(cum, K, T - base);
  }
  ancestors[j] = a;
}

__global__ __launch_bounds__(256) void k_gather_rows(const float* __restrict__ src, int64_t src_stride,
                                                    const int32_t* __restrict__ anc, int64_t n_out, int rows,
                                                    float* __restrict__ dst, int64_t dst_stride) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_out) return;
  const int32_t a = anc[j];
  // a < 0: a slot another rank fills (prefilled -1).  a >= src_stride cannot come from a completed resampling, but the
  // ancestors of a co-resident kernel that timed out are undefined (the caller repeats the call): never read outside the rows
  if ((uint64_t)(int64_t)a >= (uint64_t)src_stride) return;
  for (int r = 0; r < rows; ++r) dst[(int64_t)r * dst_stride + j] = src[(int64_t)r * src_stride + a];
}


// planned expansion for a sharded collection (gjx_shard.hip): slot run read from the device plan
int launch_expand_planned(const uint64_t* cum, int64_t K, const gjx_shard_plan* plan_dev, double u, int64_t N_total,
                          int32_t* ancestors, int64_t anc_capacity, hipStream_t st) {
  const uint64_t* bt = reinterpret_cast<const uint64_t*>(plan_dev);                       // {base, total}
  const int64_t* range = reinterpret_cast<const int64_t*>(plan_dev) + 2;                  // {slot0, n_valid}
  hipLaunchKernelGGL(k_systematic_expand<false>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, st, cum, K, bt, u, N_total,
                     (int64_t)0, anc_capacity, ancestors, (const float*)nullptr, (int64_t)0, 0, (float*)nullptr, (int64_t)0,
                     range);
  GJX_CHECK_LAUNCH("gjx_shard_resample(expand)");
  return GJX_OK;
}

// ------------------------------------------------------------------------------------------
// Effective sample size, and the weight bookkeeping of the adaptive filter (gjx_scan_filter_adaptive) fused into it.
// One block per 1024-particle tile (256 lanes x 4 particles): W = fresh ? inc : W + inc in place (ACC: 8 B read + 4 B written per
// particle; !ACC, gjx_ess: 4 B read), tile maximum m_b, s1_b = sum exp(W - m_b), s2_b = sum exp(2 (W - m_b)) by the wave reductions
// of this file.  A block publishes {m_b, s1_b} as one 8-byte and s2_b as one 4-byte agent-scope store, drains them and takes a
// ticket — ONE atomic per block (k_count_flags, gjx_scanfilter.hip) —; the block that draws the last ticket combines the tiles:
// M = max m_b, S1 = sum_b s1_b exp(m_b - M), S2 = sum_b s2_b exp(2 (m_b - M)), lane l summing tiles [l per, (l + 1) per) in order,
// then the fixed-order wave sum and the four waves in order: a function of the weights and of K alone, never of a launch geometry.
// It writes the LSE record of the step, ESS = S1^2 / S2 and the decision word the launches in front of the next step read.
// Plain vector stores, no host in the loop.  NaN and -inf weights count as dead (fmaxf drops a NaN, its term is clamped to 0).
// ------------------------------------------------------------------------------------------
struct EssArgs {
  const float* inc;            // ACC: the step's incremental log-weights
  float* W;                    // the carried log-weights (!ACC: read only)
  float* w_copy;               // ACC: W is stored here too when not NULL (the last step: the caller's logw)
  int64_t K;
  const int32_t* fresh;        // ACC: device word, != 0: the collection was resampled in front of this step (carried weights are 0); NULL: yes
  unsigned long long* pm;      // [nt] {m_b, s1_b}
  unsigned* p2;                // [nt] s2_b
  unsigned* ticket;
  float* out4;                 // !ACC: {M, S1, S2, ESS}
  float* lse_rec;              // ACC: {M, S1, lse, lse - c}
  const float* lse_prev;       // ACC: the record of the step before (c behind a skip), NULL at step 0
  float log_k;
  float* ess_out;
  int32_t* decide_out;         // or NULL (the last step)
  float tau_k;                 // ess_threshold * K
  int always;                  // ess_threshold >= 1
};

template <bool ACC>
__global__ __launch_bounds__(256) void k_ess_tiles(const EssArgs a) {
  __shared__ float red[13];
  __shared__ float fin[12];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nt = (int)gridDim.x;
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  // 16-byte accesses where the tile is whole and the buffers are aligned (kernel-uniform but for the last block)
  const bool vec = i0 + 4 <= a.K && ((((uintptr_t)a.W) | (ACC ? ((uintptr_t)a.inc | (uintptr_t)a.w_copy) : 0)) & 15) == 0;
  float w[4];
  if (ACC) {
    const bool fresh = a.fresh ? *a.fresh != 0 : true;     // grid-uniform
    if (vec) {
      const float4 q = *(const float4*)(a.inc + i0);
      w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
      if (!fresh) {
        const float4 c = *(const float4*)(a.W + i0);
        w[0] += c.x; w[1] += c.y; w[2] += c.z; w[3] += c.w;
      }
      *(float4*)(a.W + i0) = make_float4(w[0], w[1], w[2], w[3]);
      if (a.w_copy) *(float4*)(a.w_copy + i0) = make_float4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        w[k] = -INFINITY;
        if (i0 + k < a.K) {
          w[k] = a.inc[i0 + k];
          if (!fresh) w[k] += a.W[i0 + k];
          a.W[i0 + k] = w[k];
          if (a.w_copy) a.w_copy[i0 + k] = w[k];
        }
      }
    }
  } else if (vec) {
    const float4 c = *(const float4*)(a.W + i0);
    w[0] = c.x; w[1] = c.y; w[2] = c.z; w[3] = c.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = (i0 + k < a.K) ? a.W[i0 + k] : -INFINITY;
  }
  const float wm = wave_max(fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3])));
  if (lane == 0) red[wid] = wm;
  __syncthreads();
  const float bm = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float s1 = 0.0f, s2 = 0.0f;
  if (bm > -INFINITY) {      // block-uniform
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float e = fast_exp(w[k] - bm);
      e = e > 0.0f ? e : 0.0f;        // (a NaN weight: dead)
      s1 += e;
      s2 = fmaf(e, e, s2);
    }
  }
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if (lane == 0) { red[4 + wid] = s1; red[8 + wid] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float b1 = (red[4] + red[5]) + (red[6] + red[7]), b2 = (red[8] + red[9]) + (red[10] + red[11]);
    __hip_atomic_store(&a.pm[blockIdx.x], pack_f2(bm, b1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&a.p2[blockIdx.x], __float_as_uint(b2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    red[12] = (t == (unsigned)(nt - 1)) ? 1.0f : 0.0f;
  }
  __syncthreads();
  if (red[12] == 0.0f) return;
  // ---- the finishing block: every tile's partials with agent-scope loads ----
  float M = -INFINITY;
  for (int b = threadIdx.x; b < nt; b += 256)
    M = fmaxf(M, __uint_as_float((unsigned)__hip_atomic_load(&a.pm[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)));
  M = wave_max(M);
  if (lane == 0) fin[wid] = M;
  __syncthreads();
  M = fmaxf(fmaxf(fin[0], fin[1]), fmaxf(fin[2], fin[3]));
  float S1 = 0.0f, S2 = 0.0f;
  if (M > -INFINITY) {
    const int per = (nt + 255) >> 8;
    const int b0 = threadIdx.x * per, b1 = b0 + per < nt ? b0 + per : nt;
    for (int b = b0; b < b1; ++b) {
      const unsigned long long v = __hip_atomic_load(&a.pm[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const float t2 = __uint_as_float(__hip_atomic_load(&a.p2[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const float f = fast_exp(__uint_as_float((unsigned)v) - M);      // (a dead tile: exp(-inf) = 0 against sums that are 0)
      S1 = fmaf(__uint_as_float((unsigned)(v >> 32)), f, S1);
      S2 = fmaf(t2, f * f, S2);
    }
  }
  S1 = wave_sum(S1);
  S2 = wave_sum(S2);
  if (lane == 0) { fin[4 + wid] = S1; fin[8 + wid] = S2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    S1 = (fin[4] + fin[5]) + (fin[6] + fin[7]);
    S2 = (fin[8] + fin[9]) + (fin[10] + fin[11]);
    const bool live = M > -INFINITY && S2 > 0.0f;
    const float ess = live ? S1 * S1 / S2 : 0.0f;
    if (!ACC) { a.out4[0] = M; a.out4[1] = S1; a.out4[2] = S2; a.out4[3] = ess; }
    if (ACC) {
      const bool fresh = a.fresh ? *a.fresh != 0 : true;
      const float ls = logf(S1);
      const float l = live ? M + ls : -INFINITY;
      // lse(W_t) - c_t: behind a skip c_t = lse(W_{t-1}); the difference is formed from the maxima and the sums separately (two
      // numbers of the size of log-ML would cancel to a step's increment otherwise)
      float d = l - a.log_k;
      if (!fresh && a.lse_prev) d = live ? (M - a.lse_prev[0]) + (ls - logf(a.lse_prev[1])) : -INFINITY;
      a.lse_rec[0] = M; a.lse_rec[1] = S1; a.lse_rec[2] = l; a.lse_rec[3] = d;
      a.ess_out[0] = ess;
      if (a.decide_out) a.decide_out[0] = (a.always || ess < a.tau_k) ? 1 : 0;
    }
    __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// workspace: [256 B control: word 0 the ticket][pm u64 nt][p2 u32 nt]
static int ess_workspace(void* workspace, size_t workspace_bytes, int64_t nt, EssArgs& a) {
  if (!workspace || workspace_bytes < kWsHeaderBytes + 12 * (size_t)nt) return -1;
  a.ticket = (unsigned*)workspace;
  a.pm = (unsigned long long*)((char*)workspace + kWsHeaderBytes);
  a.p2 = (unsigned*)(a.pm + nt);
  return 0;
}

int launch_ess_accumulate(const float* inc, float* W, float* w_copy, int64_t K, const int32_t* fresh, float* lse_rec, const float* lse_prev,
                          float* ess_out, int32_t* decide_out, float tau, void* workspace, size_t workspace_bytes, hipStream_t st) {
  const int64_t nt = (K + kTileQ - 1) / kTileQ;
  EssArgs a;
  memset(&a, 0, sizeof(a));
  if (ess_workspace(workspace, workspace_bytes, nt, a)) return gjx_fail(GJX_EWORKSPACE, "gjx_scan_filter_adaptive: workspace too small");
  a.inc = inc; a.W = W; a.w_copy = w_copy; a.K = K; a.fresh = fresh; a.lse_rec = lse_rec; a.lse_prev = lse_prev;
  a.log_k = (float)log((double)K); a.ess_out = ess_out; a.decide_out = decide_out; a.tau_k = tau * (float)K; a.always = tau >= 1.0f;
  hipLaunchKernelGGL(k_ess_tiles<true>, dim3((unsigned)nt), dim3(256), 0, st, a);
  GJX_CHECK_LAUNCH("gjx_scan_filter_adaptive(weights + ESS)");
  return GJX_OK;
}

// ---- the tile-scaled systematic resampler as three plain launches (gjx_resample_indices_tiled): the step-by-step
//      form of what k_pf_persistent (gjx_pfilter.inl) does inside its loop; bit-identical ancestors ----
__global__ __launch_bounds__(kTileQ) void k_tiled_quantise(const float* logw, int64_t K, uint64_t* cq, uint64_t* S, int32_t* E,
                                                           uint32_t* q_out, int32_t* e_out) {
  constexpr int NW = kTileQ / 64;
  __shared__ float fred[NW];
  __shared__ uint64_t wsum[NW];
  const int wid = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * kTileQ + threadIdx.x;
  const bool active = i < K;
  const float lw[1] = {active ? logw[i] : -INFINITY};
  uint64_t q[1], inc;
  const int e = tile_quantise<kTileQ, 1>(lw, fred, wsum, q, inc);
  uint64_t base = 0, tot = 0;
  for (int w = 0; w < NW; ++w) { if (w < wid) base += wsum[w]; tot += wsum[w]; }
  if (active) { cq[i] = base + inc; if (q_out) q_out[i] = (uint32_t)q[0]; }
  if (threadIdx.x == 0) {
    const int es = tot ? e : kTileDead;
    S[blockIdx.x] = tot; E[blockIdx.x] = es;
    if (e_out) e_out[blockIdx.x] = es;
  }
}

// GATED (the adaptive filter): *gate == 0 means "this step does not resample" — nothing is read or written
template <bool GATED = false>
__global__ __launch_bounds__(1024) void k_tiled_plan(const uint64_t* S, const int32_t* E, int nt, uint64_t* P, int32_t* sh, unsigned* ctrl,
                                                     const int32_t* gate = nullptr) {
  __shared__ float fred[16];
  if (GATED && *gate == 0) return;
  __shared__ uint64_t wsum[16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float em = (float)kTileDead;
  for (int b = threadIdx.x; b < nt; b += 1024) em = fmaxf(em, (float)E[b]);
  em = wave_max(em);
  if (lane == 0) fred[wid] = em;
  __syncthreads();
  em = fred[0];
  for (int w = 1; w < 16; ++w) em = fmaxf(em, fred[w]);
  const int Emax = (int)em;
  if (threadIdx.x == 0) P[0] = 0;
  const uint64_t total = block_scan_chunked(nt, wsum, [&](int b) {
    const int s = Emax - E[b];
    sh[b] = s < 64 ? s : 64;
    return s < 64 ? S[b] >> s : 0ull;
  }, [&](int b, uint64_t p) { P[b + 1] = p; });
  if (threadIdx.x == 0 && total == 0 && ctrl) __hip_atomic_fetch_or(&ctrl[2], kStatusZeroTotal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_tiled_ancestors(const uint64_t* P, const int32_t* sh, const uint64_t* cq, int nt, int64_t K,
                                                         double u, int64_t N, int32_t* anc) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= N) return;
  const uint64_t total = P[nt];
  if (total == 0) { anc[j] = (int32_t)(j < K ? j : K - 1); return; }   // dead collection: identity, flagged by the plan
  const double step = (double)total / (double)N;
  anc[j] = (int32_t)tiled_lookup(P, sh, cq, nt, K, comb_threshold(j, u, step, total));
}

// ---- multinomial resampling by SORTED uniforms on the tile-scaled weight line (gjx_resample_sorted_multinomial_tiled): slot j's
//      threshold is floor(total * S_j / S_N+1) with S_j the running sum of the exponential spacings exp_spacing(bits(key, j)) — the
//      order statistics of N iid uniforms, so the ancestors are a multinomial draw delivered in non-decreasing order.  The spacings
//      are exact integers (gjx_device.h): their sums do not depend on how the slots are cut into tiles. ----
__global__ __launch_bounds__(kTileQ) void k_spacing_totals(key2 key, int64_t N, uint64_t* SS) {
  constexpr int NW = kTileQ / 64;
  __shared__ uint64_t wsum[NW];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * kTileQ + threadIdx.x;
  uint64_t e = j <= N ? exp_spacing(fold_in64(key, (uint64_t)j).a) : 0ull;     // (slot N: the spacing that closes the unit interval)
  e = wave_scan_u64(e);
  if (lane == 63) wsum[wid] = e;
  __syncthreads();
  if (threadIdx.x == 0) SS[blockIdx.x] = sum_partials<NW>(wsum);
}

__global__ __launch_bounds__(1024) void k_spacing_plan(const uint64_t* SS, int nb, uint64_t* SP) {
  __shared__ uint64_t wsum[16];
  if (threadIdx.x == 0) SP[0] = 0;
  block_scan_chunked(nb, wsum, [&](int b) { return SS[b]; }, [&](int b, uint64_t p) { SP[b + 1] = p; });
}

__global__ __launch_bounds__(kTileQ) void k_sorted_ancestors(const uint64_t* P, const int32_t* sh, const uint64_t* cq, int nt, int64_t K, key2 key,
                                                             const uint64_t* SP, int nb, int64_t N, int32_t* anc) {
  constexpr int NW = kTileQ / 64;
  __shared__ uint64_t wsum[NW];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * kTileQ + threadIdx.x;
  uint64_t e = j < N ? exp_spacing(fold_in64(key, (uint64_t)j).a) : 0ull;
  e = wave_scan_u64(e);
  if (lane == 63) wsum[wid] = e;
  __syncthreads();
  uint64_t Sj = SP[blockIdx.x] + e;
  for (int w = 0; w < wid; ++w) Sj += wsum[w];
  if (j >= N) return;
  const uint64_t total = P[nt];
  if (total == 0) { anc[j] = (int32_t)(j < K ? j : K - 1); return; }   // dead collection: identity, flagged by the plan
  anc[j] = (int32_t)tiled_lookup(P, sh, cq, nt, K, sorted_threshold(Sj, SP[nb], total));
}

int launch_tiled_plan(const uint64_t* S, const int32_t* E, int nt, uint64_t* P, int32_t* sh, unsigned* ctrl, hipStream_t st, const int32_t* gate) {
  if (gate) hipLaunchKernelGGL(k_tiled_plan<true>, dim3(1), dim3(1024), 0, st, S, E, nt, P, sh, ctrl, gate);
  else hipLaunchKernelGGL(k_tiled_plan<false>, dim3(1), dim3(1024), 0, st, S, E, nt, P, sh, ctrl, (const int32_t*)nullptr);
  GJX_CHECK_LAUNCH("k_tiled_plan");
  return GJX_OK;
}

}  // namespace gjx

using namespace gjx;

extern "C" int gjx_categorical_pick(const float* logw, int64_t K, int64_t particle_offset, const float* lse,
                                    uint32_t key0, uint32_t key1, int32_t rng_mode, void* out_dev,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!logw || !lse || !out_dev || K <= 0) return gjx_fail(GJX_EINVAL, "gjx_categorical_pick: bad argument");
  if (!workspace || workspace_bytes < gjx_workspace_bytes(GJX_OP_PICK, K)) return gjx_fail(GJX_EWORKSPACE, "gjx_categorical_pick: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t want = (K + 1023) / 1024;
  const int nblocks = (int)(want < 2048 ? (want < 1 ? 1 : want) : 2048);
  PickPair* partials = (PickPair*)((char*)workspace + kWsHeaderBytes);
  if (rng_mode == GJX_RNG_JAX32)
    hipLaunchKernelGGL(k_pick_partial<GJX_RNG_JAX32>, dim3(nblocks), dim3(256), 0, st, logw, K, particle_offset, lse, key2{key0, key1}, partials);
  else
    hipLaunchKernelGGL(k_pick_partial<GJX_RNG_FLAT>, dim3(nblocks), dim3(256), 0, st, logw, K, particle_offset, lse, key2{key0, key1}, partials);
  GJX_CHECK_LAUNCH("gjx_categorical_pick/partial");
  hipLaunchKernelGGL(k_pick_finish, dim3(1), dim3(256), 0, st, (const PickPair*)partials, nblocks, (PickPair*)out_dev);
  GJX_CHECK_LAUNCH("gjx_categorical_pick/finish");
  return GJX_OK;
}

extern "C" int gjx_trials_lse_pick(const float* logw, int64_t n_trials, int64_t K, int64_t particle_offset, uint32_t key0, uint32_t key1,
                                   int32_t rng_mode, float* lse_out, int32_t* pick_out, void* stream) {
  if (!logw || !lse_out || n_trials <= 0 || K <= 0 || n_trials > 0x7fffffffLL || particle_offset < 0 ||
      (pick_out && particle_offset + n_trials * K > 0x7fffffffLL))
    return gjx_fail(GJX_EINVAL, "gjx_trials_lse_pick: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const float log_k = (float)log((double)K);
  if (rng_mode == GJX_RNG_JAX32)
    hipLaunchKernelGGL(k_trials_lse_pick<GJX_RNG_JAX32>, dim3((unsigned)n_trials), dim3(256), 0, st, logw, K, particle_offset, key2{key0, key1},
                       pick_out ? 1 : 0, log_k, lse_out, pick_out);
  else
    hipLaunchKernelGGL(k_trials_lse_pick<GJX_RNG_FLAT>, dim3((unsigned)n_trials), dim3(256), 0, st, logw, K, particle_offset, key2{key0, key1},
                       pick_out ? 1 : 0, log_k, lse_out, pick_out);
  GJX_CHECK_LAUNCH("gjx_trials_lse_pick");
  return GJX_OK;
}

extern "C" int gjx_weight_cumsum(const float* x, int64_t K, int32_t is_log, const float* lse, int32_t n_partials,
                                 uint64_t* cum, uint64_t* base_total_dev, float* lse_out, int64_t K_total,
                                 void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || !cum || !base_total_dev || K <= 0 || is_log < 0 || is_log > 2 || (is_log && !lse) || (is_log == 2 && n_partials <= 0))
    return gjx_fail(GJX_EINVAL, "gjx_weight_cumsum: bad argument");
  if (!workspace || workspace_bytes < gjx_workspace_bytes(GJX_OP_RESAMPLE, K)) return gjx_fail(GJX_EWORKSPACE, "gjx_weight_cumsum: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblocks = (int)((K + kScanTile - 1) / kScanTile);
  uint64_t* bs = (uint64_t*)((char*)workspace + kWsHeaderBytes);
  const float log_k = (float)log((double)(K_total > 0 ? K_total : K));
  hipLaunchKernelGGL(k_wsum_blocks, dim3(nblocks), dim3(256), 0, st, x, K, (int)is_log, lse, (int)n_partials, lse_out, log_k, bs);
  GJX_CHECK_LAUNCH("gjx_weight_cumsum/sum");
  hipLaunchKernelGGL(k_wscan_write, dim3(nblocks), dim3(256), 0, st, x, K, (int)is_log, lse, (int)n_partials, (const uint64_t*)bs, cum, base_total_dev);
  GJX_CHECK_LAUNCH("gjx_weight_cumsum/write");
  return GJX_OK;
}

extern "C" int gjx_resample_systematic(const uint64_t* cum, int64_t K, const uint64_t* base_total_dev, double u,
                                       int64_t N_total, int64_t out_begin, int64_t n_out, int32_t* ancestors,
                                       void* stream) {
  if (!cum || !base_total_dev || !ancestors || K <= 0 || N_total <= 0 || n_out < 0 || !(u >= 0.0 && u < 1.0))
    return gjx_fail(GJX_EINVAL, "gjx_resample_systematic: bad argument");
  if (n_out == 0) return GJX_OK;
  hipLaunchKernelGGL(k_systematic_expand<false>, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cum, K,
                     base_total_dev, u, N_total, out_begin, n_out, ancestors, (const float*)nullptr, (int64_t)0, 0,
                     (float*)nullptr, (int64_t)0);
  GJX_CHECK_LAUNCH("gjx_resample_systematic");
  return GJX_OK;
}

static int env_items() {
  const char* e = getenv("GJX_RESAMPLE_ITEMS");
  const int v = e ? atoi(e) : 0;
  return (v == 1 || v == 4 || v == 16) ? v : 0;
}

extern "C" int gjx_resample_indices(const float* x, int64_t K, int32_t is_log, const float* lse, int32_t n_partials,
                                    double u, int64_t N, int32_t* ancestors, uint64_t* cum, uint64_t* base_total_dev,
                                    float* lse_out, int64_t K_total, void* workspace, size_t workspace_bytes, void* stream) {
  if (!x || K <= 0 || N <= 0 || is_log < 0 || is_log > 2 || (is_log && !lse) || (is_log == 2 && n_partials <= 0) ||
      !(u >= 0.0 && u < 1.0) || (!ancestors && !cum))
    return gjx_fail(GJX_EINVAL, "gjx_resample_indices: bad argument");
  if (!workspace || workspace_bytes < gjx_workspace_bytes(GJX_OP_RESAMPLE, K)) return gjx_fail(GJX_EWORKSPACE, "gjx_resample_indices: workspace too small");
  // One co-resident grid: the blocks all-gather their tile totals through memory, so every block must be running.
  // The capacity comes from the occupancy query (70 / 118 registers per lane at 4 / 16 particles per lane, 30 KB of
  // LDS: 4 blocks per CU on a full MI355X, fewer on a partitioned device); 1 particle per lane while the grid fits
  // (4x the waves to hide the round trips), then 4, then 16; beyond that the three-launch path runs.
  int items = env_items();
  int64_t nblocks = 0;
  const int cand[3] = {1, 4, 16};
  bool fits = false;
  for (int c = 0; c < 3 && !fits; ++c) {
    if (items && cand[c] != items) continue;
    const void* fn = cand[c] == 1 ? (const void*)k_resample_fused<1> : cand[c] == 4 ? (const void*)k_resample_fused<4> : (const void*)k_resample_fused<16>;
    const int cap = gjx_coresident_blocks(fn, 256, 0);
    nblocks = (K + 256 * (int64_t)cand[c] - 1) / (256 * (int64_t)cand[c]);
    if (nblocks <= cap) { items = cand[c]; fits = true; }
  }
  hipStream_t st = (hipStream_t)stream;
  if (!fits || !ancestors) {
    if (!cum || !base_total_dev) return gjx_fail(GJX_EUNSUPPORTED, "gjx_resample_indices: the grid would not be co-resident on this device and there are no cum/base_total buffers for the three-launch path");
    int rc = gjx_weight_cumsum(x, K, is_log, lse, n_partials, cum, base_total_dev, lse_out, K_total, workspace, workspace_bytes, stream);
    if (rc || !ancestors) return rc;
    return gjx_resample_systematic(cum, K, base_total_dev, u, N, 0, N, ancestors, stream);
  }
  unsigned* ctrl = (unsigned*)workspace + 8;  // control block words 8..10: epoch, -, error (0..7 belong to the LSE ticket)
  unsigned long long* agg = (unsigned long long*)((char*)workspace + kWsHeaderBytes);
  const float log_k = (float)log((double)(K_total > 0 ? K_total : K));
#define GJX_RF(IT) hipLaunchKernelGGL((k_resample_fused<IT>), dim3((unsigned)nblocks), dim3(256), 0, st, x, K, (int)is_log, lse, \
                                      (int)n_partials, lse_out, log_k, u, N, ancestors, cum, base_total_dev, agg, ctrl)
  if (items == 1) GJX_RF(1); else if (items == 4) GJX_RF(4); else GJX_RF(16);
#undef GJX_RF
  GJX_CHECK_LAUNCH("gjx_resample_indices");
  return GJX_OK;
}

extern "C" int gjx_resample_gather(const float* x, int64_t K, int32_t is_log, const float* lse, int32_t n_partials, double u,
                                   const float* src, int64_t src_stride, int32_t rows, float* dst, int64_t dst_stride,
                                   int32_t* ancestors, float* lse_out, int64_t K_total, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  if (!x || K <= 0 || is_log < 0 || is_log > 2 || (is_log && !lse) || (is_log == 2 && n_partials <= 0) ||
      !(u >= 0.0 && u < 1.0) || rows < 0 || (rows > 0 && (!src || !dst)) || K > 0x7fffffffLL)
    return gjx_fail(GJX_EINVAL, "gjx_resample_gather: bad argument");
  if (!workspace || workspace_bytes < gjx_workspace_bytes(GJX_OP_RESAMPLE, K)) return gjx_fail(GJX_EWORKSPACE, "gjx_resample_gather: workspace too small");
  int items = 0;
  int64_t nblocks = 0;
  const int cand[2] = {1, 4};
  const int forced = env_items();
  for (int c = 0; c < 2 && !items; ++c) {
    if (forced && cand[c] != forced) continue;
    const void* fn = cand[c] == 1 ? (const void*)k_resample_gather<1> : (const void*)k_resample_gather<4>;
    const int cap = gjx_coresident_blocks(fn, 256, 0);
    nblocks = (K + 256 * (int64_t)cand[c] - 1) / (256 * (int64_t)cand[c]);
    if (nblocks <= cap && nblocks <= kGatherMaxTiles) items = cand[c];
  }
  if (!items) return gjx_fail(GJX_EUNSUPPORTED, "gjx_resample_gather: K is too large for one co-resident grid on this device (use gjx_resample_indices + gjx_gather_rows)");
  hipStream_t st = (hipStream_t)stream;
  unsigned* ctrl = (unsigned*)workspace + 8;
  unsigned long long* agg = (unsigned long long*)((char*)workspace + kWsHeaderBytes);
  const float log_k = (float)log((double)(K_total > 0 ? K_total : K));
  unsigned long long* timeline = nullptr;   // debug: per-block phase stamps (profiles/microbench/gather_timeline.py)
  timeline = gjx::debug_timeline(64 * (size_t)nblocks);
#define GJX_RG(IT) hipLaunchKernelGGL((k_resample_gather<IT>), dim3((unsigned)nblocks), dim3(256), 0, st, x, K, (int)is_log, lse, \
                                      (int)n_partials, lse_out, log_k, u, src, src_stride, (int)rows, dst, dst_stride, ancestors, agg, ctrl, timeline)
  if (items == 1) GJX_RG(1); else GJX_RG(4);
#undef GJX_RG
  GJX_CHECK_LAUNCH("gjx_resample_gather");
  return GJX_OK;
}

// gjx_resample_gather_tiled, and (gate != NULL) its gated form: every launch reads the device word *gate first (gjx_host.h)
int gjx::resample_gather_tiled_gated(const float* logw, int64_t K, const uint64_t* tile_S, const int32_t* tile_E, int32_t lse_mode,
                                     const float* lse, int32_t n_partials, double u, const float* src, int64_t src_stride,
                                     int32_t rows, float* dst, int64_t dst_stride, int32_t* ancestors, float* lse_out,
                                     int64_t K_total, void* workspace, size_t workspace_bytes, void* stream, const int32_t* gate) {
  if (!logw || K <= 0 || !(u >= 0.0 && u < 1.0) || rows < 0 || (rows > 0 && (!src || !dst)) || K > 0x7fffffffLL ||
      (lse_mode != 0 && lse_mode != 2) || (lse_mode == 2 && (!lse || n_partials <= 0)) || ((tile_S == nullptr) != (tile_E == nullptr)))
    return gjx_fail(GJX_EINVAL, "gjx_resample_gather_tiled: bad argument");
  const int64_t nt = (K + kTileQ - 1) / kTileQ;
  if (nt > kGatherTiledMaxTiles) return gjx_fail(GJX_EUNSUPPORTED, "gjx_resample_gather_tiled: more than 65536 tiles (K > 2^26): use gjx_resample_indices_tiled + gjx_gather_rows");
  if (!workspace || workspace_bytes < gjx_workspace_bytes(GJX_OP_RESAMPLE, K) || kWsHeaderBytes + 12 * (size_t)nt > workspace_bytes)
    return gjx_fail(GJX_EWORKSPACE, "gjx_resample_gather_tiled: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  unsigned* ctrl = (unsigned*)workspace + 8;
  if (!tile_S) {   // the producer left no tile totals: one small launch over the log-weights
    uint64_t* S = (uint64_t*)((char*)workspace + kWsHeaderBytes);
    int32_t* E = (int32_t*)(S + nt);
    if (gate) hipLaunchKernelGGL(k_tile_totals<true>, dim3((unsigned)nt), dim3(kTileQ), 0, st, logw, K, S, E, gate);
    else hipLaunchKernelGGL(k_tile_totals<false>, dim3((unsigned)nt), dim3(kTileQ), 0, st, logw, K, S, E, (const int32_t*)nullptr);
    GJX_CHECK_LAUNCH("gjx_resample_gather_tiled/totals");
    tile_S = S; tile_E = E;
  }
  const float log_k = (float)log((double)(K_total > 0 ? K_total : K));
  unsigned long long* timeline = gjx::debug_timeline(64 * (size_t)nt);
  if (nt > 1024 || getenv("GJX_TILED_PLANNED")) {       // (the variable: tests run the planned form at small sizes)
    // many tiles: maximum exponent, shifts and prefix once (k_tiled_plan), behind the tile totals in the workspace
    uint64_t* Pg = (uint64_t*)((char*)workspace + kWsHeaderBytes + 12 * (size_t)nt + 16);
    Pg = (uint64_t*)(((uintptr_t)Pg + 15) & ~(uintptr_t)15);
    int32_t* shg = (int32_t*)(Pg + nt + 1);
    if ((char*)(shg + nt) > (char*)workspace + workspace_bytes) return gjx_fail(GJX_EWORKSPACE, "gjx_resample_gather_tiled: workspace too small");
    const int rc = gjx::launch_tiled_plan(tile_S, tile_E, (int)nt, Pg, shg, ctrl, st, gate);
    if (rc) return rc;
#define GJX_GT(GATED) hipLaunchKernelGGL((k_resample_gather_tiled<4, true, GATED>), dim3((unsigned)nt), dim3(256), 0, st, logw, K, tile_S, tile_E, \
                       (const uint64_t*)Pg, (const int32_t*)shg, (int)lse_mode, lse, (int)n_partials, lse_out, log_k, u, src, src_stride, (int)rows, \
                       dst, dst_stride, ancestors, ctrl, timeline, gate)
    if (gate) GJX_GT(true); else GJX_GT(false);
#undef GJX_GT
  } else {
    const size_t lds = 8 * (size_t)((nt + 2) & ~1) + 4 * (size_t)nt;
#define GJX_GT(GATED) hipLaunchKernelGGL((k_resample_gather_tiled<4, false, GATED>), dim3((unsigned)nt), dim3(256), lds, st, logw, K, tile_S, tile_E, \
                       (const uint64_t*)nullptr, (const int32_t*)nullptr, (int)lse_mode, lse, (int)n_partials, lse_out, log_k, u, src, src_stride, \
                       (int)rows, dst, dst_stride, ancestors, ctrl, timeline, gate)
    if (gate) GJX_GT(true); else GJX_GT(false);
#undef GJX_GT
  }
  GJX_CHECK_LAUNCH("gjx_resample_gather_tiled");
  return GJX_OK;
}

extern "C" int gjx_resample_gather_tiled(const float* logw, int64_t K, const uint64_t* tile_S, const int32_t* tile_E, int32_t lse_mode,
                                         const float* lse, int32_t n_partials, double u, const float* src, int64_t src_stride,
                                         int32_t rows, float* dst, int64_t dst_stride, int32_t* ancestors, float* lse_out,
                                         int64_t K_total, void* workspace, size_t workspace_bytes, void* stream) {
  return gjx::resample_gather_tiled_gated(logw, K, tile_S, tile_E, lse_mode, lse, n_partials, u, src, src_stride, rows, dst, dst_stride, ancestors,
                                          lse_out, K_total, workspace, workspace_bytes, stream, nullptr);
}

extern "C" int gjx_resample_indices_tiled(const float* logw, int64_t K, double u, int64_t N, int32_t* ancestors, uint64_t* cum,
                                          uint32_t* q_out, int32_t* e_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!logw || !ancestors || !cum || K <= 0 || N <= 0 || K > (int64_t)1 << 31) return gjx_fail(GJX_EINVAL, "gjx_resample_indices_tiled: bad argument");
  const int64_t nt = (K + kTileQ - 1) / kTileQ;
  // workspace: [256 B control][S u64 nt][P u64 nt + 1][E i32 nt][shift i32 nt]
  if (!workspace || workspace_bytes < gjx_workspace_bytes(GJX_OP_RESAMPLE, K) || 256 + 24 * (size_t)nt + 8 > workspace_bytes)
    return gjx_fail(GJX_EWORKSPACE, "gjx_resample_indices_tiled: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  uint64_t* S = (uint64_t*)((char*)workspace + kWsHeaderBytes);
  uint64_t* P = S + nt;
  int32_t* E = (int32_t*)(P + nt + 1);
  int32_t* sh = E + nt;
  hipLaunchKernelGGL(k_tiled_quantise, dim3((unsigned)nt), dim3(kTileQ), 0, st, logw, K, cum, S, E, q_out, e_out);
  hipLaunchKernelGGL(k_tiled_plan<false>, dim3(1), dim3(1024), 0, st, (const uint64_t*)S, (const int32_t*)E, (int)nt, P, sh, (unsigned*)workspace + 8, (const int32_t*)nullptr);
  hipLaunchKernelGGL(k_tiled_ancestors, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (const uint64_t*)P, (const int32_t*)sh,
                     (const uint64_t*)cum, (int)nt, K, u, N, ancestors);
  GJX_CHECK_LAUNCH("gjx_resample_indices_tiled");
  return GJX_OK;
}

extern "C" int gjx_resample_sorted_multinomial_tiled(const float* logw, int64_t K, uint32_t key0, uint32_t key1, int64_t N, int32_t* ancestors,
                                                     uint64_t* cum, uint32_t* q_out, int32_t* e_out, void* workspace, size_t workspace_bytes,
                                                     void* stream) {
  if (!logw || !ancestors || !cum || K <= 0 || N <= 0 || K > (int64_t)1 << 31 || N > (int64_t)1 << 31)
    return gjx_fail(GJX_EINVAL, "gjx_resample_sorted_multinomial_tiled: bad argument");
  const int64_t nt = (K + kTileQ - 1) / kTileQ;
  const int64_t nb = (N + 1 + kTileQ - 1) / kTileQ;        // tiles of SLOTS (N + 1 spacings)
  // workspace: [256 B control][S u64 nt][P u64 nt + 1][E i32 nt][shift i32 nt][SS u64 nb][SP u64 nb + 1]
  const size_t off_ss = (256 + 24 * (size_t)nt + 8 + 7) & ~(size_t)7;
  if (!workspace || workspace_bytes < gjx_workspace_bytes(GJX_OP_RESAMPLE, K) || off_ss + 16 * (size_t)nb + 8 > workspace_bytes)
    return gjx_fail(GJX_EWORKSPACE, "gjx_resample_sorted_multinomial_tiled: workspace too small (OP_RESAMPLE of K, and 288 + 24 ceil(K / 1024) + 16 ceil((N + 1) / 1024) bytes)");
  hipStream_t st = (hipStream_t)stream;
  uint64_t* S = (uint64_t*)((char*)workspace + kWsHeaderBytes);
  uint64_t* P = S + nt;
  int32_t* E = (int32_t*)(P + nt + 1);
  int32_t* sh = E + nt;
  uint64_t* SS = (uint64_t*)((char*)workspace + off_ss);
  uint64_t* SP = SS + nb;
  const key2 key{key0, key1};
  hipLaunchKernelGGL(k_tiled_quantise, dim3((unsigned)nt), dim3(kTileQ), 0, st, logw, K, cum, S, E, q_out, e_out);
  hipLaunchKernelGGL(k_tiled_plan<false>, dim3(1), dim3(1024), 0, st, (const uint64_t*)S, (const int32_t*)E, (int)nt, P, sh, (unsigned*)workspace + 8, (const int32_t*)nullptr);
  hipLaunchKernelGGL(k_spacing_totals, dim3((unsigned)nb), dim3(kTileQ), 0, st, key, N, SS);
  hipLaunchKernelGGL(k_spacing_plan, dim3(1), dim3(1024), 0, st, (const uint64_t*)SS, (int)nb, SP);
  hipLaunchKernelGGL(k_sorted_ancestors, dim3((unsigned)((N + kTileQ - 1) / kTileQ)), dim3(kTileQ), 0, st, (const uint64_t*)P, (const int32_t*)sh,
                     (const uint64_t*)cum, (int)nt, K, key, (const uint64_t*)SP, (int)nb, N, ancestors);
  GJX_CHECK_LAUNCH("gjx_resample_sorted_multinomial_tiled");
  return GJX_OK;
}

extern "C" int gjx_resample_gather_systematic(const uint64_t* cum, int64_t K, const uint64_t* base_total_dev, double u,
                                              int64_t N_total, int64_t out_begin, int64_t n_out, const float* src,
                                              int64_t src_stride, int32_t rows, float* dst, int64_t dst_stride,
                                              int32_t* ancestors, void* stream) {
  if (!cum || !base_total_dev || !src || !dst || !ancestors || K <= 0 || N_total <= 0 || n_out < 0 || rows < 0 ||
      !(u >= 0.0 && u < 1.0))
    return gjx_fail(GJX_EINVAL, "gjx_resample_gather_systematic: bad argument");
  if (n_out == 0) return GJX_OK;
  // particle-oriented expand of the ancestor indices (no search), then the slot-oriented, fully coalesced row copy
  const int rc = gjx_resample_systematic(cum, K, base_total_dev, u, N_total, out_begin, n_out, ancestors, stream);
  if (rc) return rc;
  return gjx_gather_rows(src, src_stride, ancestors, n_out, rows, dst, dst_stride, stream);
}

extern "C" int gjx_resample_multinomial(const uint64_t* cum, int64_t K, const uint64_t* base_total_dev,
                                        uint32_t key0, uint32_t key1, int64_t N_total, int64_t out_begin,
                                        int64_t n_out, int32_t* ancestors, void* stream) {
  (void)N_total;
  if (!cum || !base_total_dev || !ancestors || K <= 0 || n_out < 0) return gjx_fail(GJX_EINVAL, "gjx_resample_multinomial: bad argument");
  if (n_out == 0) return GJX_OK;
  hipLaunchKernelGGL(k_multinomial, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cum, K,
                     base_total_dev, key2{key0, key1}, out_begin, n_out, ancestors);
  GJX_CHECK_LAUNCH("gjx_resample_multinomial");
  return GJX_OK;
}

extern "C" int gjx_gather_rows(const float* src, int64_t src_stride, const int32_t* anc, int64_t n_out, int32_t rows,
                               float* dst, int64_t dst_stride, void* stream) {
  if (!src || !anc || !dst || n_out < 0 || rows < 0) return gjx_fail(GJX_EINVAL, "gjx_gather_rows: bad argument");
  if (n_out == 0 || rows == 0) return GJX_OK;
  hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src,
                     src_stride, anc, n_out, (int)rows, dst, dst_stride);
  GJX_CHECK_LAUNCH("gjx_gather_rows");
  return GJX_OK;
}


extern "C" int gjx_ess(const float* logw, int64_t K, float* out4, void* workspace, size_t workspace_bytes, void* stream) {
  if (!logw || !out4 || K <= 0 || K > (int64_t)1 << 31) return gjx_fail(GJX_EINVAL, "gjx_ess: bad argument");
  const int64_t nt = (K + kTileQ - 1) / kTileQ;
  EssArgs a;
  memset(&a, 0, sizeof(a));
  if (workspace_bytes < gjx_workspace_bytes(GJX_OP_RESAMPLE, K) || ess_workspace(workspace, workspace_bytes, nt, a))
    return gjx_fail(GJX_EWORKSPACE, "gjx_ess: workspace too small");
  a.W = const_cast<float*>(logw); a.K = K; a.out4 = out4;
  hipLaunchKernelGGL(k_ess_tiles<false>, dim3((unsigned)nt), dim3(256), 0, (hipStream_t)stream, a);
  GJX_CHECK_LAUNCH("gjx_ess");
  return GJX_OK;
}
