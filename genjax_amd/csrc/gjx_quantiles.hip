// gjx_quantiles.hip — weighted quantiles (gjx_weighted_quantiles) and histograms (gjx_weighted_histogram) of SoA rows under
// self-normalised log-weights.  No sort: a most-significant-digit radix SELECT on the order-preserving 32-bit keys of the values,
// 8 bits per pass, four passes; each pass reads the row and the weights once and writes no particle-sized temporary.
//
// Weights are integers: u_i = (uint64) rint(fast_exp(logw_i - M) 2^32), M the segment's maximum.  Every accumulation below is an integer
// addition (LDS and global 64-bit atomics), so the order in which the hardware serves the atomics cannot change a bit of the result.
//
// Launches of a quantile call (plain launches on the stream, nothing read back, no block waits for another):
//   memset of the counters; k_q_max: the segment maxima (integer atomic max on the ordered key of the float);
//   per pass p = 0..3:  k_q_bins<false>: a block takes a chunk of 1..8 tiles of 1024 particles of one (segment, row) and adds u_i into
//       an LDS histogram of digit p of the key, one 256-bin histogram per DISTINCT prefix among the levels (pass 0: one), then adds
//       its non-zero bins to the global histogram;
//     k_q_select: one block per (segment, row), one wave per level: scans the level's histogram for the digit in which the running
//       sum first reaches the level's remaining target, records prefix and remaining target, groups equal prefixes, and zeroes the
//       histogram for the next pass.  After the last pass the prefix is the key: unmapped and written.
// A histogram call is the same k_q_bins with the bin of the value in place of the digit (k_q_bins<true>), and k_q_normalise.
//
// Equal digits (a flip row: every lane of a wave on one of two bins) are combined inside the wave before the LDS add: up to two
// rounds of "the first active lane's bin, summed over the lanes that share it, one add by that lane"; what is left adds on its own.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "gjx_device.h"
#include "gjx_host.h"

namespace gjx {

constexpr int kQTile = 1024;                          // particles per tile: 256 lanes x 4
constexpr int kQMaxTiles = 8;                         // tiles per block at most
constexpr int kQBits = 8, kQDigits = 1 << kQBits, kQPasses = 32 / kQBits;
constexpr int kQLevels = GJX_QUANTILES_MAX_LEVELS;
constexpr int kQLdsBins = kQLevels * kQDigits > GJX_HISTOGRAM_MAX_BINS + 2 ? kQLevels * kQDigits : GJX_HISTOGRAM_MAX_BINS + 2;
constexpr uint32_t kKeyNaN = 0xFFC00000u;             // every NaN of a live particle: above +inf (0xFF800000); unmaps to the quiet NaN

typedef unsigned long long u64;

// what the select of a pass leaves for the next pass, per (segment, row)
struct QState {
  int32_t n_groups;                // distinct prefixes among the levels (0: a segment without weight)
  int32_t level_group[kQLevels];   // the histogram a level reads
  uint32_t group_prefix[kQLevels]; // the digits chosen so far, right-aligned
  u64 target[kQLevels];            // what the running sum inside the level's prefix has to reach
};

struct QArgs {
  const float* rows;
  int64_t row_stride;
  int n_rows;
  const float* logw;       // or NULL: equal weights
  int64_t K_seg;           // particles per segment
  int64_t n_segments;
  int tiles_per_block;     // 1 .. kQMaxTiles
  int nc_seg;              // blocks (chunks) per segment and row
  int64_t n_chunks;        // n_segments * nc_seg
  uint32_t* segmax;        // u32[S]: ordered key of the segment's maximum log-weight (0: none yet)
  u64* sumsq;              // u64[S]: sum of rint(e^2 2^32)
  u64* hist;               // u64[S][n_rows][bins_per_row]
  QState* state;           // [S][n_rows]
  int bins_per_row;        // quantiles: n_levels * 256; histogram: n_bins + 2
  int pass;
  int n_levels;
  float levels[kQLevels];
  float lo, hi, scale;     // histogram
  int n_bins;
  float* stats;
  float* out;              // quantiles f32[S][n_rows][n_levels], or mass f32[S][n_rows][n_bins + 2]
};

// the usual order-preserving map of the float bits, and back
GJX_DEV uint32_t ordered_key(uint32_t bits) { return bits ^ ((bits & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u); }
GJX_DEV uint32_t ordered_bits(uint32_t key) { return key ^ ((key & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu); }
// key of a row value: -0.0 folded onto +0.0, every NaN onto kKeyNaN; bits are compared, so denormals keep their order
GJX_DEV uint32_t value_key(float x) {
  const uint32_t b = __float_as_uint(x);
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return kKeyNaN;
  return ordered_key(b == 0x80000000u ? 0u : b);
}

// rint(e 2^32) for 0 <= e <= 1: one 32-bit conversion below 1 (e 2^32 <= 2^32 - 256 there), 2^32 at 1
GJX_DEV u64 weight_u(float e) { return e >= 1.0f ? (u64)1 << 32 : (u64)(uint32_t)rintf(e * 4294967296.0f); }

// the lane's four consecutive values, nv of them inside the chunk: one 16-byte load where the address allows
GJX_DEV void q_load4(const float* p, int nv, float fill, float (&x)[4]) {
  if (nv == 4 && ((uintptr_t)p & 15) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = k < nv ? p[k] : fill;
  }
}

template <unsigned CTRL, unsigned ROW_MASK>
GJX_DEV uint32_t dpp_add_u32(uint32_t v) { return v + dpp_mov<CTRL, ROW_MASK>(0u, v); }
GJX_DEV uint32_t wave_sum_u32(uint32_t v) {   // sum over the wave, in every lane
  v = dpp_add_u32<kDppShr1, 0xf>(v);
  v = dpp_add_u32<kDppShr2, 0xf>(v);
  v = dpp_add_u32<kDppShr4, 0xf>(v);
  v = dpp_add_u32<kDppShr8, 0xf>(v);
  v = dpp_add_u32<kDppBcast15, 0xa>(v);
  v = dpp_add_u32<kDppBcast31, 0xc>(v);
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
GJX_DEV u64 wave_sum_u64(u64 v) {             // any 64-bit values: butterfly through the cross-lane network
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

// h[idx] += u for the active lanes (u <= 2^32); called by whole waves.  Lanes that share the first active lane's bin are summed in
// the wave (u in two pieces of 20 and 13 bits: 64 of either fit 32 bits) and added once; two rounds, each only where at least 8
// lanes share the bin — a continuous row pays two ballots, a flip row adds twice per wave instead of 64 times on two addresses.
GJX_DEV void hist_add(u64* h, int idx, u64 u, bool active) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const u64 act = __ballot(active);
    if (act == 0) return;
    const int first = __ffsll((long long)act) - 1;
    const int i0 = __builtin_amdgcn_readlane(idx, first);
    const bool same = active && idx == i0;
    if (__popcll(__ballot(same)) < 8) break;
    const uint32_t lo = wave_sum_u32(same ? (uint32_t)u & 0xFFFFFu : 0u);
    const uint32_t hi = wave_sum_u32(same ? (uint32_t)(u >> 20) : 0u);
    if (lane == first) atomicAdd(&h[i0], ((u64)hi << 20) + lo);
    active = active && !same;
  }
  if (active) atomicAdd(&h[idx], u);
}

// the segment maxima: atomic max on the ordered key (an integer: no order of arrival to depend on); fmaxf drops a NaN
__global__ __launch_bounds__(256) void k_q_max(const QArgs a) {
  __shared__ float lds[4];
  const int64_t seg = blockIdx.x / a.nc_seg;
  const int64_t c = blockIdx.x - seg * a.nc_seg;
  const int64_t p0 = c * a.tiles_per_block * kQTile;
  float m = -INFINITY;
  for (int t = 0; t < a.tiles_per_block; ++t) {
    const int64_t i0 = p0 + (int64_t)t * kQTile + threadIdx.x * 4;
    const int64_t left = a.K_seg - i0;
    const int nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    if (nv == 0) continue;
    float w[4];
    q_load4(a.logw + seg * a.K_seg + i0, nv, -INFINITY, w);
    m = fmaxf(m, fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3])));
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
    const uint32_t key = ordered_key(__float_as_uint(m));
    if (key > a.segmax[seg]) atomicMax(&a.segmax[seg], key);          // (the word only grows: a stale read costs an atomic, no more)
  }
}

// the segment's maximum log-weight as k_q_max left it (key 0: nothing live)
GJX_DEV float segment_max(const QArgs& a, int64_t seg) {
  if (!a.logw) return 0.0f;
  const uint32_t k = a.segmax[seg];
  return k ? __uint_as_float(ordered_bits(k)) : -INFINITY;
}

// HIST: the bin of the value (0: below lo; 1 + b; n_bins + 1: at or above hi, b >= n_bins, NaN), computed unfused
GJX_DEV int value_bin(const QArgs& a, float x) {
  if (x < a.lo) return 0;
  if (!(x < a.hi)) return a.n_bins + 1;
  const float b = floorf(__fmul_rn(__fsub_rn(x, a.lo), a.scale));
  return b < (float)a.n_bins ? 1 + (int)b : a.n_bins + 1;
}

template <bool HIST>
__global__ __launch_bounds__(256) void k_q_bins(const QArgs a) {
  __shared__ u64 h[kQLdsBins];
  __shared__ uint32_t prefix[kQLevels];
  __shared__ u64 sq[4];
  const int64_t chunk = blockIdx.x % a.n_chunks;
  const int row = (int)(blockIdx.x / a.n_chunks);
  const int64_t seg = chunk / a.nc_seg;
  const int64_t c = chunk - seg * a.nc_seg;
  const int64_t sr = seg * a.n_rows + row;
  int G = 1;                                               // histograms of this block
  if (!HIST && a.pass > 0) {
    const QState* s = a.state + sr;
    G = s->n_groups;
    if (G == 0) return;                                    // a segment without weight (block-uniform)
    if (threadIdx.x < G) prefix[threadIdx.x] = s->group_prefix[threadIdx.x];
  }
  const int nb = HIST ? a.n_bins + 2 : G * kQDigits;
  for (int i = threadIdx.x; i < nb; i += 256) h[i] = 0;
  __syncthreads();
  const float M = segment_max(a, seg);
  const int hi_shift = 32 - kQBits * a.pass, lo_shift = hi_shift - kQBits;     // (pass 0: no prefix to match)
  const bool want_sq = row == 0 && (HIST || a.pass == 0);
  u64 q = 0;
  const int64_t p0 = c * a.tiles_per_block * kQTile;
  const float* xrow = a.rows + (int64_t)row * a.row_stride + seg * a.K_seg;
  for (int t = 0; t < a.tiles_per_block; ++t) {
    const int64_t i0 = p0 + (int64_t)t * kQTile + threadIdx.x * 4;
    if (p0 + (int64_t)t * kQTile >= a.K_seg) break;        // block-uniform
    const int64_t left = a.K_seg - i0;
    const int nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    float w[4], x[4];
    if (a.logw && nv > 0) {
      q_load4(a.logw + seg * a.K_seg + i0, nv, -INFINITY, w);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = k < nv ? 0.0f : -INFINITY;
    }
    if (nv > 0) {
      q_load4(xrow + i0, nv, 0.0f, x);
    } else {
      x[0] = x[1] = x[2] = x[3] = 0.0f;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float e = M > -INFINITY ? fast_exp(w[k] - M) : 0.0f;
      const u64 u = e > 0.0f ? weight_u(e) : 0;                             // (a NaN weight: dead)
      bool active = u != 0;
      int idx = 0;
      if (HIST) {
        idx = value_bin(a, x[k]);
      } else {
        const uint32_t key = value_key(x[k]);
        idx = (int)((key >> lo_shift) & (kQDigits - 1));
        if (a.pass > 0) {
          const uint32_t top = key >> hi_shift;
          int g = -1;
          for (int j = 0; j < G; ++j) g = prefix[j] == top ? j : g;
          active = active && g >= 0;
          idx += (g < 0 ? 0 : g) * kQDigits;
        }
      }
      hist_add(h, idx, u, active);
      if (want_sq && u != 0) q += weight_u(e * e);
    }
  }
  if (want_sq) {                                           // block-uniform
    q = wave_sum_u64(q);
    if ((threadIdx.x & 63) == 0) sq[threadIdx.x >> 6] = q;
  }
  __syncthreads();
  if (want_sq && threadIdx.x == 0) {
    q = sq[0] + sq[1] + sq[2] + sq[3];
    if (q) atomicAdd(&a.sumsq[seg], q);
  }
  u64* gh = a.hist + sr * a.bins_per_row;
  for (int i = threadIdx.x; i < nb; i += 256) {
    const u64 v = h[i];
    if (v) atomicAdd(&gh[i], v);
  }
}

// {max, sum e, sum e^2, ESS} from the integers: sum e = U / 2^32, sum e^2 = Q / 2^32
GJX_DEV void write_stats(const QArgs& a, int64_t seg, u64 U) {
  float* st = a.stats + 4 * seg;
  const u64 Q = a.sumsq[seg];
  if (U == 0 || Q == 0) {
    st[0] = -INFINITY; st[1] = 0.0f; st[2] = 0.0f; st[3] = 0.0f;
    return;
  }
  const double s1 = (double)U * (1.0 / 4294967296.0), s2 = (double)Q * (1.0 / 4294967296.0);
  st[0] = segment_max(a, seg);
  st[1] = (float)s1;
  st[2] = (float)s2;
  st[3] = (float)(s1 * s1 / s2);
}

// One block per (segment, row), wave l for level l.  Lane j holds bins 4j .. 4j + 3 of the level's histogram.
__global__ void k_q_select(const QArgs a) {
  __shared__ uint32_t new_prefix[kQLevels];
  __shared__ u64 new_target[kQLevels];
  const int64_t sr = blockIdx.x;
  const int64_t seg = sr / a.n_rows;
  const int row = (int)(sr - seg * a.n_rows);
  const int l = threadIdx.x >> 6, lane = threadIdx.x & 63;
  QState* s = a.state + sr;
  u64* gh = a.hist + sr * a.bins_per_row;
  const int G_old = a.pass == 0 ? 1 : s->n_groups;
  const bool last = a.pass == kQPasses - 1;
  bool dead = G_old == 0;
  if (!dead) {
    const int g = a.pass == 0 ? 0 : s->level_group[l];
    const uint32_t pre = a.pass == 0 ? 0u : s->group_prefix[g];
    const u64* hg = gh + g * kQDigits;
    u64 b[4], incl = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { b[k] = hg[4 * lane + k]; incl += b[k]; }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {                     // inclusive scan over the lanes
      const u64 o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    const u64 total = __shfl(incl, 63, 64);
    u64 t;
    if (a.pass == 0) {
      // the level's target in double: max(1, ceil(q U)), and never above U
      const double tq = ceil((double)a.levels[l] * (double)total);
      t = tq >= 18446744073709551615.0 ? total : (u64)tq;
      t = t < 1 ? 1 : (t > total ? total : t);
      if (row == 0 && threadIdx.x == 0) write_stats(a, seg, total);
    } else {
      t = s->target[l];
    }
    dead = total == 0;
    if (!dead) {
      const u64 hit = __ballot(incl >= t);
      const int j = hit ? __ffsll((long long)hit) - 1 : 63;
      if (lane == j) {
        u64 before = incl - (b[0] + b[1] + b[2] + b[3]);
        int k = 0;
        while (k < 3 && before + b[k] < t) { before += b[k]; ++k; }
        new_prefix[l] = (pre << kQBits) | (uint32_t)(4 * j + k);
        new_target[l] = t - before;
      }
    }
  } else if (a.pass == 0 && row == 0 && threadIdx.x == 0) {
    write_stats(a, seg, 0);
  }
  __syncthreads();                                         // every read of the old state is done
  if (last) {
    if (lane == 0) a.out[sr * a.n_levels + l] = dead ? NAN : __uint_as_float(ordered_bits(new_prefix[l]));
    return;
  }
  if (threadIdx.x == 0) {                                  // levels with one prefix share a histogram from here on
    int G = 0;
    if (!dead) {
      for (int i = 0; i < a.n_levels; ++i) {
        int g = -1;
        for (int j = 0; j < G; ++j) g = s->group_prefix[j] == new_prefix[i] ? j : g;
        if (g < 0) { g = G++; s->group_prefix[g] = new_prefix[i]; }
        s->level_group[i] = g;
        s->target[i] = new_target[i];
      }
    }
    s->n_groups = G;
  }
  for (int i = threadIdx.x; i < G_old * kQDigits; i += blockDim.x) gh[i] = 0;     // read and done: clean for the next pass
}

// mass = (double) bin / (double) U rounded to float, one block per (segment, row); U is the sum of the row's bins
__global__ __launch_bounds__(256) void k_q_normalise(const QArgs a) {
  __shared__ u64 part[4];
  const int64_t sr = blockIdx.x;
  const int64_t seg = sr / a.n_rows;
  const int row = (int)(sr - seg * a.n_rows);
  const u64* gh = a.hist + sr * a.bins_per_row;
  u64 s = 0;
  for (int i = threadIdx.x; i < a.bins_per_row; i += 256) s += gh[i];
  s = wave_sum_u64(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  const u64 U = part[0] + part[1] + part[2] + part[3];
  if (row == 0 && threadIdx.x == 0) write_stats(a, seg, U);
  float* mass = a.out + sr * a.bins_per_row;
  for (int i = threadIdx.x; i < a.bins_per_row; i += 256) mass[i] = U ? (float)((double)gh[i] / (double)U) : NAN;
}

// the shape both calls share; false: refused
static bool q_shape(int32_t n_rows, int64_t K, int64_t n_segments, int64_t bins_per_row, QArgs* a) {
  if (n_rows <= 0 || K <= 0 || n_segments <= 0 || K % n_segments != 0 || bins_per_row <= 0) return false;
  const int64_t K_seg = K / n_segments;
  if (K_seg > INT32_MAX || n_segments > INT32_MAX / n_rows) return false;      // U = sum u < 2^63; grid sizes
  const int64_t nt_seg = (K_seg + kQTile - 1) / kQTile;
  // enough blocks to fill the device, few enough that a block's LDS histogram is worth its zeroing and its flush, and at most
  // about 128 per (segment, row): their flushes are atomics on the same few words
  int64_t tpb = nt_seg * n_segments * n_rows / 2048;
  if (tpb < (nt_seg + 127) / 128) tpb = (nt_seg + 127) / 128;
  tpb = tpb < 1 ? 1 : (tpb > kQMaxTiles ? kQMaxTiles : tpb);
  const int64_t nc_seg = (nt_seg + tpb - 1) / tpb;
  if (nc_seg * n_segments > INT32_MAX / n_rows || n_segments * n_rows > INT64_MAX / 32 / bins_per_row) return false;     // grid; bytes
  a->n_rows = n_rows; a->K_seg = K_seg; a->n_segments = n_segments; a->tiles_per_block = (int)tpb; a->nc_seg = (int)nc_seg;
  a->n_chunks = nc_seg * n_segments; a->bins_per_row = (int)bins_per_row;
  return true;
}

// workspace: [segmax u32[S] (padded to 8)] [sumsq u64[S]] [hist] [state]; the first three are zeroed by the call
static size_t q_layout(QArgs* a, void* workspace, bool with_state, size_t* zero_bytes) {
  const size_t S = (size_t)a->n_segments, SR = S * (size_t)a->n_rows;
  const size_t o_sumsq = (S * 4 + 7) & ~(size_t)7, o_hist = o_sumsq + 8 * S, o_state = o_hist + 8 * SR * (size_t)a->bins_per_row;
  if (workspace) {
    char* base = (char*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
    a->segmax = (uint32_t*)base;
    a->sumsq = (u64*)(base + o_sumsq);
    a->hist = (u64*)(base + o_hist);
    a->state = (QState*)(base + o_state);
  }
  *zero_bytes = o_state;
  return 8 + o_state + (with_state ? SR * sizeof(QState) : 0);          // (8: the alignment of any pointer)
}

static int q_head(QArgs& a, size_t zero_bytes, hipStream_t st, const char* where) {
  hipError_t e = hipMemsetAsync(a.segmax, 0, zero_bytes, st);
  if (e != hipSuccess) return gjx_fail_hip(e, where);
  if (a.logw) {
    hipLaunchKernelGGL(k_q_max, dim3((unsigned)a.n_chunks), dim3(256), 0, st, a);
    GJX_CHECK_LAUNCH(where);
  }
  return GJX_OK;
}

}  // namespace gjx

extern "C" size_t gjx_weighted_quantiles_workspace_bytes(int32_t n_rows, int64_t K, int64_t n_segments, int32_t n_levels) {
  gjx::QArgs a;
  size_t zero;
  if (n_levels <= 0 || n_levels > GJX_QUANTILES_MAX_LEVELS || !gjx::q_shape(n_rows, K, n_segments, (int64_t)n_levels * gjx::kQDigits, &a)) return 0;
  return gjx::q_layout(&a, nullptr, true, &zero);
}

extern "C" int gjx_weighted_quantiles(const float* rows, int64_t row_stride, int32_t n_rows, const float* logw, int64_t K,
                                      int64_t n_segments, const float* levels, int32_t n_levels, float* stats, float* out,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  QArgs a;
  memset(&a, 0, sizeof(a));
  const int32_t nl = n_levels > kQLevels ? kQLevels : n_levels;          // the shape of a call over the cap is still checked
  if (!rows || !stats || !out || !workspace || !levels || row_stride < K || n_levels <= 0 ||
      !q_shape(n_rows, K, n_segments, (int64_t)nl * kQDigits, &a))
    return gjx_fail(GJX_EINVAL, "gjx_weighted_quantiles: bad argument");
  for (int32_t i = 0; i < n_levels; ++i)
    if (!(levels[i] >= 0.0f && levels[i] <= 1.0f)) return gjx_fail(GJX_EINVAL, "gjx_weighted_quantiles: a level outside [0, 1]");
  if (n_levels > kQLevels) {
    char msg[160];
    snprintf(msg, sizeof(msg), "gjx_weighted_quantiles: a call takes at most GJX_QUANTILES_MAX_LEVELS = %d levels, not %d", kQLevels, (int)n_levels);
    return gjx_fail(GJX_EUNSUPPORTED, msg);
  }
  size_t zero;
  if (workspace_bytes < q_layout(&a, workspace, true, &zero)) return gjx_fail(GJX_EWORKSPACE, "gjx_weighted_quantiles: workspace too small");
  a.rows = rows; a.row_stride = row_stride; a.logw = logw; a.n_levels = n_levels; a.stats = stats; a.out = out;
  for (int32_t i = 0; i < n_levels; ++i) a.levels[i] = levels[i];
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = q_head(a, zero, st, "gjx_weighted_quantiles(max)")) return rc;
  const dim3 bins_grid((unsigned)(a.n_chunks * n_rows)), sel_grid((unsigned)(n_segments * n_rows));
  for (a.pass = 0; a.pass < kQPasses; ++a.pass) {
    hipLaunchKernelGGL(k_q_bins<false>, bins_grid, dim3(256), 0, st, a);
    GJX_CHECK_LAUNCH("gjx_weighted_quantiles(bins)");
    hipLaunchKernelGGL(k_q_select, sel_grid, dim3(64 * n_levels), 0, st, a);
    GJX_CHECK_LAUNCH("gjx_weighted_quantiles(select)");
  }
  return GJX_OK;
}

extern "C" size_t gjx_weighted_histogram_workspace_bytes(int32_t n_rows, int64_t K, int64_t n_segments, int32_t n_bins) {
  gjx::QArgs a;
  size_t zero;
  if (n_bins <= 0 || n_bins > GJX_HISTOGRAM_MAX_BINS || !gjx::q_shape(n_rows, K, n_segments, (int64_t)n_bins + 2, &a)) return 0;
  return gjx::q_layout(&a, nullptr, false, &zero);
}

extern "C" int gjx_weighted_histogram(const float* rows, int64_t row_stride, int32_t n_rows, const float* logw, int64_t K,
                                      int64_t n_segments, float lo, float hi, int32_t n_bins, float* stats, float* mass,
                                      void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  QArgs a;
  memset(&a, 0, sizeof(a));
  const int32_t nb = n_bins > GJX_HISTOGRAM_MAX_BINS ? GJX_HISTOGRAM_MAX_BINS : n_bins;
  if (!rows || !stats || !mass || !workspace || row_stride < K || n_bins <= 0 || !(lo < hi) || !isfinite(lo) || !isfinite(hi) ||
      !q_shape(n_rows, K, n_segments, (int64_t)nb + 2, &a))
    return gjx_fail(GJX_EINVAL, "gjx_weighted_histogram: bad argument");
  if (n_bins > GJX_HISTOGRAM_MAX_BINS) {
    char msg[160];
    snprintf(msg, sizeof(msg), "gjx_weighted_histogram: a call takes at most GJX_HISTOGRAM_MAX_BINS = %d bins, not %d", GJX_HISTOGRAM_MAX_BINS, (int)n_bins);
    return gjx_fail(GJX_EUNSUPPORTED, msg);
  }
  size_t zero;
  if (workspace_bytes < q_layout(&a, workspace, false, &zero)) return gjx_fail(GJX_EWORKSPACE, "gjx_weighted_histogram: workspace too small");
  a.rows = rows; a.row_stride = row_stride; a.logw = logw; a.stats = stats; a.out = mass;
  a.lo = lo; a.hi = hi; a.n_bins = n_bins;
  a.scale = (float)n_bins / (hi - lo);                                     // float32, once, here
  const hipStream_t st = (hipStream_t)stream;
  if (int rc = q_head(a, zero, st, "gjx_weighted_histogram(max)")) return rc;
  hipLaunchKernelGGL(k_q_bins<true>, dim3((unsigned)(a.n_chunks * n_rows)), dim3(256), 0, st, a);
  GJX_CHECK_LAUNCH("gjx_weighted_histogram(bins)");
  hipLaunchKernelGGL(k_q_normalise, dim3((unsigned)(n_segments * n_rows)), dim3(256), 0, st, a);
  GJX_CHECK_LAUNCH("gjx_weighted_histogram(normalise)");
  return GJX_OK;
}
