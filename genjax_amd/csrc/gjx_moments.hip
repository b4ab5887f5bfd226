// gjx_moments.hip — weighted posterior moments of a particle collection (gjx_weighted_moments): means, and variances or a
// covariance matrix, of SoA rows under self-normalised log-weights.  Memory-bound: the weights and every row are read once.
//
// Launch 1, one block per 1024-particle tile (256 lanes x 4 particles; tiles are numbered per segment, so a tile never straddles
// two segments): e_i = exp(logw_i - tile max) once, then for the rows of the call, a batch at a time in registers,
//   rough mean  c_r  = sum e x_r / W_b                      (W_b = sum e)
//   centred     u_r  = sum e (x_r - c_r),  v_rs = sum e (x_r - c_r)(x_s - c_s)
//   mean_b,r = c_r + u_r / W_b,   M2_b,rs = v_rs - u_r u_s / W_b
// (the second pass costs no memory traffic and takes the rounding of the first sum out of the mean: the error of mean_b is relative
// to the spread of the row, not to its magnitude).  A dead particle (weight -inf or NaN: e = 0) is selected out, never multiplied
// by zero.  The block publishes {m_b, W_b, sum e^2, mean_b, M2_b} with plain stores.
// Launch 2, one block per (segment, row): M = max m_b, f_b = exp(m_b - M), and the pairwise update of Chan, Golub and LeVeque in the
// same two-pass form over the tiles: lane l takes tiles [l per, (l + 1) per) in order, then the fixed-order wave sum and the four
// waves in order — a function of the data and of K / n_segments alone.  No atomics, no block waits for another.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "gjx_device.h"
#include "gjx_host.h"

namespace gjx {

constexpr int kMomTile = 1024;                       // particles per tile
constexpr int kMomBatch = 8;                         // rows a block holds in registers at a time (means, variances)
constexpr int kCovMax = GJX_MOMENTS_MAX_COV_ROWS;    // the covariance kernel holds every row of the call in registers

struct MomArgs {
  const float* rows;
  int64_t row_stride;
  int n_rows;
  const float* logw;       // or NULL: equal weights
  int64_t K_seg;           // particles per segment
  int nt_seg;              // tiles per segment
  int64_t n_tiles;         // n_segments * nt_seg
  float* part;             // per-tile partials, field-major f32[3 + n_rows + n_second][n_tiles]: m, W, sum e^2, mean[r], M2[...]
  int want;
  float* stats;
  float* mean;
  float* second;
};

// upper-triangle index of the pair (r, s >= r) of n rows
GJX_DEV int pair_index(int r, int s, int n) { return r * n - ((r * (r - 1)) >> 1) + (s - r); }

// Sums over the 256 lanes of a block of v[j0 .. N), in every lane: the fixed-order wave sum, then the four waves in order.
// lds: 4 N floats.
template <int N>
GJX_DEV void block_sum(float (&v)[N], float* lds, int j0 = 0) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    if (j < j0) continue;
    const float s = wave_sum(v[j]);
    if (lane == 0) lds[wid * N + j] = s;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j)
    if (j >= j0) v[j] = (lds[j] + lds[N + j]) + (lds[2 * N + j] + lds[3 * N + j]);
  __syncthreads();
}

GJX_DEV float block_max(float v, float* lds) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  v = wave_max(v);
  if (lane == 0) lds[wid] = v;
  __syncthreads();
  v = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
  __syncthreads();
  return v;
}

// the lane's four consecutive values, nv of them inside the segment: one 16-byte load where the address allows
GJX_DEV void load4(const float* p, int nv, float fill, float (&x)[4]) {
  if (nv == 4 && ((uintptr_t)p & 15) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    x[0] = q.x; x[1] = q.y; x[2] = q.z; x[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = k < nv ? p[k] : fill;
  }
}

struct TileHead {
  int64_t tile, base;      // global tile number; index of the lane's first particle in logw and in every row
  int nv;                  // how many of the lane's four particles are inside the segment
  float e[4];              // exp(logw - tile max); 0: dead or outside
  float m, W, rW;          // tile max (-inf: dead tile), sum e, 1 / W (0: dead tile)
};

// the lane's place in its tile: global tile number, first particle, how many of its four are inside the segment
GJX_DEV void tile_lane(const MomArgs& a, TileHead& h) {
  h.tile = blockIdx.x;
  const int64_t seg = h.tile / a.nt_seg;
  const int64_t t = h.tile - seg * a.nt_seg;
  const int64_t i0 = (t * 256 + threadIdx.x) * 4;
  const int64_t left = a.K_seg - i0;
  h.nv = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
  h.base = seg * a.K_seg + i0;
}

// weights of the tile, and its {m, W, sum e^2} published (fields 0, 1, 2 of the partials).  MASKED (gjx_weighted_cross_moments): bit k
// of `kill` makes the lane's particle k dead before the tile's maximum and sums are taken; returns how many of those had a weight.
template <bool MASKED>
GJX_DEV int tile_head_t(const MomArgs& a, float* lds, TileHead& h, uint32_t kill) {
  tile_lane(a, h);
  float w[4];
  if (a.logw) {
    load4(a.logw + h.base, h.nv, -INFINITY, w);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = k < h.nv ? 0.0f : -INFINITY;
  }
  int killed = 0;
  if constexpr (MASKED) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if ((kill >> k) & 1u) {
        killed += w[k] > -INFINITY;                                                 // (a NaN weight was dead already)
        w[k] = -INFINITY;
      }
    }
  }
  const float bm = block_max(fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3])), lds);    // (fmaxf drops a NaN)
  float s[2] = {0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float e = bm > -INFINITY ? fast_exp(w[k] - bm) : 0.0f;
    h.e[k] = e > 0.0f ? e : 0.0f;                                                   // (a NaN weight: dead)
    s[0] += h.e[k];
    s[1] = fmaf(h.e[k], h.e[k], s[1]);
  }
  block_sum<2>(s, lds);
  h.W = s[0];
  h.m = h.W > 0.0f ? bm : -INFINITY;
  h.rW = h.W > 0.0f ? 1.0f / h.W : 0.0f;
  if (threadIdx.x == 0) {
    a.part[h.tile] = h.m;
    a.part[a.n_tiles + h.tile] = h.W;
    a.part[2 * a.n_tiles + h.tile] = s[1];
  }
  return killed;
}

GJX_DEV void tile_head(const MomArgs& a, float* lds, TileHead& h) { tile_head_t<false>(a, lds, h, 0u); }

// means and variances: kMomBatch rows at a time
__global__ __launch_bounds__(256) void k_moments_tiles(const MomArgs a) {
  __shared__ float lds[4 * 2 * kMomBatch];
  TileHead h;
  tile_head(a, lds, h);
  for (int r0 = 0; r0 < a.n_rows; r0 += kMomBatch) {
    float x[kMomBatch][4];
#pragma unroll
    for (int j = 0; j < kMomBatch; ++j) {
      if (r0 + j < a.n_rows) {
        load4(a.rows + (int64_t)(r0 + j) * a.row_stride + h.base, h.nv, 0.0f, x[j]);
      } else {
        x[j][0] = x[j][1] = x[j][2] = x[j][3] = 0.0f;
      }
    }
    float s[kMomBatch];
#pragma unroll
    for (int j = 0; j < kMomBatch; ++j) {
      s[j] = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        x[j][k] = h.e[k] > 0.0f ? x[j][k] : 0.0f;         // selected on the weight: a dead particle's NaN or inf never enters
        s[j] = fmaf(h.e[k], x[j][k], s[j]);
      }
    }
    block_sum<kMomBatch>(s, lds);
    float uv[2 * kMomBatch];
#pragma unroll
    for (int j = 0; j < kMomBatch; ++j) {
      s[j] *= h.rW;                                        // the rough mean
      float u = 0.0f, v = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float d = h.e[k] > 0.0f ? x[j][k] - s[j] : 0.0f;
        const float ed = h.e[k] * d;
        u += ed;
        v = fmaf(ed, d, v);
      }
      uv[2 * j] = u;
      uv[2 * j + 1] = v;
    }
    block_sum<2 * kMomBatch>(uv, lds);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int j = 0; j < kMomBatch; ++j) {
        if (r0 + j < a.n_rows) {
          const float u = uv[2 * j], m2 = uv[2 * j + 1] - u * u * h.rW;
          a.part[(int64_t)(3 + r0 + j) * a.n_tiles + h.tile] = s[j] + u * h.rW;
          a.part[(int64_t)(3 + a.n_rows + r0 + j) * a.n_tiles + h.tile] = m2 < 0.0f ? 0.0f : m2;
        }
      }
    }
  }
}

// row R of the upper triangle of a tile's centred products (x: centred values, u: their weighted sums), then the rows below it
template <int R>
GJX_DEV void cov_row(const MomArgs& a, const TileHead& h, const float (&x)[kCovMax][4], const float (&u)[kCovMax], float* lds) {
  const int n = a.n_rows;
  if (R < n) {                                             // block-uniform
    float p[kCovMax];
#pragma unroll
    for (int s = 0; s < kCovMax; ++s) {
      p[s] = 0.0f;
      if (s < R) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k) p[s] = fmaf(h.e[k] * x[R][k], x[s][k], p[s]);
    }
    block_sum<kCovMax>(p, lds, R);
    if (threadIdx.x == 0) {
#pragma unroll
      for (int s = 0; s < kCovMax; ++s) {
        if (s < R || s >= n) continue;
        const float m2 = p[s] - u[R] * u[s] * h.rW;
        a.part[(int64_t)(3 + n + pair_index(R, s, n)) * a.n_tiles + h.tile] = (s == R && m2 < 0.0f) ? 0.0f : m2;
      }
    }
  }
  if constexpr (R + 1 < kCovMax) cov_row<R + 1>(a, h, x, u, lds);
}

// covariance: every row of the call (n_rows <= kCovMax) in registers, the upper triangle of the centred products
__global__ __launch_bounds__(256) void k_moments_cov_tiles(const MomArgs a) {
  __shared__ float lds[4 * kCovMax];
  TileHead h;
  tile_head(a, lds, h);
  const int n = a.n_rows;
  float x[kCovMax][4];
#pragma unroll
  for (int r = 0; r < kCovMax; ++r) {
    if (r < n) {
      load4(a.rows + (int64_t)r * a.row_stride + h.base, h.nv, 0.0f, x[r]);
    } else {
      x[r][0] = x[r][1] = x[r][2] = x[r][3] = 0.0f;
    }
  }
  float c[kCovMax];
#pragma unroll
  for (int r = 0; r < kCovMax; ++r) {
    c[r] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[r][k] = h.e[k] > 0.0f ? x[r][k] : 0.0f;
      c[r] = fmaf(h.e[k], x[r][k], c[r]);
    }
  }
  block_sum<kCovMax>(c, lds);
  float u[kCovMax];
#pragma unroll
  for (int r = 0; r < kCovMax; ++r) {
    c[r] *= h.rW;
    u[r] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[r][k] = h.e[k] > 0.0f ? x[r][k] - c[r] : 0.0f;    // centred in place
      u[r] = fmaf(h.e[k], x[r][k], u[r]);
    }
  }
  block_sum<kCovMax>(u, lds);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int r = 0; r < kCovMax; ++r)
      if (r < n) a.part[(int64_t)(3 + r) * a.n_tiles + h.tile] = c[r] + u[r] * h.rW;
  }
  cov_row<0>(a, h, x, u, lds);
}

// NS == 1: block (segment, r) merges the mean and the variance of row r; NS == kCovMax: row r against the rows s = r + j >= r
template <int NS>
__global__ __launch_bounds__(256) void k_moments_merge(const MomArgs a) {
  __shared__ float lds[4 * (2 * NS + 2)];
  const int n = a.n_rows, nt = a.nt_seg;
  const int64_t seg = blockIdx.x / n;
  const int r = (int)(blockIdx.x - seg * n);
  const int ns = NS == 1 ? 1 : n - r;
  const int64_t nT = a.n_tiles;
  const float* pm = a.part + seg * nt;
  const float* pW = pm + nT;
  const float* pQ = pW + nT;
  const float* pmean = pm + 3 * nT;                        // + row * nT
  const float* psec = pmean + (int64_t)n * nT;             // + (row | pair) * nT
  float M = -INFINITY;
  for (int b = threadIdx.x; b < nt; b += 256) M = fmaxf(M, pm[b]);
  M = block_max(M, lds);
  const int per = (nt + 255) >> 8;
  const int b0 = threadIdx.x * per, b1 = b0 + per < nt ? b0 + per : nt;
  // pass 1: total weight, sum of squares, rough means
  float acc[NS + 2];
#pragma unroll
  for (int j = 0; j < NS + 2; ++j) acc[j] = 0.0f;
  for (int b = b0; b < b1; ++b) {
    const float Wb = pW[b];
    if (!(Wb > 0.0f)) continue;                            // a dead tile is skipped, not weighted by zero
    const float f = fast_exp(pm[b] - M), g = f * Wb;
    acc[0] += g;
    acc[1] = fmaf(pQ[b], f * f, acc[1]);
#pragma unroll
    for (int j = 0; j < NS; ++j)
      if (j < ns) acc[2 + j] = fmaf(g, pmean[(int64_t)(r + j) * nT + b], acc[2 + j]);
  }
  block_sum<NS + 2>(acc, lds);
  const float Wt = acc[0];
  const bool live = M > -INFINITY && Wt > 0.0f;
  const float rW = live ? 1.0f / Wt : 0.0f;
  // pass 2: centred on the rough means
  float q[2 * NS];
#pragma unroll
  for (int j = 0; j < 2 * NS; ++j) q[j] = 0.0f;
#pragma unroll
  for (int j = 0; j < NS; ++j) acc[2 + j] *= rW;
  for (int b = b0; b < b1; ++b) {
    const float Wb = pW[b];
    if (!(Wb > 0.0f)) continue;
    const float f = fast_exp(pm[b] - M), g = f * Wb;
    const float d0 = pmean[(int64_t)r * nT + b] - acc[2];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      if (j >= ns) continue;
      const float dj = pmean[(int64_t)(r + j) * nT + b] - acc[2 + j];
      const int64_t field = NS == 1 ? r : pair_index(r, r + j, n);
      q[2 * j] = fmaf(g, dj, q[2 * j]);
      q[2 * j + 1] += fmaf(g * d0, dj, f * psec[field * nT + b]);
    }
  }
  block_sum<2 * NS>(q, lds);
  if (threadIdx.x != 0) return;
  if (r == 0) {
    float* st = a.stats + 4 * seg;
    st[0] = live ? M : -INFINITY;
    st[1] = live ? Wt : 0.0f;
    st[2] = live ? acc[1] : 0.0f;
    st[3] = live && acc[1] > 0.0f ? Wt * Wt / acc[1] : 0.0f;
  }
  a.mean[seg * n + r] = live ? acc[2] + q[0] * rW : NAN;
  if (a.want == GJX_MOMENTS_MEAN) return;
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    if (j >= ns) continue;
    float c = (q[2 * j + 1] - q[0] * q[2 * j] * rW) * rW;
    if (j == 0 && c < 0.0f) c = 0.0f;                      // (a NaN stays)
    if (!live) c = NAN;
    if (NS == 1) {
      a.second[seg * n + r] = c;
    } else {
      a.second[(seg * n + r) * n + (r + j)] = c;
      a.second[(seg * n + (r + j)) * n + r] = c;           // the lower triangle is a copy: exactly symmetric
    }
  }
}

// ---- gjx_weighted_cross_moments: the pair (a_i, b_i) = (rows_a[:, i], rows_b[:, index[i]]) ----
// Launch 1, one block per tile: the lane's four indices are compared with K_b IN FRONT of tile_head_t<true>, which makes a live
// particle with a bad index dead before the tile's maximum and W are taken; the n_b parent values are gathered only where e > 0 (a
// coalesced lineage: almost nowhere) and stay in registers, centred on the tile's mean; the a rows stream through one at a time, the
// next row's load in flight while this row's n_b products are summed.  Partials, field-major f32[3 + n_a + n_b + n_a n_b][n_tiles]:
// m, W, sum e^2, mean_a[r], mean_b[s], M2[r][s].  Launch 2, one block per a row: the merge of k_moments_merge over the n_b columns.
struct CrossArgs {
  MomArgs m;               // rows = rows_a, n_rows = n_a, mean = mean_a, one segment
  const float* rows_b;
  int64_t stride_b;
  int n_b;
  int64_t K_b;
  const int32_t* index;    // or NULL: the identity
  float* mean_b;
  float* cross;
  int32_t* n_bad;
};

template <int NB>
__global__ __launch_bounds__(256) void k_cross_tiles(const CrossArgs c) {
  __shared__ float lds[4 * (NB + 1)];
  __shared__ int32_t cnt[4];
  const MomArgs& a = c.m;
  const int n_a = a.n_rows, n_b = c.n_b;
  TileHead h;
  tile_lane(a, h);
  int32_t idx[4] = {0, 0, 0, 0};
  uint32_t out = 0;
  if (c.index) {
    const int32_t* p = c.index + h.base;
    if (h.nv == 4 && ((uintptr_t)p & 15) == 0) {
      const int4 q = *reinterpret_cast<const int4*>(p);
      idx[0] = q.x; idx[1] = q.y; idx[2] = q.z; idx[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) idx[k] = k < h.nv ? p[k] : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (!((uint32_t)idx[k] < (uint32_t)c.K_b)) out |= 1u << k;      // THE compare: such an index is never an address
  }
  const int killed = tile_head_t<true>(a, lds, h, out);
  if (c.index) {                                                     // block-uniform
    const int bad = (int)__popcll(__ballot(killed & 1)) + 2 * (int)__popcll(__ballot(killed & 2)) + 4 * (int)__popcll(__ballot(killed & 4));
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = cnt[0] + cnt[1] + cnt[2] + cnt[3];
      if (n) atomicAdd(c.n_bad, n);
    }
  }
  // the parents: gathered where the particle is alive (e > 0: inside the segment, and its index passed the compare), else 0
  float b[NB][4];
#pragma unroll
  for (int s = 0; s < NB; ++s) {
    b[s][0] = b[s][1] = b[s][2] = b[s][3] = 0.0f;
    if (s >= n_b) continue;
    const float* row = c.rows_b + (int64_t)s * c.stride_b;
    if (c.index) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (h.e[k] > 0.0f && !((out >> k) & 1u)) b[s][k] = row[idx[k]];
    } else {
      load4(row + h.base, h.nv, 0.0f, b[s]);
#pragma unroll
      for (int k = 0; k < 4; ++k) b[s][k] = h.e[k] > 0.0f ? b[s][k] : 0.0f;
    }
  }
  float cb[NB], ub[NB];
#pragma unroll
  for (int s = 0; s < NB; ++s) {
    cb[s] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) cb[s] = fmaf(h.e[k], b[s][k], cb[s]);
  }
  block_sum<NB>(cb, lds);
#pragma unroll
  for (int s = 0; s < NB; ++s) {
    cb[s] *= h.rW;
    ub[s] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      b[s][k] = h.e[k] > 0.0f ? b[s][k] - cb[s] : 0.0f;             // centred in place
      ub[s] = fmaf(h.e[k], b[s][k], ub[s]);
    }
  }
  block_sum<NB>(ub, lds);
  float* pmean_b = a.part + (int64_t)(3 + n_a) * a.n_tiles + h.tile;
  float* pm2 = a.part + (int64_t)(3 + n_a + n_b) * a.n_tiles + h.tile;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int s = 0; s < NB; ++s)
      if (s < n_b) pmean_b[(int64_t)s * a.n_tiles] = cb[s] + ub[s] * h.rW;
  }
  // the a rows, one at a time
  float xn[4];
  load4(a.rows + h.base, h.nv, 0.0f, xn);
  for (int r = 0; r < n_a; ++r) {
    float x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = h.e[k] > 0.0f ? xn[k] : 0.0f;
    if (r + 1 < n_a) load4(a.rows + (int64_t)(r + 1) * a.row_stride + h.base, h.nv, 0.0f, xn);
    float ca[1] = {0.0f};
#pragma unroll
    for (int k = 0; k < 4; ++k) ca[0] = fmaf(h.e[k], x[k], ca[0]);
    block_sum<1>(ca, lds);
    const float c0 = ca[0] * h.rW;                                   // the rough mean
    float p[NB + 1];
    p[NB] = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      x[k] = h.e[k] > 0.0f ? h.e[k] * (x[k] - c0) : 0.0f;            // e (x - c0)
      p[NB] += x[k];
    }
#pragma unroll
    for (int s = 0; s < NB; ++s) {
      p[s] = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) p[s] = fmaf(x[k], b[s][k], p[s]);
    }
    block_sum<NB + 1>(p, lds);
    if (threadIdx.x == 0) {
      const float ua = p[NB];
      a.part[(int64_t)(3 + r) * a.n_tiles + h.tile] = c0 + ua * h.rW;
#pragma unroll
      for (int s = 0; s < NB; ++s)
        if (s < n_b) pm2[((int64_t)r * n_b + s) * a.n_tiles] = p[s] - ua * ub[s] * h.rW;
    }
  }
}

// block r: the mean of a row r and its n_b centred cross-moments; every block forms the b means the same way, block 0 writes them
template <int NB>
__global__ __launch_bounds__(256) void k_cross_merge(const CrossArgs c) {
  __shared__ float lds[4 * (2 * NB + 3)];
  const MomArgs& a = c.m;
  const int n_a = a.n_rows, n_b = c.n_b, nt = a.nt_seg;
  const int r = blockIdx.x;
  const int64_t nT = a.n_tiles;
  const float* pm = a.part;
  const float* pW = pm + nT;
  const float* pQ = pW + nT;
  const float* pa = pm + (int64_t)(3 + r) * nT;
  const float* pb = pm + (int64_t)(3 + n_a) * nT;                   // + s * nT
  const float* pm2 = pm + (int64_t)(3 + n_a + n_b + (int64_t)r * n_b) * nT;      // + s * nT
  float M = -INFINITY;
  for (int t = threadIdx.x; t < nt; t += 256) M = fmaxf(M, pm[t]);
  M = block_max(M, lds);
  const int per = (nt + 255) >> 8;
  const int t0 = threadIdx.x * per, t1 = t0 + per < nt ? t0 + per : nt;
  // pass 1: total weight, sum of squares, rough means
  float acc[NB + 3];
#pragma unroll
  for (int j = 0; j < NB + 3; ++j) acc[j] = 0.0f;
  for (int t = t0; t < t1; ++t) {
    const float Wt = pW[t];
    if (!(Wt > 0.0f)) continue;                            // a dead tile is skipped, not weighted by zero
    const float f = fast_exp(pm[t] - M), g = f * Wt;
    acc[0] += g;
    acc[1] = fmaf(pQ[t], f * f, acc[1]);
    acc[2] = fmaf(g, pa[t], acc[2]);
#pragma unroll
    for (int s = 0; s < NB; ++s)
      if (s < n_b) acc[3 + s] = fmaf(g, pb[(int64_t)s * nT + t], acc[3 + s]);
  }
  block_sum<NB + 3>(acc, lds);
  const float Wt = acc[0];
  const bool live = M > -INFINITY && Wt > 0.0f;
  const float rW = live ? 1.0f / Wt : 0.0f;
#pragma unroll
  for (int j = 2; j < NB + 3; ++j) acc[j] *= rW;
  // pass 2: centred on the rough means.  q[0]: sum g d_a; q[1 + 2 s]: sum g d_bs; q[2 + 2 s]: sum g d_a d_bs + f M2_rs
  float q[2 * NB + 1];
#pragma unroll
  for (int j = 0; j < 2 * NB + 1; ++j) q[j] = 0.0f;
  for (int t = t0; t < t1; ++t) {
    const float Wb = pW[t];
    if (!(Wb > 0.0f)) continue;
    const float f = fast_exp(pm[t] - M), g = f * Wb;
    const float da = pa[t] - acc[2];
    q[0] = fmaf(g, da, q[0]);
#pragma unroll
    for (int s = 0; s < NB; ++s) {
      if (s >= n_b) continue;
      const float db = pb[(int64_t)s * nT + t] - acc[3 + s];
      q[1 + 2 * s] = fmaf(g, db, q[1 + 2 * s]);
      q[2 + 2 * s] += fmaf(g * da, db, f * pm2[(int64_t)s * nT + t]);
    }
  }
  block_sum<2 * NB + 1>(q, lds);
  if (threadIdx.x != 0) return;
  if (r == 0) {
    float* st = a.stats;
    st[0] = live ? M : -INFINITY;
    st[1] = live ? Wt : 0.0f;
    st[2] = live ? acc[1] : 0.0f;
    st[3] = live && acc[1] > 0.0f ? Wt * Wt / acc[1] : 0.0f;
#pragma unroll
    for (int s = 0; s < NB; ++s)
      if (s < n_b) c.mean_b[s] = live ? acc[3 + s] + q[1 + 2 * s] * rW : NAN;
  }
  a.mean[r] = live ? acc[2] + q[0] * rW : NAN;
#pragma unroll
  for (int s = 0; s < NB; ++s)
    if (s < n_b) c.cross[(int64_t)r * n_b + s] = live ? (q[2 + 2 * s] - q[0] * q[1 + 2 * s] * rW) * rW : NAN;
}

template <int NB>
static hipError_t cross_launch(const CrossArgs& c, hipStream_t st, const char** where) {
  *where = "gjx_weighted_cross_moments(tiles)";
  hipLaunchKernelGGL(k_cross_tiles<NB>, dim3((unsigned)c.m.n_tiles), dim3(256), 0, st, c);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  *where = "gjx_weighted_cross_moments(merge)";
  hipLaunchKernelGGL(k_cross_merge<NB>, dim3((unsigned)c.m.n_rows), dim3(256), 0, st, c);
  return hipGetLastError();
}

// tiles and fields of the partials; false: a shape the call refuses
static bool cross_shape(int32_t n_a, int32_t n_b, int64_t K, int64_t* n_tiles, int64_t* fields) {
  if (n_a <= 0 || n_b <= 0 || K <= 0) return false;
  const int64_t nt = (K + kMomTile - 1) / kMomTile;
  if (nt > INT32_MAX) return false;
  *n_tiles = nt;
  *fields = 3 + (int64_t)n_a + n_b + (int64_t)n_a * n_b;
  return true;
}

// fields of the per-tile partials; false: a shape the call refuses
static bool moments_shape(int32_t n_rows, int64_t K, int64_t n_segments, int32_t want, int64_t* nt_seg, int64_t* n_tiles, int64_t* fields) {
  if (n_rows <= 0 || K <= 0 || n_segments <= 0 || K % n_segments != 0) return false;
  if (want != GJX_MOMENTS_MEAN && want != GJX_MOMENTS_VAR && want != GJX_MOMENTS_COV) return false;
  const int64_t nt = (K / n_segments + kMomTile - 1) / kMomTile;
  if (nt > INT32_MAX || nt * n_segments > INT32_MAX || n_segments * (int64_t)n_rows > INT32_MAX) return false;     // grid sizes
  *nt_seg = nt;
  *n_tiles = nt * n_segments;
  *fields = 3 + (int64_t)n_rows + (want == GJX_MOMENTS_COV ? (int64_t)n_rows * (n_rows + 1) / 2 : (int64_t)n_rows);
  return true;
}

}  // namespace gjx

extern "C" size_t gjx_weighted_moments_workspace_bytes(int32_t n_rows, int64_t K, int64_t n_segments, int32_t want) {
  int64_t nt_seg, n_tiles, fields;
  if (!gjx::moments_shape(n_rows, K, n_segments, want, &nt_seg, &n_tiles, &fields)) return 0;
  if (want == GJX_MOMENTS_COV && n_rows > GJX_MOMENTS_MAX_COV_ROWS) return 0;
  return sizeof(float) * (size_t)fields * (size_t)n_tiles;
}

extern "C" int gjx_weighted_moments(const float* rows, int64_t row_stride, int32_t n_rows, const float* logw, int64_t K,
                                    int64_t n_segments, int32_t want, float* stats, float* mean, float* second, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  using namespace gjx;
  int64_t nt_seg, n_tiles, fields;
  if (!rows || !stats || !mean || !workspace || (!second && want != GJX_MOMENTS_MEAN) || row_stride < K ||
      !moments_shape(n_rows, K, n_segments, want, &nt_seg, &n_tiles, &fields))
    return gjx_fail(GJX_EINVAL, "gjx_weighted_moments: bad argument");
  if (want == GJX_MOMENTS_COV && n_rows > GJX_MOMENTS_MAX_COV_ROWS) {
    char msg[160];
    snprintf(msg, sizeof(msg), "gjx_weighted_moments: a covariance takes at most GJX_MOMENTS_MAX_COV_ROWS = %d rows, not %d",
             GJX_MOMENTS_MAX_COV_ROWS, (int)n_rows);
    return gjx_fail(GJX_EUNSUPPORTED, msg);
  }
  if (workspace_bytes < sizeof(float) * (size_t)fields * (size_t)n_tiles)
    return gjx_fail(GJX_EWORKSPACE, "gjx_weighted_moments: workspace too small");
  MomArgs a;
  memset(&a, 0, sizeof(a));
  a.rows = rows; a.row_stride = row_stride; a.n_rows = n_rows; a.logw = logw; a.K_seg = K / n_segments; a.nt_seg = (int)nt_seg;
  a.n_tiles = n_tiles; a.part = (float*)workspace; a.want = want; a.stats = stats; a.mean = mean; a.second = second;
  const hipStream_t st = (hipStream_t)stream;
  const dim3 merge_grid((unsigned)(n_segments * n_rows));
  if (want == GJX_MOMENTS_COV) {
    hipLaunchKernelGGL(k_moments_cov_tiles, dim3((unsigned)n_tiles), dim3(256), 0, st, a);
    GJX_CHECK_LAUNCH("gjx_weighted_moments(tiles)");
    hipLaunchKernelGGL(k_moments_merge<kCovMax>, merge_grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(k_moments_tiles, dim3((unsigned)n_tiles), dim3(256), 0, st, a);
    GJX_CHECK_LAUNCH("gjx_weighted_moments(tiles)");
    hipLaunchKernelGGL(k_moments_merge<1>, merge_grid, dim3(256), 0, st, a);
  }
  GJX_CHECK_LAUNCH("gjx_weighted_moments(merge)");
  return GJX_OK;
}

extern "C" size_t gjx_weighted_cross_moments_workspace_bytes(int32_t n_a, int32_t n_b, int64_t K) {
  int64_t n_tiles, fields;
  if (!gjx::cross_shape(n_a, n_b, K, &n_tiles, &fields)) return 0;
  if (n_a > GJX_MOMENTS_MAX_COV_ROWS || n_b > GJX_MOMENTS_MAX_COV_ROWS) return 0;
  return sizeof(float) * (size_t)fields * (size_t)n_tiles;
}

extern "C" int gjx_weighted_cross_moments(const float* rows_a, int64_t stride_a, int32_t n_a, const float* rows_b, int64_t stride_b,
                                          int32_t n_b, int64_t K_b, const int32_t* index, const float* logw, int64_t K, float* stats,
                                          float* mean_a, float* mean_b, float* cross, int32_t* n_bad, void* workspace,
                                          size_t workspace_bytes, void* stream) {
  using namespace gjx;
  int64_t n_tiles, fields;
  if (!rows_a || !rows_b || !stats || !mean_a || !mean_b || !cross || !n_bad || !workspace || !cross_shape(n_a, n_b, K, &n_tiles, &fields) ||
      stride_a < K || K_b <= 0 || stride_b < K_b || (index ? K_b > INT32_MAX : K_b < K))
    return gjx_fail(GJX_EINVAL, "gjx_weighted_cross_moments: bad argument");
  if (n_a > GJX_MOMENTS_MAX_COV_ROWS || n_b > GJX_MOMENTS_MAX_COV_ROWS) {
    char msg[160];
    snprintf(msg, sizeof(msg), "gjx_weighted_cross_moments: each side takes at most GJX_MOMENTS_MAX_COV_ROWS = %d rows, not %d and %d",
             GJX_MOMENTS_MAX_COV_ROWS, (int)n_a, (int)n_b);
    return gjx_fail(GJX_EUNSUPPORTED, msg);
  }
  if (workspace_bytes < sizeof(float) * (size_t)fields * (size_t)n_tiles)
    return gjx_fail(GJX_EWORKSPACE, "gjx_weighted_cross_moments: workspace too small");
  CrossArgs c;
  memset(&c, 0, sizeof(c));
  c.m.rows = rows_a; c.m.row_stride = stride_a; c.m.n_rows = n_a; c.m.logw = logw; c.m.K_seg = K; c.m.nt_seg = (int)n_tiles;
  c.m.n_tiles = n_tiles; c.m.part = (float*)workspace; c.m.want = GJX_MOMENTS_COV; c.m.stats = stats; c.m.mean = mean_a;
  c.rows_b = rows_b; c.stride_b = stride_b; c.n_b = n_b; c.K_b = K_b; c.index = index; c.mean_b = mean_b; c.cross = cross; c.n_bad = n_bad;
  const hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(n_bad, 0, 4, st);
  if (e != hipSuccess) return gjx_fail_hip(e, "gjx_weighted_cross_moments(memset)");
  const char* where = "";
  e = n_b <= 4 ? cross_launch<4>(c, st, &where) : n_b <= 8 ? cross_launch<8>(c, st, &where) : cross_launch<16>(c, st, &where);
  if (e != hipSuccess) return gjx_fail_hip(e, where);
  return GJX_OK;
}
