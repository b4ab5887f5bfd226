// gjx_lineage.hip — descendant weights of a filter's history (gjx_lineage_weights): for every stored step t and particle j, the
// final weight of all last-step particles whose lineage passes through j.  The smoothing marginal at step t is the step's stored
// particles under these weights; the number of non-zero ones per step (the survivors) is the path-degeneracy diagnostic.
//
// Weights are the integers of gjx_quantiles.hip: u_i = (uint64) rint(fast_exp(logw_i - M) 2^32).  W_{T-1} = u, and
// W_{t-1}[a] = sum of W_t[i] over the children i of a: a backward scatter-add of 64-bit integers, so the order in which the hardware
// serves the atomics cannot change a bit of the result.
//
// Launches (plain launches on the stream, nothing read back, no block waits for another):
//   memsets of the counters and of the first destination buffer; k_l_max: the maximum log-weight (integer atomic max on the ordered
//   key); k_l_init: u into the first buffer, U = sum u and Q = sum rint(e^2 2^32) with one atomic per block;
//   per step t = T-1 .. 0, k_l_step: reads W_t, writes row t of w, counts the survivors (one atomic per block), scatters W_t into
//   W_{t-1} (t > 0) and zeroes the buffer that the NEXT launch scatters into.  Three u64[K] buffers rotate: read, add, zero.
//
// The scatter.  A wave takes 64 consecutive particles.  Resampled ancestors are non-decreasing, so the children of one parent sit in
// adjacent lanes: a ballot marks the head of every run of equal destinations, a segmented suffix sum over the 64 lanes leaves each
// run's sum in its head, and only a head whose sum is not zero issues the 64-bit atomicAdd.  Any ancestor order is correct; equal
// destinations that are not adjacent just cost an atomic each.  A coalesced lineage (W_t almost everywhere 0) issues almost nothing.
// An ancestor is used as an index in ONE place, the atomicAdd of the head, behind the compare (uint32_t)d < K.
#include <math.h>
#include <string.h>

#include "gjx_device.h"
#include "gjx_host.h"

namespace gjx {

constexpr int kLTile = 1024;                          // particles per block: 256 lanes x 4, lane l of pass k on particle 256 k + l

typedef unsigned long long u64;

// the counters at the head of the workspace, zeroed by the call
struct LCtrl {
  uint32_t maxkey;         // ordered key of the maximum log-weight (0: none yet)
  uint32_t pad_;
  u64 U;                   // sum u
  u64 Q;                   // sum rint(e^2 2^32)
  u64 pad2_[5];
};

struct LArgs {
  const int32_t* anc;      // ancestors[t-1]: the parents of step t's particles (NULL at t == 0)
  const float* logw;       // or NULL: equal weights
  int64_t K;
  bool last;               // t == T-1: this launch writes stats
  bool zero_next;          // another scatter follows the next launch's: zero its destination
  LCtrl* ctrl;
  const u64* src;          // W_t
  u64* dst;                // W_{t-1}, zero before this launch
  u64* zero;               // the third buffer
  float* w_row;            // w[t]
  int32_t* survivors;      // &survivors[t]
  int32_t* n_bad;
  float* stats;
};

// the order-preserving map of the float bits, the integer weight, and the 64-bit wave sum: as in gjx_quantiles.hip
GJX_DEV uint32_t l_ordered_key(uint32_t bits) { return bits ^ ((bits & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u); }
GJX_DEV uint32_t l_ordered_bits(uint32_t key) { return key ^ ((key & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu); }
// rint(e 2^32) for 0 <= e <= 1: one 32-bit conversion below 1 (e 2^32 <= 2^32 - 256 there), 2^32 at 1
GJX_DEV u64 l_weight_u(float e) { return e >= 1.0f ? (u64)1 << 32 : (u64)(uint32_t)rintf(e * 4294967296.0f); }
GJX_DEV u64 l_wave_sum_u64(u64 v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

GJX_DEV float l_max(const LArgs& a) {
  if (!a.logw) return 0.0f;
  const uint32_t k = a.ctrl->maxkey;
  return k ? __uint_as_float(l_ordered_bits(k)) : -INFINITY;
}

__global__ __launch_bounds__(256) void k_l_max(const LArgs a) {
  __shared__ float lds[4];
  const int64_t p0 = (int64_t)blockIdx.x * kLTile;
  float m = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = p0 + k * 256 + threadIdx.x;
    if (i < a.K) m = fmaxf(m, a.logw[i]);                  // fmaxf drops a NaN
  }
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = fmaxf(fmaxf(lds[0], lds[1]), fmaxf(lds[2], lds[3]));
    const uint32_t key = l_ordered_key(__float_as_uint(m));
    if (key > a.ctrl->maxkey) atomicMax(&a.ctrl->maxkey, key);         // (the word only grows: a stale read costs an atomic, no more)
  }
}

// W_{T-1} = u into a.dst (every entry written: the buffer needs no zeroing), U and Q
__global__ __launch_bounds__(256) void k_l_init(const LArgs a) {
  __shared__ u64 red[8];
  const int64_t p0 = (int64_t)blockIdx.x * kLTile;
  const float M = l_max(a);
  u64 su = 0, sq = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = p0 + k * 256 + threadIdx.x;
    if (i >= a.K) continue;
    const float lw = a.logw ? a.logw[i] : 0.0f;
    const float e = M > -INFINITY ? fast_exp(lw - M) : 0.0f;
    const u64 u = e > 0.0f ? l_weight_u(e) : 0;                        // (a NaN weight: dead)
    a.dst[i] = u;
    su += u;
    if (u != 0) sq += l_weight_u(e * e);
  }
  su = l_wave_sum_u64(su);
  sq = l_wave_sum_u64(sq);
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = su; red[4 + (threadIdx.x >> 6)] = sq; }
  __syncthreads();
  if (threadIdx.x == 0) {
    su = red[0] + red[1] + red[2] + red[3];
    sq = red[4] + red[5] + red[6] + red[7];
    if (su) atomicAdd(&a.ctrl->U, su);
    if (sq) atomicAdd(&a.ctrl->Q, sq);
  }
}

// {max, sum e, sum e^2, ESS} from the integers, as gjx_weighted_quantiles writes them
GJX_DEV void l_write_stats(const LArgs& a) {
  const u64 U = a.ctrl->U, Q = a.ctrl->Q;
  float* st = a.stats;
  if (U == 0 || Q == 0) {
    st[0] = -INFINITY; st[1] = 0.0f; st[2] = 0.0f; st[3] = 0.0f;
    return;
  }
  const double s1 = (double)U * (1.0 / 4294967296.0), s2 = (double)Q * (1.0 / 4294967296.0);
  st[0] = l_max(a);
  st[1] = (float)s1;
  st[2] = (float)s2;
  st[3] = (float)(s1 * s1 / s2);
}

// Called by whole waves: lane l adds v to dst[d] (the caller passes v = 0 and d = -1 for a lane that has nothing to add).  Runs of
// equal adjacent d are summed into their first lane, which adds the sum to dst[d] if it is not zero and d is inside [0, K).
GJX_DEV void l_scatter(u64* dst, int64_t K, int32_t d, u64 v) {
  if (__ballot(v != 0) == 0) return;                       // wave-uniform: nothing alive here
  const int lane = threadIdx.x & 63;
  const int32_t d_prev = __shfl_up(d, 1, 64);
  const bool head = lane == 0 || d != d_prev;
  const u64 heads = __ballot(head);
  if (heads != ~(u64)0) {                                  // (every lane its own run: nothing to combine)
    // the last lane of the lane's run: one in front of the next head above it
    const u64 above = lane == 63 ? 0 : heads >> (lane + 1);
    const int run_end = above ? lane + __ffsll((long long)above) - 1 : 63;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {                     // segmented suffix sum: after the step, v covers [lane, min(lane + 2s - 1, run_end)]
      const u64 o = __shfl_down(v, s, 64);
      if (lane + s <= run_end) v += o;
    }
  }
  if (head && v != 0 && (uint32_t)d < (uint32_t)K) atomicAdd(&dst[d], v);
}

__global__ __launch_bounds__(256) void k_l_step(const LArgs a) {
  __shared__ int32_t cnt[8];
  const int64_t p0 = (int64_t)blockIdx.x * kLTile;
  const u64 U = a.ctrl->U;
  const double Ud = (double)U;
  u64 W[4];
  int32_t d[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {                            // the loads of the four passes first
    const int64_t i = p0 + k * 256 + threadIdx.x;
    const bool in = i < a.K;
    W[k] = in ? a.src[i] : 0;
    d[k] = (in && a.anc) ? a.anc[i] : -1;
  }
  int32_t alive = 0, bad = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int64_t i = p0 + k * 256 + threadIdx.x;
    if (p0 + k * 256 >= a.K) break;                        // block-uniform
    if (i < a.K) {
      a.w_row[i] = U ? (float)((double)W[k] / Ud) : NAN;
      if (a.zero_next) a.zero[i] = 0;
    }
    alive += W[k] != 0;
    if (a.anc) {
      const bool out = (uint32_t)d[k] >= (uint32_t)a.K;    // a link that leaves [0, K): its weight is dropped, and counted
      bad += out && W[k] != 0;
      // (a lane with W = 0 keeps its d: it adds nothing and does not cut the run of its live siblings in two)
      l_scatter(a.dst, a.K, out ? -1 : d[k], out ? 0 : W[k]);
    }
  }
  alive = (int32_t)__popcll(__ballot(alive & 1)) + 2 * (int32_t)__popcll(__ballot(alive & 2)) + 4 * (int32_t)__popcll(__ballot(alive & 4));
  bad = (int32_t)__popcll(__ballot(bad & 1)) + 2 * (int32_t)__popcll(__ballot(bad & 2)) + 4 * (int32_t)__popcll(__ballot(bad & 4));
  if ((threadIdx.x & 63) == 0) { cnt[threadIdx.x >> 6] = alive; cnt[4 + (threadIdx.x >> 6)] = bad; }
  __syncthreads();
  if (threadIdx.x == 0) {
    alive = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    bad = cnt[4] + cnt[5] + cnt[6] + cnt[7];
    if (alive) atomicAdd(a.survivors, alive);
    if (bad) atomicAdd(a.n_bad, bad);
    if (a.last && blockIdx.x == 0) l_write_stats(a);
  }
}

// workspace: [LCtrl] [u64[K]] [u64[K]] [u64[K]], 8-byte aligned; 0: a shape the call refuses
static size_t l_bytes(int32_t T, int64_t K) {
  if (T <= 0 || K <= 0 || K > INT32_MAX) return 0;
  return 8 + sizeof(LCtrl) + 3 * 8 * (size_t)K;            // (8: the alignment of any pointer)
}

}  // namespace gjx

extern "C" size_t gjx_lineage_weights_workspace_bytes(int32_t T, int64_t K) { return gjx::l_bytes(T, K); }

extern "C" int gjx_lineage_weights(const int32_t* ancestors, int64_t anc_stride, int32_t T, int64_t K, const float* logw, float* stats,
                                   float* w, int32_t* survivors, int32_t* n_bad, void* workspace, size_t workspace_bytes, void* stream) {
  using namespace gjx;
  static_assert(sizeof(LCtrl) == 64, "the counters are one 64-byte block");
  const size_t need = l_bytes(T, K);
  if (!stats || !w || !survivors || !n_bad || !workspace || need == 0 || (T > 1 && (!ancestors || anc_stride < K)))
    return gjx_fail(GJX_EINVAL, "gjx_lineage_weights: bad argument");
  if (workspace_bytes < need) return gjx_fail(GJX_EWORKSPACE, "gjx_lineage_weights: workspace too small");
  const hipStream_t st = (hipStream_t)stream;
  char* base = (char*)(((uintptr_t)workspace + 7) & ~(uintptr_t)7);
  LArgs a;
  memset(&a, 0, sizeof(a));
  a.ctrl = (LCtrl*)base;
  u64* buf[3];
  for (int r = 0; r < 3; ++r) buf[r] = (u64*)(base + sizeof(LCtrl)) + (size_t)r * (size_t)K;
  a.logw = logw; a.K = K; a.n_bad = n_bad; a.stats = stats;
  // the counters and buf[0], the destination of the first scatter, in one piece; k_l_init fills buf[2]; the first step zeroes buf[1]
  hipError_t e = hipMemsetAsync(base, 0, sizeof(LCtrl) + (T > 1 ? 8 * (size_t)K : 0), st);
  if (e == hipSuccess) e = hipMemsetAsync(survivors, 0, 4 * (size_t)T, st);
  if (e == hipSuccess) e = hipMemsetAsync(n_bad, 0, 4, st);
  if (e != hipSuccess) return gjx_fail_hip(e, "gjx_lineage_weights(memset)");
  const dim3 grid((unsigned)((K + kLTile - 1) / kLTile)), block(256);
  if (logw) {
    hipLaunchKernelGGL(k_l_max, grid, block, 0, st, a);
    GJX_CHECK_LAUNCH("gjx_lineage_weights(max)");
  }
  a.dst = buf[2];
  hipLaunchKernelGGL(k_l_init, grid, block, 0, st, a);
  GJX_CHECK_LAUNCH("gjx_lineage_weights(init)");
  int r = 2;                                               // the buffer that holds W_t
  for (int t = T - 1; t >= 0; --t) {
    a.last = t == T - 1;
    a.anc = t > 0 ? ancestors + (size_t)(t - 1) * (size_t)anc_stride : nullptr;
    a.src = buf[r];
    a.dst = buf[(r + 1) % 3];
    a.zero = buf[(r + 2) % 3];
    a.zero_next = t >= 2;                                  // the launch of step t-1 scatters into it (t-1 >= 1)
    a.w_row = w + (size_t)t * (size_t)K;
    a.survivors = survivors + t;
    hipLaunchKernelGGL(k_l_step, grid, block, 0, st, a);
    GJX_CHECK_LAUNCH("gjx_lineage_weights(step)");
    r = (r + 1) % 3;
  }
  return GJX_OK;
}
