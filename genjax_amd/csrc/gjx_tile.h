// gjx_tile.h — device helpers shared by the one-launch filters (gjx_ssm.hip, gjx_pfilter.inl): agent- / system-scope
// accesses for data other blocks (or other ranks) of the SAME launch read, the propagation noise in two halves, the
// tile-scaled fixed point (GJX_WEIGHTS_TILE_SCALED, include/gjx.h), and the primitives every resampling kernel is built from
// (tile totals, prefix, source tile, re-scan round, in-tile search).
#pragma once
#include "gjx_device.h"
#include "gjx_scan.h"

namespace gjx {

constexpr int kSsmPersistMaxDy = 32;              // observation dimension the one-launch filters stage in LDS

GJX_DEV float load_agent(const float* p) { return __int_as_float(__hip_atomic_load((const int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)); }
// four consecutive floats through ONE 16-byte sc1 load (4-byte sc1 accesses run at a fraction of the 16-byte rate); the
// wait sits inside the asm because the compiler does not count an asm's memory operations
GJX_DEV void load_agent_x4(const float* p, float (&v)[4]) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 r;
  asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
  v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
}
// four consecutive floats through ONE 16-byte write-through store (completion: the caller's s_waitcnt vmcnt(0) — the compiler
// does not count an asm's memory operations)
GJX_DEV void store_agent_x4(float* p, const float (&v)[4]) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 r = {v[0], v[1], v[2], v[3]};
  asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(r) : "memory");
}
GJX_DEV void store_agent(float* p, float v) { __hip_atomic_store((int*)p, __float_as_int(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// The same accesses with the scope as a (wave-uniform) argument: `sys` selects SYSTEM scope (sc0 sc1) for memory that
// kernels of OTHER ranks read or write during the same launch — peer-mapped windows over xGMI, gjx_peer.hip.  One scalar
// branch per access; on one GPU the agent-scope form runs.
GJX_DEV float load_scoped(const float* p, bool sys) {
  return sys ? __int_as_float(__hip_atomic_load((const int*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) : load_agent(p);
}
GJX_DEV void load_scoped_x4(const float* p, float (&v)[4], bool sys) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  f4 r;
  if (sys) asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
  else asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(r) : "v"(p) : "memory");
  v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
}
GJX_DEV void store_scoped(float* p, float v, bool sys) {
  if (sys) __hip_atomic_store((int*)p, __float_as_int(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else store_agent(p, v);
}
GJX_DEV void store_scoped_u64(unsigned long long* p, unsigned long long v, bool sys) {
  if (sys) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
GJX_DEV unsigned long long load_scoped_u64(const unsigned long long* p, bool sys) {
  return sys ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
GJX_DEV void store_scoped_u32(unsigned* p, unsigned v, bool sys) {
  if (sys) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
GJX_DEV unsigned load_scoped_u32(const unsigned* p, bool sys) {
  return sys ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ---- verify mode of the sharded kernels (GJX_PEER_VERIFY=1, gjx_peer.hip): a check word per particle row, stored by the
// owner beside the row and recomputed by every reader that pulls the row.  It folds in the STEP the row belongs to and the
// particle's global index, so a reader that is served an older generation of the same addresses (the buffers ping-pong:
// the previous occupant is the row of step t - 2), a torn row, or a row of another particle cannot pass.
GJX_DEV uint32_t row_check_init(int t, uint32_t gslot) { return (0x9E3779B9u * (uint32_t)(t + 1)) ^ (gslot * 0x85EBCA6Bu); }
GJX_DEV uint32_t row_check_mix(uint32_t h, float v) {
  h ^= __float_as_uint(v);
  h *= 0x01000193u;
  return h ^ (h >> 15);
}
// pointer into rank g's copy of a window: this rank's pointer + the byte distance between the two mappings (0 for g == rank)
template <class Tp>
GJX_DEV Tp* peer_ptr(Tp* local, long long delta) { return (Tp*)((char*)local + delta); }

// standard-normal draws of slot gidx under the step's propagation key (k_ssm_step's streams), in two halves: the random
// words (the hashes: most of the VALU work, done inside the granule wait) and the normals from them (Box-Muller, done
// behind the loads of the ancestor's state).  A block's window work must stay below the ~1 us of slack the LAST block
// to publish has over the others, or that block is late again in the next step and its chain sets the step time.
template <int RNG, int DX>
struct SsmNoiseBits { uint32_t w[RNG == GJX_RNG_FLAT ? 2 * GJX_FLAT_BLOCKS(DX + (DX & 1)) : DX]; };

template <int RNG, int DX>
GJX_DEV void ssm_noise_bits(key2 skj, uint64_t gidx, SsmNoiseBits<RNG, DX>& nb) {
  if (RNG == GJX_RNG_JAX32) skj = fold_in(fold_in64(skj, gidx), 1u);
  else if (gidx >> 32) skj = threefry2x32(skj, 0xFFFFFFFFu, (uint32_t)(gidx >> 32));
  if (RNG == GJX_RNG_FLAT) {
    constexpr int NB = GJX_FLAT_BLOCKS(DX + (DX & 1));
#pragma unroll
    for (int h = 0; h < NB; ++h) {
      const key2 hh = threefry2x32(skj, (uint32_t)gidx, (1u << GJX_FLAT_SITE_SHIFT) | (uint32_t)h);
      nb.w[2 * h] = hh.a; nb.w[2 * h + 1] = hh.b;
    }
  } else {
#pragma unroll
    for (int d0 = 0; d0 < DX; ++d0) {
      const key2 h0 = threefry2x32(skj, 0u, (uint32_t)d0);
      nb.w[d0] = h0.a ^ h0.b;
    }
  }
}
template <int RNG, int DX>
GJX_DEV void ssm_noise_normals(const SsmNoiseBits<RNG, DX>& nb, float (&nz)[DX]) {
  if (RNG == GJX_RNG_FLAT) {
#pragma unroll
    for (int d0 = 0; d0 < DX; d0 += 2) {
      float n0, n1;
      box_muller(GJX_FIELD(nb.w, d0), GJX_FIELD(nb.w, d0 + 1), n0, n1);
      nz[d0] = n0;
      if (d0 + 1 < DX) nz[d0 + 1] = n1;
    }
  } else {
#pragma unroll
    for (int d0 = 0; d0 < DX; ++d0) nz[d0] = normal_from_bits_fast(nb.w[d0]);
  }
}

// ---- tile-scaled fixed point (shared by the one-launch filters and the tile-scaled resamplers of gjx_resample.hip) ----
constexpr int kTileQ = 1024;                       // particles per quantisation tile
constexpr float kTileScale = 536870912.0f;         // 2^29
constexpr int kTileDead = -524288;                 // exponent of a tile without a finite positive weight (-2^19)
constexpr float kLog2e = 1.44269504f;

GJX_DEV int tile_exponent(float tile_max) {        // e_b = ceil(max * log2 e), clamped to 20 bits; tile_max never NaN (fmaxf)
  if (!(tile_max > -INFINITY)) return kTileDead;
  const float t = ceilf(tile_max * kLog2e);
  return t < -524287.0f ? -524287 : (t > 524287.0f ? 524287 : (int)t);
}
GJX_DEV uint64_t tile_q(float lw, int e) {         // floor(2^29 * min(1, 2^(lw * log2 e - e))); NaN / -inf / dead tile -> 0
  if (e == kTileDead) return 0;
  float w = __builtin_amdgcn_exp2f(fmaf(lw, kLog2e, -(float)e));   // one rounding: the oracle uses fmaf too
  w = w > 0.0f ? w : 0.0f;
  w = w < 1.0f ? w : 1.0f;
  return (uint64_t)(uint32_t)(w * kTileScale);    // <= 2^29: one v_cvt_u32_f32 (a float -> u64 conversion is eight instructions)
}
// granule of the tiled rendezvous: tag (4 bits, != 0) | e_b + 2^19 (20 bits) | S_b (40 bits, S_b <= 2^39).  Four tag
// bits are plenty: a block rewrites its granule of one parity every second step, so a reader can only ever meet the
// tag of step t or of step t - 2
GJX_DEV unsigned long long tile_granule(unsigned long long tag, int e, uint64_t S) {
  return (tag << 60) | ((unsigned long long)(unsigned)(e - kTileDead) << 40) | (S & ((1ull << 40) - 1));
}
GJX_DEV void tile_granule_unpack(unsigned long long v, uint64_t& S, int& e) {   // (a tile without weight is dead whatever its exponent field says)
  S = v & ((1ull << 40) - 1);
  e = S ? (int)((v >> 40) & 0xFFFFFu) + kTileDead : kTileDead;
}
// the granules of a rendezvous sit one per 64-byte line: 256 blocks storing into 32 shared lines serialise in the L2 (11.6 -> 11.0 us
// per step of k_ssm_persistent; 128-byte spacing measured the same)
constexpr int kGranulePad = 8;

// ---- the pieces every resampling kernel is built from ("Resampling primitives").  They cover the arithmetic BETWEEN the
//      points other blocks or ranks observe: polls, tags, publications and their waits stay in the kernels.  A tile has TILE
//      particles, a lane takes ITEMS consecutive ones, so TILE / (64 ITEMS) waves cover a tile. ----

// One tile held by a block of THREADS lanes x ITEMS log-weights (-inf where there is no particle) -> the tile's exponent (returned, in
// every thread), the lane's fixed-point weights q, the inclusive wave scan of the lane's sum (inc), the wave totals in
// red_q[0 .. THREADS / 64).  Two barriers: red_m / red_q (THREADS / 64 words each) are free before the call, red_q is readable after it.
template <int THREADS, int ITEMS>
GJX_DEV int tile_quantise(const float (&lw)[ITEMS], float* red_m, uint64_t* red_q, uint64_t (&q)[ITEMS], uint64_t& inc) {
  constexpr int NW = THREADS / 64;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float m = lw[0];
#pragma unroll
  for (int k = 1; k < ITEMS; ++k) m = fmaxf(m, lw[k]);
  const float wm = wave_max(m);
  if (lane == 0) red_m[wid] = wm;
  __syncthreads();
  float bm = red_m[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) bm = fmaxf(bm, red_m[w]);
  const int e = tile_exponent(bm);
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) { q[k] = tile_q(lw[k], e); s += q[k]; }
  inc = wave_scan_u64(s);
  const uint64_t wt = lane63_u64(inc);
  if (lane == 0) red_q[wid] = wt;
  __syncthreads();
  return e;
}
template <int NW>
GJX_DEV uint64_t sum_partials(const uint64_t* w) {
  uint64_t t = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) t += w[k];
  return t;
}

// Tile totals P[1 .. n] -> their inclusive prefix, in place (P[0] stays): thread t owns the stretch [t per, (t + 1) per), the waves'
// sums meet in wave_partials [THREADS / 64].  shift_of(b): right shift that brings tile b's total to the common exponent (64 or
// more: the tile is shifted out), or NoShift{} for totals that are on one scale already.  THREADS > 64: every thread of the block
// calls it, one barrier inside and one at the end.  THREADS == 64: ONE wave calls it (few tiles: ceil(n / 64) entries per lane and one
// DPP scan instead of all waves and a barrier between their partial sums), no barrier, wave_partials unused.
struct NoShift {};
template <class A, class B> struct SameType { static constexpr bool value = false; };
template <class A> struct SameType<A, A> { static constexpr bool value = true; };
template <int THREADS, class ShiftOf>
GJX_DEV void prefix_in_place(uint64_t* P, int n, uint64_t* wave_partials, ShiftOf shift_of) {
  static_assert(THREADS >= 64 && (THREADS & (THREADS - 1)) == 0, "whole waves, a power of two");
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int t = THREADS == 64 ? lane : (int)threadIdx.x;
  const int per = (n + THREADS - 1) >> __builtin_ctz((unsigned)THREADS);
  const int e0 = t * per < n ? t * per : n, e1 = (e0 + per) < n ? (e0 + per) : n;
  uint64_t loc = 0;
  for (int e = e0; e < e1; ++e) {
    uint64_t g = P[e + 1];
    if constexpr (!SameType<ShiftOf, NoShift>::value) {
      const int sh = shift_of(e);
      g = sh < 64 ? g >> sh : 0;
      P[e + 1] = g;
    }
    loc += g;
  }
  const uint64_t inc = wave_scan_u64(loc);
  uint64_t run = inc - loc;
  if constexpr (THREADS > 64) {
    if (lane == 63) wave_partials[wid] = inc;
    __syncthreads();
    for (int w = 0; w < wid; ++w) run += wave_partials[w];
  }
  for (int e = e0; e < e1; ++e) { run += P[e + 1]; P[e + 1] = run; }
  if constexpr (THREADS > 64) __syncthreads();
}
template <class ShiftOf>
GJX_DEV void prefix_in_place_wave(uint64_t* P, int n, ShiftOf shift_of) { prefix_in_place<64>(P, n, nullptr, shift_of); }

// Inclusive prefix of val(0) .. val(n - 1) by ONE block of 1024 threads, 1024 entries per pass (any n): out(b, prefix) for every entry,
// the total returned in every thread.  wsum: 16 words of LDS.
template <class Val, class Out>
GJX_DEV uint64_t block_scan_chunked(int n, uint64_t* wsum, Val val, Out out) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (int b0 = 0; b0 < n; b0 += 1024) {
    const int b = b0 + threadIdx.x;
    const uint64_t inc = wave_scan_u64(b < n ? val(b) : 0ull);
    __syncthreads();
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    uint64_t base = carry, tot = 0;
    for (int w = 0; w < 16; ++w) { if (w < wid) base += wsum[w]; tot += wsum[w]; }
    if (b < n) out(b, base + inc);
    carry += tot;
  }
  return carry;
}

// Source tiles of ITEMS thresholds that do not decrease with the slot index: tile[k] = first tile t with P[t + 1] > T[k] = number of
// tiles whose inclusive prefix is <= T[k] (P[0 .. n]: the prefix, P[n] > T).  A block's slots draw from tiles near its own index
// (equal tile totals would make it exactly `own`): the nine boundaries of the eight tiles around `own` are read together (one
// LDS latency, the same addresses in every lane) and the tile of each slot is counted off.  Only a lane with a threshold outside
// that window descends: fixed trip count from the largest power of two <= n (nine dependent reads at n = 256), the first and the
// last slot together (independent reads per round); the slots between them are in the same tile unless the lane straddles a tile
// boundary (then they are searched too).
GJX_DEV int source_window_start(int n, int own) {   // first of the eight tiles around `own` (n < 8: all of them)
  return own - 4 < 0 ? 0 : (own - 4 > n - 8 ? (n - 8 < 0 ? 0 : n - 8) : own - 4);
}
template <int ITEMS>
GJX_DEV void source_tiles(const uint64_t* P, int n, int own, const uint64_t (&T)[ITEMS], int (&tile)[ITEMS]) {
  const int wlo = source_window_start(n, own);
  uint64_t Pw[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Pw[k] = P[wlo + k < n ? wlo + k : n];
  if (T[0] >= Pw[0] && T[ITEMS - 1] < Pw[8]) {
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      int tl = wlo;
#pragma unroll
      for (int w = 1; w < 8; ++w) tl += Pw[w] <= T[k] ? 1 : 0;
      tile[k] = tl;
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) tile[k] = 0;
  auto descend = [&](int k0, int k1) {
    for (int sft = 1 << (31 - __builtin_clz((unsigned)n)); sft >= 1; sft >>= 1) {
      const int pa = tile[k0] + sft, pb = tile[k1] + sft;       // P[probe] = inclusive prefix of tile probe - 1
      if (pa <= n - 1 && P[pa] <= T[k0]) tile[k0] = pa;
      if (k1 != k0 && pb <= n - 1 && P[pb] <= T[k1]) tile[k1] = pb;
    }
  };
  descend(0, ITEMS - 1);
  if constexpr (ITEMS > 2) {
    if (tile[0] == tile[ITEMS - 1]) {
#pragma unroll
      for (int k = 1; k < ITEMS - 1; ++k) tile[k] = tile[0];
    } else {
#pragma unroll
      for (int k = 1; k < ITEMS - 1; k += 2) descend(k, k + 1 < ITEMS - 1 ? k + 1 : k);
    }
  }
}
GJX_DEV int source_tile(const uint64_t* P, int n, int own, uint64_t T) {
  const uint64_t T1[1] = {T};
  int tile[1];
  source_tiles<1>(P, n, own, T1, tile);
  return tile[0];
}

// Ranks of N residuals in tiles of TILE inclusive cumulative weights: pos[k] = number of entries of cm[k] that are <= r[k] = the first
// particle whose cumulative weight exceeds it.  4-ary: three independent probes per level and slot, so the dependent chain is 5 LDS
// reads for 1024 entries instead of 10, and the probes of different slots are interleaved level by level.  The chain is not what a
// search costs a full CU, though: it is 15 8-byte reads per slot, the last three levels at scattered addresses, and 16 waves of
// four slots per lane keep the LDS busy for 2.3 - 2.5 us (k_resample_gather, K = 2^20) against 0.3 us of latency.  Callers with
// several slots per lane whose residuals do not decrease use rank_in_tiles_sorted (below), which searches once per lane.
template <int TILE, int N>
GJX_DEV void rank_in_tiles(const uint64_t* (&cm)[N], const uint64_t (&r)[N], int (&pos)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) pos[k] = 0;
#pragma unroll
  for (int q = TILE >> 2; q >= 1; q >>= 2) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const uint64_t pa = cm[k][pos[k] + q - 1], pb = cm[k][pos[k] + 2 * q - 1], pc = cm[k][pos[k] + 3 * q - 1];
      pos[k] += (pa <= r[k] ? q : 0) + (pb <= r[k] ? q : 0) + (pc <= r[k] ? q : 0);
    }
  }
}
template <int TILE>
GJX_DEV int rank_in_tile(const uint64_t* cm, uint64_t r) {
  const uint64_t* cm1[1] = {cm};
  const uint64_t r1[1] = {r};
  int pos[1];
  rank_in_tiles<TILE, 1>(cm1, r1, pos);
  return pos[0];
}
// The same ranks for the N > 1 slots of a lane when the residuals of slots that share a tile do not decrease with the slot index
// (consecutive comb thresholds): slot 0 is searched as above and anchors a window of kRankWalk entries, from the even index at or
// below its rank (16-byte reads; moved down where it would leave the tile), read ONCE for all the slots that follow in the same
// tile: pos[k] = window start + the number of its entries that are <= r[k].  Exact: every entry below the anchor's rank is <= the
// anchor's residual <= r[k] and the entries do not decrease, so those that are <= r[k] are a prefix of the window.  A window that
// is <= r[k] throughout and does not reach the tile's end says nothing about what follows: that slot is searched 4-ary and becomes
// the anchor of the slots behind it, as does a slot in another tile than the anchor's (a lane that straddles two source tiles).
// on[k] == false leaves slot k out (pos[k] = 0, nothing is read for it).  cm[k] 16-byte aligned.
// kRankWalk = 12: with the mixture model's weights at K = 2^20 (log-weights of sd 1.04; keys (0,1), (0,2), u = 0.37, 0.5) the fourth
// slot of a lane lies at most 14 entries above the even index below the first, and the share of waves (64 lanes x 4 slots) with a
// slot outside the window is 78 % for 8 entries, 0.4 - 0.55 % for 12, none for 16: 12 is the smallest below 1 %.  (Consecutive
// slots are at most 8 apart: a window per slot, anchored at its predecessor, needs 8 entries for the same share — 0.15 - 0.35 % —
// which is twice the reads for three slots and three dependent reads instead of one.)
constexpr int kRankWalk = 12;
template <int TILE, int N>
GJX_DEV void rank_in_tiles_sorted(const uint64_t* (&cm)[N], const uint64_t (&r)[N], const bool (&on)[N], int (&pos)[N]) {
  typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
  constexpr int W = kRankWalk;
  static_assert(N > 1 && W % 2 == 0 && W <= TILE && TILE % 2 == 0, "an even window inside the tile");
  const uint64_t* acm = cm[0];        // the anchor: its tile, whether it has one, its window
  bool aon = on[0];
  int base = 0;
  u64x2 win[W / 2] = {};
  auto anchor_at = [&](int at) {      // (at <= TILE: the reads stay inside the tile)
    const int even = at & ~1;
    base = even > TILE - W ? TILE - W : even;
#pragma unroll
    for (int j = 0; j < W / 2; ++j) win[j] = ((const u64x2*)(acm + base))[j];
  };
  pos[0] = 0;
  if (on[0]) {
    pos[0] = rank_in_tile<TILE>(cm[0], r[0]);
    anchor_at(pos[0]);
  }
#pragma unroll
  for (int k = 1; k < N; ++k) {
    bool full = on[k];
    pos[k] = 0;
    if (on[k] && aon && cm[k] == acm) {
      int cnt = 0;
#pragma unroll
      for (int j = 0; j < W / 2; ++j) cnt += (win[j].x <= r[k] ? 1 : 0) + (win[j].y <= r[k] ? 1 : 0);
      pos[k] = base + cnt;
      full = cnt == W && base + W < TILE;
    }
    if (full) {
      pos[k] = rank_in_tile<TILE>(cm[k], r[k]);
      if (k + 1 < N) { acm = cm[k]; aon = true; anchor_at(pos[k]); }
    }
  }
}
template <int TILE, int N>
GJX_DEV void rank_in_tiles_sorted(const uint64_t* (&cm)[N], const uint64_t (&r)[N], int (&pos)[N]) {
  bool on[N];
#pragma unroll
  for (int k = 0; k < N; ++k) on[k] = true;
  rank_in_tiles_sorted<TILE, N>(cm, r, on, pos);
}

// One round of the re-scan: the inclusive cumulative fixed-point weights of up to THREADS / 64 / (TILE / (64 ITEMS)) * CPT source tiles,
// each RELATIVE to its tile's start, into cum[tl TILE + i] (tl: the tile's index in the round).  TILE / (64 ITEMS) waves share a
// tile, 64 ITEMS particles each, and a wave takes CPT tiles: 256 threads x CPT = 3 is the form of the one-tile-per-block kernels (three
// independent DPP chains per wave), 1024 threads x CPT = 1 four tiles by four waves each.  fill(tl, o, q) gives the ITEMS fixed-point
// weights from offset o of tile tl — how they are loaded (plain, agent or system scope, peer-mapped, from registers) and quantised
// (weight_q, tile_q) is the caller's — or returns false for a tile the round leaves out (wave-uniform; its part of cum is not
// written).  wtot: LDS for the waves' totals [tiles of a round][waves per tile]; mid() runs between the barrier behind them and the
// stores to cum (verify mode).  Every thread calls it; ends in a barrier.  The caller's barrier keeps a round from overwriting a cum
// that is still being searched.
template <int THREADS, int TILE, int ITEMS, int CPT, class Fill, class Mid>
GJX_DEV void rescan_round(uint64_t* cum, uint64_t* wtot, Fill fill, Mid mid) {
  constexpr int WPT = TILE / (64 * ITEMS), NW = THREADS / 64;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int tl0 = NW == WPT ? 0 : (wid / WPT) * CPT, part = NW == WPT ? wid : wid % WPT, o = (part * 64 + lane) * ITEMS;
  uint64_t qi[CPT][ITEMS], sacc[CPT], inc[CPT];
  bool on[CPT];
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    uint64_t q[ITEMS];
    sacc[c] = 0; inc[c] = 0;
    on[c] = fill(tl0 + c, o, q);
    if (!on[c]) continue;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) { sacc[c] += q[k]; qi[c][k] = sacc[c]; }
  }
#pragma unroll
  for (int c = 0; c < CPT; ++c) if (on[c]) inc[c] = wave_scan_u64(sacc[c]);
  if constexpr (WPT > 1) {
    if (lane == 63) {
#pragma unroll
      for (int c = 0; c < CPT; ++c) if (on[c]) wtot[(tl0 + c) * WPT + part] = inc[c];   // the wave's total: offset of the next part
    }
    __syncthreads();
  }
  mid();
#pragma unroll
  for (int c = 0; c < CPT; ++c) {
    if (!on[c]) continue;
    uint64_t base = inc[c] - sacc[c];
    if constexpr (WPT > 1) for (int w = 0; w < part; ++w) base += wtot[(tl0 + c) * WPT + w];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) cum[(tl0 + c) * TILE + o + k] = base + qi[c][k];
  }
  __syncthreads();
}

// Ancestor of threshold T from the arrays the three-launch resamplers leave in memory (k_tiled_quantise, k_tiled_plan): prefix P of the
// shifted tile totals, the shifts sh, the in-tile cumulative fixed-point weights cq — two binary searches.
GJX_DEV int64_t tiled_lookup(const uint64_t* P, const int32_t* sh, const uint64_t* cq, int nt, int64_t K, uint64_t T) {
  int lo = 0, hi = nt - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (P[mid + 1] > T) hi = mid; else lo = mid + 1;
  }
  const uint64_t r = (T - P[lo]) << sh[lo];
  const uint64_t* cm = cq + (int64_t)lo * kTileQ;
  const int64_t left = K - (int64_t)lo * kTileQ;
  int l2 = 0, h2 = (int)(left < kTileQ ? left : kTileQ) - 1;
  while (l2 < h2) {
    const int mid = (l2 + h2) >> 1;
    if (cm[mid] > r) h2 = mid; else l2 = mid + 1;
  }
  return (int64_t)lo * kTileQ + l2;
}

// ---- the search of the tile-scaled systematic resampler for ONE tile of 1024 output slots (include/gjx.h,
// GJX_WEIGHTS_TILE_SCALED): lane t of a 256-thread block owns the slots tix 1024 + 4 t .. + 3 and gets their ancestors.
// Shared by k_resample_gather_tiled (gjx_resample.hip) and by generated step kernels that resample in their prologue
// (gjx_codegen.hip, gjx_run_resample): ONE body, hence the same ancestors bit for bit.  x: log-weights; S, E: {S_b, e_b} of
// every tile; !PLANNED: Pl [nt + 2], Ebl [nt] are block-shared scratch (every block reduces all nt totals), PLANNED: Pg, shg
// hold the prefix and the shifts (k_tiled_plan).  tix == 0 also finishes the LSE record of the producing run (lse_mode 2) and
// flags a dead collection.  Every thread of the block must call it (block barriers inside).
struct TiledSearchShared {
  float fred[8];
  uint64_t wsum[4];
  alignas(16) uint64_t cumL[3 * 1024];                         // cumulative q of the tiles being searched, relative to the tile's start (16-byte reads)
  uint64_t s_wtot[3][4];
  int s_range[2];
};

// LIVE: the collection being resampled was written by other blocks of THIS launch (the steps kernel of a generated filter,
// gjx_codegen.hip): S holds one tagged granule {rtag, e_b, S_b} per tile (tile_granule), published by its block once the block's
// write-through stores of the step had completed; this block polls them — the rendezvous of the step — and reads everything else
// of the previous step (log-weights, block pairs) with agent-scope loads.  E is unused.
template <bool PLANNED, bool LIVE = false>
GJX_DEV void tiled_search_tile(const float* __restrict__ x, int64_t K, const uint64_t* __restrict__ S, const int32_t* __restrict__ E,
                               const uint64_t* __restrict__ Pg, const int32_t* __restrict__ shg, const int nt, const int tix, uint64_t* const Pl,
                               int32_t* const Ebl, TiledSearchShared& sh, int lse_mode, const float* lse, int n_partials, float* lse_out,
                               float log_k_total, double u, unsigned* ctrl, unsigned long long* timeline, int32_t (&anc)[4],
                               unsigned long long rtag = 0ull) {
  static_assert(!(PLANNED && LIVE), "the live form reduces the granules itself");
#define GJX_STAMP(n) do { if (timeline && threadIdx.x == 0) timeline[tix * 8 + (n)] = __builtin_amdgcn_s_memrealtime(); } while (0)
  constexpr int ITEMS = 4, TILE = 256 * ITEMS, CH = 3;
  const uint64_t* const P = PLANNED ? Pg : Pl;
  const int32_t* const Eb = PLANNED ? E : Ebl;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t i0 = ((int64_t)tix * 256 + threadIdx.x) * ITEMS;
  auto load_tile = [&](int64_t p0, float (&v)[ITEMS]) {
    if constexpr (LIVE) {
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) v[k] = (p0 + k < K) ? load_agent(x + p0 + k) : -INFINITY;
    } else if (p0 + 4 <= K) {
      const float4 q4 = *(const float4*)(x + p0);
      v[0] = q4.x; v[1] = q4.y; v[2] = q4.z; v[3] = q4.w;
    } else {
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) v[k] = (p0 + k < K) ? x[p0 + k] : -INFINITY;
    }
  };
  // ---- every load of the head, at once: the three tiles of log-weights around the block, all tile totals (LIVE: the granules
  //      first — a tile's log-weights are complete only once its granule is there) ----
  const int w0 = tix - 1;
  float xw[CH][ITEMS];
  auto load_window = [&]() {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) xw[c][k] = -INFINITY;
      const int tc = w0 + c;
      if (tc >= 0 && tc < nt) load_tile((int64_t)tc * TILE + (int64_t)threadIdx.x * ITEMS, xw[c]);
    }
  };
  if constexpr (!LIVE) load_window();
  int Emax = 0;
  if constexpr (!PLANNED) {
  float em = (float)kTileDead;
  if constexpr (LIVE) {
    unsigned budget = (ctrl && (__hip_atomic_load(&ctrl[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kStatusPollTimeout)) ? 0u : kPollBudget;
    for (int b = threadIdx.x; b < nt; b += 256) {
      unsigned long long v = __hip_atomic_load((const unsigned long long*)&S[(size_t)b * kGranulePad], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      while ((v >> 60) != rtag && budget) {
        --budget;
        __builtin_amdgcn_s_sleep(1);
        v = __hip_atomic_load((const unsigned long long*)&S[(size_t)b * kGranulePad], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      if ((v >> 60) != rtag) { if (ctrl) __hip_atomic_fetch_or(&ctrl[2], kStatusPollTimeout, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); v = 0; }
      uint64_t sv;
      int e;
      tile_granule_unpack(v, sv, e);
      Pl[b + 1] = sv;
      Ebl[b] = e;
      em = fmaxf(em, (float)e);
    }
    __syncthreads();        // every granule of the step has been seen by some lane of this block: the whole previous step is readable
    load_window();
  } else {
  for (int b = threadIdx.x; b < nt; b += 256) {
    const uint64_t sv = S[b];
    const int e = sv ? E[b] : kTileDead;
    Pl[b + 1] = sv;
    Ebl[b] = e;
    em = fmaxf(em, (float)e);
  }
  }
  em = wave_max(em);
  if (lane == 0) sh.fred[wid] = em;
  if (threadIdx.x == 0) Pl[0] = 0;
  __syncthreads();
  Emax = (int)fmaxf(fmaxf(sh.fred[0], sh.fred[1]), fmaxf(sh.fred[2], sh.fred[3]));
  GJX_STAMP(1);
  prefix_in_place<256>(Pl, nt, sh.wsum, [&](int b) { return Emax - Ebl[b]; });
  }
  auto shift_of = [&](int t) { return PLANNED ? shg[t] : Emax - Eb[t]; };   // (a tile shifted out entirely is never a source)
  const uint64_t total = P[nt];
  GJX_STAMP(2);
  if (tix == 0) {   // block-uniform: the LSE record of the producing run (its block partials), the dead-collection flag
    if (lse_mode == 2 && lse_out) {
      float sm_sum;
      const float mx = LIVE ? block_ref_max_live(lse, n_partials, sh.fred, &sm_sum) : block_ref_max(2, lse, n_partials, sh.fred, &sm_sum);
      if (threadIdx.x == 0) {
        const float l = mx > -INFINITY ? mx + logf(sm_sum) : -INFINITY;
        lse_out[0] = mx; lse_out[1] = sm_sum; lse_out[2] = l; lse_out[3] = l - log_k_total;
      }
    }
    if (threadIdx.x == 0 && total == 0 && ctrl) __hip_atomic_fetch_or(&ctrl[2], kStatusZeroTotal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
#pragma unroll
  for (int k = 0; k < ITEMS; ++k) anc[k] = (int32_t)((i0 + k < K) ? i0 + k : K - 1);   // dead collection: identity (flagged)
  if (total > 0) {   // block-uniform
    const double step = (double)total / (double)K;
    uint64_t T[ITEMS];
    int tile[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
      const int64_t j = (i0 + k < K) ? i0 + k : K - 1;
      T[k] = comb_threshold(j, u, step, total);
    }
    source_tiles<ITEMS>(P, nt, tix, T, tile);
    // residual of every slot in its source tile's own units (< S of that tile)
    uint64_t Tr[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) Tr[k] = (T[k] - P[tile[k]]) << shift_of(tile[k]);
    if (threadIdx.x == 0) sh.s_range[0] = tile[0];
    if (threadIdx.x == 255) sh.s_range[1] = tile[ITEMS - 1];
    __syncthreads();
    const int tmin = sh.s_range[0], tmax = sh.s_range[1];
    GJX_STAMP(3);
    const bool windowed = tmin >= w0 && tmax <= w0 + 2;       // block-uniform: every source tile is among the three loaded at the top
    if (windowed) {
      // cumulative q of the window tiles the slots fall into (usually two), each against its own exponent: sh.cumL[c] for tile w0 + c
      // (the log-weights beyond K are -inf: they quantise to 0)
      rescan_round<256, TILE, ITEMS, CH>(sh.cumL, &sh.s_wtot[0][0], [&](int c, int, uint64_t (&q)[ITEMS]) {
        const int tc = w0 + c;
        if (tc < tmin || tc > tmax) return false;                 // block-uniform
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) q[k] = tile_q(xw[c][k], Eb[tc]);
        return true;
      }, [] {});
      const uint64_t* cm[ITEMS];
      int pos[ITEMS];
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) cm[k] = sh.cumL + (tile[k] - w0) * TILE;
      rank_in_tiles_sorted<TILE, ITEMS>(cm, Tr, pos);          // (the residuals of slots in one tile do not decrease: same start, same shift)
#pragma unroll
      for (int k = 0; k < ITEMS; ++k) anc[k] = (int32_t)((int64_t)tile[k] * TILE + pos[k]);
    } else {
      // collapsed or strongly drifting weights: re-scan the source tiles CH at a time (tiles without weight are skipped)
      const int ntiles = tmax - tmin + 1;
      auto next_live = [&](int at) { while (at < ntiles && P[tmin + at + 1] == P[tmin + at]) ++at; return at; };
      for (int idx = 0; idx < ntiles;) {
        const int nidx = next_live(idx + CH);
        __syncthreads();         // every lane is done searching the previous contents of sh.cumL
        rescan_round<256, TILE, ITEMS, CH>(sh.cumL, &sh.s_wtot[0][0], [&](int c, int o, uint64_t (&q)[ITEMS]) {
          if (idx + c >= ntiles) return false;
          const int tsrc = tmin + idx + c;
          float nv[ITEMS];
          load_tile((int64_t)tsrc * TILE + o, nv);
#pragma unroll
          for (int k = 0; k < ITEMS; ++k) q[k] = tile_q(nv[k], Eb[tsrc]);
          return true;
        }, [] {});
        const uint64_t* cm[ITEMS];
        bool mine[ITEMS];
        int pos[ITEMS];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
          const int kp = tile[k] - tmin;
          mine[k] = kp >= idx && kp < idx + CH;
          cm[k] = sh.cumL + (mine[k] ? (kp - idx) * TILE : 0);   // (a slot of another round is left out)
        }
        rank_in_tiles_sorted<TILE, ITEMS>(cm, Tr, mine, pos);
#pragma unroll
        for (int k = 0; k < ITEMS; ++k)
          if (mine[k]) anc[k] = (int32_t)((int64_t)tile[k] * TILE + pos[k]);
        idx = nidx;
      }
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) anc[k] = anc[k] < K ? anc[k] : (int32_t)(K - 1);
  }
#undef GJX_STAMP
}

}  // namespace gjx
