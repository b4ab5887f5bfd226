// gjx_pfilter_host.h — what the host code of the one-launch particle filters shares.  Each of them is pf_core (gjx_pfcore.h) with a model:
// its launcher fills a PfCoreArgs — here, once: pf_core_single from a PfRegion (the skeleton's area in a one-GPU workspace), pf_core_peer
// from a rank's gjx_peer_ctx — and adds the model's own arguments.  The launchers: pf_filter_launch (gjx_ssm.hip) and filter_peer
// (gjx_peer.hip) for the hand-written model (PfArgs, k_pf_persistent in gjx_pfilter.inl; pf_plan picks its kernel and grid), run_wide
// (gjx_scanfilter.hip) and scan_filter_peer_impl (gjx_peer.hip) for the kernels generated from a step program; their common steps —
// pf_step_keys, pf_pick_tiles, pf_us_words, pf_upload_steps — are here too.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/gjx.h"
#include "gjx_host.h"
#include "gjx_pfcore.h"

// a rank of a collection sharded over the GPUs of a node (created, connected and destroyed in gjx_peer.hip)
struct gjx_peer_ctx {
  int world = 0, rank = 0, rows = 0, share = 1;
  int64_t K = 0;                       // particles per rank
  int nt = 0, NT = 0;                  // quantisation tiles per rank / in total
  char* data = nullptr;                // this rank's DATA window
  char* flag = nullptr;                // this rank's FLAG window
  size_t data_bytes = 0, flag_bytes = 0;
  size_t off_rows[2] = {0, 0}, off_lw[2] = {0, 0}, off_m[2] = {0, 0};   // off_m: transition means of the resample-move filter
  size_t off_chk[2] = {0, 0};          // verify mode: one check word per particle row (u32[K], ping-pong like the rows)
  bool verify = false;                 // GJX_PEER_VERIFY=1 when the context was created
  bool verify_fault = false;           // GJX_PEER_VERIFY_FAULT=<this rank>: publish wrong check words (test hook)
  bool data_fine = false;              // DATA window in fine-grained memory (GJX_PEER_DATA=fine)
  size_t off_region[2] = {0, 0}, region_bytes = 0;
  // inside a flag region
  size_t r_aggA = 0, r_aggB = 0, r_bsum = 0, r_bmax = 0, r_ready = 0, r_gmm = 0;
  char* peer_data[GJX_MAX_RANKS];
  char* peer_flag[GJX_MAX_RANKS];
  long long* delta_dev = nullptr;      // [2][world]: byte distance to rank g's data window, then to its flag window
  bool connected = false;
  uint64_t n_filter = 0, n_gmm = 0;    // launches so far (select the flag region / the tags)
  double* us_dev = nullptr;
  uint32_t* keys_dev = nullptr;
  int t_cap = 0;
};

namespace gjx {

constexpr int kPfHostThreads = kPfCoreThreads;
constexpr int kPfHostMaxTiles = 4096;                    // quantisation tiles over all ranks (K_total <= 2^22)

struct PfArgs {
  PfCoreArgs core;
  const float* A; const float* H; const float* ys;       // ys [T][dy]
  float q, r;
  int dy;
  float* x_a; float* x_b;                                // [DX][K] ping-pong: step t writes x_b when t is odd
  // resample-move rejuvenation (MOVE kernels; requests/rejuvenate.py:70-94, k_ssm_step<.., MOVE>): after the ancestor gather
  // every particle takes n_moves random-walk Metropolis steps that leave p(x_{t-1} | parent, y_{t-1}) invariant
  float* m_a; float* m_b;                                // [DX][K] ping-pong like x: A x'_{t-1}, the mean step t propagated from
  float q0;                                              // prior scale (the transition that produced x_0)
  int n_moves;
  float move_scale;
  unsigned long long* acc_total;                         // [1] accepted moves of this rank's particles over the launch (or NULL)
};

// dynamic LDS of k_pf_persistent for NT tiles: prefix [NT + 1] u64 (padded to even), cumulative q [4][1024] u64, exponents [NT] i32
inline size_t pf_host_dyn_lds(int NT) { return 8 * (size_t)((NT + 2) & ~1) + 8 * (size_t)(kPfCoreThreads / 256) * kPfCoreThreads + 4 * (size_t)NT; }

struct PfPlan {
  const void* fn;    // kernel
  int spl;           // tiles per block
  int grid;          // blocks
  int nt;            // tiles of this rank
  size_t lds;        // dynamic LDS bytes
};
// Picks the smallest number of tiles per block whose grid is co-resident on the current device (`share` ranks on one
// device split its capacity: dry runs).  GJX_EUNSUPPORTED when the shape does not fit this kernel.
int pf_plan(int rng_mode, int dx, int dy, int64_t K_local, int n_ranks, int share, PfPlan* out, bool move = false);
void host_threefry2x32(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t out[2]);   // gjx_host_threefry2x32 as two words
void pf_step_keys(uint32_t key0, uint32_t key1, int T, std::vector<uint32_t>& keys, std::vector<double>& us);
// the same, and the resampling key k_res of every step ([T][2]): multinomial resampling draws one uniform per slot from it
void pf_step_keys_res(uint32_t key0, uint32_t key1, int T, std::vector<uint32_t>& keys, std::vector<double>& us, std::vector<uint32_t>& res_keys);

// ---- the skeleton's area in a workspace of ONE GPU, at `base` (nt tiles, `grid` blocks, T steps):
//      [256 B control][aggA 64 nt][aggB 64 nt][bsum 12 nt][bmax 12 nt][ready 4 grid, padded to 8][us 8 T][keys 8 T]([tabs 8 T]) ----
struct PfRegion {
  int nt;
  unsigned* ctrl;                                        // control block words: [0] epoch, [2] status
  unsigned long long* aggA; unsigned long long* aggB; float* bsum; float* bmax; unsigned* ready;
  double* us; uint32_t* keys; const float** tabs;        // per-step arrays (pf_upload_steps)
  size_t clear_bytes;                                    // from aggA: granules, ring and `ready` words — zero before a launch (no stale granule may pass)
  size_t bytes;                                          // what a caller must have at `base`: 8 bytes per block and 64 spare (a bound, not the end of tabs)
};
PfRegion pf_region(char* base, int64_t nt, int64_t grid, int T, bool with_tabs);

// ---- PfCoreArgs, zeroed and filled.  The launcher then sets what is its own: ancestors_all, timeline. ----
PfCoreArgs pf_core_single(int T, int64_t K, const PfRegion& rg, float* lw_even, float* lw_odd, float* lse_steps, int32_t* ancestors);
// ... of this rank of a sharded collection: the log-weights of the DATA window, the next flag region (consecutive launches alternate;
// this call advances the context's launch count), the context's step-key scratch
PfCoreArgs pf_core_peer(int T, gjx_peer_ctx* c, float* lse_steps, int32_t* ancestors);

// The smallest number of tiles per block whose grid g = ceil(nt / spl) is co-resident: g <= max_grid, g <= blocks_of(spl) / share (ranks
// that share one device — dry runs — split its capacity), g * world <= kPfHostMaxTiles `ready` words; {0, 0}: none.  blocks_of(spl) <= 0:
// no such kernel (the reason is in gjx_last_error).  It is asked only for a geometry that could fit: a generated kernel is compiled for it.
struct PfGeometry { int spl, grid; };
template <class BlocksOf>
PfGeometry pf_pick_tiles(int64_t nt, int world, int share, int64_t max_grid, BlocksOf&& blocks_of) {
  const int spls[5] = {1, 2, 4, 8, 16};
  for (int i = 0; i < 5; ++i) {
    const int64_t g = (nt + spls[i] - 1) / spls[i];
    if (g > max_grid) continue;
    int cap = blocks_of(spls[i]);
    if (cap <= 0) break;
    if (share > 1) cap /= share;
    if (g <= cap && g * world <= kPfHostMaxTiles) return {spls[i], (int)g};
  }
  return {0, 0};
}

// what a filter kernel reads as f.us: the comb offsets, or — multinomial: the sorted-uniform resampler takes the resampling KEY of a step
// where the comb takes its offset — the key's two words as one 64-bit pattern
std::vector<double> pf_us_words(const std::vector<double>& us, const std::vector<uint32_t>& res_keys, bool multinomial);
// the per-step arrays of a launch -> device (upload_words: nothing on the host has to outlive the call): us, keys, then — tabs_dev not
// NULL — the tables of the step programs (pf_upload_tabs)
int pf_upload_steps(double* us_dev, const std::vector<double>& us, uint32_t* keys_dev, const std::vector<uint32_t>& keys, const float** tabs_dev,
                    const gjx_program* steps, int T, hipStream_t st);
int pf_upload_tabs(const float** tabs_dev, const gjx_program* steps, int T, hipStream_t st);

}  // namespace gjx
