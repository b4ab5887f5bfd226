// gjx_scanfilter.hip — bootstrap filter for ANY Scan kernel (gjx_scan_filter): the step recursion of Scan.generate
// (combinators/scan.py:237-294: step t receives the carry of step t-1, weights add over steps) with systematic resampling in
// front of every step.  Host code only.  scan_filter_impl is the sequence filter_begin (refusals; FilterLayout, the ONE carving of
// the workspace) -> run_wide -> the step loop (-> run_steps_tail) -> last record; the workspace's size and the options select the form:
//   WIDE        step 0, then steps 1 .. T-1 in ONE launch of the filter kernel generated for the step program (gjx_gen_pf on the skeleton
//               of gjx_pfcore.h; its arguments and workspace area come from gjx_pfilter_host.h)
//   PER_STEP    one launch per step: the step's generated kernel resamples in its prologue (gjx_run_resample: 4 particles per lane, K a
//               multiple of 1024 up to 2^20 — every block searches the ancestors of its own tile from the previous step's log-weights
//               and tile totals, which therefore alternate between two buffers / two run workspaces)
//   STEPS       PER_STEP for steps 0 and 1, then steps 2 .. T-1 in ONE launch of the steps kernel (gjx_gen_steps)
//   TWO_LAUNCH  per step the resampling as launches of its own (resample_before_step: the tile-scaled search, which reads 4 B per particle,
//               writes 4 B and finishes the LSE record of step t-1; or the multinomial / the gated adaptive resampler; an HMC move behind
//               it) and the step's propagate + reweight kernel, whose GJX_MODE_INPUT sites read the carry through the ancestors — the
//               gather is fused into the read side, the resampled collection is never materialised
// The hand-written linear-Gaussian filters (gjx_ssm.hip, gjx_pfilter.inl) stay the fast path for that one model.
#include <math.h>
#include <string.h>

#include <vector>

#include "gjx_device.h"
#include "gjx_host.h"
#include "gjx_tile.h"
#include "gjx_pfcore.h"
#include "gjx_pfilter_host.h"

using namespace gjx;

static __global__ void k_clear_status(unsigned* ctrl) { if (threadIdx.x == 0) ctrl[2] = 0u; }
// accepted chains of one HMC move (gjx_hmc's flags f32[K]) added to the run's counter
// (a grid-stride loop over at most 64 blocks, ONE atomic per block: a wave-level atomic per 64 chains — 1024 of them on one address at
// K = 2^16 — took 13 us, four times the HMC kernel it counts for; rocprofv3, profiles/r06_moves_kernel_stats.csv)
static __global__ __launch_bounds__(256) void k_count_flags(const float* flags, int64_t K, unsigned long long* total) {
  __shared__ unsigned wcount[4];
  unsigned n = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < K; i += (int64_t)gridDim.x * 256) n += flags[i] > 0.5f ? 1u : 0u;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) n += __shfl_xor(n, off, 64);
  if ((threadIdx.x & 63) == 0) wcount[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    if (t) atomicAdd(total, (unsigned long long)t);
  }
}

static __global__ void k_merge_status(unsigned* from, unsigned* to) { if (threadIdx.x == 0 && from[2]) { atomicOr(&to[2], from[2]); from[2] = 0u; } }

// tile totals {S_b, e_b} and block pairs of a step that ran as its own launch -> the tagged granules and the pair array the steps
// kernel's first step polls / reads (gjx_gen_steps)
__global__ void k_tiles_to_granules(const uint64_t* __restrict__ S, const int32_t* __restrict__ E, const unsigned long long* __restrict__ pairs,
                                    unsigned long long* gran, unsigned long long* part, int nt, unsigned long long tag) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= nt) return;
  const uint64_t sv = S[b];
  gran[(size_t)b * kGranulePad] = tile_granule(tag, sv ? E[b] : kTileDead, sv);
  part[b] = pairs[b];
}

// what one call was given, and what every form derives from it once
struct FilterCall {
  const gjx_program* steps; int32_t T; int64_t K;
  float* logw; int32_t* ancestors; int32_t* ancestors_all; float* lse_steps;
  void* workspace; size_t workspace_bytes; void* stream;
  const gjx_filter_opts* opts; const gjx_adaptive_opts* ad;      // ad: gjx_scan_filter_adaptive (checked by adaptive_check), or NULL
  int32_t flags; int n_moves;                                    // of opts
  // key discipline of inference/pf.py: k_t = fold_in(k_{t-1}, t) (scan.py:268); (k_prop, k_res) = split(k_t); comb offset = uniform(k_res)
  std::vector<uint32_t> keys, res_keys; std::vector<double> us;
  hipStream_t st() const { return (hipStream_t)stream; }
  bool has(int32_t flag) const { return (flags & flag) != 0; }
  const gjx_program* hmc_targets() const { return opts ? opts->hmc_targets : nullptr; }
  // the resampling is launches of its own: asked for, or an HMC move / a device-side decision sits between it and the step
  bool plain_resampling() const { return has(GJX_FILTER_TWO_LAUNCH) || hmc_targets() != nullptr || ad != nullptr; }
  // GJX_FILTER_ABSOLUTE_INPUTS: an INPUT site's obs_off is the row of the previous step's WHOLE buffer (carried statics are read from
  // its INPUT rows, the carry from its own rows); otherwise the row among the previous step's own rows, which sit behind its inputs
  int in_base(const gjx_program& p) const { return has(GJX_FILTER_ABSOLUTE_INPUTS) ? 0 : input_rows(p); }
  int forced_blocks() const { return (opts && opts->coresident_blocks > 0) ? opts->coresident_blocks : 0; }   // instead of the occupancy answer
};

// the workspace of a call: [run OP_RUN][resample OP_RESAMPLE] | [run2 OP_RUN][logw2 4 K, at 256] [area, at 256] — the part behind the bar
// only where it fits (`room`) — or, multinomial: [run][resample][mn_cum 8 K + 256, at 256]
struct FilterLayout {
  int T; float* logw;
  size_t need_run, need_res;
  char* ws_run; char* ws_res; char* ws_run2; float* logw2;   // (ws_run2, logw2: the one-launch step alternates between two of each)
  char* area; size_t area_bytes;          // what a one-launch form (WIDE, STEPS) carves its granules and per-step arrays from
  uint64_t* mn_cum;                       // multinomial resampling as launches of its own: prefix sums of the fixed-point weights
  bool room, fused;                       // fused: steps resample in their kernel's prologue (until one cannot: the rest runs in the two-launch form)
  // fused: step t writes the log-weights / block pairs / tile totals of parity (T - 1 - t) & 1, so that the last step's land in `logw`
  // and in the first run workspace; the two-launch form uses one buffer throughout
  bool odd(int t) const { return fused && ((T - 1 - t) & 1); }
  float* lw_of(int t) const { return odd(t) ? logw2 : logw; }
  char* ws_of(int t) const { return odd(t) ? ws_run2 : ws_run; }
};

template <class Args, class RowsOf>
static void set_rows(Args& g, RowsOf& rows_of, int T) {     // two alternating buffers, or one per step when the run is recorded
  float* r0 = rows_of(0); float* r1 = rows_of(1);
  if (T == 2 || rows_of(2) == r0) { g.rows_a = r0; g.rows_b = r1; g.rows_all = nullptr; g.rows_step = 0; }
  else { g.rows_a = nullptr; g.rows_b = nullptr; g.rows_all = r0; g.rows_step = (int64_t)(r1 - r0); }
}

// the refusals that do not depend on the form, the layout of the workspace, the status word of THIS call, the step keys
static int filter_begin(FilterCall& a, uint32_t key0, uint32_t key1, FilterLayout& L) {
  const int64_t K = a.K;
  L.T = a.T; L.logw = a.logw;
  L.need_run = gjx_workspace_bytes(GJX_OP_RUN, K); L.need_res = gjx_workspace_bytes(GJX_OP_RESAMPLE, K);
  if (!a.workspace || a.workspace_bytes < L.need_run + L.need_res) return gjx_fail(GJX_EWORKSPACE, "gjx_scan_filter: workspace too small (OP_RUN + OP_RESAMPLE)");
  L.ws_run = (char*)a.workspace; L.ws_res = L.ws_run + L.need_run;
  const size_t logw_off = (L.need_run + L.need_res + L.need_run + 255) & ~(size_t)255;
  const size_t area_off = (logw_off + sizeof(float) * (size_t)K + 255) & ~(size_t)255;
  L.room = a.workspace_bytes >= logw_off + sizeof(float) * (size_t)K;
  L.ws_run2 = L.room ? L.ws_res + L.need_res : nullptr;
  L.logw2 = L.room ? (float*)((char*)a.workspace + logw_off) : nullptr;
  L.area = (L.room && a.workspace_bytes >= area_off) ? (char*)a.workspace + area_off : nullptr;
  L.area_bytes = L.area ? a.workspace_bytes - area_off : 0;
  L.mn_cum = nullptr;
  // an HMC move behind every resampling (gjx_filter_opts::hmc_targets): the plain two-launch step with a gather and one gjx_hmc between them
  if (const gjx_program* hmc_t = a.hmc_targets()) {
    if (a.n_moves > 0 || a.has(GJX_FILTER_ABSOLUTE_INPUTS)) return gjx_fail(GJX_EUNSUPPORTED, "gjx_scan_filter: the HMC move runs without n_moves and without carried static inputs");
    if (!a.opts->hmc_rows || !a.opts->hmc_out || !a.opts->hmc_workspace || a.opts->hmc_L < 1 || !(a.opts->hmc_eps > 0.0f))
      return gjx_fail(GJX_EINVAL, "gjx_scan_filter: hmc_targets needs hmc_rows, hmc_out, hmc_workspace, hmc_L >= 1, hmc_eps > 0");
    for (int t = 0; t + 1 < a.T; ++t)
      if (hmc_t[t].n_slots != a.steps[t].n_slots || a.opts->hmc_workspace_bytes < gjx_hmc_workspace_bytes(&hmc_t[t], K))
        return gjx_fail(GJX_EINVAL, "gjx_scan_filter: hmc_targets[t] must have the rows of step t, and hmc_workspace must hold gjx_hmc_workspace_bytes of every target");
  }
  L.fused = L.room && !a.plain_resampling() && K % 1024 == 0 && K <= (1 << 20);
  // the status word describes THIS call (a stale time-out bit would end a one-launch form at its first step)
  hipLaunchKernelGGL(k_clear_status, dim3(1), dim3(64), 0, a.st(), (unsigned*)L.ws_res + 8);
  GJX_CHECK_LAUNCH("gjx_scan_filter(status word)");
  if (a.ad) {
    const hipError_t e = hipMemsetAsync(a.ad->resampled, 0, sizeof(int32_t), a.st());      // nothing is resampled in front of step 0
    if (e != hipSuccess) return gjx_fail_hip(e, "gjx_scan_filter_adaptive(resampled[0])");
  }
  if (L.fused && a.T > 1) {
    // the second run workspace's control block must be zero like the first one's (the caller zero-fills the workspace once; be safe)
    const hipError_t e = hipMemsetAsync(L.ws_run2, 0, kWsHeaderBytes, a.st());
    if (e != hipSuccess) return gjx_fail_hip(e, "gjx_scan_filter(workspace)");
  }
  pf_step_keys_res(key0, key1, a.T, a.keys, a.us, a.res_keys);
  if (a.has(GJX_FILTER_MULTINOMIAL)) {      // plain launches, the prefix sums of the fixed-point weights behind the workspace
    if (a.n_moves > 0) return gjx_fail(GJX_EUNSUPPORTED, "gjx_scan_filter: the rejuvenation move runs with systematic resampling (the one-launch filter kernel)");
    const size_t off = (L.need_run + L.need_res + 255) & ~(size_t)255;
    if (a.workspace_bytes < off + 8 * (size_t)K + 256) return gjx_fail(GJX_EWORKSPACE, "gjx_scan_filter: multinomial resampling needs 8 K + 256 bytes beyond OP_RUN + OP_RESAMPLE");
    L.mn_cum = (uint64_t*)((char*)a.workspace + off);
    L.fused = false;
  }
  if (a.has(GJX_FILTER_ABSOLUTE_INPUTS) && a.n_moves > 0) return gjx_fail(GJX_EUNSUPPORTED, "gjx_scan_filter: no rejuvenation move with carried static inputs (GJX_FILTER_ABSOLUTE_INPUTS)");
  return GJX_OK;
}

constexpr int kNotThisForm = 1;           // (no gjx_status) run_wide, run_steps_tail: nothing ran that the other forms would not repeat
// ---- GJX_FILTER_FORM_WIDE; any other return value than kNotThisForm ends the call ----
template <class RowsOf>
static int run_wide(const FilterCall& a, RowsOf& rows_of, const FilterLayout& L, gjx_filter_info& finfo) {
  const gjx_program* steps = a.steps;
  const int T = a.T;
  const int64_t K = a.K, ntw = (K + 1023) / 1024;
  const bool multinomial = a.has(GJX_FILTER_MULTINOMIAL);
  if (!L.room || T < 2 || (multinomial && a.n_moves > 0) || a.has(GJX_FILTER_NO_WIDE) || a.plain_resampling() || ntw > kPfHostMaxTiles ||
      !L.area || L.area_bytes < pf_region(L.area, ntw, ntw, T, true).bytes || gjx_plain_launches_forced() || !steps[1].tab_dev ||
      !gen_pf_supported(&steps[1]) || !(a.n_moves == 0 || gen_pf_moves_supported(&steps[1])))
    return kNotThisForm;
  if (!periodic_steps(steps, T, gen_pf_same_kernel) || (!a.has(GJX_FILTER_ABSOLUTE_INPUTS) && input_rows(steps[1]) > steps[0].n_slots - input_rows(steps[0])))
    return kNotThisForm;
  // the kernel flavour: with the rejuvenation move, or multinomial resampling by sorted uniforms (pf_core's MULTI)
  FilterVariant fv;
  fv.moves = a.n_moves > 0; fv.multinomial = multinomial;
  const size_t dyn = pf_core_dyn_lds((int)ntw, multinomial);
  const PfGeometry geo = pf_pick_tiles(ntw, 1, 1, 2 * 1024, [&](int tiles) {
    fv.tiles = tiles;
    return a.forced_blocks() ? a.forced_blocks() : gen_pf_resident_blocks(&steps[1], encode(fv), dyn);
  });
  if (!geo.spl) return kNotThisForm;
  // step 0 (no carry to read): its program's own kernel; log-weights where the skeleton expects those of step 0
  gjx_run_opts o;
  memset(&o, 0, sizeof(o));
  gjx_run_info info = {0, 0, 0};
  int rc = gjx_run_program_ex(&steps[0], a.keys[0], a.keys[1], K, 0, rows_of(0), nullptr, nullptr, ((T - 1) & 1) ? L.logw2 : a.logw, nullptr, nullptr, nullptr,
                              nullptr, K, L.ws_run, L.need_run, a.stream, &o, &info);
  if (rc) return rc;
  const PfRegion rg = pf_region(L.area, ntw, geo.grid, T, true);
  const hipError_t e = hipMemsetAsync(L.area, 0, kWsHeaderBytes + rg.clear_bytes, a.st());   // no stale granule may pass
  if (e != hipSuccess) return gjx_fail_hip(e, "gjx_scan_filter(workspace)");
  if (int rcu = pf_upload_steps(rg.us, pf_us_words(a.us, a.res_keys, multinomial), rg.keys, a.keys, rg.tabs, steps, T, a.st())) return rcu;
  GenPfArgs ga;
  memset(&ga, 0, sizeof(ga));
  ga.core = pf_core_single(T, K, rg, a.logw, L.logw2, a.lse_steps, a.ancestors_all ? nullptr : a.ancestors);
  ga.core.ancestors_all = a.ancestors_all;
  ga.core.timeline = (a.opts && a.opts->timeline && a.opts->timeline_bytes >= (int64_t)(128 * (size_t)geo.grid)) ? (unsigned long long*)a.opts->timeline : nullptr;
  ga.tabs = rg.tabs;
  set_rows(ga, rows_of, T);
  ga.in_row0_first = (int64_t)a.in_base(steps[0]) * K; ga.in_row0 = (int64_t)a.in_base(steps[1]) * K;
  ga.n_moves = a.n_moves; ga.move_scale = a.opts ? a.opts->move_scale : 0.0f;
  ga.acc_total = (a.opts && a.n_moves > 0) ? (unsigned long long*)a.opts->accepted_total : nullptr;
  if (ga.acc_total) {
    const hipError_t ez = hipMemsetAsync(ga.acc_total, 0, sizeof(unsigned long long), a.st());
    if (ez != hipSuccess) return gjx_fail_hip(ez, "gjx_scan_filter(accept counter)");
  }
  fv.tiles = geo.spl;
  rc = gen_pf_launch(&steps[1], encode(fv), ga, geo.grid, dyn, a.st());
  if (rc) return rc == GJX_EUNSUPPORTED ? kNotThisForm : rc;      // (unsupported: the kernel could not be launched)
  // the skeleton's status bits live in ITS control block: fold them into the word the caller reads
  hipLaunchKernelGGL(k_merge_status, dim3(1), dim3(64), 0, a.st(), rg.ctrl, (unsigned*)L.ws_res + 8);
  GJX_CHECK_LAUNCH("gjx_scan_filter(status)");
  finfo.form = GJX_FILTER_FORM_WIDE; finfo.launches = 2; finfo.grid = geo.grid; finfo.tiles_per_block = geo.spl;
  return GJX_OK;
}

// The resampling in front of step t (t >= 1): where the step's kernel can resample in its prologue, the step itself (*ran, `info`);
// otherwise launches of their own — the tile-scaled search, the multinomial resampler, or the gated search of the adaptive filter, and the
// HMC move — that leave in `o` what the step's plain launch reads its carry through
template <class RowsOf>
static int resample_before_step(const FilterCall& a, RowsOf& rows_of, FilterLayout& L, int t, const gjx_run_info& prev, gjx_run_opts& o,
                                gjx_run_info& info, gjx_filter_info& finfo, bool* ran) {
  const gjx_program* steps = a.steps;
  const int64_t K = a.K;
  if (!a.has(GJX_FILTER_ABSOLUTE_INPUTS) && input_rows(steps[t]) > steps[t - 1].n_slots - input_rows(steps[t - 1]))
    return gjx_fail(GJX_EINVAL, "gjx_scan_filter: a step reads more carry rows than the step before it produced");
  const float* in = rows_of(t - 1);
  const char* pws = L.ws_of(t - 1);
  const float* lw_prev = L.lw_of(t - 1);
  const float* pairs = (const float*)(pws + kWsHeaderBytes);          // block pairs {max, sumexp} of the previous step's launch
  const bool tiles = prev.tiles_offset != 0;
  const uint64_t* tS = tiles ? (const uint64_t*)(pws + prev.tiles_offset) : nullptr;
  const int32_t* tE = tiles ? (const int32_t*)(tS + (K / 1024)) : nullptr;
  int32_t* anc_t = a.ancestors_all ? a.ancestors_all + (size_t)(t - 1) * (size_t)K : a.ancestors;
  float* lse_prev = a.lse_steps + 4 * (size_t)(t - 1);
  o.in_rows = in + (size_t)a.in_base(steps[t - 1]) * (size_t)K;      // the rows the previous step's OWN sites wrote (abs_in: its whole buffer)
  o.in_stride = K;
  int rc;
  if (L.fused && tiles) {
    gjx_run_resample rs;
    memset(&rs, 0, sizeof(rs));
    rs.logw = lw_prev; rs.tile_S = tS; rs.tile_E = tE; rs.lse_partials = pairs; rs.n_partials = prev.n_partials;
    rs.lse_out = lse_prev; rs.u = a.us[t]; rs.ancestors_out = anc_t; rs.status_ws = L.ws_res;
    o.resample = &rs;
    rc = gjx_run_program_ex(&steps[t], a.keys[2 * t], a.keys[2 * t + 1], K, 0, rows_of(t), nullptr, nullptr, L.lw_of(t), nullptr, nullptr, nullptr, nullptr, K,
                            L.ws_of(t), L.need_run, a.stream, &o, &info);
    o.resample = nullptr;
    if (rc != GJX_OK && rc != GJX_EUNSUPPORTED) return rc;
    if (rc == GJX_OK) { *ran = true; return GJX_OK; }
  }
  // a step whose kernel cannot resample in its prologue: this step and the rest in the two-launch form, which writes one
  // buffer throughout (this step still reads what step t - 1 left where it left it)
  L.fused = false;
  if (L.mn_cum) {
    // the finished LSE record of step t - 1 from the run's block pairs (the prefix sums of this call are overwritten), then the draw
    rc = gjx_weight_cumsum(lw_prev, K, 2, pairs, prev.n_partials, L.mn_cum, L.mn_cum + K /* {0, total} */, lse_prev, K, L.ws_res, L.need_res, a.stream);
    if (rc) return rc;
    rc = gjx_resample_sorted_multinomial_tiled(lw_prev, K, a.res_keys[2 * t], a.res_keys[2 * t + 1], K, anc_t, L.mn_cum, nullptr, nullptr, L.ws_res, L.need_res, a.stream);
    finfo.launches += 5;
  } else if (a.ad) {
    // the gated search on the ACCUMULATED weights: their tile totals are recomputed (the producing kernel's describe inc_{t-1}),
    // the record of step t - 1 is already written; resampled[t] == 0: identity ancestors, nothing else touched
    rc = gjx::resample_gather_tiled_gated(a.ad->logw_acc, K, nullptr, nullptr, 0, nullptr, 0, a.us[t], nullptr, 0, 0, nullptr, 0, anc_t, nullptr, K,
                                          L.ws_res, L.need_res, a.stream, a.ad->resampled + t);
    finfo.launches += K > 1024 * 1024 ? 2 : 1;
  } else
    rc = gjx_resample_gather_tiled(lw_prev, K, tS, tE, 2, pairs, prev.n_partials, a.us[t], nullptr, 0, 0, nullptr, 0, anc_t, lse_prev, K, L.ws_res, L.need_res, a.stream);
  if (rc) return rc;
  o.in_ancestors = anc_t;
  if (!a.hmc_targets()) return GJX_OK;
  // the resampled particle of step t - 1 — [its ancestor's inputs | its latent choices] — gathered, moved, and handed to the step
  const gjx_filter_opts* opts = a.opts;
  const gjx_program& tg = opts->hmc_targets[t - 1];
  rc = gjx_gather_rows(in, K, anc_t, K, tg.n_slots, opts->hmc_rows, K, a.stream);
  if (rc) return rc;
  uint32_t k1[2], k2[2];
  host_threefry2x32(a.keys[2 * t], a.keys[2 * t + 1], 0u, 0x6d6f7665u, k1);
  host_threefry2x32(k1[0], k1[1], 0u, 0u, k2);
  rc = gjx_hmc(&tg, k2[0], k2[1], K, 0, opts->hmc_eps, opts->hmc_L, 0, 1, opts->hmc_rows, opts->hmc_out, opts->hmc_out + K, opts->hmc_out + 2 * (size_t)K,
               opts->hmc_workspace, opts->hmc_workspace_bytes, a.stream);
  if (rc) return rc;
  if (opts->accepted_total) {
    hipLaunchKernelGGL(k_count_flags, dim3((unsigned)((K + 255) / 256 < 64 ? (K + 255) / 256 : 64)), dim3(256), 0, a.st(), (const float*)(opts->hmc_out + 2 * (size_t)K), K,
                       (unsigned long long*)opts->accepted_total);
    GJX_CHECK_LAUNCH("gjx_scan_filter(accepted chains)");
  }
  o.in_rows = opts->hmc_rows + (size_t)input_rows(steps[t - 1]) * (size_t)K;
  o.in_ancestors = nullptr;
  o.flags |= GJX_RUN_STORE_INPUTS;
  finfo.launches += 3;
  return GJX_OK;
}

// ---- GJX_FILTER_FORM_STEPS: steps 2 .. T-1 in ONE launch (gjx_gen_steps) when step 1 ran with the search in its prologue (`info`), the
//      remaining step programs are the same kernel, the grid is co-resident and the workspace has the room; returns like run_wide ----
template <class RowsOf>
static int run_steps_tail(const FilterCall& a, RowsOf& rows_of, const FilterLayout& L, const gjx_run_info& info, gjx_filter_info& finfo) {
  const gjx_program* steps = a.steps;
  const int T = a.T;
  const int64_t K = a.K, nt = K / 1024;
  const size_t area_need = (16 * (size_t)kGranulePad + 16) * (size_t)nt + 24 * (size_t)T + 64;   // granules, pair arrays, per-step arguments
  if (T < 4 || !L.area || K % 1024 != 0 || L.area_bytes < area_need || info.engine != 4 || info.tiles_offset == 0 || info.n_partials != (int)nt ||
      a.has(GJX_FILTER_NO_STEPS) || a.has(GJX_FILTER_ABSOLUTE_INPUTS) || gjx_plain_launches_forced() ||
      !periodic_steps(steps, T, [](const gjx_program* p, const gjx_program* q) { return gen_same_kernel(p, q, 4); }))
    return kNotThisForm;
  // (a grid the device cannot hold at once runs with as many blocks as are resident, each taking several tiles of a step in turn:
  // a block waits only at the top of a step, for granules every block publishes before it waits itself)
  const int64_t resident = a.forced_blocks() ? a.forced_blocks() : gen_steps_resident_blocks(&steps[1], 4);
  const int64_t grid = resident >= nt ? nt : resident;
  if (grid <= 0 || nt > 4 * grid) return kNotThisForm;
  hipStream_t st = a.st();
  unsigned long long* gran_a = (unsigned long long*)L.area;           // even steps
  unsigned long long* gran_b = gran_a + nt * kGranulePad;
  unsigned long long* part_a = gran_b + nt * kGranulePad;
  unsigned long long* part_b = part_a + nt;
  const float** tabs_dev = (const float**)(part_b + nt);
  uint32_t* keys_dev = (uint32_t*)(tabs_dev + T);
  double* us_dev = (double*)(keys_dev + 2 * (size_t)T);
  const hipError_t e = hipMemsetAsync(gran_a, 0, 16 * (size_t)kGranulePad * (size_t)nt, st);
  if (e != hipSuccess) return gjx_fail_hip(e, "gjx_scan_filter(step arguments)");
  if (int rcu = pf_upload_tabs(tabs_dev, steps, T, st)) return rcu;
  if (int rcu = upload_words(keys_dev, a.keys.data(), (size_t)T, st)) return rcu;
  if (int rcu = upload_words(us_dev, a.us.data(), (size_t)T, st)) return rcu;
  // tile totals {S_b, e_b} and block pairs of step 1 -> the tagged granules and the pair array the steps kernel's first step polls / reads
  const char* w1 = L.ws_of(1);
  const uint64_t* tS = (const uint64_t*)(w1 + info.tiles_offset);
  hipLaunchKernelGGL(k_tiles_to_granules, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, tS, (const int32_t*)(tS + nt),
                     (const unsigned long long*)(w1 + kWsHeaderBytes), gran_b, part_b, (int)nt, (unsigned long long)(1u % 15u) + 1ull);
  GJX_CHECK_LAUNCH("gjx_scan_filter(granules of step 1)");
  GenStepsArgs sa;
  memset(&sa, 0, sizeof(sa));
  sa.base.K = K; sa.base.offset = 0; sa.base.log_k_total = (float)log((double)K);
  sa.T0 = 2; sa.T = T; sa.tabs = tabs_dev; sa.keys = keys_dev; sa.us = us_dev;
  set_rows(sa, rows_of, T);
  sa.in_row0_first = sa.in_row0 = (int64_t)input_rows(steps[1]) * K;
  sa.logw_a = a.logw; sa.logw_b = L.logw2;
  sa.gran_a = gran_a; sa.gran_b = gran_b; sa.part_a = part_a; sa.part_b = part_b;
  sa.lse_steps = a.lse_steps; sa.anc = a.ancestors; sa.anc_all = a.ancestors_all; sa.ctrl = (unsigned*)L.ws_res + 8; sa.epoch = 0u;
  sa.timeline = gjx::debug_timeline(128 * (size_t)grid);
  const int rc = gen_steps_launch(&steps[1], 4, sa, (int)grid, st);
  if (rc) return rc == GJX_EUNSUPPORTED ? kNotThisForm : rc;
  finfo.form = GJX_FILTER_FORM_STEPS; finfo.launches += 3; finfo.grid = (int)grid; finfo.tiles_per_block = (int)((nt + grid - 1) / grid);
  return gjx_launch_lse_finish(((T - 1) & 1) ? part_b : part_a, (int)nt, K, a.lse_steps + 4 * (size_t)(T - 1), st);
}

// rows_of(t): the buffer step t writes its choices into (two alternating buffers, or one per step when the run is recorded)
// ad: accumulated weights in ad->logw_acc and a resampling in front of step t only where the device word ad->resampled[t] says so — the
// plain-launch loop with the search gated and one fused launch behind the step's kernel
template <class RowsOf>
static int scan_filter_impl(const gjx_program* steps, int32_t T, uint32_t key0, uint32_t key1, int64_t K, RowsOf&& rows_of,
                            float* logw, int32_t* ancestors, int32_t* ancestors_all, float* lse_steps, void* workspace,
                            size_t workspace_bytes, void* stream, const gjx_filter_opts* opts, gjx_filter_info* info_out,
                            const gjx_adaptive_opts* ad = nullptr) {
  FilterCall a = {steps, T, K, logw, ancestors, ancestors_all, lse_steps, workspace, workspace_bytes, stream, opts, ad, opts ? opts->flags : 0, opts ? opts->n_moves : 0};
  if (a.n_moves < 0) return gjx_fail(GJX_EINVAL, "gjx_scan_filter: n_moves < 0");
  gjx_filter_info finfo = {GJX_FILTER_FORM_TWO_LAUNCH, 0, 0, 0};
  auto report = [&](int rc_) { if (info_out) *info_out = finfo; return rc_; };
  if (info_out) *info_out = finfo;
  FilterLayout L;
  if (int rc = filter_begin(a, key0, key1, L)) return rc;
  int rc = run_wide(a, rows_of, L, finfo);
  if (rc != kNotThisForm) return report(rc);
  if (a.n_moves > 0 && T >= 2)     // (T < 2: there is no resampling, hence nothing to move: the plain forms below are the whole run)
    return report(gjx_fail(GJX_EUNSUPPORTED, "gjx_scan_filter: the rejuvenation move runs inside the filter kernel on the shared skeleton only "
                                             "(GJX_FILTER_FORM_WIDE: periodic step programs whose latent choices are the carry, no plates, a co-resident "
                                             "grid, the workspace room of the one-launch forms)"));
  gjx_run_info info = {0, 0, 0}, prev = {0, 0, 0};
  for (int t = 0; t < T; ++t) {
    gjx_run_opts o;
    memset(&o, 0, sizeof(o));
    o.flags = GJX_RUN_LEAVE_TILES;
    bool ran = false;
    if (t > 0) { if ((rc = resample_before_step(a, rows_of, L, t, prev, o, info, finfo, &ran))) return rc; }
    if (!ran) {
      rc = gjx_run_program_ex(&steps[t], a.keys[2 * t], a.keys[2 * t + 1], K, 0, rows_of(t), nullptr, nullptr, L.lw_of(t), nullptr, nullptr, nullptr, nullptr, K,
                              L.ws_of(t), L.need_run, stream, &o, &info);
      if (rc) return rc;
    }
    if (ad) {
      // W_t = (resampled in front of step t ? 0 : W_{t-1}) + inc_t in place, the record of step t, ESS_t and the decision for step t + 1
      // (the search's tile totals in ws_res are dead by now: the tile partials of this launch take their place)
      rc = gjx::launch_ess_accumulate(L.lw_of(t), ad->logw_acc, t == T - 1 ? logw : nullptr, K, t > 0 ? ad->resampled + t : nullptr,
                                      lse_steps + 4 * (size_t)t, t > 0 ? lse_steps + 4 * (size_t)(t - 1) : nullptr, ad->ess_steps + t,
                                      t + 1 < T ? ad->resampled + t + 1 : nullptr, ad->ess_threshold, L.ws_res, L.need_res, a.st());
      if (rc) return rc;
      finfo.launches += 1;
    }
    prev = info;
    finfo.launches += ran ? 1 : (t > 0 ? 2 : 1);
    if (t == 1) finfo.form = ran ? GJX_FILTER_FORM_PER_STEP : GJX_FILTER_FORM_TWO_LAUNCH;
    if (t == 1 && ran && (rc = run_steps_tail(a, rows_of, L, info, finfo)) != kNotThisForm) return report(rc);
  }
  if (ad) return report(GJX_OK);          // (every record was written by its step's fused launch)
  // the record of the last step: its block pairs are still in its run workspace
  finfo.launches += 1;
  return report(gjx_launch_lse_finish(L.ws_of(T - 1) + kWsHeaderBytes, prev.n_partials, K, lse_steps + 4 * (size_t)(T - 1), a.st()));
}

// ---- the four entry points: two buffers that alternate or the choices of EVERY step kept, each without / with adaptive resampling ----
static int fail_named(int rc, const char* who, const char* what) {
  char msg[224];
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  return gjx_fail(rc, msg);
}

// adaptive resampling (include/gjx.h, gjx_adaptive_opts)
static int adaptive_check(const char* who, const gjx_filter_opts* opts, const gjx_adaptive_opts* ad) {
  if (!ad || !ad->logw_acc || !ad->ess_steps || !ad->resampled) return fail_named(GJX_EINVAL, who, "adapt and its logw_acc, ess_steps, resampled must not be NULL");
  if (!(ad->ess_threshold >= 0.0f && ad->ess_threshold <= 1.0f)) return fail_named(GJX_EINVAL, who, "ess_threshold must be in [0, 1]");
  if (opts && opts->n_moves > 0) return fail_named(GJX_EUNSUPPORTED, who, "the rejuvenation move (n_moves > 0) runs inside the one-launch filter kernel, which resamples in front of every step");
  if (opts && opts->hmc_targets) return fail_named(GJX_EUNSUPPORTED, who, "the HMC move (hmc_targets) runs behind a resampling in front of EVERY step");
  if (opts && (opts->flags & GJX_FILTER_MULTINOMIAL)) return fail_named(GJX_EUNSUPPORTED, who, "adaptive resampling is systematic (no GJX_FILTER_MULTINOMIAL)");
  return GJX_OK;
}

static int filter_alternating(const char* who, bool adaptive, const gjx_program* steps, int32_t T, uint32_t key0, uint32_t key1, int64_t K, float* rows_a,
                              float* rows_b, float* logw, int32_t* ancestors, int32_t* ancestors_all, float* lse_steps, void* workspace,
                              size_t workspace_bytes, void* stream, const gjx_filter_opts* opts, gjx_filter_info* info_out, const gjx_adaptive_opts* adapt) {
  if (!steps || T < 1 || K <= 0 || !rows_a || !rows_b || !logw || !ancestors || !lse_steps) return fail_named(GJX_EINVAL, who, "bad argument");
  if (adaptive) if (const int rc = adaptive_check(who, opts, adapt)) return rc;
  const gjx_plain_launch_scope plain_scope(!adaptive && opts && (opts->flags & GJX_FILTER_NO_ONE_LAUNCH) == GJX_FILTER_NO_ONE_LAUNCH);
  return scan_filter_impl(steps, T, key0, key1, K, [&](int t) { return (t & 1) ? rows_b : rows_a; }, logw, ancestors, ancestors_all, lse_steps,
                          workspace, workspace_bytes, stream, opts, info_out, adapt);
}

// the same run with the choices of EVERY step kept (rows_all f32[T][rows_per_step][K]) and every resampling's ancestors: what a
// trajectory reconstruction needs (the reference's ScanTrace stacks the whole trace per particle, scan.py:56-97)
static int filter_recorded(const char* who, bool adaptive, const gjx_program* steps, int32_t T, uint32_t key0, uint32_t key1, int64_t K, float* rows_all,
                           int32_t rows_per_step, float* logw, int32_t* ancestors_all, float* lse_steps, void* workspace, size_t workspace_bytes,
                           void* stream, const gjx_filter_opts* opts, gjx_filter_info* info_out, const gjx_adaptive_opts* adapt) {
  if (!steps || T < 1 || K <= 0 || !rows_all || rows_per_step < 1 || !logw || (T > 1 && !ancestors_all) || !lse_steps) return fail_named(GJX_EINVAL, who, "bad argument");
  for (int t = 0; t < T; ++t)
    if (steps[t].n_slots > rows_per_step) return fail_named(GJX_EINVAL, who, "a step has more rows than rows_per_step");
  if (adaptive) if (const int rc = adaptive_check(who, opts, adapt)) return rc;
  int32_t* anc = ancestors_all ? ancestors_all : (int32_t*)rows_all;     // (T == 1: never written)
  const gjx_plain_launch_scope plain_scope(!adaptive && opts && (opts->flags & GJX_FILTER_NO_ONE_LAUNCH) == GJX_FILTER_NO_ONE_LAUNCH);
  return scan_filter_impl(steps, T, key0, key1, K, [&](int t) { return rows_all + (size_t)t * (size_t)rows_per_step * (size_t)K; }, logw, anc,
                          ancestors_all, lse_steps, workspace, workspace_bytes, stream, opts, info_out, adapt);
}

extern "C" int gjx_scan_filter(const gjx_program* steps, int32_t T, uint32_t key0, uint32_t key1, int64_t K, float* rows_a, float* rows_b,
                               float* logw, int32_t* ancestors, int32_t* ancestors_all, float* lse_steps, void* workspace,
                               size_t workspace_bytes, void* stream, const gjx_filter_opts* opts, gjx_filter_info* info_out) {
  return filter_alternating("gjx_scan_filter", false, steps, T, key0, key1, K, rows_a, rows_b, logw, ancestors, ancestors_all, lse_steps, workspace,
                            workspace_bytes, stream, opts, info_out, nullptr);
}
extern "C" int gjx_scan_filter_history(const gjx_program* steps, int32_t T, uint32_t key0, uint32_t key1, int64_t K, float* rows_all,
                                       int32_t rows_per_step, float* logw, int32_t* ancestors_all, float* lse_steps, void* workspace,
                                       size_t workspace_bytes, void* stream, const gjx_filter_opts* opts, gjx_filter_info* info_out) {
  return filter_recorded("gjx_scan_filter_history", false, steps, T, key0, key1, K, rows_all, rows_per_step, logw, ancestors_all, lse_steps, workspace,
                         workspace_bytes, stream, opts, info_out, nullptr);
}
extern "C" int gjx_scan_filter_adaptive(const gjx_program* steps, int32_t T, uint32_t key0, uint32_t key1, int64_t K, float* rows_a, float* rows_b,
                                        float* logw, int32_t* ancestors, int32_t* ancestors_all, float* lse_steps, void* workspace,
                                        size_t workspace_bytes, void* stream, const gjx_filter_opts* opts, gjx_filter_info* info_out,
                                        const gjx_adaptive_opts* adapt) {
  return filter_alternating("gjx_scan_filter_adaptive", true, steps, T, key0, key1, K, rows_a, rows_b, logw, ancestors, ancestors_all, lse_steps, workspace,
                            workspace_bytes, stream, opts, info_out, adapt);
}
extern "C" int gjx_scan_filter_adaptive_history(const gjx_program* steps, int32_t T, uint32_t key0, uint32_t key1, int64_t K, float* rows_all,
                                                int32_t rows_per_step, float* logw, int32_t* ancestors_all, float* lse_steps, void* workspace,
                                                size_t workspace_bytes, void* stream, const gjx_filter_opts* opts, gjx_filter_info* info_out,
                                                const gjx_adaptive_opts* adapt) {
  return filter_recorded("gjx_scan_filter_adaptive_history", true, steps, T, key0, key1, K, rows_all, rows_per_step, logw, ancestors_all, lse_steps,
                         workspace, workspace_bytes, stream, opts, info_out, adapt);
}
