// gjx_host.h — host-side helpers shared by the launchers (error reporting, the variant codes of the generated kernels; no state).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/gjx.h"

int gjx_fail(int status, const char* msg);           // records the thread-local message, returns status
int gjx_fail_hip(hipError_t e, const char* where);   // same for a HIP error

#define GJX_CHECK_LAUNCH(where)                                  \
  do {                                                           \
    hipError_t e__ = hipGetLastError();                          \
    if (e__ != hipSuccess) return gjx_fail_hip(e__, where);      \
  } while (0)

// {max,sumexp} block partials -> out[4] = {max, sumexp, lse, lse - log(K_total)}  (gjx_run.hip)
int gjx_launch_lse_finish(const void* partials_float2, int n, int64_t K_total, float* out, hipStream_t st);

// Number of thread blocks of `kernel` (block size `threads`, `dyn_lds` bytes of dynamic LDS) that are resident on the
// current device AT THE SAME TIME: occupancy query x CU count, cached per (kernel, device).  Kernels that synchronise
// their blocks through memory (granule all-gathers) must not be launched with a larger grid.  GJX_CORESIDENT_BLOCKS
// overrides the answer (tests of the fallback paths).  Returns 0 when the query fails.
int gjx_coresident_blocks(const void* kernel, int threads, size_t dyn_lds);
// While one of these lives on a thread, gjx_coresident_blocks answers 0 on that thread: every launcher below it takes its
// plain multi-launch path (GJX_WEIGHTS_PLAIN_LAUNCHES of gjx_ssm_filter_scheme: the repeat after a poll time-out).
struct gjx_plain_launch_scope {
  explicit gjx_plain_launch_scope(bool on);
  ~gjx_plain_launch_scope();
  bool on_;
};
bool gjx_plain_launches_forced();

namespace gjx {
// ---- variant codes of the generated kernels: the integers of the C ABI (gjx_program_precompile, gjx_program_filter_precompile,
//      genjax_amd/jit_manifest.py), decoded HERE and nowhere else ----
// run kernel (gjx_gen): particles per lane | flavour bits
enum : int {
  kRunPptMask = 255,
  kRunMfma = 256,       // big affine sites on the matrix cores: one particle per lane, whole waves
  kRunWide = 512,       // a block of 16 waves shares 64 x ppt particles: the instances of its plates are dealt to the waves ...
  kRunLanes4 = 1024,    // ... and to 4
  kRunLanes16 = 2048,   // ... or 16 lanes per particle
};
struct RunVariant {
  int ppt = 1;          // particles per lane
  bool mfma = false, wide = false;
  int lpp = 1;          // wide flavour: lanes per particle (1, 4, 16)
  int particles_per_block() const { return (wide ? 64 / lpp : 256) * ppt; }
};
inline int encode(const RunVariant& v) {
  return v.ppt | (v.mfma ? kRunMfma : 0) | (v.wide ? kRunWide : 0) | (v.lpp == 4 ? kRunLanes4 : (v.lpp == 16 ? kRunLanes16 : 0));
}
// false: not a kernel the emitter has (plain: ppt 1, 2, 4; matrix cores: ppt 1; wide: ppt 1, 2 with 1, 4 or 16 lanes per particle)
inline bool decode(int code, RunVariant* v) {
  RunVariant r;
  r.ppt = code & kRunPptMask;
  r.mfma = (code & kRunMfma) != 0;
  r.wide = (code & kRunWide) != 0;
  r.lpp = (code & kRunLanes16) ? 16 : ((code & kRunLanes4) ? 4 : 1);
  const int max_ppt = r.mfma ? 1 : (r.wide ? 2 : 4);
  if (code != encode(r) || (r.ppt != 1 && r.ppt != 2 && r.ppt != 4) || r.ppt > max_ppt || (r.mfma && r.wide) || (r.lpp > 1 && !r.wide)) return false;
  *v = r;
  return true;
}
// filter kernel (gjx_gen_pf): tiles per block | flavour bits
enum : int {
  kFilterTilesMask = 255,
  kFilterSharded = 256,       // runs on a collection sharded over peer-mapped windows (gjx_peer.hip)
  kFilterMoves = 512,         // a rejuvenation move behind every resampling
  kFilterMultinomial = 1024,  // multinomial resampling by sorted uniforms instead of the systematic comb (not together with the move)
};
struct FilterVariant {
  int tiles = 1;              // 1024-particle tiles per block: 1, 2, 4, 8, 16
  bool sharded = false, moves = false, multinomial = false;
};
inline int encode(const FilterVariant& v) {
  return v.tiles | (v.sharded ? kFilterSharded : 0) | (v.moves ? kFilterMoves : 0) | (v.multinomial ? kFilterMultinomial : 0);
}
inline bool decode(int code, FilterVariant* v) {
  FilterVariant r;
  r.tiles = code & kFilterTilesMask;
  r.sharded = (code & kFilterSharded) != 0;
  r.moves = (code & kFilterMoves) != 0;
  r.multinomial = (code & kFilterMultinomial) != 0;
  const int t = r.tiles;
  if (code != encode(r) || (t != 1 && t != 2 && t != 4 && t != 8 && t != 16) || (r.moves && r.multinomial)) return false;
  *v = r;
  return true;
}

// rows of a program's INPUT sites (they come first and in order)
inline int input_rows(const gjx_program& p) {
  int n = 0;
  for (int j = 0; j < p.n_sites; ++j) if (p.sites[j].mode == GJX_MODE_INPUT) n += p.sites[j].dim;
  return n;
}

// phase-stamp buffer of the profiling scripts (gjx_debug_timeline): the registered device buffer if it holds `need` bytes
unsigned long long* debug_timeline(size_t need);
struct GenArgs;
// per-program generated kernels (emitted by gjx_codegen.hip, compiled / loaded / launched by gjx_jit.hip)
int gen_pick_ppt(const gjx_program* prog, int64_t K, bool prefer4 = false);
int gen_available(const gjx_program* prog, int ppt);
int gen_launch(const gjx_program* prog, int ppt, const GenArgs& args, int grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1);
// the steps kernel of a generated filter (gjx_gen_steps): every step of a run in one launch
struct GenStepsArgs;
bool gen_same_kernel(const gjx_program* p, const gjx_program* q, int ppt);
int gen_steps_resident_blocks(const gjx_program* prog, int ppt);
int gen_steps_launch(const gjx_program* prog, int ppt, const GenStepsArgs& args, int grid, hipStream_t st);
// the filter kernel generated for a step program (gjx_gen_pf on the skeleton of gjx_pfcore.h): steps 1 .. T-1 of a run in one launch,
// 16 waves per 1024-particle tile, `spl` tiles per block
struct GenPfArgs;
bool gen_pf_supported(const gjx_program* p);
bool gen_pf_moves_supported(const gjx_program* p);   // the kernel can carry the rejuvenation move (FilterVariant::moves)
bool gen_pf_same_kernel(const gjx_program* p, const gjx_program* q);
int gen_pf_precompile(const gjx_program* prog, int spl);
int gen_pf_resident_blocks(const gjx_program* prog, int spl, size_t dyn_lds);
int gen_pf_launch(const gjx_program* prog, int spl, const GenPfArgs& args, int grid, size_t dyn_lds, hipStream_t st);
// steps 2 .. T-1 are the kernel of step 1 (a periodic Scan: they differ in tables, keys, comb offsets); same_kernel(&steps[1], &steps[u])
// compares the generated code (gen_pf_same_kernel, or gen_same_kernel at one ppt)
template <class SameKernel>
bool periodic_steps(const gjx_program* steps, int T, SameKernel&& same_kernel) {
  for (int u = 2; u < T; ++u)
    if (steps[u].n_tab != steps[1].n_tab || steps[u].n_slots != steps[1].n_slots || input_rows(steps[u]) != input_rows(steps[1]) ||
        !steps[u].tab_dev || !same_kernel(&steps[1], &steps[u]))
      return false;
  return true;
}
// n 8-byte words from HOST memory to device memory through kernel arguments (small per-run argument arrays: step keys, comb
// offsets, table pointers): no host buffer has to outlive the call, unlike an asynchronous copy from pageable memory
int upload_words(void* dst_dev, const void* src_host, size_t n_words, hipStream_t st);
// per-program generated HMC kernels (gjx_codegen.hip, gjx_jit.hip)
struct HmcGenArgs;
int hmc_gen_available(const gjx_program* prog);
int hmc_gen_launch(const gjx_program* prog, const HmcGenArgs& args, hipStream_t st);
// systematic ancestor expansion with the slot run {slot0, n_valid} read from a device plan (gjx_resample.hip)
int launch_expand_planned(const uint64_t* cum, int64_t K, const gjx_shard_plan* plan_dev, double u, int64_t N_total,
                          int32_t* ancestors, int64_t anc_capacity, hipStream_t st);
// maximum tile exponent, shifts and prefix of the shifted tile totals for the tile-scaled resampler (k_tiled_plan, gjx_resample.hip):
// P u64[nt + 1], sh i32[nt]
// gate (or NULL): a device word; 0 means "the step does not resample" and the launch does nothing (gjx_scan_filter_adaptive)
int launch_tiled_plan(const uint64_t* S, const int32_t* E, int nt, uint64_t* P, int32_t* sh, unsigned* ctrl, hipStream_t st,
                      const int32_t* gate = nullptr);
// gjx_resample_gather_tiled with every launch (tile totals, tile prefix, search) gated by the device word *gate: 0 -> identity ancestors,
// the rows copied as they are, the log-weights, tile totals and status word untouched; gate == NULL: the ungated call (gjx_resample.hip)
int resample_gather_tiled_gated(const float* logw, int64_t K, const uint64_t* tile_S, const int32_t* tile_E, int32_t lse_mode, const float* lse,
                                int32_t n_partials, double u, const float* src, int64_t src_stride, int32_t rows, float* dst, int64_t dst_stride,
                                int32_t* ancestors, float* lse_out, int64_t K_total, void* workspace, size_t workspace_bytes, void* stream,
                                const int32_t* gate);
// the fused launch of the adaptive filter (gjx_resample.hip, k_ess_tiles): W = fresh ? inc : W + inc in place (also stored to w_copy when
// not NULL), {max, sum e, sum e^2} per 1024-particle tile, and the finishing block's record of the step: lse_rec[4] (lse_prev: the record
// of the step before, read behind a skip), *ess_out, *decide_out = (ess < tau * K || tau >= 1).  fresh: a device word, or NULL = "yes"
int launch_ess_accumulate(const float* inc, float* W, float* w_copy, int64_t K, const int32_t* fresh, float* lse_rec, const float* lse_prev,
                          float* ess_out, int32_t* decide_out, float tau, void* workspace, size_t workspace_bytes, hipStream_t st);
}  // namespace gjx
