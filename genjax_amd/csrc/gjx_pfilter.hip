// gjx_pfilter.hip — host side shared by the launchers of the one-launch particle filters (declared in gjx_pfilter_host.h): the kernel /
// grid plan of k_pf_persistent, the step keys of a run, the skeleton's workspace area, the ONE place PfCoreArgs is filled (one GPU, or a
// rank of a peer context) and the upload of the per-step arrays.  The launchers themselves are in gjx_ssm.hip, gjx_peer.hip, gjx_scanfilter.hip.
#include <math.h>
#include <string.h>

#include <vector>

#include "gjx_host.h"
#include "gjx_pfilter_host.h"

namespace gjx {

const void* pf_kernel_flat(int dx, int spl, bool move);   // gjx_pfilter_flat.hip
const void* pf_kernel_jax(int dx, int spl, bool move);    // gjx_pfilter_jax.hip

int pf_plan(int rng_mode, int dx, int dy, int64_t K_local, int n_ranks, int share, PfPlan* out, bool move) {
  if (K_local <= 0 || n_ranks < 1 || n_ranks > GJX_MAX_RANKS || dy > 32) return GJX_EUNSUPPORTED;
  const int64_t nt = (K_local + kPfHostThreads - 1) / kPfHostThreads;
  if (n_ranks > 1 && K_local % kPfHostThreads) return GJX_EUNSUPPORTED;   // sharded: whole tiles per rank
  if (nt * n_ranks > kPfHostMaxTiles) return GJX_EUNSUPPORTED;
  const size_t lds = pf_host_dyn_lds((int)(nt * n_ranks));
  auto kernel = [&](int spl) { return rng_mode == GJX_RNG_JAX32 ? pf_kernel_jax(dx, spl, move) : pf_kernel_flat(dx, spl, move); };
  const PfGeometry geo = pf_pick_tiles(nt, n_ranks, share, kPfHostMaxTiles, [&](int spl) {
    const void* fn = kernel(spl);
    // (static + dynamic LDS is above the 64 KB default once NT > 2048)
    if (fn && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) { (void)hipGetLastError(); }
    return fn ? gjx_coresident_blocks(fn, kPfHostThreads, lds) : 0;
  });
  if (!geo.spl) return GJX_EUNSUPPORTED;
  out->fn = kernel(geo.spl); out->spl = geo.spl; out->grid = geo.grid; out->lds = lds; out->nt = (int)nt;
  return GJX_OK;
}

// ---- small per-run argument arrays (step keys, comb offsets, table pointers) reach the device as KERNEL ARGUMENTS: the runtime
//      copies a launch's argument block before the launch call returns, so no host buffer has to outlive the call (an asynchronous
//      copy from pageable memory may still read its source afterwards) and the library keeps no per-thread staging state ----
namespace {
constexpr int kWordsPerLaunch = 120;
struct WordChunk {
  unsigned long long w[kWordsPerLaunch];
  unsigned long long* dst;
  int n;
};
__global__ void k_upload_words(WordChunk c) {
  const int i = (int)threadIdx.x;
  if (i < c.n) c.dst[i] = c.w[i];
}
}  // namespace

int upload_words(void* dst_dev, const void* src_host, size_t n_words, hipStream_t st) {
  const unsigned long long* src = (const unsigned long long*)src_host;
  unsigned long long* dst = (unsigned long long*)dst_dev;
  for (size_t at = 0; at < n_words; at += kWordsPerLaunch) {
    WordChunk c;
    c.n = (int)(n_words - at < (size_t)kWordsPerLaunch ? n_words - at : (size_t)kWordsPerLaunch);
    memcpy(c.w, src + at, sizeof(unsigned long long) * (size_t)c.n);
    c.dst = dst + at;
    hipLaunchKernelGGL(k_upload_words, dim3(1), dim3(128), 0, st, c);
    GJX_CHECK_LAUNCH("upload_words");
  }
  return GJX_OK;
}

void host_threefry2x32(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t out[2]) {
  const uint64_t h = gjx_host_threefry2x32(k0, k1, c0, c1);
  out[0] = (uint32_t)(h >> 32); out[1] = (uint32_t)h;
}

// Key discipline of inference/pf.py: k_t = fold_in(k_{t-1}, t) (scan.py:268); (k_prop, k_res) = split(k_t); the comb
// offset of the resampling in front of step t is uniform(k_res).
void pf_step_keys(uint32_t key0, uint32_t key1, int T, std::vector<uint32_t>& keys, std::vector<double>& us) {
  std::vector<uint32_t> unused;
  pf_step_keys_res(key0, key1, T, keys, us, unused);
}

void pf_step_keys_res(uint32_t key0, uint32_t key1, int T, std::vector<uint32_t>& keys, std::vector<double>& us, std::vector<uint32_t>& res_keys) {
  keys.assign(2 * (size_t)T, 0u);
  us.assign((size_t)T, 0.0);
  res_keys.assign(2 * (size_t)T, 0u);
  uint32_t k[2] = {key0, key1};
  for (int t = 0; t < T; ++t) {
    uint32_t kt[2], kp[2], kr[2], b[2];
    host_threefry2x32(k[0], k[1], 0u, (uint32_t)t, kt);
    k[0] = kt[0]; k[1] = kt[1];
    host_threefry2x32(k[0], k[1], 0u, 0u, kp);
    host_threefry2x32(k[0], k[1], 0u, 1u, kr);
    host_threefry2x32(kr[0], kr[1], 0u, 0u, b);
    keys[2 * t] = kp[0]; keys[2 * t + 1] = kp[1];
    res_keys[2 * t] = kr[0]; res_keys[2 * t + 1] = kr[1];
    us[t] = (double)((b[0] ^ b[1]) >> 9) / 8388608.0;
  }
}

PfRegion pf_region(char* base, int64_t nt, int64_t grid, int T, bool with_tabs) {
  PfRegion r;
  const size_t tile_bytes = (16 * (size_t)kGranulePad + 24) * (size_t)nt, ready_bytes = 8 * (((size_t)grid + 1) / 2);
  r.nt = (int)nt; r.ctrl = (unsigned*)base + 8;
  r.aggA = (unsigned long long*)(base + kWsHeaderBytes); r.aggB = r.aggA + (size_t)nt * kGranulePad;
  r.bsum = (float*)(r.aggB + (size_t)nt * kGranulePad); r.bmax = r.bsum + 3 * (size_t)nt;
  r.ready = (unsigned*)(r.bmax + 3 * (size_t)nt);
  r.us = (double*)((char*)r.ready + ready_bytes); r.keys = (uint32_t*)(r.us + T);
  r.tabs = with_tabs ? (const float**)(r.keys + 2 * (size_t)T) : nullptr;
  r.clear_bytes = tile_bytes + ready_bytes;
  r.bytes = kWsHeaderBytes + tile_bytes + 8 * (size_t)grid + (with_tabs ? 24 : 16) * (size_t)T + 64;
  return r;
}

PfCoreArgs pf_core_single(int T, int64_t K, const PfRegion& rg, float* lw_even, float* lw_odd, float* lse_steps, int32_t* ancestors) {
  PfCoreArgs c;
  memset(&c, 0, sizeof(c));               // one rank: offset, rank 0; no peers, nothing to clear for a next launch, no verify mode
  c.T = T; c.K = K; c.K_total = K; c.G = 1; c.nt = rg.nt; c.NT = rg.nt;
  c.lw_even = lw_even; c.lw_odd = lw_odd;
  c.aggA = rg.aggA; c.aggB = rg.aggB; c.bsum = rg.bsum; c.bmax = rg.bmax; c.ready = rg.ready;
  c.keys = rg.keys; c.us = rg.us; c.lse_steps = lse_steps; c.ancestors = ancestors;
  c.ctrl = rg.ctrl; c.log_k = (float)log((double)K); c.first_budget = kPollBudget;
  return c;
}

PfCoreArgs pf_core_peer(int T, gjx_peer_ctx* c, float* lse_steps, int32_t* ancestors) {
  const int region = (int)(c->n_filter & 1), other = region ^ 1;
  c->n_filter += 1;
  char* rg = c->flag + c->off_region[region];
  PfCoreArgs f;
  memset(&f, 0, sizeof(f));
  f.T = T; f.K = c->K; f.K_total = c->K * c->world; f.offset = (int64_t)c->rank * c->K; f.G = c->world; f.rank = c->rank; f.nt = c->nt; f.NT = c->NT;
  f.lw_even = (float*)(c->data + c->off_lw[0]); f.lw_odd = (float*)(c->data + c->off_lw[1]);
  f.aggA = (unsigned long long*)(rg + c->r_aggA); f.aggB = (unsigned long long*)(rg + c->r_aggB);
  f.bsum = (float*)(rg + c->r_bsum); f.bmax = (float*)(rg + c->r_bmax); f.ready = (unsigned*)(rg + c->r_ready);
  f.peer_data = c->world > 1 ? c->delta_dev : nullptr;
  f.peer_flag = c->world > 1 ? c->delta_dev + c->world : nullptr;
  f.keys = c->keys_dev; f.us = c->us_dev; f.lse_steps = lse_steps; f.ancestors = ancestors;
  f.ctrl = (unsigned*)c->flag + 8; f.log_k = (float)log((double)f.K_total);
  // the other ranks' launches may be queued behind host work of their own: the first rendezvous waits for seconds, later ones ~0.1 s
  f.first_budget = c->world > 1 ? (1u << 24) : kPollBudget;
  f.zero_ptr = (unsigned long long*)(c->flag + c->off_region[other] + c->r_aggA);
  f.zero_n = (int)((c->r_bsum - c->r_aggA) / 8);
  f.verify = c->verify ? (c->verify_fault ? 2 : 1) : 0;
  f.chk_a = (unsigned*)(c->data + c->off_chk[0]); f.chk_b = (unsigned*)(c->data + c->off_chk[1]);
  return f;
}

std::vector<double> pf_us_words(const std::vector<double>& us, const std::vector<uint32_t>& res_keys, bool multinomial) {
  std::vector<double> w(us);
  if (multinomial)
    for (size_t u = 0; u < w.size(); ++u) { const uint64_t b = (uint64_t)res_keys[2 * u] | ((uint64_t)res_keys[2 * u + 1] << 32); memcpy(&w[u], &b, 8); }
  return w;
}

int pf_upload_tabs(const float** tabs_dev, const gjx_program* steps, int T, hipStream_t st) {
  std::vector<const float*> h_tabs((size_t)T, nullptr);
  for (int u = 0; u < T; ++u) h_tabs[u] = steps[u].tab_dev;
  return upload_words(tabs_dev, h_tabs.data(), (size_t)T, st);
}

int pf_upload_steps(double* us_dev, const std::vector<double>& us, uint32_t* keys_dev, const std::vector<uint32_t>& keys, const float** tabs_dev,
                    const gjx_program* steps, int T, hipStream_t st) {
  if (int rc = upload_words(us_dev, us.data(), (size_t)T, st)) return rc;
  if (int rc = upload_words(keys_dev, keys.data(), (size_t)T, st)) return rc;      // (T pairs of 32-bit words)
  return tabs_dev ? pf_upload_tabs(tabs_dev, steps, T, st) : GJX_OK;
}

}  // namespace gjx
