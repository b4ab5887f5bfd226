// gjx_jit.hip — the runtime of the per-program generated kernels.  gjx_codegen.hip turns a site list into HIP source; here that
// source is compiled with hipRTC for gfx950 and cached per structure (in memory, and as a code object next to this library so
// that a build step can pre-populate the cache; the table VALUES are run-time data, so new observations do not recompile),
// its module is loaded once per device, and its kernels are launched.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hip/hiprtc.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <atomic>
#include <chrono>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "gjx_codegen.h"
#include "gjx_device.h"
#include "gjx_host.h"
#include "gjx_pfcore.h"

using namespace gjx_codegen;

namespace {

const char* kDeviceHeader =
#include "build/gjx_device_h.inc"
    ;
const char* kApiHeader =
#include "build/gjx_h.inc"
    ;
const char* kScanHeader =
#include "build/gjx_scan_h.inc"
    ;
const char* kTileHeader =
#include "build/gjx_tile_h.inc"
    ;
const char* kPfCoreHeader =
#include "build/gjx_pfcore_h.inc"
    ;

// the three kernel families (the values enter the in-memory key only): the file name hipRTC reports and the emitter of the source
enum Flavour { kRun = 0, kHmc = 1, kFilter = 2 };   // variant code: gjx::RunVariant; 0 / 16 / 64 lanes per chain; gjx::FilterVariant
const struct { const char* source_name; Generated (*generate)(const gjx_program*, int); } kFlavours[] = {
    {"gjx_gen.hip", generate}, {"gjx_hmc_gen.hip", generate_hmc}, {"gjx_gen_pf.hip", generate_pf}};

// ---------------------------------------------------------------------------------------------------------
// hipRTC (resolved at run time: the library must not need it when no program is ever generated)
// ---------------------------------------------------------------------------------------------------------
struct Rtc {
  void* lib = nullptr;
  decltype(&hiprtcCreateProgram) Create = nullptr;
  decltype(&hiprtcCompileProgram) Compile = nullptr;
  decltype(&hiprtcGetProgramLogSize) LogSize = nullptr;
  decltype(&hiprtcGetProgramLog) Log = nullptr;
  decltype(&hiprtcGetCodeSize) CodeSize = nullptr;
  decltype(&hiprtcGetCode) Code = nullptr;
  decltype(&hiprtcDestroyProgram) Destroy = nullptr;
  bool ok = false;
};

Rtc& rtc() {
  static Rtc r;
  static std::once_flag once;
  std::call_once(once, [] {
    const char* names[] = {getenv("GJX_HIPRTC"), "libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"};
    for (const char* n : names) {
      if (!n) continue;
      r.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
      if (r.lib) break;
    }
    if (!r.lib) return;
    bool ok = true;
    auto sym = [&](const char* n) { void* p = dlsym(r.lib, n); ok = ok && p; return p; };
    r.Create = (decltype(r.Create))sym("hiprtcCreateProgram");
    r.Compile = (decltype(r.Compile))sym("hiprtcCompileProgram");
    r.LogSize = (decltype(r.LogSize))sym("hiprtcGetProgramLogSize");
    r.Log = (decltype(r.Log))sym("hiprtcGetProgramLog");
    r.CodeSize = (decltype(r.CodeSize))sym("hiprtcGetCodeSize");
    r.Code = (decltype(r.Code))sym("hiprtcGetCode");
    r.Destroy = (decltype(r.Destroy))sym("hiprtcDestroyProgram");
    r.ok = ok;
  });
  return r;
}

uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}

std::string cache_dir() {
  if (const char* e = getenv("GJX_JIT_CACHE")) return e;
  Dl_info info;
  if (dladdr((void*)&fnv1a, &info) && info.dli_fname) {
    std::string p = info.dli_fname;
    const size_t k = p.rfind('/');
    return (k == std::string::npos ? std::string(".") : p.substr(0, k)) + "/jit_cache";
  }
  return "/tmp/gjx_jit_cache";
}

struct Compiled {
  std::vector<char> code;   // code object
  Generated k;              // what the emitter said about the kernel (k.src is dropped once compiled)
  std::string error;        // non-empty: this structure cannot be generated / compiled
};

std::mutex g_mu;
std::map<uint64_t, Compiled> g_compiled;                                 // by structure key
// gjx_jit_stats: kernels compiled by hipRTC in this process, code objects taken from the on-disk cache, time spent compiling (us)
std::atomic<int64_t> g_rtc_compiles{0}, g_disk_hits{0}, g_rtc_us{0};
// a loaded module and the functions looked up in it so far (nullptr: the module has no such function)
struct Loaded { hipModule_t mod = nullptr; std::map<std::string, hipFunction_t> fns; };
std::map<std::pair<uint64_t, int>, Loaded> g_loaded;                     // by (structure key, device)

// per-program analysis cached under gjx_program.uid (0 = no caching): the site-list hash, the emitter's verdict and the
// register footprint that decides PPT — each of them a walk over the whole site list
struct ProgMeta { bool roll_pref; uint64_t sites_hash; int supported; int slots; };   // supported / slots: -1 = not computed yet
std::mutex g_meta_mu;
std::unordered_map<int32_t, ProgMeta> g_meta;

// the site list AND the expression blocks its GJX_P_EXPR parameters name (node lists are structure: gjx.h)
uint64_t sites_hash_uncached(const gjx_program* p) {
  uint64_t h = fnv1a(p->sites, sizeof(gjx_site) * (size_t)p->n_sites);
  if (p->tab)
    for (int j = 0; j < p->n_sites; ++j)
      for (int k = 0; k < GJX_MAX_PARAMS; ++k) {
        const gjx_param& q = p->sites[j].p[k];
        if (p->sites[j].mode != GJX_MODE_INPUT && q.op == GJX_P_EXPR && q.off >= 0 && q.n > 0 && q.off + GJX_EXPR_NODE_FLOATS * q.n <= p->n_tab)
          h = fnv1a(p->tab + q.off, sizeof(float) * GJX_EXPR_NODE_FLOATS * (size_t)q.n, h);
      }
  return h | 1ull;
}

ProgMeta* meta_of(const gjx_program* p) {      // call with g_meta_mu held; nullptr when the program has no uid
  if (p->uid == 0) return nullptr;
  ProgMeta& m = g_meta[p->uid];
  if (m.sites_hash == 0 || m.roll_pref != want_roll()) m = ProgMeta{want_roll(), sites_hash_uncached(p), -1, -1};
  return &m;
}

uint64_t sites_hash(const gjx_program* p) {
  std::lock_guard<std::mutex> lock(g_meta_mu);
  if (ProgMeta* m = meta_of(p)) return m->sites_hash;
  return sites_hash_uncached(p);
}

bool supported(const gjx_program* p) {
  std::lock_guard<std::mutex> lock(g_meta_mu);
  ProgMeta* m = meta_of(p);
  if (!m) return supported_uncached(p);
  if (m->supported < 0) m->supported = supported_uncached(p) ? 1 : 0;
  return m->supported == 1;
}

int register_slots(const gjx_program* p) {
  std::lock_guard<std::mutex> lock(g_meta_mu);
  ProgMeta* m = meta_of(p);
  if (!m) return register_slots_uncached(p);
  if (m->slots < 0) m->slots = register_slots_uncached(p);
  return m->slots;
}

// GJX_JIT_FP_CONTRACT=fast: the compiler's default contraction for the propagate and filter kernels too (see compile())
bool fp_contract_fast() { const char* e = getenv("GJX_JIT_FP_CONTRACT"); return e && !strcmp(e, "fast"); }

// the in-memory identity of a kernel: program structure, variant code, flavour and every knob of the emitters
uint64_t structure_key(const gjx_program* p, int code, Flavour fl = kRun) {
  uint64_t h = sites_hash(p);
  if (fl == kHmc) {   // the HMC emitter's data-dependent choice (hmc_fold_ok reads the observations): part of the kernel's identity
    std::vector<char> fold;
    if (hmc_plan_fold(p, &fold)) h = fnv1a(fold.data(), fold.size(), h);
  }
  const int32_t extra[7] = {p->n_sites, p->n_slots, p->n_tab, p->rng_mode, code, (int32_t)fl, fp_contract_fast() ? 1 : 0};
  h = fnv1a(extra, sizeof(extra), h);
  for (int i = 0; i < kNumKnobs; ++i)
    if (const char* e = getenv(kKnobs[i].name)) {
      h = fnv1a(kKnobs[i].name, strlen(kKnobs[i].name) + 1, h);
      if (kKnobs[i].by_value) h = fnv1a(e, strlen(e) + 1, h);
    }
  static const uint64_t header_hash = fnv1a(kDeviceHeader, strlen(kDeviceHeader));   // a new device header invalidates the caches
  return h ^ header_hash ^ (0x9E3779B97F4A7C15ull * GJX_ABI_VERSION);
}

// call with g_mu held
const Compiled& compile(uint64_t key, const gjx_program* prog, int code, Flavour fl) {
  auto it = g_compiled.find(key);
  if (it != g_compiled.end()) return it->second;
  Compiled& c = g_compiled[key];
  c.k = kFlavours[fl].generate(prog, code);
  std::string src;
  src.swap(c.k.src);
  if (src.empty()) { c.error = "codegen: program outside the emitter's coverage"; return c; }
  if ((size_t)c.k.lds_floats * 4 + 256 > 64 * 1024) { c.error = "the program's table does not fit the LDS budget"; return c; }
  // the code object on disk is named by the SOURCE it was compiled from (and the headers): a changed emitter or header
  // can never pick up a stale file
  char name[64];
  // generated kernels are compiled WITHOUT implicit fused multiply-adds (the explicit fmaf of the emitters and of gjx_device.h stay):
  // the same site then rounds the same way in every kernel it is compiled into — the filter kernel with one particle per lane and
  // gjx_gen with four gave a student-t draw that differed in the last bit — at no measurable cost (mixture kernel 31.6 -> 31.9 us,
  // filter steps unchanged); GJX_JIT_FP_CONTRACT=fast restores the compiler's default for experiments
  // — for the propagate and filter kernels; the HMC kernels (one kernel per program: nothing to agree with) keep the default, which is
  // worth 13 - 25 % on gradient sweeps written without explicit fmaf
  const bool no_contract = fl != kHmc && !fp_contract_fast();
  snprintf(name, sizeof(name), "%016llx", (unsigned long long)((no_contract ? 0x5bd1e995ull : 0ull) ^ fnv1a(src.data(), src.size()) ^ fnv1a(kDeviceHeader, strlen(kDeviceHeader)) ^ fnv1a(kApiHeader, strlen(kApiHeader)) ^
                                                               fnv1a(kScanHeader, strlen(kScanHeader)) ^ (fnv1a(kTileHeader, strlen(kTileHeader)) << 1) ^
                                                               (fl == kFilter ? fnv1a(kPfCoreHeader, strlen(kPfCoreHeader)) << 2 : 0ull)));
  const std::string dir = cache_dir(), path = dir + "/" + name + ".hsaco";
  if (!getenv("GJX_JIT_NO_DISK")) {
    if (FILE* f = fopen(path.c_str(), "rb")) {
      fseek(f, 0, SEEK_END);
      const long n = ftell(f);
      fseek(f, 0, SEEK_SET);
      c.code.resize((size_t)n);
      const size_t got = fread(c.code.data(), 1, (size_t)n, f);
      fclose(f);
      if (got == (size_t)n && n > 0) { g_disk_hits++; return c; }
      c.code.clear();
    }
  }
  if (getenv("GJX_JIT_DUMP")) {
    if (FILE* f = fopen((std::string(getenv("GJX_JIT_DUMP")) + "/" + name + ".hip").c_str(), "w")) { fputs(src.c_str(), f); fclose(f); }
  }
  Rtc& r = rtc();
  if (!r.ok) { c.error = "hipRTC is not available (libhiprtc.so)"; return c; }
  hiprtcProgram p;
  const char* hn[] = {"gjx_device.h", "../../include/gjx.h", "gjx_scan.h", "gjx_tile.h", "gjx_pfcore.h"};
  const char* hs[] = {kDeviceHeader, kApiHeader, kScanHeader, kTileHeader, kPfCoreHeader};
  if (r.Create(&p, src.c_str(), kFlavours[fl].source_name, 5, hs, hn) != HIPRTC_SUCCESS) { c.error = "hiprtcCreateProgram failed"; return c; }
  // (offline clang takes -mllvm -amdgpu-mfma-vgpr-form=1, which would keep matrix-core results out of the AGPRs; this hipRTC's LLVM
  // does not know the option, so the generated kernels pay 16 v_accvgpr_read per tile: about 3 %)
  const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off"};
  const auto t_rtc = std::chrono::steady_clock::now();
  const hiprtcResult rc = r.Compile(p, no_contract ? 4 : 3, opts);
  g_rtc_compiles++;
  g_rtc_us += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_rtc).count();
  if (rc != HIPRTC_SUCCESS) {
    size_t ls = 0;
    r.LogSize(p, &ls);
    std::string log(ls, 0);
    if (ls) r.Log(p, &log[0]);
    c.error = "hipRTC: " + log.substr(0, 1500);
    r.Destroy(&p);
    return c;
  }
  size_t cs = 0;
  r.CodeSize(p, &cs);
  c.code.resize(cs);
  r.Code(p, c.code.data());
  r.Destroy(&p);
  if (!getenv("GJX_JIT_NO_DISK")) {
    mkdir(dir.c_str(), 0755);
    const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
    if (FILE* f = fopen(tmp.c_str(), "wb")) {
      fwrite(c.code.data(), 1, c.code.size(), f);
      fclose(f);
      rename(tmp.c_str(), path.c_str());
    }
  }
  return c;
}

// compile (or find) the kernel without loading it: GJX_OK, or the reason in gjx_last_error
int precompile(const gjx_program* prog, int code, Flavour fl) {
  std::lock_guard<std::mutex> lock(g_mu);
  const Compiled& c = compile(structure_key(prog, code, fl), prog, code, fl);
  return c.error.empty() ? GJX_OK : gjx_fail(GJX_EUNSUPPORTED, c.error.c_str());
}

// call with g_mu held: function `name` of a compiled kernel, its module loaded on the current device at first use.
// optional: a module without the function is remembered as such and answers GJX_EUNSUPPORTED without another lookup
int load_function(uint64_t key, const Compiled& c, Flavour fl, const char* name, bool optional, hipFunction_t* fn) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return gjx_fail(GJX_EHIP, "codegen: no device");
  const auto lk = std::make_pair(key, dev);
  auto it = g_loaded.find(lk);
  if (it == g_loaded.end()) {
    hipModule_t mod;
    const hipError_t e = hipModuleLoadData(&mod, c.code.data());
    if (e != hipSuccess) return gjx_fail_hip(e, "codegen: hipModuleLoadData");
    it = g_loaded.emplace(lk, Loaded{mod, {}}).first;
  }
  Loaded& l = it->second;
  auto f = l.fns.find(name);
  if (f == l.fns.end()) {
    hipFunction_t got = nullptr;
    const hipError_t e = hipModuleGetFunction(&got, l.mod, name);
    if (e != hipSuccess) {
      if (!optional) return gjx_fail_hip(e, "codegen: hipModuleGetFunction");
      (void)hipGetLastError();
      got = nullptr;
    }
    // (filter kernel: static + dynamic LDS is above the 64 KB default once a run has more than ~2000 tiles)
    if (got && fl == kFilter && hipFuncSetAttribute((const void*)got, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024) != hipSuccess) (void)hipGetLastError();
    f = l.fns.emplace(name, got).first;
  }
  *fn = f->second;
  return *fn ? GJX_OK : GJX_EUNSUPPORTED;
}

// the function `name` of the kernel generated for (program, code, flavour) — compiled and loaded now if need be — and its entry in
// the in-memory cache (entries are never removed: the pointer outlives the lock)
int function_of(const gjx_program* prog, int code, Flavour fl, const char* name, bool optional, hipFunction_t* fn, const Compiled** c_out) {
  std::lock_guard<std::mutex> lock(g_mu);
  const uint64_t key = structure_key(prog, code, fl);
  const Compiled& c = compile(key, prog, code, fl);
  if (!c.error.empty()) return gjx_fail(GJX_EUNSUPPORTED, c.error.c_str());
  *c_out = &c;
  return load_function(key, c, fl, name, optional, fn);
}

// a launch whose arguments are one packed struct; with both events: timed by the runtime (hipExtModuleLaunchKernel)
template <class Args>
int launch_packed(hipFunction_t fn, unsigned grid, unsigned block, size_t lds_bytes, hipStream_t st, Args a, const char* what,
                  hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr) {
  size_t sz = sizeof(a);
  void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &a, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  const hipError_t e = (ev0 && ev1) ? hipExtModuleLaunchKernel(fn, (uint32_t)grid * block, 1, 1, block, 1, 1, lds_bytes, st, nullptr, config, ev0, ev1, 0)
                                    : hipModuleLaunchKernel(fn, grid, 1, 1, block, 1, 1, (unsigned)lds_bytes, st, nullptr, config);
  return e == hipSuccess ? GJX_OK : gjx_fail_hip(e, what);
}

// blocks of `fn` that are resident at the same time on the current device: min(per-CU answer, cap) x CUs, or 0 (query failed)
int resident_blocks(hipFunction_t fn, int block, size_t dyn_lds, int cap_per_cu) {
  int per_cu = 0, cus = 0, dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, block, dyn_lds) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return (per_cu > cap_per_cu ? cap_per_cu : per_cu) * cus;
}

// the whole string's length; at most cap - 1 characters and a terminator go to out
int64_t copy_out(const std::string& src, char* out, int64_t cap) {
  if (out && cap > 0) {
    const size_t n = src.size() < (size_t)cap - 1 ? src.size() : (size_t)cap - 1;
    memcpy(out, src.data(), n);
    out[n] = 0;
  }
  return (int64_t)src.size();
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------
// interface used by gjx_run.hip, gjx_scanfilter.hip, gjx_peer.hip, gjx_hmc.hip
// ---------------------------------------------------------------------------------------------------------
extern "C" int gjx_jit_stats(int64_t* out4) {
  if (!out4) return GJX_EINVAL;
  out4[0] = g_rtc_compiles.load();
  out4[1] = g_disk_hits.load();
  out4[2] = g_rtc_us.load();
  { std::lock_guard<std::mutex> lock(g_mu); out4[3] = (int64_t)g_compiled.size(); }
  return GJX_OK;
}

namespace gjx {

int gen_pick_ppt(const gjx_program* prog, int64_t K, bool prefer4) {
  const int slots = register_slots(prog);
  RunVariant v;
  v.ppt = slots <= 6 ? 4 : (slots <= 24 ? 2 : 1);
  if (prefer4 && slots <= 40) v.ppt = 4;   // a block-tile of 1024 particles = one quantisation tile (tile totals, GJX_RUN_LEAVE_TILES)
  // a big affine site goes to the matrix cores: one particle per lane, whole waves (see generate())
  if (K % 256 == 0 && !getenv("GJX_GEN_PPT") && has_mfma_site(prog)) { v.ppt = 1; v.mfma = true; return encode(v); }
  // a long plate: the instances dealt to the 16 waves of a block (the wide flavour), unless the particles alone fill the machine
  // many times over (then the plain form's single pass per particle has less overhead); GJX_GEN_WIDE = 0 / 1 forces the choice
  {
    int longest = 0;
    for (int j = 0; j < prog->n_sites; ++j) if (prog->sites[j].plate && prog->sites[j].plate_n > longest) longest = prog->sites[j].plate_n;
    const char* e = getenv("GJX_GEN_WIDE");
    // (measured, vmapped mixture: N = 4096 x K = 2^17 — 256 plain blocks, one wave per SIMD — 4.1x faster wide; N = 1024 x K = 2^20 —
    // 2048 plain blocks — 8 % slower wide: the plain form wins once the particles alone give every SIMD four waves)
    const bool want = e ? atoi(e) != 0 : (longest >= 64 && K / (256 * (int64_t)v.ppt) < 1024);
    if (want && longest >= 16 && !prefer4) {
      int wp = slots <= 4 ? 2 : 1;
      if (const char* pe = getenv("GJX_GEN_PPT")) { const int q = atoi(pe); if (q == 1 || q == 2) wp = q; }
      while (wp > 1 && K % wp != 0) wp >>= 1;
      // few particles, very many instances: 4 or 16 lanes per particle until the launch has two blocks per CU
      // (measured, N = 2^16 x K = 2^12: one lane per particle, 64 blocks, 5.36 ms; 4 lanes, 256 blocks, 1.58 ms; 16 lanes, 1024 blocks, 1.28 ms)
      int lpp = 1;
      while (lpp < 16 && (K * lpp) / (64 * (int64_t)wp) < 512 && longest >= 16 * (lpp * 4) * 16 && K % (64 * wp / (lpp * 4)) == 0) lpp *= 4;
      if (const char* le = getenv("GJX_GEN_LPP")) { const int q = atoi(le); if (q == 1 || q == 4 || q == 16) lpp = q; }
      v.ppt = wp; v.wide = true; v.lpp = lpp;
      return encode(v);
    }
  }
  if (const char* e = getenv("GJX_GEN_PPT")) v.ppt = atoi(e);
  if (v.ppt != 1 && v.ppt != 2 && v.ppt != 4) v.ppt = 1;
  while (v.ppt > 1 && K % v.ppt != 0) v.ppt >>= 1;
  return encode(v);
}

// 0: a generated kernel exists (compiled now if need be); otherwise the reason is in gjx_last_error
int gen_available(const gjx_program* prog, int ppt) {
  if (!supported(prog)) return gjx_fail(GJX_EUNSUPPORTED, "codegen: program outside the emitter's coverage");
  return precompile(prog, ppt, kRun);
}

int gen_launch(const gjx_program* prog, int ppt, const GenArgs& args, int grid, hipStream_t st, hipEvent_t ev0, hipEvent_t ev1) {
  hipFunction_t fn = nullptr;
  const Compiled* c = nullptr;
  if (const int rc = function_of(prog, ppt, kRun, "gjx_gen", false, &fn, &c)) return rc;
  return launch_packed(fn, (unsigned)grid, (unsigned)c->k.block, (size_t)c->k.lds_floats * 4, st, args, "codegen: launch", ev0, ev1);
}

// ---- the steps kernel of a generated filter (gjx_scanfilter.hip): gjx_gen_steps of the module generated for `prog` ----
// two programs run through one steps kernel only if they ARE one kernel: same structure key (sites, table size, stream layout)
bool gen_same_kernel(const gjx_program* p, const gjx_program* q, int ppt) { return structure_key(p, ppt) == structure_key(q, ppt); }

// blocks of gjx_gen_steps that are resident at the same time on the current device, or 0 (no such kernel / query failed)
int gen_steps_resident_blocks(const gjx_program* prog, int ppt) {
  if (gjx_plain_launches_forced()) return 0;
  hipFunction_t fn = nullptr;
  const Compiled* c = nullptr;
  if (function_of(prog, ppt, kRun, "gjx_gen_steps", true, &fn, &c) != GJX_OK) return 0;
  return resident_blocks(fn, c->k.block, (size_t)c->k.lds_floats * 4, 6);   // (as gjx_coresident_blocks: answers above 6 per CU are not exact; tests override through gjx_filter_opts)
}

int gen_steps_launch(const gjx_program* prog, int ppt, const GenStepsArgs& args, int grid, hipStream_t st) {
  hipFunction_t fn = nullptr;
  const Compiled* c = nullptr;
  if (const int rc = function_of(prog, ppt, kRun, "gjx_gen_steps", true, &fn, &c)) return rc;
  return launch_packed(fn, (unsigned)grid, (unsigned)c->k.block, (size_t)c->k.lds_floats * 4, st, args, "codegen: launch (steps kernel)");
}

// ---- generated filter kernels (gjx_scanfilter.hip, gjx_peer.hip): gjx_gen_pf of the module generated for a step program ----
bool gen_pf_supported(const gjx_program* p) { return pf_supported(p); }
bool gen_pf_moves_supported(const gjx_program* p) { return pf_moves_supported(p); }
// two step programs run as steps of one launch only if they ARE one kernel
bool gen_pf_same_kernel(const gjx_program* p, const gjx_program* q) { return structure_key(p, 1, kFilter) == structure_key(q, 1, kFilter); }

int gen_pf_precompile(const gjx_program* prog, int spl) {
  if (!pf_supported(prog)) return gjx_fail(GJX_EUNSUPPORTED, "codegen: step program outside the filter emitter's coverage");
  return precompile(prog, spl, kFilter);
}

// blocks of gjx_gen_pf<spl> that are resident at the same time on the current device, or 0
int gen_pf_resident_blocks(const gjx_program* prog, int spl, size_t dyn_lds) {
  if (gjx_plain_launches_forced()) return 0;
  hipFunction_t fn = nullptr;
  const Compiled* c = nullptr;
  if (function_of(prog, spl, kFilter, "gjx_gen_pf", false, &fn, &c) != GJX_OK) return 0;
  return resident_blocks(fn, c->k.block, dyn_lds, 2);
}

int gen_pf_launch(const gjx_program* prog, int spl, const GenPfArgs& args, int grid, size_t dyn_lds, hipStream_t st) {
  hipFunction_t fn = nullptr;
  const Compiled* c = nullptr;
  if (const int rc = function_of(prog, spl, kFilter, "gjx_gen_pf", false, &fn, &c)) return rc;
  return launch_packed(fn, (unsigned)grid, (unsigned)c->k.block, dyn_lds, st, args, "codegen: launch (filter kernel)");
}

// ---- generated HMC kernels (gjx_hmc.hip) ----
int hmc_gen_available(const gjx_program* prog) {
  if (!hmc_plan_fold(prog)) return gjx_fail(GJX_EUNSUPPORTED, "codegen: program outside the HMC emitter's coverage");
  return precompile(prog, 0, kHmc);
}

int hmc_gen_launch(const gjx_program* prog, const HmcGenArgs& args, hipStream_t st) {
  hipFunction_t fn = nullptr;
  const Generated* k = nullptr;
  {
    std::lock_guard<std::mutex> lock(g_mu);
    const uint64_t key0 = structure_key(prog, 0, kHmc);
    const Compiled& c0 = compile(key0, prog, 0, kHmc);
    if (!c0.error.empty()) return gjx_fail(GJX_EUNSUPPORTED, c0.error.c_str());
    // few chains over long loops (the usual shape of HMC: hundreds of chains, thousands of data): more lanes per chain, until the
    // launch has about two waves per SIMD (GJX_HMC_GEN_CPL forces 4, 16 or 64)
    int variant = 0;
    {
      int want = 4;
      while (want < c0.k.cpl_max && args.n * want < 131072) want *= 4;
      if (const char* e = getenv("GJX_HMC_GEN_CPL")) want = atoi(e);
      if ((want == 16 || want == 64) && want <= c0.k.cpl_max) variant = want;
    }
    const uint64_t key = variant ? structure_key(prog, variant, kHmc) : key0;
    const Compiled& c = variant ? compile(key, prog, variant, kHmc) : c0;
    if (!c.error.empty()) return gjx_fail(GJX_EUNSUPPORTED, c.error.c_str());
    k = &c.k;
    if (k->nostale && args.stale) return gjx_fail(GJX_EUNSUPPORTED, "codegen: the LDS-state HMC kernel of this program has no room for the stale-carry compatibility mode");
    if (k->prows > 0 && (!args.ws || args.ws_floats < 4 * (int64_t)k->prows * args.n))
      return gjx_fail(GJX_EWORKSPACE, "gjx_hmc: workspace too small (selected sites inside a plate keep their trajectory state there)");
    if (const int rc = load_function(key, c, kHmc, "gjx_hmc_gen", false, &fn)) return rc;
  }
  const int64_t threads = args.n * k->cpl;
  return launch_packed(fn, (unsigned)((threads + k->block - 1) / k->block), (unsigned)k->block, 0, st, args, "codegen: launch (HMC kernel)");
}

}  // namespace gjx

// ---------------------------------------------------------------------------------------------------------
// source of a generated kernel (debugging, tests, docs): returns the length, copies at most cap - 1 characters — and compile (or
// load from the disk cache) without launch: build steps pre-populate the cache with this on machines without a GPU (hipRTC
// cross-compiles)
// ---------------------------------------------------------------------------------------------------------
extern "C" int64_t gjx_program_hmc_source(const gjx_program* prog, char* out, int64_t cap) {
  if (!prog || !prog->sites) return GJX_EINVAL;
  const Generated g = generate_hmc(prog);
  if (g.src.empty()) return gjx_fail(GJX_EUNSUPPORTED, "codegen: program outside the HMC emitter's coverage");
  return copy_out(g.src, out, cap);
}

extern "C" int gjx_program_hmc_precompile(const gjx_program* prog) {
  if (!prog || !prog->sites) return gjx_fail(GJX_EINVAL, "gjx_program_hmc_precompile: null program");
  return gjx::hmc_gen_available(prog);
}

extern "C" int64_t gjx_program_source(const gjx_program* prog, int32_t ppt, char* out, int64_t cap) {
  if (!prog || !prog->sites) return GJX_EINVAL;
  if (!supported(prog)) return gjx_fail(GJX_EUNSUPPORTED, "codegen: program outside the emitter's coverage");
  gjx::RunVariant v;
  if (!gjx::decode(ppt, &v)) ppt = gjx::gen_pick_ppt(prog, 4);
  return copy_out(generate(prog, ppt).src, out, cap);
}

extern "C" int gjx_program_precompile(const gjx_program* prog, int32_t ppt) {
  if (!prog || !prog->sites) return gjx_fail(GJX_EINVAL, "gjx_program_precompile: null program");
  gjx::RunVariant v;
  if (!gjx::decode(ppt, &v))
    return gjx_fail(GJX_EINVAL, "gjx_program_precompile: ppt must be 1, 2, 4, 257 (1 | 256: big affine sites on the matrix cores) or 513 / 514 (| 512: the instances of a plate dealt to the 16 waves of a block; | 1024 / | 2048: and to 4 / 16 lanes per particle)");
  return gjx::gen_available(prog, ppt);
}

// the filter kernel generated for a step program (GJX_FILTER_FORM_WIDE of gjx_scan_filter)
extern "C" int64_t gjx_program_filter_source(const gjx_program* step, int32_t tiles_per_block, char* out, int64_t cap) {
  if (!step || !step->sites) return GJX_EINVAL;
  const Generated g = generate_pf(step, tiles_per_block);
  if (g.src.empty()) return gjx_fail(GJX_EUNSUPPORTED, "codegen: step program outside the filter emitter's coverage");
  return copy_out(g.src, out, cap);
}

extern "C" int gjx_program_filter_precompile(const gjx_program* step, int32_t tiles_per_block) {
  if (!step || !step->sites) return gjx_fail(GJX_EINVAL, "gjx_program_filter_precompile: null program");
  gjx::FilterVariant v;
  if (!gjx::decode(tiles_per_block, &v))
    return gjx_fail(GJX_EINVAL, "gjx_program_filter_precompile: tiles_per_block must be 1, 2, 4, 8 or 16 (| 256: the flavour for sharded collections, | 512: with the rejuvenation move, | 1024: multinomial resampling by sorted uniforms, not together with | 512)");
  return gjx::gen_pf_precompile(step, tiles_per_block);
}
