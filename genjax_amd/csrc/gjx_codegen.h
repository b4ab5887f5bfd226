// gjx_codegen.h — what the runtime of the generated kernels (gjx_jit.hip) needs from their emitters (gjx_codegen.hip).
#pragma once
#include <string>
#include <vector>

#include "../../include/gjx.h"

namespace gjx_codegen {

// a generated kernel: its source (empty: the program is outside the emitter's coverage) and what its launcher has to know —
// the same numbers the source carries in its trailing comment lines
struct Generated {
  std::string src;
  int lds_floats = 0;       // dynamic LDS of gjx_gen / gjx_gen_steps, in floats
  int block = 256;          // threads per block
  int cpl = 1;              // HMC kernels: lanes per chain
  int cpl_max = 1;          // HMC kernels: the most lanes per chain the program's loops can use
  int prows = 0;            // HMC kernels: workspace rows (selected sites inside plates), x 4 x n floats
  int nostale = 0;          // HMC kernels, LDS-state flavour without room for the first gradient: no stale-carry mode
};
Generated generate(const gjx_program* prog, int ppt_code);        // gjx_gen (+ gjx_gen_steps); code: gjx::RunVariant
Generated generate_pf(const gjx_program* step, int spl_code);     // gjx_gen_pf; code: gjx::FilterVariant
Generated generate_hmc(const gjx_program* prog, int cpl_code = 0);   // gjx_hmc_gen; code: 0 (4 lanes per chain at most), 16 or 64

bool supported_uncached(const gjx_program* p);
bool pf_supported(const gjx_program* p);
bool pf_moves_supported(const gjx_program* p);
bool has_mfma_site(const gjx_program* p);
bool want_roll();
int register_slots_uncached(const gjx_program* p);
// false: the program is outside the HMC emitter's coverage; otherwise *fold (when asked for) is the emitter's data-dependent choice
// (hmc_fold_ok reads the observations): part of the kernel's identity
bool hmc_plan_fold(const gjx_program* p, std::vector<char>* fold = nullptr);

// Every environment variable the emitters read: what a kernel's source depends on besides the program and the variant code (the
// in-memory cache key folds the table in).  by_value: the value matters, otherwise only whether the variable is set.  Choices made
// per launch — GJX_GEN_PPT, GJX_GEN_WIDE, GJX_GEN_LPP, GJX_HMC_GEN_CPL — are not here: they arrive through the variant code.
struct Knob { const char* name; bool by_value; };
extern const Knob kKnobs[];
extern const int kNumKnobs;

}  // namespace gjx_codegen
