// plan_args.h -- internal: the kernel argument blocks of a plan's passes, as the engine uploads them.
// Not part of the C ABI (include/qhbm_engine.h); declared here so that the host-only plan emulator of
// tests/sanitize/ executes a plan with the product's own pruning masks and tables instead of a copy of their logic.
#pragma once
#include <cstdint>
#include <vector>

#include "program.h"
#include "schedule.h"

namespace qhbm {

// One PassArgs per pass of `plan` (zero_mask / n_free pruning included), the concatenated programs (PassArgs::prog_off)
// and the concatenated tables: spread_hi, round thread tables, relabel tables (spread_off, tl_off, relabel_off).
// (hidden: the shared library's dynamic exports stay the C ABI alone)
__attribute__((visibility("hidden"))) void fill_args(const Plan& plan, const Model& m, std::vector<PassArgs>* args, std::vector<uint32_t>* prog,
               std::vector<uint32_t>* tables);

}  // namespace qhbm
