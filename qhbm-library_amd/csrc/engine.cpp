// engine.cpp -- C ABI (include/qhbm_engine.h) on top of the scheduler and the
// gfx950 kernels.  This is the boundary a QuantumInference subclass binds
// (/root/reference/qhbmlib/inference/qnn.py:82-84,114-139).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <iterator>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "../../include/qhbm_engine.h"
#include "cross_gram_vjp_plan.h"
#include "gram_vjp_plan.h"
#include "kernels.h"
#include "plan_args.h"
#include "program.h"
#include "rdm_index.h"
#include "subsystem_plan.h"
#include "schedule.h"

using namespace qhbm;

namespace {

std::string g_create_error;

template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  // Growing an existing buffer adds an eighth on top (per-batch buffers follow the number of unique
  // bitstrings, which wanders from step to step); the first allocation is exact.
  hipError_t reserve(size_t count, bool slack = true) {
    if (count <= n) return hipSuccess;
    if (n && slack) count += count / 8;
    release();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T));
    if (e == hipSuccess) n = count;
    return e;
  }
  hipError_t upload(const std::vector<T>& h) {
    hipError_t e = reserve(h.size());
    if (e != hipSuccess || h.empty()) return e;
    return hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  }
};

template <typename T> void swap_buf(DevBuf<T>& a, DevBuf<T>& b) { std::swap(a.p, b.p); std::swap(a.n, b.n); }

struct DevicePlan {
  Plan plan;
  std::vector<PassArgs> args;
  DevBuf<uint32_t> prog, tables, rec_offsets;
  DevBuf<CoefJob> jobs;
  DevBuf<float> coef;
  bool uploaded = false;
  void swap(DevicePlan& o) {
    std::swap(plan, o.plan);
    std::swap(args, o.args);
    swap_buf(prog, o.prog); swap_buf(tables, o.tables); swap_buf(rec_offsets, o.rec_offsets);
    swap_buf(jobs, o.jobs); swap_buf(coef, o.coef);
    std::swap(uploaded, o.uploaded);
  }
};

// What follows from one pair of plans.  The engine holds two such sets: its own members (basis-state plans) and
// qhbm_engine::dense (dense-start plans of the from-states calls); swap_plan_sets exchanges them, so every routine
// below runs either set through the same members.
// INVARIANT: every member of qhbm_engine that is derived from a plan -- built by build_plans, uploaded by upload_model or
// upload_plan, or cached per gradient mask -- has a twin here AND a line in swap_plan_sets.  A plan-dependent member
// added to the engine alone would carry the basis-state plans' data into a from-states call (and back).  What is
// derived from the model alone (the observable tables: terms, obs_groups, obs_bterms, far windows, op_scale) is shared
// by both sets, which is why upload_model's early return also asks for terms.p.
struct PlanSet {
  bool plans_valid = false, adj_valid = false, model_uploaded = false;
  DevicePlan fwd, adj;
  std::vector<std::pair<std::vector<char>, std::unique_ptr<DevicePlan>>> adj_cache;
  int64_t fwd_plans_built = 0, adj_plans_built = 0;
  DevBuf<DevTerm> global_terms;
  DevBuf<int> param_slot_begin, param_slots;
  DevBuf<float> slot_factor;
  DevBuf<ShiftPhase> shift_phases;
  int n_shift_phases = 0;
  DevBuf<float> phase_slope;
  bool shift_ready = false;  // (the shift tables and coefficient copies follow the basis-state forward plan: parked here
  size_t coef_batch_programs = 0;  // while the dense-start set is in, so that building it does not reset them)
};

struct TimedEvent {
  hipEvent_t a, b;
  int kind;  // 0 forward pass, 1 adjoint pass, 2 lambda = O psi
};

}  // namespace

struct qhbm_engine {
  int device = -1;
  std::string err;
  Model model;
  bool have_circuit = false;
  // options
  int opt_tile = 0, opt_adj_tile = 0, opt_profile = 0, opt_round = 0;
  int opt_full_fwd = 60, opt_full_adj = 60, opt_force_general = 0;
  int opt_meas_tile = 0;     // tile qubits of measurement-only passes (0 = largest)
  int opt_values_from_obs = 1;  // single observable: <psi|O|psi> from lambda = O psi, no measurement in the forward sweep
  bool retained_mu = false;     // the retained batch also holds the unweighted lambda = O psi
  int opt_cph_wave_bits = 1; // boundary controlled-phase predicates on wave bits (schedule.h Plan::cph_wave_bits)
  int opt_fwd_values_obs = -1; // forward-only calls, one observable: values from the lambda = O psi kernel (no lambda stored) instead of
                               // measurements in the passes (-1: when the plan has more than one pass, i.e. the state is in HBM anyway)
  int opt_adj_stop_early = -1; // frozen parameters: the backward sweep stops at the first live gate (-1: if the time model says that is cheaper)
  int opt_adj_plan_search = 1; // adjoint: build the scheduler's best few pass orders and keep the one with the fewest model flops
  int opt_wide_last = -1;      // forward: the last gate pass may take a tile one or two bits wider (-1: unless tile_qubits is set)
  int opt_fwd_move_low = 1;    // forward: a pass may move four of its bits onto the 128-byte line positions (schedule.h PlanOptions::move_low_bits)
  int opt_fwd_pair = 1;        // dense lean forward passes run on pairs of states, tiles in registers (pass_fwd2_kernel)
  int opt_shift_prefix = 1;    // parameter shift: a shifted program starts at the pass that holds its gate, from the base program's state
  int opt_adj_relabel = 1;     // adjoint plans move finished index bits out of the 128-byte lines (schedule.h Pass)
  int opt_obs_xcd_states = -1; // lambda = O psi: one state per XCD at a time (1), every XCD an eighth of each state (0); -1: by state size
  int opt_x_two_shear = 1;   // X**t in FULL instances as two shears, the scaling folded into the table (x_shear.h); 0: always three
  int opt_adj_exchange = 1;  // lean adjoint passes: register-resident tile pair + one LDS exchange buffer
  int retained_U = 0;  // final states of the last qhbm_expectation_retain still sit in psi
  bool retained_table = false;  // ... of a qhbm_table_expectation_retain (no lambda = O psi; only the table VJP takes them)
  int state_grad_U = 0;  // rows of state_grad the last adjoint VJP filled (qhbm_state_gradients)
  int64_t opt_chunk = 0;
  int64_t opt_budget_mb = 0;  // 0: a third of the device's memory, resolved at first use (budget_bytes)
  size_t resolved_budget = 0; // the default budget of THIS engine once a device query has succeeded
  // plans
  // (everything below that follows from a plan is exchanged by swap_plan_sets with its twin in `dense`: see PlanSet's INVARIANT)
  bool plans_valid = false;
  bool adj_valid = false;  // the backward plan matches the gradient mask (qhbm_set_gradient_mask invalidates only this)
  // Backward plans (and their device copies) of the gradient masks this model has been used with: two inference paths
  // that alternate on one engine -- the same total circuit once with the data half frozen, once fully trainable --
  // swap plans instead of re-running the plan search and re-uploading on every step.  Keyed by the
  // frozen-parameter vector; cleared whenever the circuit, the observables or a planning option changes.
  std::vector<std::pair<std::vector<char>, std::unique_ptr<DevicePlan>>> adj_cache;
  int64_t fwd_plans_built = 0, adj_plans_built = 0;  // plan searches run so far (qhbm_plan_builds: a cache hit builds nothing)
  bool model_uploaded = false;  // everything upload_model copies to the device is current
  DevicePlan fwd, adj;
  DevBuf<DevTerm> terms, global_terms;  // global_terms: measured on the final state in HBM (too wide for a tile)
  DevBuf<ObsGroup> obs_groups;
  bool terms_by_op = false;  // the uploaded terms / groups are in the (mask, observable) order of gather_multi_mode
  DevBuf<ObsBTerm> obs_bterms;    // the same terms sorted and cut for the block-grouped kernels (observable.hip)
  DevBuf<ObsBGroup> obs_bgroups;
  uint32_t n_obs_bgroups = 0;
  int opt_obs_block_bits = kObsBlockBits;  // shape of the block-grouped kernels (kernels.h): 13 or 12
  int opt_obs_split_rows = 0;              // blocks of 2^13: the halves of the workgroup split the block's rows, not a group's masks
  int opt_obs_kernel = -1;      // lambda = O psi / values: 0 = one gather per mask (apply_observable_kernel), 1 = partner blocks through
                                // LDS (observable_blocks_kernel), -1 = whichever the fitted cost model prices lower (block_kernel())
  mutable int block_choice = -1;  // cached verdict of block_kernel() (-1: not computed for the installed model / options)
  int opt_gather_multi = 0;     // 2..4 observables: 1 = the gather kernel forms lambda AND carries a value accumulator per observable
                                // (one launch).  Measured slower than the block kernel's value launch + the gather launch for lambda
                                // (config 3 as XX / YY / ZZ sums: 103 against 64.7 ms, profiles/r05_xxz3_gather_multi_ab.txt): off
                                // by default, kept selectable (tests, A/B runs)
  int opt_multi_values = -1;    // several observables: values from the block kernel after lean passes (-1: when some term flips >= 2
                                // qubits or needs a measurement-only pass, at most kMultiValueOps observables)
  DevBuf<uint64_t> probe_out;  // qhbm_clock_probe's buffers
  DevBuf<float> probe_sink;
  DevBuf<float> value_part;  // value mode: one partial of <psi|O|psi> per workgroup of apply_observable_kernel
  uint32_t n_obs_groups = 0;
  uint32_t n_gather_terms = 0;  // terms of the gather kernel's FIRST launch (all of them unless far windows took some)
  // Two-level lambda = O psi (>= 26 qubits, gather kernel, single-observable modes): every mask that leaves a
  // workgroup's block makes it read a partner run from the fabric -- at 28 qubits the 17 single flips of a TFIM cost
  // 12.6 reads of the whole 2-GiB state.  Masks that flip only bits of a seven-bit WINDOW [far_hi, far_hi + 7) (and bits
  // 0..3) go to a FAR launch instead, which works in the index space where the window has changed places with bits
  // [4, 11): there they permute the workgroup's own block (LDS copy, no gather).  A far launch reads psi and reads and
  // writes lambda once (3 state-sized transfers) whatever the number of its masks.
  struct FarWindow {
    DevBuf<DevTerm> terms;
    DevBuf<ObsGroup> groups;
    uint32_t n_terms = 0, n_groups = 0, far_hi = 0;
  };
  FarWindow far[3];
  int n_far = 0;
  int opt_far_windows = 0;   // 0 (default): never -- measured: config 5 (28 qubits, 17 far single flips) 65.0 ms in one launch,
                             // 66.2 in three: the far launches move 3 state-sized transfers each as scattered 128-byte runs at about
                             // half the rate of the streaming first launch; 1: always (any window with a mask); -1: from 26 qubits up,
                             // windows with >= 3 masks
  DevBuf<float2> psi, lam;
  DevBuf<float> state_grad, slot_factor, vals_tmp, upstream_tmp, phase_cs;
  DevBuf<ShiftPhase> shift_phases;  // gates with a cirq global_shift (qhbm_statevector restores their phases)
  int n_shift_phases = 0;
  // d theta / d p of the global phase theta those two restore (pi times global_phase_kernel's sum: every exponent is linear in
  // one parameter, so the slope is a constant of the model), zero where the gradient mask switches p off [n_params]
  DevBuf<float> phase_slope;
  // batches of shifted programs: per-program coefficient buffers, ONE set of shift tables (upload_shift_tables), accumulators
  DevBuf<float> coef_batch, shift_vals, shift_weight, vals_batch;
  DevBuf<int> shift_gates, shift_param;
  DevBuf<int> shift_dst;             // execution order -> the caller's order of the programs (ProgramOrder::dst)
  ProgramOrder shift_order;          // the parameter-shift VJP's programs (valid while shift_ready)
  DevBuf<double> prog_acc;
  size_t coef_batch_programs = 0;  // copies of the forward plan's static words already in coef_batch
  bool shift_ready = false;        // the shift tables on the device are the parameter-shift VJP's and match the model
  bool shift_tables_from_obs = false;  // ... and were ordered for values taken from the observable kernel (or in the passes)
  uint32_t shift_programs = 0, shift_gate_count = 0;
  DevBuf<float> tile_grad;              // [chunk states * tiles, slots of one adjoint pass]
  DevBuf<unsigned long long> vals64;    // [U, n_ops] fixed-point accumulators of the expectation values
  DevBuf<float> op_scale, op_inv_scale; // per op: 2^(+-shift), see program.h kValueFracBits
  std::vector<float> h_op_scale, h_op_inv_scale;
  DevBuf<double> block_cum;
  DevBuf<double> par_tables;    // qhbm_sample_parities: block and sub-block prefixes of a launch set (sample_parity.hip)
  DevBuf<uint32_t> par_masks;    // ... its masks in index space
  DevBuf<int> param_slot_begin, param_slots;
  // qhbm_program_vjps: per-element copies of bitstrings and upstream rows, the base program's states of a shared prefix,
  // the gradient rows of the programs in flight, fp64 value accumulators
  DevBuf<int8_t> pv_bits;
  DevBuf<float> pv_upstream, pv_rows;
  DevBuf<float2> pv_base;
  DevBuf<double> pv_vals;
  // energy tables (energy_table.hip): per (state, y-block) value partials, per-group folds of the table gradient, the
  // fold a chunk boundary cut, the running fp64 table gradient
  DevBuf<double> tab_vpart, tab_gpart, tab_carry, tab_gsum;
  std::vector<TimedEvent> events;
  std::vector<TimedEvent> free_events;
  // Caller-supplied start states (qhbm_*_from_states).  Their plans (schedule.h Model::dense_input) are kept BESIDE the
  // basis-state plans: built on the first such call, cached per gradient mask, invalidated by the same setters.  An
  // engine that never makes such a call builds and allocates nothing of this.
  PlanSet dense;
  bool dense_active = false;      // the dense-start set is swapped into the members above (swap_plan_sets)
  bool state_grad_dense = false;  // the rows in state_grad are a from-states VJP's (slots of the dense-start backward plan)
  const float2* import_src = nullptr;     // during a from-states call: run_forward_chunk imports its chunk first
  const float* import_upstream = nullptr; // ... and multiplies the chunk's upstream rows by ||phi||^2 into import_up
  int import_U = 0;
  DevBuf<double> import_parts, import_norm2;  // import_states.hip: scratch, ||phi_u||^2 [U]
  DevBuf<float> import_up;                    // upstream rows times ||phi_u||^2
  DevBuf<int8_t> import_bits;                 // zeros: the bitstrings the pass kernels are handed (no pass reads them)
  // a caller's cotangent as lambda (qhbm_statevector_vjp_from_states; cotangent.hip): per-slice partials, <g_u|chi_u> [U, 2]
  DevBuf<double> cot_parts, cot_dot;
  // Chebyshev evolution of caller states (qhbm_evolve_states, qhbm_apply_observables; thermal.hip)
  int opt_evolve_step = 4;                    // bound on the argument x = delta R of one step ("evolve_step_argument")
  std::vector<double> evo_host_wr;            // w_k / R (or w_k) of the call in flight: the source of an asynchronous copy
  DevBuf<double> evo_wr, evo_scale, evo_parts, evo_log_norm;  // [n_ops], [chunk], norm partials, [U] when the caller wants none
  DevBuf<float> evo_up1, evo_up2;             // [chunk, n_ops] upstream rows: (w_k / R) * scale of the state, 2 w_k / R
  // Lanczos bases of caller states (qhbm_krylov_basis; krylov.hip): per-workgroup partials of a block of inner products and
  // of ||w||^2, the round's coefficients [chunk, m] complex64
  DevBuf<double> kry_parts, kry_norm_parts;
  DevBuf<float2> kry_coef;
  // streamed Lanczos (qhbm_krylov_tridiagonal, qhbm_krylov_replay): three state buffers per chunk element at the workspace's pitch
  DevBuf<float2> kry_ring;
};

namespace {

int fail(qhbm_engine* h, const std::string& msg) {
  if (h) h->err = msg; else g_create_error = msg;
  return 1;
}

#define HIPCHK(expr)                                                                   \
  do {                                                                                 \
    hipError_t _e = (expr);                                                            \
    if (_e != hipSuccess)                                                              \
      return fail(h, std::string(#expr) + ": " + hipGetErrorString(_e));               \
  } while (0)

template <typename T> size_t buf_bytes(const DevBuf<T>& b) { return b.n * sizeof(T); }
size_t plan_bytes(const DevicePlan& d) {
  return buf_bytes(d.prog) + buf_bytes(d.tables) + buf_bytes(d.rec_offsets) + buf_bytes(d.jobs) + buf_bytes(d.coef);
}
// Every byte of device memory the engine holds (qhbm_allocated_bytes; a host-side engine cache bounds
// its footprint with it).
size_t own_bytes(const qhbm_engine* h) {
  return buf_bytes(h->psi) + buf_bytes(h->lam) + buf_bytes(h->state_grad) + buf_bytes(h->tile_grad) +
         buf_bytes(h->vals64) + buf_bytes(h->block_cum) + buf_bytes(h->par_tables) + buf_bytes(h->par_masks) + buf_bytes(h->coef_batch) + buf_bytes(h->vals_batch) +
         buf_bytes(h->value_part) + buf_bytes(h->probe_out) + buf_bytes(h->probe_sink) + buf_bytes(h->upstream_tmp) + buf_bytes(h->vals_tmp) + buf_bytes(h->prog_acc) +
         buf_bytes(h->shift_vals) + buf_bytes(h->shift_weight) + buf_bytes(h->shift_gates) + buf_bytes(h->shift_param) + buf_bytes(h->shift_dst) +
         buf_bytes(h->slot_factor) + buf_bytes(h->phase_cs) + buf_bytes(h->shift_phases) + buf_bytes(h->phase_slope) + buf_bytes(h->terms) +
         buf_bytes(h->global_terms) + buf_bytes(h->obs_groups) + buf_bytes(h->far[0].terms) + buf_bytes(h->far[0].groups) +
         buf_bytes(h->far[1].terms) + buf_bytes(h->far[1].groups) + buf_bytes(h->far[2].terms) + buf_bytes(h->far[2].groups) + buf_bytes(h->obs_bterms) + buf_bytes(h->obs_bgroups) + buf_bytes(h->op_scale) + buf_bytes(h->op_inv_scale) +
         buf_bytes(h->param_slot_begin) + buf_bytes(h->param_slots) + buf_bytes(h->pv_bits) + buf_bytes(h->pv_upstream) +
         buf_bytes(h->pv_rows) + buf_bytes(h->pv_base) + buf_bytes(h->pv_vals) + buf_bytes(h->tab_vpart) + buf_bytes(h->tab_gpart) +
         buf_bytes(h->tab_carry) + buf_bytes(h->tab_gsum) + plan_bytes(h->fwd) + plan_bytes(h->adj) + [&] {
           size_t cached = 0;  // backward plans of other gradient masks, kept with their device copies (adj_cache)
           for (const auto& kv : h->adj_cache) cached += plan_bytes(*kv.second);
           return cached;
         }() + [&] {  // the other plan set and the import's buffers (nothing before the first from-states call)
           const PlanSet& o = h->dense;
           size_t b = plan_bytes(o.fwd) + plan_bytes(o.adj) + buf_bytes(o.global_terms) + buf_bytes(o.param_slot_begin) +
                      buf_bytes(o.param_slots) + buf_bytes(o.slot_factor) + buf_bytes(o.shift_phases) + buf_bytes(o.phase_slope) + buf_bytes(h->cot_parts) + buf_bytes(h->cot_dot) + buf_bytes(h->import_parts) +
                      buf_bytes(h->import_norm2) + buf_bytes(h->import_up) + buf_bytes(h->import_bits) + buf_bytes(h->evo_wr) +
                      buf_bytes(h->evo_scale) + buf_bytes(h->evo_parts) + buf_bytes(h->evo_log_norm) + buf_bytes(h->evo_up1) +
                      buf_bytes(h->evo_up2) + buf_bytes(h->kry_parts) + buf_bytes(h->kry_norm_parts) + buf_bytes(h->kry_coef) + buf_bytes(h->kry_ring);
           for (const auto& kv : o.adj_cache) b += plan_bytes(*kv.second);
           return b;
         }();
}

// "This call consumes the workspace": the states a retaining forward left in psi are overwritten or un-applied in place,
// and the rows in state_grad are no finished adjoint VJP's any more (qhbm_state_gradients is refused until
// reduce_state_grad).  A forward-only sweep overwrites psi alone and resets retained_U alone (run_sweep).
void consume_workspace(qhbm_engine* h) {
  h->retained_U = 0;
  h->state_grad_U = 0;
}

// The ONE place where a setter declares the plans out of date (qhbm_set_circuit, qhbm_set_observables, the planning
// options).  What was computed under them goes with them: the states a retaining forward left in psi, and the
// per-state slot rows of the last adjoint VJP -- a rebuilt plan orders its slots, and maps them to parameters, in its
// own way, so qhbm_state_gradients would scatter the old rows through the new plan's tables (and read past them if the
// new plan has more slots).  qhbm_set_gradient_mask drops both itself: it invalidates the backward plan alone.
void invalidate_plans(qhbm_engine* h) {
  h->plans_valid = false;
  h->dense.plans_valid = false;  // (the dense-start plans of the from-states calls: the same setters)
  consume_workspace(h);
}

// Exchanges the basis-state plans and everything uploaded for them with the dense-start set (PlanSet), and plans for
// the matching kind of start state from then on.
void swap_plan_sets(qhbm_engine* h) {
  PlanSet& o = h->dense;
  std::swap(h->plans_valid, o.plans_valid);
  std::swap(h->adj_valid, o.adj_valid);
  std::swap(h->model_uploaded, o.model_uploaded);
  h->fwd.swap(o.fwd);
  h->adj.swap(o.adj);
  h->adj_cache.swap(o.adj_cache);
  std::swap(h->fwd_plans_built, o.fwd_plans_built);
  std::swap(h->adj_plans_built, o.adj_plans_built);
  swap_buf(h->global_terms, o.global_terms);
  swap_buf(h->param_slot_begin, o.param_slot_begin);
  swap_buf(h->param_slots, o.param_slots);
  swap_buf(h->slot_factor, o.slot_factor);
  swap_buf(h->shift_phases, o.shift_phases);
  std::swap(h->n_shift_phases, o.n_shift_phases);
  swap_buf(h->phase_slope, o.phase_slope);
  std::swap(h->shift_ready, o.shift_ready);
  std::swap(h->coef_batch_programs, o.coef_batch_programs);
  h->dense_active = !h->dense_active;
  h->model.dense_input = h->dense_active;
}

// The dense-start set for the length of a from-states call.
struct DenseScope {
  qhbm_engine* h;
  explicit DenseScope(qhbm_engine* e) : h(e) { swap_plan_sets(h); }
  ~DenseScope() {
    h->import_src = nullptr;
    h->import_upstream = nullptr;
    swap_plan_sets(h);
  }
  DenseScope(const DenseScope&) = delete;
  DenseScope& operator=(const DenseScope&) = delete;
};

int need_device(qhbm_engine* h) {
  if (h->device < 0)
    return fail(h, "engine was created without a device (planning only); no CPU fallback exists");
  HIPCHK(hipSetDevice(h->device));
  return 0;
}

}  // namespace

// (declared in plan_args.h: the host-only plan emulator of tests/sanitize/ executes plans with these arguments)
void qhbm::fill_args(const Plan& plan, const Model& m, std::vector<PassArgs>* args, std::vector<uint32_t>* prog,
                     std::vector<uint32_t>* tables) {
  args->clear();
  prog->clear();
  tables->clear();
  for (const Pass& p : plan.passes) {
    PassArgs a;
    std::memset(&a, 0, sizeof(a));
    a.flags = p.flags;
    a.n = uint32_t(plan.n_eff);
    a.c = uint32_t(p.c);
    a.n_nonlocal = uint32_t(p.nonlocal_pos.size());
    a.prog_off = uint32_t(prog->size());
    a.spread_off = uint32_t(tables->size());
    a.spread_shift = 0;  // K == c: the only entry is 0
    for (size_t i = size_t(p.c); i < p.local_phys.size(); ++i) {
      if (i == size_t(p.c)) a.spread_shift = uint32_t(p.local_phys[i]);
      else if (p.local_phys[i] != p.local_phys[i - 1] + 1) { a.spread_shift = 0xffffffffu; break; }
    }
    a.n_ops = uint32_t(m.n_ops);
    a.slot_base = uint32_t(p.slot_base);
    a.n_slots = uint32_t(p.n_slots);
    for (size_t i = 0; i < p.nonlocal_phys.size(); ++i) a.nonlocal_pos[i] = uint8_t(p.nonlocal_phys[i]);
    for (size_t i = 0; i < p.local_phys.size(); ++i) a.local_pos[i] = uint8_t(p.local_phys[i]);
    for (size_t bit = 0; bit < 32; ++bit) a.phys_of[bit] = uint8_t(bit < p.phys_of.size() ? p.phys_of[bit] : int(bit));
    for (size_t bit = 0; bit < 32; ++bit) a.log_of[a.phys_of[bit]] = uint8_t(bit);
    for (size_t i = 0; i < p.nonlocal_phys.size(); ++i) a.nonlocal_mask |= 1u << p.nonlocal_phys[i];
    for (uint32_t I = 0; I < 8; ++I) {  // (the pass kernels give a thread eight float4 of its tile: kernels.hip prefetch_tile)
      const uint32_t l = p.K >= 3 ? I << (p.K - 3) : 0u, hi = l >> a.c;
      a.row_off[I] = (l & ((1u << a.c) - 1u)) |
                     (a.spread_shift != 0xffffffffu ? hi << a.spread_shift : (hi < p.spread.size() ? p.spread[hi] : 0u));
    }
    a.frozen_old_local = p.frozen_old_local;
    prog->insert(prog->end(), p.prog.begin(), p.prog.end());
    tables->insert(tables->end(), p.spread.begin(), p.spread.end());
    a.tl_off = uint32_t(tables->size());
    tables->insert(tables->end(), p.round_tl.begin(), p.round_tl.end());
    if (p.flags & PASS_RELABEL) {
      a.frozen_new_local = p.frozen_new_local;
      while (tables->size() % 4) tables->push_back(0u);  // the store reads (l0, off0, l1, off1) as one 16-byte word
      a.relabel_off = uint32_t(tables->size());
      tables->insert(tables->end(), p.relabel_tab.begin(), p.relabel_tab.end());
      // consecutive live out-indices are adjacent amplitudes iff the lowest position the tile owns is address bit 0
      a.relabel_pairs = (p.local_phys[0] == 0 && !(p.frozen_new_local == ((1u << p.K) - 1u))) ? 1u : 0u;
      uint32_t n_live = 0;
      for (int i = 0; i < p.K; ++i) n_live += !(p.frozen_new_local >> i & 1u);
      if (n_live < 1) a.relabel_pairs = 0;
      std::memset(a.fz_src, 0xff, sizeof(a.fz_src));
      for (int i = 0; i < p.K; ++i)
        if (p.frozen_new_local >> i & 1u) {
          a.fz_local_bit[a.n_fz] = uint8_t(i);
          a.fz_out_pos[a.n_fz] = uint8_t(p.store_local_phys[size_t(i)]);
          a.fz_src[p.store_local_phys[size_t(i)]] = uint8_t(i);
          ++a.n_fz;
        }
      // (kernels.hip store_tile_relabeled: a thread's out-indices are (tid + i * threads) [* 2 for pairs])
      const uint32_t threads = 1u << (p.K - 4), entries = uint32_t(p.relabel_tab.size() / 2);
      const uint32_t count = a.relabel_pairs ? entries / 2 : entries;
      uint32_t shift = uint32_t(p.K - 4) + (a.relabel_pairs ? 1u : 0u);
      a.relabel_iters = (count + threads - 1) / threads;
      a.relabel_l1 = entries > 1 ? p.relabel_tab[2] : 0u;
      for (uint32_t i = 0; i < 16; ++i) {
        const uint64_t o = uint64_t(i) << shift;
        a.relabel_hi[i][0] = o < entries ? p.relabel_tab[2 * size_t(o)] : 0u;
        a.relabel_hi[i][1] = o < entries ? p.relabel_tab[2 * size_t(o) + 1] : 0u;
      }
    }
    args->push_back(a);
  }
  if (!plan.adjoint && !plan.dense_input) {  // (a caller-supplied start state has no zeros to count on)
    // Amplitude-space pruning of the head of the forward sweep: an index bit no non-diagonal op has
    // acted on yet still equals the input bitstring wherever psi is non-zero.  A tile of pass p that
    // differs from the input on such a bit among its NON-LOCAL bits is identically zero, stays zero
    // under the pass, and already reads as zeros in HBM (the first pass wrote them): the kernel
    // returns at once.  Config 3: half the tiles of the second (and heaviest) forward pass.
    uint32_t touched = 0;  // logical bits
    for (size_t i = 0; i < args->size(); ++i) {
      uint32_t nl = 0;
      for (uint32_t k = 0; k < (*args)[i].n_nonlocal; ++k) nl |= 1u << (*args)[i].nonlocal_pos[k];
      uint32_t touched_phys = 0;  // ... at the positions they have when pass i loads its tiles (plans that move the low bits)
      for (size_t bit = 0; bit < plan.passes[i].phys_of.size(); ++bit)
        if (touched >> bit & 1u) touched_phys |= 1u << plan.passes[i].phys_of[bit];
      if (i > 0) (*args)[i].zero_mask = nl & ~touched_phys;
      touched |= plan.passes[i].mat_bits;
    }
  }
  if (plan.adjoint) {
    // Amplitude-space pruning of the tail of the backward sweep.  At the start of adjoint pass p,
    // psi is (the circuit's FIRST ops, those of passes p..last) applied to the basis state, and no
    // bit that is non-local in all of those passes has been acted on other than diagonally: psi is
    // zero wherever such a bit differs from the input bitstring, so those tiles add nothing to any
    // gradient, and lambda there is only ever paired with zero psi in later passes.  The kernel
    // skips them outright.
    // "Acted on" means by a non-diagonal op of pass p or later; a bit that is local in a later pass
    // without a gate there (the low bits every tile holds, padding) is as good: the tiles skipped now
    // are read again then, but hold zeros of psi (to rounding) next to a stale lambda.
    uint32_t later_mat = plan.dense_tail ? ~0u : 0u;  // logical bits (dense_tail: the sweep does not end at the basis state)
    for (size_t i = args->size(); i-- > 0;) {
      uint32_t nl = 0;
      for (uint32_t k = 0; k < (*args)[i].n_nonlocal; ++k) nl |= 1u << (*args)[i].nonlocal_pos[k];
      later_mat |= plan.passes[i].mat_bits;
      uint32_t later_phys = 0;  // ... at the positions they have when pass i loads its tiles
      for (size_t bit = 0; bit < plan.passes[i].phys_of.size(); ++bit)
        if (later_mat >> bit & 1u) later_phys |= 1u << plan.passes[i].phys_of[bit];
      (*args)[i].zero_mask = nl & ~later_phys;
    }
  }
  for (size_t i = 0; i < args->size(); ++i) {
    PassArgs& a = (*args)[i];
    // the first forward pass writes ONE tile per state when nothing has to be zero-filled: every tile-id bit
    // follows the input bitstring
    if ((a.flags & PASS_INIT_BASIS) && (a.flags & PASS_NO_ZERO_FILL))
      for (uint32_t k = 0; k < a.n_nonlocal; ++k) a.zero_mask |= 1u << a.nonlocal_pos[k];
    a.n_free = a.n_nonlocal - uint32_t(__builtin_popcount(a.zero_mask));
  }
}

namespace {

double pass_flops_per_amplitude(const Plan& plan, const Pass& p, const uint32_t* dyn = nullptr);

// Modelled time of the adjoint sweep per state, in seconds: per pass the larger of its arithmetic at the rate the
// pass kernel sustains (67 TFLOP/s of qhbm_flop_model's flops: 65-69 over 20...28 qubits, depths 16 and 32, tiles of
// 2^12 and 2^13, scripts/adj_tile_ab.sh) and its tile traffic (qhbm_traffic_model's bytes) at 5.5 TB/s, the rate of
// a pass with nothing to compute (config 3: 24.6 ms per 4096 state pairs read and written).
double adjoint_plan_seconds(const Plan& plan, const Model& m) {
  std::vector<PassArgs> args;
  std::vector<uint32_t> prog, tables;
  fill_args(plan, m, &args, &prog, &tables);
  const double amps = double(size_t(1) << plan.n_eff);
  double t = 0.0;
  for (size_t i = 0; i < args.size(); ++i) {
    const Pass& p = plan.passes[i];
    const double live = 1.0 / double(1ull << __builtin_popcount(args[i].zero_mask));
    int low_missing = 0;  // a tile without some of the four low index bits still moves whole 128-byte lines
    for (uint32_t k = 0; k < args[i].n_nonlocal; ++k) low_missing += args[i].nonlocal_pos[k] < 4;
    const double lines = std::min(1.0, live * double(1u << low_missing));
    const double write_share = (p.flags & PASS_RELABEL) ? 1.0 / double(1u << __builtin_popcount(p.frozen_new_local)) : 1.0;
    const double bytes = lines * amps * 8.0 * 2.0 * (1.0 + ((p.flags & PASS_STORE) ? write_share : 0.0));
    const double flops = live * amps * pass_flops_per_amplitude(plan, p);
    // (+ a tenth of the traffic time: what the start and the end of a pass -- tiles loading, tiles draining -- add to
    // a pass bound by arithmetic; fitted on orders with 6...8 passes more than their rivals, scripts/adj_search_ab.sh)
    t += std::max(flops / 67e12, bytes / 5.5e12) + 0.1 * bytes / 5.5e12;
  }
  return t;
}

// The layout a forward pass loads is the one the pass before it stored, and the circuit ends in logical = physical: a
// function of the pass index alone.  Everything that enters the sweep behind pass 0 leans on this -- a shifted program
// that starts at pass k from the base program's state (order_programs, psi_src), the base state advanced by pass k
// (advance_base) -- and so does every consumer of final states.
bool forward_layouts_chain(const Plan& plan) {
  if (plan.passes.empty()) return true;
  std::vector<int> layout = plan.passes[0].phys_of;
  for (const Pass& p : plan.passes) {
    if (p.phys_of != layout) return false;
    if (!p.store_local_phys.empty()) {
      if (p.store_local_phys.size() != p.local_pos.size() || !(p.flags & PASS_RELABEL)) return false;
      for (size_t k = 0; k < p.local_pos.size(); ++k) layout[size_t(p.local_pos[k])] = p.store_local_phys[k];
    }
    if (p.completes_circuit || p.is_measure_only)
      for (size_t b = 0; b < layout.size(); ++b) if (layout[b] != int(b)) return false;
  }
  return true;
}

int build_plans(qhbm_engine* h) {
  if (h->plans_valid && h->adj_valid) return 0;  // (whoever invalidated them dropped the retained states and the VJP rows)
  if (!h->have_circuit) return fail(h, "qhbm_set_circuit has not been called");
  if (h->model.n_ops > kMaxOps) return fail(h, "too many observables (max 1024)");
  std::string err;
  if (!h->plans_valid) {  // (a change of the gradient mask alone keeps the forward plan: it does not depend on it)
    h->adj_cache.clear();
    PlanOptions fo;
    fo.tile_bits = h->opt_tile;
    fo.round_bits = h->opt_round;
    fo.full_threshold = h->opt_full_fwd;
    fo.meas_tile_bits = h->opt_meas_tile;
    fo.cph_wave_bits = h->opt_cph_wave_bits != 0;
    fo.wide_last_pass = h->opt_wide_last;
    fo.move_low_bits = h->opt_fwd_move_low;
    if (!build_plan(h->model, fo, &h->fwd.plan, &err)) return fail(h, "forward plan: " + err);
    if (!forward_layouts_chain(h->fwd.plan)) return fail(h, "internal: the forward passes' layouts do not chain to the identity");
    h->fwd.uploaded = false;
    ++h->fwd_plans_built;
  }
  // The backward plan.  Its pass kernel runs at the same fp32 rate whatever the plan (adjoint_plan_seconds), so the
  // plan with the least modelled time -- arithmetic, or tile traffic where a pass has little to compute -- is kept:
  //  * the scheduler's search ranks pass orders by a proxy (gates x live share); the best few complete orders and
  //    the greedy one are built out and compared;
  //  * with the tile size left to the engine, the same is done with tiles of 2^13 amplitudes, which win where no
  //    index bit finishes early and every pass is a full pass (depth-32 TFIM: - 5...9 %), and lose on chains that
  //    prune early (config 3: + 8 %).
  const bool relabel = h->opt_adj_relabel != 0 && h->opt_adj_exchange != 0;
  auto plan_adjoint_of = [&](const Model& model, int tile, Plan* out, double* seconds, std::string* e) {
    PlanOptions ao;
    ao.tile_bits = tile;
    ao.adjoint = true;
    ao.full_threshold = h->opt_full_adj;
    ao.cph_wave_bits = h->opt_cph_wave_bits != 0;
    ao.relabel = relabel;
    if (!build_plan(model, ao, out, e)) return false;
    *seconds = adjoint_plan_seconds(*out, model);
    if (!h->opt_adj_plan_search) return true;
    const std::vector<std::vector<uint32_t>> orders = out->candidate_orders;
    for (const std::vector<uint32_t>& order : orders) {
      Plan alt;
      std::string e2;
      ao.forced_order = &order;
      if (!build_plan(model, ao, &alt, &e2)) continue;
      const double f = adjoint_plan_seconds(alt, model);
      if (std::getenv("QHBM_PLAN_DEBUG"))
        std::fprintf(stderr, "[plan] tile %d candidate with %zu passes: %.4g ms per state (kept so far: %zu passes, %.4g ms)\n", tile,
                     alt.passes.size(), f * 1e3, out->passes.size(), *seconds * 1e3);
      if (f < 0.99 * *seconds) { *out = std::move(alt); *seconds = f; }
    }
    return true;
  };
  //  * with frozen parameters (qhbm_set_gradient_mask) the sweep may stop at the first gate of a live parameter --
  //    but what is left of psi there is no basis state, and nothing can be pruned any more: for a shallow circuit
  //    the full sweep with its pruned tail is the cheaper one.  Both are planned.
  auto plan_adjoint = [&](int tile, Plan* out, double* seconds, std::string* e) {
    bool any_live = false;  // (no live parameter at all: nothing to sweep, whatever the option says)
    for (const Gate& G : h->model.gates) any_live |= G.param_idx >= 0 && !h->model.frozen(G.param_idx);
    if (h->opt_adj_stop_early == 0 && !h->model.param_frozen.empty() && any_live) {
      Model whole = h->model;
      whole.stop_at_first_live_gate = false;
      return plan_adjoint_of(whole, tile, out, seconds, e);
    }
    if (!plan_adjoint_of(h->model, tile, out, seconds, e)) return false;
    if (h->opt_adj_stop_early < 0 && !h->model.param_frozen.empty() && out->dense_tail) {
      Model whole = h->model;
      whole.stop_at_first_live_gate = false;
      Plan alt;
      std::string e2;
      double f = 0.0;
      if (plan_adjoint_of(whole, tile, &alt, &f, &e2) && f < *seconds) { *out = std::move(alt); *seconds = f; }
    }
    return true;
  };
  double adj_seconds = 0.0;
  if (!plan_adjoint(h->opt_adj_tile, &h->adj.plan, &adj_seconds, &err)) return fail(h, "adjoint plan: " + err);
  if (h->opt_adj_tile == 0 && h->opt_adj_exchange != 0 && h->adj.plan.K == 12 && h->adj.plan.passes.size() > 1 &&
      h->adj.plan.n_eff >= 14) {
    Plan wide;
    std::string err2;
    double wide_seconds = 0.0;
    // (tiles of 2^13 run 3 - 4 % slower against 2^12 than the model says -- two workgroups of eight waves per CU overlap
    // their tile I/O worse than four of four; seven shapes, profiles/r05_adjoint_tile_choice.txt: they must win by that)
    if (plan_adjoint(13, &wide, &wide_seconds, &err2) && wide.K == 13 && wide_seconds < 0.966 * adj_seconds)
      h->adj.plan = std::move(wide);
  }
  h->adj.uploaded = false;
  ++h->adj_plans_built;
  h->model_uploaded = false;
  h->shift_ready = false;
  if (!h->plans_valid) h->coef_batch_programs = 0;
  h->plans_valid = true;
  h->adj_valid = true;
  return 0;
}

int upload_plan(qhbm_engine* h, DevicePlan* d) {
  if (d->uploaded) return 0;
  std::vector<uint32_t> prog, tables;
  fill_args(d->plan, h->model, &d->args, &prog, &tables);
  HIPCHK(d->prog.upload(prog));
  HIPCHK(d->tables.upload(tables));
  if (h->opt_x_two_shear) {
    HIPCHK(d->jobs.upload(d->plan.jobs));
  } else {  // every X job keeps the three-shear form
    std::vector<CoefJob> jobs = d->plan.jobs;
    for (CoefJob& jb : jobs) jb.x_full = 0;
    HIPCHK(d->jobs.upload(jobs));
  }
  HIPCHK(d->rec_offsets.upload(d->plan.record_offsets));
  {
    std::vector<float> init(d->plan.coef_init.size() + 64, 0.f);
    std::memcpy(init.data(), d->plan.coef_init.data(), d->plan.coef_init.size() * sizeof(uint32_t));
    HIPCHK(d->coef.upload(init));
  }
  d->uploaded = true;
  return 0;
}

// One term of the block-grouped kernels (kernels.h ObsBTerm): slot bits of the block layout are index bits 0, 10, 11, 12
// (blocks of 2^12: 0, 10, 11).
ObsBTerm obs_block_term(const DevTerm& d, bool new_mask, int bb) {
  const uint32_t xin = d.x & ((1u << bb) - 1u), rows = (1u << (bb - 10)) - 1u;
  const uint32_t zs = (d.z & 1u) | (((d.z >> 10) & rows) << 1);
  // variant (scripts/gen_observable_asm.py): Z bits of the three low slot bits | base sign << 3 | odd x << 4 | imaginary << 5
  const uint32_t variant = (zs & 7u) | ((xin & 1u) << 4) | ((d.ny & 1u) << 5);
  const uint32_t chunk = kObsChunkBytes, preamble = kObsPreambleBytes;
  ObsBTerm t;
  t.coeff = d.coeff;
  t.zt = (d.z >> 1) & 511u;
  t.zb = d.z >> bb;
  t.xrow = (((xin >> 1) & 511u) << 4) | (((xin >> 10) & rows) << 13);
  t.off0 = variant * chunk + preamble;
  t.off1 = (variant | (zs & 8u)) * chunk + preamble;
  // sign at the own index: (-1)^ny from the x & z overlap, and i^2 = -1 once ny >= 2
  t.meta = (d.op & 1023u) | (new_mask ? kObsNewMask : 0u) | (((d.ny + (d.ny >> 1)) & 1u) ? kObsSignBit : 0u);
  t.pad = 0u;
  return t;
}

// Copies plans, observable tables and the parameter -> slot map to the device ONCE per model: a
// compute call on an unchanged model issues no host copy and no synchronisation (it can be captured
// into a hipGraph by the caller).
bool gather_multi_mode(const qhbm_engine* h);  // (below, with the other mode predicates)

int upload_model(qhbm_engine* h) {
  if (int rc = build_plans(h)) return rc;
  if (h->terms.p && h->terms_by_op != gather_multi_mode(h)) {  // an option changed which order the gather kernel wants
    h->terms.release();
    h->model_uploaded = false;
  }
  // (the observable tables serve both plan sets: whoever released them -- an option, new observables -- is seen by either)
  if (h->model_uploaded && h->terms.p) return 0;
  if (int rc = upload_plan(h, &h->fwd)) return rc;
  if (int rc = upload_plan(h, &h->adj)) return rc;
  if (!h->terms.p) {
    // lambda = O psi gathers psi[j ^ x] once per distinct x mask: sort by x, cut into groups
    std::vector<DevTerm> t;
    for (const PauliTerm& pt : h->model.terms)
      t.push_back(DevTerm{pt.coeff, pt.x, pt.z, uint32_t(pt.ny), uint32_t(pt.op)});
    // (several observables with a value accumulator each -- gather_multi_mode --: by mask, then by observable; a group is
    // one observable's share of a mask and re-uses the partners its predecessor gathered when the mask is the same)
    const bool by_op = gather_multi_mode(h);
    h->terms_by_op = by_op;
    // the gather kernel's tables of a term list: sorted by mask (then observable), cut into groups, sign classes in order
    auto gather_tables = [&](std::vector<DevTerm>& t, std::vector<ObsGroup>* groups) {
      std::stable_sort(t.begin(), t.end(), [by_op](const DevTerm& a, const DevTerm& b) {
        return a.x != b.x ? a.x < b.x : (by_op && a.op < b.op);
      });
      groups->clear();
      for (size_t k = 0; k < t.size(); ++k) {
        const bool new_mask = k == 0 || t[k].x != t[k - 1].x;
        if (new_mask || (by_op && t[k].op != t[k - 1].op) || k % (kObsTermChunk / 2) == 0) {
          // same_x bit 0 ("re-use the predecessor's partners") only in (mask, observable) order, where bit 1 makes every
          // group fetch ALL its pairs: in the default order a mask cut at a chunk boundary gathers again, because its first
          // part may have fetched only the pairs it does not vanish on (or nothing at all)
          groups->push_back(ObsGroup{t[k].x, 0, 0, 0, 0, t[k].op, by_op ? (new_mask ? 2u : 3u) : 0u});
        }
        groups->back().end = uint32_t(k + 1);
        groups->back().has_imag |= t[k].ny & 1u;
      }
      // order the terms of every real-weight group by sign class (kernels.h ObsGroup)
      const uint32_t smask = obs_slot_mask(uint32_t(h->fwd.plan.n_eff));
      auto cls = [&](const DevTerm& d) { return (d.z & kObsThreadMask) == 0 ? 0 : ((d.z & smask) == 0 ? 1 : 2); };
      size_t begin = 0;
      for (ObsGroup& g : *groups) {
        if (!g.has_imag) {
          std::stable_sort(t.begin() + begin, t.begin() + g.end,
                           [&](const DevTerm& a, const DevTerm& b) { return cls(a) < cls(b); });
          for (size_t k = begin; k < g.end; ++k) {
            g.n_h += cls(t[k]) == 0;
            g.n_l += cls(t[k]) == 1;
          }
        }
        begin = g.end;
      }
    };
    // (the kernel skips a group's gather on same_x bit 0 and trusts that the predecessor fetched EVERY pair, which only bit 1
    // guarantees: round 5's wrong-value bug was a table with bit 0 alone)
    auto tables_ok = [](const std::vector<ObsGroup>& groups) {
      for (const ObsGroup& g : groups)
        if ((g.same_x & 1u) && !(g.same_x & 2u)) return false;
      return true;
    };
    std::vector<DevTerm> full = t;  // (every term, in the gather order: what the block-grouped tables below start from)
    {
      std::vector<ObsGroup> unused;
      gather_tables(full, &unused);
    }
    // far windows of the two-level sweep (qhbm_engine::FarWindow): top seven bits first
    h->n_far = 0;
    const int n_eff = h->fwd.plan.n_eff;
    const bool far_on = !by_op && obs_amps_per_thread(uint32_t(n_eff)) == 8u &&
                        (h->opt_far_windows > 0 || (h->opt_far_windows < 0 && n_eff >= 26));
    if (far_on) {
      for (int hi = n_eff - 7; hi >= 11 && h->n_far < 3; hi -= 7) {
        const uint32_t window = 0x7fu << hi;
        auto takes = [&](const DevTerm& d) { return (d.x & window) != 0u && (d.x & ~(window | 0xfu)) == 0u; };
        std::vector<uint32_t> masks;
        for (const DevTerm& d : t) if (takes(d)) masks.push_back(d.x);
        std::sort(masks.begin(), masks.end());
        masks.erase(std::unique(masks.begin(), masks.end()), masks.end());
        if (masks.size() < (h->opt_far_windows > 0 ? 1u : 3u)) continue;  // (three state-sized transfers must buy something)
        auto virt = [&](uint32_t v) {  // physical -> virtual index bits: the window changes places with bits [4, 11)
          const uint32_t lo = (v >> 4) & 0x7fu, top = (v >> hi) & 0x7fu;
          return (v & ~((0x7fu << 4) | window)) | (top << 4) | (lo << hi);
        };
        std::vector<DevTerm> ft, rest;
        for (const DevTerm& d : t) {
          if (takes(d)) ft.push_back(DevTerm{d.coeff, virt(d.x), virt(d.z), d.ny, d.op});
          else rest.push_back(d);
        }
        t.swap(rest);
        std::vector<ObsGroup> fg;
        gather_tables(ft, &fg);
        if (!tables_ok(fg)) return fail(h, "observable tables: a group re-uses partners its predecessor need not have fetched");
        qhbm_engine::FarWindow& w = h->far[h->n_far++];
        HIPCHK(w.terms.upload(ft));
        HIPCHK(w.groups.upload(fg));
        w.n_terms = uint32_t(ft.size());
        w.n_groups = uint32_t(fg.size());
        w.far_hi = uint32_t(hi);
      }
    }
    std::vector<ObsGroup> groups;
    gather_tables(t, &groups);
    if (!tables_ok(groups)) return fail(h, "observable tables: a group re-uses partners its predecessor need not have fetched");
    if (t.empty()) t.push_back(DevTerm{0.f, 0u, 0u, 0u, 0u});  // (every term went to a far window: the first launch still writes lambda = 0)
    HIPCHK(h->terms.upload(t));
    HIPCHK(h->obs_groups.upload(groups));
    h->n_obs_groups = uint32_t(groups.size());
    h->n_gather_terms = uint32_t(groups.empty() ? 0u : groups.back().end);
    {  // block-grouped order (kernels.h ObsBTerm): by partner block x >> block bits, then by mask, then by observable
      const int bb = h->opt_obs_block_bits;
      std::vector<DevTerm> bt = full;
      std::stable_sort(bt.begin(), bt.end(), [bb](const DevTerm& a, const DevTerm& b) {
        const uint32_t ao = a.x >> bb, bo = b.x >> bb;
        if (ao != bo) return ao < bo;
        if (a.x != b.x) return a.x < b.x;
        return a.op < b.op;
      });
      std::vector<ObsBTerm> terms2;
      std::vector<ObsBGroup> groups2;
      // A UNIT = the masks one step of the kernel applies from one fetched partner block.  The phase-timing build of
      // the kernel (-DQHBM_OBS_TIMING, profiles/r04_c4_observable_experiments.txt) shows a step of ~2750 cycles as
      // 15 - 25 % the 64-KiB store burst into LDS, 33 - 43 % the masks (~790 cycles per term and wave: 8 KiB of LDS reads
      // each), 18 - 32 % barrier skew, and NO time waiting for the prefetched blocks -- but the pipeline runs only three
      // blocks ahead, and after a group with many masks (x_out = 0: 65 of config 4's 480) it would.  Inside a window of
      // partner blocks (x_out >> 5: what the L2 holds at a time -- the order inside it is free) heavy and light units
      // therefore ALTERNATE (config 4: 53.6 -> 52.8 ms).  Cutting a heavy group into several units that fetch the block
      // again was measured and lost (units of at most 16 / 8 / 4 / 2 terms: 54.7 / 57.1 / 62.6 / 75.4 ms);
      // QHBM_OBS_UNIT_TERMS keeps the knob.  Dealing a group's odd term to BOTH halves by slot rows was measured too
      // (55.5 against 51.4 ms: scripts/experiments/patches/obs_row_split_terms.patch).
      static const size_t cap = std::getenv("QHBM_OBS_UNIT_TERMS") ? size_t(std::max(1, std::atoi(std::getenv("QHBM_OBS_UNIT_TERMS")))) : ~size_t(0) / 2;
      static const bool interleave = !std::getenv("QHBM_OBS_NO_INTERLEAVE");
      struct Unit { uint32_t xo; std::vector<std::pair<size_t, size_t>> masks; size_t terms = 0; };
      std::vector<Unit> units;
      for (size_t k = 0; k < bt.size();) {
        const uint32_t xo = bt[k].x >> bb;
        size_t e = k;
        while (e < bt.size() && (bt[e].x >> bb) == xo) ++e;
        std::vector<std::pair<size_t, size_t>> masks;  // the masks of the group [k, e) and their term ranges
        for (size_t i = k; i < e;) {
          size_t j = i;
          while (j < e && bt[j].x == bt[i].x) ++j;
          masks.emplace_back(i, j);
          i = j;
        }
        std::stable_sort(masks.begin(), masks.end(), [](const std::pair<size_t, size_t>& a, const std::pair<size_t, size_t>& b) {
          return a.second - a.first > b.second - b.first;
        });
        const size_t first_unit = units.size();
        for (const auto& m : masks) {  // first fit, largest first
          const size_t len = m.second - m.first;
          size_t u = first_unit;
          while (u < units.size() && units[u].terms + len > cap && units[u].terms > 0) ++u;
          if (u == units.size()) { units.emplace_back(); units.back().xo = xo; }
          units[u].masks.push_back(m);
          units[u].terms += len;
        }
        k = e;
      }
      if (interleave) {  // inside every window: the heaviest unit while the running load is behind the average, else the lightest
        const int window = 5 + (kObsBlockBits - bb);  // (2 MiB of partner blocks)
        std::vector<Unit> ordered;
        for (size_t a = 0; a < units.size();) {
          size_t b = a;
          while (b < units.size() && (units[b].xo >> window) == (units[a].xo >> window)) ++b;
          std::vector<Unit> win(std::make_move_iterator(units.begin() + long(a)), std::make_move_iterator(units.begin() + long(b)));
          std::stable_sort(win.begin(), win.end(), [](const Unit& x, const Unit& y) { return x.terms > y.terms; });
          double total = 0.0;
          for (const Unit& u : win) total += double(u.terms);
          const double avg = total / double(win.size());
          size_t lo = 0, hi = win.size();
          double done = 0.0;
          for (size_t step = 0; lo < hi; ++step) {
            const bool heavy = done <= avg * double(step);
            Unit& pick = heavy ? win[lo] : win[hi - 1];
            done += double(pick.terms);
            ordered.push_back(std::move(pick));
            if (heavy) ++lo; else --hi;
          }
          a = b;
        }
        units.swap(ordered);
      }
      for (const Unit& u : units) {
        // the unit's masks dealt to the two half-workgroups by term count, largest first (the halves run in step: a unit
        // costs what its larger half costs)
        std::vector<size_t> order(u.masks.size());
        for (size_t i = 0; i < order.size(); ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
          return u.masks[a].second - u.masks[a].first > u.masks[b].second - u.masks[b].first;
        });
        std::vector<size_t> half[2];
        size_t load[2] = {0, 0};
        for (size_t m : order) {
          const int hsel = bb == kObsBlockBits && load[1] < load[0] ? 1 : 0;  // (blocks of 2^12: one workgroup, every mask)
          half[hsel].push_back(m);
          load[hsel] += u.masks[m].second - u.masks[m].first;
        }
        ObsBGroup g{u.xo, uint32_t(terms2.size()), 0u, 0u};
        for (int hsel = 0; hsel < 2; ++hsel) {
          // (mask order = x order: neighbouring masks, neighbouring rows)
          std::sort(half[hsel].begin(), half[hsel].end(), [&](size_t a, size_t b) { return u.masks[a].first < u.masks[b].first; });
          for (size_t m : half[hsel])
            for (size_t i = u.masks[m].first; i < u.masks[m].second; ++i)
              terms2.push_back(obs_block_term(bt[i], i == u.masks[m].first, bb));
          if (hsel == 0) g.mid = uint32_t(terms2.size());
        }
        g.end = uint32_t(terms2.size());
        groups2.push_back(g);
      }
      terms2.push_back(ObsBTerm{0.f, 0u, 0u, 0u, 0u, 0u, 0u, 0u});  // (the kernel reads one record ahead)
      HIPCHK(h->obs_bterms.upload(terms2));
      HIPCHK(h->obs_bgroups.upload(groups2));
      h->n_obs_bgroups = uint32_t(groups2.size());
    }
    HIPCHK(h->op_scale.upload(h->h_op_scale));
    HIPCHK(h->op_inv_scale.upload(h->h_op_inv_scale));
  }
  {
    std::vector<DevTerm> gt;
    for (int ti : h->fwd.plan.global_terms) {
      const PauliTerm& pt = h->model.terms[size_t(ti)];
      gt.push_back(DevTerm{pt.coeff, pt.x, pt.z, uint32_t(pt.ny), uint32_t(pt.op)});
    }
    HIPCHK(h->global_terms.upload(gt));
  }
  // parameter -> slots map for the adjoint reduction
  const Plan& ap = h->adj.plan;
  std::vector<int> begin(size_t(h->model.n_params) + 1, 0), slots(ap.slot_gate.size());
  for (int g : ap.slot_gate) ++begin[size_t(h->model.gates[g].param_idx) + 1];
  for (size_t p = 0; p < size_t(h->model.n_params); ++p) begin[p + 1] += begin[p];
  std::vector<int> cursor(begin.begin(), begin.end() - 1);
  for (size_t s = 0; s < ap.slot_gate.size(); ++s) slots[size_t(cursor[h->model.gates[ap.slot_gate[s]].param_idx]++)] = int(s);
  HIPCHK(h->param_slot_begin.upload(begin));
  HIPCHK(h->param_slots.upload(slots));
  HIPCHK(h->slot_factor.upload(ap.slot_factor));
  {
    std::vector<ShiftPhase> sp;
    for (const Gate& G : h->model.gates)
      if (G.global_shift != 0.f)  // (an identity too: the gate is exp(i pi t global_shift) I**t, include/qhbm_engine.h)
        sp.push_back(ShiftPhase{G.param_idx, G.param_idx >= 0 ? G.scalar : 0.f, G.offset, G.global_shift});
    for (const auto& gp : h->fwd.plan.gate_phases) {  // lowered SWAP / ISWAP powers (schedule.cpp lower())
      const Gate& G = h->model.gates[size_t(gp.first)];
      sp.push_back(ShiftPhase{G.param_idx, G.param_idx >= 0 ? G.scalar : 0.f, G.offset, gp.second});
    }
    if (h->fwd.plan.const_phase != 0.0)  // lowered constant Hadamards (schedule.cpp lower())
      sp.push_back(ShiftPhase{-1, 0.f, 1.f, float(h->fwd.plan.const_phase)});
    HIPCHK(h->shift_phases.upload(sp));
    h->n_shift_phases = int(sp.size());
    // the slope of that phase (kernels.hip global_phase_kernel, term by term): t/2 per X**t and Y**t job -- the X branch
    // times jb.mult; its reduction mod 2 has no slope --, shift * t per entry above
    std::vector<double> slope(size_t(h->model.n_params), 0.0);
    for (const CoefJob& jb : h->fwd.plan.jobs)
      if ((jb.mop == MOP_X || jb.mop == MOP_Y) && jb.param_idx >= 0)
        slope[size_t(jb.param_idx)] += 0.5 * double(jb.scalar) * (jb.mop == MOP_X ? double(jb.mult) : 1.0);
    for (const ShiftPhase& p : sp)
      if (p.param_idx >= 0) slope[size_t(p.param_idx)] += double(p.shift) * double(p.scalar);
    std::vector<float> slope_f(slope.size());
    for (size_t p = 0; p < slope.size(); ++p) slope_f[p] = h->model.frozen(int(p)) ? 0.f : float(M_PI * slope[p]);
    HIPCHK(h->phase_slope.upload(slope_f));
  }
  h->model_uploaded = true;
  return 0;
}

size_t state_bytes(const qhbm_engine* h) { return size_t(8) << h->fwd.plan.n_eff; }

// Workspace budget in bytes (statevector workspace: psi, or psi + lambda).  Default: a third of the
// device's memory (96 GB of the MI355X's 288 GB, so BASELINE config 3's 4096 states x (psi, lambda) x
// 8 MiB = 64 GiB stay resident in one chunk) -- but never more than 45 % of what is FREE when the engine
// first needs it plus what it already holds, so that a second engine, another inference object or
// another rank sharing the GPU sizes itself to what is left instead of to the whole device.  Resolved
// once per engine (never process-wide: a planning-only engine or a failed query must not leave its
// 16 GiB reporting figure behind for a real engine on the same device index).
size_t budget_bytes(qhbm_engine* h) {
  if (h->opt_budget_mb > 0) return size_t(h->opt_budget_mb) << 20;
  if (h->resolved_budget) return h->resolved_budget;
  size_t free_b = 0, total_b = 0;
  if (h->device < 0 || hipSetDevice(h->device) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess || !total_b)
    return size_t(16) << 30;  // planning-only engine / failed query: the figure is only reported, not cached
  const size_t share = size_t(0.45 * double(free_b + own_bytes(h)));
  h->resolved_budget = std::max<size_t>(std::min(total_b / 3, share), size_t(64) << 20);
  return h->resolved_budget;
}

uint32_t chunk_states(qhbm_engine* h, int U) {
  // (a chunk is also a grid dimension of the per-state kernels: at most 65535)
  if (h->opt_chunk > 0) return uint32_t(std::min<int64_t>(std::min<int64_t>(h->opt_chunk, U), 65535));
  const size_t budget = budget_bytes(h);
  const size_t fit = std::max<size_t>(1, budget / state_bytes(h));
  return uint32_t(std::min<size_t>(std::min<size_t>(fit, size_t(U)), 65535));
}

hipEvent_t* timer_begin(qhbm_engine* h, int kind, hipStream_t s) {
  if (!h->opt_profile) return nullptr;
  TimedEvent ev;
  if (!h->free_events.empty()) { ev = h->free_events.back(); h->free_events.pop_back(); }
  else { (void)hipEventCreate(&ev.a); (void)hipEventCreate(&ev.b); }
  ev.kind = kind;
  (void)hipEventRecord(ev.a, s);
  h->events.push_back(ev);
  return &h->events.back().b;
}
void timer_end(hipEvent_t* e, hipStream_t s) { if (e) (void)hipEventRecord(*e, s); }

// Forward passes for one chunk.
// One observable: lambda = O psi gives <psi|O|psi> for free (apply_observable_kernel<A, true> / OBS_LAMBDA_VALUE), so
// the paths that compute lambda anyway (value + VJP, and the retained forward of an autograd caller) skip
// every measurement of the forward sweep.
bool value_mode(const qhbm_engine* h) { return h->opt_values_from_obs != 0 && h->model.n_ops == 1; }

// lambda = O psi and the values through partner blocks staged in LDS (observable.hip) instead of one gather per mask
// (apply_observable_kernel).  The gather kernel pays per mask that leaves its block of 2^11 amplitudes (one L2 gather
// of the state each), the block kernel per GROUP of masks with the same partner block of 2^13 (one staged fetch of the
// state each) plus a little per term: picoseconds per amplitude fitted on config 3 (XXZ, 20 qubits: 9 masks leave,
// 8 groups; 5.8 against 7.5) and config 4 (512 random strings, 24 qubits: 453 leave, 173 groups; 177 against 100):
//   gather  2.3 + 0.385 x (masks leaving its block)        block  0.9 + 0.43 x groups + 0.045 x terms
// ("gather_multi_values" = 1: 2..4 observables go through the gather kernel's per-observable accumulators whatever the
// cost model says -- tests and A/B runs)
bool gather_multi_forced(const qhbm_engine* h) {
  return h->opt_gather_multi > 0 && h->model.n_ops >= 2 && h->model.n_ops <= int(kObsGatherMultiOps) &&
         h->opt_values_from_obs != 0 && h->opt_multi_values != 0;
}
int obs_block_shape(const qhbm_engine* h) {
  return h->opt_obs_block_bits == kObsBlockBits && h->opt_obs_split_rows ? kObsShapeRows : h->opt_obs_block_bits;
}
bool block_kernel(const qhbm_engine* h) {
  if (gather_multi_forced(h)) return false;
  if (h->fwd.plan.n_eff < kObsBlockBits || h->opt_obs_kernel == 0) return false;
  if (h->opt_obs_kernel > 0) return true;
  if (h->block_choice >= 0) return h->block_choice != 0;
  std::vector<uint32_t> xs;
  for (const PauliTerm& t : h->model.terms) xs.push_back(t.x);
  std::sort(xs.begin(), xs.end());
  xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
  const uint32_t gather_block = 256u * obs_amps_per_thread(uint32_t(h->fwd.plan.n_eff));
  double leaving = 0.0;
  std::vector<uint32_t> outs;
  for (uint32_t x : xs) {
    leaving += x >= gather_block ? 1.0 : 0.0;
    outs.push_back(x >> h->opt_obs_block_bits);
  }
  std::sort(outs.begin(), outs.end());
  const double groups = double(std::unique(outs.begin(), outs.end()) - outs.begin());
  const double gather = 2.3 + 0.385 * leaving, block = 0.9 + 0.43 * groups + 0.045 * double(h->model.terms.size());
  h->block_choice = block < gather ? 1 : 0;
  return h->block_choice != 0;
}

// Some term flips two or more qubits, or some group needs a measurement-only pass: measuring in the tiles costs more
// than one sweep of the observable kernel over the final state.
bool wide_observables(const qhbm_engine* h) {
  bool wide = false;
  for (const Pass& p : h->fwd.plan.passes) wide |= p.is_measure_only;
  for (const auto& t : h->model.terms) wide |= __builtin_popcountll(t.x) >= 2;
  return wide;
}

// Several observables (qnn.expectation(states, [op...]), /root/reference/tests/inference/qnn_test.py:187-190): the
// forward sweep runs its lean, paired, measurement-free passes and ONE launch of the block kernel returns every
// <psi|O_t|psi>; a VJP call adds the launch that forms lambda = sum_t upstream_t O_t psi.  Sums of diagonal and
// single-flip terms (TFIM, the Z-string shards of a modular Hamiltonian) keep measuring in the tiles -- the
// Walsh-Hadamard measurement takes hundreds of shards for the price of a few.
constexpr int kMultiValueOps = 64;
bool multi_value_mode(const qhbm_engine* h) {
  // (the values of several observables always come from the block kernel -- the gather kernel has no such mode --,
  // whichever of the two forms lambda)
  if (h->opt_values_from_obs == 0 || h->opt_multi_values == 0 || h->model.n_ops < 2) return false;
  if (gather_multi_forced(h)) return true;
  if (h->fwd.plan.n_eff < kObsBlockBits || h->opt_obs_kernel == 0) return false;
  if (h->model.n_ops > int(kObsMaxValueOps)) return false;
  if (h->opt_multi_values > 0) return true;
  return h->model.n_ops <= kMultiValueOps && h->fwd.plan.passes.size() > 1 && wide_observables(h);
}

// Two to four observables through the gather kernel with a value accumulator per observable
// (apply_observable_kernel<A, OBS_GATHER_MULTI>): ONE launch returns the weighted lambda and every value -- on request only
// ("gather_multi_values" = 1): the per-observable dot products make that launch VALU-bound at 4 x the single-observable
// kernel's time.
bool gather_multi_mode(const qhbm_engine* h) { return gather_multi_forced(h); }

// Forward-only calls: whether the values come from the observable kernel (storing nothing) after lean passes.
bool forward_values_from_observable(const qhbm_engine* h) {
  if (multi_value_mode(h)) return true;
  if (!value_mode(h) || h->opt_fwd_values_obs == 0) return false;
  if (h->opt_fwd_values_obs > 0) return true;
  // measured (scripts/fwd_values_ab.sh): XXZ at 20 qubits - 17 %, 512 random Pauli strings at 24 qubits - 12 %;
  // sums of single-flip and diagonal terms (TFIM) are measured in the tiles at no traffic: + 2 % at 28 and at 16 qubits
  return wide_observables(h) && h->fwd.plan.passes.size() > 1;
}

// The coefficients of one plan for this call: exponents to matrices and phases (gate `gate`'s exponent moved by
// `shift`; -1: none), then the diagonal tables of its records.
int prepare_coefs(qhbm_engine* h, DevicePlan& d, const float* d_params, int gate, double shift, hipStream_t stream) {
  HIPCHK(launch_prep_coefs(d.jobs.p, int(d.plan.jobs.size()), d_params, d.coef.p, gate, shift, stream));
  HIPCHK(launch_combine_diag(d.coef.p, d.rec_offsets.p, int(d.plan.record_offsets.size()), 1u, 0u, stream));
  return 0;
}

// The arguments of forward pass i: the ONE place where its flags are composed.  `skip_measure`: the caller takes the
// values from the observable kernel, or takes none -- measurement groups are ignored (and the callers launch neither
// the measurement-only passes nor the wide-term kernel).  A pass stores its tiles unless it only measures, or completes
// the circuit with nobody left to read the final state: `keep_state` (lambda = O psi, sampling, a retained batch), a
// measurement-only pass or the global-term measurement behind it.  `prog_states` > 0: element e runs program
// e / prog_states on its own copy of the coefficients, `coef_stride` floats apart (PassArgs::prog_states).
PassArgs forward_pass_args(const qhbm_engine* h, size_t i, bool keep_state, bool skip_measure, uint32_t prog_states = 0,
                           uint32_t coef_stride = 0) {
  const Plan& plan = h->fwd.plan;
  const Pass& p = plan.passes[i];
  bool read_after = keep_state || !plan.global_terms.empty();  // (global terms are measured on the final state in HBM)
  for (const Pass& q : plan.passes) read_after |= q.is_measure_only;
  PassArgs a = h->fwd.args[i];
  a.flags = p.flags & (PASS_INIT_BASIS | PASS_GENERAL | PASS_NO_ZERO_FILL | PASS_RELABEL);
  if (h->opt_force_general) a.flags |= PASS_GENERAL;
  if (skip_measure) a.flags |= PASS_SKIP_MEASURE;
  if (!p.is_measure_only && (!p.completes_circuit || read_after)) a.flags |= PASS_STORE;
  a.prog_states = prog_states;
  a.coef_stride = coef_stride;
  return a;
}

// Do [a, a + a_bytes) and [b, b + b_bytes) meet?
bool ranges_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const char *p = static_cast<const char*>(a), *q = static_cast<const char*>(b);
  return p < q + b_bytes && q < p + a_bytes;
}

// Does [p, p + bytes) meet the statevector workspace?
bool aliases_workspace(const qhbm_engine* h, const void* p, size_t bytes) {
  auto meets = [&](const DevBuf<float2>& b) { return b.p && ranges_overlap(p, bytes, b.p, b.n * sizeof(float2)); };
  return meets(h->psi) || meets(h->lam) || meets(h->kry_ring);
}

// A pointer argument that must be there and a multiple of `align` bytes (h NULL: an entry point without an engine).
int check_pointer(qhbm_engine* h, const void* p, size_t align, const char* name) {
  if (!p) return fail(h, std::string(name) + " is NULL");
  if (reinterpret_cast<uintptr_t>(p) % align) return fail(h, std::string(name) + " must be " + std::to_string(align) + "-byte aligned");
  return 0;
}

// From-states calls: states s0 .. s0 + c of the caller's batch, normalised, into the workspace (import_states.hip);
// their squared norms into import_norm2, and the chunk's upstream rows times those into import_up.
int import_chunk(qhbm_engine* h, uint32_t s0, uint32_t c, hipStream_t stream) {
  const uint32_t n = uint32_t(h->model.n), n_eff = uint32_t(h->fwd.plan.n_eff);
  if (aliases_workspace(h, h->import_src, size_t(h->import_U) * (size_t(8) << n)))
    return fail(h, "d_states lies inside the engine's workspace");
  HIPCHK(h->import_parts.reserve(state_norm_parts_count(n, c)));
  hipEvent_t* ev = timer_begin(h, 0, stream);  // (profile_events: the import counts as a launch of the forward sweep)
  HIPCHK(launch_import_states(h->import_src, n, n_eff, c, s0, h->psi.p, h->import_parts.p, h->import_norm2.p, stream));
  timer_end(ev, stream);
  if (h->import_upstream) {
    const size_t w = size_t(h->model.n_ops);
    HIPCHK(launch_scale_by_norm2(h->import_upstream + size_t(s0) * w, h->import_up.p + size_t(s0) * w, c, uint32_t(w),
                                 h->import_norm2.p + s0, stream));
  }
  return 0;
}

// Forward passes for one chunk (`keep_state`, `skip_measure`: forward_pass_args).
int run_forward_chunk(qhbm_engine* h, const int8_t* d_bits, uint32_t s0, uint32_t cs, bool keep_state,
                      hipStream_t stream, bool skip_measure = false) {
  DevicePlan& d = h->fwd;
  if (h->import_src)  // a from-states call: the chunk's start states come from the caller
    if (int rc = import_chunk(h, s0, cs, stream)) return rc;
  for (size_t i = 0; i < d.plan.passes.size(); ++i) {
    const Pass& p = d.plan.passes[i];
    if (skip_measure && p.is_measure_only) continue;
    const PassArgs a = forward_pass_args(h, i, keep_state, skip_measure);
    hipEvent_t* ev = timer_begin(h, 0, stream);
    // dense lean passes without a measurement to take: two states per workgroup, tiles in registers
    const bool pair = h->opt_fwd_pair && cs >= 2 && !(a.flags & (PASS_INIT_BASIS | PASS_GENERAL)) && a.zero_mask == 0 &&
                      (skip_measure || p.n_meas_groups == 0) && pass_fwd_pair_supported(p.K);
    if (pair)
      HIPCHK(launch_pass_fwd_pair(p.K, a, cs, h->psi.p, d_bits, h->model.n, s0, d.prog.p, d.tables.p, d.coef.p, stream));
    else
      HIPCHK(launch_pass_fwd(p.K, d.plan.R, a, cs, h->psi.p, d_bits, h->model.n, d.prog.p, d.tables.p, d.coef.p,
                             h->op_scale.p, h->vals64.p, s0, stream));
    timer_end(ev, stream);
  }
  if (!d.plan.global_terms.empty() && !skip_measure)
    HIPCHK(launch_measure_global(h->psi.p, uint32_t(d.plan.n_eff), cs, h->global_terms.p,
                                 uint32_t(d.plan.global_terms.size()), h->op_scale.p, h->vals64.p,
                                 uint32_t(h->model.n_ops), s0, stream));
  return 0;
}

// Expectation values accumulate in fixed point (program.h kValueFracBits) while the passes run ...
int values_begin(qhbm_engine* h, int U, hipStream_t stream) {
  const size_t nv = size_t(U) * size_t(std::max(h->model.n_ops, 1));
  HIPCHK(h->vals64.reserve(nv));
  HIPCHK(launch_zero_fill(h->vals64.p, nv * sizeof(unsigned long long), stream));
  return 0;
}
// ... and are converted to fp32 [U, n_ops] once at the end.
int values_end(qhbm_engine* h, int U, float* d_out, hipStream_t stream) {
  if (!d_out || h->model.n_ops <= 0) return 0;
  HIPCHK(launch_values_from_fixed(h->vals64.p, h->op_inv_scale.p, d_out, uint32_t(U) * uint32_t(h->model.n_ops),
                                  uint32_t(h->model.n_ops), stream));
  return 0;
}

// The state buffers grow with headroom: the number of unique bitstrings of a sampled batch changes
// from step to step, and every new maximum would otherwise free and re-allocate tens of GiB (seconds).
int ensure_state_buffers(qhbm_engine* h, uint32_t cs, bool with_lam) {
  const size_t have = std::min(h->psi.n, with_lam ? h->lam.n : h->psi.n) >> h->fwd.plan.n_eff;
  size_t want = cs;
  if (want > have) {
    const size_t cap = std::max<size_t>(cs, budget_bytes(h) / ((with_lam ? 2 : 1) * state_bytes(h)));
    want = std::min(cap, want + std::max<size_t>(want / 8, 1));
  }
  const size_t amps = want << h->fwd.plan.n_eff;
  if (with_lam && !h->lam.p) {
    // a forward-only call may have grown psi to the whole budget: with lambda beside it the pair must
    // fit the budget again, so psi goes back to its half before lambda is allocated
    const size_t half = std::max<size_t>(amps, (budget_bytes(h) / (2 * state_bytes(h))) << h->fwd.plan.n_eff);
    if (h->psi.n > half) h->psi.release();
  }
  HIPCHK(h->psi.reserve(amps, false));
  if (with_lam) HIPCHK(h->lam.reserve(amps, false));
  return 0;
}

int run_observable_chunk(qhbm_engine* h, uint32_t s0, uint32_t c, const float* d_upstream, bool value_mode,
                         hipStream_t stream, bool store_lambda = true, bool multi_values = false,
                         const float2* src = nullptr, float2* dst = nullptr);
int run_values_chunk(qhbm_engine* h, uint32_t row0, uint32_t c, hipStream_t stream);

// One state per XCD at a time (1) or every XCD an eighth of each state (0)?  Measured on the block kernel, config 4
// (24 qubits): 61.1 against 53.6 ms per 32 states -- a 128-MiB state that all eight XCDs read sits in the Infinity
// Cache once; the gather kernel at config 3 (20 qubits): one state per XCD wins (3.7 against 5.1 fabric reads of the
// state).  By size: states of 64 MiB and more are shared by the XCDs.
bool observable_xcd_states(const qhbm_engine* h) {
  if (h->opt_obs_xcd_states >= 0) return h->opt_obs_xcd_states != 0;
  return h->fwd.plan.n_eff < 23;
}

// lambda = O psi for the chunk in the workspace.  value_mode (a single observable): unweighted, and
// <psi|O|psi> goes to the fixed-point value accumulators -- the forward sweep measured nothing.
// multi_values (gather_multi_mode): the gather kernel with a value accumulator per observable -- the weighted lambda (if
// stored) and every <psi|O_t|psi> from ONE launch.
// src / dst (default: psi / lam): the c states read and the c states written, at the workspace's pitch -- the Chebyshev
// recurrence of evolve_states rotates its buffers through them.
int run_observable_chunk(qhbm_engine* h, uint32_t s0, uint32_t c, const float* d_upstream, bool value_mode,
                         hipStream_t stream, bool store_lambda, bool multi_values, const float2* src, float2* dst) {
  const uint32_t n_eff = uint32_t(h->fwd.plan.n_eff);
  if (!src) src = h->psi.p;
  if (!dst) dst = h->lam.p;
  if (multi_values) {
    HIPCHK(h->value_part.reserve(observable_value_parts(n_eff, c) * size_t(h->model.n_ops)));
    hipEvent_t* ev = timer_begin(h, 2, stream);
    HIPCHK(launch_apply_observable(src, store_lambda ? dst : nullptr, n_eff, c, h->terms.p,
                                   h->n_gather_terms, h->obs_groups.p, h->n_obs_groups,
                                   store_lambda ? d_upstream : nullptr, uint32_t(h->model.n_ops), s0, h->op_scale.p,
                                   h->vals64.p, h->value_part.p, observable_xcd_states(h), stream, true));
    timer_end(ev, stream);
    return 0;
  }
  if (value_mode)
    HIPCHK(h->value_part.reserve(block_kernel(h) ? observable_blocks_value_parts(n_eff, c, 1u, h->opt_obs_block_bits) : observable_value_parts(n_eff, c)));
  hipEvent_t* ev = timer_begin(h, 2, stream);
  if (block_kernel(h)) {
    const int mode = !value_mode ? OBS_LAMBDA : (store_lambda ? OBS_LAMBDA_VALUE : OBS_VALUES);
    HIPCHK(launch_observable_blocks(mode, obs_block_shape(h), src, store_lambda ? dst : nullptr, n_eff, c, h->obs_bterms.p,
                                    h->obs_bgroups.p, h->n_obs_bgroups, d_upstream, uint32_t(h->model.n_ops), s0,
                                    h->op_scale.p, value_mode ? h->vals64.p : nullptr, h->value_part.p,
                                    observable_xcd_states(h), stream));
  } else {
    ObsFarLaunch far[3];
    for (int f = 0; f < h->n_far; ++f)
      far[f] = ObsFarLaunch{h->far[f].terms.p, h->far[f].n_terms, h->far[f].groups.p, h->far[f].n_groups, h->far[f].far_hi};
    HIPCHK(launch_apply_observable(src, store_lambda ? dst : nullptr, n_eff, c, h->terms.p,
                                   h->n_gather_terms, h->obs_groups.p, h->n_obs_groups, d_upstream,
                                   uint32_t(h->model.n_ops), s0, h->op_scale.p, value_mode ? h->vals64.p : nullptr,
                                   h->value_part.p, observable_xcd_states(h), stream, false, far, h->n_far));
  }
  timer_end(ev, stream);
  return 0;
}

// <psi|O_t|psi> of every observable for `c` final states in psi (rows row0 .. row0 + c of the fixed-point accumulators),
// nothing stored: one observable through either kernel, several through the block kernel (multi_value_mode).
int run_values_chunk(qhbm_engine* h, uint32_t row0, uint32_t c, hipStream_t stream) {
  if (h->model.n_ops == 1) return run_observable_chunk(h, row0, c, nullptr, true, stream, false);
  if (gather_multi_mode(h)) return run_observable_chunk(h, row0, c, nullptr, false, stream, false, true);
  const uint32_t n_eff = uint32_t(h->fwd.plan.n_eff);
  HIPCHK(h->value_part.reserve(observable_blocks_value_parts(n_eff, c, uint32_t(h->model.n_ops), h->opt_obs_block_bits)));
  hipEvent_t* ev = timer_begin(h, 2, stream);
  HIPCHK(launch_observable_blocks(OBS_VALUES_MULTI, obs_block_shape(h), h->psi.p, nullptr, n_eff, c, h->obs_bterms.p, h->obs_bgroups.p,
                                  h->n_obs_bgroups, nullptr, uint32_t(h->model.n_ops), row0, h->op_scale.p, h->vals64.p,
                                  h->value_part.p, observable_xcd_states(h), stream));
  timer_end(ev, stream);
  return 0;
}

// The backward passes of a chunk whose (psi, lambda) pair is in the workspace.  `e0`: the chunk's pairs start at that
// element of the workspace (qhbm_program_vjps runs a sub-range of a launch set's elements; 0 everywhere else).
int run_adjoint_chunk(qhbm_engine* h, const int8_t* d_bits, uint32_t s0, uint32_t c, hipStream_t stream, uint32_t e0 = 0) {
  DevicePlan& b = h->adj;
  const uint32_t n_slots = uint32_t(b.plan.slot_gate.size());
  size_t rows = 0;  // tile_grad: one row of the pass's slots per workgroup
  for (const PassArgs& ba : b.args)
    rows = std::max(rows, ((size_t(c) << ba.n_free) + reduce_tiles_scratch_rows(c, size_t(1) << ba.n_free)) *
                              std::max<uint32_t>(ba.n_slots, 1));
  HIPCHK(h->tile_grad.reserve(rows));
  for (size_t i = 0; i < b.plan.passes.size(); ++i) {
    hipEvent_t* ev = timer_begin(h, 1, stream);
    PassArgs ba = b.args[i];
    if (h->opt_force_general) ba.flags |= PASS_GENERAL;
    const size_t off = size_t(e0) << h->fwd.plan.n_eff;
    HIPCHK(launch_pass_adj(b.plan.K, h->opt_adj_exchange != 0, ba, c, h->psi.p + off, h->lam.p + off, d_bits, h->model.n,
                           b.prog.p, b.tables.p, b.coef.p, h->tile_grad.p, s0, stream));
    timer_end(ev, stream);
    // tiles of a state are added in tile order (bit-reproducible, no atomics)
    HIPCHK(launch_reduce_tiles(h->tile_grad.p, c, 1u << ba.n_free, ba.n_slots, h->state_grad.p, n_slots, ba.slot_base,
                               s0, stream));
  }
  return 0;
}

uint32_t adjoint_chunk_states(qhbm_engine* h, int U) {
  uint32_t cs = chunk_states(h, U);
  if (h->opt_chunk <= 0)  // two buffers per state
    cs = uint32_t(std::min<size_t>(std::min<size_t>(size_t(U), 65535),
                                   std::max<size_t>(1, budget_bytes(h) / (2 * state_bytes(h)))));
  return cs;
}

// ---- the per-state gradient rows (state_grad: [rows, slots of the backward plan]) have ONE owner ----
uint32_t grad_slots(const qhbm_engine* h) { return std::max<uint32_t>(uint32_t(h->adj.plan.slot_gate.size()), 1); }

hipError_t reserve_state_grad(qhbm_engine* h, size_t rows) { return h->state_grad.reserve(rows * grad_slots(h)); }

// Rows [0, rows) exist and are zero: the tile reductions of the backward passes add into them.
hipError_t begin_state_grad(qhbm_engine* h, size_t rows, hipStream_t s) {
  const hipError_t e = reserve_state_grad(h, rows);
  return e != hipSuccess ? e : launch_zero_fill(h->state_grad.p, rows * grad_slots(h) * sizeof(float), s);
}

// Value mode (one observable, values from lambda = O psi): the backward sweep ran on the UNWEIGHTED lambda that gave
// <psi|O|psi>; the upstream weight of every state goes onto its finished row instead.
hipError_t weight_state_grad(qhbm_engine* h, uint32_t rows, const float* d_upstream, hipStream_t s) {
  return launch_scale_rows(h->state_grad.p, rows, grad_slots(h), d_upstream, s);
}

// The rows of U states into d_grad [n_params], and whose rows they are: qhbm_state_gradients serves them (`servable`)
// through the plan set that filled them (`dense`: a from-states VJP's, slots of the dense-start backward plan).
int reduce_state_grad(qhbm_engine* h, int U, float* d_grad, bool dense, bool servable, hipStream_t s) {
  HIPCHK(launch_reduce_grad(h->state_grad.p, uint32_t(U), uint32_t(h->adj.plan.slot_gate.size()), h->param_slot_begin.p,
                            h->param_slots.p, h->slot_factor.p, d_grad, h->model.n_params, 0, s));
  h->state_grad_U = servable ? U : 0;
  h->state_grad_dense = dense;
  return 0;
}

// The gradient of an empty batch.
int empty_batch_grad(qhbm_engine* h, float* d_grad, hipStream_t s) {
  if (h->model.n_params) HIPCHK(launch_zero_fill(d_grad, size_t(h->model.n_params) * sizeof(float), s));
  return 0;
}

// ---- ONE driver for every sweep of the circuit over a batch of states ----
// How a batch is cut into chunks of the workspace.
enum class Chunks {
  kStates,    // chunk_states: psi alone
  kPairs,     // adjoint_chunk_states: lambda beside psi
  kBatch,     // the whole batch in one chunk (a retaining forward: the caller has asked batch_fits_backward_chunk)
  kShots,     // chunk_states, at most 65535: the sampler puts the chunk on a grid dimension
  kResident,  // the whole batch, and its final states ARE in psi (a retained VJP): no forward work at all
};

struct Sweep {
  const int8_t* d_bits; int U; const float* d_params;
  Chunks chunks = Chunks::kStates;
  int shift_gate = -1; double shift = 0.0;  // the forward coefficients are those of one shifted program (prepare_coefs)
  bool with_lam = false;  // lambda sits beside psi in the workspace
  bool backward = false;  // the caller runs backward passes: the backward plan's coefficients are prepared too
  bool keep_state = false, skip_measure = false;  // forward_pass_args
  bool values = false;    // the fixed-point accumulators are zeroed before the sweep and converted into d_out (if any) after it
  float* d_out = nullptr;
  bool passes = true;     // false: a chunk's states are imported and no pass runs (a from-states call on a circuit without gates)
};
bool batch_fits_backward_chunk(qhbm_engine* h, int U) { return adjoint_chunk_states(h, U) >= uint32_t(U); }
uint32_t sweep_chunk_states(qhbm_engine* h, const Sweep& sw) {
  switch (sw.chunks) {
    case Chunks::kStates: return chunk_states(h, sw.U);
    case Chunks::kPairs: return adjoint_chunk_states(h, sw.U);
    case Chunks::kShots: return std::min<uint32_t>(chunk_states(h, sw.U), 65535u);
    default: return uint32_t(sw.U);
  }
}

// body(s0, c) for the chunks [s0, s0 + c) of U states, at most cs at a time.
template <typename Body>
int for_each_chunk(int U, uint32_t cs, Body&& body) {
  for (uint32_t s0 = 0; s0 < uint32_t(U); s0 += cs)
    if (int rc = body(s0, std::min<uint32_t>(cs, uint32_t(U) - s0))) return rc;
  return 0;
}

// The sweep: coefficients, value accumulators, the workspace, then chunk by chunk the forward passes and `body(s0, c)`,
// the caller's own work on a chunk whose final states are in psi.  `reserve(cs)` runs once between the growth of the
// workspace and the first chunk: scratch sized by the chunk grows there, never inside the loop (a captured step must not
// allocate), and a caller's pointer is checked against the workspace where it now lies.  Retained states end here.
template <typename Reserve, typename Body>
int run_sweep(qhbm_engine* h, const Sweep& sw, hipStream_t s, Reserve&& reserve, Body&& body) {
  const bool resident = sw.chunks == Chunks::kResident;
  h->retained_U = 0;
  if (!resident)
    if (int rc = prepare_coefs(h, h->fwd, sw.d_params, sw.shift_gate, sw.shift, s)) return rc;
  if (sw.backward)
    if (int rc = prepare_coefs(h, h->adj, sw.d_params, -1, 0.0, s)) return rc;
  if (sw.values)
    if (int rc = values_begin(h, sw.U, s)) return rc;
  const uint32_t cs = sweep_chunk_states(h, sw);
  if (!resident)
    if (int rc = ensure_state_buffers(h, cs, sw.with_lam)) return rc;
  if (int rc = reserve(cs)) return rc;
  if (int rc = for_each_chunk(sw.U, cs, [&](uint32_t s0, uint32_t c) -> int {
        if (!resident)
          if (int rc = sw.passes ? run_forward_chunk(h, sw.d_bits, s0, c, sw.keep_state, s, sw.skip_measure)
                                 : import_chunk(h, s0, c, s))
            return rc;
        return body(s0, c);
      }))
    return rc;
  return sw.values ? values_end(h, sw.U, sw.d_out, s) : 0;
}
int no_reserve(uint32_t) { return 0; }  // (a caller of run_sweep with no scratch of its own)

// Expectation values.  `retain`: the batch stays in psi, lambda allocated beside it so that psi is not moved later, for
// qhbm_expectation_vjp_retained -- if it fits one backward chunk; otherwise nothing is kept.
int forward(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, float* d_out,
            int shift_gate, double shift, hipStream_t stream, bool retain = false) {
  retain = retain && batch_fits_backward_chunk(h, U);
  // One observable and a state that passes through HBM anyway: the lean (paired, measurement-free) passes and one
  // sweep of the lambda = O psi kernel for <psi|O|psi> -- nothing stored -- beat the measuring passes (config 3:
  // 148 -> 124 ms per 4096 states).  A single-pass plan measures in its tile and never writes the state.
  // A retaining call takes the values as the adjoint VJP does, and in value mode keeps the unweighted lambda (retained_mu).
  const bool vm = value_mode(h), lean = retain ? vm || multi_value_mode(h) : forward_values_from_observable(h);
  Sweep sw{d_bits, U, d_params, retain ? Chunks::kBatch : Chunks::kStates, shift_gate, shift};
  sw.with_lam = retain; sw.keep_state = retain || lean; sw.skip_measure = lean;
  sw.values = true; sw.d_out = d_out;
  if (int rc = run_sweep(h, sw, stream, no_reserve, [&](uint32_t s0, uint32_t c) -> int {
        if (!lean) return 0;
        return retain && vm ? run_observable_chunk(h, s0, c, nullptr, true, stream) : run_values_chunk(h, s0, c, stream);
      }))
    return rc;
  if (retain) { h->retained_U = U; h->retained_mu = vm; h->retained_table = false; }
  return 0;
}

// A VJP computes the values whether its caller wants them or not: without d_out_vals they go to scratch.
int values_or_scratch(qhbm_engine* h, int U, float** d_out_vals) {
  if (!*d_out_vals) HIPCHK(h->vals_tmp.reserve(size_t(U) * size_t(h->model.n_ops)));
  if (!*d_out_vals) *d_out_vals = h->vals_tmp.p;
  return 0;
}

// values + per-state gradient slots (adjoint) for a given upstream; the rows await reduce_state_grad or a scatter.
int adjoint_sweep(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                  const float* d_upstream, float* d_out_vals, hipStream_t stream) {
  consume_workspace(h);
  HIPCHK(begin_state_grad(h, size_t(U), stream));
  const bool vm = value_mode(h), mv = multi_value_mode(h);
  Sweep sw{d_bits, U, d_params, Chunks::kPairs};
  sw.with_lam = sw.backward = sw.keep_state = true; sw.skip_measure = vm || mv;
  sw.values = true; sw.d_out = d_out_vals;
  if (int rc = run_sweep(h, sw, stream, no_reserve, [&](uint32_t s0, uint32_t c) -> int {
        const bool gm = mv && gather_multi_mode(h);  // 2..4 observables on the gather kernel: values AND lambda from one launch
        if (mv && !gm)  // several observables: their values from one launch over the final states, lambda (weighted) from the next
          if (int rc = run_values_chunk(h, s0, c, stream)) return rc;
        if (int rc = run_observable_chunk(h, s0, c, d_upstream, vm, stream, true, gm)) return rc;
        return run_adjoint_chunk(h, d_bits, s0, c, stream);
      }))
    return rc;
  if (vm) HIPCHK(weight_state_grad(h, uint32_t(U), d_upstream, stream));
  return 0;
}

// The final states leave the workspace without the global phase the kernels leave out: cirq's e^{i pi t / 2} per X**t / Y**t
// and every gate's exp(i pi t global_shift).  global_phase puts (cos, sin) of it into phase_cs; apply_global_phase
// multiplies U exported states [U, 2^n] by it.
hipError_t global_phase(qhbm_engine* h, const float* d_params, hipStream_t s) {
  const hipError_t e = h->phase_cs.reserve(2);
  return e != hipSuccess ? e : launch_global_phase(h->fwd.jobs.p, int(h->fwd.plan.jobs.size()), h->shift_phases.p,
                                                   h->n_shift_phases, d_params, h->phase_cs.p, s);
}
hipError_t apply_global_phase(qhbm_engine* h, void* d_out_states, int U, hipStream_t s) {
  return launch_scale_states(static_cast<float2*>(d_out_states), size_t(U) << h->model.n, h->phase_cs.p, s);
}

// The plans that are in, and what the chooser of the adjoint tile and pass order compares (adjoint_plan_seconds).
std::string describe_plans(const qhbm_engine* h) {
  char line[96];
  std::snprintf(line, sizeof(line), "adjoint time model: %.2f us per state\n", 1e6 * adjoint_plan_seconds(h->adj.plan, h->model));
  return describe_plan(h->fwd.plan) + describe_plan(h->adj.plan) + line;
}

// The preamble of a compute call: what it requires of the engine and of its arguments, checked in this order.
enum CallNeeds : unsigned {
  kNeedCircuit = 1,      // qhbm_set_circuit has been called (the calls that upload the model learn it there)
  kNeedObservables = 2,
  kNeedTable = 4,        // `ptr` is the energy table
  kNeedStates = 8,       // `ptr` is U caller states: 16-byte aligned, outside the workspace
  kNoUpload = 16,        // the caller exchanges the plan sets first and uploads the model itself
};
int begin_call(qhbm_engine* h, int U, unsigned needs, const void* ptr = nullptr) {
  if (!h) return 1;
  if (int rc = need_device(h)) return rc;
  if (U < 0) return fail(h, "negative batch size");
  if ((needs & kNeedCircuit) && !h->have_circuit) return fail(h, "qhbm_set_circuit has not been called");
  if ((needs & kNeedObservables) && h->model.n_ops <= 0) return fail(h, "qhbm_set_observables has not been called");
  if ((needs & kNeedTable) && !ptr) return fail(h, "energy table is NULL");
  if ((needs & kNeedStates) && U > 0) {
    if (int rc = check_pointer(h, ptr, 16, "d_states")) return rc;
    if (aliases_workspace(h, ptr, size_t(U) * (size_t(8) << h->model.n)))
      return fail(h, "d_states lies inside the engine's workspace");
  }
  return (needs & kNoUpload) ? 0 : upload_model(h);
}

// ---- batches of (state, shifted program) pairs: qhbm_expectation_vjp(parameter shift), qhbm_program_vjps and
// qhbm_sample_counts.  The pairs are the ELEMENTS of a launch set: Uc states x Pc programs, element e = program
// e / c on state e % c, every program on its own copy of the coefficient buffer.  Programs run in the order of
// schedule.h order_programs(); the programs of group k start at pass k from the base program's state after passes < k.

// The shift tables of a batch in execution order.  ONE set serves every caller: the parameter-shift VJP keeps its own
// across calls (shift_ready: no synchronisation and no copy on a repeated call, so a captured step stays capturable), the
// other callers overwrite them.
int upload_shift_tables(qhbm_engine* h, const ProgramOrder& order, const int* gates, const float* shifts, hipStream_t s) {
  std::vector<int> sg(order.dst.size());
  std::vector<float> sv(order.dst.size());
  for (size_t q = 0; q < sg.size(); ++q) {
    sg[q] = std::max(gates[order.dst[q]], -1);  // any negative value = the unshifted circuit
    sv[q] = shifts[order.dst[q]];
  }
  h->shift_ready = false;
  HIPCHK(hipStreamSynchronize(s));  // synchronous copies into buffers an earlier call on this stream may still read
  HIPCHK(h->shift_gates.upload(sg));
  HIPCHK(h->shift_vals.upload(sv));
  HIPCHK(h->shift_dst.upload(order.dst));
  return 0;
}

// Launch-set geometry.  `buffers`: state-sized buffers per element -- 1 (psi), or 2 (psi and lambda: the backward passes
// run on the elements too, and their grids count).  `grid_cap`: some kernel of the caller puts the elements on a grid
// dimension of at most 65535.  Sharing takes room for Uc base states on top.  `caps_bound_base`: those count against
// the element caps as well as against the memory budget -- the parameter-shift VJP has always cut its sets that way
// ("chunk_states" = 5: 2 states x 1 program + 2 base states) and qhbm_program_vjps against the budget alone; each keeps
// its cut, so each issues the launches it always did.
struct LaunchSets {
  uint32_t stride;  // floats between the coefficient copies of two programs
  uint32_t Uc, Pc;
  bool share;
};
LaunchSets launch_set_geometry(qhbm_engine* h, int U, uint32_t n_prog, const ProgramOrder& order, int buffers, bool grid_cap,
                               bool caps_bound_base) {
  LaunchSets g;
  g.stride = uint32_t((h->fwd.plan.coef_init.size() + 64 + 63) / 64 * 64);
  const size_t states_cap = std::max<size_t>(1, budget_bytes(h) / state_bytes(h)), B = size_t(buffers);
  uint32_t max_nl = 0;
  for (const PassArgs& a : h->fwd.args) max_nl = std::max(max_nl, a.n_nonlocal);
  if (buffers == 2)
    for (const PassArgs& a : h->adj.args) max_nl = std::max(max_nl, a.n_nonlocal);
  size_t el_cap = std::max<size_t>(1, states_cap / B);
  el_cap = std::min<size_t>(el_cap, (size_t(1) << 30) >> max_nl);                             // grid.x = elements << n_nonlocal
  el_cap = std::min<size_t>(el_cap, (size_t(2) << 30) / (size_t(g.stride) * sizeof(float)));  // <= 2 GiB of coefficient copies
  if (grid_cap) el_cap = std::min<size_t>(el_cap, 65535);
  if (h->opt_chunk > 0) el_cap = std::min<size_t>(el_cap, size_t(h->opt_chunk));
  el_cap = std::max<size_t>(el_cap, 1);
  const size_t pool = caps_bound_base ? std::min(states_cap, el_cap) : states_cap;
  g.share = order.shares && pool >= B + 1;  // a buffer of base states beside one element, and a pass to skip
  g.Uc = uint32_t(std::min<size_t>(size_t(U), g.share ? std::max<size_t>(1, std::min(el_cap, pool / (B + 1))) : el_cap));
  g.Pc = uint32_t(std::max<size_t>(1, std::min<size_t>(n_prog, std::min(el_cap, (pool - (g.share ? g.Uc : 0)) / B) / g.Uc)));
  return g;
}

// coef_batch holds the forward plan's static words for Pc programs.
int grow_coef_batch(qhbm_engine* h, const LaunchSets& g, hipStream_t s) {
  if (h->coef_batch_programs >= g.Pc) return 0;
  HIPCHK(h->coef_batch.reserve(size_t(g.Pc) * g.stride));
  HIPCHK(launch_replicate(h->fwd.coef.p, h->coef_batch.p, uint32_t(h->fwd.plan.coef_init.size()), g.stride, g.Pc, s));
  h->coef_batch_programs = g.Pc;
  return 0;
}

// What the passes of a launch set do with states and values (`keep_state`, `skip_measure`: forward_pass_args).
// `takes_values` false is qhbm_sample_counts: it reads no value, so its sets never zeroed the accumulators, and its passes
// never entered the profile (qhbm_kernel_time_ms counts what it always counted).
struct LaunchSetPolicy {
  bool keep_state, skip_measure, takes_values;
};

// The forward launches of one launch set: programs [q0, q0 + nq) of group k on states [s0, s0 + c) -- their
// coefficients, the passes from k on (the first one loads the base program's states from `base` when k > 0), the
// global-term measurement.  The final states are elements 0 .. nq * c of psi, the values rows 0 .. nq * c of vals64.
int run_launch_set(qhbm_engine* h, const int8_t* d_bits, const float* d_params, const LaunchSets& g, uint32_t q0, uint32_t nq,
                   size_t k, uint32_t s0, uint32_t c, const float2* base, LaunchSetPolicy pol, hipStream_t s) {
  DevicePlan& d = h->fwd;
  const uint32_t ne = nq * c, T = uint32_t(h->model.n_ops);
  HIPCHK(launch_prep_coefs_batch(d.jobs.p, int(d.plan.jobs.size()), d_params, h->coef_batch.p, h->shift_gates.p + q0,
                                 h->shift_vals.p + q0, nq, g.stride, s));
  HIPCHK(launch_combine_diag(h->coef_batch.p, d.rec_offsets.p, int(d.plan.record_offsets.size()), nq, g.stride, s));
  if (pol.takes_values) HIPCHK(launch_zero_fill(h->vals64.p, size_t(ne) * T * sizeof(unsigned long long), s));
  const float2* src = k > 0 ? base : nullptr;
  for (size_t i = k; i < d.plan.passes.size(); ++i) {
    const Pass& p = d.plan.passes[i];
    if (pol.skip_measure && p.is_measure_only) continue;
    const PassArgs a = forward_pass_args(h, i, pol.keep_state, pol.skip_measure, c, g.stride);
    hipEvent_t* ev = pol.takes_values ? timer_begin(h, 0, s) : nullptr;
    HIPCHK(launch_pass_fwd(p.K, d.plan.R, a, ne, h->psi.p, d_bits, h->model.n, d.prog.p, d.tables.p, h->coef_batch.p,
                           h->op_scale.p, h->vals64.p, s0, s, src));
    timer_end(ev, s);
    src = nullptr;
  }
  if (!pol.skip_measure && !d.plan.global_terms.empty())
    HIPCHK(launch_measure_global(h->psi.p, uint32_t(d.plan.n_eff), ne, h->global_terms.p,
                                 uint32_t(d.plan.global_terms.size()), h->op_scale.p, h->vals64.p, T, 0u, s));
  return 0;
}

// The base program's states [s0, s0 + c) in `base` advance by pass k, on the base program's coefficients (its values
// are not taken here).
int advance_base(qhbm_engine* h, const int8_t* d_bits, size_t k, uint32_t s0, uint32_t c, float2* base, hipStream_t s) {
  DevicePlan& d = h->fwd;
  const PassArgs a = forward_pass_args(h, k, true, true);
  hipEvent_t* ev = timer_begin(h, 0, s);
  HIPCHK(launch_pass_fwd(d.plan.passes[k].K, d.plan.R, a, c, base, d_bits, h->model.n, d.prog.p, d.tables.p, d.coef.p,
                         h->op_scale.p, h->vals64.p, s0, s));
  timer_end(ev, s);
  return 0;
}

// Programs [qa, qb) (execution order) on states [s0, s0 + c): group by group, at most Pc programs per launch set;
// `after(q0, nq)` is the caller's own work on the set's final states.  Without sharing the range is one group that
// starts at pass 0.  The base program advances by pass k while a later program of the range needs it.
template <typename After>
int run_program_groups(qhbm_engine* h, const int8_t* d_bits, const float* d_params, const LaunchSets& g,
                       const ProgramOrder& order, uint32_t qa, uint32_t qb, uint32_t s0, uint32_t c, float2* base,
                       LaunchSetPolicy pol, hipStream_t s, After&& after) {
  const std::vector<Pass>& passes = h->fwd.plan.passes;
  for (size_t k = 0; k < (g.share ? passes.size() : size_t(1)); ++k) {
    const uint32_t lo = std::max(g.share && k ? order.group_end[k - 1] : 0u, qa);
    const uint32_t hi = std::min(g.share ? order.group_end[k] : qb, qb);
    for (uint32_t q0 = lo; q0 < hi; q0 += g.Pc) {
      const uint32_t nq = std::min<uint32_t>(g.Pc, hi - q0);
      if (int rc = run_launch_set(h, d_bits, d_params, g, q0, nq, k, s0, c, base, pol, s)) return rc;
      if (int rc = after(q0, nq)) return rc;
    }
    if (g.share && order.group_end[k] < qb && !passes[k].is_measure_only)
      if (int rc = advance_base(h, d_bits, k, s0, c, base, s)) return rc;
  }
  return 0;
}

// ---- energy tables: E = sum_y table[y] |y><y| (a general BitstringEnergy's modular Hamiltonian) ----
// No observables are needed: the forward runs the lean, measurement-free passes and keeps the state; the table kernel
// (energy_table.hip) takes the values, lambda = upstream E psi and the table gradient from it.
// Scratch of the table kernel for chunks of up to cs states (grown before the chunk loop, never inside it); `with_grad`:
// and the running table gradient, zeroed.
int reserve_table_scratch(qhbm_engine* h, uint32_t cs, bool with_grad, hipStream_t s) {
  const uint32_t n_eff = uint32_t(h->fwd.plan.n_eff), n = uint32_t(h->model.n);
  HIPCHK(h->tab_vpart.reserve(size_t(cs) << (n_eff - 10)));
  if (with_grad) {
    HIPCHK(h->tab_gpart.reserve(size_t((cs >> table_group_bits(n_eff)) + 2) << n));
    HIPCHK(h->tab_carry.reserve(size_t(1) << n));
    HIPCHK(h->tab_gsum.reserve(size_t(1) << n));
    HIPCHK(launch_zero_fill(h->tab_gsum.p, (size_t(1) << n) * sizeof(double), s));
  }
  return 0;
}

int run_table_chunk(qhbm_engine* h, int mode, const float* d_table, uint32_t s0, uint32_t c, int U,
                    const float* d_upstream, float* d_out, hipStream_t s) {
  hipEvent_t* ev = timer_begin(h, 2, s);
  HIPCHK(launch_energy_table(mode, h->psi.p, h->lam.p, d_table, uint32_t(h->model.n), uint32_t(h->fwd.plan.n_eff), c, s0,
                             uint32_t(U), d_upstream, h->tab_vpart.p, d_out, h->tab_gpart.p, h->tab_carry.p, h->tab_gsum.p, s));
  timer_end(ev, s);
  return 0;
}

// qhbm_table_expectation[_retain]: values of the table; `retain`: the batch stays in psi (one chunk, lambda allocated
// beside it) for the retained VJP -- if it fits one backward chunk.
int table_forward(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, const float* d_table, float* d_out,
                  bool retain, void* stream) {
  if (int rc = begin_call(h, U, kNeedTable, d_table)) return rc;
  if (U == 0) return 0;
  if (!d_out) return fail(h, "d_out is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  retain = retain && batch_fits_backward_chunk(h, U);
  Sweep sw{d_bits, U, d_params, retain ? Chunks::kBatch : Chunks::kStates};
  sw.with_lam = retain; sw.keep_state = sw.skip_measure = true;
  if (int rc = run_sweep(
          h, sw, s, [&](uint32_t cs) { return reserve_table_scratch(h, cs, false, s); },
          [&](uint32_t s0, uint32_t c) { return run_table_chunk(h, TABLE_VALUES, d_table, s0, c, U, nullptr, d_out, s); }))
    return rc;
  if (retain) { h->retained_U = U; h->retained_table = true; }
  return 0;
}

// lambda = upstream E psi, the backward sweep, d_grad; values if d_out_vals, the table gradient if d_table_grad.
// `retained`: the final states of a table_forward(retain) are in psi -- no forward passes.
int table_vjp(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, const float* d_table,
              const float* d_upstream, float* d_out_vals, float* d_grad, float* d_table_grad, bool retained, hipStream_t s) {
  const size_t dim = size_t(1) << h->model.n;
  consume_workspace(h);  // (the backward sweep un-applies psi in place: retained states are consumed)
  HIPCHK(begin_state_grad(h, size_t(U), s));
  const int mode = d_table_grad ? TABLE_LAMBDA_GRAD : TABLE_LAMBDA;
  Sweep sw{d_bits, U, d_params, retained ? Chunks::kResident : Chunks::kPairs};
  sw.with_lam = sw.backward = sw.keep_state = sw.skip_measure = true;
  if (int rc = run_sweep(
          h, sw, s, [&](uint32_t cs) { return reserve_table_scratch(h, cs, d_table_grad != nullptr, s); },
          [&](uint32_t s0, uint32_t c) -> int {
            if (int rc = run_table_chunk(h, mode, d_table, s0, c, U, d_upstream, d_out_vals, s)) return rc;
            return run_adjoint_chunk(h, d_bits, s0, c, s);
          }))
    return rc;
  if (int rc = reduce_state_grad(h, U, d_grad, false, true, s)) return rc;
  if (d_table_grad) HIPCHK(launch_doubles_to_floats(h->tab_gsum.p, d_table_grad, dim, s));
  return 0;
}

// ---- shifted programs named by the caller: (shift_gates[q], shifts[q]), a negative gate = the unshifted circuit ----
const char* const kNoTwoTermRule = "the two-term parameter-shift rule does not apply to ISWAPPOW; use the adjoint method";

// `two_term_rule`: the values of the programs are combined by the two-term shift rule, which ISWAPPOW does not obey
// (qhbm_program_vjps; the parameter-shift VJP builds its own programs and says the same of them); the sampling calls run
// any shifted program.  The sampling calls report an entry out of range before any constant exponent (a pass over the
// ranges first), qhbm_program_vjps the first entry at fault -- as each always did.
int check_shifted_programs(qhbm_engine* h, int n_programs, const int32_t* shift_gates, const float* shifts, bool two_term_rule) {
  const int n_gates = int(h->model.gates.size());
  for (int pass = two_term_rule ? 1 : 0; pass < 2; ++pass)
    for (int q = 0; q < n_programs; ++q) {
      const int g = shift_gates[q];
      if (g >= n_gates) return fail(h, "shift_gates entry out of range");
      if (pass == 0 || g < 0 || shifts[q] == 0.f) continue;
      const Gate& G = h->model.gates[size_t(g)];
      if (two_term_rule && G.kind == QHBM_GATE_ISWAPPOW) return fail(h, kNoTwoTermRule);
      if (G.param_idx < 0)
        return fail(h, "shift_gates entry addresses a gate with a constant exponent: only parametrised gates have shifted programs");
    }
  return 0;
}

// ---- signed shot sums of Pauli-Z strings (qhbm_sample_parities, qhbm_sample_parities_states; sample_parity.hip) ----
constexpr int kParityMaxMasks = 1024;
constexpr int64_t kParityMaxShots = 2147483647;

// The masks are a HOST array in qubit space; *idx = the same strings in amplitude-index space (qubit 0 = the most
// significant of the n index bits).
int check_parity_masks(qhbm_engine* h, int n, const uint64_t* masks, int T, int64_t n_shots, std::vector<uint32_t>* idx) {
  if (T < 1 || T > kParityMaxMasks) return fail(h, "T (the number of masks) must be in [1, 1024]");
  if (n_shots < 0) return fail(h, "negative shot count");
  if (n_shots > kParityMaxShots) return fail(h, "too many shots: n_shots <= 2^31 - 1");
  if (!masks) return fail(h, "masks is NULL");
  idx->assign(size_t(T), 0u);
  for (int t = 0; t < T; ++t) {
    if (n < 64 && (masks[t] >> n) != 0)
      return fail(h, "masks[" + std::to_string(t) + "] has a bit at or above n_qubits = " + std::to_string(n));
    for (int k = 0; k < n; ++k)
      if ((masks[t] >> k) & 1u) (*idx)[size_t(t)] |= 1u << (n - 1 - k);
  }
  return 0;
}

int check_parity_states_shape(int M, int n_qubits) {
  if (M <= 0) return fail(nullptr, "M (the number of states) must be positive");
  if (n_qubits < 1 || n_qubits > 31) return fail(nullptr, "n_qubits must be in [1, 31]");
  return 0;
}

constexpr size_t kParityMaskBytes = size_t(kParityMaxMasks) * sizeof(uint32_t);  // the head of the states entry's scratch

}  // namespace

// ================================================================================
extern "C" {

int qhbm_abi_version(void) { return QHBM_ABI_VERSION; }

int qhbm_create(int device, qhbm_engine** out) {
  if (!out) return fail(nullptr, "out is NULL");
  std::unique_ptr<qhbm_engine> h(new qhbm_engine());
  h->device = device;
  if (const char* bb = std::getenv("QHBM_OBS_BLOCK_BITS"))  // (A/B runs of whole programs: the options' defaults)
    if (std::atoi(bb) == kObsBlockBits || std::atoi(bb) == kObsBlockBitsSmall) h->opt_obs_block_bits = std::atoi(bb);
  if (const char* sr = std::getenv("QHBM_OBS_SPLIT_ROWS")) h->opt_obs_split_rows = std::atoi(sr) != 0;
  if (device >= 0) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || device >= count)
      return fail(nullptr, std::string("no HIP device ") + std::to_string(device) + ": " +
                               (e != hipSuccess ? hipGetErrorString(e) : "index out of range"));
    e = hipSetDevice(device);
    if (e != hipSuccess) return fail(nullptr, std::string("hipSetDevice: ") + hipGetErrorString(e));
  }
  *out = h.release();
  return 0;
}

void qhbm_destroy(qhbm_engine* h) {
  if (!h) return;
  if (h->device >= 0) (void)hipSetDevice(h->device);
  for (auto& ev : h->events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
  for (auto& ev : h->free_events) { (void)hipEventDestroy(ev.a); (void)hipEventDestroy(ev.b); }
  delete h;
}

const char* qhbm_last_error(const qhbm_engine* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int qhbm_set_circuit(qhbm_engine* h, int n_qubits, int n_gates, const qhbm_gate* gates, int n_params) {
  if (!h) return 1;
  if (n_qubits < 1 || n_qubits > 31) return fail(h, "n_qubits must be in [1, 31]");
  if (n_gates < 0 || n_params < 0 || (n_gates > 0 && !gates)) return fail(h, "bad gate list");
  static_assert(sizeof(qhbm_gate) == sizeof(Gate), "ABI gate layout");
  Model m = h->model;
  if (m.n != n_qubits) { m.terms.clear(); m.n_ops = 0; }
  m.n = n_qubits;
  m.n_params = n_params;
  m.param_frozen.clear();  // (a mask belongs to the circuit it was set for)
  m.gates.resize(size_t(n_gates));
  if (n_gates) std::memcpy(m.gates.data(), gates, size_t(n_gates) * sizeof(Gate));
  for (const Gate& G : m.gates)
    if (!std::isfinite(G.global_shift)) return fail(h, "gate with a non-finite global_shift");
  Plan probe;
  std::string err;
  Model no_obs = m;
  no_obs.terms.clear();
  no_obs.n_ops = 0;
  PlanOptions po;
  po.tile_bits = h->opt_tile;
  po.round_bits = h->opt_round;
  if (!build_plan(no_obs, po, &probe, &err)) return fail(h, err);
  h->model = std::move(m);
  h->have_circuit = true;
  invalidate_plans(h);
  h->block_choice = -1;
  return 0;
}

int qhbm_set_gradient_mask(qhbm_engine* h, const uint8_t* needs_grad, int n_params) {
  if (!h) return 1;
  if (!h->have_circuit) return fail(h, "call qhbm_set_circuit first");
  std::vector<char> frozen;
  if (needs_grad) {
    if (n_params != h->model.n_params) return fail(h, "gradient mask: n_params differs from the circuit's");
    frozen.resize(size_t(n_params));
    bool any = false;
    for (int i = 0; i < n_params; ++i) any |= (frozen[size_t(i)] = needs_grad[i] ? 0 : 1) != 0;
    if (!any) frozen.clear();
  }
  if (frozen != h->model.param_frozen) {
    // the backward plan and the shift tables depend on the mask; the forward plan does not
    const std::vector<char> leaving = h->model.param_frozen;
    auto retarget = [&]() {  // the backward plan of the plan set that is in
      if (h->plans_valid && h->adj_valid) {  // keep the plan of the mask that is leaving (at most four)
        if (h->adj_cache.size() >= 4) h->adj_cache.erase(h->adj_cache.begin());
        h->adj_cache.emplace_back(leaving, std::unique_ptr<DevicePlan>(new DevicePlan()));
        h->adj_cache.back().second->swap(h->adj);
      }
      h->adj_valid = false;
      for (size_t i = 0; i < h->adj_cache.size(); ++i)
        if (h->plans_valid && h->adj_cache[i].first == frozen) {  // seen before: swap it back in
          h->adj.swap(*h->adj_cache[i].second);
          h->adj_cache.erase(h->adj_cache.begin() + long(i));
          h->adj_valid = true;
          h->model_uploaded = false;  // (the parameter -> slot tables follow the plan: a few KiB, no planning)
          break;
        }
    };
    retarget();
    swap_plan_sets(h);  // ... and of the dense-start set (nothing to do before the first from-states call)
    retarget();
    swap_plan_sets(h);
    h->model.param_frozen = std::move(frozen);
    h->shift_ready = false;
    consume_workspace(h);
  }
  return 0;
}

int qhbm_set_observables(qhbm_engine* h, int n_ops, const int32_t* term_offsets, const float* coeffs,
                         const uint64_t* x_masks, const uint64_t* z_masks) {
  if (!h) return 1;
  if (!h->have_circuit) return fail(h, "call qhbm_set_circuit first");
  if (n_ops < 1 || n_ops > kMaxOps || !term_offsets) return fail(h, "n_ops must be in [1, 1024]");
  const int n = h->model.n;
  std::vector<PauliTerm> terms;
  for (int k = 0; k < n_ops; ++k) {
    if (term_offsets[k + 1] < term_offsets[k]) return fail(h, "term_offsets must be non-decreasing");
    for (int j = term_offsets[k]; j < term_offsets[k + 1]; ++j) {
      const uint64_t x = x_masks[j], z = z_masks[j];
      if ((x | z) >> n) return fail(h, "Pauli mask addresses a qubit >= n_qubits");
      PauliTerm t;
      t.coeff = coeffs[j];
      t.x = t.z = 0;
      for (int q = 0; q < n; ++q) {
        if (x >> q & 1) t.x |= 1u << (n - 1 - q);
        if (z >> q & 1) t.z |= 1u << (n - 1 - q);
      }
      t.ny = __builtin_popcountll(x & z);
      t.op = k;
      terms.push_back(t);
    }
  }
  // fixed-point scale of every op's accumulator: partial sums are bounded by B = sum |c_k|
  h->h_op_scale.assign(size_t(n_ops), 0.f);
  h->h_op_inv_scale.assign(size_t(n_ops), 0.f);
  for (int k = 0; k < n_ops; ++k) {
    double bound = 0.0;
    for (int j = term_offsets[k]; j < term_offsets[k + 1]; ++j) bound += std::fabs(double(coeffs[j]));
    int e = 0;
    if (bound > 0.0) (void)std::frexp(bound, &e);  // bound <= 2^e
    e = std::max(-60, std::min(60, e));
    h->h_op_scale[size_t(k)] = float(std::ldexp(1.0, kValueFracBits - e));
    h->h_op_inv_scale[size_t(k)] = float(std::ldexp(1.0, e - kValueFracBits));
  }
  h->model.n_ops = n_ops;
  h->model.terms = std::move(terms);
  invalidate_plans(h);
  h->block_choice = -1;
  h->terms.release();
  return 0;
}

int qhbm_set_option(qhbm_engine* h, const char* name, int64_t value) {
  if (!h || !name) return 1;
  const std::string k(name);
  if (k == "tile_qubits") { h->opt_tile = int(value); invalidate_plans(h); h->block_choice = -1; }
  else if (k == "round_qubits") { h->opt_round = int(value); invalidate_plans(h); }
  else if (k == "force_general_kernels") h->opt_force_general = int(value);
  else if (k == "full_diag_threshold") { h->opt_full_fwd = int(value); invalidate_plans(h); }
  else if (k == "adjoint_full_diag_threshold") { h->opt_full_adj = int(value); invalidate_plans(h); }
  else if (k == "adjoint_tile_qubits") { h->opt_adj_tile = int(value); invalidate_plans(h); }
  else if (k == "adjoint_exchange") { h->opt_adj_exchange = int(value); invalidate_plans(h); }
  else if (k == "x_two_shear") { h->opt_x_two_shear = value != 0; invalidate_plans(h); h->adj_cache.clear(); h->dense.adj_cache.clear(); }
  else if (k == "adjoint_relabel") { h->opt_adj_relabel = int(value); invalidate_plans(h); }
  else if (k == "forward_pairs") h->opt_fwd_pair = int(value);
  else if (k == "shift_prefix_sharing") { h->opt_shift_prefix = int(value); h->shift_ready = false; }
  else if (k == "forward_values_from_observable") h->opt_fwd_values_obs = int(value);
  else if (k == "adjoint_stop_early") { h->opt_adj_stop_early = int(value); invalidate_plans(h); }
  else if (k == "adjoint_plan_search") { h->opt_adj_plan_search = int(value); invalidate_plans(h); }
  else if (k == "wide_last_pass") { h->opt_wide_last = int(value); invalidate_plans(h); }
  else if (k == "forward_move_low_bits") { h->opt_fwd_move_low = int(value); invalidate_plans(h); }
  else if (k == "observable_xcd_states") h->opt_obs_xcd_states = int(value);
  else if (k == "observable_kernel") { h->opt_obs_kernel = int(value); h->block_choice = -1; }
  else if (k == "observable_split_rows") h->opt_obs_split_rows = value != 0;
  else if (k == "observable_block_bits") {
    if (value != kObsBlockBits && value != kObsBlockBitsSmall) return fail(h, "observable_block_bits: 12 or 13");
    h->opt_obs_block_bits = int(value); h->block_choice = -1; h->terms.release(); h->model_uploaded = false;
  }
  else if (k == "multi_observable_values") h->opt_multi_values = int(value);
  else if (k == "gather_multi_values") h->opt_gather_multi = int(value);
  else if (k == "observable_far_windows") { h->opt_far_windows = int(value); h->terms.release(); h->model_uploaded = false; }
  else if (k == "measure_tile_qubits") { h->opt_meas_tile = int(value); invalidate_plans(h); }
  else if (k == "values_from_observable") h->opt_values_from_obs = int(value);
  else if (k == "cph_wave_bits") { h->opt_cph_wave_bits = int(value); invalidate_plans(h); }
  else if (k == "chunk_states") h->opt_chunk = value;
  else if (k == "evolve_step_argument") {
    if (value < 1 || value > 64) return fail(h, "evolve_step_argument: 1 .. 64");
    h->opt_evolve_step = int(value);
  }
  else if (k == "workspace_budget_mb") h->opt_budget_mb = std::max<int64_t>(0, value);  // 0 = default
  else if (k == "profile_events") h->opt_profile = int(value);
  else return fail(h, "unknown option '" + k + "'");
  return 0;
}

int qhbm_workspace_bytes(qhbm_engine* h, int U, int with_vjp, size_t* out) {
  if (!h || !out) return 1;
  if (int rc = build_plans(h)) return rc;
  const uint32_t cs = with_vjp ? adjoint_chunk_states(h, U) : chunk_states(h, U);  // as the calls chunk
  size_t b = size_t(cs) * state_bytes(h) * (with_vjp ? 2 : 1);
  if (with_vjp) {
    b += size_t(U) * h->adj.plan.slot_gate.size() * sizeof(float);
    size_t rows = 0;  // per-tile gradient rows of the widest adjoint pass
    for (const Pass& p : h->adj.plan.passes)
      rows = std::max(rows, ((size_t(cs) << p.nonlocal_pos.size()) +
                             reduce_tiles_scratch_rows(cs, size_t(1) << p.nonlocal_pos.size())) * size_t(std::max(p.n_slots, 1)));
    b += rows * sizeof(float);
  }
  b += size_t(U) * size_t(std::max(h->model.n_ops, 1)) * sizeof(unsigned long long);
  *out = b;
  return 0;
}

int qhbm_allocated_bytes(qhbm_engine* h, size_t* out) {
  if (!h || !out) return 1;
  *out = own_bytes(h);
  return 0;
}

int qhbm_retained_states(qhbm_engine* h, int* out_U) {
  if (!h || !out_U) return 1;
  *out_U = h->retained_U;
  return 0;
}

int qhbm_expectation(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, float* d_out,
                     void* stream) {
  if (int rc = begin_call(h, U, kNeedObservables)) return rc;
  if (U == 0) return 0;
  return forward(h, d_bits, U, d_params, d_out, -1, 0.0, static_cast<hipStream_t>(stream));
}

int qhbm_expectation_retain(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, float* d_out,
                            void* stream) {
  if (int rc = begin_call(h, U, kNeedObservables)) return rc;
  if (U == 0) return 0;
  return forward(h, d_bits, U, d_params, d_out, -1, 0.0, static_cast<hipStream_t>(stream), true);
}

int qhbm_expectation_vjp_retained(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                                  const float* d_upstream, float* d_grad, void* stream) {
  if (int rc = begin_call(h, U, kNeedObservables)) return rc;
  if (U <= 0 || h->retained_U != U) return fail(h, "no retained forward state for this batch");
  if (h->retained_table) return fail(h, "the retained states are an energy-table call's: use qhbm_table_expectation_vjp_retained");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool mu = h->retained_mu;  // lambda = O psi (unweighted) was computed with the values: the rows are weighted instead
  consume_workspace(h);  // the backward sweep un-applies psi in place: the state is consumed
  HIPCHK(begin_state_grad(h, size_t(U), s));
  Sweep sw{d_bits, U, d_params, Chunks::kResident};
  sw.with_lam = sw.backward = true;
  if (int rc = run_sweep(h, sw, s, no_reserve, [&](uint32_t s0, uint32_t c) -> int {
        if (!mu)
          if (int rc = run_observable_chunk(h, s0, c, d_upstream, false, s)) return rc;
        return run_adjoint_chunk(h, d_bits, s0, c, s);
      }))
    return rc;
  if (mu) HIPCHK(weight_state_grad(h, uint32_t(U), d_upstream, s));
  return reduce_state_grad(h, U, d_grad, false, true, s);
}

int qhbm_state_gradients(qhbm_engine* h, int U, float* d_rows, void* stream) {
  if (!h || !d_rows) return 1;
  if (int rc = need_device(h)) return rc;
  // (rows of a from-states VJP: the slots are those of the dense-start backward plan)
  std::optional<DenseScope> scope;
  if (h->state_grad_dense && h->state_grad_U > 0) scope.emplace(h);
  if (U <= 0 || U != h->state_grad_U || !h->plans_valid || !h->adj_valid)
    return fail(h, "qhbm_state_gradients: the last call was not an adjoint VJP on this many states");
  HIPCHK(launch_scatter_jac(h->state_grad.p, uint32_t(U), uint32_t(h->adj.plan.slot_gate.size()),
                            h->param_slot_begin.p, h->param_slots.p, h->slot_factor.p, d_rows, 1u, 0u,
                            uint32_t(h->model.n_params), static_cast<hipStream_t>(stream)));
  return 0;
}

int qhbm_statevector(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                     void* d_out_states, void* stream) {
  if (int rc = begin_call(h, U, 0)) return rc;
  if (U == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t row = size_t(8) << h->model.n, pitch = size_t(8) << h->fwd.plan.n_eff;
  Sweep sw{d_bits, U, d_params};
  sw.keep_state = sw.values = true;  // (values of installed observables are a by-product; they stay in the fixed-point scratch)
  if (int rc = run_sweep(h, sw, s, no_reserve, [&](uint32_t s0, uint32_t c) -> int {
        // idle padding qubits (n < 10) are the high index bits and stay |0>: keep the first 2^n amplitudes
        HIPCHK(hipMemcpy2DAsync(static_cast<char*>(d_out_states) + size_t(s0) * row, row, h->psi.p, pitch, row, c,
                                hipMemcpyDeviceToDevice, s));
        return 0;
      }))
    return rc;
  HIPCHK(global_phase(h, d_params, s));
  HIPCHK(apply_global_phase(h, d_out_states, U, s));
  return 0;
}

// ---- caller-supplied start states (include/qhbm_engine.h): the same sweeps on the dense-start plan set, the chunk's
// states imported by run_forward_chunk (import_chunk) ----
}  // extern "C"

namespace {

// The import's per-call buffers; from here on run_forward_chunk imports (the DenseScope of the call ends that).
int begin_import(qhbm_engine* h, const void* d_states, int U, const float* d_upstream, hipStream_t stream) {
  HIPCHK(h->import_norm2.reserve(size_t(U)));
  const size_t nb = (size_t(U) * size_t(h->model.n) + 15u) & ~size_t(15);
  if (nb > h->import_bits.n) {
    HIPCHK(h->import_bits.reserve(nb, false));
    HIPCHK(launch_zero_fill(h->import_bits.p, h->import_bits.n, stream));
  }
  if (d_upstream) HIPCHK(h->import_up.reserve(size_t(U) * size_t(h->model.n_ops)));
  h->import_src = static_cast<const float2*>(d_states);
  h->import_upstream = d_upstream;
  h->import_U = U;
  return 0;
}

// The final states of a from-states chunk leave the workspace for the caller's rows [s0, s0 + c): idle padding qubits
// stay |0>, so the first 2^n amplitudes of a row, times ||phi|| -- the state as given, evolved (the phase follows once,
// over the whole output: apply_global_phase).
hipError_t export_chunk(qhbm_engine* h, void* d_out_states, uint32_t s0, uint32_t c, hipStream_t s) {
  const uint32_t n = uint32_t(h->model.n);
  return launch_scale_copy_states(h->psi.p, uint32_t(h->fwd.plan.n_eff), static_cast<float2*>(d_out_states) + (size_t(s0) << n), n, n,
                                  c, nullptr, h->import_norm2.p + s0, s);
}

}  // namespace

extern "C" {

int qhbm_expectation_from_states(qhbm_engine* h, const void* d_states, int U, const float* d_params, float* d_out,
                                 void* stream) {
  if (int rc = begin_call(h, U, kNeedCircuit | kNeedObservables | kNeedStates | kNoUpload, d_states)) return rc;
  DenseScope scope(h);
  if (int rc = upload_model(h)) return rc;
  if (U == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = begin_import(h, d_states, U, nullptr, s)) return rc;
  if (int rc = forward(h, h->import_bits.p, U, d_params, d_out, -1, 0.0, s)) return rc;
  // the sweep ran on phi / ||phi||: the values of the states as given
  if (d_out) HIPCHK(launch_scale_by_norm2(d_out, d_out, uint32_t(U), uint32_t(h->model.n_ops), h->import_norm2.p, s));
  return 0;
}

int qhbm_expectation_vjp_from_states(qhbm_engine* h, const void* d_states, int U, const float* d_params,
                                     const float* d_upstream, float* d_out_vals, float* d_grad, void* stream) {
  if (int rc = begin_call(h, U, kNeedCircuit | kNeedObservables | kNeedStates | kNoUpload, d_states)) return rc;
  if (!d_grad || (U > 0 && !d_upstream)) return fail(h, "d_upstream or d_grad is NULL");
  DenseScope scope(h);
  if (int rc = upload_model(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (U == 0) return empty_batch_grad(h, d_grad, s);
  if (int rc = values_or_scratch(h, U, &d_out_vals)) return rc;
  if (int rc = begin_import(h, d_states, U, d_upstream, s)) return rc;
  // lambda = sum_k (upstream[u, k] ||phi_u||^2) O_k psi_u on the normalised psi_u: the gradient of the states as given
  if (int rc = adjoint_sweep(h, h->import_bits.p, U, d_params, h->import_up.p, d_out_vals, s)) return rc;
  HIPCHK(launch_scale_by_norm2(d_out_vals, d_out_vals, uint32_t(U), uint32_t(h->model.n_ops), h->import_norm2.p, s));
  return reduce_state_grad(h, U, d_grad, true, true, s);
}

int qhbm_statevector_from_states(qhbm_engine* h, const void* d_states, int U, const float* d_params, void* d_out_states,
                                 void* stream) {
  if (int rc = begin_call(h, U, kNeedCircuit | kNeedStates | kNoUpload, d_states)) return rc;
  if (U > 0 || d_out_states)
    if (int rc = check_pointer(h, d_out_states, 16, "d_out_states")) return rc;
  DenseScope scope(h);
  if (int rc = upload_model(h)) return rc;
  if (U == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (int rc = begin_import(h, d_states, U, nullptr, s)) return rc;
  Sweep sw{h->import_bits.p, U, d_params};
  sw.keep_state = sw.values = true;  // (by-product values of installed observables stay in the scratch)
  // (a circuit without gates: the imported states are the result.  The plan's one pass would load and store them
  // unchanged; it is skipped -- and with it the by-product values of installed observables, which nobody can read --
  // so that the forward events of such a call time the import alone: scripts/from_states_time.py measures it this way)
  sw.passes = !h->model.gates.empty();
  auto export_rows = [&](uint32_t s0, uint32_t c) -> int { HIPCHK(export_chunk(h, d_out_states, s0, c, s)); return 0; };
  if (int rc = run_sweep(h, sw, s, no_reserve, export_rows)) return rc;
  HIPCHK(global_phase(h, d_params, s));
  HIPCHK(apply_global_phase(h, d_out_states, U, s));
  return 0;
}

int qhbm_statevector_vjp_from_states(qhbm_engine* h, const void* d_states, int U, const float* d_params,
                                     const void* d_cotangent, void* d_out_states, float* d_grad, void* stream) {
  if (int rc = begin_call(h, U, kNeedCircuit | kNeedStates | kNoUpload, d_states)) return rc;
  if (!d_grad) return fail(h, "d_grad is NULL");
  if (d_out_states)
    if (int rc = check_pointer(h, d_out_states, 16, "d_out_states")) return rc;
  const size_t bytes = size_t(U) * (size_t(8) << h->model.n);
  if (U > 0) {
    if (int rc = check_pointer(h, d_cotangent, 16, "d_cotangent")) return rc;
    if (aliases_workspace(h, d_cotangent, bytes)) return fail(h, "d_cotangent lies inside the engine's workspace");
    if (d_out_states && (ranges_overlap(d_out_states, bytes, d_cotangent, bytes) || ranges_overlap(d_out_states, bytes, d_states, bytes)))
      return fail(h, "d_out_states overlaps d_states or d_cotangent");
  }
  DenseScope scope(h);
  if (int rc = upload_model(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  consume_workspace(h);
  if (U == 0) return empty_batch_grad(h, d_grad, s);
  if (int rc = begin_import(h, d_states, U, nullptr, s)) return rc;
  HIPCHK(begin_state_grad(h, size_t(U), s));
  HIPCHK(global_phase(h, d_params, s));
  const uint32_t n = uint32_t(h->model.n), n_eff = uint32_t(h->fwd.plan.n_eff);
  const float2* cot = static_cast<const float2*>(d_cotangent);
  Sweep sw{h->import_bits.p, U, d_params, Chunks::kPairs};
  sw.with_lam = sw.backward = sw.keep_state = sw.skip_measure = true;
  if (int rc = run_sweep(
          h, sw, s,
          [&](uint32_t cs) -> int {
            // (the buffers may have moved: the check again, on the workspace the sweep will use)
            if (aliases_workspace(h, d_cotangent, bytes)) return fail(h, "d_cotangent lies inside the engine's workspace");
            HIPCHK(h->cot_parts.reserve(cotangent_parts_count(n, cs)));
            HIPCHK(h->cot_dot.reserve(size_t(U) * 2));
            return 0;
          },
          [&](uint32_t s0, uint32_t c) -> int {
            if (d_out_states) HIPCHK(export_chunk(h, d_out_states, s0, c, s));  // before the backward sweep un-applies psi in place
            hipEvent_t* ev = timer_begin(h, 2, s);  // (profile_events: the cotangent import counts as the lambda launch)
            HIPCHK(launch_cotangent_import(cot, h->psi.p, n, n_eff, c, s0, h->import_norm2.p, h->phase_cs.p, h->lam.p,
                                           h->cot_parts.p, h->cot_dot.p, s));
            timer_end(ev, s);
            return run_adjoint_chunk(h, h->import_bits.p, s0, c, s);
          }))
    return rc;
  if (d_out_states) HIPCHK(apply_global_phase(h, d_out_states, U, s));
  // (qhbm_state_gradients is refused after this call: the rows lack the phase term, which goes into d_grad alone)
  if (int rc = reduce_state_grad(h, U, d_grad, true, false, s)) return rc;
  HIPCHK(launch_cotangent_phase_grad(h->cot_dot.p, h->import_norm2.p, uint32_t(U), h->phase_cs.p, h->phase_slope.p, d_grad,
                                     uint32_t(h->model.n_params), s));
  return 0;
}

int qhbm_describe_schedule_from_states(qhbm_engine* h, char* buf, size_t buf_len) {
  if (!h || !buf || !buf_len) return 1;
  DenseScope scope(h);
  if (int rc = build_plans(h)) return rc;
  std::snprintf(buf, buf_len, "%s", describe_plans(h).c_str());
  return 0;
}

// ---- Chebyshev evolution of caller-supplied states (include/qhbm_engine.h): e^{-tau H} and e^{-i tau H}
// for H = sum_k w_k O_k over the installed observables, from repeated launches of the lambda = O psi kernels ----
}  // extern "C"

namespace {

// What (weights, tau, mode) and the installed observables fix: nothing of it is read from the device.
struct EvolvePlan {
  double R = 0.0;  // sum_k |w_k| sum_j |c_kj| >= ||H||
  int steps = 0;   // m = ceil(|tau| R / evolve_step_argument)
  int terms = 0;   // K: H-applications of one step
  double x = 0.0;  // |tau| R / m
  std::vector<double> re, im;  // c_0 .. c_K of a step: sum_k c_k T_k(H / R)
};

// f_k proportional to I_k(x) (mode 0) or J_k(x) (mode 1), k = 0 .. N, by Miller's backward recurrence; normalised with
// I_0 + 2 sum I_k = e^x (so the result is e^{-x} I_k) or J_0 + 2 sum J_2k = 1.
std::vector<double> bessel_sequence(double x, int mode) {
  const int N = 2 * int(std::ceil(x)) + 64;
  std::vector<double> f(size_t(N) + 2, 0.0);
  f[size_t(N)] = 1.0;
  for (int k = N; k >= 1; --k) {
    const double up = mode == 0 ? f[size_t(k) + 1] : -f[size_t(k) + 1];
    f[size_t(k) - 1] = (2.0 * double(k) / x) * f[size_t(k)] + up;
    if (std::fabs(f[size_t(k) - 1]) > 1e250)
      for (int j = k - 1; j <= N; ++j) f[size_t(j)] *= 1e-250;
  }
  double norm = f[0];
  for (int k = 1; k <= N; ++k)
    if (mode == 0 || k % 2 == 0) norm += 2.0 * f[size_t(k)];
  for (double& v : f) v /= norm;
  f.pop_back();
  return f;
}

// R = sum_k |w_k| sum_j |c_kj| over the installed observables (weights NULL: ones); refuses a weight that is not finite
int weighted_radius(qhbm_engine* h, const double* weights, double* R) {
  std::vector<double> op_sum(size_t(h->model.n_ops), 0.0);
  for (const PauliTerm& t : h->model.terms) op_sum[size_t(t.op)] += std::fabs(double(t.coeff));
  *R = 0.0;
  for (int k = 0; k < h->model.n_ops; ++k) {
    const double w = weights ? weights[k] : 1.0;
    if (!std::isfinite(w)) return fail(h, "a weight is not finite");
    *R += std::fabs(w) * op_sum[size_t(k)];
  }
  return 0;
}

int make_evolve_plan(qhbm_engine* h, const double* weights, double tau, int mode, EvolvePlan* out) {
  if (h->model.n_ops <= 0) return fail(h, "qhbm_set_observables has not been called");
  if (mode != 0 && mode != 1) return fail(h, "mode must be 0 (imaginary time) or 1 (real time)");
  if (!std::isfinite(tau)) return fail(h, "tau is not finite");
  if (mode == 0 && tau < 0.0) return fail(h, "tau < 0 in imaginary time (mode 0)");
  EvolvePlan p;
  if (int rc = weighted_radius(h, weights, &p.R)) return rc;
  const double arg = std::fabs(tau) * p.R;
  if (!std::isfinite(arg) || arg > 1e9) return fail(h, "|tau| R is too large");
  p.steps = int(std::ceil(arg / double(h->opt_evolve_step)));
  if (p.steps > 0) {
    p.x = arg / double(p.steps);
    const std::vector<double> a = bessel_sequence(p.x, mode);
    // cut where the discarded tail 2 sum |a_k| falls below 2^-30 (at least one term)
    double tail = 0.0;
    int K = int(a.size()) - 1;
    while (K > 1 && tail + 2.0 * std::fabs(a[size_t(K)]) < std::ldexp(1.0, -30)) tail += 2.0 * std::fabs(a[size_t(K--)]);
    p.terms = K;
    const double sgn = tau >= 0.0 ? 1.0 : -1.0;
    for (int k = 0; k <= K; ++k) {
      const double v = (k ? 2.0 : 1.0) * a[size_t(k)];
      if (mode == 0) {
        p.re.push_back(k % 2 ? -v : v);
        p.im.push_back(0.0);
      } else {  // (-i sgn)^k
        static const double cr[4] = {1.0, 0.0, -1.0, 0.0}, ci[4] = {0.0, -1.0, 0.0, 1.0};
        p.re.push_back(cr[k % 4] * v);
        p.im.push_back(ci[k % 4] * sgn * v);
      }
    }
  }
  *out = std::move(p);
  return 0;
}

int check_evolve_states(qhbm_engine* h, const void* d_states, int U, const char* what) {
  if (U <= 0) return fail(h, "U must be positive");
  if (!h->have_circuit) return fail(h, "qhbm_set_circuit has not been called");
  if (h->model.n_ops <= 0) return fail(h, "qhbm_set_observables has not been called");
  if (int rc = check_pointer(h, d_states, 16, what)) return rc;
  if (aliases_workspace(h, d_states, size_t(U) * (size_t(8) << h->model.n)))
    return fail(h, std::string(what) + " lies inside the engine's workspace");
  return 0;
}

// w_k * factor (weights NULL: ones) to the device, in stream order; the host copy lives in the engine
int upload_evolve_weights(qhbm_engine* h, const double* weights, double factor, hipStream_t s) {
  const size_t n_ops = size_t(h->model.n_ops);
  h->evo_host_wr.resize(n_ops);
  for (size_t k = 0; k < n_ops; ++k) h->evo_host_wr[k] = (weights ? weights[k] : 1.0) * factor;
  HIPCHK(h->evo_wr.reserve(n_ops));
  HIPCHK(hipMemcpyAsync(h->evo_wr.p, h->evo_host_wr.data(), n_ops * sizeof(double), hipMemcpyHostToDevice, s));
  return 0;
}

// out = H in for c states under the upstream rows in evo_up1; in, out: rows at the caller's pitch of 2^n amplitudes.
// n = n_eff: that is the workspace's pitch, and the observable kernel reads and writes the caller's rows.  Otherwise the
// rows are staged through psi and the result leaves lam for `out` -- unless `out` is lam itself, where it stays, at the
// workspace's pitch (qhbm_krylov_basis orthogonalises it there).
int apply_h_chunk(qhbm_engine* h, const float2* in, float2* out, uint32_t c, hipStream_t s) {
  const uint32_t n = uint32_t(h->model.n), n_eff = uint32_t(h->fwd.plan.n_eff);
  if (n == n_eff) return run_observable_chunk(h, 0, c, h->evo_up1.p, false, s, true, false, in, out);
  HIPCHK(launch_scale_copy_states(in, n, h->psi.p, n_eff, n, c, nullptr, nullptr, s));
  if (int rc = run_observable_chunk(h, 0, c, h->evo_up1.p, false, s)) return rc;
  if (out != h->lam.p) HIPCHK(launch_scale_copy_states(h->lam.p, n_eff, out, n, n, c, nullptr, nullptr, s));
  return 0;
}

}  // namespace

extern "C" {

int qhbm_describe_evolution(qhbm_engine* h, const double* weights, double tau, int mode, char* buf, size_t buf_len) {
  if (!h || !buf || !buf_len) return 1;
  EvolvePlan p;
  if (int rc = make_evolve_plan(h, weights, tau, mode, &p)) return rc;
  std::snprintf(buf, buf_len, "R=%.17g steps=%d terms_per_step=%d applications=%d", p.R, p.steps, p.terms, p.steps * p.terms);
  return 0;
}

int qhbm_apply_observables(qhbm_engine* h, const void* d_states, int U, const double* weights, void* d_out_states,
                           void* stream) {
  if (!h) return 1;
  if (int rc = need_device(h)) return rc;
  if (int rc = check_evolve_states(h, d_states, U, "d_states")) return rc;
  if (int rc = check_evolve_states(h, d_out_states, U, "d_out_states")) return rc;
  const size_t row = size_t(8) << h->model.n;
  if (ranges_overlap(d_states, size_t(U) * row, d_out_states, size_t(U) * row)) return fail(h, "d_out_states overlaps d_states");
  if (weights)
    for (int k = 0; k < h->model.n_ops; ++k)
      if (!std::isfinite(weights[k])) return fail(h, "a weight is not finite");
  DenseScope scope(h);
  if (int rc = upload_model(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  consume_workspace(h);
  const uint32_t n = uint32_t(h->model.n), n_eff = uint32_t(h->fwd.plan.n_eff), n_ops = uint32_t(h->model.n_ops);
  if (int rc = upload_evolve_weights(h, weights, 1.0, s)) return rc;
  const uint32_t cs = adjoint_chunk_states(h, U);
  HIPCHK(h->evo_up1.reserve(size_t(cs) * n_ops));
  if (n != n_eff)
    if (int rc = ensure_state_buffers(h, cs, true)) return rc;
  return for_each_chunk(U, cs, [&](uint32_t s0, uint32_t c) -> int {
    const float2* in = reinterpret_cast<const float2*>(static_cast<const char*>(d_states) + size_t(s0) * row);
    float2* out = reinterpret_cast<float2*>(static_cast<char*>(d_out_states) + size_t(s0) * row);
    HIPCHK(launch_evolve_init(c, nullptr, nullptr, nullptr, h->evo_wr.p, n_ops, h->evo_up1.p, nullptr, s));
    return apply_h_chunk(h, in, out, c, s);
  });
}

int qhbm_evolve_states(qhbm_engine* h, void* d_states, int U, const double* weights, double tau, int mode,
                       double* d_log_norms, void* stream) {
  if (!h) return 1;
  if (int rc = need_device(h)) return rc;
  if (int rc = check_evolve_states(h, d_states, U, "d_states")) return rc;
  EvolvePlan ep;
  if (int rc = make_evolve_plan(h, weights, tau, mode, &ep)) return rc;
  if (mode == 1 && d_log_norms) return fail(h, "d_log_norms must be NULL in real time (mode 1)");
  DenseScope scope(h);
  if (int rc = upload_model(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  consume_workspace(h);
  const uint32_t n = uint32_t(h->model.n), n_eff = uint32_t(h->fwd.plan.n_eff), n_ops = uint32_t(h->model.n_ops);
  const size_t row = size_t(8) << n, pitch = size_t(1) << n_eff;
  // R = 0 (H = 0), and no step in real time: the identity -- the states are not written
  const bool identity = ep.R == 0.0 || (ep.steps == 0 && mode == 1);
  if (identity && !d_log_norms) return 0;
  // four state buffers per chunk element: t_{k-1}, t_k in psi, w and the sum in lam
  uint32_t cs = chunk_states(h, U);
  if (h->opt_chunk <= 0)
    cs = uint32_t(std::min<size_t>(std::min<size_t>(size_t(U), 65535), std::max<size_t>(1, budget_bytes(h) / (4 * state_bytes(h)))));
  if (int rc = ensure_state_buffers(h, 2 * cs, true)) return rc;
  if (aliases_workspace(h, d_states, size_t(U) * row)) return fail(h, "d_states lies inside the engine's workspace");
  if (int rc = upload_evolve_weights(h, weights, ep.R > 0.0 ? 1.0 / ep.R : 0.0, s)) return rc;
  HIPCHK(h->import_norm2.reserve(size_t(U)));
  HIPCHK(h->import_parts.reserve(state_norm_parts_count(n, cs)));
  HIPCHK(h->evo_scale.reserve(cs));
  HIPCHK(h->evo_parts.reserve(state_norm_parts_count(n_eff, cs)));
  HIPCHK(h->evo_up1.reserve(size_t(cs) * n_ops));
  HIPCHK(h->evo_up2.reserve(size_t(cs) * n_ops));
  double* log_norm = d_log_norms;
  if (mode == 0 && !log_norm) {
    HIPCHK(h->evo_log_norm.reserve(size_t(U)));
    log_norm = h->evo_log_norm.p;
  }
  auto c32 = [&](int k) { return make_float2(float(ep.re[size_t(k)]), float(ep.im[size_t(k)])); };
  for (uint32_t s0 = 0; s0 < uint32_t(U); s0 += cs) {
    const uint32_t c = std::min<uint32_t>(cs, uint32_t(U) - s0);
    float2 *A = h->psi.p, *B = h->psi.p + size_t(cs) * pitch, *W = h->lam.p, *ACC = h->lam.p + size_t(cs) * pitch;
    float2* rows = reinterpret_cast<float2*>(static_cast<char*>(d_states) + size_t(s0) * row);
    // the sum starts as phi / ||phi|| (zeros for norm 0); ||phi||^2 stays on the device
    HIPCHK(launch_import_states(static_cast<const float2*>(d_states), n, n_eff, c, s0, ACC, h->import_parts.p, h->import_norm2.p, s));
    HIPCHK(launch_evolve_init(c, h->import_norm2.p + s0, mode == 0 ? log_norm + s0 : nullptr, h->evo_scale.p, h->evo_wr.p, n_ops,
                              h->evo_up1.p, h->evo_up2.p, s));
    if (identity) continue;
    for (int step = 0; step < ep.steps; ++step) {
      for (int k = 1; k <= ep.terms; ++k) {
        const bool first = k == 1, with_norm = mode == 0 && k == ep.terms;
        // w = (1 / R) H (sum * scale) for the first term (the rescale rides on the upstream row), (2 / R) H t_k after it
        if (int rc = run_observable_chunk(h, 0, c, first ? h->evo_up1.p : h->evo_up2.p, false, s, true, false, first ? ACC : B, W))
          return rc;
        hipEvent_t* ev = timer_begin(h, 0, s);  // (profile_events: the recurrence's sweeps count as forward launches)
        HIPCHK(launch_cheb_step(first, with_norm, W, A, ACC, n_eff, c, c32(0), c32(k), h->evo_scale.p, h->evo_parts.p, s));
        timer_end(ev, s);
        if (first) std::swap(B, W);  // t_1 was written as w
        else std::swap(A, B);        // t_{k+1} replaced t_{k-1}
      }
      // e^{delta R} never touches an amplitude: it enters the log norm as + x
      if (mode == 0)
        HIPCHK(launch_finish_step(h->evo_parts.p, n_eff, c, ep.x, log_norm + s0, h->evo_scale.p, h->evo_wr.p, n_ops, h->evo_up1.p, s));
    }
    // imaginary time: the sum over its norm; real time: back to the norm of the state as given
    HIPCHK(launch_scale_copy_states(ACC, n_eff, rows, n, n, c, mode == 0 ? h->evo_scale.p : nullptr,
                                    mode == 1 ? h->import_norm2.p + s0 : nullptr, s));
  }
  return 0;
}

// ---- Lanczos bases of caller-supplied states (include/qhbm_engine.h; krylov.hip) ----
}  // extern "C"

namespace {

constexpr int kKrylovMaxSteps = 1024;

int check_krylov_shape(qhbm_engine* h, int U, int m, int reorth) {
  if (U <= 0) return fail(h, "U must be positive");
  if (m < 1 || m > kKrylovMaxSteps) return fail(h, "m must be in [1, 1024]");
  if (reorth != 0 && reorth != 1) return fail(h, "reorth must be 0 (local) or 1 (full)");
  if (!h->have_circuit) return fail(h, "qhbm_set_circuit has not been called");
  if (h->model.n_ops <= 0) return fail(h, "qhbm_set_observables has not been called");
  return 0;
}

// Sweeps of one state's words by the project / subtract / normalise kernels of a whole basis, in units of one state
// (8 * 2^n bytes): per round and block of nb rows, project reads w and nb rows, subtract reads w and nb rows and writes w;
// the normalised write reads w and writes a row; the import reads the start state twice and writes row 0.
double krylov_state_sweeps(int m, int reorth) {
  double sweeps = 3.0;
  for (int j = 0; j < m; ++j) {
    const int lo = reorth ? 0 : std::max(0, j - 1), rows = j - lo + 1, blocks = (rows + kKrylovBlock - 1) / kKrylovBlock;
    sweeps += double(reorth ? 2 : 1) * double(3 * blocks + 2 * rows) + (j + 1 < m ? 2.0 : 0.0);
  }
  return sweeps;
}

}  // namespace

extern "C" {

int qhbm_describe_krylov(qhbm_engine* h, int U, int m, int reorth, char* buf, size_t buf_len) {
  if (!h || !buf || !buf_len) return 1;
  if (int rc = check_krylov_shape(h, U, m, reorth)) return rc;
  DenseScope scope(h);
  if (int rc = build_plans(h)) return rc;
  const double state = double(size_t(8) << h->model.n);
  const uint32_t cs = adjoint_chunk_states(h, U);
  std::snprintf(buf, buf_len, "basis_bytes=%.17g workspace_bytes=%.17g applications=%d chunk_states=%u krylov_bytes_per_state=%.17g",
                double(m) * double(U) * state, 2.0 * double(cs) * double(state_bytes(h)), m, cs, krylov_state_sweeps(m, reorth) * state);
  return 0;
}

int qhbm_krylov_basis(qhbm_engine* h, const void* d_start_states, int U, const double* weights, int m, int reorth,
                      void* d_basis, double* d_alpha, double* d_beta, int32_t* d_lengths, void* stream) {
  if (!h) return 1;
  if (int rc = need_device(h)) return rc;
  if (int rc = check_krylov_shape(h, U, m, reorth)) return rc;
  if (int rc = check_evolve_states(h, d_start_states, U, "d_start_states")) return rc;
  if (int rc = check_pointer(h, d_basis, 16, "d_basis")) return rc;
  if (int rc = check_pointer(h, d_alpha, 8, "d_alpha")) return rc;
  if (int rc = check_pointer(h, d_beta, 8, "d_beta")) return rc;
  if (int rc = check_pointer(h, d_lengths, 4, "d_lengths")) return rc;
  const uint32_t n = uint32_t(h->model.n);
  const size_t row = size_t(8) << n, basis_bytes = size_t(m) * size_t(U) * row;
  if (ranges_overlap(d_start_states, size_t(U) * row, d_basis, basis_bytes)) return fail(h, "d_basis overlaps d_start_states");
  double R = 0.0;
  if (int rc = weighted_radius(h, weights, &R)) return rc;
  DenseScope scope(h);
  if (int rc = upload_model(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  consume_workspace(h);
  const uint32_t n_eff = uint32_t(h->fwd.plan.n_eff), n_ops = uint32_t(h->model.n_ops);
  const uint32_t cs = adjoint_chunk_states(h, U);
  if (int rc = ensure_state_buffers(h, cs, true)) return rc;
  if (aliases_workspace(h, d_start_states, size_t(U) * row)) return fail(h, "d_start_states lies inside the engine's workspace");
  if (aliases_workspace(h, d_basis, basis_bytes)) return fail(h, "d_basis lies inside the engine's workspace");
  if (int rc = upload_evolve_weights(h, weights, 1.0, s)) return rc;
  HIPCHK(h->import_norm2.reserve(size_t(U)));
  HIPCHK(h->import_parts.reserve(state_norm_parts_count(n, cs)));
  HIPCHK(h->evo_scale.reserve(cs));
  HIPCHK(h->evo_up1.reserve(size_t(cs) * n_ops));
  HIPCHK(h->kry_parts.reserve(krylov_coef_parts_count(n, cs)));
  HIPCHK(h->kry_norm_parts.reserve(state_norm_parts_count(n, cs)));
  HIPCHK(h->kry_coef.reserve(size_t(cs) * size_t(m)));
  HIPCHK(launch_zero_fill(d_alpha, size_t(U) * size_t(m) * sizeof(double), s));
  const double threshold = std::ldexp(R, -16);
  const size_t amps = size_t(1) << n, stride = size_t(U) * amps;  // amplitudes from one basis row to the next
  float2* basis = static_cast<float2*>(d_basis);
  float2* W = h->lam.p;
  const int rounds = reorth ? 2 : 1;
  for (uint32_t s0 = 0; s0 < uint32_t(U); s0 += cs) {
    const uint32_t c = std::min<uint32_t>(cs, uint32_t(U) - s0);
    // v_0 = phi / ||phi|| straight into row 0 at the caller's pitch (zeros for norm 0); ||phi||^2 stays on the device
    hipEvent_t* iev = timer_begin(h, 0, s);  // (profile_events: the import and the Krylov kernels count as forward launches)
    HIPCHK(launch_import_states(static_cast<const float2*>(d_start_states), n, n, c, s0, basis + size_t(s0) * amps, h->import_parts.p,
                                h->import_norm2.p, s));
    timer_end(iev, s);
    HIPCHK(launch_krylov_init(c, h->import_norm2.p + s0, m, d_lengths + s0, h->evo_scale.p, s));
    HIPCHK(launch_evolve_init(c, nullptr, nullptr, nullptr, h->evo_wr.p, n_ops, h->evo_up1.p, nullptr, s));
    for (int j = 0; j < m; ++j) {
      const float2* vj = basis + size_t(j) * stride + size_t(s0) * amps;
      // w = H v_j: row j of the chunk is contiguous, so at n = n_eff the observable kernel reads the basis itself
      if (int rc = apply_h_chunk(h, vj, W, c, s)) return rc;
      hipEvent_t* ev = timer_begin(h, 0, s);
      const int lo = reorth ? 0 : std::max(0, j - 1), rows = j - lo + 1;
      for (int round = 0; round < rounds; ++round) {
        // classical Gram-Schmidt: every c_i of the round from the same w, then the subtractions, i ascending
        for (int b0 = 0; b0 < rows; b0 += kKrylovBlock) {
          const int nb = std::min(kKrylovBlock, rows - b0), i0 = lo + b0;
          HIPCHK(launch_krylov_project(W, n_eff, basis + size_t(i0) * stride + size_t(s0) * amps, stride, n, c, uint32_t(nb),
                                       h->kry_parts.p, h->kry_coef.p, uint32_t(m), uint32_t(b0), j >= i0 && j < i0 + nb ? j - i0 : -1,
                                       d_alpha + size_t(s0) * size_t(m) + size_t(j), uint64_t(m), s));
        }
        for (int b0 = 0; b0 < rows; b0 += kKrylovBlock) {
          const int nb = std::min(kKrylovBlock, rows - b0), i0 = lo + b0;
          const bool last = round + 1 == rounds && b0 + nb == rows;
          HIPCHK(launch_krylov_subtract(W, n_eff, basis + size_t(i0) * stride + size_t(s0) * amps, stride, n, c, uint32_t(nb),
                                        h->kry_coef.p + b0, uint32_t(m), last ? h->kry_norm_parts.p : nullptr, s));
        }
      }
      HIPCHK(launch_krylov_norm(h->kry_norm_parts.p, n, c, threshold, j, d_beta + size_t(s0) * size_t(m), uint64_t(m), d_lengths + s0,
                                h->evo_scale.p, s));
      // v_{j+1} = w / beta_j (scale 0 after a breakdown: zeros)
      if (j + 1 < m)
        HIPCHK(launch_scale_copy_states(W, n_eff, basis + size_t(j + 1) * stride + size_t(s0) * amps, n, n, c, h->evo_scale.p, nullptr, s));
      timer_end(ev, s);
    }
  }
  return 0;
}

int qhbm_krylov_combine(const void* d_basis, int m, int U, int n_qubits, const void* d_coef, int S, void* d_out_states,
                        void* stream) {
  if (m < 1 || m > kKrylovMaxSteps) return fail(nullptr, "m must be in [1, 1024]");
  if (U <= 0) return fail(nullptr, "U must be positive");
  if (S < 1) return fail(nullptr, "S must be at least 1");
  if (n_qubits < 1 || n_qubits > 34) return fail(nullptr, "n_qubits must be in [1, 34]");
  if (int rc = check_pointer(nullptr, d_basis, 16, "d_basis")) return rc;
  if (int rc = check_pointer(nullptr, d_coef, 8, "d_coef")) return rc;
  if (int rc = check_pointer(nullptr, d_out_states, 16, "d_out_states")) return rc;
  hipError_t e = launch_krylov_combine(static_cast<const float2*>(d_basis), uint32_t(m), uint32_t(U), uint32_t(n_qubits),
                                       static_cast<const float2*>(d_coef), uint32_t(S), static_cast<float2*>(d_out_states),
                                       static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_krylov_combine: ") + hipGetErrorString(e));
  return 0;
}

// ---- streamed Lanczos: the same results without a stored basis (include/qhbm_engine.h; krylov.hip) ----
}  // extern "C"

namespace {

constexpr uint32_t kKrylovRing = 3;             // v_{j-1}, v_j and v_{j+1} of pass one (the replay turns two of them)
constexpr uint32_t kKrylovStreamBuffers = 5;    // psi, lam and the ring: state buffers per chunk element

int check_krylov_stream_shape(qhbm_engine* h, int U, int m, int S) {
  if (int rc = check_krylov_shape(h, U, m, 0)) return rc;
  if (S < 1) return fail(h, "S must be at least 1");
  return 0;
}

uint32_t krylov_stream_chunk_states(qhbm_engine* h, int U) {
  uint32_t cs = chunk_states(h, U);
  if (h->opt_chunk <= 0)
    cs = uint32_t(std::min<size_t>(std::min<size_t>(size_t(U), 65535),
                                   std::max<size_t>(1, budget_bytes(h) / (kKrylovStreamBuffers * state_bytes(h)))));
  return cs;
}

// Rows j - 1 and j of pass one lie in the ring's slots (j - 1) % 3 and j % 3: the second slot follows the first, or the
// pair wraps (j % 3 == 0) and it lies two slots below it.
bool krylov_ring_wraps(int j) { return j >= 1 && j % int(kKrylovRing) == 0; }

// The byte model in units of one state (8 * 2^n bytes).  Pass one launches what the stored local route launches, on ring
// slots for basis rows: krylov_state_sweeps(m, 0).
double krylov_tridiagonal_sweeps(int m) { return krylov_state_sweeps(m, 0); }

// The replay, per group of sb outputs: the import 3; step 0 subtracts one row (3) and the scaled copy reads w and v_0 and
// writes v_1 and the outputs (3 + sb); every later step subtracts two rows (4) and the scaled copy reads w and the outputs
// and writes v_{j+1} and the outputs (2 + 2 sb).  m = 1: one import, and the combine kernel reads v_0 once per group and
// writes the outputs.
double krylov_replay_sweeps(int m, int S) {
  if (m == 1) return 3.0 + double((S + kKrylovBlock - 1) / kKrylovBlock) + double(S);
  double sweeps = 0.0;
  for (int s0 = 0; s0 < S; s0 += kKrylovBlock) {
    const int sb = std::min(kKrylovBlock, S - s0);
    sweeps += 3.0 + double(6 + sb) + double(m - 2) * double(6 + 2 * sb);
  }
  return sweeps;
}

// What both passes reserve: the workspace, the ring beside it and the scratch of the import and of the sums.
int reserve_krylov_stream(qhbm_engine* h, int U, uint32_t cs) {
  const uint32_t n = uint32_t(h->model.n), n_eff = uint32_t(h->fwd.plan.n_eff), n_ops = uint32_t(h->model.n_ops);
  if (int rc = ensure_state_buffers(h, cs, true)) return rc;
  HIPCHK(h->kry_ring.reserve((size_t(kKrylovRing) * cs) << n_eff, false));
  HIPCHK(h->import_norm2.reserve(size_t(U)));
  HIPCHK(h->import_parts.reserve(state_norm_parts_count(n, cs)));
  HIPCHK(h->evo_scale.reserve(cs));
  HIPCHK(h->evo_up1.reserve(size_t(cs) * n_ops));
  HIPCHK(h->kry_parts.reserve(krylov_coef_parts_count(n_eff, cs)));
  HIPCHK(h->kry_norm_parts.reserve(state_norm_parts_count(n_eff, cs)));
  return 0;
}

}  // namespace

extern "C" {

int qhbm_describe_krylov_stream(qhbm_engine* h, int U, int m, int S, char* buf, size_t buf_len) {
  if (!h || !buf || !buf_len) return 1;
  if (int rc = check_krylov_stream_shape(h, U, m, S)) return rc;
  DenseScope scope(h);
  if (int rc = build_plans(h)) return rc;
  const double state = double(size_t(8) << h->model.n);
  const uint32_t cs = krylov_stream_chunk_states(h, U);
  const int groups = (S + kKrylovBlock - 1) / kKrylovBlock;
  std::snprintf(buf, buf_len,
                "workspace_bytes=%.17g chunk_states=%u tridiagonal_applications=%d replay_applications=%d "
                "tridiagonal_bytes_per_state=%.17g replay_bytes_per_state=%.17g",
                double(kKrylovStreamBuffers) * double(cs) * double(state_bytes(h)), cs, m, (m - 1) * groups,
                krylov_tridiagonal_sweeps(m) * state, krylov_replay_sweeps(m, S) * state);
  return 0;
}

int qhbm_krylov_tridiagonal(qhbm_engine* h, const void* d_start_states, int U, const double* weights, int m, double* d_alpha,
                            double* d_beta, int32_t* d_lengths, void* d_recurrence, void* stream) {
  if (!h) return 1;
  if (int rc = need_device(h)) return rc;
  if (int rc = check_krylov_stream_shape(h, U, m, 1)) return rc;
  if (int rc = check_evolve_states(h, d_start_states, U, "d_start_states")) return rc;
  if (int rc = check_pointer(h, d_alpha, 8, "d_alpha")) return rc;
  if (int rc = check_pointer(h, d_beta, 8, "d_beta")) return rc;
  if (int rc = check_pointer(h, d_lengths, 4, "d_lengths")) return rc;
  if (int rc = check_pointer(h, d_recurrence, 8, "d_recurrence")) return rc;
  double R = 0.0;
  if (int rc = weighted_radius(h, weights, &R)) return rc;
  DenseScope scope(h);
  if (int rc = upload_model(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  consume_workspace(h);
  const uint32_t n = uint32_t(h->model.n), n_eff = uint32_t(h->fwd.plan.n_eff), n_ops = uint32_t(h->model.n_ops);
  const size_t row = size_t(8) << n;
  const uint32_t cs = krylov_stream_chunk_states(h, U);
  if (int rc = reserve_krylov_stream(h, U, cs)) return rc;
  if (aliases_workspace(h, d_start_states, size_t(U) * row)) return fail(h, "d_start_states lies inside the engine's workspace");
  if (int rc = upload_evolve_weights(h, weights, 1.0, s)) return rc;
  HIPCHK(launch_zero_fill(d_alpha, size_t(U) * size_t(m) * sizeof(double), s));
  HIPCHK(launch_zero_fill(d_recurrence, size_t(U) * size_t(m) * 2 * sizeof(float2), s));  // (the pair of step 0 is (0, c_0))
  const double threshold = std::ldexp(R, -16);
  const size_t slot = size_t(cs) << n_eff;  // amplitudes from one slot of the ring to the next
  float2* rec = static_cast<float2*>(d_recurrence);
  float2* W = h->lam.p;
  for (uint32_t s0 = 0; s0 < uint32_t(U); s0 += cs) {
    const uint32_t c = std::min<uint32_t>(cs, uint32_t(U) - s0);
    auto ring = [&](int j) { return h->kry_ring.p + size_t(j % int(kKrylovRing)) * slot; };
    // v_0 = phi / ||phi|| into slot 0 at the workspace's pitch (zeros for norm 0 and in the padding)
    hipEvent_t* iev = timer_begin(h, 0, s);
    HIPCHK(launch_import_states(static_cast<const float2*>(d_start_states), n, n_eff, c, s0, ring(0), h->import_parts.p,
                                h->import_norm2.p, s));
    timer_end(iev, s);
    HIPCHK(launch_krylov_init(c, h->import_norm2.p + s0, m, d_lengths + s0, h->evo_scale.p, s));
    HIPCHK(launch_evolve_init(c, nullptr, nullptr, nullptr, h->evo_wr.p, n_ops, h->evo_up1.p, nullptr, s));
    for (int j = 0; j < m; ++j) {
      // w = H v_j: the ring has the workspace's pitch, so the observable kernel reads the slot itself at every n
      if (int rc = run_observable_chunk(h, 0, c, h->evo_up1.p, false, s, true, false, ring(j), W)) return rc;
      hipEvent_t* ev = timer_begin(h, 0, s);
      // the step's pair in d_recurrence is the coefficient row of the project and subtract kernels: (c_{j-1}, c_j), (0, c_0)
      float2* pair = rec + (size_t(s0) * size_t(m) + size_t(j)) * 2;
      const uint32_t pair_pitch = 2 * uint32_t(m);
      double* alpha_j = d_alpha + size_t(s0) * size_t(m) + size_t(j);
      if (j == 0) {
        HIPCHK(launch_krylov_project(W, n_eff, ring(0), 0, n_eff, c, 1, h->kry_parts.p, pair, pair_pitch, 1, 0, alpha_j, uint64_t(m), s));
        HIPCHK(launch_krylov_subtract(W, n_eff, ring(0), 0, n_eff, c, 1, pair + 1, pair_pitch, h->kry_norm_parts.p, s));
      } else {
        // rows j - 1 and j in ONE launch of two rows, the launch of the stored route: where the pair wraps in the ring, row j
        // lies two slots BELOW row j - 1 and the stride is negative
        const int64_t stride = krylov_ring_wraps(j) ? -2 * int64_t(slot) : int64_t(slot);
        HIPCHK(launch_krylov_project(W, n_eff, ring(j - 1), stride, n_eff, c, 2, h->kry_parts.p, pair, pair_pitch, 0, 1, alpha_j,
                                     uint64_t(m), s));
        HIPCHK(launch_krylov_subtract(W, n_eff, ring(j - 1), stride, n_eff, c, 2, pair, pair_pitch, h->kry_norm_parts.p, s));
      }
      HIPCHK(launch_krylov_norm(h->kry_norm_parts.p, n_eff, c, threshold, j, d_beta + size_t(s0) * size_t(m), uint64_t(m),
                                d_lengths + s0, h->evo_scale.p, s));
      // v_{j+1} = w / beta_j over v_{j-2} (scale 0 after a breakdown: zeros)
      if (j + 1 < m) HIPCHK(launch_scale_copy_states(W, n_eff, ring(j + 1), n_eff, n, c, h->evo_scale.p, nullptr, s));
      timer_end(ev, s);
    }
  }
  return 0;
}

int qhbm_krylov_replay(qhbm_engine* h, const void* d_start_states, int U, const double* weights, int m, const double* d_beta,
                       const int32_t* d_lengths, const void* d_recurrence, const void* d_coef, int S, void* d_out_states,
                       void* stream) {
  if (!h) return 1;
  if (int rc = need_device(h)) return rc;
  if (int rc = check_krylov_stream_shape(h, U, m, S)) return rc;
  if (int rc = check_evolve_states(h, d_start_states, U, "d_start_states")) return rc;
  if (int rc = check_pointer(h, d_beta, 8, "d_beta")) return rc;
  if (int rc = check_pointer(h, d_lengths, 4, "d_lengths")) return rc;
  if (int rc = check_pointer(h, d_recurrence, 8, "d_recurrence")) return rc;
  if (int rc = check_pointer(h, d_coef, 8, "d_coef")) return rc;
  if (int rc = check_pointer(h, d_out_states, 16, "d_out_states")) return rc;
  const uint32_t n = uint32_t(h->model.n);
  const size_t amps = size_t(1) << n, row = amps * sizeof(float2), out_bytes = size_t(U) * size_t(S) * row;
  if (ranges_overlap(d_start_states, size_t(U) * row, d_out_states, out_bytes)) return fail(h, "d_out_states overlaps d_start_states");
  if (aliases_workspace(h, d_out_states, out_bytes)) return fail(h, "d_out_states lies inside the engine's workspace");
  if (weights)
    for (int k = 0; k < h->model.n_ops; ++k)
      if (!std::isfinite(weights[k])) return fail(h, "a weight is not finite");
  DenseScope scope(h);
  if (int rc = upload_model(h)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  consume_workspace(h);
  const uint32_t n_eff = uint32_t(h->fwd.plan.n_eff), n_ops = uint32_t(h->model.n_ops);
  const uint32_t cs = krylov_stream_chunk_states(h, U);
  if (int rc = reserve_krylov_stream(h, U, cs)) return rc;
  if (aliases_workspace(h, d_start_states, size_t(U) * row)) return fail(h, "d_start_states lies inside the engine's workspace");
  if (aliases_workspace(h, d_out_states, out_bytes)) return fail(h, "d_out_states lies inside the engine's workspace");
  if (int rc = upload_evolve_weights(h, weights, 1.0, s)) return rc;
  const size_t slot = size_t(cs) << n_eff;
  const float2* rec = static_cast<const float2*>(d_recurrence);
  const float2* coef = static_cast<const float2*>(d_coef);
  float2* out = static_cast<float2*>(d_out_states);
  float2* W = h->lam.p;
  for (uint32_t s0 = 0; s0 < uint32_t(U); s0 += cs) {
    const uint32_t c = std::min<uint32_t>(cs, uint32_t(U) - s0);
    HIPCHK(launch_evolve_init(c, nullptr, nullptr, nullptr, h->evo_wr.p, n_ops, h->evo_up1.p, nullptr, s));
    if (m == 1) {  // out = coef[., 0] v_0: the combine kernel over the one row, imported at the caller's pitch
      hipEvent_t* ev = timer_begin(h, 0, s);
      HIPCHK(launch_import_states(static_cast<const float2*>(d_start_states), n, n, c, s0, h->kry_ring.p, h->import_parts.p,
                                  h->import_norm2.p, s));
      HIPCHK(launch_krylov_combine(h->kry_ring.p, 1, c, n, coef + size_t(s0) * size_t(S), uint32_t(S),
                                   out + size_t(s0) * size_t(S) * amps, s));
      timer_end(ev, s);
      continue;
    }
    for (int g0 = 0; g0 < S; g0 += kKrylovBlock) {  // the recurrence runs once per group of eight outputs
      const uint32_t sb = uint32_t(std::min(kKrylovBlock, S - g0));
      float2 *cur = h->kry_ring.p, *nxt = h->kry_ring.p + slot;
      hipEvent_t* iev = timer_begin(h, 0, s);
      HIPCHK(launch_import_states(static_cast<const float2*>(d_start_states), n, n_eff, c, s0, cur, h->import_parts.p,
                                  h->import_norm2.p, s));
      timer_end(iev, s);
      for (int j = 0; j + 1 < m; ++j) {
        if (int rc = run_observable_chunk(h, 0, c, h->evo_up1.p, false, s, true, false, cur, W)) return rc;
        hipEvent_t* ev = timer_begin(h, 0, s);
        // w -= c_{j-1} v_{j-1} + c_j v_j by THE launch of pass one (the kernel instance decides the bits: DESIGN.md 6o), on
        // the recorded pair; nxt holds v_{j-1}, one slot above or below cur
        const float2* pair = rec + (size_t(s0) * size_t(m) + size_t(j)) * 2;
        if (j == 0)
          HIPCHK(launch_krylov_subtract(W, n_eff, cur, 0, n_eff, c, 1, pair + 1, 2 * uint32_t(m), h->kry_norm_parts.p, s));
        else
          HIPCHK(launch_krylov_subtract(W, n_eff, nxt, int64_t(cur - nxt), n_eff, c, 2, pair, 2 * uint32_t(m), h->kry_norm_parts.p, s));
        HIPCHK(launch_krylov_replay(uint32_t(j), W, cur, nxt, n, n_eff, c, d_beta + size_t(s0) * size_t(m) + size_t(j), uint64_t(m),
                                    coef + (size_t(s0) * size_t(S) + size_t(g0)) * size_t(m), uint32_t(m), uint32_t(S), sb,
                                    out + (size_t(s0) * size_t(S) + size_t(g0)) * amps, s));
        timer_end(ev, s);
        std::swap(cur, nxt);  // v_{j+1} replaced v_{j-1}
      }
    }
  }
  return 0;
}

// ---- the weighted Gram matrix of M states (include/qhbm_engine.h; gram.hip) ----
static int check_gram_shape(int M, int n_qubits) {
  if (M < 1 || M > kGramMaxStates) return fail(nullptr, "M must be in [1, " + std::to_string(kGramMaxStates) + "]");
  if (n_qubits < 1 || n_qubits > 31) return fail(nullptr, "n_qubits must be in [1, 31]");
  return 0;
}

int qhbm_gram_scratch_bytes(int M, int n_qubits, size_t* out) {
  if (!out) return fail(nullptr, "out is NULL");
  if (int rc = check_gram_shape(M, n_qubits)) return rc;
  *out = gram_parts_count(uint32_t(n_qubits), uint32_t(M)) * sizeof(double);
  return 0;
}

int qhbm_weighted_gram(const void* d_states, int M, int n_qubits, const float* d_table, void* d_scratch, double* d_gram,
                       void* stream) {
  if (int rc = check_gram_shape(M, n_qubits)) return rc;
  if (int rc = check_pointer(nullptr, d_states, 16, "d_states")) return rc;
  if (d_table)
    if (int rc = check_pointer(nullptr, d_table, 8, "d_table")) return rc;
  if (int rc = check_pointer(nullptr, d_scratch, 8, "d_scratch")) return rc;
  if (int rc = check_pointer(nullptr, d_gram, 8, "d_gram")) return rc;
  hipError_t e = launch_weighted_gram(static_cast<const float2*>(d_states), uint32_t(M), uint32_t(n_qubits), d_table,
                                      static_cast<double*>(d_scratch), d_gram, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_weighted_gram: ") + hipGetErrorString(e));
  return 0;
}

// ---- the cross-Gram matrix of two ensembles (include/qhbm_engine.h; cross_gram.hip) ----
static int check_cross_gram_shape(int M, int K, int n_qubits) {
  if (M < 1 || M > kGramMaxStates) return fail(nullptr, "M must be in [1, " + std::to_string(kGramMaxStates) + "]");
  if (K < 1 || K > kGramMaxStates) return fail(nullptr, "K must be in [1, " + std::to_string(kGramMaxStates) + "]");
  if (n_qubits < 1 || n_qubits > 31) return fail(nullptr, "n_qubits must be in [1, 31]");
  return 0;
}

int qhbm_cross_gram_scratch_bytes(int M, int K, int n_qubits, size_t* out) {
  if (!out) return fail(nullptr, "out is NULL");
  if (int rc = check_cross_gram_shape(M, K, n_qubits)) return rc;
  *out = cross_gram_parts_count(uint32_t(n_qubits), uint32_t(M), uint32_t(K)) * sizeof(double);
  return 0;
}

int qhbm_cross_gram(const void* d_bras, int M, const void* d_kets, int K, int n_qubits, const float* d_table, void* d_scratch,
                    double* d_out, void* stream) {
  if (int rc = check_cross_gram_shape(M, K, n_qubits)) return rc;
  if (int rc = check_pointer(nullptr, d_bras, 16, "d_bras")) return rc;
  if (int rc = check_pointer(nullptr, d_kets, 16, "d_kets")) return rc;
  if (d_table)
    if (int rc = check_pointer(nullptr, d_table, 8, "d_table")) return rc;
  if (int rc = check_pointer(nullptr, d_scratch, 8, "d_scratch")) return rc;
  if (int rc = check_pointer(nullptr, d_out, 8, "d_out")) return rc;
  hipError_t e = launch_cross_gram(static_cast<const float2*>(d_bras), uint32_t(M), static_cast<const float2*>(d_kets), uint32_t(K),
                                   uint32_t(n_qubits), d_table, static_cast<double*>(d_scratch), d_out,
                                   static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_cross_gram: ") + hipGetErrorString(e));
  return 0;
}

// ---- the VJP of the cross-Gram matrix (include/qhbm_engine.h; cross_gram_vjp.hip, cross_gram_vjp_plan.h) ----
int qhbm_cross_gram_vjp_scratch_bytes(int M, int K, int n_qubits, size_t* out) {
  if (!out) return fail(nullptr, "out is NULL");
  if (int rc = check_cross_gram_shape(M, K, n_qubits)) return rc;
  *out = cgv_plan(n_qubits, M, K).scratch_bytes;
  return 0;
}

int qhbm_cross_gram_vjp(const void* d_bras, int M, const void* d_kets, int K, int n_qubits, const float* d_table,
                        const void* d_cotangent, void* d_out_bras, void* d_out_kets, double* d_table_grad, void* d_scratch,
                        void* stream) {
  if (int rc = check_cross_gram_shape(M, K, n_qubits)) return rc;
  if (int rc = check_pointer(nullptr, d_bras, 16, "d_bras")) return rc;
  if (int rc = check_pointer(nullptr, d_kets, 16, "d_kets")) return rc;
  if (d_table)
    if (int rc = check_pointer(nullptr, d_table, 8, "d_table")) return rc;
  if (int rc = check_pointer(nullptr, d_cotangent, 8, "d_cotangent")) return rc;
  if (!d_out_bras && !d_out_kets && !d_table_grad)
    return fail(nullptr, "d_out_bras, d_out_kets and d_table_grad are all NULL: nothing to compute");
  if (d_out_bras)
    if (int rc = check_pointer(nullptr, d_out_bras, 16, "d_out_bras")) return rc;
  if (d_out_kets)
    if (int rc = check_pointer(nullptr, d_out_kets, 16, "d_out_kets")) return rc;
  if (d_table_grad)
    if (int rc = check_pointer(nullptr, d_table_grad, 8, "d_table_grad")) return rc;
  if (int rc = check_pointer(nullptr, d_scratch, 8, "d_scratch")) return rc;
  const size_t bra_bytes = size_t(M) * (size_t(8) << n_qubits), ket_bytes = size_t(K) * (size_t(8) << n_qubits);
  if (d_out_bras) {
    if (ranges_overlap(d_out_bras, bra_bytes, d_bras, bra_bytes)) return fail(nullptr, "d_out_bras overlaps d_bras");
    if (ranges_overlap(d_out_bras, bra_bytes, d_kets, ket_bytes)) return fail(nullptr, "d_out_bras overlaps d_kets");
  }
  if (d_out_kets) {
    if (ranges_overlap(d_out_kets, ket_bytes, d_bras, bra_bytes)) return fail(nullptr, "d_out_kets overlaps d_bras");
    if (ranges_overlap(d_out_kets, ket_bytes, d_kets, ket_bytes)) return fail(nullptr, "d_out_kets overlaps d_kets");
  }
  if (d_out_bras && d_out_kets && ranges_overlap(d_out_bras, bra_bytes, d_out_kets, ket_bytes))
    return fail(nullptr, "d_out_bras overlaps d_out_kets");
  hipError_t e = launch_cross_gram_vjp(static_cast<const float2*>(d_bras), uint32_t(M), static_cast<const float2*>(d_kets), uint32_t(K),
                                       uint32_t(n_qubits), d_table, static_cast<const float2*>(d_cotangent),
                                       static_cast<float2*>(d_out_bras), static_cast<float2*>(d_out_kets), d_table_grad, d_scratch,
                                       static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_cross_gram_vjp: ") + hipGetErrorString(e));
  return 0;
}

// ---- the reduced density matrix of M states (include/qhbm_engine.h; reduced.hip, rdm_index.h) ----
static int check_reduced_shape(int M, int n_qubits, uint64_t keep_mask) {
  if (M < 1 || M > kRdmMaxStates) return fail(nullptr, "M must be in [1, 65536]");
  switch (rdm_check(n_qubits, keep_mask)) {
    case 0: return 0;
    case 1: return fail(nullptr, "n_qubits must be in [1, 31]");
    case 2: return fail(nullptr, "keep_mask has a bit at or above n_qubits");
    default: return fail(nullptr, "keep_mask must keep between 1 and min(n_qubits, 10) qubits");
  }
}

int qhbm_reduced_density_scratch_bytes(int M, int n_qubits, uint64_t keep_mask, size_t* out) {
  if (!out) return fail(nullptr, "out is NULL");
  if (int rc = check_reduced_shape(M, n_qubits, keep_mask)) return rc;
  *out = rdm_plan(n_qubits, keep_mask, M).scratch_bytes;
  return 0;
}

int qhbm_reduced_density(const void* d_states, int M, int n_qubits, uint64_t keep_mask, const double* d_weights,
                         void* d_scratch, double* d_rho, void* stream) {
  if (int rc = check_reduced_shape(M, n_qubits, keep_mask)) return rc;
  if (int rc = check_pointer(nullptr, d_states, 16, "d_states")) return rc;
  if (d_weights)
    if (int rc = check_pointer(nullptr, d_weights, 8, "d_weights")) return rc;
  if (int rc = check_pointer(nullptr, d_scratch, 8, "d_scratch")) return rc;
  if (int rc = check_pointer(nullptr, d_rho, 8, "d_rho")) return rc;
  hipError_t e = launch_reduced_density(static_cast<const float2*>(d_states), uint32_t(M), uint32_t(n_qubits), keep_mask,
                                        d_weights, static_cast<double*>(d_scratch), d_rho, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_reduced_density: ") + hipGetErrorString(e));
  return 0;
}

// ---- a dense operator on k qubits of M states (include/qhbm_engine.h; subsystem_apply.hip, subsystem_plan.h) ----
int qhbm_subsystem_apply_scratch_bytes(int M, int n_qubits, uint64_t keep_mask, size_t* out) {
  if (!out) return fail(nullptr, "out is NULL");
  if (int rc = check_reduced_shape(M, n_qubits, keep_mask)) return rc;
  *out = sub_plan(n_qubits, keep_mask, M).scratch_bytes;
  return 0;
}

int qhbm_subsystem_apply(const void* d_states, int M, int n_qubits, uint64_t keep_mask, const void* d_operator,
                         const double* d_scale, void* d_out, double* d_dots, void* d_scratch, void* stream) {
  if (int rc = check_reduced_shape(M, n_qubits, keep_mask)) return rc;
  if (int rc = check_pointer(nullptr, d_states, 16, "d_states")) return rc;
  if (int rc = check_pointer(nullptr, d_operator, 8, "d_operator")) return rc;
  if (d_scale)
    if (int rc = check_pointer(nullptr, d_scale, 8, "d_scale")) return rc;
  if (int rc = check_pointer(nullptr, d_out, 16, "d_out")) return rc;
  if (d_dots)
    if (int rc = check_pointer(nullptr, d_dots, 8, "d_dots")) return rc;
  if (int rc = check_pointer(nullptr, d_scratch, 8, "d_scratch")) return rc;
  const size_t bytes = size_t(M) * (size_t(8) << n_qubits);
  if (ranges_overlap(d_out, bytes, d_states, bytes)) return fail(nullptr, "d_out overlaps d_states");
  hipError_t e = launch_subsystem_apply(static_cast<const float2*>(d_states), uint32_t(M), uint32_t(n_qubits), keep_mask,
                                        static_cast<const float2*>(d_operator), d_scale, static_cast<float2*>(d_out), d_dots,
                                        d_scratch, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_subsystem_apply: ") + hipGetErrorString(e));
  return 0;
}

// ---- the VJP of the weighted Gram matrix (include/qhbm_engine.h; gram_vjp.hip, gram_vjp_plan.h) ----
int qhbm_gram_vjp_scratch_bytes(int M, int n_qubits, size_t* out) {
  if (!out) return fail(nullptr, "out is NULL");
  if (int rc = check_gram_shape(M, n_qubits)) return rc;
  *out = gv_plan(n_qubits, M).scratch_bytes;
  return 0;
}

int qhbm_weighted_gram_vjp(const void* d_states, int M, int n_qubits, const float* d_table, const void* d_cotangent,
                           void* d_out_states, double* d_table_grad, void* d_scratch, void* stream) {
  if (int rc = check_gram_shape(M, n_qubits)) return rc;
  if (int rc = check_pointer(nullptr, d_states, 16, "d_states")) return rc;
  if (d_table)
    if (int rc = check_pointer(nullptr, d_table, 8, "d_table")) return rc;
  if (int rc = check_pointer(nullptr, d_cotangent, 8, "d_cotangent")) return rc;
  if (!d_out_states && !d_table_grad) return fail(nullptr, "d_out_states and d_table_grad are both NULL: nothing to compute");
  if (d_out_states)
    if (int rc = check_pointer(nullptr, d_out_states, 16, "d_out_states")) return rc;
  if (d_table_grad)
    if (int rc = check_pointer(nullptr, d_table_grad, 8, "d_table_grad")) return rc;
  if (int rc = check_pointer(nullptr, d_scratch, 8, "d_scratch")) return rc;
  const size_t bytes = size_t(M) * (size_t(8) << n_qubits);
  if (d_out_states && ranges_overlap(d_out_states, bytes, d_states, bytes)) return fail(nullptr, "d_out_states overlaps d_states");
  hipError_t e = launch_gram_vjp(static_cast<const float2*>(d_states), uint32_t(M), uint32_t(n_qubits), d_table,
                                 static_cast<const float2*>(d_cotangent), static_cast<float2*>(d_out_states), d_table_grad,
                                 d_scratch, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_weighted_gram_vjp: ") + hipGetErrorString(e));
  return 0;
}

int qhbm_random_states(void* d_states, int U, int n_qubits, uint64_t seed, uint64_t first_state, void* stream) {
  if (U < 0) return fail(nullptr, "negative batch size");
  if (n_qubits < 1 || n_qubits > 34) return fail(nullptr, "n_qubits must be in [1, 34]");
  if (U == 0) return 0;
  if (int rc = check_pointer(nullptr, d_states, 16, "d_states")) return rc;
  if (first_state + uint64_t(U) > (uint64_t(1) << 32)) return fail(nullptr, "first_state + U exceeds 2^32");
  hipError_t e = launch_random_states(static_cast<float2*>(d_states), uint32_t(U), uint32_t(n_qubits), seed, uint32_t(first_state),
                                      static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_random_states: ") + hipGetErrorString(e));
  return 0;
}

int qhbm_table_expectation(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, const float* d_table,
                           float* d_out, void* stream) {
  return table_forward(h, d_bits, U, d_params, d_table, d_out, false, stream);
}

int qhbm_table_expectation_retain(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, const float* d_table,
                                  float* d_out, void* stream) {
  return table_forward(h, d_bits, U, d_params, d_table, d_out, true, stream);
}

int qhbm_table_expectation_vjp(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, const float* d_table,
                               const float* d_upstream, float* d_out_vals, float* d_grad, float* d_table_grad,
                               void* stream) {
  if (int rc = begin_call(h, U, kNeedTable, d_table)) return rc;
  if (!d_grad || (U > 0 && !d_upstream)) return fail(h, "d_grad / d_upstream is NULL");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (U == 0) {
    h->retained_U = 0;
    if (int rc = empty_batch_grad(h, d_grad, s)) return rc;
    if (d_table_grad) HIPCHK(launch_zero_fill(d_table_grad, (size_t(1) << h->model.n) * sizeof(float), s));
    return 0;
  }
  return table_vjp(h, d_bits, U, d_params, d_table, d_upstream, d_out_vals, d_grad, d_table_grad, false, s);
}

int qhbm_table_expectation_vjp_retained(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                                        const float* d_table, const float* d_upstream, float* d_grad,
                                        float* d_table_grad, void* stream) {
  if (int rc = begin_call(h, U, kNeedTable, d_table)) return rc;
  if (U <= 0 || h->retained_U != U || !h->retained_table)
    return fail(h, "no retained energy-table forward state for this batch");
  if (!d_grad || !d_upstream) return fail(h, "d_grad / d_upstream is NULL");
  return table_vjp(h, d_bits, U, d_params, d_table, d_upstream, nullptr, d_grad, d_table_grad, true,
                   static_cast<hipStream_t>(stream));
}

int qhbm_parity_energy(const int8_t* d_bits, int64_t n_rows, int n_bits, const uint64_t* d_masks,
                       const float* d_thetas, int n_terms, float* d_energy, void* stream) {
  if (n_rows < 0 || n_terms < 0) return fail(nullptr, "negative size");
  if (n_bits < 1 || n_bits > 64) return fail(nullptr, "n_bits must be in [1, 64]");
  hipError_t e = launch_parity_energy(d_bits, n_rows, n_bits, d_masks, d_thetas, n_terms, d_energy,
                                      static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_parity_energy: ") + hipGetErrorString(e));
  return 0;
}

int qhbm_parity_energy_vjp(const int8_t* d_bits, int64_t n_rows, int n_bits, const uint64_t* d_masks,
                           int n_terms, const float* d_weights, float* d_grad, void* stream) {
  if (n_rows < 0 || n_terms < 0) return fail(nullptr, "negative size");
  if (n_bits < 1 || n_bits > 64) return fail(nullptr, "n_bits must be in [1, 64]");
  hipError_t e = launch_parity_energy_vjp(d_bits, n_rows, n_bits, d_masks, n_terms, d_weights, d_grad,
                                          static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_parity_energy_vjp: ") + hipGetErrorString(e));
  return 0;
}

int qhbm_gwg_sample(uint64_t* d_chain_states, int n_chains, int n_bits, const uint64_t* d_masks, const float* d_thetas,
                    int n_terms, uint64_t seed, uint64_t step0, int64_t n_steps, int8_t* d_out_samples,
                    int32_t* d_out_accepted, void* stream) {
  if (n_chains < 0 || n_terms < 0 || n_steps < 0) return fail(nullptr, "qhbm_gwg_sample: negative size");
  if (n_bits < 1 || n_bits > 64) return fail(nullptr, "qhbm_gwg_sample: n_bits must be in [1, 64]");
  if (n_chains > 0 && !d_chain_states) return fail(nullptr, "qhbm_gwg_sample: d_chain_states is NULL");
  if (n_terms > 0 && (!d_masks || !d_thetas)) return fail(nullptr, "qhbm_gwg_sample: d_masks / d_thetas is NULL");
  if (gwg_lds_bytes(n_bits, n_terms) > kGwgLdsMax)
    return fail(nullptr, "qhbm_gwg_sample: " + std::to_string(n_terms) + " terms over " + std::to_string(n_bits) +
                             " bits need " + std::to_string(gwg_lds_bytes(n_bits, n_terms)) + " bytes of LDS, " +
                             std::to_string(kGwgLdsMax) + " fit");
  hipError_t e = launch_gwg_sample(d_chain_states, n_chains, n_bits, d_masks, d_thetas, n_terms, seed, step0, n_steps,
                                   d_out_samples, d_out_accepted, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_gwg_sample: ") + hipGetErrorString(e));
  return 0;
}

int qhbm_walsh_hadamard(float* d_data, int n_bits, void* stream) {
  if (n_bits < 1 || n_bits > 30) return fail(nullptr, "qhbm_walsh_hadamard: n_bits must be in [1, 30]");
  if (!d_data) return fail(nullptr, "qhbm_walsh_hadamard: d_data is NULL");
  hipError_t e = launch_walsh_hadamard(d_data, d_data, n_bits, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_walsh_hadamard: ") + hipGetErrorString(e));
  return 0;
}

int qhbm_parity_table(const uint64_t* d_masks, const float* d_thetas, int n_terms, int n_bits, float* d_table,
                      void* stream) {
  if (n_terms < 0) return fail(nullptr, "qhbm_parity_table: negative size");
  if (n_bits < 1 || n_bits > 30) return fail(nullptr, "qhbm_parity_table: n_bits must be in [1, 30]");
  if (!d_table) return fail(nullptr, "qhbm_parity_table: d_table is NULL");
  if (n_terms > 0 && (!d_masks || !d_thetas)) return fail(nullptr, "qhbm_parity_table: d_masks / d_thetas is NULL");
  hipError_t e = launch_parity_table(d_masks, d_thetas, n_terms, n_bits, d_table, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_parity_table: ") + hipGetErrorString(e));
  return 0;
}

int qhbm_parity_table_vjp(const uint64_t* d_masks, int n_terms, int n_bits, const float* d_weights, float* d_scratch,
                          float* d_grad, void* stream) {
  if (n_terms < 0) return fail(nullptr, "qhbm_parity_table_vjp: negative size");
  if (n_bits < 1 || n_bits > 30) return fail(nullptr, "qhbm_parity_table_vjp: n_bits must be in [1, 30]");
  if (!d_weights || !d_scratch) return fail(nullptr, "qhbm_parity_table_vjp: d_weights / d_scratch is NULL");
  if (d_weights == d_scratch) return fail(nullptr, "qhbm_parity_table_vjp: d_scratch must not be d_weights");
  if (n_terms > 0 && (!d_masks || !d_grad)) return fail(nullptr, "qhbm_parity_table_vjp: d_masks / d_grad is NULL");
  hipError_t e = launch_parity_table_vjp(d_masks, n_terms, n_bits, d_weights, d_scratch, d_grad,
                                         static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_parity_table_vjp: ") + hipGetErrorString(e));
  return 0;
}

int qhbm_sample(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, int n_shots,
                uint64_t seed, int shift_gate, double shift, int8_t* d_out_samples, void* stream) {
  if (!h) return 1;
  if (int rc = need_device(h)) return rc;
  if (U < 0 || n_shots < 0) return fail(h, "negative batch size or shot count");
  if (shift_gate >= int(h->model.gates.size())) return fail(h, "shift_gate out of range");
  if (shift_gate < 0) shift_gate = -1;  // any negative value = the unshifted circuit (never the sentinel of a lowered fixed op)
  else if (shift != 0.0 && h->model.gates[size_t(shift_gate)].param_idx < 0)
    return fail(h, "shift_gate addresses a gate with a constant exponent: only parametrised gates have shifted programs "
                   "(tfq ParameterShift.get_gradient_circuits shifts symbols), and a lowered constant gate cannot be shifted");
  if (int rc = upload_model(h)) return rc;
  if (U == 0 || n_shots == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t n_eff = uint32_t(h->fwd.plan.n_eff);
  Sweep sw{d_bits, U, d_params, Chunks::kShots, shift_gate, shift};
  sw.keep_state = sw.values = true;  // (measurement by-products land in the fixed-point scratch)
  return run_sweep(
      h, sw, s, [&](uint32_t cs) -> int { HIPCHK(h->block_cum.reserve(size_t(cs) << (n_eff - 10))); return 0; },
      [&](uint32_t s0, uint32_t c) -> int {
        // shots are drawn in slices of <= 65535 (grid.x); the shot index feeds the counter RNG
        HIPCHK(launch_sample(h->psi.p, n_eff, h->model.n, c, h->block_cum.p, uint32_t(n_shots), seed, s0, d_out_samples, s));
        return 0;
      });
}

int qhbm_sample_counts(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, int n_programs,
                       const int32_t* shift_gates, const float* shifts, int n_shots, uint64_t seed,
                       int32_t* d_out_counts, void* stream) {
  if (!h) return 1;
  if (int rc = need_device(h)) return rc;
  if (U < 0 || n_shots < 0 || n_programs < 0) return fail(h, "negative batch size, program or shot count");
  if (n_programs && (!shift_gates || !shifts)) return fail(h, "shift_gates / shifts are NULL");
  if (h->model.n > 24) return fail(h, "qhbm_sample_counts keeps 2^n counters per (program, state): n_qubits <= 24; use qhbm_sample");
  if (int rc = check_shifted_programs(h, n_programs, shift_gates, shifts, false)) return rc;
  if (int rc = upload_model(h)) return rc;
  if (U == 0 || n_programs == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DevicePlan& d = h->fwd;
  consume_workspace(h);
  // every program from pass 0, in the caller's order (no prefix sharing here)
  const uint32_t n_prog = uint32_t(n_programs), n_eff = uint32_t(d.plan.n_eff);
  const ProgramOrder order = order_programs(d.plan, h->model.gates.size(), shift_gates, n_prog, false, true);
  if (int rc = upload_shift_tables(h, order, shift_gates, shifts, s)) return rc;
  const LaunchSets g = launch_set_geometry(h, U, n_prog, order, 1, true, false);
  if (int rc = ensure_state_buffers(h, g.Uc * g.Pc, false)) return rc;
  HIPCHK(h->block_cum.reserve((size_t(g.Uc) * g.Pc) << (n_eff - 10)));
  if (int rc = values_begin(h, int(g.Uc * g.Pc), s)) return rc;  // measurement by-products land in the fixed-point scratch
  if (int rc = grow_coef_batch(h, g, s)) return rc;
  if (n_eff > uint32_t(kMinTileBits))
    HIPCHK(launch_zero_fill(d_out_counts, ((size_t(n_prog) * size_t(U)) << h->model.n) * sizeof(int32_t), s));
  return for_each_chunk(U, g.Uc, [&](uint32_t s0, uint32_t c) -> int {
    auto draw = [&](uint32_t q0, uint32_t nq) -> int {
      HIPCHK(launch_sample_counts(h->psi.p, n_eff, h->model.n, nq * c, c, q0, h->block_cum.p, uint32_t(n_shots), seed, s0,
                                  uint32_t(U), d_out_counts, s));
      return 0;
    };
    return run_program_groups(h, d_bits, d_params, g, order, 0u, n_prog, s0, c, nullptr, {true, true, false}, s, draw);
  });
}

int qhbm_sample_parities(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, int n_programs,
                         const int32_t* shift_gates, const float* shifts, const uint64_t* masks, int T, int64_t n_shots,
                         uint64_t seed, int32_t* d_out, void* stream) {
  if (!h) return 1;
  if (U < 0 || n_programs < 0) return fail(h, "negative batch size or program count");
  if (n_programs && (!shift_gates || !shifts)) return fail(h, "shift_gates / shifts are NULL");
  if (h->model.n < 1 || h->model.n > 31) return fail(h, "qhbm_sample_parities needs a circuit of 1 .. 31 qubits (qhbm_set_circuit)");
  std::vector<uint32_t> idx_masks;
  if (int rc = check_parity_masks(h, h->model.n, masks, T, n_shots, &idx_masks)) return rc;
  if (int rc = check_shifted_programs(h, n_programs, shift_gates, shifts, false)) return rc;
  if (U && n_programs && !d_out) return fail(h, "d_out is NULL");
  if (int rc = need_device(h)) return rc;
  if (int rc = upload_model(h)) return rc;
  if (U == 0 || n_programs == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  DevicePlan& d = h->fwd;
  consume_workspace(h);
  const uint32_t n_prog = uint32_t(n_programs), n_eff = uint32_t(d.plan.n_eff);
  HIPCHK(launch_zero_fill(d_out, size_t(n_prog) * size_t(U) * size_t(T) * sizeof(int32_t), s));
  if (n_shots == 0) return 0;
  // every program from pass 0, in the caller's order, as in qhbm_sample_counts
  const ProgramOrder order = order_programs(d.plan, h->model.gates.size(), shift_gates, n_prog, false, true);
  if (int rc = upload_shift_tables(h, order, shift_gates, shifts, s)) return rc;
  LaunchSets g = launch_set_geometry(h, U, n_prog, order, 1, true, false);
  {  // the prefix tables of an element count against the workspace budget beside its state
    const size_t per_element = state_bytes(h) + shot_parity_table_doubles(n_eff, 1) * sizeof(double);
    const size_t cap = std::max<size_t>(1, budget_bytes(h) / per_element);
    if (size_t(g.Uc) * g.Pc > cap) {
      g.Uc = uint32_t(std::min<size_t>(g.Uc, cap));
      g.Pc = uint32_t(std::max<size_t>(1, cap / g.Uc));
    }
  }
  if (int rc = ensure_state_buffers(h, g.Uc * g.Pc, false)) return rc;
  HIPCHK(h->par_tables.reserve(shot_parity_table_doubles(n_eff, size_t(g.Uc) * g.Pc)));
  HIPCHK(h->par_masks.reserve(size_t(kParityMaxMasks)));
  if (int rc = values_begin(h, int(g.Uc * g.Pc), s)) return rc;  // measurement by-products land in the fixed-point scratch
  if (int rc = grow_coef_batch(h, g, s)) return rc;
  HIPCHK(launch_shot_parity_masks(idx_masks.data(), uint32_t(T), h->par_masks.p, s));
  return for_each_chunk(U, g.Uc, [&](uint32_t s0, uint32_t c) -> int {
    auto draw = [&](uint32_t q0, uint32_t nq) -> int {
      HIPCHK(launch_shot_parities(h->psi.p, n_eff, h->model.n, nq * c, c, q0, h->par_tables.p, h->par_masks.p, uint32_t(T),
                                  uint32_t(n_shots), seed, s0, uint32_t(U), 0u, 0u, d_out, s));
      return 0;
    };
    return run_program_groups(h, d_bits, d_params, g, order, 0u, n_prog, s0, c, nullptr, {true, true, false}, s, draw);
  });
}

int qhbm_sample_parities_scratch_bytes(int M, int n_qubits, int64_t n_shots, size_t* out) {
  if (!out) return fail(nullptr, "out is NULL");
  if (int rc = check_parity_states_shape(M, n_qubits)) return rc;
  if (n_shots < 0) return fail(nullptr, "negative shot count");
  if (n_shots > kParityMaxShots) return fail(nullptr, "too many shots: n_shots <= 2^31 - 1");
  *out = kParityMaskBytes + shot_parity_table_doubles(uint32_t(n_qubits), size_t(std::min(M, 65535))) * sizeof(double);
  return 0;
}

int qhbm_sample_parities_states(const void* d_states, int M, int n_qubits, const uint64_t* masks, int T, int64_t n_shots,
                                uint64_t seed, uint64_t first_row, uint32_t program, void* d_scratch, int32_t* d_out,
                                void* stream) {
  if (int rc = check_parity_states_shape(M, n_qubits)) return rc;
  std::vector<uint32_t> idx_masks;
  if (int rc = check_parity_masks(nullptr, n_qubits, masks, T, n_shots, &idx_masks)) return rc;
  if (first_row + uint64_t(M) > (uint64_t(1) << 32)) return fail(nullptr, "first_row + M exceeds 2^32");
  if (int rc = check_pointer(nullptr, d_states, 16, "d_states")) return rc;
  if (int rc = check_pointer(nullptr, d_scratch, 8, "d_scratch")) return rc;
  if (int rc = check_pointer(nullptr, d_out, 4, "d_out")) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const uint32_t n = uint32_t(n_qubits);
  hipError_t e = launch_zero_fill(d_out, size_t(M) * size_t(T) * sizeof(int32_t), s);
  uint32_t* d_masks = static_cast<uint32_t*>(d_scratch);
  double* tables = reinterpret_cast<double*>(static_cast<char*>(d_scratch) + kParityMaskBytes);
  if (e == hipSuccess && n_shots > 0) e = launch_shot_parity_masks(idx_masks.data(), uint32_t(T), d_masks, s);
  // states in slices of 65535 (grid.y); the slices run in stream order and share the tables
  for (uint32_t m0 = 0; e == hipSuccess && n_shots > 0 && m0 < uint32_t(M); m0 += 65535u) {
    const uint32_t c = std::min<uint32_t>(65535u, uint32_t(M) - m0);
    e = launch_shot_parities(static_cast<const float2*>(d_states) + (size_t(m0) << n), n, n_qubits, c, c, 0u, tables, d_masks,
                             uint32_t(T), uint32_t(n_shots), seed, m0, uint32_t(M), uint32_t(first_row), program, d_out, s);
  }
  if (e != hipSuccess) return fail(nullptr, std::string("qhbm_sample_parities_states: ") + hipGetErrorString(e));
  return 0;
}

int qhbm_expectation_vjp(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                         const float* d_upstream, float* d_out_vals, float* d_grad, int method,
                         void* stream) {
  if (int rc = begin_call(h, U, kNeedObservables)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int P = h->model.n_params;
  if (U == 0) return empty_batch_grad(h, d_grad, s);
  if (int rc = values_or_scratch(h, U, &d_out_vals)) return rc;
  if (method == QHBM_GRAD_ADJOINT) {
    if (int rc = adjoint_sweep(h, d_bits, U, d_params, d_upstream, d_out_vals, s)) return rc;
    return reduce_state_grad(h, U, d_grad, false, true, s);
  }
  if (method != QHBM_GRAD_PARAMETER_SHIFT) return fail(h, "unknown gradient method");
  // tfq ParameterShift / baselines/train.py:190-240: exponent c*s -> shift the gate's exponent by
  // +-1/2, weight +-pi*c/2, one pair of forwards per gate occurrence.  The (state, shifted program)
  // pairs are the batch: as many programs as the workspace holds run in ONE launch set, each on
  // its own copy of the coefficient buffer (PassArgs::prog_states).
  if (int rc = forward(h, d_bits, U, d_params, d_out_vals, -1, 0.0, s)) return rc;
  DevicePlan& d = h->fwd;
  const bool from_obs = forward_values_from_observable(h);
  if (!h->shift_ready || h->shift_tables_from_obs != from_obs) {  // shift tables: once per model
    h->shift_tables_from_obs = from_obs;
    std::vector<int> sg, sp;
    std::vector<float> sv, sw;
    for (size_t g = 0; g < h->model.gates.size(); ++g) {
      const Gate& G = h->model.gates[g];
      if (G.param_idx < 0 || G.kind == QHBM_GATE_I || h->model.frozen(G.param_idx)) continue;
      if (G.kind == QHBM_GATE_ISWAPPOW)
        return fail(h, kNoTwoTermRule);
      sg.push_back(int(g)); sg.push_back(int(g));
      sv.push_back(0.5f); sv.push_back(-0.5f);
      sp.push_back(G.param_idx);
      sw.push_back(float(1.5707963267948966 * double(G.scalar)));
    }
    // The sums of program q land at prog_acc[dst[q]], i.e. in GATE order whatever the execution order: the combination per
    // parameter adds in the order it always did.
    h->shift_order = order_programs(d.plan, h->model.gates.size(), sg.data(), sg.size(), h->opt_shift_prefix != 0, from_obs);
    if (int rc = upload_shift_tables(h, h->shift_order, sg.data(), sv.data(), s)) return rc;
    HIPCHK(h->shift_param.upload(sp));
    HIPCHK(h->shift_weight.upload(sw));
    h->shift_programs = uint32_t(sg.size());
    h->shift_gate_count = uint32_t(sp.size());
    h->shift_ready = true;
  }
  const uint32_t n_prog = h->shift_programs, n_shift_gates = h->shift_gate_count;
  if (n_prog == 0) return empty_batch_grad(h, d_grad, s);
  const LaunchSets g = launch_set_geometry(h, U, n_prog, h->shift_order, 1, false, true);
  if (int rc = ensure_state_buffers(h, g.Uc * g.Pc, false)) return rc;
  if (g.share) HIPCHK(h->lam.reserve(size_t(g.Uc) << d.plan.n_eff, false));   // the base states live where lambda would
  const uint32_t T = uint32_t(h->model.n_ops);
  const size_t nvb = size_t(g.Uc) * g.Pc * T;
  HIPCHK(h->vals64.reserve(nvb));
  HIPCHK(h->vals_batch.reserve(nvb));
  HIPCHK(h->prog_acc.reserve(n_prog));
  HIPCHK(launch_zero_fill(h->prog_acc.p, size_t(n_prog) * sizeof(double), s));
  if (int rc = grow_coef_batch(h, g, s)) return rc;
  consume_workspace(h);
  // The values of a shifted program come the way a forward-only call takes them: where that is the observable kernel
  // (wide terms: lean passes, then one sweep over the final states, the lower block of every pair only), the
  // shifted programs do the same -- config 4's 480 masks cost 51 measurement passes per program otherwise.  The base
  // program's coefficients are those the forward call above prepared.
  if (int rc = for_each_chunk(U, g.Uc, [&](uint32_t s0, uint32_t c) -> int {
    auto accumulate = [&](uint32_t q0, uint32_t nq) -> int {
      if (from_obs)
        if (int rc = run_values_chunk(h, 0u, nq * c, s)) return rc;
      HIPCHK(launch_values_from_fixed(h->vals64.p, h->op_inv_scale.p, h->vals_batch.p, nq * c * T, T, s));
      HIPCHK(launch_shift_program_accumulate(h->vals_batch.p, d_upstream, nq, c, T, s0, h->prog_acc.p, s, h->shift_dst.p + q0));
      return 0;
    };
    return run_program_groups(h, d_bits, d_params, g, h->shift_order, 0u, n_prog, s0, c, h->lam.p, {from_obs, from_obs, true}, s,
                              accumulate);
  }))
    return rc;
  HIPCHK(launch_shift_combine(h->prog_acc.p, h->shift_param.p, h->shift_weight.p, int(n_shift_gates), d_grad, P, s));
  return 0;
}

// One adjoint VJP per parameter-shifted program (the information matrix of a QHBM: every shifted occurrence of the
// first half of circuit + inverse, gradient taken over the second half).  The (program, state) pairs are the ELEMENTS
// of a launch set, as in the parameter-shift VJP: the forward passes run on per-program coefficient copies
// (PassArgs::prog_states), sharing the base program's prefix; lambda = O psi and the backward sweep then run over the
// same elements.  The observable and adjoint kernels index their per-state rows by element, so they read per-element
// copies of the bitstrings and the upstream (launch_replicate_rows) -- no kernel of the default path learns a new map.
// The backward sweep runs on the shared, unshifted coefficients: gates in front of the first live gate (circuit order)
// are never un-applied into a gradient.  A program whose shifted gate lies at or behind that gate gets the backward
// sweep of its own coefficients, one sweep per such program.
int qhbm_program_vjps(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, int n_programs,
                      const int32_t* shift_gates, const float* shifts, const float* d_upstream,
                      const float* d_row_weights, float* d_prog_vals, float* d_prog_grad, void* stream) {
  if (!h) return 1;
  if (n_programs < 0) return fail(h, "n_programs must be >= 0");
  if (n_programs && (!shift_gates || !shifts)) return fail(h, "shift_gates / shifts are NULL");
  if (int rc = begin_call(h, U, kNeedObservables)) return rc;
  const int n_gates = int(h->model.gates.size());
  if (int rc = check_shifted_programs(h, n_programs, shift_gates, shifts, true)) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int P = h->model.n_params;
  const uint32_t T = uint32_t(h->model.n_ops), n_prog = uint32_t(n_programs);
  if (n_prog == 0) return 0;
  if (P) HIPCHK(launch_zero_fill(d_prog_grad, size_t(n_prog) * size_t(P) * sizeof(float), s));
  if (U == 0) {
    if (d_prog_vals) HIPCHK(launch_zero_fill(d_prog_vals, size_t(n_prog) * T * sizeof(float), s));
    return 0;
  }
  DevicePlan& d = h->fwd;
  DevicePlan& b = h->adj;
  consume_workspace(h);
  const uint32_t n_slots = uint32_t(b.plan.slot_gate.size()), ns1 = grad_slots(h);
  // values and lambda exactly as the adjoint VJP (adjoint_sweep) takes them: an unshifted program is its d_grad bit for bit
  const bool vm = value_mode(h), mv = multi_value_mode(h), gm = mv && gather_multi_mode(h), skip = vm || mv;
  const ProgramOrder order = order_programs(d.plan, size_t(n_gates), shift_gates, n_prog, h->opt_shift_prefix != 0, skip);
  int first_live = n_gates;  // the backward sweep un-applies gates behind this one only
  for (int g = 0; g < n_gates; ++g) {
    const Gate& G = h->model.gates[size_t(g)];
    if (G.param_idx >= 0 && !h->model.frozen(G.param_idx)) { first_live = g; break; }
  }
  std::vector<int> sg(n_prog);  // (execution order, as the device tables)
  std::vector<float> sv(n_prog);
  std::vector<char> swept(n_prog);
  for (uint32_t q = 0; q < n_prog; ++q) {
    sg[q] = shift_gates[order.dst[q]];
    sv[q] = shifts[order.dst[q]];
    swept[q] = sg[q] >= first_live && sv[q] != 0.f;
  }
  if (int rc = upload_shift_tables(h, order, shift_gates, shifts, s)) return rc;
  // every element with psi and lambda; the base program's states of a shared prefix in a buffer of their own
  const LaunchSets g = launch_set_geometry(h, U, n_prog, order, 2, true, false);
  const uint32_t Uc = g.Uc, Pc = g.Pc;
  // gradient rows of the programs in flight: [R, U, n_slots] (a quarter of the budget, at least one program)
  const size_t row_bytes = size_t(U) * ns1 * sizeof(float);
  const uint32_t R = uint32_t(std::max<size_t>(1, std::min<size_t>(std::min<size_t>(n_prog, 65535), budget_bytes(h) / 4 / row_bytes)));
  const uint32_t n_eff = uint32_t(d.plan.n_eff), n = uint32_t(h->model.n);
  const size_t ne_max = size_t(Uc) * Pc;
  if (int rc = ensure_state_buffers(h, uint32_t(ne_max), true)) return rc;
  if (g.share) HIPCHK(h->pv_base.reserve(size_t(Uc) << n_eff, false));
  HIPCHK(h->pv_bits.reserve(ne_max * n));
  HIPCHK(h->pv_upstream.reserve(ne_max * T));
  HIPCHK(h->vals64.reserve(ne_max * T));
  HIPCHK(h->vals_batch.reserve(ne_max * T));
  HIPCHK(reserve_state_grad(h, ne_max));
  HIPCHK(h->pv_rows.reserve(size_t(R) * U * ns1, false));
  HIPCHK(h->pv_vals.reserve(size_t(n_prog) * T));
  HIPCHK(launch_zero_fill(h->pv_vals.p, size_t(n_prog) * T * sizeof(double), s));
  // coefficients: the base program's (forward) and the shared backward ones
  if (int rc = prepare_coefs(h, d, d_params, -1, 0.0, s)) return rc;
  auto prep_adjoint = [&](int gate, double shift) { return prepare_coefs(h, b, d_params, gate, shift, s); };
  if (int rc = prep_adjoint(-1, 0.0)) return rc;
  bool adjoint_shifted = false;
  if (int rc = grow_coef_batch(h, g, s)) return rc;
  for (uint32_t qa = 0; qa < n_prog; qa += R) {
    const uint32_t qb = std::min<uint32_t>(n_prog, qa + R);
    for (uint32_t s0 = 0; s0 < uint32_t(U); s0 += Uc) {
      const uint32_t c = std::min<uint32_t>(Uc, uint32_t(U) - s0);
      HIPCHK(launch_replicate_rows(d_bits, h->pv_bits.p, n, c, s0, Pc * c, s));
      HIPCHK(launch_replicate_rows(d_upstream, h->pv_upstream.p, T * uint32_t(sizeof(float)), c, s0, Pc * c, s));
      // the caller's own work on a launch set: lambda = O psi, the backward sweeps, rows and values of its programs
      auto backward = [&](uint32_t q0, uint32_t nq) -> int {
        const uint32_t ne = nq * c;
        if (mv && !gm)
          if (int rc = run_values_chunk(h, 0u, ne, s)) return rc;
        HIPCHK(begin_state_grad(h, ne, s));
        if (int rc = run_observable_chunk(h, 0u, ne, h->pv_upstream.p, vm, s, true, gm)) return rc;
        // backward sweeps: runs of programs on the shared coefficients, a program behind the first live gate on its own
        for (uint32_t j = 0; j < nq;) {
          uint32_t j1 = j + 1;
          if (swept[q0 + j]) {
            if (int rc = prep_adjoint(sg[q0 + j], double(sv[q0 + j]))) return rc;
            adjoint_shifted = true;
          } else {
            while (j1 < nq && !swept[q0 + j1]) ++j1;
            if (adjoint_shifted)
              if (int rc = prep_adjoint(-1, 0.0)) return rc;
            adjoint_shifted = false;
          }
          if (int rc = run_adjoint_chunk(h, h->pv_bits.p, j * c, (j1 - j) * c, s, j * c)) return rc;
          j = j1;
        }
        if (vm) HIPCHK(weight_state_grad(h, ne, h->pv_upstream.p, s));
        HIPCHK(launch_scatter_program_rows(h->state_grad.p, h->pv_rows.p, n_slots, c, s0, uint32_t(U), q0 - qa, ne, s));
        HIPCHK(launch_values_from_fixed(h->vals64.p, h->op_inv_scale.p, h->vals_batch.p, ne * T, T, s));
        HIPCHK(launch_accumulate_program_values(h->vals_batch.p, d_row_weights, nq, c, T, s0, h->shift_dst.p + q0,
                                                h->pv_vals.p, s));
        return 0;
      };
      // (the final states feed lambda: every pass that is not measurement-only stores)
      if (int rc = run_program_groups(h, d_bits, d_params, g, order, qa, qb, s0, c, h->pv_base.p, {true, skip, true}, s, backward))
        return rc;
    }
    HIPCHK(launch_reduce_program_grad(h->pv_rows.p, uint32_t(U), n_slots, h->param_slot_begin.p, h->param_slots.p,
                                      h->slot_factor.p, h->shift_dst.p + qa, qb - qa, d_prog_grad, P, s));
  }
  if (adjoint_shifted)
    if (int rc = prep_adjoint(-1, 0.0)) return rc;
  if (d_prog_vals) HIPCHK(launch_doubles_to_floats(h->pv_vals.p, d_prog_vals, size_t(n_prog) * T, s));
  return 0;
}

int qhbm_expectation_jacobian(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                              float* d_out_vals, float* d_jac, void* stream) {
  if (int rc = begin_call(h, U, kNeedObservables)) return rc;
  if (U == 0) return 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int T = h->model.n_ops, P = h->model.n_params;
  const size_t nv = size_t(U) * T;
  HIPCHK(h->upstream_tmp.reserve(nv));
  if (int rc = values_or_scratch(h, U, &d_out_vals)) return rc;
  std::vector<float> up(nv);
  for (int k = 0; k < T; ++k) {
    for (size_t i = 0; i < nv; ++i) up[i] = (int(i % size_t(T)) == k) ? 1.f : 0.f;
    HIPCHK(hipMemcpyAsync(h->upstream_tmp.p, up.data(), nv * sizeof(float), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    if (int rc = adjoint_sweep(h, d_bits, U, d_params, h->upstream_tmp.p, d_out_vals, s)) return rc;
    HIPCHK(launch_scatter_jac(h->state_grad.p, uint32_t(U), uint32_t(h->adj.plan.slot_gate.size()),
                              h->param_slot_begin.p, h->param_slots.p, h->slot_factor.p, d_jac, uint32_t(T),
                              uint32_t(k), uint32_t(P), s));
  }
  return 0;
}

int qhbm_num_passes(qhbm_engine* h, int* forward_passes, int* backward_passes) {
  if (!h) return 1;
  if (int rc = build_plans(h)) return rc;
  if (forward_passes) *forward_passes = int(h->fwd.plan.passes.size());
  if (backward_passes) *backward_passes = int(h->adj.plan.passes.size());
  return 0;
}

int qhbm_describe_schedule(qhbm_engine* h, char* buf, size_t buf_len) {
  if (!h || !buf || !buf_len) return 1;
  if (int rc = build_plans(h)) return rc;
  std::string s = describe_plans(h);
  if (!h->model.terms.empty()) {  // which kernel forms lambda = O psi / the values (bench.py names it in `roofline.kernel`)
    s += std::string("observable kernel: lambda = ") + (block_kernel(h) ? "observable_blocks_kernel" : "apply_observable_kernel");
    s += std::string(" values = ") + (gather_multi_mode(h) ? "apply_observable_kernel (an accumulator per observable)"
                                      : multi_value_mode(h) || (value_mode(h) && block_kernel(h)) ? "observable_blocks_kernel"
                                      : value_mode(h)                                            ? "apply_observable_kernel"
                                                                                                  : "measured in the passes");
    s += "\n";
  }
  std::snprintf(buf, buf_len, "%s", s.c_str());
  return 0;
}

int qhbm_kernel_time_ms(qhbm_engine* h, int reset, double* fwd_ms, int64_t* fwd_launches, double* bwd_ms,
                        int64_t* bwd_launches, double* obs_ms, int64_t* obs_launches) {
  if (!h) return 1;
  double ms[3] = {0.0, 0.0, 0.0};
  int64_t cnt[3] = {0, 0, 0};
  if (h->device >= 0 && !h->events.empty()) {
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipEventSynchronize(h->events.back().b));
    for (auto& ev : h->events) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, ev.a, ev.b) == hipSuccess) { ms[ev.kind] += t; ++cnt[ev.kind]; }
    }
  }
  if (fwd_ms) *fwd_ms = ms[0];
  if (fwd_launches) *fwd_launches = cnt[0];
  if (bwd_ms) *bwd_ms = ms[1];
  if (bwd_launches) *bwd_launches = cnt[1];
  if (obs_ms) *obs_ms = ms[2];
  if (obs_launches) *obs_launches = cnt[2];
  if (reset) {
    h->free_events.insert(h->free_events.end(), h->events.begin(), h->events.end());
    h->events.clear();
  }
  return 0;
}

}  // extern "C"

namespace {

// fp32 operations (FMA = 2) the gate arithmetic of one pass kernel executes per AMPLITUDE of a tile it
// does not skip, from the plan's instance records -- the counts are those of the inline-asm sequences
// in kernels.hip (v_pk_fma_f32 = 4, v_pk_mul_f32 / v_pk_add_f32 = 2 per amplitude pair of lanes):
//   forward   X**t three shears 6, two shears 4 (x_shear.h; + 0.125 per instance that has one: entry 0 of its table)
//             | PH1 3 (half the amplitudes x (mul + fma)) | PH2 1.5 | FULL table 5.625
//             | boundary CPH 3 x (share of waves whose predicate is on) | Y 6 | dense 2x2 14 | dense 4x4 32
//   adjoint   X 16 (psi 6 + lambda 6 + inner product 4), two shears 12 (+ 0.25 per instance) | PH1 8 | PH2 4 | FULL 15.75 (two tables 11.25 + the ten
//             partial sums as scalar differences, round 5: 15 x (mul + fma) + 27 adds = 4.5) | CPH 8 x share | Y 16 |
//             dense 2x2 44 | dense 4x4 on (psi, lambda) + generator 96
// Rounds whose waves are dead (OP_ROUND word 4) run on 2^-popc(dead mask) of the waves.  Wave
// reductions, address arithmetic and record decoding are NOT counted: this is the arithmetic the gate
// set requires of this kernel design, the numerator of a compute roofline against the fp32 vector peak.
// Which X gates ran as two shears is decided per call on the device: `dyn` = the coefficient buffer as the last call
// left it (qhbm_flop_model reads it back); without it every X counts as three shears, which is also what the plan
// search compares (the choice depends on the parameters, a plan must not).
double pass_flops_per_amplitude(const Plan& plan, const Pass& p, const uint32_t* dyn) {
  const RecordLayout L(plan.R, plan.adjoint);
  const bool adj = plan.adjoint;
  double total = 0.0;
  size_t round_i = 0;
  for (size_t pc = 0; pc < p.prog.size();) {
    const uint32_t w0 = p.prog[pc], opc = w0 & 0xffu;
    if (opc == OP_END) break;
    if (opc == OP_ROUND) {
      const uint32_t n_inst = (w0 & ~kRoundNoBarrier) >> 8, first = p.prog[pc + 2], dead = p.prog[pc + 4];
      const uint32_t wmask = round_i < p.round_wavemasks.size() ? p.round_wavemasks[round_i] : 0u;
      const double alive = adj ? 1.0 / double(1u << __builtin_popcount(dead)) : 1.0;
      double f = 0.0;
      for (uint32_t i = 0; i < n_inst; ++i) {
        const uint32_t* rec = &plan.coef_init[first + size_t(i) * size_t(L.words())];
        const uint32_t h0 = rec[0], h1 = rec[1];
        const bool full = (h1 & kFullDiagFlag) != 0;
        f += (adj ? 16.0 : 6.0) * __builtin_popcount(h0 & 0xfu);
        if (const uint32_t x2 = dyn && full ? dyn[first + size_t(i) * size_t(L.words()) + size_t(L.x2_mask())] & h0 & 0xfu : 0u)
          f += (adj ? 0.25 : 0.125) - (adj ? 4.0 : 2.0) * __builtin_popcount(x2);
        if (full) f += adj ? 15.75 : 5.625;
        else f += (adj ? 8.0 : 3.0) * __builtin_popcount((h0 >> 8) & 0xfu) + (adj ? 4.0 : 1.5) * __builtin_popcount((h0 >> 16) & 0x3fu);
        for (int k = 0; k < 8; ++k) {
          if (!(h1 >> k & 1u)) continue;
          const uint32_t pred = rec[L.pred(k)];
          const bool uniform = (pred >> 8) != 0 || (wmask >> (pred & 0xffu) & 1u);  // tile bit or wave bit: half skip
          f += (adj ? 8.0 : 3.0) * (uniform ? 0.5 : 1.0);
        }
        f += (adj ? 16.0 : 6.0) * __builtin_popcount((h1 >> 16) & 0xfu) + (adj ? 44.0 : 14.0) * __builtin_popcount((h1 >> 24) & 0xfu);
      }
      total += alive * f;
      ++round_i;
      pc += kRoundWords;
    } else if (opc == OP_GATE2) {
      total += adj ? 96.0 : 32.0;
      pc += kGate2Words;
    } else if (opc == OP_MEASURE_WHT) {  // |psi|^2, ten butterfly stages, the terms spread over the threads
      total += 3.0 + 10.0 + 2.0 * double(w0 >> 8) / double(size_t(1) << (plan.K - plan.R));
      pc += size_t(kWhtHeaderWords) + size_t(w0 >> 8) * kMeasTermWords;
    } else {  // OP_MEASURE: [op | n_groups << 8] then groups x {[xl] [n_terms] terms x 4 words}
      const uint32_t n_groups = w0 >> 8;
      ++pc;
      for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t n_terms = p.prog[pc + 1];
        total += 6.0 + double(n_terms);  // conj(psi[l ^ x]) psi[l] (3 FMA) + one signed add per term (upper bound)
        pc += 2 + size_t(n_terms) * kMeasTermWords;
      }
    }
  }
  return total;
}

// Executed micro-ops of one pass, in WAVE-EXECUTIONS per state (a micro-op a wave runs once counts 1): the weights
// of a dynamic instruction mix (scripts/instruction_mix.py multiplies them with the per-micro-op instruction counts of
// the compiled kernel).  Columns: qhbm_engine.h QHBM_CENSUS_*.
void pass_census(const Plan& plan, const Pass& p, double tiles_per_state, double* out) {
  const RecordLayout L(plan.R, plan.adjoint);
  const bool adj = plan.adjoint;
  const double waves = double(size_t(1) << (plan.K - plan.R)) / 64.0 * tiles_per_state;
  out[QHBM_CENSUS_TILES] += tiles_per_state;
  size_t round_i = 0;
  for (size_t pc = 0; pc < p.prog.size();) {
    const uint32_t w0 = p.prog[pc], opc = w0 & 0xffu;
    if (opc == OP_END) break;
    if (opc != OP_ROUND) {
      if (opc == OP_GATE2) pc += kGate2Words;
      else if (opc == OP_MEASURE_WHT) pc += size_t(kWhtHeaderWords) + size_t(w0 >> 8) * kMeasTermWords;
      else {
        const uint32_t n_groups = w0 >> 8;
        ++pc;
        for (uint32_t g = 0; g < n_groups; ++g) pc += 2 + size_t(p.prog[pc + 1]) * kMeasTermWords;
      }
      continue;
    }
    const uint32_t n_inst = (w0 & ~kRoundNoBarrier) >> 8, first = p.prog[pc + 2], dead = p.prog[pc + 4];
    const uint32_t wmask = round_i < p.round_wavemasks.size() ? p.round_wavemasks[round_i] : 0u;
    const double alive = (adj ? 1.0 / double(1u << __builtin_popcount(dead)) : 1.0) * waves;
    out[QHBM_CENSUS_ROUNDS] += waves;
    out[(w0 & kRoundNoBarrier) ? QHBM_CENSUS_ROUNDS_NO_BARRIER : QHBM_CENSUS_ROUNDS_BARRIER] += waves;
    for (uint32_t i = 0; i < n_inst; ++i) {
      const uint32_t* rec = &plan.coef_init[first + size_t(i) * size_t(L.words())];
      const uint32_t h0 = rec[0], h1 = rec[1];
      const bool full = (h1 & kFullDiagFlag) != 0;
      out[QHBM_CENSUS_INSTANCES] += alive;
      for (int j = 0; j < 4; ++j) {
        if (!(h0 >> j & 1u)) continue;
        const bool slot = !adj || rec[L.slot_x(j)] != 0xffffffffu;
        out[slot ? QHBM_CENSUS_X : QHBM_CENSUS_X_NO_SLOT] += alive;
      }
      if (full) out[QHBM_CENSUS_FULL] += alive;
      out[QHBM_CENSUS_PH1] += alive * __builtin_popcount((h0 >> 8) & 0xfu);
      out[QHBM_CENSUS_PH2] += alive * __builtin_popcount((h0 >> 16) & 0x3fu);
      for (int k = 0; k < 8; ++k) {
        if (!(h1 >> k & 1u)) continue;
        const uint32_t pred = rec[L.pred(k)];
        if ((pred >> 8) != 0) { out[QHBM_CENSUS_CPH_TILE_ON] += 0.5 * alive; out[QHBM_CENSUS_CPH_OFF] += 0.5 * alive; }
        else if (wmask >> (pred & 0xffu) & 1u) { out[QHBM_CENSUS_CPH_WAVE_ON] += 0.5 * alive; out[QHBM_CENSUS_CPH_OFF] += 0.5 * alive; }
        else out[QHBM_CENSUS_CPH_LANE] += alive;
      }
      if (adj) {  // eight-wide reductions, counted as instance_adj tests them: one per SET that has a value -- the set's
        // levels 2 and 3 and quad stages (kernels.hip add_slots8).  CPH set; PH2 set (per-term, or FULL with pair terms);
        // X + PH1 set (X gates that own a slot: bits 12..15, not every X).  Level 1 is QHBM_CENSUS_LEVEL1; the
        // lane-bit-5 stage and the store of the X + PH1 and PH2 sets run once in EVERY instance (QHBM_CENSUS_INSTANCES),
        // the CPH set's with its count here.
        if (h1 & 0xffu) out[QHBM_CENSUS_REDUCE8] += alive;
        if (full && ((h0 >> 24) & 0x3fu)) out[QHBM_CENSUS_REDUCE8] += alive;
        if ((h0 >> 16) & 0x3fu) out[QHBM_CENSUS_REDUCE8] += alive;
        if (((h0 >> 8) & 0xffu) || (full && ((h0 >> 4) & 0xfu))) out[QHBM_CENSUS_REDUCE8] += alive;
        out[QHBM_CENSUS_LEVEL1] += alive * level1_adds(rec);
      }
    }
    ++round_i;
    pc += kRoundWords;
  }
}

}  // namespace

// The chip's sustained packed-fp32 rate and shader clock right now (bench.py calls it straight after its timed region,
// with the chip as warm as the timed kernels left it): one probe launch (kernels.hip clock_probe_kernel) timed with HIP
// events.  ghz = shader cycles per real time inside the waves; cycles_per_pk_fma = kernel time x ghz / instructions of a
// SIMD; tflops = 4 flop x 64 lanes x SIMDs / cycles_per_pk_fma x ghz.  Synchronises the stream.
extern "C" int qhbm_clock_probe(qhbm_engine* h, double* ghz, double* cycles_per_pk_fma, double* tflops, void* stream_v) {
  if (!h) return 1;
  if (int rc = need_device(h)) return rc;
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, h->device));
  const uint32_t n_cus = uint32_t(prop.multiProcessorCount);
  const uint32_t n_waves = clock_probe_waves(n_cus);
  // (the probe's buffers stay with the engine: bench.py probes after every run)
  DevBuf<uint64_t>& out = h->probe_out;
  DevBuf<float>& sink = h->probe_sink;
  HIPCHK(out.reserve(size_t(2) * n_waves));
  HIPCHK(sink.reserve(1));
  struct Events {  // destroyed on every exit path
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~Events() {
      if (e0) (void)hipEventDestroy(e0);
      if (e1) (void)hipEventDestroy(e1);
    }
  } ev;
  HIPCHK(hipEventCreate(&ev.e0));
  HIPCHK(hipEventCreate(&ev.e1));
  HIPCHK(launch_clock_probe(out.p, sink.p, n_cus, stream));  // warm-up: code object load, clocks
  HIPCHK(hipEventRecord(ev.e0, stream));
  HIPCHK(launch_clock_probe(out.p, sink.p, n_cus, stream));
  HIPCHK(hipEventRecord(ev.e1, stream));
  HIPCHK(hipEventSynchronize(ev.e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, ev.e0, ev.e1));
  std::vector<uint64_t> host(size_t(2) * n_waves);
  HIPCHK(hipMemcpy(host.data(), out.p, host.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  double cyc = 0.0, ticks = 0.0;
  for (uint32_t w = 0; w < n_waves; ++w) { cyc += double(host[2 * w]); ticks += double(host[2 * w + 1]); }
  if (ticks <= 0.0 || ms <= 0.f) return fail(h, "clock probe: no time elapsed");
  const double g = cyc / ticks * 0.1;  // s_memrealtime ticks at 100 MHz
  const double per = double(ms) * 1e6 * g / clock_probe_instructions_per_simd();
  if (ghz) *ghz = g;
  if (cycles_per_pk_fma) *cycles_per_pk_fma = per;
  if (tflops) *tflops = 256.0 / per * g * 1e9 * double(n_cus) * 4.0 / 1e12;
  return 0;
}

extern "C" int qhbm_plan_builds(qhbm_engine* h, int64_t* forward_plans, int64_t* backward_plans) {
  if (!h) return 1;
  if (forward_plans) *forward_plans = h->fwd_plans_built;
  if (backward_plans) *backward_plans = h->adj_plans_built;
  return 0;
}

extern "C" int qhbm_census_columns(void) { return QHBM_CENSUS_COLUMNS; }

extern "C" int qhbm_op_census(qhbm_engine* h, int adjoint, int max_passes, double* out, int* n_passes) {
  if (!h || !out || !n_passes) return 1;
  if (int rc = build_plans(h)) return rc;
  const DevicePlan& d = adjoint ? h->adj : h->fwd;
  std::vector<PassArgs> args;
  std::vector<uint32_t> prog, tables;
  fill_args(d.plan, h->model, &args, &prog, &tables);
  *n_passes = int(args.size());
  for (int i = 0; i < max_passes * QHBM_CENSUS_COLUMNS; ++i) out[i] = 0.0;
  for (size_t i = 0; i < args.size() && int(i) < max_passes; ++i) {
    const Pass& p = d.plan.passes[i];
    // the first forward pass computes on ONE tile per state; later passes on the tiles they launch
    const double tiles = (!adjoint && (p.flags & PASS_INIT_BASIS)) ? 1.0 : double(size_t(1) << args[i].n_free);
    pass_census(d.plan, p, tiles, out + i * QHBM_CENSUS_COLUMNS);
  }
  return 0;
}

namespace {
}  // namespace

extern "C" int qhbm_flop_model(qhbm_engine* h, int U, int with_vjp, double* fwd_flops, double* obs_flops,
                               double* bwd_flops) {
  if (!h) return 1;
  if (int rc = build_plans(h)) return rc;
  const double amps = double(size_t(1) << h->fwd.plan.n_eff) * double(U);
  double f = 0.0, o = 0.0, b = 0.0;
  const bool from_obs = with_vjp ? (value_mode(h) || multi_value_mode(h)) : forward_values_from_observable(h);  // no measurement in the sweep
  // the coefficient buffers as the last call left them: which X gates ran as two shears (pass_flops_per_amplitude)
  std::vector<uint32_t> dyn_f, dyn_b;
  auto read_back = [&](const DevicePlan& d, std::vector<uint32_t>* out) -> hipError_t {
    if (h->device < 0 || !d.uploaded || !h->opt_x_two_shear || d.coef.n < d.plan.coef_init.size()) return hipSuccess;
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    out->resize(d.plan.coef_init.size());
    if (e == hipSuccess && !out->empty()) e = hipMemcpy(out->data(), d.coef.p, out->size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    return e;
  };
  HIPCHK(read_back(h->fwd, &dyn_f));
  if (with_vjp) HIPCHK(read_back(h->adj, &dyn_b));
  {
    std::vector<PassArgs> args;
    std::vector<uint32_t> prog, tables;
    fill_args(h->fwd.plan, h->model, &args, &prog, &tables);
    for (size_t i = 0; i < args.size(); ++i) {
      const Pass& p = h->fwd.plan.passes[i];
      if (from_obs && p.is_measure_only) continue;
      const double live = 1.0 / double(1ull << __builtin_popcount(args[i].zero_mask));
      // the first pass computes on ONE tile per state (the others write zeros and return)
      const double share = (p.flags & PASS_INIT_BASIS) ? 1.0 / double(1ull << p.nonlocal_pos.size()) : live;
      Pass q = p;
      if (from_obs) {  // PASS_SKIP_MEASURE: cut the program at its first measurement
        for (size_t pc = 0; pc < q.prog.size();) {
          const uint32_t opc = q.prog[pc] & 0xffu;
          if (opc == OP_END) break;
          if (opc == OP_MEASURE || opc == OP_MEASURE_WHT) { q.prog[pc] = OP_END; break; }
          pc += opc == OP_ROUND ? size_t(kRoundWords) : size_t(kGate2Words);
        }
      }
      f += share * amps * pass_flops_per_amplitude(h->fwd.plan, q, dyn_f.empty() ? nullptr : dyn_f.data());
    }
  }
  if (with_vjp || from_obs) {
    // lambda = O psi: one packed FMA per amplitude and X-mask group (4), one add per term whose sign varies
    // inside a thread's amplitudes (upper bound: every term), <psi|O|psi> 4 in value mode
    std::vector<uint32_t> xs;
    for (const PauliTerm& t : h->model.terms) xs.push_back(t.x);
    std::sort(xs.begin(), xs.end());
    const double groups = double(std::unique(xs.begin(), xs.end()) - xs.begin());
    o = amps * (4.0 * groups + double(h->model.terms.size()) + (value_mode(h) ? 4.0 : 0.0));
  }
  if (with_vjp) {
    std::vector<PassArgs> args;
    std::vector<uint32_t> prog, tables;
    fill_args(h->adj.plan, h->model, &args, &prog, &tables);
    for (size_t i = 0; i < args.size(); ++i) {
      const double live = 1.0 / double(1ull << __builtin_popcount(args[i].zero_mask));
      b += live * amps * pass_flops_per_amplitude(h->adj.plan, h->adj.plan.passes[i], dyn_b.empty() ? nullptr : dyn_b.data());
    }
  }
  if (fwd_flops) *fwd_flops = f;
  if (obs_flops) *obs_flops = o;
  if (bwd_flops) *bwd_flops = b;
  return 0;
}

extern "C" {

int qhbm_traffic_model(qhbm_engine* h, int U, int with_vjp, double* fwd_bytes, double* obs_bytes,
                       double* bwd_bytes) {
  if (!h) return 1;
  if (int rc = build_plans(h)) return rc;
  const double tile_all = double(state_bytes(h)) * double(U);  // every tile of every state, once
  double f = 0.0, o = 0.0, b = 0.0;
  bool measure_only_after = !h->fwd.plan.global_terms.empty();
  for (const Pass& p : h->fwd.plan.passes) measure_only_after |= p.is_measure_only;
  const bool from_obs = with_vjp ? (value_mode(h) || multi_value_mode(h)) : forward_values_from_observable(h);  // no measurement in the sweep
  {
    std::vector<PassArgs> fargs;
    std::vector<uint32_t> fprog, ftables;
    fill_args(h->fwd.plan, h->model, &fargs, &fprog, &ftables);
    for (size_t i = 0; i < fargs.size(); ++i) {
      const Pass& p = h->fwd.plan.passes[i];
      if (from_obs && p.is_measure_only) continue;  // the values come from lambda = O psi
      const double live = 1.0 / double(1ull << __builtin_popcount(fargs[i].zero_mask));  // tiles not skipped
      if (!(p.flags & PASS_INIT_BASIS)) f += live * tile_all;  // the first pass writes the basis state, reads nothing
      if (!p.is_measure_only && (!p.completes_circuit || from_obs || with_vjp || measure_only_after)) f += live * tile_all;
    }
  }
  if (!with_vjp && from_obs) o = tile_all;  // psi read (gathered through L2), nothing written
  if (with_vjp) {
    o = 2.0 * tile_all;  // psi read (gathered through L2), lambda written
    if (multi_value_mode(h) && !gather_multi_mode(h)) o += tile_all;  // ... and the launch that returns the values of several observables
    std::vector<PassArgs> args;
    std::vector<uint32_t> prog, tables;
    fill_args(h->adj.plan, h->model, &args, &prog, &tables);
    for (size_t i = 0; i < args.size(); ++i) {
      double live = 1.0 / double(1ull << __builtin_popcount(args[i].zero_mask));  // tiles not skipped
      // a tile without some of the four low index bits still moves whole 128-byte lines
      {
        int low_missing = 0;
        for (uint32_t k = 0; k < args[i].n_nonlocal; ++k) low_missing += args[i].nonlocal_pos[k] < 4;
        live = std::min(1.0, live * double(1u << low_missing));
      }
      const Pass& ap = h->adj.plan.passes[i];
      double write_share = 1.0;  // a relabeling store writes only the amplitudes whose finished bits equal the input
      if (ap.flags & PASS_RELABEL) write_share = 1.0 / double(1u << __builtin_popcount(ap.frozen_new_local));
      b += live * tile_all * 2.0 * (1.0 + ((ap.flags & PASS_STORE) ? write_share : 0.0));
    }
  }
  if (fwd_bytes) *fwd_bytes = f;
  if (obs_bytes) *obs_bytes = o;
  if (bwd_bytes) *bwd_bytes = b;
  return 0;
}

}  // extern "C"
