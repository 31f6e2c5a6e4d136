// plan_emulate.h -- executes the scheduler's plans on the CPU in complex128, and a dense oracle to compare with.
//
// Test infrastructure, not product (tests/sanitize/plan_fuzz.cpp drives it).  Two independent halves:
//
//   * the ORACLE: a dense gate-by-gate simulator from the matrices documented in include/qhbm_engine.h
//     (G**t = sum_k exp(i pi t e_k) P_k, times exp(i pi t global_shift)), Pauli-sum values straight from the masks,
//     the gradient by a plain adjoint sweep.  It knows nothing about plans, passes, tiles or lowered micro-ops.
//
//   * the EMULATOR: reads a Plan the way the gfx950 kernels read it -- the pass arguments fill_args() derives, program
//     words, instance records, thread tables, predicates, physical layouts, pruning masks -- and executes it on a
//     state array addressed PHYSICALLY, in double.  Every amplitude a plan claims it need not write or read is
//     poisoned with NaN, so a wrong pruning claim reaches a result.
//
// Coefficients are the mathematical meaning of each micro-op (X**t as c I - i s X, not the kernels' three shears),
// restated in double from prep_coefs_kernel / combine_diag_kernel.
#pragma once
#include <complex>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/qhbm_engine.h"
#include "../../qhbm-library_amd/csrc/plan_args.h"
#include "../../qhbm-library_amd/csrc/schedule.h"

namespace emu {

typedef std::complex<double> cd;

// ---- oracle -----------------------------------------------------------------------------------------------------
// U = exp(i pi t shift) G**t and the generator A with dU/dt = i pi (A + shift) U, row-major, matrix index of a
// two-qubit gate = (bit of q0) << 1 | (bit of q1).  Returns the number of qubits (1 or 2).
int oracle_gate(int kind, double t, double shift, cd U[16], cd A[16]);
double oracle_exponent(const qhbm::Gate& g, const std::vector<double>& params);
// |basis> run through the circuit; 2^n amplitudes, qubit q <-> index bit n - 1 - q
std::vector<cd> oracle_state(const qhbm::Model& m, const std::vector<double>& params, uint32_t basis);
std::vector<double> oracle_values(const qhbm::Model& m, const std::vector<cd>& psi);
// sum_k up[k] O_k psi
std::vector<cd> oracle_apply_observables(const qhbm::Model& m, const std::vector<cd>& psi, const std::vector<double>& up);
// d/d params of sum_k up[k] <psi|O_k|psi>
std::vector<double> oracle_gradient(const qhbm::Model& m, const std::vector<double>& params, uint32_t basis,
                                    const std::vector<double>& up);

// ---- emulator ---------------------------------------------------------------------------------------------------
struct Emulation {
  const qhbm::Model* m = nullptr;
  const qhbm::Plan* plan = nullptr;
  std::vector<qhbm::PassArgs> args;      // as fill_args derives them (a test may corrupt them afterwards)
  std::vector<uint32_t> prog, tables;
  std::vector<double> cf;                // coefficient buffer in double (static words stay in plan->coef_init)
  std::string err;                       // first structural problem met while executing (empty: none)
};
// fill_args + coefficient preparation for `params`
void emu_prepare(const qhbm::Model& m, const qhbm::Plan& plan, const std::vector<double>& params, Emulation* e);

struct ForwardResult {
  std::vector<double> values;   // per observable: every measurement contribution of every pass and tile + global terms
  std::vector<cd> final_state;  // logical order, 2^n_eff amplitudes, after the pass with completes_circuit
  bool have_final = false;
};
// `skip_measure`: every measurement op and measure-only pass skipped (PASS_SKIP_MEASURE, engine.cpp run_forward_chunk)
bool emu_forward(Emulation* e, uint32_t basis, bool skip_measure, ForwardResult* out);

struct AdjointResult {
  std::vector<double> slots;   // one value per gradient slot of the plan
  std::vector<double> grad;    // per parameter: sum over its slots of slot_factor * slot value
  std::vector<double> bar;     // per parameter: 4 * 2^-24 * sum |slot_factor * slot value| + 1e-10
};
// psi, lambda: logical order, 2^n_eff amplitudes (the emulator lays them out as the first backward pass loads them)
bool emu_adjoint(Emulation* e, uint32_t basis, const std::vector<cd>& psi, const std::vector<cd>& lam, AdjointResult* out);

}  // namespace emu
