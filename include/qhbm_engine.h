/*
 * qhbm_engine.h -- C ABI of the MI355X-native expectation engine.
 *
 * This is the drop-in boundary for the hot path of google/qhbm-library:
 *
 *   qhbmlib/inference/qnn.py:82-84   QuantumInference._expectation(circuits,
 *       symbol_names, symbol_values, observables)            <- qhbm_expectation
 *   qhbmlib/inference/qnn.py:134-138 tfq.layers.Expectation()(circuits,
 *       symbol_names, symbol_values, operators) forward       <- qhbm_expectation
 *   qhbmlib/inference/qnn.py:90-99   adjoint backward of that op (VJP w.r.t.
 *       symbol_values, summed through the tile of qnn.py:75-76) <- qhbm_expectation_vjp
 *   qhbmlib/inference/qnn.py:168,192-194 ParameterShift gradient circuits
 *       (rule restated in baselines/train.py:190-240)          <- qhbm_expectation_vjp(method=1)
 *   qhbmlib/models/circuit.py:129-136 bit-injection X**bit     <- `bits` argument
 *   qhbmlib/models/circuit.py:138-178 append / inverse         <- gate list passed to qhbm_set_circuit
 *
 * Conventions
 *   - qubit q in [0, n_qubits). Qubit 0 is the MOST significant bit of a basis
 *     index (cirq big-endian; qhbmlib/inference/ebm.py:445-447).
 *   - `bits` is row-major [U, n_qubits] int8; column j initialises qubit j.
 *   - exponent of a gate: t = scalar * params[param_idx] + offset
 *     (param_idx < 0: t = offset).  Inverse circuit = reversed gate list with
 *     scalar and offset negated (circuit.py:164-176).
 *   - Pauli masks are in QUBIT space: bit q of x_mask set  <=> X or Y on qubit q,
 *     bit q of z_mask set <=> Z or Y on qubit q.
 *   - All pointers named d_* are DEVICE pointers (HBM); the others are host
 *     pointers.  Work is enqueued on `stream` (a hipStream_t cast to void*;
 *     NULL = default stream) and is asynchronous with respect to the host.
 *   - Every function returns 0 on success, non-zero on error;
 *     qhbm_last_error() gives the message.  No exceptions cross the ABI.
 *   - One engine per device; an engine is not thread-safe, distinct engines are
 *     independent.
 */
#ifndef QHBM_ENGINE_H_
#define QHBM_ENGINE_H_

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QHBM_ABI_VERSION 5

/* Gate kinds: the one-parameter "power gate" families of cirq 0.14.1 that
 * tensorflow-quantum 0.6.1 serialises.  A gate is
 * G**t with the cirq matrix convention
 *     G**t = sum_k exp(i*pi*t*e_k) P_k      (eigen-exponents e_k, projectors P_k)
 * times cirq's global phase exp(i*pi*t*global_shift) (qhbm_gate::global_shift; 0 for the
 * plain power gates).  rx/ry/rz(theta) are XPOW/YPOW/ZPOW with scalar = 1/pi and
 * global_shift = -0.5.  The phase never changes an expectation value, a gradient or a
 * sample, so the hot path ignores it; qhbm_statevector applies the product of all gates'
 * phases to the exported states, which therefore equal cirq's final_state_vector -- and the
 * matrix tfq.layers.Unitary returns (qhbmlib/inference/qnn_utils.py:23-33) -- exactly, not up
 * to a phase.  PhasedXPow, FSim and PhasedISwapPow are lowered by the host to products of
 * these kinds. */
enum qhbm_gate_kind {
  QHBM_GATE_I = 0,
  QHBM_GATE_XPOW = 1,
  QHBM_GATE_YPOW = 2,
  QHBM_GATE_ZPOW = 3,
  QHBM_GATE_HPOW = 4,
  QHBM_GATE_CZPOW = 5,
  QHBM_GATE_CNOTPOW = 6,  /* q0 = control, q1 = target */
  QHBM_GATE_SWAPPOW = 7,
  QHBM_GATE_ISWAPPOW = 8,
  QHBM_GATE_XXPOW = 9,
  QHBM_GATE_YYPOW = 10,
  QHBM_GATE_ZZPOW = 11,
  QHBM_GATE_KIND_COUNT = 12
};

typedef struct qhbm_gate {
  int32_t kind;      /* enum qhbm_gate_kind */
  int32_t q0;        /* first qubit */
  int32_t q1;        /* second qubit, -1 for one-qubit gates */
  int32_t param_idx; /* index into params[], -1 = constant exponent */
  float scalar;      /* exponent = scalar * params[param_idx] + offset */
  float offset;
  float global_shift; /* cirq EigenGate global_shift: the gate is exp(i*pi*t*global_shift) * G**t
                         (ABI v3; cirq.rx/ry/rz and tfq.util.exponential's
                         rotations -- qhbmlib/models/circuit.py:268-272 -- carry -0.5) */
} qhbm_gate;

/* Gradient method for qhbm_expectation_vjp. */
enum qhbm_grad_method {
  QHBM_GRAD_ADJOINT = 0,        /* adjoint sweep, what tfq.layers.Expectation uses */
  QHBM_GRAD_PARAMETER_SHIFT = 1 /* two shifted forwards per gate occurrence */
};

typedef struct qhbm_engine qhbm_engine;

/* ---- lifetime ---------------------------------------------------------- */
int qhbm_abi_version(void);
/* Creates an engine bound to HIP device `device`. */
int qhbm_create(int device, qhbm_engine** out);
void qhbm_destroy(qhbm_engine* h);
/* Message of the last failing call on this engine (or of qhbm_create when
 * h == NULL).  Valid until the next call. */
const char* qhbm_last_error(const qhbm_engine* h);

/* ---- model ------------------------------------------------------------- */
/* Every setter below, and qhbm_set_option, may be called on a live handle between compute calls.  What survives:
 *   - the observables survive qhbm_set_circuit if and only if n_qubits is unchanged (they are kept, masks and scales as
 *     installed); after a circuit of another size the calls that need observables fail with "qhbm_set_observables has
 *     not been called" until they are installed again;
 *   - the gradient mask never survives qhbm_set_circuit, not even for a circuit with as many parameters;
 *   - options survive everything;
 *   - the states kept by qhbm_expectation_retain / qhbm_table_expectation_retain and the rows qhbm_state_gradients
 *     serves survive NO setter that invalidates a plan: qhbm_set_circuit, qhbm_set_observables, a planning option of
 *     qhbm_set_option (whatever the value, the current one included), and qhbm_set_gradient_mask with a mask that differs
 *     from the installed one.  qhbm_retained_states reads 0 from that moment on, and the retained VJPs and
 *     qhbm_state_gradients fail and write nothing.  A setter that changes no plan drops nothing: the installed mask
 *     again, or an option that takes no part in planning ("chunk_states", "workspace_budget_mb", "profile_events",
 *     "values_from_observable", "shift_prefix_sharing", "observable_kernel" and the other kernel choices). */
/* Installs the total circuit (bit-injector excluded: it is the `bits`
 * argument).  Replaces tfq serialisation + append_circuit
 * (circuit.py:129-160).  The gate list is copied. */
int qhbm_set_circuit(qhbm_engine* h, int n_qubits, int n_gates,
                     const qhbm_gate* gates, int n_params);

/* Which parameters want a gradient (optional; after qhbm_set_circuit, which resets it).  needs_grad[p] == 0 freezes
 * parameter p: its entries of every gradient the engine returns are 0, its gates get no gradient work (no slot in the
 * adjoint sweep, no shifted programs under the parameter-shift rule), and the adjoint sweep STOPS at the first gate,
 * in circuit order, of a parameter that is not frozen -- the leading gates of frozen parameters are never un-applied.
 * The reference has no such notion (tfq's differentiators return d/d(symbol) for every symbol, qnn.py:75-76, used or
 * not); the host mirror derives the mask from torch's requires_grad of the circuits that make up the total circuit
 * (QMHL with a fixed data QHBM: the data circuit's half).  NULL restores "all".  Host pointer, n_params entries. */
int qhbm_set_gradient_mask(qhbm_engine* h, const uint8_t* needs_grad, int n_params);

/* Installs n_ops observables; op k is sum_{j in [term_offsets[k],
 * term_offsets[k+1])} coeffs[j] * Pauli(x_masks[j], z_masks[j]).
 * Replaces the tiled PauliSum protos of qnn.py:133.  Arrays are copied. */
int qhbm_set_observables(qhbm_engine* h, int n_ops, const int32_t* term_offsets,
                         const float* coeffs, const uint64_t* x_masks,
                         const uint64_t* z_masks);

/* ---- tuning ------------------------------------------------------------ */
/* Optional knobs (name -> value); unknown names are an error.
 *   "tile_qubits"          log2 amplitudes of one LDS tile (10..14), 0 = auto
 *   "adjoint_tile_qubits"  the same for the backward sweep (10..13), 0 = auto (12, or 13 when that plan's
 *                          modelled time -- arithmetic of qhbm_flop_model, tile traffic -- is at least 2 % lower)
 *   "chunk_states"         states simulated per launch group, 0 = auto
 *   "workspace_budget_mb"  cap on the statevector workspace; 0 = a third of the device's memory
 *   "profile_events"       record HIP events around the pass kernels (qhbm_kernel_time_ms)
 *   "shift_prefix_sharing" parameter-shift VJP and qhbm_program_vjps: 1 (default) = a shifted program starts at the
 *                          first forward pass that reads its gate, from the base program's state -- on plans whose
 *                          first pass writes one tile per state (every index bit meets a non-diagonal gate); a plan
 *                          with an idle or diagonal-only qubit zero-fills in its first pass and runs every program
 *                          from the basis state; 0 = always from the basis state.  The outputs are the same bits.
 * Developer knobs for A/B measurements (defaults are the measured best): "measure_tile_qubits"
 * (tile of measurement-only passes, 0 = largest), "adjoint_exchange" (1 = register-resident tile
 * pair with one LDS exchange buffer, 0 = both tiles in LDS), "full_diag_threshold" /
 * "adjoint_full_diag_threshold", "round_qubits" (must be 4), "force_general_kernels",
 * "cph_wave_bits" (1 = the scheduler's layout choices of round 2: the partner bits of boundary
 * controlled phases and the bits with no gate left become wave bits, so that whole waves skip work
 * on predicates that are off / on zeros of psi, and adjoint tail passes use tiles without the low
 * index bits; 0 = the plain layout, for A/B measurements), "values_from_observable" (1 = with a single
 * observable the expectation value is taken from lambda = O psi in the calls that compute lambda
 * anyway, and the forward sweep measures nothing; 0 = always measure in the forward sweep),
 * "adjoint_stop_early" (with frozen parameters, qhbm_set_gradient_mask: 1 = the backward sweep stops at the first
 * gate of a live parameter, 0 = it runs to the basis state and prunes its tail, -1 = whichever the time model prefers),
 * "adjoint_plan_search" (1 = the backward plan is the one with the least modelled time among the pass orders the
 * scheduler ranked best and the greedy order; 0 = the scheduler's first choice),
 * "forward_values_from_observable" (forward-only calls with a single observable: -1 = the same kernel, storing
 * nothing, supplies the value when the plan has more than one pass and some term flips two or more qubits or
 * needs a measurement-only pass; 0 = measure in the passes; 1 = always),
 * "adjoint_relabel" (1 = adjoint plans move finished index bits out of the 128-byte lines when the finishing
 * pass stores its tiles), "x_two_shear" (1 = an X**t next to a full diagonal table whose angle is at most pi / 3
 * runs as two shears, its scaling folded into the table; 0 = always three shears), "forward_pairs" (1 = dense
 * lean forward passes run on pairs of states with the tiles in registers), "wide_last_pass" (-1 = the last forward gate pass may take a tile one or two bits
 * wider when that saves a pass, unless tile_qubits is set; 0 = never; 1 = always), "forward_move_low_bits" (1 = a forward
 * pass may leave any four of its index bits on the 128-byte line positions when it stores, where a cost model prefers
 * the plan that results -- tiles of contiguous bits, fewer full passes; the last gate pass restores the layout; 0 = never:
 * the plans and result bits of before; 2 = also with tile_qubits set and whenever such a plan exists), "observable_xcd_states"
 * (lambda = O psi: 1 = one state per XCD at a time, 0 = every XCD an eighth of each state, -1 = by state size: states of
 * 64 MiB and more are shared), "observable_kernel" (lambda = O psi and <psi|O|psi>: 0 = one L2 gather per X-mask and
 * block of 2^11 amplitudes, 1 = partner blocks of 2^13 amplitudes staged in LDS once per group of masks that share them
 * (states of >= 13 qubits), -1 = whichever a fitted cost model prefers: the block kernel for operators with many masks),
 * "observable_block_bits" (shape of that block kernel: 13 (default) = blocks of 2^13 amplitudes under ONE workgroup of 1024
 * threads per CU whose two halves split a group's masks; 12 = blocks of 2^12 under TWO independent workgroups of 512 threads
 * per CU, every mask of a group applied by the one workgroup -- measured SLOWER, 94.4 against 51.2 ms for lambda on BASELINE
 * config 4: the co-resident workgroups drift apart and the window of partner blocks leaves the L2, hit rate 0.27 against
 * 0.77; kept for A/B runs), "observable_split_rows" (blocks of 2^13: 1 = the two halves of the workgroup split the block's
 * ROWS and each applies every mask of a group, instead of splitting the group's masks -- measured SLOWER, 57.6 against 51.3 ms:
 * twice the instructions per term; 0 = default),
 * "multi_observable_values" (several observables: -1 = their values come from ONE launch of the block kernel over the
 * final states, after lean measurement-free passes, when some term flips two or more qubits and there are at most 64
 * observables; 0 = always measured in the passes; 1 = always from the kernel, up to 256 observables),
 * "gather_multi_values" (2..4 observables: 1 = the gather kernel forms lambda AND carries a value accumulator per
 * observable -- one launch instead of two; 0 (default) = the values from the block kernel's own launch: the one-launch
 * form measured SLOWER, 103 against 64.7 ms on BASELINE config 3 split into its XX / YY / ZZ sums),
 * "observable_far_windows" (gather kernel, one observable or lambda alone: the masks that flip only bits of a seven-bit
 * window of far index bits (and bits 0..3) are applied by an extra launch per window that works in the index space with
 * that window swapped into bits 4..10 -- no partner run of theirs crosses the fabric.  0 (default) = never: measured NOT
 * faster at 28 qubits (65.0 ms in one launch, 66.2 in three); 1 = always, any window that holds a mask; -1 = from 26
 * qubits up, windows with three masks or more).
 */
int qhbm_set_option(qhbm_engine* h, const char* name, int64_t value);

/* Bytes of device workspace the engine will hold for a batch of U states
 * (forward only, or forward + adjoint when with_vjp != 0). */
int qhbm_workspace_bytes(qhbm_engine* h, int U, int with_vjp, size_t* out);

/* Bytes of device memory the engine holds right now (statevector workspace and gradient
 * partials); a host-side cache of engines uses it to bound its total footprint. */
int qhbm_allocated_bytes(qhbm_engine* h, size_t* out);

/* ---- hot path ---------------------------------------------------------- */
/* out[u, k] = <x_u| C(params)^dagger  O_k  C(params) |x_u>
 *   d_bits   [U, n_qubits] int8   (device)
 *   d_params [n_params]    float  (device)
 *   d_out    [U, n_ops]    float  (device) */
int qhbm_expectation(qhbm_engine* h, const int8_t* d_bits, int U,
                     const float* d_params, float* d_out, void* stream);

/* Values plus one vector-Jacobian product:
 *   d_grad[p] = sum_{u,k} d_upstream[u,k] * d out[u,k] / d params[p]
 *   d_upstream [U, n_ops] float, d_out_vals [U, n_ops] float (may be NULL),
 *   d_grad [n_params] float (overwritten). */
int qhbm_expectation_vjp(qhbm_engine* h, const int8_t* d_bits, int U,
                         const float* d_params, const float* d_upstream,
                         float* d_out_vals, float* d_grad, int method,
                         void* stream);

/* The same pair as two calls for an autograd-style caller (forward now, backward later, as
 * tf.custom_gradient / torch.autograd.Function drive qnn.py:134-138): qhbm_expectation_retain
 * is qhbm_expectation but leaves the final states in the workspace when the batch fits one
 * backward chunk; qhbm_expectation_vjp_retained then runs only lambda = O psi and the backward
 * sweep on them (same bits and params as the retaining call) and consumes them.  It fails if
 * nothing is retained -- any other compute call, or a batch too large, drops the states -- and
 * the caller falls back to qhbm_expectation_vjp. */
int qhbm_expectation_retain(qhbm_engine* h, const int8_t* d_bits, int U,
                            const float* d_params, float* d_out, void* stream);
int qhbm_expectation_vjp_retained(qhbm_engine* h, const int8_t* d_bits, int U,
                                  const float* d_params, const float* d_upstream,
                                  float* d_grad, void* stream);
/* Number of states the workspace currently retains for qhbm_expectation_vjp_retained: U right
 * after a qhbm_expectation_retain that kept its states, 0 otherwise (batch larger than one
 * backward chunk, or any compute call since). */
int qhbm_retained_states(qhbm_engine* h, int* out_U);

/* Per-state rows of the last adjoint VJP (qhbm_expectation_vjp with method 0, or
 * qhbm_expectation_vjp_retained) on U states:
 *   d_rows[u, p] = sum_k d_upstream[u, k] * d out[u, k] / d params[p]       [U, n_params] float
 * so that sum_u d_rows[u, :] is that call's d_grad up to the fp32 rounding of each row and of d_grad.  A multi-GPU host gathers the rows of every
 * rank and adds them in global state order: the [P] gradient is then bit-identical for any number
 * of ranks (SURVEY.md 8e "fixed-order summation"); an all-reduce of d_grad is the fast path.  A forward-only
 * qhbm_expectation in between keeps the rows; another VJP, qhbm_expectation_jacobian, qhbm_sample_counts,
 * qhbm_program_vjps and every setter that invalidates a plan (see "model" above) drop them: the call then fails and
 * writes nothing. */
int qhbm_state_gradients(qhbm_engine* h, int U, float* d_rows, void* stream);

/* Full Jacobian d_jac[u, k, p] (tests / small n only; adjoint). */
int qhbm_expectation_jacobian(qhbm_engine* h, const int8_t* d_bits, int U,
                              const float* d_params, float* d_out_vals,
                              float* d_jac, void* stream);

/* Final state vectors C(params)|x_u> (the data behind
 * qhbmlib/inference/qnn_utils.py:23-33 `unitary` (tfq.layers.Unitary) and
 * qhbm_utils.py:24-116 `density_matrix` / `fidelity`).
 *   d_out_states [U, 2^n_qubits] complex64 as interleaved (re, im) floats (device);
 *   amplitude index = the bitstring read as a big-endian binary number (qubit 0 is
 *   the most significant bit, as cirq orders `final_state_vector`), global phase included
 *   (every gate's exp(i*pi*t*global_shift) and the e^{i*pi*t/2} of cirq's X**t / Y**t).
 * Observables need not be installed. */
int qhbm_statevector(qhbm_engine* h, const int8_t* d_bits, int U,
                     const float* d_params, void* d_out_states, void* stream);

/* ---- Circuits that start from caller-supplied states (quantum data) ----
 * Added WITHIN ABI version 5: purely additive, no existing entry point changes, QHBM_ABI_VERSION stays 5.
 *
 *   d_states [U, 2^n_qubits] complex64 as interleaved (re, im) floats (device, 16-byte aligned), the amplitude index
 *   being the bitstring read big-endian: exactly what qhbm_statevector writes.  The buffer is only read, and must not
 *   lie inside the engine's workspace (an error).  The states need not be normalised: the engine normalises its copy
 *   (its values accumulate in fixed point on the premise ||psi|| = 1) and keeps ||phi_u||^2 on the device, so that
 *   every output is the plain quadratic (values, gradients) or linear (states) function of the states AS GIVEN.  A
 *   state of norm 0 gives zeros.
 *
 * The circuit runs on dense-start plans, kept beside the basis-state plans: built on the first such
 * call, cached per gradient mask, invalidated by the same setters; qhbm_plan_builds and qhbm_num_passes keep
 * reporting the basis-state plans.  chunk_states, workspace_budget_mb and profile_events apply as for the bits calls.
 * Each call is "another compute call": it drops the states of qhbm_expectation_retain, and the VJP replaces the rows
 * qhbm_state_gradients serves.
 *
 * OUT OF SCOPE from caller states: the parameter-shift method, the retain / vjp_retained pair, energy tables (a caller
 * reaches them through qhbm_statevector_vjp_from_states below), sampling and qhbm_program_vjps.
 *
 *   qhbm_expectation_from_states       d_out[u, k] = <phi_u| C^dagger O_k C |phi_u>  (not divided by the norm)
 *   qhbm_expectation_vjp_from_states   the adjoint method only: d_grad [n_params] = sum_{u,k} d_upstream[u, k] *
 *                                      d(value[u, k]) / d(params), d_out_vals [U, n_ops] may be NULL; the gradient
 *                                      mask applies as in qhbm_expectation_vjp
 *   qhbm_statevector_from_states       d_out_states [U, 2^n_qubits] = C |phi_u>, global phase as qhbm_statevector
 *                                      (16-byte aligned; observables need not be installed)
 *   qhbm_describe_schedule_from_states the dense-start plans as text; works without a device */
int qhbm_expectation_from_states(qhbm_engine* h, const void* d_states, int U, const float* d_params,
                                 float* d_out, void* stream);
int qhbm_expectation_vjp_from_states(qhbm_engine* h, const void* d_states, int U, const float* d_params,
                                     const float* d_upstream, float* d_out_vals, float* d_grad, void* stream);
int qhbm_statevector_from_states(qhbm_engine* h, const void* d_states, int U, const float* d_params,
                                 void* d_out_states, void* stream);
int qhbm_describe_schedule_from_states(qhbm_engine* h, char* buf, size_t buf_len);

/* ---- Differentiating final states: the adjoint VJP from a caller's cotangent states ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 * The contract is stated on the states qhbm_statevector_from_states returns: psi_u = C(params) phi_u, global phase
 * included, not normalised.  For a real loss L and the cotangent g_u = dL/dRe psi_u + i dL/dIm psi_u (torch's
 * convention for a complex tensor, so that dL = sum_u Re<g_u|dpsi_u>):
 *   d_grad[p] = sum_u Re<g_u| d psi_u / d params[p]>                                   [n_params] float
 * -- the backward sweep on lambda_u = 1/2 ||phi_u|| e^{-i theta} g_u, minus (d theta / d p) sum_u Im<g_u|psi_u> for the
 * global phase theta(params) no kernel applies.  Any real function of the final states is differentiable through it.
 *
 *   d_states, d_cotangent  [U, 2^n_qubits] complex64 in the row order of qhbm_statevector, device, 16-byte aligned, only
 *                          read, outside the engine's workspace (NULL, misaligned or aliasing: refused with a message)
 *   d_out_states           NULL, or [U, 2^n_qubits] complex64 (16-byte aligned, overlapping neither input): receives exactly
 *                          what qhbm_statevector_from_states would have written -- the same forward serves both outputs
 *   d_grad                 [n_params] float, overwritten; U == 0 zero-fills it
 * No observables are needed.  The call runs on the dense-start plans, honours qhbm_set_gradient_mask (masked entries are
 * exactly 0) and chunk_states; no floating-point atomics: two calls give identical bits, whatever chunk_states.  It drops
 * the states of qhbm_expectation_retain, and qhbm_state_gradients is refused after it (its rows would lack the phase term).
 * There is no entry from bitstrings -- the basis-state plans prune leading diagonal gates and idle qubits, which is valid
 * for expectation values and wrong for a phase-sensitive cotangent: basis starts go through this entry as one-hot states.
 * OUT OF SCOPE: the gradient with respect to d_states, the parameter-shift method. */
int qhbm_statevector_vjp_from_states(qhbm_engine* h, const void* d_states, int U, const float* d_params,
                                     const void* d_cotangent, void* d_out_states /* may be NULL */, float* d_grad,
                                     void* stream);

/* ---- Evolving caller-supplied states: matrix-free thermal targets ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 * H = sum_k weights[k] O_k over the INSTALLED observables (qhbm_set_observables); `weights` is a host array of n_ops
 * doubles, NULL = all ones.  R = sum_k |w_k| sum_j |c_kj| >= ||H||.  e^{-tau H} phi and e^{-i tau H} phi are Chebyshev sums
 * in H / R built from repeated launches of the lambda = O psi kernels on device-resident states:
 *   imaginary time  e^{-d H} = e^{d R} [a_0 T_0 + 2 sum_k (-1)^k a_k T_k(H / R)],  a_k = e^{-x} I_k(x),  x = d R
 *   real time       e^{-i d H} = J_0(x) T_0 + 2 sum_k (-i)^k J_k(x) T_k(H / R)
 * tau is split into m = ceil(|tau| R / s) equal steps (engine option "evolve_step_argument" s, default 4, so x <= 4); the
 * coefficients come from Miller's backward recurrence in float64 on the host and the sum is cut where the discarded
 * tail 2 sum |a_k| falls below 2^-30.  In imaginary time the state is renormalised after every step and
 * log ||.|| is accumulated per state in float64 on the device; the factor e^{d R} enters that log norm only.  m and the
 * number of terms depend on (tau, R, mode) alone: nothing is read back, the call is asynchronous on `stream`.
 *
 * State layout, alignment and the rule that the states must not lie inside the workspace: as for
 * qhbm_expectation_from_states.  The circuit may be empty (it is not applied).  Four state buffers per chunk element
 * are cut from workspace_budget_mb / chunk_states.  Results do not depend on the chunking, nor on which other states
 * share the call (no floating-point atomics).  Like every compute call these drop retained states and VJP rows.
 * Refused, each with a message: no observables installed; U <= 0; tau not finite, or tau < 0 in mode 0; d_log_norms
 * given in mode 1; states inside the workspace.  R = 0 is the identity: the states are unchanged and the log norms are
 * log ||phi_u||.
 *
 *   qhbm_apply_observables   d_out_states[u] = H phi_u of the states as given (d_out_states must not overlap d_states)
 *   qhbm_evolve_states       in place.  mode 0: phi_u <- e^{-tau H} phi_u / ||e^{-tau H} phi_u|| (zeros for a state of norm
 *                            0), d_log_norms [U] (device, float64, may be NULL) = log ||e^{-tau H} phi_u|| of the input AS
 *                            GIVEN (-inf for norm 0).  mode 1: phi_u <- e^{-i tau H} phi_u, the norm as given, any sign of
 *                            tau; d_log_norms must be NULL.
 *   qhbm_describe_evolution  "R=... steps=... terms_per_step=... applications=..." of such a call; needs no device
 *   qhbm_random_states       d_states [U, 2^n_qubits] complex64 = random-sign states: for state u = first_state + row and
 *                            the group g = j >> 6 of 64 amplitudes, one Philox4x32-10 call with key (seed low, seed
 *                            high) and counter {g low, g high, u, 0x54505153}; amplitude j takes bits 2 (j & 63) (sign
 *                            of the real part) and 2 (j & 63) + 1 (imaginary part) of the 128 output bits, word index
 *                            first, least significant bit first; each part has magnitude float(2^{-(n + 1) / 2}), so
 *                            ||r|| = 1 and E[|r><r|] = I / 2^n.  No engine: the current device. */
int qhbm_apply_observables(qhbm_engine* h, const void* d_states, int U, const double* weights, void* d_out_states,
                           void* stream);
int qhbm_evolve_states(qhbm_engine* h, void* d_states, int U, const double* weights, double tau, int mode,
                       double* d_log_norms, void* stream);
int qhbm_describe_evolution(qhbm_engine* h, const double* weights, double tau, int mode, char* buf, size_t len);
int qhbm_random_states(void* d_states, int U, int n_qubits, uint64_t seed, uint64_t first_state, void* stream);

/* ---- Krylov spaces of caller-supplied states: ground states, spectra, whole beta ladders ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 * H, `weights` and R as for qhbm_evolve_states.  Per start state phi the Lanczos recurrence, j = 0 .. m - 1:
 *   v_0 = phi / ||phi||;  w = H v_j;  per round c_i = <v_i, w> for i in [lo, j] (float64 sums), then
 *   w <- w - sum_i c_i v_i, i ascending, c_i rounded to complex64;  alpha_j = sum over rounds of Re c_j;
 *   beta_j = ||w|| (float64);  v_{j+1} = w / beta_j.
 * reorth = 1: lo = 0 and two rounds (full reorthogonalisation, classical Gram-Schmidt twice); reorth = 0: lo = max(0, j - 1)
 * and one round (local).  beta_j <= 2^-16 R: the space is exhausted -- length = j + 1, beta_j = 0, every later alpha and
 * beta is 0 and every later basis row is exact zeros; otherwise length = m.  beta_{m-1} is stored although v_m is not
 * (residuals need it).  A start state of norm 0 has length 0 and an all-zero basis.  T = tridiag(alpha[:length],
 * beta[:length - 1]) then holds what the space knows of H: V e^{-tau T} e_1 ||phi|| ~ e^{-tau H} phi for every tau at once.
 *
 *   qhbm_krylov_basis     d_basis [m, U, 2^n] complex64, STEP-MAJOR and caller-owned (row j of consecutive states is
 *                         contiguous); d_alpha, d_beta [U, m] float64; d_lengths [U] int32; all on the device.  Asynchronous
 *                         on `stream`, nothing is read back: the breakdown decision lives on the device.  Two state buffers
 *                         per chunk element are cut from workspace_budget_mb / chunk_states; results do not depend on the
 *                         chunking nor on which other states share the call (no floating-point atomics).  Refused, each with
 *                         a message: m outside [1, 1024]; reorth not 0 or 1; U <= 0; no observables installed; a NULL or
 *                         misaligned pointer (states 16 bytes); the basis or the start states inside the workspace; the
 *                         basis overlapping the start states.
 *   qhbm_krylov_combine   d_out_states[u, s] = sum_j d_coef[u, s, j] d_basis[j, u], j ascending in fp32; d_coef [U, S, m]
 *                         complex64, d_out_states [U, S, 2^n_qubits].  No engine: the current device.  Refused: S < 1, m
 *                         outside [1, 1024], U <= 0, a NULL or misaligned pointer.
 *   qhbm_describe_krylov  "basis_bytes=... workspace_bytes=... applications=... chunk_states=... krylov_bytes_per_state=..."
 *                         of such a call: the bytes the project / subtract / normalise kernels and the import move per
 *                         state by the model of DESIGN.md 6h; needs no device */
int qhbm_krylov_basis(qhbm_engine* h, const void* d_start_states, int U, const double* weights, int m, int reorth,
                      void* d_basis, double* d_alpha, double* d_beta, int32_t* d_lengths, void* stream);
int qhbm_krylov_combine(const void* d_basis, int m, int U, int n_qubits, const void* d_coef, int S, void* d_out_states,
                        void* stream);
int qhbm_describe_krylov(qhbm_engine* h, int U, int m, int reorth, char* buf, size_t len);

/* ---- Streamed Lanczos: the same results without a stored basis, in two passes ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 * H, `weights`, R, the breakdown threshold 2^-16 R and the conventions of qhbm_krylov_basis.  The basis of m rows is
 * replaced by a ring of three state buffers per chunk element in engine-owned memory (at the workspace's pitch), so the
 * memory of a call does not grow with m.  Full reorthogonalisation needs the stored basis and is not offered here.
 *
 *   qhbm_krylov_tridiagonal  pass one: the recurrence of qhbm_krylov_basis(reorth = 0).  d_alpha, d_beta [U, m] float64 and
 *                            d_lengths [U] int32 are, bit for bit, what that call writes.  d_recurrence [U, m, 2] complex64:
 *                            the complex64-rounded coefficients (c_{j-1}, c_j) step j subtracted, (0, c_0) for j = 0 -- with
 *                            beta all a replay needs: v_{j+1} = (H v_j - c_{j-1} v_{j-1} - c_j v_j) / beta_j.
 *   qhbm_krylov_replay       pass two: d_out_states[u, s] = sum_j d_coef[u, s, j] v_j(u), j ascending in fp32; d_coef
 *                            [U, S, m] complex64, d_out_states [U, S, 2^n] (the layout of qhbm_krylov_combine).  v_0 is
 *                            imported again from d_start_states, which the caller has left unchanged, and every later v_j is
 *                            regenerated from d_beta and d_recurrence with NO inner products: bit for bit the row the stored
 *                            route would hold.  The scale of step j is 1 / beta_j, 0 where beta_j = 0 (an exhausted space, a
 *                            start state of norm 0): exact zeros from there on.  S > 8 runs the recurrence once per group of
 *                            eight outputs.  d_lengths is checked like the other pointers; the kernels do not read it.
 *   qhbm_describe_krylov_stream  "workspace_bytes=... chunk_states=... tridiagonal_applications=... replay_applications=...
 *                            tridiagonal_bytes_per_state=... replay_bytes_per_state=..." of such a pair of calls by the byte
 *                            model of DESIGN.md 6o; workspace_bytes does not depend on m; needs no device.
 * Both passes are asynchronous on `stream` and read nothing back; results do not depend on the chunking nor on which other
 * states share the call.  Refused, each with a message and every buffer untouched: m outside [1, 1024]; U <= 0; S < 1; no
 * observables installed; a NULL or misaligned pointer (states 16 bytes, the rest their element size); start states or
 * outputs inside the engine's workspace; outputs overlapping the start states. */
int qhbm_krylov_tridiagonal(qhbm_engine* h, const void* d_start_states, int U, const double* weights, int m, double* d_alpha,
                            double* d_beta, int32_t* d_lengths, void* d_recurrence, void* stream);
int qhbm_krylov_replay(qhbm_engine* h, const void* d_start_states, int U, const double* weights, int m, const double* d_beta,
                       const int32_t* d_lengths, const void* d_recurrence, const void* d_coef, int S, void* d_out_states,
                       void* stream);
int qhbm_describe_krylov_stream(qhbm_engine* h, int U, int m, int S, char* buf, size_t len);

/* ---- The weighted Gram matrix of M states: fidelity, entropy and relative entropy of state-vector data ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 *   G[i, j] = sum_x t(x) conj(s_i(x)) s_j(x)
 * for M states s_i of 2^n_qubits amplitudes and a real table t over the bitstrings.  With a_m = U^dagger phi_m and
 * sigma = sum_m w_m |phi_m><phi_m|, W = diag(w): tr(rho sigma) = sum_m w_m G_p[m, m]; the fidelity is (sum_i sqrt(lambda_i))^2
 * over the spectrum of W^1/2 G_p W^1/2; tr sigma, tr sigma^2, S(sigma) come from the spectrum of W^1/2 G_1 W^1/2; the cross
 * entropy is sum_m w_m G_E[m, m] + log Z.
 *
 *   qhbm_weighted_gram       d_states [M, 2^n_qubits] complex64, interleaved, 16-byte aligned; d_table [2^n_qubits] float32,
 *                            8-byte aligned, indexed like the amplitudes, or NULL for t = 1; d_gram [M, M, 2] float64
 *                            (re, im), row-major; all on the device.  No engine: the current device.  Asynchronous on
 *                            `stream`; allocates nothing, synchronises nothing.  d_scratch: qhbm_gram_scratch_bytes bytes,
 *                            8-byte aligned, which may hold anything (every partial that is read is written first).
 *                            Order of additions: a product is float x float in float64 (exact), the column operand s_j
 *                            times t first (exact); a thread adds its words in word order with fused multiply-adds, the 64
 *                            lanes of a wave meet in a fixed shuffle tree, the waves add in wave order and the slices in
 *                            slice order in a second kernel; no floating-point atomics.  The slices depend on n_qubits
 *                            alone, so G[i, j] depends neither on M nor on which other states share the call.  Only
 *                            j >= i is summed: G[j, i] is written as the conjugate of G[i, j] and Im G[i, i] as 0.
 *                            Refused, each with a message and before anything is launched: M outside [1, 1024]; n_qubits
 *                            outside [1, 31]; d_states, d_scratch or d_gram NULL; a misaligned pointer.
 *   qhbm_gram_scratch_bytes  *out = the bytes of d_scratch such a call needs: 16 M^2 min(2^n_qubits / 2048, 256), at least
 *                            16 M^2; needs no device.  Refused: M or n_qubits as above, out NULL. */
int qhbm_gram_scratch_bytes(int M, int n_qubits, size_t* out);
int qhbm_weighted_gram(const void* d_states, int M, int n_qubits, const float* d_table, void* d_scratch, double* d_gram,
                       void* stream);

/* ---- Reduced density matrices: the partial trace of a state ensemble ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 *   rho_A[a, a'] = sum_m w_m sum_b phi_m(a, b) conj(phi_m(a', b))
 * for M states phi_m of 2^n_qubits amplitudes and a subset A of k kept qubits.  keep_mask is in QUBIT space (bit q set <=>
 * qubit q is kept; qubit 0 is the most significant bit of an amplitude index); row index a is the kept qubits' bits read
 * big-endian in ascending qubit order, b the same for the other qubits.
 *
 *   qhbm_reduced_density     d_states [M, 2^n_qubits] complex64, interleaved, 16-byte aligned; d_weights [M] float64, or
 *                            NULL for all ones; d_rho [2^k, 2^k, 2] float64 (re, im), row-major; all on the device.  No
 *                            engine: the current device.  Asynchronous on `stream`; allocates nothing, synchronises
 *                            nothing.  d_scratch: qhbm_reduced_density_scratch_bytes bytes, 8-byte aligned, which may hold
 *                            anything (every partial that is read is written first).  k = n_qubits is allowed: the
 *                            environment is empty and rho = sum_m w_m |phi_m><phi_m|.
 *                            Order of additions: a product is float x float in float64 (exact); the column operand
 *                            phi_m(a', b) is multiplied by w_m first (one rounding per amplitude); a thread adds its
 *                            environment values in ascending (m, b) order with fused multiply-adds, the threads that
 *                            share an output meet in a fixed shuffle tree, then in wave order, and the slices add in
 *                            slice order in a second kernel; no floating-point atomics.  The grid depends on
 *                            (n_qubits, keep_mask, M) alone: two calls give the same bits.  Only a' >= a is summed:
 *                            rho[a', a] is written as the conjugate of rho[a, a'] and Im rho[a, a] as 0.
 *                            Refused, each with a message and before anything is launched: M outside [1, 65536];
 *                            n_qubits outside [1, 31]; a keep_mask bit at or above n_qubits; k outside
 *                            [1, min(n_qubits, 10)]; d_states, d_scratch or d_rho NULL; a misaligned pointer.
 *   qhbm_reduced_density_scratch_bytes  *out = the bytes of d_scratch such a call needs (csrc/rdm_index.h rdm_plan: 16
 *                            bytes per tile entry, upper-triangle tile and slice); needs no device.  Refused: the shape
 *                            as above, out NULL. */
int qhbm_reduced_density_scratch_bytes(int M, int n_qubits, uint64_t keep_mask, size_t* out);
int qhbm_reduced_density(const void* d_states, int M, int n_qubits, uint64_t keep_mask, const double* d_weights,
                         void* d_scratch, double* d_rho, void* stream);

/* ---- A dense operator on k arbitrary qubits of every state: the VJP of the reduced density matrix ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 *   out_m = scale_m (A (x) 1_env) phi_m,     dots_m = <phi_m|(A (x) 1_env)|phi_m>   (taken before scaling)
 * keep_mask, the row order of A and the limits are those of qhbm_reduced_density: A acts on the kept qubits read
 * big-endian in ascending qubit order, 1 <= k <= min(n_qubits, 10), n_qubits <= 31, M <= 65536, k = n_qubits allowed.  For a
 * real loss L of rho_A with cotangent Gamma = dL/dRe rho + i dL/dIm rho, A = Gamma + Gamma^H and scale = the weights give
 * the cotangent of the states in `out` and 1/2 Re dots is the cotangent of the weights.
 *
 *   qhbm_subsystem_apply     d_states, d_out [M, 2^n_qubits] complex64, interleaved, 16-byte aligned, not overlapping;
 *                            d_operator [2^k, 2^k] complex64, row-major, 8-byte aligned; d_scale [M] float64 or NULL for
 *                            all ones; d_dots [M, 2] float64 (re, im) or NULL; all on the device.  No engine: the current
 *                            device.  Asynchronous on `stream`; allocates nothing, synchronises nothing.  d_scratch:
 *                            qhbm_subsystem_apply_scratch_bytes bytes, 8-byte aligned, which may hold anything.
 *                            Arithmetic: an output is an f32 fused-multiply-add chain over a' ascending of the real
 *                            embedding Re = A_r phi_r - A_i phi_i, Im = A_r phi_i + A_i phi_r (k <= 3 vector code, k >= 4
 *                            v_mfma_f32_16x16x4_f32, which is such a chain bit for bit), times scale_m in float64, rounded
 *                            once.  dots: conj(phi) times the unscaled f32 output, float x float in float64 (exact); a
 *                            thread adds its elements in row order, the lanes of a wave meet in a fixed shuffle tree, the
 *                            waves in wave order, the workgroups of a state in order in a second kernel; no
 *                            floating-point atomics.  The grid depends on (n_qubits, keep_mask, M) alone: two calls give
 *                            the same bits in d_out and d_dots.
 *                            Refused, each with a message and before anything is launched: the shapes
 *                            qhbm_reduced_density refuses; d_states, d_operator, d_out or d_scratch NULL; a misaligned
 *                            pointer; d_out overlapping d_states.
 *   qhbm_subsystem_apply_scratch_bytes  *out = the bytes of d_scratch such a call needs (csrc/subsystem_plan.h sub_plan: the
 *                            transposed operator, 8 * 4^k bytes from k = 4 on, and 16 bytes per state and workgroup of
 *                            it); needs no device.  Refused: the shape as above, out NULL. */
int qhbm_subsystem_apply_scratch_bytes(int M, int n_qubits, uint64_t keep_mask, size_t* out);
int qhbm_subsystem_apply(const void* d_states, int M, int n_qubits, uint64_t keep_mask, const void* d_operator,
                         const double* d_scale, void* d_out, double* d_dots, void* d_scratch, void* stream);

/* ---- The VJP of the weighted Gram matrix: state metrics as losses ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 *   c_j(x) = sum_i H[i, j] a_i(x),    out_j(x) = t(x) c_j(x),    table_grad(x) = 1/2 sum_j Re(conj(c_j(x)) a_j(x))
 * for the M states a_i and the table t of qhbm_weighted_gram.  For a real loss L of G with cotangent
 * Gamma = dL/dRe G + i dL/dIm G, H = Gamma + Gamma^H gives the cotangent of the states in `out` and that of the table in
 * `table_grad`.  H is used as given: the call does not symmetrise it.
 *
 *   qhbm_weighted_gram_vjp   d_states, d_out_states [M, 2^n_qubits] complex64, interleaved, 16-byte aligned, not
 *                            overlapping; d_table [2^n_qubits] float32, 8-byte aligned, or NULL for t = 1 (out = c);
 *                            d_cotangent = H, [M, M] complex64, row-major, 8-byte aligned; d_table_grad [2^n_qubits]
 *                            float64; all on the device.  Either of d_out_states and d_table_grad may be NULL and is then
 *                            not computed; the other's bits do not change.  No engine: the current device.  Asynchronous
 *                            on `stream`; allocates nothing, synchronises nothing.  d_scratch:
 *                            qhbm_gram_vjp_scratch_bytes bytes, 8-byte aligned, which may hold anything.
 *                            Arithmetic: c_j(x) is an f32 fused-multiply-add chain over i ascending of the real embedding
 *                            Re = H_r a_r - H_i a_i, Im = H_r a_i + H_i a_r (M <= 8 vector code, M >= 9
 *                            v_mfma_f32_16x16x4_f32, which is such a chain bit for bit); out = t c, one rounding per
 *                            part.  table_grad: the unscaled c times a, float x float in float64 (exact), Re then Im,
 *                            j ascending in one accumulator, halved at the end; one workgroup finishes an x, so there
 *                            are no partials and no floating-point atomics: two calls give the same bits.
 *                            Refused, each with a message and before anything is launched: the shapes qhbm_weighted_gram
 *                            refuses; d_states, d_cotangent or d_scratch NULL; d_out_states and d_table_grad both NULL;
 *                            a misaligned pointer; d_out_states overlapping d_states.
 *   qhbm_gram_vjp_scratch_bytes  *out = the bytes of d_scratch such a call needs (csrc/gram_vjp_plan.h gv_plan: 16 for
 *                            M <= 8, where none is used; above, H as two zero-padded float planes, 8 P^2 bytes with
 *                            P = 16 ceil(M / 16) up to 64 and 64 ceil(M / 64) beyond); needs no device.  Refused: M or
 *                            n_qubits as above, out NULL. */
int qhbm_gram_vjp_scratch_bytes(int M, int n_qubits, size_t* out);
int qhbm_weighted_gram_vjp(const void* d_states, int M, int n_qubits, const float* d_table, const void* d_cotangent,
                           void* d_out_states, double* d_table_grad, void* d_scratch, void* stream);

/* ---- The cross-Gram matrix of two ensembles: overlap, fidelity and trace distance of state ensembles ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 *   C[i, j] = sum_x t(x) conj(a_i(x)) b_j(x)
 * for M bras a_i and K kets b_j of 2^n_qubits amplitudes, in two buffers, and a real table t over the bitstrings.  For
 * sigma = sum_m w_m |a_m><a_m| and tau = sum_k v_k |b_k><b_k|, X = W^1/2 C V^1/2 with t = 1: tr(sigma tau) = ||X||_F^2; the
 * Uhlmann fidelity is (sum of the singular values of X)^2; the non-zero spectrum of sigma - tau is that of J Gamma, Gamma
 * the Gram matrix of the M + K scaled states (blocks G_A, X, X^H, G_B; the diagonal blocks from qhbm_weighted_gram) and
 * J = diag(1_M, -1_K).
 *
 *   qhbm_cross_gram          d_bras [M, 2^n_qubits] and d_kets [K, 2^n_qubits] complex64, interleaved, 16-byte aligned; both
 *                            are only read and may alias or overlap; d_table [2^n_qubits] float32, 8-byte aligned, indexed
 *                            like the amplitudes, or NULL for t = 1; d_out [M, K, 2] float64 (re, im), row-major; all on
 *                            the device.  No engine: the current device.  Asynchronous on `stream`; allocates nothing,
 *                            synchronises nothing.  d_scratch: qhbm_cross_gram_scratch_bytes bytes, 8-byte aligned, which
 *                            may hold anything (every partial that is read is written first).
 *                            Order of additions: qhbm_weighted_gram's own.  A product is float x float in float64 (exact),
 *                            the column operand b_j times t first (exact); a thread adds its words in word order with
 *                            the same eight fused multiply-adds per word and pair, the 64 lanes of a wave meet in the
 *                            same shuffle tree, the waves add in wave order and the slices in slice order in a second
 *                            kernel; no floating-point atomics.  The slices are qhbm_weighted_gram's and depend on
 *                            n_qubits alone, so C[i, j] depends neither on M, nor on K, nor on which other states share
 *                            the call, and two calls give the same bits.  Every (i, j) is summed on its own: nothing is
 *                            mirrored, nothing is forced to zero.
 *                            Equality with qhbm_weighted_gram: with d_bras == d_kets (and M == K) C[i, j] has the bits of
 *                            G[i, j] for j > i, both parts, and Re C[i, i] those of Re G[i, i]; Im C[i, i] is what the
 *                            roundings leave (G writes 0) and C[j, i] for j > i is conj(G[i, j]) within the bound only.
 *                            Error, per part and to first order: |dC[i, j]| <= 2 (2^n_qubits + 4) 2^-53
 *                            sum_x |t| |a_i| |b_j|.
 *                            Refused, each with a message and before anything is launched: M or K outside [1, 1024];
 *                            n_qubits outside [1, 31]; d_bras, d_kets, d_scratch or d_out NULL; a misaligned pointer
 *                            (states 16 bytes; table, scratch and out 8).
 *   qhbm_cross_gram_scratch_bytes  *out = the bytes of d_scratch such a call needs: 16 M K min(2^n_qubits / 2048, 256), at
 *                            least 16 M K; needs no device.  Refused: M, K or n_qubits as above, out NULL. */
int qhbm_cross_gram_scratch_bytes(int M, int K, int n_qubits, size_t* out);
int qhbm_cross_gram(const void* d_bras, int M, const void* d_kets, int K, int n_qubits, const float* d_table, void* d_scratch,
                    double* d_out, void* stream);

/* ---- The VJP of the cross-Gram matrix: two-ensemble metrics as losses ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 * For a real loss L of C = qhbm_cross_gram's matrix with cotangent Gamma = dL/dRe C + i dL/dIm C, [M, K]
 * (dL = Re sum conj(Gamma[i, j]) dC[i, j]), and c_j(x) = sum_i Gamma[i, j] a_i(x):
 *   out_kets_j(x) = t(x) c_j(x)       out_bras_i(x) = t(x) sum_j conj(Gamma[i, j]) b_j(x)       table_grad(x) = sum_j Re(conj(c_j(x)) b_j(x))
 * -- the cotangents of the kets, of the bras and of the table.  Gamma is used as given: nothing is symmetrised, so there is
 * no factor 1/2 in table_grad.
 *
 *   qhbm_cross_gram_vjp      d_bras, d_out_bras [M, 2^n_qubits] and d_kets, d_out_kets [K, 2^n_qubits] complex64,
 *                            interleaved, 16-byte aligned; d_table [2^n_qubits] float32, 8-byte aligned, or NULL for t = 1;
 *                            d_cotangent = Gamma, [M, K] complex64, row-major, 8-byte aligned; d_table_grad [2^n_qubits]
 *                            float64; all on the device.  Each of d_out_bras, d_out_kets and d_table_grad may be NULL and is
 *                            then not computed; the others' bits do not change.  d_bras and d_kets are only read and may
 *                            alias or overlap each other.  No engine: the current device.  Asynchronous on `stream`;
 *                            allocates nothing, synchronises nothing.  d_scratch: qhbm_cross_gram_vjp_scratch_bytes bytes,
 *                            8-byte aligned, which may hold anything.
 *                            Each state output is one sweep out_s(x) = t(x) sum_r W[r, s] src_r(x): for the kets src = bras
 *                            and W = Gamma, for the bras src = kets and W[r, s] = conj(Gamma[s, r]).  The sum is an f32
 *                            fused-multiply-add chain over r ascending of the real embedding Re = W_r s_r - W_i s_i,
 *                            Im = W_r s_i + W_i s_r (up to 8 source rows vector code, from 9 on v_mfma_f32_16x16x4_f32,
 *                            which is such a chain bit for bit; the switch looks at the SOURCE side's row count only);
 *                            out = t times it, one rounding per part.  table_grad: the unscaled c times b, float x float
 *                            in float64 (exact), Re then Im, j ascending in one accumulator; one workgroup finishes an x,
 *                            so there are no partials and no floating-point atomics: two calls give the same bits.
 *                            Error, per part: |d out_s(x)| <= (2 R + 4) 2^-24 |t(x)| sum_r (|Re W_rs| + |Im W_rs|)
 *                            (|Re src_r(x)| + |Im src_r(x)|), R the number of source rows.
 *                            Refused, each with a message and before anything is launched: the shapes qhbm_cross_gram
 *                            refuses; d_bras, d_kets, d_cotangent or d_scratch NULL; all three outputs NULL; a misaligned
 *                            pointer (states and state outputs 16 bytes, the rest 8); a state output overlapping either
 *                            input or the other state output.
 *   qhbm_cross_gram_vjp_scratch_bytes  *out = the bytes of d_scratch such a call needs (csrc/cross_gram_vjp_plan.h
 *                            cgv_plan): per side with 9 or more source rows, W as two zero-padded float planes of
 *                            16 ceil(R / 16) x Ps floats, Ps = 16 ceil(S / 16) up to 64 and 64 ceil(S / 64) beyond; at
 *                            least 16, never 0; needs no device.  Refused: M, K or n_qubits as above, out NULL. */
int qhbm_cross_gram_vjp_scratch_bytes(int M, int K, int n_qubits, size_t* out);
int qhbm_cross_gram_vjp(const void* d_bras, int M, const void* d_kets, int K, int n_qubits, const float* d_table,
                        const void* d_cotangent, void* d_out_bras, void* d_out_kets, double* d_table_grad, void* d_scratch,
                        void* stream);

/* Computational-basis samples of the final states (tfq.layers.Sample as used at
 * qhbmlib/inference/qnn.py:169,177-181,286-291):
 *   d_out_samples [U, n_shots, n_qubits] int8 (device); shot j of state u is drawn from
 *   |<x|C(params)|x_u>|^2 with a counter-based generator keyed by (seed, u, j), so a call is
 *   reproducible and independent of chunking.
 * shift_gate >= 0 adds `shift` to the exponent of that gate of the installed circuit: one
 * program of tfq.differentiators.ParameterShift.get_gradient_circuits (qnn.py:192-199);
 * pass -1, 0.0 for the unshifted circuit. */
int qhbm_sample(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                int n_shots, uint64_t seed, int shift_gate, double shift,
                int8_t* d_out_samples, void* stream);

/* Shot COUNTS of several parameter-shifted programs in one launch set -- what the sampled
 * estimators reduce their shots to (qnn.py:170-226: tfq.layers.SampledExpectation with the
 * ParameterShift differentiator samples 2 programs per gate occurrence; a Pauli-string estimate is a
 * signed sum of the counts, a BitstringEnergy average a weighted one):
 *   d_out_counts [n_programs, U, 2^n_qubits] int32 (device): how many of the n_shots shots of
 *   C_q(params)|x_u> gave outcome x (index = the bitstring read big-endian, as qhbm_statevector);
 *   program q is the installed circuit with `shifts[q]` added to the exponent of gate
 *   `shift_gates[q]` (HOST arrays of n_programs entries; gate < 0 = the unshifted circuit).
 * Shot j of (q, u) is drawn with a counter-based generator keyed by (seed, q, u, j): a call is
 * reproducible and independent of how the engine cuts the (program, state) pairs into launch sets.
 * n_qubits <= 24 (one counter per outcome); larger registers use qhbm_sample per program. */
int qhbm_sample_counts(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                       int n_programs, const int32_t* shift_gates, const float* shifts,
                       int n_shots, uint64_t seed, int32_t* d_out_counts, void* stream);

/* ---- Pauli-string estimates from shots, at any register width ----
 * Added WITHIN ABI version 5: purely additive, QHBM_ABI_VERSION stays 5.
 *
 * A Pauli-Z-string estimate needs neither the shots nor a counter per outcome, only T integers per (program, state):
 *   out[q, s, t] = sum_{j < n_shots} (-1)^popcount(x_j & m_t)                                   int32
 * THE DRAW.  For element (program q, state row s) and shot j:
 *   uniform   exactly that of qhbm_sample_counts: Philox4x32-10, counter {j, s, 0x51b0c6a1, q}, key (seed low, seed high),
 *             u = c0 2^-32 + c1 2^-64 in float64;
 *   mass      p(x) = re^2 + im^2 of the complex64 amplitude in float64: both products exact, one rounding in the sum;
 *   outcome   the first x whose inclusive prefix sum_{y <= x} p(y) exceeds u * total (one float64 multiply; total = sum p as
 *             the kernel sums it).  Every sum is float64 in this fixed order: a sub-block of 16 consecutive amplitudes is
 *             added in index order; the 64 sub-block masses of a block of 1024 amplitudes meet in a Hillis-Steele scan
 *             (offsets 1, 2, 4, ..., 32); the block masses meet in the scan of qhbm_sample (256 at a time, offsets 1 .. 128,
 *             a running carry).  The shot takes the first block whose prefix exceeds v = u * total, subtracts the prefix of
 *             the blocks before it, takes the first sub-block of that block whose prefix exceeds the rest r, and the first
 *             amplitude at which (prefix of the sub-blocks before) + p_0 + p_1 + ... exceeds r.  There is no fp32 step.
 *             An outcome of zero mass is never drawn: where no prefix exceeds (u can round to 1), or where a scanned and a
 *             sequential prefix differ in the last place, the shot takes the last outcome of non-zero mass at or before
 *             the place the search reached.  A state of total 0 (or not > 0) draws nothing and its sums are 0.  For states
 *             whose partial sums are all exact in float64 this is searchsorted(cumsum(p), u * total, side = "right"),
 *             clamped to the last outcome of non-zero mass, whatever the order of additions;
 *   masks     `masks` is a HOST array of T uint64 in QUBIT space, as keep_mask of qhbm_reduced_density: bit k set <=> qubit
 *             k, and qubit 0 is the most significant bit of the amplitude index.  Mask 0 gives +n_shots.  (Host, like
 *             shift_gates: a mask bit at or above n_qubits is refused before anything is launched, and the words reach the
 *             device as kernel arguments -- no copy, nothing to synchronise with.)
 * Integer atomics only: the result is bit-reproducible and independent of chunking, of launch-set cuts and of the order in
 * which shots are processed.  Limits: 1 <= T <= 1024, 0 <= n_shots <= 2^31 - 1, n_qubits <= 31.
 *
 *   qhbm_sample_parities         d_out [n_programs, U, T] int32 (device, overwritten).  Programs and their validation exactly
 *                                as in qhbm_sample_counts (HOST shift_gates / shifts; gate < 0 = the unshifted circuit; a
 *                                shifted constant-exponent gate is refused).  The prefix tables (1/16 of a state) are engine
 *                                owned and count against workspace_budget_mb when the launch sets are cut.  No limit on
 *                                n_qubits beyond the engine's; idle padding qubits are the high index bits and stay |0>.
 *   qhbm_sample_parities_states  d_states [M, 2^n_qubits] complex64, 16-byte aligned, only read, need not be normalised;
 *                                d_out [M, T] int32 (overwritten).  Counter words: s = first_row + m, q = program.  No
 *                                engine: the current device.  Asynchronous on `stream`; allocates nothing, synchronises
 *                                nothing.  d_scratch: qhbm_sample_parities_scratch_bytes bytes, 8-byte aligned, which may
 *                                hold anything.  Refused, each with a message and before anything is launched: M <= 0;
 *                                n_qubits outside [1, 31]; T outside [1, 1024]; n_shots negative or above 2^31 - 1; masks,
 *                                d_states, d_scratch or d_out NULL; a misaligned pointer; a mask bit at or above n_qubits;
 *                                first_row + M above 2^32.
 *   qhbm_sample_parities_scratch_bytes  *out = 4096 + 8 min(M, 65535) (2^max(n - 10, 0) + 2^max(n - 4, 0)); needs no device.
 *                                Refused: the shape and the shot count as above, out NULL. */
int qhbm_sample_parities(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params, int n_programs,
                         const int32_t* shift_gates, const float* shifts, const uint64_t* masks, int T, int64_t n_shots,
                         uint64_t seed, int32_t* d_out, void* stream);
int qhbm_sample_parities_scratch_bytes(int M, int n_qubits, int64_t n_shots, size_t* out);
int qhbm_sample_parities_states(const void* d_states, int M, int n_qubits, const uint64_t* masks, int T, int64_t n_shots,
                                uint64_t seed, uint64_t first_row, uint32_t program, void* d_scratch, int32_t* d_out,
                                void* stream);

/* One adjoint VJP per parameter-shifted program, all programs in one launch set -- the rows of the BKM information
 * matrix of a QHBM (baselines/train.py:161-249: every circuit variable shifted by +-1/2, a full gradient per shifted
 * expectation).  Program q is the installed circuit with `shifts[q]` added to the exponent of gate `shift_gates[q]`
 * (HOST arrays of n_programs entries; gate < 0 = the unshifted circuit), as in qhbm_sample_counts:
 *   d_prog_grad [n_programs, n_params] float (device):  d_prog_grad[q, p] = sum_{u,k} d_upstream[u,k] * d out_q[u,k] / d params[p]
 *       (entries of parameters frozen by qhbm_set_gradient_mask are 0; a shift may target a frozen parameter's gate)
 *   d_prog_vals [n_programs, n_ops]   float (device, may be NULL):  d_prog_vals[q, k] = sum_u row_weights[u] * out_q[u,k]
 *   d_upstream [U, n_ops] float, d_row_weights [U] float or NULL (= 1).
 * States are added in state order in fp64 and no atomics are used: the outputs do not depend on chunk_states or
 * shift_prefix_sharing, and a program with shift_gates[q] < 0 returns the d_grad of qhbm_expectation_vjp(method 0)
 * bit for bit.  Errors: a gate index out of range, a shifted ISWAPPOW gate (no two-term rule), n_programs < 0, no
 * observables installed. */
int qhbm_program_vjps(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                      int n_programs, const int32_t* shift_gates, const float* shifts,
                      const float* d_upstream, const float* d_row_weights,
                      float* d_prog_vals, float* d_prog_grad, void* stream);

/* A diagonal observable given as a TABLE of energies, E = sum_y d_table[y] |y><y| -- the modular Hamiltonian of a general
 * BitstringEnergy (an MLP on the bits; qhbmlib/models/energy.py), which is no Pauli sum:
 *   d_table [2^n_qubits] float (device), indexed like qhbm_statevector (the bitstring read big-endian, qubit 0 most
 *   significant); d_out[u] = <x_u| C^dagger E C |x_u> = sum_y d_table[y] |<y|C|x_u>|^2      [U] float (device)
 * No observables need be installed (as for qhbm_statevector): the forward runs the lean, measurement-free passes and
 * one streaming pass of the table kernel over the final states.  The _retain form leaves the final states in the
 * workspace, as qhbm_expectation_retain does, for one qhbm_table_expectation_vjp_retained. */
int qhbm_table_expectation(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                           const float* d_table, float* d_out, void* stream);
int qhbm_table_expectation_retain(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                                  const float* d_table, float* d_out, void* stream);
/* Values plus one vector-Jacobian product of the table expectation:
 *   d_grad[p] = sum_u d_upstream[u] * d out[u] / d params[p]            [n_params] float (overwritten; the gradient mask
 *                                                                       of qhbm_set_gradient_mask applies as in qhbm_expectation_vjp)
 *   d_table_grad[y] = sum_u d_upstream[u] |<y|C|x_u>|^2                  [2^n_qubits] float (overwritten), NULL = not wanted
 *   d_out_vals [U] float, may be NULL.
 * lambda = upstream E psi, then the adjoint sweep.  Values, d_grad and d_table_grad are summed in fp64 in an order fixed by
 * the state index, with no atomics: bit-identical for any chunk_states.  The _retained form runs on the states a
 * qhbm_table_expectation_retain kept (same bits, params and table) and consumes them; it fails if nothing suitable is
 * retained -- any other compute call drops the states -- and the caller falls back to qhbm_table_expectation_vjp.
 * Errors: d_table NULL, U < 0. */
int qhbm_table_expectation_vjp(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                               const float* d_table, const float* d_upstream, float* d_out_vals,
                               float* d_grad, float* d_table_grad, void* stream);
int qhbm_table_expectation_vjp_retained(qhbm_engine* h, const int8_t* d_bits, int U, const float* d_params,
                                        const float* d_table, const float* d_upstream, float* d_grad,
                                        float* d_table_grad, void* stream);

/* ---- EBM side -------------------------------------------- */
/* Spin-parity energies of bitstrings on the current HIP device (no engine handle):
 *   d_energy[i] = sum_k d_thetas[k] * prod_{q in S_k} (1 - 2 x_i[q]),  S_k = set bits of d_masks[k]
 * over the COLUMNS of d_bits [n_rows, n_bits] int8.  This is BernoulliEnergy / KOBE
 * (qhbmlib/models/energy.py:123-209: SpinsFromBitstrings -> Parity -> VariableDot,
 * energy_utils.py:39-110) as one kernel; qhbmlib/inference/ebm.py:458-461 evaluates it over
 * all 2^n bitstrings after every variable update. */
int qhbm_parity_energy(const int8_t* d_bits, int64_t n_rows, int n_bits,
                       const uint64_t* d_masks, const float* d_thetas, int n_terms,
                       float* d_energy, void* stream);
/* Its VJP with respect to thetas: d_grad[k] = sum_i d_weights[i] * parity_k(x_i) (overwritten), summed in fp64
 * in a fixed order: bit-identical from call to call. */
int qhbm_parity_energy_vjp(const int8_t* d_bits, int64_t n_rows, int n_bits,
                           const uint64_t* d_masks, int n_terms, const float* d_weights,
                           float* d_grad, void* stream);

/* Gibbs-With-Gradients chains (qhbmlib/inference/ebm.py:564-760) of the same energies, entirely on the device
 * (DESIGN.md 6d).  The energy is multilinear in x, so the sampler's first-order estimate is exact:
 *   h_j(x) = (E(x) - E(x ^ e_j)) / 2 = sum_{k : j in S_k} d_thetas[k] * parity_k(x),   L(x) = logsumexp_j h_j(x);
 * a step proposes bit i with probability exp(h_i(x) - L(x)) and accepts the flip with probability
 * min(1, exp(L(x) - L(x ^ e_i))), the reference's exp(E(x) - E(x')) q(i|x') / q(i|x).
 * d_chain_states[c] holds chain c (column q of the bitstring = bit q) and is advanced in place by n_steps steps; step t
 * of the call is ABSOLUTE step step0 + t and draws Philox4x32-10 with key (seed mod 2^32, seed >> 32) and counter
 * {step mod 2^32, step >> 32, 0x47574731, c} (qhbm_sample uses 0x51b0c6a1 in the third word): output words 0, 1 make the
 * fp64 uniform u1 = c0 2^-32 + c1 2^-64 that picks the first bit whose inclusive fp32 prefix of exp(h_j - max h) exceeds
 * u1 times their sum, words 2, 3 make u2, compared with expf(min(0, L(x) - L(x'))).  The trajectory of chain c does not
 * depend on n_chains, on how a run is cut into calls (continue with step0 + n_steps), or on d_out_samples.
 * d_out_samples, if not NULL, takes the state after every step: [n_steps, n_chains, n_bits] int8 (NULL: burn-in);
 * d_out_accepted, if not NULL, takes the number of accepted steps per chain of this call (overwritten).
 * Mask bits at or above n_bits are ignored, a zero mask belongs to no bit, equal masks add.  One wave runs one chain with
 * the term table and one membership bitmap per bit in LDS: 12 n_terms + 4 ceil(n_terms / 32) n_bits bytes, at most
 * 160 KiB -- more is an error, there is no slower path.  Runs on the current device and the given stream; no host
 * synchronisation, no allocation; n_steps == 0 and n_chains == 0 do nothing. */
int qhbm_gwg_sample(uint64_t* d_chain_states, int n_chains, int n_bits,
                    const uint64_t* d_masks, const float* d_thetas, int n_terms,
                    uint64_t seed, uint64_t step0, int64_t n_steps,
                    int8_t* d_out_samples, int32_t* d_out_accepted, void* stream);

/* The table of ALL 2^n_bits energies of the same form by a fast Walsh-Hadamard transform: n 2^n additions
 * instead of n_terms 2^n parity evaluations, and no bitstring table.  1 <= n_bits <= 30.
 * qhbm_walsh_hadamard transforms d_data[2^n_bits] in place, unnormalised: H[y] = sum_m c[m] (-1)^popcount(y & m).
 * qhbm_parity_table overwrites d_table[y] with sum_k d_thetas[k] * parity_k(bitstring y), where bitstring y holds its
 * column q at bit n_bits-1-q of y (the row order of qhbm_statevector's amplitudes); column q is bit q of a mask.  Mask
 * bits at or above n_bits are ignored, a zero mask is a constant term, equal masks add in ascending term order;
 * n_terms == 0 gives zeros.
 * qhbm_parity_table_vjp overwrites d_grad[k] with sum_y d_weights[y] * parity_k(bitstring y): d_weights is transformed
 * into d_scratch (a second array of 2^n_bits floats, not d_weights) and never modified.
 * The order of the additions is a function of n_bits alone: bit-identical from call to call; each output carries at
 * most n_bits (+ the multiplicity of a mask) roundings.  No atomics, no allocation, no host synchronisation; they run on
 * the current device and the given stream. */
int qhbm_walsh_hadamard(float* d_data, int n_bits, void* stream);
int qhbm_parity_table(const uint64_t* d_masks, const float* d_thetas, int n_terms, int n_bits,
                      float* d_table, void* stream);
int qhbm_parity_table_vjp(const uint64_t* d_masks, int n_terms, int n_bits,
                          const float* d_weights, float* d_scratch,
                          float* d_grad, void* stream);

/* ---- introspection (tests, bench, DESIGN.md numbers) ------------------- */
/* Number of HBM passes (kernel launches over the state) the scheduler emits
 * for one forward of the installed circuit + observables. */
int qhbm_num_passes(qhbm_engine* h, int* forward_passes, int* backward_passes);
/* Human-readable description of the schedule, written into buf. */
int qhbm_describe_schedule(qhbm_engine* h, char* buf, size_t buf_len);
/* Accumulated HIP-event time (ms) and launch count of the pass kernels (forward passes, adjoint
 * passes, lambda = O psi) since the last call with reset != 0.  Timing is only recorded when the
 * option "profile_events" is non-zero; it synchronises the stream.  Any out pointer may be NULL. */
int qhbm_kernel_time_ms(qhbm_engine* h, int reset, double* fwd_ms,
                        int64_t* fwd_launches, double* bwd_ms,
                        int64_t* bwd_launches, double* obs_ms,
                        int64_t* obs_launches);
/* HBM bytes one call on U states must move under the installed schedule if every tile a pass
 * touches is read once and written once (tiles the kernels skip as identically zero excluded):
 * summed over the forward passes, lambda = O psi, and the adjoint passes (with_vjp != 0).  This
 * is the byte count bench.py's roofline divides by the measured kernel time. */
int qhbm_traffic_model(qhbm_engine* h, int U, int with_vjp, double* fwd_bytes,
                       double* obs_bytes, double* bwd_bytes);
/* fp32 operations (one FMA = 2) the gate arithmetic of one call on U states executes under the
 * installed schedule, counted from the plan's instance records with the per-micro-op costs of the
 * kernels' packed-fp32 sequences (X**t as three shears: 6 per amplitude forward, 16 in the adjoint
 * incl. lambda and the inner product; phases, FULL tables, boundary phases on the share of waves that
 * run them; tiles and waves the kernels skip as identically zero excluded; wave reductions, address
 * arithmetic and record decoding NOT counted): forward passes, lambda = O psi, adjoint passes.
 * bench.py divides it by the measured kernel time for a compute roofline against the fp32 vector
 * peak (157.3 TFLOP/s). */
int qhbm_flop_model(qhbm_engine* h, int U, int with_vjp, double* fwd_flops,
                    double* obs_flops, double* bwd_flops);

/* Executed micro-ops of every pass of the forward (adjoint == 0) or backward schedule, in
 * WAVE-EXECUTIONS per state (a micro-op a wave of 64 threads runs once counts 1; tiles and waves the
 * kernels skip excluded): out[pass * QHBM_CENSUS_COLUMNS + column], at most max_passes rows;
 * *n_passes = passes of the schedule.  scripts/instruction_mix.py weighs the per-micro-op
 * instruction counts of the compiled pass kernels with it (the dynamic instruction mix). */
enum {
  QHBM_CENSUS_TILES = 0,         /* workgroups per state */
  QHBM_CENSUS_ROUNDS,            /* register rounds (one LDS exchange each but the first) */
  QHBM_CENSUS_ROUNDS_BARRIER,    /* ... whose exchange needs the barriers */
  QHBM_CENSUS_ROUNDS_NO_BARRIER,
  QHBM_CENSUS_INSTANCES,         /* instance records decoded */
  QHBM_CENSUS_X,                 /* X**t (adjoint: with a gradient slot) */
  QHBM_CENSUS_X_NO_SLOT,         /* adjoint: X**t of a frozen parameter (no inner product) */
  QHBM_CENSUS_FULL,              /* 15-entry diagonal table */
  QHBM_CENSUS_PH1,
  QHBM_CENSUS_PH2,
  QHBM_CENSUS_CPH_TILE_ON,       /* boundary phase, predicate = tile bit, on */
  QHBM_CENSUS_CPH_WAVE_ON,       /* predicate = thread bit that is uniform over the wave, on */
  QHBM_CENSUS_CPH_LANE,          /* predicate varies inside the wave */
  QHBM_CENSUS_CPH_OFF,           /* predicate evaluated, off in the whole wave */
  QHBM_CENSUS_REDUCE8,           /* adjoint: eight-wide wave reductions of gradient partials: sets that have a value */
  QHBM_CENSUS_LEVEL1,            /* adjoint: level-1 adds of those reductions, issued where a partial is made: one per
                                    header bit of a micro-op with a partial, ten per FULL record */
  QHBM_CENSUS_COLUMNS
};
int qhbm_op_census(qhbm_engine* h, int adjoint, int max_passes, double* out, int* n_passes);
/* The row stride of qhbm_op_census IN THE LIBRARY (its QHBM_CENSUS_COLUMNS).  Columns are appended within an ABI
 * version (QHBM_CENSUS_LEVEL1 was; libraries without this entry point write 15 columns), so a caller that may meet a
 * library built from another header sizes `out` as max_passes * qhbm_census_columns() and strides its rows by it
 * (qhbmlib_amd/_engine.py op_census does); a buffer sized by an older header's QHBM_CENSUS_COLUMNS is too small for
 * this library. */
int qhbm_census_columns(void);

/* Plan searches this engine has run so far: forward plans (rebuilt when the circuit, the observables or a planning
 * option changes) and backward plans (also per gradient mask; a mask the engine has seen before is served from its
 * cache and builds nothing).  Either pointer may be NULL. */
int qhbm_plan_builds(qhbm_engine* h, int64_t* forward_plans, int64_t* backward_plans);
/* Sustained packed-fp32 rate and shader clock of the device RIGHT NOW: one probe launch (every SIMD issues
 * v_pk_fma_f32 from four waves, the pass kernels' occupancy) timed with HIP events, s_memtime / s_memrealtime read
 * inside the waves.  ghz: shader clock during the probe; cycles_per_pk_fma: issue cost per wave instruction and SIMD;
 * tflops: the packed-fp32 rate that follows (4 flop x 64 lanes per instruction) -- the ATTAINABLE ceiling bench.py
 * prints beside the nominal 157.3 TFLOP/s.  Synchronises `stream`.  Any out pointer may be NULL. */
int qhbm_clock_probe(qhbm_engine* h, double* ghz, double* cycles_per_pk_fma, double* tflops, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QHBM_ENGINE_H_ */
