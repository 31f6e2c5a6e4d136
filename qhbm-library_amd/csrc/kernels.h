// kernels.h -- launch entry points of the kernel objects (host side): kernels.hip (the pass kernels, with gwg.hip and
// parity_table.hip), observable.hip (with energy_table.hip, cotangent.hip, subsystem_apply.hip, gram_vjp.hip, cross_gram.hip and cross_gram_vjp.hip) and states.hip (import_states.hip, thermal.hip, krylov.hip,
// gram.hip, reduced.hip).  A .hip file reaches another one's kernels through these declarations only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "program.h"
#include "schedule.h"

namespace qhbm {

struct DevTerm {  // one Pauli term, amplitude-index bit space
  float coeff;
  uint32_t x, z;
  uint32_t ny;
  uint32_t op;
};

// Terms of equal x mask, consecutive in the x-sorted term array: [previous end, end).  A group
// never straddles a multiple of kObsTermChunk / 2 (the kernel stages that many terms in LDS at a time).
// Within a group of real weights the terms are ordered by how their sign (-1)^{popc(j & z)} varies
// inside a workgroup of apply_observable_kernel (j = block | slot bits | tid << 1: a thread owns A / 2
// adjacent pairs, slot s = index bit 0 and the bits from 9 up): first the n_h terms whose z misses the
// thread bits (one pre-summed weight per slot), then the n_l terms whose z misses the slot bits (one
// signed sum per thread), then the rest (per amplitude).
struct ObsGroup {
  uint32_t x, end;
  uint32_t has_imag;  // some term of the group has an odd number of Y factors (imaginary weight)
  uint32_t n_h, n_l;
  // Several observables with a value accumulator each (apply_observable_kernel<A, OBS_GATHER_MULTI>, at most
  // kObsGatherMultiOps of them): the terms are sorted by (x, observable), a group holds ONE observable's terms of one mask,
  // and a group whose mask equals the previous group's re-uses its gathered partners (same_x bit 0; bit 1: the array is
  // in that order at all -- no group may then skip partner pairs as vanishing, its successor may need them).
  uint32_t op, same_x;
};
enum ObsGatherMode : int {
  OBS_GATHER_LAMBDA = 0,  // lambda = sum_k upstream[s, op_k] c_k P_k psi
  OBS_GATHER_VALUE = 1,   // one observable: lambda = O psi (unweighted) and <psi|O|psi>
  OBS_GATHER_MULTI = 2,   // 2..kObsGatherMultiOps observables: the weighted lambda (if asked for) AND every <psi|O_t|psi>
};
constexpr uint32_t kObsGatherMultiOps = 4;
// A far launch of the two-level lambda = O psi sweep (engine.cpp far_windows, kernels.hip obs_phys): the terms whose masks
// flip only index bits [far_hi, far_hi + 7) (and bits 0..3), with x and z given in the VIRTUAL index space in which that
// window has changed places with bits [4, 11).
struct ObsFarLaunch {
  const DevTerm* terms;
  uint32_t n_terms;
  const ObsGroup* groups;
  uint32_t n_groups;
  uint32_t far_hi;
};
constexpr uint32_t obs_amps_per_thread(uint32_t n) { return n >= 11 ? 8u : 4u; }  // A of apply_observable_kernel<A>
constexpr uint32_t kObsThreadMask = 0x1feu;                                        // index bits 1..8 = the thread
constexpr uint32_t obs_slot_mask(uint32_t n) { return 1u | ((obs_amps_per_thread(n) / 2u - 1u) << 9); }  // bit 0 and 9 (, 10)
constexpr uint32_t kObsTermChunk = 512;  // 2 x the terms staged in LDS at a time (13 KiB: five workgroups per CU)

// ---- block-grouped Pauli sums (observable.hip) ---------------------------------------------------
// lambda = O psi and <psi|O|psi> for operators with MANY X-masks (BASELINE config 4: 512 random strings, 480 masks).
// A workgroup owns a BLOCK of 2^kObsBlockBits consecutive amplitudes.  A mask x = x_out (block bits) | x_in (bits inside
// the block) pairs the block with the partner block b ^ x_out: the terms come sorted by x_out and cut into GROUPS of
// equal x_out, the partner block of a group is fetched ONCE into LDS and every mask of the group reads it from there at
// l ^ x_in (config 4: 173 fetches per block instead of 453 gathers).
// Two shapes of the same kernel (observable.hip): blocks of 2^13 under ONE workgroup of 1024 threads per CU whose two halves
// split a group's masks, or blocks of 2^12 under TWO independent workgroups of 512 threads per CU that apply every mask of
// their groups (engine option "observable_block_bits").
constexpr int kObsBlockBits = 13;      // the larger shape: what the engine requires of a state before it picks these kernels
constexpr int kObsBlockBitsSmall = 12;
constexpr int kObsShapeRows = 113;     // launch_observable_blocks `block_bits`: blocks of 2^13 (the tables of 13), the halves split the ROWS
constexpr uint32_t kObsNewMask = 1u << 12;   // ObsBTerm::meta: the term's x differs from the previous term's
constexpr uint32_t kObsMaxValueOps = 256;    // per-op value cells of a workgroup (one row per wave: 16 KiB) must fit LDS
struct ObsBTerm {  // 32 bytes, one s_load_dwordx8: everything the kernel would otherwise derive per term with scalar ALU work
  float coeff;
  uint32_t zt;     // Z mask on the thread bits: (z >> 1) & 511
  uint32_t zb;     // Z mask on the block bits: z >> block bits
  uint32_t xrow;   // byte-address XOR of the partner rows in the LDS buffer: ((x >> 1) & 511) << 4 | ((x >> 10) & 7) << 13
                   // (blocks of 2^12: four rows, (x >> 10) & 3)
  uint32_t off0;   // jump-table offset of the variant for slots 0..7 (observable_variants.inc) ...
  uint32_t off1;   // ... and for slots 8..15 (base sign flipped when z holds the highest slot bit; blocks of 2^12: unused)
  uint32_t meta;   // op (bits 0..9) | kObsNewMask | kObsSignBit when i^ny (-1)^ny contributes a minus sign
  uint32_t pad;
};
constexpr uint32_t kObsSignBit = 1u << 13;
constexpr uint32_t kObsChunkBytes = 68, kObsPreambleBytes = 12;  // layout of the variant tables (scripts/gen_observable_asm.py)
struct ObsBGroup {
  uint32_t xout;  // x >> block bits: partner block = block ^ xout
  uint32_t begin, end;  // terms [begin, end) ...
  uint32_t mid;         // ... of which [begin, mid) are the first half-workgroup's masks, [mid, end) the second's (blocks of 2^12: = end)
};
enum ObsBlocksMode : int {
  OBS_LAMBDA = 0,        // lambda = sum_k upstream[s, op_k] c_k P_k psi
  OBS_LAMBDA_VALUE = 1,  // one observable: lambda = O psi (unweighted) and <psi|O|psi>
  OBS_VALUES = 2,        // one observable: <psi|O|psi> only (nothing stored)
  OBS_VALUES_MULTI = 3,  // n_ops <= kObsMaxValueOps observables: <psi|O_t|psi> for every t (nothing stored)
};
// value modes: value_part holds observable_blocks_value_parts(n, n_states, n_ops) floats of scratch
size_t observable_blocks_value_parts(uint32_t n, uint32_t n_states, uint32_t n_ops, int block_bits);
// `block_bits`: kObsBlockBits or kObsBlockBitsSmall -- the one the tables `terms` / `groups` were built for
hipError_t launch_observable_blocks(int mode, int block_bits, const float2* psi, float2* lam, uint32_t n, uint32_t n_states,
                                    const ObsBTerm* terms, const ObsBGroup* groups, uint32_t n_groups,
                                    const float* upstream, uint32_t n_ops, uint32_t state0, const float* op_scale,
                                    unsigned long long* out64, float* value_part, bool xcd_states, hipStream_t stream);

size_t fwd_lds_bytes(int K);
size_t adj_lds_bytes(int K, bool exchange);

// op_scale[k] = 2^(kValueFracBits - ceil(log2 sum|c|)) of op k; out64 [U, n_ops] fixed-point accumulators.
hipError_t launch_pass_fwd(int K, int R, const PassArgs& a, uint32_t n_states, float2* psi, const int8_t* bits,
                           int n_user, const uint32_t* prog, const uint32_t* tables, const float* coef,
                           const float* op_scale, unsigned long long* out64, uint32_t state0, hipStream_t stream,
                           const float2* psi_src = nullptr /* batched programs: element e LOADS the tile of state
                           e % prog_states of this buffer and stores into its own element of psi */);
// The same pass on PAIRS of consecutive states, tile pair in registers (kernels.hip pass_fwd2_kernel): only for
// lean passes that prune nothing, load nothing stale and measure nothing (or whose measurements are ignored).
bool pass_fwd_pair_supported(int K);
hipError_t launch_pass_fwd_pair(int K, const PassArgs& a, uint32_t n_states, float2* psi, const int8_t* bits, int n_user,
                                uint32_t state0, const uint32_t* prog, const uint32_t* tables, const float* coef,
                                hipStream_t stream);
// p[0 .. bytes) = 0 by a kernel (not a memset node: see kernels.hip)
hipError_t launch_zero_fill(void* p, size_t bytes, hipStream_t stream);
hipError_t launch_values_from_fixed(const unsigned long long* acc, const float* inv_scale, float* out, uint32_t count,
                                    uint32_t n_ops, hipStream_t stream);
// tile_grad [n_states * tiles, a.n_slots]: one gradient row per workgroup.  `exchange` selects the
// register-resident tile pair with one LDS exchange buffer (lean programs only).
hipError_t launch_pass_adj(int K, bool exchange, const PassArgs& a, uint32_t n_states, float2* psi, float2* lam,
                           const int8_t* bits, int n_user, const uint32_t* prog, const uint32_t* tables,
                           const float* coef, float* tile_grad, uint32_t state0, hipStream_t stream);
// tile_grad must have room for reduce_tiles_scratch_rows(n_states, n_tiles) more rows of n_slots floats.
size_t reduce_tiles_scratch_rows(size_t n_states, size_t n_tiles);
hipError_t launch_reduce_tiles(float* tile_grad, uint32_t n_states, uint32_t n_tiles, uint32_t n_slots,
                               float* state_grad, uint32_t n_slots_total, uint32_t slot_base, uint32_t state0,
                               hipStream_t stream);
// (value mode, out64 != null: `value_part` holds observable_value_parts(n, n_states) floats of scratch)
size_t observable_value_parts(uint32_t n, uint32_t n_states);
// (out64 != null: the values go to the fixed-point accumulators -- one observable, or `multi` (terms and groups in the
// (x, observable) order of OBS_GATHER_MULTI; value_part then holds observable_value_parts(n, n_states) x n_ops floats))
hipError_t launch_apply_observable(const float2* psi, float2* lam, uint32_t n, uint32_t n_states,
                                   const DevTerm* terms, uint32_t n_terms, const ObsGroup* groups,
                                   uint32_t n_groups, const float* upstream, uint32_t n_ops, uint32_t state0,
                                   const float* op_scale, unsigned long long* out64, float* value_part,
                                   bool xcd_states, hipStream_t stream, bool multi = false,
                                   const struct ObsFarLaunch* far = nullptr, int n_far = 0);
// Terms measured on the final state in HBM (X-mask wider than a tile); accumulates into out64.
hipError_t launch_measure_global(const float2* psi, uint32_t n, uint32_t n_states, const DevTerm* terms,
                                 uint32_t n_terms, const float* op_scale, unsigned long long* out64, uint32_t n_ops,
                                 uint32_t state0, hipStream_t stream);
hipError_t launch_parity_energy(const int8_t* bits, int64_t n_rows, int n, const uint64_t* masks,
                                const float* thetas, int n_terms, float* energy, hipStream_t stream);
hipError_t launch_parity_energy_vjp(const int8_t* bits, int64_t n_rows, int n, const uint64_t* masks, int n_terms,
                                    const float* w, float* grad, hipStream_t stream);
// Gibbs-With-Gradients chains of a spin-parity energy (gwg.hip): n_steps Metropolis steps of n_chains chains, one wave
// each, whose uint64 states (column q = bit q) are read and written in place.  Step t of the call uses the random numbers
// of absolute step step0 + t; out (or null) takes [n_steps, n_chains, n_bits] int8, accepted (or null) [n_chains] counts.
// The term table and the per-bit membership bitmaps take gwg_lds_bytes(n_bits, n_terms) of LDS, at most kGwgLdsMax.
constexpr size_t kGwgLdsMax = 160u * 1024u;  // the LDS of one CU
size_t gwg_lds_bytes(int n_bits, int n_terms);
hipError_t launch_gwg_sample(uint64_t* states, int n_chains, int n_bits, const uint64_t* masks, const float* thetas,
                             int n_terms, uint64_t seed, uint64_t step0, int64_t n_steps, int8_t* out, int32_t* accepted,
                             hipStream_t stream);
// Walsh-Hadamard transform over float[2^n_bits] and the spin-parity energy tables built on it (parity_table.hip),
// 1 <= n_bits <= 30.  dst = WHT(src): src == dst transforms in place, otherwise src is only read.  The table is zero
// filled, the thetas scattered to the bit-reversed masks and transformed; its VJP transforms `weights` into `scratch`
// and gathers grad[k] = scratch[rev(mask_k)].  wht_num_passes: launches over the array.
int wht_num_passes(int n_bits);
hipError_t launch_walsh_hadamard(const float* src, float* dst, int n_bits, hipStream_t stream);
hipError_t launch_parity_table(const uint64_t* masks, const float* thetas, int n_terms, int n_bits, float* table,
                               hipStream_t stream);
hipError_t launch_parity_table_vjp(const uint64_t* masks, int n_terms, int n_bits, const float* weights, float* scratch,
                                   float* grad, hipStream_t stream);
// block_cum: n_states * 2^n / 1024 doubles of scratch.
hipError_t launch_sample(const float2* psi, uint32_t n, int n_user, uint32_t n_states, double* block_cum,
                         uint32_t n_shots, uint64_t seed, uint32_t state0, int8_t* out, hipStream_t stream);
// One gate with a non-zero cirq global_shift: phase exp(i pi shift (scalar * params[param_idx] + offset)).
struct ShiftPhase {
  int32_t param_idx;
  float scalar, offset, shift;
};
// Shot counts per outcome for n_elements = programs x prog_states (program, state) elements whose final
// states sit consecutively in psi (element e = program prog0 + e / prog_states on state state0 + e % prog_states):
// out [programs, n_states_total, 2^n_user] int32 (zeroed by the caller for n > 10).  block_cum: n_elements * 2^n / 1024 doubles.
hipError_t launch_sample_counts(const float2* psi, uint32_t n, int n_user, uint32_t n_elements, uint32_t prog_states,
                                uint32_t prog0, double* block_cum, uint32_t n_shots, uint64_t seed, uint32_t state0,
                                uint32_t n_states_total, int* out, hipStream_t stream);
// Signed shot sums of Pauli-Z strings (sample_parity.hip): out[program, state, t] += sum over n_shots shots of
// (-1)^popcount(x & mask_t) for the n_elements <= 65535 elements of launch_sample_counts' layout, rows 2^row_bits amplitudes
// apart; out is zeroed by the caller.  d_masks [T] uint32 in INDEX space, written by launch_shot_parity_masks from a HOST
// array (the words travel as kernel arguments).  tables: shot_parity_table_doubles(row_bits, n_elements) doubles of scratch
// that may hold anything.  ctr_state / ctr_prog are added to the state row / program in the Philox counter alone.
size_t shot_parity_table_doubles(uint32_t row_bits, size_t n_elements);
hipError_t launch_shot_parity_masks(const uint32_t* host_masks, uint32_t T, uint32_t* d_masks, hipStream_t stream);
hipError_t launch_shot_parities(const float2* psi, uint32_t row_bits, int n_user, uint32_t n_elements, uint32_t prog_states,
                                uint32_t prog0, double* tables, const uint32_t* d_masks, uint32_t T, uint32_t n_shots,
                                uint64_t seed, uint32_t state0, uint32_t n_states_total, uint32_t ctr_state, uint32_t ctr_prog, int* out,
                                hipStream_t stream);
hipError_t launch_global_phase(const CoefJob* jobs, int n_jobs, const ShiftPhase* shifts, int n_shifts,
                               const float* params, float* out_cs, hipStream_t stream);
hipError_t launch_scale_states(float2* st, size_t count, const float* cs, hipStream_t stream);
hipError_t launch_prep_coefs(const CoefJob* jobs, int n_jobs, const float* params, float* coef,
                             int shift_gate, double shift, hipStream_t stream);
// n_programs coefficient buffers coef_stride floats apart (1, 0 for the usual single program)
hipError_t launch_combine_diag(float* coef, const uint32_t* rec_offsets, int n_records, uint32_t n_programs,
                               uint32_t coef_stride, hipStream_t stream);
// Batched parameter-shift programs: program y shifts the exponent of gate shift_gates[y] by shifts[y].
hipError_t launch_prep_coefs_batch(const CoefJob* jobs, int n_jobs, const float* params, float* coef,
                                   const int* shift_gates, const float* shifts, uint32_t n_programs,
                                   uint32_t coef_stride, hipStream_t stream);
hipError_t launch_replicate(const float* src, float* dst, uint32_t words, uint32_t stride, uint32_t copies,
                            hipStream_t stream);
hipError_t launch_shift_program_accumulate(const float* vals, const float* upstream, uint32_t n_programs, uint32_t c,
                                           uint32_t n_ops, uint32_t s0, double* prog_acc, hipStream_t stream,
                                           const int* dst_index = nullptr /* program q adds to prog_acc[dst_index[q]] */);
hipError_t launch_shift_combine(const double* prog_acc, const int* gate_param, const float* gate_weight,
                                int n_shift_gates, float* grad, int n_params, hipStream_t stream);
hipError_t launch_reduce_grad(const float* state_grad, uint32_t U, uint32_t n_slots,
                              const int* param_slot_begin, const int* param_slots,
                              const float* slot_factor, float* grad, int n_params, int accumulate,
                              hipStream_t stream);
hipError_t launch_scale_rows(float* rows, uint32_t U, uint32_t width, const float* w, hipStream_t stream);
// sustained packed-fp32 issue rate and shader clock (engine.cpp qhbm_clock_probe)
hipError_t launch_clock_probe(uint64_t* out, float* sink, uint32_t n_cus, hipStream_t stream);
uint32_t clock_probe_waves(uint32_t n_cus);
double clock_probe_instructions_per_simd();
hipError_t launch_scatter_jac(const float* state_grad, uint32_t U, uint32_t n_slots,
                              const int* param_slot_begin, const int* param_slots,
                              const float* slot_factor, float* jac, uint32_t n_ops, uint32_t op,
                              uint32_t n_params, hipStream_t stream);

// ---- qhbm_program_vjps (kernels.hip, after the reductions of the adjoint VJP) ----
// dst[e, :] = src[state0 + e % c, :] for e < n_elements (rows of row_bytes bytes): per-element copies of per-state rows
hipError_t launch_replicate_rows(const void* src, void* dst, uint32_t row_bytes, uint32_t c, uint32_t state0,
                                 uint32_t n_elements, hipStream_t stream);
// rows[(prog0 + e / c) * U + state0 + e % c, :] = elem_rows[e, :]  (n_slots floats per row)
hipError_t launch_scatter_program_rows(const float* elem_rows, float* rows, uint32_t n_slots, uint32_t c, uint32_t state0,
                                       uint32_t U, uint32_t prog0, uint32_t n_elements, hipStream_t stream);
// grad[dst[q], p] = reduce_grad of program q's [U, n_slots] rows (the order of launch_reduce_grad)
hipError_t launch_reduce_program_grad(const float* rows, uint32_t U, uint32_t n_slots, const int* param_slot_begin,
                                      const int* param_slots, const float* slot_factor, const int* dst, uint32_t n_programs,
                                      float* grad, int n_params, hipStream_t stream);
// acc[dst[q], k] += sum_u w[state0 + u] * vals[q * c + u, k], u in order, fp64 (w NULL: 1)
hipError_t launch_accumulate_program_values(const float* vals, const float* w, uint32_t n_programs, uint32_t c,
                                            uint32_t n_ops, uint32_t state0, const int* dst, double* acc,
                                            hipStream_t stream);
hipError_t launch_doubles_to_floats(const double* src, float* dst, size_t count, hipStream_t stream);

// ---- energy tables (energy_table.hip): E = sum_y table[y] |y><y| over the c final states of a chunk ----
enum TableMode : int {
  TABLE_VALUES = 0,       // d_out[s0 + i] = <psi_i|E|psi_i>, nothing stored
  TABLE_LAMBDA = 1,       // lambda_i = upstream[s0 + i] E psi_i (zeros at padded indices), values as above if d_out
  TABLE_LAMBDA_GRAD = 2,  // ... and gsum[y] += sum_i upstream[s0 + i] |psi_i[y]|^2 (fp64, order fixed by global state index)
};
// States per group of the 2-D grid, log2 (a function of n_eff only: the fold order of the table gradient depends on it).
uint32_t table_group_bits(uint32_t n_eff);
// Groups (rows of gpart, each 2^n doubles) a chunk [s0, s0 + c) touches.
uint32_t table_groups(uint32_t s0, uint32_t c, uint32_t n_eff);
// vpart: c * 2^(n_eff - 10) doubles of scratch; gpart: table_groups() * 2^n; carry, gsum: 2^n (TABLE_LAMBDA_GRAD only,
// gsum zeroed before the first chunk); d_out may be NULL (no values wanted).
hipError_t launch_energy_table(int mode, const float2* psi, float2* lam, const float* table, uint32_t n, uint32_t n_eff,
                               uint32_t c, uint32_t s0, uint32_t U, const float* upstream, double* vpart, float* d_out,
                               double* gpart, double* carry, double* gsum, hipStream_t stream);

// ---- caller-supplied start states (import_states.hip) ----
// Doubles of scratch a squared norm of each of c states at a pitch of 2^n amplitudes needs (state_sweep.h: one partial
// per slice): the `parts` of launch_import_states and launch_cheb_step, the `norm_parts` of launch_krylov_subtract.
size_t state_norm_parts_count(uint32_t n, uint32_t c);
// Input states s0 .. s0 + c of `src` ([., 2^n] complex64, read only, 16-byte aligned): norm2[s0 + i] = ||phi||^2 in fp64
// (fixed order, no atomics), psi element i = phi / ||phi|| at a pitch of 2^n_eff amplitudes, zeros in the padding and
// for a state of norm 0.  Reads the input twice.
hipError_t launch_import_states(const float2* src, uint32_t n, uint32_t n_eff, uint32_t c, uint32_t s0, float2* psi,
                                double* parts, double* norm2, hipStream_t stream);
// out[r, k] = in[r, k] * norm2[r] (in == out allowed)
hipError_t launch_scale_by_norm2(const float* in, float* out, uint32_t rows, uint32_t width, const double* norm2,
                                 hipStream_t stream);
// dst row r (2^n_dst amplitudes) = src row r (2^n_src amplitudes), its first 2^n_copy amplitudes times
// scale[r] * sqrt(norm2[r]) (either may be NULL: 1; both NULL: a plain copy), zeros behind them.
hipError_t launch_scale_copy_states(const float2* src, uint32_t n_src, float2* dst, uint32_t n_dst, uint32_t n_copy, uint32_t c,
                                    const double* scale, const double* norm2, hipStream_t stream);

// ---- Chebyshev evolution of caller-supplied states (thermal.hip) ----
// One term of the recurrence over the chunk's c states (w, tprev, acc: [c, 2^n_eff], distinct buffers):
//   first:      tprev = t_0 = acc * scale[i], acc = c0 t_0 + coef w            (w = t_1)
//   otherwise:  tprev = t_{k+1} = w - tprev,  acc += coef t_{k+1}
// with_norm: parts[i, .] = per-workgroup sums of |acc|^2 (fp64) for launch_finish_step.
hipError_t launch_cheb_step(bool first, bool with_norm, const float2* w, float2* tprev, float2* acc, uint32_t n_eff, uint32_t c,
                            float2 c0, float2 coef, const double* scale, double* parts, hipStream_t stream);
// Per state i < c: norm = sqrt(sum of its parts, in index order), log_norm[i] += log(norm) + x, scale[i] = 1 / norm (0 for
// norm 0), up1[i, k] = float(wr[k] * scale[i]) for k < n_ops.
hipError_t launch_finish_step(const double* parts, uint32_t n_eff, uint32_t c, double x, double* log_norm, double* scale,
                              const double* wr, uint32_t n_ops, float* up1, hipStream_t stream);
// scale[i] = 1, log_norm[i] = log(norm2[i]) / 2, up1[i, k] = float(wr[k]), up2[i, k] = float(2 wr[k]); scale, log_norm
// (with norm2), up1 and up2 may each be NULL.
hipError_t launch_evolve_init(uint32_t c, const double* norm2, double* log_norm, double* scale, const double* wr, uint32_t n_ops,
                              float* up1, float* up2, hipStream_t stream);
// Random-sign states (include/qhbm_engine.h qhbm_random_states): out [n_states, 2^n]
hipError_t launch_random_states(float2* out, uint32_t n_states, uint32_t n, uint64_t seed, uint32_t first_state,
                                hipStream_t stream);

// ---- Lanczos bases of caller-supplied states and sums over a stored basis (krylov.hip) ----
constexpr int kKrylovBlock = 8;  // basis rows of one project / subtract sweep, outputs of one combine or replay sweep
// Doubles of scratch one project sweep (`parts`) of a chunk of c states of n qubits needs.
size_t krylov_coef_parts_count(uint32_t n, uint32_t c);
// scale[i] = 1, lengths[i] = m for i < c; a state with norm2[i] = 0: scale 0, length 0.
hipError_t launch_krylov_init(uint32_t c, const double* norm2, int m, int32_t* lengths, double* scale, hipStream_t stream);
// c_k = <v_k, w> for the nb <= 8 basis rows at `rows` (row k of the chunk's state i at rows + k row_stride_amps + i 2^n)
// -- row_stride_amps may be negative (the ring of qhbm_krylov_tridiagonal: row k + 1 below row k in memory) --
// and the chunk's c states w (pitch 2^n_w amplitudes), complex fp64 in a fixed order; coef[i, first + k] = c_k rounded to
// complex64; alpha_at >= 0: alpha[i alpha_pitch] += Re c_{alpha_at}.
hipError_t launch_krylov_project(const float2* w, uint32_t n_w, const float2* rows, int64_t row_stride_amps, uint32_t n, uint32_t c,
                                 uint32_t nb, double* parts, float2* coef, uint32_t coef_pitch, uint32_t first, int alpha_at,
                                 double* alpha, uint64_t alpha_pitch, hipStream_t stream);
// w -= sum_k coef[i, k] v_k over the same rows, k ascending, fp32; norm_parts (or NULL): per-workgroup sums of |w|^2.
hipError_t launch_krylov_subtract(float2* w, uint32_t n_w, const float2* rows, int64_t row_stride_amps, uint32_t n, uint32_t c,
                                  uint32_t nb, const float2* coef, uint32_t coef_pitch, double* norm_parts, hipStream_t stream);
// Per state i < c with scale[i] != 0: norm = sqrt(sum of its parts); norm <= threshold: lengths[i] = j + 1, beta 0, scale 0;
// else beta[i beta_pitch + j] = norm, scale[i] = 1 / norm.  scale[i] = 0 stays: beta 0.
hipError_t launch_krylov_norm(const double* norm_parts, uint32_t n, uint32_t c, double threshold, int j, double* beta,
                              uint64_t beta_pitch, int32_t* lengths, double* scale, hipStream_t stream);
// out[u, s] = sum_j coef[u, s, j] basis[j, u]: basis [m, U, 2^n], coef [U, S, m], out [U, S, 2^n]
hipError_t launch_krylov_combine(const float2* basis, uint32_t m, uint32_t U, uint32_t n, const float2* coef, uint32_t S,
                                 float2* out, hipStream_t stream);
// The scaled copy of a step of the replay of a recorded recurrence (qhbm_krylov_replay), which also accumulates: for the
// chunk's c states, all three at a pitch of 2^n_eff amplitudes (w = H v_j - c_{j-1} v_{j-1} - c_j v_j as
// launch_krylov_subtract left it, vcur = v_j, vnext = v_{j-1} on entry),
//   vnext = v_{j+1} = float(double(w) f), f = 1 / beta[i beta_pitch] (0 where that is 0); zeros in the padding
//   out[i, s] += coef[i, s, j + 1] v_{j+1} for s < sb <= 8   (j = 0: out[i, s] = coef[i, s, 0] v_0 + coef[i, s, 1] v_1)
// beta: beta_j of the chunk's first state; coef [., S, m] and out [., S, 2^n] at the chunk's first state and the group's
// first output.  vcur is read at j = 0 only.
hipError_t launch_krylov_replay(uint32_t j, const float2* w, const float2* vcur, float2* vnext, uint32_t n, uint32_t n_eff,
                                uint32_t c, const double* beta, uint64_t beta_pitch, const float2* coef, uint32_t m, uint32_t S,
                                uint32_t sb, float2* out, hipStream_t stream);

// ---- the weighted Gram matrix of M states (gram.hip) ----
constexpr int kGramMaxStates = 1024;
// Doubles of scratch (`parts`) one Gram matrix of M states of n qubits needs.
size_t gram_parts_count(uint32_t n, uint32_t M);
// gram[i, j] = sum_x table[x] conj(states[i, x]) states[j, x] (table NULL: 1), complex fp64 in a fixed order, [M, M, 2];
// states [M, 2^n]; M in [1, kGramMaxStates], n in [1, 31].  Every partial that is read is written first: `parts` may hold anything.
hipError_t launch_weighted_gram(const float2* states, uint32_t M, uint32_t n, const float* table, double* parts, double* gram,
                                hipStream_t stream);

// ---- the cross-Gram matrix of M bras and K kets (cross_gram.hip) ----
// Doubles of scratch (`parts`) one cross-Gram matrix of M x K states of n qubits needs.
size_t cross_gram_parts_count(uint32_t n, uint32_t M, uint32_t K);
// out[i, j] = sum_x table[x] conj(bras[i, x]) kets[j, x] (table NULL: 1), complex fp64 in launch_weighted_gram's order of
// additions, [M, K, 2], every entry summed on its own; bras [M, 2^n], kets [K, 2^n], both only read (they may overlap);
// M, K in [1, kGramMaxStates], n in [1, 31].  Every partial that is read is written first: `parts` may hold anything.
hipError_t launch_cross_gram(const float2* bras, uint32_t M, const float2* kets, uint32_t K, uint32_t n, const float* table,
                             double* parts, double* out, hipStream_t stream);

// ---- the VJP of the cross-Gram matrix (cross_gram_vjp.hip; the plan is cross_gram_vjp_plan.h's) ----
// For a cotangent gamma [M, K] (complex64, row-major, used as given) of launch_cross_gram's matrix, c_j(x) = sum_i gamma[i, j]
// bras[i, x] in f32: out_kets[j, x] = table[x] c_j(x), out_bras[i, x] = table[x] sum_j conj(gamma[i, j]) kets[j, x] (table NULL:
// 1), complex64 [K, 2^n] and [M, 2^n]; table_grad[x] = sum_j Re(conj(c_j(x)) kets[j, x]), fp64 in a fixed order, [2^n].  Each
// output may be NULL (not all three).  Shape limits as launch_cross_gram.  `scratch`: cgv_plan(n, M, K).scratch_bytes bytes,
// which may hold anything.
hipError_t launch_cross_gram_vjp(const float2* bras, uint32_t M, const float2* kets, uint32_t K, uint32_t n, const float* table,
                                 const float2* gamma, float2* out_bras, float2* out_kets, double* table_grad, void* scratch,
                                 hipStream_t stream);

// ---- the reduced density matrix of M states (reduced.hip; the plan is rdm_index.h's) ----
// rho[a, a'] = sum_m weights[m] sum_b phi_m(a, b) conj(phi_m(a', b)) (weights NULL: 1), complex fp64 in a fixed order,
// [2^k, 2^k, 2]; states [M, 2^n]; keep_mask in qubit space, k = popcount in [1, min(n, 10)], n in [1, 31], M in [1, 65536].
// `parts`: rdm_plan(n, keep_mask, M).scratch_bytes bytes, which may hold anything.
hipError_t launch_reduced_density(const float2* states, uint32_t M, uint32_t n, uint64_t keep_mask, const double* weights,
                                  double* parts, double* rho, hipStream_t stream);

// ---- a caller's cotangent of the final states as the backward sweep's lambda (cotangent.hip) ----
// Doubles of scratch (`parts`) one chunk of c states of n qubits needs.
size_t cotangent_parts_count(uint32_t n, uint32_t c);
// Cotangent rows s0 .. s0 + c of `cot` ([., 2^n] complex64, read only, 16-byte aligned) against the chunk's final states
// chi (pitch 2^n_eff): lam element i = 1/2 sqrt(norm2[s0 + i]) (phase_cs[0] - i phase_cs[1]) cot at the same pitch, zeros in
// the padding; dot[2 (s0 + i)], [.. + 1] = Re, Im <cot|chi>, fp64 in a fixed order.  `parts` may hold anything.
hipError_t launch_cotangent_import(const float2* cot, const float2* chi, uint32_t n, uint32_t n_eff, uint32_t c, uint32_t s0,
                                   const double* norm2, const float* phase_cs, float2* lam, double* parts, double* dot,
                                   hipStream_t stream);
// grad[p] -= slope[p] sum_u sqrt(norm2[u]) Im((phase_cs[0] + i phase_cs[1]) dot_u), u in order, fp64; entries with slope 0
// keep their bits.
hipError_t launch_cotangent_phase_grad(const double* dot, const double* norm2, uint32_t U, const float* phase_cs, const float* slope,
                                       float* grad, uint32_t n_params, hipStream_t stream);

// ---- a dense operator on k arbitrary qubits of M states (subsystem_apply.hip; the plan is subsystem_plan.h's) ----
// out[m] = scale[m] (op (x) 1) states[m] (scale NULL: 1), complex64; op [2^k, 2^k] complex64 row-major on the kept qubits of
// keep_mask in ascending order; dots [M, 2] = <states[m]|(op (x) 1)|states[m]> before scaling, fp64 in a fixed order, or NULL.
// Shape limits as launch_reduced_density.  `scratch`: sub_plan(n, keep_mask, M).scratch_bytes bytes, which may hold anything.
hipError_t launch_subsystem_apply(const float2* states, uint32_t M, uint32_t n, uint64_t keep_mask, const float2* op,
                                  const double* scale, float2* out, double* dots, void* scratch, hipStream_t stream);

// ---- the VJP of the weighted Gram matrix (gram_vjp.hip; the plan is gram_vjp_plan.h's) ----
// c_j(x) = sum_i H[i, j] states[i, x] in f32; out[j, x] = table[x] c_j(x) (table NULL: c itself), complex64 [M, 2^n], or NULL;
// table_grad[x] = 1/2 sum_j Re(conj(c_j(x)) states[j, x]), fp64 in a fixed order, [2^n], or NULL (not both).  H [M, M]
// complex64 row-major, used as given.  Shape limits as launch_weighted_gram.  `scratch`: gv_plan(n, M).scratch_bytes bytes,
// which may hold anything.
hipError_t launch_gram_vjp(const float2* states, uint32_t M, uint32_t n, const float* table, const float2* H, float2* out,
                           double* table_grad, void* scratch, hipStream_t stream);

}  // namespace qhbm
