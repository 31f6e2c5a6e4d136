"""ctypes binding of the HIP engine's C ABI (include/qhbm_engine.h).

There is no CPU fallback: if `libqhbm_engine.so` is missing or no GPU is
present, every compute call raises.  torch is used for device memory and
streams only.
"""
import ctypes
import os
import warnings

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QHBM_ENGINE_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libqhbm_engine.so")

# Gate kinds: values of enum qhbm_gate_kind.
GATE_I = 0
GATE_XPOW = 1
GATE_YPOW = 2
GATE_ZPOW = 3
GATE_HPOW = 4
GATE_CZPOW = 5
GATE_CNOTPOW = 6
GATE_SWAPPOW = 7
GATE_ISWAPPOW = 8
GATE_XXPOW = 9
GATE_YYPOW = 10
GATE_ZZPOW = 11

ABI_VERSION = 5  # include/qhbm_engine.h QHBM_ABI_VERSION

GRAD_ADJOINT = 0
GRAD_PARAMETER_SHIFT = 1

ABI_SYMBOLS = (
    "qhbm_abi_version", "qhbm_create", "qhbm_destroy", "qhbm_last_error",
    "qhbm_set_circuit", "qhbm_set_gradient_mask", "qhbm_set_observables", "qhbm_set_option",
    "qhbm_workspace_bytes", "qhbm_allocated_bytes", "qhbm_expectation", "qhbm_expectation_vjp",
    "qhbm_expectation_retain", "qhbm_expectation_vjp_retained", "qhbm_retained_states", "qhbm_state_gradients",
    "qhbm_expectation_jacobian", "qhbm_statevector", "qhbm_sample", "qhbm_sample_counts", "qhbm_program_vjps", "qhbm_parity_energy", "qhbm_parity_energy_vjp",
    "qhbm_gwg_sample", "qhbm_walsh_hadamard", "qhbm_parity_table", "qhbm_parity_table_vjp",
    "qhbm_num_passes", "qhbm_describe_schedule",
    "qhbm_kernel_time_ms", "qhbm_traffic_model", "qhbm_flop_model", "qhbm_op_census", "qhbm_census_columns", "qhbm_clock_probe", "qhbm_plan_builds",
    "qhbm_table_expectation", "qhbm_table_expectation_retain", "qhbm_table_expectation_vjp",
    "qhbm_table_expectation_vjp_retained",
    "qhbm_expectation_from_states", "qhbm_expectation_vjp_from_states", "qhbm_statevector_from_states",
    "qhbm_describe_schedule_from_states", "qhbm_statevector_vjp_from_states",
    "qhbm_apply_observables", "qhbm_evolve_states", "qhbm_describe_evolution", "qhbm_random_states",
    "qhbm_krylov_basis", "qhbm_krylov_combine", "qhbm_describe_krylov",
    "qhbm_krylov_tridiagonal", "qhbm_krylov_replay", "qhbm_describe_krylov_stream",
    "qhbm_gram_scratch_bytes", "qhbm_weighted_gram",
    "qhbm_reduced_density_scratch_bytes", "qhbm_reduced_density",
    "qhbm_subsystem_apply_scratch_bytes", "qhbm_subsystem_apply",
    "qhbm_gram_vjp_scratch_bytes", "qhbm_weighted_gram_vjp",
    "qhbm_cross_gram_scratch_bytes", "qhbm_cross_gram",
    "qhbm_cross_gram_vjp_scratch_bytes", "qhbm_cross_gram_vjp",
    "qhbm_sample_parities", "qhbm_sample_parities_scratch_bytes", "qhbm_sample_parities_states",
)


class QhbmGate(ctypes.Structure):
  _fields_ = [("kind", ctypes.c_int32), ("q0", ctypes.c_int32),
              ("q1", ctypes.c_int32), ("param_idx", ctypes.c_int32),
              ("scalar", ctypes.c_float), ("offset", ctypes.c_float),
              ("global_shift", ctypes.c_float)]


class EngineError(RuntimeError):
  pass


_lib = None


def load_library():
  """Loads libqhbm_engine.so (built by `__graft_entry__.build()`)."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise EngineError(
        f"{LIB_PATH} not found: build the HIP extension first "
        "(python -c 'import __graft_entry__ as g; g.build()'); "
        "there is no CPU fallback.")
  lib = ctypes.CDLL(LIB_PATH)
  vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
  lib.qhbm_abi_version.restype = i32
  found = lib.qhbm_abi_version()
  if found != ABI_VERSION:
    # an OLDER library handed in on purpose (QHBM_ENGINE_LIB, the one-box A/B runs of scripts/r05_ab.sh) is tolerated
    # with a warning: the optional symbols below are skipped; anything else is a stale build
    if os.environ.get("QHBM_ENGINE_LIB") and found < ABI_VERSION:
      warnings.warn(f"{LIB_PATH} exports ABI v{found}, this binding is written for v{ABI_VERSION}: newer entry "
                    "points are unavailable")
    else:
      raise EngineError(f"{LIB_PATH} exports ABI v{found}, this binding needs v{ABI_VERSION}: rebuild the engine "
                        "(python -c 'import __graft_entry__ as g; g.build()')")
  lib.qhbm_create.argtypes = [i32, ctypes.POINTER(vp)]
  lib.qhbm_destroy.argtypes = [vp]
  lib.qhbm_destroy.restype = None
  lib.qhbm_last_error.argtypes = [vp]
  lib.qhbm_last_error.restype = ctypes.c_char_p
  lib.qhbm_set_circuit.argtypes = [vp, i32, i32, ctypes.POINTER(QhbmGate), i32]
  lib.qhbm_set_gradient_mask.argtypes = [vp, vp, i32]
  lib.qhbm_set_observables.argtypes = [vp, i32, vp, vp, vp, vp]
  lib.qhbm_set_option.argtypes = [vp, ctypes.c_char_p, i64]
  lib.qhbm_workspace_bytes.argtypes = [vp, i32, i32,
                                       ctypes.POINTER(ctypes.c_size_t)]
  lib.qhbm_allocated_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_size_t)]
  lib.qhbm_retained_states.argtypes = [vp, ctypes.POINTER(i32)]
  lib.qhbm_expectation.argtypes = [vp, vp, i32, vp, vp, vp]
  lib.qhbm_expectation_vjp.argtypes = [vp, vp, i32, vp, vp, vp, vp, i32, vp]
  lib.qhbm_expectation_retain.argtypes = [vp, vp, i32, vp, vp, vp]
  lib.qhbm_expectation_vjp_retained.argtypes = [vp, vp, i32, vp, vp, vp, vp]
  lib.qhbm_state_gradients.argtypes = [vp, i32, vp, vp]
  lib.qhbm_expectation_jacobian.argtypes = [vp, vp, i32, vp, vp, vp, vp]
  lib.qhbm_statevector.argtypes = [vp, vp, i32, vp, vp, vp]
  lib.qhbm_sample.argtypes = [vp, vp, i32, vp, i32, ctypes.c_uint64, i32, ctypes.c_double, vp, vp]
  lib.qhbm_sample_counts.argtypes = [vp, vp, i32, vp, i32, vp, vp, i32, ctypes.c_uint64, vp, vp]
  lib.qhbm_parity_energy.argtypes = [vp, i64, i32, vp, vp, i32, vp, vp]
  lib.qhbm_parity_energy_vjp.argtypes = [vp, i64, i32, vp, i32, vp, vp, vp]
  lib.qhbm_gwg_sample.argtypes = [vp, i32, i32, vp, vp, i32, ctypes.c_uint64, ctypes.c_uint64, i64, vp, vp, vp]
  lib.qhbm_walsh_hadamard.argtypes = [vp, i32, vp]
  lib.qhbm_parity_table.argtypes = [vp, vp, i32, i32, vp, vp]
  lib.qhbm_parity_table_vjp.argtypes = [vp, i32, i32, vp, vp, vp, vp]
  lib.qhbm_num_passes.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
  lib.qhbm_describe_schedule.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
  lib.qhbm_kernel_time_ms.argtypes = [
      vp, i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64),
      ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64),
      ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i64)]
  lib.qhbm_traffic_model.argtypes = [vp, i32, i32] + [ctypes.POINTER(ctypes.c_double)] * 3
  lib.qhbm_flop_model.argtypes = [vp, i32, i32] + [ctypes.POINTER(ctypes.c_double)] * 3
  try:
    lib.qhbm_op_census.argtypes = [vp, i32, i32, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(i32)]
    lib.qhbm_plan_builds.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64)]
    lib.qhbm_clock_probe.argtypes = [vp] + [ctypes.POINTER(ctypes.c_double)] * 3 + [vp]
    lib.qhbm_program_vjps.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.qhbm_table_expectation.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    lib.qhbm_table_expectation_retain.argtypes = [vp, vp, i32, vp, vp, vp, vp]
    lib.qhbm_table_expectation_vjp.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.qhbm_table_expectation_vjp_retained.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, vp]
    lib.qhbm_expectation_from_states.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.qhbm_expectation_vjp_from_states.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.qhbm_statevector_from_states.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.qhbm_describe_schedule_from_states.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
    lib.qhbm_statevector_vjp_from_states.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.qhbm_apply_observables.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.qhbm_evolve_states.argtypes = [vp, vp, i32, vp, ctypes.c_double, i32, vp, vp]
    lib.qhbm_describe_evolution.argtypes = [vp, vp, ctypes.c_double, i32, ctypes.c_char_p, ctypes.c_size_t]
    lib.qhbm_random_states.argtypes = [vp, i32, i32, ctypes.c_uint64, ctypes.c_uint64, vp]
    lib.qhbm_krylov_basis.argtypes = [vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.qhbm_krylov_combine.argtypes = [vp, i32, i32, i32, vp, i32, vp, vp]
    lib.qhbm_describe_krylov.argtypes = [vp, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    lib.qhbm_krylov_tridiagonal.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.qhbm_krylov_replay.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp, vp]
    lib.qhbm_describe_krylov_stream.argtypes = [vp, i32, i32, i32, ctypes.c_char_p, ctypes.c_size_t]
    lib.qhbm_gram_scratch_bytes.argtypes = [i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    lib.qhbm_weighted_gram.argtypes = [vp, i32, i32, vp, vp, vp, vp]
    lib.qhbm_reduced_density_scratch_bytes.argtypes = [i32, i32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_size_t)]
    lib.qhbm_reduced_density.argtypes = [vp, i32, i32, ctypes.c_uint64, vp, vp, vp, vp]
    lib.qhbm_subsystem_apply_scratch_bytes.argtypes = [i32, i32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_size_t)]
    lib.qhbm_subsystem_apply.argtypes = [vp, i32, i32, ctypes.c_uint64, vp, vp, vp, vp, vp, vp]
    lib.qhbm_sample_parities.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, i32, i64, ctypes.c_uint64, vp, vp]
    lib.qhbm_sample_parities_scratch_bytes.argtypes = [i32, i32, i64, ctypes.POINTER(ctypes.c_size_t)]
    lib.qhbm_sample_parities_states.argtypes = [vp, i32, i32, vp, i32, i64, ctypes.c_uint64, ctypes.c_uint64,
                                                ctypes.c_uint32, vp, vp, vp]
    lib.qhbm_gram_vjp_scratch_bytes.argtypes = [i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    lib.qhbm_weighted_gram_vjp.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
    lib.qhbm_cross_gram_scratch_bytes.argtypes = [i32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    lib.qhbm_cross_gram.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp]
    lib.qhbm_cross_gram_vjp_scratch_bytes.argtypes = [i32, i32, i32, ctypes.POINTER(ctypes.c_size_t)]
    lib.qhbm_cross_gram_vjp.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp]
  except AttributeError:  # an older library given through QHBM_ENGINE_LIB (A/B runs): the probe is optional there
    pass
  _lib = lib
  return lib


def _check_global(rc):
  if rc != 0:
    raise EngineError(load_library().qhbm_last_error(None).decode())


class _ParityEnergyFunction(torch.autograd.Function):
  """energies[i] = sum_k thetas[k] * parity_k(bits[i]) on the GPU (qhbm_parity_energy); the
  backward is qhbm_parity_energy_vjp.  `masks` is an int64 CUDA tensor of column masks."""

  @staticmethod
  def forward(ctx, thetas, bits, masks):
    lib = load_library()
    bits = bits.to(torch.int8).contiguous()
    th = thetas.detach().to(device=bits.device, dtype=torch.float32).contiguous()
    out = torch.empty((bits.shape[0],), dtype=torch.float32, device=bits.device)
    with torch.cuda.device(bits.device):
      _check_global(lib.qhbm_parity_energy(
          bits.data_ptr(), bits.shape[0], bits.shape[1], masks.data_ptr(), th.data_ptr(),
          masks.numel(), out.data_ptr(),
          ctypes.c_void_p(torch.cuda.current_stream(bits.device).cuda_stream)))
    ctx.bits, ctx.masks = bits, masks
    ctx.theta_device = thetas.device
    return out

  @staticmethod
  def backward(ctx, upstream):
    lib = load_library()
    bits, masks = ctx.bits, ctx.masks
    w = upstream.to(device=bits.device, dtype=torch.float32).contiguous()
    grad = torch.empty((masks.numel(),), dtype=torch.float32, device=bits.device)
    with torch.cuda.device(bits.device):
      _check_global(lib.qhbm_parity_energy_vjp(
          bits.data_ptr(), bits.shape[0], bits.shape[1], masks.data_ptr(), masks.numel(),
          w.data_ptr(), grad.data_ptr(),
          ctypes.c_void_p(torch.cuda.current_stream(bits.device).cuda_stream)))
    return grad.to(ctx.theta_device), None, None


def parity_sums(bits, masks, weights):
  """[M] float32: sum_i weights[i] * parity_m(bits[i]) over CUDA `bits` [N, n] for int64 CUDA column `masks` [M]
  (qhbm_parity_energy_vjp, no autograd)."""
  lib = load_library()
  bits = bits.to(torch.int8).contiguous()
  w = weights.to(device=bits.device, dtype=torch.float32).contiguous()
  out = torch.empty((masks.numel(),), dtype=torch.float32, device=bits.device)
  with torch.cuda.device(bits.device):
    _check_global(lib.qhbm_parity_energy_vjp(
        bits.data_ptr(), bits.shape[0], bits.shape[1], masks.data_ptr(), masks.numel(), w.data_ptr(), out.data_ptr(),
        ctypes.c_void_p(torch.cuda.current_stream(bits.device).cuda_stream)))
  return out


def parity_energy(thetas, bits, masks):
  """Differentiable (w.r.t. `thetas`) spin-parity energies of CUDA `bits` [N, n]."""
  if not bits.is_cuda:
    raise EngineError("parity_energy runs on the GPU: pass CUDA bitstrings (CPU tensors use the torch layers)")
  return _ParityEnergyFunction.apply(thetas, bits, masks)


WHT_MAX_BITS = 30   # csrc/parity_table.hip kWhtMaxBits
WHT_TILE_BITS = 14  # kWhtTileBits: up to here the transform is one launch
WHT_ROW_BITS = 9    # kWhtRowBits: index bits every further pass adds


def walsh_hadamard_passes(n_bits):
  """Launches over the array of one transform of 2^n_bits floats (csrc/parity_table.hip wht_num_passes)."""
  return 1 if n_bits <= WHT_TILE_BITS else 1 + -(-(n_bits - WHT_TILE_BITS) // WHT_ROW_BITS)


def _table_bits(n_bits, what):
  n_bits = int(n_bits)
  if not 1 <= n_bits <= WHT_MAX_BITS:
    raise EngineError(f"{what}: n_bits must be in [1, {WHT_MAX_BITS}], got {n_bits}")
  return n_bits


def walsh_hadamard_(tensor):
  """Unnormalised Walsh-Hadamard transform of a contiguous float32 CUDA tensor of 2^n entries, IN PLACE
  (qhbm_walsh_hadamard): H[y] = sum_m c[m] (-1)^popcount(y & m).  Returns the tensor."""
  if not (torch.is_tensor(tensor) and tensor.is_cuda and tensor.dtype == torch.float32 and tensor.is_contiguous()):
    raise EngineError("walsh_hadamard_ needs a contiguous float32 CUDA tensor")
  size = tensor.numel()
  if size < 2 or size & (size - 1):
    raise EngineError(f"walsh_hadamard_ needs 2^n entries with 1 <= n <= {WHT_MAX_BITS}, got {size}")
  n_bits = _table_bits(size.bit_length() - 1, "walsh_hadamard_")
  with torch.cuda.device(tensor.device):
    _check_global(load_library().qhbm_walsh_hadamard(
        tensor.data_ptr(), n_bits, ctypes.c_void_p(torch.cuda.current_stream(tensor.device).cuda_stream)))
  return tensor


class _ParityTableFunction(torch.autograd.Function):
  """table[y] = sum_k thetas[k] * parity_k(bitstring y) over all 2^n_bits bitstrings by a Walsh-Hadamard transform
  (qhbm_parity_table); the backward is qhbm_parity_table_vjp on the upstream.  `masks` is an int64 CUDA tensor of
  column masks; the table lives on its device."""

  @staticmethod
  def forward(ctx, thetas, masks, n_bits):
    lib = load_library()
    dev = masks.device
    th = thetas.detach().to(device=dev, dtype=torch.float32).contiguous()
    out = torch.empty((1 << n_bits,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
      _check_global(lib.qhbm_parity_table(
          masks.data_ptr(), th.data_ptr(), masks.numel(), n_bits, out.data_ptr(),
          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    ctx.masks, ctx.n_bits = masks, n_bits
    ctx.theta_device = thetas.device
    return out

  @staticmethod
  def backward(ctx, upstream):
    lib = load_library()
    masks, n_bits = ctx.masks, ctx.n_bits
    dev = masks.device
    w = upstream.to(device=dev, dtype=torch.float32).contiguous()
    scratch = torch.empty_like(w)
    grad = torch.empty((masks.numel(),), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
      _check_global(lib.qhbm_parity_table_vjp(
          masks.data_ptr(), masks.numel(), n_bits, w.data_ptr(), scratch.data_ptr(), grad.data_ptr(),
          ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return grad.to(ctx.theta_device), None, None


def parity_table(thetas, masks, n_bits):
  """Differentiable (w.r.t. `thetas`) float32 CUDA table [2^n_bits] of the spin-parity energies of ALL bitstrings, row
  y = the bitstring whose column q is bit n_bits-1-q of y (`energy_utils.all_bitstrings`), for int64 CUDA column `masks`:
  n 2^n additions whatever the number of terms, and no bitstring table.  1 <= n_bits <= 30."""
  n_bits = _table_bits(n_bits, "parity_table")
  if not (torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.int64):
    raise EngineError("parity_table runs on the GPU: pass the column masks as an int64 CUDA tensor")
  masks = masks.contiguous()
  if masks.numel() != thetas.numel():
    raise EngineError(f"parity_table: {masks.numel()} masks for {thetas.numel()} thetas")
  return _ParityTableFunction.apply(thetas, masks, n_bits)


GWG_LDS_MAX = 160 * 1024  # csrc/kernels.h kGwgLdsMax


def gwg_lds_bytes(n_bits, n_terms):
  """LDS one Gibbs-With-Gradients chain needs (csrc/gwg.hip gwg_lds_bytes): the 12-byte term table and one membership
  bitmap over the terms per bit.  More than GWG_LDS_MAX does not run."""
  return (12 * n_terms + 4 * ((n_terms + 31) // 32) * n_bits + 15) & ~15


def gwg_sample(states, n_bits, masks, thetas, seed, step0, n_steps, write_samples=True, count_accepted=False):
  """n_steps Gibbs-With-Gradients steps of the chains `states` (int64 CUDA [n_chains], column q of a bitstring = bit q;
  advanced IN PLACE) under E(x) = sum_k thetas[k] parity_k(x) with int64 CUDA column `masks` (qhbm_gwg_sample).  Step t
  draws the random numbers of absolute step step0 + t.  Returns (samples, accepted): int8 CUDA [n_steps, n_chains, n_bits]
  or None, int32 CUDA [n_chains] or None."""
  lib = load_library()
  if not (states.is_cuda and states.dtype == torch.int64 and states.dim() == 1 and states.is_contiguous()):
    raise EngineError("gwg_sample needs a contiguous int64 CUDA vector of chain states")
  dev = states.device
  masks = masks.to(device=dev, dtype=torch.int64).contiguous()
  th = thetas.detach().to(device=dev, dtype=torch.float32).contiguous()
  if masks.numel() != th.numel():
    raise EngineError(f"gwg_sample: {masks.numel()} masks for {th.numel()} thetas")
  n_chains, n_steps = states.numel(), int(n_steps)
  out = torch.empty((max(n_steps, 0), n_chains, int(n_bits)), dtype=torch.int8, device=dev) if write_samples else None
  acc = torch.zeros((n_chains,), dtype=torch.int32, device=dev) if count_accepted else None
  with torch.cuda.device(dev):
    _check_global(lib.qhbm_gwg_sample(
        states.data_ptr(), n_chains, int(n_bits), masks.data_ptr(), th.data_ptr(), masks.numel(),
        int(seed) & (2**64 - 1), int(step0) & (2**64 - 1), n_steps,
        out.data_ptr() if out is not None else None, acc.data_ptr() if acc is not None else None,
        ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
  return out, acc


def random_states(num_states, n_qubits, seed, first_state=0, device=None):
  """complex64 [num_states, 2^n_qubits] random-sign states of norm 1 with E[|r><r|] = I / 2^n, written by the engine's
  `random_states_kernel` from Philox4x32-10 (include/qhbm_engine.h qhbm_random_states): row m is state
  `first_state` + m of `seed`, whatever the batch it is drawn in."""
  if not torch.cuda.is_available():
    raise EngineError("random_states needs a GPU: the engine has no CPU fallback")
  device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
  out = torch.empty((int(num_states), 1 << int(n_qubits)), dtype=torch.complex64, device=device)
  with torch.cuda.device(device):
    _check_global(load_library().qhbm_random_states(out.data_ptr(), int(num_states), int(n_qubits),
                                                    int(seed) & (2**64 - 1), int(first_state),
                                                    torch.cuda.current_stream().cuda_stream))
  return out


def krylov_combine(basis, coef):
  """out[u, s] = sum_j coef[u, s, j] basis[j, u] for a step-major basis [m, U, 2^n] and coefficients [U, S, m], both
  complex64 on one device: complex64 [U, S, 2^n], every basis word read once per eight outputs (include/qhbm_engine.h
  qhbm_krylov_combine)."""
  if not (torch.is_tensor(basis) and basis.is_cuda and basis.dtype == torch.complex64 and basis.dim() == 3 and basis.is_contiguous()):
    raise EngineError("krylov_combine needs a contiguous complex64 CUDA basis [m, U, 2^n]")
  m, num, dim = (int(v) for v in basis.shape)
  n = dim.bit_length() - 1
  if dim != (1 << n) or n < 1:
    raise ValueError(f"basis rows have {dim} amplitudes: not a power of two")
  coef = torch.as_tensor(coef).to(device=basis.device, dtype=torch.complex64).contiguous()
  if coef.dim() != 3 or coef.shape[0] != num or coef.shape[2] != m:
    raise ValueError(f"coef must have shape [{num}, S, {m}], got {tuple(coef.shape)}")
  out = torch.empty((num, int(coef.shape[1]), dim), dtype=torch.complex64, device=basis.device)
  with torch.cuda.device(basis.device):
    _check_global(load_library().qhbm_krylov_combine(basis.data_ptr(), m, num, n, coef.data_ptr(), int(coef.shape[1]),
                                                     out.data_ptr(), torch.cuda.current_stream().cuda_stream))
  return out


def gram_scratch_bytes(num_states, n_qubits):
  """Bytes of scratch one `qhbm_weighted_gram` of `num_states` states of `n_qubits` qubits needs (no device needed)."""
  out = ctypes.c_size_t()
  _check_global(load_library().qhbm_gram_scratch_bytes(int(num_states), int(n_qubits), ctypes.byref(out)))
  return int(out.value)


def weighted_gram(states, table=None):
  """G[i, j] = sum_x table[x] conj(states[i, x]) states[j, x] (table None: 1) for M device-resident states [M, 2^n]:
  complex128 [M, M], summed in float64 in a fixed order, Hermitian bit for bit with an exactly real diagonal
  (include/qhbm_engine.h qhbm_weighted_gram).  complex128 states and a float64 table are cast to complex64 / float32; the
  scratch is this call's own."""
  if not (torch.is_tensor(states) and states.is_cuda and states.dim() == 2 and states.is_complex()):
    raise EngineError("weighted_gram needs complex CUDA states [M, 2^n]: the engine has no CPU fallback")
  states = states.to(torch.complex64).contiguous()
  num, dim = (int(v) for v in states.shape)
  n = dim.bit_length() - 1
  if dim != (1 << n) or n < 1:
    raise ValueError(f"states have {dim} amplitudes: not a power of two, or fewer than two")
  if table is not None:
    if not (torch.is_tensor(table) and table.is_cuda and table.device == states.device):
      raise EngineError("weighted_gram needs the table on the states' device")
    if tuple(table.shape) != (dim,):
      raise ValueError(f"table must have shape [{dim}], got {tuple(table.shape)}")
    table = table.detach().to(torch.float32).contiguous()
  with torch.cuda.device(states.device):
    scratch = torch.empty(gram_scratch_bytes(num, n) // 8, dtype=torch.float64, device=states.device)
    out = torch.empty((num, num, 2), dtype=torch.float64, device=states.device)
    _check_global(load_library().qhbm_weighted_gram(states.data_ptr(), num, n, None if table is None else table.data_ptr(),
                                                    scratch.data_ptr(), out.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream))
  return torch.view_as_complex(out)


def cross_gram_scratch_bytes(num_bras, num_kets, n_qubits):
  """Bytes of scratch one `qhbm_cross_gram` of `num_bras` x `num_kets` states of `n_qubits` qubits needs (no device needed)."""
  out = ctypes.c_size_t()
  _check_global(load_library().qhbm_cross_gram_scratch_bytes(int(num_bras), int(num_kets), int(n_qubits), ctypes.byref(out)))
  return int(out.value)


def cross_gram(bras, kets, table=None):
  """C[i, j] = sum_x table[x] conj(bras[i, x]) kets[j, x] (table None: 1) for M bras [M, 2^n] and K kets [K, 2^n], both
  device-resident and only read (views of one buffer are fine): complex128 [M, K], every entry summed on its own in float64
  in `weighted_gram`'s order of additions (include/qhbm_engine.h qhbm_cross_gram).  complex128 states and a float64 table
  are cast to complex64 / float32; the scratch is this call's own.  Not differentiable."""
  for name, states in (("bras", bras), ("kets", kets)):
    if not (torch.is_tensor(states) and states.is_cuda and states.dim() == 2 and states.is_complex()):
      raise EngineError(f"cross_gram needs complex CUDA {name} [M, 2^n]: the engine has no CPU fallback")
  if kets.device != bras.device:
    raise EngineError("cross_gram needs bras and kets on one device")
  bras = bras.detach().to(torch.complex64).contiguous()
  kets = kets.detach().to(torch.complex64).contiguous()
  if bras.data_ptr() % 16:  # (a view at an odd offset: the kernel loads 16-byte words)
    bras = bras.clone()
  if kets.data_ptr() % 16:
    kets = kets.clone()
  num, dim = (int(v) for v in bras.shape)
  n = dim.bit_length() - 1
  if dim != (1 << n) or n < 1:
    raise ValueError(f"bras have {dim} amplitudes: not a power of two, or fewer than two")
  if int(kets.shape[1]) != dim:
    raise ValueError(f"bras have {dim} amplitudes, kets {int(kets.shape[1])}")
  num_kets = int(kets.shape[0])
  if table is not None:
    if not (torch.is_tensor(table) and table.is_cuda and table.device == bras.device):
      raise EngineError("cross_gram needs the table on the states' device")
    if table.is_complex() or tuple(table.shape) != (dim,):
      raise ValueError(f"table must be real and have shape [{dim}], got {table.dtype} {tuple(table.shape)}")
    table = table.detach().to(torch.float32).contiguous()
  with torch.cuda.device(bras.device):
    scratch = torch.empty(cross_gram_scratch_bytes(num, num_kets, n) // 8, dtype=torch.float64, device=bras.device)
    out = torch.empty((num, num_kets, 2), dtype=torch.float64, device=bras.device)
    _check_global(load_library().qhbm_cross_gram(bras.data_ptr(), num, kets.data_ptr(), num_kets, n,
                                                 None if table is None else table.data_ptr(), scratch.data_ptr(),
                                                 out.data_ptr(), torch.cuda.current_stream().cuda_stream))
  return torch.view_as_complex(out)


def cross_gram_vjp_scratch_bytes(num_bras, num_kets, n_qubits):
  """Bytes of scratch one `qhbm_cross_gram_vjp` of `num_bras` x `num_kets` states of `n_qubits` qubits needs (no device
  needed)."""
  out = ctypes.c_size_t()
  _check_global(load_library().qhbm_cross_gram_vjp_scratch_bytes(int(num_bras), int(num_kets), int(n_qubits), ctypes.byref(out)))
  return int(out.value)


def cross_gram_vjp(bras, kets, table, cotangent, want_bras=True, want_kets=True, want_table=True):
  """The VJP of `cross_gram` for M bras [M, 2^n], K kets [K, 2^n], its table (None: ones) and torch's cotangent Gamma [M, K]
  of C (used as given): with c[j] = sum_i Gamma[i, j] bras[i],
  (table * sum_j conj(Gamma[i, j]) kets[j] as complex64 [M, 2^n], table * c as complex64 [K, 2^n],
  sum_j Re(conj(c[j]) kets[j]) as float64 [2^n]) -- the cotangents of the bras, of the kets and of the table, from one call
  of the HIP engine (include/qhbm_engine.h qhbm_cross_gram_vjp); an output that is not wanted is None and is not computed.
  complex128 inputs are cast to complex64 and a float64 table to float32; the scratch is this call's own.  Not
  differentiable."""
  for name, states in (("bras", bras), ("kets", kets)):
    if not (torch.is_tensor(states) and states.is_cuda and states.dim() == 2 and states.is_complex()):
      raise EngineError(f"cross_gram_vjp needs complex CUDA {name} [M, 2^n]: the engine has no CPU fallback")
  if kets.device != bras.device:
    raise EngineError("cross_gram_vjp needs bras and kets on one device")
  if not (want_bras or want_kets or want_table):
    raise ValueError("cross_gram_vjp: no output is wanted")
  bras = bras.detach().to(torch.complex64).contiguous()
  kets = kets.detach().to(torch.complex64).contiguous()
  if bras.data_ptr() % 16:  # (a view at an odd offset: the entry point asks for 16-byte alignment)
    bras = bras.clone()
  if kets.data_ptr() % 16:
    kets = kets.clone()
  num, dim = (int(v) for v in bras.shape)
  n = dim.bit_length() - 1
  if dim != (1 << n) or n < 1:
    raise ValueError(f"bras have {dim} amplitudes: not a power of two, or fewer than two")
  if int(kets.shape[1]) != dim:
    raise ValueError(f"bras have {dim} amplitudes, kets {int(kets.shape[1])}")
  num_kets = int(kets.shape[0])
  if table is not None:
    if not (torch.is_tensor(table) and table.is_cuda and table.device == bras.device):
      raise EngineError("cross_gram_vjp needs the table on the states' device")
    if table.is_complex() or tuple(table.shape) != (dim,):
      raise ValueError(f"table must be real and have shape [{dim}], got {table.dtype} {tuple(table.shape)}")
    table = table.detach().to(torch.float32).contiguous()
    if table.data_ptr() % 8:
      table = table.clone()
  cotangent = torch.as_tensor(cotangent)
  if not cotangent.is_complex() or tuple(cotangent.shape) != (num, num_kets):
    raise ValueError(f"cotangent must be complex of shape [{num}, {num_kets}], got {cotangent.dtype} {tuple(cotangent.shape)}")
  cotangent = cotangent.detach().to(device=bras.device, dtype=torch.complex64).contiguous()
  with torch.cuda.device(bras.device):
    scratch = torch.empty(cross_gram_vjp_scratch_bytes(num, num_kets, n) // 8, dtype=torch.float64, device=bras.device)
    out_bras = torch.empty_like(bras) if want_bras else None
    out_kets = torch.empty_like(kets) if want_kets else None
    grad = torch.empty(dim, dtype=torch.float64, device=bras.device) if want_table else None
    _check_global(load_library().qhbm_cross_gram_vjp(
        bras.data_ptr(), num, kets.data_ptr(), num_kets, n, None if table is None else table.data_ptr(), cotangent.data_ptr(),
        None if out_bras is None else out_bras.data_ptr(), None if out_kets is None else out_kets.data_ptr(),
        None if grad is None else grad.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream))
  return out_bras, out_kets, grad


def reduced_density_scratch_bytes(num_states, n_qubits, keep_mask):
  """Bytes of scratch one `qhbm_reduced_density` of `num_states` states of `n_qubits` qubits onto the qubits of
  `keep_mask` (bit q set: qubit q is kept) needs (no device needed)."""
  out = ctypes.c_size_t()
  _check_global(load_library().qhbm_reduced_density_scratch_bytes(int(num_states), int(n_qubits), int(keep_mask),
                                                                  ctypes.byref(out)))
  return int(out.value)


def reduced_density(states, keep_mask, weights=None):
  """rho_A[a, a'] = sum_m weights[m] sum_b states[m, (a, b)] conj(states[m, (a', b)]) (weights None: 1) for M
  device-resident states [M, 2^n] and the kept qubits of `keep_mask` (bit q set: qubit q, the q-th most significant bit of an
  amplitude index, is kept; a reads them big-endian in ascending order): complex128 [2^k, 2^k], summed in float64 in a
  fixed order, Hermitian bit for bit with an exactly real diagonal (include/qhbm_engine.h qhbm_reduced_density).
  complex128 states are cast to complex64 and the weights to float64; the scratch is this call's own.  Not differentiable."""
  if not (torch.is_tensor(states) and states.is_cuda and states.dim() == 2 and states.is_complex()):
    raise EngineError("reduced_density needs complex CUDA states [M, 2^n]: the engine has no CPU fallback")
  states = states.detach().to(torch.complex64).contiguous()
  if states.data_ptr() % 16:  # (a view at an odd offset: the gather loads 16-byte words)
    states = states.clone()
  num, dim = (int(v) for v in states.shape)
  n = dim.bit_length() - 1
  if dim != (1 << n) or n < 1:
    raise ValueError(f"states have {dim} amplitudes: not a power of two, or fewer than two")
  keep_mask = int(keep_mask)
  if keep_mask < 0 or keep_mask >= 1 << 64:
    raise ValueError(f"keep_mask {keep_mask} is not a 64-bit mask")
  if weights is not None:
    weights = torch.as_tensor(weights).detach().to(device=states.device, dtype=torch.float64).contiguous()
    if tuple(weights.shape) != (num,):
      raise ValueError(f"weights must have shape [{num}], got {tuple(weights.shape)}")
  with torch.cuda.device(states.device):
    scratch = torch.empty(reduced_density_scratch_bytes(num, n, keep_mask) // 8, dtype=torch.float64, device=states.device)
    dim_a = 1 << bin(keep_mask).count("1")
    out = torch.empty((dim_a, dim_a, 2), dtype=torch.float64, device=states.device)
    _check_global(load_library().qhbm_reduced_density(states.data_ptr(), num, n, keep_mask,
                                                      None if weights is None else weights.data_ptr(),
                                                      scratch.data_ptr(), out.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream))
  return torch.view_as_complex(out)


def subsystem_apply_scratch_bytes(num_states, n_qubits, keep_mask):
  """Bytes of scratch one `qhbm_subsystem_apply` of `num_states` states of `n_qubits` qubits on the qubits of `keep_mask`
  (bit q set: qubit q is kept) needs (no device needed)."""
  out = ctypes.c_size_t()
  _check_global(load_library().qhbm_subsystem_apply_scratch_bytes(int(num_states), int(n_qubits), int(keep_mask),
                                                                  ctypes.byref(out)))
  return int(out.value)


def subsystem_apply(states, keep_mask, operator, scale=None, want_dots=False):
  """out[m] = scale[m] (operator (x) 1) states[m] (scale None: 1) for M device-resident states [M, 2^n] and a dense
  [2^k, 2^k] operator on the kept qubits of `keep_mask` (as `reduced_density`: bit q set keeps qubit q, rows read the kept
  qubits big-endian in ascending order): complex64 [M, 2^n], f32 arithmetic in a fixed order (include/qhbm_engine.h
  qhbm_subsystem_apply).  With `want_dots` also dots[m] = <states[m]|(operator (x) 1)|states[m]>, taken before scaling,
  complex128 [M].  complex128 states and operators are cast to complex64 and the scale to float64; the scratch is this
  call's own.  Not differentiable."""
  if not (torch.is_tensor(states) and states.is_cuda and states.dim() == 2 and states.is_complex()):
    raise EngineError("subsystem_apply needs complex CUDA states [M, 2^n]: the engine has no CPU fallback")
  states = states.detach().to(torch.complex64).contiguous()
  if states.data_ptr() % 16:  # (a view at an odd offset: the entry point asks for 16-byte alignment)
    states = states.clone()
  num, dim = (int(v) for v in states.shape)
  n = dim.bit_length() - 1
  if dim != (1 << n) or n < 1:
    raise ValueError(f"states have {dim} amplitudes: not a power of two, or fewer than two")
  keep_mask = int(keep_mask)
  if keep_mask < 0 or keep_mask >= 1 << 64:
    raise ValueError(f"keep_mask {keep_mask} is not a 64-bit mask")
  dim_a = 1 << bin(keep_mask).count("1")
  operator = torch.as_tensor(operator)
  if not operator.is_complex() or tuple(operator.shape) != (dim_a, dim_a):
    raise ValueError(f"operator must be complex of shape [{dim_a}, {dim_a}], got {operator.dtype} {tuple(operator.shape)}")
  operator = operator.detach().to(device=states.device, dtype=torch.complex64).contiguous()
  if scale is not None:
    scale = torch.as_tensor(scale).detach().to(device=states.device, dtype=torch.float64).contiguous()
    if tuple(scale.shape) != (num,):
      raise ValueError(f"scale must have shape [{num}], got {tuple(scale.shape)}")
  with torch.cuda.device(states.device):
    scratch = torch.empty(subsystem_apply_scratch_bytes(num, n, keep_mask) // 8, dtype=torch.float64, device=states.device)
    out = torch.empty_like(states)
    dots = torch.empty((num, 2), dtype=torch.float64, device=states.device) if want_dots else None
    _check_global(load_library().qhbm_subsystem_apply(states.data_ptr(), num, n, keep_mask, operator.data_ptr(),
                                                      None if scale is None else scale.data_ptr(), out.data_ptr(),
                                                      None if dots is None else dots.data_ptr(), scratch.data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream))
  return (out, torch.view_as_complex(dots)) if want_dots else out


def gram_vjp_scratch_bytes(num_states, n_qubits):
  """Bytes of scratch one `qhbm_weighted_gram_vjp` of `num_states` states of `n_qubits` qubits needs (no device needed)."""
  out = ctypes.c_size_t()
  _check_global(load_library().qhbm_gram_vjp_scratch_bytes(int(num_states), int(n_qubits), ctypes.byref(out)))
  return int(out.value)


def weighted_gram_vjp(states, table, cotangent, want_states=True, want_table=True):
  """The VJP of `weighted_gram` for M device-resident states [M, 2^n], its table (None: ones) and a cotangent matrix H
  [M, M] (H = Gamma + Gamma^H for torch's cotangent Gamma of G; used as given): with c[j] = sum_i H[i, j] states[i],
  (table * c as complex64 [M, 2^n], 1/2 sum_j Re(conj(c[j]) states[j]) as float64 [2^n]) -- the cotangents of the states and
  of the table, from one pass in the HIP engine (include/qhbm_engine.h qhbm_weighted_gram_vjp); an output that is not
  wanted is None and is not computed.  complex128 inputs are cast to complex64 and a float64 table to float32; the scratch is
  this call's own.  Not differentiable."""
  if not (torch.is_tensor(states) and states.is_cuda and states.dim() == 2 and states.is_complex()):
    raise EngineError("weighted_gram_vjp needs complex CUDA states [M, 2^n]: the engine has no CPU fallback")
  if not (want_states or want_table):
    raise ValueError("weighted_gram_vjp: neither output is wanted")
  states = states.detach().to(torch.complex64).contiguous()
  if states.data_ptr() % 16:  # (a view at an odd offset: the entry point asks for 16-byte alignment)
    states = states.clone()
  num, dim = (int(v) for v in states.shape)
  n = dim.bit_length() - 1
  if dim != (1 << n) or n < 1:
    raise ValueError(f"states have {dim} amplitudes: not a power of two, or fewer than two")
  if table is not None:
    if not (torch.is_tensor(table) and table.is_cuda and table.device == states.device):
      raise EngineError("weighted_gram_vjp needs the table on the states' device")
    if tuple(table.shape) != (dim,):
      raise ValueError(f"table must have shape [{dim}], got {tuple(table.shape)}")
    table = table.detach().to(torch.float32).contiguous()
    if table.data_ptr() % 8:
      table = table.clone()
  cotangent = torch.as_tensor(cotangent)
  if not cotangent.is_complex() or tuple(cotangent.shape) != (num, num):
    raise ValueError(f"cotangent must be complex of shape [{num}, {num}], got {cotangent.dtype} {tuple(cotangent.shape)}")
  cotangent = cotangent.detach().to(device=states.device, dtype=torch.complex64).contiguous()
  with torch.cuda.device(states.device):
    scratch = torch.empty(gram_vjp_scratch_bytes(num, n) // 8, dtype=torch.float64, device=states.device)
    out = torch.empty_like(states) if want_states else None
    grad = torch.empty(dim, dtype=torch.float64, device=states.device) if want_table else None
    _check_global(load_library().qhbm_weighted_gram_vjp(states.data_ptr(), num, n, None if table is None else table.data_ptr(),
                                                        cotangent.data_ptr(), None if out is None else out.data_ptr(),
                                                        None if grad is None else grad.data_ptr(), scratch.data_ptr(),
                                                        torch.cuda.current_stream().cuda_stream))
  return out, grad


def _parity_masks(masks):
  """The masks of a sample_parities call as a HOST uint64 array (the C entries validate them before they launch)."""
  if torch.is_tensor(masks):
    masks = masks.detach().cpu().numpy()
  m = np.asarray(masks)
  if m.ndim != 1 or m.size < 1:
    raise ValueError("masks must be a non-empty 1-D sequence of integers")
  if m.dtype.kind == "i" and (m < 0).any():
    raise ValueError("masks must be non-negative")
  return np.ascontiguousarray(m, dtype=np.uint64)


def sample_parities_scratch_bytes(num_states, n_qubits, n_shots):
  """Bytes of scratch one `qhbm_sample_parities_states` call needs (no device needed)."""
  out = ctypes.c_size_t()
  _check_global(load_library().qhbm_sample_parities_scratch_bytes(int(num_states), int(n_qubits), int(n_shots),
                                                                  ctypes.byref(out)))
  return int(out.value)


def sample_parities_states(states, masks, n_shots, seed=0, first_row=0, program=0):
  """int32 [M, T]: out[m, t] = sum over `n_shots` shots x drawn from |states[m]|^2 (not necessarily normalised) of
  (-1)^popcount(x & masks[t]); bit k of a mask is qubit k, the k-th most significant bit of an amplitude index.  Shot j of
  row m uses the uniform of qhbm_sample_counts with counter words (j, first_row + m, program): row m of a call equals a
  one-state call with first_row = m, bit for bit (include/qhbm_engine.h qhbm_sample_parities_states).  complex128 states
  are cast to complex64; the scratch is this call's own.  Not differentiable."""
  if not (torch.is_tensor(states) and states.is_cuda and states.dim() == 2 and states.is_complex()):
    raise EngineError("sample_parities_states needs complex CUDA states [M, 2^n]: the engine has no CPU fallback")
  states = states.detach().to(torch.complex64).contiguous()
  if states.data_ptr() % 16:
    states = states.clone()
  num, dim = (int(v) for v in states.shape)
  n = dim.bit_length() - 1
  if dim != (1 << n) or n < 1:
    raise ValueError(f"states have {dim} amplitudes: not a power of two, or fewer than two")
  m = _parity_masks(masks)
  with torch.cuda.device(states.device):
    scratch = torch.empty(sample_parities_scratch_bytes(num, n, n_shots) // 8, dtype=torch.float64, device=states.device)
    out = torch.empty((num, len(m)), dtype=torch.int32, device=states.device)
    _check_global(load_library().qhbm_sample_parities_states(
        states.data_ptr(), num, n, m.ctypes.data, len(m), int(n_shots), int(seed) & (2**64 - 1), int(first_row),
        int(program), scratch.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream))
  return out


class Engine:
  """One engine per device.  `device=None` makes a planning-only engine
  (schedules can be inspected, compute calls raise)."""

  def __init__(self, device=0):
    self._lib = load_library()
    self._h = ctypes.c_void_p()
    dev = -1 if device is None else int(device)
    if self._lib.qhbm_create(dev, ctypes.byref(self._h)) != 0:
      raise EngineError(self._lib.qhbm_last_error(None).decode())
    self.device = None if device is None else torch.device("cuda", dev)
    self.n_qubits = 0
    self.n_params = 0
    self.n_ops = 0
    self.retained = None

  def close(self):
    if getattr(self, "_h", None) is not None and self._h:
      self._lib.qhbm_destroy(self._h)
      self._h = None

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint: disable=broad-except
      pass

  def _check(self, rc):
    if rc != 0:
      raise EngineError(self._lib.qhbm_last_error(self._h).decode())

  # ---- model -------------------------------------------------------------
  def _setter_done(self):
    """A setter that invalidates a plan drops the retained states (include/qhbm_engine.h): the token follows."""
    if self.retained is not None and self.retained_states() == 0:
      self.retained = None

  def set_circuit(self, n_qubits, gates, n_params):
    """gates: iterable of (kind, q0, q1, param_idx, scalar, offset[, global_shift])."""
    gates = list(gates)
    arr = (QhbmGate * max(len(gates), 1))()
    for i, g in enumerate(gates):
      kind, q0, q1, pidx, scalar, offset = g[:6]
      arr[i] = QhbmGate(int(kind), int(q0), int(q1), int(pidx), float(scalar),
                        float(offset), float(g[6]) if len(g) > 6 else 0.0)
    self._check(
        self._lib.qhbm_set_circuit(self._h, int(n_qubits), len(gates), arr,
                                   int(n_params)))
    if n_qubits != self.n_qubits:
      self.n_ops = 0
    self.n_qubits, self.n_params = int(n_qubits), int(n_params)
    self._grad_mask = None  # (qhbm_set_circuit resets the engine's mask)
    self._setter_done()

  def set_observables(self, ops):
    """ops: list of ops, each a list of (coeff, x_mask, z_mask), qubit space."""
    offsets = [0]
    coeffs, xs, zs = [], [], []
    for op in ops:
      for coeff, x, z in op:
        coeffs.append(coeff)
        xs.append(x)
        zs.append(z)
      offsets.append(len(coeffs))
    off = np.asarray(offsets, dtype=np.int32)
    cf = np.asarray(coeffs, dtype=np.float32)
    xm = np.asarray(xs, dtype=np.uint64)
    zm = np.asarray(zs, dtype=np.uint64)
    self._check(
        self._lib.qhbm_set_observables(self._h, len(ops), off.ctypes.data,
                                       cf.ctypes.data, xm.ctypes.data,
                                       zm.ctypes.data))
    self.n_ops = len(ops)
    self._setter_done()

  def set_gradient_mask(self, needs_grad):
    """needs_grad: one truth value per parameter (None: all).  Frozen parameters get zero gradient entries and no
    gradient work; the adjoint sweep stops at the first gate of a parameter that is not frozen
    (include/qhbm_engine.h qhbm_set_gradient_mask).  Reset by set_circuit."""
    key = None if needs_grad is None else tuple(bool(f) for f in needs_grad)
    if key == getattr(self, "_grad_mask", None):
      return
    if key is None:
      self._check(self._lib.qhbm_set_gradient_mask(self._h, None, 0))
    else:
      mask = np.ascontiguousarray(np.asarray(key, dtype=np.uint8))
      if mask.shape != (self.n_params,):
        raise EngineError(f"gradient mask of shape {mask.shape} for {self.n_params} parameters")
      self._check(self._lib.qhbm_set_gradient_mask(self._h, mask.ctypes.data, self.n_params))
    self._grad_mask = key
    self._setter_done()

  def set_option(self, name, value):
    self._check(self._lib.qhbm_set_option(self._h, name.encode(), int(value)))
    self._setter_done()

  # ---- introspection -------------------------------------------------------
  def num_passes(self):
    f, b = ctypes.c_int(), ctypes.c_int()
    self._check(self._lib.qhbm_num_passes(self._h, ctypes.byref(f),
                                          ctypes.byref(b)))
    return f.value, b.value

  def describe_schedule(self):
    buf = ctypes.create_string_buffer(1 << 16)
    self._check(self._lib.qhbm_describe_schedule(self._h, buf, len(buf)))
    return buf.value.decode()

  def workspace_bytes(self, num_states, with_vjp=False):
    out = ctypes.c_size_t()
    self._check(
        self._lib.qhbm_workspace_bytes(self._h, int(num_states), int(with_vjp),
                                       ctypes.byref(out)))
    return out.value

  def allocated_bytes(self):
    """Device memory this engine holds right now (workspace + gradient partials)."""
    out = ctypes.c_size_t()
    self._check(self._lib.qhbm_allocated_bytes(self._h, ctypes.byref(out)))
    return out.value

  def retained_states(self):
    """Number of final states the workspace keeps for `expectation_vjp_retained` (0: none)."""
    out = ctypes.c_int()
    self._check(self._lib.qhbm_retained_states(self._h, ctypes.byref(out)))
    return out.value

  def kernel_time_ms(self, reset=True):
    f, b, o = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    nf, nb, no = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    self._check(
        self._lib.qhbm_kernel_time_ms(self._h, int(reset), ctypes.byref(f),
                                      ctypes.byref(nf), ctypes.byref(b),
                                      ctypes.byref(nb), ctypes.byref(o), ctypes.byref(no)))
    return {"fwd_ms": f.value, "fwd_launches": nf.value, "bwd_ms": b.value,
            "bwd_launches": nb.value, "obs_ms": o.value, "obs_launches": no.value}

  def traffic_model(self, num_states, with_vjp=True):
    """HBM bytes one call must move (every touched tile read and written once): dict of
    forward / lambda = O psi / adjoint bytes (include/qhbm_engine.h qhbm_traffic_model)."""
    f, o, b = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    self._check(self._lib.qhbm_traffic_model(self._h, int(num_states), int(with_vjp), ctypes.byref(f),
                                             ctypes.byref(o), ctypes.byref(b)))
    return {"fwd_bytes": f.value, "obs_bytes": o.value, "bwd_bytes": b.value}

  def flop_model(self, num_states, with_vjp=True):
    """fp32 operations (FMA = 2) of the gate arithmetic of one call: dict of forward / lambda = O psi /
    adjoint flops (include/qhbm_engine.h qhbm_flop_model)."""
    f, o, b = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    self._check(self._lib.qhbm_flop_model(self._h, int(num_states), int(with_vjp), ctypes.byref(f),
                                          ctypes.byref(o), ctypes.byref(b)))
    return {"fwd_flops": f.value, "obs_flops": o.value, "bwd_flops": b.value}

  def plan_builds(self):
    """(forward, backward) plan searches run so far (include/qhbm_engine.h qhbm_plan_builds)."""
    f, b = ctypes.c_int64(), ctypes.c_int64()
    self._check(self._lib.qhbm_plan_builds(self._h, ctypes.byref(f), ctypes.byref(b)))
    return f.value, b.value

  def clock_probe(self):
    """The chip's sustained packed-fp32 rate right now: dict of `ghz` (shader clock during the probe),
    `cycles_per_pk_fma` and `tflops` (include/qhbm_engine.h qhbm_clock_probe).  Synchronises the stream."""
    if self.device is None:
      raise EngineError("planning-only engine: no device, no CPU fallback")
    g, c, t = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    self._check(self._lib.qhbm_clock_probe(self._h, ctypes.byref(g), ctypes.byref(c), ctypes.byref(t), self._stream()))
    return {"ghz": g.value, "cycles_per_pk_fma": c.value, "tflops": t.value}

  CENSUS_COLUMNS = ("tiles", "rounds", "rounds_barrier", "rounds_no_barrier", "instances", "x", "x_no_slot", "full",
                    "ph1", "ph2", "cph_tile_on", "cph_wave_on", "cph_lane", "cph_off", "reduce8", "level1")

  def op_census(self, adjoint=True, max_passes=64):
    """Executed micro-ops per pass in wave-executions per state (include/qhbm_engine.h qhbm_op_census):
    a list of dicts, one per pass of the forward or backward schedule."""
    import numpy as np  # pylint: disable=import-outside-toplevel
    try:  # the library's own row stride; one from before the entry point writes 15 columns (A/B runs: QHBM_ENGINE_LIB)
      ncol = int(self._lib.qhbm_census_columns())
    except AttributeError:
      ncol = 15
    out = np.zeros((max_passes, ncol), np.float64)
    n = ctypes.c_int()
    self._check(self._lib.qhbm_op_census(self._h, int(bool(adjoint)), max_passes,
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(n)))
    names = self.CENSUS_COLUMNS  # (a column the library does not have yet reads 0)
    return [{name: (out[i, c] if c < ncol else 0.0) for c, name in enumerate(names)} for i in range(min(n.value, max_passes))]

  # ---- hot path --------------------------------------------------------------
  def _prep(self, bits, params):
    if self.device is None:
      raise EngineError("planning-only engine: no device, no CPU fallback")
    bits = torch.as_tensor(bits).to(device=self.device, dtype=torch.int8)
    bits = bits.contiguous()
    if bits.dim() != 2 or bits.shape[1] != self.n_qubits:
      raise ValueError(
          f"bitstrings must have shape [batch, {self.n_qubits}], got "
          f"{tuple(bits.shape)}")
    params = torch.as_tensor(params).to(device=self.device,
                                        dtype=torch.float32).contiguous()
    if params.numel() != self.n_params:
      raise ValueError(f"expected {self.n_params} parameters")
    return bits, params

  def _stream(self):
    return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

  def expectation(self, bits, params, retain=False):
    """Values [batch, n_ops].  With `retain`, the final states stay in the workspace for one
    `expectation_vjp_retained` (same bits and params); `self.retained` is then a token, or None
    when the batch was too large to keep."""
    bits, params = self._prep(bits, params)
    out = torch.empty((bits.shape[0], self.n_ops), dtype=torch.float32,
                      device=self.device)
    fn = self._lib.qhbm_expectation_retain if retain else self._lib.qhbm_expectation
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(fn(self._h, bits.data_ptr(), bits.shape[0], params.data_ptr(), out.data_ptr(),
                     self._stream()))
    # (the C side keeps nothing when the batch exceeds one backward chunk: ask, do not assume)
    if retain and bits.shape[0] > 0 and self.retained_states() == bits.shape[0]:
      self._retain_count = getattr(self, "_retain_count", 0) + 1
      self.retained = self._retain_count
    return out

  def expectation_vjp_retained(self, bits, params, upstream):
    """grad[n_params] from the states kept by `expectation(..., retain=True)`; raises
    EngineError if they are gone (then call `expectation_vjp`)."""
    bits, params = self._prep(bits, params)
    upstream = torch.as_tensor(upstream).to(
        device=self.device, dtype=torch.float32).contiguous()
    if tuple(upstream.shape) != (bits.shape[0], self.n_ops):
      raise ValueError("upstream must have shape [batch, n_ops]")
    grad = torch.zeros((self.n_params,), dtype=torch.float32, device=self.device)
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(
          self._lib.qhbm_expectation_vjp_retained(self._h, bits.data_ptr(), bits.shape[0],
                                                  params.data_ptr(), upstream.data_ptr(),
                                                  grad.data_ptr(), self._stream()))
    return grad

  def expectation_vjp(self, bits, params, upstream, method=GRAD_ADJOINT):
    self.retained = None
    bits, params = self._prep(bits, params)
    upstream = torch.as_tensor(upstream).to(
        device=self.device, dtype=torch.float32).contiguous()
    if tuple(upstream.shape) != (bits.shape[0], self.n_ops):
      raise ValueError("upstream must have shape [batch, n_ops]")
    vals = torch.empty((bits.shape[0], self.n_ops), dtype=torch.float32,
                       device=self.device)
    grad = torch.zeros((self.n_params,), dtype=torch.float32,
                       device=self.device)
    with torch.cuda.device(self.device):
      self._check(
          self._lib.qhbm_expectation_vjp(self._h, bits.data_ptr(),
                                         bits.shape[0], params.data_ptr(),
                                         upstream.data_ptr(), vals.data_ptr(),
                                         grad.data_ptr(), int(method),
                                         self._stream()))
    return vals, grad

  def _table(self, table):
    table = torch.as_tensor(table).to(device=self.device, dtype=torch.float32).contiguous()
    if table.numel() != (1 << self.n_qubits):
      raise ValueError(f"an energy table has 2^{self.n_qubits} = {1 << self.n_qubits} entries, got {table.numel()}")
    return table

  def _table_upstream(self, upstream, batch):
    upstream = torch.as_tensor(upstream).to(device=self.device, dtype=torch.float32).contiguous()
    if upstream.numel() != batch:
      raise ValueError(f"upstream must have {batch} entries (one per state), got {tuple(upstream.shape)}")
    return upstream

  def table_expectation(self, bits, params, table, retain=False):
    """Values [batch] of the diagonal observable sum_y table[y] |y><y| (table [2^n], indexed like `statevector`).
    Needs no installed observables.  With `retain` the final states stay for one `table_expectation_vjp_retained`
    (`self.retained` is then a token, or None when the batch was too large to keep)."""
    bits, params = self._prep(bits, params)
    table = self._table(table)
    out = torch.empty((bits.shape[0],), dtype=torch.float32, device=self.device)
    fn = self._lib.qhbm_table_expectation_retain if retain else self._lib.qhbm_table_expectation
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(fn(self._h, bits.data_ptr(), bits.shape[0], params.data_ptr(), table.data_ptr(), out.data_ptr(),
                     self._stream()))
    if retain and bits.shape[0] > 0 and self.retained_states() == bits.shape[0]:
      self._retain_count = getattr(self, "_retain_count", 0) + 1
      self.retained = self._retain_count
    return out

  def table_expectation_vjp(self, bits, params, table, upstream, table_grad=True):
    """(vals [batch], grad [n_params], table_grad [2^n] or None) for the upstream [batch] of `table_expectation`."""
    self.retained = None
    bits, params = self._prep(bits, params)
    table = self._table(table)
    upstream = self._table_upstream(upstream, bits.shape[0])
    vals = torch.empty((bits.shape[0],), dtype=torch.float32, device=self.device)
    grad = torch.zeros((self.n_params,), dtype=torch.float32, device=self.device)
    tgrad = torch.empty((1 << self.n_qubits,), dtype=torch.float32, device=self.device) if table_grad else None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_table_expectation_vjp(
          self._h, bits.data_ptr(), bits.shape[0], params.data_ptr(), table.data_ptr(), upstream.data_ptr(),
          vals.data_ptr(), grad.data_ptr(), tgrad.data_ptr() if tgrad is not None else None, self._stream()))
    return vals, grad, tgrad

  def table_expectation_vjp_retained(self, bits, params, table, upstream, table_grad=True):
    """(grad [n_params], table_grad [2^n] or None) from the states kept by `table_expectation(..., retain=True)`;
    raises EngineError if they are gone (then call `table_expectation_vjp`)."""
    bits, params = self._prep(bits, params)
    table = self._table(table)
    upstream = self._table_upstream(upstream, bits.shape[0])
    grad = torch.zeros((self.n_params,), dtype=torch.float32, device=self.device)
    tgrad = torch.empty((1 << self.n_qubits,), dtype=torch.float32, device=self.device) if table_grad else None
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_table_expectation_vjp_retained(
          self._h, bits.data_ptr(), bits.shape[0], params.data_ptr(), table.data_ptr(), upstream.data_ptr(),
          grad.data_ptr(), tgrad.data_ptr() if tgrad is not None else None, self._stream()))
    return grad, tgrad

  def state_gradients(self, num_states):
    """[num_states, n_params] rows of the last adjoint VJP (their sum over states is its gradient)."""
    rows = torch.empty((int(num_states), self.n_params), dtype=torch.float32, device=self.device)
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_state_gradients(self._h, int(num_states), rows.data_ptr(), self._stream()))
    return rows

  def statevector(self, bits, params):
    """Final states C(params)|x_u>, complex64 [batch, 2^n] (qubit 0 = most significant bit)."""
    self.retained = None
    bits, params = self._prep(bits, params)
    out = torch.empty((bits.shape[0], 1 << self.n_qubits), dtype=torch.complex64,
                      device=self.device)
    with torch.cuda.device(self.device):
      self._check(
          self._lib.qhbm_statevector(self._h, bits.data_ptr(), bits.shape[0],
                                     params.data_ptr(), out.data_ptr(),
                                     self._stream()))
    return out

  # ---- circuits that start from caller-supplied states (include/qhbm_engine.h) ----
  def describe_schedule_from_states(self):
    """The dense-start plans the from-states calls run (works without a device)."""
    buf = ctypes.create_string_buffer(1 << 16)
    self._check(self._lib.qhbm_describe_schedule_from_states(self._h, buf, len(buf)))
    return buf.value.decode()

  def _prep_states(self, states, params):
    if self.device is None:
      raise EngineError("planning-only engine: no device, no CPU fallback")
    states = torch.as_tensor(states)
    if not states.is_complex():
      raise ValueError("states must be a complex tensor of shape [batch, 2^n]")
    if states.dim() != 2 or states.shape[1] != (1 << self.n_qubits):
      raise ValueError(f"states must have shape [batch, {1 << self.n_qubits}], got {tuple(states.shape)}")
    states = states.to(device=self.device, dtype=torch.complex64).contiguous()
    if states.data_ptr() % 16:  # (a view at an odd offset: the import loads 16-byte words)
      states = states.clone()
    params = torch.as_tensor(params).to(device=self.device, dtype=torch.float32).contiguous()
    if params.numel() != self.n_params:
      raise ValueError(f"expected {self.n_params} parameters")
    return states, params

  def expectation_from_states(self, states, params):
    """Values [batch, n_ops] of <phi_u| C^dagger O_k C |phi_u> for states [batch, 2^n] complex64 in the layout of
    `statevector`; not divided by the norm, the input is never written."""
    states, params = self._prep_states(states, params)
    out = torch.empty((states.shape[0], self.n_ops), dtype=torch.float32, device=self.device)
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_expectation_from_states(self._h, states.data_ptr(), states.shape[0], params.data_ptr(),
                                                         out.data_ptr(), self._stream()))
    return out

  def expectation_vjp_from_states(self, states, params, upstream):
    """(vals [batch, n_ops], grad [n_params]) by the adjoint method; the gradient mask applies as in
    `expectation_vjp`, and `state_gradients` then serves this call's rows."""
    states, params = self._prep_states(states, params)
    upstream = torch.as_tensor(upstream).to(device=self.device, dtype=torch.float32).contiguous()
    if tuple(upstream.shape) != (states.shape[0], self.n_ops):
      raise ValueError("upstream must have shape [batch, n_ops]")
    vals = torch.empty((states.shape[0], self.n_ops), dtype=torch.float32, device=self.device)
    grad = torch.zeros((self.n_params,), dtype=torch.float32, device=self.device)
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_expectation_vjp_from_states(
          self._h, states.data_ptr(), states.shape[0], params.data_ptr(), upstream.data_ptr(), vals.data_ptr(),
          grad.data_ptr(), self._stream()))
    return vals, grad

  def statevector_from_states(self, states, params):
    """C(params)|phi_u>, complex64 [batch, 2^n], global phase as `statevector`."""
    states, params = self._prep_states(states, params)
    out = torch.empty((states.shape[0], 1 << self.n_qubits), dtype=torch.complex64, device=self.device)
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_statevector_from_states(self._h, states.data_ptr(), states.shape[0], params.data_ptr(),
                                                         out.data_ptr(), self._stream()))
    return out

  def statevector_vjp_from_states(self, states, params, cotangent, want_states=False):
    """The adjoint VJP of the final states psi = `statevector_from_states(states, params)`: grad [n_params] =
    sum_u Re<g_u| d psi_u / d params> for the cotangent g [batch, 2^n] (dL/dRe psi + i dL/dIm psi of a real loss L, torch's
    convention; complex128 is cast).  `want_states`: (psi, grad), psi from the same forward.  No observables needed; the
    gradient mask applies; `state_gradients` is refused after this call."""
    states, params = self._prep_states(states, params)
    cotangent = torch.as_tensor(cotangent)
    if not cotangent.is_complex() or tuple(cotangent.shape) != tuple(states.shape):
      raise ValueError(f"cotangent must be a complex tensor of shape {tuple(states.shape)}")
    cotangent = cotangent.to(device=self.device, dtype=torch.complex64).contiguous()
    if cotangent.data_ptr() % 16:
      cotangent = cotangent.clone()
    out = torch.empty_like(states) if want_states else None
    grad = torch.zeros((self.n_params,), dtype=torch.float32, device=self.device)
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_statevector_vjp_from_states(
          self._h, states.data_ptr(), states.shape[0], params.data_ptr(), cotangent.data_ptr(),
          None if out is None else out.data_ptr(), grad.data_ptr(), self._stream()))
    return (out, grad) if want_states else grad

  # ---- evolving caller-supplied states under H = sum_k w_k O_k of the installed observables ----
  def _weights(self, weights):
    if weights is None:
      return None
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    if w.shape != (self.n_ops,):
      raise ValueError(f"{w.shape[0]} weights for {self.n_ops} observables")
    return w

  def describe_evolution(self, tau, mode=0, weights=None):
    """{"R", "steps", "terms_per_step", "applications"} of `evolve_states(..., tau, mode, weights)`; needs no device."""
    w = self._weights(weights)
    buf = ctypes.create_string_buffer(256)
    self._check(self._lib.qhbm_describe_evolution(self._h, None if w is None else w.ctypes.data, float(tau), int(mode),
                                                  buf, len(buf)))
    fields = dict(item.split("=") for item in buf.value.decode().split())
    return {k: float(v) if k == "R" else int(v) for k, v in fields.items()}

  def apply_observables(self, states, weights=None):
    """H phi_u for states [batch, 2^n] complex64, H = sum_k weights[k] O_k (default: all ones); a new tensor."""
    states, _ = self._prep_states(states, np.zeros(self.n_params, np.float32))
    w = self._weights(weights)
    out = torch.empty_like(states)
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_apply_observables(self._h, states.data_ptr(), states.shape[0],
                                                   None if w is None else w.ctypes.data, out.data_ptr(), self._stream()))
    return out

  def evolve_states(self, states, tau, mode=0, weights=None, in_place=False):
    """mode 0: (e^{-tau H} phi_u normalised, float64 [batch] log ||e^{-tau H} phi_u|| of the states as given);
    mode 1: (e^{-i tau H} phi_u, None).  The input is copied unless `in_place` (then it must be a contiguous, 16-byte
    aligned complex64 tensor on the engine's device, and is overwritten)."""
    given = states
    states, _ = self._prep_states(states, np.zeros(self.n_params, np.float32))
    if in_place:
      if states.data_ptr() != torch.as_tensor(given).data_ptr():
        raise ValueError("in_place needs a contiguous, 16-byte aligned complex64 tensor on the engine's device")
    elif torch.is_tensor(given) and states.data_ptr() == given.data_ptr():
      states = states.clone()
    w = self._weights(weights)
    log_norms = torch.empty((states.shape[0],), dtype=torch.float64, device=self.device) if int(mode) == 0 else None
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_evolve_states(self._h, states.data_ptr(), states.shape[0],
                                               None if w is None else w.ctypes.data, float(tau), int(mode),
                                               None if log_norms is None else log_norms.data_ptr(), self._stream()))
    return states, log_norms

  def describe_krylov(self, num_states, num_steps, reorthogonalise=True):
    """{"basis_bytes", "workspace_bytes", "applications", "chunk_states", "krylov_bytes_per_state"} of
    `krylov_basis` on `num_states` states; needs no device."""
    buf = ctypes.create_string_buffer(512)
    self._check(self._lib.qhbm_describe_krylov(self._h, int(num_states), int(num_steps), int(bool(reorthogonalise)), buf, len(buf)))
    fields = dict(item.split("=") for item in buf.value.decode().split())
    return {k: int(v) if k in ("applications", "chunk_states") else float(v) for k, v in fields.items()}

  def krylov_basis(self, states, num_steps, weights=None, reorthogonalise=True):
    """(basis [m, batch, 2^n] complex64 step-major, alpha [batch, m], beta [batch, m] float64, lengths [batch] int32,
    start norms [batch] float64), all on the device: the Lanczos recurrence of H = sum_k weights[k] O_k from each state
    (include/qhbm_engine.h qhbm_krylov_basis).  The input is never written."""
    states, _ = self._prep_states(states, np.zeros(self.n_params, np.float32))
    w = self._weights(weights)
    m, num = int(num_steps), states.shape[0]
    if not 1 <= m <= 1024:
      raise ValueError("num_steps must be in [1, 1024]")
    basis = torch.empty((m, num, 1 << self.n_qubits), dtype=torch.complex64, device=self.device)
    alpha = torch.empty((num, m), dtype=torch.float64, device=self.device)
    beta = torch.empty((num, m), dtype=torch.float64, device=self.device)
    lengths = torch.empty((num,), dtype=torch.int32, device=self.device)
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_krylov_basis(self._h, states.data_ptr(), num, None if w is None else w.ctypes.data, m,
                                              int(bool(reorthogonalise)), basis.data_ptr(), alpha.data_ptr(), beta.data_ptr(),
                                              lengths.data_ptr(), self._stream()))
    norms = torch.linalg.vector_norm(torch.view_as_real(states).flatten(1), dim=1, dtype=torch.float64)
    return basis, alpha, beta, lengths, norms

  def describe_krylov_stream(self, num_states, num_steps, num_outputs=1):
    """{"workspace_bytes", "chunk_states", "tridiagonal_applications", "replay_applications", "tridiagonal_bytes_per_state",
    "replay_bytes_per_state"} of `krylov_tridiagonal` and of a `krylov_replay` of `num_outputs` outputs per state on
    `num_states` states; needs no device."""
    buf = ctypes.create_string_buffer(512)
    self._check(self._lib.qhbm_describe_krylov_stream(self._h, int(num_states), int(num_steps), int(num_outputs), buf, len(buf)))
    fields = dict(item.split("=") for item in buf.value.decode().split())
    return {k: float(v) if k.endswith("bytes") or k.endswith("per_state") else int(v) for k, v in fields.items()}

  def krylov_tridiagonal(self, states, num_steps, weights=None):
    """Pass one of the streamed Lanczos recurrence (include/qhbm_engine.h qhbm_krylov_tridiagonal): (alpha [batch, m], beta
    [batch, m] float64, lengths [batch] int32, recurrence [batch, m, 2] complex64, start norms [batch] float64), all on the
    device.  alpha, beta and lengths are bit for bit those of `krylov_basis(reorthogonalise=False)`; no basis is stored.
    The input is never written."""
    states, _ = self._prep_states(states, np.zeros(self.n_params, np.float32))
    w = self._weights(weights)
    m, num = int(num_steps), states.shape[0]
    if not 1 <= m <= 1024:
      raise ValueError("num_steps must be in [1, 1024]")
    alpha = torch.empty((num, m), dtype=torch.float64, device=self.device)
    beta = torch.empty((num, m), dtype=torch.float64, device=self.device)
    lengths = torch.empty((num,), dtype=torch.int32, device=self.device)
    recurrence = torch.empty((num, m, 2), dtype=torch.complex64, device=self.device)
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_krylov_tridiagonal(self._h, states.data_ptr(), num, None if w is None else w.ctypes.data, m,
                                                    alpha.data_ptr(), beta.data_ptr(), lengths.data_ptr(),
                                                    recurrence.data_ptr(), self._stream()))
    norms = torch.linalg.vector_norm(torch.view_as_real(states).flatten(1), dim=1, dtype=torch.float64)
    return alpha, beta, lengths, recurrence, norms

  def krylov_replay(self, states, beta, lengths, recurrence, coef, weights=None):
    """Pass two (qhbm_krylov_replay): out[u, s] = sum_j coef[u, s, j] v_j(u), complex64 [batch, S, 2^n], for coefficients
    [batch, S, m]; the v_j are regenerated from the SAME `states` and `weights` and from what `krylov_tridiagonal` returned
    for them.  The input is never written."""
    states, _ = self._prep_states(states, np.zeros(self.n_params, np.float32))
    w = self._weights(weights)
    num = states.shape[0]
    beta = torch.as_tensor(beta).to(device=self.device, dtype=torch.float64).contiguous()
    if beta.dim() != 2 or beta.shape[0] != num or not 1 <= beta.shape[1] <= 1024:
      raise ValueError(f"beta must have shape [{num}, m] with m in [1, 1024], got {tuple(beta.shape)}")
    m = int(beta.shape[1])
    lengths = torch.as_tensor(lengths).to(device=self.device, dtype=torch.int32).contiguous()
    recurrence = torch.as_tensor(recurrence).to(device=self.device, dtype=torch.complex64).contiguous()
    coef = torch.as_tensor(coef).to(device=self.device, dtype=torch.complex64).contiguous()
    if tuple(lengths.shape) != (num,) or tuple(recurrence.shape) != (num, m, 2):
      raise ValueError(f"lengths must have shape [{num}] and recurrence [{num}, {m}, 2]")
    if coef.dim() != 3 or coef.shape[0] != num or coef.shape[1] < 1 or coef.shape[2] != m:
      raise ValueError(f"coef must have shape [{num}, S, {m}] with S >= 1, got {tuple(coef.shape)}")
    out = torch.empty((num, int(coef.shape[1]), 1 << self.n_qubits), dtype=torch.complex64, device=self.device)
    self.retained = None
    with torch.cuda.device(self.device):
      self._check(self._lib.qhbm_krylov_replay(self._h, states.data_ptr(), num, None if w is None else w.ctypes.data, m,
                                               beta.data_ptr(), lengths.data_ptr(), recurrence.data_ptr(), coef.data_ptr(),
                                               int(coef.shape[1]), out.data_ptr(), self._stream()))
    return out

  def sample(self, bits, params, n_shots, seed=0, shift_gate=-1, shift=0.0):
    """int8 [batch, n_shots, n_qubits]: computational-basis samples of C(params)|x_u>;
    `shift_gate`/`shift` select one parameter-shifted program (see include/qhbm_engine.h)."""
    self.retained = None
    bits, params = self._prep(bits, params)
    out = torch.empty((bits.shape[0], int(n_shots), self.n_qubits), dtype=torch.int8,
                      device=self.device)
    with torch.cuda.device(self.device):
      self._check(
          self._lib.qhbm_sample(self._h, bits.data_ptr(), bits.shape[0], params.data_ptr(),
                                int(n_shots), int(seed) & (2**64 - 1), int(shift_gate),
                                float(shift), out.data_ptr(), self._stream()))
    return out

  def sample_counts(self, bits, params, n_shots, seed=0, shift_gates=(-1,), shifts=(0.0,)):
    """int32 [n_programs, batch, 2^n]: how many of `n_shots` shots of every (shifted program, state)
    pair gave each outcome -- all programs in one launch set (include/qhbm_engine.h qhbm_sample_counts)."""
    self.retained = None
    bits, params = self._prep(bits, params)
    sg = np.ascontiguousarray(shift_gates, dtype=np.int32)
    sv = np.ascontiguousarray(shifts, dtype=np.float32)
    if sg.shape != sv.shape or sg.ndim != 1:
      raise ValueError("shift_gates and shifts must be 1-D and of equal length")
    out = torch.empty((len(sg), bits.shape[0], 1 << self.n_qubits), dtype=torch.int32, device=self.device)
    with torch.cuda.device(self.device):
      self._check(
          self._lib.qhbm_sample_counts(self._h, bits.data_ptr(), bits.shape[0], params.data_ptr(), len(sg),
                                       sg.ctypes.data, sv.ctypes.data, int(n_shots), int(seed) & (2**64 - 1),
                                       out.data_ptr(), self._stream()))
    return out

  def sample_parities(self, bits, params, masks, n_shots, seed=0, shift_gates=(-1,), shifts=(0.0,)):
    """int32 [n_programs, batch, T]: sum over `n_shots` shots of (-1)^popcount(x & masks[t]) for every (shifted program,
    state) pair, all programs in one launch set and at any register width: neither shots nor per-outcome counters are
    stored (include/qhbm_engine.h qhbm_sample_parities).  Bit k of a mask is qubit k; the uniforms are those of
    `sample_counts`."""
    self.retained = None
    bits, params = self._prep(bits, params)
    sg = np.ascontiguousarray(shift_gates, dtype=np.int32)
    sv = np.ascontiguousarray(shifts, dtype=np.float32)
    if sg.shape != sv.shape or sg.ndim != 1:
      raise ValueError("shift_gates and shifts must be 1-D and of equal length")
    m = _parity_masks(masks)
    out = torch.empty((len(sg), bits.shape[0], len(m)), dtype=torch.int32, device=self.device)
    with torch.cuda.device(self.device):
      self._check(
          self._lib.qhbm_sample_parities(self._h, bits.data_ptr(), bits.shape[0], params.data_ptr(), len(sg),
                                         sg.ctypes.data, sv.ctypes.data, m.ctypes.data, len(m), int(n_shots),
                                         int(seed) & (2**64 - 1), out.data_ptr(), self._stream()))
    return out

  def program_vjps(self, bits, params, shift_gates, shifts, upstream, row_weights=None):
    """(prog_vals [n_programs, n_ops], prog_grad [n_programs, n_params]): one adjoint VJP of `upstream` per
    parameter-shifted program -- `shifts[q]` added to the exponent of gate `shift_gates[q]`, a negative gate = the
    unshifted circuit -- and the row-weighted sums of its values, all programs in one launch set
    (include/qhbm_engine.h qhbm_program_vjps)."""
    self.retained = None
    bits, params = self._prep(bits, params)
    sg = np.ascontiguousarray(shift_gates, dtype=np.int32)
    sv = np.ascontiguousarray(shifts, dtype=np.float32)
    if sg.shape != sv.shape or sg.ndim != 1:
      raise ValueError("shift_gates and shifts must be 1-D and of equal length")
    upstream = torch.as_tensor(upstream).to(device=self.device, dtype=torch.float32).contiguous()
    if tuple(upstream.shape) != (bits.shape[0], self.n_ops):
      raise ValueError("upstream must have shape [batch, n_ops]")
    w_ptr = None
    if row_weights is not None:
      row_weights = torch.as_tensor(row_weights).to(device=self.device, dtype=torch.float32).contiguous()
      if tuple(row_weights.shape) != (bits.shape[0],):
        raise ValueError("row_weights must have shape [batch]")
      w_ptr = row_weights.data_ptr()
    vals = torch.empty((len(sg), self.n_ops), dtype=torch.float32, device=self.device)
    grad = torch.empty((len(sg), self.n_params), dtype=torch.float32, device=self.device)
    with torch.cuda.device(self.device):
      self._check(
          self._lib.qhbm_program_vjps(self._h, bits.data_ptr(), bits.shape[0], params.data_ptr(), len(sg),
                                      sg.ctypes.data, sv.ctypes.data, upstream.data_ptr(), w_ptr, vals.data_ptr(),
                                      grad.data_ptr(), self._stream()))
    return vals, grad

  def expectation_jacobian(self, bits, params):
    self.retained = None
    bits, params = self._prep(bits, params)
    vals = torch.empty((bits.shape[0], self.n_ops), dtype=torch.float32,
                       device=self.device)
    jac = torch.zeros((bits.shape[0], self.n_ops, self.n_params),
                      dtype=torch.float32, device=self.device)
    with torch.cuda.device(self.device):
      self._check(
          self._lib.qhbm_expectation_jacobian(self._h, bits.data_ptr(),
                                              bits.shape[0], params.data_ptr(),
                                              vals.data_ptr(), jac.data_ptr(),
                                              self._stream()))
    return vals, jac
