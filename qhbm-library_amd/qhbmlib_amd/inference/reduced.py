"""Reduced density matrices of state ensembles: the partial trace on the GPU.

For sigma = sum_m w_m |phi_m><phi_m| given as M state vectors of n qubits and a subset A of k <= 10 of them,

    rho_A[a, a'] = sum_m w_m sum_b phi_m(a, b) conj(phi_m(a', b))

is summed by the engine's fused gather kernel (`_engine.reduced_density`) from the states where they lie: no permuted copy,
no 2^n amplitudes on the host.  Row index a reads the kept qubits big-endian in ascending order of the data's sorted qubit
list -- the layout `qnn_utils.unitary` would give on the kept qubits alone -- whatever order the caller names them in.

By default these are reported numbers and quantum data for `qmhl`, like `state_metrics`, and carry no graph.
`reduced_density_matrix(..., differentiable=True)` makes rho_A of a `(states, weights)` pair an autograd node:
for a real loss with cotangent Gamma = dL/dRe rho + i dL/dIm rho,

    dL/dphi_m = w_m ((Gamma + Gamma^H) (x) 1) phi_m,      dL/dw_m = 1/2 <phi_m|((Gamma + Gamma^H) (x) 1)|phi_m>,

one dense-operator kernel on the kept qubits of every state (`_engine.subsystem_apply`, which `apply_operator` exposes on
its own).  With states from `AnalyticQuantumInference.final_states*` the gradient reaches the circuit's variables (6l).
The entropy and distance helpers stay float-returning host functions.
"""
import numbers

import torch

from qhbmlib_amd import _engine
from qhbmlib_amd import utils
from qhbmlib_amd.data import quantum_data
from qhbmlib_amd.inference import qnn

MAX_KEPT_QUBITS = 10  # kRdmMaxKeep of the engine (csrc/rdm_index.h)
MAX_STATES_PER_CALL = 65536  # kRdmMaxStates

_ENGINES = qnn._EngineCache(max_engines=2)  # pylint: disable=protected-access


def _device():
  if not torch.cuda.is_available():
    raise _engine.EngineError("reduced density matrices need an MI355X: the kernel is HIP-only and has no CPU fallback")
  return torch.device("cuda", torch.cuda.current_device())


def _source(source):
  """(states on the device, float64 weights or None, sorted qubit list or None, n) of any accepted source."""
  if hasattr(source, "data") and callable(source.data) and not isinstance(source, quantum_data.StateVectorData):
    source = source.data()  # a ThermalEnsemble
  if isinstance(source, quantum_data.StateVectorData):
    return source._device_states(), source.weights, source.qubits, source.num_qubits  # pylint: disable=protected-access
  if isinstance(source, (tuple, list)) and len(source) == 2:
    states, weights = source
    states = torch.as_tensor(states)
    if not states.is_complex() or states.dim() != 2:
      raise ValueError(f"states must be a complex tensor of shape [M, 2^n], got {states.dtype} {tuple(states.shape)}")
    n = int(states.shape[1]).bit_length() - 1
    if states.shape[1] != (1 << n) or n < 1:
      raise ValueError(f"states have {states.shape[1]} amplitudes: not a power of two")
    if weights is not None:
      weights = torch.as_tensor(weights).to(torch.float64).reshape(-1)
      if weights.shape[0] != states.shape[0]:
        raise ValueError(f"{weights.shape[0]} weights for {states.shape[0]} states")
    return states.detach().to(device=_device(), dtype=torch.complex64), weights, None, n
  raise TypeError("a source is StateVectorData, a ThermalEnsemble or a (states, weights) pair")


def _positions(qubits, data_qubits, n):
  """Ascending positions in the data's sorted qubit list of `qubits`: qubit objects of that list, or integers."""
  qubits = list(qubits)
  if not qubits:
    raise ValueError("no qubits to keep")
  if all(isinstance(q, numbers.Integral) and not isinstance(q, bool) for q in qubits):  # (numpy integers included)
    positions = [int(q) for q in qubits]
    if any(p < 0 or p >= n for p in positions):
      raise ValueError(f"qubit positions {positions} are not all in [0, {n})")
  else:
    if data_qubits is None:
      raise ValueError("the data names no qubits: give integer positions")
    ordered = list(data_qubits)
    missing = [q for q in qubits if q not in ordered]
    if missing:
      raise ValueError(f"qubits {missing} are not in the data")
    positions = [ordered.index(q) for q in qubits]
  if len(set(positions)) != len(positions):
    raise ValueError("a qubit is named twice")
  if len(positions) > MAX_KEPT_QUBITS:
    raise ValueError(f"{len(positions)} kept qubits: rho_A has at most 2^{MAX_KEPT_QUBITS} rows")
  return sorted(positions)


def _mask(positions):
  return sum(1 << p for p in positions)


class _ReducedDensityFunction(torch.autograd.Function):
  """rho_A of (states [M, 2^n] complex64 on the device, weights [M] float64 or None) as an autograd node.  Forward is
  `_engine.reduced_density`; backward one `_engine.subsystem_apply` of H = Gamma + Gamma^H.  The states stay
  resident for backward.  Once differentiable only: the backward is a kernel call without a graph of its own."""

  @staticmethod
  def forward(ctx, states, weights, mask):
    ctx.mask = mask
    ctx.has_weights = weights is not None
    ctx.save_for_backward(*((states, weights) if ctx.has_weights else (states,)))
    return _engine.reduced_density(states, mask, weights)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gamma):
    states = ctx.saved_tensors[0]
    weights = ctx.saved_tensors[1] if ctx.has_weights else None
    need_states, need_weights = ctx.needs_input_grad[0], ctx.has_weights and ctx.needs_input_grad[1]
    if not (need_states or need_weights):
      return None, None, None
    gamma = gamma.to(torch.complex128)
    hermitian = (gamma + gamma.conj().transpose(0, 1)).to(torch.complex64)
    result = _engine.subsystem_apply(states, ctx.mask, hermitian, scale=weights, want_dots=need_weights)
    out, dots = result if need_weights else (result, None)
    grad_weights = (0.5 * dots.real).to(weights.dtype) if need_weights else None
    return (out if need_states else None), grad_weights, None


def _differentiable_pair(source):
  """(states complex64 [M, 2^n] on the device, weights float64 [M] on the device or None, n) of a `(states, weights)` pair,
  graphs kept."""
  if hasattr(source, "data") and callable(source.data) or isinstance(source, quantum_data.StateVectorData):
    raise ValueError("differentiable=True needs a (states, weights) pair: the states of StateVectorData and of a "
                     "ThermalEnsemble carry no graph")
  if not (isinstance(source, (tuple, list)) and len(source) == 2):
    raise TypeError("differentiable=True needs a (states, weights) pair")
  states, weights = source
  device = _device()
  states = torch.as_tensor(states)
  if not states.is_complex() or states.dim() != 2:
    raise ValueError(f"states must be a complex tensor of shape [M, 2^n], got {states.dtype} {tuple(states.shape)}")
  n = int(states.shape[1]).bit_length() - 1
  if states.shape[1] != (1 << n) or n < 1:
    raise ValueError(f"states have {states.shape[1]} amplitudes: not a power of two")
  states = states.to(device=device, dtype=torch.complex64).contiguous()
  if weights is not None:
    weights = torch.as_tensor(weights).to(device=device, dtype=torch.float64).reshape(-1)
    if weights.shape[0] != states.shape[0]:
      raise ValueError(f"{weights.shape[0]} weights for {states.shape[0]} states")
  return states, weights, n


def reduced_density_matrix(source, qubits, differentiable=False):
  """rho_A of `source` on `qubits`: complex128 [2^k, 2^k] on the device, Hermitian bit for bit.

  `source`: `StateVectorData`, a `ThermalEnsemble` (through `.data()`), or a `(states, weights)` pair ([M, 2^n] complex,
  [M] or None) with integer positions.  `qubits`: qubit objects of the data's sorted qubit list or integer positions in
  it, in any order -- the result always uses ascending order; duplicates and qubits not in the data are refused.  The
  weights enter as given: rho_A has the trace of sigma.

  `differentiable=False` (default): a reported number, no graph.  `differentiable=True`: `source` must be a
  `(states, weights)` pair; the result is an autograd node over the states (e.g. `final_states_from_states` of an
  inference, whose circuit variables the gradient then reaches) and over the weights, whichever require grad, with the same
  forward bits.  Exact thermal weights reach a circuit's variables as the pair
  `(q_inference.final_states(all_bitstrings), probabilities)`.  The states stay resident until backward; double backward is
  refused."""
  if differentiable:
    states, weights, n = _differentiable_pair(source)
    positions = _positions(qubits, None, n)
    return _ReducedDensityFunction.apply(states, weights, _mask(positions))
  states, weights, data_qubits, n = _source(source)
  positions = _positions(qubits, data_qubits, n)
  with torch.no_grad():
    return _engine.reduced_density(states, _mask(positions), weights)


def apply_operator(source_or_states, qubits, operator):
  """[M, 2^n] complex64: (operator (x) 1) |phi_m> for every state of `source_or_states` -- a source as in
  `reduced_density_matrix` (its weights are not used) or a bare complex tensor [M, 2^n] -- and a dense [2^k, 2^k] `operator`
  on `qubits` (k <= 10), given on the kept qubits in ascending order whatever order they are named in: a local quench, a
  projector, a Kraus operator.  f32 arithmetic on the device in a fixed order (`_engine.subsystem_apply`).  Not
  differentiable."""
  if torch.is_tensor(source_or_states):
    source_or_states = (source_or_states, None)
  states, _, data_qubits, n = _source(source_or_states)
  positions = _positions(qubits, data_qubits, n)
  with torch.no_grad():
    return _engine.subsystem_apply(states, _mask(positions), torch.as_tensor(operator))


def _entropy_of(rho):
  """von Neumann entropy of rho / tr rho: float64 `eigvalsh` on the host, eigenvalues clamped at 0, 0 log 0 = 0."""
  rho = rho.detach().to(device="cpu", dtype=torch.complex128)
  lam = torch.linalg.eigvalsh(0.5 * (rho + rho.conj().transpose(0, 1))).clamp_min(0.0)
  total = torch.sum(lam)
  if not float(total) > 0.0:
    raise ValueError("rho_A has no positive eigenvalue")
  lam = lam / total
  positive = lam[lam > 0]
  return float(-torch.sum(positive * torch.log(positive)))


def subsystem_entropy(source, qubits):
  """S(rho_A / tr rho_A) in nats, as a float (a host number: for a trainable entropy write it on
  `reduced_density_matrix(..., differentiable=True)`)."""
  return _entropy_of(reduced_density_matrix(source, qubits))


def mutual_information(source, a, b):
  """I(A : B) = S(A) + S(B) - S(A u B) in nats, as a float; overlapping `a` and `b` are refused.  Not differentiable."""
  states, weights, data_qubits, n = _source(source)
  pos_a, pos_b = _positions(a, data_qubits, n), _positions(b, data_qubits, n)
  if set(pos_a) & set(pos_b):
    raise ValueError("subsystems a and b overlap")
  if len(pos_a) + len(pos_b) > MAX_KEPT_QUBITS:
    raise ValueError(f"a and b together keep more than {MAX_KEPT_QUBITS} qubits")
  with torch.no_grad():
    parts = [_entropy_of(_engine.reduced_density(states, _mask(p), weights)) for p in (pos_a, pos_b, sorted(pos_a + pos_b))]
  return parts[0] + parts[1] - parts[2]


def trace_distance(rho, sigma):
  """1/2 sum |eigenvalues of rho - sigma|, float64 `eigvalsh` on the host, as a float."""
  delta = (torch.as_tensor(rho).detach().to(device="cpu", dtype=torch.complex128) -
           torch.as_tensor(sigma).detach().to(device="cpu", dtype=torch.complex128))
  if delta.dim() != 2 or delta.shape[0] != delta.shape[1]:
    raise ValueError(f"density matrices are square and of one size, got a difference of shape {tuple(delta.shape)}")
  return float(0.5 * torch.sum(torch.abs(torch.linalg.eigvalsh(0.5 * (delta + delta.conj().transpose(0, 1))))))


def _model_engine(model, device):
  """An engine with the model's circuit installed and no observables, cached here by content (two engines at most).  Not
  the quantum inference's own cache: an engine without observables put there could evict one a training loop is using."""
  circ = model.q_inference.circuit
  qubits = circ.qubits
  names = list(circ.symbol_names)
  flat_gates = circ.pqc.flat_gates(qubits, names)
  key = qnn._ContentKey((device.index, len(qubits), tuple(flat_gates), len(names)))  # pylint: disable=protected-access

  def make():
    eng = _engine.Engine(device.index)
    eng.set_circuit(len(qubits), flat_gates, len(names))
    return eng
  return _ENGINES.get(key, make)


def sampled_ensemble_reduced(model, bitstrings, counts, num_samples, qubits, max_state_bytes=2**31, differentiable=False):
  """rho_A of sum_u (counts_u / num_samples) U|x_u><x_u|U^dagger for given unique `bitstrings` [U, n] and `counts` [U]:
  states from an engine with the model's circuit (`statevector`, cached by content) in chunks of at most `max_state_bytes`
  and at most 65536 states, one kernel call per chunk, the chunk results added in chunk order in float64.

  `differentiable=True`: the states are `model.q_inference.final_states(bitstrings)`, so the gradient of any real function
  of the result reaches the circuit's variables; the counts carry none.  The states must stay resident for backward, so
  the ensemble is one chunk: one that does not fit `max_state_bytes` (or has more than 65536 states) is refused."""
  device = _device()
  circ = model.q_inference.circuit
  n = len(circ.qubits)
  positions = _positions(qubits, sorted(circ.qubits), n)
  mask = _mask(positions)
  bitstrings = torch.as_tensor(bitstrings)
  weights = torch.as_tensor(counts).to(torch.float64).reshape(-1) / float(num_samples)
  if bitstrings.dim() != 2 or bitstrings.shape[1] != n or bitstrings.shape[0] != weights.shape[0] or bitstrings.shape[0] < 1:
    raise ValueError(f"bitstrings {tuple(bitstrings.shape)} and counts {tuple(weights.shape)} do not describe states of {n} qubits")
  chunk = min(MAX_STATES_PER_CALL, max(1, int(max_state_bytes) // (8 << n)))
  if differentiable:
    if bitstrings.shape[0] > chunk:
      raise ValueError(f"differentiable=True keeps all {bitstrings.shape[0]} states of {n} qubits resident for backward: "
                       f"more than the {chunk} that fit max_state_bytes={int(max_state_bytes)} and one kernel call")
    states = model.q_inference.final_states(bitstrings)
    return _ReducedDensityFunction.apply(states, weights.detach().to(states.device), mask)
  with torch.no_grad():
    eng = _model_engine(model, device)
    bits = qnn._engine_bits(circ, bitstrings)  # pylint: disable=protected-access
    values = circ.symbol_values.detach().to(torch.float32)
    total = None
    for u0 in range(0, bits.shape[0], chunk):
      states = eng.statevector(bits[u0:u0 + chunk], values)
      part = _engine.reduced_density(states, mask, weights[u0:u0 + chunk])
      total = part if total is None else total + part
  return total


def sampled_reduced_density_matrix(qhbm, qubits, num_samples, max_state_bytes=2**31, differentiable=False):
  """rho_A of the QHBM's sampled ensemble sum_u (counts_u / num_samples) U|x_u><x_u|U^dagger: bitstrings and counts as
  `QHBM.circuits(num_samples)` takes them (one sample set, deduplicated), then `sampled_ensemble_reduced`.  `qubits`: qubit
  objects of the model circuit or integer positions in its sorted qubit list.  `differentiable=True`: differentiable with
  respect to the circuit's variables (the sampled counts carry no gradient), one chunk only -- see
  `sampled_ensemble_reduced`."""
  qhbm.agree_seeds()
  samples = qhbm.e_inference.sample(num_samples)
  bitstrings, _, counts = utils.unique_bitstrings_with_counts(samples)
  return sampled_ensemble_reduced(qhbm, bitstrings, counts, num_samples, qubits, max_state_bytes, differentiable)
