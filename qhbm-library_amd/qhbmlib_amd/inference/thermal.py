"""Matrix-free thermal targets: e^{-tau H} and e^{-i tau H} on device-resident state vectors, thermal pure quantum states.

The reference builds the target of both losses -- the thermal state of a Pauli-sum Hamiltonian, its log Z and entropy --
with a dense `eigh` (baselines/utils.py `get_thermal_state`, `log_partition_function`), which ends near 12 qubits.  Here
H = sum_k w_k O_k is only ever APPLIED, by the engine's lambda = O psi kernels, inside a Chebyshev expansion of the
exponential (`qhbm_evolve_states`).  For random-sign vectors r_m with E[|r><r|] = I / 2^n,

  phi_m = e^{-beta H / 2} r_m / ||.||,   l_m = 2 log ||e^{-beta H / 2} r_m||,
  Z ~ 2^n mean_m e^{l_m},   rho_beta ~ sum_m softmax(l)_m |phi_m><phi_m|,

(Sugiura and Shimizu, Phys. Rev. Lett. 111, 010401 (2013)); started from all 2^n basis states instead the same sums are
exact.  The ensemble is quantum data for `qmhl` (`data.StateVectorData`) and carries the log Z a VQT loss is held against.
"""
import math

import numpy as np
import torch

from qhbmlib_amd import _engine
from qhbmlib_amd import ir

MAX_BASIS_QUBITS = 14  # a basis start holds all 2^n states of 2^n amplitudes
DEFAULT_VECTORS = 16


def _operator_list(operators):
  if isinstance(operators, (ir.PauliSum, ir.PauliString)):
    operators = [operators]
  operators = [ir.as_pauli_sum(op) for op in operators]
  if not operators:
    raise ValueError("no operators given")
  return operators


def _qubits_of(operators, qubits):
  if qubits is None:
    qubits = set()
    for op in operators:
      qubits |= op.qubits()
  qubits = sorted(qubits)
  if not qubits:
    raise ValueError("the operators act on no qubit: pass `qubits`")
  return qubits


def _engine_for(operators, qubits, device=None):
  """An engine over an empty circuit on `qubits` with `operators` installed."""
  if not torch.cuda.is_available():
    raise _engine.EngineError("the thermal routines need an MI355X: the engine is HIP-only and has no CPU fallback")
  eng = _engine.Engine(torch.cuda.current_device() if device is None else device)
  eng.set_circuit(len(qubits), [], 0)
  eng.set_observables([list(op.masks(qubits)) for op in operators])
  return eng


def _check_states(states, n):
  states = torch.as_tensor(states)
  if not states.is_complex() or states.dim() != 2 or states.shape[1] != (1 << n):
    raise ValueError(f"states must be a complex tensor of shape [M, {1 << n}] ({n} qubits), got {states.dtype} {tuple(states.shape)}")
  return states


def imaginary_time_evolution(operators, states, tau, weights=None, qubits=None):
  """(e^{-tau H} phi_m normalised, float64 [M] log ||e^{-tau H} phi_m|| of the states as given) for H = sum_k weights[k]
  operators[k] (default weights: ones); `states` is [M, 2^n] complex, amplitude index = the bitstring read big-endian
  over the sorted qubits.  Not differentiable."""
  operators = _operator_list(operators)
  qubits = _qubits_of(operators, qubits)
  eng = _engine_for(operators, qubits)
  return eng.evolve_states(_check_states(states, len(qubits)), float(tau), 0, weights)


def real_time_evolution(operators, states, tau, weights=None, qubits=None):
  """e^{-i tau H} phi_m, the norms as given; any sign of `tau`."""
  operators = _operator_list(operators)
  qubits = _qubits_of(operators, qubits)
  eng = _engine_for(operators, qubits)
  return eng.evolve_states(_check_states(states, len(qubits)), float(tau), 1, weights)[0]


class ThermalEnsemble:
  """Thermal pure quantum states of H = sum_k weights[k] operators[k] at inverse temperature `beta`.

  `states` [M, 2^n] complex64, normalised, on the device; `log_weights` float64 [M] = 2 log ||e^{-beta H / 2} r_m||."""

  def __init__(self, operators, weights, qubits, beta, states, log_weights, start):
    self.operators = operators
    self.operator_weights = weights
    self.qubits = qubits
    self.beta = float(beta)
    self.states = states
    self.log_weights = log_weights
    self.start = start
    self._inference = None

  @property
  def num_qubits(self):
    return len(self.qubits)

  def log_partition(self):
    """log Z: n log 2 + logsumexp(l) - log M from random vectors, logsumexp(l) (exact) from the basis."""
    total = torch.logsumexp(self.log_weights, 0)
    if self.start == "basis":
      return total
    return total + self.num_qubits * math.log(2.0) - math.log(self.log_weights.shape[0])

  @property
  def weights(self):
    """softmax(l): the weights of the states in rho_beta ~ sum_m w_m |phi_m><phi_m|."""
    return torch.softmax(self.log_weights, 0)

  def _states_inference(self):
    if self._inference is None:
      from qhbmlib_amd.inference import qnn  # pylint: disable=import-outside-toplevel
      from qhbmlib_amd.models import circuit  # pylint: disable=import-outside-toplevel
      empty = circuit.QuantumCircuit(ir.Circuit(), self.qubits, [], [], [], "thermal_ensemble", tfq_compat_bit_order=False)
      self._inference = qnn.AnalyticQuantumInference(empty)
    return self._inference

  def expectation(self, observables):
    """[len(observables)] of Tr(rho_beta O_j) ~ sum_m w_m <phi_m| O_j |phi_m> (float64), through
    `AnalyticQuantumInference.expectation_from_states`."""
    values = self._states_inference().expectation_from_states(self.states, _operator_list(observables))  # [M, n_ops]
    return self.weights.to(values.device) @ values.double()

  def energy(self):
    """<H> = sum_k weights[k] Tr(rho_beta operators[k])."""
    values = self.expectation(self.operators)
    if self.operator_weights is None:
      return values.sum()
    return (torch.as_tensor(self.operator_weights, dtype=torch.float64, device=values.device) * values).sum()

  def entropy(self):
    """S = beta <H> + log Z."""
    return self.beta * self.energy() + self.log_partition()

  def data(self):
    """The ensemble as quantum data: `qmhl(ensemble.data(), qhbm)`."""
    from qhbmlib_amd.data import quantum_data  # pylint: disable=import-outside-toplevel
    return quantum_data.StateVectorData(self.states, self.weights, self.qubits)


def thermal_ensemble(operators, beta, num_vectors=None, seed=None, qubits=None, start="random", weights=None):
  """The `ThermalEnsemble` of H = sum_k weights[k] operators[k] at `beta`.

  start="random": `num_vectors` (default 16) random-sign vectors from the engine's counter-based generator under `seed`
  (default 0): an estimate whose error falls as 1 / sqrt(M 2^n) at high temperature (typicality).
  start="basis": all 2^n basis states -- exact, M = 2^n, at most 14 qubits."""
  operators = _operator_list(operators)
  qubits = _qubits_of(operators, qubits)
  n = len(qubits)
  if not np.isfinite(beta) or beta < 0:
    raise ValueError(f"beta must be finite and >= 0, got {beta}")
  eng = _engine_for(operators, qubits)
  if start == "basis":
    if n > MAX_BASIS_QUBITS:
      raise ValueError(f"start='basis' holds 2^n states of 2^n amplitudes: refused above {MAX_BASIS_QUBITS} qubits (got {n})")
    if num_vectors is not None and num_vectors != (1 << n):
      raise ValueError(f"start='basis' has 2^n = {1 << n} vectors")
    starts = torch.eye(1 << n, dtype=torch.complex64, device=eng.device)
  elif start == "random":
    count = DEFAULT_VECTORS if num_vectors is None else int(num_vectors)
    if count < 1:
      raise ValueError("num_vectors must be positive")
    starts = _engine.random_states(count, n, 0 if seed is None else seed, device=eng.device)
  else:
    raise ValueError(f"start must be 'random' or 'basis', got {start!r}")
  states, log_norms = eng.evolve_states(starts, 0.5 * float(beta), 0, weights, in_place=True)
  eng.close()
  return ThermalEnsemble(operators, None if weights is None else [float(w) for w in weights], qubits, beta, states,
                         2.0 * log_norms, start)
