"""Quantum data (reference: qhbmlib/data/quantum_data.py:25-41, qhbm_data.py:26-38)."""
import abc

import torch


class QuantumData(abc.ABC):
  """Interface for quantum datasets."""

  @abc.abstractmethod
  def expectation(self, observable):
    """Average of `observable` against this data source."""
    raise NotImplementedError()


class QHBMData(QuantumData):
  """QuantumData defined by a QHBM (qhbm_data.py:26-38)."""

  def __init__(self, input_qhbm):
    self.qhbm = input_qhbm

  def expectation(self, observable):
    return self.qhbm.expectation(observable).squeeze(0)


class StateVectorData(QuantumData):
  """QuantumData given as state vectors: the mixture sum_m w_m |phi_m><phi_m|.

  `states`: [M, 2^n] complex tensor, amplitude index = the bitstring read big-endian over the sorted qubits (the row
  order of `qnn_utils.unitary`, what the engine's `statevector` returns).  `weights`: [M] (default 1 / M each, so that
  un-normalised rows sqrt(p_m) phi_m with unit weights describe a mixture too).  `qubits`: the qubits the states live
  on (default: those of the Hamiltonian they are first measured with).

  `expectation(hamiltonian)` = sum_m w_m <phi_m| K |phi_m> runs in the HIP engine from the states themselves
  (`AnalyticQuantumInference.expectation_from_states` over an empty circuit) and is differentiable with respect to
  the Hamiltonian's variables, so `qmhl(StateVectorData(...), qhbm)` trains a QHBM on data that is no QHBM: the
  eigen-ensemble of a density matrix, ground states, another simulator's output.

  `energy_tables` ("off", "general" or "all"; also an attribute that may be set later) is handed to that inference:
  "off" (default) takes Hamiltonians with a Pauli-form energy only and raises TypeError for any other, "general" measures
  an energy that is no `PauliMixin` -- an MLP on the bits -- through its table on the final states, so that `qmhl` fits
  such a model to state-vector data too (`AnalyticQuantumInference.expectation_from_states`)."""

  def __init__(self, states, weights=None, qubits=None, energy_tables="off"):
    states = torch.as_tensor(states)
    if not states.is_complex() or states.dim() != 2 or states.shape[0] < 1:
      raise ValueError(f"states must be a complex tensor of shape [M, 2^n], got {states.dtype} {tuple(states.shape)}")
    n = int(states.shape[1]).bit_length() - 1
    if states.shape[1] != (1 << n) or n < 1:
      raise ValueError(f"states have {states.shape[1]} amplitudes: not a power of two")
    if weights is None:
      weights = torch.full((states.shape[0],), 1.0 / states.shape[0], dtype=torch.float64)
    weights = torch.as_tensor(weights).to(torch.float64).reshape(-1)
    if weights.shape[0] != states.shape[0]:
      raise ValueError(f"{weights.shape[0]} weights for {states.shape[0]} states")
    if qubits is not None and len(qubits) != n:
      raise ValueError(f"{len(qubits)} qubits for states of {n} qubits")
    self.states = states.detach()  # (in the precision given; the engine takes a complex64 copy: _device_states)
    self.weights = weights.detach()
    self.qubits = None if qubits is None else sorted(qubits)
    self.num_qubits = n
    self.energy_tables = energy_tables
    self._inference = None
    self._on_device = None

  @classmethod
  def from_density_matrix(cls, sigma, rtol=1e-10, qubits=None, energy_tables="off"):
    """The eigen-ensemble of a density matrix: `torch.linalg.eigh` in float64 / complex128, eigenvalues below
    `rtol` * (the largest) dropped, the kept eigenvalues as weights of their eigenvectors."""
    sigma = torch.as_tensor(sigma)
    sigma = sigma.to(torch.complex128 if sigma.is_complex() else torch.float64)
    if sigma.dim() != 2 or sigma.shape[0] != sigma.shape[1]:
      raise ValueError(f"a density matrix is square, got {tuple(sigma.shape)}")
    evals, evecs = torch.linalg.eigh(0.5 * (sigma + sigma.conj().transpose(0, 1)))
    keep = evals > rtol * evals.max()
    states = evecs[:, keep].transpose(0, 1).to(torch.complex128)
    return cls(states, evals[keep], qubits, energy_tables)

  @classmethod
  def thermal(cls, operators, beta, **kwargs):
    """The thermal state of H = sum_k operators[k] at inverse temperature `beta` as quantum data, without a dense
    matrix: thermal pure quantum states from the engine's imaginary-time evolution
    (`inference.thermal_ensemble(operators, beta, **kwargs).data()`; `start="basis"` is exact up to 14 qubits)."""
    from qhbmlib_amd.inference import thermal  # pylint: disable=import-outside-toplevel
    return thermal.thermal_ensemble(operators, beta, **kwargs).data()

  @classmethod
  def ground_state(cls, operators, **kwargs):
    """The ground state of H = sum_k operators[k] as quantum data (one state, weight 1), without a dense matrix: the
    lowest Ritz vector of a restarted Krylov space (`inference.ground_state(operators, **kwargs)`; `store_basis=False`
    keeps three vectors in memory, not the whole basis)."""
    from qhbmlib_amd.inference import krylov, thermal  # pylint: disable=import-outside-toplevel
    ops = thermal._operator_list(operators)  # pylint: disable=protected-access
    qubits = thermal._qubits_of(ops, kwargs.get("qubits"))  # pylint: disable=protected-access
    _, state, _, _ = krylov.ground_state(operators, **kwargs)
    return cls(state.reshape(1, -1), torch.ones(1, dtype=torch.float64), qubits)

  def _inference_for(self, qubits):
    # (imported here: qhbmlib_amd.inference imports the losses, which take QuantumData)
    from qhbmlib_amd.inference import qnn  # pylint: disable=import-outside-toplevel
    from qhbmlib_amd import ir  # pylint: disable=import-outside-toplevel
    from qhbmlib_amd.models import circuit  # pylint: disable=import-outside-toplevel
    qubits = sorted(qubits)
    if self.qubits is None:
      if len(qubits) != self.num_qubits:
        raise ValueError(f"the Hamiltonian acts on {len(qubits)} qubits, the states live on {self.num_qubits}")
      self.qubits = qubits
    elif qubits != self.qubits:
      raise ValueError("the Hamiltonian's qubits are not the data's")
    if self._inference is None:  # created once: its engine cache then serves every later call
      # (an empty circuit on the data's qubits: no bitstring is ever injected, so the bit-order flag chooses nothing)
      empty = circuit.QuantumCircuit(ir.Circuit(), self.qubits, [], [], [], "state_vector_data", tfq_compat_bit_order=False)
      self._inference = qnn.AnalyticQuantumInference(empty)
    if self.energy_tables not in self._inference.ENERGY_TABLES:
      raise ValueError(f"energy_tables must be one of {self._inference.ENERGY_TABLES}, got {self.energy_tables!r}")
    self._inference.energy_tables = self.energy_tables
    return self._inference

  def _device_states(self):
    """The complex64 copy the engine reads, made once: a step of `qmhl` moves no state to the device again."""
    if self._on_device is None:
      device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else self.states.device
      self._on_device = self.states.to(device=device, dtype=torch.complex64).contiguous()
    return self._on_device

  def expectation(self, observable):
    """sum_m w_m <phi_m| observable |phi_m> as a scalar; `observable` is a Hamiltonian with a Pauli-form energy, or
    with any energy that has a table when `energy_tables` is "general"."""
    q_inference = self._inference_for(observable.circuit.qubits)
    values = q_inference.expectation_from_states(self._device_states(), observable)  # [M, 1]
    weights = self.weights.to(device=values.device, dtype=values.dtype)
    return torch.sum(weights * values.squeeze(-1))

  def sampled_expectation(self, observable, num_shots, seed=None):
    """The shot-noise estimate of sum_m w_m <phi_m| observable |phi_m> from `num_shots` computational-basis shots per
    state and measurement basis, drawn and reduced on the device (`qhbm_sample_parities_states`).
    `observable`: a PauliSum / PauliString (a scalar comes back) or a list of them ([n_ops]).  The strings are grouped by
    their X/Y pattern as `SampledQuantumInference` groups them; a group's states are rotated once (X: H, Y: rx(pi / 2))
    by `statevector_from_states`, Z-only groups are sampled as given.  Rows need not be normalised: a row's estimate is
    scaled by its squared norm.  `seed` None draws a fresh one.  Not differentiable."""
    import math  # pylint: disable=import-outside-toplevel
    from qhbmlib_amd import _engine, ir  # pylint: disable=import-outside-toplevel
    from qhbmlib_amd.inference import ebm  # pylint: disable=import-outside-toplevel
    single = not isinstance(observable, (list, tuple))
    ops = [ir.as_pauli_sum(op) for op in ([observable] if single else observable)]
    num_shots = int(num_shots)
    if num_shots < 1:
      raise ValueError("num_shots must be positive")
    qubits = self.qubits
    if qubits is None:
      qubits = sorted(set().union(*[op.qubits() for op in ops]))
      if len(qubits) != self.num_qubits:
        raise ValueError(f"the observable acts on {len(qubits)} qubits, the states live on {self.num_qubits}: "
                         "give the data its `qubits`")
    qindex = {q: i for i, q in enumerate(qubits)}
    strings, mix = [], []
    for t, op in enumerate(ops):
      for term in op.terms:
        if any(q not in qindex for q in term.paulis):
          raise ValueError("the observable's qubits are not the data's")
        strings.append(term)
        mix.append((t, term.coefficient))
    groups = {}
    for k, st in enumerate(strings):
      key = tuple(sorted((qindex[q], p) for q, p in st.paulis.items() if p in ("X", "Y")))
      groups.setdefault(key, []).append(k)
    states = self._device_states()
    if not states.is_cuda:
      raise _engine.EngineError("sampled_expectation needs an MI355X: the engine is HIP-only, no CPU fallback")
    seed = int(ebm.fresh_seed() if seed is None else seed) & (2**63 - 1)
    estimates = torch.ones((states.shape[0], len(strings)), dtype=torch.float64, device=states.device)
    program = 0
    for key, members in groups.items():
      rotated = states
      if key:
        rot = ir.Circuit([ir.H(qubits[i]) if p == "X" else ir.rx(math.pi / 2)(qubits[i]) for i, p in key])
        eng = _engine.Engine(states.device.index)
        eng.set_circuit(self.num_qubits, rot.flat_gates(qubits, []), 0)
        rotated = eng.statevector_from_states(states, torch.zeros(0))
        del eng
      masks = [sum(1 << qindex[q] for q in strings[k].paulis) for k in members]
      for lo in range(0, len(masks), 1024):   # (the entry takes 1024 masks; every call its own random stream)
        sums = _engine.sample_parities_states(rotated, masks[lo:lo + 1024], num_shots, seed, program=program)
        estimates[:, members[lo:lo + 1024]] = sums.to(torch.float64) / float(num_shots)
        program += 1
    values = torch.zeros((states.shape[0], len(ops)), dtype=torch.float64, device=states.device)
    for k, (t, c) in enumerate(mix):
      values[:, t] += c * estimates[:, k]
    norm2 = (states.real.to(torch.float64)**2 + states.imag.to(torch.float64)**2).sum(1)
    out = torch.sum((self.weights.to(states.device) * norm2).unsqueeze(1) * values, dim=0)
    return out[0] if single else out

  def metrics(self, model, **kwargs):
    """`inference.state_metrics(model, self, **kwargs)`: trace, purity, entropy, overlap, fidelity, cross entropy and
    relative entropy of this data against the QHBM `model`, matrix-free: python floats, or with
    `differentiable=True` 0-dim tensors that train the model's variables."""
    from qhbmlib_amd.inference.state_metrics import state_metrics  # pylint: disable=import-outside-toplevel
    return state_metrics(model, self, **kwargs)

  def fidelity(self, model, **kwargs):
    """(tr sqrt(sqrt(sigma) rho sqrt(sigma)))^2 against the QHBM `model`, as a float; `differentiable=True`: as a loss."""
    return self.metrics(model, **kwargs).fidelity

  def relative_entropy(self, model, **kwargs):
    """D(sigma || rho) = tr sigma (log sigma - log rho) against the QHBM `model`, as a float; `differentiable=True`: as a
    loss."""
    return self.metrics(model, **kwargs).relative_entropy

  def fidelity_to(self, other, differentiable=False):
    """(tr sqrt(sqrt(sigma) tau sqrt(sigma)))^2 of this data sigma against another state ensemble tau (`StateVectorData`, a
    `ThermalEnsemble` or a `(states, weights)` pair), both as given: `inference.ensemble_metrics(self, other).fidelity`
    (DESIGN.md 6p).  `differentiable=True`: a 0-dim float64 tensor whose gradient reaches the states and weights of a
    `(states, weights)` pair that require grad; this data is a constant."""
    from qhbmlib_amd.inference.ensemble_metrics import ensemble_metrics  # pylint: disable=import-outside-toplevel
    return ensemble_metrics(self, other, differentiable=differentiable).fidelity

  def trace_distance_to(self, other, differentiable=False):
    """1/2 ||sigma - tau||_1 of this data against another state ensemble, both as given:
    `inference.ensemble_metrics(self, other).trace_distance`.  `differentiable=True`: as `fidelity_to`."""
    from qhbmlib_amd.inference.ensemble_metrics import ensemble_metrics  # pylint: disable=import-outside-toplevel
    return ensemble_metrics(self, other, differentiable=differentiable).trace_distance

  def reduced(self, qubits, rtol=1e-10):
    """The quantum data of subsystem A = `qubits` (qubit objects of this data or integer positions in its sorted qubit
    list): the eigen-ensemble of rho_A = tr_B sigma, summed on the GPU without moving the states
    (`inference.reduced_density_matrix`), as `from_density_matrix(rho_A, rtol, qubits=kept)`.  Not
    differentiable."""
    from qhbmlib_amd.inference import reduced  # pylint: disable=import-outside-toplevel
    positions = reduced._positions(qubits, self.qubits, self.num_qubits)  # pylint: disable=protected-access
    kept = None if self.qubits is None else [self.qubits[p] for p in positions]
    rho = reduced.reduced_density_matrix(self, positions)
    return StateVectorData.from_density_matrix(rho.cpu(), rtol, qubits=kept)

  def entropy(self):
    """S(sigma) = -tr sigma log sigma of the data as given, as a float (no model needed)."""
    from qhbmlib_amd.inference.state_metrics import data_entropy  # pylint: disable=import-outside-toplevel
    return data_entropy(self)
