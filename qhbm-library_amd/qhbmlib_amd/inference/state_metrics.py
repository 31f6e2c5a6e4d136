"""Fidelity, entropy and relative entropy of state-vector data against a QHBM, without a 2^n x 2^n matrix.

The reference reports its metrics from dense matrices (baselines/train.py:482-500 through qhbm_utils.py:62-116); the
mirror of that route is `qhbm_utils.fidelity` and stops near 12 qubits.  For rho = U diag(p) U^dagger, p = softmax(-E),
and data sigma = sum_m w_m |phi_m><phi_m| given as M state vectors, every metric is a function of three M x M matrices

    G_t[m, m'] = sum_x t(x) conj(a_m(x)) a_m'(x),   a_m = U^dagger phi_m,   t in {1, p, E}

which the engine sums in float64 in one streaming kernel (`_engine.weighted_gram`).  With B = Phi W^1/2 the operators
sqrt(sigma) rho sqrt(sigma) and B^dagger rho B = W^1/2 G_p W^1/2 share their non-zero spectrum (both are X^dagger X and
X X^dagger of X = sqrt(rho) B up to the polar factor of B), and so do sigma = B B^dagger and B^dagger B = W^1/2 G_1 W^1/2.

With `differentiable=True` the same numbers are autograd nodes over the model's variables: a_m is the
differentiable final state of the inverse circuit (6l), E the energy's table with its graph, and G_p, G_E go through
`weighted_gram`, whose backward is one fused kernel (`_engine.weighted_gram_vjp`) from the cotangent of G to those of the
states and of the table.
"""
import dataclasses
import weakref

import torch

from qhbmlib_amd import _engine
from qhbmlib_amd.data import quantum_data
from qhbmlib_amd.inference import qnn
from qhbmlib_amd.models import energy_utils
from qhbmlib_amd.models import hamiltonian


@dataclasses.dataclass(frozen=True)
class StateMetrics:
  """What `state_metrics` returns; python floats (0-dim float64 tensors with `differentiable=True`), nothing normalised
  (sigma as given: `trace` says what it sums to)."""
  trace: float             # tr sigma
  purity: float            # tr sigma^2
  entropy: float           # S(sigma) = -tr sigma log sigma, in nats
  overlap: float           # tr(rho sigma)
  fidelity: float          # (tr sqrt(sqrt(sigma) rho sqrt(sigma)))^2
  log_partition: float     # log Z = log sum_x exp(-E(x))
  cross_entropy: float     # -tr(sigma log rho) = sum_m w_m <a_m| E |a_m> + log Z tr sigma
  relative_entropy: float  # D(sigma || rho) = -S(sigma) + cross entropy: what QMHL minimises, up to S(sigma)


_ENGINES = qnn._EngineCache(max_engines=2)  # pylint: disable=protected-access


def _device():
  if not torch.cuda.is_available():
    raise _engine.EngineError("state metrics need an MI355X: the Gram kernel is HIP-only and has no CPU fallback")
  return torch.device("cuda", torch.cuda.current_device())


def _inverse_circuit_engine(model, device):
  """(engine with the model circuit's inverse installed and no observables, its parameter values); cached by content."""
  dagger = model.circuit_dagger
  qubits = dagger.qubits
  names = list(dagger.symbol_names)
  flat_gates = dagger.pqc.flat_gates(qubits, names)
  key = qnn._ContentKey((device.index, len(qubits), tuple(flat_gates), len(names)))  # pylint: disable=protected-access

  def make():
    eng = _engine.Engine(device.index)
    eng.set_circuit(len(qubits), flat_gates, len(names))
    return eng
  return _ENGINES.get(key, make), dagger.symbol_values.detach().to(torch.float32)


def _weighted_spectrum(gram, weights):
  """Eigenvalues of W^1/2 G W^1/2 (float64, on the host, clamped at 0)."""
  root = torch.sqrt(weights).to(torch.complex128)
  b = root.unsqueeze(1) * gram.cpu() * root.unsqueeze(0)
  return torch.linalg.eigvalsh(0.5 * (b + b.conj().transpose(0, 1))).clamp_min(0.0)


def _partition(energies):
  """(log Z, p = exp(-E - log Z) as float32) of a float32 energy table, through float64."""
  e64 = energies.to(torch.float64)
  log_z = torch.logsumexp(-e64, 0)
  return log_z, torch.exp(-e64 - log_z).to(torch.float32)


def _weights_of(data):
  weights = data.weights.to(device="cpu", dtype=torch.float64)
  if bool((weights < 0).any()):
    raise ValueError("the weights of a mixture are not negative")
  return weights


def _sigma_metrics(gram_one, weights):
  """(trace, purity, entropy) of sigma from G_1."""
  lam = _weighted_spectrum(gram_one, weights)
  trace = float(torch.sum(weights * gram_one.cpu().diagonal().real))
  positive = lam[lam > 0]
  return trace, float(torch.sum(lam * lam)), float(-torch.sum(positive * torch.log(positive)))  # (0 log 0 = 0)


def data_entropy(data):
  """S(sigma) of state-vector data, from the spectrum of W^1/2 G_1 W^1/2 (no model needed).  Not differentiable."""
  _device()
  return _sigma_metrics(_engine.weighted_gram(data._device_states()), _weights_of(data))[2]  # pylint: disable=protected-access


class _WeightedGramFunction(torch.autograd.Function):
  """G_t of (states [M, 2^n] complex on the device, table [2^n] real or None) as an autograd node.  Forward is
  `_engine.weighted_gram`; backward one `_engine.weighted_gram_vjp` of H = Gamma + Gamma^H.  The states and
  the table stay resident for backward.  Once differentiable only: the backward is a kernel call without a graph of its
  own."""

  @staticmethod
  def forward(ctx, states, table):
    ctx.has_table = table is not None
    ctx.save_for_backward(*((states, table) if ctx.has_table else (states,)))
    return _engine.weighted_gram(states, table)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gamma):
    states = ctx.saved_tensors[0]
    table = ctx.saved_tensors[1] if ctx.has_table else None
    need_states, need_table = ctx.needs_input_grad[0], ctx.has_table and ctx.needs_input_grad[1]
    if not (need_states or need_table):
      return None, None
    gamma = gamma.to(torch.complex128)
    hermitian = (gamma + gamma.conj().transpose(0, 1)).to(torch.complex64)
    out, grad = _engine.weighted_gram_vjp(states, table, hermitian, want_states=need_states, want_table=need_table)
    return (out.to(states.dtype) if need_states else None), (grad.to(table.dtype) if need_table else None)


def weighted_gram(states, table=None):
  """G[i, j] = sum_x table[x] conj(states[i, x]) states[j, x] (table None: ones) of M device-resident states [M, 2^n]:
  complex128 [M, M] with the bits of `_engine.weighted_gram`, as an autograd node over `states` and `table`, whichever
  require grad.  The table is a real tensor on the states' device (float32 in the kernel: a float64 table
  is cast, its gradient comes back in its own dtype); the states are used as complex64.  For a real loss with cotangent
  Gamma of G, backward forms H = Gamma + Gamma^H in complex128, casts it to complex64 and makes one engine call:
  the states receive table * sum_i H[i, j] states[i], the table 1/2 sum_j Re(conj(c_j) states[j]) with the unscaled c.
  Double backward is refused."""
  if not (torch.is_tensor(states) and states.is_cuda and states.dim() == 2 and states.is_complex()):
    raise _engine.EngineError("weighted_gram needs complex CUDA states [M, 2^n]: the engine has no CPU fallback")
  if table is not None:
    if not (torch.is_tensor(table) and table.is_cuda and table.device == states.device):
      raise _engine.EngineError("weighted_gram needs the table on the states' device")
    if table.is_complex() or not table.is_floating_point():
      raise ValueError(f"table must be a real floating-point tensor, got {table.dtype}")
    if tuple(table.shape) != (states.shape[1],):
      raise ValueError(f"table must have shape [{states.shape[1]}], got {tuple(table.shape)}")
  return _WeightedGramFunction.apply(states, table)


_INFERENCES = weakref.WeakKeyDictionary()  # model -> AnalyticQuantumInference(model.circuit_dagger)


def _inverse_circuit_inference(model):
  """The private inference of the model's inverse circuit (it shares the variables of `model.circuit`), one per model
  object: a training loop builds its engine once."""
  found = _INFERENCES.get(model)
  if found is None or found.circuit is not model.circuit_dagger:
    found = qnn.AnalyticQuantumInference(model.circuit_dagger)
    _INFERENCES[model] = found
  return found


def _differentiable_metrics(model, data, table, max_qubits, n, weights, device):
  """`state_metrics` as autograd nodes over the model's variables: 0-dim float64 tensors on the host."""
  states = data._device_states()  # pylint: disable=protected-access
  if states.requires_grad or data.states.requires_grad:
    raise ValueError("state_metrics is not differentiable with respect to the data: its states require grad")
  weights = weights.detach()
  amplitudes = _inverse_circuit_inference(model).final_states_from_states(states)
  energies = energy_utils.energy_table(model.energy, n, max_qubits, method=table).to(device)
  e64 = energies.to(torch.float64)
  log_z = torch.logsumexp(-e64, 0)
  probs = torch.exp(-e64 - log_z)
  with torch.no_grad():
    gram_one = _engine.weighted_gram(states)
    trace, purity, entropy = (torch.tensor(v, dtype=torch.float64) for v in _sigma_metrics(gram_one, weights))
  gram_p = weighted_gram(amplitudes, probs).cpu()
  gram_e = weighted_gram(amplitudes, energies).cpu()
  overlap = torch.sum(weights * gram_p.diagonal().real)
  root = torch.sqrt(weights).to(torch.complex128)
  b = root.unsqueeze(1) * gram_p * root.unsqueeze(0)
  lam = torch.linalg.eigvalsh(0.5 * (b + b.conj().transpose(0, 1)))
  # (an eigenvalue at or below 0 -- a rounded zero of a rank-deficient sigma -- contributes nothing and carries no gradient:
  # the derivative of sqrt is unbounded there)
  fidelity = torch.sum(torch.sqrt(lam[lam > 0]))**2
  log_partition = log_z.cpu()
  cross = torch.sum(weights * gram_e.diagonal().real) + log_partition * trace
  return StateMetrics(trace, purity, entropy, overlap, fidelity, log_partition, cross, cross - entropy)


def state_metrics(model: hamiltonian.Hamiltonian, data: quantum_data.StateVectorData, table: str = "terms",
                  max_qubits: int = 24, differentiable: bool = False) -> StateMetrics:
  """Metrics of the QHBM `model` (rho = U diag(softmax(-E)) U^dagger) against `data` (sigma = sum_m w_m |phi_m><phi_m|,
  the states neither orthogonal nor normalised by assumption), matrix-free: one run of the inverse circuit on the M
  states, one energy table (`energy_utils.energy_table(model.energy, n, max_qubits, method=table)`: any energy, MLP
  energies included) and three weighted Gram matrices in the HIP engine, then M x M eigenproblems in float64 on the host.

  Table index and amplitude index are the bitstring read big-endian over the sorted qubits, as in `density_matrix` and
  `fidelity`; no `tfq_compat_bit_order` permutation applies, because `qnn_utils.unitary` applies none either.
  `differentiable=False` (default): reported numbers, python floats, no graph.

  `differentiable=True`: the same `StateMetrics` with 0-dim float64 tensors (on the host), every model-dependent field an
  autograd node over the circuit's and the energy's variables: `fidelity`, `overlap`, `cross_entropy`,
  `relative_entropy` and `log_partition` are losses; for normalised data the gradient of `relative_entropy` is that of
  `qmhl`.  The three Gram matrices have the bits of the default path.  `trace`, `purity` and `entropy` depend on the data
  alone and are constants.  In the fidelity an eigenvalue of W^1/2 G_p W^1/2 at or below 0 contributes nothing and carries
  no gradient.  No gradient reaches the data's states or weights; states that require grad are refused.  The final
  states, both tables and their cotangents are resident together until backward; double backward is refused."""
  if not isinstance(data, quantum_data.StateVectorData):
    raise TypeError("state_metrics takes StateVectorData")
  qubits = sorted(model.circuit.qubits)
  n = len(qubits)
  if data.num_qubits != n:
    raise ValueError(f"the model acts on {n} qubits, the states live on {data.num_qubits}")
  if data.qubits is not None and list(data.qubits) != qubits:
    raise ValueError("the model's qubits are not the data's")
  if n > max_qubits:
    raise ValueError(f"an energy table over {n} qubits has 2^{n} entries: above max_qubits = {max_qubits}")
  weights = _weights_of(data)
  device = _device()
  if differentiable:
    return _differentiable_metrics(model, data, table, max_qubits, n, weights, device)
  with torch.no_grad():
    eng, values = _inverse_circuit_engine(model, device)
    amplitudes = eng.statevector_from_states(data._device_states(), values)  # pylint: disable=protected-access
    energies = energy_utils.energy_table(model.energy, n, max_qubits, method=table).detach().to(device)
    log_z, probs = _partition(energies)
    # (t = 1: U drops out of G_1 = Phi^dagger Phi, so the data's own metrics come from the states as given and
    # `data.entropy()` is the same number to the last bit)
    gram_one = _engine.weighted_gram(data._device_states())  # pylint: disable=protected-access
    gram_p = _engine.weighted_gram(amplitudes, probs)
    gram_e = _engine.weighted_gram(amplitudes, energies)
    trace, purity, entropy = _sigma_metrics(gram_one, weights)
    overlap = float(torch.sum(weights * gram_p.cpu().diagonal().real))
    fidelity = float(torch.sum(torch.sqrt(_weighted_spectrum(gram_p, weights)))**2)
    log_partition = float(log_z)
    cross = float(torch.sum(weights * gram_e.cpu().diagonal().real)) + log_partition * trace
  return StateMetrics(trace, purity, entropy, overlap, fidelity, log_partition, cross, cross - entropy)
