"""float64 restatement of the VQT and QMHL losses on a GIVEN weighted multiset of bitstrings, with every gradient block
(tests/test_loss_ref_cpu.py checks it, tests/test_losses_hamiltonian_gpu.py holds the mirror and the engine to it).

Only numpy and the oracle are used: the circuit part is `oracle.qhbm_oracle` (complex128) below `C_ORACLE_FROM` qubits and
the threaded fp32 C restatement `oracle.qhbm_cpu` from there on; the product package is never imported.

Notation.  Rows x_i with weights w_i (counts / sum of counts, or any non-negative weights).  A spin-parity energy
E_t(x) = sum_k t_k parity_k(x) (Bernoulli: one term per bit; KOBE: all subsets up to `order`) has the Pauli shards
Z_{S_k}.  For a total circuit T (first circuit, then the INVERSE of the second) and shard coefficients c,

    s_k(x) = <x| T^dag Z_{S_k} T |x>,     value(x) = sum_k c_k s_k(x).

VQT against the Hamiltonian V_psi K_vartheta V_psi^dag with the model (E_theta, U_phi), T = U_phi then V_psi^dag:
    f_i   = beta * value(x_i) - E_theta(x_i)            (c = vartheta)
    loss  = sum_i w_i f_i - log Z_theta                 (the energies inside f and log Z are constants)
    d/d(phi, psi)  = beta * sum_i w_i d value(x_i)      (the combined operator through T, split at len(phi))
    d/d vartheta_k = beta * sum_i w_i s_k(x_i)
    d/d theta      = (sum_i w_i dE_i)(sum_i w_i f_i) - sum_i w_i f_i dE_i      (score function)

QMHL of the model (E_theta, U_phi) against data drawn from the QHBM (E^d_thetad, U^d_phid), T = U^d then U_phi^dag:
    g_i   = value(x_i)                                  (c = theta)
    loss  = sum_i w_i g_i + log Z_theta
    d/d theta_k    = sum_i w_i s_k(x_i) - sum_x p_theta(x) parity_k(x)
    d/d(phid, phi) = sum_i w_i d value(x_i)             (split at len(phid))
    d/d thetad     = the score-function form with g in place of f.

Bit order.  With `tfq_compat=True` column j of a row drives qubit `O.tfq_bit_permutation(n)[j]` of the circuit (the
injector); energies are evaluated on the rows as given and shard masks name the unpermuted qubits.
"""
import numpy as np

from oracle import qhbm_oracle as O

C_ORACLE_FROM = 16   # qubits from which the circuit part goes through the C restatement


class SpinEnergy:
  """E_t(x) = sum_k t_k prod_{j in S_k} (1 - 2 x_j): `order=None` is the Bernoulli energy (S_k = {k}), otherwise a KOBE
  of that order.  `shards` are the Z-string observables in the oracle's mask form, one per term."""

  def __init__(self, n, thetas, order=None, shards=None):
    self.n, self.order = int(n), order
    self.thetas = np.asarray(thetas, dtype=np.float64)
    self.index_sets = [(i,) for i in range(n)] if order is None else O.parity_indices(n, order)
    assert len(self.index_sets) == self.thetas.shape[0]
    if shards is None:
      shards = O.bernoulli_shards(n) if order is None else O.kobe_shards(n, order)
    self.shards = shards

  def with_thetas(self, thetas):
    return SpinEnergy(self.n, thetas, self.order, self.shards)

  def features(self, bits):
    """[U, K] = dE/dt on each row."""
    return O.parities(np.asarray(bits), self.index_sets)

  def energy(self, bits):
    return self.features(bits) @ self.thetas

  def _all_features(self):
    return self.features(O.all_bitstrings(self.n))

  def probabilities(self):
    """p_t(x) over all bitstrings in itertools.product order."""
    logits = -(self._all_features() @ self.thetas)
    p = np.exp(logits - logits.max())
    return p / p.sum()

  def log_partition(self):
    if self.order is None:   # sum_i log(e^t_i + e^-t_i)
      return float(np.sum(np.logaddexp(self.thetas, -self.thetas)))
    return float(np.logaddexp.reduce(-(self._all_features() @ self.thetas)))

  def log_partition_grad(self):
    """d log Z / dt_k = -sum_x p_t(x) parity_k(x); for the Bernoulli energy tanh(t_k)."""
    if self.order is None:
      return np.tanh(self.thetas)
    return -(self.probabilities() @ self._all_features())


def offset_gates(gates, offset):
  """The same gates with every parameter index moved up by `offset` (the second circuit of a sum)."""
  return [(g[0], g[1], g[2], g[3] + offset if g[3] >= 0 else g[3]) + tuple(g[4:]) for g in gates]


def total_circuit(first_gates, n_first, second_gates):
  """`first` followed by the inverse of `second`, over the parameter vector [first..., second...]."""
  return list(first_gates) + O.inverse_gates(offset_gates(second_gates, n_first))


def normalised(weights):
  w = np.asarray(weights, dtype=np.float64)
  return w / w.sum()


def shard_values(n, gates, params, bits, shards):
  """[U, K] of s_k(x_u), float64."""
  bits = np.asarray(bits, dtype=np.int8)
  if n >= C_ORACLE_FROM:
    from oracle import qhbm_cpu as C   # pylint: disable=import-outside-toplevel
    return C.expectation(n, gates, params, bits, shards).astype(np.float64)
  out = np.zeros((bits.shape[0], len(shards)))
  for u, row in enumerate(bits):
    psi = O.simulate(n, gates, params, row)
    for k, op in enumerate(shards):
      out[u, k] = O.op_expectation(psi, op)
  return out


def combined_gradient(n, gates, params, bits, shards, coeffs, row_weights):
  """[P] = sum_u row_weights_u d/dparams <x_u| T^dag (sum_k coeffs_k shard_k) T |x_u>: ONE operator, one adjoint sweep
  per row."""
  bits = np.asarray(bits, dtype=np.int8)
  combined = [[(float(t) * c, x, z) for t, op in zip(coeffs, shards) for c, x, z in op]]
  if n >= C_ORACLE_FROM:
    from oracle import qhbm_cpu as C   # pylint: disable=import-outside-toplevel
    _, grad = C.expectation_vjp(n, gates, params, bits, combined, np.asarray(row_weights, np.float32)[:, None])
    return grad.astype(np.float64)
  _, jac = O.expectation_jacobian(n, gates, params, bits, combined)
  return np.asarray(row_weights, dtype=np.float64) @ jac[:, 0, :]


def score_function_gradient(weights, features, values):
  """(sum w dE)(sum w v) - sum w v dE: the gradient of sum_x p_t(x) v(x) with respect to t, estimated on the multiset."""
  return (weights @ features) * (weights @ values) - weights @ (features * values[:, None])


def modular_expectation(n, first_gates, first_params, ham_energy, ham_gates, ham_params, bits, tfq_compat=False):
  """[U] of <x| U^dag (V K V^dag) U |x> and the [U, K] shard values behind it."""
  gates = total_circuit(first_gates, len(first_params), ham_gates)
  params = np.concatenate([first_params, ham_params]).astype(np.float64)
  s = shard_values(n, gates, params, O.apply_bit_order(np.asarray(bits), tfq_compat), ham_energy.shards)
  return s @ ham_energy.thetas, s


def vqt_hamiltonian(n, model_energy, model_gates, phi, target_energy, target_gates, psi, beta, bits, weights,
                    tfq_compat=False, circuit_gradients=True):
  """dict(loss, theta, phi, vartheta, psi, f): the VQT loss on the multiset and its four gradient blocks; `f` are the
  per-row values beta h(x_i) - E_theta(x_i).  `circuit_gradients=False` leaves the adjoint sweeps out (phi, psi: None)."""
  bits = np.asarray(bits, dtype=np.int8)
  w = normalised(weights)
  phi, psi = np.asarray(phi, np.float64), np.asarray(psi, np.float64)
  gates = total_circuit(model_gates, len(phi), target_gates)
  params = np.concatenate([phi, psi])
  injected = O.apply_bit_order(bits, tfq_compat)
  s = shard_values(n, gates, params, injected, target_energy.shards)
  f = beta * (s @ target_energy.thetas) - model_energy.energy(bits)
  phi_grad = psi_grad = None
  if circuit_gradients:
    circuit_grad = beta * combined_gradient(n, gates, params, injected, target_energy.shards, target_energy.thetas, w)
    phi_grad, psi_grad = circuit_grad[:len(phi)], circuit_grad[len(phi):]
  return dict(loss=float(w @ f - model_energy.log_partition()),
              theta=score_function_gradient(w, model_energy.features(bits), f), phi=phi_grad, psi=psi_grad,
              vartheta=beta * (w @ s), f=f)


def qmhl_qhbm_data(n, data_energy, data_gates, phid, model_energy, model_gates, phi, bits, weights, tfq_compat=False,
                   circuit_gradients=True):
  """dict(loss, theta, phi, thetad, phid, g): the QMHL loss of the model against data from a QHBM whose multiset is
  (bits, weights), and its four gradient blocks; `g` are the per-row values.  `circuit_gradients=False` leaves the
  adjoint sweeps out (phi, phid: None)."""
  bits = np.asarray(bits, dtype=np.int8)
  w = normalised(weights)
  phid, phi = np.asarray(phid, np.float64), np.asarray(phi, np.float64)
  gates = total_circuit(data_gates, len(phid), model_gates)
  params = np.concatenate([phid, phi])
  injected = O.apply_bit_order(bits, tfq_compat)
  s = shard_values(n, gates, params, injected, model_energy.shards)
  g = s @ model_energy.thetas
  phi_grad = phid_grad = None
  if circuit_gradients:
    circuit_grad = combined_gradient(n, gates, params, injected, model_energy.shards, model_energy.thetas, w)
    phid_grad, phi_grad = circuit_grad[:len(phid)], circuit_grad[len(phid):]
  return dict(loss=float(w @ g + model_energy.log_partition()),
              theta=w @ s + model_energy.log_partition_grad(), phi=phi_grad, phid=phid_grad,
              thetad=score_function_gradient(w, data_energy.features(bits), g), g=g)


def qhbm_expectation(n, energy_gates, params, bits, weights, ops, tfq_compat=False):
  """[T] weighted average of <x_i| U^dag O_t U |x_i> over the multiset (QHBM.expectation of a list of Pauli sums)."""
  vals = shard_values(n, energy_gates, np.asarray(params, np.float64), O.apply_bit_order(np.asarray(bits), tfq_compat), ops)
  return normalised(weights) @ vals
