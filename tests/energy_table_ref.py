"""Exact restatements behind the energy-table tests (no engine code is used here).

A table E[y] over the 2^n amplitude indices (qubit 0 most significant) IS the Pauli operator sum_S c_S Z_S with
c = the Walsh-Hadamard transform of E divided by 2^n: `table_as_pauli_op` writes it in the oracle's (coeff, x_mask,
z_mask) form, so `O.expectation_jacobian` gives the values and Jacobian of a table exactly.  `diag_vjp` is the same
adjoint restated for a diagonal operator (lambda = E psi), cheap enough for n = 12."""
import numpy as np
import torch

from oracle import qhbm_oracle as O


def walsh(table):
  """c[s] = 2^-n sum_y E[y] (-1)^{popc(s & y)}, index-bit space, fp64."""
  c = np.asarray(table, dtype=np.float64).copy()
  h = 1
  while h < c.size:
    c = c.reshape(-1, 2, h)
    c = np.stack([c[:, 0] + c[:, 1], c[:, 0] - c[:, 1]], axis=1).reshape(-1)
    h *= 2
  return c / c.size


def table_as_pauli_op(table, n):
  """The table as an oracle op: Z strings in QUBIT space (index bit n-1-q <-> qubit q)."""
  op = []
  for s, coeff in enumerate(walsh(table)):
    z = 0
    for q in range(n):
      if s >> (n - 1 - q) & 1:
        z |= 1 << q
    op.append((float(coeff), 0, z))
  return op


def probabilities(n, gates, params, bits):
  """[U, 2^n] |<y|C|x_u>|^2 in fp64 (O.simulate, C order = qubit 0 most significant)."""
  return np.stack([np.abs(O.simulate(n, gates, params, b).ravel()) ** 2 for b in np.asarray(bits)])


def oracle_vjp(n, gates, params, bits, table, upstream):
  """(values [U], grad [P], table_grad [2^n]) through O.expectation_jacobian of the Walsh form."""
  vals, jac = O.expectation_jacobian(n, gates, params, bits, [table_as_pauli_op(table, n)])
  up = np.asarray(upstream, dtype=np.float64)
  return vals[:, 0], np.einsum("u,up->p", up, jac[:, 0, :]), up @ probabilities(n, gates, params, bits)


def diag_vjp(n, gates, params, bits, table, upstream=None):
  """(values [U], jacobian [U, P], probabilities [U, 2^n]): O.expectation_jacobian's adjoint with lambda = E psi."""
  diag = np.asarray(table, dtype=np.float64).reshape((2,) * n)
  bits = np.asarray(bits)
  vals = np.zeros(bits.shape[0])
  jac = np.zeros((bits.shape[0], len(params)))
  probs = np.zeros((bits.shape[0], 1 << n))
  for b, row in enumerate(bits):
    psi = O.simulate(n, gates, params, row)
    probs[b] = np.abs(psi.ravel()) ** 2
    lam = diag * psi
    vals[b] = float(np.real(np.vdot(psi.ravel(), lam.ravel())))
    for g in reversed(gates):
      kind, q0, q1, pidx, scalar = g[:5]
      shift = O.gate_global_shift(g)
      t = O.gate_exponent(g, params)
      qs = (q0,) if O.gate_num_qubits(kind) == 1 else (q0, q1)
      u_dag = O.gate_matrix(kind, t, shift).conj().T
      psi = O._apply_matrix(psi, u_dag, qs)  # pylint: disable=protected-access
      if pidx >= 0:
        dpsi = O._apply_matrix(psi, O.gate_matrix_derivative(kind, t, shift), qs)  # pylint: disable=protected-access
        jac[b, pidx] += scalar * 2.0 * float(np.real(np.vdot(lam.ravel(), dpsi.ravel())))
      lam = O._apply_matrix(lam, u_dag, qs)  # pylint: disable=protected-access
  return vals, jac, probs


def random_table(n, rng):
  """Mixed signs, a dynamic range of 10^3."""
  return (rng.choice([-1.0, 1.0], 1 << n) * 10.0 ** rng.uniform(-1.5, 1.5, 1 << n)).astype(np.float32)


def kobe2_table(n, thetas):
  """Diagonal of the KOBE-2 operator sum_k theta_k Z_{S_k} (S_k: O.parity_indices(n, 2) order)."""
  return O.kobe_energy(O.all_bitstrings(n), np.asarray(thetas, dtype=np.float64), 2).astype(np.float32)


def kobe2_op(n, thetas):
  return [(float(t) * c, x, z) for t, shard in zip(thetas, O.kobe_shards(n, 2)) for c, x, z in shard]


def mlp_layers(n, hidden, seed):
  """An MLP energy's layers (spins -> Linear -> Tanh -> Linear), deterministic weights."""
  from qhbmlib_amd import models
  gen = torch.Generator().manual_seed(seed)
  l1, l2 = torch.nn.Linear(n, hidden), torch.nn.Linear(hidden, 1)
  with torch.no_grad():
    for p in list(l1.parameters()) + list(l2.parameters()):
      p.copy_(torch.rand(p.shape, generator=gen) * 2.0 - 1.0)
  return [models.SpinsFromBitstrings(), l1, torch.nn.Tanh(), l2]


def mlp_table_f64(energy, n):
  """(table [2^n] in fp64 as a function of fp64 copies (W1, b1, W2, b2) of an `mlp_layers` energy's weights, the copies):
  the MLP restated in torch fp64 on the CPU."""
  lin = [l for l in energy.energy_layers if isinstance(l, torch.nn.Linear)]
  params = [t.detach().cpu().double().requires_grad_(True) for l in lin for t in (l.weight, l.bias)]
  w1, b1, w2, b2 = params
  spins = 1.0 - 2.0 * torch.from_numpy(O.all_bitstrings(n).astype(np.float64))
  return (torch.tanh(spins @ w1.T + b1) @ w2.T + b2).reshape(-1), params


def mlp_grads(energy):
  """The autograd .grad of an `mlp_layers` energy's weights, in mlp_table_f64's order."""
  lin = [l for l in energy.energy_layers if isinstance(l, torch.nn.Linear)]
  return [t for l in lin for t in (l.weight, l.bias)]
