"""Complex128 restatement of the from-states calls (`qhbm_expectation_from_states`, `..._vjp_from_states`,
`qhbm_statevector_from_states`): a gate list applied to a GIVEN state, the values of Pauli-sum observables and the
VJP of a given upstream, from the oracle's own gate matrices.  Nothing of the engine is used here.

States are [M, 2^n] arrays, amplitude index = the bitstring read big-endian (qubit 0 most significant): the layout of
`qhbm_statevector`.  Nothing is normalised: values and gradients are the plain quadratic functions of the states."""
import numpy as np

from oracle import qhbm_oracle as O


def _gate_qubits(gate):
  kind, q0, q1 = gate[:3]
  return (q0,) if O.gate_num_qubits(kind) == 1 else (q0, q1)


def apply_circuit(n, gates, params, state):
  """C(params) |state>; `state` has 2^n amplitudes, the result the shape (2,) * n."""
  psi = np.asarray(state, dtype=np.complex128).reshape((2,) * n)
  for g in gates:
    mat = O.gate_matrix(g[0], O.gate_exponent(g, params), O.gate_global_shift(g))
    psi = O._apply_matrix(psi, mat, _gate_qubits(g))  # pylint: disable=protected-access
  return psi


def final_states(n, gates, params, states):
  """[M, 2^n] complex128: C |phi_m>, global phase included."""
  return np.stack([apply_circuit(n, gates, params, s).reshape(-1) for s in np.asarray(states)])


def values(n, gates, params, states, ops):
  """[M, T]: <phi_m| C^dagger O_t C |phi_m>."""
  out = np.zeros((len(states), len(ops)))
  for m, s in enumerate(np.asarray(states)):
    psi = apply_circuit(n, gates, params, s)
    for t, op in enumerate(ops):
      out[m, t] = O.op_expectation(psi, op)
  return out


def values_and_rows(n, gates, params, states, ops, upstream):
  """(values [M, T], rows [M, P]): rows[m] = sum_t upstream[m, t] d values[m, t] / d params, by the adjoint recursion
  of `O.expectation_jacobian` started from the given state instead of a basis state."""
  params = np.asarray(params, dtype=np.float64)
  upstream = np.asarray(upstream, dtype=np.float64)
  vals = np.zeros((len(states), len(ops)))
  rows = np.zeros((len(states), len(params)))
  for m, s in enumerate(np.asarray(states)):
    psi_final = apply_circuit(n, gates, params, s)
    lam = np.zeros_like(psi_final)
    for t, op in enumerate(ops):
      o_psi = O.apply_op(psi_final, op)
      vals[m, t] = float(np.real(np.vdot(psi_final.ravel(), o_psi.ravel())))
      lam = lam + upstream[m, t] * o_psi
    psi = psi_final
    for g in reversed(gates):
      kind, pidx, scalar = g[0], g[3], g[4]
      shift = O.gate_global_shift(g)
      t_g = O.gate_exponent(g, params)
      qs = _gate_qubits(g)
      u_dag = O.gate_matrix(kind, t_g, shift).conj().T
      psi = O._apply_matrix(psi, u_dag, qs)  # pylint: disable=protected-access
      if pidx >= 0:
        dpsi = O._apply_matrix(psi, O.gate_matrix_derivative(kind, t_g, shift), qs)  # pylint: disable=protected-access
        rows[m, pidx] += scalar * 2.0 * float(np.real(np.vdot(lam.ravel(), dpsi.ravel())))
      lam = O._apply_matrix(lam, u_dag, qs)  # pylint: disable=protected-access
  return vals, rows


def values_and_vjp(n, gates, params, states, ops, upstream):
  """(values [M, T], grad [P])."""
  vals, rows = values_and_rows(n, gates, params, states, ops, upstream)
  return vals, rows.sum(0)


def random_states(num, n, seed, normalise=True):
  """[num, 2^n] complex128 seeded complex Gaussians."""
  rng = np.random.default_rng(seed)
  st = rng.normal(size=(num, 1 << n)) + 1j * rng.normal(size=(num, 1 << n))
  if normalise:
    st /= np.linalg.norm(st, axis=1, keepdims=True)
  return st


def basis_states(bits):
  """[U, 2^n] complex128: |x_u> for bits [U, n]."""
  bits = np.asarray(bits)
  n = bits.shape[1]
  idx = (bits.astype(np.int64) << np.arange(n - 1, -1, -1)).sum(1)
  st = np.zeros((bits.shape[0], 1 << n), dtype=np.complex128)
  st[np.arange(bits.shape[0]), idx] = 1.0
  return st


def op_abs_sum(op):
  return float(sum(abs(c) for c, _, _ in op))
