"""Circuits with spectator qubits, their observables and a stacked fp64 oracle (tests/test_spectator_qubits_*.py).

A spectator is a qubit that no non-diagonal gate acts on before the last layer, if ever:

  idle  -- no gate at all;
  diag  -- Z powers, and CZ / ZZ powers with its neighbours, all parametrised;
  late  -- its only non-diagonal gate (X**t) is in the last layer.

A forward plan whose index bits all meet a non-diagonal gate writes one tile per state in its first pass
(PASS_NO_ZERO_FILL); with an idle or diagonal-only qubit the first pass zero-fills every tile instead.  The circuits
below reach both branches at sizes the numpy oracle still checks.
"""
import numpy as np

from oracle import qhbm_oracle as O
from tests.test_engine_gpu import random_circuit

# family -> {qubit: role}.  Qubit 0 is the top index bit, qubit n - 1 index bit 0.
FAMILIES = {
    "idle_low": lambda n: {n - 1: "idle"},
    "idle_top": lambda n: {0: "idle"},
    "diag": lambda n: {n // 2: "diag"},
    "late": lambda n: {1: "late"},
    "idle_diag": lambda n: {0: "idle", n - 2: "diag"},
}

# the kinds of the extra gates: every kind the two-term shift rule applies to
SHIFT_KINDS = [k for k in range(1, 12) if k != O.GATE_ISWAPPOW]


def spectator_circuit(n, family, seed, layers=2, extra=12):
  """(gates, n_params, roles, layer_of_param): an HEA (O.hea_gates) with the family's spectators, and `extra` random
  gates of every shift-rule kind on the other qubits in front of the last layer.  `layer_of_param[p]` is the HEA layer
  of parameter p (the extra gates reuse HEA parameters)."""
  roles = FAMILIES[family](n)
  rng = np.random.default_rng(seed)
  hea, names = O.hea_gates(n, layers, "s")
  n_params = len(names)
  layer_of_param = np.array([int(s.split("_")[2]) for s in names])
  per_layer = 2 * n + (n - 1)
  free = [q for q in range(n) if q not in roles]
  mixed = random_circuit(rng, len(free), extra, n_params, kinds=SHIFT_KINDS)
  mixed = [(g[0], free[g[1]], free[g[2]] if g[2] >= 0 else -1) + tuple(g[3:]) for g in mixed]
  gates = []
  for layer in range(layers):
    if layer == layers - 1:
      gates += mixed
    for g in hea[layer * per_layer:(layer + 1) * per_layer]:
      qs = [q for q in g[1:3] if q >= 0]
      if any(roles.get(q) == "idle" for q in qs):
        continue
      if g[0] == O.GATE_XPOW and (roles.get(g[1]) == "diag" or (roles.get(g[1]) == "late" and layer < layers - 1)):
        continue
      gates.append(g)
    for q, role in roles.items():   # a parametrised ZZ power with a neighbour: still diagonal
      if role == "diag":
        gates.append((O.GATE_ZZPOW, q, q - 1 if q > 0 else q + 1, int(rng.integers(n_params)), 0.8, 0.1))
  return gates, n_params, roles, layer_of_param


def idle_or_diag(roles):
  """The spectators whose input bit every final state keeps."""
  return [q for q, r in sorted(roles.items()) if r in ("idle", "diag")]


def _flip_term(coeff, q, other=None):
  """coeff * X_q (Y_q when `other` is None and coeff < 0), times Z_other if given."""
  x, z = 1 << q, 0
  if other is None and coeff < 0:
    z |= 1 << q
  if other is not None:
    z |= 1 << other
  return (float(coeff), x, z)


def op_sets(n, roles, seed):
  """name -> list of observables.  'ham': TFIM + XXZ, measured in the passes.  'wide': one random Pauli sum of 40
  terms, a quarter of them with X or Y on a spectator, plus terms whose only flip is on a spectator (the observable
  kernel; forward-only calls take the value from it too).  'shards': Z on every qubit and X / Y on every spectator,
  one observable each."""
  spec = sorted(roles)
  rng = np.random.default_rng(seed)
  wide = []
  for i, (c, x, z) in enumerate(O.random_pauli_op(n, 40, seed, p_identity=0.6)):
    if i % 4 == 0:
      q = spec[i // 4 % len(spec)]
      x |= 1 << q
      if rng.random() < 0.5:
        z |= 1 << q
    wide.append((c, x, z))
  other = next(q for q in range(n) if q not in roles)
  for q in spec:
    wide += [_flip_term(0.8, q), _flip_term(-0.6, q), _flip_term(0.5, q, other)]
  shards = [[(1.0, 0, 1 << q)] for q in range(n)]
  for q in spec:
    shards += [[(1.0, 1 << q, 0)], [(1.0, 1 << q, 1 << q)]]
  return {"ham": [O.tfim_ring_op(n), O.xxz_chain_op(n)], "wide": [wide], "shards": shards}


def shard_index(n, roles, q, pauli):
  """Index of the shard observable `pauli` (Z, X or Y) on spectator q in op_sets(...)['shards']."""
  if pauli == "Z":
    return q
  return n + 2 * sorted(roles).index(q) + (0 if pauli == "X" else 1)


def flipped(bits, roles):
  """The bitstrings with every spectator column flipped: their states lie where the states of `bits` must be 0."""
  out = np.array(bits, copy=True)
  for q in roles:
    out[:, q] ^= 1
  return out


def stacked_jacobian(n, gates, params, bits, ops):
  """(values [B, T], Jacobian [B, T, P], final states [B, 2^n]) in complex128: O.expectation_jacobian's adjoint
  recursion with the T lambdas carried as one trailing axis, psi simulated once per bitstring."""
  bits = np.asarray(bits)
  n_params = len(params)
  vals = np.zeros((bits.shape[0], len(ops)))
  jac = np.zeros((bits.shape[0], len(ops), n_params))
  states = np.zeros((bits.shape[0], 1 << n), np.complex128)
  for b, row in enumerate(bits):
    psi = O.simulate(n, gates, params, row)
    states[b] = psi.ravel()
    lam = np.stack([O.apply_op(psi, op) for op in ops], axis=-1)
    vals[b] = np.real(psi.ravel().conj() @ lam.reshape(-1, len(ops)))
    for g in reversed(gates):
      kind, q0, q1, pidx, scalar = g[:5]
      t = O.gate_exponent(g, params)
      shift = O.gate_global_shift(g)
      qs = (q0,) if O.gate_num_qubits(kind) == 1 else (q0, q1)
      u_dag = O.gate_matrix(kind, t, shift).conj().T
      psi = O._apply_matrix(psi, u_dag, qs)  # pylint: disable=protected-access
      if pidx >= 0:
        dpsi = O._apply_matrix(psi, O.gate_matrix_derivative(kind, t, shift), qs)  # pylint: disable=protected-access
        jac[b, :, pidx] += scalar * 2.0 * np.real(dpsi.ravel() @ lam.reshape(-1, len(ops)).conj())
      lam = O._apply_matrix(lam, u_dag, qs)  # pylint: disable=protected-access
  return vals, jac, states


def op_norm(ops):
  return np.array([sum(abs(c) for c, _, _ in op) for op in ops])
