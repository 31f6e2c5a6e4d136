"""Numpy checkers of the BKM information matrix (reference baselines/train.py:161-249).

`reference_loop` restates the reference's loop on the gate-by-gate oracle: every circuit variable shifted by +-1/2
(all of its occurrences), a full gradient of the modular-Hamiltonian expectation per shifted point.  `dense_blocks`
is the closed form -d^2/d theta_i d theta'_j tr[rho(theta) K(theta')] with dense complex128 matrices and central
differences -- independent of every shift rule."""
import math

import numpy as np

from oracle import qhbm_oracle as O


def total_gates(gates, n_params):
  """Model circuit followed by its inverse on a second copy of the parameters (indices + n_params)."""
  inv = []
  for g in reversed(gates):
    kind, q0, q1, p, s, o = g[:6]
    inv.append((kind, q0, q1, p + n_params if p >= 0 else p, -s, -o) + tuple(g[6:]))
  return list(gates) + inv


def _g(n, gates, theta, theta_p, bits, shards, weights, phi):
  """(d/dphi' f [K], d/dtheta' f [P]) of f = sum_u w_u sum_k phi_k <shard_k>_u on the total circuit."""
  p = len(theta)
  vals, jac = O.expectation_jacobian(n, total_gates(gates, p), np.concatenate([theta, theta_p]), bits, shards)
  w = np.asarray(weights, np.float64)
  return w @ vals, np.einsum("u,k,ukp->p", w, np.asarray(phi, np.float64), jac)[p:]


def reference_loop(n, gates, theta, phi, parity_sets, shards, bits, weights):
  """(ebm [T, T], cross [P, T], qnn [P, P]) as train.py:176-240 computes them, on fixed weighted bitstrings."""
  theta = np.asarray(theta, np.float64)
  w = np.asarray(weights, np.float64)
  jac_e = O.parities(bits, parity_sets)
  mu = w @ jac_e
  ebm = (jac_e - mu).T @ (w[:, None] * (jac_e - mu))
  p = len(theta)
  cross = np.zeros((p, len(shards)))
  qnn = np.zeros((p, p))
  for i in range(p):
    lo, hi = theta.copy(), theta.copy()
    lo[i] -= 0.5
    hi[i] += 0.5
    gphi_lo, gth_lo = _g(n, gates, lo, theta, bits, shards, w, phi)
    gphi_hi, gth_hi = _g(n, gates, hi, theta, bits, shards, w, phi)
    cross[i] = 0.5 * math.pi * (gphi_lo - gphi_hi)
    qnn[i] = 0.5 * math.pi * (gth_lo - gth_hi)
  return ebm, cross, qnn


def assemble(ebm, cross, qnn, symmetrize=True):
  m = np.block([[ebm, cross.T], [cross, qnn]])
  return (m + m.T) / 2.0 if symmetrize else m


def _unitary(n, gates, params):
  cols = [O.simulate(n, gates, params, b).reshape(-1) for b in O.all_bitstrings(n)]
  return np.stack(cols, 1)


def dense_blocks(n, gates, theta, phi, parity_sets, bits, weights, h=1e-4):
  """(cross [P, T], qnn [P, P]): -d^2/d theta_i d theta'_j tr[rho(theta) K(theta')], rho = sum_x w(x) U|x><x|U^dag,
  K(theta') = U(theta') diag(E_phi) U(theta')^dag -- dense matrices, central differences."""
  theta = np.asarray(theta, np.float64)
  p = len(theta)
  index = [int("".join(str(int(v)) for v in b), 2) for b in np.asarray(bits)]
  pw = np.zeros(2**n)
  np.add.at(pw, index, np.asarray(weights, np.float64))
  par = O.parities(O.all_bitstrings(n), parity_sets)     # [2^n, T]
  energies = par @ np.asarray(phi, np.float64)

  def rho(t):
    u = _unitary(n, gates, t)
    return (u * pw[None, :]) @ u.conj().T

  def kmat(t, diag):
    u = _unitary(n, gates, t)
    return (u * diag[None, :]) @ u.conj().T

  def dtheta(fn):
    out = []
    for i in range(p):
      e = np.zeros(p)
      e[i] = h
      out.append((fn(theta + e) - fn(theta - e)) / (2 * h))
    return out

  drho = dtheta(rho)
  dk = dtheta(lambda t: kmat(t, energies))
  qnn = -np.array([[np.real(np.trace(drho[i] @ dk[j])) for j in range(p)] for i in range(p)])
  k_t = [kmat(theta, par[:, t]) for t in range(par.shape[1])]
  cross = -np.array([[np.real(np.trace(drho[i] @ k_t[t])) for t in range(par.shape[1])] for i in range(p)])
  return cross, qnn
