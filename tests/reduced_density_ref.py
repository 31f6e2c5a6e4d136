"""A complex128 numpy restatement of the reduced density matrix: reshape, transpose, matmul.

    rho_A[a, a'] = sum_m w_m sum_b phi_m(a, b) conj(phi_m(a', b))

Qubit 0 is the most significant bit of an amplitude index (axis 0 of the [2] * n view); a reads the kept qubits big-endian
in ascending order, b the others.  Nothing here shares code with the product: the kernel's index arithmetic is deposits and
extracts of bit masks (csrc/rdm_index.h), this is numpy's axis bookkeeping."""
import numpy as np


def _panels(states, kept):
  """[M, 2^k, 2^(n-k)] view of the states with the kept qubits' axes first (both groups in ascending qubit order)."""
  states = np.asarray(states)
  num, dim = states.shape
  n = dim.bit_length() - 1
  assert dim == 1 << n
  kept = sorted(int(q) for q in kept)
  assert len(set(kept)) == len(kept) and all(0 <= q < n for q in kept) and kept
  env = [q for q in range(n) if q not in kept]
  view = states.reshape([num] + [2] * n).transpose([0] + [1 + q for q in kept] + [1 + q for q in env])
  return view.reshape(num, 1 << len(kept), 1 << len(env))


def reduced(states, kept, weights=None):
  """(rho_A complex128 [2^k, 2^k], S float64 [2^k, 2^k]) with S[a, a'] = sum_m |w_m| sum_b |phi_m(a, b)| |phi_m(a', b)|,
  what the rounding-error bound of a sum in any order is proportional to."""
  panels = _panels(states, kept).astype(np.complex128)
  num = panels.shape[0]
  w = np.ones(num) if weights is None else np.asarray(weights, dtype=np.float64).reshape(num)
  rho = np.einsum("m,mab,mcb->ac", w.astype(np.complex128), panels, panels.conj())
  mags = np.abs(panels)
  bound = np.einsum("m,mab,mcb->ac", np.abs(w), mags, mags)
  return rho, bound


def keep_mask(kept):
  """The engine's mask: bit q set <=> qubit q is kept."""
  return sum(1 << int(q) for q in set(kept))


def dense_sigma(states, weights=None):
  states = np.asarray(states).astype(np.complex128)
  w = np.ones(states.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
  return np.einsum("m,mi,mj->ij", w.astype(np.complex128), states, states.conj())


def dense_partial_trace(sigma, kept):
  """tr_B of a dense 2^n x 2^n matrix, index by index (no reshape: independent of `reduced`)."""
  sigma = np.asarray(sigma, dtype=np.complex128)
  dim = sigma.shape[0]
  n = dim.bit_length() - 1
  kept = sorted(int(q) for q in kept)
  k = len(kept)

  def row_of(index):
    a = 0
    for q in kept:
      a = (a << 1) | ((index >> (n - 1 - q)) & 1)
    return a
  kept_bits = sum(1 << (n - 1 - q) for q in kept)
  out = np.zeros((1 << k, 1 << k), dtype=np.complex128)
  for i in range(dim):
    for j in range(dim):
      if (i & ~kept_bits) == (j & ~kept_bits):
        out[row_of(i), row_of(j)] += sigma[i, j]
  return out


def entropy(rho):
  """von Neumann entropy of rho / tr rho in nats, eigenvalues clamped at 0, 0 log 0 = 0."""
  lam = np.clip(np.linalg.eigvalsh(0.5 * (rho + rho.conj().T)), 0.0, None)
  lam = lam / lam.sum()
  lam = lam[lam > 0]
  return float(-(lam * np.log(lam)).sum())
