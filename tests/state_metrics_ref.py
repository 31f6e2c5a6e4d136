"""complex128 numpy restatement of the state-vector metrics: the weighted Gram matrix the HIP kernel sums,
and every metric `inference.state_metrics` derives from three of them.  No GPU, no engine; written from the formulas,
not from the kernel."""
import numpy as np


def gram(states, table=None):
  """G[i, j] = sum_x table[x] conj(states[i, x]) states[j, x] in complex128; `table` None: ones."""
  s = np.asarray(states).astype(np.complex128)
  t = np.ones(s.shape[1]) if table is None else np.asarray(table).astype(np.float64)
  return s.conj() @ (s * t[None, :]).T


def gram_bound(states, table=None):
  """sum_x |table[x]| |states[i, x]| |states[j, x]| in float64: what the kernel's error bound is a multiple of."""
  a = np.abs(np.asarray(states).astype(np.complex128))
  t = np.ones(a.shape[1]) if table is None else np.abs(np.asarray(table).astype(np.float64))
  return a @ (a * t[None, :]).T


def _spectrum(gram_matrix, weights):
  root = np.sqrt(np.asarray(weights, dtype=np.float64))
  b = root[:, None] * gram_matrix * root[None, :]
  return np.clip(np.linalg.eigvalsh((b + b.conj().T) / 2), 0.0, None)


def metrics(unitary, energies, states, weights):
  """dict of trace, purity, entropy, overlap, fidelity, log_partition, cross_entropy, relative_entropy of
  sigma = sum_m weights[m] |states[m]><states[m]| against rho = U diag(softmax(-energies)) U^dagger, through
  a_m = U^dagger states[m] and the Gram matrices with t in {1, p, E}."""
  u = np.asarray(unitary).astype(np.complex128)
  e = np.asarray(energies).astype(np.float64)
  w = np.asarray(weights, dtype=np.float64)
  a = (u.conj().T @ np.asarray(states).astype(np.complex128).T).T
  shift = (-e).max()
  log_z = shift + np.log(np.sum(np.exp(-e - shift)))
  p = np.exp(-e - log_z)
  g1, gp, ge = gram(a), gram(a, p), gram(a, e)
  lam = _spectrum(g1, w)
  pos = lam[lam > 0]
  trace = float(np.sum(w * np.diag(g1).real))
  entropy = float(-np.sum(pos * np.log(pos)))
  cross = float(np.sum(w * np.diag(ge).real) + log_z * trace)
  return {"trace": trace, "purity": float(np.sum(lam**2)), "entropy": entropy,
          "overlap": float(np.sum(w * np.diag(gp).real)),
          "fidelity": float(np.sum(np.sqrt(_spectrum(gp, w)))**2), "log_partition": float(log_z),
          "cross_entropy": cross, "relative_entropy": cross - entropy}


def dense_sigma(states, weights):
  s = np.asarray(states).astype(np.complex128)
  return (s.T * np.asarray(weights, dtype=np.float64)[None, :]) @ s.conj()


def dense_sigma_metrics(sigma, rho):
  """(trace, purity, entropy, D(sigma || rho) on sigma's support) from dense matrices by eigendecomposition."""
  lam, vec = np.linalg.eigh((sigma + sigma.conj().T) / 2)
  keep = lam > 1e-13 * lam.max()
  lam, vec = lam[keep], vec[:, keep]
  r, rv = np.linalg.eigh((rho + rho.conj().T) / 2)
  log_rho = (rv * np.log(r)[None, :]) @ rv.conj().T
  cross = -np.real(np.trace(sigma @ log_rho))
  entropy = float(-np.sum(lam * np.log(lam)))
  return float(np.real(np.trace(sigma))), float(np.real(np.trace(sigma @ sigma))), entropy, float(cross - entropy)
