"""complex128 numpy restatement of the cross-Gram matrix the HIP kernel sums (csrc/cross_gram.hip), and the
DENSE route to the metrics of two state ensembles: sigma and tau as 2^n x 2^n matrices, sqrt(sigma) by `eigh`,
1/2 ||sigma - tau||_1 by `eigvalsh`.  No GPU, no engine; written from the formulas, not from the kernel."""
import numpy as np

EPS = 2.0**-53


def cross_gram(bras, kets, table=None):
  """C[i, j] = sum_x table[x] conj(bras[i, x]) kets[j, x] in complex128; `table` None: ones."""
  a = np.asarray(bras).astype(np.complex128)
  b = np.asarray(kets).astype(np.complex128)
  t = np.ones(a.shape[1]) if table is None else np.asarray(table).astype(np.float64)
  return a.conj() @ (b * t[None, :]).T


def cross_gram_bound(bras, kets, table=None):
  """sum_x |table[x]| |bras[i, x]| |kets[j, x]| in float64: what the kernel's error bound is a multiple of."""
  a = np.abs(np.asarray(bras).astype(np.complex128))
  b = np.abs(np.asarray(kets).astype(np.complex128))
  t = np.ones(a.shape[1]) if table is None else np.abs(np.asarray(table).astype(np.float64))
  return a @ (b * t[None, :]).T


def dense(states, weights):
  """sum_m weights[m] |states[m]><states[m]| as a 2^n x 2^n complex128 matrix."""
  s = np.asarray(states).astype(np.complex128)
  return (s.T * np.asarray(weights, dtype=np.float64)[None, :]) @ s.conj()


def _sqrt_psd(rho):
  """sqrt(rho) by `eigh`.  Eigenvalues below 1e-10 of the largest are the rounded zeros of a rank-deficient rho and are
  dropped -- the root of a rounded zero (1e-17 -> 3e-9) would otherwise be the largest error of the whole route; the inputs
  of the tests keep their non-zero eigenvalues within a factor 1e4 of the largest."""
  lam, vec = np.linalg.eigh((rho + rho.conj().T) / 2)
  keep = lam > 1e-10 * lam.max()
  return (vec[:, keep] * np.sqrt(lam[keep])[None, :]) @ vec[:, keep].conj().T


def dense_metrics(sigma, tau):
  """dict of trace_a, trace_b, purity_a, purity_b, overlap, fidelity, trace_distance from the dense matrices: the fidelity
  as the squared nuclear norm of sqrt(sigma) sqrt(tau) (= (tr sqrt(sqrt(sigma) tau sqrt(sigma)))^2)."""
  singular = np.linalg.svd(_sqrt_psd(sigma) @ _sqrt_psd(tau), compute_uv=False)
  delta = sigma - tau
  return {"trace_a": float(np.trace(sigma).real), "trace_b": float(np.trace(tau).real),
          "purity_a": float(np.trace(sigma @ sigma).real), "purity_b": float(np.trace(tau @ tau).real),
          "overlap": float(np.trace(sigma @ tau).real), "fidelity": float(np.sum(singular)**2),
          "trace_distance": float(0.5 * np.sum(np.abs(np.linalg.eigvalsh((delta + delta.conj().T) / 2))))}


def joint_gram(states_a, weights_a, states_b, weights_b):
  """Gamma: the Gram matrix of the M + K scaled states [sqrt(w_m) a_m, sqrt(v_k) b_k] (complex128)."""
  a = np.asarray(states_a).astype(np.complex128) * np.sqrt(np.asarray(weights_a, dtype=np.float64))[:, None]
  b = np.asarray(states_b).astype(np.complex128) * np.sqrt(np.asarray(weights_b, dtype=np.float64))[:, None]
  both = np.concatenate([a, b], 0)
  return both.conj() @ both.T


def well_conditioned_ensembles(n, num_a, num_b, seed, orthogonal=False):
  """(states_a [M, 2^n], weights_a, states_b [K, 2^n], weights_b) complex128 / float64 with M + K <= 2^n: random complex
  states, neither orthogonal nor normalised, with random positive weights, whose joint Gram matrix has a condition number
  of a few -- a random orthonormal frame of M + K columns times I + 0.3 N / ||N||_2, N complex Gaussian (singular values in
  [0.7, 1.3]), weights uniform in [0.5, 1] / (number of states).  `orthogonal`: the two ensembles are mixed among
  themselves only, so their supports are orthogonal."""
  rng = np.random.default_rng(seed)
  total, dim = num_a + num_b, 1 << n
  assert total <= dim
  frame = np.linalg.qr(rng.normal(size=(dim, total)) + 1j * rng.normal(size=(dim, total)))[0]
  noise = rng.normal(size=(total, total)) + 1j * rng.normal(size=(total, total))
  if orthogonal:
    noise[:num_a, num_a:] = 0.0
    noise[num_a:, :num_a] = 0.0
  mix = np.eye(total) + 0.3 * noise / np.linalg.norm(noise, 2)
  states = (frame @ mix).T
  return (states[:num_a], rng.uniform(0.5, 1.0, num_a) / num_a, states[num_a:], rng.uniform(0.5, 1.0, num_b) / num_b)
