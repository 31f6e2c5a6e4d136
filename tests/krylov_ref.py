"""float64 / complex128 restatement of the engine's Krylov routines (include/qhbm_engine.h qhbm_krylov_basis,
qhbm_krylov_combine), for the tests.  The product never imports it.  Built on `thermal_ref.apply_h`.

Per start state phi, for j = 0 .. m - 1:
  v_0 = phi / ||phi||;  w = H v_j
  per round: c_i = <v_i, w> for i in [lo, j] (all from the same w, float64 sums), then w <- w - sum_i c_i v_i, i ascending
  alpha_j = sum over rounds of Re c_j;  beta_j = ||w||;  beta_j <= 2^-16 R: exhausted (length j + 1, beta_j = 0, zeros after)
  v_{j+1} = w / beta_j
reorth=True: lo = 0, two rounds; reorth=False: lo = max(0, j - 1), one round.

`dtype=np.float32` runs the same arithmetic with complex64 vectors, float32 operator coefficients and the c_i rounded to
complex64 before they are used; inner products, norms, alpha and beta stay float64, as on the device: the rounding an fp32
implementation of the algorithm has, which the GPU tests' bars are derived from."""
import numpy as np

from tests import thermal_ref as T

BREAKDOWN = 2.0**-16


def lanczos(n, ops, starts, m, weights=None, reorth=True, dtype=np.float64, raw_norms=None):
  """(basis [m, U, 2^n], alpha [U, m], beta [U, m], lengths [U] int32, start norms [U]) as `Engine.krylov_basis`.
  `raw_norms` (a list): gets ||w|| [U] of every step as computed, before the breakdown rule puts zeros."""
  cdtype = np.complex64 if dtype == np.float32 else np.complex128
  starts = np.asarray(starts, cdtype)
  num, dim = starts.shape
  threshold = BREAKDOWN * T.radius(n, ops, weights)
  norms = np.linalg.norm(starts.astype(np.complex128), axis=1)
  basis = np.zeros((m, num, dim), cdtype)
  alpha, beta = np.zeros((num, m)), np.zeros((num, m))
  lengths = np.where(norms > 0, m, 0).astype(np.int32)
  scale = np.where(norms > 0, 1.0 / np.where(norms > 0, norms, 1.0), 0.0)
  live = norms > 0
  basis[0] = (starts.astype(np.complex128) * scale[:, None]).astype(cdtype)
  for j in range(m):
    w = T.apply_h(n, ops, basis[j], weights, dtype).astype(cdtype)
    lo = 0 if reorth else max(0, j - 1)
    for _ in range(2 if reorth else 1):
      rows = basis[lo:j + 1].astype(np.complex128)
      coef = np.einsum("iud,ud->iu", rows.conj(), w.astype(np.complex128))
      alpha[:, j] += coef[j - lo].real
      coef = coef.astype(cdtype)
      for i in range(lo, j + 1):
        w = (w - coef[i - lo][:, None] * basis[i]).astype(cdtype)
    norm = np.linalg.norm(w.astype(np.complex128), axis=1)
    if raw_norms is not None:
      raw_norms.append(norm)
    broke = live & (norm <= threshold)
    lengths[broke] = j + 1
    live = live & ~broke
    beta[:, j] = np.where(live, norm, 0.0)
    scale = np.where(live, 1.0 / np.where(live, norm, 1.0), 0.0)
    if j + 1 < m:
      basis[j + 1] = (w.astype(np.complex128) * scale[:, None]).astype(cdtype)
  return basis, alpha, beta, lengths, norms


def combine(basis, coef):
  """out[u, s] = sum_j coef[u, s, j] basis[j, u]: complex128 for a complex128 basis; for a complex64 basis the
  coefficients rounded to complex64 and the sum in complex64 with j ascending, as `qhbm_krylov_combine` adds."""
  if basis.dtype == np.complex128:
    return np.einsum("usj,jud->usd", np.asarray(coef, np.complex128), basis)
  coef = np.asarray(coef).astype(np.complex64)
  out = np.zeros(coef.shape[:2] + basis.shape[2:], np.complex64)
  for j in range(basis.shape[0]):
    out = (out + coef[:, :, j, None] * basis[j][:, None, :]).astype(np.complex64)
  return out


def _unit(vec):
  norm = np.linalg.norm(vec.astype(np.complex128))
  return vec * vec.real.dtype.type(1.0 / norm) if norm > 0 else vec


def tridiagonal(alpha, beta, length):
  k = int(length)
  return np.diag(alpha[:k]) + np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1)


def ritz(alpha, beta, length):
  """(theta [k], S [k, k]) of T = tridiag(alpha[:k], beta[:k - 1]), k = length."""
  if length == 0:
    return np.zeros(0), np.zeros((0, 0))
  return np.linalg.eigh(tridiagonal(alpha, beta, length))


def evolve(basis, alpha, beta, lengths, norms, tau, mode):
  """(states, log norms) from the stored space: mode 0 V e^{-tau T} e_1 normalised with log ||e^{-tau T} e_1|| + log ||phi||
  from T alone, mode 1 ||phi|| V e^{-i tau T} e_1 and None.  The sums over the basis are `combine`'s: complex128 for a
  complex128 basis, complex64 with j ascending for a complex64 one."""
  m, num, _ = basis.shape
  coef = np.zeros((num, 1, m), np.complex128)
  logs = np.full(num, -np.inf)
  for u in range(num):
    k = int(lengths[u])
    if k == 0:
      continue
    theta, s = ritz(alpha[u], beta[u], k)
    if mode == 0:
      e = s @ (np.exp(-tau * (theta - theta[0])) * s[0])
      logs[u] = np.log(np.linalg.norm(e)) - tau * theta[0] + np.log(norms[u])
    else:
      e = s @ (np.exp(-1j * tau * theta) * s[0]) * norms[u]
    coef[u, 0, :k] = e
  out = combine(basis, coef)[:, 0]
  if mode == 0:
    out = np.stack([_unit(v) for v in out])
  return out, (logs if mode == 0 else None)


def ground(basis, alpha, beta, lengths):
  """(theta_min [U], theta_max [U], ground vectors [U, 2^n] normalised) from the stored space."""
  m, num, _ = basis.shape
  lo, hi, coef = np.zeros(num), np.zeros(num), np.zeros((num, 1, m), np.complex128)
  for u in range(num):
    k = int(lengths[u])
    theta, s = ritz(alpha[u], beta[u], k)
    lo[u], hi[u] = theta[0], theta[-1]
    coef[u, 0, :k] = s[:, 0]
  return lo, hi, np.stack([_unit(v) for v in combine(basis, coef)[:, 0]])


def align(vec, want):
  """vec times the phase that makes <want, vec> real and positive."""
  overlap = np.vdot(want, vec)
  return vec * (np.conj(overlap) / abs(overlap))


def sweep_log_weights(alpha, beta, lengths, norms, betas):
  """l_m(beta) [B, M] = log sum_i S_m[0, i]^2 e^{-beta theta_i} + 2 log ||phi_m||."""
  out = np.full((len(betas), len(lengths)), -np.inf)
  for u in range(len(lengths)):
    if lengths[u] == 0:
      continue
    theta, s = ritz(alpha[u], beta[u], lengths[u])
    for b, value in enumerate(betas):
      out[b, u] = T.logsumexp(np.log(s[0]**2 + 1e-300) - value * theta) + 2.0 * np.log(norms[u])
  return out


def ground_state(n, ops, start, num_steps=24, max_restarts=8, tolerance=2.0**-20, weights=None, reorth=True, dtype=np.float64):
  """(E_0, state, residual, restarts) as `inference.ground_state`: restarted from the lowest Ritz vector until
  beta_{k-1} |S[k - 1, 0]| <= tolerance R."""
  radius = T.radius(n, ops, weights)
  current, restarts = np.asarray(start).reshape(1, -1), 0
  while True:
    basis, alpha, beta, lengths, _ = lanczos(n, ops, current, num_steps, weights, reorth, dtype)
    theta, s = ritz(alpha[0], beta[0], lengths[0])
    residual = float(beta[0, lengths[0] - 1] * abs(s[-1, 0]))
    current = ground(basis, alpha, beta, lengths)[2]
    if residual <= tolerance * radius or restarts >= max_restarts:
      return float(theta[0]), current[0], residual, restarts
    restarts += 1
