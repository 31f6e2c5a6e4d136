"""Krylov spaces of a Pauli-sum Hamiltonian: ground states, spectral extremes and whole beta ladders from one run.

`thermal.thermal_ensemble` reaches e^{-beta H / 2} r by a Chebyshev sum whose number of H-applications grows with beta
R, one evolution per beta.  The Lanczos recurrence (`qhbm_krylov_basis`) instead stores the basis V of
span{phi, H phi, ..., H^{m-1} phi} and the tridiagonal T = V^dagger H V, and everything else is a function of T:

  e^{-tau H} phi ~ ||phi|| V e^{-tau T} e_1 for EVERY tau (mode 1: e^{-i tau T}),
  l(beta) = log <phi| e^{-beta H} |phi> ~ log sum_i S[0, i]^2 e^{-beta theta_i} + 2 log ||phi||   (T = S theta S^T),
  the extreme Ritz pairs (theta_0, V S[:, 0]) -> (E_0, ground state), theta_{k-1} -> E_max,

(finite-temperature Lanczos: Jaklic and Prelovsek, Phys. Rev. B 49, 5065 (1994)).  Everything of size 2^n is a kernel
of the engine over device-resident vectors; everything of size m^3 is float64 numpy on the host (`ritz`,
`evolution_coefficients`, `ftlm_log_weights`, `ftlm_energy`: plain functions of (alpha, beta, lengths), no device).

`store_basis=False` gives the same results without V in memory, m U 2^n amplitudes: pass one
(`qhbm_krylov_tridiagonal`) runs the local recurrence on three vectors and keeps T and the coefficients it subtracted; what
is a number is a function of T and costs nothing more; what is a vector, sum_j coef[j] v_j, costs one replay of the
recurrence (`qhbm_krylov_replay`), which regenerates each v_j bit for bit and adds it into up to eight outputs as it passes.
"""
import math

import numpy as np
import torch

from qhbmlib_amd import _engine
from qhbmlib_amd.inference import thermal

DEFAULT_STEPS = 48


# ---- host side: functions of T alone (float64) --------------------------------------------------------------------------------
def ritz(alpha, beta, length):
  """(theta [k], S [k, k]) of T = tridiag(alpha[:k], beta[:k - 1]), k = length: float64 `numpy.linalg.eigh`."""
  k = int(length)
  if k == 0:
    return np.zeros(0), np.zeros((0, 0))
  alpha, beta = np.asarray(alpha, np.float64), np.asarray(beta, np.float64)
  return np.linalg.eigh(np.diag(alpha[:k]) + np.diag(beta[:k - 1], 1) + np.diag(beta[:k - 1], -1))


def evolution_coefficients(theta, s, tau, mode, num_steps):
  """(coefficients [num_steps] of the basis rows, log ||e^{-tau T} e_1|| or None): mode 0 S (e^{-tau (theta - theta_0)} *
  S[0]) with its log norm - tau theta_0 apart, mode 1 S (e^{-i tau theta} * S[0])."""
  out = np.zeros(int(num_steps), np.complex128)
  k = len(theta)
  if k == 0:
    return out, (-np.inf if mode == 0 else None)
  if mode == 0:
    e = s @ (np.exp(-tau * (theta - theta[0])) * s[0])
    out[:k] = e
    return out, float(np.log(np.linalg.norm(e)) - tau * theta[0])
  out[:k] = s @ (np.exp(-1j * tau * theta) * s[0])
  return out, None


def _logsumexp(v):
  v = np.asarray(v, np.float64)
  top = v.max(initial=-np.inf)
  return float(top + np.log(np.exp(v - top).sum())) if np.isfinite(top) else float(top)


def ftlm_log_weights(pairs, norms, betas):
  """l_m(beta) [B, M] = log sum_i S_m[0, i]^2 e^{-beta theta_i} + 2 log ||phi_m|| from the Ritz pairs of M states."""
  out = np.full((len(betas), len(pairs)), -np.inf)
  for u, (theta, s) in enumerate(pairs):
    if len(theta) == 0 or norms[u] <= 0:
      continue
    with np.errstate(divide="ignore"):
      log_overlap = 2.0 * np.log(np.abs(s[0]))
    for b, value in enumerate(betas):
      out[b, u] = _logsumexp(log_overlap - value * theta) + 2.0 * math.log(norms[u])
  return out


def ftlm_energy(pairs, norms, betas):
  """<H>(beta) [B] = sum_m sum_i ||phi_m||^2 S_m[0, i]^2 theta_i e^{-beta theta_i} / the same sum without theta_i; NaN when
  no state has a space (every length or norm 0: Z = 0)."""
  out = np.full(len(betas), np.nan)
  for b, value in enumerate(betas):
    logs, thetas = [], []
    for u, (theta, s) in enumerate(pairs):
      if len(theta) == 0 or norms[u] <= 0:
        continue
      with np.errstate(divide="ignore"):
        logs.append(2.0 * np.log(np.abs(s[0])) - value * theta + 2.0 * math.log(norms[u]))
      thetas.append(theta)
    if not logs:
      continue
    logs, thetas = np.concatenate(logs), np.concatenate(thetas)
    w = np.exp(logs - logs.max())
    out[b] = float((w * thetas).sum() / w.sum())
  return out


def ftlm_log_partition(log_weights, num_qubits, start):
  """log Z [B] from l [B, M]: n log 2 + logsumexp_m(l) - log M from random vectors, logsumexp_m(l) (exact) from the basis."""
  total = np.array([_logsumexp(row) for row in log_weights])
  if start == "basis":
    return total
  return total + num_qubits * math.log(2.0) - math.log(log_weights.shape[1])


# ---- device side ------------------------------------------------------------------------------------------------------------------
def _normalise(states):
  """states / ||states|| per row (float64 norms; a row of norm 0 stays zeros)."""
  norms = torch.linalg.vector_norm(torch.view_as_real(states).flatten(1), dim=1, dtype=torch.float64)
  inv = torch.where(norms > 0, 1.0 / norms, torch.zeros_like(norms))
  return states * inv.to(torch.float32)[:, None]


class KrylovSpace:
  """The stored Lanczos spaces of M start states under H = sum_k weights[k] operators[k].

  `basis` [m, M, 2^n] complex64 (step-major) on the device; `alpha`, `beta` float64 [M, m] and `lengths` [M] on the host
  (read back once, on first use); `norms` float64 [M]: ||phi_m|| of the states as given; `radius`: R >= ||H||."""

  def __init__(self, operators, weights, qubits, basis, alpha, beta, lengths, norms, radius):
    self.operators = operators
    self.operator_weights = weights
    self.qubits = qubits
    self.basis = basis
    self._device = (alpha, beta, lengths, norms)
    self._host = None
    self._pairs = None
    self.radius = float(radius)

  @property
  def num_qubits(self):
    return len(self.qubits)

  @property
  def num_steps(self):
    return int(self.basis.shape[0])

  @property
  def num_vectors(self):
    return int(self.basis.shape[1])

  def _read(self):
    if self._host is None:
      self._host = tuple(t.cpu().numpy() for t in self._device)
    return self._host

  @property
  def alpha(self):
    return self._read()[0]

  @property
  def beta(self):
    return self._read()[1]

  @property
  def lengths(self):
    return self._read()[2]

  @property
  def norms(self):
    return self._read()[3]

  def ritz(self):
    """Per state the float64 eigenpairs (theta [k], S [k, k]) of T = tridiag(alpha[:k], beta[:k - 1]), k = length."""
    if self._pairs is None:
      alpha, beta, lengths, _ = self._read()
      self._pairs = [ritz(alpha[u], beta[u], lengths[u]) for u in range(self.num_vectors)]
    return self._pairs

  def residuals(self):
    """Per state beta_{k-1} |S[k - 1, i]| [k]: ||H y_i - theta_i y_i|| of the Ritz vectors; 0 after a breakdown."""
    _, beta, lengths, _ = self._read()
    return [beta[u, int(lengths[u]) - 1] * np.abs(s[-1]) if len(theta) else np.zeros(0)
            for u, (theta, s) in enumerate(self.ritz())]

  def _combine(self, coef):
    coef = torch.from_numpy(np.ascontiguousarray(coef.astype(np.complex64)))
    return _engine.krylov_combine(self.basis, coef)

  def ritz_states(self, indices=(0,)):
    """[M, len(indices), 2^n] complex64: the Ritz vectors V S[:, i] (negative i counts from the top), normalised on the
    device; zeros for a state of length 0."""
    indices = [int(i) for i in np.atleast_1d(indices)]
    coef = np.zeros((self.num_vectors, len(indices), self.num_steps), np.complex128)
    for u, (theta, s) in enumerate(self.ritz()):
      if len(theta):
        coef[u, :, :len(theta)] = s[:, indices].T
    out = self._combine(coef)
    return _normalise(out.flatten(0, 1)).reshape(out.shape)

  def evolve(self, tau, mode=0):
    """As `Engine.evolve_states` from the stored space, for any `tau` without another H-application.  mode 0: (e^{-tau H}
    phi_m normalised, float64 [M] log ||e^{-tau H} phi_m|| of the states as given, from T alone); mode 1: (e^{-i tau H}
    phi_m, None)."""
    if mode not in (0, 1):
      raise ValueError("mode must be 0 (imaginary time) or 1 (real time)")
    if not np.isfinite(tau) or (mode == 0 and tau < 0):
      raise ValueError(f"tau must be finite, and >= 0 in imaginary time, got {tau}")
    norms = self.norms
    coef = np.zeros((self.num_vectors, 1, self.num_steps), np.complex128)
    logs = np.full(self.num_vectors, -np.inf)
    for u, (theta, s) in enumerate(self.ritz()):
      coef[u, 0], log_norm = evolution_coefficients(theta, s, float(tau), mode, self.num_steps)
      if mode == 0 and len(theta):
        logs[u] = log_norm + math.log(norms[u])
      if mode == 1:
        coef[u, 0] *= norms[u]
    out = self._combine(coef)[:, 0]
    if mode == 1:
      return out, None
    return _normalise(out), torch.from_numpy(logs).to(out.device)

  def evolve_many(self, taus, mode=0):
    """`evolve` for every tau of `taus` from ONE sum over the space (a streamed space: one replay per eight taus): (states
    [M, len(taus), 2^n], float64 [M, len(taus)] log norms, or None in real time)."""
    if mode not in (0, 1):
      raise ValueError("mode must be 0 (imaginary time) or 1 (real time)")
    taus = np.asarray(taus, np.float64).reshape(-1)
    if len(taus) < 1 or not np.isfinite(taus).all() or (mode == 0 and (taus < 0).any()):
      raise ValueError(f"taus must be finite (at least one), and >= 0 in imaginary time, got {taus}")
    norms = self.norms
    coef = np.zeros((self.num_vectors, len(taus), self.num_steps), np.complex128)
    logs = np.full((self.num_vectors, len(taus)), -np.inf)
    for u, (theta, s) in enumerate(self.ritz()):
      for t, tau in enumerate(taus):
        coef[u, t], log_norm = evolution_coefficients(theta, s, float(tau), mode, self.num_steps)
        if mode == 0 and len(theta):
          logs[u, t] = log_norm + math.log(norms[u])
        if mode == 1:
          coef[u, t] *= norms[u]
    out = self._combine(coef)
    if mode == 1:
      return out, None
    return _normalise(out.flatten(0, 1)).reshape(out.shape), torch.from_numpy(logs).to(out.device)


class StreamedKrylovSpace(KrylovSpace):
  """The Lanczos spaces of M start states WITHOUT a stored basis (`krylov_space(store_basis=False)`): the
  interface of `KrylovSpace`, `basis` is None.  `alpha`, `beta`, `lengths`, `norms`, `radius`, `ritz()` and `residuals()`
  come from pass one alone.  `ritz_states`, `evolve` and `evolve_many` cost one replay of the recurrence per eight outputs:
  the space keeps the start states, the operators and the weights, and opens an engine per replay."""

  def __init__(self, operators, weights, qubits, starts, alpha, beta, lengths, recurrence, norms, radius):
    super().__init__(operators, weights, qubits, None, alpha, beta, lengths, norms, radius)
    self.starts = starts
    self.recurrence = recurrence
    self.replays = 0  # replays of the recurrence this space has paid for

  @property
  def num_steps(self):
    return int(self._device[0].shape[1])

  @property
  def num_vectors(self):
    return int(self._device[0].shape[0])

  def _combine(self, coef):
    coef = torch.from_numpy(np.ascontiguousarray(coef.astype(np.complex64)))
    eng = thermal._engine_for(self.operators, self.qubits)  # pylint: disable=protected-access
    try:
      _, beta, lengths, _ = self._device
      out = eng.krylov_replay(self.starts, beta, lengths, self.recurrence, coef, self.operator_weights)
      torch.cuda.current_stream(eng.device).synchronize()  # (the engine's workspace goes with it)
    finally:
      eng.close()
    self.replays += 1
    return out


def _starts(eng, n, states, num_vectors, seed):
  if states is not None:
    return thermal._check_states(states, n)  # pylint: disable=protected-access
  count = thermal.DEFAULT_VECTORS if num_vectors is None else int(num_vectors)
  if count < 1:
    raise ValueError("num_vectors must be positive")
  return _engine.random_states(count, n, 0 if seed is None else seed, device=eng.device)


def _radius(operators, qubits, weights):
  sums = [sum(abs(float(np.float32(c))) for c, _, _ in op.masks(qubits)) for op in operators]
  weights = [1.0] * len(sums) if weights is None else weights
  return float(sum(abs(float(w)) * s for w, s in zip(weights, sums)))


def _reorthogonalise(reorthogonalise, store_basis):
  """None: full with a stored basis, local without one; full reorthogonalisation needs the stored basis."""
  if reorthogonalise is None:
    return bool(store_basis)
  if reorthogonalise and not store_basis:
    raise ValueError("store_basis=False runs the local recurrence: full reorthogonalisation (reorthogonalise=True) needs "
                     "the stored basis")
  return bool(reorthogonalise)


def krylov_space(operators, states=None, num_steps=DEFAULT_STEPS, num_vectors=None, seed=None, weights=None, qubits=None,
                 reorthogonalise=None, store_basis=True):
  """The `KrylovSpace` of H = sum_k weights[k] operators[k] from `states` [M, 2^n], or (states=None) from `num_vectors`
  (default 16) random-sign vectors of the engine's generator under `seed` (default 0): the vectors `thermal_ensemble`
  draws for the same seed.  `reorthogonalise`: full (two rounds of classical Gram-Schmidt against every stored vector) or
  local (the three-term recurrence); None: full with a stored basis, local without.  `store_basis=False`: a
  `StreamedKrylovSpace` -- no basis in memory, vectors by a replay of the recurrence (local only)."""
  reorthogonalise = _reorthogonalise(reorthogonalise, store_basis)
  operators = thermal._operator_list(operators)  # pylint: disable=protected-access
  qubits = thermal._qubits_of(operators, qubits)  # pylint: disable=protected-access
  eng = thermal._engine_for(operators, qubits)  # pylint: disable=protected-access
  starts = _starts(eng, len(qubits), states, num_vectors, seed)
  if not store_basis:
    alpha, beta, lengths, recurrence, norms = eng.krylov_tridiagonal(starts, int(num_steps), weights)
    torch.cuda.current_stream(eng.device).synchronize()  # (the engine's workspace goes with it)
    eng.close()
    starts = torch.as_tensor(starts).to(device=alpha.device, dtype=torch.complex64)
    return StreamedKrylovSpace(operators, None if weights is None else [float(w) for w in weights], qubits, starts, alpha, beta,
                               lengths, recurrence, norms, _radius(operators, qubits, weights))
  basis, alpha, beta, lengths, norms = eng.krylov_basis(starts, int(num_steps), weights, reorthogonalise)
  torch.cuda.current_stream(eng.device).synchronize()  # (the engine's workspace goes with it)
  eng.close()
  return KrylovSpace(operators, None if weights is None else [float(w) for w in weights], qubits, basis, alpha, beta, lengths,
                     norms, _radius(operators, qubits, weights))


class ThermalSweep:
  """log Z, <H> and S on a ladder of inverse temperatures from ONE Krylov space per start vector (finite-temperature
  Lanczos), and the `ThermalEnsemble` of any rung."""

  def __init__(self, space, betas, start):
    self.space = space
    self.betas = np.asarray(betas, np.float64).reshape(-1)
    self.start = start
    self.log_weights = ftlm_log_weights(space.ritz(), space.norms, self.betas)  # [B, M]

  def log_partition(self):
    """float64 [B], by the rule of `ThermalEnsemble.log_partition`."""
    return ftlm_log_partition(self.log_weights, self.space.num_qubits, self.start)

  def energy(self):
    """float64 [B]: <H>(beta)."""
    return ftlm_energy(self.space.ritz(), self.space.norms, self.betas)

  def entropy(self):
    """float64 [B]: S = beta <H> + log Z."""
    return self.betas * self.energy() + self.log_partition()

  def ensemble(self, beta):
    """The `ThermalEnsemble` at `beta` (any beta >= 0, on the ladder or not): states e^{-beta H / 2} r_m normalised from the
    stored basis, log weights l_m(beta) from T."""
    states, _ = self.space.evolve(0.5 * float(beta), 0)
    log_weights = torch.from_numpy(ftlm_log_weights(self.space.ritz(), self.space.norms, [float(beta)])[0]).to(states.device)
    return thermal.ThermalEnsemble(self.space.operators, self.space.operator_weights, self.space.qubits, beta, states,
                                   log_weights, self.start)


def thermal_sweep(operators, betas, num_vectors=None, num_steps=DEFAULT_STEPS, seed=None, start="random", qubits=None,
                  weights=None, reorthogonalise=None, store_basis=True):
  """The `ThermalSweep` of H = sum_k weights[k] operators[k] over `betas`.  start="random": `num_vectors` (default 16)
  random-sign vectors, the ones `thermal_ensemble` draws for the same `seed`; start="basis": all 2^n basis states (exact
  once the spaces are exhausted, at most 14 qubits).  `store_basis=False`: log Z, <H> and S from pass one alone, no basis in
  memory; `ensemble(beta)` then costs one replay."""
  _reorthogonalise(reorthogonalise, store_basis)
  operators = thermal._operator_list(operators)  # pylint: disable=protected-access
  qubits = thermal._qubits_of(operators, qubits)  # pylint: disable=protected-access
  betas = np.asarray(betas, np.float64).reshape(-1)
  if not np.isfinite(betas).all() or (betas < 0).any():
    raise ValueError("betas must be finite and >= 0")
  n = len(qubits)
  states = None
  if start == "basis":
    if n > thermal.MAX_BASIS_QUBITS:
      raise ValueError(f"start='basis' holds 2^n states of 2^n amplitudes: refused above {thermal.MAX_BASIS_QUBITS} qubits (got {n})")
    if num_vectors is not None and num_vectors != (1 << n):
      raise ValueError(f"start='basis' has 2^n = {1 << n} vectors")
    states = torch.eye(1 << n, dtype=torch.complex64)
  elif start != "random":
    raise ValueError(f"start must be 'random' or 'basis', got {start!r}")
  space = krylov_space(operators, states, min(int(num_steps), 1 << n) if start == "basis" else num_steps, num_vectors, seed,
                       weights, qubits, reorthogonalise, store_basis)
  return ThermalSweep(space, betas, start)


def ground_state(operators, num_steps=24, max_restarts=8, tolerance=2.0**-20, state=None, seed=None, weights=None, qubits=None,
                 reorthogonalise=None, store_basis=True):
  """(E_0 float64, state [2^n] complex64 on the device, residual, restarts): the lowest Ritz pair of a space of
  `num_steps`, restarted from its Ritz vector until residual = ||H y - theta y|| <= tolerance R or `max_restarts` restarts
  are spent.  Starts from `state` or from a random-sign vector under `seed`.  `store_basis=False`: one pass and one replay
  per restart, three vectors in memory."""
  _reorthogonalise(reorthogonalise, store_basis)
  operators = thermal._operator_list(operators)  # pylint: disable=protected-access
  qubits = thermal._qubits_of(operators, qubits)  # pylint: disable=protected-access
  current = None if state is None else torch.as_tensor(state).reshape(1, -1)
  restarts = 0
  while True:
    space = krylov_space(operators, current, num_steps, 1, seed, weights, qubits, reorthogonalise, store_basis)
    theta, _ = space.ritz()[0]
    if len(theta) == 0:
      raise ValueError("the start state has norm 0")
    residual = float(space.residuals()[0][0])
    current = space.ritz_states([0])[:, 0]
    if residual <= tolerance * space.radius or restarts >= int(max_restarts):
      return float(theta[0]), current[0], residual, restarts
    restarts += 1


def spectrum_extremes(operators, num_steps=DEFAULT_STEPS, seed=None, weights=None, qubits=None, state=None, reorthogonalise=None,
                      store_basis=True):
  """((theta_min, residual), (theta_max, residual)) of one Krylov space from `state` (default: a random-sign vector):
  Ritz values lie inside [E_min, E_max] and converge to its ends first.  `store_basis=False`: pass one alone, no replay."""
  _reorthogonalise(reorthogonalise, store_basis)
  space = krylov_space(operators, None if state is None else torch.as_tensor(state).reshape(1, -1), num_steps, 1, seed, weights,
                       qubits, reorthogonalise, store_basis)
  theta, _ = space.ritz()[0]
  if len(theta) == 0:
    raise ValueError("the start state has norm 0")
  res = space.residuals()[0]
  return (float(theta[0]), float(res[0])), (float(theta[-1]), float(res[-1]))
