"""The cases tests/test_krylov_cpu.py and tests/test_krylov_gpu.py share, each restatement run computed once.

H is the TFIM ring as two observables with weights [1.0, 0.7] (tests/test_thermal_gpu.py's), R = 17 at n = 10.
A BAR is 8 x the error of the fp32 restatement (tests/krylov_ref.py, dtype=float32) on the same case: against the
restatement's float64 run for element-wise rows (alpha, beta, basis), against `eigh` (thermal_ref.Dense) for derived
quantities.  The margin is for another summation order: the kernels add a state's words in a tree, numpy pairwise."""
import functools

import numpy as np

from oracle import qhbm_oracle as O
from tests import krylov_ref as K
from tests import thermal_ref as T

WEIGHTS = [1.0, 0.7]
BETAS = (0.5, 4.0)
TIMES = (1.0, -2.5)
MARGIN = 8.0


def tfim_parts(n):
  op = O.tfim_ring_op(n)
  return [op[:n], op[n:]]


def starts(n):
  """n = 3: all 8 basis states; n = 10: two random-sign states and a basis state (tests/test_thermal_gpu.py `_starts`);
  n = 13: three random-sign states."""
  if n == 3:
    return T.basis_states(n).astype(np.complex64)
  if n == 13:
    return T.random_states(3, n, 21)
  return np.concatenate([T.random_states(2, n, 21), T.basis_states(n)[[5]].astype(np.complex64)])


BASIS_CASES = ((3, 8), (10, 12), (13, 8))  # (n, m) of the element-wise comparison


@functools.lru_cache(maxsize=None)
def run(n, m, reorth, single):
  """(basis, alpha, beta, lengths, norms, raw ||w|| [m, U]) of the restatement; `single`: the fp32 arithmetic."""
  raw = []
  out = K.lanczos(n, tfim_parts(n), starts(n), m, WEIGHTS, reorth, np.float32 if single else np.float64, raw)
  return out + (np.stack(raw),)


@functools.lru_cache(maxsize=None)
def dense(n):
  return T.Dense(n, tfim_parts(n), WEIGHTS)


@functools.lru_cache(maxsize=None)
def elementwise_errors(n, m, reorth):
  """(alpha, beta, basis): the largest |fp32 - float64| of the restatement on one case."""
  a, b = run(n, m, reorth, True), run(n, m, reorth, False)
  assert np.array_equal(a[3], b[3])
  return tuple(float(np.abs(a[i] - b[i]).max()) for i in (1, 2, 0))


@functools.lru_cache(maxsize=None)
def derived_errors(reorth):
  """The fp32 restatement at n = 10, m = 48 against `eigh`: dict of the largest errors of theta_min, theta_max, the ground
  vector (phase aligned, amplitudes), evolve(beta, 0) states and log norms, evolve(t, 1) states, |V^dagger V - I|."""
  n, m = 10, 48
  r = run(n, m, reorth, True)
  d = dense(n)
  given = starts(n).astype(np.complex128)
  lo, hi, vecs = K.ground(*r[:4])
  out = {"theta_min": float(np.abs(lo - d.evals[0]).max()), "theta_max": float(np.abs(hi - d.evals[-1]).max()),
         "ground": max(float(np.abs(K.align(v, d.evecs[:, 0]) - d.evecs[:, 0]).max()) for v in vecs)}
  state_err, log_err, real_err = 0.0, 0.0, 0.0
  for beta in BETAS:
    want, want_log = d.evolve(given, beta, 0)
    got, got_log = K.evolve(*r[:5], beta, 0)
    state_err, log_err = max(state_err, float(np.abs(got - want).max())), max(log_err, float(np.abs(got_log - want_log).max()))
  for t in TIMES:
    real_err = max(real_err, float(np.abs(K.evolve(*r[:5], t, 1)[0] - d.evolve(given, t, 1)[0]).max()))
  out.update(states=state_err, log_norms=log_err, real_time=real_err)
  gram = 0.0
  for u in range(r[0].shape[1]):
    v = r[0][:, u].astype(np.complex128)
    gram = max(gram, float(np.abs(v.conj() @ v.T - np.eye(m)).max()))
  out["gram"] = gram
  return out


# ---- thermal_sweep: finite-temperature Lanczos on the two cases of the GPU test -----------------------------------------------------------
SWEEP_CASES = {"basis": (3, 8), "random": (10, 48)}  # start -> (n, m); random: 4 random-sign vectors of seed 77
SWEEP_SEED, SWEEP_VECTORS = 77, 4


def sweep_starts(start):
  n, _ = SWEEP_CASES[start]
  return T.basis_states(n).astype(np.complex64) if start == "basis" else T.random_states(SWEEP_VECTORS, n, SWEEP_SEED)


@functools.lru_cache(maxsize=None)
def sweep_exact(start):
  """From `eigh`, per beta of BETAS: l_m [B, M] = log <r_m| e^{-beta H} |r_m>, log Z [B] by the rule of the start, <H> [B] =
  sum_m <r_m| H e^{-beta H} |r_m> / sum_m <r_m| e^{-beta H} |r_m> (the estimator itself: exact for the basis start), S [B],
  and the states e^{-beta H / 2} r_m normalised [B, M, 2^n]."""
  n, _ = SWEEP_CASES[start]
  d, given = dense(n), sweep_starts(start).astype(np.complex128)
  overlaps = np.abs(given @ d.evecs.conj())**2  # |<v_i|r_m>|^2
  with np.errstate(divide="ignore"):
    logs = np.log(overlaps)
  lw = np.array([[T.logsumexp(row - beta * d.evals) for row in logs] for beta in BETAS])
  log_z = np.array([T.log_partition(row, n, start) for row in lw])
  energy = np.array([(overlaps * np.exp(-beta * (d.evals - d.evals[0])) * d.evals).sum() / (overlaps * np.exp(-beta * (d.evals - d.evals[0]))).sum()
                     for beta in BETAS])
  states = np.stack([d.evolve(given, 0.5 * beta, 0)[0] for beta in BETAS])
  return lw, log_z, energy, np.array(BETAS) * energy + log_z, states


@functools.lru_cache(maxsize=None)
def sweep_run(start, reorth, single):
  """(l_m [B, M], log Z [B], <H> [B], S [B], ensemble states [B, M, 2^n], ensemble <H> [B]) of the restatement, by the
  product's host functions (`inference.krylov.ftlm_*`) on the restatement's alpha and beta; ensemble <H> = sum_m
  softmax(l)_m <phi_m| H |phi_m> over the restatement's evolve(beta / 2, 0) states."""
  from qhbmlib_amd.inference import krylov  # pylint: disable=import-outside-toplevel
  n, m = SWEEP_CASES[start]
  r = K.lanczos(n, tfim_parts(n), sweep_starts(start), m, WEIGHTS, reorth, np.float32 if single else np.float64)
  pairs = [krylov.ritz(r[1][u], r[2][u], r[3][u]) for u in range(r[0].shape[1])]
  lw = krylov.ftlm_log_weights(pairs, r[4], BETAS)
  log_z = krylov.ftlm_log_partition(lw, n, start)
  energy = krylov.ftlm_energy(pairs, r[4], BETAS)
  states = np.stack([K.evolve(*r, 0.5 * beta, 0)[0] for beta in BETAS])
  ens_energy = np.array([T.energy(n, tfim_parts(n), states[b], lw[b], WEIGHTS)[0] for b in range(len(BETAS))])
  return lw, log_z, energy, np.array(BETAS) * energy + log_z, states, ens_energy


@functools.lru_cache(maxsize=None)
def sweep_errors(start):
  """The fp32 restatement of the sweep against `eigh`, the larger of the two modes and of the betas: dict of the largest
  errors of l_m, log Z, <H>, S, the ensemble's states and the ensemble's <H>."""
  exact = sweep_exact(start)
  out = dict(log_weights=0.0, log_z=0.0, energy=0.0, entropy=0.0, states=0.0, ensemble_energy=0.0)
  for reorth in (True, False):
    got = sweep_run(start, reorth, True)
    for key, a, b in zip(("log_weights", "log_z", "energy", "entropy", "states"), got, exact):
      out[key] = max(out[key], float(np.abs(a - b).max()))
    out["ensemble_energy"] = max(out["ensemble_energy"], float(np.abs(got[5] - exact[2]).max()))
  return out
