"""float64 / complex128 restatement of the engine's matrix-free thermal targets (include/qhbm_engine.h
qhbm_evolve_states, qhbm_apply_observables, qhbm_random_states), for the tests.  The product never imports it.

An operator is a list of (coeff, x_mask, z_mask) in qubit space (bit q = qubit q, qubit 0 = the most significant index
bit), as `Engine.set_observables` takes it.  H = sum_k w_k O_k, R = sum_k |w_k| sum_j |c_kj| >= ||H||, H~ = H / R.

  imaginary time  e^{-d H} = e^{d R} [a_0 T_0 + 2 sum_{k>=1} (-1)^k a_k T_k(H~)],  a_k = e^{-x} I_k(x),  x = d R
  real time       e^{-i d H} = J_0(x) T_0 + 2 sum_{k>=1} (-i)^k J_k(x) T_k(H~)
  t_0 = phi, t_1 = H~ t_0, t_{k+1} = 2 H~ t_k - t_{k-1}

tau is split into m = ceil(|tau| R / 4) equal steps; in imaginary time the state is renormalised after every step and
log ||.|| accumulates, the factor e^{d R} entering it as + x.  `dtype=np.float32` runs the same arithmetic with complex64
states and float32 operator coefficients (log norms stay float64, as on the device): the rounding an fp32 implementation
of the algorithm has, which the GPU tests' tolerance is derived from."""
import math

import numpy as np

from oracle.sampling import philox4x32_10

STEP_ARGUMENT = 4.0
TAIL = 2.0**-30          # the engine cuts a step's series where the discarded tail 2 sum |a_k| falls below this
SERIES_EXACT = 2.0**-60  # a cut below float64 rounding: the stepwise algorithm without its truncation error
RANDOM_STATES_TAG = 0x54505153


# ---- H from masks -------------------------------------------------------------------------------------------------------------
def index_masks(n, op):
  """[(coeff, x, z, ny)] with the masks in amplitude-index space (qubit q = index bit n - 1 - q)."""
  out = []
  for coeff, x, z in op:
    xi = sum(1 << (n - 1 - q) for q in range(n) if x >> q & 1)
    zi = sum(1 << (n - 1 - q) for q in range(n) if z >> q & 1)
    out.append((float(np.float32(coeff)), xi, zi, bin(x & z).count("1")))
  return out


def _parity(v):
  v = v.copy()
  for s in (32, 16, 8, 4, 2, 1):
    v ^= v >> s
  return v & 1


def radius(n, ops, weights=None):
  """R = sum_k |w_k| sum_j |c_kj| (coefficients as the engine holds them: float32)."""
  weights = np.ones(len(ops)) if weights is None else np.asarray(weights, np.float64)
  return float(sum(abs(w) * sum(abs(float(np.float32(c))) for c, _, _ in op) for w, op in zip(weights, ops)))


def apply_h(n, ops, states, weights=None, dtype=np.float64):
  """H phi for states [..., 2^n], matrix-free: (P phi)[j] = i^ny (-1)^{popc((j ^ x) & z)} phi[j ^ x]."""
  cdtype = np.complex64 if dtype == np.float32 else np.complex128
  states = np.asarray(states, cdtype)
  weights = np.ones(len(ops)) if weights is None else np.asarray(weights, np.float64)
  j = np.arange(1 << n, dtype=np.int64)
  out = np.zeros_like(states)
  for w, op in zip(weights, ops):
    for coeff, x, z, ny in index_masks(n, op):
      sign = 1.0 - 2.0 * _parity((j ^ x) & z)
      factor = (dtype(w * coeff) * (1j**ny)) * sign
      out = out + factor.astype(cdtype) * states[..., j ^ x]
  return out


def dense_h(n, ops, weights=None):
  """The 2^n x 2^n matrix of H, term by term from Kronecker products (independent of `apply_h`)."""
  paulis = {0: np.eye(2), 1: np.array([[0, 1], [1, 0]]), 2: np.array([[1, 0], [0, -1]]), 3: np.array([[0, -1j], [1j, 0]])}
  weights = np.ones(len(ops)) if weights is None else np.asarray(weights, np.float64)
  h = np.zeros((1 << n, 1 << n), np.complex128)
  for w, op in zip(weights, ops):
    for coeff, x, z in op:
      m = np.ones((1, 1), np.complex128)
      for q in range(n):
        m = np.kron(m, paulis[(x >> q & 1) | (z >> q & 1) << 1])
      h += w * float(np.float32(coeff)) * m
  return h


# ---- coefficients -------------------------------------------------------------------------------------------------------------
def bessel_sequence(x, mode):
  """e^{-x} I_k(x) (mode 0) or J_k(x) (mode 1) for k = 0 .. N by Miller's backward recurrence, normalised with
  a_0 + 2 sum a_k = 1 or J_0 + 2 sum J_2k = 1."""
  top = 2 * int(math.ceil(x)) + 64
  f = np.zeros(top + 2)
  f[top] = 1.0
  for k in range(top, 0, -1):
    f[k - 1] = (2.0 * k / x) * f[k] + (f[k + 1] if mode == 0 else -f[k + 1])
    if abs(f[k - 1]) > 1e250:
      f[k - 1:] *= 1e-250
  norm = f[0] + 2.0 * (f[1:].sum() if mode == 0 else f[2::2].sum())
  return (f / norm)[:top + 1]


def step_coefficients(x, mode, sign=1.0, tail=None):
  """c_0 .. c_K with sum_k c_k T_k(H~) = e^{-x H~} e^{-x} ... (mode 0: without the factor e^{x}) or e^{-i sign x H~}
  (mode 1), cut where the discarded tail 2 sum |a_k| falls below `tail` (default 2^-30, the engine's cut); K >= 1."""
  a = bessel_sequence(x, mode)
  cut = TAIL if tail is None else tail
  k_top, dropped = len(a) - 1, 0.0
  while k_top > 1 and dropped + 2.0 * abs(a[k_top]) < cut:
    dropped += 2.0 * abs(a[k_top])
    k_top -= 1
  k = np.arange(k_top + 1)
  base = np.where(k == 0, 1.0, 2.0) * a[:k_top + 1]
  if mode == 0:
    return (base * (-1.0)**k).astype(np.complex128)
  return base * (-1j * sign)**k


def evolution_plan(n, ops, tau, mode, weights=None, step_argument=STEP_ARGUMENT, tail=None):
  """dict(R, steps, terms_per_step, applications, x): what `Engine.describe_evolution` reports."""
  r = radius(n, ops, weights)
  steps = int(math.ceil(abs(tau) * r / step_argument))
  x = abs(tau) * r / steps if steps else 0.0
  terms = len(step_coefficients(x, mode, 1.0, tail)) - 1 if steps else 0
  return dict(R=r, steps=steps, terms_per_step=terms, applications=steps * terms, x=x)


# ---- the stepwise algorithm -----------------------------------------------------------------------------------------------------
def evolve(n, ops, states, tau, mode=0, weights=None, dtype=np.float64, step_argument=STEP_ARGUMENT, tail=None):
  """(states, log_norms) as `Engine.evolve_states`: mode 0 returns e^{-tau H} phi normalised and log ||e^{-tau H} phi||
  of the states as given; mode 1 returns e^{-i tau H} phi and None.  `tail`: where the series is cut (default: the
  engine's 2^-30, an error the engine's fp32 amplitudes cannot see; SERIES_EXACT sums the series to float64 precision)."""
  cdtype = np.complex64 if dtype == np.float32 else np.complex128
  states = np.array(states, dtype=cdtype)
  plan = evolution_plan(n, ops, tau, mode, weights, step_argument, tail)
  norms = np.linalg.norm(states.astype(np.complex128), axis=-1)
  with np.errstate(divide="ignore"):
    log_norms = np.log(norms)
  if plan["R"] == 0.0 or (plan["steps"] == 0 and mode == 1):
    return states, (log_norms if mode == 0 else None)
  scale = np.where(norms > 0, 1.0 / np.where(norms > 0, norms, 1.0), 0.0)
  acc = (states * scale[..., None]).astype(cdtype)
  scaled = np.ones(len(ops)) if weights is None else np.asarray(weights, np.float64)
  scaled = scaled / plan["R"]
  coef = step_coefficients(plan["x"], mode, 1.0 if tau >= 0 else -1.0, tail).astype(cdtype) if plan["steps"] else None
  for _ in range(plan["steps"]):
    t_prev = acc
    t_cur = apply_h(n, ops, t_prev, scaled, dtype)
    acc = coef[0] * t_prev + coef[1] * t_cur
    for k in range(2, len(coef)):
      t_next = (2.0 * apply_h(n, ops, t_cur, scaled, dtype) - t_prev).astype(cdtype)
      acc = (acc + coef[k] * t_next).astype(cdtype)
      t_prev, t_cur = t_cur, t_next
    if mode == 0:
      step_norm = np.linalg.norm(acc.astype(np.complex128), axis=-1)
      with np.errstate(divide="ignore"):
        log_norms = log_norms + np.log(step_norm) + plan["x"]
      inv = np.where(step_norm > 0, 1.0 / np.where(step_norm > 0, step_norm, 1.0), 0.0)
      acc = (acc * inv[..., None]).astype(cdtype)
  if mode == 0:
    return acc, log_norms
  return (acc * norms[..., None]).astype(cdtype), None


# ---- random states ----------------------------------------------------------------------------------------------------------------
def random_state_magnitude(n):
  """float32(2^{-(n + 1) / 2}) from exact powers of two and one correctly rounded square root."""
  return np.float32(math.ldexp(math.sqrt(0.5) if (n + 1) % 2 else 1.0, -((n + 1) // 2)))


def random_states(num, n, seed, first_state=0):
  """complex64 [num, 2^n]: the states `qhbm_random_states` writes, bit for bit."""
  seed = int(seed) & (2**64 - 1)
  key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
  j = np.arange(1 << n, dtype=np.uint64)
  g = j >> np.uint64(6)
  groups = np.unique(g)
  out = np.empty((num, 1 << n), np.complex64)
  mag = random_state_magnitude(n)
  bit = (np.uint64(2) * (j & np.uint64(63))).astype(np.int64)
  for m in range(num):
    counter = np.zeros((len(groups), 4), np.uint64)
    counter[:, 0] = groups & np.uint64(0xFFFFFFFF)
    counter[:, 1] = groups >> np.uint64(32)
    counter[:, 2] = (first_state + m) & 0xFFFFFFFF
    counter[:, 3] = RANDOM_STATES_TAG
    words = philox4x32_10(counter, key).astype(np.uint64)[g.astype(np.int64)]  # [2^n, 4]
    word = words[np.arange(1 << n), bit >> 5]
    re_neg = (word >> (bit & 31).astype(np.uint64)) & np.uint64(1)
    im_neg = (word >> ((bit & 31) + 1).astype(np.uint64)) & np.uint64(1)
    out[m] = (np.where(re_neg == 1, -mag, mag) + 1j * np.where(im_neg == 1, -mag, mag)).astype(np.complex64)
  return out


def basis_states(n, dtype=np.complex128):
  return np.eye(1 << n, dtype=dtype)


# ---- estimators -------------------------------------------------------------------------------------------------------------------
def logsumexp(v):
  v = np.asarray(v, np.float64)
  top = v.max()
  return float(top + np.log(np.exp(v - top).sum())) if np.isfinite(top) else float(top)


def log_partition(log_weights, n, start):
  """log Z from l_m = 2 log ||e^{-beta H / 2} r_m||: n log 2 + logsumexp(l) - log M (random), logsumexp(l) (basis)."""
  if start == "basis":
    return logsumexp(log_weights)
  return n * math.log(2.0) + logsumexp(log_weights) - math.log(len(log_weights))


def ensemble_weights(log_weights):
  w = np.exp(np.asarray(log_weights, np.float64) - np.max(log_weights))
  return w / w.sum()


def thermal_ensemble(n, ops, beta, start_states, weights=None, dtype=np.float64, tail=None):
  """(states, log_weights) = (e^{-beta H / 2} r_m normalised, 2 log ||e^{-beta H / 2} r_m||)."""
  states, log_norms = evolve(n, ops, start_states, 0.5 * beta, 0, weights, dtype, tail=tail)
  return states, 2.0 * log_norms


def energy(n, ops, states, log_weights, weights=None):
  """<H> = sum_m w_m <phi_m| H |phi_m>, w = softmax(l)."""
  states = np.asarray(states, np.complex128)
  per_state = np.real(np.sum(states.conj() * apply_h(n, ops, states, weights), axis=-1))
  return float(ensemble_weights(log_weights) @ per_state), per_state


def typicality_standard_errors(n, ops, states, log_weights, weights=None):
  """Standard errors of the estimates of log Z and <H> from the spread of the l_m over the M random vectors
  (delta method on Z^ = mean(z_m), z_m = e^{l_m}, and on the ratio mean(z_m e_m) / mean(z_m))."""
  lw = np.asarray(log_weights, np.float64)
  z = np.exp(lw - lw.max())
  m = len(z)
  mean_energy, per_state = energy(n, ops, states, lw, weights)
  se_log_z = float(np.std(z, ddof=1) / (np.sqrt(m) * z.mean()))
  se_energy = float(np.std(z * (per_state - mean_energy), ddof=1) / (np.sqrt(m) * z.mean()))
  return se_log_z, se_energy


# ---- dense route (n <= 10) --------------------------------------------------------------------------------------------------------
class Dense:
  """eigh of the dense H: exact e^{-tau H} phi, e^{-i tau H} phi, log Z, <H>, entropy and rho_beta."""

  def __init__(self, n, ops, weights=None):
    if n > 10:
      raise ValueError("the dense route is for n <= 10")
    self.n = n
    self.h = dense_h(n, ops, weights)
    self.evals, self.evecs = np.linalg.eigh(self.h)

  def evolve(self, states, tau, mode=0):
    states = np.asarray(states, np.complex128)
    spectral = states @ self.evecs.conj()  # <v_i|phi_u>
    phase = np.exp(-tau * self.evals) if mode == 0 else np.exp(-1j * tau * self.evals)
    out = (spectral * phase) @ self.evecs.T
    if mode == 1:
      return out, None
    norms = np.linalg.norm(out, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
      return np.where(norms[..., None] > 0, out / np.where(norms > 0, norms, 1.0)[..., None], 0.0), np.log(norms)

  def log_partition(self, beta):
    return logsumexp(-beta * self.evals)

  def probabilities(self, beta):
    return np.exp(-beta * self.evals - self.log_partition(beta))

  def energy(self, beta):
    return float(self.probabilities(beta) @ self.evals)

  def entropy(self, beta):
    return beta * self.energy(beta) + self.log_partition(beta)

  def thermal_state(self, beta):
    return (self.evecs * self.probabilities(beta)) @ self.evecs.conj().T
