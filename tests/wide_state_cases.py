"""The cases tests/test_wide_states_cpu.py and tests/test_wide_states_gpu.py share: the state-sweep features (state import,
`apply_observables`, Chebyshev evolution, the Lanczos basis, streamed Lanczos, the from-states circuit calls and the cotangent
import of the final-state VJP) at n = 20, the smallest width at which a state has more than 256 partials (512 slices of 1024
words) and the second-level sums (`sweep_row_sum`, `sweep_row_sum2` of csrc/state_sweep.h) take a second trip.  Every case
builder takes n (even), so that tests/test_wide_states_cpu.py can hold the same builders to the dense route at n = 12; every
restatement run is computed once per case (`functools.lru_cache`) and never written.

H       two observables, weights [1.0, -0.5], 8 Pauli strings chosen by the class of index bit they flip or sign (qubit q is
        index bit n - 1 - q): X on bit 0 (the partner inside a 16-byte word), on bit 10 (inside a slice of 2048 amplitudes), on
        bit 14 (across slices), on bit n - 1 (across the halves of the state), a two-flip string (bits 3 and 16), a string with
        one Y (bit 12, with Z on bit 0), one with two (bits 0 and n - 1) and a Z string on bits 0, 9 and n - 1.  The coefficients are multiples of 2^-4, the same numbers in float32 and float64;
        R = 4.0625.
        Bits 9 and 10 are the circuit's middle qubits, so every qubit the circuit acts on is measured.
states  real and imaginary parts +-2^-(n/2) with seeded signs, rows scaled by 1, 2 and 2^-3: every partial sum of |phi|^2 is a
        multiple of 2^-(n+6) below 2^3, exact in float64 in any order, and the squared norms are exactly 2, 8 and 2^-5.
circuit 8 gates over 4 parameters on qubits 0, n/2 - 1, n/2 and n - 1, one of them between qubit 0 and qubit n - 1, four in
        rotation form (global_shift -0.5); the circuit's states have parts +-1, norm^2 = 2^(n+1).

Bars (MARGIN = 8, the factor of tests/test_thermal_gpu.py and tests/krylov_cases.py: the kernels add their terms in another
order than the restatement).  The figures are measured on the CPU at n = 20; tests/test_wide_states_cpu.py recomputes them
and asserts that they lie within x / : 2.5 of these:
  evolution   fp32 restatement (`thermal_ref.evolve(dtype=float32)`) against its float64 run, the larger of imaginary and real
              time at TAU_ONE (real time per unit norm): states 3.2e-10, log norms 5.4e-8.  The two-step case (TAU_TWO,
              imaginary time) has no fp32 run of its own -- it would cost the CPU tests another 25 s -- and uses these bars
  Lanczos     fp32 restatement (`krylov_ref.lanczos(dtype=float32)`) against its float64 run, m = 4, the larger of the two
              modes: alpha 4.3e-8, beta 2.2e-8, basis 1.0e-9; |V^dagger V - I| of the fp32 run in full mode 3.4e-8
"""
import functools

import numpy as np

from oracle import qhbm_oracle as O
from tests import final_states_ref as F
from tests import from_states_ref as R
from tests import krylov_ref as K
from tests import thermal_ref as T

N = 20
WEIGHTS = [1.0, -0.5]
SCALES = (1.0, 2.0, 2.0**-3)
NORM2 = (2.0, 8.0, 2.0**-5)
MARGIN = 8.0
KRYLOV_STEPS = 4
TAU_ONE, TAU_TWO = 0.125, 1.0   # one Chebyshev step of at most 12 terms; two steps (imaginary time only)
SEED = 2020

# the fp32 restatement's errors at n = 20 (module docstring)
DOCUMENTED = dict(states=3.2e-10, log_norms=5.4e-8, alpha=4.3e-8, beta=2.2e-8, basis=1.0e-9, gram=3.4e-8)


# ---- H ------------------------------------------------------------------------------------------------------------------------
def _term(n, coeff, paulis):
  """One Pauli string from {index bit: 'X' | 'Y' | 'Z'}, the bits named as at n = 20: bit 19 is n - 1 at every width, the
  others fold modulo n - 1, which keeps the 8 strings distinct at n = 12."""
  return O.pauli_term(coeff, {n - 1 - (n - 1 if bit == 19 else bit % (n - 1)): p for bit, p in paulis.items()})


def hamiltonian(n):
  """The two observables of the module docstring; at n = 20 the index bits are the ones named there, bit 19 standing for
  n - 1 at every width."""
  top = 19
  first = [_term(n, 0.75, {0: "X"}), _term(n, -0.625, {10: "X"}), _term(n, 0.5, {14: "X"}), _term(n, 0.6875, {top: "X"})]
  second = [_term(n, 0.875, {3: "X", 16: "X"}), _term(n, -0.375, {12: "Y", 0: "Z"}), _term(n, 0.625, {0: "Y", top: "Y"}),
            _term(n, 1.125, {0: "Z", 9: "Z", top: "Z"})]
  return [first, second]


def diagonal_part(n):
  """The terms of H that flip nothing, as one observable."""
  return [[t for op in hamiltonian(n) for t in op if t[1] == 0]]


def num_terms(n):
  return sum(len(op) for op in hamiltonian(n))


# ---- states -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def starts(n):
  """complex64 [3, 2^n]: parts +-2^-(n/2) with seeded signs, rows scaled by 1, 2 and 2^-3."""
  assert n % 2 == 0
  rng = np.random.default_rng(SEED + n)
  signs = 1.0 - 2.0 * rng.integers(0, 2, size=(3, 1 << n, 2))
  out = ((signs[..., 0] + 1j * signs[..., 1]) * 2.0**-(n // 2) * np.array(SCALES)[:, None]).astype(np.complex64)
  out.setflags(write=False)
  return out


def starts_with_zero_row(n):
  out = starts(n).copy()
  out[1] = 0
  return out


BASIS_INDEX = 0b10000000010000000101  # index bits 0, 2, 10 and 19


def basis_start(n):
  out = np.zeros((1, 1 << n), np.complex64)
  out[0, BASIS_INDEX & ((1 << n) - 1)] = 1
  return out


# ---- apply_observables --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def applied(n):
  """H phi of the three start states and of the basis state, complex128 [4, 2^n]."""
  given = np.concatenate([starts(n), basis_start(n)]).astype(np.complex128)
  return T.apply_h(n, hamiltonian(n), given, WEIGHTS)


# ---- evolution ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def evolved(n, tau, mode, single=False, tail=None):
  """(states, log norms or None) of `thermal_ref.evolve` on the start states; `single`: the fp32 arithmetic; `tail`: where
  the series is cut (default: where the engine cuts it)."""
  return T.evolve(n, hamiltonian(n), starts(n), tau, mode, WEIGHTS, dtype=np.float32 if single else np.float64, tail=tail)


@functools.lru_cache(maxsize=None)
def evolution_errors(n):
  """(states, log norms): the fp32 restatement against its float64 run at TAU_ONE, the larger of imaginary time (normalised
  states) and real time (per unit norm of the state as given)."""
  s64, l64 = evolved(n, TAU_ONE, 0)
  s32, l32 = evolved(n, TAU_ONE, 0, True)
  norms = np.sqrt(np.array(NORM2))[:, None]
  real = float((np.abs(evolved(n, TAU_ONE, 1, True)[0] - evolved(n, TAU_ONE, 1)[0]) / norms).max())
  errors = max(float(np.abs(s32 - s64).max()), real), float(np.abs(l32 - l64).max())
  print(f"n={n} fp32 restatement of the evolution against float64: states {errors[0]:.3e} log norms {errors[1]:.3e}")
  return errors


def evolution_bars(n):
  state_err, log_err = evolution_errors(n)
  return MARGIN * state_err, MARGIN * log_err


# ---- Lanczos ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lanczos(n, reorth, single=False):
  """(basis, alpha, beta, lengths, norms, raw ||w|| [m, U]) of `krylov_ref.lanczos`, m = KRYLOV_STEPS."""
  raw = []
  out = K.lanczos(n, hamiltonian(n), starts(n), KRYLOV_STEPS, WEIGHTS, reorth, np.float32 if single else np.float64, raw)
  return out + (np.stack(raw),)


@functools.lru_cache(maxsize=None)
def lanczos_errors(n):
  """dict(alpha, beta, basis, gram): |fp32 - float64| of the restatement, the larger of the two modes; gram: |V^dagger V - I|
  of the fp32 run in full mode."""
  out = dict(alpha=0.0, beta=0.0, basis=0.0)
  for reorth in (True, False):
    a, b = lanczos(n, reorth, True), lanczos(n, reorth)
    assert np.array_equal(a[3], b[3])
    for key, i in (("alpha", 1), ("beta", 2), ("basis", 0)):
      out[key] = max(out[key], float(np.abs(a[i] - b[i]).max()))
  basis = lanczos(n, True, True)[0]
  out["gram"] = max(float(np.abs(gram(basis[:, u]) - np.eye(KRYLOV_STEPS)).max()) for u in range(basis.shape[1]))
  print(f"n={n} fp32 restatement of the Lanczos run against float64: {out}")
  return out


def gram(rows):
  v = np.asarray(rows).astype(np.complex128)
  return v.conj() @ v.T


def lanczos_bars(n):
  return {key: MARGIN * value for key, value in lanczos_errors(n).items()}


# ---- circuits from wide states ------------------------------------------------------------------------------------------------
def circuit(n):
  """(gates, n_params): 8 gates over 4 parameters on qubits 0, n/2 - 1, n/2 and n - 1; four in rotation form."""
  lo, mid, mid2, hi = 0, n // 2 - 1, n // 2, n - 1
  gates = [(O.GATE_XPOW, lo, -1, 0, 1.0, 0.0, -0.5),
           (O.GATE_ZPOW, hi, -1, 1, 1.0, 0.0, -0.5),
           (O.GATE_XPOW, mid, -1, 2, 1.0, 0.0),
           (O.GATE_YPOW, mid2, -1, 3, 1.0, 0.0),
           (O.GATE_CZPOW, lo, hi, 1, 0.5, 0.25),
           (O.GATE_CZPOW, mid, mid2, 2, -1.0, 0.3),
           (O.GATE_XPOW, hi, -1, 3, 0.7, 0.1, -0.5),
           (O.GATE_ZPOW, mid2, -1, 0, 1.0, -0.2, -0.5)]
  return gates, 4


PARAMS = np.array([0.37, -0.81, 0.55, 0.23])
COTANGENT_SCALES = np.array([1.0, -0.5, 0.75])


@functools.lru_cache(maxsize=None)
def circuit_states(n):
  """complex64 [3, 2^n] with parts +-1: norm^2 = 2^(n+1) exactly."""
  rng = np.random.default_rng(SEED + 100 + n)
  signs = 1.0 - 2.0 * rng.integers(0, 2, size=(3, 1 << n, 2))
  out = (signs[..., 0] + 1j * signs[..., 1]).astype(np.complex64)
  out.setflags(write=False)
  return out


def circuit_upstream(n):
  return np.random.default_rng(SEED + 200 + n).normal(size=(3, 2))


@functools.lru_cache(maxsize=None)
def circuit_reference(n):
  """(values [3, 2], gradient [4], final states [3, 2^n]) of tests/from_states_ref.py for H's two observables."""
  gates, _ = circuit(n)
  given = circuit_states(n).astype(np.complex128)
  vals, rows = R.values_and_rows(n, gates, PARAMS, given, hamiltonian(n), circuit_upstream(n))
  return vals, rows.sum(0), R.final_states(n, gates, PARAMS, given)


@functools.lru_cache(maxsize=None)
def cotangent(n):
  """complex64 [3, 2^n]: g_u = i c_u psi_u + a seeded Gaussian part, so that Im<g_u|psi_u> = -c_u ||psi_u||^2 up to the
  Gaussian part's sqrt(2^n) -- the phase term of the gradient is of the order of the gradient."""
  finals = circuit_reference(n)[2]
  rng = np.random.default_rng(SEED + 300 + n)
  noise = rng.normal(size=finals.shape) + 1j * rng.normal(size=finals.shape)
  out = (1j * COTANGENT_SCALES[:, None] * finals + noise).astype(np.complex64)
  out.setflags(write=False)
  return out


@functools.lru_cache(maxsize=None)
def cotangent_reference(n):
  """(gradient [4], phase term [4]) of tests/final_states_ref.py for `cotangent` as the engine is given it (complex64)."""
  gates, n_params = circuit(n)
  given, cot = circuit_states(n).astype(np.complex128), cotangent(n).astype(np.complex128)
  return F.vjp(n, gates, PARAMS, given, cot), F.phase_term(gates, n_params, circuit_reference(n)[2], cot)
