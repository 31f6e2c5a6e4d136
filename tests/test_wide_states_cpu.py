"""The conditions tests/test_wide_states_gpu.py rests on, checked without a GPU (cases: tests/wide_state_cases.py).

  * the Hamiltonian has 8 terms and flips or signs an index bit of every class the observable kernels treat differently;
  * the start states' squared norms are exactly 2, 8 and 2^-5 in float64 in any order of summation;
  * the Lanczos case is nowhere near a breakdown (every ||w|| / R of live rows above 0.1; measured 0.37) and the evolution
    case has one step at TAU_ONE and two at TAU_TWO;
  * the fp32 restatements' errors behind the bars are the documented ones (`wide_state_cases.DOCUMENTED`, x / : 2.5);
  * the two shapes added to tests/test_reduced_density_vjp_gpu.py have 512 partials per state and component;
  * the circuit's documented phase slope is non-zero for every parameter, and the cotangent's phase term dominates the bar;
  * at n = 12 the same case builders agree with the dense route within 1e-9: H as a 4096 x 4096 matrix
    (`thermal_ref.dense_h`) applied, exponentiated and run through Lanczos, and the circuit as `oracle.qhbm_oracle.unitary`.
    `thermal_ref.Dense` stops at 10 qubits and an `eigh` of this size takes 20 s, so e^{-tau H} phi and e^{-i tau H} phi are
    Taylor series of dense matrix-vector products, summed until a term is below 2^-60 of the sum.
The n = 20 references take about a minute in all; they are cached per case and shared by the tests of this module, which
therefore run in one worker.  Every comparison prints its figure beside its bar."""
import numpy as np
import pytest

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from tests import final_states_ref as F
from tests import from_states_ref as R
from tests import reduced_density_ref as RD
from tests import thermal_ref as T
from tests import wide_state_cases as W

pytestmark = pytest.mark.xdist_group("wide_states")

N = W.N
SMALL = 12


def _close(what, got, want, bar):
  err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)), initial=0.0))
  print(f"{what}: max error {err:.3e}  bar {bar:.3e}")
  assert np.isfinite(np.asarray(got)).all() and err <= bar, (what, err, bar)


# ---- the cases themselves ---------------------------------------------------------------------------------------------------------
def test_the_hamiltonian_reaches_every_class_of_index_bit():
  ops = W.hamiltonian(N)
  assert len(ops) == len(W.WEIGHTS) == 2 and W.num_terms(N) == 8
  terms = [t for op in ops for t in T.index_masks(N, op)]
  assert all(float(np.float32(c)) == raw for (c, _, _, _), (raw, _, _) in zip(terms, [t for op in ops for t in op]))
  single = [x for _, x, _, _ in terms if bin(x).count("1") == 1]
  assert 1 << 0 in single                                    # the partner inside a 16-byte word
  assert any(1 << b in single for b in range(1, 11))         # inside a slice of 2048 amplitudes
  assert any(1 << b in single for b in range(11, 19))        # across slices
  assert 1 << 19 in single                                   # across the halves of the state
  assert any(bin(x).count("1") == 2 and ny == 0 for _, x, _, ny in terms)
  assert sorted(ny for _, _, _, ny in terms) == [0] * 6 + [1, 2]
  assert any(x == 0 and z & 1 and z >> 19 & 1 for _, x, z, _ in terms)
  assert len({x for _, x, _, _ in terms}) == 8               # eight groups by X mask, the diagonal one among them
  assert T.radius(N, ops, W.WEIGHTS) == 4.0625
  assert len(W.diagonal_part(N)[0]) == 1


def test_the_start_states_have_exact_norms():
  starts = W.starts(N)
  assert starts.dtype == np.complex64 and starts.shape == (3, 1 << N)
  for u, want in enumerate(W.NORM2):
    squares = starts[u].real.astype(np.float64)**2 + starts[u].imag.astype(np.float64)**2
    running = np.cumsum(squares[::-1])
    assert np.sum(squares) == want == np.sum(squares[::-1]) == running[-1]  # (pairwise, pairwise reversed, one by one)
    assert (np.abs(starts[u].real) == 2.0**-10 * W.SCALES[u]).all() and (np.abs(starts[u].imag) == 2.0**-10 * W.SCALES[u]).all()
  zero = W.starts_with_zero_row(N)
  assert (zero[1] == 0).all() and np.array_equal(zero[[0, 2]], starts[[0, 2]])
  assert np.count_nonzero(W.basis_start(N)) == 1 and W.basis_start(N)[0, W.BASIS_INDEX] == 1
  circuit_states = W.circuit_states(N)
  assert (np.abs(circuit_states.real) == 1).all() and (np.abs(circuit_states.imag) == 1).all()


def test_the_evolution_plans_have_one_step_and_two():
  ops = W.hamiltonian(N)
  for mode in (0, 1):
    plan = T.evolution_plan(N, ops, W.TAU_ONE, mode, W.WEIGHTS)
    assert plan["steps"] == 1 and plan["terms_per_step"] <= 12, plan
  assert T.evolution_plan(N, ops, W.TAU_TWO, 0, W.WEIGHTS)["steps"] == 2


def test_the_circuit_has_a_phase_slope_and_the_cotangent_a_phase_term():
  gates, n_params = W.circuit(N)
  assert len(gates) == 8 and n_params == 4
  assert {q for g in gates for q in g[1:3] if q >= 0} == {0, 9, 10, 19} and any(sorted(g[1:3]) == [0, 19] for g in gates)
  assert sum(1 for g in gates if g[3] >= 0 and O.gate_global_shift(g) == -0.5) >= 2
  slope = F.documented_phase_slope(gates, n_params)
  print(f"documented phase slope {slope}")
  assert (np.abs(slope) > 1.0).sum() >= 2
  want, phase = W.cotangent_reference(N)
  bar = 1e-4 * max(1.0, float(np.abs(want).max()))
  print(f"gradient {want}  phase term {phase}  bar {bar:.3e}")
  assert np.abs(phase).min() >= 100.0 * bar
  vals, grad, _ = W.circuit_reference(N)
  assert (np.abs(grad) > 1.0).all() and (np.abs(vals) > 1.0).all()  # (every parameter is felt by the measured qubits)


# ---- the bars ---------------------------------------------------------------------------------------------------------------------
def _documented(name, got):
  want = W.DOCUMENTED[name]
  print(f"{name}: fp32 restatement off by {got:.3e}  documented {want:.3e}")
  assert want / 2.5 < got < 2.5 * want, (name, got, want)


def test_the_lanczos_case_is_far_from_a_breakdown_and_its_bars_are_the_documented_ones():
  radius = T.radius(N, W.hamiltonian(N), W.WEIGHTS)
  for reorth in (True, False):
    for single in (False, True):
      run = W.lanczos(N, reorth, single)
      raw = run[5] / radius
      print(f"reorth={reorth} fp32={single}: lengths {run[3]}  smallest ||w|| / R {raw.min():.3f}")
      assert run[3].tolist() == [W.KRYLOV_STEPS] * 3 and (raw > 0.1).all()
  for name, got in W.lanczos_errors(N).items():
    _documented(name, got)


def test_the_evolution_bars_are_the_documented_ones():
  state_err, log_err = W.evolution_errors(N)
  _documented("states", state_err)
  _documented("log_norms", log_err)


def test_the_new_subsystem_shapes_have_more_than_256_partials():
  """tests/test_reduced_density_vjp_gpu.py's two wide rows: 16 bytes (one complex128) per state and partial; the matrix
  kernel keeps the transposed operator, 8 * 4^k bytes, in front of them."""
  vector = E.subsystem_apply_scratch_bytes(2, 20, RD.keep_mask((7,)))
  matrix = E.subsystem_apply_scratch_bytes(2, 19, RD.keep_mask((0, 6, 12, 18)))
  assert vector // (16 * 2) == 512 > 256 and vector % 32 == 0
  assert (matrix - 8 * 4**4) // (16 * 2) == 512 > 256


# ---- the same builders against the dense route at n = 12 --------------------------------------------------------------------------
def _dense_exp(matrix, vectors, factor):
  """e^{factor * matrix} applied to the rows of `vectors`: the Taylor series, until a term is below 2^-60 of the sum."""
  total, term, k = vectors.copy(), vectors.copy(), 0
  while np.abs(term).max() > 2.0**-60 * np.abs(total).max():
    k += 1
    term = (factor / k) * (term @ matrix.T)
    total = total + term
  return total


def _dense_lanczos(matrix, start, m, reorth):
  """The recurrence of tests/krylov_ref.py's docstring on one start vector, H a matrix."""
  basis, alpha, beta = np.zeros((m, len(start)), np.complex128), np.zeros(m), np.zeros(m)
  basis[0] = start / np.linalg.norm(start)
  for j in range(m):
    w = matrix @ basis[j]
    lo = 0 if reorth else max(0, j - 1)
    for _ in range(2 if reorth else 1):
      coef = basis[lo:j + 1].conj() @ w
      alpha[j] += coef[j - lo].real
      w = w - coef @ basis[lo:j + 1]
    beta[j] = np.linalg.norm(w)
    if j + 1 < m:
      basis[j + 1] = w / beta[j]
  return basis, alpha, beta


@pytest.fixture(scope="module")
def dense_h():
  return T.dense_h(SMALL, W.hamiltonian(SMALL), W.WEIGHTS)


def test_small_apply_evolution_and_lanczos_against_the_dense_matrix(dense_h):
  n = SMALL
  assert W.num_terms(n) == 8 and len({(x, z) for op in W.hamiltonian(n) for _, x, z in op}) == 8
  given = np.concatenate([W.starts(n), W.basis_start(n)]).astype(np.complex128)
  _close("n=12 apply", W.applied(n), given @ dense_h.T, 1e-9)
  starts = given[:3]
  norms = np.linalg.norm(starts, axis=1)
  np.testing.assert_array_equal((starts.real**2 + starts.imag**2).sum(axis=1), np.array(W.NORM2))
  for tau in (W.TAU_ONE, W.TAU_TWO):
    want = _dense_exp(dense_h, starts, -tau)
    want_norms = np.linalg.norm(want, axis=1)
    got, logs = W.evolved(n, tau, 0, tail=T.SERIES_EXACT)
    _close(f"n=12 tau={tau} imaginary time, states", got, want / want_norms[:, None], 1e-9)
    _close(f"n=12 tau={tau} imaginary time, log norms", logs, np.log(want_norms), 1e-9)
    cut, cut_logs = W.evolved(n, tau, 0)  # (the series cut where the engine cuts it: 2^-30)
    _close(f"n=12 tau={tau} imaginary time, the engine's cut, states", cut, got, 2.0**-29)
    _close(f"n=12 tau={tau} imaginary time, the engine's cut, log norms", cut_logs, logs, 2.0**-29)
  got, none = W.evolved(n, W.TAU_ONE, 1, tail=T.SERIES_EXACT)
  assert none is None
  _close("n=12 real time", got, _dense_exp(dense_h, starts, -1j * W.TAU_ONE), 1e-9)
  for reorth in (True, False):
    basis, alpha, beta, lengths, got_norms, _ = W.lanczos(n, reorth)
    assert lengths.tolist() == [W.KRYLOV_STEPS] * 3
    _close(f"n=12 reorth={reorth} start norms", got_norms, norms, 1e-12)
    for u in range(3):
      want_basis, want_alpha, want_beta = _dense_lanczos(dense_h, starts[u], W.KRYLOV_STEPS, reorth)
      _close(f"n=12 reorth={reorth} state {u} alpha", alpha[u], want_alpha, 1e-9)
      _close(f"n=12 reorth={reorth} state {u} beta", beta[u], want_beta, 1e-9)
      _close(f"n=12 reorth={reorth} state {u} basis", basis[:, u], want_basis, 1e-9)


def _five_point(f, params, h=1e-3):
  """The fourth-order central difference of f at params: truncation h^4 f^(5) / 30 ~ 1e-12 |f| pi^5, rounding 2^-53 |f| / h."""
  grad = np.zeros(len(params))
  for p in range(len(params)):
    def at(step):
      shifted = np.array(params, dtype=np.float64)
      shifted[p] += step
      return f(shifted)
    grad[p] = (8.0 * (at(h) - at(-h)) - (at(2 * h) - at(-2 * h))) / (12.0 * h)
  return grad


def test_small_circuit_references_against_the_dense_unitary():
  n = SMALL
  gates, n_params = W.circuit(n)
  given = W.circuit_states(n).astype(np.complex128)
  norm2 = 2.0**(n + 1)
  unitary = O.unitary(n, gates, W.PARAMS)
  vals, grad, finals = W.circuit_reference(n)
  want_finals = given @ unitary.T
  _close("n=12 final states", finals, want_finals, 1e-9)
  dense_ops = [T.dense_h(n, [op]) for op in W.hamiltonian(n)]
  values_of = lambda states: np.stack([np.real(np.einsum("ui,ij,uj->u", states.conj(), op, states)) for op in dense_ops], axis=1)
  _close("n=12 values", vals, values_of(want_finals), 1e-9 * norm2)
  upstream = W.circuit_upstream(n)
  want_grad = _five_point(lambda p: float((upstream * values_of(R.final_states(n, gates, p, given))).sum()), W.PARAMS)
  _close("n=12 gradient of the values", grad, want_grad, 1e-9 * max(1.0, float(np.abs(want_grad).max())))
  cot = W.cotangent(n).astype(np.complex128)
  got, phase = W.cotangent_reference(n)
  want = _five_point(lambda p: float(np.real(np.sum(cot.conj() * R.final_states(n, gates, p, given)))), W.PARAMS)
  _close("n=12 gradient through the cotangent", got, want, 1e-9 * max(1.0, float(np.abs(want).max())))
  overlap = sum(float(np.imag(np.vdot(g, psi))) for g, psi in zip(cot, want_finals))
  _close("n=12 phase term", phase, -F.documented_phase_slope(gates, n_params) * overlap, 1e-9 * norm2)
