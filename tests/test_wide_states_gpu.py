"""The state-sweep features at 20 qubits on the GPU, each against its float64 restatement (tests/wide_state_cases.py has the
cases, tests/test_wide_states_cpu.py the conditions they rest on).

n = 20 is n = n_eff with 512 slices per state: the second-level sums of csrc/state_sweep.h (`sweep_row_sum`,
`sweep_row_sum2`) take two trips in `import_norm_finish`, `finish_step_kernel`, `krylov_coef_kernel`, `krylov_norm_kernel`
and `cotangent_finish`, the partials buffers hold 512 entries per row, the default chunk rules cut calls by the workspace
budget, and the observable kernels run as lambda = O psi on caller buffers with one state per XCD.  Three states per call.

Bars (figures of the fp32 restatements: tests/wide_state_cases.py) and, after each, the engine's largest error on an MI355X
  1 import norms   log norms within 1 ulp of 0.5 log(norm^2) -- the squared norms 2, 8 and 2^-5 are exact in float64 in any
                   order of summation, so the ulp is for `log` alone; the states come back bit for bit.  Measured: 0 ulp
  2 apply          (T + 2) 2^-24 R max|phi| per amplitude, T = 8: the fp32 bound of a T-term sum (tests/test_thermal_gpu.py),
                   4.2e-10 for the state of norm^2 2^-5.  Measured: 0 -- with parts +-2^-10 and coefficients that are
                   multiples of 2^-4 every product and sum is exact in fp32, so any difference is a wrong partner or sign
  3 evolution      8 x the fp32 restatement against its float64 run on this case: states 2.6e-9 (per unit norm), log norms
                   4.3e-7; the round trip tau, -tau within twice the state bar.  Measured: states 3.0e-10 (one step) and
                   1.0e-9 (two steps), log norms 5.0e-8 and 9.3e-8, real time 0.12 of its bar, there and back 0.08
  4 Lanczos        8 x the fp32 restatement against its float64 run on this case, the larger of the two modes: alpha 3.5e-7,
                   beta 1.8e-7, basis 8.1e-9, |V^dagger V - I| 2.7e-7 (full mode); start norms within 1 ulp.  Measured: alpha
                   4.1e-8, beta 2.8e-8, basis 7.8e-10, |V^dagger V - I| 3.4e-8, start norms equal
  5 streamed       bit for bit against the stored local route; general coefficients (m + 4) 2^-23 sum_j |c_j| max|v_j| against
                   `krylov_combine` over the stored basis (tests/test_krylov_stream_gpu.py), 6.1e-9.  Measured: 1.9e-9
  6 budget chunks  bit for bit
  7 circuits       values 2e-5 max(1, sum|c|) ||phi||^2 = 107, gradients 1e-4 max(1, ||grad||_inf) = 3.5, amplitudes
                   5e-6 ||phi|| / 2^10 = 7.1e-6 (tests/test_from_states_gpu.py; the last factor restores the per-amplitude scale
                   the bar has at one tile).  Measured: values 5.3e-3, gradient 0.26, amplitudes 7.5e-7
  8 cotangent      gradients 1e-4 max(1, ||grad||_inf) = 412 (tests/test_final_states_gpu.py), the reference's phase term
                   (4.1e6) at least 100 x the bar.  Measured: 0.26

Which test a wrong second-level sum fails (checked once on builds of scratch copies of csrc/state_sweep.h, reads in bounds):
  `sweep_row_sum` stepping 2 x 256 (slices 256..511 lost): the 89 tests of the thermal, Krylov, streamed and final-state
      modules at n <= 16 pass; fails 1 (norm^2 halves), 3 in imaginary time (`finish_step_kernel`), 4 (`krylov_norm_kernel`:
      beta) and the basis state's length.  Real time, 7 and 8 pass: the import's wrong norm divides and multiplies the same state
  `sweep_row_sum2` stepping 2 x 256: the same 89 tests and every narrower subsystem shape pass; fails 4 (`krylov_coef_kernel`),
      8 (`cotangent_finish`) and the two wide shapes of tests/test_reduced_density_vjp_gpu.py (`subsys_dots_finish`)
  `sweep_row_sum2` reading row[2 * i] for its imaginary row: differs from row[slices + i] at every number of slices; fails 4, 8,
      every shape of tests/test_reduced_density_vjp_gpu.py and the Krylov and final-state tests at small n as well
Every comparison prints its largest error beside its bar before it asserts.
"""
import functools
import math

import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from tests import thermal_ref as T
from tests import wide_state_cases as W

pytestmark = pytest.mark.gpu

N = W.N
STATE_BYTES = 8 << N
M = W.KRYLOV_STEPS


def _engine(ops, gates=(), n_params=0, **options):
  eng = E.Engine(0)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(N, list(gates), n_params)
  if ops:
    eng.set_observables(ops)
  return eng


def _np(t):
  return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _close(what, got, want, bar):
  got = _np(got)
  err = np.abs(got - want)
  print(f"{what}: max error {np.max(err, initial=0.0):.3e}  bar {np.min(bar):.3e}  worst {np.max(err / bar, initial=0.0):.3f} of its bar")
  assert np.isfinite(got).all(), what
  assert (err <= bar).all(), (what, float(np.max(err)), float(np.min(bar)))


def _close_complex(what, got, want, bar):
  got = _np(got)
  _close(what + " real", got.real, want.real, bar)
  _close(what + " imag", got.imag, want.imag, bar)


def _same(a, b):
  if a is None or b is None:
    return a is None and b is None
  return torch.equal(torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _starts():
  return torch.tensor(W.starts(N)).cuda()


# ---- 1. the import's norms --------------------------------------------------------------------------------------------------------
def test_import_norms_are_exact():
  """H = 0 (all weights zero): `evolve_states` is the import and `evolve_init_kernel` alone.  One lost or doubled slice of
  `import_norm_finish`'s sum moves a squared norm by a factor 1 -+ 2^-9, a log norm by 1e-3."""
  eng = _engine(W.hamiltonian(N))
  zero = [0.0, 0.0]
  assert eng.describe_evolution(1.0, 0, zero)["R"] == 0.0
  starts = _starts()
  before = starts.clone()
  for given, norm2 in ((starts, W.NORM2), (torch.from_numpy(W.starts_with_zero_row(N)).cuda(), (W.NORM2[0], 0.0, W.NORM2[2]))):
    got, logs = eng.evolve_states(given, 1.0, 0, zero)
    assert logs.dtype == torch.float64 and _same(got, given)
    logs = logs.cpu().numpy()
    for u, value in enumerate(norm2):
      if value == 0.0:
        assert logs[u] == -np.inf, logs
        continue
      want = 0.5 * math.log(value)
      print(f"norm^2 = {value}: log norm {logs[u]!r}  want {want!r}  ulp {np.spacing(abs(want)):.3e}")
      assert abs(logs[u] - want) <= np.spacing(abs(want)), (u, logs[u], want)
  assert _same(starts, before)


# ---- 2. apply_observables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [{"observable_kernel": 0}, {"observable_kernel": 1}, {"chunk_states": 2}],
                         ids=["kernel0", "kernel1", "chunks_of_2"])
def test_apply_observables_against_the_restatement(options):
  ops, want = W.hamiltonian(N), W.applied(N)
  eng = _engine(ops, **options)
  factor = (W.num_terms(N) + 2) * 2.0**-24 * T.radius(N, ops, W.WEIGHTS)
  starts = _starts()
  before = starts.clone()
  got = eng.apply_observables(starts, W.WEIGHTS)
  assert _same(starts, before)
  _close_complex(f"apply {options}", got, want[:3], factor * np.abs(W.starts(N)).max(axis=1, keepdims=True))
  basis = torch.from_numpy(W.basis_start(N)).cuda()
  got = eng.apply_observables(basis, W.WEIGHTS)
  _close_complex(f"apply {options}, basis state", got, want[3:], factor)
  assert int((got != 0).sum()) == int((want[3] != 0).sum()) == 8  # (one amplitude per term)


# ---- 3. imaginary and real time ---------------------------------------------------------------------------------------------------
def test_imaginary_time_one_step_and_two():
  ops = W.hamiltonian(N)
  state_bar, log_bar = W.evolution_bars(N)
  eng = _engine(ops)
  for tau, steps in ((W.TAU_ONE, 1), (W.TAU_TWO, 2)):
    plan = eng.describe_evolution(tau, 0, W.WEIGHTS)
    assert plan["steps"] == steps and plan["terms_per_step"] <= 12, plan
    want, want_log = W.evolved(N, tau, 0)
    got, logs = eng.evolve_states(_starts(), tau, 0, W.WEIGHTS)
    _close_complex(f"tau={tau} states", got, want, state_bar)
    _close(f"tau={tau} log norms", logs, want_log, log_bar)
    norms = torch.linalg.vector_norm(got.to(torch.complex128), dim=1)
    # (sum / ||sum||: the fp32 scale and the fp32 product are each within 2^-24 relative, and the norm follows them)
    _close(f"tau={tau} norms of the returned states", norms, 1.0, 2.0**-22)


def test_real_time_and_back():
  ops = W.hamiltonian(N)
  state_bar, _ = W.evolution_bars(N)
  eng = _engine(ops)
  plan = eng.describe_evolution(W.TAU_ONE, 1, W.WEIGHTS)
  assert plan["steps"] == 1 and plan["terms_per_step"] <= 12, plan
  bar = state_bar * np.sqrt(np.array(W.NORM2))[:, None]
  got, none = eng.evolve_states(_starts(), W.TAU_ONE, 1, W.WEIGHTS)
  assert none is None
  _close_complex("real time", got, W.evolved(N, W.TAU_ONE, 1)[0], bar)
  back, _ = eng.evolve_states(got, -W.TAU_ONE, 1, W.WEIGHTS)
  _close_complex("forward and back", back, W.starts(N).astype(np.complex128), 2 * bar)


# ---- 4. the Lanczos basis ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stored(reorth):
  """`krylov_basis` of the start states on a default engine: computed once per mode and never written."""
  return _engine(W.hamiltonian(N)).krylov_basis(_starts(), M, W.WEIGHTS, reorth)


@pytest.mark.parametrize("reorth", [True, False], ids=["full", "local"])
def test_lanczos_basis_against_the_restatement(reorth):
  want_basis, want_alpha, want_beta, want_lengths, want_norms, _ = W.lanczos(N, reorth)
  bars = W.lanczos_bars(N)
  starts = _starts()
  before = starts.clone()
  basis, alpha, beta, lengths, norms = _stored(reorth)
  assert _same(starts, before)
  assert basis.shape == (M, 3, 1 << N) and lengths.cpu().tolist() == want_lengths.tolist() == [M] * 3
  _close(f"reorth={reorth} alpha", alpha, want_alpha, bars["alpha"])
  _close(f"reorth={reorth} beta", beta, want_beta, bars["beta"])
  _close_complex(f"reorth={reorth} basis", basis, want_basis, bars["basis"])
  _close(f"reorth={reorth} start norms", norms, want_norms, np.spacing(want_norms))
  if reorth:
    for u in range(3):
      _close(f"state {u} |V^dagger V - I|", W.gram(_np(basis[:, u])), np.eye(M), bars["gram"])


def test_a_zero_row_has_length_zero_and_leaves_its_neighbours_alone():
  whole = _stored(True)
  given = torch.from_numpy(W.starts_with_zero_row(N)).cuda()
  basis, alpha, beta, lengths, norms = _engine(W.hamiltonian(N)).krylov_basis(given, M, W.WEIGHTS, True)
  assert lengths.cpu().tolist() == [M, 0, M] and norms[1] == 0
  assert (torch.view_as_real(basis[:, 1]) == 0).all() and (alpha[1] == 0).all() and (beta[1] == 0).all()
  for u in (0, 2):
    assert _same(basis[:, u], whole[0][:, u]) and _same(alpha[u], whole[1][u]) and _same(beta[u], whole[2][u])


def test_a_basis_state_under_the_diagonal_part_has_length_one():
  (diagonal,) = W.diagonal_part(N)
  assert len(diagonal) == 1
  coeff, _, z = diagonal[0]
  z_index = sum(1 << (N - 1 - q) for q in range(N) if z >> q & 1)
  sign = -1.0 if bin(W.BASIS_INDEX & z_index).count("1") % 2 else 1.0
  start = torch.from_numpy(W.basis_start(N)).cuda()
  basis, alpha, beta, lengths, _ = _engine([diagonal]).krylov_basis(start, M)
  assert lengths.cpu().tolist() == [1]
  assert alpha[0, 0].item() == sign * float(np.float32(coeff)) and (alpha[0, 1:] == 0).all() and (beta == 0).all()
  assert _same(basis[0], start) and (torch.view_as_real(basis[1:]) == 0).all()


# ---- 5. streamed Lanczos ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pass_one():
  return _engine(W.hamiltonian(N)).krylov_tridiagonal(_starts(), M, W.WEIGHTS)


def _one_hot(picks):
  coef = torch.zeros((3, len(picks), M), dtype=torch.complex64)
  for s, j in enumerate(picks):
    coef[:, s, j] = 1
  return coef


def test_pass_one_gives_the_bits_of_the_stored_local_route():
  stored = _stored(False)
  alpha, beta, lengths, recurrence, norms = _pass_one()
  assert recurrence.shape == (3, M, 2) and recurrence.dtype == torch.complex64
  assert _same(alpha, stored[1]) and _same(beta, stored[2]) and _same(lengths, stored[3]) and _same(norms, stored[4])
  assert (torch.view_as_real(recurrence[:, 0, 0]) == 0).all()
  assert torch.equal(recurrence[:, :, 1].real, alpha.to(torch.float32))


def test_one_hot_replays_are_the_rows_of_the_stored_local_basis():
  basis = _stored(False)[0]
  _, beta, lengths, recurrence, _ = _pass_one()
  eng = _engine(W.hamiltonian(N))
  picks = (0, 1, 2, M - 1)
  out = eng.krylov_replay(_starts(), beta, lengths, recurrence, _one_hot(picks), W.WEIGHTS)
  assert out.shape == (3, len(picks), 1 << N)
  for s, j in enumerate(picks):
    assert _same(out[:, s], basis[j]), (s, j)


def test_nine_outputs_against_combine_over_the_stored_basis():
  """Nine outputs: a group of eight and a group of one."""
  basis = _stored(False)[0]
  _, beta, lengths, recurrence, _ = _pass_one()
  rng = np.random.default_rng(W.SEED + 9)
  coef = torch.from_numpy((rng.normal(size=(3, 9, M)) + 1j * rng.normal(size=(3, 9, M))).astype(np.complex64))
  got = _engine(W.hamiltonian(N)).krylov_replay(_starts(), beta, lengths, recurrence, coef, W.WEIGHTS)
  want = _np(E.krylov_combine(basis, coef))
  row_max = _np(basis.abs().amax(dim=2))  # [m, U]
  bar = (M + 4) * 2.0**-23 * np.einsum("usj,ju->us", np.abs(coef.numpy()), row_max)[:, :, None]
  _close_complex("replay of 9 outputs against combine", got, want, bar)


# ---- 6. chunks from the budget ----------------------------------------------------------------------------------------------------
def test_the_budget_cuts_the_evolution_into_single_states():
  """40 MB / (4 buffers x 8 MB) = 1 state per chunk.  No describe call reports the evolution's chunk, so the workspace the
  engine holds afterwards proves it: 4 state buffers (32 MB) at one state per chunk, 8 at two, 12 at three."""
  ops = W.hamiltonian(N)
  roomy, tight, single = _engine(ops, workspace_budget_mb=1024), _engine(ops, workspace_budget_mb=40), _engine(ops, chunk_states=1)
  for tau, mode in ((W.TAU_ONE, 0), (W.TAU_TWO, 0), (W.TAU_ONE, 1)):
    want = roomy.evolve_states(_starts(), tau, mode, W.WEIGHTS)
    for other in (tight, single):
      got = other.evolve_states(_starts(), tau, mode, W.WEIGHTS)
      assert _same(got[0], want[0]) and _same(got[1], want[1]), (tau, mode)
  assert 4 * STATE_BYTES <= tight.allocated_bytes() < 6 * STATE_BYTES <= 12 * STATE_BYTES <= roomy.allocated_bytes()


def test_the_budget_cuts_the_krylov_calls_into_pairs():
  """Stored basis: 40 MB / (2 x 8 MB) = 2 states per chunk; streamed: 80 MB / (5 x 8 MB) = 2."""
  ops = W.hamiltonian(N)
  tight = _engine(ops, workspace_budget_mb=40)
  assert tight.describe_krylov(3, M, True)["chunk_states"] == tight.describe_krylov(3, M, False)["chunk_states"] == 2
  roomy = _engine(ops, workspace_budget_mb=1024)
  assert roomy.describe_krylov(3, M, True)["chunk_states"] == roomy.describe_krylov_stream(3, M, 9)["chunk_states"] == 3
  single = _engine(ops, chunk_states=1)
  assert single.describe_krylov(3, M, True)["chunk_states"] == single.describe_krylov_stream(3, M, 9)["chunk_states"] == 1
  for reorth in (True, False):
    want = roomy.krylov_basis(_starts(), M, W.WEIGHTS, reorth)
    assert all(_same(a, b) for a, b in zip(want, _stored(reorth)))
    for other in (tight, single):
      got = other.krylov_basis(_starts(), M, W.WEIGHTS, reorth)
      assert all(_same(a, b) for a, b in zip(got, want)), reorth
  streamed = _engine(ops, workspace_budget_mb=80)
  assert streamed.describe_krylov_stream(3, M, 9)["chunk_states"] == 2
  rng = np.random.default_rng(W.SEED + 6)
  coef = torch.from_numpy((rng.normal(size=(3, 9, M)) + 1j * rng.normal(size=(3, 9, M))).astype(np.complex64))
  want = roomy.krylov_tridiagonal(_starts(), M, W.WEIGHTS)
  want_out = roomy.krylov_replay(_starts(), want[1], want[2], want[3], coef, W.WEIGHTS)
  for other in (streamed, single):
    got = other.krylov_tridiagonal(_starts(), M, W.WEIGHTS)
    assert all(_same(a, b) for a, b in zip(got, want))
    assert _same(other.krylov_replay(_starts(), got[1], got[2], got[3], coef, W.WEIGHTS), want_out)


# ---- 7. circuits from wide states -------------------------------------------------------------------------------------------------
def test_circuits_from_wide_states():
  gates, n_params = W.circuit(N)
  ops = W.hamiltonian(N)
  want_vals, want_grad, want_finals = W.circuit_reference(N)
  states = torch.tensor(W.circuit_states(N)).cuda()
  before = states.clone()
  norm2 = 2.0**(N + 1)
  eng = _engine(ops, gates, n_params)
  vals, grad = eng.expectation_vjp_from_states(states, W.PARAMS, W.circuit_upstream(N))
  value_bar = 2e-5 * np.array([max(1.0, sum(abs(c) for c, _, _ in op)) for op in ops])[None, :] * norm2
  _close("values", vals, want_vals, value_bar)
  _close("gradient", grad, want_grad, 1e-4 * max(1.0, float(np.abs(want_grad).max())))
  _close("forward-only values", eng.expectation_from_states(states, W.PARAMS), want_vals, value_bar)
  finals = eng.statevector_from_states(states, W.PARAMS)
  _close_complex("final states", finals, want_finals, 5e-6 * math.sqrt(norm2) / 2.0**10)
  assert _same(states, before)


# ---- 8. the cotangent of wide final states ----------------------------------------------------------------------------------------
def test_cotangent_of_wide_final_states():
  gates, n_params = W.circuit(N)
  want, phase = W.cotangent_reference(N)
  bar = 1e-4 * max(1.0, float(np.abs(want).max()))
  print(f"phase term {np.abs(phase).max():.3e}  ||grad||_inf {np.abs(want).max():.3e}  bar {bar:.3e}")
  assert np.abs(phase).min() >= 100.0 * bar  # (a wrong sum in `cotangent_finish` moves the gradient by a share of this term)
  eng = _engine(None, gates, n_params)
  states, cot = torch.tensor(W.circuit_states(N)).cuda(), torch.tensor(W.cotangent(N)).cuda()
  out, grad = eng.statevector_vjp_from_states(states, W.PARAMS, cot, want_states=True)
  _close("gradient", grad, want, bar)
  _close_complex("exported states", out, W.circuit_reference(N)[2], 5e-6 * math.sqrt(2.0**(N + 1)) / 2.0**10)
  eng.set_option("chunk_states", 2)
  assert torch.equal(eng.statevector_vjp_from_states(states, W.PARAMS, cot), grad)
