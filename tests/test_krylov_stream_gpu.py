"""Streamed Lanczos on the GPU (`qhbm_krylov_tridiagonal`, `qhbm_krylov_replay`, `inference.krylov_space(store_basis=False)`
and what passes `store_basis` through) against the stored route (`qhbm_krylov_basis(reorth = 0)`,
`qhbm_krylov_combine`), the two-pass restatement (tests/krylov_stream_ref.py) and `eigh`.

Shapes: n = 3 (padded pitch, one slice), n = 10 (n = n_eff), n = 13 (block observable kernel, several slices); three states
with chunk_states = 2 (a short last chunk); m = 12, and m = 48 where derived quantities are held.  Operators and start
vectors are tests/krylov_cases.py's: every ||w|| / R stays out of [2^-19, 0.1] (tests/test_krylov_cpu.py checks it).

Bars
  T, rows        bit for bit: alpha, beta, lengths of pass one against the stored local route; one-hot replays against its rows
  general coef   per component (m + 4) 2^-23 sum_j |coef_j| max_i |v_j[i]|: replay and `krylov_combine` are fp32 recursive
                 sums of the same m products, each within half that of the exact sum.  The largest difference is printed
  derived        8 x the error of the fp32 two-pass restatement against `eigh` on the same case (n = 10, m = 48), computed
                 here from tests/krylov_stream_ref.py -- tests/test_krylov_stream_cpu.py proves that restatement equal, bit for
                 bit, to `krylov_ref.lanczos(reorth=False)`, whose errors the bars of tests/test_krylov_gpu.py are
  ground_state   8 x the fp32 restatement of the same restarted run against `eigh`, the larger of the two modes (the local
                 mode's is the two-pass restatement; see the test)
Every comparison prints its largest error beside its bar before it asserts.  The refusal of start states or outputs inside
the engine's workspace is not exercised: no interface hands out an address of the workspace."""
import functools

import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir
from qhbmlib_amd.inference import krylov
from tests import krylov_cases as C
from tests import krylov_ref as K
from tests import krylov_stream_ref as S
from tests import thermal_ref as T

pytestmark = pytest.mark.gpu

WEIGHTS = C.WEIGHTS
SHAPES = [(3, 12, {}), (10, 12, {"chunk_states": 2}), (13, 12, {"chunk_states": 2})]


def _engine(n, ops, **options):
  eng = E.Engine(0)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(n, [], 0)
  if ops:
    eng.set_observables(ops)
  return eng


def _np(t):
  return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _close(what, got, want, bar):
  got = _np(got)
  err = np.abs(got - want)
  print(f"{what}: max error {np.max(err, initial=0.0):.3e}  bar {np.min(bar):.3e}")
  assert np.isfinite(got).all(), what
  assert (err <= bar).all(), (what, float(np.max(err)), float(np.min(bar)))


def _same(a, b):
  return torch.equal(torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else torch.equal(a, b)


def _tfim_operators(n):
  """The TFIM ring's two parts as PauliSums: the masks of `krylov_cases.tfim_parts`."""
  qubits = ir.GridQubit.rect(1, n)
  field = ir.PauliSum([ir.PauliString(ir.PX(q), coefficient=-1.0) for q in qubits])
  bonds = ir.PauliSum([ir.PauliString(ir.PZ(qubits[i]), ir.PZ(qubits[(i + 1) % n]), coefficient=-1.0) for i in range(n)])
  assert [field.masks(qubits), bonds.masks(qubits)] == [[tuple(t) for t in part] for part in C.tfim_parts(n)]
  return [field, bonds]


@functools.lru_cache(maxsize=None)
def _routes(n, m):
  """(start states, the stored local route's (basis, alpha, beta, lengths, norms), pass one's (alpha, beta, lengths,
  recurrence, norms)) on the device, each computed once and never written."""
  starts = torch.from_numpy(C.starts(n)).cuda()
  eng = _engine(n, C.tfim_parts(n))
  return starts, eng.krylov_basis(starts, m, WEIGHTS, False), eng.krylov_tridiagonal(starts, m, WEIGHTS)


def _one_hot(num, picks, m):
  coef = torch.zeros((num, len(picks), m), dtype=torch.complex64)
  for s, j in enumerate(picks):
    coef[:, s, j] = 1
  return coef


# ---- 1. T is the stored route's T ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,options", SHAPES)
def test_pass_one_gives_the_bits_of_the_stored_local_route(n, m, options):
  starts, stored, _ = _routes(n, m)
  before = starts.clone()
  alpha, beta, lengths, recurrence, norms = _engine(n, C.tfim_parts(n), **options).krylov_tridiagonal(starts, m, WEIGHTS)
  assert _same(starts, before)
  assert alpha.dtype == beta.dtype == norms.dtype == torch.float64 and lengths.dtype == torch.int32
  assert recurrence.shape == (starts.shape[0], m, 2) and recurrence.dtype == torch.complex64
  assert _same(alpha, stored[1]) and _same(beta, stored[2]) and _same(lengths, stored[3]) and _same(norms, stored[4])
  assert lengths.cpu().tolist() == C.run(n, m, False, False)[3].tolist()
  # the recorded pairs: (0, c_0) at step 0, and Re c_j is alpha_j rounded to fp32
  assert (torch.view_as_real(recurrence[:, 0, 0]) == 0).all()
  assert torch.equal(recurrence[:, :, 1].real, alpha.to(torch.float32))
  if n == 3:
    assert (lengths < m).all()  # (the case that has breakdowns)


# ---- 2. the replayed basis is the one T belongs to ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,m,options", SHAPES)
def test_one_hot_replays_are_the_rows_of_the_stored_local_basis(n, m, options):
  starts, (basis, _, _, _, _), (_, beta, lengths, recurrence, _) = _routes(n, m)
  eng = _engine(n, C.tfim_parts(n), **options)
  before = starts.clone()
  for picks in ((0, 1, 2, m - 1, 3, 4, 5, 6), (0, 1, 2, m - 1, 3, 4, 5, 6, 7)):  # eight at a time; nine: two groups
    out = eng.krylov_replay(starts, beta, lengths, recurrence, _one_hot(starts.shape[0], picks, m), WEIGHTS)
    assert out.shape == (starts.shape[0], len(picks), 1 << n) and out.dtype == torch.complex64 and _same(starts, before)
    for s, j in enumerate(picks):
      assert _same(out[:, s], basis[j]), (n, len(picks), s, j)


# ---- 3. general coefficients ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_outputs", [1, 8, 9])
@pytest.mark.parametrize("n,m,options", SHAPES)
def test_general_coefficients_against_combine_over_the_stored_basis(n, m, options, num_outputs):
  starts, (basis, _, _, _, _), (_, beta, lengths, recurrence, _) = _routes(n, m)
  rng = np.random.default_rng(1000 * n + num_outputs)
  shape = (starts.shape[0], num_outputs, m)
  coef = torch.from_numpy((rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64))
  got = _engine(n, C.tfim_parts(n), **options).krylov_replay(starts, beta, lengths, recurrence, coef, WEIGHTS)
  want = _np(E.krylov_combine(basis, coef))
  row_max = np.abs(_np(basis)).max(axis=2)  # [m, U]
  bar = (m + 4) * 2.0**-23 * np.einsum("usj,ju->us", np.abs(coef.numpy()), row_max)[:, :, None]
  print(f"n={n} S={num_outputs}: largest |replay - combine| = {np.abs(_np(got) - want).max():.3e}")
  _close(f"replay n={n} S={num_outputs} real", got.real, want.real, bar)
  _close(f"replay n={n} S={num_outputs} imag", got.imag, want.imag, bar)


# ---- 4. derived quantities at n = 10, m = 48 ---------------------------------------------------------------------------------------------------
def _unit_rows(states):
  return np.stack([K._unit(v) for v in states])  # pylint: disable=protected-access


@functools.lru_cache(maxsize=None)
def _derived_bars():
  """8 x the fp32 two-pass restatement against `eigh` at n = 10, m = 48 on `krylov_cases.starts`: theta_min, theta_max, the
  ground vector, e^{-4 H} phi and its log norm, e^{-itH} phi."""
  n, m, beta_value = 10, 48, 4.0
  ops, starts, d = C.tfim_parts(n), C.starts(n), C.dense(n)
  given = starts.astype(np.complex128)
  alpha, beta, lengths, recurrence, norms = S.tridiagonal(n, ops, starts, m, WEIGHTS, np.float32)
  pairs = [K.ritz(alpha[u], beta[u], lengths[u]) for u in range(len(lengths))]
  replay = lambda coef: S.replay(n, ops, starts, beta, recurrence, coef, WEIGHTS, np.float32)
  out = {"theta_min": max(abs(theta[0] - d.evals[0]) for theta, _ in pairs),
         "theta_max": max(abs(theta[-1] - d.evals[-1]) for theta, _ in pairs)}
  vecs = _unit_rows(replay(np.stack([s[:, 0] for _, s in pairs])[:, None, :])[:, 0])
  out["ground"] = max(float(np.abs(K.align(v, d.evecs[:, 0]) - d.evecs[:, 0]).max()) for v in vecs)
  coef, logs = np.zeros((3, 1, m), np.complex128), np.zeros(3)
  for u, (theta, s) in enumerate(pairs):
    coef[u, 0], log_norm = krylov.evolution_coefficients(theta, s, beta_value, 0, m)
    logs[u] = log_norm + np.log(norms[u])
  want, want_log = d.evolve(given, beta_value, 0)
  out["states"] = float(np.abs(_unit_rows(replay(coef)[:, 0]) - want).max())
  out["log_norms"] = float(np.abs(logs - want_log).max())
  out["real_time"] = 0.0
  for t in C.TIMES:
    for u, (theta, s) in enumerate(pairs):
      coef[u, 0] = krylov.evolution_coefficients(theta, s, t, 1, m)[0] * norms[u]
    out["real_time"] = max(out["real_time"], float(np.abs(replay(coef)[:, 0] - d.evolve(given, t, 1)[0]).max()))
  print(f"fp32 two-pass restatement against eigh, n = 10, m = 48: {out}")
  return {key: C.MARGIN * float(value) for key, value in out.items()}


def test_a_streamed_space_against_eigh():
  n, m, beta_value = 10, 48, 4.0
  bars, d = _derived_bars(), C.dense(n)
  starts = C.starts(n)
  given = starts.astype(np.complex128)
  ops = _tfim_operators(n)
  space = inference.krylov_space(ops, torch.from_numpy(starts), m, weights=WEIGHTS, store_basis=False)
  assert isinstance(space, inference.StreamedKrylovSpace) and space.basis is None and space.lengths.tolist() == [m] * 3
  assert space.radius == T.radius(n, C.tfim_parts(n), WEIGHTS) and space.num_steps == m and space.num_vectors == 3
  pairs = space.ritz()
  _close("theta_min", [theta[0] for theta, _ in pairs], d.evals[0], bars["theta_min"])
  _close("theta_max", [theta[-1] for theta, _ in pairs], d.evals[-1], bars["theta_max"])
  assert all(r.shape == (m,) and r[0] <= 2.0**-10 for r in space.residuals()) and space.replays == 0
  ground = _np(space.ritz_states([0]))[:, 0].astype(np.complex128)
  want = d.evecs[:, 0]
  for u in range(3):
    aligned = K.align(ground[u], want)
    _close(f"ground vector from state {u}", np.stack([aligned.real, aligned.imag]), np.stack([want.real, want.imag]), bars["ground"])
  want, want_log = d.evolve(given, beta_value, 0)
  got, logs = space.evolve(beta_value, 0)
  assert got.shape == (3, 1 << n) and got.dtype == torch.complex64 and logs.dtype == torch.float64 and logs.shape == (3,)
  _close("e^{-4 H} states", torch.view_as_real(got), np.stack([want.real, want.imag], -1), bars["states"])
  _close("e^{-4 H} log norms", logs, want_log, bars["log_norms"])
  assert space.replays == 2
  many, many_logs = space.evolve_many([0.5, beta_value], 0)
  assert many.shape == (3, 2, 1 << n) and many_logs.shape == (3, 2) and space.replays == 3
  # (the same sums in another instance of the kernel, SB = 2: held to the same bars, not to the same bits)
  assert _same(many_logs[:, 1], logs)
  _close("evolve_many e^{-4 H} states", torch.view_as_real(many[:, 1]), np.stack([want.real, want.imag], -1), bars["states"])
  for t in C.TIMES:
    want = d.evolve(given, t, 1)[0]
    got, none = space.evolve(t, 1)
    assert none is None
    _close(f"t={t} states", torch.view_as_real(got), np.stack([want.real, want.imag], -1), bars["real_time"])
  both, none = space.evolve_many(C.TIMES, 1)
  assert none is None and both.shape == (3, len(C.TIMES), 1 << n)
  for k, t in enumerate(C.TIMES):
    want = d.evolve(given, t, 1)[0]
    _close(f"evolve_many t={t} states", torch.view_as_real(both[:, k]), np.stack([want.real, want.imag], -1), bars["real_time"])
  (lo, lo_res), (hi, hi_res) = inference.spectrum_extremes(ops, weights=WEIGHTS, seed=21, store_basis=False)
  _close("spectrum_extremes theta_min", lo, d.evals[0], bars["theta_min"])
  _close("spectrum_extremes theta_max", hi, d.evals[-1], bars["theta_max"])
  assert 0 <= lo_res <= 2.0**-10 and 0 <= hi_res <= 2.0**-10
  with pytest.raises(ValueError, match="full reorthogonalisation"):
    inference.krylov_space(ops, torch.from_numpy(starts), m, weights=WEIGHTS, store_basis=False, reorthogonalise=True)


@functools.lru_cache(maxsize=None)
def _sweep_bars():
  """8 x the fp32 two-pass restatement's finite-temperature Lanczos against `eigh` on the sweep's own start vectors."""
  (n, m), ops = C.SWEEP_CASES["random"], C.tfim_parts(C.SWEEP_CASES["random"][0])
  starts = C.sweep_starts("random")
  alpha, beta, lengths, recurrence, norms = S.tridiagonal(n, ops, starts, m, WEIGHTS, np.float32)
  pairs = [krylov.ritz(alpha[u], beta[u], lengths[u]) for u in range(len(lengths))]
  lw = krylov.ftlm_log_weights(pairs, norms, C.BETAS)
  log_z, energy = krylov.ftlm_log_partition(lw, n, "random"), krylov.ftlm_energy(pairs, norms, C.BETAS)
  _, want_log_z, want_energy, want_entropy, want_states = C.sweep_exact("random")
  coef = np.zeros((len(lengths), len(C.BETAS), m), np.complex128)
  for u, (theta, s) in enumerate(pairs):
    for b, value in enumerate(C.BETAS):
      coef[u, b] = krylov.evolution_coefficients(theta, s, 0.5 * value, 0, m)[0]
  states = S.replay(n, ops, starts, beta, recurrence, coef, WEIGHTS, np.float32)
  errors = dict(log_z=np.abs(log_z - want_log_z).max(), energy=np.abs(energy - want_energy).max(),
                entropy=np.abs(np.array(C.BETAS) * energy + log_z - want_entropy).max(),
                states=max(np.abs(_unit_rows(states[:, b]) - want_states[b]).max() for b in range(len(C.BETAS))))
  print(f"fp32 two-pass restatement of the sweep against eigh: {errors}")
  return {key: C.MARGIN * float(value) for key, value in errors.items()}


def test_a_streamed_sweep_against_eigh():
  (n, m), num, seed = C.SWEEP_CASES["random"], C.SWEEP_VECTORS, C.SWEEP_SEED
  bars = _sweep_bars()
  _, want_log_z, want_energy, want_entropy, want_states = C.sweep_exact("random")
  sweep = inference.thermal_sweep(_tfim_operators(n), C.BETAS, num_vectors=num, num_steps=m, seed=seed, weights=WEIGHTS, store_basis=False)
  assert isinstance(sweep.space, inference.StreamedKrylovSpace) and sweep.space.basis is None
  log_z, energy, entropy = sweep.log_partition(), sweep.energy(), sweep.entropy()
  for b, beta in enumerate(C.BETAS):
    _close(f"beta={beta} log Z", log_z[b], want_log_z[b], bars["log_z"])
    _close(f"beta={beta} <H>", energy[b], want_energy[b], bars["energy"])
    _close(f"beta={beta} S", entropy[b], want_entropy[b], bars["entropy"])
  assert sweep.space.replays == 0  # (numbers are functions of T alone)
  ens = sweep.ensemble(C.BETAS[1])
  assert isinstance(ens, inference.ThermalEnsemble) and ens.states.shape == (num, 1 << n) and sweep.space.replays == 1
  _close("ensemble states against eigh", torch.view_as_real(ens.states), np.stack([want_states[1].real, want_states[1].imag], -1), bars["states"])


def _restated_ground_state(n, ops, start, num_steps=24, max_restarts=8, tolerance=2.0**-20):
  """`inference.ground_state(store_basis=False)` by the fp32 two-pass restatement: one pass and one replay per restart."""
  radius = T.radius(n, ops, WEIGHTS)
  current, restarts = np.asarray(start).reshape(1, -1), 0
  while True:
    alpha, beta, lengths, recurrence, _ = S.tridiagonal(n, ops, current, num_steps, WEIGHTS, np.float32)
    theta, s = K.ritz(alpha[0], beta[0], lengths[0])
    residual = float(beta[0, lengths[0] - 1] * abs(s[-1, 0]))
    coef = np.zeros((1, 1, num_steps), np.complex128)
    coef[0, 0, :lengths[0]] = s[:, 0]
    current = _unit_rows(S.replay(n, ops, current, beta, recurrence, coef, WEIGHTS, np.float32)[:, 0])
    if residual <= tolerance * radius or restarts >= max_restarts:
      return float(theta[0]), current[0], restarts
    restarts += 1


def test_ground_state_without_a_stored_basis():
  n = 10
  d = C.dense(n)
  want = d.evecs[:, 0]
  radius = T.radius(n, C.tfim_parts(n), WEIGHTS)
  # the bar of tests/test_krylov_gpu.py's ground-state test, by that file's rule for what both modes must meet: 8 x the fp32
  # restatement of the same restarted run, the LARGER of the two modes -- full: `krylov_ref.ground_state`, as there; local:
  # the two-pass restatement.  One scalar against `eigh` can come out far below the fp32 rounding of the run by accident
  # (measured: the local restatement is off by 2.3e-9 in E_0, the full one by 1.3e-7, at |E_0| = 11.3 with an fp32 ulp of
  # 9.5e-7), and such an accident is no bar
  start = T.random_states(1, n, 0)
  local_energy, local_state, local_restarts = _restated_ground_state(n, C.tfim_parts(n), start)
  full_energy, full_state, _, full_restarts = K.ground_state(n, C.tfim_parts(n), start, weights=WEIGHTS, dtype=np.float32)
  energy_errors = [abs(local_energy - d.evals[0]), abs(full_energy - d.evals[0])]
  state_errors = [float(np.abs(K.align(v, want) - want).max()) for v in (local_state, full_state)]
  print(f"fp32 restatements (local two-pass, full): E_0 off by {energy_errors}, the vector by {state_errors}, "
        f"{local_restarts} and {full_restarts} restart(s)")
  energy_bar, state_bar = C.MARGIN * max(energy_errors), C.MARGIN * max(state_errors)
  ops = _tfim_operators(n)
  energy, state, residual, restarts = inference.ground_state(ops, weights=WEIGHTS, store_basis=False)
  assert isinstance(energy, float) and state.shape == (1 << n,) and state.dtype == torch.complex64
  _close("E_0", energy, d.evals[0], energy_bar)
  aligned = K.align(_np(state).astype(np.complex128), want)
  _close("ground vector", np.stack([aligned.real, aligned.imag]), np.stack([want.real, want.imag]), state_bar)
  print(f"residual {residual:.3e}  tolerance R {2.0**-20 * radius:.3e}  restarts {restarts}")
  assert 0 <= residual <= 2.0**-20 * radius and restarts <= 4
  source = data.StateVectorData.ground_state(ops, weights=WEIGHTS, store_basis=False)
  assert source.states.shape == (1, 1 << n) and source.weights.tolist() == [1.0] and source.num_qubits == n
  assert _same(source.states[0].to(state.device), state)


# ---- 5. breakdown and zero starts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 10])
def test_a_basis_state_under_a_diagonal_hamiltonian_replays_its_first_row_alone(n):
  m, index = 5, 5
  total_z = [[(1.0, 0, 1 << q) for q in range(n)]]
  start = torch.from_numpy(T.basis_states(n)[[index]].astype(np.complex64)).cuda()
  eng = _engine(n, total_z)
  alpha, beta, lengths, recurrence, _ = eng.krylov_tridiagonal(start, m)
  assert lengths.cpu().tolist() == [1]
  assert alpha[0, 0].item() == n - 2 * bin(index).count("1") and (alpha[0, 1:] == 0).all() and (beta == 0).all()
  out = eng.krylov_replay(start, beta, lengths, recurrence, _one_hot(1, range(m), m))
  assert _same(out[:, 0], start) and (torch.view_as_real(out[:, 1:]) == 0).all()
  coef = torch.from_numpy(np.random.default_rng(n).normal(size=(1, 2, m, 2)).astype(np.float32)).view(torch.complex64)[..., 0]
  out = eng.krylov_replay(start, beta, lengths, recurrence, coef)  # coef_0 v_0, and exact zeros from every later row
  want = torch.zeros((1, 2, 1 << n), dtype=torch.complex64)
  want[0, :, index] = coef[0, :, 0]
  assert _same(out.cpu(), want)


def test_a_zero_state_has_length_zero_zero_outputs_and_leaves_its_neighbours_alone():
  n, m = 10, 6
  starts = C.starts(n).copy()
  eng = _engine(n, C.tfim_parts(n), chunk_states=2)
  coef = torch.from_numpy(np.random.default_rng(6).normal(size=(3, 2, m, 2)).astype(np.float32)).view(torch.complex64)[..., 0]
  whole = eng.krylov_tridiagonal(torch.from_numpy(starts), m, WEIGHTS)
  whole_out = eng.krylov_replay(torch.from_numpy(starts), whole[1], whole[2], whole[3], coef, WEIGHTS)
  starts[1] = 0
  alpha, beta, lengths, recurrence, norms = eng.krylov_tridiagonal(torch.from_numpy(starts), m, WEIGHTS)
  assert lengths.cpu().tolist() == [m, 0, m] and norms[1] == 0
  assert (alpha[1] == 0).all() and (beta[1] == 0).all() and (torch.view_as_real(recurrence[1]) == 0).all()
  out = eng.krylov_replay(torch.from_numpy(starts), beta, lengths, recurrence, coef, WEIGHTS)
  assert (torch.view_as_real(out[1]) == 0).all()
  for u in (0, 2):
    assert _same(alpha[u], whole[0][u]) and _same(beta[u], whole[1][u]) and _same(recurrence[u], whole[3][u])
    assert _same(out[u], whole_out[u])
  space = inference.krylov_space(_tfim_operators(n), torch.from_numpy(starts), m, weights=WEIGHTS, store_basis=False)
  states, logs = space.evolve(0.5, 0)
  assert (states[1] == 0).all() and logs[1] == -np.inf and torch.isfinite(logs[[0, 2]]).all() and torch.isfinite(torch.view_as_real(states)).all()


# ---- 6. bits -----------------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_runs_chunks_or_company():
  n, m = 10, 12
  starts, _, first = _routes(n, m)
  rng = np.random.default_rng(7)
  coef = torch.from_numpy((rng.normal(size=(3, 9, m)) + 1j * rng.normal(size=(3, 9, m))).astype(np.complex64))
  eng = _engine(n, C.tfim_parts(n))
  replay = lambda engine, rows, pass_one, c: engine.krylov_replay(rows, pass_one[1], pass_one[2], pass_one[3], c, WEIGHTS)
  first_out = replay(eng, starts, first, coef)
  again = eng.krylov_tridiagonal(starts, m, WEIGHTS)
  assert all(_same(a, b) for a, b in zip(first, again)) and _same(first_out, replay(eng, starts, again, coef))
  for chunk in (1, 2, 3):
    other_engine = _engine(n, C.tfim_parts(n), chunk_states=chunk)
    other = other_engine.krylov_tridiagonal(starts, m, WEIGHTS)
    assert all(_same(a, b) for a, b in zip(first, other)), chunk
    assert _same(first_out, replay(other_engine, starts, other, coef)), chunk
  for u in range(3):
    alone = eng.krylov_tridiagonal(starts[u:u + 1], m, WEIGHTS)
    assert all(_same(a[u:u + 1], b) for a, b in zip(first, alone))
    assert _same(first_out[u:u + 1], replay(eng, starts[u:u + 1], alone, coef[u:u + 1]))


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_buffer_untouched():
  n, m, num, outputs = 6, 4, 3, 2
  eng = _engine(n, C.tfim_parts(n))
  lib, h = eng._lib, eng._h  # pylint: disable=protected-access
  states = torch.from_numpy(T.random_states(num, n, 3)).cuda()
  alpha = torch.full((num, m), 7.0, dtype=torch.float64, device="cuda")
  beta, lengths = alpha.clone(), torch.full((num,), 7, dtype=torch.int32, device="cuda")
  recurrence = torch.full((num, m, 2), 7.0, dtype=torch.complex64, device="cuda")
  coef = torch.ones((num, outputs, m), dtype=torch.complex64, device="cuda")
  out = torch.full((num + 1, outputs, 1 << n), 7.0, dtype=torch.complex64, device="cuda")
  before = states.clone()

  def one(handle=h, start=states.data_ptr(), count=num, steps=m, a=alpha.data_ptr(), b=beta.data_ptr(), k=lengths.data_ptr(),
          r=recurrence.data_ptr()):
    return lib.qhbm_krylov_tridiagonal(handle, start, count, None, steps, a, b, k, r, None)

  def two(handle=h, start=states.data_ptr(), count=num, steps=m, b=beta.data_ptr(), k=lengths.data_ptr(), r=recurrence.data_ptr(),
          c=coef.data_ptr(), s=outputs, dst=out.data_ptr()):
    return lib.qhbm_krylov_replay(handle, start, count, None, steps, b, k, r, c, s, dst, None)

  def refused(rc, text, handle=h):
    message = lib.qhbm_last_error(handle).decode()
    assert rc != 0 and text in message, message
    torch.cuda.synchronize()
    assert _same(states, before) and (alpha == 7.0).all() and (beta == 7.0).all() and (lengths == 7).all()
    assert (recurrence == 7.0).all() and (out == 7.0).all() and (coef == 1.0).all()

  bare = _engine(n, None)
  for call in (one, two):
    refused(call(steps=0), "m must be in [1, 1024]")
    refused(call(steps=1025), "m must be in [1, 1024]")
    refused(call(count=0), "U must be positive")
    refused(call(count=-3), "U must be positive")
    refused(call(handle=bare._h), "qhbm_set_observables has not been called", bare._h)  # pylint: disable=protected-access
    refused(call(start=None), "d_start_states is NULL")
    refused(call(b=None), "d_beta is NULL")
    refused(call(k=None), "d_lengths is NULL")
    refused(call(r=None), "d_recurrence is NULL")
    refused(call(start=states.data_ptr() + 8, count=2), "16-byte aligned")
    refused(call(b=beta.data_ptr() + 4), "8-byte aligned")
    refused(call(k=lengths.data_ptr() + 2), "4-byte aligned")
    refused(call(r=recurrence.data_ptr() + 4), "8-byte aligned")
  refused(one(a=None), "d_alpha is NULL")
  refused(one(a=alpha.data_ptr() + 4), "8-byte aligned")
  refused(two(s=0), "S must be at least 1")
  refused(two(s=-1), "S must be at least 1")
  refused(two(c=None), "d_coef is NULL")
  refused(two(dst=None), "d_out_states is NULL")
  refused(two(c=coef.data_ptr() + 4), "8-byte aligned")
  refused(two(dst=out.data_ptr() + 8), "16-byte aligned")
  refused(two(dst=states.data_ptr()), "d_out_states overlaps d_start_states")
  refused(two(start=out.data_ptr() + 16 * (1 << n)), "d_out_states overlaps d_start_states")
  with pytest.raises(E.EngineError, match="qhbm_set_observables has not been called"):
    bare.krylov_tridiagonal(states, m)
  with pytest.raises(ValueError, match="num_steps"):
    eng.krylov_tridiagonal(states, 0)
  with pytest.raises(ValueError, match="coef must have shape"):
    eng.krylov_replay(states, beta, lengths, recurrence, coef[:, :0])
  with pytest.raises(E.EngineError, match="S must be at least 1"):
    eng.describe_krylov_stream(num, m, 0)
  # the engine is as good as before
  fresh = _engine(n, C.tfim_parts(n))
  got, want = eng.krylov_tridiagonal(states, m, WEIGHTS), fresh.krylov_tridiagonal(states, m, WEIGHTS)
  assert all(_same(a, b) for a, b in zip(got, want))
  stored = fresh.krylov_basis(states, m, WEIGHTS, False)
  assert _same(got[0], stored[1]) and _same(got[1], stored[2]) and _same(got[2], stored[3])
  picks = _one_hot(num, range(m), m)
  assert _same(eng.krylov_replay(states, got[1], got[2], got[3], picks, WEIGHTS).transpose(0, 1), stored[0])
