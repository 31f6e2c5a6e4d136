"""Matrix-free thermal targets on the GPU (`qhbm_apply_observables`, `qhbm_evolve_states`, `qhbm_random_states`,
`inference.thermal_ensemble`, `data.StateVectorData.thermal`) against tests/thermal_ref.py and its `eigh` route.

Tolerances
  apply      |delta| <= (T + 2) 2^-24 R max|phi| per amplitude, T the number of Pauli terms: the fp32 bound of a T-term sum.
  evolution  8 x the error of an fp32 run of the restatement (`thermal_ref.evolve(dtype=float32)`) against its float64 run
             on the cases of test 2, the largest over those cases (the kernels add their terms in another order than the
             restatement, so a margin of the 2 sqrt(T) kind is expected).  Measured on the CPU: the fp32 restatement is off
             by 1.21e-7 (normalised states) and 5.87e-7 (log norms), so the bars are 9.7e-7 and 4.7e-6; `_bars()` recomputes
             both from the restatement and asserts that they are these.  The restatement's float64 run itself is within
             2e-9 / 5e-9 of `eigh` on these cases (the series is cut at 2^-30).
             On an MI355X the engine's largest errors on these cases were 1.9e-7 (states) and 4.2e-7 (log norms).
Every comparison prints its largest error beside its bar before it asserts.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir, models
from tests import thermal_ref as T
from tests.test_host_api import hea_circuit

pytestmark = pytest.mark.gpu

WEIGHTS = [1.0, 0.7]
BETAS = (0.5, 4.0)


def tfim_parts(n):
  op = O.tfim_ring_op(n)
  return [op[:n], op[n:]]


def _engine(n, ops, **options):
  eng = E.Engine(0)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(n, [], 0)
  if ops:
    eng.set_observables(ops)
  return eng


def _close(what, got, want, bar):
  got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
  err = np.abs(got - want)
  print(f"{what}: max error {np.max(err, initial=0.0):.3e}  bar {np.min(bar):.3e}")
  assert np.isfinite(got).all(), what
  assert (err <= bar).all(), (what, float(np.max(err)), float(np.min(bar)))


def _starts(n):
  """Test 2's start states: n = 3 all 8 basis states; n = 10 two random-sign states and one basis state."""
  if n == 3:
    return T.basis_states(n).astype(np.complex64)
  return np.concatenate([T.random_states(2, n, 21), T.basis_states(n)[[5]].astype(np.complex64)])


@functools.lru_cache(maxsize=None)
def _case(n, beta):
  """(starts, eigh states, eigh log norms, fp32-restatement error of states, of log norms) of one case of test 2."""
  ops, starts = tfim_parts(n), _starts(n)
  want, want_log = T.Dense(n, ops, WEIGHTS).evolve(starts.astype(np.complex128), beta, 0)
  s64, l64 = T.evolve(n, ops, starts, beta, 0, WEIGHTS)
  s32, l32 = T.evolve(n, ops, starts, beta, 0, WEIGHTS, dtype=np.float32)
  return starts, want, want_log, float(np.abs(s32 - s64).max()), float(np.abs(l32 - l64).max())


@functools.lru_cache(maxsize=None)
def _bars():
  """(state bar, log-norm bar): 8 x the fp32 restatement's largest error over the cases of test 2."""
  cases = [_case(n, beta) for n in (3, 10) for beta in BETAS]
  state_err, log_err = max(c[3] for c in cases), max(c[4] for c in cases)
  print(f"fp32 restatement against float64: states {state_err:.3e} log norms {log_err:.3e}")
  assert 0.5e-7 < state_err < 2.5e-7 and 2e-7 < log_err < 1.2e-6  # (the docstring's 1.21e-7 and 5.87e-7, libm aside)
  return 8.0 * state_err, 8.0 * log_err


# ---- 1. apply -------------------------------------------------------------------------------------------------------------------------
def _check_apply(n, ops, weights, options):
  rng = np.random.default_rng(100 + n)
  states = (rng.normal(size=(3, 1 << n)) + 1j * rng.normal(size=(3, 1 << n))).astype(np.complex64)
  eng = _engine(n, ops, chunk_states=2, **options)
  given = torch.from_numpy(states).cuda()
  before = given.clone()
  got = eng.apply_observables(given, weights)
  assert torch.equal(torch.view_as_real(given), torch.view_as_real(before))
  want = T.apply_h(n, ops, states.astype(np.complex128), weights)
  terms = sum(len(op) for op in ops)
  bar = (terms + 2) * 2.0**-24 * T.radius(n, ops, weights) * np.abs(states).max(axis=1, keepdims=True)
  _close(f"apply n={n} {options} real", got.real, want.real, bar)
  _close(f"apply n={n} {options} imag", got.imag, want.imag, bar)


@pytest.mark.parametrize("n", [3, 10, 12])
def test_apply_tfim_as_two_weighted_observables(n):
  _check_apply(n, tfim_parts(n), WEIGHTS, {})


@pytest.mark.parametrize("kernel", [0, 1])
def test_apply_random_strings_with_y(kernel):
  n = 14
  op = O.random_pauli_op(n, 40, 9)
  assert any(bin(x & z).count("1") % 2 for _, x, z in op) and any(x >> 3 for _, x, z in op)
  _check_apply(n, [op], None, {"observable_kernel": kernel})


# ---- 2. imaginary time ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("n", [3, 10])
def test_imaginary_time_against_eigh(n, beta):
  starts, want, want_log, _, _ = _case(n, beta)
  state_bar, log_bar = _bars()
  eng = _engine(n, tfim_parts(n))
  plan = eng.describe_evolution(beta, 0, WEIGHTS)
  assert plan["steps"] == T.evolution_plan(n, tfim_parts(n), beta, 0, WEIGHTS)["steps"] and (plan["steps"] > 1) == (beta > 0.5 or n == 10)
  got, log_norms = eng.evolve_states(torch.from_numpy(starts), beta, 0, WEIGHTS)
  assert log_norms.dtype == torch.float64
  _close(f"n={n} beta={beta} states real", got.real, want.real, state_bar)
  _close(f"n={n} beta={beta} states imag", got.imag, want.imag, state_bar)
  _close(f"n={n} beta={beta} log norms", log_norms, want_log, log_bar)
  # states as given: three times the state, log 3 more
  scaled, scaled_log = eng.evolve_states(torch.from_numpy(3.0 * starts), beta, 0, WEIGHTS)
  _close(f"n={n} beta={beta} scaled input, states", torch.view_as_real(scaled), np.stack([want.real, want.imag], -1), state_bar)
  _close(f"n={n} beta={beta} scaled input, log norms", scaled_log, want_log + np.log(3.0), log_bar)


def test_a_state_of_norm_zero_gives_zeros_and_minus_infinity():
  n = 10
  starts = _starts(n).copy()
  starts[1] = 0
  got, log_norms = _engine(n, tfim_parts(n)).evolve_states(torch.from_numpy(starts), 0.5, 0, WEIGHTS)
  assert (got[1] == 0).all() and log_norms[1] == -np.inf
  assert torch.isfinite(log_norms[[0, 2]]).all() and torch.isfinite(torch.view_as_real(got)).all()


# ---- 3. exactness with a basis start ----------------------------------------------------------------------------------------------------------
def _tfim_sum(n):
  qubits = ir.GridQubit.rect(1, n)
  terms = [ir.PauliString(ir.PX(q), coefficient=-1.0) for q in qubits]
  terms += [ir.PauliString(ir.PZ(qubits[i]), ir.PZ(qubits[(i + 1) % n]), coefficient=-1.0) for i in range(n)]
  total = ir.PauliSum(terms)
  assert total.masks(qubits) == [tuple(t) for t in O.tfim_ring_op(n)]
  return total, qubits


@pytest.mark.parametrize("n", [4, 10])
def test_basis_start_is_exact(n):
  beta = 1.0
  state_bar, log_bar = _bars()
  ham, _ = _tfim_sum(n)
  dense = T.Dense(n, [O.tfim_ring_op(n)])
  ens = inference.thermal_ensemble(ham, beta, start="basis")
  assert ens.states.shape == (1 << n, 1 << n) and ens.log_weights.dtype == torch.float64
  radius = T.radius(n, [O.tfim_ring_op(n)])
  # log Z = logsumexp of 2^n log weights, each 2 x a log norm; <H>: test 2's state tolerance scaled by R >= ||H||
  _close(f"n={n} log Z", ens.log_partition(), T.logsumexp(-beta * dense.evals), 2 * log_bar)
  energy_bar = state_bar * radius
  _close(f"n={n} <H>", ens.energy(), dense.energy(beta), energy_bar)
  _close(f"n={n} entropy", ens.entropy(), dense.entropy(beta), beta * energy_bar + 2 * log_bar)
  if n == 4:
    states = ens.states.cpu().numpy().astype(np.complex128)
    rho = np.einsum("m,mi,mj->ij", ens.weights.cpu().numpy(), states, states.conj())
    # sum_m w_m |phi_m><phi_m|: each entry a convex combination of products of two amplitudes <= 1, either off by the state
    # bar; the weights sum to one, each off by 2 x the log-norm bar relative
    _close("n=4 rho", np.stack([rho.real, rho.imag]), np.stack([dense.thermal_state(beta).real, dense.thermal_state(beta).imag]),
           2 * state_bar + 4 * log_bar)
  with pytest.raises(ValueError, match="refused above 14 qubits"):
    inference.thermal_ensemble(_tfim_sum(15)[0], beta, start="basis")


# ---- 4. bits ----------------------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_runs_chunks_or_company():
  n, beta = 10, 4.0
  starts = torch.from_numpy(_starts(n)).cuda()
  eng = _engine(n, tfim_parts(n))
  a, la = eng.evolve_states(starts, beta, 0, WEIGHTS)
  b, lb = eng.evolve_states(starts, beta, 0, WEIGHTS)
  assert torch.equal(torch.view_as_real(a), torch.view_as_real(b)) and torch.equal(la, lb)
  one = _engine(n, tfim_parts(n), chunk_states=1)
  c, lc = one.evolve_states(starts, beta, 0, WEIGHTS)
  assert torch.equal(torch.view_as_real(a), torch.view_as_real(c)) and torch.equal(la, lc)
  for u in range(3):
    d, ld = eng.evolve_states(starts[u:u + 1], beta, 0, WEIGHTS)
    assert torch.equal(torch.view_as_real(a[u:u + 1]), torch.view_as_real(d)) and torch.equal(la[u:u + 1], ld)
  r1, _ = eng.evolve_states(starts, 1.3, 1, WEIGHTS)
  r2, _ = one.evolve_states(starts, 1.3, 1, WEIGHTS)
  assert torch.equal(torch.view_as_real(r1), torch.view_as_real(r2))


# ---- 5. real time -----------------------------------------------------------------------------------------------------------------------------
def test_real_time_against_eigh_and_back():
  n, t = 10, 1.3
  state_bar, _ = _bars()
  starts = _starts(n) * np.array([1.0, 2.0, 0.5], np.float32)[:, None]
  norms = np.linalg.norm(starts.astype(np.complex128), axis=1)
  eng = _engine(n, tfim_parts(n))
  got, none = eng.evolve_states(torch.from_numpy(starts), t, 1, WEIGHTS)
  assert none is None
  want = T.Dense(n, tfim_parts(n), WEIGHTS).evolve(starts.astype(np.complex128), t, 1)[0]
  bar = state_bar * norms[:, None]
  _close("real time, real part", got.real, want.real, bar)
  _close("real time, imaginary part", got.imag, want.imag, bar)
  _close("real time norms", torch.linalg.norm(got.to(torch.complex128), dim=1), norms, state_bar * norms)
  back, _ = eng.evolve_states(got, -t, 1, WEIGHTS)
  _close("forward and back", torch.view_as_real(back), np.stack([starts.real, starts.imag], -1), 2 * bar[:, :, None])


# ---- 6. random states -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 10, 13])
def test_random_states_equal_the_restatement(n):
  got = E.random_states(3, n, 0xDEADBEEF12345, device="cuda:0")
  want = T.random_states(3, n, 0xDEADBEEF12345)
  assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
  tail = E.random_states(1, n, 0xDEADBEEF12345, first_state=2, device="cuda:0")
  assert torch.equal(torch.view_as_real(tail), torch.view_as_real(got[2:]))
  norms = torch.linalg.norm(got.to(torch.complex128), dim=1).cpu().numpy()
  assert np.abs(norms - 1.0).max() <= 2.0**-20


# ---- 7. the ensemble on the restatement's own vectors -----------------------------------------------------------------------------------------
def test_ensemble_matches_the_restatement_on_the_same_vectors():
  n, num, beta, seed = 10, 16, 1.0, 77
  state_bar, log_bar = _bars()
  ham, qubits = _tfim_sum(n)
  ops = [O.tfim_ring_op(n)]
  ens = inference.thermal_ensemble(ham, beta, num_vectors=num, seed=seed)
  assert ens.states.shape == (num, 1 << n) and ens.qubits == sorted(qubits)
  starts = T.random_states(num, n, seed)
  states, lw = T.thermal_ensemble(n, ops, beta, starts)
  radius = T.radius(n, ops)
  _close("log weights", ens.log_weights, lw, 2 * log_bar)
  _close("log Z", ens.log_partition(), T.log_partition(lw, n, "random"), 2 * log_bar)
  _close("<H>", ens.energy(), T.energy(n, ops, states, lw)[0], state_bar * radius)  # (test 2's tolerance scaled by R)
  source = ens.data()
  assert isinstance(source, data.StateVectorData) and source.num_qubits == n
  np.testing.assert_allclose(source.weights.sum().item(), 1.0, atol=1e-12)


# ---- 8. through the loss ----------------------------------------------------------------------------------------------------------------------
def _set(param, values):
  with torch.no_grad():
    param.copy_(torch.as_tensor(np.asarray(values), dtype=torch.float32))


def test_qmhl_from_thermal_data_equals_qmhl_from_the_dense_thermal_state():
  n, layers, beta = 4, 2, 1.0
  ham, qubits = _tfim_sum(n)
  sigma = T.Dense(n, [O.tfim_ring_op(n)]).thermal_state(beta)
  rng = np.random.default_rng(11)
  energy = models.KOBE(list(range(n)), 2)
  energy.build([None, n])
  _set(energy.post_process[0].kernel, rng.uniform(-0.5, 0.5, tuple(energy.post_process[0].kernel.shape)))
  circ = models.DirectQuantumCircuit(hea_circuit(qubits, layers, "th"))
  _set(circ.trainable_variables[0], rng.uniform(-1, 1, tuple(circ.trainable_variables[0].shape)))
  model = inference.QHBM(inference.AnalyticEnergyInference(energy, 16, initial_seed=1), inference.AnalyticQuantumInference(circ))
  variables = [energy.post_process[0].kernel, circ.trainable_variables[0]]

  def loss_and_grads(source):
    for v in variables:
      v.grad = None
    loss = inference.qmhl(source, model)
    loss.backward()
    return float(loss.detach()), [v.grad.detach().cpu().numpy().copy() for v in variables]

  want_loss, want_grads = loss_and_grads(data.StateVectorData.from_density_matrix(torch.from_numpy(sigma), qubits=qubits))
  got_loss, got_grads = loss_and_grads(data.StateVectorData.thermal(ham, beta, start="basis"))
  _close("qmhl loss", got_loss, want_loss, 2e-5)  # (the bars of tests/test_from_states_gpu.py's density-matrix case)
  for name, a, b in zip(("theta", "phi"), got_grads, want_grads):
    _close("qmhl d/d " + name, a, b, 2e-4)


# ---- 9. refusals and the trivial case -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_buffer_untouched_and_zero_weights_are_the_identity():
  n = 6
  eng = _engine(n, tfim_parts(n))
  lib, h = eng._lib, eng._h  # pylint: disable=protected-access
  states = torch.from_numpy(2.0 * T.random_states(3, n, 3)).cuda()
  before = states.clone()
  logs = torch.full((3,), 7.0, dtype=torch.float64, device="cuda")
  same = lambda: torch.equal(torch.view_as_real(states), torch.view_as_real(before)) and bool((logs == 7.0).all())

  def refused(rc, text):
    message = lib.qhbm_last_error(h).decode()
    assert rc != 0 and text in message, message
    torch.cuda.synchronize()
    assert same()

  bare = _engine(n, None)
  rc = bare._lib.qhbm_evolve_states(bare._h, states.data_ptr(), 3, None, 1.0, 0, logs.data_ptr(), None)  # pylint: disable=protected-access
  assert rc != 0 and "qhbm_set_observables has not been called" in bare._lib.qhbm_last_error(bare._h).decode()  # pylint: disable=protected-access
  rc = bare._lib.qhbm_apply_observables(bare._h, states.data_ptr(), 3, None, before.data_ptr(), None)  # pylint: disable=protected-access
  assert rc != 0 and "qhbm_set_observables has not been called" in bare._lib.qhbm_last_error(bare._h).decode()  # pylint: disable=protected-access
  refused(lib.qhbm_evolve_states(h, states.data_ptr(), 0, None, 1.0, 0, logs.data_ptr(), None), "U must be positive")
  refused(lib.qhbm_evolve_states(h, states.data_ptr(), -2, None, 1.0, 0, logs.data_ptr(), None), "U must be positive")
  refused(lib.qhbm_evolve_states(h, states.data_ptr(), 3, None, float("nan"), 0, logs.data_ptr(), None), "tau is not finite")
  refused(lib.qhbm_evolve_states(h, states.data_ptr(), 3, None, float("inf"), 1, None, None), "tau is not finite")
  refused(lib.qhbm_evolve_states(h, states.data_ptr(), 3, None, -0.5, 0, logs.data_ptr(), None), "tau < 0")
  refused(lib.qhbm_evolve_states(h, states.data_ptr(), 3, None, 0.5, 1, logs.data_ptr(), None), "d_log_norms must be NULL")
  refused(lib.qhbm_evolve_states(h, None, 3, None, 0.5, 0, logs.data_ptr(), None), "d_states is NULL")
  refused(lib.qhbm_evolve_states(h, states.data_ptr() + 8, 2, None, 0.5, 0, logs.data_ptr(), None), "16-byte aligned")
  with pytest.raises(E.EngineError, match="tau < 0"):
    eng.evolve_states(states, -1.0, 0)
  with pytest.raises(E.EngineError, match="qhbm_set_observables has not been called"):
    bare.evolve_states(states, 1.0, 0)
  # all weights zero: H = 0, the states and log ||phi|| come back unchanged
  out, log_norms = eng.evolve_states(states, 1.0, 0, [0.0, 0.0], in_place=True)
  assert out.data_ptr() == states.data_ptr() and torch.equal(torch.view_as_real(states), torch.view_as_real(before))
  np.testing.assert_allclose(log_norms.cpu().numpy(), np.log(2.0), atol=1e-6)
  out, none = eng.evolve_states(states, 1.0, 1, [0.0, 0.0], in_place=True)
  assert none is None and torch.equal(torch.view_as_real(states), torch.view_as_real(before))
  # the engine is as good as before, the installed circuit is not applied, and a retained batch is dropped
  gates, names = O.hea_gates(n, 1, "th")
  eng.set_circuit(n, gates, len(names))
  eng.set_observables(tfim_parts(n))
  eng.expectation(np.zeros((2, n), np.int8), np.full(len(names), 0.3, np.float32), retain=True)
  assert eng.retained_states() == 2
  got, _ = eng.evolve_states(states, 0.5, 0, WEIGHTS)
  assert eng.retained_states() == 0
  want = T.evolve(n, tfim_parts(n), before.cpu().numpy(), 0.5, 0, WEIGHTS)[0]
  _close("after the refusals", torch.view_as_real(got), np.stack([want.real, want.imag], -1), _bars()[0])
