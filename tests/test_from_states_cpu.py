"""Circuits that start from caller-supplied states, the parts that need no GPU: the complex128 restatement the GPU
tests compare with (`tests/from_states_ref.py`) against central differences and against the oracle's basis-state
functions; the dense-start plans of a planning-only engine; `StateVectorData.from_density_matrix`."""
import os

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import data
from tests import from_states_ref as R

needs_library = pytest.mark.skipif(not os.path.exists(E.LIB_PATH),
                                   reason="engine library not built (run __graft_entry__.build())")


def _case(n, layers, seed, num=3):
  rng = np.random.default_rng(seed)
  gates, names = O.hea_gates(n, layers, "fs")
  params = rng.uniform(-1, 1, len(names))
  ops = [O.tfim_ring_op(n), O.random_pauli_op(n, 12, seed + 1)]
  upstream = rng.normal(size=(num, len(ops)))
  return gates, params, ops, upstream


@pytest.mark.parametrize("n", [3, 6])
def test_restatement_vjp_matches_central_differences(n):
  """Step 1e-5 in float64, agreement 1e-7 relative to the largest gradient entry."""
  gates, params, ops, upstream = _case(n, 2, 10 + n)
  states = R.random_states(3, n, 20 + n)
  _, grad = R.values_and_vjp(n, gates, params, states, ops, upstream)
  step = 1e-5
  numeric = np.zeros_like(grad)
  for p in range(len(params)):
    hi, lo = params.copy(), params.copy()
    hi[p] += step
    lo[p] -= step
    numeric[p] = np.sum(upstream * (R.values(n, gates, hi, states, ops) - R.values(n, gates, lo, states, ops))) / (2 * step)
  assert np.abs(grad - numeric).max() <= 1e-7 * np.abs(grad).max()


@pytest.mark.parametrize("n", [3, 6])
def test_restatement_on_basis_states_is_the_oracle(n):
  gates, params, ops, upstream = _case(n, 2, 30 + n, num=4)
  bits = np.random.default_rng(n).integers(0, 2, size=(4, n)).astype(np.int8)
  vals, rows = R.values_and_rows(n, gates, params, R.basis_states(bits), ops, upstream)
  want_vals, want_jac = O.expectation_jacobian(n, gates, params, bits, ops)
  np.testing.assert_allclose(vals, want_vals, rtol=0, atol=1e-12)
  np.testing.assert_allclose(vals, O.expectation(n, gates, params, bits, ops), rtol=0, atol=1e-12)
  np.testing.assert_allclose(rows, np.einsum("bt,btp->bp", upstream, want_jac), rtol=0, atol=1e-12)
  want_states = np.stack([O.simulate(n, gates, params, b).reshape(-1) for b in bits])
  np.testing.assert_allclose(R.final_states(n, gates, params, R.basis_states(bits)), want_states, rtol=0, atol=1e-12)


def test_restatement_is_quadratic_in_the_states():
  n = 3
  gates, params, ops, upstream = _case(n, 1, 5)
  states = R.random_states(3, n, 6)
  v1, g1 = R.values_and_vjp(n, gates, params, states, ops, upstream)
  v3, g3 = R.values_and_vjp(n, gates, params, 3.0 * states, ops, upstream)
  np.testing.assert_allclose(v3, 9.0 * v1, rtol=1e-13)
  np.testing.assert_allclose(g3, 9.0 * g1, rtol=1e-12, atol=1e-13)


@needs_library
def test_dense_start_plans_prune_nothing_and_leave_the_basis_plans_alone():
  eng = E.Engine(device=None)
  gates, names = O.hea_gates(20, 16)
  eng.set_circuit(20, gates, len(names))
  eng.set_observables([O.xxz_chain_op(20)])
  before, builds = eng.describe_schedule(), eng.plan_builds()
  assert "[basis tile only]" in before or "[zero-fill]" in before
  dense = eng.describe_schedule_from_states()
  assert "forward plan" in dense and "adjoint" in dense
  assert "[zero-fill]" not in dense and "[basis tile only]" not in dense
  assert "[loads caller states]" in dense
  assert "stale-local-bits" not in dense and "moves-local-bits" not in dense
  for line in dense.splitlines():  # no wave of any adjoint round is declared dead
    if " dead=" in line:
      assert set(line.split(" dead=")[1].split()[0].split(",")) == {"0"}, line
  assert eng.describe_schedule() == before
  assert eng.plan_builds() == builds
  assert eng.describe_schedule_from_states() == dense  # cached: same text, and still no basis-state plan built
  assert eng.plan_builds() == builds


@needs_library
def test_dense_start_plans_follow_the_setters():
  eng = E.Engine(device=None)
  gates, names = O.hea_gates(12, 3)
  eng.set_circuit(12, gates, len(names))
  eng.set_observables([O.tfim_ring_op(12)])
  eng.set_option("tile_qubits", 10)
  eng.set_option("adjoint_tile_qubits", 10)
  dense = eng.describe_schedule_from_states()
  assert "tile_bits=10" in dense
  eng.set_option("tile_qubits", 0)
  eng.set_option("adjoint_tile_qubits", 0)
  assert "tile_bits=12" in eng.describe_schedule_from_states()
  frozen = [False] * 24 + [True] * (len(names) - 24)
  eng.set_gradient_mask(frozen)
  masked = eng.describe_schedule_from_states()
  eng.set_gradient_mask(None)
  assert eng.describe_schedule_from_states() != masked
  gates5, names5 = O.hea_gates(5, 1)
  eng.set_circuit(5, gates5, len(names5))
  assert "n=5 " in eng.describe_schedule_from_states()


@needs_library
def test_from_states_without_a_device_fails_loudly():
  eng = E.Engine(device=None)
  gates, names = O.hea_gates(4, 2)
  eng.set_circuit(4, gates, len(names))
  eng.set_observables([O.tfim_ring_op(4)])
  states = torch.zeros((1, 16), dtype=torch.complex64)
  with pytest.raises(E.EngineError, match="no CPU fallback|no device"):
    eng.expectation_from_states(states, np.zeros(len(names), np.float32))
  with pytest.raises(E.EngineError, match="no CPU fallback|no device"):
    eng.expectation_vjp_from_states(states, np.zeros(len(names), np.float32), np.ones((1, 1), np.float32))
  with pytest.raises(E.EngineError, match="no CPU fallback|no device"):
    eng.statevector_from_states(states, np.zeros(len(names), np.float32))


def _dense_op(n, op):
  eye = np.eye(1 << n, dtype=np.complex128)
  return np.stack([O.apply_op(eye[j].reshape((2,) * n), op).reshape(-1) for j in range(1 << n)], axis=1)


def _thermal(n, beta):
  h = _dense_op(n, O.tfim_ring_op(n))
  w, v = np.linalg.eigh(h)
  p = np.exp(-beta * (w - w.min()))
  return (v * (p / p.sum())) @ v.conj().T


def test_from_density_matrix_reproduces_a_thermal_state():
  sigma = _thermal(3, 1.0)
  source = data.StateVectorData.from_density_matrix(torch.from_numpy(sigma))
  st, w = source.states.numpy(), source.weights.numpy()
  assert st.shape == (8, 8) and source.num_qubits == 3
  np.testing.assert_allclose(np.einsum("m,mi,mj->ij", w, st, st.conj()), sigma, rtol=0, atol=1e-12)
  assert source.states.dtype == torch.complex128  # kept in the precision of the eigendecomposition


def test_from_density_matrix_drops_a_zero_eigenvalue():
  rng = np.random.default_rng(3)
  vecs = np.linalg.qr(rng.normal(size=(8, 8)) + 1j * rng.normal(size=(8, 8)))[0]
  probs = np.array([0.5, 0.3, 0.2, 0, 0, 0, 0, 0.0])
  sigma = (vecs * probs) @ vecs.conj().T
  source = data.StateVectorData.from_density_matrix(torch.from_numpy(sigma))
  assert source.states.shape == (3, 8)
  np.testing.assert_allclose(np.sort(source.weights.numpy()), [0.2, 0.3, 0.5], rtol=0, atol=1e-12)
  st, w = source.states.numpy(), source.weights.numpy()
  np.testing.assert_allclose(np.einsum("m,mi,mj->ij", w, st, st.conj()), sigma, rtol=0, atol=1e-12)


def test_state_vector_data_checks_its_arguments():
  with pytest.raises(ValueError):
    data.StateVectorData(torch.zeros((2, 6), dtype=torch.complex64))
  with pytest.raises(ValueError):
    data.StateVectorData(torch.zeros((2, 8), dtype=torch.float32))
  with pytest.raises(ValueError):
    data.StateVectorData(torch.zeros((2, 8), dtype=torch.complex64), weights=[1.0])
  source = data.StateVectorData(torch.zeros((4, 8), dtype=torch.complex128))
  np.testing.assert_allclose(source.weights.numpy(), 0.25)
