"""qhbm_sample_parities_states / qhbm_sample_parities on the GPU.

States entry: EXACT integer equality with the flat numpy definition (tests/sample_parity_ref.py restated_sums) on dyadic
states, where every partial sum is exact in float64 in every order of additions (n + 24 <= 53), so the equality holds for
any correct kernel -- no tolerance.
Engine entry: bit-identical under other chunkings and a small workspace budget; against the complex128 oracle with the
thresholds of tests/test_sampling_exact_gpu.py (a shot the restatement may place either way moves a sum by at most 2).
Mirror: SampledQuantumInference(pauli_estimator="parities") at the reference's tolerance and against the analytic
inference at 18 qubits, where the default route would materialise the shots."""
import itertools
import math

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import inference, ir, models
from tests import sample_parity_ref as R
from tests.test_host_api import hea_circuit
from tests.test_host_gpu import _jacobian, _set
from tests.test_sampling_exact_gpu import SEED, Ref, _delta, _dense_case, _engine, _gpu_ref, _restated_counts

pytestmark = pytest.mark.gpu

ODD_SHOTS = 65539


def _gpu(states):
  return torch.from_numpy(np.ascontiguousarray(states)).cuda()


def _check_rows(got, states, masks, shots, program, first_row=0):
  got = got.cpu().numpy()
  assert got.dtype == np.int32 and got.shape == (states.shape[0], len(masks))
  p = R.masses(states)
  for m in range(states.shape[0]):
    want = R.restated_sums(p[m], masks, shots, first_row + m, SEED, program)
    assert (got[m] == want).all(), (m, np.flatnonzero(got[m] != want)[:8], got[m][:4], want[:4])


@pytest.mark.parametrize("n,num,n_masks,shots", [
    (1, 1, 1, 4099), (5, 3, 4, ODD_SHOTS), (10, 2, 8, 2**20), (11, 2, 65, ODD_SHOTS), (13, 1, 1024, 2**18),
    (20, 2, 57, 2**18), (24, 1, 210, ODD_SHOTS)])
def test_states_entry_is_the_flat_definition_on_dyadic_states(n, num, n_masks, shots):
  rng = np.random.default_rng(1000 + n)
  states = R.dyadic_states(rng, num, n)
  masks = R.mask_set(rng, n, n_masks)
  got = E.sample_parities_states(_gpu(states), masks, shots, seed=SEED, program=2)
  _check_rows(got, states, masks, shots, 2)
  if n_masks > 1:
    assert (got[:, 0] == shots).all()   # mask 0


@pytest.mark.parametrize("n", [11, 26])
def test_mass_at_both_ends_only(n):
  """Index 0 and index 2^n - 1: every block between them has no mass."""
  rng = np.random.default_rng(n)
  masks = R.mask_set(rng, n, 9)
  masks[2] = 1   # qubit 0 alone: the two outcomes differ in it
  states = torch.zeros((1, 1 << n), dtype=torch.complex64, device="cuda")
  states[0, 0] = 0.5
  states[0, -1] = 0.25j
  got = E.sample_parities_states(states, masks, ODD_SHOTS, seed=SEED, first_row=5).cpu().numpy()
  want = R.restated_sums([0.25, 0.0625], masks, ODD_SHOTS, 5, SEED, 0, support=[0, (1 << n) - 1], n_qubits=n)
  assert (got[0] == want).all()
  assert 0 < abs(int(got[0, 2])) < ODD_SHOTS   # both ends were drawn, 4 : 1


def test_mass_in_the_first_block_only_and_a_basis_state_and_a_zero_state():
  n = 13
  rng = np.random.default_rng(7)
  masks = R.mask_set(rng, n, 12)
  states = np.zeros((4, 1 << n), np.complex64)
  states[0, :1024] = R.dyadic_states(rng, 1, 10)[0]                 # the first block alone
  basis = int(rng.integers(1 << n))
  states[1, basis] = -0.5j                                          # a basis state
  states[3] = R.dyadic_states(rng, 1, n)[0]                         # (row 2 stays all zero)
  got = E.sample_parities_states(_gpu(states), masks, ODD_SHOTS, seed=SEED)
  _check_rows(got, states, masks, ODD_SHOTS, 0)
  got = got.cpu().numpy()
  signs = R.sums_of_counts([basis], [1], masks, n)
  assert (got[1] == ODD_SHOTS * signs).all() and set(np.abs(got[1]).tolist()) == {ODD_SHOTS}
  assert not got[2].any()
  assert got[3].any()


def test_rows_do_not_depend_on_their_neighbours_and_calls_repeat():
  n, num = 12, 5
  rng = np.random.default_rng(11)
  states = _gpu(R.dyadic_states(rng, num, n))
  masks = R.mask_set(rng, n, 20)
  both = E.sample_parities_states(states, masks, ODD_SHOTS, seed=SEED, program=1)
  again = E.sample_parities_states(states, masks, ODD_SHOTS, seed=SEED, program=1)
  assert torch.equal(both, again)
  for m in range(num):
    alone = E.sample_parities_states(states[m:m + 1], masks, ODD_SHOTS, seed=SEED, first_row=m, program=1)
    assert torch.equal(alone[0], both[m]), m
  assert not torch.equal(both, E.sample_parities_states(states, masks, ODD_SHOTS, seed=SEED, program=0))
  assert not E.sample_parities_states(states, masks, 0, seed=SEED).any()   # no shots: zeros


# ---- the engine entry ----

def _shiftable(gates):
  """A parametrised gate to shift: a single-qubit one if there is one."""
  own = [g for g, t in enumerate(gates) if t[3] >= 0]
  single = [g for g in own if gates[g][2] < 0]
  return (single or own)[0]


def _programs(gates, count):
  g = _shiftable(gates)
  return ([-1, g, g][:count] if count > 1 else [g]), ([0.0, 0.5, -0.5][:count] if count > 1 else [0.5])


def _shifted(gates, gate, shift):
  if gate < 0 or shift == 0.0:
    return list(gates)
  out = list(gates)
  k, a, b, p, s, o = out[gate][:6]
  out[gate] = (k, a, b, p, s, o + shift)   # exponent = scalar * param + offset
  return out


@pytest.mark.parametrize("n,opts", [(11, {}), (13, {"tile_qubits": 10})])
def test_engine_entry_bits_do_not_depend_on_the_cut(n, opts):
  gates, n_params, params, bits, _ = _dense_case(n, 2, seed=300 + n)
  rng = np.random.default_rng(n)
  bits = rng.integers(0, 2, size=(7, n)).astype(np.int8)
  masks = R.mask_set(rng, n, 33)
  sg, sv = _programs(gates, 3)
  want = _engine(n, gates, n_params, **opts).sample_parities(bits, params, masks, ODD_SHOTS, SEED, sg, sv)
  assert want.shape == (3, 7, 33) and (want[:, :, 0] == ODD_SHOTS).all()
  assert not torch.equal(want[1], want[2])   # (the two shifts give different programs)
  for extra in ({"chunk_states": 1}, {"workspace_budget_mb": 1}, {"chunk_states": 2, "workspace_budget_mb": 1}):
    got = _engine(n, gates, n_params, **opts, **extra).sample_parities(bits, params, masks, ODD_SHOTS, SEED, sg, sv)
    assert torch.equal(got, want), extra


@pytest.mark.parametrize("n,rows,programs,opts", [
    (3, 2, 3, {"chunk_states": 1}), (10, 2, 2, {}), (11, 2, 3, {"chunk_states": 1}), (16, 2, 2, {}), (20, 1, 2, {})])
def test_engine_entry_against_the_oracle(n, rows, programs, opts):
  """|S_gpu[t] - S_ref[t]| <= 2 ambiguous(delta) against the complex128 oracle, and <= 2e-3 shots against the
  restatement on the engine's own probabilities; the shifted programs' references are the oracle and an engine on the
  circuit with that gate's offset moved by the shift."""
  gates, n_params, params, bits, _ = _dense_case(n, rows, seed=200 + n)
  rng = np.random.default_rng(n)
  masks = R.mask_set(rng, n, 16)
  sg, sv = _programs(gates, programs)
  assert any(g >= 0 and s != 0.0 for g, s in zip(sg, sv))
  got = _engine(n, gates, n_params, **opts).sample_parities(bits, params, masks, ODD_SHOTS, SEED, sg, sv).cpu().numpy()
  dim = 1 << n
  for q, (g, s) in enumerate(zip(sg, sv)):
    moved = _shifted(gates, g, s)
    psi = _engine(n, moved, n_params).statevector(bits, params)
    for r in range(rows):
      ref = Ref.dense(np.abs(O.simulate(n, moved, params, list(bits[r])).ravel())**2)
      delta = _delta(psi[r], ref)
      counts, ambiguous = _restated_counts(ref, ODD_SHOTS, r, q, delta, dim)
      want = R.sums_of_counts(np.arange(dim), counts, masks, n)
      off = np.abs(got[q, r].astype(np.int64) - want)
      print(f"n={n} program={q} row={r}: max |dS| = {off.max()}, ambiguous = {ambiguous}, delta = {delta:.3g}")
      assert (off <= 2 * ambiguous).all(), (q, r, off.max(), ambiguous, delta)
      own, _ = _restated_counts(_gpu_ref(psi[r]), ODD_SHOTS, r, q, 0.0, dim)
      off_own = np.abs(got[q, r].astype(np.int64) - R.sums_of_counts(np.arange(dim), own, masks, n))
      print(f"    on the engine's own probabilities: max |dS| = {off_own.max()}")
      assert (off_own <= 2e-3 * ODD_SHOTS).all(), (q, r, off_own.max())


# ---- the mirror ----

def test_expectation_x_pow_sampled_from_parities():
  """tests/test_sampled_inference_gpu.py test_expectation_x_pow_sampled on the parities route (atol 2e-2, 10^6 shots)."""
  num_bits = 3
  qubits = ir.GridQubit.rect(1, num_bits)
  p_qnn = models.DirectQuantumCircuit(ir.Circuit(ir.X(q)**ir.Symbol("p") for q in qubits), name="p_qnn")
  _set(p_qnn.trainable_variables[0], [0.37])
  initial_states = torch.tensor(2 * list(itertools.product([0, 1], repeat=num_bits)), dtype=torch.int8)
  sin_pi_p, cos_pi_p = math.sin(math.pi * 0.37), math.cos(math.pi * 0.37)
  qnn = inference.SampledQuantumInference(p_qnn, int(1e6), initial_seed=7, pauli_estimator="parities")
  for pauli, val, grad in ((ir.PX, lambda s: 0.0, lambda s: 0.0),
                           (ir.PY, lambda s: -((-1.0)**s) * sin_pi_p, lambda s: -((-1.0)**s) * math.pi * cos_pi_p),
                           (ir.PZ, lambda s: ((-1.0)**s) * cos_pi_p, lambda s: -((-1.0)**s) * math.pi * sin_pi_p)):
    ops = [1.0 * pauli(q) for q in qubits]
    actual, (jac,) = _jacobian(lambda: qnn.expectation(initial_states, ops), p_qnn.trainable_variables)
    expected = [[val(s) for s in bits] for bits in initial_states.tolist()]
    expected_grad = [[grad(s) for s in bits] for bits in initial_states.tolist()]
    assert actual.shape == (16, 3)
    np.testing.assert_allclose(actual.detach().cpu().numpy(), expected, atol=2e-2)
    np.testing.assert_allclose(jac[:, :, 0], expected_grad, atol=2e-2)


def test_wide_register_values_and_jacobian_against_the_analytic_inference():
  """18 qubits, depth-1 HEA, 2 states, Z strings + one X string + one Y string, 2 10^5 shots, fixed seed.  An estimate is
  a mean of +-1 per string: |error| <= 6 sum|c_k| / sqrt(shots) is six standard deviations at the least; a parameter
  with one gate occurrence takes two shifted estimates at weight pi / 2 each: 6 pi sum|c_k| / sqrt(shots)."""
  n, shots = 18, 200000
  qubits = ir.GridQubit.rect(1, n)
  circ = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "w"))
  rng = np.random.default_rng(18)
  _set(circ.trainable_variables[0], rng.uniform(0.1, 0.9, len(circ.symbol_names)))
  coeffs = [0.7, -0.4, 0.5, 0.3, -0.6]
  op = (coeffs[0] * ir.PZ(qubits[0]) * ir.PZ(qubits[1]) + coeffs[1] * ir.PZ(qubits[5]) +
        coeffs[2] * ir.PZ(qubits[9]) * ir.PZ(qubits[10]) * ir.PZ(qubits[17]) +
        coeffs[3] * ir.PX(qubits[3]) * ir.PX(qubits[4]) + coeffs[4] * ir.PY(qubits[12]) * ir.PZ(qubits[13]))
  states = torch.tensor(rng.integers(0, 2, size=(2, n)), dtype=torch.int8)
  exact, (exact_jac,) = _jacobian(lambda: inference.AnalyticQuantumInference(circ).expectation(states, [op]),
                                  circ.trainable_variables)
  qnn = inference.SampledQuantumInference(circ, shots, initial_seed=3, pauli_estimator="parities")
  got, (jac,) = _jacobian(lambda: qnn.expectation(states, [op]), circ.trainable_variables)
  norm = sum(abs(c) for c in coeffs)
  names = circ.symbol_names
  flat = circ.pqc.flat_gates(qubits, names)
  occurrences = np.array([sum(1 for g in flat if g[3] == p) for p in range(len(names))])
  assert (occurrences >= 1).all()
  err = np.abs(got.detach().cpu().numpy() - exact.detach().cpu().numpy())
  err_jac = np.abs(jac - exact_jac)
  print("values: max error", err.max(), "bound", 6 * norm / math.sqrt(shots))
  print("jacobian: max error", err_jac.max(), "bound per occurrence", 6 * math.pi * norm / math.sqrt(shots))
  assert np.abs(exact_jac).max() > 0.05   # (the comparison is not between zeros)
  assert (err <= 6 * norm / math.sqrt(shots)).all()
  assert (err_jac <= 6 * math.pi * norm / math.sqrt(shots) * occurrences).all()


def test_state_vector_data_sampled_expectation_of_the_tfim_ground_state():
  """The 8-qubit TFIM ring's ground state: the sampled <H> (Z-only strings sampled as given, X strings after one rotation)
  against the exact value from the same states (what `expectation` computes: expectation_from_states), within
  6 sum|c_k| / sqrt(shots); a list of observables gives one value each; an un-normalised row is scaled by its norm."""
  from qhbmlib_amd import data  # pylint: disable=import-outside-toplevel
  n, shots = 8, 200000
  qubits = ir.GridQubit.rect(1, n)
  zz = ir.PZ(qubits[0]) * ir.PZ(qubits[1])
  for a, b in zip(qubits[1:], qubits[2:] + qubits[:1]):
    zz = zz + ir.PZ(a) * ir.PZ(b)
  xs = ir.PX(qubits[0])
  for q in qubits[1:]:
    xs = xs + ir.PX(q)
  source = data.StateVectorData.ground_state([zz, xs], weights=[-1.0, -1.0], seed=3)
  hamiltonian = -1.0 * zz - xs
  states = source._device_states()  # pylint: disable=protected-access
  exact = source._inference_for(qubits).expectation_from_states(states, [hamiltonian, zz, xs])[0]  # pylint: disable=protected-access
  exact = exact.detach().cpu().numpy().astype(np.float64)
  got = float(source.sampled_expectation(hamiltonian, shots, seed=5))
  bound = 6 * 2 * n / math.sqrt(shots)
  print("sampled <H> =", got, "exact =", exact[0], "bound", bound)
  assert exact[0] < -n   # (the ground state of the critical ring: about -1.28 n)
  assert abs(got - exact[0]) <= bound
  assert got == float(source.sampled_expectation(hamiltonian, shots, seed=5))   # a seed fixes the estimate
  both = source.sampled_expectation([zz, xs], shots, seed=6).cpu().numpy()
  assert both.shape == (2,) and (np.abs(both - exact[1:]) <= 6 * n / math.sqrt(shots)).all()
  doubled = data.StateVectorData(2.0 * source.states, source.weights, qubits)
  assert abs(float(doubled.sampled_expectation(hamiltonian, shots, seed=5)) - 4.0 * got) <= 1e-9 * abs(got)
