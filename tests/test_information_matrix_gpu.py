"""qhbm_program_vjps (one adjoint VJP per parameter-shifted program) and the BKM information matrix on the MI355X.

Engine: every program against the numpy oracle; the unshifted program bit for bit against qhbm_expectation_vjp;
outputs bit-identical however the work is cut; prefix sharing sound on plans whose first pass zero-fills.
Mirror: information_matrix against the numpy restatement of the reference's loop, the dense closed form, central
differences of a QAIA circuit, and the reference-shaped loop through the mirror."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import inference, ir, models
from tests import info_matrix_ref as R

pytestmark = pytest.mark.gpu

_SCRIPT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "info_matrix_time.py")


def _timing_script():
  spec = importlib.util.spec_from_file_location("info_matrix_time", _SCRIPT)
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  return mod


def _engine(n, gates, n_params, ops, **options):
  eng = E.Engine(0)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(n, gates, n_params)
  eng.set_observables(ops)
  return eng


def _random_circuit(rng, n, n_gates, n_params):
  gates = []
  for _ in range(n_gates):
    kind = int(rng.integers(12))
    q0 = int(rng.integers(n))
    q1 = -1
    if O.gate_num_qubits(kind) == 2:
      q1 = int(rng.integers(n - 1))
      q1 += q1 >= q0
    if rng.random() < 0.8:
      gates.append((kind, q0, q1, int(rng.integers(n_params)), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-0.5, 0.5))))
    else:
      gates.append((kind, q0, q1, -1, 0.0, float(rng.uniform(-1, 1))))
  return gates


def _shifted(gates, g, shift):
  if g < 0:
    return gates
  out = list(gates)
  k, q0, q1, p, s, o = out[g][:6]
  out[g] = (k, q0, q1, p, s, o + shift) + tuple(out[g][6:])
  return out


def _oracle_programs(n, gates, params, bits, ops, shift_gates, shifts, up, w, mask=None):
  vals, grads = [], []
  for g, sh in zip(shift_gates, shifts):
    v, jac = O.expectation_jacobian(n, _shifted(gates, g, sh), params, bits, ops)
    vals.append(w @ v)
    gr = np.einsum("uk,ukp->p", up, jac)
    grads.append(np.where(mask, gr, 0.0) if mask is not None else gr)
  return np.array(vals), np.array(grads)


def _programs(gates, rng, count, allow_iswap=False):
  cand = [g for g, gate in enumerate(gates)
          if gate[3] >= 0 and (allow_iswap or gate[0] != E.GATE_ISWAPPOW)]
  picks = [int(rng.choice(cand)) for _ in range(count)] + [-1]
  shifts = [float(rng.choice([0.5, -0.5, 0.3])) for _ in range(count)] + [0.0]
  return picks, shifts


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_program_vjps_against_the_oracle(n):
  rng = np.random.default_rng(100 + n)
  n_params = 6
  gates = _random_circuit(rng, n, 24, n_params)
  params = rng.uniform(-1, 1, n_params).astype(np.float32)
  bits = rng.integers(0, 2, size=(5, n)).astype(np.int8)
  ops = [O.random_pauli_op(n, 6, n + 1, p_identity=0.5), O.tfim_ring_op(n) if n > 2 else [(1.0, 0, 1)]]
  up = rng.normal(size=(5, len(ops))).astype(np.float32)
  w = rng.uniform(0.1, 1.0, 5).astype(np.float32)
  sg, sv = _programs(gates, rng, 7)
  for mask in (None, rng.random(n_params) < 0.5):
    eng = _engine(n, gates, n_params, ops)
    if mask is not None:
      eng.set_gradient_mask(mask)
    vals, grad = eng.program_vjps(bits, params, sg, sv, up, row_weights=w)
    want_vals, want_grad = _oracle_programs(n, gates, params.astype(np.float64), bits, ops, sg, sv, up, w, mask)
    for q in range(len(sg)):
      np.testing.assert_allclose(grad[q].cpu().numpy(), want_grad[q], rtol=0,
                                 atol=1e-4 * max(1.0, np.abs(want_grad[q]).max()), err_msg=f"program {q}")
      np.testing.assert_allclose(vals[q].cpu().numpy(), want_vals[q], rtol=0,
                                 atol=1e-4 * max(1.0, np.abs(want_vals[q]).max()), err_msg=f"program {q}")
  # without row weights the values are plain sums over the states
  vals1, _ = eng.program_vjps(bits, params, sg, sv, up)
  np.testing.assert_allclose(vals1.cpu().numpy(), _oracle_programs(n, gates, params.astype(np.float64), bits, ops, sg, sv,
                                                                   up, np.ones(5))[0], atol=1e-4 * 5)


def test_program_vjps_errors():
  n = 4
  gates = [(E.GATE_XPOW, 0, -1, 0, 1.0, 0.0), (E.GATE_ISWAPPOW, 1, 2, 1, 1.0, 0.0), (E.GATE_ZPOW, 3, -1, -1, 0.0, 0.3)]
  eng = _engine(n, gates, 2, [[(1.0, 0, 1)]])
  bits = np.zeros((2, n), np.int8)
  up = np.ones((2, 1), np.float32)
  with pytest.raises(E.EngineError, match="ISWAPPOW"):
    eng.program_vjps(bits, [0.1, 0.2], [1], [0.5], up)
  with pytest.raises(E.EngineError, match="out of range"):
    eng.program_vjps(bits, [0.1, 0.2], [3], [0.5], up)
  with pytest.raises(E.EngineError, match="constant exponent"):
    eng.program_vjps(bits, [0.1, 0.2], [2], [0.5], up)
  vals, grad = eng.program_vjps(bits, [0.1, 0.2], [1, 0], [0.0, 0.5], up)   # ISWAPPOW unshifted is fine
  assert torch.isfinite(grad).all() and torch.isfinite(vals).all()
  no_obs = E.Engine(0)
  no_obs.set_circuit(n, gates, 2)
  no_obs.n_ops = 1
  with pytest.raises(E.EngineError, match="qhbm_set_observables"):
    no_obs.program_vjps(bits, [0.1, 0.2], [0], [0.5], up)


@pytest.mark.parametrize("n,tile,ops_kind", [(4, 0, "one"), (5, 0, "two"), (13, 10, "one"), (14, 10, "shards")])
def test_unshifted_program_is_the_adjoint_vjp_bit_for_bit(n, tile, ops_kind):
  rng = np.random.default_rng(300 + n)
  gates, names = O.hea_gates(n, 3, "u")
  params = rng.uniform(-1, 1, len(names)).astype(np.float32)
  ops = {"one": [O.xxz_chain_op(n)], "two": [O.tfim_ring_op(n), O.xxz_chain_op(n)],
         "shards": O.kobe_shards(n, 2)}[ops_kind]
  bits = rng.integers(0, 2, size=(6, n)).astype(np.int8)
  up = rng.normal(size=(6, len(ops))).astype(np.float32)
  opts = dict(tile_qubits=tile, adjoint_tile_qubits=tile) if tile else {}
  for mask in (None, np.arange(len(names)) >= len(names) // 2):
    eng = _engine(n, gates, len(names), ops, **opts)
    if mask is not None:
      eng.set_gradient_mask(mask)
    _, want = eng.expectation_vjp(bits, params, up)
    _, grad = eng.program_vjps(bits, params, [0, -1, 3], [0.5, 0.0, -0.5], up)
    assert torch.equal(grad[1], want), float((grad[1] - want).abs().max())


def _bkm_engine_case(n, layers, seed):
  """Model circuit + inverse on a second copy of the parameters, gradient mask on the second half, programs = shifted
  occurrences of the first half -- the information-matrix call."""
  rng = np.random.default_rng(seed)
  gates, names = O.hea_gates(n, layers, "b")
  p = len(names)
  total = R.total_gates(gates, p)
  theta = rng.uniform(-1, 1, p).astype(np.float32)
  params = np.concatenate([theta, theta])
  mask = np.arange(2 * p) >= p
  occ = [g for g, gate in enumerate(gates) if gate[3] >= 0]
  sg = [g for g in occ for _ in (0, 1)]
  sv = [0.5, -0.5] * len(occ)
  return total, 2 * p, params, mask, sg, sv


@pytest.mark.parametrize("n,tile", [(11, 10), (13, 10)])
def test_outputs_do_not_depend_on_how_the_work_is_cut(n, tile):
  total, n_params, params, mask, sg, sv = _bkm_engine_case(n, 2, 500 + n)
  rng = np.random.default_rng(n)
  ops = O.kobe_shards(n, 2)[:8]
  bits = rng.integers(0, 2, size=(5, n)).astype(np.int8)
  up = rng.normal(size=(5, len(ops))).astype(np.float32)
  w = rng.uniform(0.1, 1, 5).astype(np.float32)
  sg, sv = sg[:24] + [-1, len(total) - 1], sv[:24] + [0.0, 0.5]   # and one program behind the first live gate
  results = []
  for chunk in (1, 3, 0):
    for sharing in (0, 1):
      eng = _engine(n, total, n_params, ops, tile_qubits=tile, chunk_states=chunk, shift_prefix_sharing=sharing)
      eng.set_gradient_mask(mask)
      vals, grad = eng.program_vjps(bits, params, sg, sv, up, row_weights=w)
      results.append((chunk, sharing, vals.clone(), grad.clone()))
  for chunk, sharing, vals, grad in results[1:]:
    assert torch.equal(vals, results[0][2]), (chunk, sharing)
    assert torch.equal(grad, results[0][3]), (chunk, sharing, float((grad - results[0][3]).abs().max()))
  want_vals, want_grad = _oracle_programs(n, total, params.astype(np.float64), bits, ops, sg[-4:], sv[-4:], up, w, mask)
  np.testing.assert_allclose(results[0][3][-4:].cpu().numpy(), want_grad, atol=1e-4 * max(1.0, np.abs(want_grad).max()))
  np.testing.assert_allclose(results[0][2][-4:].cpu().numpy(), want_vals, atol=1e-4 * max(1.0, np.abs(want_vals).max()))


def test_prefix_sharing_with_a_diagonal_only_qubit():
  """a qubit with only diagonal gates at n above the tile size -- the plan's first pass zero-fills,
  and a program that starts behind it would read stale amplitudes.  Sharing on equals sharing off bit for bit, over
  several launch sets and calls with other bitstrings in between, and matches the C oracle."""
  from oracle import qhbm_cpu as C
  n, tile = 14, 10
  rng = np.random.default_rng(77)
  n_params = 8
  gates = []
  for layer in range(3):
    for q in range(n - 1):   # qubit n - 1: Z powers and controlled phases only
      gates.append((E.GATE_XPOW, q, -1, int(rng.integers(n_params)), 1.0, float(rng.uniform(-0.3, 0.3))))
    for q in range(n):
      gates.append((E.GATE_ZPOW, q, -1, int(rng.integers(n_params)), 1.0, 0.1))
    for q in range(layer % 2, n - 1, 2):
      gates.append((E.GATE_CZPOW, q, q + 1, int(rng.integers(n_params)), 1.0, 0.0))
  params = rng.uniform(-1, 1, n_params).astype(np.float32)
  ops = [O.tfim_ring_op(n), O.xxz_chain_op(n)]
  bits = rng.integers(0, 2, size=(4, n)).astype(np.int8)
  bits[:, n - 1] = [0, 1, 1, 0]
  up = rng.normal(size=(4, 2)).astype(np.float32)
  live = [g for g, gate in enumerate(gates) if gate[3] >= 0]
  sg = [int(g) for g in rng.choice(live, 10, replace=False)] + [-1]
  sv = [0.5] * 10 + [0.0]
  results = []
  for sharing in (0, 1):
    eng = _engine(n, gates, n_params, ops, tile_qubits=tile, adjoint_tile_qubits=tile, chunk_states=2,
                  shift_prefix_sharing=sharing)
    assert eng.num_passes()[0] > 1
    eng.expectation(1 - bits, params)                  # leaves other states in the workspace
    results.append(eng.program_vjps(bits, params, sg, sv, up))
  assert torch.equal(results[0][0], results[1][0])
  assert torch.equal(results[0][1], results[1][1])
  for q in (0, 4, 10):
    _, want = C.expectation_vjp(n, _shifted(gates, sg[q], sv[q]), params, bits, ops, up)
    np.testing.assert_allclose(results[1][1][q].cpu().numpy(), want, atol=1e-4 * max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("ops_kind", ["shards", "tfim + xxz"])
def test_prefix_sharing_with_programs_that_no_pass_reads(ops_kind):
  """Programs whose shifted gate no record of any pass reads -- a parametrised identity, and the unshifted program
  (a negative gate) -- start at the last pass that stores its state: never at a measurement-only pass (shards), never
  behind the first measuring pass when the passes measure.  Sharing on equals sharing off bit for bit, launch sets
  whole and cut, and both match the C oracle."""
  from oracle import qhbm_cpu as C
  n, tile = 13, 10
  rng = np.random.default_rng(1300)
  gates, names = O.hea_gates(n, 3, "nr")
  n_params = len(names)
  ident = len(gates) // 2
  gates = gates[:ident] + [(E.GATE_I, 4, -1, 2, 0.9, 0.2)] + gates[ident:]
  params = rng.uniform(-1, 1, n_params).astype(np.float32)
  ops = {"shards": [[(1.0, 0, 1 << q)] for q in range(n)] + [[(0.5, 0, (1 << q) | (1 << ((q + 5) % n)))] for q in range(n)],
         "tfim + xxz": [O.tfim_ring_op(n), O.xxz_chain_op(n)]}[ops_kind]
  bits = rng.integers(0, 2, size=(3, n)).astype(np.int8)
  up = rng.normal(size=(3, len(ops))).astype(np.float32)
  live = [g for g, gate in enumerate(gates) if gate[3] >= 0 and g != ident]
  sg = [live[0], ident, live[len(live) // 2], ident, live[-1], -1]
  sv = [0.5, 0.5, -0.5, -0.5, 0.5, 0.0]
  for chunk in (0, 5):
    results = []
    for sharing in (0, 1):
      eng = _engine(n, gates, n_params, ops, tile_qubits=tile, adjoint_tile_qubits=tile, chunk_states=chunk,
                    shift_prefix_sharing=sharing)
      assert eng.num_passes()[0] > 1
      eng.expectation(1 - bits, params)                  # leaves other states in the workspace
      vals, grad = eng.program_vjps(bits, params, sg, sv, up)
      results.append((vals.clone(), grad.clone()))
    assert torch.equal(results[0][0], results[1][0]), chunk
    assert torch.equal(results[0][1], results[1][1]), (chunk, float((results[0][1] - results[1][1]).abs().max()))
    for q in (1, 2, 3, 5):
      want_v, want = C.expectation_vjp(n, _shifted(gates, sg[q], sv[q]), params, bits, ops, up)
      for vals, grad in results:
        np.testing.assert_allclose(grad[q].cpu().numpy(), want, atol=1e-4 * max(1.0, np.abs(want).max()), err_msg=f"program {q}")
        np.testing.assert_allclose(vals[q].cpu().numpy(), want_v.sum(0), atol=1e-4 * max(1.0, np.abs(want_v).max()),
                                   err_msg=f"program {q}")


def test_twenty_qubits_against_the_c_oracle():
  from oracle import qhbm_cpu as C
  n = 20
  total, n_params, params, mask, sg, sv = _bkm_engine_case(n, 1, 2020)
  rng = np.random.default_rng(20)
  ops = O.kobe_shards(n, 1)[:4]
  bits = rng.integers(0, 2, size=(2, n)).astype(np.int8)
  up = rng.normal(size=(2, len(ops))).astype(np.float32)
  sg, sv = [sg[0], sg[1], sg[-2], -1], [sv[0], sv[1], sv[-2], 0.0]
  eng = _engine(n, total, n_params, ops)
  eng.set_gradient_mask(mask)
  vals, grad = eng.program_vjps(bits, params, sg, sv, up)
  for q in range(len(sg)):
    want_v, want = C.expectation_vjp(n, _shifted(total, sg[q], sv[q]), params, bits, ops, up)
    want = np.where(mask, want, 0.0)
    np.testing.assert_allclose(grad[q].cpu().numpy(), want, atol=1e-4 * max(1.0, np.abs(want).max()))
    np.testing.assert_allclose(vals[q].cpu().numpy(), want_v.sum(0), atol=1e-4 * max(1.0, np.abs(want_v).max()))


# ---- the information matrix through the mirror ----------------------------------------------------------------------
def _hea_qhbm(n, layers, seed=0, samples=16):
  torch.manual_seed(seed)
  mod = _timing_script()
  return mod.build(n, layers, seed=seed)


def _oracle_view(qhbm):
  ham = qhbm.modular_hamiltonian
  circ = ham.circuit
  gates = circ.pqc.flat_gates(circ.qubits, circ.symbol_names)
  theta = circ.symbol_values.detach().cpu().numpy().astype(np.float64)
  phi = ham.energy.post_process[0].kernel.detach().cpu().numpy().astype(np.float64)
  sets = list(ham.energy._parity_index_sets())  # pylint: disable=protected-access
  shards = O.kobe_shards(len(circ.qubits), 2)
  return gates, theta, phi, sets, shards


def test_information_matrix_exact_mode_equals_the_reference_loop():
  """The reference experiment's shape (4 qubits, qhea 7 layers, KOBE-2: D = 87), exact distribution."""
  n = 4
  qhbm, _ = _hea_qhbm(n, 7, seed=1)
  m = inference.information_matrix(qhbm, symmetrize=False).cpu().numpy()
  gates, theta, phi, sets, shards = _oracle_view(qhbm)
  bits = O.all_bitstrings(n)
  e = O.parities(bits, sets) @ phi
  w = np.exp(-e - (-e).max())
  w /= w.sum()
  ebm, cross, qnn = R.reference_loop(n, gates, theta, phi, sets, shards, bits, w)
  want = R.assemble(ebm, cross, qnn, symmetrize=False)
  assert m.shape == (87, 87)
  np.testing.assert_allclose(m, want, atol=2e-4 * max(1.0, np.abs(want).max()))


@pytest.mark.parametrize("n", [3, 4])
def test_symmetrized_matrix_equals_the_dense_closed_form(n):
  qhbm, _ = _hea_qhbm(n, 2, seed=n)
  m = inference.information_matrix(qhbm).cpu().numpy()
  gates, theta, phi, sets, _ = _oracle_view(qhbm)
  bits = O.all_bitstrings(n)
  e = O.parities(bits, sets) @ phi
  w = np.exp(-e - (-e).max())
  w /= w.sum()
  cross, qnn = R.dense_blocks(n, gates, theta, phi, sets, bits, w)
  jac = O.parities(bits, sets)
  mu = w @ jac
  ebm = (jac - mu).T @ (w[:, None] * (jac - mu))
  want = R.assemble(ebm, cross, qnn, symmetrize=True)
  np.testing.assert_allclose(m, want, atol=2e-4 * max(1.0, np.abs(want).max()))


def test_sampled_mode_equals_the_loop_on_the_same_samples():
  n = 4
  qhbm, copy = _hea_qhbm(n, 3, seed=7)
  qhbm.e_inference.seed = 1234
  m = inference.information_matrix(qhbm, num_samples=200, symmetrize=False)
  qhbm.e_inference.seed = 1234
  mod = _timing_script()
  bits, weights = mod.fixed_samples(qhbm, 200)
  cross, qnn = mod.mirror_loop(qhbm, copy, bits, weights)
  n_e = cross.shape[1]
  gates, theta, phi, sets, shards = _oracle_view(qhbm)
  ebm, _, _ = R.reference_loop(n, gates[:0], theta[:0], phi, sets, shards, bits.cpu().numpy(), weights.cpu().numpy())
  np.testing.assert_allclose(m[:n_e, :n_e].cpu().numpy(), ebm, atol=1e-5)
  scale = max(1.0, float(qnn.abs().max()))
  np.testing.assert_allclose(m[n_e:, :n_e].cpu().numpy(), cross.cpu().numpy(), atol=1e-4 * scale)
  np.testing.assert_allclose(m[n_e:, n_e:].cpu().numpy(), qnn.cpu().numpy(), atol=1e-4 * scale)


def test_qaia_matrix_equals_central_differences():
  """Symbols that are functions of the variables (QAIA: eta_l * theta_b): the symbol-space blocks mapped with
  J = d symbol_values / d variables equal complex128 central differences of tr[rho K'] in the VARIABLES."""
  n = 3
  torch.manual_seed(11)
  qubits = ir.GridQubit.rect(1, n)
  classical = [ir.PauliSum.from_pauli_strings(ir.PZ(q)) for q in qubits]
  quantum = [ir.PauliSum.from_pauli_strings(ir.PX(q)) for q in qubits]
  circ = models.QAIA(quantum, classical, 2).to("cuda")
  energy = models.BernoulliEnergy(list(range(n))).to("cuda")
  qhbm = inference.QHBM(inference.AnalyticEnergyInference(energy, 8), inference.AnalyticQuantumInference(circ))
  m = inference.information_matrix(qhbm, symmetrize=False).cpu().numpy().astype(np.float64)
  gates = circ.pqc.flat_gates(circ.qubits, circ.symbol_names)
  variables = [v.detach().cpu().numpy().astype(np.float64) for v in circ.trainable_variables]
  sizes = [v.size for v in variables]
  flat0 = np.concatenate([v.reshape(-1) for v in variables])
  phi = energy.post_process[0].kernel.detach().cpu().numpy().astype(np.float64)
  sets = [(i,) for i in range(n)]
  bits = O.all_bitstrings(n)
  w = np.exp(-(O.parities(bits, sets) @ phi))
  w /= w.sum()

  def symbols(flat):
    with torch.no_grad():
      for v, chunk in zip(circ.trainable_variables, np.split(flat, np.cumsum(sizes)[:-1])):
        v.copy_(torch.as_tensor(chunk.reshape(v.shape), dtype=torch.float32))
      vals = circ.symbol_values.detach().cpu().numpy().astype(np.float64)
    return vals

  # symbol values are multilinear in the variables: evaluate them in float64 from the embedding directly
  etas, thetas, gammas = [v.reshape(v.shape) for v in variables]

  def sym64(flat):
    e, t, g = np.split(flat, np.cumsum(sizes)[:-1])
    g = g.reshape(gammas.shape)
    return np.concatenate([np.concatenate([e[l] * t, g[l]]) for l in range(len(e))])

  np.testing.assert_allclose(sym64(flat0), symbols(flat0), atol=1e-6)
  symbols(flat0)
  h = 1e-4

  def rho_k(flat_a, flat_b, diag):
    ua = R._unitary(n, gates, sym64(flat_a))  # pylint: disable=protected-access
    ub = R._unitary(n, gates, sym64(flat_b))  # pylint: disable=protected-access
    rho = (ua * w[None, :]) @ ua.conj().T
    k = (ub * diag[None, :]) @ ub.conj().T
    return float(np.real(np.trace(rho @ k)))

  energies = O.parities(bits, sets) @ phi
  d = flat0.size
  qnn = np.zeros((d, d))
  for i in range(d):
    for j in range(d):
      ei, ej = np.eye(d)[i] * h, np.eye(d)[j] * h
      qnn[i, j] = -(rho_k(flat0 + ei, flat0 + ej, energies) - rho_k(flat0 + ei, flat0 - ej, energies)
                    - rho_k(flat0 - ei, flat0 + ej, energies) + rho_k(flat0 - ei, flat0 - ej, energies)) / (4 * h * h)
  par = O.parities(bits, sets)
  cross = np.zeros((d, n))
  for i in range(d):
    ei = np.eye(d)[i] * h
    for k in range(n):
      cross[i, k] = -(rho_k(flat0 + ei, flat0, par[:, k]) - rho_k(flat0 - ei, flat0, par[:, k])) / (2 * h)
  scale = max(1.0, np.abs(qnn).max())
  np.testing.assert_allclose(m[n:, n:], qnn, atol=5e-4 * scale)
  np.testing.assert_allclose(m[n:, :n], cross, atol=5e-4 * scale)


def test_config2_shape_matches_the_mirror_loop():
  """Config 2's shape (12 qubits, 8 layers, KOBE-2, 1024 samples, D = 358): the batched matrix equals the loop of the
  reference through the mirror -- engine against engine by two paths."""
  mod = _timing_script()
  qhbm, copy = mod.build(12, 8, seed=3)
  bits, weights = mod.fixed_samples(qhbm, 1024)
  qhbm.e_inference.sample = lambda num: bits.repeat_interleave(torch.round(weights * num).to(torch.long).to(bits.device), 0)
  m = inference.information_matrix(qhbm, num_samples=1024, symmetrize=False)
  cross, qnn = mod.mirror_loop(qhbm, copy, bits, weights)
  n_e = cross.shape[1]
  assert m.shape == (358, 358)
  scale = float(m.abs().max())
  assert float((m[n_e:, :n_e] - cross.to(m.device)).abs().max()) <= 1e-4 * scale
  assert float((m[n_e:, n_e:] - qnn.to(m.device)).abs().max()) <= 1e-4 * scale
