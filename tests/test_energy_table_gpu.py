"""Energy tables on the MI355X: qhbm_table_expectation* against exact restatements, and the host mirror's
`energy_tables` route (a general BitstringEnergy measured exactly) through AnalyticQuantumInference, qmhl and
CapturedLoss.  Expected values come from the numpy oracle (small n: the Walsh form of the table through
O.expectation_jacobian; n = 12: the same adjoint restated for a diagonal operator) or the C oracle (n = 13, 20)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import qhbm_cpu
from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir, models, utils
from tests import energy_table_ref as R
from tests.test_engine_gpu import random_circuit
from tests.test_host_api import hea_circuit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(n, gates, n_params, **options):
  eng = E.Engine(0)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(n, gates, n_params)
  return eng


def _run(eng, bits, params, table, up, retained=False):
  """(values, grad, table_grad) as numpy; `retained`: through the retaining forward and the retained VJP."""
  if retained:
    vals = eng.table_expectation(bits, params, table, retain=True)
    if eng.retained is None:  # (a chunk_states below the batch keeps nothing: the caller falls back, as the mirror does)
      with pytest.raises(E.EngineError, match="no retained"):
        eng.table_expectation_vjp_retained(bits, params, table, up)
      _, grad, tgrad = eng.table_expectation_vjp(bits, params, table, up)
    else:
      grad, tgrad = eng.table_expectation_vjp_retained(bits, params, table, up)
  else:
    vals, grad, tgrad = eng.table_expectation_vjp(bits, params, table, up)
  torch.cuda.synchronize()
  return vals.cpu().numpy(), grad.cpu().numpy(), tgrad.cpu().numpy()


@pytest.mark.parametrize("n", [3, 6, 9])
@pytest.mark.parametrize("family", ["hea", "all kinds"])
def test_engine_against_the_walsh_form_of_the_table(n, family):
  rng = np.random.default_rng(10 * n + len(family))
  if family == "hea":
    gates, names = O.hea_gates(n, 2)
    n_params = len(names)
  else:
    n_params = 6
    gates = random_circuit(rng, n, 4 * n, n_params)
  params = rng.uniform(-1, 1, n_params).astype(np.float32)
  bits = rng.integers(0, 2, (5, n)).astype(np.int8)
  table = R.random_table(n, rng)
  up = rng.normal(size=5).astype(np.float32)
  want_vals, want_grad, want_tgrad = R.oracle_vjp(n, gates, params.astype(np.float64), bits, table, up)
  eng = _engine(n, gates, n_params)
  for retained in (False, True):
    vals, grad, tgrad = _run(eng, bits, params, table, up, retained)
    emax = np.abs(table).max()
    assert np.abs(vals - want_vals).max() <= 1e-5 * emax
    assert np.abs(grad - want_grad).max() <= 1e-4 * max(np.abs(want_grad).max(), 1e-3 * emax)
    assert np.abs(tgrad - want_tgrad).max() <= 1e-5 * np.abs(up).sum()
  only = eng.table_expectation(bits, params, table).cpu().numpy()
  assert np.abs(only - want_vals).max() <= 1e-5 * np.abs(table).max()


@pytest.mark.parametrize("n", [13, 20])
def test_large_n_against_the_c_oracle(n):
  rng = np.random.default_rng(n)
  gates, names = O.hea_gates(n, 2 if n == 20 else 3)
  params = rng.uniform(-1, 1, len(names)).astype(np.float32)
  thetas = rng.uniform(-1, 1, len(O.parity_indices(n, 2)))
  op = R.kobe2_op(n, thetas)
  table = R.kobe2_table(n, thetas)
  bits = rng.integers(0, 2, (2, n)).astype(np.int8)
  up = np.array([0.7, -1.3], np.float32)
  want_vals, want_grad = qhbm_cpu.expectation_vjp(n, gates, params, bits, [op], up[:, None])
  states = qhbm_cpu.statevector(n, gates, params, bits)
  want_tgrad = up.astype(np.float64) @ (np.abs(states.astype(np.complex128)) ** 2)
  vals, grad, tgrad = _run(_engine(n, gates, len(names)), bits, params, table, up)
  norm = np.abs(thetas).sum()
  assert np.abs(vals - want_vals[:, 0]).max() <= 1e-5 * norm
  assert np.abs(grad - want_grad).max() <= 1e-4 * max(np.abs(want_grad).max(), 1.0)
  assert np.abs(tgrad - want_tgrad).max() <= 1e-5 * np.abs(up).sum()


def test_bit_identical_for_any_chunking_retained_or_not():
  n, U = 11, 9
  rng = np.random.default_rng(5)
  gates, names = O.hea_gates(n, 2)
  params = rng.uniform(-1, 1, len(names)).astype(np.float32)
  bits = rng.integers(0, 2, (U, n)).astype(np.int8)
  table = R.random_table(n, rng)
  up = rng.normal(size=U).astype(np.float32)
  ref = _run(_engine(n, gates, len(names)), bits, params, table, up)
  for chunk in (1, 3, 0):
    eng = _engine(n, gates, len(names), chunk_states=chunk)
    for retained in (False, True, False):
      got = _run(eng, bits, params, table, up, retained)
      for a, b in zip(ref, got):
        assert np.array_equal(a, b), (chunk, retained)
    if chunk == 0:  # the batch fits one chunk: the retained forward kept its states
      eng.table_expectation(bits, params, table, retain=True)
      assert eng.retained is not None
    only = eng.table_expectation(bits, params, table).cpu().numpy()
    assert np.array_equal(only, ref[0])


def test_dirty_workspace_gives_the_bits_of_a_fresh_engine():
  rng = np.random.default_rng(8)
  g12, n12 = O.hea_gates(12, 2)
  eng = _engine(12, g12, len(n12))
  eng.set_observables([O.xxz_chain_op(12)])
  bits12 = rng.integers(0, 2, (6, 12)).astype(np.int8)
  eng.expectation_vjp(bits12, rng.uniform(-1, 1, len(n12)).astype(np.float32), np.ones((6, 1), np.float32))
  n = 5
  gates, names = O.hea_gates(n, 2)
  params = rng.uniform(-1, 1, len(names)).astype(np.float32)
  bits = rng.integers(0, 2, (4, n)).astype(np.int8)
  table = R.random_table(n, rng)
  up = rng.normal(size=4).astype(np.float32)
  eng.set_circuit(n, gates, len(names))
  dirty = _run(eng, bits, params, table, up)
  fresh = _run(_engine(n, gates, len(names)), bits, params, table, up)
  for a, b in zip(dirty, fresh):
    assert np.array_equal(a, b)


def test_gradient_mask_freezes_the_data_half():
  n = 8
  rng = np.random.default_rng(9)
  data_gates, data_names = O.hea_gates(n, 2, "d")
  model_gates, model_names = O.hea_gates(n, 2, "m")
  nd = len(data_names)
  shifted = [(k, q0, q1, p + nd if p >= 0 else p, s, o) for k, q0, q1, p, s, o in model_gates]
  gates = data_gates + O.inverse_gates(shifted)
  n_params = nd + len(model_names)
  params = rng.uniform(-1, 1, n_params).astype(np.float32)
  bits = rng.integers(0, 2, (4, n)).astype(np.int8)
  table = R.random_table(n, rng)
  up = rng.normal(size=4).astype(np.float32)
  eng = _engine(n, gates, n_params)
  _, full, tfull = _run(eng, bits, params, table, up)
  eng.set_gradient_mask([False] * nd + [True] * len(model_names))
  _, masked, tmasked = _run(eng, bits, params, table, up)
  assert np.all(masked[:nd] == 0)
  assert np.abs(masked[nd:] - full[nd:]).max() <= 1e-5 * max(np.abs(full).max(), 1.0)
  assert np.abs(tmasked - tfull).max() <= 1e-6 * np.abs(up).sum()


def _total(circuit, ham):
  total = circuit + ham.circuit_dagger
  gates = total.pqc.flat_gates(total.qubits, total.symbol_names)
  return total, gates, total.symbol_values.detach().cpu().double().numpy()


def _by_name(total, jac_or_grad, circuit):
  idx = [list(total.symbol_names).index(s) for s in circuit.symbol_names]
  return np.asarray(jac_or_grad)[..., idx]


def test_mirror_general_energy_matches_the_oracle():
  n = 4
  qubits = ir.GridQubit.rect(1, n)
  torch.manual_seed(3)
  circ = models.DirectQuantumCircuit(hea_circuit(qubits, 2, "m"))
  circ_h = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "h"))
  with torch.no_grad():
    circ.trainable_variables[0].uniform_(-1, 1)
    circ_h.trainable_variables[0].uniform_(-1, 1)
  energy = models.BitstringEnergy(list(range(n)), R.mlp_layers(n, 6, 4))
  ham = models.Hamiltonian(energy, circ_h)
  states = torch.tensor([[0, 1, 1, 0], [1, 0, 0, 1], [0, 1, 1, 0], [1, 1, 1, 0]], dtype=torch.int8)
  q = inference.AnalyticQuantumInference(circ, energy_tables="general")
  vals = q.expectation(states, ham)
  assert vals.shape == (4, 1)
  up = torch.tensor([[0.5], [-1.0], [0.25], [2.0]])
  (vals * up.to(vals.device)).sum().backward()
  total, gates, params = _total(circ, ham)
  table64, wts = R.mlp_table_f64(energy, n)
  uniq, idx, _ = O.unique_bitstrings_with_counts(states.numpy())
  v, jac, probs = R.diag_vjp(n, gates, params, uniq, table64.detach().numpy())
  up_u = np.zeros(len(uniq))
  np.add.at(up_u, idx, up.numpy()[:, 0])
  np.testing.assert_allclose(vals.detach().cpu().numpy()[:, 0], v[idx], atol=2e-5)
  g_total = up_u @ jac
  np.testing.assert_allclose(circ.trainable_variables[0].grad.cpu().numpy(), _by_name(total, g_total, circ), atol=2e-5)
  np.testing.assert_allclose(circ_h.trainable_variables[0].grad.cpu().numpy(), _by_name(total, g_total, circ_h), atol=2e-5)
  (table64 * torch.from_numpy(up_u @ probs)).sum().backward()
  for got, want in zip(R.mlp_grads(energy), wts):
    np.testing.assert_allclose(got.grad.cpu().numpy(), want.grad.numpy(), atol=2e-5)


def test_mirror_kobe2_all_matches_off_at_12_qubits():
  n = 12
  qubits = ir.GridQubit.rect(1, n)

  def run(mode):
    torch.manual_seed(12)
    circ = models.DirectQuantumCircuit(hea_circuit(qubits, 2, "m"))
    circ_h = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "h"))
    energy = models.KOBE(list(range(n)), 2)
    with torch.no_grad():
      circ.trainable_variables[0].uniform_(-1, 1)
      circ_h.trainable_variables[0].uniform_(-1, 1)
      energy.post_process[0].kernel.uniform_(-0.5, 0.5)
    states = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (16, n)).astype(np.int8))
    vals = inference.AnalyticQuantumInference(circ, energy_tables=mode).expectation(states, models.Hamiltonian(energy, circ_h))
    vals.sum().backward()
    grads = [energy.post_process[0].kernel.grad, circ.trainable_variables[0].grad, circ_h.trainable_variables[0].grad]
    return vals.detach().cpu().numpy(), [g.cpu().numpy() for g in grads]

  v_off, g_off = run("off")
  v_all, g_all = run("all")
  np.testing.assert_allclose(v_all, v_off, atol=2e-5 * 66)
  for a, b in zip(g_all, g_off):
    np.testing.assert_allclose(a, b, atol=1e-4 * max(1.0, np.abs(b).max()))


class FixedData(data.QuantumData):
  """Data given as bitstring samples through a fixed circuit (qmhl_loss_test.py:206-215's pattern)."""

  def __init__(self, samples, q_infer):
    self.samples, self.q_infer = samples, q_infer

  def expectation(self, observable):
    return torch.mean(self.q_infer.expectation(self.samples, observable))


def test_qmhl_with_an_mlp_model_energy_matches_the_oracle():
  n = 4
  qubits = ir.GridQubit.rect(1, n)
  torch.manual_seed(21)
  data_circuit = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "d"))
  model_circuit = models.DirectQuantumCircuit(hea_circuit(qubits, 2, "m"))
  with torch.no_grad():
    data_circuit.trainable_variables[0].uniform_(-1, 1)
    model_circuit.trainable_variables[0].uniform_(-1, 1)
  data_circuit.trainable_variables[0].requires_grad_(False)
  energy = models.BitstringEnergy(list(range(n)), R.mlp_layers(n, 4, 8))
  qhbm = inference.QHBM(inference.AnalyticEnergyInference(energy, 16, initial_seed=2),
                        inference.AnalyticQuantumInference(model_circuit))
  samples = torch.tensor([[0, 0, 1, 1], [1, 0, 1, 0], [0, 0, 1, 1], [1, 1, 0, 1], [0, 1, 0, 0]], dtype=torch.int8)
  data_q = inference.AnalyticQuantumInference(data_circuit, energy_tables="general")
  loss = inference.qmhl(FixedData(samples, data_q), qhbm)
  loss.backward()
  ham = qhbm.modular_hamiltonian
  total, gates, params = _total(data_circuit, ham)
  table64, wts = R.mlp_table_f64(energy, n)
  _, jac, probs = R.diag_vjp(n, gates, params, samples.numpy(), table64.detach().numpy())
  w = np.full(len(samples), 1.0 / len(samples))
  want = (table64 * torch.from_numpy(w @ probs)).sum() + torch.logsumexp(-table64, 0)
  want.backward()
  assert abs(float(loss) - float(want)) <= 2e-5 * max(1.0, abs(float(want)))
  np.testing.assert_allclose(model_circuit.trainable_variables[0].grad.cpu().numpy(),
                             _by_name(total, w @ jac, model_circuit), atol=2e-5)
  for got, ref in zip(R.mlp_grads(energy), wts):
    np.testing.assert_allclose(got.grad.cpu().numpy(), ref.grad.numpy(), atol=2e-5)


def test_tfq_compat_bit_order_permutes_the_injector_not_the_table():
  n = 12
  qubits = ir.GridQubit.rect(1, n)
  torch.manual_seed(4)
  circ = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "m"), tfq_compat_bit_order=True)
  circ_h = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "h"), tfq_compat_bit_order=True)
  with torch.no_grad():
    circ.trainable_variables[0].uniform_(-1, 1)
    circ_h.trainable_variables[0].uniform_(-1, 1)
  energy = models.BitstringEnergy(list(range(n)), R.mlp_layers(n, 3, 5))
  ham = models.Hamiltonian(energy, circ_h)
  states = torch.from_numpy(np.random.default_rng(3).integers(0, 2, (3, n)).astype(np.int8))
  vals = inference.AnalyticQuantumInference(circ, energy_tables="general").expectation(states, ham)
  vals.sum().backward()
  total, gates, params = _total(circ, ham)
  table = R.mlp_table_f64(energy, n)[0].detach().numpy()
  v, jac, _ = R.diag_vjp(n, gates, params, O.apply_bit_order(states.numpy(), True), table)
  assert not np.array_equal(O.apply_bit_order(states.numpy(), True), states.numpy())
  np.testing.assert_allclose(vals.detach().cpu().numpy()[:, 0], v, atol=2e-5 * np.abs(table).max())
  np.testing.assert_allclose(circ.trainable_variables[0].grad.cpu().numpy(), _by_name(total, jac.sum(0), circ),
                             atol=1e-4 * max(1.0, np.abs(jac.sum(0)).max()))


def test_captured_qmhl_step_with_an_mlp_model_energy_replays_the_eager_bits():
  n, samples = 6, 64
  qubits = ir.GridQubit.rect(1, n)
  torch.manual_seed(6)
  model_circuit = models.DirectQuantumCircuit(hea_circuit(qubits, 2, "qm")).to("cuda")
  energy = models.BitstringEnergy(list(range(n)), R.mlp_layers(n, 4, 6)).to("cuda")
  with torch.no_grad():
    model_circuit.trainable_variables[0].uniform_(-1, 1)
  model = inference.QHBM(inference.AnalyticEnergyInference(energy, samples, initial_seed=6),
                         inference.AnalyticQuantumInference(model_circuit))
  data_circuit = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "qd")).to("cuda")
  data_energy = models.BernoulliEnergy(list(range(n))).to("cuda")
  with torch.no_grad():
    data_circuit.trainable_variables[0].uniform_(-1, 1)
    data_energy.post_process[0].kernel.uniform_(-0.4, 0.4)
  data_qhbm = inference.QHBM(inference.BernoulliEnergyInference(data_energy, samples, initial_seed=4),
                             inference.AnalyticQuantumInference(data_circuit, energy_tables="general"))
  for p in data_qhbm.parameters():
    p.requires_grad_(False)
  variables = list(energy.parameters()) + model_circuit.trainable_variables
  source = data.QHBMData(data_qhbm)
  step = inference.CapturedLoss(lambda: inference.qmhl(source, model), [data_qhbm.e_inference], variables,
                                exact_inferences=[model.e_inference])
  with torch.no_grad():
    drawn = data_qhbm.e_inference.sample(samples).cuda()
  rows, _, counts = utils.unique_bitstrings_with_counts(drawn)
  want_loss = step.eager([(rows, counts)]).clone()
  want = [v.grad.detach().clone() for v in variables]
  for _ in range(2):
    got = step([(rows, counts)])
    torch.cuda.synchronize()
    assert torch.equal(got, want_loss) and all(torch.equal(v.grad, w) for v, w in zip(variables, want))
  assert any(float(w.abs().max()) > 0 for w in want)


def test_timing_script_reports_parity():
  out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "energy_table_time.py"), "--n", "10", "--states", "8",
                        "--energy", "mlp", "--route", "table", "--steps", "2"], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
  assert out.returncode == 0, out.stderr[-2000:]
  line = json.loads(out.stdout.strip().splitlines()[-1])
  for key in ("step_ms", "table_kernel_ms", "table_launches", "model_bytes", "tb_per_s", "parity"):
    assert key in line, key
  assert line["parity"]["ok"], line["parity"]
