"""`qhbm_weighted_gram_vjp` (csrc/gram_vjp.hip) and the differentiable `inference.state_metrics` on the GPU,
against the complex128 restatement of tests/state_metrics_vjp_ref.py.

1. The kernel through the C ABI on the same complex64 / float32 inputs, `out`, `table_grad` and the scratch pre-filled with
   NaN.  The bar needs no measurement.  A real or imaginary part of c_j(x) = sum_i H[i, j] a_i(x) is a sum of N = 2 M real
   products (the real embedding Re = H_r a_r - H_i a_i, Im = H_r a_i + H_i a_r) made as an f32 fused-multiply-add chain: at
   most N roundings on the way of any product, each relative 2^-24 to a partial sum no larger than
   T = sum_i (|Re H_ij| + |Im H_ij|) (|Re a_i| + |Im a_i|), then one more for the table; the second-order term
   N^2 2^-48 / 2 is below 2^-24 for N <= 2048.  So |out - want| <= (2 M + 4) 2^-24 |t(x)| T per part in ANY summation order,
   asserted elementwise; table_grad, summed exactly in float64 from the unscaled f32 c, is held to half the sum over j of
   the same term without t times (|Re a_j| + |Im a_j|).
2. The autograd node `inference.weighted_gram` against the restatement, on both kernels.
3. Gradients through the mirror: two HEA layers with a KOBE-2 or an MLP energy against full-rank and rank-3 data at 4 and 6
   qubits, and one case at 12: the gradients of fidelity, overlap, cross entropy and relative entropy for the circuit's and
   the energy's variables against the restatement composed with `tests/final_states_ref.vjp`, at the bar of DESIGN.md
   6f / 6l / 6m, 1e-4 max(1, ||grad||_inf).
4. An independent route on the device: for normalised data the gradient of `relative_entropy` is that of `qmhl`.
5. Regressions (the default path, the forward bits) and refusals.
"""
import ctypes
import dataclasses
import functools
import importlib

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir, models
from tests import energy_table_ref as T
from tests import final_states_ref as F
from tests import from_states_ref as S
from tests import state_metrics_ref as R
from tests import state_metrics_vjp_ref as V
from tests.test_from_states_gpu import _close, _grad_bar
from tests.test_host_api import hea_circuit
from tests.test_state_metrics_gpu import _datasets, _set

pytestmark = pytest.mark.gpu

metrics_lib = importlib.import_module("qhbmlib_amd.inference.state_metrics")  # (the package exports the function under this name)

# (n, M): one word; less than one slice; exactly one slice (11 qubits = 1024 words) and two; fewer columns than a matrix
# tile; both sides of the switch (8 | 15); a ragged and an exact multiple of 16; several row tiles; the largest M
SHAPES = [(1, 1), (2, 3), (5, 4), (10, 5), (11, 8), (12, 8), (13, 15), (3, 16), (1, 17), (12, 17), (5, 33), (11, 33), (3, 1024)]
TABLES = ["none", "positive", "signed"]
METRICS = ("fidelity", "overlap", "cross_entropy", "relative_entropy")


def _bits32(a):
  return np.ascontiguousarray(a).view(np.int64)


def _bits64(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _raw_vjp(states, table, hermitian, want_states=True, want_table=True):
  """qhbm_weighted_gram_vjp through the C ABI on NaN-filled out, table_grad and scratch: (out complex64 [M, 2^n] numpy,
  table_grad float64 [2^n] numpy)."""
  lib = E.load_library()
  num, dim = states.shape
  n = dim.bit_length() - 1
  nan = float("nan")
  scratch = torch.full((E.gram_vjp_scratch_bytes(num, n) // 8,), nan, dtype=torch.float64, device="cuda")
  out = torch.full((num, dim), complex(nan, nan), dtype=torch.complex64, device="cuda")
  grad = torch.full((dim,), nan, dtype=torch.float64, device="cuda")
  rc = lib.qhbm_weighted_gram_vjp(states.data_ptr(), num, n, None if table is None else table.data_ptr(), hermitian.data_ptr(),
                                  out.data_ptr() if want_states else None, grad.data_ptr() if want_table else None,
                                  scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
  assert rc == 0, lib.qhbm_last_error(None).decode()
  return out.cpu().numpy(), grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(n, num):
  """(complex64 states, a Hermitian complex64 H with one zero row and column, {table name: float32 table or None}): one
  draw per shape."""
  rng = np.random.default_rng(1000 * n + num)
  dim = 1 << n
  states = ((rng.normal(size=(num, dim)) + 1j * rng.normal(size=(num, dim))) / np.sqrt(2 * dim)).astype(np.complex64)
  h = rng.normal(size=(num, num)) + 1j * rng.normal(size=(num, num))
  h = h + h.conj().T
  if num > 1:  # (a single state keeps its one entry)
    h[num // 2, :] = 0
    h[:, num // 2] = 0
  signed = rng.normal(size=dim) * 10.0**rng.uniform(-3, 3, dim)
  signed[rng.integers(0, dim, max(1, dim // 8))] = 0.0
  tables = {"none": None, "positive": rng.uniform(0.05, 1.0, dim).astype(np.float32), "signed": signed.astype(np.float32)}
  return states, h.astype(np.complex64), tables


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("n,num", SHAPES)
def test_kernel_matches_the_restatement(n, num, table):
  states, hermitian, tables = _case(n, num)
  t = tables[table]
  assert np.array_equal(hermitian, hermitian.conj().T)
  d_states, d_h = torch.from_numpy(states).cuda(), torch.from_numpy(hermitian).cuda()
  d_table = None if t is None else torch.from_numpy(t).cuda()
  want_out, want_grad = V.gram_vjp(states, t, hermitian)
  out_bar, grad_bar = V.gram_vjp_bounds(states, t, hermitian)
  eps = (2.0 * num + 4.0) * 2.0**-24
  out, grad = _raw_vjp(d_states, d_table, d_h)
  err = np.maximum(np.abs(out.real - want_out.real), np.abs(out.imag - want_out.imag))
  err_grad = np.abs(grad - want_grad)
  live, live_grad = out_bar > 0, grad_bar > 0
  worst = float(np.max(err[live] / (eps * out_bar[live]))) if live.any() else 0.0
  worst_grad = float(np.max(err_grad[live_grad] / (eps * grad_bar[live_grad]))) if live_grad.any() else 0.0
  print(f"n={n} M={num} {table}: worst out {worst:.3g} table_grad {worst_grad:.3g} of the bound")
  assert np.all(np.isfinite(out.real)) and np.all(np.isfinite(out.imag)) and np.all(np.isfinite(grad))
  assert np.all(err <= eps * out_bar) and np.all(err_grad <= eps * grad_bar)
  assert np.abs(out).max() > 0 and np.abs(grad).max() > 0
  # the same bits from a second call, from calls with one output only, and from the binding (its own scratch)
  again, grad_again = _raw_vjp(d_states, d_table, d_h)
  assert np.array_equal(_bits32(out), _bits32(again)) and np.array_equal(_bits64(grad), _bits64(grad_again))
  only_out, nans = _raw_vjp(d_states, d_table, d_h, want_table=False)
  assert np.array_equal(_bits32(out), _bits32(only_out)) and np.all(np.isnan(nans))
  nans, only_grad = _raw_vjp(d_states, d_table, d_h, want_states=False)
  assert np.array_equal(_bits64(grad), _bits64(only_grad)) and np.all(np.isnan(nans.real))
  bound_out, bound_grad = E.weighted_gram_vjp(d_states, d_table, d_h)
  assert bound_out.dtype == torch.complex64 and bound_grad.dtype == torch.float64
  assert np.array_equal(_bits32(bound_out.cpu().numpy()), _bits32(out)) and np.array_equal(_bits64(bound_grad.cpu().numpy()), _bits64(grad))
  assert E.weighted_gram_vjp(d_states, d_table, d_h, want_states=False)[0] is None
  assert E.weighted_gram_vjp(d_states, d_table, d_h, want_table=False)[1] is None


def test_hand_checks_on_the_device():
  """M = 1, L = G: g = 2 t a and tbar = |a|^2, exactly (one product, no sum); L = Re G_01 and L = Im G_01 move rows."""
  states, _, tables = _case(10, 5)
  t = tables["positive"]
  d_states, d_table = torch.from_numpy(states[:2].copy()).cuda(), torch.from_numpy(t).cuda()
  out, grad = _raw_vjp(d_states[:1], d_table, torch.full((1, 1), 2.0, dtype=torch.complex64, device="cuda"))
  assert np.array_equal(out[0], (2 * states[0]) * t)
  assert np.array_equal(grad, 0.5 * (2.0 * states[0].real.astype(np.float64)**2 + 2.0 * states[0].imag.astype(np.float64)**2))
  for gamma01, factor in ((1.0, 1.0), (1j, 1j)):
    gamma = np.zeros((2, 2), dtype=np.complex64)
    gamma[0, 1] = gamma01
    out, _ = _raw_vjp(d_states, d_table, torch.from_numpy(gamma + gamma.conj().T).cuda())
    assert np.array_equal(out[1], (factor * states[0]).astype(np.complex64) * t)
    assert np.array_equal(out[0], (np.conj(factor) * states[1]).astype(np.complex64) * t)


# ---- the autograd node --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,num", [(6, 5), (12, 8), (7, 17)])
def test_autograd_node_against_the_restatement(n, num):
  states, _, tables = _case(n, num)
  table = tables["signed" if num == 5 else "positive"].astype(np.float64)
  leaf = torch.from_numpy(states).cuda().requires_grad_(True)
  d_table = torch.from_numpy(table).cuda().requires_grad_(True)
  gram = inference.weighted_gram(leaf, d_table)
  assert gram.dtype == torch.complex128 and gram.requires_grad
  plain = E.weighted_gram(leaf.detach(), d_table.detach())
  assert torch.equal(torch.view_as_real(gram.detach()), torch.view_as_real(plain))  # the same forward bits
  table32 = table.astype(np.float32)
  gram_ref = R.gram(states, table32)
  weights = V.loss_aux("quad", num, n)
  # Re tr(W G W G), through torch
  w = torch.from_numpy(weights).cuda()
  loss = ((w[:, None] * gram * w[None, :]) @ gram).diagonal().sum().real
  got_states, got_table = torch.autograd.grad(loss, [leaf, d_table], retain_graph=True)
  assert got_states.dtype == torch.complex64 and got_table.dtype == torch.float64
  want_states, want_table = V.vjp(states, table32, V.quadratic_loss(gram_ref, weights)[1])
  _close(f"n={n} M={num} quadratic d/d states", got_states, want_states, _grad_bar(want_states))
  _close(f"n={n} M={num} quadratic d/d table", got_table, want_table, _grad_bar(want_table))
  # a complex128 cotangent that is not Hermitian, handed to autograd as it is
  gamma = V.loss_aux("lin", num, n + 1)
  got_states, got_table = torch.autograd.grad(gram, [leaf, d_table], grad_outputs=torch.from_numpy(gamma).cuda(), retain_graph=True)
  want_states, want_table = V.vjp(states, table32, gamma)
  _close(f"n={n} M={num} general Gamma d/d states", got_states, want_states, _grad_bar(want_states))
  _close(f"n={n} M={num} general Gamma d/d table", got_table, want_table, _grad_bar(want_table))
  assert np.abs(want_states).max() > 1e-3 and np.abs(want_table).max() > 1e-3
  # only what requires grad is delivered; no table: ones
  gram_t = inference.weighted_gram(leaf.detach(), d_table)
  (only_table,) = torch.autograd.grad(gram_t, [d_table], grad_outputs=torch.from_numpy(gamma).cuda())
  assert torch.equal(only_table, got_table)
  gram_1 = inference.weighted_gram(leaf)
  (only_states,) = torch.autograd.grad((gram_1.abs()**2).sum(), [leaf], create_graph=True)  # sum |G_ij|^2: Gamma = 2 G
  want = V.vjp(states, None, 2.0 * R.gram(states))[0]
  _close(f"n={n} M={num} no table d/d states", only_states, want, _grad_bar(want))
  with pytest.raises(RuntimeError, match="differentiate twice"):
    only_states.abs().sum().backward()


# ---- gradients through the mirror ---------------------------------------------------------------------------------------------
class _Model:
  """Two HEA layers and a KOBE-2 or MLP energy without bit-reversal or bit-flip symmetry, with what the restatement needs:
  the inverse circuit's gate list, the float32 parameter values the model holds, the float64 energies."""

  def __init__(self, n, kind):
    self.n, self.kind = n, kind
    rng = np.random.default_rng(140 + n)
    tag = f"gv{n}{kind}"
    self.circ = models.DirectQuantumCircuit(hea_circuit(ir.GridQubit.rect(1, n), 2, tag))
    gates, names = O.hea_gates(n, 2, tag)
    assert self.circ.symbol_names == names
    _set(self.circ.trainable_variables[0], rng.uniform(-1, 1, len(names)))
    self.params = self.circ.trainable_variables[0].detach().double().numpy().copy()
    self.inverse = O.inverse_gates(gates)
    if kind == "kobe":
      self.energy = models.KOBE(list(range(n)), 2)
      self.energy.build([None, n])
      _set(self.energy.trainable_variables[0], rng.uniform(-1, 1, self.energy.trainable_variables[0].shape))
      self.thetas = self.energy.trainable_variables[0].detach().double().numpy().reshape(-1).copy()
      self.parities = O.parities(O.all_bitstrings(n), O.parity_indices(n, 2)).astype(np.float64)
      self.energies = self.parities @ self.thetas
      self.energy_variables = [self.energy.trainable_variables[0]]
    else:
      self.energy = models.BitstringEnergy(list(range(n)), T.mlp_layers(n, 5, 17 + n) + [torch.nn.Flatten(0)])
      self.table64, self.copies = T.mlp_table_f64(self.energy, n)
      self.energies = self.table64.detach().numpy()
      self.energy_variables = T.mlp_grads(self.energy)
    self.model = models.Hamiltonian(self.energy, self.circ)
    self.variables = [self.circ.trainable_variables[0]] + self.energy_variables

  def energy_gradients(self, ebar):
    """The gradients of the energy's variables for a cotangent of its table."""
    if self.kind == "kobe":
      return [self.parities.T @ ebar]
    return [g.numpy() for g in torch.autograd.grad(self.table64, self.copies, grad_outputs=torch.from_numpy(ebar), retain_graph=True)]

  def reference(self, source):
    """metric -> (value, [gradient of the circuit's parameters] + gradients of the energy's variables)."""
    states = source.states.numpy().astype(np.complex64).astype(np.complex128)  # (as the engine reads them)
    weights = source.weights.numpy().astype(np.float64)
    amplitudes = S.final_states(self.n, self.inverse, self.params, states)
    values = V.metric_values(amplitudes, self.energies, weights)
    out = {}
    for metric, (cot, ebar) in V.metric_gradients(amplitudes, self.energies, weights).items():
      if metric == "relative_entropy":
        out[metric] = (values[metric], out["cross_entropy"][1])
        continue
      out[metric] = (values[metric], [F.vjp(self.n, self.inverse, self.params, states, cot)] + self.energy_gradients(ebar))
    return out


@functools.lru_cache(maxsize=None)
def _model(n, kind):
  return _Model(n, kind)


def _hold_gradients(label, m, source, differentiable_metrics):
  want = m.reference(source)
  for metric in METRICS:
    value, want_grads = want[metric]
    field = getattr(differentiable_metrics, metric)
    assert field.dtype == torch.float64 and field.dim() == 0 and field.requires_grad
    got_grads = torch.autograd.grad(field, m.variables, retain_graph=True)
    # (the bars of tests/test_state_metrics_gpu.py: rtol 1e-4 for fidelity and overlap, 1e-5 max |E| for the entropies)
    value_bar = 1e-4 * abs(value) if metric in ("fidelity", "overlap") else 1e-5 * float(np.abs(m.energies).max())
    _close(f"{label} {metric} value", field, value, value_bar)
    for k, (got, expected) in enumerate(zip(got_grads, want_grads)):
      expected = np.asarray(expected).reshape(tuple(got.shape))
      _close(f"{label} {metric} d/d variable {k}", got, expected, _grad_bar(expected))
    # (the check is not of zeros; fidelity and overlap of random data fall with 2^-n, the entropies do not)
    floor = 1e-3 if metric in ("cross_entropy", "relative_entropy") else 1e-5
    assert np.abs(want_grads[0]).max() > floor and max(np.abs(g).max() for g in want_grads[1:]) > floor


@pytest.mark.parametrize("kind", ["kobe", "mlp"])
@pytest.mark.parametrize("n", [4, 6])
def test_mirror_gradients_of_the_four_metrics(n, kind):
  m = _model(n, kind)
  for name, (source, _) in _datasets(n).items():
    if name == "weighted":
      continue
    plain = inference.state_metrics(m.model, source)
    got = inference.state_metrics(m.model, source, differentiable=True)
    assert all(isinstance(getattr(plain, f.name), float) for f in dataclasses.fields(plain))  # the default path is as it was
    for field in dataclasses.fields(plain):
      value = getattr(got, field.name)
      assert torch.is_tensor(value) and value.dtype == torch.float64 and value.dim() == 0, field.name
      np.testing.assert_allclose(float(value), getattr(plain, field.name), rtol=1e-12, atol=0, err_msg=field.name)
    assert not (got.trace.requires_grad or got.purity.requires_grad or got.entropy.requires_grad)
    _hold_gradients(f"n={n} {kind} {name}", m, source, got)
    assert float(source.fidelity(m.model, differentiable=True)) == float(got.fidelity)
    assert float(source.relative_entropy(m.model, differentiable=True)) == float(got.relative_entropy)
    assert source.metrics(m.model, differentiable=True).overlap.requires_grad


def test_mirror_gradients_at_twelve_qubits():
  """Nine unnormalised states: the matrix kernel with a ragged row strip over 64 column tiles."""
  n = 12
  m = _model(n, "kobe")
  rng = np.random.default_rng(12)
  states = rng.normal(size=(9, 1 << n)) + 1j * rng.normal(size=(9, 1 << n))
  states *= rng.uniform(0.5, 1.0, (9, 1)) / np.linalg.norm(states, axis=1, keepdims=True)
  source = data.StateVectorData(torch.from_numpy(states), torch.from_numpy(rng.uniform(0.05, 0.15, 9)))
  _hold_gradients("n=12 kobe nine states", m, source, inference.state_metrics(m.model, source, differentiable=True))


@pytest.mark.parametrize("n", [4, 6])
def test_differentiable_gram_matrices_have_the_bits_of_the_default_path(n):
  m = _model(n, "kobe")
  source, _ = _datasets(n)["rank_3"]
  device = torch.device("cuda", torch.cuda.current_device())
  states = source._device_states()  # pylint: disable=protected-access
  with torch.no_grad():
    eng, values = metrics_lib._inverse_circuit_engine(m.model, device)  # pylint: disable=protected-access
    plain_amps = eng.statevector_from_states(states, values)
    energies = models.energy_utils.energy_table(m.model.energy, n).detach().to(device)
    _, probs = metrics_lib._partition(energies)  # pylint: disable=protected-access
  q = metrics_lib._inverse_circuit_inference(m.model)  # pylint: disable=protected-access
  assert q is metrics_lib._inverse_circuit_inference(m.model)  # pylint: disable=protected-access  (one per model object)
  amps = q.final_states_from_states(states)
  assert amps.requires_grad and torch.equal(torch.view_as_real(amps.detach()), torch.view_as_real(plain_amps))
  table = models.energy_utils.energy_table(m.model.energy, n).to(device)
  e64 = table.to(torch.float64)
  p64 = torch.exp(-e64 - torch.logsumexp(-e64, 0))
  for t_plain, t_node in ((probs, p64), (energies, table)):
    node = inference.weighted_gram(amps, t_node)
    assert node.requires_grad
    assert torch.equal(torch.view_as_real(node.detach()), torch.view_as_real(E.weighted_gram(plain_amps, t_plain)))


# ---- an independent route on the device -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["kobe", "mlp"])
def test_relative_entropy_gradient_is_the_qmhl_gradient(kind):
  """Normalised data: D(sigma || rho) = qmhl - S(sigma), so the two device routes -- the Pauli route (KOBE) or the table on
  the final states (`energy_tables="general"`, MLP) against the Gram VJP -- give one gradient."""
  n = 6
  m = _model(n, kind)
  sigma = _datasets(n)["rank_3"][1]
  source = data.StateVectorData.from_density_matrix(torch.from_numpy(sigma), energy_tables="general" if kind == "mlp" else "off")
  np.testing.assert_allclose(float(source.weights.sum()), 1.0, rtol=0, atol=1e-12)
  qhbm = inference.QHBM(inference.AnalyticEnergyInference(m.energy, 16, initial_seed=3), inference.AnalyticQuantumInference(m.circ))
  loss = inference.qmhl(source, qhbm)
  want = [g.detach().cpu().numpy() for g in torch.autograd.grad(loss, m.variables)]
  got_metrics = inference.state_metrics(m.model, source, differentiable=True)
  got = torch.autograd.grad(got_metrics.relative_entropy, m.variables)
  _close(f"{kind} relative entropy + S(sigma) against qmhl", got_metrics.relative_entropy + got_metrics.entropy, float(loss.detach()),
         2e-5 * max(1.0, float(np.abs(m.energies).max())))
  for k, (a, b) in enumerate(zip(got, want)):
    _close(f"{kind} d/d variable {k} against qmhl", a, b, _grad_bar(b))
  assert np.abs(want[0]).max() > 1e-3


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_refused_arguments_return_a_message_and_launch_nothing():
  lib = E.load_library()
  n, num = 6, 4
  dim = 1 << n
  states = torch.ones((2 * num, dim + 2), dtype=torch.complex64, device="cuda").reshape(-1)
  out = torch.full((num * dim + 2,), complex(-7.0, -7.0), dtype=torch.complex64, device="cuda")
  table = torch.ones(dim + 2, dtype=torch.float32, device="cuda")
  hermitian = torch.ones(num * num + 1, dtype=torch.complex64, device="cuda")
  grad = torch.full((dim + 1,), -7.0, dtype=torch.float64, device="cuda")
  scratch = torch.zeros(E.gram_vjp_scratch_bytes(num, n) // 8 + 1, dtype=torch.float64, device="cuda")
  stream = torch.cuda.current_stream().cuda_stream
  good = dict(s=states.data_ptr(), m=num, n=n, t=table.data_ptr(), h=hermitian.data_ptr(), o=out.data_ptr(), g=grad.data_ptr(),
              p=scratch.data_ptr())
  refused = [
      (dict(m=0), "M must be in [1, 1024]"), (dict(m=-1), "M must be"), (dict(m=1025), "M must be"),
      (dict(n=0), "n_qubits must be in [1, 31]"), (dict(n=32), "n_qubits must be"),
      (dict(s=None), "d_states is NULL"), (dict(h=None), "d_cotangent is NULL"), (dict(p=None), "d_scratch is NULL"),
      (dict(o=None, g=None), "both NULL"),
      (dict(s=states.data_ptr() + 8), "d_states must be 16-byte aligned"),
      (dict(o=out.data_ptr() + 8), "d_out_states must be 16-byte aligned"),
      (dict(t=table.data_ptr() + 4), "d_table must be 8-byte aligned"),
      (dict(h=hermitian.data_ptr() + 4), "d_cotangent must be 8-byte aligned"),
      (dict(g=grad.data_ptr() + 4), "d_table_grad must be 8-byte aligned"),
      (dict(p=scratch.data_ptr() + 4), "d_scratch must be 8-byte aligned"),
      (dict(o=states.data_ptr()), "d_out_states overlaps d_states"),
      (dict(o=states.data_ptr() + 8 * dim * (num - 1) + 16), "d_out_states overlaps d_states"),   # the last state's tail
  ]
  for change, message in refused:
    a = dict(good, **change)
    rc = lib.qhbm_weighted_gram_vjp(a["s"], a["m"], a["n"], a["t"], a["h"], a["o"], a["g"], a["p"], stream)
    assert rc != 0, change
    assert message in lib.qhbm_last_error(None).decode(), (change, lib.qhbm_last_error(None).decode())
  torch.cuda.synchronize()
  assert torch.all(torch.view_as_real(out) == -7.0) and torch.all(grad == -7.0) and torch.all(scratch == 0.0)
  # the good call goes through, NULL table included: c_j = sum of four ones times ones, tbar = 1/2 * 4 * 4
  assert lib.qhbm_weighted_gram_vjp(good["s"], num, n, None, good["h"], good["o"], good["g"], good["p"], stream) == 0
  torch.cuda.synchronize()
  assert torch.all(torch.view_as_real(out[:num * dim]) == 4.0 * torch.tensor([1.0, 0.0], device="cuda"))
  assert torch.all(torch.view_as_real(out[num * dim:]) == -7.0)
  assert torch.all(grad[:dim] == 8.0) and grad[dim] == -7.0
  size = ctypes.c_size_t()
  for bad_m, bad_n in [(0, 6), (1025, 6), (4, 0), (4, 32)]:
    assert lib.qhbm_gram_vjp_scratch_bytes(bad_m, bad_n, ctypes.byref(size)) != 0


def test_binding_and_mirror_refusals():
  states = torch.ones((3, 16), dtype=torch.complex64, device="cuda")
  table = torch.ones(16, dtype=torch.float32, device="cuda")
  hermitian = torch.eye(3, dtype=torch.complex64)
  with pytest.raises(E.EngineError, match="CUDA states"):
    E.weighted_gram_vjp(states.cpu(), None, hermitian)
  with pytest.raises(ValueError, match="neither output"):
    E.weighted_gram_vjp(states, table, hermitian, want_states=False, want_table=False)
  with pytest.raises(ValueError, match="table must have shape"):
    E.weighted_gram_vjp(states, table[:8], hermitian)
  with pytest.raises(E.EngineError, match="table on the states' device"):
    E.weighted_gram_vjp(states, table.cpu(), hermitian)
  with pytest.raises(ValueError, match="cotangent must be complex of shape"):
    E.weighted_gram_vjp(states, table, torch.eye(2, dtype=torch.complex64))
  with pytest.raises(ValueError, match="cotangent must be complex of shape"):
    E.weighted_gram_vjp(states, table, torch.eye(3))
  with pytest.raises(ValueError, match="power of two"):
    E.weighted_gram_vjp(states[:, :12], None, hermitian)
  with pytest.raises(E.EngineError, match="CUDA states"):
    inference.weighted_gram(states.cpu())
  with pytest.raises(ValueError, match="table must have shape"):
    inference.weighted_gram(states, table[:8])
  with pytest.raises(ValueError, match="real floating-point"):
    inference.weighted_gram(states, table.to(torch.complex64))
  with pytest.raises(E.EngineError, match="table on the states' device"):
    inference.weighted_gram(states, table.cpu())
  m = _model(4, "kobe")
  leaf = torch.ones((2, 16), dtype=torch.complex64).requires_grad_(True)
  source = data.StateVectorData(leaf)  # (the constructor detaches: only states put there afterwards can carry a graph)
  source.states = leaf
  with pytest.raises(ValueError, match="require grad"):
    inference.state_metrics(m.model, source, differentiable=True)
  with pytest.raises(TypeError, match="StateVectorData"):
    inference.state_metrics(m.model, (leaf.detach(), None), differentiable=True)
  with pytest.raises(ValueError, match="qubits"):
    inference.state_metrics(m.model, data.StateVectorData(torch.ones((2, 32), dtype=torch.complex64)), differentiable=True)
  # double backward is refused
  source = _datasets(4)["rank_3"][0]
  fidelity = inference.state_metrics(m.model, source, differentiable=True).fidelity
  (g,) = torch.autograd.grad(fidelity, [m.variables[1]], create_graph=True)
  with pytest.raises(RuntimeError, match="differentiate twice"):
    g.sum().backward()
  # and the default call still reports python floats
  assert isinstance(inference.state_metrics(m.model, source).fidelity, float)
