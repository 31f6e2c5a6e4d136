"""The adjoint VJP of final states from a caller's cotangent (`qhbm_statevector_vjp_from_states`,
`AnalyticQuantumInference.final_states*`, the table route of `expectation_from_states`) against the
complex128 restatement of tests/final_states_ref.py (GPU only).

Bars are those of tests/test_from_states_gpu.py, unchanged:
  gradients   1e-4 * max(1, ||grad||_inf)
  amplitudes  5e-6 (times max(1, ||phi||) for states that are not normalised, as there)
Every comparison prints its largest error beside its bar before it asserts.  tests/test_final_states_cpu.py holds the
restatement itself to central differences and asserts that under the phase-sensitive loss (B) the global-phase term is
at least 10 % of ||grad||_inf; the larger shapes used only here assert that share themselves.

Not exercised: a cotangent inside the engine's workspace -- no interface hands out an address of the workspace (the
check is `d_states`' own, which tests/test_krylov_gpu.py cannot reach either)."""
import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir, models
from tests import energy_table_ref as T
from tests import final_states_ref as F
from tests import from_states_ref as R
from tests.test_from_states_gpu import AMPLITUDE_ATOL, _c64, _close, _dense_op, _engine, _grad_bar, _passes, _set
from tests.test_host_api import hea_circuit

pytestmark = pytest.mark.gpu


class _Case:
  """A circuit, states and the three losses' cotangents (rounded to complex64: what the engine is given) with the
  restatement's gradients, computed once per shape."""

  def __init__(self, name, num=3, kinds="ABC"):
    self.name = name
    self.n, self.gates, self.params, states = F.case(name, num)
    self.states = _c64(states)
    self.finals = R.final_states(self.n, self.gates, self.params, states)
    self.cot, self.want, self.aux = {}, {}, {}
    for kind in kinds:
      self.aux[kind] = F.loss_aux(kind, num, self.n, F.aux_seed(name))
      _, cot = F.loss_of(kind, self.finals, self.aux[kind])
      self.cot[kind] = _c64(cot)
      cot64 = self.cot[kind].numpy().astype(np.complex128)
      self.want[kind] = F.vjp(self.n, self.gates, self.params, states, cot64)
      if kind == "B":
        share = np.abs(F.phase_term(self.gates, len(self.params), self.finals, cot64)).max() / np.abs(self.want[kind]).max()
        print(f"{name} loss B: phase term / ||grad||_inf = {share:.3f}")
        assert share >= 0.10

  def engine(self, **options):
    return _engine(self.n, self.gates, len(self.params), None, **options)

  def check(self, what, kind, grad):
    _close(f"{self.name} loss {kind} {what}", grad, self.want[kind], _grad_bar(self.want[kind]))


_CASES = {}


def _case(name, num=3, kinds="ABC"):
  key = (name, num, kinds)
  if key not in _CASES:
    _CASES[key] = _Case(name, num, kinds)
  return _CASES[key]


def _dirty(eng, c, seed=5):
  """A call on other data first: whatever the padding of the workspace holds afterwards, it is not zeros."""
  other = _c64(R.random_states(len(c.states), c.n, seed))
  eng.statevector_vjp_from_states(other, np.random.default_rng(seed).uniform(-1, 1, len(c.params)), other)


# ---- 1. padding and one tile, the three losses, states of norms 0.5, 1 and 3 --------------------------------------------------
@pytest.mark.parametrize("kind", ["A", "B", "C"])
@pytest.mark.parametrize("n", [3, 6, 10])
def test_padding_and_one_tile(n, kind):
  c = _case(f"hea{n}")
  eng = c.engine()
  _dirty(eng, c)
  c.check("gradient", kind, eng.statevector_vjp_from_states(c.states, c.params, c.cot[kind]))


# ---- 2. several passes, several chunks: identical bits --------------------------------------------------------------------------
@pytest.mark.parametrize("n,options", [(12, {"tile_qubits": 10, "adjoint_tile_qubits": 10}), (16, {})])
def test_several_passes_and_chunks(n, options):
  c = _case(f"hea{n}", 5, "B")
  eng = c.engine(**options)
  if n == 12:
    fwd, bwd = _passes(eng.describe_schedule_from_states())
    assert fwd > 1 and bwd > 1
  eng.set_option("chunk_states", 2)  # chunks of 2, 2 and 1
  out, grad = eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"], want_states=True)
  c.check("chunked gradient", "B", grad)
  again = eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"])
  assert torch.equal(grad, again)
  assert torch.equal(torch.view_as_real(out), torch.view_as_real(eng.statevector_from_states(c.states, c.params)))
  eng.set_option("chunk_states", 0)
  out0, grad0 = eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"], want_states=True)
  assert torch.equal(grad, grad0)
  assert torch.equal(torch.view_as_real(out), torch.view_as_real(out0))
  scale = np.maximum(np.linalg.norm(c.states.numpy().astype(np.complex128), axis=1), 1.0)
  _close(f"n={n} exported states", out0, c.finals, AMPLITUDE_ATOL * scale[:, None])


# ---- 3. every gate kind: the phase slope of every lowered kind ------------------------------------------------------------------------
def test_all_gate_kinds_under_the_phase_sensitive_loss():
  c = _case("all_kinds")
  eng = c.engine()
  _dirty(eng, c)
  for kind in "BAC":
    c.check("gradient", kind, eng.statevector_vjp_from_states(c.states, c.params, c.cot[kind]))


# ---- 4. norms ------------------------------------------------------------------------------------------------------------------------------
def test_norms_scale_lambda_and_the_phase_term():
  """Loss (B) with a FIXED cotangent is linear in the state: state u alone, at norms 0.5, 1 and 3, gives 0.5, 1 and 3 times
  the restatement's gradient of the unit state -- sweep term (lambda carries ||phi||) and phase term (<g|psi> carries it)."""
  n = 10
  c = _case(f"hea{n}")
  eng = c.engine()
  unit = c.states.numpy().astype(np.complex128)
  unit /= np.linalg.norm(unit, axis=1, keepdims=True)
  cot = c.cot["B"]
  for u, scale in enumerate((0.5, 1.0, 3.0, 0.0)):
    u = u % 3
    state = _c64(unit[u:u + 1] * scale)
    base = F.vjp(n, c.gates, c.params, _c64(unit[u:u + 1]).numpy().astype(np.complex128), cot[u:u + 1].numpy().astype(np.complex128))
    out, grad = eng.statevector_vjp_from_states(state, c.params, cot[u:u + 1], want_states=True)
    _close(f"norm {scale} gradient", grad, scale * base, max(scale, 1e-30) * _grad_bar(base))
    if scale == 0.0:
      assert (grad == 0).all() and (torch.view_as_real(out) == 0).all()


# ---- 5. d_out_states ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 6])
def test_out_states_are_the_bits_of_statevector_from_states(n):
  c = _case(f"hea{n}")
  eng = c.engine()
  want = eng.statevector_from_states(c.states, c.params)
  grad = eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"])
  out, grad_too = eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"], want_states=True)
  assert torch.equal(torch.view_as_real(out), torch.view_as_real(want))
  assert torch.equal(grad, grad_too)  # (the export changes nothing of the gradient)
  _close(f"n={n} exported states", out, c.finals, AMPLITUDE_ATOL * 3.0)


# ---- 6. gradient mask ----------------------------------------------------------------------------------------------------------------
def test_gradient_mask():
  n = 12
  c = _case(f"hea{n}", 5, "B")
  _, names = O.hea_gates(n, 2, "fv")
  first_layer = np.array(["_fv_0_" in name for name in names])
  assert 0 < first_layer.sum() < len(names)
  eng = c.engine(tile_qubits=10, adjoint_tile_qubits=10, adjoint_stop_early=0)
  full = eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"])
  eng.set_gradient_mask(~first_layer)
  masked = eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"])
  keep = torch.from_numpy(~first_layer).cuda()
  differ = int((masked[keep] != full[keep]).sum())
  print(f"masked entries non-zero: {int((masked[~keep] != 0).sum())}; live entries with other bits: {differ}, "
        f"max difference {float((masked[keep] - full[keep]).abs().max()):.3e}")
  assert (masked[~keep] == 0).all()
  assert torch.equal(masked[keep], full[keep])
  eng.set_gradient_mask(None)
  lifted = eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"])
  assert torch.equal(lifted, full)
  c.check("mask lifted", "B", lifted)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry_point():
  n = 6
  c = _case(f"hea{n}")
  eng = c.engine()
  lib, h = eng._lib, eng._h  # pylint: disable=protected-access
  params = torch.from_numpy(c.params.astype(np.float32)).cuda()
  states, cot = c.states.cuda(), c.cot["B"].cuda()
  sv = torch.zeros((3, 1 << n), dtype=torch.complex64, device="cuda")
  grad = torch.ones(len(c.params), dtype=torch.float32, device="cuda")

  def call(states_ptr, num, cot_ptr, out_ptr, grad_ptr=grad.data_ptr()):
    return lib.qhbm_statevector_vjp_from_states(h, states_ptr, num, params.data_ptr(), cot_ptr, out_ptr, grad_ptr, None)

  def refused(rc, text):
    assert rc != 0
    assert text in lib.qhbm_last_error(h).decode(), lib.qhbm_last_error(h).decode()

  refused(call(states.data_ptr(), 3, None, None), "d_cotangent is NULL")
  refused(call(states.data_ptr(), 3, cot.data_ptr() + 8, None), "d_cotangent must be 16-byte aligned")
  refused(call(None, 3, cot.data_ptr(), None), "d_states is NULL")
  refused(call(states.data_ptr(), -1, cot.data_ptr(), None), "negative batch size")
  refused(call(states.data_ptr(), 3, cot.data_ptr(), sv.data_ptr() + 8), "d_out_states must be 16-byte aligned")
  refused(call(states.data_ptr(), 3, cot.data_ptr(), cot.data_ptr()), "d_out_states overlaps")
  refused(call(states.data_ptr(), 3, cot.data_ptr(), None, None), "d_grad is NULL")
  assert (grad == 1).all()  # nothing was written by a refused call
  bare = E.Engine(0)
  assert bare._lib.qhbm_statevector_vjp_from_states(bare._h, states.data_ptr(), 3, params.data_ptr(), cot.data_ptr(), None,  # pylint: disable=protected-access
                                                    grad.data_ptr(), None) != 0
  assert "qhbm_set_circuit has not been called" in bare._lib.qhbm_last_error(bare._h).decode()  # pylint: disable=protected-access
  # no states: the gradient is zero-filled, nothing is read
  assert call(None, 0, None, None) == 0
  torch.cuda.synchronize()
  assert (grad == 0).all()
  with pytest.raises(ValueError):
    eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"][:2])
  with pytest.raises(ValueError):
    eng.statevector_vjp_from_states(c.states, c.params, torch.zeros((3, 1 << n)))
  # the engine is as good as before every refusal; the rows of this call are not served
  c.check("after the refusals", "B", eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"]))
  with pytest.raises(E.EngineError, match="last call was not an adjoint VJP"):
    eng.state_gradients(3)
  # ... whatever an earlier VJP left: a from-states VJP with an observable, then this entry
  with_op = _engine(n, c.gates, len(c.params), [O.tfim_ring_op(n)])
  with_op.expectation_vjp_from_states(c.states, c.params, np.ones((3, 1)))
  assert with_op.state_gradients(3).shape == (3, len(c.params))
  c.check("beside an observable", "B", with_op.statevector_vjp_from_states(c.states, c.params, c.cot["B"]))
  with pytest.raises(E.EngineError, match="last call was not an adjoint VJP"):
    with_op.state_gradients(3)
  # a complex128 cotangent is cast
  got128 = eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"].to(torch.complex128))
  assert torch.equal(got128, eng.statevector_vjp_from_states(c.states, c.params, c.cot["B"]))


# ---- 8. mirror ---------------------------------------------------------------------------------------------------------------------------
def _mirror_circuit(n, layers, name, seed, **kwargs):
  kwargs.setdefault("tfq_compat_bit_order", False)
  circ = models.DirectQuantumCircuit(hea_circuit(ir.GridQubit.rect(1, n), layers, name), **kwargs)
  gates, names = O.hea_gates(n, layers, name)
  assert circ.symbol_names == names
  _set(circ.trainable_variables[0], np.random.default_rng(seed).uniform(-1, 1, len(names)))
  return circ, gates, circ.trainable_variables[0].detach().double().numpy().copy()


@pytest.mark.parametrize("n,tfq_compat", [(6, False), (11, True)])
def test_mirror_final_states_of_bitstrings(n, tfq_compat):
  """(from 11 qubits on the reference's bit order permutes the bitstring columns: the one-hot rows must follow it)"""
  circ, gates, params = _mirror_circuit(n, 2, "fb", 31, tfq_compat_bit_order=tfq_compat)
  q = inference.AnalyticQuantumInference(circ)
  bits = torch.from_numpy(np.random.default_rng(32).integers(0, 2, size=(5, n)).astype(np.int8))
  got = q.final_states(bits)
  assert got.shape == (5, 1 << n) and got.dtype == torch.complex64 and got.requires_grad
  engine_bits = O.apply_bit_order(bits.numpy(), tfq_compat)
  assert np.array_equal(engine_bits, bits.numpy()) != tfq_compat
  eng = _engine(n, gates, len(params), None)
  _close(f"tfq_compat={tfq_compat} final_states against Engine.statevector", got, eng.statevector(engine_bits, params).cpu().numpy(),
         AMPLITUDE_ATOL)
  _close(f"tfq_compat={tfq_compat} final_states against the restatement", got,
         R.final_states(n, gates, params, R.basis_states(engine_bits)), AMPLITUDE_ATOL)


def test_mirror_autograd_through_final_states_from_states():
  n = 6
  circ, gates, params = _mirror_circuit(n, 2, "fm", 33)
  q = inference.AnalyticQuantumInference(circ)
  states64 = R.random_states(3, n, 34).astype(np.complex64)
  states = states64.astype(np.complex128)
  finals = R.final_states(n, gates, params, states)
  psi = q.final_states_from_states(torch.from_numpy(states64))
  _close("final_states_from_states", psi, finals, AMPLITUDE_ATOL)
  variable = circ.trainable_variables[0]
  # (A) and (B) written in torch on the engine's output; the restatement's cotangent on its own finals
  targets_a, coef = F.loss_aux("A", 3, n, 35)
  overlap = (torch.from_numpy(targets_a).to(psi.device).conj() * psi.to(torch.complex128)).sum(1)
  loss_a = (torch.from_numpy(coef).to(psi.device) * (overlap.real**2 + overlap.imag**2)).sum()
  (got_a,) = torch.autograd.grad(loss_a, [variable], retain_graph=True)
  want_value, cot = F.overlap_loss(finals, targets_a, coef)
  want_a = F.vjp(n, gates, params, states, cot)
  _close("loss (A) value", loss_a, want_value, 2e-5 * max(1.0, abs(want_value)))
  _close("loss (A) autograd", got_a, want_a, _grad_bar(want_a))
  targets_b, z = F.loss_aux("B", 3, n, 36)
  overlap = (torch.from_numpy(targets_b).to(psi.device).conj() * psi.to(torch.complex128)).sum(1)
  loss_b = (torch.from_numpy(z).to(psi.device) * overlap).real.sum()
  (got_b,) = torch.autograd.grad(loss_b, [variable], retain_graph=True)
  want_value, cot = F.linear_loss(finals, targets_b, z)
  want_b = F.vjp(n, gates, params, states, cot)
  share = np.abs(F.phase_term(gates, len(params), finals, cot)).max() / np.abs(want_b).max()
  print(f"mirror loss B: phase term / ||grad||_inf = {share:.3f}")
  assert share >= 0.10
  _close("loss (B) value", loss_b, want_value, 2e-5 * max(1.0, abs(want_value)))
  _close("loss (B) autograd", got_b, want_b, _grad_bar(want_b))
  # a complex128 cotangent handed to autograd is accepted
  (got_128,) = torch.autograd.grad(psi, [variable], grad_outputs=torch.from_numpy(cot).to(psi.device), retain_graph=True)
  _close("complex128 cotangent", got_128, want_b, _grad_bar(want_b))
  # refusals of the mirror
  with pytest.raises(ValueError, match="not differentiable"):
    q.final_states_from_states(torch.from_numpy(states64).requires_grad_(True))
  with pytest.raises(ValueError, match="shape"):
    q.final_states_from_states(torch.from_numpy(states64[:, :-1]))
  sharded = inference.AnalyticQuantumInference(circ, process_group=True)
  sharded._group = lambda: object()  # (a group, without initialising torch.distributed for it)  pylint: disable=protected-access
  for call in (lambda: sharded.final_states_from_states(torch.from_numpy(states64)),
               lambda: sharded.final_states(torch.zeros((1, n), dtype=torch.int8))):
    with pytest.raises(ValueError, match="not sharded"):
      call()


# ---- 9. consistency with the routes that exist --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [6, 12])
def test_table_route_from_basis_states_is_the_bitstring_table_route(n):
  """Data that are basis states: `expectation_from_states(one-hot rows, H_mlp)` and its gradients against
  `expectation(bits, H_mlp)` of the existing table route, circuit variables and MLP weights."""
  circ, _, _ = _mirror_circuit(n, 2, "tc", 41)
  circ_h, _, _ = _mirror_circuit(n, 1, "th", 42)
  energy = models.BitstringEnergy(list(range(n)), T.mlp_layers(n, 5, 43))
  ham = models.Hamiltonian(energy, circ_h)
  bits = np.unique(np.random.default_rng(44).integers(0, 2, size=(4, n)).astype(np.int8), axis=0)
  up = torch.from_numpy(np.random.default_rng(45).normal(size=(len(bits), 1))).float().cuda()
  variables = [circ.trainable_variables[0], circ_h.trainable_variables[0]] + T.mlp_grads(energy)
  q = inference.AnalyticQuantumInference(circ, energy_tables="general")
  want = q.expectation(torch.from_numpy(bits), ham)
  want_grads = torch.autograd.grad((want * up).sum(), variables)
  got = q.expectation_from_states(torch.from_numpy(R.basis_states(bits)), ham)
  assert got.shape == want.shape == (len(bits), 1) and got.dtype == want.dtype
  got_grads = torch.autograd.grad((got * up).sum(), variables)
  e_max = float(energy(torch.from_numpy(O.all_bitstrings(n))).detach().abs().max())
  _close(f"n={n} values", got, want.detach().cpu().numpy(), 2e-5 * max(1.0, e_max))
  for name, a, b in zip(("circuit", "Hamiltonian circuit", "W1", "b1", "W2", "b2"), got_grads, want_grads):
    _close(f"n={n} gradient {name}", a, b.cpu().numpy(), _grad_bar(b.cpu().numpy()))


@pytest.mark.parametrize("n", [6, 12])
def test_table_route_of_a_pauli_energy_is_the_pauli_route(n):
  """`energy_tables="all"` sends a BernoulliEnergy through its table on the final states too: values and gradients of the
  Pauli route of `expectation_from_states`, from random states."""
  circ, _, _ = _mirror_circuit(n, 2, "pc", 51)
  circ_h, _, _ = _mirror_circuit(n, 1, "ph", 52)
  energy = models.BernoulliEnergy(list(range(n)))
  energy.build([None, n])
  _set(energy.trainable_variables[0], np.random.default_rng(53).uniform(-1, 1, energy.trainable_variables[0].shape))
  ham = models.Hamiltonian(energy, circ_h)
  states = torch.from_numpy(R.random_states(3, n, 54).astype(np.complex64))
  up = torch.from_numpy(np.random.default_rng(55).normal(size=(3, 1))).float().cuda()
  variables = [circ.trainable_variables[0], circ_h.trainable_variables[0], energy.trainable_variables[0]]
  want = inference.AnalyticQuantumInference(circ).expectation_from_states(states, ham)
  want_grads = torch.autograd.grad((want * up).sum(), variables)
  got = inference.AnalyticQuantumInference(circ, energy_tables="all").expectation_from_states(states, ham)
  got_grads = torch.autograd.grad((got * up).sum(), variables)
  theta_sum = float(energy.trainable_variables[0].detach().abs().sum())
  _close(f"n={n} values", got, want.detach().cpu().numpy(), 2e-5 * max(1.0, theta_sum))
  for name, a, b in zip(("circuit", "Hamiltonian circuit", "energy"), got_grads, want_grads):
    _close(f"n={n} gradient {name}", a, b.cpu().numpy(), _grad_bar(b.cpu().numpy()))
  general = models.BitstringEnergy(list(range(n)), [torch.nn.Linear(n, 1)])
  with pytest.raises(TypeError, match="General Hamiltonians not accepted"):  # "off" stays as it was
    inference.AnalyticQuantumInference(circ).expectation_from_states(states, models.Hamiltonian(general, circ_h))


# ---- 10. the first user: QMHL of an MLP-energy QHBM against state-vector data ----------------------------------------------------------------
def test_qmhl_of_an_mlp_energy_model_from_a_density_matrix():
  """sigma = the thermal state of the TFIM ring at beta = 1 on 4 qubits; the model an MLP energy (the one the general-table
  tests build) under an HEA.  Loss = sum_m w_m sum_y E(y) |<y|U^dagger phi_m>|^2 + log Z restated in float64, value to
  2e-5 * max(1, |loss|) and every gradient block to 2e-5: the bars of
  tests/test_energy_table_gpu.py::test_qmhl_with_an_mlp_model_energy_matches_the_oracle.  Without the table route from
  states this raises TypeError ("General Hamiltonians not accepted"), as it still does with `energy_tables="off"`."""
  n, layers = 4, 2
  h = _dense_op(n, O.tfim_ring_op(n))
  w, v = np.linalg.eigh(h)
  p = np.exp(-(w - w.min()))
  sigma = (v * (p / p.sum())) @ v.conj().T
  circ, gates, phi = _mirror_circuit(n, layers, "qf", 61)
  energy = models.BitstringEnergy(list(range(n)), T.mlp_layers(n, 4, 8))
  model = inference.QHBM(inference.AnalyticEnergyInference(energy, 16, initial_seed=2), inference.AnalyticQuantumInference(circ))
  with pytest.raises(TypeError, match="General Hamiltonians not accepted"):
    inference.qmhl(data.StateVectorData.from_density_matrix(torch.from_numpy(sigma)), model)
  source = data.StateVectorData.from_density_matrix(torch.from_numpy(sigma), energy_tables="general")
  loss = inference.qmhl(source, model)
  loss.backward()
  # the restatement: the states as the engine reads them (complex64), through U^dagger in complex128
  states = source.states.numpy().astype(np.complex64).astype(np.complex128)
  weights = source.weights.numpy()
  inverse = O.inverse_gates(gates)
  finals = R.final_states(n, inverse, phi, states)
  table64, wts = T.mlp_table_f64(energy, n)
  probs = np.abs(finals)**2
  want = (table64 * torch.from_numpy(weights @ probs)).sum() + torch.logsumexp(-table64, 0)
  want.backward()
  _, cot = F.table_loss(finals, table64.detach().numpy(), weights)
  want_phi = F.vjp(n, inverse, phi, states, cot)
  _close("qmhl loss", loss, float(want.detach()), 2e-5 * max(1.0, abs(float(want.detach()))))
  _close("qmhl d/d phi", circ.trainable_variables[0].grad, want_phi, 2e-5)
  for name, got, ref in zip(("W1", "b1", "W2", "b2"), T.mlp_grads(energy), wts):
    _close("qmhl d/d " + name, got.grad, ref.grad.numpy(), 2e-5)
  again = inference.qmhl(source, model)  # the data's inference and its engine are created once
  assert float(again.detach()) == float(loss.detach()) and len(source._inference._engines) == 1  # pylint: disable=protected-access
