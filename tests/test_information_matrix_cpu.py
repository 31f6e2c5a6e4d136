"""The BKM information matrix and the natural-gradient step on the host: the checkers themselves, the XOR-mask
identity of the EBM block, natural_gradient against numpy, and the error paths (all before any engine call)."""
import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import inference, ir, models
from qhbmlib_amd.inference import information
from tests import info_matrix_ref as R


@pytest.mark.parametrize("n", [2, 3])
def test_reference_loop_equals_the_dense_closed_form(n):
  """The numpy restatement of train.py:161-249 (parameter shift of every variable, adjoint gradient of the copy)
  equals -d^2/d theta_i d theta'_j tr[rho(theta) K(theta')] of dense complex128 matrices; exact mode is symmetric."""
  rng = np.random.default_rng(40 + n)
  gates, names = O.hea_gates(n, 2, "m")
  theta = rng.uniform(-1, 1, len(names))
  sets = O.parity_indices(n, 2)
  phi = rng.uniform(-1, 1, len(sets))
  bits = O.all_bitstrings(n)
  energies = O.parities(bits, sets) @ phi
  weights = np.exp(-energies) / np.exp(-energies).sum()
  ebm, cross, qnn = R.reference_loop(n, gates, theta, phi, sets, O.kobe_shards(n, 2), bits, weights)
  want_cross, want_qnn = R.dense_blocks(n, gates, theta, phi, sets, bits, weights)
  np.testing.assert_allclose(qnn, want_qnn, atol=1e-6)
  np.testing.assert_allclose(cross, want_cross, atol=1e-6)
  m = R.assemble(ebm, cross, qnn, symmetrize=False)
  np.testing.assert_allclose(m, m.T, atol=1e-6)


@pytest.mark.parametrize("kind", ["bernoulli", "kobe"])
def test_xor_mask_second_moment_equals_the_autograd_jacobian(kind):
  """sum_x w(x) parity_a(x) parity_b(x) = sum_x w(x) parity_{a xor b}(x): the EBM block from the distinct XOR masks
  equals the weighted covariance of the energy's autograd Jacobian with respect to its variables."""
  n = 5
  torch.manual_seed(3)
  energy = models.BernoulliEnergy(list(range(n))) if kind == "bernoulli" else models.KOBE(list(range(n)), 3)
  rng = np.random.default_rng(9)
  bits = torch.as_tensor(rng.integers(0, 2, size=(17, n)), dtype=torch.int8)
  w = torch.as_tensor(rng.random(17), dtype=torch.float64)
  w = w / w.sum()
  name = next(k for k, v in energy.named_parameters() if v is energy.post_process[0].kernel)
  kernel = energy.post_process[0].kernel.detach().clone()
  jac = torch.autograd.functional.jacobian(
      lambda k: torch.func.functional_call(energy, {name: k}, (bits,)), kernel).to(torch.float64)
  mu = w @ jac
  want = (jac - mu).T @ (w[:, None] * (jac - mu))
  got = information.energy_covariance(energy, bits, w)
  np.testing.assert_allclose(got.numpy(), want.numpy(), atol=1e-12)


def test_natural_gradient_against_numpy():
  rng = np.random.default_rng(5)
  a = rng.normal(size=(7, 7))
  m = (a + a.T) / 2.0                         # indefinite: the eigenvalue regulariser lifts it
  grads = [torch.as_tensor(rng.normal(size=(3,)), dtype=torch.float32),
           torch.as_tensor(rng.normal(size=(2, 2)), dtype=torch.float32)]
  flat = np.concatenate([g.numpy().reshape(-1) for g in grads]).astype(np.float64)
  for eig, reg, l2 in ((True, 1.0, 1e-2), (False, 0.5, 0.0), (True, 100.0, 1e-3)):
    got = information.natural_gradient(torch.as_tensor(m, dtype=torch.float32), grads, reg=reg, eigval_reg=eig,
                                       l2_regularizer=l2)
    if eig:
      min_eig = float(np.linalg.eigvalsh(m.astype(np.float32)).min())
      r = reg + abs(min(min_eig, 0.0)) if min_eig <= reg else 0.0
    else:
      r = reg
    A = m.astype(np.float32).astype(np.float64) + r * np.eye(7)
    want = np.linalg.solve(A.T @ A + l2 * np.eye(7), A.T @ flat)
    assert [tuple(g.shape) for g in got] == [(3,), (2, 2)]
    np.testing.assert_allclose(np.concatenate([g.numpy().reshape(-1) for g in got]), want, rtol=1e-4, atol=1e-5)
  # a well-conditioned matrix is not lifted (smallest eigenvalue above reg)
  spd = np.eye(7) * 5.0
  got = information.natural_gradient(torch.as_tensor(spd, dtype=torch.float32), grads, reg=1.0, l2_regularizer=0.0)
  np.testing.assert_allclose(np.concatenate([g.numpy().reshape(-1) for g in got]), flat / 5.0, rtol=1e-5)


def _qhbm(q_inference_cls=inference.AnalyticQuantumInference, e_cls=inference.AnalyticEnergyInference, energy=None,
          **q_kwargs):
  n = 3
  qubits = ir.GridQubit.rect(1, n)
  circ = ir.Circuit()
  for i, q in enumerate(qubits):
    circ += ir.X(q)**ir.Symbol(f"a{i}")
  energy = energy if energy is not None else models.KOBE(list(range(n)), 2)
  if q_inference_cls is inference.SampledQuantumInference:
    q_inf = q_inference_cls(models.DirectQuantumCircuit(circ), 10, **q_kwargs)
  else:
    q_inf = q_inference_cls(models.DirectQuantumCircuit(circ), **q_kwargs)
  return inference.QHBM(e_cls(energy, 10), q_inf)


class _NotPauli(models.BitstringEnergy):
  def __init__(self):
    super().__init__([0, 1, 2], [torch.nn.Identity()])


def test_error_paths_raise_before_any_engine_call(monkeypatch):
  def no_engine(*args, **kwargs):
    raise AssertionError("the engine was called")
  monkeypatch.setattr(information, "circuit_blocks", no_engine)
  with pytest.raises(TypeError, match="General Hamiltonians not accepted"):
    information.information_matrix(_qhbm(energy=_NotPauli()))
  with pytest.raises(TypeError, match="SampledQuantumInference"):
    information.information_matrix(_qhbm(inference.SampledQuantumInference))
  with pytest.raises(ValueError, match="not sharded yet"):
    information.information_matrix(_qhbm(process_group=True))
  with pytest.raises(ValueError, match="AnalyticEnergyInference"):
    information.information_matrix(_qhbm(e_cls=inference.BernoulliEnergyInference,
                                         energy=models.BernoulliEnergy([0, 1, 2])))
