"""`qhbm_subsystem_apply` (csrc/subsystem_apply.hip) and the differentiable reduced density matrix of `inference.reduced`
on the GPU, against the complex128 restatement of tests/reduced_density_vjp_ref.py.

1. The kernel through the C ABI on the same complex64 inputs, `out`, `dots` and the scratch pre-filled with NaN.  The bar
   needs no measurement.  A real or imaginary part of an output is a sum of N = 2 * 2^k real products (the real embedding
   Re = A_r phi_r - A_i phi_i, Im = A_r phi_i + A_i phi_r) made as an f32 fused-multiply-add chain: at most N roundings on
   the way of any product, each relative 2^-24 to a partial sum no larger than T = sum |a| |b|, then one more for the
   scale; the second-order term N^2 2^-48 / 2 is below 2^-24 for N <= 2048.  So |got - want| <= (N + 4) 2^-24 |scale_m|
   (Abar phibar)[a, b] with Abar = |Re A| + |Im A|, phibar likewise, in ANY summation order, and it is asserted
   elementwise; `dots`, summed in float64 from the unscaled f32 outputs, is held to the same bound summed against phibar.
   Shapes: those of the issue, both sides of the vector / matrix switch (k = 3 and k = 4), a vector shape of several
   slices and a matrix shape of several column tiles, and one of each with 512 partials per state and component (n = 20
   and 19: the second trip of `subsys_dots_finish`'s row sums; tests/test_wide_states_cpu.py asserts the count).
2. Gradients through the mirror: a depth-2 HEA at 6 qubits (k = 2: the vector kernel) and 12 qubits (k = 5: the matrix
   kernel), `final_states_from_states` -> `reduced_density_matrix(differentiable=True)` -> the three losses, against the
   restatement composed with `tests/final_states_ref.vjp`, at the bar of DESIGN.md 6f / 6l, 1e-4 max(1, ||grad||_inf).
3. An independent oracle on the device: Re tr(rho_A B) for B a Pauli sum on A against `expectation_from_states`.
4. `sampled_ensemble_reduced(differentiable=True)` and the exact-weights recipe.
5. Regressions (the default path's bits) and refusals.
"""
import functools
import types

import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir
from qhbmlib_amd.inference import reduced as reduced_lib
from tests import final_states_ref as F
from tests import from_states_ref as S
from tests import reduced_density_ref as R
from tests import reduced_density_vjp_ref as V
from tests.test_final_states_gpu import _mirror_circuit
from tests.test_from_states_gpu import AMPLITUDE_ATOL, _close, _grad_bar

pytestmark = pytest.mark.gpu

# (n, kept qubits, M)
SHAPES = [
    (3, (0, 1, 2), 2),                                # k = n
    (3, (1,), 1),
    (6, (0, 5), 3),
    (10, (1, 4, 9), 2),                               # k = 3, the last vector size; index bit 0 kept
    (9, (0, 3, 5, 8), 2),                             # k = 4, the first matrix size: one 16-row strip, 16 a' per stage
    (10, (0, 2, 3, 5, 6, 8), 2),                      # index bit 0 not kept
    (11, (0, 2, 4, 6, 10), 2),                        # k = 5: two strips
    (11, (0, 1, 3, 5, 6, 8, 10), 2),                  # seven scattered qubits: two row tiles, a padded column tile
    (12, (0, 1, 2, 3, 4, 5, 6, 7, 8, 9), 2),          # the largest operator, four environment values
    (14, (0, 1, 2, 4, 5, 6, 8, 9, 10, 12), 3),        # several environment blocks
    (12, (3,), 2),                                    # the vector kernel over two slices
    (12, (0, 3, 7, 11), 2),                           # the matrix kernel over four column tiles
    (20, (7,), 2),                                    # the vector kernel over 512 slices: `subsys_dots_finish` sums in two trips
    (19, (0, 6, 12, 18), 2),                          # the matrix kernel, one row tile and 512 column tiles: two trips again
]
SCALES = ["null", "scaled"]


def _f64_bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _raw_apply(states, mask, operator, scale=None, want_dots=True):
  """qhbm_subsystem_apply through the C ABI on NaN-filled out, dots and scratch: (out complex64 [M, 2^n], dots complex128 [M])."""
  lib = E.load_library()
  num, dim = states.shape
  n = dim.bit_length() - 1
  nan = float("nan")
  scratch = torch.full((E.subsystem_apply_scratch_bytes(num, n, mask) // 8,), nan, dtype=torch.float64, device="cuda")
  out = torch.full((num, dim), complex(nan, nan), dtype=torch.complex64, device="cuda")
  dots = torch.full((num, 2), nan, dtype=torch.float64, device="cuda")
  rc = lib.qhbm_subsystem_apply(states.data_ptr(), num, n, mask, operator.data_ptr(), None if scale is None else scale.data_ptr(),
                                out.data_ptr(), dots.data_ptr() if want_dots else None, scratch.data_ptr(),
                                torch.cuda.current_stream().cuda_stream)
  assert rc == 0, lib.qhbm_last_error(None).decode()
  return out.cpu().numpy(), np.ascontiguousarray(dots.cpu().numpy()).view(np.complex128).reshape(num)


@functools.lru_cache(maxsize=None)
def _case(n, kept, num):
  """(complex64 states, complex64 operator, float64 scale with a negative and -- from two states on -- a zero entry) and the
  restatement's (out, dots, out_bound, dots_bound) without and with the scale: one draw and one reference per shape."""
  rng = np.random.default_rng(1000 * n + 10 * len(kept) + num)
  dim, edge = 1 << n, 1 << len(kept)
  states = ((rng.normal(size=(num, dim)) + 1j * rng.normal(size=(num, dim))) / np.sqrt(2 * dim)).astype(np.complex64)
  operator = (rng.normal(size=(edge, edge)) + 1j * rng.normal(size=(edge, edge))).astype(np.complex64)
  scale = np.array([-1.5, 0.0, 0.75])[:num]
  want = {"null": V.apply(states, kept, operator, None), "scaled": V.apply(states, kept, operator, scale)}
  return states, operator, scale, want


def _hold(got, want, bound, label):
  err_re, err_im = np.abs(got.real - want.real), np.abs(got.imag - want.imag)
  live = bound > 0
  worst = max(float(np.max(err_re[live] / bound[live])), float(np.max(err_im[live] / bound[live]))) if live.any() else 0.0
  print(f"{label}: worst {worst:.3g} of the bound, max error {max(err_re.max(), err_im.max()):.3g}")
  assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag)), label
  assert np.all(err_re <= bound) and np.all(err_im <= bound), label


@pytest.mark.parametrize("scaled", SCALES)
@pytest.mark.parametrize("n,kept,num", SHAPES)
def test_kernel_matches_the_restatement(n, kept, num, scaled):
  states, operator, scale, want = _case(n, kept, num)
  want_out, want_dots, out_bar, dots_bar = want[scaled]
  mask = R.keep_mask(kept)
  d_states, d_op = torch.from_numpy(states).cuda(), torch.from_numpy(operator).cuda()
  d_scale = torch.from_numpy(scale).cuda() if scaled == "scaled" else None
  eps = (2.0 * 2.0**len(kept) + 4.0) * 2.0**-24
  label = f"n={n} kept={kept} M={num} {scaled}"
  out, dots = _raw_apply(d_states, mask, d_op, d_scale)
  _hold(out, want_out, eps * out_bar, label + " out")
  _hold(dots, want_dots, eps * dots_bar, label + " dots")
  if scaled == "scaled" and num >= 2:
    assert np.all(out[1] == 0)  # the zero of the scale; dots are taken before scaling
    assert abs(dots[1]) > 0
  # the same bits from a second call, with and without dots, and from the binding (its own scratch)
  again, dots_again = _raw_apply(d_states, mask, d_op, d_scale)
  assert np.array_equal(out.view(np.int64), again.view(np.int64))
  assert np.array_equal(_f64_bits(dots.real), _f64_bits(dots_again.real)) and np.array_equal(_f64_bits(dots.imag), _f64_bits(dots_again.imag))
  without, nans = _raw_apply(d_states, mask, d_op, d_scale, want_dots=False)
  assert np.array_equal(out.view(np.int64), without.view(np.int64)) and np.all(np.isnan(nans.real))
  bound_out, bound_dots = E.subsystem_apply(d_states, mask, d_op, scale=d_scale, want_dots=True)
  assert bound_out.dtype == torch.complex64 and bound_dots.dtype == torch.complex128
  assert np.array_equal(bound_out.cpu().numpy().view(np.int64), out.view(np.int64))
  assert np.array_equal(_f64_bits(bound_dots.cpu().numpy().real), _f64_bits(dots.real))


def test_identity_and_permutation_operators_are_exact():
  """A = 1 returns the states' bits and dots = the squared norm; a permutation matrix with phases moves amplitudes without
  rounding -- on both kernels."""
  for n, kept in [(8, (2, 7)), (10, (0, 3, 4, 8, 9))]:
    rng = np.random.default_rng(n)
    states = ((rng.normal(size=(2, 1 << n)) + 1j * rng.normal(size=(2, 1 << n))) / np.sqrt(2 << n)).astype(np.complex64)
    edge = 1 << len(kept)
    d_states = torch.from_numpy(states).cuda()
    out, dots = _raw_apply(d_states, R.keep_mask(kept), torch.eye(edge, dtype=torch.complex64, device="cuda"))
    assert np.array_equal(out.view(np.int64), states.view(np.int64))
    norm2 = np.sum(states.real.astype(np.float64)**2 + states.imag.astype(np.float64)**2, axis=1)
    rounding = 2.0 * 2.0**n * 2.0**-53  # (at most 2 * 2^n float64 additions on the way of a product, each relative 2^-53)
    np.testing.assert_allclose(dots.real, norm2, rtol=rounding, atol=0)
    assert np.all(np.abs(dots.imag) <= rounding * norm2)
    perm = rng.permutation(edge)
    phases = np.array([1, 1j, -1, -1j])[rng.integers(0, 4, edge)]
    operator = np.zeros((edge, edge), dtype=np.complex64)
    operator[np.arange(edge), perm] = phases
    out, _ = _raw_apply(d_states, R.keep_mask(kept), torch.from_numpy(operator).cuda())
    want, _, _, _ = V.apply(states, kept, operator)
    assert np.array_equal(out, want.astype(np.complex64))


# ---- gradients through the mirror ----------------------------------------------------------------------------------------------
def _torch_loss(kind, rho, aux):
  aux = [torch.from_numpy(np.asarray(a)).to(rho.device) for a in aux]
  if kind == "a":
    return (rho @ aux[0]).diagonal().sum().real
  if kind == "b":
    return (rho * rho.conj()).real.sum()
  if kind == "c":
    return ((rho - aux[0]).abs()**2).sum()
  return (aux[0].conj() * rho).real.sum()


class _MirrorCase:
  """A depth-2 HEA, three complex64 states of norms 0.5, 1, 3 / 2 and weights, with the restatement's rho_A and, per loss,
  (value, gradient of the circuit's parameters, gradient of the weights): computed once per shape."""

  def __init__(self, n, kept, tag):
    self.n, self.kept = n, kept
    self.circ, self.gates, self.params = _mirror_circuit(n, 2, tag, 71 + n)
    self.states64 = (V.random_states(3, n, 72 + n) * np.array([0.5, 1.0, 1.5])[:, None]).astype(np.complex64)
    self.states = self.states64.astype(np.complex128)
    self.weights = np.array([0.5, 0.2, 0.3])
    self.finals = S.final_states(n, self.gates, self.params, self.states)
    self.rho, _ = R.reduced(self.finals, kept, self.weights)
    self.aux, self.want = {}, {}
    for kind in ("a", "b", "c", "lin"):
      self.aux[kind] = V.loss_aux(kind, len(kept), 73 + n)
      value, gamma = V.loss_of(kind, self.rho, self.aux[kind])
      cot, grad_weights = V.vjp(self.finals, self.weights, kept, gamma)
      self.want[kind] = (value, F.vjp(n, self.gates, self.params, self.states, cot), grad_weights, gamma)


@functools.lru_cache(maxsize=None)
def _mirror_case(n, kept):
  return _MirrorCase(n, kept, f"rv{n}")


@pytest.mark.parametrize("n,kept", [(6, (1, 4)), (12, (0, 3, 5, 8, 11))])
def test_mirror_gradients_of_the_three_losses(n, kept):
  c = _mirror_case(n, kept)
  q = inference.AnalyticQuantumInference(c.circ)
  variable = c.circ.trainable_variables[0]
  weights = torch.from_numpy(c.weights).cuda().requires_grad_(True)
  psi = q.final_states_from_states(torch.from_numpy(c.states64))
  rho = inference.reduced_density_matrix((psi, weights), list(reversed(kept)), differentiable=True)
  assert rho.dtype == torch.complex128 and rho.requires_grad
  plain = inference.reduced_density_matrix((psi.detach(), weights.detach()), list(kept))
  assert torch.equal(torch.view_as_real(rho.detach()), torch.view_as_real(plain))  # the same forward bits
  for kind in ("a", "b", "c"):
    want_value, want_theta, want_weights, _ = c.want[kind]
    loss = _torch_loss(kind, rho, c.aux[kind])
    got_theta, got_weights = torch.autograd.grad(loss, [variable, weights], retain_graph=True)
    assert got_weights.dtype == torch.float64
    _close(f"n={n} loss ({kind}) value", loss, want_value, 2e-5 * max(1.0, abs(want_value)))
    _close(f"n={n} loss ({kind}) d/d theta", got_theta, want_theta, _grad_bar(want_theta))
    _close(f"n={n} loss ({kind}) d/d weights", got_weights, want_weights, _grad_bar(want_weights))
    assert np.abs(want_theta).max() > 1e-3 and np.abs(want_weights).max() > 1e-3
  # a complex128 cotangent that is not Hermitian, handed to autograd as it is
  _, want_theta, want_weights, gamma = c.want["lin"]
  got_theta, got_weights = torch.autograd.grad(rho, [variable, weights], grad_outputs=torch.from_numpy(gamma).cuda(), retain_graph=True)
  _close(f"n={n} general Gamma d/d theta", got_theta, want_theta, _grad_bar(want_theta))
  _close(f"n={n} general Gamma d/d weights", got_weights, want_weights, _grad_bar(want_weights))
  # only what requires grad is delivered: the weights alone, from states without a graph
  rho_w = inference.reduced_density_matrix((psi.detach(), weights), list(kept), differentiable=True)
  (only_weights,) = torch.autograd.grad(_torch_loss("b", rho_w, ()), [weights])
  _close(f"n={n} weights alone", only_weights, c.want["b"][2], _grad_bar(c.want["b"][2]))
  # no weights: all ones
  rho_1 = inference.reduced_density_matrix((psi, None), list(kept), differentiable=True)
  ones = np.ones(3)
  rho_ref, _ = R.reduced(c.finals, kept, ones)
  value, gamma = V.loss_of("c", rho_ref, c.aux["c"])
  want = F.vjp(n, c.gates, c.params, c.states, V.vjp(c.finals, ones, kept, gamma)[0])
  (got,) = torch.autograd.grad(_torch_loss("c", rho_1, c.aux["c"]), [variable])
  _close(f"n={n} no weights d/d theta", got, want, _grad_bar(want))


_PAULI = {"X": np.array([[0, 1], [1, 0]], dtype=np.complex128), "Y": np.array([[0, -1j], [1j, 0]]),
          "Z": np.array([[1, 0], [0, -1]], dtype=np.complex128), "I": np.eye(2, dtype=np.complex128)}


@pytest.mark.parametrize("n,kept", [(6, (1, 4)), (12, (0, 3, 5, 8, 11))])
def test_trace_loss_of_a_pauli_sum_is_expectation_from_states(n, kept):
  """sum_m w_m <psi_m|B|psi_m> = Re tr(rho_A B): the Pauli route of the engine (lambda = B psi in the gather kernel, the
  adjoint sweep) against the new route (rho_A, then the operator kernel, then the sweep from cotangent states)."""
  c = _mirror_case(n, kept)
  qubits = sorted(c.circ.qubits)
  terms = [(0.7, {kept[0]: "X", kept[-1]: "Z"}), (-0.4, {kept[-1]: "Y"}), (0.3, {kept[0]: "Z"}), (0.5, {kept[0]: "Y", kept[1]: "Y"})]
  pauli_sum = None
  dense = np.zeros((1 << len(kept),) * 2, dtype=np.complex128)
  for coef, paulis in terms:
    string = ir.PauliString(*[(qubits[q], p) for q, p in paulis.items()], coefficient=coef)
    pauli_sum = ir.PauliSum.from_pauli_strings([string]) if pauli_sum is None else pauli_sum + string
    factor = np.eye(1)
    for q in kept:  # ascending: the first kept qubit is the row index's most significant bit
      factor = np.kron(factor, _PAULI[paulis.get(q, "I")])
    dense += coef * factor
  q = inference.AnalyticQuantumInference(c.circ)
  variable = c.circ.trainable_variables[0]
  states = torch.from_numpy(c.states64)
  weights = torch.from_numpy(c.weights).cuda()
  values = q.expectation_from_states(states, [pauli_sum])
  want_value = (weights * values.double().reshape(-1)).sum()
  (want,) = torch.autograd.grad(want_value, [variable])
  rho = inference.reduced_density_matrix((q.final_states_from_states(states), weights), list(kept), differentiable=True)
  loss = _torch_loss("a", rho, (dense,))
  (got,) = torch.autograd.grad(loss, [variable])
  want = want.cpu().numpy()
  _close(f"n={n} value against the Pauli route", loss, float(want_value.detach()), 2e-5 * max(1.0, sum(abs(t[0]) for t in terms) * 2.25))
  _close(f"n={n} gradient against the Pauli route", got, want, _grad_bar(want))
  assert np.abs(want).max() > 1e-2


def test_sampled_ensemble_differentiable():
  n, kept = 6, (0, 4)
  circ, gates, params = _mirror_circuit(n, 2, "rs", 81)
  model = types.SimpleNamespace(q_inference=inference.AnalyticQuantumInference(circ))
  rng = np.random.default_rng(82)
  bits = np.unique(rng.integers(0, 2, size=(7, n)).astype(np.int8), axis=0)
  counts = rng.integers(1, 20, size=len(bits))
  num_samples = int(counts.sum())
  weights = counts / num_samples
  basis = S.basis_states(bits)
  finals = S.final_states(n, gates, params, basis)
  rho_ref, _ = R.reduced(finals, kept, weights)
  aux = V.loss_aux("c", len(kept), 83)
  _, gamma = V.loss_of("c", rho_ref, aux)
  want = F.vjp(n, gates, params, basis, V.vjp(finals, weights, kept, gamma)[0])
  rho = reduced_lib.sampled_ensemble_reduced(model, torch.from_numpy(bits), torch.from_numpy(counts), num_samples, list(kept),
                                             differentiable=True)
  # (an entry of rho_A from amplitudes within AMPLITUDE_ATOL: 2 ATOL sum_m w_m sum_b |phi_m(a', b)| <= 2 ATOL sqrt(2^(n-k)))
  _close("sampled rho_A", rho, rho_ref, 2 * AMPLITUDE_ATOL * np.sqrt(2.0**(n - len(kept))))
  (got,) = torch.autograd.grad(_torch_loss("c", rho, aux), [circ.trainable_variables[0]])
  _close("sampled d/d theta", got, want, _grad_bar(want))
  assert np.abs(want).max() > 1e-3
  plain = reduced_lib.sampled_ensemble_reduced(model, torch.from_numpy(bits), torch.from_numpy(counts), num_samples, list(kept))
  assert not plain.requires_grad
  _close("sampled rho_A, default path", plain, rho_ref, 2 * AMPLITUDE_ATOL * np.sqrt(2.0**(n - len(kept))))
  # one chunk only: the states must stay resident
  with pytest.raises(ValueError, match="resident"):
    reduced_lib.sampled_ensemble_reduced(model, torch.from_numpy(bits), torch.from_numpy(counts), num_samples, list(kept),
                                         max_state_bytes=(len(bits) - 1) * (8 << n), differentiable=True)


def test_exact_weights_recipe_reaches_theta_and_the_weights():
  """(q_inference.final_states(all bitstrings), probabilities) as a pair: the gradient of the circuit's parameters and of
  the probabilities, held to the restatement."""
  n, kept = 4, (1, 2)
  circ, gates, params = _mirror_circuit(n, 2, "rx", 91)
  q = inference.AnalyticQuantumInference(circ)
  all_bits = np.array([[(x >> (n - 1 - j)) & 1 for j in range(n)] for x in range(1 << n)], dtype=np.int8)
  logits = np.random.default_rng(92).normal(size=1 << n)
  probs = np.exp(-logits) / np.exp(-logits).sum()
  basis = S.basis_states(all_bits)
  finals = S.final_states(n, gates, params, basis)
  rho_ref, _ = R.reduced(finals, kept, probs)
  _, gamma = V.loss_of("b", rho_ref, ())
  cot, want_probs = V.vjp(finals, probs, kept, gamma)
  want_theta = F.vjp(n, gates, params, basis, cot)
  d_probs = torch.from_numpy(probs).cuda().requires_grad_(True)
  rho = inference.reduced_density_matrix((q.final_states(torch.from_numpy(all_bits)), d_probs), list(kept), differentiable=True)
  got_theta, got_probs = torch.autograd.grad(_torch_loss("b", rho, ()), [circ.trainable_variables[0], d_probs])
  _close("exact weights d/d theta", got_theta, want_theta, _grad_bar(want_theta))
  _close("exact weights d/d probabilities", got_probs, want_probs, _grad_bar(want_probs))
  assert np.abs(want_theta).max() > 1e-3


# ---- regressions and refusals ----------------------------------------------------------------------------------------------------
def test_default_path_keeps_its_bits_and_apply_operator_is_the_kernel():
  n, kept = 8, (1, 6)
  rng = np.random.default_rng(8)
  states = torch.from_numpy(((rng.normal(size=(3, 1 << n)) + 1j * rng.normal(size=(3, 1 << n))) / 16).astype(np.complex64)).cuda()
  weights = torch.tensor([0.2, 0.5, 0.3], dtype=torch.float64, device="cuda")
  mask = R.keep_mask(kept)
  direct = E.reduced_density(states, mask, weights)
  for differentiable in (False, True):
    got = inference.reduced_density_matrix((states, weights), list(kept), differentiable=differentiable)
    assert torch.equal(torch.view_as_real(got), torch.view_as_real(direct))
    assert not got.requires_grad
  operator = torch.from_numpy((rng.normal(size=(4, 4)) + 1j * rng.normal(size=(4, 4))).astype(np.complex64))
  applied = inference.apply_operator(states, [6, 1], operator)
  assert applied.shape == states.shape and applied.dtype == torch.complex64 and not applied.requires_grad
  assert torch.equal(torch.view_as_real(applied), torch.view_as_real(E.subsystem_apply(states, mask, operator.cuda())))
  source = data.StateVectorData(states.cpu(), weights.cpu(), ir.GridQubit.rect(1, n))
  by_object = inference.apply_operator(source, [source.qubits[6], source.qubits[1]], operator.to(torch.complex128))
  assert torch.equal(torch.view_as_real(by_object), torch.view_as_real(applied))
  with pytest.raises(ValueError, match="operator must be complex of shape"):
    inference.apply_operator(states, [1], operator)


def test_refused_arguments_return_a_message_and_launch_nothing():
  lib = E.load_library()
  n, num, mask = 8, 2, 0b1001
  dim = 1 << n
  states = torch.ones((2 * num, dim + 2), dtype=torch.complex64, device="cuda").reshape(-1)
  out = torch.full((num * dim + 2,), complex(-7.0, -7.0), dtype=torch.complex64, device="cuda")
  operator = torch.ones(4 * 4 + 1, dtype=torch.complex64, device="cuda")
  scale = torch.ones(num + 1, dtype=torch.float64, device="cuda")
  dots = torch.full((2 * num + 1,), -7.0, dtype=torch.float64, device="cuda")
  scratch = torch.zeros(E.subsystem_apply_scratch_bytes(num, n, mask) // 8 + 1, dtype=torch.float64, device="cuda")
  stream = torch.cuda.current_stream().cuda_stream
  good = dict(s=states.data_ptr(), m=num, n=n, k=mask, a=operator.data_ptr(), c=scale.data_ptr(), o=out.data_ptr(), d=dots.data_ptr(),
              p=scratch.data_ptr())
  refused = [
      (dict(o=states.data_ptr()), "d_out overlaps d_states"),
      (dict(o=states.data_ptr() + 8 * dim * (num - 1) + 16), "d_out overlaps d_states"),   # the last state's tail
      (dict(s=None), "d_states is NULL"),
      (dict(a=None), "d_operator is NULL"),
      (dict(o=None), "d_out is NULL"),
      (dict(p=None), "d_scratch is NULL"),
      (dict(s=states.data_ptr() + 8), "d_states must be 16-byte aligned"),
      (dict(o=out.data_ptr() + 8), "d_out must be 16-byte aligned"),
      (dict(a=operator.data_ptr() + 4), "d_operator must be 8-byte aligned"),
      (dict(c=scale.data_ptr() + 4), "d_scale must be 8-byte aligned"),
      (dict(d=dots.data_ptr() + 4), "d_dots must be 8-byte aligned"),
      (dict(p=scratch.data_ptr() + 4), "d_scratch must be 8-byte aligned"),
      (dict(n=12, k=(1 << 11) - 1), "between 1 and"),     # k = 11
      (dict(k=0), "between 1 and"),
      (dict(k=1 << n), "at or above n_qubits"),
      (dict(m=0), "M must be"),
      (dict(m=65537), "M must be"),
      (dict(n=32), "n_qubits must be"),
  ]
  for change, message in refused:
    a = dict(good, **change)
    rc = lib.qhbm_subsystem_apply(a["s"], a["m"], a["n"], a["k"], a["a"], a["c"], a["o"], a["d"], a["p"], stream)
    assert rc != 0, change
    assert message in lib.qhbm_last_error(None).decode(), (change, lib.qhbm_last_error(None).decode())
  torch.cuda.synchronize()
  assert torch.all(torch.view_as_real(out) == -7.0) and torch.all(dots == -7.0) and torch.all(scratch == 0.0)
  # the good call goes through, NULL scale and dots included
  assert lib.qhbm_subsystem_apply(good["s"], num, n, mask, good["a"], None, good["o"], None, good["p"], stream) == 0
  torch.cuda.synchronize()
  assert torch.all(torch.view_as_real(out[:num * dim]) == 4.0 * torch.tensor([1.0, 0.0], device="cuda"))  # four ones times ones
  assert torch.all(torch.view_as_real(out[num * dim:]) == -7.0) and torch.all(dots == -7.0)
  with pytest.raises(E.EngineError, match="between 1 and"):
    E.subsystem_apply(torch.ones((1, 1 << 12), dtype=torch.complex64, device="cuda"), (1 << 11) - 1,
                      torch.ones((1 << 11, 1 << 11), dtype=torch.complex64))
  with pytest.raises(ValueError, match="scale must have shape"):
    E.subsystem_apply(out[:num * dim].reshape(num, dim), mask, operator[:16].reshape(4, 4), scale=scale)


def test_mirror_refusals_and_double_backward():
  n, kept = 4, (0, 2)
  rng = np.random.default_rng(4)
  host = (rng.normal(size=(2, 1 << n)) + 1j * rng.normal(size=(2, 1 << n))).astype(np.complex64)
  weights = torch.tensor([0.4, 0.6], dtype=torch.float64)
  source = data.StateVectorData(torch.from_numpy(host), weights, ir.GridQubit.rect(1, n))
  with pytest.raises(ValueError, match="carry no graph"):
    inference.reduced_density_matrix(source, [0, 2], differentiable=True)
  with pytest.raises(TypeError, match="pair"):
    inference.reduced_density_matrix(torch.from_numpy(host), [0, 2], differentiable=True)
  with pytest.raises(ValueError, match="twice"):
    inference.reduced_density_matrix((torch.from_numpy(host), weights), [1, 1], differentiable=True)
  # states as a leaf: their gradient is the kernel's output, against the restatement
  states = torch.from_numpy(host).cuda().requires_grad_(True)
  d_weights = weights.cuda().requires_grad_(True)
  rho = inference.reduced_density_matrix((states, d_weights), list(kept), differentiable=True)
  loss = _torch_loss("b", rho, ())
  got_states, got_weights = torch.autograd.grad(loss, [states, d_weights], create_graph=True)
  rho_ref, _ = R.reduced(host, kept, weights.numpy())
  want_states, want_weights = V.vjp(host, weights.numpy(), kept, 2.0 * rho_ref)
  _close("d/d states", got_states, want_states, _grad_bar(want_states))
  _close("d/d weights", got_weights, want_weights, _grad_bar(want_weights))
  with pytest.raises(RuntimeError, match="differentiate twice"):
    got_weights.sum().backward()
