"""Circuits that start from caller-supplied states (`qhbm_*_from_states`, `AnalyticQuantumInference.expectation_from_states`,
`data.StateVectorData`) against the complex128 restatement of tests/from_states_ref.py (GPU only).

Tolerances are those tests/test_engine_gpu.py holds the bits calls to at these sizes, scaled by the squared norm of the
states where they are not normalised:
  values     2e-5 * max(1, sum|c_k|) * ||phi||^2
  gradients  1e-4 * max(1, ||grad||_inf)
Amplitudes: 5e-6, the bar of the `statevector` comparisons in tests/test_engine_gpu.py
(`np.testing.assert_allclose(row, O.simulate(...).ravel(), atol=5e-6)`).
Every comparison prints its largest error beside its bar before it asserts.
"""
import itertools
import re

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir, models
from tests import from_states_ref as R
from tests import golden_util as G
from tests.test_host_api import hea_circuit

pytestmark = pytest.mark.gpu

AMPLITUDE_ATOL = 5e-6  # tests/test_engine_gpu.py, the statevector comparisons


def _ops(n, seed):
  return [O.tfim_ring_op(n), O.random_pauli_op(n, 12, seed)]


def _value_bar(ops, norm2=1.0):
  return 2e-5 * np.array([max(1.0, R.op_abs_sum(op)) for op in ops])[None, :] * np.reshape(norm2, (-1, 1))


def _grad_bar(want):
  return 1e-4 * max(1.0, float(np.abs(want).max()))


def _close(what, got, want, bar):
  got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
  err = np.abs(got - want)
  print(f"{what}: max error {err.max(initial=0.0):.3e}  bar {np.min(bar):.3e}")
  assert np.isfinite(got).all(), what
  assert (err <= bar).all(), (what, float(err.max()), float(np.min(bar)))


def _engine(n, gates, n_params, ops, **options):
  eng = E.Engine(0)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(n, gates, n_params)
  if ops:
    eng.set_observables(ops)
  return eng


def _c64(states):
  return torch.from_numpy(np.asarray(states).astype(np.complex64))


class _Case:
  """Circuit, operators, states and upstream of one shape, with the restatement's values, rows and gradient computed
  once on the complex64-rounded states (what the engine is given)."""

  def __init__(self, n, layers, num, seed, gates=None, n_params=None, states=None):
    rng = np.random.default_rng(seed)
    if gates is None:
      gates, names = O.hea_gates(n, layers, "fs")
      n_params = len(names)
    self.n, self.gates, self.n_params = n, gates, n_params
    self.params = rng.uniform(-1, 1, n_params)
    self.ops = _ops(n, seed + 1)
    self.states = _c64(R.random_states(num, n, seed + 2) if states is None else states)
    self.upstream = rng.normal(size=(num, len(self.ops)))
    self.want_vals, self.want_rows = R.values_and_rows(n, gates, self.params, self.states.numpy().astype(np.complex128),
                                                       self.ops, self.upstream)
    self.want_grad = self.want_rows.sum(0)

  def engine(self, **options):
    return _engine(self.n, self.gates, self.n_params, self.ops, **options)

  def check(self, what, vals, grad, norm2=1.0):
    _close(what + " values", vals, self.want_vals, _value_bar(self.ops, norm2))
    _close(what + " gradient", grad, self.want_grad, _grad_bar(self.want_grad))


def _passes(text):
  """(forward, backward) pass counts of a schedule description."""
  return tuple(int(x) for x in re.findall(r"plan: n=\d+ n_eff=\d+ tile_bits=\d+ round_bits=\d+ passes=(\d+)", text))


_CASES = {}


def _case(key, *args, **kwargs):
  if key not in _CASES:
    _CASES[key] = _Case(*args, **kwargs)
  return _CASES[key]


# ---- 1. padding and one tile --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 6, 10])
def test_padding_and_one_tile(n):
  c = _case(("one", n), n, 2, 3, 100 + n)
  eng = c.engine()
  vals, grad = eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  c.check(f"n={n}", vals, grad)
  _close(f"n={n} forward-only values", eng.expectation_from_states(c.states, c.params), c.want_vals, _value_bar(c.ops))


# ---- 2. several passes, several chunks; 8. rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,options", [(12, {"tile_qubits": 10, "adjoint_tile_qubits": 10}), (16, {})])
def test_several_passes_and_chunks(n, options):
  c = _case(("multi", n), n, 3, 5, 200 + n)
  eng = c.engine(**options)
  if n == 12:
    fwd, bwd = _passes(eng.describe_schedule_from_states())
    assert fwd > 1 and bwd > 1
  eng.set_option("chunk_states", 2)  # chunks of 2, 2 and 1
  vals, grad = eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  c.check(f"n={n} chunked", vals, grad)
  rows = eng.state_gradients(5)  # (the header's promise for the bits call: the rows of the last adjoint VJP sum to d_grad)
  _close(f"n={n} rows", rows, c.want_rows, _grad_bar(c.want_grad))
  # (fp32 sums of a few hundred slot values per parameter, in two orders: 2^-24 per addition of the sum of magnitudes)
  _close(f"n={n} rows sum", rows.double().sum(0), grad.double().cpu().numpy(), 64 * 2.0**-24 * max(1.0, float(np.abs(c.want_rows).sum(0).max())))
  again_vals, again_grad = eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  assert torch.equal(vals, again_vals) and torch.equal(grad, again_grad)
  forward_vals = eng.expectation_from_states(c.states, c.params)
  _close(f"n={n} chunked forward-only", forward_vals, c.want_vals, _value_bar(c.ops))
  eng.set_option("chunk_states", 0)
  vals0, grad0 = eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  c.check(f"n={n} one chunk", vals0, grad0)
  _close(f"n={n} one chunk forward-only", eng.expectation_from_states(c.states, c.params), c.want_vals, _value_bar(c.ops))


# ---- 3. no pruning where the basis-state plans prune ---------------------------------------------------------------------
def _spectator_circuit(n, idle, diagonal):
  """HEA-like layers in which qubit `idle` has no gate and qubit `diagonal` only Z powers and CZ powers."""
  gates, p = [], 0
  for _ in range(3):
    for q in range(n):
      if q == idle:
        continue
      if q != diagonal:
        gates.append((E.GATE_XPOW, q, -1, p, 1.0, 0.0))
        p += 1
      gates.append((E.GATE_ZPOW, q, -1, p, 1.0, 0.0))
      p += 1
    for start in (0, 1):
      for q0 in range(start, n - 1, 2):
        if idle in (q0, q0 + 1):
          continue
        gates.append((E.GATE_CZPOW, q0, q0 + 1, p, 1.0, 0.0))
        p += 1
  return gates, p


@pytest.mark.parametrize("idle,diagonal", [(0, 11), (11, 0)])
def test_nothing_is_pruned_on_a_dirty_workspace(idle, diagonal):
  """Qubit q is index bit n - 1 - q: the two sub-cases put the gate-free qubit among the highest and the diagonal-only one
  among the lowest index bits, and the other way round.  The basis-state plans zero-fill, skip tiles and clear stale
  halves on exactly these bits; random states carry weight on both of their values.  The workspace is dirty: the same
  engine first runs a bits VJP on five bitstrings."""
  n = 12
  gates, n_params = _spectator_circuit(n, idle, diagonal)
  c = _case(("spectator", idle), n, 0, 5, 300 + idle, gates=gates, n_params=n_params)
  eng = c.engine(tile_qubits=10, adjoint_tile_qubits=10)
  fwd, bwd = _passes(eng.describe_schedule_from_states())
  assert fwd > 1 and bwd > 1
  rng = np.random.default_rng(7)
  bits = rng.integers(0, 2, size=(5, n)).astype(np.int8)
  eng.expectation_vjp(bits, rng.uniform(-1, 1, n_params), rng.normal(size=(5, len(c.ops))))
  vals, grad = eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  c.check(f"idle={idle}", vals, grad)
  eng.expectation_vjp(bits, rng.uniform(-1, 1, n_params), rng.normal(size=(5, len(c.ops))))
  _close(f"idle={idle} forward-only", eng.expectation_from_states(c.states, c.params), c.want_vals, _value_bar(c.ops))
  eng.expectation_vjp(bits, rng.uniform(-1, 1, n_params), rng.normal(size=(5, len(c.ops))))
  got = eng.statevector_from_states(c.states, c.params).cpu().numpy()
  _close(f"idle={idle} states", got, R.final_states(n, gates, c.params, c.states.numpy().astype(np.complex128)), AMPLITUDE_ATOL)


# ---- 4. basis states agree with the bits call ------------------------------------------------------------------------------
def test_basis_states_agree_with_the_bits_call():
  n = 12
  bits = np.random.default_rng(41).integers(0, 2, size=(5, n)).astype(np.int8)
  c = _case("basis", n, 3, 5, 400, states=R.basis_states(bits))
  want_vals, want_jac = O.expectation_jacobian(n, c.gates, c.params, bits, c.ops)
  np.testing.assert_allclose(c.want_vals, want_vals, rtol=0, atol=1e-12)
  fresh = c.engine(tile_qubits=10, adjoint_tile_qubits=10)
  fresh_vals = fresh.expectation(bits, c.params)
  fresh_vjp = fresh.expectation_vjp(bits, c.params, c.upstream)
  eng = c.engine(tile_qubits=10, adjoint_tile_qubits=10)
  vals, grad = eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  c.check("basis states", vals, grad)
  _close("from-states against bits values", vals, fresh_vjp[0].cpu().numpy(), _value_bar(c.ops))
  _close("from-states against bits gradient", grad, fresh_vjp[1].cpu().numpy(), _grad_bar(c.want_grad))
  _close("forward-only", eng.expectation_from_states(c.states, c.params), c.want_vals, _value_bar(c.ops))
  # the two plan sets do not disturb each other: the bits calls of this engine are a fresh engine's, bit for bit
  builds = eng.plan_builds()
  assert torch.equal(eng.expectation(bits, c.params), fresh_vals)
  after_vals, after_grad = eng.expectation_vjp(bits, c.params, c.upstream)
  assert torch.equal(after_vals, fresh_vjp[0]) and torch.equal(after_grad, fresh_vjp[1])
  assert eng.plan_builds() == (builds[0] + 1, builds[1] + 1) == fresh.plan_builds()
  eng.expectation_from_states(c.states, c.params)
  assert eng.plan_builds() == fresh.plan_builds()  # (the dense-start plans were cached, and are not counted here)


# ---- 5. composition, global phase included -----------------------------------------------------------------------------------
def _composition(n, gates, n_params, params, bits, options):
  half = len(gates) // 2
  a = _engine(n, gates[:half], n_params, None, **options)
  b = _engine(n, gates[half:], n_params, None, **options)
  whole = _engine(n, gates, n_params, None, **options)
  mid = a.statevector(bits, params)
  got = b.statevector_from_states(mid, params).cpu().numpy()
  _close(f"n={n} B(A|x>) against (A + B)|x>", got, whole.statevector(bits, params).cpu().numpy(), AMPLITUDE_ATOL)
  want = np.stack([O.simulate(n, gates, params, list(x)).ravel() for x in bits])
  _close(f"n={n} B(A|x>) against the oracle", got, want, AMPLITUDE_ATOL)


def test_composition_of_all_gate_kinds():
  g = G.load("all_kinds_n5.npz")
  _composition(int(g["n"]), G.gates_of(g["gates"]), len(g["params"]), g["params"], g["bits"], {})


def test_composition_of_hea_halves_over_several_passes():
  n = 12
  gates, names = O.hea_gates(n, 4, "cmp")
  rng = np.random.default_rng(55)
  _composition(n, gates, len(names), rng.uniform(-1, 1, len(names)), rng.integers(0, 2, size=(3, n)).astype(np.int8),
               {"tile_qubits": 10})


def test_a_circuit_without_gates_returns_the_states():
  """No gate, no pass: the import (normalise, pad) and the export (rescale) alone, on 11 qubits and on 3 (padding)."""
  for n in (11, 3):
    eng = _engine(n, [], 0, None)
    states = _c64(2.0 * R.random_states(3, n, 70 + n))
    got = eng.statevector_from_states(states, np.zeros(0, np.float32)).cpu().numpy()
    _close(f"n={n} identity", got, states.numpy(), 2.0 * AMPLITUDE_ATOL)  # (states of norm 2: the bar scales with ||phi||)


# ---- 6. norms ----------------------------------------------------------------------------------------------------------------
def test_norms_scale_values_and_gradients():
  n = 10
  unit = R.random_states(4, n, 61)
  scale = np.array([0.5, 3.0, 0.0, 1.0])
  c = _case("norms", n, 2, 4, 600, states=unit * scale[:, None])
  norm2 = np.linalg.norm(c.states.numpy().astype(np.complex128), axis=1)**2
  np.testing.assert_allclose(norm2, scale**2, atol=1e-6)
  base_vals, base_rows = R.values_and_rows(n, c.gates, c.params, _c64(unit).numpy().astype(np.complex128), c.ops, c.upstream)
  # the restatement itself scales by 0.25 and 9 (up to the complex64 rounding of 3 phi: 1.2e-7 relative)
  np.testing.assert_allclose(c.want_vals, base_vals * (scale**2)[:, None], atol=1e-4)
  np.testing.assert_allclose(c.want_rows, base_rows * (scale**2)[:, None], atol=1e-4)
  eng = c.engine()
  dev_states = c.states.cuda()
  before = dev_states.clone()
  vals, grad = eng.expectation_vjp_from_states(dev_states, c.params, c.upstream)
  rows = eng.state_gradients(4)
  assert torch.equal(torch.view_as_real(dev_states), torch.view_as_real(before))  # the input is only read
  bar2 = np.maximum(norm2, 0.0)
  _close("scaled values", vals, c.want_vals, _value_bar(c.ops, bar2))
  for u in range(4):
    _close(f"scaled row {u}", rows[u], c.want_rows[u], max(scale[u]**2, 0.0) * _grad_bar(base_rows[u]))
  _close("scaled gradient", grad, c.want_grad, 9.0 * _grad_bar(base_rows))
  assert (vals[2] == 0).all() and (rows[2] == 0).all()  # the state of norm 0: exact zeros
  forward_vals = eng.expectation_from_states(dev_states, c.params)
  _close("scaled forward-only values", forward_vals, c.want_vals, _value_bar(c.ops, bar2))
  assert (forward_vals[2] == 0).all()
  out = eng.statevector_from_states(dev_states, c.params).cpu().numpy()
  want = R.final_states(n, c.gates, c.params, c.states.numpy().astype(np.complex128))
  _close("scaled states", out, want, AMPLITUDE_ATOL * np.maximum(scale, 1.0)[:, None])
  assert (out[2] == 0).all()
  assert torch.equal(torch.view_as_real(dev_states), torch.view_as_real(before))


@pytest.mark.parametrize("n,options", [(10, {}), (12, {"tile_qubits": 10, "adjoint_tile_qubits": 10})])
def test_one_observable_with_norms(n, options):
  """ONE observable: the engine's value mode -- values from lambda = O psi, the sweep on the unweighted lambda, the upstream
  put onto the gradient rows afterwards -- from states of norm 0.5, 3 and 1.  The upstream the rows are weighted with
  must carry ||phi||^2 exactly once."""
  rng = np.random.default_rng(650 + n)
  gates, names = O.hea_gates(n, 2, "one")
  params = rng.uniform(-1, 1, len(names))
  scale = np.array([0.5, 3.0, 1.0])
  states = _c64(R.random_states(3, n, 651 + n) * scale[:, None])
  upstream = rng.normal(size=(3, 1))
  for op in (O.xxz_chain_op(n), O.tfim_ring_op(n)):  # (terms that flip two qubits, and single flips measured in the tiles)
    want_vals, want_rows = R.values_and_rows(n, gates, params, states.numpy().astype(np.complex128), [op], upstream)
    eng = _engine(n, gates, len(names), [op], **options)
    vals, grad = eng.expectation_vjp_from_states(states, params, upstream)
    rows = eng.state_gradients(3)
    _close(f"n={n} one observable values", vals, want_vals, _value_bar([op], scale**2))
    for u in range(3):
      _close(f"n={n} one observable row {u}", rows[u], want_rows[u], scale[u]**2 * _grad_bar(want_rows[u] / scale[u]**2))
    _close(f"n={n} one observable gradient", grad, want_rows.sum(0), 9.0 * _grad_bar(want_rows / (scale**2)[:, None]))
    _close(f"n={n} one observable forward-only", eng.expectation_from_states(states, params), want_vals, _value_bar([op], scale**2))


def test_errors_of_the_c_entry_points():
  """The refusals the header names, driven through the C ABI itself (the binding checks shapes before it calls)."""
  import ctypes
  n = 6
  c = _case(("one", n), n, 2, 3, 100 + n)
  eng = c.engine()
  lib, h = eng._lib, eng._h  # pylint: disable=protected-access
  params = torch.zeros(c.n_params, dtype=torch.float32, device="cuda")
  states = c.states.cuda()
  out = torch.zeros((3, 2), dtype=torch.float32, device="cuda")
  grad = torch.zeros(c.n_params, dtype=torch.float32, device="cuda")
  up = torch.ones((3, 2), dtype=torch.float32, device="cuda")
  sv = torch.zeros((3, 1 << n), dtype=torch.complex64, device="cuda")

  def refused(rc, text):
    assert rc != 0
    assert text in lib.qhbm_last_error(h).decode(), lib.qhbm_last_error(h).decode()

  refused(lib.qhbm_expectation_from_states(h, None, 3, params.data_ptr(), out.data_ptr(), None), "d_states is NULL")
  refused(lib.qhbm_expectation_vjp_from_states(h, None, 3, params.data_ptr(), up.data_ptr(), out.data_ptr(), grad.data_ptr(), None),
          "d_states is NULL")
  refused(lib.qhbm_statevector_from_states(h, None, 3, params.data_ptr(), sv.data_ptr(), None), "d_states is NULL")
  refused(lib.qhbm_expectation_from_states(h, states.data_ptr(), -1, params.data_ptr(), out.data_ptr(), None), "negative batch size")
  refused(lib.qhbm_statevector_from_states(h, states.data_ptr(), -1, params.data_ptr(), sv.data_ptr(), None), "negative batch size")
  refused(lib.qhbm_expectation_from_states(h, states.data_ptr() + 8, 2, params.data_ptr(), out.data_ptr(), None), "16-byte aligned")
  bare = E.Engine(0)
  refused_bare = bare._lib.qhbm_statevector_from_states(bare._h, states.data_ptr(), 3, params.data_ptr(), sv.data_ptr(), None)  # pylint: disable=protected-access
  assert refused_bare != 0 and "qhbm_set_circuit has not been called" in bare._lib.qhbm_last_error(bare._h).decode()  # pylint: disable=protected-access
  assert lib.qhbm_expectation_from_states(h, None, 0, params.data_ptr(), None, None) == 0  # (no states: nothing to read)
  # the engine is as good as before every refusal
  vals, got = eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  c.check("after the refusals", vals, got)
  assert ctypes.sizeof(ctypes.c_void_p) == 8


# ---- 7. gradient mask ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stop_early", [0, 1])
def test_gradient_mask(stop_early):
  n = 12
  c = _case(("multi", n), n, 3, 5, 200 + n)
  _, names = O.hea_gates(n, 3, "fs")
  first_layer = np.array(["_fs_0_" in name for name in names])
  assert 0 < first_layer.sum() < len(names)
  eng = c.engine(tile_qubits=10, adjoint_tile_qubits=10, adjoint_stop_early=stop_early)
  eng.set_gradient_mask(~first_layer)
  vals, grad = eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  grad = grad.cpu().numpy()
  assert (grad[first_layer] == 0).all()
  _close(f"stop_early={stop_early} values", vals, c.want_vals, _value_bar(c.ops))
  _close(f"stop_early={stop_early} live gradient", grad[~first_layer], c.want_grad[~first_layer], _grad_bar(c.want_grad))
  eng.set_gradient_mask(None)
  vals, grad = eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  c.check(f"stop_early={stop_early} mask lifted", vals, grad)


# ---- 8. lifecycle ----------------------------------------------------------------------------------------------------------------
def test_lifecycle():
  n = 12
  c = _case(("multi", n), n, 3, 5, 200 + n)
  eng = c.engine(tile_qubits=10, adjoint_tile_qubits=10)
  bits = np.random.default_rng(3).integers(0, 2, size=(5, n)).astype(np.int8)
  eng.expectation(bits, c.params, retain=True)
  assert eng.retained_states() == 5
  eng.expectation_from_states(c.states, c.params)
  assert eng.retained_states() == 0
  with pytest.raises(E.EngineError, match="no retained forward state"):
    eng.expectation_vjp_retained(bits, c.params, c.upstream)
  with pytest.raises(ValueError):
    eng.expectation_from_states(c.states[:, :-1], c.params)
  with pytest.raises(ValueError):
    eng.expectation_from_states(torch.zeros((2, 1 << n), dtype=torch.float32), c.params)
  with pytest.raises(E.EngineError, match="has not been called"):
    _engine(n, c.gates, c.n_params, None).expectation_from_states(c.states, c.params)
  # rows follow the last VJP, whichever kind it was
  eng.expectation_vjp_from_states(c.states, c.params, c.upstream)
  _, bits_grad = eng.expectation_vjp(bits, c.params, c.upstream)
  _close("rows of the bits VJP", eng.state_gradients(5).double().sum(0), bits_grad.double().cpu().numpy(),
         64 * 2.0**-24 * max(1.0, float(bits_grad.abs().max()) * 5))
  # another circuit on another number of qubits
  small = _case(("one", 6), 6, 2, 3, 106)
  eng.set_circuit(small.n, small.gates, small.n_params)
  eng.set_observables(small.ops)
  with pytest.raises(E.EngineError, match="last call was not an adjoint VJP"):
    eng.state_gradients(5)
  vals, grad = eng.expectation_vjp_from_states(small.states, small.params, small.upstream)
  small.check("after set_circuit", vals, grad)
  with pytest.raises(ValueError):
    eng.expectation_from_states(c.states, small.params)
  empty_vals, empty_grad = eng.expectation_vjp_from_states(small.states[:0], small.params, small.upstream[:0])
  assert empty_vals.shape == (0, 2) and (empty_grad == 0).all()


# ---- 9. mirror ---------------------------------------------------------------------------------------------------------------------
def _set(param, values):
  with torch.no_grad():
    param.copy_(torch.as_tensor(np.asarray(values), dtype=torch.float32))


def test_mirror_matches_the_bits_path_and_its_gradients():
  """U = U1 U2 on 5 qubits and a Hamiltonian (KOBE-2, HEA): sum_x p(x) <x| U^dagger K U |x> through `expectation` on the
  32 bitstrings, and through `expectation_from_states` of an inference over U2 given the 32 states U1|x>.  Gradients
  with respect to U2's variables, the Hamiltonian's circuit and its energy agree to 2e-4, the bar tests/test_host_gpu.py
  holds Jacobians of a Hamiltonian's expectation to."""
  n = 5
  qubits = ir.GridQubit.rect(1, n)
  rng = np.random.default_rng(90)
  u1 = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "u1"))
  u2 = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "u2"))
  hc = models.DirectQuantumCircuit(hea_circuit(qubits, 2, "hc"))
  for circ in (u1, u2, hc):
    _set(circ.trainable_variables[0], rng.uniform(-1, 1, circ.trainable_variables[0].shape))
  energy = models.KOBE(list(range(n)), 2)
  energy.build([None, n])
  _set(energy.post_process[0].kernel, rng.uniform(-0.5, 0.5, energy.post_process[0].kernel.shape))
  ham = models.Hamiltonian(energy, hc)
  ebm = models.KOBE(list(range(n)), 2)
  ebm.build([None, n])
  _set(ebm.post_process[0].kernel, rng.uniform(-0.5, 0.5, ebm.post_process[0].kernel.shape))
  all_bits = torch.tensor(list(itertools.product([0, 1], repeat=n)), dtype=torch.int8)
  with torch.no_grad():
    probs = torch.softmax(-ebm(all_bits).double().reshape(-1), 0)  # the exact EBM probabilities
  variables = [u2.trainable_variables[0], hc.trainable_variables[0], energy.post_process[0].kernel]

  whole = inference.AnalyticQuantumInference(u1 + u2)
  want = (probs.to("cuda") * whole.expectation(all_bits, ham).double().reshape(-1)).sum()
  want_grads = torch.autograd.grad(want, variables)

  states = inference.unitary(u1).transpose(0, 1).contiguous()  # row x = U1 |x>
  part = inference.AnalyticQuantumInference(u2)
  values = part.expectation_from_states(states, ham)
  assert values.shape == (32, 1)
  got = (probs.to(values.device) * values.double().reshape(-1)).sum()
  got_grads = torch.autograd.grad(got, variables)
  _close("mirror value", got, float(want.detach()), 2e-5 * max(1.0, float(energy.post_process[0].kernel.detach().abs().sum())))
  for name, a, b in zip(("U2", "Hamiltonian circuit", "Hamiltonian energy"), got_grads, want_grads):
    _close("mirror gradient " + name, a, b.cpu().numpy(), 2e-4)
  assert u1.trainable_variables[0].grad is None
  # complex128 is cast; states that require grad and sharded inferences are refused
  values128 = part.expectation_from_states(states.to(torch.complex128), ham)
  assert torch.equal(values128, values)
  with pytest.raises(ValueError, match="not differentiable"):
    part.expectation_from_states(states.clone().requires_grad_(True), ham)
  general = models.BitstringEnergy(list(range(n)), [torch.nn.Linear(n, 1)])
  with pytest.raises(TypeError, match="General Hamiltonians not accepted"):
    part.expectation_from_states(states, models.Hamiltonian(general, hc))


# ---- 10. QMHL from a density matrix --------------------------------------------------------------------------------------------------
def _dense_op(n, op):
  eye = np.eye(1 << n, dtype=np.complex128)
  return np.stack([O.apply_op(eye[j].reshape((2,) * n), op).reshape(-1) for j in range(1 << n)], axis=1)


def test_qmhl_from_a_density_matrix():
  """sigma = the thermal state of the TFIM ring at beta = 1 on 4 qubits, in float64; the model a KOBE-2 energy under an
  HEA.  Loss = Tr(sigma U diag(E_theta) U^dagger) + log Z from `O.unitary` in complex128 to 2e-5, gradients against
  central differences (step 1e-5, float64) of that dense expression to 2e-4."""
  n, layers = 4, 2
  h = _dense_op(n, O.tfim_ring_op(n))
  w, v = np.linalg.eigh(h)
  p = np.exp(-(w - w.min()))
  sigma = (v * (p / p.sum())) @ v.conj().T
  rng = np.random.default_rng(11)
  gates, names = O.hea_gates(n, layers, "qm")
  phi = rng.uniform(-1, 1, len(names))
  all_bits = O.all_bitstrings(n)
  energy = models.KOBE(list(range(n)), 2)
  energy.build([None, n])
  thetas = rng.uniform(-0.5, 0.5, tuple(energy.post_process[0].kernel.shape))
  _set(energy.post_process[0].kernel, thetas)
  circ = models.DirectQuantumCircuit(hea_circuit(ir.GridQubit.rect(1, n), layers, "qm"))
  assert circ.symbol_names == names
  _set(circ.trainable_variables[0], phi)
  thetas = energy.post_process[0].kernel.detach().double().numpy().copy()  # (the float32 values the model holds)
  phi = circ.trainable_variables[0].detach().double().numpy().copy()

  def dense_loss(th, ph):
    u = O.unitary(n, gates, ph)
    e = O.kobe_energy(all_bits, th.reshape(-1), 2)
    k = (u * e) @ u.conj().T
    return float(np.real(np.trace(sigma @ k))) + float(np.log(np.sum(np.exp(-e))))

  def central(f, x):
    g = np.zeros(x.size)
    for i in range(x.size):
      hi, lo = x.reshape(-1).copy(), x.reshape(-1).copy()
      hi[i] += 1e-5
      lo[i] -= 1e-5
      g[i] = (f(hi.reshape(x.shape)) - f(lo.reshape(x.shape))) / 2e-5
    return g

  model = inference.QHBM(inference.AnalyticEnergyInference(energy, 16, initial_seed=1), inference.AnalyticQuantumInference(circ))
  source = data.StateVectorData.from_density_matrix(torch.from_numpy(sigma))
  loss = inference.qmhl(source, model)
  loss.backward()
  _close("qmhl loss", loss, dense_loss(thetas, phi), 2e-5)
  _close("qmhl d/d theta", energy.post_process[0].kernel.grad.reshape(-1), central(lambda t: dense_loss(t, phi), thetas), 2e-4)
  _close("qmhl d/d phi", circ.trainable_variables[0].grad, central(lambda x: dense_loss(thetas, x), phi), 2e-4)
  again = inference.qmhl(source, model)  # the data's inference and its engine are created once
  assert float(again.detach()) == float(loss.detach()) and len(source._inference._engines) == 1  # pylint: disable=protected-access
