"""Every engine entry point on circuits with spectator qubits, on a dirty workspace.

A spectator (tests/spectator_cases.py) is an idle qubit, a diagonal-only qubit, or a qubit whose only non-diagonal
gate is in the last layer.  With an idle or diagonal-only qubit the forward plan's first pass zero-fills every tile and
later passes rely on those zeros; with every bit acted on, the first pass writes one tile per state and later passes
prune tiles (zero_mask) and clear what they load (frozen_old_local).  Either way a call must never read memory it did
not write.  So every call under test runs on an engine that has just run, with the same options, the same entry point
and an adjoint VJP (which fills lambda) on bitstrings that differ from the tested ones on every spectator column and on
other parameters: stale amplitudes then sit exactly where the tested states must be zero, and any read of them carries
O(1) of wrong norm.  Each output must equal the same call on a fresh engine bit for bit, and match the complex128
oracle (the C oracle at 20 qubits), a closed form, or an exact invariant.

Tolerances follow tests/test_engine_gpu.py: values 2e-5 * sum|c_k| (5e-5 from 18 qubits), gradients and Jacobians
1e-4 * max(1, |grad|_inf) (shift rule 3e-4), states 5e-6.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from tests import spectator_cases as S
from tests.test_engine_gpu import _engine

pytestmark = pytest.mark.gpu

SIZES = (11, 13, 14)
FAMILIES = tuple(S.FAMILIES)
OPSETS = ("ham", "wide", "shards")
MULTI = {"tile_qubits": 10, "adjoint_tile_qubits": 10}
B = 3


def _single(n):
  """The control: one forward pass (the backward sweep is capped at tiles of 13 qubits)."""
  return {"tile_qubits": n, "adjoint_tile_qubits": min(n, 13)}


class _Case:
  """One circuit of a family at n qubits, its parameters, bitstrings (every spectator column holds both values) and
  the spectator-flipped bitstrings and other parameters the priming calls use."""

  def __init__(self, n, family):
    seed = 1000 * n + FAMILIES.index(family)
    self.n, self.family = n, family
    self.gates, self.n_params, self.roles, self.layer_of_param = S.spectator_circuit(n, family, seed)
    rng = np.random.default_rng(seed)
    self.params = rng.uniform(-1, 1, self.n_params).astype(np.float32)
    self.other = rng.uniform(-1, 1, self.n_params).astype(np.float32)
    self.bits = rng.integers(0, 2, size=(B, n)).astype(np.int8)
    for i, q in enumerate(sorted(self.roles)):
      self.bits[:, q] = (np.arange(B) + i) % 2
    self.flip = S.flipped(self.bits, self.roles)
    self.ops = S.op_sets(n, self.roles, seed)
    self._up = {k: rng.normal(size=(B, len(v))).astype(np.float32) for k, v in self.ops.items()}
    self._up_other = {k: rng.normal(size=(B, len(v))).astype(np.float32) for k, v in self.ops.items()}
    self.live = [g for g, gate in enumerate(self.gates) if gate[3] >= 0]
    self._oracle = {}

  def up(self, opset):
    return self._up[opset]

  def up_other(self, opset):
    return self._up_other[opset]

  def oracle(self, opset, gates=None):
    """(values [B, T], Jacobian [B, T, P], final states [B, 2^n]) in complex128."""
    key = (opset, None if gates is None else tuple(gates))
    if key not in self._oracle:
      self._oracle[key] = S.stacked_jacobian(self.n, gates or self.gates, self.params.astype(np.float64), self.bits,
                                             self.ops[opset])
    return self._oracle[key]


@functools.lru_cache(maxsize=None)
def _case(n, family):
  return _Case(n, family)


def _outputs(out):
  return tuple(t.clone() for t in (out if isinstance(out, tuple) else (out,)))


def _primed_and_fresh(c, opset, call, options=None, mask=None):
  """`call(eng, bits, params)` on a primed engine and on a fresh one; asserts they agree bit for bit and returns the
  primed outputs as numpy arrays.  Priming: an adjoint VJP, then `call` itself, both on the spectator-flipped
  bitstrings and the other parameters."""
  options = MULTI if options is None else options
  outs = []
  for primed in (True, False):
    eng = _engine(c.n, c.gates, c.n_params, c.ops[opset], **options)
    if mask is not None:
      eng.set_gradient_mask(mask)
    fwd_passes = eng.num_passes()[0]
    assert (fwd_passes > 1) if options.get("tile_qubits", 0) < c.n else fwd_passes == 1, (options, fwd_passes)
    if primed:
      eng.expectation_vjp(c.flip, c.other, c.up_other(opset))
      call(eng, c.flip, c.other)
    outs.append(_outputs(call(eng, c.bits, c.params)))
    del eng
  for i, (a, b) in enumerate(zip(*outs)):
    assert torch.equal(a, b), (f"output {i} depends on workspace history: max |primed - fresh| = "
                               f"{float((a - b).abs().max())}")
  return [t.cpu().numpy() for t in outs[0]]


def _up(c, opset, params):
  """The upstream of the call under test, or of the priming call (other parameters)."""
  return c.up(opset) if params is c.params else c.up_other(opset)


def _value_tol(ops, rel=2e-5):
  return rel * np.maximum(S.op_norm(ops), 1.0)[None, :]


def _assert_values(got, want, ops, what, rel=2e-5):
  err = np.abs(got - want)
  tol = _value_tol(ops, rel)
  assert (err <= tol).all(), f"{what}: max err {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"


def _assert_grad(got, want, what, rel=1e-4):
  np.testing.assert_allclose(got, want, atol=rel * max(1.0, float(np.abs(want).max())), rtol=0, err_msg=what)


# ---- values, the retained pair, the adjoint VJP, its rows and the Jacobian ------------------------------------------
@pytest.mark.parametrize("opset", OPSETS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_forward_and_adjoint_entry_points(n, family, opset):
  c = _case(n, family)
  ops = c.ops[opset]
  up = c.up(opset)
  want_v, want_j, _ = c.oracle(opset)
  want_rows = np.einsum("bt,btp->bp", up, want_j)
  want_g = want_rows.sum(0)
  first = {}
  for options in (MULTI, _single(n)):
    tag = f"{family} n={n} {opset} tile={options['tile_qubits']}"
    (v,) = _primed_and_fresh(c, opset, lambda e, b, p: e.expectation(b, p), options)
    _assert_values(v, want_v, ops, f"expectation, {tag}")
    first.setdefault("values", v)

    def retained(e, b, p):
      vals = e.expectation(b, p, retain=True)
      assert e.retained is not None
      return vals, e.expectation_vjp_retained(b, p, _up(c, opset, p))
    v, g = _primed_and_fresh(c, opset, retained, options)
    _assert_values(v, want_v, ops, f"retained values, {tag}")
    _assert_grad(g, want_g, f"retained VJP, {tag}")

    def adjoint(e, b, p):
      vals, grad = e.expectation_vjp(b, p, _up(c, opset, p))
      return vals, grad, e.state_gradients(B)
    v, g, rows = _primed_and_fresh(c, opset, adjoint, options)
    _assert_values(v, want_v, ops, f"adjoint values, {tag}")
    _assert_grad(g, want_g, f"adjoint VJP, {tag}")
    _assert_grad(rows, want_rows, f"state_gradients rows, {tag}")

    v, jac = _primed_and_fresh(c, opset, lambda e, b, p: e.expectation_jacobian(b, p), options)
    _assert_values(v, want_v, ops, f"Jacobian values, {tag}")
    _assert_grad(jac, want_j, f"Jacobian, {tag}")
    first.setdefault("jac", jac)

  # a gradient mask that freezes the first layer: the backward sweep stops at the first live gate, or runs to the
  # basis state and prunes its tail
  mask = c.layer_of_param != 0
  assert mask.any() and not mask.all()
  for stop_early in (1, 0):
    opts = dict(MULTI, adjoint_stop_early=stop_early)
    _, g = _primed_and_fresh(c, opset, lambda e, b, p: e.expectation_vjp(b, p, _up(c, opset, p)), opts, mask=mask)
    assert (g[~mask] == 0).all()
    _assert_grad(g[mask], want_g[mask], f"masked adjoint VJP, stop_early={stop_early}, {family} n={n} {opset}")

  if opset == "shards":  # closed forms for a qubit that keeps its input bit: <Z> = (-1)^b, <X> = <Y> = 0, no gradient
    v, jac = first["values"], first["jac"]
    for q in S.idle_or_diag(c.roles):
      z, x, y = (S.shard_index(n, c.roles, q, p) for p in "ZXY")
      np.testing.assert_allclose(v[:, z], 1.0 - 2.0 * c.bits[:, q], atol=2e-5, err_msg=f"<Z_{q}>")
      np.testing.assert_allclose(v[:, [x, y]], 0.0, atol=2e-5, err_msg=f"<X_{q}>, <Y_{q}>")
      np.testing.assert_allclose(jac[:, [z, x, y], :], 0.0, atol=1e-4, err_msg=f"d<P_{q}>/dparams")


# ---- the parameter-shift VJP: prefix sharing on and off, every launch-set geometry -----------------------------------
@pytest.mark.parametrize("opset", OPSETS)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_parameter_shift_vjp(n, family, opset):
  c = _case(n, family)
  ops = c.ops[opset]
  want_v, want_j, _ = c.oracle(opset)
  want_g = np.einsum("bt,btp->p", c.up(opset), want_j)

  def shift(e, b, p):
    return e.expectation_vjp(b, p, _up(c, opset, p), method=E.GRAD_PARAMETER_SHIFT)
  results = {}
  for chunk in (0, 1, 2, 5):
    for sharing in (0, 1):
      results[chunk, sharing] = _primed_and_fresh(c, opset, shift, dict(MULTI, chunk_states=chunk,
                                                                      shift_prefix_sharing=sharing))
  for key, (v, g) in results.items():
    tag = f"{family} n={n} {opset} chunk={key[0]} sharing={key[1]}"
    assert np.array_equal(v, results[0, 0][0]) and np.array_equal(g, results[0, 0][1]), f"{tag}: not bit for bit"
    _assert_values(v, want_v, ops, f"shift-rule values, {tag}")
    _assert_grad(g, want_g, f"shift-rule VJP, {tag}", rel=3e-4)


# ---- program VJPs (one adjoint VJP per shifted program) ---------------------------------------------------------------
def _shifted(gates, g, s):
  if g < 0:
    return list(gates)
  out = list(gates)
  out[g] = out[g][:5] + (out[g][5] + s,) + tuple(out[g][6:])
  return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_program_vjps(n, family):
  c = _case(n, family)
  picks = [c.live[i] for i in np.linspace(0, len(c.live) - 1, 5).astype(int)]
  sg = [g for g in picks for _ in (0, 1)] + [-1]
  sv = [0.5, -0.5] * len(picks) + [0.0]
  for opset in OPSETS:
    ops = c.ops[opset]

    def programs(e, b, p, opset=opset):
      return e.program_vjps(b, p, sg, sv, _up(c, opset, p))
    results = {}
    for chunk in (0, 1, 2, 5):
      for sharing in (0, 1):
        results[chunk, sharing] = _primed_and_fresh(c, opset, programs, dict(MULTI, chunk_states=chunk,
                                                                           shift_prefix_sharing=sharing))
    for key, (v, g) in results.items():
      assert np.array_equal(v, results[0, 0][0]) and np.array_equal(g, results[0, 0][1]), (family, n, opset, key)
    vals, grad = results[0, 1]
    checked = [len(sg) - 1] + ([0, len(sg) - 2] if opset == "ham" else [])   # the unshifted program; two shifted
    for q in checked:
      want_v, want_j, _ = c.oracle(opset, _shifted(c.gates, sg[q], sv[q]) if sg[q] >= 0 else None)
      want = np.einsum("bt,btp->p", c.up(opset), want_j)
      _assert_grad(grad[q], want, f"program {q} ({sg[q]}, {sv[q]}), {family} n={n} {opset}")
      np.testing.assert_allclose(vals[q], want_v.sum(0), atol=B * _value_tol(ops).max(), rtol=0,
                                 err_msg=f"program {q} values, {family} n={n} {opset}")


# ---- statevectors and samples: exact zeros, exact spectator bits ------------------------------------------------------
def _spectator_bit(index, n, q):
  return (index >> (n - 1 - q)) & 1


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("n", SIZES)
def test_statevector_and_samples(n, family):
  c = _case(n, family)
  keep = S.idle_or_diag(c.roles)
  _, _, want_states = c.oracle("ham")
  index = np.arange(1 << n)
  for options in (MULTI, _single(n)):
    (sv,) = _primed_and_fresh(c, "ham", lambda e, b, p: e.statevector(b, p), options)
    np.testing.assert_allclose(sv, want_states, atol=5e-6, rtol=0, err_msg=f"{family} n={n}")
    for q in keep:
      off = _spectator_bit(index[None, :], n, q) != c.bits[:, q:q + 1]
      assert (sv[off] == 0).all(), f"qubit {q}: amplitudes away from the input bit are not exactly 0"

  shots = 512
  g_mid = c.live[len(c.live) // 2]
  for shift_gate, shift in ((-1, 0.0), (g_mid, 0.5)):
    (smp,) = _primed_and_fresh(c, "ham", lambda e, b, p: e.sample(b, p, shots, seed=7, shift_gate=shift_gate,
                                                                  shift=shift))
    assert smp.shape == (B, shots, n)
    for q in keep:
      assert (smp[:, :, q] == c.bits[:, None, q]).all(), f"qubit {q}: a shot lost its input bit"
  sg, sv_ = (-1, c.live[0], g_mid, c.live[-1]), (0.0, 0.5, -0.5, 0.5)
  for options in (MULTI, dict(MULTI, chunk_states=2)):
    (counts,) = _primed_and_fresh(c, "ham", lambda e, b, p: e.sample_counts(b, p, shots, seed=9, shift_gates=sg,
                                                                             shifts=sv_), options)
    assert counts.shape == (len(sg), B, 1 << n)
    assert (counts.sum(-1) == shots).all()
    for q in keep:
      off = _spectator_bit(index[None, :], n, q) != c.bits[:, q:q + 1]
      assert (counts[:, off] == 0).all(), f"qubit {q}: counts away from the input bit"


# ---- a default plan at 20 qubits against the C oracle -----------------------------------------------------------------
def test_default_plan_at_twenty_qubits_against_the_c_oracle():
  from oracle import qhbm_cpu as C
  n = 20
  gates, n_params, roles, _ = S.spectator_circuit(n, "idle_diag", 2020, layers=1, extra=8)
  rng = np.random.default_rng(2020)
  params = rng.uniform(-1, 1, n_params).astype(np.float32)
  other = rng.uniform(-1, 1, n_params).astype(np.float32)
  bits = rng.integers(0, 2, size=(2, n)).astype(np.int8)
  for i, q in enumerate(sorted(roles)):
    bits[:, q] = [i % 2, 1 - i % 2]
  flip = S.flipped(bits, roles)
  sets = S.op_sets(n, roles, 20)
  for opset in ("ham", "wide"):
    ops = sets[opset]
    up = rng.normal(size=(2, len(ops))).astype(np.float32)
    want_v, want_g = C.expectation_vjp(n, gates, params, bits, ops, up)
    gtol = 2e-4 * max(1.0, float(np.abs(want_g).max()))
    results = {}
    for sharing in (0, 1):
      eng = _engine(n, gates, n_params, ops, shift_prefix_sharing=sharing)
      assert eng.num_passes()[0] > 1
      eng.expectation_vjp(flip, other, up)
      eng.expectation_vjp(flip, other, up, method=E.GRAD_PARAMETER_SHIFT)
      v, g = eng.expectation_vjp(bits, params, up, method=E.GRAD_PARAMETER_SHIFT)
      results[sharing] = (v.clone(), g.clone())
      np.testing.assert_allclose(g.cpu().numpy(), want_g, atol=1.5 * gtol, rtol=0, err_msg=f"shift rule, {opset}")
      eng.expectation(flip, other)
      v = eng.expectation(bits, params).cpu().numpy()
      _assert_values(v, want_v, ops, f"values at 20 qubits, {opset}", rel=5e-5)
      v, g = eng.expectation_vjp(bits, params, up)
      np.testing.assert_allclose(g.cpu().numpy(), want_g, atol=gtol, rtol=0, err_msg=f"adjoint, {opset}")
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), opset
  eng.statevector(flip, other)
  sv = eng.statevector(bits, params).cpu().numpy()
  want = C.statevector(n, gates, params, bits)
  np.testing.assert_allclose(sv, want, atol=5e-6, rtol=0)
  index = np.arange(1 << n)
  for q in S.idle_or_diag(roles):
    assert (sv[_spectator_bit(index[None, :], n, q) != bits[:, q:q + 1]] == 0).all(), q


# ---- prefix sharing stays on where it is sound ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hea", "idle_diag"])
def test_prefix_sharing_is_used_only_where_the_first_pass_writes_one_tile(kind):
  """Prefix sharing stays on for an HEA plan (every bit acted on: PASS_NO_ZERO_FILL), and is off on a plan whose first
  pass zero-fills -- there a program starting behind it would read tiles it never wrote.  With sharing the programs run
  in launch sets grouped by the pass they start at, each skipping the passes in front of it, plus the base program's
  own passes: the forward launches differ from the unshared run's.  Without it the launches are the same."""
  n = 13
  if kind == "hea":
    gates, names = O.hea_gates(n, 2, "h")
    n_params = len(names)
  else:
    gates, n_params, _, _ = S.spectator_circuit(n, kind, 13)
  rng = np.random.default_rng(5)
  params = rng.uniform(-1, 1, n_params).astype(np.float32)
  bits = rng.integers(0, 2, size=(2, n)).astype(np.int8)
  ops = [O.random_pauli_op(n, 40, 13, p_identity=0.6)]   # config 4's kind: values from the observable kernel
  up = rng.normal(size=(2, 1)).astype(np.float32)
  launches, grads = {}, {}
  for sharing in (0, 1):
    eng = _engine(n, gates, n_params, ops, profile_events=1, shift_prefix_sharing=sharing, **MULTI)
    assert eng.num_passes()[0] > 1
    zero_fill = "[zero-fill]" in eng.describe_schedule()
    assert zero_fill == (kind != "hea")
    eng.kernel_time_ms(reset=True)
    _, g = eng.expectation_vjp(bits, params, up, method=E.GRAD_PARAMETER_SHIFT)
    launches[sharing] = eng.kernel_time_ms(reset=True)["fwd_launches"]
    grads[sharing] = g.clone()
  assert torch.equal(grads[0], grads[1])
  if kind == "hea":
    assert launches[1] != launches[0], launches
  else:
    assert launches[1] == launches[0], launches
