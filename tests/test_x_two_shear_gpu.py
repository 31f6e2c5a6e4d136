"""X**t as two shears with its scaling folded into the FULL diagonal table (csrc/x_shear.h, engine option
`x_two_shear`) against oracle/qhbm_oracle.py: values and the full Jacobian.

The form is chosen per gate and per call from the reduced exponent (|t| <= 2/3, theta <= pi / 3), so the X exponents
are PINNED: the boundary 2/3 as a float and its float neighbours either side, both signs, 0, +-1 (theta = +-pi / 2),
exponents far outside one period, and ordinary values either side of the boundary, dealt to neighbouring qubits so that
the X gates of one instance straddle the boundary (one flagged, one not: the inner product of the flagged gate's
neighbour must not see its pending scaling).  Cases: n = 5, depth 2 (one tile; X + Z + CZ of a layer in one instance)
and n = 13, depth 3 on tiles of 2^10 (several passes, the relabeling store, tile bits in the boundary predicates),
three bitstrings.  Tolerances are those of tests/test_engine_gpu.py for the same quantities."""
import functools

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E

pytestmark = pytest.mark.gpu

B = np.float32(2.0 / 3.0)
PINNED = [0.5, 0.8, float(np.nextafter(B, np.float32(0))), float(np.nextafter(B, np.float32(1))), -1.0, 0.0, 10000.25, -0.66,
          1.0, float(B), -float(B), -float(np.nextafter(B, np.float32(1))), -float(np.nextafter(B, np.float32(0))), 0.3, -20001.75,
          0.95, -0.1, 0.7, 0.6, -0.9]
CASES = {"n5": dict(n=5, layers=2, options={}),
         "n13": dict(n=13, layers=3, options=dict(tile_qubits=10, adjoint_tile_qubits=10))}


def _op_norm(ops):
  return np.array([sum(abs(c) for c, _, _ in op) for op in ops])


def _engine(n, gates, n_params, ops, **options):
  eng = E.Engine(0)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(n, gates, n_params)
  eng.set_observables(ops)
  return eng


@functools.lru_cache(maxsize=None)
def _case(name, variant="base"):
  """Circuit, float32 parameters with the X exponents pinned, bitstrings, observables and the oracle's values and
  Jacobian -- computed once per (case, variant) and shared, never modified."""
  c = CASES[name]
  n, layers = c["n"], c["layers"]
  rng = np.random.default_rng(1000 * n + layers)
  gates, names = O.hea_gates(n, layers, "x2")
  P = len(names)
  params = rng.uniform(-1, 1, P).astype(np.float32)
  xs = [g for g in gates if g[0] == O.GATE_XPOW]
  for i, g in enumerate(xs):
    params[g[3]] = np.float32(PINNED[i % len(PINNED)])
  if variant == "tied":  # every parameter drives two or three gates; the X exponents stay pinned through the offsets
    T = P // 2 - 1
    tied = rng.uniform(-1, 1, T).astype(np.float32)
    gates = [(k, a, b, p % T, 1.0, float(np.float32(params[p]) - tied[p % T])) for (k, a, b, p, s, o) in gates]
    params, P = tied, T
  if variant == "inverse":  # U(params) then the inverse circuit with parameters of its own: diagonal, then X, per qubit
    inv = [(k, a, b, p + P, -s, -o) for (k, a, b, p, s, o) in reversed(gates)]
    gates = gates + inv
    second = rng.uniform(-1, 1, P).astype(np.float32)
    for i, g in enumerate(xs):
      second[g[3]] = np.float32(PINNED[(i + 7) % len(PINNED)])
    params, P = np.concatenate([params, second]), 2 * P
  ops = [O.xxz_chain_op(n), O.tfim_ring_op(n)]
  bits = rng.integers(0, 2, size=(3, n)).astype(np.int8)
  vals, jac = O.expectation_jacobian(n, gates, params.astype(np.float64), bits, ops)
  vals.setflags(write=False)
  jac.setflags(write=False)
  return dict(n=n, gates=gates, P=P, params=params, ops=ops, bits=bits, vals=vals, jac=jac, options=c["options"])


def _check(c, eng, label):
  vals, jac = eng.expectation_jacobian(c["bits"], c["params"])
  scale = max(1.0, np.abs(c["jac"]).max())
  ev = np.abs(vals.cpu().numpy() - c["vals"]).max()
  ej = np.abs(jac.cpu().numpy() - c["jac"]).max()
  print(f"{label}: max |dval| = {ev:.3g}, max |djac| = {ej:.3g} (scale {scale:.3g})")
  np.testing.assert_allclose(vals.cpu().numpy(), c["vals"], atol=2e-5 * _op_norm(c["ops"]).max(), rtol=0, err_msg=label)
  np.testing.assert_allclose(jac.cpu().numpy(), c["jac"], atol=1e-4 * scale, rtol=0, err_msg=label)
  return vals, jac


@pytest.mark.parametrize("name", sorted(CASES))
def test_option_on_and_off_match_the_oracle_and_the_flop_model_counts_what_ran(name):
  c = _case(name)
  flops = {}
  for on in (1, 0):
    eng = _engine(c["n"], c["gates"], c["P"], c["ops"], x_two_shear=on, **c["options"])
    _check(c, eng, f"{name} x_two_shear={on}")
    flops[on] = eng.flop_model(3, True)
  # the pinned set has gates either side of the boundary in FULL instances: fewer flops ran with the option on, in both
  # sweeps, and the model (read back from the records of the call above) says so
  assert flops[1]["fwd_flops"] < flops[0]["fwd_flops"] and flops[1]["bwd_flops"] < flops[0]["bwd_flops"], flops
  # ... and the planning-only count (no call yet) is the three-shear one, whatever the option
  fresh = _engine(c["n"], c["gates"], c["P"], c["ops"], **c["options"]).flop_model(3, True)
  assert fresh["bwd_flops"] == flops[0]["bwd_flops"] and fresh["fwd_flops"] == flops[0]["fwd_flops"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_frozen_x_gates_have_no_slot_and_the_rest_is_unchanged(name):
  c = _case(name)
  rng = np.random.default_rng(7)
  mask = np.ones(c["P"], bool)
  x_params = [g[3] for g in c["gates"] if g[0] == O.GATE_XPOW]
  mask[x_params[1::2]] = False          # every other X gate loses its gradient slot, first layer included
  mask[x_params[0]] = True              # (so that the sweep still runs to the first gate)
  up = rng.normal(size=(3, 2)).astype(np.float32)
  want = np.einsum("bt,btp->p", up, c["jac"])
  tol = 1e-4 * max(1.0, np.abs(want).max())
  for on in (1, 0):
    eng = _engine(c["n"], c["gates"], c["P"], c["ops"], x_two_shear=on, **c["options"])
    eng.set_gradient_mask(mask)
    vals, grad = eng.expectation_vjp(c["bits"], c["params"], up)
    got = grad.cpu().numpy()
    np.testing.assert_allclose(vals.cpu().numpy(), c["vals"], atol=2e-5 * _op_norm(c["ops"]).max(), rtol=0)
    assert (got[~mask] == 0).all()
    np.testing.assert_allclose(got[mask], want[mask], atol=tol, rtol=0)


@pytest.mark.parametrize("variant", ["tied", "inverse"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_tied_parameters_and_an_appended_inverse_circuit(name, variant):
  """Tied: a parameter's gradient is the sum over gates of either form.  Inverse: the appended half lists a layer as
  diagonal-then-X per qubit; the scheduler puts such an X into the NEXT instance, in front of that instance's table
  (schedule.cpp emit_round), so the folding is as valid there as in the ansatz -- and an X in an instance without a
  FULL table keeps three shears."""
  c = _case(name, variant)
  for on in (1, 0):
    eng = _engine(c["n"], c["gates"], c["P"], c["ops"], x_two_shear=on, **c["options"])
    _check(c, eng, f"{name} {variant} x_two_shear={on}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_parameter_shift_vjp_equals_the_adjoint_vjp(name):
  """The shifted programs have coefficient buffers -- and two-shear flags -- of their own: a shift of +-1/2 moves a
  gate across the boundary in one program and not in the other."""
  c = _case(name)
  rng = np.random.default_rng(11)
  up = rng.normal(size=(3, 2)).astype(np.float32)
  want = np.einsum("bt,btp->p", up, c["jac"])
  tol = 1e-4 * max(1.0, np.abs(want).max())
  eng = _engine(c["n"], c["gates"], c["P"], c["ops"], **c["options"])
  vals, grad = eng.expectation_vjp(c["bits"], c["params"], up)
  svals, sgrad = eng.expectation_vjp(c["bits"], c["params"], up, E.GRAD_PARAMETER_SHIFT)
  np.testing.assert_allclose(grad.cpu().numpy(), want, atol=tol, rtol=0)
  np.testing.assert_allclose(sgrad.cpu().numpy(), want, atol=3 * tol, rtol=0)
  np.testing.assert_allclose(svals.cpu().numpy(), c["vals"], atol=1e-4, rtol=0)
  # and the engine's own buffers are intact afterwards
  v2, g2 = eng.expectation_vjp(c["bits"], c["params"], up)
  assert torch.equal(vals, v2) and torch.equal(grad, g2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bit_reproducible_with_the_option_on(name):
  """As tests/test_engine_gpu.py states it: two runs, a chunked batch and a single-row call give identical bits per
  state."""
  c = _case(name)
  eng = _engine(c["n"], c["gates"], c["P"], c["ops"], x_two_shear=1, **c["options"])
  v1, j1 = eng.expectation_jacobian(c["bits"], c["params"])
  v2, j2 = eng.expectation_jacobian(c["bits"], c["params"])
  assert torch.equal(v1, v2) and torch.equal(j1, j2)
  eng.set_option("chunk_states", 2)
  v3, j3 = eng.expectation_jacobian(c["bits"], c["params"])
  assert torch.equal(v1, v3) and torch.equal(j1, j3)
  eng.set_option("chunk_states", 0)
  v4, j4 = eng.expectation_jacobian(c["bits"][1:2], c["params"])
  assert torch.equal(v1[1:2], v4) and torch.equal(j1[1:2], j4)
  assert torch.equal(eng.expectation(c["bits"][2:3], c["params"]), v1[2:3])


def test_two_x_gates_of_one_instance_straddle_the_boundary():
  """The case the order 'first every shear, then every inner product' guards, built on purpose and ASSERTED to be what
  runs: one layer on four qubits is one instance (X, Z on every qubit and the three CZ: a FULL table) on the four register
  bits of one round.  The flop model, read back from the records of the call, counts 2 flop per amplitude less for every
  two-shear X of the forward sweep and 0.125 more for every instance that has one (entry 0 of its table): with all four
  exponents under 2/3 the option saves 4 x 2 - 0.125 -- four X gates in ONE FULL instance -- and with exponents
  (0.5, 0.8, 0.3, 0.9) it saves 2 x 2 - 0.125: the same instance holds two flagged and two unflagged gates."""
  n, U = 4, 3
  gates, names = O.hea_gates(n, 1, "sx")
  P = len(names)
  rng = np.random.default_rng(44)
  ops = [O.xxz_chain_op(n), O.tfim_ring_op(n)]
  bits = rng.integers(0, 2, size=(U, n)).astype(np.int8)
  x_params = [g[3] for g in gates if g[0] == O.GATE_XPOW]
  base = rng.uniform(-1, 1, P).astype(np.float32)
  saved = {}
  for label, xs in (("all under", (0.5, -0.6, 0.3, 0.1)), ("straddle", (0.5, 0.8, 0.3, 0.9))):
    params = base.copy()
    params[x_params] = np.float32(xs)
    want_vals, want_jac = O.expectation_jacobian(n, gates, params.astype(np.float64), bits, ops)
    c = dict(bits=bits, params=params, vals=want_vals, jac=want_jac, ops=ops)
    flops = {}
    for on in (1, 0):
      eng = _engine(n, gates, P, ops, x_two_shear=on)
      _check(c, eng, f"{label} x_two_shear={on}")
      flops[on] = eng.flop_model(U, True)
    amps = float(U << 10)  # (states of fewer than 10 qubits are padded to one tile of 2^10)
    saved[label] = ((flops[0]["fwd_flops"] - flops[1]["fwd_flops"]) / amps, (flops[0]["bwd_flops"] - flops[1]["bwd_flops"]) / amps)
    print(label, "flop per amplitude saved (forward, adjoint):", saved[label])
  assert saved["all under"] == pytest.approx((4 * 2 - 0.125, 4 * 4 - 0.25), rel=1e-9), saved
  assert saved["straddle"] == pytest.approx((2 * 2 - 0.125, 2 * 4 - 0.25), rel=1e-9), saved
