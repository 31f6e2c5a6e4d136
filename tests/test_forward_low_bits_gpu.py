"""Forward plans that move the low index bits (engine option `forward_move_low_bits`) against the C oracle, against the
plans without the freedom, and against themselves.

Shapes: 13 and 14 qubits (tiles of 2^10: two and three gate passes and more; with the tile size left to the engine these
registers are ONE tile and nothing can move, so these two cases set `tile_qubits` and ask for the moving plan with option
value 2), 16 qubits at depth 16 (the engine's own choice, option value 1, tiles of 2^12), and 20 qubits at depth 4 with
4 states (tiles of 2^12 and a wide last pass; the cost model sees nothing to gain at that depth, so value 2 again).
Every case asserts that at least one forward pass permutes.

Tolerances are those of tests/test_engine_gpu.py: values 5e-5 * sum|c_k| (n > 12), gradients 1e-4 * max(1, |grad|_inf),
amplitudes 5e-6, parameter-shift gradients 5e-4 * max(1, |grad|_inf).  On against off is held to the same bars, not bit for
bit: gates that commute run in another order."""
import functools
import re

import numpy as np
import pytest

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E

pytestmark = pytest.mark.gpu

# (n, layers, states, options that make the plan permute)
CASES = {
    "n13": (13, 4, 5, {"tile_qubits": 10, "adjoint_tile_qubits": 10, "forward_move_low_bits": 2}),
    "n14": (14, 5, 5, {"tile_qubits": 10, "adjoint_tile_qubits": 10, "forward_move_low_bits": 2}),
    "n16": (16, 16, 4, {"forward_move_low_bits": 1}),
    "n20": (20, 4, 4, {"forward_move_low_bits": 2}),
}


def _op_norm(ops):
  return np.array([sum(abs(c) for c, _, _ in op) for op in ops])


def _engine(n, gates, n_params, ops, **options):
  eng = E.Engine(0)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(n, gates, n_params)
  eng.set_observables(ops)
  return eng


def _off(options):
  return dict(options, forward_move_low_bits=0)


def _forward_text(eng):
  return eng.describe_schedule().split("adjoint")[0]


def _permuting_passes(eng):
  return len(re.findall(r" moves-to-low=\[", _forward_text(eng)))


@functools.lru_cache(maxsize=None)
def _case(name):
  """The circuit, its inputs and the oracle's answers, computed once per case."""
  n, layers, count, options = CASES[name]
  rng = np.random.default_rng(1000 + n)
  gates, names = O.hea_gates(n, layers, name)
  params = rng.uniform(-1, 1, len(names))
  ops = [O.xxz_chain_op(n)]
  bits = rng.integers(0, 2, size=(count, n)).astype(np.int8)
  up = rng.normal(size=(count, 1))
  vals, jac = O.expectation_jacobian(n, gates, params, bits, ops)
  return dict(n=n, gates=gates, n_params=len(names), params=params, ops=ops, bits=bits, up=up, vals=vals, jac=jac,
              options=options)


@pytest.mark.parametrize("name", list(CASES))
def test_values_gradients_and_states_against_the_oracle(name):
  c = _case(name)
  n, ops = c["n"], c["ops"]
  eng = _engine(n, c["gates"], c["n_params"], ops, **c["options"])
  assert _permuting_passes(eng) >= 1, _forward_text(eng)
  off = _engine(n, c["gates"], c["n_params"], ops, **_off(c["options"]))
  assert _permuting_passes(off) == 0
  vtol = 5e-5 * np.maximum(_op_norm(ops), 1.0)[None, :]
  # values measured in the passes
  got = eng.expectation(c["bits"], c["params"]).cpu().numpy()
  err = np.abs(got - c["vals"])
  print(name, "values: max err", err.max(), "bar", vtol.max())
  assert (err <= vtol).all()
  assert (np.abs(got - off.expectation(c["bits"], c["params"]).cpu().numpy()) <= vtol).all()
  # adjoint VJP and per-state gradient rows (the adjoint's first pass reads the final states: identity layout)
  want_grad = np.einsum("bt,btp->p", c["up"], c["jac"])
  gtol = 1e-4 * max(1.0, np.abs(want_grad).max())
  vals, grad = eng.expectation_vjp(c["bits"], c["params"], c["up"])
  gerr = np.abs(grad.cpu().numpy() - want_grad).max()
  print(name, "vjp: max err", gerr, "bar", gtol)
  assert gerr <= gtol
  assert (np.abs(vals.cpu().numpy() - c["vals"]) <= vtol).all()
  _, grad_off = off.expectation_vjp(c["bits"], c["params"], c["up"])
  assert np.abs(grad.cpu().numpy() - grad_off.cpu().numpy()).max() <= gtol
  _, jac = eng.expectation_jacobian(c["bits"], c["params"])
  jtol = 1e-4 * max(1.0, np.abs(c["jac"]).max())
  jerr = np.abs(jac.cpu().numpy() - c["jac"]).max()
  print(name, "gradient rows: max err", jerr, "bar", jtol)
  assert jerr <= jtol
  # exported states
  want_sv = np.stack([O.simulate(n, c["gates"], c["params"], list(b)).ravel() for b in c["bits"][:2]])
  sv = eng.statevector(c["bits"][:2], c["params"]).cpu().numpy()
  serr = np.abs(sv - want_sv).max()
  print(name, "statevector: max err", serr, "bar 5e-6")
  assert serr <= 5e-6
  assert np.abs(sv - off.statevector(c["bits"][:2], c["params"]).cpu().numpy()).max() <= 5e-6


@pytest.mark.parametrize("name", ["n13", "n16"])
def test_bit_for_bit_with_itself(name):
  """Two runs; chunked against unchunked batches; a shard against the batch; parameter-shift programs with shared
  against unshared prefixes; the retained two-call VJP against the one-call VJP."""
  c = _case(name)
  n, ops = c["n"], c["ops"]
  rng = np.random.default_rng(7)
  bits = rng.integers(0, 2, size=(9, n)).astype(np.int8)
  up = rng.normal(size=(9, 1))
  eng = _engine(n, c["gates"], c["n_params"], ops, **c["options"])
  assert _permuting_passes(eng) >= 1
  v1, g1 = eng.expectation_vjp(bits, c["params"], up)
  v2, g2 = eng.expectation_vjp(bits, c["params"], up)
  assert np.array_equal(v1.cpu().numpy(), v2.cpu().numpy()) and np.array_equal(g1.cpu().numpy(), g2.cpu().numpy())
  e1 = eng.expectation(bits, c["params"]).cpu().numpy()
  s1 = eng.statevector(bits, c["params"]).cpu().numpy()
  chunked = _engine(n, c["gates"], c["n_params"], ops, chunk_states=4, **c["options"])
  assert np.array_equal(chunked.expectation(bits, c["params"]).cpu().numpy(), e1)
  assert np.array_equal(chunked.statevector(bits, c["params"]).cpu().numpy(), s1)
  vc, _ = chunked.expectation_vjp(bits, c["params"], up)
  assert np.array_equal(vc.cpu().numpy(), v1.cpu().numpy())
  # a shard of the batch (odd start, odd count: the paired kernel's last state runs twice)
  assert np.array_equal(eng.expectation(bits[3:8], c["params"]).cpu().numpy(), e1[3:8])
  assert np.array_equal(eng.statevector(bits[3:8], c["params"]).cpu().numpy(), s1[3:8])
  # parameter shift: shifted programs start from the base program's state behind the passes they share
  ps = eng.expectation_vjp(bits[:3], c["params"], up[:3], E.GRAD_PARAMETER_SHIFT)
  unshared = _engine(n, c["gates"], c["n_params"], ops, shift_prefix_sharing=0, **c["options"])
  pu = unshared.expectation_vjp(bits[:3], c["params"], up[:3], E.GRAD_PARAMETER_SHIFT)
  assert np.array_equal(ps[0].cpu().numpy(), pu[0].cpu().numpy()) and np.array_equal(ps[1].cpu().numpy(), pu[1].cpu().numpy())
  want_grad = np.einsum("bt,btp->p", up[:3], O.expectation_jacobian(n, c["gates"], c["params"], bits[:3], ops)[1])
  assert np.abs(ps[1].cpu().numpy() - want_grad).max() <= 5e-4 * max(1.0, np.abs(want_grad).max())
  # the retained two-call VJP against the one-call VJP
  kept = eng.expectation(bits, c["params"], retain=True)
  assert eng.retained is not None and np.array_equal(kept.cpu().numpy(), v1.cpu().numpy())
  assert np.array_equal(eng.expectation_vjp_retained(bits, c["params"], up).cpu().numpy(), g1.cpu().numpy())


@pytest.mark.parametrize("name", ["n13", "n16"])
def test_measured_in_passes_several_observables_masks_and_shears(name):
  """TFIM and XXZ as three observables (sums measured inside passes that load a moved layout), an end-to-end X X term that
  no gate pass can hold (a measure-only pass behind the restored layout), a frozen-parameter mask, and `x_two_shear` on
  and off.  That the plan has such passes is asserted from describe_schedule."""
  c = _case(name)
  n = c["n"]
  zz = [O.pauli_term(1.0, [(q, "Z"), (q + 1, "Z")]) for q in range(n - 1)]
  xx = [O.pauli_term(1.0, [(q, "X"), (q + 1, "X")]) for q in range(n - 1)]
  yy = [O.pauli_term(1.0, [(q, "Y"), (q + 1, "Y")]) for q in range(n - 1)]
  ends = [O.pauli_term(1.0, [(0, "X"), (n - 1, "X")])]
  ops = [O.tfim_ring_op(n), xx, yy, zz, ends]
  bits, params = c["bits"], c["params"]
  want_vals, want_jac = O.expectation_jacobian(n, c["gates"], params, bits, ops)
  up = np.random.default_rng(3).normal(size=(bits.shape[0], len(ops)))
  want_grad = np.einsum("bt,btp->p", up, want_jac)
  vtol = 5e-5 * np.maximum(_op_norm(ops), 1.0)[None, :]
  gtol = 1e-4 * max(1.0, np.abs(want_grad).max())
  for shear in (1, 0):
    eng = _engine(n, c["gates"], c["n_params"], ops, x_two_shear=shear, **c["options"])
    assert _permuting_passes(eng) >= 1
    lines = [l for l in _forward_text(eng).splitlines() if re.match(r"\s+pass \d+:", l)]
    assert any("[measure-only]" in l and " at=" not in l for l in lines), lines
    moved_and_measuring = [l for l in lines if " at=" in l and int(re.search(r"meas_groups=(\d+)", l).group(1)) > 0
                           and re.search(r"local=\[([\d,]+)\]", l).group(1) != re.search(r" at=([\d,]+)", l).group(1)]
    assert moved_and_measuring, lines
    got = eng.expectation(bits, params).cpu().numpy()
    assert (np.abs(got - want_vals) <= vtol).all(), np.abs(got - want_vals).max()
    vals, grad = eng.expectation_vjp(bits, params, up)
    assert (np.abs(vals.cpu().numpy() - want_vals) <= vtol).all()
    assert np.abs(grad.cpu().numpy() - want_grad).max() <= gtol
  mask = np.arange(c["n_params"]) % 3 != 0
  eng.set_gradient_mask(mask)
  _, grad = eng.expectation_vjp(bits, params, up)
  grad = grad.cpu().numpy()
  assert np.abs(grad[mask] - want_grad[mask]).max() <= gtol
