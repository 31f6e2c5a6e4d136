"""The eight-wide gradient reductions of the adjoint kernels (csrc/kernels.hip add_slot_l1 / add_slots8 / store_slots8 /
store_slots8x2): level 1 is issued where a partial is made, the X + PH1 set and the PH2 set of an instance share their
last stage and their store.  Per-state gradient rows (`state_gradients`) and values against the C oracle
(oracle/qhbm_cpu.py), with the tolerances of tests/test_x_two_shear_gpu.py.

SETS: per size a handful of circuits whose instances between them reduce every combination of sets, ASSERTED on the
plans (describe_schedule's `records by sets reduced`).  `mixed`: two ansatz layers with every CZ pair of four
neighbouring qubits (FULL tables, one with all ten terms, others with few), X exponents either side of 2/3, X gates
frozen by the gradient mask (no slot) -- instances with X + PH1 and PH2, and with all three sets.  The others are a few
gates each and make ONE kind of instance: only an X; only a PH1; X + PH1 without PH2; only a PH2 (its X gates are
frozen), so that the shared stage runs with either side undefined; only a CPH, with a predicate that is off in whole
waves from 11 qubits on and in whole tiles at 14; a FULL table with the fewest terms the planner's default allows (four:
it makes a table when 18 PH1 + 10 PH2 > 60) and, with the engine option `adjoint_full_diag_threshold` lowered to 25, a
FULL table with TWO terms -- eight of its ten level-1 adds feed lanes without a slot (the table with all ten terms is in
ALONE).  Sizes: single-tile plans at 10 .. 13 qubits (one, two, four and eight
waves per workgroup store cells) and 14 qubits on tiles of 2^12 (tile-bit predicates, the tile-order reduction);
two-shear X on and off.  Two runs, and the batch cut by `chunk_states`, give identical bits.

ALONE: one partial alone in a set.  A last layer with every gate trainable in which the X exponents are exactly 0 except
where the target needs a superposition (those X gates come first and are frozen), every qubit starts in |0> and the
observable has X terms on the target's qubits only: every amplitude outside the target's subspace is exactly zero, and
so is -- in exact arithmetic AND in floats, a sum of products with a zero factor -- every gradient but the target's
set-mates.  The rows must match the oracle, and the entries that are exactly zero must come out as exact zeros: a
partial stored from the wrong lane, or an undefined bank that reaches a stored lane, shows.  The targets run over every
X, Z and CZ gate of the layer, and the plans are ASSERTED to put a slot at every value position of every set
(`slots at value position`)."""
import functools
import re

import numpy as np
import pytest
import torch

from oracle import qhbm_cpu as C
from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E

pytestmark = pytest.mark.gpu

X, Z, CZ = O.GATE_XPOW, O.GATE_ZPOW, O.GATE_CZPOW
SIZES = {"n10": (10, 10), "n11": (11, 11), "n12": (12, 12), "n13": (13, 13), "n14_k12": (14, 12)}


def _op_norm(ops):
  return np.array([sum(abs(c) for c, _, _ in op) for op in ops])


def _engine(device, n, gates, n_params, ops, mask=None, **options):
  eng = E.Engine(device)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(n, gates, n_params)
  eng.set_observables(ops)
  if mask is not None:
    eng.set_gradient_mask(mask)
  return eng


def _adjoint_lines(eng):
  text = eng.describe_schedule()
  return text[text.index("adjoint"):]


def slot_positions(eng):
  """[4 groups][8 value positions] records with a slot there, and [16] records by the sets they reduce."""
  m = re.search(r"slots at value position 0\.\.7, by group: (\S+) (\S+) (\S+) (\S+); records by sets reduced 0\.\.15: (\S+)",
                _adjoint_lines(eng))
  return (np.array([[int(t) for t in m.group(g).split("/")] for g in (1, 2, 3, 4)]),
          np.array([int(t) for t in m.group(5).split("/")]))


class _Circuit:
  def __init__(self):
    self.gates, self.values, self.frozen = [], [], []

  def add(self, kind, q0, q1, value, frozen=False):
    self.gates.append((kind, q0, q1, len(self.values), 1.0, 0.0))
    self.values.append(value)
    self.frozen.append(frozen)

  @property
  def params(self):
    return np.array(self.values, np.float32)

  @property
  def mask(self):
    return ~np.array(self.frozen, bool)


def mixed_circuit(n):
  rng = np.random.default_rng(100 + n)
  t = lambda: float(rng.uniform(-0.6, 0.6))  # (|t| < 2/3: the X gates next to a table run as two shears when the option is on)
  c = _Circuit()
  for q in range(n):  # first layer: FULL tables; the X of every third qubit frozen (no slot)
    c.add(X, q, -1, t(), frozen=q % 3 == 1)
    c.add(Z, q, -1, t())
  for q0 in list(range(0, n - 1, 2)) + list(range(1, n - 1, 2)):
    c.add(CZ, q0, q0 + 1, t())
  for a, b in ((0, 2), (0, 3), (1, 3)):  # with the chain: all six pairs of qubits 0..3 -- a table with all ten terms
    c.add(CZ, a, b, t())
  for q in range(n):  # second layer: X above 2/3 on odd qubits (three shears), no Z on qubits 4, 5 (tables with few terms)
    c.add(X, q, -1, 0.8 if q % 2 else t())
    if q not in (4, 5):
      c.add(Z, q, -1, t())
  for q0 in range(0, n - 1, 2):
    c.add(CZ, q0, q0 + 1, t())
  # a ragged third layer: gates that depend on each other through their qubits, some X frozen
  c.add(X, 2, -1, t())
  c.add(Z, 2, -1, t())
  c.add(X, 2, -1, t())
  c.add(CZ, 2, 3, t())
  c.add(X, 3, -1, t())
  c.add(CZ, n - 1, 3, t())
  c.add(X, n - 1, -1, t())
  c.add(Z, n - 1, -1, t())
  c.add(X, 6, -1, t(), frozen=True)
  c.add(CZ, 6, 7, t())
  c.add(X, 7, -1, t())
  c.add(CZ, 7, 8, t())
  c.add(CZ, 8, 9, t())
  c.add(X, 8, -1, t(), frozen=True)
  return c


def lone_circuit(kind, n):
  """A few gates that make one kind of instance (frozen X gates put a qubit into superposition without a slot)."""
  c = _Circuit()
  if kind == "x":
    c.add(X, 3, -1, 0.4)
  elif kind == "ph1":
    c.add(X, 3, -1, 0.5, frozen=True)
    c.add(Z, 3, -1, 0.3)
  elif kind == "x_ph1":
    c.add(X, 3, -1, 0.4)
    c.add(Z, 3, -1, 0.3)
  elif kind == "ph2":  # (the frozen CZ keeps the first X out of the instance of the frozen ones)
    c.add(X, 3, -1, 0.4)
    c.add(CZ, 3, 4, 0.2, frozen=True)
    c.add(X, 3, -1, 0.5, frozen=True)
    c.add(X, 4, -1, 0.5, frozen=True)
    c.add(CZ, 3, 4, 0.3)
  elif kind in ("full_two", "full_four"):
    # FULL tables with few terms: most of the ten level-1 adds behind full_partials feed lanes that have no slot.  The
    # planner makes a table when 18 PH1 + 10 PH2 exceeds `adjoint_full_diag_threshold` (default 60: four terms at the
    # least, here four PH1); with the threshold at 25 (FULL_TWO_OPTIONS) one PH1 and one PH2 make a table of TWO terms.
    for q in range(4 if kind == "full_four" else 2):
      c.add(X, q, -1, 0.5 - 0.1 * q)
    if kind == "full_four":
      for q in range(4):
        c.add(Z, q, -1, 0.3 + 0.05 * q)
    else:
      c.add(Z, 0, -1, 0.3)
      c.add(CZ, 0, 1, 0.2)
  elif kind == "cph_wave":  # the partner qubit stays a basis state: a thread bit (a wave bit from 11 qubits on)
    c.add(X, n - 1, -1, 0.5, frozen=True)
    c.add(CZ, n - 1, 4, 0.3)
  elif kind == "cph_tile":  # at 14 qubits on tiles of 2^12 qubit 1 is a tile bit
    c.add(X, 3, -1, 0.5, frozen=True)
    c.add(CZ, 3, 1, 0.3)
  return c


# circuit -> the set combinations its records must show, and no others (bit 0: X + PH1, bit 1: PH2, bit 2: CPH)
LONE = {"x": {1}, "ph1": {1}, "x_ph1": {1}, "ph2": {1, 2}, "cph_wave": None, "cph_tile": None, "full_two": {3}, "full_four": {1}}
FULL_TWO_OPTIONS = dict(adjoint_full_diag_threshold=25)
# circuit -> (FULL records, their PH1 terms, their PH2 terms) of its adjoint plan
FULL_TERMS = {"full_two": (1, 1, 1), "full_four": (1, 4, 0)}
CIRCUITS = ["mixed"] + sorted(LONE)


@functools.lru_cache(maxsize=None)
def _case(name, circuit):
  """Circuit, parameters, bitstrings, upstream weights, and the oracle's values and per-state rows: computed once per
  size and circuit and shared, never modified."""
  n, K = SIZES[name]
  c = mixed_circuit(n) if circuit == "mixed" else lone_circuit(circuit, n)
  rng = np.random.default_rng(7 * n)
  ops = [O.xxz_chain_op(n), O.tfim_ring_op(n)]
  bits = rng.integers(0, 2, size=(3, n)).astype(np.int8)
  bits[0], bits[1] = 1, 0  # (a boundary phase next to a basis-state qubit is on in the first state and off in the second)
  up = rng.normal(size=(3, 2)).astype(np.float32)
  return dict(n=n, K=K, c=c, ops=ops, bits=bits, up=up, **_oracle(n, c, bits, ops, up))


def _oracle(n, c, bits, ops, up):
  rows, vals = [], []
  for u in range(bits.shape[0]):  # (the C oracle returns the sum over states: one call per state gives the rows)
    v, g = C.expectation_vjp(n, c.gates, c.params, bits[u:u + 1], ops, up[u:u + 1])
    vals.append(v[0])
    rows.append(np.where(c.mask, g, 0.0))
  vals, rows = np.array(vals), np.array(rows)
  vals.setflags(write=False)
  rows.setflags(write=False)
  return dict(vals=vals, rows=rows)


def _run(eng, c, bits, up):
  vals, grad = eng.expectation_vjp(bits, c.params, up)
  rows = eng.state_gradients(bits.shape[0])
  return vals, grad, rows


def _check(label, case, vals, grad, rows):
  want = case["rows"]
  scale = max(1.0, np.abs(want).max())
  ev = np.abs(vals.cpu().numpy() - case["vals"]).max()
  er = np.abs(rows.cpu().numpy() - want).max()
  print(f"{label}: max |dval| = {ev:.3g}, max |drow| = {er:.3g} (scale {scale:.3g})")
  np.testing.assert_allclose(vals.cpu().numpy(), case["vals"], atol=2e-5 * _op_norm(case["ops"]).max(), rtol=0, err_msg=label)
  np.testing.assert_allclose(rows.cpu().numpy(), want, atol=1e-4 * scale, rtol=0, err_msg=label)
  np.testing.assert_allclose(grad.cpu().numpy(), want.sum(0), atol=1e-4 * max(1.0, np.abs(want.sum(0)).max()), rtol=0, err_msg=label)


@pytest.mark.parametrize("two_shear", [1, 0])
@pytest.mark.parametrize("name", sorted(SIZES))
def test_every_combination_of_sets_matches_the_oracle_row_by_row(name, two_shear):
  seen = set()
  for circuit in CIRCUITS:
    case = _case(name, circuit)
    c = case["c"]
    label = f"{name} {circuit} x_two_shear={two_shear}"
    eng = _engine(0, case["n"], c.gates, len(c.values), case["ops"], c.mask, x_two_shear=two_shear,
                  tile_qubits=case["K"], adjoint_tile_qubits=case["K"], **(FULL_TWO_OPTIONS if circuit == "full_two" else {}))
    _, sets = slot_positions(eng)
    combos = {m for m in range(1, 16) if sets[m]}
    seen |= combos
    census = eng.op_census(adjoint=True)
    if circuit == "mixed":
      text = _adjoint_lines(eng)
      full = re.search(r"FULL-PH1=(\d+) FULL-PH2=(\d+)", text)
      assert int(full.group(1)) > 0 and int(full.group(2)) > 0, text
      assert {3, 7} <= combos, (label, sets)
      assert sum(r["x_no_slot"] for r in census) > 0                 # a frozen X is un-applied without a partial
    elif LONE[circuit] is not None:
      assert combos == LONE[circuit], (label, sets)
    if circuit in FULL_TERMS:
      m = re.search(r"\(FULL (\d+)\) .* FULL-PH1=(\d+) FULL-PH2=(\d+)", _adjoint_lines(eng))
      assert tuple(int(m.group(i)) for i in (1, 2, 3)) == FULL_TERMS[circuit], (label, _adjoint_lines(eng))
    if circuit == "cph_wave" and case["n"] <= 13:
      assert combos == {4}, (label, sets)
    if circuit == "cph_wave" and 10 < case["n"] <= 13:
      assert sum(r["cph_wave_on"] for r in census) > 0 and sum(r["cph_off"] for r in census) > 0, (label, census)
    if circuit == "cph_tile" and name == "n14_k12":
      assert combos == {4} and sum(r["cph_tile_on"] for r in census) > 0, (label, sets, census)
    vals, grad, rows = _run(eng, c, case["bits"], case["up"])
    _check(label, case, vals, grad, rows)
    assert (rows.cpu().numpy()[:, ~c.mask] == 0).all(), label
    # two runs, and the batch cut into chunks, give identical bits
    vals2, grad2, rows2 = _run(eng, c, case["bits"], case["up"])
    assert torch.equal(vals, vals2) and torch.equal(grad, grad2) and torch.equal(rows, rows2), label
    eng.set_option("chunk_states", 2)
    vals3, grad3, rows3 = _run(eng, c, case["bits"], case["up"])
    assert torch.equal(vals, vals3) and torch.equal(grad, grad3) and torch.equal(rows, rows3), label
  # only X + PH1 | only PH2 | X + PH1 and PH2 | only CPH | all three: every combination the shared stage can meet
  assert {1, 2, 3, 4, 7} <= seen, seen


def alone_circuit(n, target):
  """`target` = (kind, q0, q1) of the last layer's gate whose partial is nonzero (with the Z gates of its qubits, for a
  CZ): see the module docstring."""
  kind, q0, q1 = target
  hot = [q0] if kind != CZ else [q0, q1]
  c = _Circuit()
  if kind != X:
    for q in hot:
      c.add(X, q, -1, 0.5, frozen=True)
  for q in range(n):
    if kind == X or q not in hot:
      c.add(X, q, -1, 0.37 if (kind == X and q == q0) else 0.0)
    if not (kind == X and q == q0):
      c.add(Z, q, -1, 0.21 + 0.01 * q)
  for a in list(range(0, n - 1, 2)) + list(range(1, n - 1, 2)):
    c.add(CZ, a, a + 1, 0.3 + 0.01 * a)
  for a, b in ((0, 2), (0, 3), (1, 3)):
    c.add(CZ, a, b, 0.17)
  live = [i for i, g in enumerate(c.gates) if not c.frozen[i] and set(q for q in g[1:3] if q >= 0) <= set(hot)
          and (g[0] != X or kind == X)]
  ops = [[O.pauli_term(1.0, [(q, "X")]) for q in hot] + [O.pauli_term(0.5, [(q, "Z"), ((q + 1) % n, "Z")]) for q in range(n)]]
  return c, ops, live


def alone_targets(n):
  return ([(X, q, -1) for q in range(n)] + [(Z, q, -1) for q in range(n)] + [(CZ, q, q + 1) for q in range(n - 1)]
          + [(CZ, 0, 2), (CZ, 0, 3), (CZ, 1, 3)])


def k4_circuit(n, pair, all_terms):
  """X on qubits 0..3 only (their round's register bits), exponent 0 but on `pair`; then every Z and CZ on those four
  qubits (a FULL table with all ten terms) or the pair's CZ alone (a per-term PH2): the PH2 partial of `pair` is the
  only one of its set that is not exactly zero."""
  c = _Circuit()
  for q in range(4):
    c.add(X, q, -1, 0.5 if q in pair else 0.0)
  if all_terms:
    for q in range(4):
      c.add(Z, q, -1, 0.21 + 0.01 * q)
    for a in range(4):
      for b in range(a + 1, 4):
        c.add(CZ, a, b, 0.3 + 0.01 * (a + 4 * b))
  else:
    c.add(CZ, pair[0], pair[1], 0.3)
  live = [i for i, g in enumerate(c.gates) if set(q for q in g[1:3] if q >= 0) <= set(pair)]
  ops = [[O.pauli_term(1.0, [(q, "X")]) for q in pair] + [O.pauli_term(0.5, [(q, "Z"), ((q + 1) % n, "Z")]) for q in range(n)]]
  return c, ops, live


def _check_alone(label, n, K, c, ops, live):
  """Runs the circuit on |0..0>; returns the plan's slot positions and the largest deviation from the oracle."""
  bits = np.zeros((1, n), np.int8)
  up = np.ones((1, 1), np.float32)
  eng = _engine(0, n, c.gates, len(c.values), ops, c.mask, tile_qubits=K, adjoint_tile_qubits=K)
  vals, grad, rows = _run(eng, c, bits, up)
  want_vals, want = C.expectation_vjp(n, c.gates, c.params, bits, ops, up)
  want = np.where(c.mask, want, 0.0)
  got = rows.cpu().numpy()[0]
  dead = np.ones(len(c.values), bool)
  dead[live] = False
  # the construction: nothing but the live partials in the oracle either (its X partial carries Im<lam|psi>: rounding)
  assert np.abs(want[dead]).max() < 2e-6 and np.abs(want[live]).max() > 1e-3, (label, want)
  assert (got[dead] == 0).all(), (label, np.nonzero(got * dead)[0], got[got * dead != 0])
  np.testing.assert_allclose(got, want, atol=1e-4 * max(1.0, np.abs(want).max()), rtol=0, err_msg=label)
  np.testing.assert_allclose(vals.cpu().numpy(), want_vals, atol=2e-5 * _op_norm(ops).max(), rtol=0, err_msg=label)
  assert torch.equal(grad, rows[0]), label
  return slot_positions(eng)[0], np.abs(got - want).max()


@pytest.mark.parametrize("name", ["n10", "n14_k12"])
def test_one_partial_alone_at_every_position_of_every_set(name):
  n, K = SIZES[name]
  at = np.zeros((4, 8), int)
  worst = 0.0
  for target in alone_targets(n):  # (one plan: every gate of the layer has a slot, and every one is the target once)
    c, ops, live = alone_circuit(n, target)
    got, err = _check_alone(f"{name} {target}", n, K, c, ops, live)
    at, worst = np.maximum(at, got), max(worst, err)
  print(name, "slots at value position, by group:", at.tolist(), "max |drow| =", worst)
  # X at 0..3 and PH1 at 4..7 of group 0, the eight boundary phases of group 2
  assert (at[0] > 0).all() and (at[2] > 0).all(), at
  pairs = [(a, b) for a in range(4) for b in range(a + 1, 4)]
  for all_terms in (True, False):
    at = np.zeros((4, 8), int)
    for pair in pairs:
      c, ops, live = k4_circuit(n, pair, all_terms)
      got, err = _check_alone(f"{name} k4 {pair} all_terms={all_terms}", n, K, c, ops, live)
      if all_terms:
        assert (got[1][:6] == 1).all() and (got[0][4:] == 1).all(), (pair, got)  # ONE table with all ten terms: six pairs, four PH1
      else:
        assert got[1].sum() == 1, (pair, got)         # one per-term PH2
      at, worst = at + got, max(worst, err)
    print(name, "k4 all_terms =", all_terms, "PH2 slots:", at[1].tolist(), "max |drow| =", worst)
    assert (at[1][:6] > 0).all(), at                  # the six pairs between them sit at the six positions
