"""Forward plans that move the low index bits (engine option `forward_move_low_bits`), from planning-only engines: the
headline plan has two full-state passes and at most 0.6 of the forward bytes, ends in the identity layout, and the
option off gives the plans of before, to the letter; single tiles, dense-start plans and plans with a Y gate never move."""
import os
import re

import numpy as np
import pytest

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "headline_schedule_without_low_bit_moves.txt")


def _planner(n, gates, n_params, ops, **options):
  eng = E.Engine(None)
  for k, v in options.items():
    eng.set_option(k, v)
  eng.set_circuit(n, gates, n_params)
  eng.set_observables(ops)
  return eng


def _headline(**options):
  n, layers = 20, 16
  gates, names = O.hea_gates(n, layers, "c3")
  return _planner(n, gates, len(names), [O.xxz_chain_op(n)], **options)


def _forward_passes(text):
  """(K, logical bits of the tile, their positions at load, bits the store moves to positions 0..3 or None)."""
  out = []
  for line in text.split("adjoint")[0].splitlines():
    m = re.match(r"\s+pass \d+: K=(\d+) c=\d+ local=\[([\d,]+)\]", line)
    if not m:
      continue
    local = [int(b) for b in m.group(2).split(",")]
    at = re.search(r" at=([\d,]+)", line)
    moved = re.search(r" moves-to-low=\[([\d,]+)\]", line)
    out.append(dict(K=int(m.group(1)), local=local, at=[int(b) for b in at.group(1).split(",")] if at else sorted(local),
                    moves=[int(b) for b in moved.group(1).split(",")] if moved else None,
                    measure_only="[measure-only]" in line))
  return out


def test_headline_plan_has_two_full_passes_and_ends_in_the_identity_layout():
  on, off = _headline(forward_move_low_bits=1), _headline(forward_move_low_bits=0)
  passes = _forward_passes(on.describe_schedule())
  assert any(p["moves"] for p in passes)
  # a full state's worth of tiles: 2^(n - K) per state
  rows = on.op_census(adjoint=False)
  gate_rows = [(r, p) for r, p in zip(rows, passes) if not p["measure_only"]]
  full = [r for r, p in gate_rows if r["tiles"] >= 2 ** (20 - p["K"])]
  assert len(full) <= 2, [(r["tiles"], p["K"]) for r, p in gate_rows]
  ratio = on.traffic_model(4096, True)["fwd_bytes"] / off.traffic_model(4096, True)["fwd_bytes"]
  assert ratio <= 0.6, ratio
  # the last gate pass restores logical = physical: it holds index bits 0..3 and puts them back on positions 0..3, and
  # everything after it (a measure-only pass) sits at its own positions
  last = [p for p in passes if not p["measure_only"]][-1]
  assert last["moves"] is not None and sorted(last["moves"]) == [0, 1, 2, 3]
  assert sorted(last["at"]) == sorted(last["local"])  # in place: the tile owns the positions of its own bits
  for p in passes:
    if p["measure_only"]:
      assert p["at"] == sorted(p["local"]) and p["moves"] is None
  # every pass holds the four bits that sit on the 128-byte line when it loads
  assert all(p["at"][:4] == [0, 1, 2, 3] for p in passes)
  # the same X gates as before
  assert sum(r["x"] / r["tiles"] for r in rows if r["tiles"]) == pytest.approx(
      sum(r["x"] / r["tiles"] for r in off.op_census(adjoint=False) if r["tiles"]))


def test_option_off_is_the_plan_of_before():
  with open(GOLDEN) as f:
    assert _headline(forward_move_low_bits=0).describe_schedule() == f.read()


def test_backward_plan_does_not_depend_on_the_option():
  on, off = _headline(forward_move_low_bits=1).describe_schedule(), _headline(forward_move_low_bits=0).describe_schedule()
  assert on != off and on[on.index("adjoint"):] == off[off.index("adjoint"):]


@pytest.mark.parametrize("n,layers", [(4, 2), (10, 3), (12, 8)])
def test_single_tiles_do_not_move(n, layers):
  gates, names = O.hea_gates(n, layers, "small")
  ops = [O.xxz_chain_op(n), O.tfim_ring_op(n)]
  texts = [_planner(n, gates, len(names), ops, forward_move_low_bits=v).describe_schedule() for v in (0, 1, 2)]
  assert texts[0] == texts[1] == texts[2] and "moves-to-low" not in texts[0]


def test_dense_start_plans_do_not_move():
  n, layers = 16, 16
  gates, names = O.hea_gates(n, layers, "dense")
  ops = [O.xxz_chain_op(n)]
  on, off = (_planner(n, gates, len(names), ops, forward_move_low_bits=v) for v in (1, 0))
  assert "moves-to-low" in on.describe_schedule()  # (the basis-state plan of this circuit does move)
  assert on.describe_schedule_from_states() == off.describe_schedule_from_states()


def test_plans_with_a_y_gate_do_not_move(monkeypatch):
  """A Y**t that stays a Y micro-op (no lean lowering) turns its pass over to the general kernel, which has no moving store."""
  monkeypatch.setenv("QHBM_NO_LEAN_CLIFFORD", "1")
  n, layers = 16, 16
  gates, names = O.hea_gates(n, layers, "y")
  P = len(names)
  gates = gates + [(O.GATE_YPOW, 5, -1, 0, 1.0, 0.0)]
  ops = [O.xxz_chain_op(n)]
  texts = [_planner(n, gates, P, ops, forward_move_low_bits=v).describe_schedule() for v in (0, 1)]
  assert texts[0] == texts[1] and "moves-to-low" not in texts[0]
  monkeypatch.delenv("QHBM_NO_LEAN_CLIFFORD")
  assert "moves-to-low" in _planner(n, gates, P, ops, forward_move_low_bits=1).describe_schedule()  # (lowered to X: lean)


def test_explicit_tile_size_keeps_the_plan_unless_forced():
  n, layers = 14, 5
  gates, names = O.hea_gates(n, layers, "tile")
  ops = [O.xxz_chain_op(n)]
  texts = [_planner(n, gates, len(names), ops, tile_qubits=10, forward_move_low_bits=v).describe_schedule() for v in (0, 1, 2)]
  assert texts[0] == texts[1] and "moves-to-low" in texts[2]
