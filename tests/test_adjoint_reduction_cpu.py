"""The count of level-1 adds of the adjoint's gradient reductions (qhbm_op_census column `level1`, describe_schedule's
`level1_adds`), from planning-only engines: kernels.hip issues one such add where a partial is made -- one per header
bit of a micro-op with a partial (an X gate that owns a slot, a per-term PH1 or PH2, a CPH whether its predicate is on
or off in the wave) and ten per FULL record -- so the count follows from the census columns that count those micro-ops."""
import re

import numpy as np
import pytest

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E


def _planner(n, gates, n_params, ops, mask=None):
  eng = E.Engine(None)
  eng.set_circuit(n, gates, n_params)
  eng.set_observables(ops)
  if mask is not None:
    eng.set_gradient_mask(mask)
  return eng


def _formula(row):
  return (row["x"] + row["ph1"] + row["ph2"] + row["cph_tile_on"] + row["cph_wave_on"] + row["cph_lane"] + row["cph_off"]
          + 10 * row["full"])


def _inverted(n, layers):
  gates, names = O.hea_gates(n, layers, "inv")
  P = len(names)
  return gates + [(k, a, b, p + P, -s, -o) for (k, a, b, p, s, o) in reversed(gates)], 2 * P


def test_level1_adds_of_the_headline_plan():
  """20 qubits, depth 16, XXZ: per state 652 726 level-1 adds where eight per reduction would be 1 403 416."""
  n, layers = 20, 16
  gates, names = O.hea_gates(n, layers, "c3")
  eng = _planner(n, gates, len(names), [O.xxz_chain_op(n)])
  adj = eng.op_census(adjoint=True)
  for row in adj:
    assert row["level1"] == _formula(row) and row["level1"] > 0, row
  assert sum(r["level1"] for r in adj) == 652726 and 8 * sum(r["reduce8"] for r in adj) == 1403416
  assert all(r["level1"] == 0 for r in eng.op_census(adjoint=False))
  # describe_schedule: per pass, the adds of a wave that runs every record of the pass once
  static = [int(m) for m in re.findall(r" level1_adds=(\d+)", eng.describe_schedule())]
  assert len(static) == len(adj) and all(s > 0 for s in static)
  # (a pass whose waves are all alive in every round executes exactly that per wave)
  for s, row in zip(static, adj):
    assert row["level1"] <= s * row["tiles"] * 4 + 1e-9, (s, row)


@pytest.mark.parametrize("frozen", [False, True])
def test_level1_adds_of_an_inverted_circuit(frozen):
  """U then its inverse with parameters of its own (instances without a FULL table, X gates in front of a table), and
  with every other parameter frozen: an X without a slot has no partial and no add."""
  n = 13
  gates, P = _inverted(n, 3)
  mask = (np.arange(P) % 2 == 0) if frozen else None
  eng = _planner(n, gates, P, [O.xxz_chain_op(n), O.tfim_ring_op(n)], mask)
  adj = eng.op_census(adjoint=True)
  assert sum(r["ph1"] + r["ph2"] for r in adj) > 0 and sum(r["full"] for r in adj) > 0
  assert (sum(r["x_no_slot"] for r in adj) > 0) == frozen
  for row in adj:
    assert row["level1"] == _formula(row), row
