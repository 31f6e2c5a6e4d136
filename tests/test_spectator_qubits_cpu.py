"""The spectator-qubit cases of tests/test_spectator_qubits_gpu.py, checked without a GPU: each family reaches the
forward-plan branch it is meant for (a planning-only engine), and the stacked oracle equals O.expectation_jacobian."""
import re

import numpy as np
import pytest

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from tests import spectator_cases as S

DIAGONAL = (O.GATE_ZPOW, O.GATE_CZPOW, O.GATE_ZZPOW)


def _forward_plan(n, gates, n_params, ops, tile):
  eng = E.Engine(None)
  eng.set_option("tile_qubits", tile)
  eng.set_option("adjoint_tile_qubits", min(tile, 13))
  eng.set_circuit(n, gates, n_params)
  eng.set_observables(ops)
  text = eng.describe_schedule().split("adjoint")[0]
  local = [set(map(int, m.split(","))) for m in re.findall(r"local=\[([0-9,]*)\]", text)]
  return eng.num_passes()[0], text, local


@pytest.mark.parametrize("family", list(S.FAMILIES))
@pytest.mark.parametrize("n", [11, 13, 14])
def test_each_family_reaches_its_first_pass_branch(n, family):
  gates, n_params, roles, _ = S.spectator_circuit(n, family, 1000 * n)
  for q, role in roles.items():
    on_q = [g for g in gates if q in g[1:3]]
    if role == "idle":
      assert not on_q
    elif role == "diag":
      assert on_q and all(g[0] in DIAGONAL for g in on_q) and any(g[0] == O.GATE_ZZPOW for g in on_q)
    else:
      flips = [i for i, g in enumerate(gates) if q in g[1:3] and g[0] not in DIAGONAL]
      assert len(flips) == 1 and flips[0] > len(gates) // 2
  for opset, ops in S.op_sets(n, roles, n).items():
    passes, text, local = _forward_plan(n, gates, n_params, ops, 10)
    assert passes > 1, opset
    # one idle or diagonal-only bit: the first pass zero-fills; a late-touched one: it writes one tile per state
    assert ("[zero-fill]" in text) == (family != "late"), (opset, text)
    assert ("[basis tile only]" in text) == (family == "late"), (opset, text)
    if family == "idle_low":       # index bit 0: local in every pass
      assert all(0 in s for s in local)
    if family == "idle_top":       # the top index bit: non-local in some pass, local in another
      assert any(n - 1 not in s for s in local) and any(n - 1 in s for s in local)
    passes, text, _ = _forward_plan(n, gates, n_params, ops, n)
    assert passes == 1 and "[zero-fill]" in text   # the single-pass control


def test_hea_plans_write_one_tile_per_state():
  n = 13
  gates, names = O.hea_gates(n, 2, "h")
  passes, text, _ = _forward_plan(n, gates, len(names), [O.tfim_ring_op(n)], 10)
  assert passes > 1 and "[basis tile only]" in text and "[zero-fill]" not in text


@pytest.mark.parametrize("family", list(S.FAMILIES))
def test_stacked_oracle_equals_the_numpy_oracle(family):
  n = 6
  gates, n_params, roles, _ = S.spectator_circuit(n, family, 6)
  rng = np.random.default_rng(6)
  params = rng.uniform(-1, 1, n_params)
  bits = rng.integers(0, 2, size=(3, n)).astype(np.int8)
  for ops in S.op_sets(n, roles, 6).values():
    vals, jac, states = S.stacked_jacobian(n, gates, params, bits, ops)
    want_vals, want_jac = O.expectation_jacobian(n, gates, params, bits, ops)
    np.testing.assert_allclose(vals, want_vals, atol=1e-12)
    np.testing.assert_allclose(jac, want_jac, atol=1e-12)
    for row, b in zip(states, bits):
      np.testing.assert_allclose(row, O.simulate(n, gates, params, b).ravel(), atol=1e-14)
  for q in S.idle_or_diag(roles):   # the closed forms the GPU tests use hold in the oracle
    shards = S.op_sets(n, roles, 6)["shards"]
    vals, jac, _ = S.stacked_jacobian(n, gates, params, bits, shards)
    z, x, y = (S.shard_index(n, roles, q, p) for p in "ZXY")
    np.testing.assert_allclose(vals[:, z], 1.0 - 2.0 * bits[:, q], atol=1e-12)
    np.testing.assert_allclose(vals[:, [x, y]], 0.0, atol=1e-12)
    np.testing.assert_allclose(jac[:, [z, x, y]], 0.0, atol=1e-12)
