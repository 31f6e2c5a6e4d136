"""The complex128 restatement of the final-states VJP (tests/final_states_ref.py) against central differences of its
three losses in float64 -- step 1e-5, bar 1e-7 * max(1, ||grad||_inf): the truncation error h^2 f''' / 6 of losses whose
third derivatives are O(pi^3 |scalar|^3 |loss|) is ~1e-8 here, the rounding error 2^-53 |loss| / h ~1e-11.  No engine, no GPU.

The GPU tests (tests/test_final_states_gpu.py) hold the engine to this restatement, so what must be true of the
restatement for those tests to bite is asserted here too: under the phase-sensitive loss (B) the share of the gradient
that comes through the global phase alone is at least 10 % of ||grad||_inf -- a thousand times the GPU bar."""
import numpy as np
import pytest

from oracle import qhbm_oracle as O
from tests import final_states_ref as F
from tests import from_states_ref as R

STEP = 1e-5


def _bar(grad):
  return 1e-7 * max(1.0, float(np.abs(grad).max()))


def _central(n, gates, params, states, kind, aux):
  out = np.zeros(len(params))
  for p in range(len(params)):
    hi, lo = params.copy(), params.copy()
    hi[p] += STEP
    lo[p] -= STEP
    out[p] = (F.loss_of(kind, R.final_states(n, gates, hi, states), aux)[0] -
              F.loss_of(kind, R.final_states(n, gates, lo, states), aux)[0]) / (2 * STEP)
  return out


@pytest.mark.parametrize("kind", ["A", "B", "C"])
@pytest.mark.parametrize("name", ["hea3", "hea6", "hea10", "all_kinds"])
def test_vjp_matches_central_differences(name, kind):
  n, gates, params, states = F.case(name)
  aux = F.loss_aux(kind, 3, n, F.aux_seed(name))
  finals = R.final_states(n, gates, params, states)
  _, cot = F.loss_of(kind, finals, aux)
  got = F.vjp(n, gates, params, states, cot)
  want = _central(n, gates, params, states, kind, aux)
  err = float(np.abs(got - want).max())
  print(f"{name} loss {kind}: max |vjp - central| {err:.3e}  bar {_bar(want):.3e}  ||grad||_inf {np.abs(want).max():.3e}")
  assert err <= _bar(want)
  share = float(np.abs(F.phase_term(gates, len(params), finals, cot)).max()) / float(np.abs(got).max())
  print(f"{name} loss {kind}: phase term / ||grad||_inf = {share:.3f}")
  if kind == "B":  # (what makes the GPU bar of 1e-4 bite on a kernel that drops the phase term)
    assert share >= 0.10
  if kind in ("A", "C"):  # <g|psi> is real for these: the phase cannot matter
    assert share <= 1e-12


def test_all_kinds_circuit_has_every_phase_source():
  """The circuit the GPU test differentiates under loss (B): every gate kind, rotation-form shifts, X powers whose
  parameter carries a multiplier other than 1."""
  _, gates, _, _ = F.case("all_kinds")
  assert {g[0] for g in gates} == set(range(12))
  assert any(O.gate_global_shift(g) == -0.5 and g[3] >= 0 for g in gates)
  assert any(g[0] == O.GATE_XPOW and g[3] >= 0 and abs(g[4]) != 1.0 for g in gates)


@pytest.mark.parametrize("n", [3, 6])
def test_table_loss_is_a_diagonal_pauli_sum(n):
  """(C) against `values_and_vjp` of tests/from_states_ref.py: E[y] = sum_S theta_S (-1)^{|y & S|} is the table of the
  diagonal Pauli sum sum_S theta_S Z_S, and w is its upstream."""
  rng = np.random.default_rng(930 + n)
  gates, names = O.hea_gates(n, 2, "fv")
  params = rng.uniform(-1, 1, len(names))
  states = R.random_states(3, n, 940 + n) * np.array([0.5, 1.0, 3.0])[:, None]
  masks = sorted({int(m) for m in rng.integers(1, 1 << n, size=6)})
  thetas = rng.normal(size=len(masks))
  op = [(float(t), 0, m) for t, m in zip(thetas, masks)]  # (coefficient, x mask, z mask) in qubit space
  # amplitude index y reads the bitstring big-endian: qubit q is index bit n - 1 - q
  y = np.arange(1 << n)
  table = np.zeros(1 << n)
  for t, m in zip(thetas, masks):
    idx_mask = sum(1 << (n - 1 - q) for q in range(n) if m >> q & 1)
    table += t * (1.0 - 2.0 * (np.array([bin(v & idx_mask).count("1") for v in y]) & 1))
  w = rng.normal(size=3)
  finals = R.final_states(n, gates, params, states)
  value, cot = F.table_loss(finals, table, w)
  want_vals, want_grad = R.values_and_vjp(n, gates, params, states, [op], w[:, None])
  np.testing.assert_allclose(value, float(np.sum(w * want_vals[:, 0])), rtol=0, atol=1e-10)
  got = F.vjp(n, gates, params, states, cot)
  np.testing.assert_allclose(got, want_grad, rtol=0, atol=1e-10 * max(1.0, float(np.abs(want_grad).max())))
