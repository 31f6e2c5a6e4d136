"""The sessions of tests/lifecycle_cases.py are what they claim to be (no GPU: planner-only engines and the oracle).

A session can only catch a stale plan, scale, table, mask or answer if the step in front of it had another one.  Here:
every setter a session says changes the schedule does; consecutive calls of one kind have oracle outputs that differ by
100 tolerances at least; the refusal sequences of the GPU module never move to a configuration that needs more slots,
parameters or workspace (an engine that serves stale rows anyway then stays inside memory it owns); and every random
walk reaches every entry point, with a setter of each kind between two calls."""
import functools

import numpy as np
import pytest

from qhbmlib_amd import _engine as E
from tests import lifecycle_cases as L


@functools.lru_cache(maxsize=None)
def _walk(name):
  return L.walk(L.sessions()[name])


_PLANS = {}


def _plan(shadow):
  """(num_passes, describe_schedule) of a planner-only engine configured like `shadow`."""
  key = shadow.key()
  if key not in _PLANS:
    eng = shadow.configure(E.Engine(device=None))
    _PLANS[key] = (eng.num_passes(), eng.describe_schedule())
  return _PLANS[key]


def test_the_sessions_are_the_ones_named():
  assert tuple(L.sessions()) == L.SESSION_NAMES
  assert 3 <= len(L.WALK_SEEDS) <= 5
  for seed in L.WALK_SEEDS:
    assert abs(len(L.sessions()[f"random walk {seed}"]["steps"]) - L.WALK_STEPS) <= 6
  params = [L.circuit(c)[2] for c in L.CIRCUITS]
  assert len(set(params)) == len(params), params
  assert {L.circuit(c)[0] for c in L.CIRCUITS} == {4, 11, 13, 14}


def test_ingredients_have_the_mechanisms():
  """The zero-filling plan, the multi-pass plans, the padded tile; wide terms, 65 operators, >= 32 diagonal terms;
  consecutive observable lists 2^20 apart."""
  for name in L.CIRCUITS:
    s = L.Shadow()
    s.apply(0, ("set_circuit", name))
    (fwd, bwd), text = _plan(s)
    assert (fwd > 1 and bwd > 1) if s.n > 10 else (fwd == 1 and "n_eff=10" in text), (name, fwd, bwd)
    # the first pass zero-fills where an index bit meets no non-diagonal gate: the idle padding of 4 qubits, and diag11
    assert ("[zero-fill]" in text) == (name == "diag11" or s.n < 10), name
    assert ("[basis tile only]" in text) != ("[zero-fill]" in text), name
  for n in (4, 11, 13, 14):
    for name in ("wide3", "wide65"):
      ops = L.op_list(name, n)
      assert all(bin(x).count("1") >= 2 for op in ops for _, x, _ in op)
      assert len({(x, z) for op in ops for _, x, z in op}) == sum(len(op) for op in ops)
    assert len(L.op_list("wide65", n)) == 65 and all(len(op) == 1 for op in L.op_list("wide65", n))
  shards = L.op_list("shards", 11)
  assert len(shards) >= 32 and all(x == 0 for op in shards for _, x, _ in op)
  assert L.op_list("xxz", 11, 20)[0][0][0] == 2.0 ** 20 * L.op_list("xxz", 11)[0][0][0]
  for name in L.SESSION_NAMES:
    last = None
    for _, step, _, _, _, _ in _walk(name):
      if step[0] == "set_observables":
        assert last is None or abs(step[2] - last) == 20, (name, step)
        last = step[2]
  kinds = {g[0] for g in L.circuit("rand11")[1]}
  assert kinds == set(range(12)), kinds


@pytest.mark.parametrize("name", L.SESSION_NAMES)
def test_claimed_plan_changes_are_plan_changes(name):
  checked = 0
  for i, step, before, after, changed, _ in _walk(name):
    if step[0] == "call" or before.circuit is None:
      continue
    claims = step[0] in ("set_circuit", "set_observables") or (step[0] == "set_option" and step[3] is True)
    if step[0] == "set_gradient_mask":
      claims = changed
    if not claims:
      continue
    assert changed, (i, step)
    assert _plan(before) != _plan(after), f"step {i} {step}: the schedule is the one it was"
    checked += 1
  assert checked >= 1, checked


def test_option_flips_cover_the_options_of_the_issue():
  flipped = {o[0] for o in L.OPTION_FLIPS}
  assert flipped == {"tile_qubits", "adjoint_tile_qubits", "adjoint_exchange", "observable_kernel",
                     "values_from_observable", "chunk_states", "workspace_budget_mb", "shift_prefix_sharing"}
  # the lean non-exchange adjoint runs at K = 10 and at K = 11
  tiles = set()
  for _, step, before, _, _, _ in _walk("option flips"):
    if step[0] == "call" and step[1] == "vjp_adjoint" and before.options.get("adjoint_exchange", 1) == 0:
      tiles.add(before.options["adjoint_tile_qubits"])
      assert "adjoint plan" in _plan(before)[1] and "relabeling" not in _plan(before)[1]
  assert tiles == {10, 11}, tiles
  # the small budget cuts the batch at 14 qubits into several backward chunks
  for _, step, before, _, _, _ in _walk("option flips"):
    if step[0] == "call" and before.options.get("workspace_budget_mb"):
      eng = before.configure(E.Engine(device=None))
      one, all_ = eng.workspace_bytes(1, True), eng.workspace_bytes(step[2], True)
      state = 2 * 8 << before.n
      assert before.n == 14 and (all_ - one) < (step[2] - 1) * state / 2, (one, all_)


def _corner(a, b):
  """The leading corner two arrays of one rank share."""
  idx = tuple(slice(0, min(x, y)) for x, y in zip(a.shape, b.shape))
  return a[idx], b[idx], idx


@pytest.mark.parametrize("name", L.SESSION_NAMES)
def test_a_stale_answer_is_100_tolerances_away(name):
  """Consecutive calls of one kind: every output of the later one differs from the earlier one's -- on the corner
  they share, whatever the shapes -- by at least 100 times the tolerance the GPU module applies to it.  Shot counts,
  whose bar there is 2e-3 of the shots moved (each counted twice), must differ in a fifth of the shots."""
  last = {}
  compared = 0
  for i, step, before, _, _, inp in _walk(name):
    if step[0] != "call":
      continue
    kind = step[1]
    for label, want, tol in L.oracle(before, inp, kind):
      # the answer a stale engine would give: the last one of the same entry point, and the last one of the same
      # quantity from whichever entry point (values, grad, ...)
      for key in ((kind, label), label):
        if key in last and want.size and last[key][1].size:
          j, old = last[key]
          a, b, idx = _corner(want, old)
          assert a.size, (i, j, label)
          diff = np.abs(a - b)
          if tol is None:
            assert diff.sum(-1).min() >= 100 * 2e-3 * L.N_SHOTS, (i, j, label, diff.sum(-1))
          else:
            t = np.broadcast_to(np.asarray(tol, np.float64), want.shape)[idx] if np.ndim(tol) else tol
            far = float((diff / t).max())
            assert far >= 100.0, f"steps {j} and {i} ({kind}, {label}): {far:.3g} tolerances apart"
          compared += 1
        if want.size:  # (no states: there is nothing a stale answer could be mistaken for)
          last[key] = (i, want)
  assert compared >= 3, compared


def test_refusal_sequences_stay_inside_owned_memory():
  """No event of the consumer contract leads to a configuration with more gradient slots, parameters or workspace than
  the one the producer ran in."""
  base = L.Shadow()
  for i, s in enumerate(L.REFUSAL_BASE):
    base.apply(i, s)
  eng = base.configure(E.Engine(device=None))
  slots = L.adjoint_slots(eng.describe_schedule())
  work = eng.workspace_bytes(L.REFUSAL_U, True)
  assert slots > 0
  for event in L.SETTER_EVENTS + L.NO_CHANGE_EVENTS:
    after = base.copy()
    after.apply(len(L.REFUSAL_BASE), event)
    e2 = after.configure(E.Engine(device=None))
    assert after.n == base.n and after.n_params <= base.n_params, event
    assert L.adjoint_slots(e2.describe_schedule()) <= slots, (event, L.adjoint_slots(e2.describe_schedule()), slots)
    assert e2.workspace_bytes(L.REFUSAL_U, True) <= work, (event, e2.workspace_bytes(L.REFUSAL_U, True), work)
    if event[0] == "set_option" and event[3] is False:   # an option at the value it has: the very same schedule
      assert e2.describe_schedule() == eng.describe_schedule(), event
    elif event in L.SETTER_EVENTS and event != ("set_circuit", "hea11x2"):
      assert after.key() != base.key(), event
  planning = {name for name, _ in L.PLANNING_OPTIONS}
  assert planning == {e[1] for e in L.SETTER_EVENTS if e[0] == "set_option"}
  # every option whose setter invalidates the plans (the planner builds another schedule for SOME value of it), and
  # each at the value a new engine under BASE_OPTIONS has
  assert all(L.BASE_OPTIONS.get(name, value) == value for name, value in L.PLANNING_OPTIONS)
  # one slot per parameter in the base: a row is then ONE rounded product (test_rows_outlive_a_forward_only_call)
  assert slots == base.n_params
  for event in L.NO_CHANGE_EVENTS:
    after = base.copy()
    assert not after.apply(len(L.REFUSAL_BASE), event), event
  assert set(L.CALL_EVENTS_ROWS) <= set(L.CALL_EVENTS_STATES) <= set(L.KINDS)


@pytest.mark.parametrize("seed", L.WALK_SEEDS)
def test_random_walks_are_complete(seed):
  steps = L.sessions()[f"random walk {seed}"]["steps"]
  calls = [i for i, s in enumerate(steps) if s[0] == "call"]
  assert {steps[i][1] for i in calls} == set(L.KINDS)
  between = {s[0] for s in steps[calls[0]:calls[-1]] if s[0] != "call"}
  assert between == {"set_circuit", "set_observables", "set_gradient_mask", "set_option"}, between
  assert {0, 1, 2} <= {steps[i][2] for i in calls}


def test_retention_is_claimed_both_ways():
  """The sessions hold retaining forwards that must keep their states and ones that must not (a chunk size below the
  batch): engine_call asserts either, so a retain that never keeps anything cannot pass for the documented fall-back."""
  seen = set()
  for name in L.SESSION_NAMES:
    for _, step, before, _, _, _ in _walk(name):
      if step[0] == "call" and step[1] in ("retained", "table_retained"):
        seen.add((step[1], before.retains(step[2])))
  assert {("retained", True), ("table_retained", True)} <= seen and False in {r for _, r in seen}, seen
  assert None not in {r for _, r in seen}, seen   # (no session leaves the question open)


def test_random_walks_grow_and_shrink_the_batch():
  sizes = [s[2] for seed in L.WALK_SEEDS for s in L.sessions()[f"random walk {seed}"]["steps"] if s[0] == "call"]
  assert {0, 1, 2, 3, 9, 33} <= set(sizes), sorted(set(sizes))


def test_scripted_sessions_hold_what_the_issue_lists():
  w = {name: _walk(name) for name in L.SESSION_NAMES}
  sizes = [b.n for _, s, _, b, _, _ in w["shrink-and-grow"] if s[0] == "set_circuit"]
  assert sizes == [14, 4, 13, 11]
  # same-n swap: a circuit of the same size arrives and the observables are NOT installed again
  swaps = [(i, s) for i, s, before, after, _, _ in w["same-n circuit swap"]
           if s[0] == "set_circuit" and before.circuit and after.ops]
  assert len(swaps) >= 3
  for i, _ in swaps:
    assert w["same-n circuit swap"][i + 1][1][0] == "call"
  lists = [s[1] for _, s, _, _, _, _ in w["observable swap"] if s[0] == "set_observables"]
  assert lists == ["xxz", "wide65", "wide3", "shards", "xxz"]
  masks = [(i, s[1], b) for i, s, _, b, _, _ in w["mask walk"] if s[0] == "set_gradient_mask"]
  assert len({k for _, k, _ in masks[:5]}) == 5 and len({b.circuit for _, _, b in masks[:5]}) == 1
  # ... then a circuit with other gates, and the FIRST mask again: the same vector, element for element, as the one
  # whose plan for the old circuit the four-entry cache still holds (masks 1 to 4 pushed out the all-live plan alone)
  (i0, k0, old), (i5, k5, new) = masks[0], masks[5]
  assert k5 == k0 and w["mask walk"][i5 - 1][1] == ("set_circuit", L.MASK_TWIN)
  assert old.n == new.n and old.n_params == new.n_params and old.gates != new.gates
  assert old.mask_array().shape == new.mask_array().shape and (old.mask_array() == new.mask_array()).all()
  assert w["mask walk"][i5 + 1][1][:2] == ("call", "vjp_adjoint")
  # the old circuit's plan under that mask gives another gradient altogether: the parameters are numbered backwards
  assert sorted(g[3] for g in old.gates) == sorted(g[3] for g in new.gates)
  assert all(a[:3] == b[:3] and a[3] == old.n_params - 1 - b[3] for a, b in zip(old.gates, new.gates))
  for order in (w["entry-point interleave"][2:14], w["entry-point interleave"][14:]):
    assert {s[1] for _, s, _, _, _, _ in order} == set(L.KINDS)
  assert [s[1] for _, s, _, _, _, _ in w["entry-point interleave"][2:14]] != \
         [s[1] for _, s, _, _, _, _ in w["entry-point interleave"][14:]]
