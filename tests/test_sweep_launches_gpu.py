"""How many kernels every circuit entry point of the engine launches per chunk of states, and that cutting a batch
into chunks changes no bit of any output (GPU only).

Every entry point runs a batch of 5 states twice on one engine: with `chunk_states` = 2 (chunks of 2, 2 and 1) and with
`chunk_states` = 0 (one chunk: `workspace_budget_mb` is set, so the chunk size does not follow the free memory).  The
engine counts its launches on state-sized data when `profile_events` is on (`kernel_time_ms`): forward launches (the
passes; a from-states call adds the import of its chunk), backward launches (the adjoint passes) and observable
launches (lambda = O psi, the values, the energy table, the cotangent import).  The expected counts are
(chunks) x (launches per chunk), derived here from `describe_schedule` / `describe_schedule_from_states` / `num_passes`
and the way the values are taken:

  F   forward passes, Fg of them not measurement-only, B backward passes (basis-state or dense-start plans)
  lean    the values come from the observable kernel (one observable: value mode; several: multi-value mode) --
          `describe_schedule` names the kernel -- and the passes skip every measurement: Fg launches, else F
  forward-only calls take them that way only when it is cheaper (several observables: always; one: a term that
          flips two qubits or a measurement-only pass, and a plan of more than one pass)

A retaining call keeps the batch only when it fits one backward chunk: under `chunk_states` = 2 it keeps nothing and
runs as the plain call does, and the retained VJPs are refused.
"""
import re

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E

pytestmark = pytest.mark.gpu

U = 5
CHUNK = 2
CHUNKS = 3  # 2, 2, 1


def _ops(name, n):
  if name == "xxz":
    return [O.xxz_chain_op(n)]
  if name == "tfim":
    return [O.tfim_ring_op(n)]
  return [O.xxz_chain_op(n), O.tfim_ring_op(n), O.random_pauli_op(n, 6, 3)]


# name: (qubits, observables, options)
CASES = {
    "a_xxz11_value_mode": (11, "xxz", {}),
    "b_xxz11_measured": (11, "xxz", {"values_from_observable": 0}),
    "c_three12_multi": (12, "three", {"multi_observable_values": 1}),
    "c_three12_gather_multi": (12, "three", {"multi_observable_values": 1, "gather_multi_values": 1}),
    "d_tfim11": (11, "tfim", {}),
    "e_xxz8_padded": (8, "xxz", {}),
}


class _Setup:
  """One engine per case, its inputs, and what its schedules say."""

  def __init__(self, name):
    self.n, ops_name, options = CASES[name]
    n = self.n
    rng = np.random.default_rng(11)
    gates, names = O.hea_gates(n, 2, "sweep")
    self.params = rng.uniform(-1, 1, len(names)).astype(np.float32)
    self.ops = _ops(ops_name, n)
    self.bits = rng.integers(0, 2, size=(U, n)).astype(np.int8)
    self.up = rng.normal(size=(U, len(self.ops))).astype(np.float32)
    self.table = torch.as_tensor(rng.normal(size=1 << n).astype(np.float32))
    self.table_up = rng.normal(size=U).astype(np.float32)
    self.states = E.random_states(U, n, 7)
    self.cot = E.random_states(U, n, 8)
    eng = E.Engine(0)
    eng.set_option("profile_events", 1)
    eng.set_option("workspace_budget_mb", 256)
    eng.set_option("tile_qubits", 10)
    eng.set_option("adjoint_tile_qubits", 10)
    for key, value in options.items():
      eng.set_option(key, value)
    eng.set_circuit(n, gates, len(names))
    eng.set_observables(self.ops)
    self.eng = eng
    text = eng.describe_schedule()
    self.basis = self._plan(text)
    self.dense = self._plan(eng.describe_schedule_from_states())
    assert (self.basis["F"], self.basis["B"]) == eng.num_passes()
    values = re.search(r"observable kernel: lambda = \S+ values = (.*)", text).group(1)
    self.lean = values != "measured in the passes"  # value mode or multi-value mode
    self.gather_multi = values.startswith("apply_observable_kernel (an accumulator")
    self.one_op = len(self.ops) == 1
    self.wide_terms = any(bin(x).count("1") >= 2 for op in self.ops for _, x, _ in op)
    print(f"{name}: forward passes {self.basis['F']} ({self.basis['Fg']} with gates), backward {self.basis['B']}; "
          f"dense-start {self.dense['F']} ({self.dense['Fg']}), {self.dense['B']}; values = {values}")

  @staticmethod
  def _plan(text):
    fwd, adj = re.split(r"^adjoint[^\n]* plan:", text, maxsplit=1, flags=re.M)
    f = int(re.search(r"forward plan:.* passes=(\d+)", fwd).group(1))
    b = int(re.search(r" passes=(\d+)", adj).group(1))
    fm = len(re.findall(r"^  pass \d+:.*\[measure-only\]", fwd, flags=re.M))
    return {"F": f, "Fg": f - fm, "Fm": fm, "B": b}

  def forward_only_from_observable(self, plan):
    """Does a forward-only call on `plan` take its values from the observable kernel after lean passes?"""
    if not self.lean:
      return False
    if not self.one_op:
      return True
    return (self.wide_terms or plan["Fm"] > 0) and plan["F"] > 1


def _counts(eng):
  t = eng.kernel_time_ms()
  return t["fwd_launches"], t["bwd_launches"], t["obs_launches"]


def _run(s, chunk, call):
  """`call()` under `chunk_states` = chunk: (outputs, (forward, backward, observable) launches)."""
  s.eng.set_option("chunk_states", chunk)
  torch.cuda.synchronize()
  s.eng.kernel_time_ms()
  out = call()
  torch.cuda.synchronize()
  return out, _counts(s.eng)


def _tensors(out):
  if out is None:
    return []
  if torch.is_tensor(out):
    return [out]
  return [t for o in out for t in _tensors(o)]


def _check(s, what, call, per_chunk, chunked_per_chunk=None):
  """Both chunkings of `call`: launch counts = chunks x per_chunk (forward, backward, observable), equal outputs.
  `chunked_per_chunk`: a retaining call, which under chunking keeps nothing and runs as the plain call -- its outputs
  are compared by the caller, with the plain call's."""
  whole, got_whole = _run(s, 0, call)
  parts, got_parts = _run(s, CHUNK, call)
  want_whole = tuple(per_chunk)
  want_parts = tuple(CHUNKS * k for k in (chunked_per_chunk or per_chunk))
  print(f"  {what}: one chunk {got_whole} (derived {want_whole}), {CHUNKS} chunks {got_parts} (derived {want_parts})")
  assert got_whole == want_whole, what
  assert got_parts == want_parts, what
  a, b = _tensors(whole), _tensors(parts)
  assert len(a) == len(b) and a
  if chunked_per_chunk is not None:
    return whole, parts
  for x, y in zip(a, b):
    assert torch.equal(x, y), what
  return whole


@pytest.mark.parametrize("name", sorted(CASES))
def test_launches_per_chunk_and_chunking_is_exact(name):
  s = _Setup(name)
  eng, ba, de = s.eng, s.basis, s.dense
  lean_f = ba["Fg"] if s.lean else ba["F"]          # forward launches of a chunk whose values the observable kernel takes
  lean_fd = (de["Fg"] if s.lean else de["F"]) + 1   # ... from caller states: the import first
  # lambda = O psi and the values of one chunk of an adjoint VJP: several observables on the block kernel take the values
  # in a launch of their own
  obs_vjp = 2 if (s.lean and not s.one_op and not s.gather_multi) else 1

  # ---- expectation values -------------------------------------------------------------------------------------------------
  fo = s.forward_only_from_observable(ba)
  plain = (ba["Fg"] if fo else ba["F"], 0, 1 if fo else 0)
  vals = _check(s, "expectation", lambda: eng.expectation(s.bits, s.params), plain)
  kept = (lean_f, 0, 1 if s.lean else 0)
  kept_vals, unkept_vals = _check(s, "expectation(retain)", lambda: eng.expectation(s.bits, s.params, retain=True), kept, plain)
  assert eng.retained is None and eng.retained_states() == 0  # (the chunked call came last: nothing kept)
  assert torch.equal(unkept_vals, vals)
  assert fo != s.lean or torch.equal(kept_vals, vals)  # (the same bits where both take the values the same way)

  # ---- adjoint VJPs -------------------------------------------------------------------------------------------------------
  adjoint = (lean_f, ba["B"], obs_vjp)
  v, grad = _check(s, "expectation_vjp", lambda: eng.expectation_vjp(s.bits, s.params, s.up), adjoint)
  assert torch.equal(v, kept_vals)  # (a retaining forward takes the values as the adjoint VJP does)
  assert eng.state_gradients(U).shape == (U, len(s.params))  # (the rows of the last adjoint VJP are served)

  eng.set_option("chunk_states", 0)
  eng.expectation(s.bits, s.params, retain=True)
  assert eng.retained is not None
  torch.cuda.synchronize()
  eng.kernel_time_ms()
  grad_kept = eng.expectation_vjp_retained(s.bits, s.params, s.up)
  torch.cuda.synchronize()
  got = _counts(eng)
  want = (0, ba["B"], 0 if (s.lean and s.one_op) else 1)  # value mode kept lambda = O psi beside psi
  print(f"  expectation_vjp_retained: {got} (derived {want})")
  assert got == want
  # (the same launches as the adjoint VJP's, so the same bits -- except where that VJP took lambda from the gather kernel's
  # launch with an accumulator per observable, which the retained one never runs)
  assert s.gather_multi or torch.equal(grad_kept, grad)
  eng.set_option("chunk_states", CHUNK)
  eng.expectation(s.bits, s.params, retain=True)
  with pytest.raises(E.EngineError, match="no retained forward state"):
    eng.expectation_vjp_retained(s.bits, s.params, s.up)

  # ---- caller-supplied start states ---------------------------------------------------------------------------------------
  fod = s.forward_only_from_observable(de)
  _check(s, "expectation_from_states", lambda: eng.expectation_from_states(s.states, s.params),
         ((de["Fg"] if fod else de["F"]) + 1, 0, 1 if fod else 0))
  _check(s, "expectation_vjp_from_states", lambda: eng.expectation_vjp_from_states(s.states, s.params, s.up),
         (lean_fd, de["B"], obs_vjp))

  # ---- final states -------------------------------------------------------------------------------------------------------
  _check(s, "statevector", lambda: eng.statevector(s.bits, s.params), (ba["F"], 0, 0))
  _check(s, "statevector_from_states", lambda: eng.statevector_from_states(s.states, s.params), (de["F"] + 1, 0, 0))
  _check(s, "statevector_vjp_from_states",
         lambda: eng.statevector_vjp_from_states(s.states, s.params, s.cot, want_states=True), (de["Fg"] + 1, de["B"], 1))
  with pytest.raises(E.EngineError, match="qhbm_state_gradients"):
    eng.state_gradients(U)

  # ---- energy tables: lean passes, the table kernel counts as the observable launch ----------------------------------------
  table = (ba["Fg"], 0, 1)
  tv = _check(s, "table_expectation", lambda: eng.table_expectation(s.bits, s.params, s.table), table)
  tk, tu = _check(s, "table_expectation(retain)", lambda: eng.table_expectation(s.bits, s.params, s.table, retain=True),
                  table, table)
  assert torch.equal(tk, tv) and torch.equal(tu, tv)
  _, tgrad, ttab = _check(s, "table_expectation_vjp",
                          lambda: eng.table_expectation_vjp(s.bits, s.params, s.table, s.table_up), (ba["Fg"], ba["B"], 1))
  eng.set_option("chunk_states", 0)
  eng.table_expectation(s.bits, s.params, s.table, retain=True)
  assert eng.retained is not None
  torch.cuda.synchronize()
  eng.kernel_time_ms()
  kept_grad, kept_tab = eng.table_expectation_vjp_retained(s.bits, s.params, s.table, s.table_up)
  torch.cuda.synchronize()
  got = _counts(eng)
  print(f"  table_expectation_vjp_retained: {got} (derived {(0, ba['B'], 1)})")
  assert got == (0, ba["B"], 1)
  assert torch.equal(kept_grad, tgrad) and torch.equal(kept_tab, ttab)

  # ---- sampling: its launches follow the forward passes; the shots must not depend on the chunking -------------------------
  eng.set_option("chunk_states", 0)
  whole = eng.sample(s.bits, s.params, 64, seed=5)
  eng.set_option("chunk_states", CHUNK)
  parts = eng.sample(s.bits, s.params, 64, seed=5)
  assert torch.equal(whole, parts)
