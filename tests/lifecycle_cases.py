"""Sessions on ONE live engine, a shadow of the configuration it ought to be in, and the complex128 oracle of every
compute step (tests/test_lifecycle_cases_cpu.py, tests/test_engine_lifecycle_gpu.py).  Nothing here creates an engine
or needs a GPU: `Shadow.configure`, `apply_setter` and `engine_call` drive the engine a test hands them.

A session is a list of steps:

  ("set_circuit", name)                        a circuit of CIRCUITS
  ("set_observables", name, e)                 the list OP_LISTS[name] of the circuit's size, every coefficient times 2^e
  ("set_gradient_mask", k)                     mask number k of the installed circuit (None: every parameter live)
  ("set_option", option, value, plan)          plan: the session claims that the schedule changes
  ("call", kind, U)                            one compute entry point (KINDS) on U states

The inputs of a call are drawn from (the session's seed, the step's index), so that two calls never share them.
`Shadow` follows the setters; from it a test configures a fresh engine (`Shadow.configure`) and asks `oracle` for the
expected outputs and the tolerance of each.

Sizes are the smallest at which a mechanism exists under tile_qubits = adjoint_tile_qubits = 10: 4 qubits are padded
with idle qubits up to the 2^10 tile, 11 to 14 take several passes, `diag11` has a diagonal-only qubit (its forward
plan zero-fills in the first pass), `rand11` holds every gate kind.
"""
import functools
import re

import numpy as np

from oracle import qhbm_oracle as O
from tests import energy_table_ref as T
from tests import spectator_cases as S
from tests.test_engine_gpu import random_circuit
from tests.test_sampling_exact_gpu import Ref, _restated_counts

# the options every session starts from: the small tiles, and the engine's own defaults of the options that get flipped
BASE_OPTIONS = {"tile_qubits": 10, "adjoint_tile_qubits": 10, "adjoint_exchange": 1, "adjoint_stop_early": -1,
                "observable_kernel": -1, "values_from_observable": 1, "chunk_states": 0, "workspace_budget_mb": 0,
                "shift_prefix_sharing": 1}
N_SHOTS = 4099

KINDS = ("expectation", "retained", "vjp_adjoint", "vjp_shift", "jacobian", "state_gradients", "statevector",
         "sample_counts", "program_vjps", "table_expectation", "table_vjp", "table_retained")
# calls that need no installed observables (include/qhbm_engine.h)
NO_OBSERVABLES = ("statevector", "sample_counts", "table_expectation", "table_vjp", "table_retained")
# calls after which qhbm_state_gradients serves rows
ROW_PRODUCERS = ("vjp_adjoint", "retained")


# ---- ingredients ------------------------------------------------------------------------------------------------------
def _rand_gates(n, n_gates, n_params, seed):
  """Every gate kind; ISWAP powers keep a constant exponent (no two-term shift rule exists for them)."""
  gates = random_circuit(np.random.default_rng(seed), n, n_gates, n_params)
  return [g if g[0] != O.GATE_ISWAPPOW else (g[0], g[1], g[2], -1, 0.0, g[5] + g[4] * 0.3) for g in gates]


@functools.lru_cache(maxsize=None)
def circuit(name):
  """(n, gates, n_params).  The parameter counts of CIRCUITS all differ; MASK_TWIN is the one circuit that shares its
  count, with hea11x2, so that one and the same mask vector fits both."""
  if name == "hea11x2r":   # the gates of hea11x2, the parameters numbered backwards
    n, gates, P = circuit("hea11x2")
    return n, tuple(g if g[3] < 0 else g[:3] + (P - 1 - g[3],) + g[4:] for g in gates), P
  if name.startswith("hea"):
    n, layers = {"hea4": (4, 2), "hea11": (11, 1), "hea11x2": (11, 2), "hea13": (13, 1), "hea14": (14, 1)}[name]
    gates, names = O.hea_gates(n, layers, name)
    return n, tuple(gates), len(names)
  if name == "diag11":
    gates, n_params, roles, _ = S.spectator_circuit(11, "diag", seed=5, layers=3, extra=8)
    assert list(roles.values()) == ["diag"]
    return 11, tuple(gates), n_params
  if name == "rand11":
    return 11, tuple(_rand_gates(11, 48, 7, seed=11)), 7
  if name == "rand4":
    return 4, tuple(_rand_gates(4, 24, 5, seed=4)), 5
  raise KeyError(name)


CIRCUITS = ("hea4", "rand4", "hea11", "hea11x2", "diag11", "rand11", "hea13", "hea14")
MASK_TWIN = "hea11x2r"


def _wide_terms(n):
  """Single Pauli strings that flip two qubits (XX, XY, YX, YY on a pair, Z on up to two others), without repeats."""
  out = []
  for d in range(1, n):
    for q in range(n - d):
      for ya, yb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        for zs in range(4):
          x = (1 << q) | (1 << (q + d))
          z = (ya << q) | (yb << (q + d))
          others = [r for r in range(n) if r not in (q, q + d)]
          for i in range(2):
            if zs >> i & 1:
              z |= 1 << others[(q + i * 3) % len(others)]
          out.append((x, z))
  seen, uniq = set(), []
  for t in out:
    if t not in seen:
      seen.add(t)
      uniq.append(t)
  return uniq


@functools.lru_cache(maxsize=None)
def op_list(name, n, exponent=0):
  """The observable list `name` on n qubits with every coefficient times 2^exponent (exact in fp32).
    xxz     one XXZ chain                                        (value mode: the value comes with lambda = O psi)
    wide3   three operators of six terms that flip >= 2 qubits   (one launch of the block kernel for the values)
    wide65  65 single-term operators that flip 2 qubits          (one past the limit of that path: measured in passes)
    shards  the KOBE-2 Z strings, one operator each, >= 32 terms (Walsh-Hadamard measurement; n >= 8)"""
  rng = np.random.default_rng(1000 + n)
  scale = 2.0 ** exponent
  if name == "xxz":
    ops = [O.xxz_chain_op(n)]
  elif name == "wide3":
    terms = _wide_terms(n)
    picks = rng.choice(len(terms), size=18, replace=False)
    ops = [[(float(np.float32(rng.uniform(0.5, 1.5) * rng.choice([-1, 1]))),) + terms[i] for i in picks[6 * k:6 * k + 6]]
           for k in range(3)]
  elif name == "wide65":
    terms = _wide_terms(n)
    picks = rng.choice(len(terms), size=65, replace=False)
    ops = [[(float(np.float32(rng.uniform(0.5, 1.5) * rng.choice([-1, 1]))),) + terms[i]] for i in picks]
  elif name == "shards":
    ops = O.kobe_shards(n, 2)
  else:
    raise KeyError(name)
  return tuple(tuple((c * scale, x, z) for c, x, z in op) for op in ops)


OP_LISTS = ("xxz", "wide3", "wide65", "shards")


def mask(k, n_params):
  """Mask number k (needs_grad per parameter): a random 60 % live, never all and never none; None = all live."""
  if k is None:
    return None
  m = np.random.default_rng(7000 + 31 * k + n_params).random(n_params) < 0.6
  m[k % n_params] = True
  m[(k + 1) % n_params] = False
  return m


# ---- the shadow -------------------------------------------------------------------------------------------------------
class Shadow:
  """What the engine ought to hold after the steps applied so far."""

  def __init__(self):
    self.options = dict(BASE_OPTIONS)
    self.circuit = None     # name
    self.ops = None         # (name, exponent); None: not installed (never, or dropped by a circuit of another size)
    self.mask = None        # mask number
    self.rows_from = None   # index of the adjoint VJP whose rows qhbm_state_gradients serves

  def copy(self):
    c = Shadow()
    c.options, c.circuit, c.ops, c.mask, c.rows_from = dict(self.options), self.circuit, self.ops, self.mask, self.rows_from
    return c

  @property
  def n(self):
    return circuit(self.circuit)[0]

  @property
  def gates(self):
    return list(circuit(self.circuit)[1])

  @property
  def n_params(self):
    return circuit(self.circuit)[2]

  def op_list(self):
    return [list(op) for op in op_list(self.ops[0], self.n, self.ops[1])] if self.ops else []

  def mask_array(self):
    return mask(self.mask, self.n_params)

  def key(self):
    return (tuple(sorted(self.options.items())), self.circuit, self.ops, self.mask)

  def retains(self, U):
    """Whether a retaining forward on U states keeps them (include/qhbm_engine.h: the batch must fit ONE backward
    chunk, psi and lambda side by side).  None: no claim -- a budget is set and the engine chooses the tile itself."""
    if U <= 0:
      return False
    if self.options["chunk_states"] > 0:
      return self.options["chunk_states"] >= U
    if self.options["workspace_budget_mb"] > 0:
      if self.options["tile_qubits"] <= 0:
        return None
      state = 8 << max(self.n, self.options["tile_qubits"])
      return max(1, (self.options["workspace_budget_mb"] << 20) // (2 * state)) >= U
    return True   # (the default budget is 64 MiB at the very least: 256 states of 2^14 amplitudes with their lambda)

  def apply(self, index, step):
    """Follows one step.  Returns True if a setter changed the configuration."""
    kind = step[0]
    before = self.key()
    if kind == "set_circuit":
      old_n = self.n if self.circuit else None
      self.circuit = step[1]
      if old_n != self.n:
        self.ops = None     # observables survive a new circuit iff the size is unchanged
      self.mask = None      # the mask never does
      self.rows_from = None  # (a re-installed circuit rebuilds the plans even when it is the same one)
      return True
    if kind == "set_observables":
      self.ops = (step[1], step[2])
      self.rows_from = None
      return True
    if kind == "set_gradient_mask":
      self.mask = step[1]
    elif kind == "set_option":
      self.options[step[1]] = step[2]
    elif kind == "call":
      if step[1] in ROW_PRODUCERS:
        self.rows_from = index if step[2] > 0 else None
      elif step[1] not in ("expectation", "state_gradients"):
        self.rows_from = None
      return False
    changed = self.key() != before
    if changed:
      self.rows_from = None
    return changed

  def configure(self, eng):
    """Brings a NEW engine straight into this configuration: options, circuit, observables, mask."""
    for k, v in self.options.items():
      eng.set_option(k, v)
    eng.set_circuit(self.n, self.gates, self.n_params)
    if self.ops:
      eng.set_observables(self.op_list())
    if self.mask is not None:
      eng.set_gradient_mask(self.mask_array())
    return eng


def apply_setter(eng, shadow_after, step):
  """The setter `step` on a live engine (`shadow_after`: the shadow once the step is applied)."""
  kind = step[0]
  if kind == "set_circuit":
    n, gates, n_params = circuit(step[1])
    eng.set_circuit(n, list(gates), n_params)
  elif kind == "set_observables":
    eng.set_observables(shadow_after.op_list())
  elif kind == "set_gradient_mask":
    eng.set_gradient_mask(shadow_after.mask_array())
  elif kind == "set_option":
    eng.set_option(step[1], step[2])
  else:
    raise ValueError(step)


# ---- inputs and oracle ------------------------------------------------------------------------------------------------
class Inputs:
  """What one call is given.  Everything is rounded to fp32 first, so the oracle sees what the engine sees."""

  def __init__(self, seed, index, shadow, kind, U):
    rng = np.random.default_rng([seed, index])
    n, P, T_ = shadow.n, shadow.n_params, len(shadow.op_list())
    self.kind, self.U = kind, U
    self.bits = rng.integers(0, 2, size=(U, n)).astype(np.int8)
    self.params = rng.uniform(-1, 1, P).astype(np.float32)
    self.upstream = rng.normal(size=(U, T_)).astype(np.float32)
    self.table = self.table_upstream = self.weights = self.shift_gates = self.shifts = None
    if kind.startswith("table"):
      self.table = T.random_table(n, rng)
      self.table_upstream = rng.normal(size=U).astype(np.float32)
    if kind in ("sample_counts", "program_vjps"):
      shiftable = [i for i, g in enumerate(shadow.gates) if g[3] >= 0 and g[0] != O.GATE_ISWAPPOW]
      g = int(rng.choice(shiftable))
      self.shift_gates, self.shifts = [-1, g, g], [0.0, 0.5, -0.5]
      self.weights = rng.uniform(0.5, 1.5, U).astype(np.float32)


def _kept(eng, retains, inp):
  """Whether the retaining forward kept its states; where the shadow says which (`retains`), that it did as it says."""
  kept = eng.retained is not None
  assert retains is None or kept == retains, \
      f"a retaining forward on {inp.U} states {'kept' if kept else 'did not keep'} them; the configuration says otherwise"
  return kept


def engine_call(eng, inp, kind=None, retains=None):
  """Runs the call on `eng`; a tuple of device tensors.  `retains`: Shadow.retains of the batch, for the retained kinds."""
  kind = kind or inp.kind
  b, p = inp.bits, inp.params
  if kind == "expectation":
    return (eng.expectation(b, p),)
  if kind == "retained":
    vals = eng.expectation(b, p, retain=True)
    if not _kept(eng, retains, inp):  # (the batch did not fit one backward chunk: the documented fall-back)
      return vals, eng.expectation_vjp(b, p, inp.upstream)[1]
    return vals, eng.expectation_vjp_retained(b, p, inp.upstream)
  if kind == "vjp_adjoint":
    return eng.expectation_vjp(b, p, inp.upstream)
  if kind == "vjp_shift":
    return eng.expectation_vjp(b, p, inp.upstream, 1)
  if kind == "jacobian":
    return eng.expectation_jacobian(b, p)
  if kind == "state_gradients":
    return (eng.state_gradients(inp.U),)
  if kind == "statevector":
    return (eng.statevector(b, p),)
  if kind == "sample_counts":
    from tests.test_sampling_exact_gpu import SEED  # pylint: disable=import-outside-toplevel
    return (eng.sample_counts(b, p, N_SHOTS, seed=SEED, shift_gates=inp.shift_gates, shifts=inp.shifts),)
  if kind == "program_vjps":
    return eng.program_vjps(b, p, inp.shift_gates, inp.shifts, inp.upstream, inp.weights)
  if kind == "table_expectation":
    return (eng.table_expectation(b, p, inp.table),)
  if kind == "table_vjp":
    return eng.table_expectation_vjp(b, p, inp.table, inp.table_upstream)
  if kind == "table_retained":
    vals = eng.table_expectation(b, p, inp.table, retain=True)
    if not _kept(eng, retains, inp):
      return eng.table_expectation_vjp(b, p, inp.table, inp.table_upstream)
    return (vals,) + tuple(eng.table_expectation_vjp_retained(b, p, inp.table, inp.table_upstream))
  raise KeyError(kind)


def _shifted(gates, gate, shift):
  if gate < 0:
    return gates
  g = gates[gate]
  return gates[:gate] + [tuple(g[:5]) + (g[5] + shift,) + tuple(g[6:])] + gates[gate + 1:]


def _value_rel(n):
  return 1e-5 if n <= 12 else 5e-5


def _grad_tol(want, rel=1e-4):
  return rel * max(1.0, float(np.abs(want).max()) if want.size else 0.0)


def oracle(shadow, inp, kind=None):
  """[(name, expected, tolerance)] of the call, one entry per output of `engine_call`, in complex128.  The bars are the
  suite's own (tests/test_engine_gpu.py, test_spectator_qubits_gpu.py, test_energy_table_gpu.py): values
  1e-5 sum|c| (n <= 12) or 5e-5 sum|c|, gradients / rows / Jacobians 1e-4 max(1, |.|_inf), the shift rule 3e-4, states
  5e-6, table values 2e-5 max|E|, table gradients 1e-5 sum|upstream| at most (see below).  `expected` of sample_counts is the restated
  histogram of the fp64 probabilities; its tolerance is None (the test derives it from the engine's own state, as
  tests/test_sampling_exact_gpu.py does)."""
  kind = kind or inp.kind
  n, gates, ops = shadow.n, shadow.gates, shadow.op_list()
  params = inp.params.astype(np.float64)
  live = shadow.mask_array()
  live = np.ones(shadow.n_params, bool) if live is None else live
  norm = S.op_norm(ops) if ops else np.zeros(0)
  vtol = (_value_rel(n) * norm)[None, :]
  up = inp.upstream.astype(np.float64)
  if kind == "statevector":
    want = np.stack([O.simulate(n, gates, params, list(b)).ravel() for b in inp.bits]) if inp.U else np.zeros((0, 1 << n))
    return [("states", want, 5e-6)]
  if kind == "sample_counts":
    want = np.zeros((len(inp.shift_gates), inp.U, 1 << n), np.int64)
    for q, (g, s) in enumerate(zip(inp.shift_gates, inp.shifts)):
      for r, b in enumerate(inp.bits):
        ref = Ref.dense(np.abs(O.simulate(n, _shifted(gates, g, s), params, list(b)).ravel()) ** 2)
        want[q, r] = _restated_counts(ref, N_SHOTS, r, q, 0.0, 1 << n)[0]
    return [("counts", want, None)]
  if kind.startswith("table"):
    vals, jac, probs = T.diag_vjp(n, gates, params, inp.bits, inp.table)
    tup = inp.table_upstream.astype(np.float64)
    out = [("table values", vals, 2e-5 * float(np.abs(inp.table).max()))]
    if kind != "table_expectation":
      grad = (tup @ jac) * live
      # table_grad[y] = sum_u up_u |psi_u(y)|^2.  An amplitude within the states' bar d = 5e-6 moves |psi|^2 by at most
      # 2 |psi| d + d^2, and the fp32 result rounds once more: never looser than the 1e-5 sum|up| of
      # tests/test_energy_table_gpu.py, and tight enough at small probabilities to tell one table gradient from another
      tg_tol = np.abs(tup) @ (1e-5 * np.sqrt(probs) + 2.5e-11) + 2.0 ** -23 * (np.abs(tup) @ probs)
      tg_tol = np.minimum(tg_tol, 1e-5 * float(np.abs(tup).sum()))
      out += [("table grad", grad, _grad_tol(grad)), ("table_grad", tup @ probs, tg_tol)]
    return out
  if kind == "program_vjps":
    w = inp.weights.astype(np.float64)
    pv, pg = [], []
    for g, s in zip(inp.shift_gates, inp.shifts):
      vals, jac, _ = S.stacked_jacobian(n, _shifted(gates, g, s), params, inp.bits, ops)
      pv.append(w @ vals)
      pg.append(np.einsum("ut,utp->p", up, jac) * live)
    pg = np.stack(pg)
    # a weighted sum of U values, each within the value bar: the weights' 1-norm times that bar
    return [("program values", np.stack(pv), vtol * float(np.abs(w).sum())), ("program gradients", pg, _grad_tol(pg))]
  vals, jac, _ = S.stacked_jacobian(n, gates, params, inp.bits, ops)
  jac = jac * live[None, None, :]
  if kind == "expectation":
    return [("values", vals, vtol)]
  if kind == "jacobian":
    return [("values", vals, vtol), ("jacobian", jac, _grad_tol(jac))]
  if kind == "state_gradients":
    rows = np.einsum("ut,utp->up", up, jac)
    return [("rows", rows, _grad_tol(rows))]
  grad = np.einsum("ut,utp->p", up, jac)
  return [("values", vals, vtol), ("grad", grad, _grad_tol(grad, 3e-4 if kind == "vjp_shift" else 1e-4))]


# ---- sessions ---------------------------------------------------------------------------------------------------------
def walk(case):
  """[(index, step, shadow before, shadow after, changed, inputs)] of a session: `changed` for setters (the
  configuration differs), `inputs` for calls.  A state_gradients call gets the inputs of the VJP whose rows it serves."""
  shadow, out, inputs = Shadow(), [], {}
  for i, step in enumerate(case["steps"]):
    before = shadow.copy()
    changed = shadow.apply(i, step)
    inp = None
    if step[0] == "call":
      if step[1] == "state_gradients":
        assert before.rows_from is not None, (case["name"], i, "state_gradients without rows to serve")
        inp = inputs[before.rows_from]
      else:
        assert before.ops or step[1] in NO_OBSERVABLES, (case["name"], i, step)
        inp = Inputs(case["seed"], i, before, step[1], step[2])
      inputs[i] = inp
    out.append((i, step, before, shadow.copy(), changed, inp))
  return out


def _c(kind, U):
  return ("call", kind, U)


def _after_circuit(name, ops, e, U):
  """set_circuit, a statevector on the bare circuit, the observables, then a forward, an adjoint VJP with its rows and a
  statevector."""
  return [("set_circuit", name), _c("statevector", 1), ("set_observables", ops, e), _c("expectation", U),
          _c("vjp_adjoint", U), _c("state_gradients", U), _c("statevector", U)]


def _shrink_and_grow():
  steps = (_after_circuit("hea14", "xxz", 0, 2) + _after_circuit("hea4", "wide3", 20, 9) +
           _after_circuit("hea13", "xxz", 0, 2) + _after_circuit("hea11", "wide3", 20, 33))
  return {"name": "shrink-and-grow", "seed": 101, "steps": steps}


def _same_n_swap():
  steps = [("set_circuit", "hea11"), ("set_observables", "wide3", 0), _c("expectation", 2), _c("vjp_adjoint", 2),
           ("set_circuit", "diag11"), _c("expectation", 9), _c("vjp_adjoint", 9), _c("state_gradients", 9),
           ("set_circuit", "rand11"), _c("retained", 2), _c("jacobian", 1), _c("vjp_shift", 2),
           ("set_circuit", "hea11x2"), _c("vjp_adjoint", 3), _c("expectation", 0), _c("expectation", 3)]
  return {"name": "same-n circuit swap", "seed": 102, "steps": steps}


def _observable_swap():
  steps = [("set_circuit", "hea11x2")]
  for ops, e, U in (("xxz", 0, 1), ("wide65", 20, 9), ("wide3", 0, 33), ("shards", 20, 2), ("xxz", 0, 2)):
    steps += [("set_observables", ops, e), _c("expectation", U), _c("vjp_adjoint", U), _c("state_gradients", U),
              _c("retained", min(U, 9))]
  return {"name": "observable swap", "seed": 103, "steps": steps}


# option -> (circuit, observables, the two values, whether the schedule changes, batch)
OPTION_FLIPS = (
    ("tile_qubits", "hea13", "xxz", (10, 0), True, 2),
    ("adjoint_tile_qubits", "hea13", "wide3", (10, 11), True, 2),
    ("adjoint_exchange", "hea13", "xxz", (1, 0), True, 2),
    ("adjoint_exchange", "hea13", "xxz", (1, 0), True, 3),          # ... at adjoint_tile_qubits = 11 (see _option_flips)
    ("observable_kernel", "hea13", "wide3", (0, 1), False, 2),      # (another kernel for the same plans)
    ("values_from_observable", "hea11", "xxz", (1, 0), False, 9),
    ("chunk_states", "hea11", "wide3", (0, 2), False, 9),
    ("workspace_budget_mb", "hea14", "xxz", (0, 1), False, 9),      # 1 MiB: four states of 2^14 amplitudes and lambda
    ("shift_prefix_sharing", "hea11", "xxz", (1, 0), False, 2),
)


def _option_flips():
  steps, circ_now, ops_now, exponent = [], None, None, 20
  for option, circ, ops, (a, b), plan, U in OPTION_FLIPS:
    if circ != circ_now:
      steps.append(("set_circuit", circ))
      if circ_now is None or circuit(circ)[0] != circuit(circ_now)[0]:
        ops_now = None
      circ_now = circ
    if ops != ops_now:
      exponent = 20 - exponent
      steps.append(("set_observables", ops, exponent))
      ops_now = ops
    kind = "vjp_shift" if option == "shift_prefix_sharing" else "vjp_adjoint"
    wide = option == "adjoint_exchange" and U == 3
    if wide:
      steps += [("set_option", "adjoint_tile_qubits", 11, True)]
    if BASE_OPTIONS[option] != a:   # (observable_kernel: the engine's default is -1, its own choice)
      steps += [("set_option", option, a, None)]
    steps += [_c(kind, U), ("set_option", option, b, plan), _c(kind, U), _c("expectation", U),
              ("set_option", option, a, plan), _c(kind, U)]
    if kind == "vjp_adjoint":
      steps += [_c("state_gradients", U)]
    if wide:
      steps += [("set_option", "adjoint_tile_qubits", 10, True)]
  return {"name": "option flips", "seed": 104, "steps": steps}


def _mask_walk():
  steps = [("set_circuit", "hea11x2"), ("set_observables", "xxz", 0)]
  # five masks: the fifth evicts the all-live plan from the four-entry cache, which then holds the plans of masks 0 to 3
  for k in (0, 1, 2, 3, 4):
    steps += [("set_gradient_mask", k), _c("vjp_adjoint", 2), _c("state_gradients", 2)]
  # a circuit with as many parameters and other gates, then the very vector of mask 0 again (mask() depends on the
  # parameter count alone): the cache still holds a plan under exactly that key, planned for the old circuit
  steps += [("set_circuit", MASK_TWIN), ("set_gradient_mask", 0), _c("vjp_adjoint", 2), _c("state_gradients", 2),
            ("set_gradient_mask", 4), _c("vjp_adjoint", 2), ("set_gradient_mask", 0), _c("vjp_adjoint", 2),
            _c("state_gradients", 2)]
  steps += [("set_circuit", "diag11"), ("set_gradient_mask", 0), _c("vjp_adjoint", 2), _c("state_gradients", 2),
            _c("vjp_shift", 1), ("set_gradient_mask", None), _c("vjp_adjoint", 2),
            ("set_gradient_mask", 0), _c("jacobian", 1), _c("program_vjps", 2), _c("table_vjp", 2)]
  return {"name": "mask walk", "seed": 105, "steps": steps}


def _interleave():
  first = ("expectation", "retained", "vjp_adjoint", "state_gradients", "vjp_shift", "jacobian", "statevector",
           "sample_counts", "program_vjps", "table_expectation", "table_vjp", "table_retained")
  second = ("table_retained", "sample_counts", "retained", "table_expectation", "vjp_adjoint", "expectation",
            "state_gradients", "program_vjps", "statevector", "vjp_shift", "table_vjp", "jacobian")
  steps = [("set_circuit", "rand11"), ("set_observables", "wide3", 0)]
  for order, sizes in ((first, (1, 9, 2)), (second, (2, 3, 1))):
    for j, kind in enumerate(order):
      steps.append(_c(kind, sizes[j % 3] if kind != "state_gradients" else 0))
  return {"name": "entry-point interleave", "seed": 106, "steps": _fix_row_sizes(steps)}


def _fix_row_sizes(steps):
  """state_gradients asks for as many rows as the VJP in front of it ran on."""
  out, last = [], 0
  for s in steps:
    if s[0] == "call" and s[1] in ROW_PRODUCERS:
      last = s[2]
    elif s[0] == "call" and s[1] == "state_gradients":
      s = _c("state_gradients", last)
    out.append(s)
  return out


WALK_STEPS = 25
WALK_SEEDS = (1, 2, 3, 4)
_WALK_CIRCUITS = ("hea4", "rand4", "hea11", "diag11", "rand11", "hea13", "hea14")
# (whether a flip changes the schedule depends on the circuit it meets: a walk claims nothing, plan = None)
_WALK_OPTIONS = (("tile_qubits", (10, 0)), ("adjoint_tile_qubits", (10, 11)), ("adjoint_exchange", (1, 0)),
                 ("observable_kernel", (0, 1)), ("values_from_observable", (1, 0)), ("chunk_states", (0, 2)),
                 ("shift_prefix_sharing", (1, 0)))


def random_walk(seed):
  """About WALK_STEPS steps drawn from the same ingredients: every entry point once (shuffled), a setter between any
  two of them -- one of each kind at least -- and batch sizes that grow and shrink.  The oracle is kept affordable: more
  than three states only up to 11 qubits and three observables; 65 observables and the shards only up to 11 qubits."""
  rng = np.random.default_rng(9000 + seed)
  shadow, steps = Shadow(), []

  def push(step):
    shadow.apply(len(steps), step)
    steps.append(step)

  push(("set_circuit", str(rng.choice(["hea11", "rand11", "hea13"]))))
  push(("set_observables", "xxz", 0))
  kinds = [k for k in KINDS if k != "state_gradients"]
  rng.shuffle(kinds)
  setters = ["set_circuit", "set_observables", "set_gradient_mask", "set_option"]
  setters += list(rng.choice(setters, size=len(kinds) - 1 - len(setters)))
  rng.shuffle(setters)
  sizes = [1, 9, 2, 0, 33]
  exponent = 0
  for j, kind in enumerate(kinds):
    setter = setters[j - 1] if j else None
    if setter == "set_circuit":
      push(("set_circuit", str(rng.choice([c for c in _WALK_CIRCUITS if c != shadow.circuit]))))
    elif setter == "set_gradient_mask":
      push(("set_gradient_mask", int(rng.choice([k for k in range(5) if k != shadow.mask]))))
    elif setter == "set_option":
      name, values = _WALK_OPTIONS[int(rng.integers(len(_WALK_OPTIONS)))]
      push(("set_option", name, values[1] if shadow.options.get(name, values[0]) == values[0] else values[0], None))
    if setter == "set_observables" or not shadow.ops:
      names = OP_LISTS if 8 <= shadow.n <= 11 else ("xxz", "wide3")
      exponent = 20 - exponent
      push(("set_observables", str(rng.choice([o for o in names if not shadow.ops or o != shadow.ops[0]])), exponent))
    U = sizes[j % len(sizes)]
    if U > 3 and (shadow.n > 11 or len(shadow.op_list()) > 3 or kind == "program_vjps"):
      U = 3
    if U == 0 and kind not in ("expectation", "vjp_adjoint", "statevector", "table_vjp"):
      U = 1
    push(_c(kind, U))
    if kind in ROW_PRODUCERS and U > 0:   # its rows, directly or behind a forward-only call
      if rng.random() < 0.5:
        push(_c("expectation", 1))
      push(_c("state_gradients", U))
  return {"name": f"random walk {seed}", "seed": 200 + seed, "steps": steps}


@functools.lru_cache(maxsize=None)
def sessions():
  cases = [_shrink_and_grow(), _same_n_swap(), _observable_swap(), _option_flips(), _mask_walk(), _interleave()]
  cases += [random_walk(s) for s in WALK_SEEDS]
  return {c["name"]: c for c in cases}


SESSION_NAMES = ("shrink-and-grow", "same-n circuit swap", "observable swap", "option flips", "mask walk",
                 "entry-point interleave") + tuple(f"random walk {s}" for s in WALK_SEEDS)


# ---- the consumer contract ---------------------------------------------------------------------------------------------
# Every sequence starts from REFUSAL_BASE, runs a producer on REFUSAL_U states, then an event, then a consumer that must
# raise and write nothing.  An event that is a setter is followed by a forward-only qhbm_expectation, which rebuilds the
# plans.  No event's configuration needs more gradient slots, parameters or workspace than the base
# (tests/test_lifecycle_cases_cpu.py): an engine that serves the stale rows anyway reads memory it owns.
REFUSAL_U = 3
REFUSAL_BASE = [("set_circuit", "hea11x2"), ("set_observables", "wide3", 0)]
PRODUCERS = ("expectation_retain", "table_expectation_retain", "expectation_vjp", "expectation_vjp_retained")
CONSUMERS = ("expectation_vjp_retained", "table_expectation_vjp_retained", "state_gradients")
SETTER_EVENTS = (
    ("set_circuit", "hea11"),                       # same size, half the parameters and slots
    ("set_circuit", "hea11x2"),                     # the very same circuit again: the plans are rebuilt all the same
    ("set_observables", "xxz", 0),
    ("set_option", "tile_qubits", 0, True),
    ("set_option", "adjoint_tile_qubits", 11, True),
    ("set_option", "adjoint_exchange", 0, True),
    ("set_option", "adjoint_stop_early", 0, True),
    ("set_gradient_mask", 1),                       # (no forward-only call needed: the mask alone drops both)
)
# ... and every planning option at the value it already has: the header promises the drop "whatever the value"
PLANNING_OPTIONS = (("tile_qubits", 10), ("adjoint_tile_qubits", 10), ("adjoint_exchange", 1), ("adjoint_stop_early", -1),
                    ("round_qubits", 0), ("full_diag_threshold", 60), ("adjoint_full_diag_threshold", 60),
                    ("x_two_shear", 1), ("adjoint_relabel", 1), ("adjoint_plan_search", 1), ("wide_last_pass", -1),
                    ("measure_tile_qubits", 0), ("cph_wave_bits", 1))
SETTER_EVENTS += tuple(("set_option", name, value, False) for name, value in PLANNING_OPTIONS)
# compute entry points that drop the retained states (every one) / the rows (include/qhbm_engine.h)
CALL_EVENTS_STATES = ("expectation", "vjp_adjoint", "vjp_shift", "jacobian", "statevector", "sample_counts",
                      "program_vjps", "table_expectation", "table_vjp")
CALL_EVENTS_ROWS = ("vjp_shift", "jacobian", "sample_counts", "program_vjps")
# setters that change nothing and must drop nothing
NO_CHANGE_EVENTS = (
    ("set_gradient_mask", None),                    # the mask the engine already has (all live)
    ("set_option", "chunk_states", 0, False),       # options that take no part in planning, at their current value
    ("set_option", "workspace_budget_mb", 0, False),
    ("set_option", "values_from_observable", 1, False),
    ("set_option", "shift_prefix_sharing", 1, False),
)


def adjoint_slots(schedule):
  """Gradient slots of the backward plan, from Engine.describe_schedule()."""
  text = schedule[schedule.index("adjoint"):]
  return sum(int(m) for m in re.findall(r"slots=(\d+)", text))
