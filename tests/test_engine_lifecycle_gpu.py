"""One LIVE engine, reconfigured between compute calls, against a fresh engine and the complex128 oracle.

Every other GPU module builds an engine for one configuration and never changes it.  The C ABI allows every setter on a
live handle, and a lot of state survives from call to call inside the engine: the plans and their validity flags, the
four cached backward plans, retained states, the rows of the last adjoint VJP, shift tables, the observable scales, the
workspace buffers, which only grow.  The sessions of tests/lifecycle_cases.py swap circuits of other sizes, observable
lists of other lengths and scales (2^20 apart), gradient masks and plan-changing options between calls.  After every
compute step:

  (a) the outputs equal, bit for bit, the same call on a fresh engine configured straight into the shadow state;
  (b) they meet the oracle within the suite's own bars (lifecycle_cases.oracle).

The consumer contract is a table of its own: after a producer (a retaining forward, an adjoint VJP) and an event that
makes its product stale, qhbm_expectation_vjp_retained / qhbm_table_expectation_vjp_retained / qhbm_state_gradients
must fail and write nothing, and qhbm_retained_states must read 0.  The converse too: a setter that changes nothing
drops nothing, and a forward-only call keeps the rows.

tests/test_lifecycle_cases_cpu.py shows without a GPU that the sessions can fail: plans change where claimed, a stale
answer is at least 100 tolerances away, and no refusal sequence moves to a configuration that needs more memory than
the one before it.

Wall time on one MI355X: 11.4 s for the whole module, next to the rest of the GPU suite's 510 s of a 1200 s budget
(slowest test: the observable swap, 2.9 s).  What that figure is: 94 tests, every session run to its last step, but
with the live engines on the engine's default tiles and not on BASE_OPTIONS, which made the ten session tests fail.
The module as it stands (BASE_OPTIONS on the live engine, 52 more contract cases of a few launches each, nine more
steps in the mask walk) has not been timed.
"""
import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from tests import lifecycle_cases as L
from tests.test_sampling_exact_gpu import Ref, _delta, _gpu_ref, _restated_counts

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def _check_counts(got, shadow, inp, failures, where):
  """qhbm_sample_counts against the restated sampler (tests/test_sampling_exact_gpu.py _counts_and_check): a shot may
  leave the fp64 histogram only where the engine's own fp32 state explains it."""
  n, dim = shadow.n, 1 << shadow.n
  params = inp.params.astype(np.float64)
  got = got.cpu().numpy()
  scratch = E.Engine(0)
  for k, v in shadow.options.items():
    scratch.set_option(k, v)
  for q, (g, s) in enumerate(zip(inp.shift_gates, inp.shifts)):
    gates = L._shifted(shadow.gates, g, s)  # pylint: disable=protected-access
    scratch.set_circuit(n, gates, shadow.n_params)
    psi = scratch.statevector(inp.bits, inp.params)
    for r, b in enumerate(inp.bits):
      ref = Ref.dense(np.abs(O.simulate(n, gates, params, list(b)).ravel()) ** 2)
      delta = _delta(psi[r], ref)
      want, ambiguous = _restated_counts(ref, L.N_SHOTS, r, q, delta, dim)
      off = int(np.abs(got[q, r].astype(np.int64) - want).sum())
      own, _ = _restated_counts(_gpu_ref(psi[r]), L.N_SHOTS, r, q, 0.0, dim)
      moved = int(np.abs(got[q, r].astype(np.int64) - own).sum())
      if got[q, r].sum() != L.N_SHOTS or off > 2 * ambiguous or moved > 2e-3 * L.N_SHOTS:
        failures.append(f"{where}: counts of program {q}, state {r}: {off} off the fp64 histogram ({ambiguous} "
                        f"ambiguous shots), {moved} off the engine's own")


@pytest.mark.parametrize("name", L.SESSION_NAMES)
def test_session(name):
  case = L.sessions()[name]
  steps = case["steps"]
  live = E.Engine(0)
  for k, v in L.BASE_OPTIONS.items():   # what every session starts from; everything after it is a step of the session
    live.set_option(k, v)
  failures = []
  for i, step, before, after, _, inp in L.walk(case):
    if step[0] != "call":
      L.apply_setter(live, after, step)
      continue
    kind = step[1]
    where = f"{name}, step {i} {step}"
    retains = before.retains(inp.U)
    got = L.engine_call(live, inp, kind, retains)
    fresh = before.configure(E.Engine(0))
    if kind == "state_gradients":   # (a fresh engine has rows to serve once it has run the same VJP)
      L.engine_call(fresh, inp, steps[before.rows_from][1])
    again = L.engine_call(fresh, inp, kind, retains)
    wants = L.oracle(before, inp, kind)
    assert len(got) == len(again) == len(wants), where
    for g, f, (label, want, tol) in zip(got, again, wants):
      assert g.shape == f.shape == tuple(want.shape), (where, label, g.shape, f.shape, want.shape)
      if not torch.equal(g, f):
        d = (g.double() - f.double()).abs() if not g.is_complex() else (g - f).abs()
        failures.append(f"{where}: {label} differs from a fresh engine's, max |live - fresh| = {float(d.max()):.6g}")
      if tol is None:
        _check_counts(g, before, inp, failures, where)
      elif want.size:
        err = np.abs(g.cpu().numpy() - want)
        if not (err <= tol).all():
          worst = float((err / tol).max())
          failures.append(f"{where}: {label} misses the oracle, max err {float(err.max()):.6g} = {worst:.3g} tolerances")
    del fresh
  assert not failures, "\n".join(failures)


def test_compute_calls_after_a_circuit_of_another_size_ask_for_observables():
  """qhbm_set_circuit keeps the observables iff the size is unchanged; after another size the calls that need them fail
  with the message of a handle that never had any, and the calls that need none still run."""
  shadow = L.Shadow()
  for i, s in enumerate(L.REFUSAL_BASE):
    shadow.apply(i, s)
  eng = shadow.configure(E.Engine(0))
  inp = L.Inputs(1, 0, shadow, "vjp_adjoint", 2)
  eng.expectation_vjp(inp.bits, inp.params, inp.upstream)
  small = L.Shadow()
  small.apply(0, ("set_circuit", "hea4"))
  L.apply_setter(eng, small, ("set_circuit", "hea4"))
  inp4 = L.Inputs(1, 1, small, "statevector", 2)
  for call in (lambda: eng.expectation(inp4.bits, inp4.params),
               lambda: eng.expectation(inp4.bits, inp4.params, retain=True),
               lambda: eng.expectation_vjp(inp4.bits, inp4.params, np.zeros((2, eng.n_ops), np.float32)),
               lambda: eng.expectation_jacobian(inp4.bits, inp4.params)):
    with pytest.raises(E.EngineError, match="qhbm_set_observables has not been called"):
      call()
  assert eng.retained_states() == 0
  with pytest.raises(E.EngineError):
    eng.state_gradients(2)
  (want,) = L.oracle(small, inp4, "statevector")
  np.testing.assert_allclose(eng.statevector(inp4.bits, inp4.params).cpu().numpy(), want[1], atol=want[2], rtol=0)


# ---- the consumer contract --------------------------------------------------------------------------------------------
class _Setup:
  """A fresh engine in the refusal base configuration and the inputs of producer, event and consumer."""

  def __init__(self):
    self.shadow = L.Shadow()
    for i, s in enumerate(L.REFUSAL_BASE):
      self.shadow.apply(i, s)
    self.eng = self.shadow.configure(E.Engine(0))
    self.inp = L.Inputs(7, 0, self.shadow, "table_vjp", L.REFUSAL_U)

  def produce(self, producer):
    e, i = self.eng, self.inp
    if producer == "expectation_retain":
      e.expectation(i.bits, i.params, retain=True)
    elif producer == "table_expectation_retain":
      e.table_expectation(i.bits, i.params, i.table, retain=True)
    elif producer == "expectation_vjp":
      return e.expectation_vjp(i.bits, i.params, i.upstream)[1]
    elif producer == "expectation_vjp_retained":
      e.expectation(i.bits, i.params, retain=True)
      return e.expectation_vjp_retained(i.bits, i.params, i.upstream)
    else:
      raise KeyError(producer)
    assert e.retained_states() == L.REFUSAL_U
    return None

  def event(self, event):
    """Applies the event; the inputs the consumers are then called with (those of the shadow after it)."""
    after = self.shadow.copy()
    if event[0] == "call":
      inp = L.Inputs(7, 1, after, event[1], 2)
      L.engine_call(self.eng, inp, event[1])
      return self.inp
    if event[0] == "set_gradient_mask":   # (through the ABI: the Python wrapper skips a mask it has already sent)
      if event[1] == "ones":
        m = np.ones(after.n_params, np.uint8)
      else:
        after.apply(len(L.REFUSAL_BASE), event)
        m = None if event[1] is None else after.mask_array().astype(np.uint8)
      rc = self.eng._lib.qhbm_set_gradient_mask(self.eng._h, None if m is None else m.ctypes.data,  # pylint: disable=protected-access
                                                0 if m is None else after.n_params)
      assert rc == 0
    else:
      after.apply(len(L.REFUSAL_BASE), event)
      L.apply_setter(self.eng, after, event)
    self.shadow = after
    return L.Inputs(7, 0, after, "table_vjp", L.REFUSAL_U)

  def consume(self, consumer, inp):
    """The consumer through the ABI on sentinel-filled outputs: (return code, message, the outputs)."""
    e, lib = self.eng, self.eng._lib  # pylint: disable=protected-access
    dev = e.device
    bits = torch.as_tensor(inp.bits).to(dev)
    params = torch.as_tensor(inp.params).to(dev)
    up = torch.as_tensor(inp.upstream).to(dev).contiguous()
    tup = torch.as_tensor(inp.table_upstream).to(dev)
    table = torch.as_tensor(inp.table).to(dev)
    U, P = inp.U, e.n_params
    outs = {"grad": torch.full((P,), SENTINEL, device=dev), "rows": torch.full((U, P), SENTINEL, device=dev),
            "table_grad": torch.full((1 << e.n_qubits,), SENTINEL, device=dev)}
    with torch.cuda.device(dev):
      if consumer == "expectation_vjp_retained":
        rc = lib.qhbm_expectation_vjp_retained(e._h, bits.data_ptr(), U, params.data_ptr(), up.data_ptr(),  # pylint: disable=protected-access
                                               outs["grad"].data_ptr(), e._stream())  # pylint: disable=protected-access
      elif consumer == "table_expectation_vjp_retained":
        rc = lib.qhbm_table_expectation_vjp_retained(e._h, bits.data_ptr(), U, params.data_ptr(), table.data_ptr(),  # pylint: disable=protected-access
                                                     tup.data_ptr(), outs["grad"].data_ptr(), outs["table_grad"].data_ptr(),
                                                     e._stream())  # pylint: disable=protected-access
      elif consumer == "state_gradients":
        rc = lib.qhbm_state_gradients(e._h, U, outs["rows"].data_ptr(), e._stream())  # pylint: disable=protected-access
      else:
        raise KeyError(consumer)
    torch.cuda.synchronize()
    return rc, lib.qhbm_last_error(e._h).decode(), outs  # pylint: disable=protected-access

  def refused(self, consumer, inp, where):
    rc, _, outs = self.consume(consumer, inp)
    with pytest.raises(E.EngineError):
      self.eng._check(rc)  # pylint: disable=protected-access
    for label, t in outs.items():
      assert bool((t == SENTINEL).all()), f"{where}: the refused {consumer} wrote into {label}"


_STATE_PRODUCERS = ("expectation_retain", "table_expectation_retain")
_ROW_PRODUCERS = ("expectation_vjp", "expectation_vjp_retained")
assert set(_STATE_PRODUCERS + _ROW_PRODUCERS) == set(L.PRODUCERS)


@pytest.mark.parametrize("event", L.SETTER_EVENTS, ids=lambda e: " ".join(str(x) for x in e[:3]))
@pytest.mark.parametrize("producer", L.PRODUCERS)
def test_setter_makes_the_product_stale(producer, event):
  """Producer, a setter that invalidates a plan, a forward-only call that rebuilds the plans: every consumer must
  refuse and write nothing, and from the setter on qhbm_retained_states reads 0."""
  s = _Setup()
  s.produce(producer)
  inp = s.event(event)
  where = f"{producer}, then {event}"
  assert s.eng.retained_states() == 0, f"{where}: retained_states() still reports states the retained call refuses"
  if event[0] != "set_gradient_mask":   # (that event goes through the ABI; the wrapper's token follows its own setters)
    assert s.eng.retained is None, f"{where}: the wrapper still holds a token for states the engine dropped"
  if event[0] != "set_gradient_mask":
    s.eng.expectation(inp.bits, inp.params)
  assert s.eng.retained_states() == 0, where
  for consumer in L.CONSUMERS:
    s.refused(consumer, inp, where)
  # and the engine is none the worse: the next VJP and its rows are a fresh engine's
  got = L.engine_call(s.eng, inp, "vjp_adjoint") + L.engine_call(s.eng, inp, "state_gradients")
  fresh = s.shadow.configure(E.Engine(0))
  want = L.engine_call(fresh, inp, "vjp_adjoint") + L.engine_call(fresh, inp, "state_gradients")
  for g, w in zip(got, want):
    assert torch.equal(g, w), where


@pytest.mark.parametrize("producer,event", [(p, e) for p in _STATE_PRODUCERS for e in L.CALL_EVENTS_STATES] +
                         [(p, e) for p in _ROW_PRODUCERS for e in L.CALL_EVENTS_ROWS])
def test_compute_call_drops_the_product(producer, event):
  """The entry points the header says drop the retained states (every other compute call) or the rows."""
  s = _Setup()
  s.produce(producer)
  inp = s.event(("call", event))
  where = f"{producer}, then a {event} call"
  assert s.eng.retained_states() == 0, where
  consumers = L.CONSUMERS if producer in _ROW_PRODUCERS else ("expectation_vjp_retained", "table_expectation_vjp_retained")
  for consumer in consumers:
    s.refused(consumer, inp, where)


_SAME = L.NO_CHANGE_EVENTS + (("set_gradient_mask", "ones"),)   # an explicit all-live mask IS the mask of a new circuit


@pytest.mark.parametrize("event", _SAME, ids=lambda e: " ".join(str(x) for x in e[:3]))
@pytest.mark.parametrize("producer", L.PRODUCERS)
def test_a_setter_that_changes_nothing_drops_nothing(producer, event):
  """The installed mask again, or an option that takes no part in planning set to its current value: the consumer still
  succeeds, and its output is the one of an engine that never saw the setter."""
  consumer = {"expectation_retain": "expectation_vjp_retained", "table_expectation_retain": "table_expectation_vjp_retained",
              "expectation_vjp": "state_gradients", "expectation_vjp_retained": "state_gradients"}[producer]
  outs = []
  for with_event in (True, False):
    s = _Setup()
    s.produce(producer)
    if with_event:
      s.event(event)
    if producer in _STATE_PRODUCERS:
      assert s.eng.retained_states() == L.REFUSAL_U, (producer, event)
    rc, msg, out = s.consume(consumer, s.inp)
    assert rc == 0, (producer, event, msg)
    outs.append(out)
  for label in outs[0]:
    assert torch.equal(outs[0][label], outs[1][label]), (producer, event, label)
  touched = {"expectation_vjp_retained": ["grad"], "table_expectation_vjp_retained": ["grad", "table_grad"],
             "state_gradients": ["rows"]}[consumer]
  for label in touched:
    assert not bool((outs[0][label] == SENTINEL).any()), (producer, event, label)


def test_rows_outlive_a_forward_only_call():
  """After a forward-only qhbm_expectation the rows of the adjoint VJP before it are still served: the same bits as
  before the call, as a fresh engine's, and their sum over the states is that VJP's gradient up to the fp32 rounding
  of each.  Equality is no property of the engine: reduce_grad_kernel adds factor * slot over all states in fp64 and
  rounds once to fp32, scatter_jac_kernel rounds each state's row to fp32.  In this configuration every parameter has
  ONE slot (tests/test_lifecycle_cases_cpu.py), so a row is one correctly rounded product and the gradient the
  correctly rounded sum of the same products: with u = 2^-24,
      |sum_u rows[u, p] - grad[p]| <= u (sum_u |rows[u, p]| + |grad[p]|)
  (the 2^-20 on top covers the second-order terms and the fp64 additions)."""
  s = _Setup()
  grad = s.produce("expectation_vjp")
  before = s.eng.state_gradients(L.REFUSAL_U)
  other = L.Inputs(7, 2, s.shadow, "expectation", 9)
  s.eng.expectation(other.bits, other.params)
  after = s.eng.state_gradients(L.REFUSAL_U)
  assert torch.equal(before, after)
  fresh = s.shadow.configure(E.Engine(0))
  fresh.expectation_vjp(s.inp.bits, s.inp.params, s.inp.upstream)
  assert torch.equal(fresh.state_gradients(L.REFUSAL_U), after)
  total = after.double().sum(0).cpu().numpy()
  g = grad.double().cpu().numpy()
  bound = 2.0 ** -24 * (1 + 2.0 ** -20) * (after.double().abs().sum(0).cpu().numpy() + np.abs(g))
  assert np.abs(g).max() > 0 and (np.abs(total - g) <= bound).all(), (np.abs(total - g) / np.maximum(bound, 1e-300)).max()
  (_, want, tol), = L.oracle(s.shadow, s.inp, "state_gradients")
  assert (np.abs(after.cpu().numpy() - want) <= tol).all()
  with pytest.raises(E.EngineError):       # ... but only for the batch they were computed on
    s.eng.state_gradients(L.REFUSAL_U - 1)
