"""The random cases the plan emulator ran on the CPU (tests/sanitize/plan_fuzz.cpp --dump-cases, committed as
tests/golden/plan_fuzz_cases.json), on the real engine against the numpy oracle in complex128.

Together with tests/test_sanitize_cpu.py this locates a disagreement: the emulator executes the same plans from the
same scheduler in double and agrees with a dense oracle there, so a case that fails HERE is a kernel's doing (or the
upload's), one that fails THERE the scheduler's.  Every case carries the options its plans were built with -- tile sizes,
relabeling, wave-bit mapping, FULL thresholds, wide last pass, measurement tile, plan search, gradient mask and whether the
sweep stops early, the lean lowering on or off -- and the sample holds every feature the emulation counts at least twice.

Bars: those of tests/test_engine_gpu.py (fp32 engine against a complex128 oracle): values 5e-5 * sum|c_k|, gradients
1e-4 * max(1, ||grad||_inf), amplitudes 3e-6.  One engine per case, closed after it.  GPU only."""
import numpy as np
import pytest

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from tests.test_plan_fuzz_cases_cpu import case_inputs, load_cases

pytestmark = pytest.mark.gpu

CASES = load_cases()


@pytest.mark.parametrize("case", CASES, ids=[f"case{c['case']}-os{c['option_set']}-n{c['n']}" for c in CASES])
def test_engine_on_emulated_case(case, monkeypatch):
  n, P = case["n"], case["n_params"]
  gates, ops, params, bits, up_op = case_inputs(case)
  up = np.tile(up_op, (bits.shape[0], 1))
  if case["lean_lowering"]:
    monkeypatch.delenv("QHBM_NO_LEAN_CLIFFORD", raising=False)
  else:
    monkeypatch.setenv("QHBM_NO_LEAN_CLIFFORD", "1")
  mask = None if case["gradient_mask"] is None else np.asarray(case["gradient_mask"], dtype=bool)
  want_vals, jac = O.expectation_jacobian(n, gates, params, bits, ops)
  want_rows = np.einsum("bt,btp->bp", up, jac)
  if mask is not None:
    want_rows = want_rows * mask[None, :]
  want_grad = want_rows.sum(axis=0)
  norm = np.array([sum(abs(c) for c, _, _ in op) for op in ops])
  val_bar = 5e-5 * np.maximum(norm, 1e-30)[None, :]
  grad_bar = 1e-4 * max(1.0, np.abs(want_grad).max())
  row_bar = 1e-4 * max(1.0, np.abs(want_rows).max())

  eng = E.Engine(0)
  try:
    for name, value in case["options"].items():
      eng.set_option(name, value)
    eng.set_circuit(n, gates, P)
    eng.set_observables(ops)
    if mask is not None:
      eng.set_gradient_mask(mask)

    vals = eng.expectation(bits, params).cpu().numpy()
    assert (np.abs(vals - want_vals) <= val_bar).all(), ("expectation", np.abs(vals - want_vals).max())

    vals2, grad = eng.expectation_vjp(bits, params, up)
    vals2, grad = vals2.cpu().numpy(), grad.cpu().numpy()
    assert (np.abs(vals2 - want_vals) <= val_bar).all(), ("vjp values", np.abs(vals2 - want_vals).max())
    assert np.abs(grad - want_grad).max() <= grad_bar, ("vjp", np.abs(grad - want_grad).max(), grad_bar)
    if mask is not None:
      assert (grad[~mask] == 0).all()
    rows = eng.state_gradients(bits.shape[0]).cpu().numpy()
    assert np.abs(rows - want_rows).max() <= row_bar, ("state gradients", np.abs(rows - want_rows).max(), row_bar)

    sv = eng.statevector(bits, params).cpu().numpy()
    for b in range(bits.shape[0]):
      want_sv = O.simulate(n, gates, params, bits[b]).reshape(-1)
      assert np.abs(sv[b] - want_sv).max() <= 3e-6, ("statevector", b, np.abs(sv[b] - want_sv).max())

    vals3 = eng.expectation(bits, params, retain=True).cpu().numpy()
    assert (np.abs(vals3 - want_vals) <= val_bar).all(), ("retained values", np.abs(vals3 - want_vals).max())
    assert eng.retained is not None
    grad3 = eng.expectation_vjp_retained(bits, params, up).cpu().numpy()
    assert np.abs(grad3 - want_grad).max() <= grad_bar, ("retained vjp", np.abs(grad3 - want_grad).max(), grad_bar)
  finally:
    eng.close()
