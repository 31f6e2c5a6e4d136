"""The complex128 restatement of the weighted Gram matrix's VJP and of the state metrics' gradients
(tests/state_metrics_vjp_ref.py, what the GPU tests compare the engine with) against central differences in float64 --
step 1e-5, bar 1e-7 * max(1, ||grad||_inf), as tests/test_final_states_cpu.py and tests/test_reduced_density_vjp_cpu.py.
Then what needs no GPU of the new entry points: the ABI symbols, the scratch size, the launch plan's checker and a
stand-alone compile of the kernels' translation unit."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import state_metrics_ref as R
from tests import state_metrics_vjp_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qhbm-library_amd", "csrc")
STEP = 1e-5
SHAPES = [(n, num) for n in (3, 4, 5) for num in (1, 3, 5)]


def _bar(grad):
  return 1e-7 * max(1.0, float(np.abs(grad).max()))


def _case(n, num):
  """(non-orthogonal states of norms 0.5 ... 1.5, a signed table)"""
  states = V.random_states(num, n, 100 * n + num) * np.linspace(0.5, 1.5, num)[:, None]
  table = np.random.default_rng(200 * n + num).normal(size=1 << n)
  return states, table


def _central_states(f, states):
  """dL/dRe a + i dL/dIm a, amplitude by amplitude."""
  grad = np.zeros(states.shape, dtype=np.complex128)
  for m in range(states.shape[0]):
    for x in range(states.shape[1]):
      for unit in (1.0, 1j):
        hi, lo = states.copy(), states.copy()
        hi[m, x] += STEP * unit
        lo[m, x] -= STEP * unit
        grad[m, x] += unit * (f(hi) - f(lo)) / (2 * STEP)
  return grad


def _central_real(f, vector):
  grad = np.zeros(vector.shape)
  for x in range(vector.size):
    hi, lo = vector.copy(), vector.copy()
    hi[x] += STEP
    lo[x] -= STEP
    grad[x] = (f(hi) - f(lo)) / (2 * STEP)
  return grad


def _hold(label, got, want):
  err = float(np.abs(got - want).max())
  print(f"{label}: error {err:.3e} (bar {_bar(want):.3e}, ||grad|| {np.abs(want).max():.3e})")
  assert err <= _bar(want), label


@pytest.mark.parametrize("kind", ["lin", "quad", "fid"])
@pytest.mark.parametrize("n,num", SHAPES)
def test_gram_vjp_matches_central_differences(n, num, kind):
  """Re sum conj(B_ij) G_ij with a B that is not Hermitian, Re tr(W G W G) and (sum sqrt(lambda(W^1/2 G W^1/2)))^2."""
  states, table = _case(n, num)
  if kind == "fid":  # (a root of the spectrum: defined for a positive table, as the fidelity's p = softmax(-E) is)
    table = np.abs(table) + 0.1
  aux = V.loss_aux(kind, num, 7 * n + num)
  if kind == "lin" and num > 1:
    assert np.abs(aux - aux.conj().T).max() > 0.1
  _, gamma = V.loss_of(kind, R.gram(states, table), aux)
  got_states, got_table = V.vjp(states, table, gamma)
  want_states = _central_states(lambda s: V.loss_of(kind, R.gram(s, table), aux)[0], states)
  want_table = _central_real(lambda t: V.loss_of(kind, R.gram(states, t), aux)[0], table)
  _hold(f"n={n} M={num} loss {kind}: states", got_states, want_states)
  _hold(f"n={n} M={num} loss {kind}: table", got_table, want_table)
  assert np.abs(want_states).max() > 1e-3 and np.abs(want_table).max() > 1e-4  # (the check is not of zeros)
  # no table: ones, and the states' cotangent alone
  _, gamma = V.loss_of(kind, R.gram(states), aux)
  _hold(f"n={n} M={num} loss {kind}: states, no table", V.vjp(states, None, gamma)[0],
        _central_states(lambda s: V.loss_of(kind, R.gram(s), aux)[0], states))


@pytest.mark.parametrize("metric", ["overlap", "fidelity", "cross_entropy", "relative_entropy"])
@pytest.mark.parametrize("n,num", SHAPES)
def test_metric_gradients_match_central_differences(n, num, metric):
  """The losses through p = softmax(-E) and through E itself: the gradients with respect to the amplitudes a = U^dagger phi
  and to the energy table."""
  states, energies = _case(n, num)
  weights = np.random.default_rng(300 * n + num).uniform(0.1, 0.6, num)
  got_states, got_energies = V.metric_gradients(states, energies, weights)[metric]
  constants = V.data_constants(states, weights)
  want_states = _central_states(lambda s: V.metric_values(s, energies, weights, constants)[metric], states)
  want_energies = _central_real(lambda e: V.metric_values(states, e, weights, constants)[metric], energies)
  _hold(f"n={n} M={num} {metric}: amplitudes", got_states, want_states)
  _hold(f"n={n} M={num} {metric}: energies", got_energies, want_energies)
  assert np.abs(want_states).max() > 1e-3 and np.abs(want_energies).max() > 1e-4


def test_metric_values_are_those_of_the_forward_restatement():
  n, num = 4, 3
  states, energies = _case(n, num)
  weights = np.array([0.2, 0.5, 0.3])
  unitary = np.linalg.qr(V.random_states(1 << n, n, 5).T)[0]
  want = R.metrics(unitary, energies, (unitary @ states.T).T, weights)
  got = V.metric_values(states, energies, weights)
  for key, value in got.items():
    np.testing.assert_allclose(value, want[key], rtol=1e-12, atol=1e-13)


def test_hand_checks():
  rng = np.random.default_rng(1)
  a = rng.normal(size=(2, 8)) + 1j * rng.normal(size=(2, 8))
  t = rng.normal(size=8)
  # M = 1, L = G: g = 2 t a, tbar = |a|^2
  out, grad = V.vjp(a[:1], t, np.ones((1, 1)))
  np.testing.assert_allclose(out, 2 * t * a[:1], atol=1e-14)
  np.testing.assert_allclose(grad, np.abs(a[0])**2, atol=1e-14)
  # L = Re G_01: g_1 = t a_0, g_0 = t a_1
  gamma = np.zeros((2, 2), dtype=np.complex128)
  gamma[0, 1] = 1.0
  out, grad = V.vjp(a, t, gamma)
  np.testing.assert_allclose(out[1], t * a[0], atol=1e-14)
  np.testing.assert_allclose(out[0], t * a[1], atol=1e-14)
  np.testing.assert_allclose(grad, np.real(np.conj(a[0]) * a[1]), atol=1e-14)
  # L = Im G_01: g_1 = i t a_0
  gamma[0, 1] = 1j
  out, grad = V.vjp(a, t, gamma)
  np.testing.assert_allclose(out[1], 1j * t * a[0], atol=1e-14)
  np.testing.assert_allclose(out[0], -1j * t * a[1], atol=1e-14)
  np.testing.assert_allclose(grad, np.imag(np.conj(a[0]) * a[1]), atol=1e-14)
  # the bound terms dominate the outputs they bound
  h = gamma + gamma.conj().T
  out, grad = V.gram_vjp(a, t, h)
  out_bar, grad_bar = V.gram_vjp_bounds(a, t, h)
  assert np.all(np.abs(out.real) <= out_bar + 1e-15) and np.all(np.abs(out.imag) <= out_bar + 1e-15)
  assert np.all(np.abs(grad) <= grad_bar + 1e-15)


# ---- the entry points, without a device ------------------------------------------------------------------------------------
NEW_SYMBOLS = ("qhbm_gram_vjp_scratch_bytes", "qhbm_weighted_gram_vjp")


def test_abi_symbols_and_version():
  from qhbmlib_amd import _engine as E  # pylint: disable=import-outside-toplevel
  with open(os.path.join(ROOT, "include", "qhbm_engine.h")) as f:
    header = f.read()
  assert int(re.search(r"#define QHBM_ABI_VERSION (\d+)", header).group(1)) == 5 == E.ABI_VERSION
  lib = E.load_library()
  assert lib.qhbm_abi_version() == 5
  for sym in NEW_SYMBOLS:
    assert re.search(r"\bint " + sym + r"\(", header), sym
    assert sym in E.ABI_SYMBOLS
    getattr(lib, sym)


def test_scratch_size_needs_no_device_and_refuses_bad_shapes():
  from qhbmlib_amd import _engine as E  # pylint: disable=import-outside-toplevel
  # vector kernel (M <= 8): none is used, the call answers 16
  for num, n in [(1, 1), (8, 24), (5, 31)]:
    assert E.gram_vjp_scratch_bytes(num, n) == 16
  # matrix kernel: H as two zero-padded float planes of P x P, P = M rounded up to 16 (to 64 beyond 64); no term in n
  for num, pitch in [(9, 16), (16, 16), (17, 32), (33, 48), (64, 64), (65, 128), (1024, 1024)]:
    assert E.gram_vjp_scratch_bytes(num, 3) == E.gram_vjp_scratch_bytes(num, 31) == 8 * pitch * pitch
  lib = E.load_library()
  out = ctypes.c_size_t()
  for args, text in [((0, 6), "M must be in [1, 1024]"), ((1025, 6), "M must be in"), ((-1, 6), "M must be in"),
                     ((1, 0), "n_qubits must be in [1, 31]"), ((1, 32), "n_qubits must be in [1, 31]")]:
    assert lib.qhbm_gram_vjp_scratch_bytes(*args, ctypes.byref(out)) != 0
    assert text in lib.qhbm_last_error(None).decode(), (args, lib.qhbm_last_error(None).decode())
  assert lib.qhbm_gram_vjp_scratch_bytes(1, 6, None) != 0
  assert "out is NULL" in lib.qhbm_last_error(None).decode()
  with pytest.raises(E.EngineError, match="CUDA states"):
    E.weighted_gram_vjp(np.zeros((1, 4)), None, np.eye(1))
  from qhbmlib_amd import inference  # pylint: disable=import-outside-toplevel
  with pytest.raises(E.EngineError, match="CUDA states"):
    inference.weighted_gram(np.zeros((1, 4)))


def test_gram_vjp_plan_under_asan_and_ubsan(tmp_path):
  """tests/gram_vjp_plan/gram_vjp_plan_check.cpp: every n <= 13 and M in {1, 3, 4, 5, 8, 15, 16, 17, 33, 64, 1024} walked as
  the kernels walk them -- each output word and table_grad entry written once, reads in bounds, LDS entries stored before
  they are read, the H planes inside the scratch, the grid within launch limits at 31 qubits and 1024 states."""
  cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
  assert cxx, "no host C++ compiler"
  src = os.path.join(ROOT, "tests", "gram_vjp_plan")
  build = subprocess.run(["make", f"CXX={cxx}", f"OUT={tmp_path}"], cwd=src, capture_output=True, text=True, timeout=600)
  assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
  run = subprocess.run([str(tmp_path / "gram_vjp_plan_check")], capture_output=True, text=True, timeout=900, env=env)
  tail = run.stdout[-3000:] + run.stderr[-3000:]
  assert run.returncode == 0, tail
  assert "gram_vjp_plan_check: 143 shapes" in run.stdout and "gram_vjp_plan_check: 0 failures" in run.stdout, tail
  assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, tail


def test_translation_unit_compiles_alone_for_gfx950():
  hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  assert os.path.exists(hipcc), "no hipcc"
  run = subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-Wall", "-Wno-unused-function", "-x", "hip",
                        "gram_vjp.hip"], cwd=CSRC, capture_output=True, text=True, timeout=600)
  assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
  # it is part of observable.o, and of no other object
  with open(os.path.join(CSRC, "observable.hip")) as f:
    assert '#include "gram_vjp.hip"' in f.read()
  with open(os.path.join(CSRC, "states.hip")) as f:
    assert "gram_vjp" not in f.read()
