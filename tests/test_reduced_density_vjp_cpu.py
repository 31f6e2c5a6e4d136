"""The complex128 restatement of the reduced density matrix's VJP and of `qhbm_subsystem_apply`
(tests/reduced_density_vjp_ref.py, what the GPU tests compare the engine with) against central differences in float64 --
step 1e-5, bar 1e-7 * max(1, ||grad||_inf), as tests/test_final_states_cpu.py: the losses are polynomials of degree at most
four in the amplitudes, so the truncation error h^2 f''' / 6 is ~1e-10 and the rounding error 2^-53 |loss| / h ~1e-11.
Then what needs no GPU of the new entry points: the ABI symbols, the scratch size, the launch plan's checker and a
stand-alone compile of the kernels' translation unit."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import reduced_density_ref as R
from tests import reduced_density_vjp_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qhbm-library_amd", "csrc")
STEP = 1e-5

# (n, kept qubits): contiguous, non-contiguous, index bit 0 kept and not, k = n
SHAPES = [(4, (0, 1)), (4, (1, 3)), (4, (0, 1, 2, 3)), (5, (0, 2, 4)), (5, (3,)), (6, (1, 2, 5)), (6, (0, 3)), (6, (0, 1, 2, 3, 4, 5))]
WEIGHTS = np.array([0.5, -0.3, 1.2])


def _bar(grad):
  return 1e-7 * max(1.0, float(np.abs(grad).max()))


def _loss(kind, aux, states, weights, kept):
  return V.loss_of(kind, R.reduced(states, kept, weights)[0], aux)[0]


def _central_states(kind, aux, states, weights, kept):
  """dL/dRe phi + i dL/dIm phi, amplitude by amplitude."""
  grad = np.zeros(states.shape, dtype=np.complex128)
  for m in range(states.shape[0]):
    for x in range(states.shape[1]):
      for unit in (1.0, 1j):
        hi, lo = states.copy(), states.copy()
        hi[m, x] += STEP * unit
        lo[m, x] -= STEP * unit
        grad[m, x] += unit * (_loss(kind, aux, hi, weights, kept) - _loss(kind, aux, lo, weights, kept)) / (2 * STEP)
  return grad


def _central_weights(kind, aux, states, weights, kept):
  grad = np.zeros(len(weights))
  for m in range(len(weights)):
    hi, lo = weights.copy(), weights.copy()
    hi[m] += STEP
    lo[m] -= STEP
    grad[m] = (_loss(kind, aux, states, hi, kept) - _loss(kind, aux, states, lo, kept)) / (2 * STEP)
  return grad


@pytest.mark.parametrize("kind", ["a", "b", "c", "lin"])
@pytest.mark.parametrize("n,kept", SHAPES)
def test_vjp_matches_central_differences(n, kept, kind):
  """(a)-(c) of the issue, and "lin": Re tr(Gamma^H rho) with a Gamma that is not Hermitian."""
  states = V.random_states(3, n, 100 * n + len(kept)) * np.array([0.5, 1.0, 1.5])[:, None]
  aux = V.loss_aux(kind, len(kept), 7 * n + len(kept))
  rho, _ = R.reduced(states, kept, WEIGHTS)
  _, gamma = V.loss_of(kind, rho, aux)
  if kind == "lin":
    assert np.abs(gamma - gamma.conj().T).max() > 0.1
  got_states, got_weights = V.vjp(states, WEIGHTS, kept, gamma)
  want_states = _central_states(kind, aux, states, WEIGHTS, kept)
  want_weights = _central_weights(kind, aux, states, WEIGHTS, kept)
  err_s, err_w = float(np.abs(got_states - want_states).max()), float(np.abs(got_weights - want_weights).max())
  print(f"n={n} kept={kept} loss {kind}: states {err_s:.3e} (bar {_bar(want_states):.3e}), weights {err_w:.3e} "
        f"(bar {_bar(want_weights):.3e})")
  assert err_s <= _bar(want_states)
  assert err_w <= _bar(want_weights)
  assert np.abs(want_states).max() > 1e-3 and np.abs(want_weights).max() > 1e-3  # (the check is not of zeros)


@pytest.mark.parametrize("n,kept", SHAPES)
def test_apply_is_the_dense_operator_and_the_vjp_is_one_apply(n, kept):
  """`apply` against kron-built dense matrices, index by index, and the identity the engine's backward rests on:
  grad_states = apply(H, scale = w), grad_weights = 1/2 Re dots, H = Gamma + Gamma^H."""
  k = len(kept)
  states = V.random_states(3, n, 31 * n + k)
  (op,) = V.loss_aux("lin", k, 5 * n + k)
  scale = np.array([0.0, -1.5, 2.0])
  out, dots, out_bar, dots_bar = V.apply(states, kept, op, scale)
  # the dense operator, built from the convention alone: row index = kept bits big-endian, the rest untouched
  dim = 1 << n
  kept_sorted = sorted(kept)

  def row_of(index):
    a = 0
    for q in kept_sorted:
      a = (a << 1) | ((index >> (n - 1 - q)) & 1)
    return a
  kept_bits = sum(1 << (n - 1 - q) for q in kept_sorted)
  dense = np.zeros((dim, dim), dtype=np.complex128)
  for i in range(dim):
    for j in range(dim):
      if (i & ~kept_bits) == (j & ~kept_bits):
        dense[i, j] = op[row_of(i), row_of(j)]
  want = states @ dense.T
  np.testing.assert_allclose(out, scale[:, None] * want, rtol=0, atol=1e-13)
  np.testing.assert_allclose(dots, np.einsum("mx,mx->m", states.conj(), want), rtol=0, atol=1e-13)
  assert np.all(np.abs(out) <= out_bar + 1e-15) and np.all(np.abs(dots) <= dots_bar + 1e-15)
  gamma = op
  grad_states, grad_weights = V.vjp(states, scale, kept, gamma)
  via_apply, via_dots, _, _ = V.apply(states, kept, gamma + gamma.conj().T, scale)
  np.testing.assert_allclose(grad_states, via_apply, rtol=0, atol=1e-13)
  np.testing.assert_allclose(grad_weights, 0.5 * via_dots.real, rtol=0, atol=1e-13)
  assert np.abs(via_dots.imag).max() <= 1e-13  # (Hermitian: the expectation is real)


# ---- the entry points, without a device ------------------------------------------------------------------------------------
NEW_SYMBOLS = ("qhbm_subsystem_apply_scratch_bytes", "qhbm_subsystem_apply")


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
  # vector kernel: 16 bytes per state and slice of 1024 environment values
  assert E.subsystem_apply_scratch_bytes(3, 6, 0b100001) == 3 * 16
  assert E.subsystem_apply_scratch_bytes(2, 14, 0b1) == 2 * 16 * 8
  # matrix kernel: the transposed operator, then 16 bytes per state and tile (64 rows x 64 environment values)
  assert E.subsystem_apply_scratch_bytes(2, 12, 0x3ff) == 8 * 4**10 + 2 * 16 * 16
  assert E.subsystem_apply_scratch_bytes(3, 14, 0x3ff << 2) == 8 * 4**10 + 3 * 16 * 16
  assert E.subsystem_apply_scratch_bytes(1, 16, 0b1111) == 8 * 4**4 + 16 * (4096 // 64)
  lib = E.load_library()
  out = ctypes.c_size_t()
  for args, text in [((0, 6, 1), "M must be in [1, 65536]"), ((65537, 6, 1), "M must be in"), ((1, 32, 1), "n_qubits must be in [1, 31]"),
                     ((1, 6, 1 << 6), "at or above n_qubits"), ((1, 12, 0x7ff), "between 1 and min(n_qubits, 10)"),
                     ((1, 6, 0), "between 1 and min(n_qubits, 10)")]:
    assert lib.qhbm_subsystem_apply_scratch_bytes(*args, ctypes.byref(out)) != 0
    assert text in lib.qhbm_last_error(None).decode(), (args, lib.qhbm_last_error(None).decode())
  assert lib.qhbm_subsystem_apply_scratch_bytes(1, 6, 1, None) != 0
  assert "out is NULL" in lib.qhbm_last_error(None).decode()
  with pytest.raises(E.EngineError, match="CUDA states"):
    E.subsystem_apply(np.zeros((1, 4)), 1, np.eye(2))


def test_subsystem_plan_under_asan_and_ubsan(tmp_path):
  """tests/subsystem_plan/subsystem_plan_check.cpp: every n <= 12 and every mask with k <= 10 walked as the kernels walk
  them -- each amplitude written once, reads in bounds, LDS tiles stored once, partials inside the scratch."""
  cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
  assert cxx, "no host C++ compiler"
  src = os.path.join(ROOT, "tests", "subsystem_plan")
  build = subprocess.run(["make", f"CXX={cxx}", f"OUT={tmp_path}"], cwd=src, capture_output=True, text=True, timeout=600)
  assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
  run = subprocess.run([str(tmp_path / "subsystem_plan_check")], capture_output=True, text=True, timeout=900, env=env)
  tail = run.stdout[-3000:] + run.stderr[-3000:]
  assert run.returncode == 0, tail
  assert "subsystem_plan_check: 8164 masks" in run.stdout and "subsystem_plan_check: 0 failures" in run.stdout, tail
  assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, tail


def test_translation_unit_compiles_alone_for_gfx950():
  hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  assert os.path.exists(hipcc), "no hipcc"
  run = subprocess.run([hipcc, "-std=c++17", "--offload-arch=gfx950", "-fsyntax-only", "-Wall", "-Wno-unused-function", "-x", "hip",
                        "subsystem_apply.hip"], cwd=CSRC, capture_output=True, text=True, timeout=600)
  assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
  # it is part of observable.o, and of no other object
  with open(os.path.join(CSRC, "observable.hip")) as f:
    assert '#include "subsystem_apply.hip"' in f.read()
  with open(os.path.join(CSRC, "states.hip")) as f:
    assert "subsystem_apply" not in f.read()
