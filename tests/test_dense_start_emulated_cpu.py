"""The dense-start plans of the from-states calls on the CPU (tests/sanitize/dense_start.cpp; host only, built with
AddressSanitizer + UBSan on top of the sanitizer build tests/test_sanitize_cpu.py uses).

The plan emulator's forward half starts from a bitstring and cannot be handed a state, so the driver checks the forward
plan's arguments structurally (no basis-state pass, no pruning mask, no stale-half clearing -- on a circuit whose
basis-state plans do prune) and EXECUTES the backward plans from psi = C phi for a dense random phi: gradients against
central differences (step 1e-5, bar 1e-7 of the largest entry), with a gradient mask stopping early and not, at 12
qubits in tiles of 2^10 (an idle qubit and a diagonal-only qubit at either end of the index) and at 6 qubits (padding)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "sanitize")
CSRC = os.path.join(ROOT, "qhbm-library_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.mark.timeout(1500)
def test_dense_start_plans_emulated_from_a_random_state():
  if not shutil.which(HIPCC):
    pytest.skip("no hipcc")
  # the kernel launchers the engine links against come from the product build (never called here)
  subprocess.run(["make", "kernels.o", "observable.o", "states.o"], cwd=CSRC, check=True, capture_output=True, timeout=1200)
  build = subprocess.run(["make", "-j4", "-f", "dense_start.mk", "_build/dense_start"], cwd=SAN, capture_output=True, text=True,
                         timeout=900)
  assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
  run = subprocess.run([os.path.join(SAN, "_build", "dense_start")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **ENV))
  tail = run.stdout[-2000:] + run.stderr[-3000:]
  print(run.stdout)
  assert run.returncode == 0, tail
  assert "dense_start: 0 failures" in run.stdout and run.stdout.count("max gradient error") == 7, tail
  assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, tail
