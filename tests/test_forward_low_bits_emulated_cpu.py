"""Forward plans that move the low index bits, executed on the CPU against the dense oracle
(tests/forward_low_bits/moved_plan_check.cpp; a stand-alone host program built with AddressSanitizer + UBSan on top of
the sanitizer build tests/test_sanitize_cpu.py uses, and run directly).

The plan emulator of tests/sanitize/ stores every tile in place and keeps covering the plans without the freedom; the
program runs that emulator's forward executor with the moving store (driven by the same PassArgs) on random
hardware-efficient and inverted circuits, 13..16 qubits, depth 2..6, three basis states each, and holds the final state
(1e-10 per amplitude) and the values of an XXZ chain and a TFIM ring (1e-10 max(1, sum |c_k|)) to the dense oracle.  Every
case has at least one pass that permutes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests", "forward_low_bits")
CSRC = os.path.join(ROOT, "qhbm-library_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.mark.timeout(1500)
def test_moving_forward_plans_emulated_against_the_dense_oracle():
  if not shutil.which(HIPCC):
    pytest.skip("no hipcc")
  # the kernel launchers the engine links against come from the product build (never called here)
  subprocess.run(["make", "kernels.o", "observable.o", "states.o"], cwd=CSRC, check=True, capture_output=True, timeout=1200)
  build = subprocess.run(["make", "-j4", "_build/moved_plan_check"], cwd=HERE, capture_output=True, text=True, timeout=900)
  assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
  run = subprocess.run([os.path.join(HERE, "_build", "moved_plan_check")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **ENV))
  tail = run.stdout[-2000:] + run.stderr[-3000:]
  print(run.stdout)
  assert run.returncode == 0, tail
  assert "moved_plan_check: 0 failures" in run.stdout and run.stdout.count(" moving), state error ") == 9, tail
  assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, tail
