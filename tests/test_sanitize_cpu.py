"""AddressSanitizer + UndefinedBehaviorSanitizer run of the HOST scheduler.

tests/sanitize/plan_fuzz.cpp plans >= 2,000 random circuits over all twelve gate kinds x tile / relabel / wave-bit /
FULL-threshold options at 3..28 qubits with planning-only engines (no device) and checks every plan structurally:
every lowered micro-op scheduled exactly once, <= 384 gradient slots per adjoint pass and each written once, programs
and tables inside their buffers, cost models finite, a plan rebuilt after gradient-mask changes identical to a
fresh engine's, and the execution order of a batch of shifted programs on every forward plan (schedule.h order_programs: a
permutation, no program behind the pass that reads its gate or behind the first measuring pass, every start pass storing).  csrc/schedule.cpp and csrc/engine.cpp are compiled with -fsanitize=address,undefined (host only; GPU
sanitizers are not available on this pool): any report aborts the run.  A clean log is committed as
profiles/r05_sanitizer_plan_fuzz.txt.

`plan_fuzz --emulate` then EXECUTES plans of the same generator (3..16 qubits, the same option sets, gradient masks, forced
pass orders, measurement tiles, the lean lowering on and off) on a CPU emulator in complex128 that reads programs, records,
thread tables, predicates, physical layouts and fill_args' pruning masks as the kernels do, on poisoned memory, and compares
final states, values and gradients with a dense gate-by-gate oracle (tests/sanitize/plan_emulate.h); the run's per-feature
counts must meet the floors it prints.  Log: profiles/plan_emulation_fuzz.txt."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = os.path.join(ROOT, "tests", "sanitize")
CSRC = os.path.join(ROOT, "qhbm-library_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
FUZZ = os.path.join(SAN, "_build", "plan_fuzz")
EMULATE_CASES, EMULATE_SEED = 360, 20261016
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_fuzz_cases.json")
FIXTURE_CASES, FIXTURE_SEED = 36, 20261016


def _build():
  if not shutil.which(HIPCC):
    pytest.skip("no hipcc")
  # the kernel launchers the engine links against come from the product build (never called here)
  subprocess.run(["make", "kernels.o", "observable.o", "states.o"], cwd=CSRC, check=True, capture_output=True, timeout=1200)
  build = subprocess.run(["make", "-j4"], cwd=SAN, capture_output=True, text=True, timeout=900)
  assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]


@pytest.mark.timeout(1500)
def test_scheduler_under_asan_and_ubsan_on_random_circuits():
  _build()
  env = dict(os.environ, **ENV)
  cases = int(os.environ.get("QHBM_FUZZ_CASES", "2000"))
  run = subprocess.run([FUZZ, str(cases), "20261003"], capture_output=True, text=True,
                       timeout=1200, env=env)
  tail = run.stdout[-1500:] + run.stderr[-3000:]
  assert run.returncode == 0, tail
  assert f"plan_fuzz: {cases} cases" in run.stdout and "plan_fuzz: 0 failures" in run.stdout, tail
  assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, tail
  # the program-order property met what it is about: plans that shared, programs that started behind pass 0
  line = next(l for l in run.stdout.splitlines() if l.startswith("plan_fuzz: program orders"))
  counts = {name: int(count) for name, count in (item.split("=") for item in line.split()[3:])}
  assert set(counts) == {"shared", "programs_behind_pass_0"}, line
  assert counts["shared"] > 0 and counts["programs_behind_pass_0"] > 0, line


@pytest.mark.timeout(1500)
def test_scheduler_plans_emulated_against_dense_oracle():
  """The plans are executed, not only parsed: states, values and gradients of every emulated plan agree with the dense
  oracle within the bars of plan_fuzz.cpp (1e-10; gradients: the float rounding of slot_factor on top), every corruption
  of the self test is accepted by the structural check and rejected by the emulation, and the run exercised every
  feature at least as often as its floor."""
  _build()
  run = subprocess.run([FUZZ, "--emulate", str(EMULATE_CASES), str(EMULATE_SEED)], capture_output=True, text=True, timeout=1200,
                       env=dict(os.environ, **ENV))
  print(run.stdout[-6000:])
  tail = run.stdout[-3000:] + run.stderr[-3000:]
  assert run.returncode == 0, tail
  assert f"plan_emulate: {EMULATE_CASES} cases" in run.stdout and "plan_emulate: 0 failures" in run.stdout, tail
  assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, tail
  assert "corruptions listed, 0 problems" in run.stdout and "ACCEPTED by emulation" not in run.stdout, tail
  assert run.stdout.count("accepted by check_plan, rejected by emulation") == 13, tail
  floors = dict(fwd_multi_pass=400, adj_multi_pass=400, relabel=100, no_zero_fill=100, dense_tail=50, early_measure=100,
                measure_only_pass=50, wht=50, global_terms=30, wide_pass=20, general=200, gate2=100, full=200, cph_tile=200,
                cph_thread=200, dead_mask=50, forced_order=100, grad_mask=200, padded=150)
  line = next(l for l in run.stdout.splitlines() if l.startswith("plan_emulate: features"))
  counts = {}
  for item in line.split()[2:]:
    name, rest = item.split("=")
    count, floor = rest.split("/")
    counts[name] = int(count)
    assert int(floor) == floors[name], (name, floor)  # (the binary prints the floors it was written for)
  assert set(counts) == set(floors), sorted(set(floors) ^ set(counts))
  short = {k: (counts[k], floors[k]) for k in floors if counts[k] < floors[k]}
  assert not short, f"features emulated less often than their floor: {short}"
  # every entry of candidate_orders is rebuilt and emulated: the greedy order (the last entry) has a count of its own
  ranks = next(l for l in run.stdout.splitlines() if l.startswith("plan_emulate: forced orders by entry"))
  greedy, floor = ranks.split("last(greedy)=")[1].split()[0].split("/")
  assert int(floor) == 50 and int(greedy) >= 50, ranks
  by_entry = [int(item.split(":")[1]) for item in ranks.split("candidate_orders")[1].split("last(greedy)")[0].split()]
  assert all(c > 0 for c in by_entry[:4]), ranks  # (the middle entries too)


@pytest.mark.timeout(900)
def test_plan_fuzz_cases_fixture_is_what_the_generator_writes(tmp_path):
  """tests/golden/plan_fuzz_cases.json (the cases tests/test_plan_fuzz_cases_gpu.py runs on the engine) is the output of
  `plan_fuzz --dump-cases`, byte for byte: it cannot drift from the generator."""
  _build()
  out = tmp_path / "cases.json"
  run = subprocess.run([FUZZ, "--dump-cases", str(FIXTURE_CASES), str(FIXTURE_SEED), str(out)], capture_output=True, text=True,
                       timeout=800, env=dict(os.environ, **ENV))
  assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
  with open(out, "rb") as a, open(FIXTURE, "rb") as b:
    assert a.read() == b.read(), "regenerate with: tests/sanitize/_build/plan_fuzz --dump-cases %d %d %s" % (
        FIXTURE_CASES, FIXTURE_SEED, "tests/golden/plan_fuzz_cases.json")
