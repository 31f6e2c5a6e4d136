"""Times the thermal-state construction of `qhbm_evolve_states` on one GPU, in one process, after a warm-up.

  python scripts/thermal_time.py [--qubits 20] [--beta 1.0] [--vectors 16] [--repeats 3] [--out profiles/thermal_time.json]

Workload: TFIM ring, `--qubits` qubits, `--vectors` random-sign vectors, e^{-beta H / 2} on each (what
`inference.thermal_ensemble(H, beta)` runs).  Reported, not asserted:
  * total time of the call (device events around it) and time per H-application (total / (steps x terms per step));
  * the share spent in `cheb_step_kernel`, from the engine's own events (`profile_events`: in an evolve call the
    recurrence's sweeps are the forward launches, the lambda = O psi launches the observable launches);
  * that kernel's bytes / time as a fraction of 8 TB/s: it reads three and writes two state-sized buffers per term,
    40 bytes per amplitude (the first term of a step reads two: 32);
  * in the same run, the bare lambda = O psi launch on the same states (`apply_observables`), so that the overhead of
    the recurrence is a ratio of two numbers from one box;
  * the shader clock the box ran at (`clock_probe`).

Prints one JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

from oracle import qhbm_oracle as O  # noqa: E402
from qhbmlib_amd import _engine as E  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def timed(fn, repeats):
  """Mean milliseconds of `fn()` over `repeats` runs after one warm-up run (device events)."""
  fn()
  torch.cuda.synchronize()
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(repeats):
    fn()
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) / repeats


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--qubits", type=int, default=20)
  ap.add_argument("--beta", type=float, default=1.0)
  ap.add_argument("--vectors", type=int, default=16)
  ap.add_argument("--repeats", type=int, default=3)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  n, tau = args.qubits, 0.5 * args.beta
  eng = E.Engine(0)
  eng.set_circuit(n, [], 0)
  eng.set_observables([O.tfim_ring_op(n)])
  clock = eng.clock_probe()
  plan = eng.describe_evolution(tau, 0)
  starts = E.random_states(args.vectors, n, 1, device="cuda:0")
  work = starts.clone()

  def evolve():
    work.copy_(starts)
    eng.evolve_states(work, tau, 0, in_place=True)

  total_ms = timed(evolve, args.repeats)
  copy_ms = timed(lambda: work.copy_(starts), args.repeats)
  apply_ms = timed(lambda: eng.apply_observables(starts), args.repeats)
  eng.set_option("profile_events", 1)
  evolve()
  torch.cuda.synchronize()
  eng.kernel_time_ms(reset=True)
  for _ in range(args.repeats):
    evolve()
  torch.cuda.synchronize()
  events = eng.kernel_time_ms(reset=True)
  eng.close()
  cheb_ms, obs_ms = events["fwd_ms"] / args.repeats, events["obs_ms"] / args.repeats
  amps = float(args.vectors) * float(1 << n)
  cheb_bytes = amps * (40.0 * plan["applications"] - 8.0 * plan["steps"])
  evolve_ms = total_ms - copy_ms
  line = {"gpu": torch.cuda.get_device_name(0), "clock_ghz": clock["ghz"], "qubits": n, "beta": args.beta, "vectors": args.vectors,
          "operator": "tfim_ring", "R": plan["R"], "steps": plan["steps"], "terms_per_step": plan["terms_per_step"],
          "applications": plan["applications"], "total_ms": evolve_ms, "ms_per_application": evolve_ms / plan["applications"],
          "cheb_step_ms": cheb_ms, "cheb_step_launches": events["fwd_launches"] / args.repeats,
          "cheb_step_share": cheb_ms / evolve_ms, "cheb_step_bytes_per_s": cheb_bytes / (cheb_ms * 1e-3),
          "cheb_step_share_of_8TBps": cheb_bytes / (cheb_ms * 1e-3) / PEAK_BYTES_PER_S,
          "observable_ms_in_call": obs_ms, "observable_ms_per_application": obs_ms / plan["applications"],
          "bare_apply_ms": apply_ms, "application_over_bare_apply": (evolve_ms / plan["applications"]) / apply_ms}
  text = json.dumps(line)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
