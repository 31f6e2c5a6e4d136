"""Times streamed Lanczos (`qhbm_krylov_tridiagonal`, `qhbm_krylov_replay`) against the stored local route on one
GPU, both routes alternated in one process after a warm-up of every shape.

  python scripts/krylov_stream_time.py [--qubits 20] [--vectors 16] [--steps 64] [--repeats 4] [--large-qubits 24]
                                       [--out profiles/krylov_stream.json]

Workload: TFIM ring, `--vectors` random-sign vectors, `--steps` Lanczos steps.  Reported, not asserted:
  * at `--qubits` (20 / 16 / 64: the stored basis is 8 GiB): `krylov_basis(reorthogonalise=False)` against `krylov_tridiagonal`,
    device events around each call, the two alternated `--repeats` times (every time listed, and the median); pass one
    followed by a replay of S = 1 and of S = 8 outputs; the replay's own sweeps (import, subtract, scaled copy with
    accumulate: the engine's `profile_events`, in a run of their own) and their bytes -- by the model
    `describe_krylov_stream` reports -- per second, as a share of the 8 TB/s peak: memory-bound kernels, so bytes over
    bandwidth is the bound;
  * at `--large-qubits` (24: a stored basis would be 128 GiB), streamed only: the bytes the engine holds during the pass
    (`allocated_bytes`), what torch holds at its peak and what the device reports used; wall clock of
    `thermal_sweep(store_basis=False)`; the largest |log Z difference| against `thermal_ensemble` on the same vectors at
    `--beta`;
  * the shader clock the box ran at (`clock_probe`).
Every figure is from one run on one box.

Prints one JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

from oracle import qhbm_oracle as O  # noqa: E402
from qhbmlib_amd import _engine as E  # noqa: E402
from qhbmlib_amd import inference, ir  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12


def tfim_sum(n):
  qubits = ir.GridQubit.rect(1, n)
  terms = [ir.PauliString(ir.PX(q), coefficient=-1.0) for q in qubits]
  terms += [ir.PauliString(ir.PZ(qubits[i]), ir.PZ(qubits[(i + 1) % n]), coefficient=-1.0) for i in range(n)]
  return ir.PauliSum(terms)


def event_ms(fn):
  begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  begin.record()
  out = fn()
  end.record()
  torch.cuda.synchronize()
  return out, begin.elapsed_time(end)


def wall_ms(fn):
  torch.cuda.synchronize()
  start = time.perf_counter()
  out = fn()
  torch.cuda.synchronize()
  return out, 1e3 * (time.perf_counter() - start)


def summary(times):
  return {"ms": [float(t) for t in times], "median_ms": float(statistics.median(times))}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--qubits", type=int, default=20)
  ap.add_argument("--vectors", type=int, default=16)
  ap.add_argument("--steps", type=int, default=64)
  ap.add_argument("--repeats", type=int, default=4)
  ap.add_argument("--large-qubits", type=int, default=24)
  ap.add_argument("--beta", type=float, default=1.0)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  n, num, m = args.qubits, args.vectors, args.steps
  eng = E.Engine(0)
  eng.set_circuit(n, [], 0)
  eng.set_observables([O.tfim_ring_op(n)])
  clock = eng.clock_probe()
  starts = E.random_states(num, n, 1, device="cuda:0")
  line = {"gpu": torch.cuda.get_device_name(0), "clock_ghz": clock["ghz"], "qubits": n, "vectors": num, "steps": m,
          "operator": "tfim_ring", "one_run_on_one_box": True, "repeats": args.repeats}
  rng = np.random.default_rng(0)
  coefs = {s: torch.from_numpy((rng.normal(size=(num, s, m)) + 1j * rng.normal(size=(num, s, m))).astype(np.complex64)).cuda()
           for s in (1, 8)}

  # warm-up of every shape: the workspace, the ring, the caching allocator's 8 GiB, every kernel's code object
  eng.set_option("profile_events", 0)
  stored = eng.krylov_basis(starts, m, None, False)
  one = eng.krylov_tridiagonal(starts, m)
  for s in (1, 8):
    eng.krylov_replay(starts, one[1], one[2], one[3], coefs[s])
  torch.cuda.synchronize()
  line["same_t"] = bool(torch.equal(stored[1], one[0]) and torch.equal(stored[2], one[1]) and torch.equal(stored[3], one[2]))
  combined = E.krylov_combine(stored[0], coefs[8])
  line["max_abs_replay_minus_combine"] = float((eng.krylov_replay(starts, one[1], one[2], one[3], coefs[8]) - combined).abs().max())
  del stored, combined
  times = {"stored_local": [], "tridiagonal": [], "tridiagonal_and_replay_1": [], "tridiagonal_and_replay_8": []}
  for _ in range(args.repeats):  # the routes alternate inside every repeat
    times["stored_local"].append(event_ms(lambda: eng.krylov_basis(starts, m, None, False))[1])
    times["tridiagonal"].append(event_ms(lambda: eng.krylov_tridiagonal(starts, m))[1])
    for s in (1, 8):
      def both(s=s):
        got = eng.krylov_tridiagonal(starts, m)
        return eng.krylov_replay(starts, got[1], got[2], got[3], coefs[s])
      times[f"tridiagonal_and_replay_{s}"].append(event_ms(both)[1])
  line["routes"] = {key: summary(value) for key, value in times.items()}
  line["routes"]["tridiagonal_over_stored_local"] = line["routes"]["tridiagonal"]["median_ms"] / line["routes"]["stored_local"]["median_ms"]
  line["stored_basis_bytes"] = eng.describe_krylov(num, m, False)["basis_bytes"]

  # the replay's own sweeps by the engine's events, in a run of their own (events around every launch slow the host)
  eng.set_option("profile_events", 1)
  line["replay_kernels"] = {}
  for s in (1, 8):
    model = eng.describe_krylov_stream(num, m, s)
    eng.kernel_time_ms(reset=True)
    for _ in range(args.repeats):
      eng.krylov_replay(starts, one[1], one[2], one[3], coefs[s])
    torch.cuda.synchronize()
    events = eng.kernel_time_ms(reset=True)
    sweeps_ms, obs_ms = events["fwd_ms"] / args.repeats, events["obs_ms"] / args.repeats
    moved = model["replay_bytes_per_state"] * num
    line["replay_kernels"][f"S={s}"] = {"sweeps_ms": sweeps_ms, "observable_ms": obs_ms, "model_bytes": moved,
                                        "bytes_per_s": moved / (sweeps_ms * 1e-3),
                                        "share_of_8TBps": moved / (sweeps_ms * 1e-3) / PEAK_BYTES_PER_S,
                                        "applications": model["replay_applications"]}
  line["workspace_bytes"] = eng.describe_krylov_stream(num, m, 1)["workspace_bytes"]
  eng.close()
  del starts, one, coefs
  torch.cuda.empty_cache()

  # ---- the large case: streamed only ----
  big = args.large_qubits
  if big > 0:
    ham = tfim_sum(big)
    free_before, total = torch.cuda.mem_get_info()
    torch.cuda.reset_peak_memory_stats()
    eng = E.Engine(0)
    eng.set_circuit(big, [], 0)
    eng.set_observables([O.tfim_ring_op(big)])
    starts = E.random_states(num, big, 1, device="cuda:0")
    (alpha, beta, lengths, recurrence, _), first_ms = event_ms(lambda: eng.krylov_tridiagonal(starts, m))
    held = eng.allocated_bytes()
    free_during, _ = torch.cuda.mem_get_info()
    _, again_ms = event_ms(lambda: eng.krylov_tridiagonal(starts, m))
    coef = torch.zeros((num, 1, m), dtype=torch.complex64)
    coef[:, 0, 0] = 1
    _, replay_ms = event_ms(lambda: eng.krylov_replay(starts, beta, lengths, recurrence, coef))
    large = {"qubits": big, "stored_basis_bytes_if_stored": float(m) * num * 8.0 * 2.0**big,
             "start_states_bytes": float(num) * 8.0 * 2.0**big, "engine_allocated_bytes": float(held),
             "model_workspace_bytes": eng.describe_krylov_stream(num, m, 1)["workspace_bytes"],
             "torch_peak_allocated_bytes": float(torch.cuda.max_memory_allocated()),
             "device_used_bytes_during": float(free_before - free_during), "device_total_bytes": float(total),
             "tridiagonal_first_call_ms": first_ms, "tridiagonal_ms": again_ms, "replay_1_ms": replay_ms}
    eng.close()
    del starts, alpha, beta, lengths, recurrence
    torch.cuda.empty_cache()
    sweep, large["thermal_sweep_streamed_wall_ms"] = wall_ms(
        lambda: inference.thermal_sweep(ham, [args.beta], num_vectors=num, num_steps=m, seed=1, store_basis=False))
    log_z = float(sweep.log_partition()[0])
    del sweep
    torch.cuda.empty_cache()
    cheb, large["thermal_ensemble_wall_ms"] = wall_ms(lambda: inference.thermal_ensemble(ham, args.beta, num_vectors=num, seed=1))
    large.update(beta=args.beta, log_z_streamed=log_z, log_z_thermal_ensemble=float(cheb.log_partition()),
                 abs_log_z_difference=abs(log_z - float(cheb.log_partition())))
    line["large"] = large
  text = json.dumps(line)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
