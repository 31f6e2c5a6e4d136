"""Times the Krylov engine (`qhbm_krylov_basis`, `inference.thermal_sweep`) on one GPU, in one process, after a warm-up.

  python scripts/krylov_time.py [--qubits 20] [--vectors 16] [--steps 64] [--repeats 2] [--out profiles/krylov_time.json]

Workload: TFIM ring, `--qubits` qubits, `--vectors` random-sign vectors, `--steps` Lanczos steps (20 / 16 / 64: a basis of
8 GiB).  Reported, not asserted:
  * per reorthogonalisation mode: total time of `krylov_basis` (device events around it) and time per step, split by the
    engine's own events (`profile_events`) into the lambda = O psi launches and the project / subtract / normalise
    kernels (with the import), and the latter's bytes -- by the model `describe_krylov` reports -- per second, as a
    fraction of 8 TB/s;
  * an 8-rung ladder, beta = 0.25 .. 2: one `thermal_sweep` (the basis, the Ritz pairs, log Z, <H> and S of all rungs; once
    per mode) against eight `thermal_ensemble` calls, wall clock around each route (engine construction and workspace
    allocation included, as a user pays them), and the largest |log Z difference| between the routes on the same
    random vectors;
  * the shader clock the box ran at (`clock_probe`).
Every figure is from one run on one box.

Prints one JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
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


def wall_ms(fn):
  torch.cuda.synchronize()
  start = time.perf_counter()
  out = fn()
  torch.cuda.synchronize()
  return out, 1e3 * (time.perf_counter() - start)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--qubits", type=int, default=20)
  ap.add_argument("--vectors", type=int, default=16)
  ap.add_argument("--steps", type=int, default=64)
  ap.add_argument("--repeats", type=int, default=2)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  n, num, m = args.qubits, args.vectors, args.steps
  eng = E.Engine(0)
  eng.set_circuit(n, [], 0)
  eng.set_observables([O.tfim_ring_op(n)])
  clock = eng.clock_probe()
  starts = E.random_states(num, n, 1, device="cuda:0")
  line = {"gpu": torch.cuda.get_device_name(0), "clock_ghz": clock["ghz"], "qubits": n, "vectors": num, "steps": m,
          "operator": "tfim_ring", "one_run_on_one_box": True}
  for name, reorth in (("full", True), ("local", False)):
    model = eng.describe_krylov(num, m, reorth)
    eng.set_option("profile_events", 0)
    eng.krylov_basis(starts, m, None, reorth)  # warm-up: the workspace, the caching allocator's 8 GiB
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    for _ in range(args.repeats):
      eng.krylov_basis(starts, m, None, reorth)
    end.record()
    torch.cuda.synchronize()
    total_ms = begin.elapsed_time(end) / args.repeats
    eng.set_option("profile_events", 1)
    eng.kernel_time_ms(reset=True)
    for _ in range(args.repeats):
      eng.krylov_basis(starts, m, None, reorth)
    torch.cuda.synchronize()
    events = eng.kernel_time_ms(reset=True)
    krylov_ms, obs_ms = events["fwd_ms"] / args.repeats, events["obs_ms"] / args.repeats
    moved = model["krylov_bytes_per_state"] * num
    line[name] = {"total_ms": total_ms, "ms_per_step": total_ms / m, "observable_ms": obs_ms, "observable_ms_per_step": obs_ms / m,
                  "krylov_kernels_ms": krylov_ms, "krylov_kernels_ms_per_step": krylov_ms / m,
                  "krylov_model_bytes": moved, "krylov_bytes_per_s": moved / (krylov_ms * 1e-3),
                  "krylov_share_of_8TBps": moved / (krylov_ms * 1e-3) / PEAK_BYTES_PER_S,
                  "basis_bytes": model["basis_bytes"], "workspace_bytes": model["workspace_bytes"]}
  eng.close()
  del starts
  torch.cuda.empty_cache()

  ham, betas, seed = tfim_sum(n), np.linspace(0.25, 2.0, 8), 1
  inference.thermal_ensemble(ham, 0.25, num_vectors=num, seed=seed)  # warm-up of the Chebyshev route
  inference.thermal_sweep(ham, betas[:1], num_vectors=num, num_steps=m, seed=seed)  # ... and of this one
  torch.cuda.empty_cache()

  def ladder_sweep(reorth=True):
    sweep = inference.thermal_sweep(ham, betas, num_vectors=num, num_steps=m, seed=seed, reorthogonalise=reorth)
    return sweep.log_partition(), sweep.energy(), sweep.entropy()

  def ladder_chebyshev():
    return np.array([float(inference.thermal_ensemble(ham, float(b), num_vectors=num, seed=seed).log_partition()) for b in betas])

  (sweep_log_z, _, _), sweep_ms = wall_ms(ladder_sweep)
  torch.cuda.empty_cache()
  (local_log_z, _, _), local_ms = wall_ms(lambda: ladder_sweep(False))
  torch.cuda.empty_cache()
  cheb_log_z, cheb_ms = wall_ms(ladder_chebyshev)
  line["ladder"] = {"betas": [float(b) for b in betas], "thermal_sweep_ms": sweep_ms, "thermal_sweep_local_ms": local_ms,
                    "eight_thermal_ensembles_ms": cheb_ms, "speedup": cheb_ms / sweep_ms, "speedup_local": cheb_ms / local_ms,
                    "max_abs_log_z_difference": float(np.abs(sweep_log_z - cheb_log_z).max()),
                    "max_abs_log_z_difference_local": float(np.abs(local_log_z - cheb_log_z).max()),
                    "log_z_sweep": [float(v) for v in sweep_log_z]}
  text = json.dumps(line)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
