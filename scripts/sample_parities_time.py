"""Times `Engine.sample_parities` (qhbm_sample_parities) on one GPU, in one process, against what the tree
did for the same estimate before it: `Engine.sample` (materialised int8 shots) plus the float32 mask matmul of
`SampledQuantumInference._pauli_estimator`.

  python scripts/sample_parities_time.py [--rounds 5] [--step-limit 300] [--out profiles/sample_parities.json]

Workload: a depth-1 hardware-efficient circuit (X and Z powers on every qubit, two layers of CZ powers) on U random basis
states, one unshifted program, T random Z-string masks:
  (n = 20, U = 8, T = 57, shots 10^5 and 10^6) and (n = 24, U = 2, T = 210, shots 10^6).
Per case both routes are warmed up once, then run ALTERNATELY for `--rounds` rounds; a round of a route is a window of
as many calls as fill 50 ms (sized from the warm-up, at most 200) between a device synchronise and the next (host clock),
reported per call: the median, the least and the largest window of each route, and the peak
of `torch.cuda.max_memory_allocated` over a call of each route (reset before it; the engine's own workspace comes from
hipMalloc and is not in that figure for either route).  The two estimates of the warm-up are compared: with one seed both
routes take the same uniform per shot (program 0), so they differ only by the shots that the fp32 scan inside a block of
`draw_kernel` places elsewhere than the float64 table does -- far below the shot noise 1 / sqrt(shots); the largest
difference is reported.
Reported, not asserted: one run on one box.  Each step runs under a watchdog of `--step-limit` seconds that ends the
process.  Prints one JSON line and, with --out, writes it to that file."""
import argparse
import faulthandler
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

from qhbmlib_amd import _engine as E  # noqa: E402

CASES = ((20, 8, 57, 10**5), (20, 8, 57, 10**6), (24, 2, 210, 10**6))


class Step:
  """A watchdog around one step: the process exits (with every thread's traceback) when it runs past the limit."""

  def __init__(self, name, limit):
    self.name, self.limit = name, limit

  def __enter__(self):
    print(f"[sample_parities_time] {self.name}", file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(self.limit, exit=True)

  def __exit__(self, *exc):
    faulthandler.cancel_dump_traceback_later()
    return False


def hea(n):
  """(kind, q0, q1, param_idx, scalar, offset) of one hardware-efficient layer; every gate has its own parameter."""
  gates = []
  for q in range(n):
    gates.append((E.GATE_XPOW, q, -1, len(gates), 1.0, 0.0))
    gates.append((E.GATE_ZPOW, q, -1, len(gates), 1.0, 0.0))
  for first in (0, 1):
    for q in range(first, n - 1, 2):
      gates.append((E.GATE_CZPOW, q, q + 1, len(gates), 1.0, 0.0))
  return gates


WINDOW_MS = 50.0
MAX_CALLS = 200


def timed(fn, calls=1):
  """Milliseconds per call over a window of `calls` calls that ends in a device synchronise."""
  torch.cuda.synchronize()
  begin = time.perf_counter()
  for _ in range(calls):
    out = fn()
  torch.cuda.synchronize()
  del out
  return (time.perf_counter() - begin) * 1e3 / calls


def peak_bytes(fn):
  torch.cuda.synchronize()
  torch.cuda.reset_peak_memory_stats()
  base = torch.cuda.memory_allocated()
  out = fn()
  torch.cuda.synchronize()
  del out
  return int(torch.cuda.max_memory_allocated() - base)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=5)
  ap.add_argument("--step-limit", type=int, default=300)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  line = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_ms": WINDOW_MS, "one_run_on_one_box": True,
          "cases": []}

  def flush():
    text = json.dumps(line)
    if args.out:
      with open(args.out, "w") as f:
        f.write(text + "\n")
    return text

  for n, num, n_masks, shots in CASES:
    rng = np.random.default_rng(n * 1000 + n_masks)
    gates = hea(n)
    params = rng.uniform(0.1, 0.9, len(gates)).astype(np.float32)
    bits = rng.integers(0, 2, size=(num, n)).astype(np.int8)
    masks = np.array([int(rng.integers(1, 1 << n)) for _ in range(n_masks)], np.uint64)
    # the mask matrix of _pauli_estimator: [T, n] float32, column q = qubit q
    rows = torch.tensor([[(int(m) >> q) & 1 for q in range(n)] for m in masks], dtype=torch.float32, device="cuda")
    eng = E.Engine(0)
    eng.set_circuit(n, gates, len(gates))

    def parities(seed=1):
      return eng.sample_parities(bits, params, masks, shots, seed).to(torch.float32)[0] / float(shots)      # [U, T]

    def outcomes(seed=1):
      drawn = eng.sample(bits, params, shots, seed)                                                         # [U, shots, n] int8
      ones = torch.matmul(drawn.to(torch.float32), rows.t())                                                # [U, shots, T]
      return (1.0 - 2.0 * torch.remainder(ones, 2.0)).mean(1)

    with Step(f"n={n} U={num} T={n_masks} shots={shots}: warm-up", args.step_limit):
      a, b = parities(), outcomes()
      torch.cuda.synchronize()
      difference = float((a - b).abs().max())
      del a, b
    routes = (("parities", parities), ("outcomes", outcomes))
    with Step(f"n={n} U={num} T={n_masks} shots={shots}: window sizes", args.step_limit):
      calls = {name: int(min(MAX_CALLS, max(1, WINDOW_MS / max(timed(fn), 1e-3)))) for name, fn in routes}
    times = {"parities": [], "outcomes": []}
    with Step(f"n={n} U={num} T={n_masks} shots={shots}: {args.rounds} alternating rounds", args.step_limit):
      for r in range(args.rounds):
        for name, fn in routes:
          times[name].append(timed(lambda: fn(2 + r), calls[name]))
    with Step(f"n={n} U={num} T={n_masks} shots={shots}: peak memory", args.step_limit):
      peaks = {"parities": peak_bytes(parities), "outcomes": peak_bytes(outcomes)}
    row = {"qubits": n, "states": num, "masks": n_masks, "shots": shots, "max_abs_difference_of_estimates": difference,
           "shot_noise_scale": 1.0 / float(np.sqrt(shots))}
    for name in ("parities", "outcomes"):
      row[name] = {"median_ms": statistics.median(times[name]), "min_ms": min(times[name]), "max_ms": max(times[name]),
                   "all_ms": times[name], "calls_per_window": calls[name], "peak_torch_bytes": peaks[name]}
    row["outcomes_over_parities_median"] = row["outcomes"]["median_ms"] / row["parities"]["median_ms"]
    line["cases"].append(row)
    flush()
    del eng, rows
    torch.cuda.empty_cache()
  print(flush())


if __name__ == "__main__":
  main()
