#!/usr/bin/env python
"""Host cost of one engine call where the host dominates: 10 qubits, one state, one observable.

Wall time per call of `qhbm_expectation` and of `qhbm_expectation_vjp` (adjoint) through the C ABI with preallocated
arguments, over `--calls` calls after a warm-up, one synchronisation at the end; `--repeats` such figures each, so that
two builds can be compared against the spread of either (QHBM_ENGINE_LIB selects the other build's library).  Prints
one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import qhbm_oracle as O  # noqa: E402
from qhbmlib_amd import _engine as E  # noqa: E402


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("--calls", type=int, default=3000)
  ap.add_argument("--warmup", type=int, default=300)
  ap.add_argument("--repeats", type=int, default=5)
  args = ap.parse_args()
  n = 10
  rng = np.random.default_rng(0)
  gates, names = O.hea_gates(n, 2, "host")
  eng = E.Engine(0)
  eng.set_option("workspace_budget_mb", 256)
  eng.set_circuit(n, gates, len(names))
  eng.set_observables([O.xxz_chain_op(n)])
  bits, params = eng._prep(rng.integers(0, 2, size=(1, n)).astype(np.int8), rng.uniform(-1, 1, len(names)))
  up = torch.ones((1, 1), dtype=torch.float32, device=eng.device)
  vals = torch.empty((1, 1), dtype=torch.float32, device=eng.device)
  grad = torch.zeros((len(names),), dtype=torch.float32, device=eng.device)
  lib, h, stream = eng._lib, eng._h, eng._stream()
  b, p, u, v, g = bits.data_ptr(), params.data_ptr(), up.data_ptr(), vals.data_ptr(), grad.data_ptr()
  calls = {
      "expectation": lambda: lib.qhbm_expectation(h, b, 1, p, v, stream),
      "expectation_vjp": lambda: lib.qhbm_expectation_vjp(h, b, 1, p, u, v, g, E.GRAD_ADJOINT, stream),
  }
  out = {}
  for name, call in calls.items():
    us = []
    for _ in range(args.repeats):
      for _ in range(args.warmup):
        eng._check(call())
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      for _ in range(args.calls):
        call()
      torch.cuda.synchronize()
      us.append((time.perf_counter() - t0) / args.calls * 1e6)
    eng._check(call())
    out[name + "_us_per_call"] = [round(x, 3) for x in us]
  print(json.dumps(out))


if __name__ == "__main__":
  main()
