"""Times the from-states calls of the engine against the bits calls on one GPU, in one process, after a warm-up.

  python scripts/from_states_time.py [--repeats 5] [--states20 32] [--out profiles/from_states.json]

Two things are measured:
  * `expectation_vjp_from_states` against `expectation_vjp` on the same circuit and operator -- what the dense-start
    plans give up (no basis-state first pass, no zero-tile pruning at the head of the forward sweep and the
    tail of the backward sweep) plus the import -- at BASELINE config 2's size (12 qubits, depth-8 HEA, TFIM, 1024
    states) and at 20 qubits (depth-16 HEA, XXZ chain, --states20 states).  The from-states call is given the basis
    states of the same bitstrings, so both calls compute the same numbers.
  * the import alone (csrc/import_states.hip): `statevector_from_states` on a circuit without gates runs nothing else
    in the forward sweep; its time is read from the engine's own events (`profile_events`).  The import reads the
    input twice and writes the workspace once: 24 bytes per amplitude.  The rate is quoted against the 5.5 TB/s the
    project measured for a pass with nothing to compute (csrc/engine.cpp adjoint_plan_seconds).

Prints one JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

from oracle import qhbm_oracle as O  # noqa: E402
from qhbmlib_amd import _engine as E  # noqa: E402

EMPTY_PASS_BYTES_PER_S = 5.5e12   # csrc/engine.cpp adjoint_plan_seconds: a pass with nothing to compute


def timed(fn, repeats):
  """Mean milliseconds of `fn()` over `repeats` runs after two warm-up runs (device events)."""
  for _ in range(2):
    fn()
  torch.cuda.synchronize()
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(repeats):
    fn()
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) / repeats


def basis_states(bits):
  n = bits.shape[1]
  index = (bits.astype(np.int64) << np.arange(n - 1, -1, -1)).sum(1)
  states = torch.zeros((bits.shape[0], 1 << n), dtype=torch.complex64, device="cuda")
  states[torch.arange(bits.shape[0], device="cuda"), torch.from_numpy(index).cuda()] = 1.0
  return states


def compare(n, layers, op, num_states, repeats):
  rng = np.random.default_rng(n)
  gates, names = O.hea_gates(n, layers, "t")
  eng = E.Engine(0)
  eng.set_circuit(n, gates, len(names))
  eng.set_observables([op])
  params = torch.from_numpy(rng.uniform(-1, 1, len(names)).astype(np.float32)).cuda()
  bits_np = rng.integers(0, 2, size=(num_states, n)).astype(np.int8)
  bits = torch.from_numpy(bits_np).cuda()
  upstream = torch.from_numpy(rng.normal(size=(num_states, 1)).astype(np.float32)).cuda()
  states = basis_states(bits_np)
  bits_ms = timed(lambda: eng.expectation_vjp(bits, params, upstream), repeats)
  states_ms = timed(lambda: eng.expectation_vjp_from_states(states, params, upstream), repeats)
  v0, g0 = eng.expectation_vjp(bits, params, upstream)
  v1, g1 = eng.expectation_vjp_from_states(states, params, upstream)
  fwd_bits_ms = timed(lambda: eng.expectation(bits, params), repeats)
  fwd_states_ms = timed(lambda: eng.expectation_from_states(states, params), repeats)
  text = eng.describe_schedule(), eng.describe_schedule_from_states()
  model = [float(t.split("adjoint time model: ")[1].split(" us")[0]) for t in text]
  eng.close()
  return {"n": n, "layers": layers, "states": num_states, "gates": len(gates),
          "vjp_bits_ms": bits_ms, "vjp_from_states_ms": states_ms, "vjp_ratio": states_ms / bits_ms,
          "forward_bits_ms": fwd_bits_ms, "forward_from_states_ms": fwd_states_ms,
          "forward_ratio": fwd_states_ms / fwd_bits_ms,
          "adjoint_model_us_per_state": {"bits": model[0], "from_states": model[1]},
          "max_value_difference": float((v0 - v1).abs().max()), "max_gradient_difference": float((g0 - g1).abs().max())}


def import_alone(n, num_states, repeats):
  eng = E.Engine(0)
  eng.set_circuit(n, [], 0)
  eng.set_option("profile_events", 1)
  rng = np.random.default_rng(1)
  states = torch.from_numpy((rng.normal(size=(num_states, 1 << n)) + 1j * rng.normal(size=(num_states, 1 << n))).astype(np.complex64)).cuda()
  params = torch.zeros((0,), dtype=torch.float32, device="cuda")
  for _ in range(2):
    eng.statevector_from_states(states, params)
  torch.cuda.synchronize()
  eng.kernel_time_ms(reset=True)
  for _ in range(repeats):
    eng.statevector_from_states(states, params)
  torch.cuda.synchronize()
  t = eng.kernel_time_ms(reset=True)
  eng.close()
  ms = t["fwd_ms"] / repeats
  amps = float(num_states) * float(1 << n)
  moved = 24.0 * amps / (ms * 1e-3)
  return {"n": n, "states": num_states, "import_ms": ms, "launches_per_call": t["fwd_launches"] / repeats,
          "bytes_per_amplitude": 24, "bytes_per_s": moved, "input_and_output_once_bytes_per_s": 16.0 * amps / (ms * 1e-3),
          "empty_pass_bytes_per_s": EMPTY_PASS_BYTES_PER_S, "share_of_empty_pass_rate": moved / EMPTY_PASS_BYTES_PER_S}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--states20", type=int, default=32)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  line = {"gpu": torch.cuda.get_device_name(0),
          "config2_size": compare(12, 8, O.tfim_ring_op(12), 1024, args.repeats),
          "n20": compare(20, 16, O.xxz_chain_op(20), args.states20, args.repeats),
          "import": [import_alone(20, 1, args.repeats), import_alone(20, args.states20, args.repeats)]}
  text = json.dumps(line)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
