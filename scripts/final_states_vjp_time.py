"""Times the adjoint VJP of final states from a caller's cotangent (`statevector_vjp_from_states`) against
`expectation_vjp_from_states` with ONE observable on the same circuit and states, on one GPU, in one process.

  python scripts/final_states_vjp_time.py [--repeats 5] [--rounds 3] [--out profiles/final_states_vjp.json]

The two routes differ in how lambda is made -- a streaming pass over (cotangent, final state) against lambda = O psi --
and in one small kernel for the global-phase term; forward and backward sweeps are the same.  They are timed ALTERNATELY
(`--rounds` rounds of `--repeats` calls each, after two warm-up calls per route; device events) at 20 qubits with 8 states
and 24 qubits with 2 states, depth-16 HEA, XXZ chain.  The cotangent is 2 upstream O psi of the observable route, so
both compute the same gradient; their largest difference is reported.

The import kernel alone (csrc/cotangent.hip) is read from the engine's own events (`profile_events`: the cotangent import
is booked as the lambda launch, its small finishing kernel included): it reads 16 bytes and writes 8 per amplitude, and
the rate is quoted against the MI355X's 8 TB/s HBM peak.

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

HBM_PEAK_BYTES_PER_S = 8e12


def _window(fn, repeats):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(repeats):
    fn()
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) / repeats


def compare(n, layers, num_states, repeats, rounds):
  rng = np.random.default_rng(n)
  gates, names = O.hea_gates(n, layers, "t")
  op = O.xxz_chain_op(n)
  with_op, bare = E.Engine(0), E.Engine(0)
  for eng in (with_op, bare):
    eng.set_circuit(n, gates, len(names))
  with_op.set_observables([op])
  params = torch.from_numpy(rng.uniform(-1, 1, len(names)).astype(np.float32)).cuda()
  states = torch.randn((num_states, 1 << n), dtype=torch.complex64, device="cuda", generator=torch.Generator("cuda").manual_seed(n))
  states /= states.abs().pow(2).sum(1, keepdim=True).sqrt()
  upstream = torch.from_numpy(rng.normal(size=(num_states, 1)).astype(np.float32)).cuda()
  # the cotangent of sum_u upstream_u <psi_u|O|psi_u>: 2 upstream O psi, from the engine's own lambda = O psi kernels
  final = bare.statevector_from_states(states, params)
  cotangent = 2.0 * upstream.to(torch.complex64) * with_op.apply_observables(final)
  del final

  observable = lambda: with_op.expectation_vjp_from_states(states, params, upstream)
  cotangent_route = lambda: bare.statevector_vjp_from_states(states, params, cotangent)
  for fn in (observable, cotangent_route, observable, cotangent_route):  # warm-up: plans, uploads, workspaces
    fn()
  torch.cuda.synchronize()
  obs_ms, cot_ms = [], []
  for _ in range(rounds):
    obs_ms.append(_window(observable, repeats))
    cot_ms.append(_window(cotangent_route, repeats))
  _, g_obs = observable()
  g_cot = cotangent_route()
  # the import kernel alone, from the engine's events
  bare.set_option("profile_events", 1)
  cotangent_route()
  torch.cuda.synchronize()
  bare.kernel_time_ms(reset=True)
  for _ in range(repeats):
    cotangent_route()
  torch.cuda.synchronize()
  t = bare.kernel_time_ms(reset=True)
  import_ms = t["obs_ms"] / repeats
  moved = 24.0 * float(num_states) * float(1 << n)
  for eng in (with_op, bare):
    eng.close()
  obs, cot = float(np.median(obs_ms)), float(np.median(cot_ms))
  return {"n": n, "layers": layers, "states": num_states, "gates": len(gates),
          "observable_route_ms": obs, "cotangent_route_ms": cot, "ratio": cot / obs,
          "observable_route_ms_rounds": obs_ms, "cotangent_route_ms_rounds": cot_ms,
          "max_gradient_difference": float((g_obs - g_cot).abs().max()), "gradient_inf_norm": float(g_obs.abs().max()),
          "import": {"ms": import_ms, "launches_per_call": t["obs_launches"] / repeats, "bytes_per_amplitude": 24,
                     "bytes_per_s": moved / (import_ms * 1e-3), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
                     "share_of_hbm_peak": moved / (import_ms * 1e-3) / HBM_PEAK_BYTES_PER_S,
                     "share_of_cotangent_route": import_ms / cot},
          "sweep_ms_per_call": {"forward": t["fwd_ms"] / repeats, "backward": t["bwd_ms"] / repeats}}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("final_states_vjp_time.py needs a GPU: the engine has no CPU fallback")
  line = {"gpu": torch.cuda.get_device_name(0),
          "n20": compare(20, 16, 8, args.repeats, args.rounds),
          "n24": compare(24, 16, 2, args.repeats, args.rounds)}
  text = json.dumps(line)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
