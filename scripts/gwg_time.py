"""Times one draw of GibbsWithGradientsInference -- burn-in plus `--samples` samples -- with the chain on the device
(`chain="device"`, csrc/gwg.hip) against the host chain (`chain="host"`, the reference's loop: autograd through the
energy, a host generator) on one GPU, in one process, after a warm-up.

  python scripts/gwg_time.py --n 20 [--samples 4096] [--burnin 1000] [--host-steps 64] [--out profiles/gwg_chain_n20.json]

The energy is a KOBE-2 over --n bits on the GPU with theta uniform in [-0.1, 0.1] (tests/test_ebm_gpu.py's config-3
model).  The device chain is timed whole (mean of --repeats draws, each a fresh burn-in) with 1, 64 and 1024 chains:
with c chains a draw is burn-in + ceil(samples / c) steps.  The host chain costs several synchronising round trips per
step: it is timed on --host-steps steps after a warm-up and EXTRAPOLATED linearly to burn-in + samples steps (labelled
so).  Prints one JSON line and, with --out, writes it to that file."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

from qhbmlib_amd import inference, models  # noqa: E402

CONFIG3_STEP_MS = 336.0   # README.md, config 3: the VQT step the samples feed


def energy_of(n):
  energy = models.KOBE(list(range(n)), 2).to("cuda")
  torch.manual_seed(0)
  with torch.no_grad():
    energy.post_process[0].kernel.uniform_(-0.1, 0.1)
  return energy


def time_device(n, samples, burnin, chains, repeats):
  layer = inference.GibbsWithGradientsInference(energy_of(n), samples, burnin, initial_seed=1, chain="device",
                                                num_chains=chains)
  layer.sample(samples)   # warm-up: library load, the LDS opt-in, the first burn-in
  torch.cuda.synchronize()
  total = 0.0
  for _ in range(repeats):
    t0 = time.perf_counter()
    layer._ready_inference()   # pylint: disable=protected-access  (a variable update triggers exactly this)
    out = layer.sample(samples)
    torch.cuda.synchronize()
    total += time.perf_counter() - t0
  steps = burnin + -(-samples // chains)
  ms = total * 1e3 / repeats
  return {"chains": chains, "steps_per_draw": steps, "draw_ms": ms, "us_per_step": ms * 1e3 / steps,
          "distinct_samples": int(torch.unique(out, dim=0).shape[0])}


def time_host(n, samples, burnin, host_steps):
  layer = inference.GibbsWithGradientsInference(energy_of(n), samples, 0, initial_seed=1, chain="host")
  layer.sample(8)   # warm-up
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  layer.sample(host_steps)
  torch.cuda.synchronize()
  per_step = (time.perf_counter() - t0) / host_steps
  return {"timed_steps": host_steps, "ms_per_step": per_step * 1e3,
          "draw_ms_extrapolated": per_step * 1e3 * (burnin + samples),
          "note": f"linear extrapolation from {host_steps} timed steps to {burnin + samples}"}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--n", type=int, default=20)
  ap.add_argument("--samples", type=int, default=4096)
  ap.add_argument("--burnin", type=int, default=1000)
  ap.add_argument("--host-steps", type=int, default=64)
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  device = [time_device(args.n, args.samples, args.burnin, c, args.repeats) for c in (1, 64, 1024)]
  host = time_host(args.n, args.samples, args.burnin, args.host_steps)
  line = {"n": args.n, "energy": "kobe2", "terms": args.n + args.n * (args.n - 1) // 2, "samples": args.samples,
          "burnin": args.burnin, "gpu": torch.cuda.get_device_name(0), "device": device, "host": host,
          "speedup_one_chain": host["draw_ms_extrapolated"] / device[0]["draw_ms"],
          "config3_step_ms": CONFIG3_STEP_MS, "device_draw_below_config3_step": device[0]["draw_ms"] < CONFIG3_STEP_MS}
  text = json.dumps(line)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
