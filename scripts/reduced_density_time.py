"""Times the reduced-density kernels (`qhbm_reduced_density`) on one GPU, in one process, against the only route the tree
offered before them.

  python scripts/reduced_density_time.py [--repeats 3] [--step-limit 120] [--out profiles/reduced_density.json]

Reported, not asserted (every figure is from one run on one box):
  * streaming: the rate the project's own streaming kernel reaches in this process -- `krylov_combine` with one row and one
    output (one 16-byte read and one write per word) -- and a device-to-device `copy_`, as scripts/state_metrics_time.py
    takes them;
  * kernel: time of one `qhbm_reduced_density` (device events around a window of calls after a warm-up, through the C ABI with
    scratch and output allocated outside) at n in {20, 24}, k in {1, 4, 8, 10}, M in {1, 8}, for three masks: the k highest qubits (the environment is
    the low index bits), the k lowest (the kept bits are the low index bits) and k qubits spread evenly over the register.
    Bytes by the model 8 M 2^n x (tile rows = max(1, 2^(k-6))): every tile reads its row panel and, off the diagonal, its
    column panel once.  Fused multiply-adds as executed: 4 per output, environment value and launched tile;
  * binding: the same call through `_engine.reduced_density`, which allocates its scratch and output per call -- the
    like-for-like partner of the next figure;
  * gram_route: the same matrix through `permute(...).contiguous()` of each state (runs of neighbouring qubits of one kind
    merged into one axis) and `weighted_gram` on its [2^k, 2^(n-k)] view, conjugated, the weights applied and the states
    added on the host side of the call in float64 -- and the largest entrywise difference between the two results.
A timed window is at least 20 ms long (up to 400 calls), sized from one timed call after a warm-up; the routes are not
alternated and no spread is taken, so differences of a few per cent between two figures mean nothing.  The gram route runs
about seven launches and several allocations per state from python: at 20 qubits it is bound by that host work (some 40
microseconds per state), not by the GPU, and its ratio to the raw kernel time says so, not how the kernels compare.  The
20-qubit streaming figure moves 128 MiB, which the Infinity Cache holds: it is not an HBM rate.
Each step runs under a watchdog of `--step-limit` seconds that ends the process (nothing more is started on the GPU after
a step that hangs).  Prints one JSON line and, with --out, writes it to that file."""
import argparse
import faulthandler
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

from qhbmlib_amd import _engine as E  # noqa: E402

MAX_COPY_DIMS = 16  # torch's strided copy on the device refuses tensors of more dimensions


class Step:
  """A watchdog around one step: the process exits (with every thread's traceback) when it runs past the limit."""

  def __init__(self, name, limit):
    self.name, self.limit = name, limit

  def __enter__(self):
    print(f"[reduced_density_time] {self.name}", file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(self.limit, exit=True)

  def __exit__(self, *exc):
    faulthandler.cancel_dump_traceback_later()
    return False


WINDOW_MS = 20.0   # a timed window is at least this long (and at least `repeats` calls, at most MAX_CALLS)
MAX_CALLS = 400


def event_ms(fn, repeats):
  """Mean time of one call over a window of at least WINDOW_MS: a warm-up call, one timed call to size the window."""
  def window(calls):
    torch.cuda.synchronize()
    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    begin.record()
    for _ in range(calls):
      fn()
    end.record()
    torch.cuda.synchronize()
    return begin.elapsed_time(end) / calls
  fn()  # warm-up
  first = window(1)
  return window(int(min(MAX_CALLS, max(repeats, WINDOW_MS / max(first, 1e-3)))))


def kept_qubits(n, k, kind):
  if kind == "high":    # the k most significant index bits
    return list(range(k))
  if kind == "low":     # the k least significant index bits
    return list(range(n - k, n))
  return sorted({(2 * i + 1) * n // (2 * k) for i in range(k)})  # spread evenly


def gram_route(states, kept, weights):
  """rho_A through permute + contiguous + weighted_gram, per state; complex128 [2^k, 2^k] on the device."""
  num, dim = states.shape
  n = dim.bit_length() - 1
  k = len(kept)

  def runs_of(first, last):
    """[(kept?, length)] of the qubits first..last-1: neighbours of one kind become one axis."""
    runs = []
    for q in range(first, last):
      keep = q in kept
      if runs and runs[-1][0] == keep:
        runs[-1][1] += 1
      else:
        runs.append([keep, 1])
    return runs

  def gather(state):
    runs = runs_of(0, n)
    if len(runs) <= MAX_COPY_DIMS:
      order = [i for i, (keep, _) in enumerate(runs) if keep] + [i for i, (keep, _) in enumerate(runs) if not keep]
      return state.reshape([1 << length for _, length in runs]).permute(order).contiguous()
    # more axes than a strided copy takes: the low half of the qubits first, then the high half (two copies)
    half = n // 2
    low, high = runs_of(half, n), runs_of(0, half)
    kept_low = sum(length for keep, length in low if keep)
    order = [0] + [1 + i for i, (keep, _) in enumerate(low) if keep] + [1 + i for i, (keep, _) in enumerate(low) if not keep]
    state = state.reshape([1 << half] + [1 << length for _, length in low]).permute(order).contiguous()
    axes = len(high)
    order = [i for i, (keep, _) in enumerate(high) if keep] + [axes] + [i for i, (keep, _) in enumerate(high) if not keep] + [axes + 1]
    shape = [1 << length for _, length in high] + [1 << kept_low, 1 << (n - half - kept_low)]
    return state.reshape(shape).permute(order).contiguous()
  total = None
  for m in range(num):
    rows = gather(states[m]).reshape(1 << k, 1 << (n - k))
    part = E.weighted_gram(rows).conj() * float(weights[m])
    total = part if total is None else total + part
  return total


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=3)
  ap.add_argument("--step-limit", type=int, default=120)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  lib = E.load_library()
  stream = lambda: torch.cuda.current_stream().cuda_stream
  line = {"gpu": torch.cuda.get_device_name(0), "repeats": args.repeats, "window_ms": WINDOW_MS, "one_run_on_one_box": True, "streaming": [],
          "kernel": []}

  def flush():
    text = json.dumps(line)
    if args.out:
      with open(args.out, "w") as f:
        f.write(text + "\n")
    return text

  for n in (20, 24):
    with Step(f"streaming yardstick n={n}", args.step_limit):
      basis = E.random_states(8, n, 1).reshape(1, 8, 1 << n)
      coef = torch.full((8, 1, 1), 0.5 + 0.5j, dtype=torch.complex64, device="cuda")
      moved = 2 * basis.numel() * 8
      combine_ms = event_ms(lambda: E.krylov_combine(basis, coef), args.repeats)
      target = torch.empty_like(basis)
      copy_ms = event_ms(lambda: target.copy_(basis), args.repeats)
      line["streaming"].append({"qubits": n, "states": 8, "bytes": moved, "krylov_combine_ms": combine_ms,
                                "krylov_combine_bytes_per_s": moved / (combine_ms * 1e-3), "copy_ms": copy_ms,
                                "copy_bytes_per_s": moved / (copy_ms * 1e-3)})
      del basis, target
  rate = {row["qubits"]: row["krylov_combine_bytes_per_s"] for row in line["streaming"]}
  flush()

  for n in (20, 24):
    all_states = E.random_states(8, n, 2)
    all_weights = torch.rand(8, dtype=torch.float64, device="cuda") * 0.9 + 0.1
    for k in (1, 4, 8, 10):
      for num in (1, 8):
        for kind in ("high", "low", "spread"):
          with Step(f"n={n} k={k} M={num} {kind}", args.step_limit):
            kept = kept_qubits(n, k, kind)
            mask = sum(1 << q for q in kept)
            states, weights = all_states[:num], all_weights[:num].contiguous()
            scratch_bytes = E.reduced_density_scratch_bytes(num, n, mask)
            scratch = torch.empty(scratch_bytes // 8, dtype=torch.float64, device="cuda")
            out = torch.empty((1 << k, 1 << k, 2), dtype=torch.float64, device="cuda")

            def call():
              rc = lib.qhbm_reduced_density(states.data_ptr(), num, n, mask, weights.data_ptr(), scratch.data_ptr(),
                                            out.data_ptr(), stream())
              if rc != 0:
                raise RuntimeError(lib.qhbm_last_error(None).decode())
            ms = event_ms(call, args.repeats)
            host_weights = weights.cpu()
            # like for like: both routes through their python bindings, which allocate scratch and output per call
            binding_ms = event_ms(lambda: E.reduced_density(states, mask, weights), args.repeats)
            route_ms = event_ms(lambda: gram_route(states, kept, host_weights), args.repeats)
            difference = float((gram_route(states, kept, host_weights) - torch.view_as_complex(out)).abs().max())
            tile_rows = 1 << max(0, k - 6)
            tiles = tile_rows * (tile_rows + 1) // 2
            edge = 1 << min(k, 6)
            unique = num * 8 * (1 << n)
            fmas = 4.0 * tiles * edge * edge * num * (1 << (n - k))
            line["kernel"].append({
                "qubits": n, "kept": k, "states": num, "mask": kind, "kept_qubits": kept, "ms": ms,
                "scratch_bytes": scratch_bytes, "unique_bytes": unique, "model_bytes": unique * tile_rows,
                "unique_bytes_per_s": unique / (ms * 1e-3), "share_of_streaming_rate": unique / (ms * 1e-3) / rate[n],
                "fp64_fma_per_s": fmas / (ms * 1e-3), "binding_ms": binding_ms, "gram_route_ms": route_ms,
                "gram_route_over_fused": route_ms / ms, "gram_route_over_binding": route_ms / binding_ms,
                "max_abs_difference": difference})
            del scratch, out
          flush()
    del all_states
  print(flush())


if __name__ == "__main__":
  main()
