"""Times the backward of the differentiable reduced density matrix (`_engine.subsystem_apply`) against the
route torch alone offers, on one GPU, in one process.

  python scripts/reduced_density_vjp_time.py [--repeats 5] [--rounds 3] [--out profiles/reduced_density_vjp.json]

Both routes compute grad_states = w_m ((Gamma + Gamma^H) (x) 1) phi_m and the dots <phi_m|(H (x) 1)|phi_m> from the same
states, weights and H:
  engine   one `subsystem_apply` (scale = weights, want_dots): the states are read where they lie;
  torch    `permute().contiguous()` to [M, 2^k, 2^(n-k)], a complex matmul with H, the dots from the product, the scale, and
           `permute().contiguous()` back: two more copies of [M, 2^n] (neighbouring qubits of one kind are one axis; a mask
           with more axes than a strided copy takes, the spread ones from k = 10 on, needs two copies each way).
They are timed ALTERNATELY (`--rounds` rounds of `--repeats` calls each, after a warm-up call per route; device events) at
20 qubits with 8 states and 24 qubits with 2 states, k in {1, 4, 6, 10}, for the three masks of
scripts/reduced_density_time.py (the k highest qubits, the k lowest, k spread evenly); median and range of the windows, the
largest difference of the two results, and the peak of torch's allocator above the resident inputs are reported.

The kernel alone (scratch and output allocated outside, the C entry point, device events) is quoted against both roofs of
the MI355X -- 8 TB/s for its 16 bytes per amplitude, 155 TF (f32-input matrix instructions, measured peak) for its
8 * 2^k flop per amplitude -- and the shape's bound is the one that takes longer.

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

from qhbmlib_amd import _engine as E  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8e12
MATRIX_F32_PEAK_FLOPS = 155e12


def kept_qubits(n, k, kind):
  if kind == "high":    # the k most significant index bits
    return list(range(k))
  if kind == "low":     # the k least significant index bits
    return list(range(n - k, n))
  return sorted({(2 * i + 1) * n // (2 * k) for i in range(k)})  # spread evenly


def _window(fn, repeats):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(repeats):
    fn()
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) / repeats


MAX_COPY_DIMS = 16  # a strided copy of torch takes no more axes


def _copy_steps(num, n, kept):
  """[(shape, order)]: `x.reshape(shape).permute(order).contiguous()` in turn takes [M, 2^n] to [M, 2^k, 2^(n-k)].
  Neighbouring qubits of one kind are one axis; a mask with more axes than a strided copy takes is gathered in two copies,
  the low half of the qubits first, then the high half."""
  def runs_of(first, last):
    runs = []
    for q in range(first, last):
      keep = q in kept
      if runs and runs[-1][0] == keep:
        runs[-1][1] += 1
      else:
        runs.append([keep, 1])
    return runs
  runs = runs_of(0, n)
  if len(runs) + 1 <= MAX_COPY_DIMS:
    order = [0] + [1 + i for i, (keep, _) in enumerate(runs) if keep] + [1 + i for i, (keep, _) in enumerate(runs) if not keep]
    return [([num] + [1 << length for _, length in runs], order)]
  half = n // 2
  low, high = runs_of(half, n), runs_of(0, half)
  kept_low = sum(length for keep, length in low if keep)
  first = ([num, 1 << half] + [1 << length for _, length in low],
           [0, 1] + [2 + i for i, (keep, _) in enumerate(low) if keep] + [2 + i for i, (keep, _) in enumerate(low) if not keep])
  axes = len(high)
  second = ([num] + [1 << length for _, length in high] + [1 << kept_low, 1 << (n - half - kept_low)],
            [0] + [1 + i for i, (keep, _) in enumerate(high) if keep] + [1 + axes] +
            [1 + i for i, (keep, _) in enumerate(high) if not keep] + [2 + axes])
  return [first, second]


def torch_route(states, kept, hermitian, weights):
  """(grad_states [M, 2^n] complex64, dots [M] complex64) through permute + contiguous + matmul + permute back."""
  num, dim = states.shape
  n = dim.bit_length() - 1
  k = len(kept)
  steps = _copy_steps(num, n, kept)
  panels = states
  for shape, order in steps:
    panels = panels.reshape(shape).permute(order).contiguous()
  panels = panels.reshape(num, 1 << k, 1 << (n - k))
  product = torch.matmul(hermitian, panels)
  dots = (panels.conj() * product).sum((1, 2))
  product = product * weights.to(product.dtype)[:, None, None]
  for shape, order in reversed(steps):
    inverse = [order.index(i) for i in range(len(order))]
    product = product.reshape([shape[i] for i in order]).permute(inverse).contiguous()
  return product.reshape(num, dim), dots


def _peak_above(fn):
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  result = fn()
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - base
  del result
  return int(peak)


def compare(n, k, num, kind, repeats, rounds):
  kept = kept_qubits(n, k, kind)
  mask = sum(1 << q for q in kept)
  gen = torch.Generator("cuda").manual_seed(100 * n + k)
  states = torch.randn((num, 1 << n), dtype=torch.complex64, device="cuda", generator=gen)
  states /= states.abs().pow(2).sum(1, keepdim=True).sqrt()
  gamma = torch.randn((1 << k, 1 << k), dtype=torch.complex128, device="cuda", generator=gen)
  hermitian = (gamma + gamma.conj().transpose(0, 1)).to(torch.complex64)
  weights = torch.rand(num, dtype=torch.float64, device="cuda", generator=gen)

  engine = lambda: E.subsystem_apply(states, mask, hermitian, scale=weights, want_dots=True)
  other = lambda: torch_route(states, kept, hermitian, weights)
  out_e, dots_e = engine()
  out_t, dots_t = other()
  difference = float((out_e - out_t).abs().max())
  dots_difference = float((dots_e - dots_t.to(torch.complex128)).abs().max())
  scale_of_result = float(out_t.abs().max())
  del out_e, out_t, dots_e, dots_t
  engine_ms, torch_ms = [], []
  for _ in range(rounds):
    engine_ms.append(_window(engine, repeats))
    torch_ms.append(_window(other, repeats))
  engine_peak, torch_peak = _peak_above(engine), _peak_above(other)

  # the kernel alone: the C entry point on buffers allocated outside the window
  lib = E.load_library()
  scratch = torch.empty(E.subsystem_apply_scratch_bytes(num, n, mask) // 8, dtype=torch.float64, device="cuda")
  out = torch.empty_like(states)
  dots = torch.empty((num, 2), dtype=torch.float64, device="cuda")
  stream = torch.cuda.current_stream().cuda_stream

  def kernel():
    rc = lib.qhbm_subsystem_apply(states.data_ptr(), num, n, mask, hermitian.data_ptr(), weights.data_ptr(), out.data_ptr(),
                                  dots.data_ptr(), scratch.data_ptr(), stream)
    assert rc == 0, lib.qhbm_last_error(None).decode()
  kernel()
  torch.cuda.synchronize()
  kernel_ms = [_window(kernel, repeats) for _ in range(rounds)]
  ms = float(np.median(kernel_ms))
  amplitudes = float(num) * float(1 << n)
  moved, flops = 16.0 * amplitudes, 8.0 * float(1 << k) * amplitudes
  memory_floor_ms, matrix_floor_ms = moved / HBM_PEAK_BYTES_PER_S * 1e3, flops / MATRIX_F32_PEAK_FLOPS * 1e3
  e_med, t_med = float(np.median(engine_ms)), float(np.median(torch_ms))
  return {"qubits": n, "kept": k, "states": num, "mask": kind, "kept_qubits": kept,
          "engine_ms": e_med, "engine_ms_range": [min(engine_ms), max(engine_ms)],
          "torch_ms": t_med, "torch_ms_range": [min(torch_ms), max(torch_ms)], "engine_over_torch": e_med / t_med,
          "engine_peak_bytes": engine_peak, "torch_peak_bytes": torch_peak, "state_bytes": int(8 * amplitudes),
          "max_difference": difference, "max_dots_difference": dots_difference, "result_inf_norm": scale_of_result,
          "kernel": {"ms": ms, "ms_range": [min(kernel_ms), max(kernel_ms)], "bytes_per_s": moved / (ms * 1e-3),
                     "share_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S, "flops": flops,
                     "flops_per_s": flops / (ms * 1e-3), "share_of_matrix_f32_peak": flops / (ms * 1e-3) / MATRIX_F32_PEAK_FLOPS,
                     "bound": "memory" if memory_floor_ms >= matrix_floor_ms else "compute",
                     "floor_ms": max(memory_floor_ms, matrix_floor_ms)}}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("reduced_density_vjp_time.py needs a GPU: the engine has no CPU fallback")
  rows = []
  for n, num in ((20, 8), (24, 2)):
    for k in (1, 4, 6, 10):
      for kind in ("high", "low", "spread"):
        rows.append(compare(n, k, num, kind, args.repeats, args.rounds))
        torch.cuda.empty_cache()
  line = {"gpu": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
          "matrix_f32_peak_flops": MATRIX_F32_PEAK_FLOPS, "repeats": args.repeats, "rounds": args.rounds, "rows": rows}
  text = json.dumps(line)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
