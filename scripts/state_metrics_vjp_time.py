"""Times the backward of the differentiable state metrics (`_engine.weighted_gram_vjp`) against the route
torch alone offers, on one GPU, in one process.

  python scripts/state_metrics_vjp_time.py [--repeats 5] [--rounds 3] [--out profiles/state_metrics_vjp.json]

Both routes compute out_j = t sum_i H[i, j] a_i and table_grad = 1/2 sum_j Re(conj(c_j) a_j) from the same states, table
and H:
  engine   one `weighted_gram_vjp` with its allocations: the states are read once;
  torch    a complex64 `H.T @ a`, the product with t, and the float64 reduction for table_grad: three more passes and two
           more copies of [M, 2^n].
They are timed ALTERNATELY (`--rounds` windows of `--repeats` calls each, after a warm-up call per route; device events) at
(n, M) = (20, 8), (20, 32), (24, 8), (24, 32), the shapes of DESIGN.md 6i's table; median, least and largest window, the
largest difference of the two results and the peak of torch's allocator above the resident inputs are reported.

The kernel alone (scratch and outputs allocated outside, the C entry point, device events) is quoted against both roofs of
the MI355X -- 8 TB/s for its 16 M + 4 + 8 bytes per amplitude, 155 TF (f32-input matrix instructions, measured peak) for its
8 M^2 flop per amplitude -- and the shape's bound is the one that takes longer.

One whole step: `state_metrics(..., differentiable=True).fidelity.backward()` at 20 qubits and 8 states (KOBE order 2
under two HEA layers, random-sign data, `table="terms"`), beside the forward-only call; host clock around a device
synchronise.

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

from qhbmlib_amd import _engine as E  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8e12
MATRIX_F32_PEAK_FLOPS = 155e12
SHAPES = ((20, 8), (20, 32), (24, 8), (24, 32))


def _window(fn, repeats):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(repeats):
    fn()
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) / repeats


def torch_route(states, table, hermitian):
  """(out [M, 2^n] complex64, table_grad [2^n] float64) through a complex GEMM, a product and a reduction."""
  c = hermitian.transpose(0, 1) @ states
  grad = 0.5 * (c.real.double() * states.real.double() + c.imag.double() * states.imag.double()).sum(0)
  return c * table, grad


def _peak_above(fn):
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  result = fn()
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - base
  del result
  return int(peak)


def compare(n, num, repeats, rounds):
  gen = torch.Generator("cuda").manual_seed(100 * n + num)
  states = torch.randn((num, 1 << n), dtype=torch.complex64, device="cuda", generator=gen)
  states /= states.abs().pow(2).sum(1, keepdim=True).sqrt()
  table = torch.rand(1 << n, dtype=torch.float32, device="cuda", generator=gen)
  gamma = torch.randn((num, num), dtype=torch.complex128, device="cuda", generator=gen)
  hermitian = (gamma + gamma.conj().transpose(0, 1)).to(torch.complex64)

  engine = lambda: E.weighted_gram_vjp(states, table, hermitian)
  other = lambda: torch_route(states, table, hermitian)
  out_e, grad_e = engine()
  out_t, grad_t = other()
  difference = float((out_e - out_t).abs().max())
  grad_difference = float((grad_e - grad_t).abs().max())
  scale_of_result = float(out_t.abs().max())
  del out_e, out_t, grad_e, grad_t
  engine_ms, torch_ms = [], []
  for _ in range(rounds):
    engine_ms.append(_window(engine, repeats))
    torch_ms.append(_window(other, repeats))
  engine_peak, torch_peak = _peak_above(engine), _peak_above(other)

  # the kernel alone: the C entry point on buffers allocated outside the window
  lib = E.load_library()
  scratch = torch.empty(E.gram_vjp_scratch_bytes(num, n) // 8, dtype=torch.float64, device="cuda")
  out = torch.empty_like(states)
  grad = torch.empty(1 << n, dtype=torch.float64, device="cuda")
  stream = torch.cuda.current_stream().cuda_stream

  def kernel():
    rc = lib.qhbm_weighted_gram_vjp(states.data_ptr(), num, n, table.data_ptr(), hermitian.data_ptr(), out.data_ptr(),
                                    grad.data_ptr(), scratch.data_ptr(), stream)
    assert rc == 0, lib.qhbm_last_error(None).decode()
  kernel()
  torch.cuda.synchronize()
  kernel_ms = [_window(kernel, repeats) for _ in range(rounds)]
  ms = float(np.median(kernel_ms))
  amplitudes = float(1 << n)
  moved, flops = (16.0 * num + 4.0 + 8.0) * amplitudes, 8.0 * num * num * amplitudes
  memory_floor_ms, matrix_floor_ms = moved / HBM_PEAK_BYTES_PER_S * 1e3, flops / MATRIX_F32_PEAK_FLOPS * 1e3
  e_med, t_med = float(np.median(engine_ms)), float(np.median(torch_ms))
  return {"qubits": n, "states": num, "path": "vector" if num <= 8 else "matrix",
          "engine_ms": e_med, "engine_ms_range": [min(engine_ms), max(engine_ms)],
          "torch_ms": t_med, "torch_ms_range": [min(torch_ms), max(torch_ms)], "engine_over_torch": e_med / t_med,
          "engine_peak_bytes": engine_peak, "torch_peak_bytes": torch_peak, "state_bytes": int(8 * num * amplitudes),
          "max_difference": difference, "max_table_grad_difference": grad_difference, "result_inf_norm": scale_of_result,
          "kernel": {"ms": ms, "ms_range": [min(kernel_ms), max(kernel_ms)], "bytes": moved, "bytes_per_s": moved / (ms * 1e-3),
                     "share_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S, "flops": flops,
                     "flops_per_s": flops / (ms * 1e-3), "share_of_matrix_f32_peak": flops / (ms * 1e-3) / MATRIX_F32_PEAK_FLOPS,
                     "bound": "memory" if memory_floor_ms >= matrix_floor_ms else "compute",
                     "floor_ms": max(memory_floor_ms, matrix_floor_ms)}}


def _hea(ir, qubits, layers, name):
  circuit = ir.Circuit()
  for layer in range(layers):
    for k, q in enumerate(qubits):
      sx, sz = ir.symbols(f"sx_{name}_{layer}_{k} sz_{name}_{layer}_{k}")
      circuit += [ir.X(q)**sx, ir.Z(q)**sz]
    for k, (q0, q1) in enumerate(zip(qubits[::2], qubits[1::2])):
      circuit += ir.CZPowGate(ir.Symbol(f"sc_{name}_{layer}_{2 * k}"))(q0, q1)
    for k, (q0, q1) in enumerate(zip(qubits[1::2], qubits[2::2])):
      circuit += ir.CZPowGate(ir.Symbol(f"sc_{name}_{layer}_{2 * k + 1}"))(q0, q1)
  return circuit


def fidelity_step(n, num, repeats):
  """One training step on the fidelity at n qubits and `num` random-sign states, the model of scripts/state_metrics_time.py
  (KOBE order 2 under two HEA layers): host-clock milliseconds (median, least, largest of `repeats` after a warm-up) of the
  forward-only call and of forward + backward."""
  from qhbmlib_amd import data, inference, ir, models  # pylint: disable=import-outside-toplevel
  gen = torch.Generator().manual_seed(n)
  energy = models.KOBE(list(range(n)), 2)
  energy.build([None, n])
  circ = models.DirectQuantumCircuit(_hea(ir, ir.GridQubit.rect(1, n), 2, f"v{n}"))
  with torch.no_grad():
    for p in list(energy.parameters()) + list(circ.parameters()):
      p.copy_(torch.rand(p.shape, generator=gen) * 2.0 - 1.0)
  energy.to("cuda")
  model = models.Hamiltonian(energy, circ)
  source = data.StateVectorData(E.random_states(num, n, 5), torch.full((num,), 1.0 / num, dtype=torch.float64))
  variables = list(circ.parameters()) + list(energy.parameters())

  def forward_only():
    return inference.state_metrics(model, source).fidelity

  def step():
    for v in variables:
      v.grad = None
    inference.state_metrics(model, source, differentiable=True).fidelity.backward()

  def clock(fn):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
      begin = time.perf_counter()
      fn()
      torch.cuda.synchronize()
      times.append((time.perf_counter() - begin) * 1e3)
    return {"ms": float(np.median(times)), "ms_range": [min(times), max(times)]}
  return {"qubits": n, "states": num, "forward_only": clock(forward_only), "forward_and_backward": clock(step),
          "gradient_inf_norms": [float(v.grad.abs().max()) for v in variables]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--out", default=None)
  ap.add_argument("--no-step", action="store_true", help="leave out the whole fidelity step")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("state_metrics_vjp_time.py needs a GPU: the engine has no CPU fallback")
  rows = []
  for n, num in SHAPES:
    rows.append(compare(n, num, args.repeats, args.rounds))
    torch.cuda.empty_cache()
  line = {"gpu": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
          "matrix_f32_peak_flops": MATRIX_F32_PEAK_FLOPS, "repeats": args.repeats, "rounds": args.rounds, "rows": rows}
  if not args.no_step:
    line["fidelity_step"] = fidelity_step(20, 8, args.repeats)
  text = json.dumps(line)
  print(text)
  if args.out:
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
