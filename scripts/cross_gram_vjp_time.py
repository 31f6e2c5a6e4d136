"""Times the backward of the differentiable two-ensemble metrics (`_engine.cross_gram_vjp`) against the two
routes that existed before it, on one GPU, in one process.

  python scripts/cross_gram_vjp_time.py [--repeats 5] [--rounds 3] [--out profiles/cross_gram_vjp.json]

For M bras, K kets, a table t and a cotangent Gamma [M, K] all three routes compute out_bras = t conj(Gamma) kets,
out_kets = t Gamma^T bras and table_grad = sum_j Re(conj(c_j) kets_j):
  engine   one `cross_gram_vjp` with its allocations;
  torch    complex64 GEMMs, the products with t, and the float64 reduction for table_grad;
  concat   `torch.cat([bras, kets])` and one `weighted_gram_vjp` on the M + K states with H = [[0, Gamma], [Gamma^H, 0]]
           (the route DESIGN.md 6p exists to avoid: a copy of both ensembles and (M + K)^2 work).
Two requests are timed: the bras' cotangent alone -- the usual training shape, a circuit's final states against fixed targets
-- and all three outputs.  The routes are timed ALTERNATELY (`--rounds` windows of `--repeats` calls each, after a warm-up call
per route; device events) at (n, M, K) = (20, 8, 8), (24, 8, 8), (24, 32, 2), (24, 2, 32); median, least and largest window, the
largest difference of the results and the peak of torch's allocator above the resident inputs are reported, and per shape a
`loses` list names the requests at which the engine's median is not the least.

The kernels alone (scratch and outputs allocated outside, the C entry point, device events) are quoted against both roofs of
the MI355X per side sweep -- 8 TB/s for 8 R + 8 S + 4 bytes per amplitude (+ 8 S + 8 for the partner rows and table_grad on
the kets' side), 155 TF (f32-input matrix instructions, measured peak) for 8 R S flop per amplitude.

One whole step: `ensemble_metrics((final states, w), target, differentiable=True).fidelity.backward()` at 20 qubits, 8 states
against 8 targets, two HEA layers, beside the forward-only call; host clock around a device synchronise.

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
SHAPES = ((20, 8, 8), (24, 8, 8), (24, 32, 2), (24, 2, 32))


def _window(fn, repeats):
  start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  for _ in range(repeats):
    fn()
  stop.record()
  torch.cuda.synchronize()
  return start.elapsed_time(stop) / repeats


def _peak_above(fn):
  torch.cuda.synchronize()
  base = torch.cuda.memory_allocated()
  torch.cuda.reset_peak_memory_stats()
  result = fn()
  torch.cuda.synchronize()
  peak = torch.cuda.max_memory_allocated() - base
  del result
  return int(peak)


def torch_route(bras, kets, table, gamma, everything):
  """(out_bras, out_kets or None, table_grad or None) through complex GEMMs, products and a reduction."""
  out_bras = (gamma.conj() @ kets) * table
  if not everything:
    return out_bras, None, None
  c = gamma.transpose(0, 1) @ bras
  grad = (c.real.double() * kets.real.double() + c.imag.double() * kets.imag.double()).sum(0)
  return out_bras, c * table, grad


def concat_route(bras, kets, table, gamma, everything):
  """The same through one buffer of M + K states and `weighted_gram_vjp`: its H = [[0, Gamma], [Gamma^H, 0]] gives the bras'
  rows t conj(Gamma) kets and the kets' rows t Gamma^T bras, and its halved table sum is the cross-Gram one."""
  num = bras.shape[0]
  both = torch.cat([bras, kets], 0)
  hermitian = torch.zeros((both.shape[0], both.shape[0]), dtype=torch.complex64, device=bras.device)
  hermitian[:num, num:] = gamma
  hermitian[num:, :num] = gamma.conj().transpose(0, 1)
  out, grad = E.weighted_gram_vjp(both, table, hermitian, want_states=True, want_table=everything)
  return out[:num], (out[num:] if everything else None), grad


def _median_range(values):
  return {"ms": float(np.median(values)), "ms_range": [min(values), max(values)]}


def _side(rows, outputs, sums, amplitudes, ms):
  moved = (8.0 * rows + 8.0 * outputs + 4.0 + ((8.0 * outputs + 8.0) if sums else 0.0)) * amplitudes
  flops = 8.0 * rows * outputs * amplitudes
  memory_floor_ms, matrix_floor_ms = moved / HBM_PEAK_BYTES_PER_S * 1e3, flops / MATRIX_F32_PEAK_FLOPS * 1e3
  return {"source_rows": rows, "output_rows": outputs, "path": "vector" if rows <= 8 else "matrix", "ms": ms, "bytes": moved,
          "bytes_per_s": moved / (ms * 1e-3), "share_of_hbm_peak": moved / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S, "flops": flops,
          "flops_per_s": flops / (ms * 1e-3), "share_of_matrix_f32_peak": flops / (ms * 1e-3) / MATRIX_F32_PEAK_FLOPS,
          "bound": "memory" if memory_floor_ms >= matrix_floor_ms else "compute", "floor_ms": max(memory_floor_ms, matrix_floor_ms)}


def compare(n, num, num_kets, repeats, rounds):
  gen = torch.Generator("cuda").manual_seed(1000 * n + 10 * num + num_kets)
  bras = torch.randn((num, 1 << n), dtype=torch.complex64, device="cuda", generator=gen)
  kets = torch.randn((num_kets, 1 << n), dtype=torch.complex64, device="cuda", generator=gen)
  bras /= bras.abs().pow(2).sum(1, keepdim=True).sqrt()
  kets /= kets.abs().pow(2).sum(1, keepdim=True).sqrt()
  table = torch.rand(1 << n, dtype=torch.float32, device="cuda", generator=gen)
  gamma = torch.randn((num, num_kets), dtype=torch.complex64, device="cuda", generator=gen)
  row = {"qubits": n, "bras": num, "kets": num_kets, "state_bytes": int(8 * (num + num_kets) << n), "loses": []}
  for request, everything in (("bras_only", False), ("all_outputs", True)):
    routes = {"engine": lambda: E.cross_gram_vjp(bras, kets, table, gamma, want_kets=everything, want_table=everything),
              "torch": lambda: torch_route(bras, kets, table, gamma, everything),
              "concat": lambda: concat_route(bras, kets, table, gamma, everything)}
    results = {name: fn() for name, fn in routes.items()}
    differences = {}
    for name in ("torch", "concat"):
      differences[name] = [None if got is None else float((got - want).abs().max())
                           for got, want in zip(results["engine"], results[name])]
    scale = float(results["torch"][0].abs().max())
    del results
    windows = {name: [] for name in routes}
    for _ in range(rounds):
      for name, fn in routes.items():
        windows[name].append(_window(fn, repeats))
    entry = {name: dict(_median_range(w), peak_bytes=_peak_above(routes[name])) for name, w in windows.items()}
    entry["max_difference_to"] = differences
    entry["result_inf_norm"] = scale
    least = min(entry[name]["ms"] for name in routes)
    if entry["engine"]["ms"] > least:
      row["loses"].append({"request": request, "to": [name for name in ("torch", "concat") if entry[name]["ms"] < entry["engine"]["ms"]]})
    row[request] = entry
    torch.cuda.empty_cache()

  # the kernels alone: the C entry point on buffers allocated outside the window, one side per call
  lib = E.load_library()
  scratch = torch.empty(E.cross_gram_vjp_scratch_bytes(num, num_kets, n) // 8, dtype=torch.float64, device="cuda")
  out_bras, out_kets = torch.empty_like(bras), torch.empty_like(kets)
  grad = torch.empty(1 << n, dtype=torch.float64, device="cuda")
  stream = torch.cuda.current_stream().cuda_stream

  def kernel(want_bras, want_kets, want_table):
    def call():
      rc = lib.qhbm_cross_gram_vjp(bras.data_ptr(), num, kets.data_ptr(), num_kets, n, table.data_ptr(), gamma.data_ptr(),
                                   out_bras.data_ptr() if want_bras else None, out_kets.data_ptr() if want_kets else None,
                                   grad.data_ptr() if want_table else None, scratch.data_ptr(), stream)
      assert rc == 0, lib.qhbm_last_error(None).decode()
    call()
    torch.cuda.synchronize()
    return float(np.median([_window(call, repeats) for _ in range(rounds)]))
  amplitudes = float(1 << n)
  row["kernels"] = {"bra_side": _side(num_kets, num, False, amplitudes, kernel(True, False, False)),
                    "ket_side_with_table_grad": _side(num, num_kets, True, amplitudes, kernel(False, True, True)),
                    "all_outputs_ms": kernel(True, True, True)}
  return row


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


def fidelity_step(n, num, num_targets, repeats):
  """One training step on the fidelity of a circuit's final states against fixed targets at n qubits (two HEA layers,
  random-sign inputs and targets): host-clock milliseconds (median, least, largest of `repeats` after a warm-up) of the
  forward-only call and of forward + backward."""
  from qhbmlib_amd import inference, ir, models  # pylint: disable=import-outside-toplevel
  gen = torch.Generator().manual_seed(n)
  circ = models.DirectQuantumCircuit(_hea(ir, ir.GridQubit.rect(1, n), 2, f"c{n}"))
  with torch.no_grad():
    for p in circ.parameters():
      p.copy_(torch.rand(p.shape, generator=gen) * 2.0 - 1.0)
  q = inference.AnalyticQuantumInference(circ)
  inputs, targets = E.random_states(num, n, 5), E.random_states(num_targets, n, 6)
  w = torch.full((num,), 1.0 / num, dtype=torch.float64)
  v = torch.full((num_targets,), 1.0 / num_targets, dtype=torch.float64)
  variables = list(circ.parameters())

  def forward_only():
    with torch.no_grad():
      return inference.ensemble_metrics((q.final_states_from_states(inputs), w), (targets, v)).fidelity

  def step():
    for p in variables:
      p.grad = None
    inference.ensemble_metrics((q.final_states_from_states(inputs), w), (targets, v), differentiable=True).fidelity.backward()

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
  return {"qubits": n, "states": num, "targets": num_targets, "forward_only": clock(forward_only),
          "forward_and_backward": clock(step), "gradient_inf_norms": [float(p.grad.abs().max()) for p in variables]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--rounds", type=int, default=3)
  ap.add_argument("--out", default=None)
  ap.add_argument("--no-step", action="store_true", help="leave out the whole fidelity step")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("cross_gram_vjp_time.py needs a GPU: the engine has no CPU fallback")
  rows = []
  for n, num, num_kets in SHAPES:
    rows.append(compare(n, num, num_kets, args.repeats, args.rounds))
    torch.cuda.empty_cache()
  line = {"gpu": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK_BYTES_PER_S,
          "matrix_f32_peak_flops": MATRIX_F32_PEAK_FLOPS, "repeats": args.repeats, "rounds": args.rounds, "rows": rows}
  if not args.no_step:
    line["fidelity_step"] = fidelity_step(20, 8, 8, args.repeats)
  text = json.dumps(line)
  print(text)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      f.write(text + "\n")


if __name__ == "__main__":
  main()
