"""Times the weighted Gram kernel (`qhbm_weighted_gram`) and `inference.state_metrics` on one GPU, in one process.

  python scripts/state_metrics_time.py [--repeats 5] [--step-limit 120] [--out profiles/state_metrics.json]

Reported, not asserted (every figure is from one run on one box):
  * kernel: time of one `qhbm_weighted_gram` (device events around `--repeats` calls after a warm-up, scratch allocated
    outside) at (n, M) in {(20, 8), (20, 32), (24, 8), (24, 32)}, with and without a table; the bytes it moves by the model
    ceil(M/4) (ceil(M/4) + 1) / 2 tiles x (8 rows x 8 B + 4 B of table) x 2^n amplitudes; that rate as a fraction of the
    rate the project's own streaming kernel reaches in this process: `krylov_combine` with one row and one output (one
    16-byte read and one write per word, thermal.hip's shape) on a buffer of the same size class -- and, for scale,
    a device-to-device `copy_`;
  * whole metric against the dense route: `state_metrics` and `inference.fidelity` at n = 10 and 12 with M = 8, wall clock
    after one warm-up call each (engine construction is cached in the first and paid per call in the second, as a user
    pays them);
  * the split of `state_metrics` at n = 22, M = 8: inverse circuit, energy table (both methods), the three Gram calls,
    the host eigenproblems.
Each step runs under a watchdog of `--step-limit` seconds that ends the process (nothing more is started on the GPU
after a step that hangs).  Prints one JSON line and, with --out, writes it to that file."""
import argparse
import faulthandler
import importlib
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
from qhbmlib_amd import data, inference, ir, models  # noqa: E402
from qhbmlib_amd.models import energy_utils  # noqa: E402

SM = importlib.import_module("qhbmlib_amd.inference.state_metrics")  # (`inference.state_metrics` is the function)


class Step:
  """A watchdog around one step: the process exits (with every thread's traceback) when it runs past the limit."""

  def __init__(self, name, limit):
    self.name, self.limit = name, limit

  def __enter__(self):
    print(f"[state_metrics_time] {self.name}", file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(self.limit, exit=True)

  def __exit__(self, *exc):
    faulthandler.cancel_dump_traceback_later()
    return False


def event_ms(fn, repeats):
  fn()  # warm-up
  torch.cuda.synchronize()
  begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  begin.record()
  for _ in range(repeats):
    fn()
  end.record()
  torch.cuda.synchronize()
  return begin.elapsed_time(end) / repeats


def wall_ms(fn):
  torch.cuda.synchronize()
  start = time.perf_counter()
  out = fn()
  torch.cuda.synchronize()
  return out, 1e3 * (time.perf_counter() - start)


def gram_model_bytes(n, num, with_table):
  tile_rows = (num + 3) // 4
  return tile_rows * (tile_rows + 1) // 2 * (8 * 8 + (4 if with_table else 0)) * (1 << n)


def hea(qubits, layers, name):
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


def kobe_model(n, seed, device):
  qubits = ir.GridQubit.rect(1, n)
  gen = torch.Generator().manual_seed(seed)
  energy = models.KOBE(list(range(n)), 2)
  energy.build([None, n])
  circ = models.DirectQuantumCircuit(hea(qubits, 2, f"t{n}"))
  with torch.no_grad():
    for p in list(energy.parameters()) + list(circ.parameters()):
      p.copy_(torch.rand(p.shape, generator=gen) * 2.0 - 1.0)
  energy.to(device)
  return models.Hamiltonian(energy, circ)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--repeats", type=int, default=5)
  ap.add_argument("--step-limit", type=int, default=120)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  lib = E.load_library()
  stream = lambda: torch.cuda.current_stream().cuda_stream
  line = {"gpu": torch.cuda.get_device_name(0), "repeats": args.repeats, "one_run_on_one_box": True, "kernel": [], "whole": [],
          "streaming": []}

  def flush():
    text = json.dumps(line)
    if args.out:
      with open(args.out, "w") as f:
        f.write(text + "\n")
    return text

  # ---- the yardstick: what the project's own streaming kernel and a plain copy reach here ----
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

  # ---- the kernel ----
  for n, num in ((20, 8), (20, 32), (24, 8), (24, 32)):
    with Step(f"kernel n={n} M={num}", args.step_limit):
      states = E.random_states(num, n, 2)
      table = torch.rand(1 << n, dtype=torch.float32, device="cuda")
      scratch = torch.empty(E.gram_scratch_bytes(num, n) // 8, dtype=torch.float64, device="cuda")
      out = torch.empty((num, num, 2), dtype=torch.float64, device="cuda")
      for with_table in (False, True):
        t_ptr = table.data_ptr() if with_table else None

        def call():
          rc = lib.qhbm_weighted_gram(states.data_ptr(), num, n, t_ptr, scratch.data_ptr(), out.data_ptr(), stream())
          if rc != 0:
            raise RuntimeError(lib.qhbm_last_error(None).decode())
        ms = event_ms(call, args.repeats)
        moved = gram_model_bytes(n, num, with_table)
        line["kernel"].append({"qubits": n, "states": num, "table": with_table, "ms": ms, "model_bytes": moved,
                               "model_bytes_per_s": moved / (ms * 1e-3),
                               "share_of_streaming_rate": moved / (ms * 1e-3) / rate[n],
                               "unique_bytes": num * 8 * (1 << n) + (4 << n if with_table else 0),
                               # (eight fused multiply-adds per pair and 16-byte word, 16 pairs per tile)
                               "fp64_fma_per_s": moved / (64 + (4 if with_table else 0)) / 2 * 128.0 / (ms * 1e-3)})
      del states, table, scratch, out
    flush()

  # ---- the whole metric against the dense route ----
  for n in (10, 12):
    with Step(f"whole metric n={n}", args.step_limit):
      model = kobe_model(n, n, "cpu")   # (the dense route evaluates the energy on the CPU)
      rng = np.random.default_rng(n)
      raw = rng.normal(size=(8, 1 << n)) + 1j * rng.normal(size=(8, 1 << n))
      raw /= np.linalg.norm(raw, axis=1, keepdims=True)
      source = data.StateVectorData(torch.from_numpy(raw))
      sigma = torch.from_numpy((raw.T / 8.0) @ raw.conj())
      inference.state_metrics(model, source)  # warm-up
      got, metrics_ms = wall_ms(lambda: inference.state_metrics(model, source))
      float(inference.fidelity(model, sigma).detach())  # warm-up
      dense, dense_ms = wall_ms(lambda: float(inference.fidelity(model, sigma).detach()))
      line["whole"].append({"qubits": n, "states": 8, "state_metrics_ms": metrics_ms, "dense_fidelity_ms": dense_ms,
                            "speedup": dense_ms / metrics_ms, "fidelity": got.fidelity, "dense_fidelity": dense})
    flush()

  # ---- where the time of one state_metrics call goes at 22 qubits ----
  n, num = 22, 8
  with Step(f"split n={n}", args.step_limit):
    model = kobe_model(n, n, "cuda")
    source = data.StateVectorData(E.random_states(num, n, 3), qubits=model.circuit.qubits)
    device = torch.device("cuda", torch.cuda.current_device())
    weights = source.weights
    inference.state_metrics(model, source, table="transform")  # warm-up: the engine, its workspace
    _, total_ms = wall_ms(lambda: inference.state_metrics(model, source, table="transform"))
    eng, values = SM._inverse_circuit_engine(model, device)  # pylint: disable=protected-access
    amps, circuit_ms = wall_ms(lambda: eng.statevector_from_states(source._device_states(), values))  # pylint: disable=protected-access
    with torch.no_grad():
      energy_utils.energy_table(model.energy, n, 24, method="transform")
      energies, transform_ms = wall_ms(lambda: energy_utils.energy_table(model.energy, n, 24, method="transform"))
      energy_utils.energy_table(model.energy, n, 24, method="terms")
      _, terms_ms = wall_ms(lambda: energy_utils.energy_table(model.energy, n, 24, method="terms"))
      SM._partition(energies)  # pylint: disable=protected-access
      (_, probs), partition_ms = wall_ms(lambda: SM._partition(energies))  # pylint: disable=protected-access
    grams, gram_ms = wall_ms(lambda: [E.weighted_gram(source._device_states()), E.weighted_gram(amps, probs),  # pylint: disable=protected-access
                                      E.weighted_gram(amps, energies)])
    _, host_ms = wall_ms(lambda: [SM._weighted_spectrum(g, weights) for g in grams])  # pylint: disable=protected-access
    line["split"] = {"qubits": n, "states": num, "table": "transform", "state_metrics_ms": total_ms,
                     "inverse_circuit_ms": circuit_ms, "table_transform_ms": transform_ms, "table_terms_ms": terms_ms,
                     "partition_ms": partition_ms, "three_grams_ms": gram_ms, "host_eigenproblems_ms": host_ms}
  print(flush())


if __name__ == "__main__":
  main()
