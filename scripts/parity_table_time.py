"""Times the table of all 2^n energies of a spin-parity energy, and its VJP, built BY TERMS (qhbm_parity_energy /
qhbm_parity_energy_vjp over the bitstring table, T 2^n parity evaluations) against BY TRANSFORM (qhbm_parity_table /
qhbm_parity_table_vjp, a Walsh-Hadamard transform: n 2^n additions), and one QMHL step with
`energy_tables="all"` both ways.

  python scripts/parity_table_time.py --out profiles/parity_table.json [--shapes kobe2:20,kobe3:20,kobe3:24,kobe2:28]
                                      [--qmhl kobe3:20] [--reps 5]

Both paths run in ONE process, alternating, after a warm-up, timed with HIP events (mean over --reps).  Per shape the JSON
holds the four times, which path wins, the agreement of the two results, and for the raw transform its time, the bytes it
moves -- passes x 8 B x 2^n, every pass reads and writes the array once -- and that rate against the 8 TB/s HBM peak.
No time is fixed in advance.  It needs an MI355X: there is no CPU fallback and no estimate."""
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
from qhbmlib_amd import data, inference, ir, models  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s


def hea(qubits, layers, name):
  circuit = ir.Circuit()
  for layer in range(layers):
    for i, q in enumerate(qubits):
      circuit += [ir.X(q)**ir.Symbol(f"sx_{name}_{layer}_{i}"), ir.Z(q)**ir.Symbol(f"sz_{name}_{layer}_{i}")]
    pairs = list(zip(qubits[::2], qubits[1::2])) + list(zip(qubits[1::2], qubits[2::2]))
    for i, (q0, q1) in enumerate(pairs):
      circuit += ir.CZPowGate(ir.Symbol(f"sc_{name}_{layer}_{i}"))(q0, q1)
  return circuit


class FixedData(data.QuantumData):
  """Data given as bitstring samples through a fixed circuit."""

  def __init__(self, samples, q_infer):
    self.samples, self.q_infer = samples, q_infer

  def expectation(self, observable):
    return torch.mean(self.q_infer.expectation(self.samples, observable))


def parse_shape(text):
  kind, n = text.split(":")
  if not kind.startswith("kobe"):
    raise SystemExit(f"shape {text!r}: kobe<order>:<bits>")
  return int(kind[4:]), int(n)


def bitstring_table(n, device):
  """int8 [2^n, n] in `all_bitstrings` order, built in slices (the one-shot form goes through an int64 [2^n, n])."""
  out = torch.empty((1 << n, n), dtype=torch.int8, device=device)
  shifts = torch.arange(n - 1, -1, -1, dtype=torch.int64, device=device).unsqueeze(0)
  step = 1 << min(n, 22)
  for lo in range(0, 1 << n, step):
    index = torch.arange(lo, lo + step, dtype=torch.int64, device=device).unsqueeze(1)
    out[lo:lo + step] = ((index >> shifts) & 1).to(torch.int8)
  return out


def timed(fns, reps):
  """Mean milliseconds of each callable: one warm-up round, then `reps` rounds that alternate between them."""
  for fn in fns:
    fn()
  torch.cuda.synchronize()
  total = [0.0] * len(fns)
  for _ in range(reps):
    for i, fn in enumerate(fns):
      start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      start.record()
      fn()
      stop.record()
      stop.synchronize()
      total[i] += start.elapsed_time(stop)
  return [t / reps for t in total]


def time_shape(order, n, reps):
  dev = torch.device("cuda")
  energy = models.KOBE(list(range(n)), order).to(dev)
  kernel = energy.post_process[0].kernel
  with torch.no_grad():
    kernel.uniform_(-0.5, 0.5)
  masks = energy._parity_masks(dev)   # pylint: disable=protected-access
  thetas = kernel.detach()
  bits = bitstring_table(n, dev)
  weights = torch.rand(1 << n, device=dev)
  results = {}

  def table_terms():
    results["table_terms"] = E.parity_energy(thetas, bits, masks)

  def table_transform():
    results["table_transform"] = E.parity_table(thetas, masks, n)

  def vjp_terms():
    results["vjp_terms"] = E.parity_sums(bits, masks, weights)

  lib = E.load_library()
  scratch = torch.empty_like(weights)
  grad = torch.empty(masks.numel(), device=dev)
  stream = torch.cuda.current_stream(dev).cuda_stream

  def vjp_transform():
    rc = lib.qhbm_parity_table_vjp(masks.data_ptr(), masks.numel(), n, weights.data_ptr(), scratch.data_ptr(),
                                   grad.data_ptr(), stream)
    if rc != 0:
      raise E.EngineError(lib.qhbm_last_error(None).decode())
    results["vjp_transform"] = grad

  raw = torch.rand(1 << n, device=dev)
  t_tt, t_tf, t_vt, t_vf, t_raw = timed([table_terms, table_transform, vjp_terms, vjp_transform,
                                         lambda: E.walsh_hadamard_(raw)], reps)
  passes = E.walsh_hadamard_passes(n)
  moved = passes * 8.0 * (1 << n)
  norm = float(thetas.abs().sum())
  row = {
      "energy": f"kobe{order}", "n": n, "terms": int(masks.numel()), "reps": reps,
      "bitstring_table_bytes": int(bits.numel()),
      "table_terms_ms": t_tt, "table_transform_ms": t_tf, "vjp_terms_ms": t_vt, "vjp_transform_ms": t_vf,
      "table_winner": "transform" if t_tf < t_tt else "terms", "table_speedup": t_tt / t_tf,
      "vjp_winner": "transform" if t_vf < t_vt else "terms", "vjp_speedup": t_vt / t_vf,
      "transform_passes": passes, "transform_kernel_ms": t_raw, "transform_bytes": moved,
      "transform_tb_per_s": moved / (t_raw * 1e-3) / 1e12, "transform_share_of_8tb_per_s": moved / (t_raw * 1e-3) / HBM_PEAK,
      "table_max_abs_difference": float((results["table_terms"] - results["table_transform"]).abs().max()),
      "table_scale": norm,
      "vjp_max_abs_difference": float((results["vjp_terms"] - results["vjp_transform"]).abs().max()),
      "vjp_scale": float(weights.sum()),
  }
  del bits, weights, scratch, raw, results
  torch.cuda.empty_cache()
  return row


def time_qmhl(order, n, reps, states, layers):
  """One QMHL step (loss + backward) on fixed data samples with the model's modular Hamiltonian measured through its
  table (`energy_tables="all"`): "terms" = today's tables on both sides (the quantum inference's and the analytic EBM
  inference's), "transform" = both by the Walsh-Hadamard transform."""
  dev = "cuda"
  qubits = ir.GridQubit.rect(1, n)
  samples = torch.from_numpy(np.random.default_rng(1).integers(0, 2, (states, n)).astype(np.int8))
  steps, losses = {}, {}
  for way in ("terms", "transform"):
    torch.manual_seed(0)
    energy = models.KOBE(list(range(n)), order).to(dev)
    model_circuit = models.DirectQuantumCircuit(hea(qubits, layers, "m"), tfq_compat_bit_order=False).to(dev)
    data_circuit = models.DirectQuantumCircuit(hea(qubits, layers, "d"), tfq_compat_bit_order=False).to(dev)
    with torch.no_grad():
      model_circuit.trainable_variables[0].uniform_(-1, 1)
      data_circuit.trainable_variables[0].uniform_(-1, 1)
    data_circuit.trainable_variables[0].requires_grad_(False)
    e_inf = inference.AnalyticEnergyInference(energy, 16, initial_seed=1,
                                              table="transform" if way == "transform" else "bitstrings")
    qhbm = inference.QHBM(e_inf, inference.AnalyticQuantumInference(model_circuit))
    data_q = inference.AnalyticQuantumInference(data_circuit, energy_tables="all", max_table_qubits=max(24, n),
                                                parity_tables=way)
    source = FixedData(samples, data_q)
    variables = list(energy.parameters()) + model_circuit.trainable_variables

    def step(source=source, qhbm=qhbm, variables=variables, way=way):
      for v in variables:
        v.grad = None
      loss = inference.qmhl(source, qhbm)
      loss.backward()
      losses[way] = float(loss)

    steps[way] = step
  t_terms, t_transform = timed([steps["terms"], steps["transform"]], reps)
  return {"energy": f"kobe{order}", "n": n, "states": states, "layers": layers, "reps": reps,
          "step_terms_ms": t_terms, "step_transform_ms": t_transform,
          "winner": "transform" if t_transform < t_terms else "terms", "speedup": t_terms / t_transform,
          "loss_terms": losses["terms"], "loss_transform": losses["transform"]}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--out", default=None)
  ap.add_argument("--shapes", default="kobe2:20,kobe3:20,kobe3:24,kobe2:28")
  ap.add_argument("--qmhl", default="kobe3:20")
  ap.add_argument("--qmhl-states", type=int, default=64)
  ap.add_argument("--qmhl-layers", type=int, default=2)
  ap.add_argument("--reps", type=int, default=5)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("parity_table_time.py needs an MI355X: the kernels have no CPU fallback, and a time is measured or "
                     "it is not reported")
  out = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "shapes": [], "qmhl": None}
  for text in [s for s in args.shapes.split(",") if s]:
    row = time_shape(*parse_shape(text), args.reps)
    out["shapes"].append(row)
    print(json.dumps(row), flush=True)
  if args.qmhl:
    out["qmhl"] = time_qmhl(*parse_shape(args.qmhl), args.reps, args.qmhl_states, args.qmhl_layers)
    print(json.dumps(out["qmhl"]), flush=True)
  if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
      json.dump(out, f, indent=1)
      f.write("\n")


if __name__ == "__main__":
  main()
