"""Times the BKM information matrix two ways, alternating, in one process (warm-up, device synchronisation):

  batched  `inference.information_matrix`: one qhbm_program_vjps call (every shifted occurrence a program);
  loop     the reference's form (baselines/train.py:161-249) through the mirror: for every circuit variable and
           shift +-1/2, `AnalyticQuantumInference.expectation(bits, Hamiltonian(copy))` + `torch.autograd.grad`,
           2 P_c calls, on the SAME weighted bitstrings.

Prints one JSON line per shape: programs, element-states (programs x unique states), seconds of both forms and the
max |difference| of the rows both computed.  `--loop-rows R` times only the first R variables of the loop (the
per-row time is then measured on those rows, and the difference is taken over them).

  python scripts/info_matrix_time.py [--shapes ref,c2,c3] [--repeats 2] [--loop-rows 0]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

from qhbmlib_amd import inference, ir, models, utils  # noqa: E402
from qhbmlib_amd.inference import information  # noqa: E402

SHAPES = {  # name: (qubits, layers, samples or None = exact)
    "ref": (4, 7, 500),     # the reference experiment: 4 qubits, qhea 7 layers, KOBE-2 (D = 87)
    "c2": (12, 8, 1024),    # BASELINE config 2's shape (D = 358)
    "c3": (20, 16, 16),     # config 3's circuit, 16 samples (1888 programs, D = 1154)
}


def hea(qubits, layers, name):
  """The qhea ansatz of the reference's experiments: X**s, Z**s per qubit, CZ**s on a brick of pairs."""
  circuit = ir.Circuit()
  for layer in range(layers):
    for i, q in enumerate(qubits):
      circuit += [ir.X(q)**ir.Symbol(f"sx_{name}_{layer}_{i}"), ir.Z(q)**ir.Symbol(f"sz_{name}_{layer}_{i}")]
    pairs = list(zip(qubits[::2], qubits[1::2])) + list(zip(qubits[1::2], qubits[2::2]))
    for i, (q0, q1) in enumerate(pairs):
      circuit += ir.CZPowGate(ir.Symbol(f"sc_{name}_{layer}_{i}"))(q0, q1)
  return circuit


def build(n, layers, device="cuda", seed=0):
  """(qhbm, copy Hamiltonian with its own symbols and the same variable values)."""
  torch.manual_seed(seed)
  qubits = ir.GridQubit.rect(1, n)
  energy = models.KOBE(list(range(n)), 2).to(device)
  circuit = models.DirectQuantumCircuit(hea(qubits, layers, "m"), tfq_compat_bit_order=False).to(device)
  qhbm = inference.QHBM(inference.AnalyticEnergyInference(energy, 16, initial_seed=seed),
                        inference.AnalyticQuantumInference(circuit))
  energy_copy = models.KOBE(list(range(n)), 2).to(device)
  circuit_copy = models.DirectQuantumCircuit(hea(qubits, layers, "c"), tfq_compat_bit_order=False).to(device)
  with torch.no_grad():
    for c, v in zip(energy_copy.trainable_variables + circuit_copy.trainable_variables,
                    energy.trainable_variables + circuit.trainable_variables):
      c.copy_(v)
  return qhbm, models.Hamiltonian(energy_copy, circuit_copy)


def mirror_loop(qhbm, copy, bits, weights, rows=None):
  """(cross [R, P_e], qnn [R, P_c]) of train.py:190-240 through the mirror, on fixed weighted bitstrings."""
  variable = qhbm.modular_hamiltonian.circuit.trainable_variables[0]
  copy_vars = [copy.energy.trainable_variables[0], copy.circuit.trainable_variables[0]]
  base = variable.detach().clone()
  w = weights.to(device=bits.device, dtype=torch.float32)
  cross, qnn = [], []

  def grads(i, shift):
    with torch.no_grad():
      variable.copy_(base)
      variable[i] += shift
    f = torch.sum(w * qhbm.q_inference.expectation(bits, copy)[:, 0])
    return torch.autograd.grad(f, copy_vars)

  try:
    for i in range(base.numel() if rows is None else min(rows, base.numel())):
      ge_lo, gc_lo = grads(i, -0.5)
      ge_hi, gc_hi = grads(i, 0.5)
      cross.append(0.5 * math.pi * (ge_lo - ge_hi))
      qnn.append(0.5 * math.pi * (gc_lo - gc_hi))
  finally:
    with torch.no_grad():
      variable.copy_(base)
  return torch.stack(cross), torch.stack(qnn)


def fixed_samples(qhbm, num_samples):
  bits, _, counts = utils.unique_bitstrings_with_counts(qhbm.e_inference.sample(num_samples))
  return bits, counts.to(torch.float64) / float(num_samples)


def time_shape(name, repeats, loop_rows):
  n, layers, samples = SHAPES[name]
  qhbm, copy = build(n, layers)
  bits, weights = fixed_samples(qhbm, samples)
  e_inf = qhbm.e_inference
  # the batched form draws its samples from the EBM: hand it the same set
  e_inf.sample = lambda num, _b=bits, _w=weights: _b.repeat_interleave(
      torch.round(_w * num).to(torch.long).to(_b.device), 0)
  n_e = copy.energy.trainable_variables[0].numel()
  best = {"batched": float("inf"), "loop": float("inf")}
  matrix = loop = None
  for rep in range(repeats + 1):   # repetition 0 is the warm-up
    for form in ("batched", "loop"):
      torch.cuda.synchronize()
      t0 = time.perf_counter()
      if form == "batched":
        matrix = information.information_matrix(qhbm, num_samples=samples, symmetrize=False)
      else:
        loop = mirror_loop(qhbm, copy, bits, weights, loop_rows or None)
      torch.cuda.synchronize()
      if rep:
        best[form] = min(best[form], time.perf_counter() - t0)
  rows = loop[0].shape[0]
  delta = max(float((matrix[n_e:n_e + rows, :n_e] - loop[0].to(matrix.device)).abs().max()),
              float((matrix[n_e:n_e + rows, n_e:] - loop[1].to(matrix.device)).abs().max()))
  scale = float(matrix.abs().max())
  programs = 2 * sum(1 for g in qhbm.modular_hamiltonian.circuit.pqc.flat_gates(
      qhbm.modular_hamiltonian.circuit.qubits, qhbm.modular_hamiltonian.circuit.symbol_names) if g[3] >= 0)
  return {"shape": name, "qubits": n, "layers": layers, "samples": samples, "unique_states": int(bits.shape[0]),
          "D": int(matrix.shape[0]), "programs": programs, "element_states": programs * int(bits.shape[0]),
          "batched_s": best["batched"], "loop_rows": rows, "loop_s": best["loop"],
          "loop_s_per_row": best["loop"] / rows, "max_abs_delta": delta, "max_abs_entry": scale}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--shapes", default="ref,c2,c3")
  ap.add_argument("--repeats", type=int, default=2)
  ap.add_argument("--loop-rows", type=int, default=0, help="time only this many loop rows (0 = all)")
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("needs an MI355X")
  for name in args.shapes.split(","):
    print(json.dumps(time_shape(name, args.repeats, args.loop_rows)), flush=True)


if __name__ == "__main__":
  main()
