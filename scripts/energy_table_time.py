"""Times one QMHL step through the host mirror with the model's modular Hamiltonian measured through its energy TABLE
(`AnalyticQuantumInference(energy_tables=...)`, one streaming pass of csrc/energy_table.hip over the final states) or
through its Pauli shards (the default route, KOBE only), on fixed data samples.

  python scripts/energy_table_time.py --n 20 --states 4096 --energy kobe2|mlp --route table|shards [--steps 3]

Prints one JSON line: the step time (ms, mean over --steps after a warm-up step), the time and launch count per step of
the engine's `obs` bucket (--route table: the table kernel and its finishing launches; shards: lambda = O psi and the
value launches), the byte model of the table kernel per step -- the retaining forward reads psi once (8 B per
amplitude), the backward reads psi and writes lambda (16 B) --, the rate that gives, and `parity`: the values of two
data states against the C oracle (qhbm_cpu statevectors, fp64 energies)."""
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

from oracle import qhbm_cpu  # noqa: E402
from oracle import qhbm_oracle as O  # noqa: E402
from qhbmlib_amd import data, inference, ir, models  # noqa: E402


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


def table_f64(energy, kind, n):
  """The energy of every bitstring in fp64, restated on the host (row y = y read big-endian)."""
  rows = O.all_bitstrings(n)
  if kind == "kobe2":
    return O.kobe_energy(rows, energy.post_process[0].kernel.detach().cpu().double().numpy(), 2)
  lin = [l for l in energy.energy_layers if isinstance(l, torch.nn.Linear)]
  w1, b1, w2, b2 = [t.detach().cpu().double() for l in lin for t in (l.weight, l.bias)]
  spins = 1.0 - 2.0 * torch.from_numpy(rows.astype(np.float64))
  return (torch.tanh(spins @ w1.T + b1) @ w2.T + b2).reshape(-1).numpy()


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--n", type=int, default=12)
  ap.add_argument("--states", type=int, default=1024)
  ap.add_argument("--energy", choices=("kobe2", "mlp"), default="kobe2")
  ap.add_argument("--route", choices=("table", "shards"), default="table")
  ap.add_argument("--layers", type=int, default=4)
  ap.add_argument("--steps", type=int, default=3)
  args = ap.parse_args()
  if args.route == "shards" and args.energy != "kobe2":
    raise SystemExit("--route shards needs a Pauli energy (--energy kobe2)")
  n, dev = args.n, "cuda"
  torch.manual_seed(0)
  qubits = ir.GridQubit.rect(1, n)
  if args.energy == "kobe2":
    energy = models.KOBE(list(range(n)), 2).to(dev)
  else:
    energy = models.BitstringEnergy(list(range(n)), [models.SpinsFromBitstrings(), torch.nn.Linear(n, 8),
                                                     torch.nn.Tanh(), torch.nn.Linear(8, 1)]).to(dev)
  model_circuit = models.DirectQuantumCircuit(hea(qubits, args.layers, "m"), tfq_compat_bit_order=False).to(dev)
  data_circuit = models.DirectQuantumCircuit(hea(qubits, args.layers, "d"), tfq_compat_bit_order=False).to(dev)
  with torch.no_grad():
    model_circuit.trainable_variables[0].uniform_(-1, 1)
    data_circuit.trainable_variables[0].uniform_(-1, 1)
  data_circuit.trainable_variables[0].requires_grad_(False)
  mode = "off" if args.route == "shards" else ("all" if args.energy == "kobe2" else "general")
  qhbm = inference.QHBM(inference.AnalyticEnergyInference(energy, 16, initial_seed=1),
                        inference.AnalyticQuantumInference(model_circuit))
  data_q = inference.AnalyticQuantumInference(data_circuit, energy_tables=mode)
  rng = np.random.default_rng(1)
  samples = torch.from_numpy(rng.integers(0, 2, (args.states, n)).astype(np.int8))
  source = FixedData(samples, data_q)
  variables = list(energy.parameters()) + model_circuit.trainable_variables

  def step():
    for v in variables:
      v.grad = None
    loss = inference.qmhl(source, qhbm)
    loss.backward()
    return loss

  step()  # warm-up: plans, workspaces, the energy's table rows
  engines = list(data_q._engines._engines.values())  # pylint: disable=protected-access
  for eng in engines:
    eng.set_option("profile_events", 1)
    eng.kernel_time_ms(reset=True)
  torch.cuda.synchronize()
  t0 = time.perf_counter()
  for _ in range(args.steps):
    loss = step()
  torch.cuda.synchronize()
  step_ms = (time.perf_counter() - t0) * 1e3 / args.steps
  obs_ms, obs_launches = 0.0, 0
  for eng in engines:
    t = eng.kernel_time_ms(reset=True)
    obs_ms += t["obs_ms"]
    obs_launches += t["obs_launches"]
    eng.set_option("profile_events", 0)
  obs_ms /= args.steps
  unique = int(torch.unique(samples, dim=0).shape[0])
  model_bytes = 24.0 * (1 << n) * unique

  ham = qhbm.modular_hamiltonian
  with torch.no_grad():
    got = data_q.expectation(samples[:2], ham).cpu().numpy()[:, 0]
  total = data_circuit + ham.circuit_dagger
  gates = total.pqc.flat_gates(total.qubits, total.symbol_names)
  params = total.symbol_values.detach().cpu().numpy().astype(np.float32)
  table = table_f64(energy, args.energy, n)
  states = qhbm_cpu.statevector(n, gates, params, samples[:2].numpy())
  want = (np.abs(states.astype(np.complex128)) ** 2) @ table
  scale = float(np.abs(table).max())
  err = float(np.abs(got - want).max())
  table_route = args.route == "table"
  print(json.dumps({
      "n": n, "states": args.states, "unique_states": unique, "energy": args.energy, "route": args.route,
      "layers": args.layers, "steps": args.steps, "loss": float(loss), "step_ms": step_ms,
      "table_kernel_ms": obs_ms, "table_launches": obs_launches // args.steps,
      "model_bytes": model_bytes if table_route else None,
      "tb_per_s": model_bytes / (obs_ms * 1e-3) / 1e12 if table_route and obs_ms > 0 else None,
      "parity": {"max_abs_err": err, "scale": scale, "ok": bool(err <= 1e-4 * max(scale, 1.0))},
  }))


if __name__ == "__main__":
  main()
