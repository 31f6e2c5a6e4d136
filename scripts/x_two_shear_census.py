"""Which share of the X**t micro-op EXECUTIONS of a workload's plans sits next to a FULL diagonal table -- the gates that
may run as two shears (csrc/x_shear.h).  Planning only, no GPU:
    python scripts/x_two_shear_census.py [--qubits 20 --layers 16]  > profiles/x_two_shear_census.txt
The plan description lists, per pass and round, the X micro-ops inside FULL records and all X micro-ops (`x_full=`) and
the round's dead-wave mask (`dead=`, adjoint); a round's micro-ops execute on  live tiles x waves per tile x
2^-popcount(dead)  waves per state.  The live tiles come from `op_census`, whose X column must equal the sum formed here
(checked; a wider last forward pass counted with its own waves): the eligible executions are weighted exactly as the executed ones."""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  sys.path.insert(0, p)
from oracle import qhbm_oracle as O  # noqa: E402
from qhbmlib_amd import _engine as E  # noqa: E402


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--qubits", type=int, default=20)
  ap.add_argument("--layers", type=int, default=16)
  args = ap.parse_args()
  n, layers = args.qubits, args.layers
  gates, names = O.hea_gates(n, layers, "c")
  eng = E.Engine(None)
  eng.set_circuit(n, gates, len(names))
  eng.set_observables([O.xxz_chain_op(n)])
  text = eng.describe_schedule()
  print(f"x_two_shear census: {n}-qubit XXZ, depth-{layers} hardware-efficient ansatz ({len(gates)} gates, "
        f"{sum(g[0] == O.GATE_XPOW for g in gates)} of them X**t)")
  plans = text.split("adjoint")[0], text[text.index("adjoint"):]
  shares = {}
  for (plan, adjoint), part in zip((("forward", False), ("adjoint", True)), plans):
    line = next(l for l in part.splitlines() if "census:" in l)
    x = int(re.search(r" X=(\d+)", line).group(1))
    xf = int(re.search(r"X-in-FULL=(\d+)", line).group(1))
    full = re.search(r"instances=(\d+) \(FULL (\d+)\)", line)
    rows = eng.op_census(adjoint=adjoint)
    print(f"{plan}: instances {full.group(1)} (FULL {full.group(2)}), X micro-ops {x}, next to a FULL table {xf} "
          f"-> static share {xf / max(x, 1):.4f}")
    tot = tot_f = 0.0
    passes = [l for l in part.splitlines() if l.startswith("  pass ")]
    assert len(passes) == len(rows), (len(passes), len(rows))
    K_plan = int(re.search(r"tile_bits=(\d+)", part).group(1))
    for i, (l, r) in enumerate(zip(passes, rows)):
      K = int(re.search(r"K=(\d+)", l).group(1))
      pairs = [tuple(map(int, t.split("/"))) for t in re.search(r"x_full=(\S*)", l).group(1).split(",") if t]
      dead = [int(t, 16) for t in re.search(r"dead=(\S*)", l).group(1).split(",") if t] if adjoint else [0] * len(pairs)
      waves = r["tiles"] * (1 << (K - 4)) / 64.0
      ex = sum(waves * b / (1 << bin(d).count("1")) for (a, b), d in zip(pairs, dead))
      exf = sum(waves * a / (1 << bin(d).count("1")) for (a, b), d in zip(pairs, dead))
      # (op_census counts the waves of the PLAN's tile size; a wider last forward pass has 2^(K - K_plan) times as many)
      assert abs(ex / (1 << (K - K_plan)) - (r["x"] + r["x_no_slot"])) < 1e-6 * max(1.0, ex), (plan, i, ex, r["x"] + r["x_no_slot"])
      print(f"  pass {i}: live tiles per state {r['tiles']:.0f}, X executions {ex:.0f}, of them next to a FULL table {exf:.0f}"
            + (f" ({exf / ex:.3f})" if ex else ""))
      tot += ex
      tot_f += exf
    shares[plan] = tot_f / tot
    print(f"{plan}: X executions per state {tot:.0f} (wave-executions, checked against op_census), eligible {tot_f:.0f} "
          f"-> EXECUTED share {tot_f / tot:.4f}")
  print("with exponents uniform over a period, 2/3 of the eligible gates fall under theta_max = pi / 3:")
  print(f"  forward  X = 6 of ~13.3 flop per amplitude (0.45): saving 0.45 x 1/3 x 2/3 x {shares['forward']:.3f} = "
        f"{0.45 / 3 * 2 / 3 * shares['forward']:.4f} of the sweep's gate arithmetic")
  print(f"  adjoint  X un-application = 0.31 of the VALU instructions: saving 0.31 x 1/3 x 2/3 x {shares['adjoint']:.3f} = "
        f"{0.31 / 3 * 2 / 3 * shares['adjoint']:.4f}")


if __name__ == "__main__":
  main()
