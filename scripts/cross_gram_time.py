"""Times the cross-Gram kernel (`qhbm_cross_gram`) against the two routes there were before it, on one GPU, in one process.

  python scripts/cross_gram_time.py [--rounds 7] [--step-limit 180] [--out profiles/cross_gram.json]

Reported, not asserted (every figure is from one run on one box).  At (n, M, K) in {(20, 8, 8), (24, 8, 8), (24, 32, 2),
(24, 1, 32)}, alternating the routes round by round (device events around one call each, after a warm-up of each; the median
and the fastest of `--rounds` rounds):
  * cross      one `qhbm_cross_gram` through the C ABI, scratch allocated outside; with the bytes it moves by the model
               ceil(M/4) ceil(K/4) tiles x (rows of the tile x 8 B) x 2^n amplitudes -- one streaming read of a tile's bras
               and kets per tile -- and that rate;
  * concat     what the kernel replaces, exactly: `torch.cat` of both ensembles into one [M + K, 2^n] buffer (a second
               resident copy), then `qhbm_weighted_gram` on M + K states, of which the M x K block is wanted; the copy and
               the kernel are timed together and the kernel alone as well;
  * einsum     torch's complex64 `einsum("ix,jx->ij", conj(a), b)`: float32 accumulation, no fixed order; with torch's
               peak memory above the inputs, and its largest deviation from the kernel's result.
`loses` names the routes that were faster than the new kernel at that shape.
Then the use the tests close the loop with: the fidelity of `thermal_ensemble` to `thermal_sweep` of the 57-term XXZ chain
at 20 qubits from the same two start states, over the product of the traces.
Each step runs under a watchdog of `--step-limit` seconds that ends the process (nothing more is started on the GPU after a
step that hangs).  Prints one JSON line and, with --out, writes it to that file."""
import argparse
import faulthandler
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

from qhbmlib_amd import _engine as E  # noqa: E402
from qhbmlib_amd import inference, ir  # noqa: E402

SHAPES = ((20, 8, 8), (24, 8, 8), (24, 32, 2), (24, 1, 32))


class Step:
  """A watchdog around one step: the process exits (with every thread's traceback) when it runs past the limit."""

  def __init__(self, name, limit):
    self.name, self.limit = name, limit

  def __enter__(self):
    print(f"[cross_gram_time] {self.name}", file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(self.limit, exit=True)

  def __exit__(self, *exc):
    faulthandler.cancel_dump_traceback_later()
    return False


def once_ms(fn):
  begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  begin.record()
  out = fn()
  end.record()
  torch.cuda.synchronize()
  return begin.elapsed_time(end), out


def cross_model_bytes(n, num_a, num_b):
  """sum over the tiles of (bras + kets of the tile) x 8 bytes x 2^n: every tile streams its own rows once."""
  rows = 0
  for i0 in range(0, num_a, 4):
    for j0 in range(0, num_b, 4):
      rows += min(4, num_a - i0) + min(4, num_b - j0)
  return rows * 8 * (1 << n)


def check(rc, lib):
  if rc != 0:
    raise RuntimeError(lib.qhbm_last_error(None).decode())


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument("--rounds", type=int, default=7)
  ap.add_argument("--step-limit", type=int, default=180)
  ap.add_argument("--out", default=None)
  args = ap.parse_args()
  if not torch.cuda.is_available():
    raise SystemExit("cross_gram_time needs a GPU: nothing is timed on a CPU")
  lib = E.load_library()
  stream = lambda: torch.cuda.current_stream().cuda_stream
  line = {"gpu": torch.cuda.get_device_name(0), "rounds": args.rounds, "one_run_on_one_box": True, "shapes": []}

  def flush():
    text = json.dumps(line)
    if args.out:
      with open(args.out, "w") as f:
        f.write(text + "\n")
    return text

  for n, num_a, num_b in SHAPES:
    with Step(f"n={n} M={num_a} K={num_b}", args.step_limit):
      bras, kets = E.random_states(num_a, n, 2), E.random_states(num_b, n, 3)
      scratch = torch.empty(E.cross_gram_scratch_bytes(num_a, num_b, n) // 8, dtype=torch.float64, device="cuda")
      out = torch.empty((num_a, num_b, 2), dtype=torch.float64, device="cuda")
      both = num_a + num_b
      gram_scratch = torch.empty(E.gram_scratch_bytes(both, n) // 8, dtype=torch.float64, device="cuda")
      gram_out = torch.empty((both, both, 2), dtype=torch.float64, device="cuda")

      def cross():
        check(lib.qhbm_cross_gram(bras.data_ptr(), num_a, kets.data_ptr(), num_b, n, None, scratch.data_ptr(), out.data_ptr(),
                                  stream()), lib)

      def gram_of(buffer):
        check(lib.qhbm_weighted_gram(buffer.data_ptr(), both, n, None, gram_scratch.data_ptr(), gram_out.data_ptr(), stream()), lib)

      def concat():
        buffer = torch.cat([bras, kets], 0)
        gram_of(buffer)
        return buffer

      def einsum():
        return torch.einsum("ix,jx->ij", bras.conj(), kets)

      held = concat()           # warm-ups, and the buffer for the kernel-alone figure
      cross()
      loose = einsum()
      torch.cuda.synchronize()
      exact = torch.view_as_complex(out).clone()
      block = torch.view_as_complex(gram_out)[:num_a, num_a:].clone()
      base = torch.cuda.memory_allocated()
      torch.cuda.reset_peak_memory_stats()
      einsum()
      torch.cuda.synchronize()
      einsum_peak = torch.cuda.max_memory_allocated() - base
      times = {"cross": [], "concat": [], "concat_kernel_alone": [], "einsum": []}
      for _ in range(args.rounds):
        times["cross"].append(once_ms(cross)[0])
        times["concat"].append(once_ms(concat)[0])
        times["concat_kernel_alone"].append(once_ms(lambda: gram_of(held))[0])
        times["einsum"].append(once_ms(einsum)[0])
      row = {"qubits": n, "bras": num_a, "kets": num_b}
      for key, values in times.items():
        row[key + "_ms_median"], row[key + "_ms_min"] = statistics.median(values), min(values)
      moved = cross_model_bytes(n, num_a, num_b)
      row.update({
          "cross_model_bytes": moved, "cross_model_bytes_per_s": moved / (row["cross_ms_median"] * 1e-3),
          "unique_bytes": both * 8 * (1 << n), "concat_extra_resident_bytes": both * 8 * (1 << n),
          "pairs_wanted": num_a * num_b, "pairs_concat_sums": both * (both + 1) // 2,
          "einsum_peak_bytes_above_inputs": int(einsum_peak),
          "einsum_max_abs_deviation": float((loose.to(torch.complex128) - exact).abs().max()),
          "concat_block_equals_cross_bits": bool(torch.equal(torch.view_as_real(block), torch.view_as_real(exact))),
          "loses": [key for key in ("concat", "einsum") if row[key + "_ms_median"] < row["cross_ms_median"]]})
      line["shapes"].append(row)
      del bras, kets, scratch, out, gram_scratch, gram_out, held, loose, exact, block
      torch.cuda.empty_cache()
    flush()

  with Step("thermal ensembles at 20 qubits", args.step_limit):
    n, beta = 20, 0.5
    qubits = ir.GridQubit.rect(1, n)
    xxz = ir.PauliSum()
    for a, b in zip(qubits[:-1], qubits[1:]):
      xxz += ir.PX(a) * ir.PX(b) + ir.PY(a) * ir.PY(b) + 0.5 * ir.PZ(a) * ir.PZ(b)
    chebyshev = inference.thermal_ensemble([xxz], beta, num_vectors=2, seed=5)
    krylov = inference.thermal_sweep([xxz], [beta], num_vectors=2, num_steps=24, seed=5).ensemble(beta)
    got = inference.ensemble_metrics(chebyshev, krylov)
    line["thermal_20_qubits"] = {"beta": beta, "terms": len(xxz.terms), "vectors": 2, "krylov_steps": 24, "trace_a": got.trace_a,
                                 "trace_b": got.trace_b, "overlap": got.overlap, "fidelity": got.fidelity,
                                 "fidelity_over_traces": got.fidelity / (got.trace_a * got.trace_b),
                                 "trace_distance": got.trace_distance}
  print(flush())


if __name__ == "__main__":
  main()
