#!/usr/bin/env python
"""One SHA-256 per (entry point, case, chunking) over the raw bytes of every output tensor of the engine's circuit
entry points: the A/B of a change that must not move a bit.

  QHBM_ENGINE_LIB=<the other build's libqhbm_engine.so> python scripts/entry_point_digests.py --out a.json
  python scripts/entry_point_digests.py --out b.json

The shapes are those of tests/test_sweep_launches_gpu.py (5 states, chunks of 2 / one chunk, tiles of 2^10, the
workspace budget set); on top: the parameter-shift VJP with and without prefix sharing, qhbm_program_vjps with an
unshifted program and one behind the first live gate under a gradient mask, the counting and parity samplers with
three programs, and the Jacobian.  Digests compare builds on one machine; they are not portable across compilers."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "qhbm-library_amd")):
  if _p not in sys.path:
    sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from qhbmlib_amd import _engine as E  # noqa: E402
from tests.test_sweep_launches_gpu import CASES, CHUNK, _Setup, _tensors  # noqa: E402


def digest(out):
  h = hashlib.sha256()
  torch.cuda.synchronize()
  for t in _tensors(out):
    t = t.contiguous()
    if t.is_complex():
      t = torch.view_as_real(t)
    h.update(t.cpu().numpy().tobytes())
  return h.hexdigest()


def calls(s):
  """name -> a call on the setup's engine (the retained VJPs make their own retaining forward)."""
  e = s.eng
  n_gates = 2 * (2 * s.n) + 2 * (s.n - 1)  # the two-layer ansatz of the setup
  needs_grad = [i >= len(s.params) // 2 for i in range(len(s.params))]
  # an unshifted program, two shifted ones, and the last parametrised gate: behind the first live gate under `needs_grad`
  progs = ([-1, 0, 1, n_gates - 1], [0.0, 0.5, -0.5, 0.5])
  three = ([-1, 0, 3], [0.0, 0.5, -0.5])
  masks = [1, 3, (1 << s.n) - 1]

  def retained():
    e.expectation(s.bits, s.params, retain=True)
    return e.expectation_vjp_retained(s.bits, s.params, s.up) if e.retained is not None else None

  def table_retained():
    e.table_expectation(s.bits, s.params, s.table, retain=True)
    return e.table_expectation_vjp_retained(s.bits, s.params, s.table, s.table_up) if e.retained is not None else None

  def shift(sharing):
    e.set_option("shift_prefix_sharing", sharing)
    out = e.expectation_vjp(s.bits, s.params, s.up, method=E.GRAD_PARAMETER_SHIFT)
    e.set_option("shift_prefix_sharing", 1)
    return out

  def masked_program_vjps():
    e.set_gradient_mask(needs_grad)
    out = e.program_vjps(s.bits, s.params, progs[0], progs[1], s.up, row_weights=np.abs(s.table_up))
    e.set_gradient_mask(None)
    return out

  return {
      "expectation": lambda: e.expectation(s.bits, s.params),
      "expectation_retain": lambda: e.expectation(s.bits, s.params, retain=True),
      "expectation_vjp": lambda: (e.expectation_vjp(s.bits, s.params, s.up), e.state_gradients(len(s.bits))),
      "expectation_vjp_retained": retained,
      "expectation_from_states": lambda: e.expectation_from_states(s.states, s.params),
      "expectation_vjp_from_states": lambda: (e.expectation_vjp_from_states(s.states, s.params, s.up),
                                              e.state_gradients(len(s.bits))),
      "statevector": lambda: e.statevector(s.bits, s.params),
      "statevector_from_states": lambda: e.statevector_from_states(s.states, s.params),
      "statevector_vjp_from_states": lambda: e.statevector_vjp_from_states(s.states, s.params, s.cot, want_states=True),
      "table_expectation": lambda: e.table_expectation(s.bits, s.params, s.table),
      "table_expectation_retain": lambda: e.table_expectation(s.bits, s.params, s.table, retain=True),
      "table_expectation_vjp": lambda: e.table_expectation_vjp(s.bits, s.params, s.table, s.table_up),
      "table_expectation_vjp_retained": table_retained,
      "sample": lambda: e.sample(s.bits, s.params, 64, seed=5),
      "sample_shifted": lambda: e.sample(s.bits, s.params, 64, seed=5, shift_gate=1, shift=0.5),
      "expectation_vjp_parameter_shift_sharing0": lambda: shift(0),
      "expectation_vjp_parameter_shift_sharing1": lambda: shift(1),
      "program_vjps": lambda: e.program_vjps(s.bits, s.params, progs[0], progs[1], s.up),
      "program_vjps_masked": masked_program_vjps,
      "sample_counts": lambda: e.sample_counts(s.bits, s.params, 64, seed=9, shift_gates=three[0], shifts=three[1]),
      "sample_parities": lambda: e.sample_parities(s.bits, s.params, masks, 64, seed=9, shift_gates=three[0],
                                                   shifts=three[1]),
      "expectation_jacobian": lambda: e.expectation_jacobian(s.bits, s.params),
  }


def main():
  ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  ap.add_argument("--out", help="write the list here as JSON as well")
  args = ap.parse_args()
  digests = {}
  for case in sorted(CASES):
    s = _Setup(case)
    for name, call in calls(s).items():
      for chunk in (CHUNK, 0):
        s.eng.set_option("chunk_states", chunk)
        key = f"{name}/{case}/chunk_states={chunk}"
        digests[key] = digest(call())
        print(digests[key], key)
  if args.out:
    with open(args.out, "w") as f:
      json.dump(digests, f, indent=1, sort_keys=True)
      f.write("\n")


if __name__ == "__main__":
  main()
