"""Two independent dense simulators on the cases of tests/golden/plan_fuzz_cases.json: the numpy oracle
(oracle/qhbm_oracle.py) against the values and gradients the C++ oracle of tests/sanitize/plan_emulate.cpp wrote into the
fixture (plan_fuzz --dump-cases).  Both work in complex128 on unit vectors with at most a few hundred gates and terms:
they agree to 1e-10 or one of them is wrong.  No GPU, no build."""
import json
import os

import numpy as np

from oracle import qhbm_oracle as O

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_fuzz_cases.json")


def load_cases():
  with open(FIXTURE) as f:
    return json.load(f)["cases"]


def _f32(x):
  """The fixture prints every float32 the generator drew with 9 significant digits: back through float32, exactly."""
  return float(np.float32(x))


def case_inputs(case):
  gates = [tuple(g[:4]) + (_f32(g[4]), _f32(g[5]), _f32(g[6])) for g in case["gates"]]
  ops = [[(_f32(c), int(x), int(z)) for c, x, z in op] for op in case["observables"]]
  params = np.asarray(case["params"], dtype=np.float32).astype(np.float64)
  bits = np.asarray(case["bitstrings"], dtype=np.int8)
  up = np.asarray(case["upstream"], dtype=np.float32).astype(np.float64)
  return gates, ops, params, bits, up


def test_fixture_sample_covers_every_feature_twice():
  cases = load_cases()
  seen = {}
  for c in cases:
    for f in c["features"]:
      seen[f] = seen.get(f, 0) + 1
  wanted = ["fwd_multi_pass", "adj_multi_pass", "relabel", "no_zero_fill", "dense_tail", "early_measure", "measure_only_pass",
            "wht", "global_terms", "wide_pass", "general", "gate2", "full", "cph_tile", "cph_thread", "dead_mask", "forced_order",
            "grad_mask", "padded"]
  assert all(seen.get(f, 0) >= 2 for f in wanted), seen
  assert 4 * sum(10 <= c["n"] <= 16 for c in cases) >= 3 * len(cases)
  assert os.path.getsize(FIXTURE) <= max(os.path.getsize(os.path.join(os.path.dirname(FIXTURE), f))
                                         for f in os.listdir(os.path.dirname(FIXTURE)) if f.endswith(".npz"))


def test_numpy_oracle_and_cpp_oracle_agree():
  worst_v = worst_g = 0.0
  for case in load_cases():
    gates, ops, params, bits, up = case_inputs(case)
    vals, jac = O.expectation_jacobian(case["n"], gates, params, bits, ops)
    grads = np.einsum("t,btp->bp", up, jac)
    dv = np.abs(vals - np.asarray(case["oracle_values"])).max()
    dg = np.abs(grads - np.asarray(case["oracle_gradients"])).max()
    worst_v, worst_g = max(worst_v, dv), max(worst_g, dg)
    assert dv <= 1e-10 and dg <= 1e-10, (case["case"], dv, dg)
  print(f"largest difference: values {worst_v:.3g}, gradients {worst_g:.3g} (bar 1e-10)")
