"""Inputs of the loss tests (tests/test_loss_ref_cpu.py, tests/test_losses_hamiltonian_gpu.py), built with numpy
generators only, and the expected side from tests/loss_ref.py, computed once per process.

A case holds two parts, each a spin-parity energy plus a hardware-efficient ansatz with its own symbol names:

  a -- the model QHBM (E_theta, U_phi);
  b -- the target Hamiltonian of `vqt` (K_vartheta, V_psi), and the data QHBM of `qmhl` (E^d_thetad, U^d_phid);

and an explicit multiset: at most 8 distinct bitstrings with unequal counts, one of them 1.  The GPU tests impose it with
`e_inference.fixed_samples(bitstrings, counts)`, so both sides see the same inputs.

Sizes: 3 qubits is a single tile; 13 qubits is the smallest size at which the default plans have more than one pass.
The bit-order cases (`compat`: both circuits built with tfq_compat_bit_order=True) are at 12 qubits -- the permutation
is non-trivial from 11 on -- and at 20 qubits with 4 states and one layer per circuit, where the C oracle takes over.
"""
import functools

import numpy as np

from oracle import qhbm_oracle as O
from tests import loss_ref as R

COUNTS = [7, 1, 3, 12, 5, 2, 9, 4]

#             n  order a/b   layers a/b  states beta  seed  compat
SPECS = {
    "n3": (3, (2, 2), (2, 2), 5, 0.625, 3, False),
    "n3_bernoulli": (3, (None, None), (1, 2), 6, 1.75, 4, False),
    "n4": (4, (2, 2), (2, 1), 6, 1.0, 5, False),
    "n13": (13, (2, 2), (2, 1), 8, 0.625, 13, False),
    "n12_compat": (12, (2, 2), (2, 1), 4, 1.75, 12, True),
    "n20_compat": (20, (2, 2), (1, 1), 4, 1.0, 21, True),
}
LOSS_CASES = ["n3", "n3_bernoulli", "n13"]
COMPAT_CASES = ["n12_compat", "n20_compat"]
SELF_CASE = "n3_self"          # part b is part a under other symbol names; small weights (see `self_sampling_sigma`)
SELF_THETA_SCALE = 0.1
SELF_SAMPLES = 200000


def _f32(x):
  """Rounded to float32, kept as float64: the mirror's float32 variables then hold exactly the reference's inputs."""
  return np.asarray(x, dtype=np.float32).astype(np.float64)


def _part(rng, n, order, layers, name, theta_scale=1.0):
  n_theta = n if order is None else len(O.parity_indices(n, order))
  magnitude = theta_scale * rng.uniform(0.2, 1.0, n_theta)   # bounded away from 0: every shard carries weight
  return dict(order=order, layers=layers, name=name, thetas=_f32(magnitude * rng.choice([-1.0, 1.0], n_theta)),
              values=_f32(rng.uniform(-1.0, 1.0, len(O.hea_symbol_names(n, layers, name)))))


@functools.lru_cache(maxsize=None)
def case(name):
  if name == SELF_CASE:
    return _self_case()
  n, orders, layers, states, beta, seed, compat = SPECS[name]
  rng = np.random.default_rng(seed)
  a = _part(rng, n, orders[0], layers[0], "a")
  b = _part(rng, n, orders[1], layers[1], "b")
  bits = _rows(rng, n, states)
  if compat:   # every row must change under the injector permutation
    assert (O.apply_bit_order(bits, True) != bits).any(axis=1).all(), name
  return dict(name=name, n=n, beta=beta, compat=compat, a=a, b=b, bits=bits, counts=np.array(COUNTS[:states], np.int64))


def _rows(rng, n, states):
  picked = rng.choice(1 << n, size=states, replace=False)                 # distinct rows
  return ((picked[:, None] >> np.arange(n - 1, -1, -1)[None, :]) & 1).astype(np.int8)


def _self_case():
  """qmhl_loss_test.py:48-80: the data QHBM carries the model's weights (other symbol names, the same values)."""
  n, rng = 3, np.random.default_rng(33)
  a = _part(rng, n, 2, 2, "a", SELF_THETA_SCALE)
  return dict(name=SELF_CASE, n=n, beta=1.0, compat=False, a=a, b=dict(a, name="b"), bits=_rows(rng, n, 5),
              counts=np.array(COUNTS[:5], np.int64))


def self_sampling_sigma():
  """Standard deviation of the self-QMHL loss over SELF_SAMPLES model samples: with the data equal to the model every
  per-sample value is E_theta(x), so it is sqrt(Var_p E / N)."""
  e = energy(case(SELF_CASE)["a"], 3)
  p, values = e.probabilities(), e.energy(O.all_bitstrings(3))
  return float(np.sqrt((p @ values**2 - (p @ values)**2) / SELF_SAMPLES))


def energy(part, n):
  return R.SpinEnergy(n, part["thetas"], part["order"])


def gates(part, n):
  return O.hea_gates(n, part["layers"], part["name"])[0]


def vqt_reference(c, **overrides):
  """R.vqt_hamiltonian on the case: model a, target b."""
  n, a, b = c["n"], c["a"], c["b"]
  kw = dict(model_energy=energy(a, n), model_gates=gates(a, n), phi=a["values"], target_energy=energy(b, n),
            target_gates=gates(b, n), psi=b["values"], beta=c["beta"], bits=c["bits"], weights=c["counts"],
            tfq_compat=c["compat"])
  kw.update(overrides)
  return R.vqt_hamiltonian(n, **kw)


def qmhl_reference(c, **overrides):
  """R.qmhl_qhbm_data on the case: data b, model a."""
  n, a, b = c["n"], c["a"], c["b"]
  kw = dict(data_energy=energy(b, n), data_gates=gates(b, n), phid=b["values"], model_energy=energy(a, n),
            model_gates=gates(a, n), phi=a["values"], bits=c["bits"], weights=c["counts"], tfq_compat=c["compat"])
  kw.update(overrides)
  return R.qmhl_qhbm_data(n, **kw)


@functools.lru_cache(maxsize=None)
def expected_vqt(name):
  return vqt_reference(case(name))


@functools.lru_cache(maxsize=None)
def expected_qmhl(name):
  return qmhl_reference(case(name))


def permuted_shards(part, n):
  """The WRONG shards of a bit-order case: every Z string moved to the qubits the injector permutation names."""
  perm = O.tfq_bit_permutation(n)
  return [[(c, x, sum(1 << perm[q] for q in range(n) if (z >> q) & 1)) for c, x, z in op] for op in energy(part, n).shards]


@functools.lru_cache(maxsize=None)
def expected_modular(name, injector=True, shards=False):
  """[U] of <x| U_a^dag (V_b K_b V_b^dag) U_a |x> on the case's rows.  `injector=True, shards=False` is what the
  bit-order flag asks for; the other combinations are the two wrong behaviours."""
  c = case(name)
  n, a, b = c["n"], c["a"], c["b"]
  ham = energy(b, n)
  if shards:
    ham = R.SpinEnergy(n, ham.thetas, ham.order, permuted_shards(b, n))
  return R.modular_expectation(n, gates(a, n), a["values"], ham, gates(b, n), b["values"], c["bits"],
                               tfq_compat=c["compat"] and injector)[0]


# ---- the project's bars (SURVEY.md 8c and the tests named) ----------------------------------------------------------
def loss_bar(beta, thetas):
  """tests/test_ebm_gpu.py: 5e-5 * (beta * sum|c_k| + 1)."""
  return 5e-5 * (beta * float(np.abs(thetas).sum()) + 1.0)


def circuit_bar(want):
  return 1e-4 * max(1.0, float(np.abs(want).max()))


def shift_bar(want):
  return 3e-4 * max(1.0, float(np.abs(want).max()))


def shard_bar(beta):
  """Single Pauli strings (tests/test_golden_large_gpu.py): 5e-5 per unit coefficient."""
  return 5e-5 * beta


SCORE_BAR = 2e-4   # tests/test_ebm_gpu.py
