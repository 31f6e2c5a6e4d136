"""The low-rank identities behind `inference.state_metrics`, on the CPU in complex128.

`tests/state_metrics_ref.py` computes every metric of sigma = sum_m w_m |phi_m><phi_m| against rho = U diag(p) U^dagger
from M x M Gram matrices; here it is held to the dense 2^n x 2^n formulas: `oracle.qhbm_oracle.fidelity_direct` (the
sqrtm formula the reference's test uses) and eigendecompositions of sigma and rho.

Tolerances: fidelity rtol 1e-5 -- the direct formula itself moves by 7e-7 between float64 and complex64-rounded inputs
at these sizes, this is two orders above; 1e-4 (the project's fidelity rtol) with an exactly duplicated state, where
sqrt() of an eigenvalue that is 0 up to rounding turns eps into sqrt(eps).  Everything linear or entropic: 1e-10.
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from tests import state_metrics_ref as R

SHAPES = [(4, 1), (4, 3), (6, 5), (8, 8)]
VARIANTS = ["orthonormal", "nonorthogonal", "unnormalised", "duplicate"]
CASES = [(n, m, v) for n, m in SHAPES for v in VARIANTS if not (v == "duplicate" and m == 1)]


def _haar(dim, rng):
  q, r = np.linalg.qr(rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim)))
  return q * (np.diag(r) / np.abs(np.diag(r)))[None, :]


def _ensemble(n, m, variant, rng):
  dim = 1 << n
  raw = rng.normal(size=(m, dim)) + 1j * rng.normal(size=(m, dim))
  weights = rng.uniform(0.2, 1.0, m)
  if variant == "orthonormal":
    states = _haar(dim, rng)[:, :m].T
    weights /= weights.sum()
  elif variant == "unnormalised":  # (norms of order 1: the absolute 1e-10 below is for quantities of order 1)
    states = raw / np.linalg.norm(raw, axis=1, keepdims=True) * rng.uniform(0.5, 1.5, (m, 1))
  else:
    states = raw / np.linalg.norm(raw, axis=1, keepdims=True)
    if variant == "duplicate":
      states[-1] = np.exp(0.7j) * states[0]
  return np.ascontiguousarray(states), weights


def _model(n, rng):
  unitary = _haar(1 << n, rng)
  energies = rng.normal(size=1 << n) * 1.5
  p = np.exp(-energies)
  p /= p.sum()
  return unitary, energies, (unitary * p[None, :]) @ unitary.conj().T


@pytest.mark.parametrize("n,m,variant", CASES)
def test_low_rank_metrics_equal_the_dense_ones(n, m, variant):
  rng = np.random.default_rng(1000 * n + 10 * m + VARIANTS.index(variant))
  unitary, energies, rho = _model(n, rng)
  states, weights = _ensemble(n, m, variant, rng)
  got = R.metrics(unitary, energies, states, weights)
  sigma = R.dense_sigma(states, weights)
  want_f = O.fidelity_direct(rho, sigma)
  print(f"fidelity low-rank {got['fidelity']:.15g} direct {want_f:.15g} rel {abs(got['fidelity'] - want_f) / want_f:.3g}")
  np.testing.assert_allclose(got["fidelity"], want_f, rtol=1e-4 if variant == "duplicate" else 1e-5)
  trace, purity, entropy, rel = R.dense_sigma_metrics(sigma, rho)
  print(f"trace {got['trace'] - trace:.3g} purity {got['purity'] - purity:.3g} entropy {got['entropy'] - entropy:.3g} "
        f"D {got['relative_entropy'] - rel:.3g}")
  np.testing.assert_allclose(got["trace"], trace, rtol=0, atol=1e-10)
  np.testing.assert_allclose(got["purity"], purity, rtol=0, atol=1e-10)
  np.testing.assert_allclose(got["entropy"], entropy, rtol=0, atol=1e-10)
  np.testing.assert_allclose(got["relative_entropy"], rel, rtol=0, atol=1e-10)
  np.testing.assert_allclose(got["overlap"], np.real(np.trace(rho @ sigma)), rtol=0, atol=1e-10)
  assert got["relative_entropy"] == got["cross_entropy"] - got["entropy"]


def test_one_state_gives_its_expectation_of_rho():
  rng = np.random.default_rng(5)
  unitary, energies, rho = _model(5, rng)
  phi = rng.normal(size=32) + 1j * rng.normal(size=32)
  phi /= np.linalg.norm(phi)
  got = R.metrics(unitary, energies, phi[None, :], [1.0])
  want = np.real(phi.conj() @ rho @ phi)
  np.testing.assert_allclose(got["fidelity"], want, rtol=1e-12)
  np.testing.assert_allclose(got["overlap"], want, rtol=1e-12)
  np.testing.assert_allclose(got["entropy"], 0.0, atol=1e-12)
  np.testing.assert_allclose(got["purity"], 1.0, rtol=1e-12)


def test_the_eigen_ensemble_of_rho_has_fidelity_one_and_no_relative_entropy():
  rng = np.random.default_rng(6)
  n = 5
  unitary, energies, _ = _model(n, rng)
  p = np.exp(-energies)
  p /= p.sum()
  got = R.metrics(unitary, energies, unitary.T, p)
  np.testing.assert_allclose(got["fidelity"], 1.0, rtol=1e-12)
  np.testing.assert_allclose(got["relative_entropy"], 0.0, atol=1e-12)
  np.testing.assert_allclose(got["trace"], 1.0, rtol=1e-12)
  np.testing.assert_allclose(got["entropy"], -np.sum(p * np.log(p)), rtol=1e-12)


def test_gram_is_the_weighted_inner_product():
  rng = np.random.default_rng(7)
  s = rng.normal(size=(3, 8)) + 1j * rng.normal(size=(3, 8))
  t = rng.normal(size=8)
  g = R.gram(s, t)
  for i in range(3):
    for j in range(3):
      np.testing.assert_allclose(g[i, j], sum(t[x] * np.conj(s[i, x]) * s[j, x] for x in range(8)), rtol=1e-13)
  assert np.all(R.gram_bound(s, t) >= np.abs(g) - 1e-12)


def test_abi_lists_the_gram_entry_points():
  assert {"qhbm_gram_scratch_bytes", "qhbm_weighted_gram"} <= set(E.ABI_SYMBOLS)


@pytest.mark.skipif(not os.path.exists(E.LIB_PATH), reason="engine library not built")
def test_library_exports_them_and_sizes_the_scratch_without_a_device():
  lib = ctypes.CDLL(E.LIB_PATH)
  for name in ("qhbm_gram_scratch_bytes", "qhbm_weighted_gram"):
    assert hasattr(lib, name)
  assert E.gram_scratch_bytes(1, 1) == 16
  assert E.gram_scratch_bytes(5, 11) == 16 * 25 and E.gram_scratch_bytes(5, 12) == 2 * 16 * 25
  assert E.gram_scratch_bytes(8, 24) == E.gram_scratch_bytes(8, 20) == 16 * 64 * 256
  for bad in ((0, 4), (1025, 4), (4, 0), (4, 32)):
    with pytest.raises(E.EngineError):
      E.gram_scratch_bytes(*bad)
