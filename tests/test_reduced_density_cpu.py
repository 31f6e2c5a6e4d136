"""The numpy restatement of the reduced density matrix (tests/reduced_density_ref.py, what the GPU tests compare the
kernel with) held to closed forms, without a GPU."""
import itertools

import numpy as np
import pytest

from tests import reduced_density_ref as R


def _random_states(num, n, seed):
  rng = np.random.default_rng(seed)
  states = rng.normal(size=(num, 1 << n)) + 1j * rng.normal(size=(num, 1 << n))
  return states / np.linalg.norm(states, axis=1, keepdims=True)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5])
def test_every_mask_equals_the_dense_partial_trace(n):
  states = _random_states(3, n, n)
  weights = np.array([0.5, 0.3, 0.2])
  sigma = R.dense_sigma(states, weights)
  for k in range(1, n + 1):
    for kept in itertools.combinations(range(n), k):
      rho, bound = R.reduced(states, kept, weights)
      np.testing.assert_allclose(rho, R.dense_partial_trace(sigma, kept), rtol=0, atol=1e-14)
      assert np.all(np.abs(rho) <= bound + 1e-15)
      np.testing.assert_allclose(np.trace(rho).real, 1.0, rtol=0, atol=1e-14)
      # the caller's order does not matter: ascending is the layout
      np.testing.assert_array_equal(R.reduced(states, tuple(reversed(kept)), weights)[0], rho)


@pytest.mark.parametrize("kept", [(0,), (2, 3), (0, 4), (1, 2, 4)])
def test_ghz_reduces_to_half_half(kept):
  n = 5
  state = np.zeros((1, 1 << n), dtype=np.complex128)
  state[0, 0] = state[0, -1] = np.sqrt(0.5)
  rho, _ = R.reduced(state, kept)
  want = np.zeros_like(rho)
  want[0, 0] = want[-1, -1] = 0.5
  np.testing.assert_allclose(rho, want, rtol=0, atol=1e-15)


def test_product_state_reduces_to_rank_one():
  rng = np.random.default_rng(7)
  factors = [rng.normal(size=2) + 1j * rng.normal(size=2) for _ in range(5)]
  factors = [f / np.linalg.norm(f) for f in factors]
  state = factors[0]
  for f in factors[1:]:
    state = np.kron(state, f)   # qubit 0 is the most significant bit
  for kept in [(0,), (3,), (1, 3), (0, 2, 4)]:
    rho, _ = R.reduced(state[None, :], kept)
    local = factors[kept[0]]
    for q in kept[1:]:
      local = np.kron(local, factors[q])
    np.testing.assert_allclose(rho, np.outer(local, local.conj()), rtol=0, atol=1e-14)
    assert np.linalg.matrix_rank(rho, tol=1e-12) == 1


def test_bell_pair_entropy_and_mutual_information():
  state = np.zeros((1, 4), dtype=np.complex128)
  state[0, 0] = state[0, 3] = np.sqrt(0.5)
  s_a = R.entropy(R.reduced(state, (0,))[0])
  s_b = R.entropy(R.reduced(state, (1,))[0])
  s_ab = R.entropy(R.reduced(state, (0, 1))[0])
  np.testing.assert_allclose(s_a, np.log(2.0), rtol=0, atol=1e-14)
  np.testing.assert_allclose(s_a + s_b - s_ab, 2.0 * np.log(2.0), rtol=0, atol=1e-12)


@pytest.mark.parametrize("kept", [(0,), (1, 4), (0, 2, 5), (3, 4, 5), (0, 1, 2, 3, 4)])
def test_a_pure_state_has_the_same_purity_on_both_sides(kept):
  n = 6
  state = _random_states(1, n, 11)
  rest = tuple(q for q in range(n) if q not in kept)
  rho_a, rho_b = R.reduced(state, kept)[0], R.reduced(state, rest)[0]
  np.testing.assert_allclose(np.trace(rho_a @ rho_a).real, np.trace(rho_b @ rho_b).real, rtol=0, atol=1e-14)


@pytest.mark.parametrize("n,k", [(3, 1), (5, 2), (6, 6), (7, 3)])
def test_the_top_k_mask_is_the_conjugate_gram_matrix_of_the_row_view(n, k):
  state = _random_states(1, n, 100 + n)
  rho, _ = R.reduced(state, range(k))
  rows = state.reshape(1 << k, 1 << (n - k))
  gram = rows.conj() @ rows.T   # G[i, j] = sum_x conj(s_i(x)) s_j(x), what qhbm_weighted_gram sums
  np.testing.assert_allclose(rho, gram.conj(), rtol=0, atol=1e-14)


def test_keep_mask_is_in_qubit_space():
  assert R.keep_mask((0,)) == 1 and R.keep_mask((3, 1)) == 0b1010 and R.keep_mask((2, 2)) == 0b100
