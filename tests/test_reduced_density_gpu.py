"""The reduced-density kernels (csrc/reduced.hip) and `inference.reduced` on the GPU.

1. `qhbm_reduced_density` against `tests/reduced_density_ref.reduced` on the same complex64 states, scratch and output
   pre-filled with NaN.  Bound, per part (re or im) of an entry, derived and not tuned.  With T = M 2^(n-k) environment
   values, a part is a sum of 2 T products.  A product is float x float in float64: 48 bits, exact.  The column operand is
   multiplied by w_m first: one rounding, relative 2^-53, on the way of each product (none when the weights are NULL).
   The additions form a tree -- a thread's chain of fused multiply-adds over its environment values (the first one adds
   to 0.0 and is exact), the shuffle tree over the groups of a wave (at most 6 levels), the four waves in order, then the
   slices in order (at most 511 more) -- and an addition rounds only when both operands are non-zero, so on no path from
   a product to the result are there more roundings than the tree has additions of two non-zero operands: 2 T - 1,
   whatever the tree's shape (idle groups, waves and short slices hold exact zeros).  Each is relative 2^-53 to a partial
   sum no larger than S[a, a'] = sum_m |w_m| sum_b |phi_m(a, b)| |phi_m(a', b)| to first order.  With the weight's
   rounding: |d| <= 2 T 2^-53 S, i.e. c = 0 extra roundings for the order implemented; the issue's c = 8 is kept as the
   allowance, and kernel and reference together get twice (2 T + 8) 2^-53 S[a, a'].
2. Exact cases, compared with ==.
3. Two gather patterns against each other at 20 qubits, and the top-k mask against the Gram kernel.
4. Refusals, each with its message, nothing launched.
5. The mirror (`inference.reduced`) at n = 4 and 6 against the dense partial trace built on the host in complex128.
6. The pipeline: ground state of a TFIM ring on 8 qubits -> `.reduced` -> `qmhl`.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir, models
from qhbmlib_amd.inference import reduced as reduced_lib
from qhbmlib_amd.models import energy_utils
from tests import reduced_density_ref as R
from tests.test_host_api import hea_circuit

pytestmark = pytest.mark.gpu

# (n, kept qubits, M): small shapes for every tile edge, mask kind and environment size of the plan (csrc/rdm_index.h)
SHAPES = [
    (1, (0,), 1),
    (2, (0,), 3),
    (2, (1,), 3),
    (3, (0, 2), 1),
    (5, (1, 3), 3),
    (6, tuple(range(6)), 2),                  # empty environment
    (10, tuple(range(10)), 3),                # k = n = 10
    (11, tuple(range(10)), 1),                # an environment of one bit, the lowest
    (12, (10, 11), 1),                        # kept bits inside a 16-byte word and a 128-byte line
    (12, tuple(range(10)), 2),
    (13, (2, 3, 5, 7, 11, 12), 2),
    (14, (0, 5, 13), 3),                      # several slices
    (14, (0, 2, 4, 6, 8, 10, 12, 13), 1),     # the LDS-staged path, several tiles (64 divides 2^8: no ragged tile exists)
    (16, (0, 15), 1),
    # The shapes above give every workgroup exactly one block (slices = blocks).  These two give slices of several
    # blocks that cross state boundaries, so the prefetch of the next block, the masked increment, the carry of m and the
    # reload of w_m are what the result depends on:
    (10, (0, 9), 1024),                       # 1024 blocks (one a state) in 512 slices: every slice spans two states
    (21, (0, 9, 20), 3),                      # 3 x 1024 blocks in 512 slices of 6: the increment inside a state, and 2 slices
                                              # that cross into the next state
]
WEIGHTS = ["none", "weighted"]


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _raw_reduced(states, mask, weights=None):
  """qhbm_reduced_density through the C ABI on a NaN-filled scratch and output: complex128 numpy [2^k, 2^k]."""
  lib = E.load_library()
  num, dim = states.shape
  n = dim.bit_length() - 1
  edge = 1 << bin(mask).count("1")
  scratch = torch.full((E.reduced_density_scratch_bytes(num, n, mask) // 8,), float("nan"), dtype=torch.float64, device="cuda")
  out = torch.full((edge, edge, 2), float("nan"), dtype=torch.float64, device="cuda")
  rc = lib.qhbm_reduced_density(states.data_ptr(), num, n, mask, None if weights is None else weights.data_ptr(),
                                scratch.data_ptr(), out.data_ptr(), torch.cuda.current_stream().cuda_stream)
  assert rc == 0, lib.qhbm_last_error(None).decode()
  # (a view, not re + 1j * im: that sum turns an imaginary part of -0.0 into +0.0)
  return np.ascontiguousarray(out.cpu().numpy()).view(np.complex128).reshape(edge, edge)


@functools.lru_cache(maxsize=None)
def _case(n, num):
  """(complex64 states, float64 weights uniform in [0.1, 1] with one exactly 0) as numpy, one draw per shape."""
  rng = np.random.default_rng(1000 * n + num)
  dim = 1 << n
  states = ((rng.normal(size=(num, dim)) + 1j * rng.normal(size=(num, dim))) / np.sqrt(2 * dim)).astype(np.complex64)
  weights = rng.uniform(0.1, 1.0, num)
  weights[int(rng.integers(num))] = 0.0
  return states, weights


def _entry_bound(n, k, num, magnitude_sums):
  return 2.0 * (2.0 * num * 2.0**(n - k) + 8.0) * 2.0**-53 * magnitude_sums


def _hold(got, want, bound, label):
  err_re, err_im = np.abs(got.real - want.real), np.abs(got.imag - want.imag)
  live = bound > 0
  worst = max(float(np.max(err_re[live] / bound[live])), float(np.max(err_im[live] / bound[live]))) if live.any() else 0.0
  print(f"{label}: worst {worst:.3g} of the bound")
  assert np.all(err_re <= bound) and np.all(err_im <= bound), label


@pytest.mark.parametrize("weighted", WEIGHTS)
@pytest.mark.parametrize("n,kept,num", SHAPES)
def test_kernel_matches_the_float64_restatement(n, kept, num, weighted):
  states, weights = _case(n, num)
  w = weights if weighted == "weighted" else None
  mask = R.keep_mask(kept)
  d_states = torch.from_numpy(states).cuda()
  d_weights = None if w is None else torch.from_numpy(w).cuda()
  got = _raw_reduced(d_states, mask, d_weights)
  want, sums = R.reduced(states, kept, w)
  assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag))
  _hold(got, want, _entry_bound(n, len(kept), num, sums), f"n={n} kept={kept} M={num} {weighted}")
  # Hermitian bit for bit, the diagonal exactly real, and the same bits from a second call
  assert np.array_equal(_bits(got.real), _bits(got.real.T))
  assert np.all(np.diagonal(got).imag == 0.0)
  off = ~np.eye(got.shape[0], dtype=bool)
  assert np.array_equal(_bits(got.imag[off]), _bits((-got.imag.T)[off]))
  again = _raw_reduced(d_states, mask, d_weights)
  assert np.array_equal(_bits(got.real), _bits(again.real)) and np.array_equal(_bits(got.imag), _bits(again.imag))
  # the binding: same kernel, its own scratch
  bound_call = E.reduced_density(d_states, mask, d_weights).cpu().numpy()
  assert bound_call.dtype == np.complex128
  assert np.array_equal(_bits(bound_call.real), _bits(got.real)) and np.array_equal(_bits(bound_call.imag), _bits(got.imag))


# ---- exact cases ------------------------------------------------------------------------------------------------------
def test_plus_state_reduces_to_exact_eighths():
  """|+>^14 has amplitudes 2^-7: every product is 2^-14 and every partial sum of the 2^11 of an entry is representable."""
  states = torch.full((1, 1 << 14), 2.0**-7, dtype=torch.complex64, device="cuda")
  got = _raw_reduced(states, R.keep_mask((0, 5, 13)))
  assert got.shape == (8, 8)
  assert np.all(got.real == 2.0**-3) and np.all(got.imag == 0.0)


@pytest.mark.parametrize("kept", [(0, 11), (3, 4, 7, 10)])
def test_ghz_reduces_to_its_two_exact_corners(kept):
  """GHZ on 12 qubits with amplitude float32(sqrt(1/2)): entries [0, 0] and [last, last] are its square as a double,
  exactly, and every other entry is exactly 0.  (With a non-empty environment that includes [0, last] and [last, 0]:
  |0..0> and |1..1> differ on the traced qubits, as the closed form diag(1/2, 0, ..., 0, 1/2) of the CPU tests says;
  the two coherences survive only at k = n, the next test.)"""
  n = 12
  amp = np.float32(np.sqrt(0.5))
  host = np.zeros((1, 1 << n), dtype=np.complex64)
  host[0, 0] = host[0, -1] = amp
  got = _raw_reduced(torch.from_numpy(host).cuda(), R.keep_mask(kept))
  want = np.zeros_like(got)
  last = got.shape[0] - 1
  want[0, 0] = want[last, last] = float(amp) * float(amp)   # (exact in float64)
  assert np.array_equal(got.real, want.real) and np.all(got.imag == 0.0)


def test_ghz_on_every_qubit_keeps_its_coherences():
  """k = n: entries [0, 0], [0, last], [last, 0], [last, last] are float32(sqrt(1/2))^2 exactly, all others 0."""
  n = 10
  amp = np.float32(np.sqrt(0.5))
  host = np.zeros((1, 1 << n), dtype=np.complex64)
  host[0, 0] = host[0, -1] = amp
  got = _raw_reduced(torch.from_numpy(host).cuda(), R.keep_mask(range(n)))
  want = np.zeros_like(got)
  last = (1 << n) - 1
  want[0, 0] = want[0, last] = want[last, 0] = want[last, last] = float(amp) * float(amp)
  assert np.array_equal(got.real, want.real) and np.all(got.imag == 0.0)


def test_random_sign_states_have_exact_marginals():
  """Every part of `random_states` at 21 qubits is +-2^-11, so |phi(x)|^2 = 2^-21 exactly and each of the 2 * 2^18 products
  of a diagonal entry with k = 3 is 2^-22: every partial sum is a multiple of 2^-22 below 1, representable, and the
  diagonal is 2^-3 with no rounding in any order (the argument of test_state_metrics_gpu's exact norm)."""
  states = E.random_states(2, 21, 5)
  for row in range(2):
    got = _raw_reduced(states[row:row + 1], R.keep_mask((0, 9, 20)))
    assert np.all(np.diagonal(got).real == 2.0**-3) and np.all(np.diagonal(got).imag == 0.0)
  both = _raw_reduced(states, R.keep_mask((0, 9, 20)))
  assert np.all(np.diagonal(both).real == 2.0**-2)


# ---- two gather patterns against each other ---------------------------------------------------------------------------
def test_both_halves_of_a_pure_state_have_the_same_purity_and_the_top_half_is_the_gram_matrix():
  """One random-sign state of 20 qubits, A = qubits 0-9 (the environment is the 10 low index bits: a word holds two
  environment values), B = qubits 10-19 (the kept bits are the low ones: a word holds two rows).  tr rho_A^2 = tr rho_B^2
  for any vector (both are the sum of the fourth powers of its Schmidt coefficients).

  Bound.  tr rho^2 = ||rho||_F^2, so |d tr rho^2| <= 2 ||rho||_F ||d rho||_F to first order.  The kernel's entrywise bound
  is eps S[a, a'] per part with eps = (2 * 2^10 + 8) 2^-53 (test 1: T = 2^10 environment values, no weights), and
  sum S^2 <= (tr rho)^2 because S[a, a'] <= sqrt(rho[a, a] rho[a', a']) by Cauchy-Schwarz; so ||d rho||_F <= eps tr rho per
  part.  Two matrices: |tr rho_A^2 - tr rho_B^2| <= 4 ||rho||_F eps (tr rho)^2 as the issue states it (tr rho = 1 - 6e-8
  here; counting real and imaginary parts separately would allow sqrt(2) more, which is not taken).  With ||rho||_F <= 1
  that is at most 9.2e-13; the assertion uses the measured ||rho||_F, about 0.044 for a random state.

  Cross-check against the Gram kernel: for the top-k mask the state viewed as [2^10, 2^10] gives rho_A = conj(G), within
  the sum of the two kernels' own bounds, (2 * 2^10 + 8) 2^-53 S (here) + 2 (2^10 + 4) 2^-53 S (gram.hip's header)."""
  n, half = 20, 10
  state = E.random_states(1, n, 9)
  rho_a = E.reduced_density(state, R.keep_mask(range(half))).cpu().numpy()
  rho_b = E.reduced_density(state, R.keep_mask(range(half, n))).cpu().numpy()
  purity_a, purity_b = float(np.sum(np.abs(rho_a)**2)), float(np.sum(np.abs(rho_b)**2))
  trace = float(np.trace(rho_a).real)
  eps = (2.0 * 2.0**half + 8.0) * 2.0**-53
  bound = 4.0 * np.sqrt(max(purity_a, purity_b)) * eps * trace**2
  print(f"tr rho_A^2 {purity_a!r} tr rho_B^2 {purity_b!r} difference {purity_a - purity_b:.3g} bound {bound:.3g} "
        f"({abs(purity_a - purity_b) / bound:.3g} of it)")
  np.testing.assert_allclose(np.trace(rho_b).real, trace, rtol=0, atol=2.0 * eps * trace)
  assert abs(purity_a - purity_b) <= bound
  gram = E.weighted_gram(state.reshape(1 << half, 1 << half)).cpu().numpy()
  magnitudes = state.abs().to(torch.float64).reshape(1 << half, 1 << half)
  sums = (magnitudes @ magnitudes.transpose(0, 1)).cpu().numpy()
  both = (eps + 2.0 * (2.0**half + 4.0) * 2.0**-53) * sums
  _hold(rho_a, gram.conj(), both, "rho_A against conj(G)")


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refused_arguments_return_a_message_and_launch_nothing():
  lib = E.load_library()
  n, num, mask = 12, 2, 0b11
  states = torch.ones((num, (1 << n) + 2), dtype=torch.complex64, device="cuda")
  weights = torch.ones(num + 1, dtype=torch.float64, device="cuda")
  scratch = torch.zeros(E.reduced_density_scratch_bytes(num, n, mask) // 8 + 1, dtype=torch.float64, device="cuda")
  out = torch.full((4 * 4 * 2 + 1,), -7.0, dtype=torch.float64, device="cuda")
  stream = torch.cuda.current_stream().cuda_stream
  good = dict(s=states.data_ptr(), m=num, n=n, k=mask, w=weights.data_ptr(), p=scratch.data_ptr(), r=out.data_ptr())
  refused = [
      (dict(k=0), "between 1 and"),                       # k = 0
      (dict(k=(1 << 11) - 1), "between 1 and"),           # k = 11
      (dict(n=3, k=0b1111), "at or above n_qubits"),      # more kept qubits than qubits: a mask bit >= n
      (dict(k=1 << n), "at or above n_qubits"),           # a mask bit >= n
      (dict(m=0), "M must be"),
      (dict(m=65537), "M must be"),
      (dict(n=0, k=0), "n_qubits must be"),
      (dict(n=32), "n_qubits must be"),
      (dict(s=states.data_ptr() + 8), "16-byte aligned"),  # a misaligned states pointer
      (dict(s=None), "NULL"),
      (dict(p=None), "NULL"),
      (dict(r=None), "NULL"),                              # NULL output
      (dict(w=weights.data_ptr() + 4), "8-byte aligned"),
      (dict(r=out.data_ptr() + 4), "8-byte aligned"),
  ]
  for change, message in refused:
    a = dict(good, **change)
    rc = lib.qhbm_reduced_density(a["s"], a["m"], a["n"], a["k"], a["w"], a["p"], a["r"], stream)
    assert rc != 0, change
    assert message in lib.qhbm_last_error(None).decode(), (change, lib.qhbm_last_error(None).decode())
  size = ctypes.c_size_t()
  for m, nq, k in [(0, 6, 1), (65537, 6, 1), (4, 0, 1), (4, 32, 1), (4, 6, 0), (4, 6, 1 << 6), (4, 12, (1 << 11) - 1)]:
    assert lib.qhbm_reduced_density_scratch_bytes(m, nq, k, ctypes.byref(size)) != 0
    assert lib.qhbm_last_error(None).decode()
  assert lib.qhbm_reduced_density_scratch_bytes(4, 6, 1, None) != 0
  torch.cuda.synchronize()
  assert torch.all(out == -7.0) and torch.all(scratch == 0.0)
  with pytest.raises(E.EngineError):
    E.reduced_density(states[:, :1 << n].cpu(), mask)
  with pytest.raises(ValueError):
    E.reduced_density(states[:, :1 << n], mask, weights)   # three weights for two states
  with pytest.raises(E.EngineError, match="between 1 and"):
    E.reduced_density(states[:, :1 << n], 0)


# ---- the mirror -------------------------------------------------------------------------------------------------------
def _set(param, values):
  with torch.no_grad():
    param.copy_(torch.as_tensor(np.asarray(values), dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _weighted_data(n):
  """(StateVectorData of five complex64 states on a line of n qubits, states, weights): neither orthogonal nor normalised."""
  rng = np.random.default_rng(170 + n)
  states = rng.normal(size=(5, 1 << n)) + 1j * rng.normal(size=(5, 1 << n))
  states *= rng.uniform(0.5, 1.0, (5, 1)) / np.linalg.norm(states, axis=1, keepdims=True)
  states = states.astype(np.complex64)
  weights = rng.uniform(0.05, 0.2, 5)
  qubits = ir.GridQubit.rect(1, n)
  return data.StateVectorData(torch.from_numpy(states), torch.from_numpy(weights), qubits), states, weights


@functools.lru_cache(maxsize=None)
def _qhbm(n, layers, num_samples, tag):
  """A KOBE-2 energy under an HEA on a line of n qubits, with a fixed sampler seed: every call draws the same samples."""
  rng = np.random.default_rng(50 + n)
  energy = models.KOBE(list(range(n)), 2)
  energy.build([None, n])
  _set(energy.trainable_variables[0], rng.uniform(-1, 1, tuple(energy.trainable_variables[0].shape)))
  circ = models.DirectQuantumCircuit(hea_circuit(ir.GridQubit.rect(1, n), layers, tag))
  _set(circ.trainable_variables[0], rng.uniform(-1, 1, len(circ.symbol_names)))
  return inference.QHBM(inference.AnalyticEnergyInference(energy, num_samples, initial_seed=3),
                        inference.AnalyticQuantumInference(circ))


@pytest.mark.parametrize("n", [4, 6])
def test_mirror_matches_the_dense_partial_trace(n):
  source, states, weights = _weighted_data(n)
  sigma = R.dense_sigma(states, weights)
  qubits = source.qubits
  for kept in [(0,), (1, n - 1), (0, 2, 3), tuple(range(n))]:
    got = inference.reduced_density_matrix(source, list(kept))
    assert got.is_cuda and got.dtype == torch.complex128
    _, sums = R.reduced(states, kept, weights)
    _hold(got.cpu().numpy(), R.dense_partial_trace(sigma, kept), _entry_bound(n, len(kept), 5, sums), f"n={n} kept={kept}")
    # qubit objects in descending order = ascending integer positions, bit for bit; so is a (states, weights) pair
    by_object = inference.reduced_density_matrix(source, [qubits[q] for q in reversed(kept)])
    assert torch.equal(torch.view_as_real(by_object), torch.view_as_real(got))
    pair = inference.reduced_density_matrix((torch.from_numpy(states), torch.from_numpy(weights)), list(reversed(kept)))
    assert torch.equal(torch.view_as_real(pair), torch.view_as_real(got))
    by_numpy = inference.reduced_density_matrix(source, np.array(kept, dtype=np.int64)[::-1])   # numpy integer positions
    assert torch.equal(torch.view_as_real(by_numpy), torch.view_as_real(got))
  # entropies: data-only quantities, 1e-6 absolute
  for kept in [(0,), (1, n - 1), (0, 2, 3)]:
    want = R.entropy(R.dense_partial_trace(sigma, kept))
    got = inference.subsystem_entropy(source, list(kept))
    print(f"n={n} S{kept} {got!r} ({got - want:+.2g})")
    assert isinstance(got, float)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
  a, b = (0,), (2, 3)
  want = (R.entropy(R.dense_partial_trace(sigma, a)) + R.entropy(R.dense_partial_trace(sigma, b)) -
          R.entropy(R.dense_partial_trace(sigma, a + b)))
  got = inference.mutual_information(source, [qubits[0]], [qubits[3], qubits[2]])
  print(f"n={n} I(A:B) {got!r} ({got - want:+.2g})")
  np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)
  rho_a = inference.reduced_density_matrix(source, [0, 1])
  assert inference.trace_distance(rho_a, rho_a) == 0.0
  other = R.dense_partial_trace(sigma, (2, 3))
  delta = rho_a.cpu().numpy() - other
  np.testing.assert_allclose(inference.trace_distance(rho_a, torch.from_numpy(other)),
                             0.5 * np.abs(np.linalg.eigvalsh(0.5 * (delta + delta.conj().T))).sum(), rtol=0, atol=1e-12)


def test_mirror_refuses_what_does_not_fit():
  source, _, _ = _weighted_data(4)
  with pytest.raises(ValueError, match="twice"):
    inference.reduced_density_matrix(source, [1, 1])
  with pytest.raises(ValueError, match="not in the data"):
    inference.reduced_density_matrix(source, [ir.GridQubit(1, 0)])
  with pytest.raises(ValueError, match="positions"):
    inference.reduced_density_matrix(source, [4])
  with pytest.raises(ValueError, match="overlap"):
    inference.mutual_information(source, [0, 1], [1, 2])
  with pytest.raises(ValueError, match="no qubits"):
    inference.reduced_density_matrix(source, [])
  with pytest.raises(TypeError):
    inference.reduced_density_matrix(torch.ones(2, 4), [0])


def test_a_thermal_ensemble_is_its_data():
  qubits = ir.GridQubit.rect(1, 4)
  zz = ir.PZ(qubits[0]) * ir.PZ(qubits[1])
  for a, b in zip(qubits[1:], qubits[2:] + qubits[:1]):
    zz = zz + ir.PZ(a) * ir.PZ(b)
  xs = ir.PX(qubits[0])
  for q in qubits[1:]:
    xs = xs + ir.PX(q)
  ensemble = inference.thermal_ensemble([zz, xs], 0.7, num_vectors=4, seed=2, weights=[-1.0, -1.0])
  got = inference.reduced_density_matrix(ensemble, [qubits[2], qubits[0]])
  want = inference.reduced_density_matrix(ensemble.data(), [0, 2])
  assert torch.equal(torch.view_as_real(got), torch.view_as_real(want))
  np.testing.assert_allclose(float(got.diagonal().real.sum()), 1.0, rtol=0, atol=1e-6)
  assert inference.subsystem_entropy(ensemble, [0, 2]) == inference.subsystem_entropy(ensemble.data(), [0, 2])


@pytest.mark.parametrize("n", [4, 6])
def test_sampled_ensemble_in_three_chunks_and_in_one(n):
  num_samples = 64
  model = _qhbm(n, 2, num_samples, f"rdm{n}")
  kept = (0, n - 2)
  samples = model.e_inference.sample(num_samples)
  from qhbmlib_amd import utils  # pylint: disable=import-outside-toplevel
  bitstrings, _, counts = utils.unique_bitstrings_with_counts(samples)
  unique = int(bitstrings.shape[0])
  assert unique >= 3
  per_chunk = -(-unique // 3)
  assert -(-unique // per_chunk) == 3, unique
  one = inference.sampled_reduced_density_matrix(model, list(kept), num_samples)
  three = inference.sampled_reduced_density_matrix(model, list(kept), num_samples, max_state_bytes=per_chunk * (8 << n))
  # the restatement on the same bitstrings and counts, from the engine's own complex64 states
  eng = reduced_lib._model_engine(model, torch.device("cuda", torch.cuda.current_device()))  # pylint: disable=protected-access
  circ = model.q_inference.circuit
  from qhbmlib_amd.inference import qnn  # pylint: disable=import-outside-toplevel
  states = eng.statevector(qnn._engine_bits(circ, bitstrings), circ.symbol_values.detach().to(torch.float32))  # pylint: disable=protected-access
  weights = counts.cpu().numpy().astype(np.float64) / num_samples
  want, sums = R.reduced(states.cpu().numpy(), kept, weights)
  # (the chunk results are added in float64: two more roundings, inside the allowance of 8)
  bound = _entry_bound(n, len(kept), unique, sums)
  _hold(one.cpu().numpy(), want, bound, f"n={n} one chunk")
  _hold(three.cpu().numpy(), want, bound, f"n={n} three chunks")
  _hold(three.cpu().numpy(), one.cpu().numpy(), bound, f"n={n} three chunks against one")
  np.testing.assert_allclose(float(one.diagonal().real.sum()), 1.0, rtol=0, atol=1e-5)
  by_object = inference.sampled_reduced_density_matrix(model, [circ.qubits[n - 2], circ.qubits[0]], num_samples)
  assert torch.equal(torch.view_as_real(by_object), torch.view_as_real(one))


def test_more_states_than_one_call_takes_are_split_whatever_max_state_bytes_says():
  """70000 rows of bitstrings (the 16 of 4 qubits, repeated) with a `max_state_bytes` that would admit them all: the engine
  takes 65536 states a call, so the mirror makes two calls.  Against the restatement on the engine's own states."""
  n, rows, kept = 4, 70000, (1, 2)
  model = _qhbm(n, 2, 64, "rdm4")
  circ = model.q_inference.circuit
  basis = torch.tensor([[(x >> (n - 1 - q)) & 1 for q in range(n)] for x in range(1 << n)], dtype=torch.int8)
  order = torch.arange(rows) % (1 << n)
  got = reduced_lib.sampled_ensemble_reduced(model, basis[order], torch.ones(rows), rows, list(kept), max_state_bytes=2**40)
  eng = reduced_lib._model_engine(model, torch.device("cuda", torch.cuda.current_device()))  # pylint: disable=protected-access
  from qhbmlib_amd.inference import qnn  # pylint: disable=import-outside-toplevel
  states = eng.statevector(qnn._engine_bits(circ, basis), circ.symbol_values.detach().to(torch.float32)).cpu().numpy()  # pylint: disable=protected-access
  counts = np.bincount(order.numpy(), minlength=1 << n).astype(np.float64)
  want, sums = R.reduced(states, kept, counts / rows)
  # (the restatement adds 16 weighted states, the kernel 70000 copies at weight 1 / 70000: the bound is the kernel's shape's)
  _hold(got.cpu().numpy(), want, _entry_bound(n, len(kept), rows, sums), "70000 states in two calls")
  np.testing.assert_allclose(float(got.diagonal().real.sum()), 1.0, rtol=0, atol=1e-5)


# ---- the pipeline -----------------------------------------------------------------------------------------------------
def test_subsystem_qmhl_from_a_ground_state():
  """Ground state of the TFIM ring on 8 qubits -> rho_A of its first three qubits on the GPU -> quantum data -> qmhl of a
  3-qubit KOBE-2 / one-layer HEA QHBM: loss and gradients finite, and equal to the same call on the eigen-ensemble of the
  dense partial trace of the same state within 1e-5 x the largest |energy| (the project's expectation tolerance)."""
  n, k = 8, 3
  qubits = ir.GridQubit.rect(1, n)
  zz = ir.PZ(qubits[0]) * ir.PZ(qubits[1])
  for a, b in zip(qubits[1:], qubits[2:] + qubits[:1]):
    zz = zz + ir.PZ(a) * ir.PZ(b)
  xs = ir.PX(qubits[0])
  for q in qubits[1:]:
    xs = xs + ir.PX(q)
  source = data.StateVectorData.ground_state([zz, xs], weights=[-1.0, -1.0], seed=3)
  part = source.reduced(qubits[:k])
  assert part.num_qubits == k and list(part.qubits) == list(qubits[:k])
  np.testing.assert_allclose(float(part.weights.sum()), 1.0, rtol=0, atol=1e-5)
  state = source._device_states().cpu().numpy()  # pylint: disable=protected-access
  dense = R.dense_partial_trace(R.dense_sigma(state), range(k))
  reference = data.StateVectorData.from_density_matrix(torch.from_numpy(dense), qubits=qubits[:k])

  model = _qhbm(k, 1, 16, "rdmpipe")
  energy = model.e_inference.energy
  variables = list(model.trainable_variables)
  e_max = float(energy_utils.energy_table(energy, k, 24, method="terms").detach().abs().max())
  bar = 1e-5 * e_max

  def loss_and_grads(source_a):
    loss = inference.qmhl(source_a, model)
    grads = torch.autograd.grad(loss, variables)
    return float(loss.detach()), [g.detach().cpu().double().numpy() for g in grads]
  got_loss, got_grads = loss_and_grads(part)
  want_loss, want_grads = loss_and_grads(reference)
  print(f"qmhl {got_loss!r} against {want_loss!r} ({got_loss - want_loss:+.2g}), bar {bar:.3g}; subsystem entropy "
        f"{inference.subsystem_entropy(source, qubits[:k])!r}")
  assert np.isfinite(got_loss) and all(np.all(np.isfinite(g)) for g in got_grads)
  assert len(got_grads) >= 2
  np.testing.assert_allclose(got_loss, want_loss, rtol=0, atol=bar)
  for g, w in zip(got_grads, want_grads):
    print(f"  gradient block {g.shape}: max difference {np.max(np.abs(g - w)):.3g}")
    np.testing.assert_allclose(g, w, rtol=0, atol=bar)
