"""qhbm_parity_energy / qhbm_parity_energy_vjp against a numpy uint64-popcount restatement in fp64, across the
kernels' edges: LDS term chunks of 1024 (forward), term groups and row sweeps of the VJP, masks that use bit 63.

With dyadic inputs (theta = j / 64, |j| <= 64; integer weights in [-8, 8]) every partial sum is exact in fp32, so the
outputs must EQUAL the reference: an error of logic cannot hide in a tolerance.  Random inputs check a stated rounding
bound and bit-identical repeats (the VJP reduces in a fixed order, no atomics)."""
import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd import inference, models
from qhbmlib_amd.inference import information

pytestmark = pytest.mark.gpu


def _reference(bits, masks, thetas, weights):
  """fp64 (energies [rows], weighted parity sums [terms]) with parity_k(x_i) = (-1)^popcount(x_i & m_k),
  x_i = sum_q bits[i, q] 2^q (column q = bit q), in row chunks."""
  n = bits.shape[1]
  energy, sums = np.zeros(bits.shape[0]), np.zeros(masks.size)
  for r0 in range(0, bits.shape[0], 1 << 16):
    x = (bits[r0:r0 + (1 << 16)].astype(np.uint64) << np.arange(n, dtype=np.uint64)).sum(1, dtype=np.uint64)
    s = 1.0 - 2.0 * (np.bitwise_count(x[:, None] & masks[None, :]) & 1)
    energy[r0:r0 + x.size] = s @ np.asarray(thetas, np.float64)
    sums += np.asarray(weights[r0:r0 + x.size], np.float64) @ s
  return energy, sums


def _inputs(rng, n, rows, terms):
  bits = rng.integers(0, 2, size=(rows, n)).astype(np.int8)
  # random 64-bit masks: bit 63 in about half of them; bits at or above n never match (x has n bits)
  masks = rng.integers(0, 2**63, size=terms, dtype=np.uint64) | (rng.integers(0, 2, size=terms, dtype=np.uint64) << np.uint64(63))
  if terms:
    masks[0] = np.uint64(1 << (n - 1))      # the highest column alone (bit 63 at n = 64)
  return bits, masks


def _run(bits, masks, thetas, weights):
  d_bits = torch.from_numpy(bits).cuda()
  d_masks = torch.from_numpy(masks.view(np.int64)).cuda()
  th = torch.from_numpy(thetas.astype(np.float32)).cuda().requires_grad_(True)
  energy = E.parity_energy(th, d_bits, d_masks)
  w = torch.from_numpy(weights.astype(np.float32)).cuda()
  if masks.size:
    (grad,) = torch.autograd.grad(energy, th, w)
  else:
    grad = torch.zeros(0)
  sums = E.parity_sums(d_bits, d_masks, w)
  return energy.detach().cpu().numpy(), grad.cpu().numpy(), sums.cpu().numpy()


def _check_exact(n, rows, terms, seed, zero=False):
  rng = np.random.default_rng(seed)
  bits, masks = _inputs(rng, n, rows, terms)
  thetas = rng.integers(-64, 65, size=terms) / 64.0
  weights = rng.integers(-8, 9, size=rows).astype(np.float64)
  if zero:
    thetas[:] = 0.0
    weights[:] = 0.0
  want_e, want_g = _reference(bits, masks, thetas, weights)
  got_e, got_g, got_s = _run(bits, masks, thetas, weights)
  assert got_e.shape == (rows,) and got_g.shape == (terms,)
  np.testing.assert_array_equal(got_e, want_e.astype(np.float32))
  np.testing.assert_array_equal(got_g, want_g.astype(np.float32))
  np.testing.assert_array_equal(got_s, want_g.astype(np.float32))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64])
def test_exact_every_width(n):
  _check_exact(n, 2049, 1025, seed=n)


@pytest.mark.parametrize("terms", [0, 1, 1023, 1024, 1025, 2500])
def test_exact_every_term_count(terms):
  _check_exact(64, 2049, terms, seed=terms)


@pytest.mark.parametrize("rows", [0, 1, 255, 256, 257, 2047, 2048, 2049, 3 * 2048 + 1])
def test_exact_every_row_count(rows):
  _check_exact(33, rows, 1025, seed=rows)


def test_exact_a_million_rows():
  _check_exact(20, 2**20, 37, seed=7)


def test_zero_weights_give_exact_zeros():
  _check_exact(64, 3 * 2048 + 1, 1025, seed=1, zero=True)


def test_random_inputs_within_the_rounding_bound_and_bit_identical_repeats():
  """Forward: an fp32 sum of K terms in order, |e - e_ref| <= K 2^-24 sum_k |theta_k|.
  VJP: an fp64 sum of N rows rounded once to fp32, |g - g_ref| <= 2^-24 |g_ref| + N 2^-52 sum_i |w_i| -- an fp32
  accumulation (the earlier kernel) misses it by an order of magnitude at N = 2^20."""
  rng = np.random.default_rng(11)
  n, rows, terms = 20, 2**20, 210
  bits, masks = _inputs(rng, n, rows, terms)
  thetas = rng.normal(size=terms).astype(np.float32)
  weights = rng.normal(size=rows).astype(np.float32)
  want_e, want_g = _reference(bits, masks, thetas, weights)
  runs = [_run(bits, masks, thetas, weights) for _ in range(3)]
  got_e, got_g, got_s = runs[0]
  assert np.all(np.abs(got_e - want_e) <= terms * 2.0**-24 * np.abs(thetas).sum())
  bound = 2.0**-24 * np.abs(want_g) + rows * 2.0**-52 * np.abs(weights).sum()
  assert np.all(np.abs(got_g - want_g) <= bound), np.abs(got_g - want_g).max()
  np.testing.assert_array_equal(got_s, got_g)
  for e, g, sm in runs[1:]:
    assert e.tobytes() == got_e.tobytes()
    assert g.tobytes() == got_g.tobytes()
    assert sm.tobytes() == got_s.tobytes()


def test_mirror_energy_covariance_and_entropy_gradient_repeat_bit_for_bit():
  """energy_covariance (one parity sum per distinct xor mask over the rows) and the entropy gradient of
  AnalyticEnergyInference (all 2^16 bitstrings) run the VJP over more rows than one workgroup of the earlier kernel
  held: repeats must agree to the bit, and the covariance must match its host fp64 path."""
  n = 16
  rng = np.random.default_rng(5)
  energy = models.KOBE(list(range(n)), 2)
  with torch.no_grad():
    energy.post_process[0].kernel.copy_(torch.as_tensor(rng.uniform(-0.5, 0.5, n + n * (n - 1) // 2)))
  rows = 3 * 2048 + 5
  bits = torch.as_tensor(rng.integers(0, 2, size=(rows, n)), dtype=torch.int8)
  w = torch.as_tensor(rng.random(rows), dtype=torch.float64)
  w = w / w.sum()
  host = information.energy_covariance(energy, bits, w)
  dev = energy.to("cuda")
  covs = [information.energy_covariance(dev, bits.cuda(), w.cuda()).cpu() for _ in range(3)]
  for c in covs[1:]:
    assert c.numpy().tobytes() == covs[0].numpy().tobytes()
  # each parity sum: fp32 weights (relative 2^-24 each), fp64 sum, one fp32 rounding of a value <= 1; the covariance
  # is second - mu mu^T with |mu| <= 1: at most (3 + 3) x 2^-24 per entry, plus fp64 noise
  np.testing.assert_allclose(covs[0].numpy(), host.numpy(), rtol=0, atol=8 * 2.0**-24)
  inf = inference.AnalyticEnergyInference(dev, 10, initial_seed=1)
  grads = [torch.autograd.grad(inf.entropy(), dev.post_process[0].kernel)[0].cpu() for _ in range(3)]
  for g in grads[1:]:
    assert g.numpy().tobytes() == grads[0].numpy().tobytes()
