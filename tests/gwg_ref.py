"""Exact host restatement of the device Gibbs-With-Gradients chain (qhbm_gwg_sample, csrc/gwg.hip), for the tests.

The chain.  For E(x) = sum_k theta_k s_k(x), s_k(x) = (-1)^popcount(x & mask_k), let
    h_j(x) = (E(x) - E(x ^ e_j)) / 2 = sum_{k : bit j in mask_k} theta_k s_k(x),     L(x) = logsumexp_j h_j(x).
Absolute step t of chain c draws Philox4x32-10 (`oracle.sampling.philox4x32_10`) with key (seed mod 2^32, seed >> 32)
and counter {t mod 2^32, t >> 32, COUNTER_TAG, c}; u1 = w0 2^-32 + w1 2^-64 and u2 = w2 2^-32 + w3 2^-64 in fp64.  With
p_j = exp(h_j - max h) and its inclusive prefix sums in bit order, the step picks the first bit i whose prefix exceeds
u1 * sum p (the last bit if none does) and accepts x' = x ^ e_i iff u2 <= exp(min(0, L(x) - L(x'))).  Everything here is
fp64; the kernel does the same in fp32 from the same uniforms.

When do the two agree step for step?  The tests use DYADIC theta (multiples of 2^-8, |h| < 2^15), so every h_j, max h and
h_j - max h is exact in fp32 as it is here.  What is left are these fp32 operations of the kernel (eps = 2^-24):

  p_j = expf(h_j - max h)          relative error <= 2 ulp = 4 eps (the device library documents 1 ulp)
  prefix_j, sum p                  a Hillis-Steele scan: every prefix is a binary tree of at most 6 levels of sums of
                                   non-negative numbers, relative error <= 6 eps on top of the 4 eps of its inputs:
                                   <= 10 eps < 2^-20 each
  pick: prefix_j > u1 * sum p      (compared in fp64) can differ from the exact comparison only if
                                   |prefix_j / sum p - u1| <= 2 * 2^-20 = 2^-19                                    (P)
  L = max h + logf(sum p)          sum p is in [1, 64]: its relative error moves the logarithm by <= 2^-20; logf adds
                                   <= 2 ulp of a value below ln 64 < 8, i.e. <= 2^-20; the sum rounds once, <= eps |L|:
                                   |dL| <= 2^-19 + eps |L|
  a = L - L'                       one more rounding, <= eps |a|
  A = expf(min(0, a))              |dA/da| <= 1 for a <= 0, and expf adds <= 2 ulp of a value <= 1, i.e. <= 2 eps:
                                   |dA| <= e_A := 2^-18 + 2 eps + eps (|L| + |L'| + |a|)                           (A)

A step is AMBIGUOUS when u1 is within delta of an interior boundary prefix_j / sum p (j < n_bits - 1) or u2 is within
delta of A (for A = 1 that also covers a that rounds across zero), with
    delta = max(2^-16, 4 e_A):
at least 4 x the bound (A), and at least 8 x the bound (P).  On a run without an ambiguous step the kernel must
reproduce every sample, every final state and every accepted count; the GPU tests use only such runs, and
tests/test_gwg_ref_cpu.py asserts that their cases have none.  The product never imports this module.
"""
import numpy as np

from oracle.sampling import philox4x32_10

COUNTER_TAG = 0x47574731   # third counter word ("GWG1"); the shot sampler's is 0x51B0C6A1
DELTA_FLOOR = 2.0**-16
_EPS = 2.0**-24


def live_masks(masks, n_bits):
  """uint64 masks with the bits at or above n_bits cleared (the kernel ignores them)."""
  keep = np.uint64(2**n_bits - 1)
  return np.asarray(masks, dtype=np.uint64) & keep


def membership(masks, n_bits):
  """float64 [n_terms, n_bits]: 1 where bit j is in mask k."""
  m = live_masks(masks, n_bits)
  return ((m[:, None] >> np.arange(n_bits, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.float64)


def half_deltas(x, masks, thetas, n_bits):
  """h [chains, n_bits] of packed states x [chains] (uint64)."""
  m = live_masks(masks, n_bits)
  x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
  signs = 1.0 - 2.0 * (np.bitwise_count(x[:, None] & m[None, :]) & 1)
  return (signs * np.asarray(thetas, np.float64)[None, :]) @ membership(masks, n_bits)


def log_norm(h):
  """(max h, p = exp(h - max h), L = max h + log sum p) along the last axis."""
  top = h.max(-1)
  p = np.exp(h - top[..., None])
  return top, p, top + np.log(p.sum(-1))


def proposal_probs(x, masks, thetas, n_bits):
  """q(j | x) = softmax(d(x) / 2)_j, [chains, n_bits]."""
  _, p, _ = log_norm(half_deltas(x, masks, thetas, n_bits))
  return p / p.sum(-1, keepdims=True)


def acceptance(x, i, masks, thetas, n_bits):
  """min(1, exp(L(x) - L(x ^ e_i))) for packed states x [chains] and bit indices i [chains]."""
  x = np.atleast_1d(np.asarray(x, dtype=np.uint64))
  y = x ^ (np.uint64(1) << np.asarray(i, dtype=np.uint64))
  _, _, lx = log_norm(half_deltas(x, masks, thetas, n_bits))
  _, _, ly = log_norm(half_deltas(y, masks, thetas, n_bits))
  return np.exp(np.minimum(0.0, lx - ly))


def uniforms(seed, step0, n_steps, n_chains):
  """(u1, u2), fp64 [n_steps, n_chains]: the uniforms of absolute steps step0 .. step0 + n_steps - 1."""
  seed = int(seed) & (2**64 - 1)
  steps = np.arange(n_steps, dtype=np.uint64) + np.uint64(step0)
  counter = np.zeros((n_steps, n_chains, 4), np.uint64)
  counter[..., 0] = (steps & np.uint64(0xFFFFFFFF))[:, None]
  counter[..., 1] = (steps >> np.uint64(32))[:, None]
  counter[..., 2] = COUNTER_TAG
  counter[..., 3] = np.arange(n_chains, dtype=np.uint64)[None, :]
  w = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)).astype(np.float64)
  return w[..., 0] * 2.0**-32 + w[..., 1] * 2.0**-64, w[..., 2] * 2.0**-32 + w[..., 3] * 2.0**-64


def pack(bits):
  """uint64 [rows] of int bit rows [rows, n] (column q = bit q)."""
  bits = np.asarray(bits).astype(np.uint64)
  return (bits << np.arange(bits.shape[1], dtype=np.uint64)[None, :]).sum(1, dtype=np.uint64)


def unpack(states, n_bits):
  """int8 [..., n_bits] of packed states."""
  s = np.asarray(states, dtype=np.uint64)
  return ((s[..., None] >> np.arange(n_bits, dtype=np.uint64)) & np.uint64(1)).astype(np.int8)


def run(states, n_bits, masks, thetas, seed, step0, n_steps):
  """The chains from packed `states` [chains] for n_steps steps.  Returns a dict:
  samples int8 [n_steps, chains, n_bits], states uint64 [chains] (final), accepted int64 [chains],
  ambiguous bool [n_steps, chains], delta float64 [n_steps, chains]."""
  x = np.array(states, dtype=np.uint64).reshape(-1)
  n_chains = x.size
  u1, u2 = uniforms(seed, step0, n_steps, n_chains)
  samples = np.zeros((n_steps, n_chains, n_bits), np.int8)
  ambiguous = np.zeros((n_steps, n_chains), bool)
  deltas = np.zeros((n_steps, n_chains))
  accepted = np.zeros(n_chains, np.int64)
  _, p, lx = log_norm(half_deltas(x, masks, thetas, n_bits))
  for t in range(n_steps):
    cum = np.cumsum(p, -1)
    total = cum[:, -1]
    over = cum > (u1[t] * total)[:, None]
    pick = np.where(over.any(1), over.argmax(1), n_bits - 1)
    y = x ^ (np.uint64(1) << pick.astype(np.uint64))
    _, py, ly = log_norm(half_deltas(y, masks, thetas, n_bits))
    a = lx - ly
    prob = np.exp(np.minimum(0.0, a))
    delta = np.maximum(DELTA_FLOOR, 4.0 * (2.0**-18 + 2.0 * _EPS + _EPS * (np.abs(lx) + np.abs(ly) + np.abs(a))))
    near_pick = (np.abs(cum[:, :-1] / total[:, None] - u1[t][:, None]) <= delta[:, None]).any(1)
    ambiguous[t] = near_pick | (np.abs(u2[t] - prob) <= delta)
    deltas[t] = delta
    take = u2[t] <= prob
    x = np.where(take, y, x)
    p = np.where(take[:, None], py, p)
    lx = np.where(take, ly, lx)
    accepted += take
    samples[t] = unpack(x, n_bits)
  return dict(samples=samples, states=x, accepted=accepted, ambiguous=ambiguous, delta=deltas)


# ---- the exact cases of tests/test_gwg_chain_gpu.py (tests/test_gwg_ref_cpu.py checks that none has an ambiguous step) ----

def kobe_masks(n_bits, order):
  """Masks of a KOBE in the order of energy_utils.Parity: all index sets of size 1, then 2, ... up to `order`."""
  import itertools  # pylint: disable=import-outside-toplevel
  sets = [c for k in range(1, order + 1) for c in itertools.combinations(range(n_bits), k)]
  return np.array([sum(1 << q for q in c) for c in sets], dtype=np.uint64)


def _dyadic(rng, size, denom):
  return rng.integers(-64, 65, size=size) / float(denom)


def exact_case(name):
  """dict(n_bits, masks, thetas, states, seed, n_steps) of a named exact case; theta is dyadic."""
  seed = EXACT_SEEDS[name]
  rng = np.random.default_rng(seed)
  if name == "n1":
    n, masks, thetas, chains, steps = 1, kobe_masks(1, 1), np.array([0.75]), 2, 64
  elif name == "bernoulli5":
    n, masks, chains, steps = 5, kobe_masks(5, 1), 3, 2048
    thetas = _dyadic(rng, 5, 64)
  elif name == "kobe2_n12":
    n, masks, chains, steps = 12, kobe_masks(12, 2), 8, 512
    thetas = _dyadic(rng, masks.size, 64)
  elif name == "kobe2_n33":
    n, masks, chains, steps = 33, kobe_masks(33, 2), 2, 128
    thetas = _dyadic(rng, masks.size, 64)
  elif name == "kobe3_n20":
    n, masks, chains, steps = 20, kobe_masks(20, 3), 2, 256
    thetas = _dyadic(rng, masks.size, 256)
  elif name in ("edges_n64", "edges_n40"):
    # order 1, random masks that use bit 63, a zero mask, a duplicated mask; at 40 bits the same masks carry bits >= n
    n = 64 if name == "edges_n64" else 40
    chains, steps = 2, 64
    extra = rng.integers(0, 2**63, size=6, dtype=np.uint64) | (np.uint64(1) << np.uint64(63))
    masks = np.concatenate([kobe_masks(n, 1), extra, np.array([0], np.uint64), extra[:1]])
    thetas = _dyadic(rng, masks.size, 64)
  elif name == "theta0_n7":
    n, masks, chains, steps = 7, kobe_masks(7, 2), 2, 128
    thetas = np.zeros(masks.size)
  elif name == "theta128_n5":
    n, masks, chains, steps = 5, kobe_masks(5, 1), 2, 256
    thetas = np.full(5, 128.0)
    return dict(n_bits=n, masks=masks, thetas=thetas, states=np.zeros(chains, np.uint64), seed=seed, n_steps=steps)
  else:
    raise KeyError(name)
  states = rng.integers(0, 2**63, size=chains, dtype=np.uint64) & np.uint64(2**n - 1)
  if n == 64:
    states[0] |= np.uint64(1) << np.uint64(63)
  return dict(n_bits=n, masks=masks, thetas=thetas, states=states, seed=seed, n_steps=steps)


# Seeds (they also seed the case's theta and initial states) picked so that the restatement has no ambiguous step.
EXACT_SEEDS = {
    "n1": 1, "bernoulli5": 3, "kobe2_n12": 11, "kobe2_n33": 1, "kobe3_n20": 3, "edges_n64": 1, "edges_n40": 1,
    "theta0_n7": 1, "theta128_n5": 2,
}


def stats_case():
  """The 4-bit KOBE-2 of the statistical check: (n_bits, masks, thetas), dyadic theta.  Its entropy is 5 % below
  log 16 and its rarest bitstring has probability 0.02."""
  rng = np.random.default_rng(6)
  masks = kobe_masks(4, 2)
  return 4, masks, rng.integers(-24, 25, size=masks.size) / 64.0


def exact_probs(n_bits, masks, thetas):
  """Boltzmann probabilities of all 2^n packed states 0 .. 2^n - 1."""
  x = np.arange(2**n_bits, dtype=np.uint64)
  m = live_masks(masks, n_bits)
  e = (1.0 - 2.0 * (np.bitwise_count(x[:, None] & m[None, :]) & 1)) @ np.asarray(thetas, np.float64)
  w = np.exp(-(e - e.min()))
  return w / w.sum()


def _entropy(p):
  p = np.asarray(p, dtype=np.float64)
  p = p[p > 0]
  return float(-(p * np.log(p)).sum())


def check_statistics(samples, n_bits, masks, thetas):
  """The reference's criteria (ebm_test.py:879-947, as in tests/test_gwg_cpu.py) for int8 samples [m, n_bits]: entropy
  within rtol 1e-2, not uniform, every bitstring visited, every probability within 2e-2."""
  expected = exact_probs(n_bits, masks, thetas)
  counts = np.bincount(pack(samples).astype(np.int64), minlength=2**n_bits)
  actual = counts / counts.sum()
  np.testing.assert_allclose(_entropy(actual), _entropy(expected), rtol=1e-2)
  assert abs(_entropy(actual) - np.log(2**n_bits)) > 2e-2 * np.log(2**n_bits)
  assert np.all(counts > 0)
  assert np.all(np.abs(actual - expected) < 2e-2)


# ---- the mirror-level case: GibbsWithGradientsInference(KOBE-2 over 9 bits, chain="device") ----
MIRROR_BURNIN = 50
MIRROR_SEED = 1


def mirror_case(num_chains):
  """(n_bits, masks, thetas, seed, initial packed states): what the inference built with initial_seed = MIRROR_SEED
  runs, its initial states drawn here as it draws them (chain 0, then the others, from one torch generator)."""
  import torch  # pylint: disable=import-outside-toplevel
  n = 9
  masks = kobe_masks(n, 2)
  thetas = np.random.default_rng(9).integers(-64, 65, size=masks.size) / 64.0
  gen = torch.Generator().manual_seed(MIRROR_SEED)
  rows = torch.bernoulli(torch.full((n,), 0.5), generator=gen).reshape(1, n)
  if num_chains > 1:
    rows = torch.cat([rows, torch.bernoulli(torch.full((num_chains - 1, n), 0.5), generator=gen)], 0)
  return n, masks, thetas, MIRROR_SEED, pack(rows.numpy())
