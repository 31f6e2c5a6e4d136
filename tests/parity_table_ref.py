"""Numpy restatement behind the parity-table tests (no engine code is used here).

The table of all 2^n energies of E(x) = sum_k theta_k (-1)^popcount(x & mask_k) is the unnormalised Walsh-Hadamard
transform H[y] = sum_m c[m] (-1)^popcount(y & m) of the coefficient vector c with theta_k at index rev_n(mask_k): column
q of a bitstring is mask bit q, and table index y holds column q at bit n-1-q (`energy_utils.all_bitstrings`).  The VJP
sum_y w[y] parity_k(y) is entry rev_n(mask_k) of the transform of w.

TILE_BITS, ROW_BITS and the pass boundaries restate the launcher's constants (csrc/parity_table.hip kWhtTileBits,
kWhtRowBits; `_engine.WHT_TILE_BITS`, `_engine.WHT_ROW_BITS`)."""
import itertools

import numpy as np

MAX_BITS = 30
TILE_BITS = 14                 # K: up to here one launch
ROW_BITS = 9                   # index bits each further pass adds
N2 = TILE_BITS + 1             # smallest n with 2 passes
N3 = TILE_BITS + ROW_BITS + 1  # smallest n with 3 passes; a fourth pass would start at 33 > MAX_BITS


def num_passes(n):
  return 1 if n <= TILE_BITS else 1 + -(-(n - TILE_BITS) // ROW_BITS)


def raw_sizes():
  """Every n from 1 to N2 + 1, the three sizes around every further pass boundary, and 29, 30 (byte offsets pass 2^31, 2^32)."""
  return sorted(set(range(1, N2 + 2)) | {N3 - 1, N3, N3 + 1} | {29, 30})


def boundaries(n):
  """Index bits where the transform of 2^n entries changes pass, tile or register geometry: the register rounds of a tile
  (5, 9, 13), the tile and the pass boundaries, and where the shifted last pass starts its rows."""
  out = {5, 9, 13, TILE_BITS, TILE_BITS + ROW_BITS, n - ROW_BITS}
  return sorted(b for b in out if 0 < b < n)


def _butterflies(c):
  h = 1
  while h < c.size:
    c = c.reshape(-1, 2, h)
    c = np.stack([c[:, 0] + c[:, 1], c[:, 0] - c[:, 1]], axis=1).reshape(-1)
    h *= 2
  return c


def wht_f64(x):
  return _butterflies(np.asarray(x, dtype=np.float64).copy())


def wht_i64(x):
  return _butterflies(np.asarray(x, dtype=np.int64).copy())


def rev_n(m, n):
  """The low n bits of m reversed (bits at or above n are dropped)."""
  m = np.asarray(m, dtype=np.uint64)
  out = np.zeros_like(m)
  for q in range(n):
    out |= ((m >> np.uint64(q)) & np.uint64(1)) << np.uint64(n - 1 - q)
  return out


def scatter(masks, thetas, n, dtype=np.float64):
  """c[rev_n(mask_k)] += theta_k in ascending term order, in `dtype` arithmetic (float32: the kernel's own roundings)."""
  c = np.zeros(1 << n, dtype=dtype)
  for idx, th in zip(rev_n(masks, n), np.asarray(thetas)):
    c[int(idx)] = dtype(c[int(idx)] + dtype(th))
  return c


def multiplicity(masks, n):
  """d: the largest number of terms that share one mask (1 for distinct masks, 0 for no terms)."""
  idx = rev_n(masks, n)
  return int(np.unique(idx, return_counts=True)[1].max()) if idx.size else 0


def _odd(x):
  """popcount(x) & 1 of uint64 values."""
  x = np.asarray(x, dtype=np.uint64).copy()
  for s in (32, 16, 8, 4, 2, 1):
    x ^= x >> np.uint64(s)
  return (x & np.uint64(1)).astype(np.int64)


def sparse_eval(positions, values, ys, dtype=np.int64):
  """H[y] = sum_j values[j] (-1)^popcount(y & positions[j]) for every y of `ys`: single outputs of the transform of a
  sparse input, on the host."""
  positions = np.asarray(positions, dtype=np.uint64)
  values = np.asarray(values, dtype=dtype)
  ys = np.asarray(ys, dtype=np.uint64)
  out = np.zeros(ys.shape, dtype=dtype)
  for lo in range(0, ys.size, 512):
    sign = 1 - 2 * _odd(ys[lo:lo + 512, None] & positions[None, :])
    out[lo:lo + 512] = (sign.astype(dtype) * values[None, :]).sum(1)
  return out


def table(masks, thetas, n):
  """float64 [2^n] energies in `all_bitstrings` order through scatter + transform."""
  return wht_f64(scatter(masks, thetas, n))


def vjp(masks, weights, n):
  """float64 [T]: sum_y weights[y] parity_k(y)."""
  return wht_f64(weights)[rev_n(masks, n).astype(np.int64)]


def table_by_terms(index_sets, thetas, n):
  """float64 [2^n]: sum_k theta_k prod_{q in S_k} (1 - 2 x_q) over the rows of itertools.product([0, 1], repeat=n)."""
  bits = np.array(list(itertools.product([0, 1], repeat=n)), dtype=np.int64).reshape(1 << n, n)
  spins = 1 - 2 * bits
  out = np.zeros(1 << n)
  for ix, th in zip(index_sets, thetas):
    out += th * np.prod(spins[:, list(ix)], axis=1)
  return out


def kobe_index_sets(n, order):
  """`energy_utils.Parity` order: all groups of size 1..order in itertools.combinations order."""
  sets = []
  for i in range(1, order + 1):
    sets.extend(itertools.combinations(range(n), i))
  return sets


def masks_of(index_sets):
  return np.asarray([sum(1 << int(q) for q in ix) for ix in index_sets], dtype=np.uint64)


# ---- case generators ------------------------------------------------------------------------------------------------
def structured_indices(n):
  """0, 2^n - 1, every single bit and every pair of bits (so every pair on either side of every boundary)."""
  out = [0, (1 << n) - 1] + [1 << a for a in range(n)]
  out += [(1 << a) | (1 << b) for a in range(n) for b in range(a + 1, n)]
  return np.unique(np.asarray(out, dtype=np.uint64))


DENSE_MAX_BITS = 20


def raw_case(n, seed=0):
  """(positions uint64 [S] or None, values int64): an integer-valued input of the raw transform with sum |x| < 2^24.
  Up to 20 bits dense entries in -7..7 (positions None, values [2^n]); above, a random support of 2^12 positions plus
  the structured ones, entries in -7..7 without zero."""
  rng = np.random.default_rng(1000 * n + seed)
  if n <= DENSE_MAX_BITS:
    return None, rng.integers(-7, 8, 1 << n).astype(np.int64)
  positions = np.unique(np.concatenate([rng.integers(0, 1 << n, 1 << 12).astype(np.uint64), structured_indices(n)]))
  values = rng.integers(1, 8, positions.size) * rng.choice([-1, 1], positions.size)
  return positions, values.astype(np.int64)


def raw_outputs(n, seed=0):
  """At least 4096 output indices to compare above 22 bits: random ones plus the structured ones."""
  rng = np.random.default_rng(2000 * n + seed)
  return np.unique(np.concatenate([rng.integers(0, 1 << n, 4096).astype(np.uint64), structured_indices(n)]))


def dyadic_thetas(count, rng):
  """Multiples of 2^-6 with |theta| <= 1: every partial sum of up to 2^18 of them is exact in fp32."""
  return rng.integers(-64, 65, count).astype(np.float64) / 64.0


TABLE_BITS = (1, 2, 5, 12, N2, N2 + 1)


def hand_made_terms(n):
  """{name: (masks, thetas)}: a zero mask, three equal masks, a mask with bits at or above n, no terms."""
  top = np.uint64(1) << np.uint64(n - 1)
  high = (np.uint64(1) << np.uint64(n)) | (np.uint64(1) << np.uint64(40)) | (np.uint64(1) << np.uint64(63))
  return {
      "zero mask": (np.asarray([0, 1, 3], np.uint64), np.asarray([0.5, -0.25, 0.75])),
      "three equal masks": (np.asarray([5, top | np.uint64(1), 5, 2, 5], np.uint64),
                            np.asarray([0.5, -1.0, 0.25, 0.125, -0.015625])),
      "bits at or above n": (np.asarray([np.uint64(3) | high, high, top], np.uint64), np.asarray([1.0, -0.5, 0.25])),
      "no terms": (np.zeros(0, np.uint64), np.zeros(0)),
  }


def integer_weights(n, seed=0):
  return np.random.default_rng(3000 * n + seed).integers(-7, 8, 1 << n).astype(np.float32)


def exactness_violations():
  """Strings naming every exact case whose partial sums are not integers (or dyadic multiples of one unit) of magnitude
  below 2^24; empty = every bit-for-bit comparison of the GPU tests is justified."""
  bad = []
  for n in raw_sizes():
    _, values = raw_case(n)
    if not np.abs(values).sum() < 2**24:
      bad.append(f"raw n={n}: sum |x| = {np.abs(values).sum()}")
  rng = np.random.default_rng(0)
  for n in TABLE_BITS + (20,):
    for order in (1, 2, 3):
      count = len(kobe_index_sets(n, order))
      th = dyadic_thetas(count, rng) * 64.0
      if not (np.array_equal(th, np.round(th)) and count * 64 < 2**24):
        bad.append(f"table n={n} order={order}: {count} terms in units of 2^-6")
  for n in (7, N2):
    for name, (_, th) in hand_made_terms(n).items():
      units = np.asarray(th) * 64.0
      if not (np.array_equal(units, np.round(units)) and np.abs(units).sum() < 2**24):
        bad.append(f"hand-made '{name}' n={n}")
  for n in VJP_EXACT_BITS:
    w = integer_weights(n)
    if not (np.array_equal(w, np.round(w)) and np.abs(w.astype(np.float64)).sum() < 2**24):
      bad.append(f"vjp n={n}: sum |w| = {np.abs(w).sum()}")
  return bad


VJP_EXACT_BITS = (5, 12, N2, N2 + 1, 20)
