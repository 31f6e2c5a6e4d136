"""The flat definition of qhbm_sample_parities in numpy, and the dyadic states on which it is exact.

For a state row with masses p (float64), shot j takes the uniform u_j of the engine's sampler
(oracle.sampling.engine_uniforms: Philox4x32-10, counter {j, row, 0x51b0c6a1, program}) and the outcome
    x_j = searchsorted(cumsum(p), u_j * total, side="right"),   total = cumsum(p)[-1],
clamped to the last outcome of non-zero mass; the result is S[t] = sum_j (-1)^popcount(x_j & m_t) with the masks in
qubit space (bit k = qubit k = the k-th most significant bit of the outcome index).

DYADIC states have amplitudes +-2^-e or +-i 2^-e, e in [0, 12], or exact zeros: every mass is a multiple of 2^-24 and
every partial sum of up to 2^n of them is below 2^n, so for n + 24 <= 53 all partial sums are exact in float64 in EVERY
order of additions, and u * total - (an exact prefix) is exact as well.  A correct kernel therefore draws exactly the
outcomes of the flat definition, whatever tree it adds in: the GPU tests ask for integer equality.
"""
import numpy as np

from oracle import sampling as S


def index_masks(masks, n):
  """Qubit-space masks -> masks over the bits of the outcome index (qubit 0 = most significant of n bits)."""
  out = np.zeros(len(masks), np.int64)
  for t, m in enumerate(masks):
    m = int(m)
    assert 0 <= m < (1 << n), (m, n)
    for k in range(n):
      if (m >> k) & 1:
        out[t] |= 1 << (n - 1 - k)
  return out


def restated_outcomes(p, n_shots, row, seed, program=0):
  """int64 [n_shots]: positions in `p` drawn by the flat definition (p float64, not necessarily normalised; a row of
  total 0 has no outcomes and returns None)."""
  p = np.asarray(p, np.float64)
  cum = np.cumsum(p)
  total = cum[-1]
  if not total > 0:
    return None
  u = S.engine_uniforms(n_shots, row, seed, program)
  x = np.searchsorted(cum, u * total, side="right")
  return np.minimum(x, np.flatnonzero(p > 0)[-1])


def sums_of_counts(vals, counts, masks, n):
  """int64 [T]: sum over the outcome indices `vals`, each taken `counts` times, of (-1)^popcount(x & mask_t)."""
  idx = index_masks(masks, n)
  vals, counts = np.asarray(vals, np.int64), np.asarray(counts, np.int64)
  out = np.zeros(len(idx), np.int64)
  for t, m in enumerate(idx):
    par = vals & m
    for sh in (32, 16, 8, 4, 2, 1):
      par = par ^ (par >> sh)
    out[t] = int((counts * (1 - 2 * (par & 1))).sum())
  return out


def signed_sums(outcomes, masks, n):
  """int64 [T]: sum over the outcome indices of (-1)^popcount(x & mask_t) (None: no outcomes)."""
  if outcomes is None:
    return np.zeros(len(masks), np.int64)
  vals, counts = np.unique(np.asarray(outcomes, np.int64), return_counts=True)
  return sums_of_counts(vals, counts, masks, n)


def restated_sums(p, masks, n_shots, row, seed, program=0, support=None, n_qubits=None):
  """int64 [T] of the flat definition.  `p`: the masses of all 2^n outcomes, or -- with `support` (sorted outcome
  indices) and `n_qubits` -- of those outcomes alone, every other mass being an exact zero (which moves no prefix)."""
  p = np.asarray(p, np.float64)
  n = int(n_qubits) if n_qubits is not None else int(p.size).bit_length() - 1
  x = restated_outcomes(p, n_shots, row, seed, program)
  if x is not None and support is not None:
    x = np.asarray(support, np.int64)[x]
  return signed_sums(x, masks, n)


def masses(states):
  """float64 masses of complex64 states: re^2 + im^2 with exact products, one rounding in the sum."""
  s = np.asarray(states)
  return s.real.astype(np.float64)**2 + s.imag.astype(np.float64)**2


def dyadic_states(rng, num, n, zero_share=0.3):
  """complex64 [num, 2^n]: amplitudes +-2^-e or +-i 2^-e, e in [0, 12], `zero_share` of them exact zeros; not normalised."""
  shape = (num, 1 << n)
  mag = np.ldexp(1.0, -rng.integers(0, 13, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
  mag[rng.random(shape) < zero_share] = 0.0
  imag = rng.random(shape) < 0.5
  out = np.where(imag, 1j * mag, mag).astype(np.complex64)
  if not (np.abs(out).sum(axis=1) > 0).all():   # (a row must keep some mass: only possible at tiny n)
    out[:, 0] = 1.0
  return out


def mask_set(rng, n, count):
  """`count` qubit-space masks: 0, all ones, then random ones (a single mask: all ones)."""
  full = (1 << n) - 1
  fixed = [0, full] if count > 1 else [full]
  return np.array(fixed + [int(rng.integers(0, full + 1)) for _ in range(count - len(fixed))], np.uint64)
