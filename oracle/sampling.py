"""Exact host restatement of the engine's sampler (qhbm_sample / qhbm_sample_counts), for the tests.

The engine draws shot j of state row s of program q from the counter-based generator Philox4x32-10
(Salmon et al., SC'11; the Random123 reference constants) with counter {j, s, 0x51b0c6a1, q} and key
(seed mod 2^32, seed >> 32), turns the first two output words into one fp64 uniform
u = c0 2^-32 + c1 2^-64 in [0, 1), and returns the first outcome whose inclusive cumulative
probability exceeds u.  Given the probabilities, every shot is therefore a pure function that can
be restated here in numpy.  The product never imports this module.
"""
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_SHIFT = np.uint64(32)
COUNTER_TAG = 0x51B0C6A1  # third counter word of every draw


def philox4x32_10(counter, key):
  """Philox4x32-10 of counters [..., 4] (uint32 words c0..c3) under keys [..., 2] (k0, k1), broadcast
  against each other; returns the four uint32 output words [..., 4]."""
  counter = np.asarray(counter, dtype=np.uint64)
  key = np.asarray(key, dtype=np.uint64)
  c0, c1, c2, c3 = (counter[..., i] for i in range(4))
  k0, k1 = key[..., 0], key[..., 1]
  for r in range(10):
    p0, p1 = _M0 * c0, _M1 * c2  # 32 x 32 -> 64-bit products, exact in uint64
    c0, c1, c2, c3 = ((p1 >> _SHIFT) ^ c1 ^ k0, p1 & _LO, (p0 >> _SHIFT) ^ c3 ^ k1, p0 & _LO)
    if r < 9:
      k0, k1 = (k0 + np.uint64(_W0)) & _LO, (k1 + np.uint64(_W1)) & _LO
  return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def engine_uniforms(n_shots, state_row, seed, program=0, shot0=0):
  """fp64 [n_shots]: the uniforms of shots shot0 .. shot0 + n_shots - 1 of (state_row, program)."""
  shots = np.arange(shot0, shot0 + n_shots, dtype=np.uint64)
  counter = np.zeros((n_shots, 4), np.uint64)
  counter[:, 0] = shots
  counter[:, 1] = state_row
  counter[:, 2] = COUNTER_TAG
  counter[:, 3] = program
  seed = int(seed) & (2**64 - 1)
  out = philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))
  # the same two fp64 operations as the kernel: both products are exact, the sum rounds once
  return out[:, 0].astype(np.float64) * 2.0**-32 + out[:, 1].astype(np.float64) * 2.0**-64


def cdf(probs):
  """Inclusive fp64 prefix sums of `probs`, normalised to end at exactly 1."""
  c = np.cumsum(np.asarray(probs, dtype=np.float64))
  return c / c[-1]


def inverse_cdf(cum, u):
  """The first outcome whose inclusive prefix `cum` exceeds u (u in [0, cum[-1]))."""
  return np.searchsorted(cum, u, side="right")


def restated_outcomes(probs, n_shots, state_row, seed, program=0):
  """int64 [n_shots]: the outcomes the engine's sampler would draw from `probs` if it computed them exactly."""
  return inverse_cdf(cdf(probs), engine_uniforms(n_shots, state_row, seed, program))
