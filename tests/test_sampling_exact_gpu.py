"""qhbm_sample / qhbm_sample_counts shot for shot against the exact host restatement of the sampler
(oracle/sampling.py: the same Philox4x32-10 uniform per (shot, state row, program), inverted through the fp64 CDF
of the complex128 reference probabilities).

A shot may differ from the restatement only where the kernels' own rounding can move it: u within delta of a
reference CDF boundary, delta = ||p_gpu - p_ref||_1 (p_gpu from qhbm_statevector of the same call) + the worst case of
the fp32 scan inside a 1024-amplitude block, 1024 2^-24 (largest block mass).  Every mismatch must be explained by
delta; against the restatement on the engine's own probabilities, at most 10^-3 of the shots may differ.
Generator-free checks: outcomes of zero reference probability never appear, and a G-test of the full histogram on the
dense states."""
import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from oracle import sampling as S
from qhbmlib_amd import _engine as E
from tests.test_engine_gpu import random_circuit

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15


def _engine(n, gates, n_params, **opts):
  eng = E.Engine(0)
  for k, v in opts.items():
    eng.set_option(k, v)
  eng.set_circuit(n, gates, n_params)
  return eng


def _index(samples):
  """int64 outcome index of int8 samples [..., n] (qubit 0 = most significant bit)."""
  n = samples.shape[-1]
  return (samples.astype(np.int64) << np.arange(n - 1, -1, -1, dtype=np.int64)).sum(-1)


class Ref:
  """The reference distribution of one state row: its support (sorted outcome indices) and fp64 probabilities."""

  def __init__(self, support, probs):
    keep = probs > 0
    self.support = np.asarray(support, np.int64)[keep]
    self.probs = np.asarray(probs, np.float64)[keep]
    self.cum = S.cdf(self.probs)

  @staticmethod
  def dense(p):
    return Ref(np.arange(p.size), p)


def _delta(psi, ref):
  """||p_gpu - p_ref||_1 (both normalised) + the fp32 in-block scan bound, from the GPU state psi [2^n]."""
  p = psi.abs().to(torch.float64)**2
  p = p / p.sum()
  sup = torch.from_numpy(ref.support).to(psi.device)
  ps = p[sup]
  l1 = float((p.sum() - ps.sum()).abs() + (ps - torch.from_numpy(ref.probs / ref.probs.sum()).to(psi.device)).abs().sum())
  block = float(p.reshape(-1, 1024).sum(1).max()) if p.numel() >= 1024 else 1.0
  # + the global-phase rescaling qhbm_statevector applies after the sampler's state (|c + is| = 1 in fp32)
  return l1 + 1024 * 2.0**-24 * block + 4 * 2.0**-24


def _gpu_ref(psi):
  """The restatement's distribution on the engine's own fp32 state (complex64 [2^n] -> fp64 probabilities)."""
  return Ref.dense(np.abs(psi.cpu().numpy().astype(np.complex128))**2)


def _check_shots(got, ref, delta, row, program=0, gpu_ref=None):
  """got: int64 [n_shots] outcome indices drawn by the engine for (row, program).  Every shot must be delta-consistent
  with the reference; at most 10^-3 of them may differ from the restatement -- on the engine's own probabilities
  `gpu_ref` where given (above ~20 qubits the fp32 state alone moves more shots than that off the fp64 CDF), else on
  the reference."""
  u = S.engine_uniforms(got.size, row, SEED, program)
  k_ref = S.inverse_cdf(ref.cum, u)
  pos = np.searchsorted(ref.support, got)
  in_support = (pos < ref.support.size) & (ref.support[np.minimum(pos, ref.support.size - 1)] == got)
  assert in_support.all(), f"zero-probability outcomes drawn: {np.unique(got[~in_support])[:8]}"
  mismatch = pos != k_ref
  lower = np.where(pos > 0, ref.cum[np.maximum(pos - 1, 0)], 0.0)
  explained = (u >= lower - delta) & (u < ref.cum[pos] + delta)
  assert explained[mismatch].all(), (np.flatnonzero(mismatch & ~explained)[:8], delta)
  if gpu_ref is not None:
    mismatch = gpu_ref.support[S.inverse_cdf(gpu_ref.cum, u)] != got
  assert mismatch.sum() <= 1e-3 * got.size, (int(mismatch.sum()), got.size, delta)


def _restated_counts(ref, n_shots, row, program, delta, dim):
  u = S.engine_uniforms(n_shots, row, SEED, program)
  k = S.inverse_cdf(ref.cum, u)
  lower = np.where(k > 0, ref.cum[np.maximum(k - 1, 0)], 0.0)
  ambiguous = int(((u - lower < delta) | (ref.cum[k] - u <= delta)).sum())
  return np.bincount(ref.support[k], minlength=dim), ambiguous


def _g_test(counts, ref):
  """p-value of the G-test of the full histogram (bins of expectation < 5 pooled)."""
  from scipy import stats  # pylint: disable=import-outside-toplevel
  shots = counts.sum()
  expect = ref.probs / ref.probs.sum() * shots
  obs = counts[ref.support].astype(np.float64)
  small = expect < 5
  e = np.append(expect[~small], expect[small].sum())
  o = np.append(obs[~small], obs[small].sum())
  e, o = e[e > 0], o[e > 0]
  g = 2.0 * np.sum(np.where(o > 0, o * np.log(np.where(o > 0, o, 1.0) / e), 0.0))
  return float(stats.chi2.sf(g, max(1, e.size - 1)))


def _dense_case(n, rows, seed):
  rng = np.random.default_rng(seed)
  n_params = 4
  kinds = [E.GATE_XPOW, E.GATE_YPOW, E.GATE_ZPOW, E.GATE_HPOW] if n == 1 else None
  gates = random_circuit(rng, n, max(6, 3 * n), n_params, kinds)
  params = rng.uniform(-1, 1, n_params).astype(np.float32)
  bits = rng.integers(0, 2, size=(rows, n)).astype(np.int8)
  refs = [Ref.dense(np.abs(O.simulate(n, gates, params, list(b)).ravel())**2) for b in bits]
  return gates, n_params, params, bits, refs


def _ghz(n):
  return [(E.GATE_HPOW, 0, -1, -1, 0.0, 1.0)] + [(E.GATE_CNOTPOW, q, q + 1, -1, 0.0, 1.0) for q in range(n - 1)]


def _interleaved_product(n, seed):
  """Gates only on the pairs (j, n-1-j): the exact fp64 distribution is a product over the pairs."""
  rng = np.random.default_rng(seed)
  gates, p = [], np.ones((2,) * n)
  for j in range(n // 2):
    t = rng.uniform(-1, 1, 3)
    pair = [(E.GATE_YPOW, 0, -1, -1, 0.0, t[0]), (E.GATE_CNOTPOW, 0, 1, -1, 0.0, 1.0),
            (E.GATE_XPOW, 1, -1, -1, 0.0, t[1]), (E.GATE_XXPOW, 0, 1, -1, 0.0, t[2])]
    pp = np.abs(O.simulate(2, pair, [], [0, 0]))**2
    shape = [1] * n
    shape[j] = shape[n - 1 - j] = 2
    p = p * pp.reshape(shape)
    remap = {0: j, 1: n - 1 - j}
    gates += [(g[0], remap[g[1]], remap.get(g[2], -1), g[3], g[4], g[5]) for g in pair]
  return gates, p.ravel()


def _sample_and_check(eng, bits, params, refs, n_shots, dense=False):
  psi = eng.statevector(bits, params)
  deltas = [_delta(psi[r], refs[r]) for r in range(len(refs))]
  gpu_refs = [_gpu_ref(psi[r]) if eng.n_qubits <= 24 else None for r in range(len(refs))]
  out = eng.sample(bits, params, n_shots, seed=SEED).cpu().numpy()
  assert out.shape == (bits.shape[0], n_shots, eng.n_qubits)
  for r, ref in enumerate(refs):
    idx = _index(out[r])
    _check_shots(idx, ref, deltas[r], r, gpu_ref=gpu_refs[r])
    if dense and n_shots >= 65536:
      assert _g_test(np.bincount(idx, minlength=1 << eng.n_qubits), ref) >= 1e-6


@pytest.mark.parametrize("n,shots,opts", [
    (1, 65536 + 3, {}), (3, 1, {}), (9, 65535, {}), (10, 65536 + 3, {}), (11, 65536 + 3, {"chunk_states": 1}),
    (13, 2**20, {"tile_qubits": 10}), (16, 65536 + 3, {}), (20, 65536 + 3, {})])
def test_sample_dense_shot_for_shot(n, shots, opts):
  gates, n_params, params, bits, refs = _dense_case(n, 3 if "chunk_states" in opts else 2, seed=n)
  _sample_and_check(_engine(n, gates, n_params, **opts), bits, params, refs, shots, dense=True)


@pytest.mark.parametrize("n", [11, 24, 26])
def test_sample_ghz_and_basis_states(n):
  """GHZ: two outcomes, every block between them without mass.  Basis states: |1...1> (the last amplitude of the last
  block) and a random one -- every shot is that outcome."""
  half = Ref(np.array([0, (1 << n) - 1]), np.array([0.5, 0.5]))
  _sample_and_check(_engine(n, _ghz(n), 0), np.zeros((1, n), np.int8), np.zeros(0, np.float32), [half], 65536 + 3)
  rng = np.random.default_rng(n)
  bits = np.stack([np.ones(n, np.int8), rng.integers(0, 2, n).astype(np.int8)])
  eng = _engine(n, [(E.GATE_I, 0, -1, -1, 0.0, 1.0)], 0)
  out = eng.sample(bits, np.zeros(0, np.float32), 4099, seed=SEED).cpu().numpy()
  assert (out == bits[:, None, :]).all()


def test_sample_interleaved_block_product_24():
  n = 24
  gates, p = _interleaved_product(n, seed=3)
  _sample_and_check(_engine(n, gates, 0), np.zeros((1, n), np.int8), np.zeros(0, np.float32), [Ref.dense(p)],
                    65536 + 3)


def test_sample_tiny_probability_beside_exact_zeros():
  n, t = 16, 1e-3
  gates = [(E.GATE_XPOW, 5, -1, -1, 0.0, t)]
  p1 = float(np.abs(O.simulate(1, [(E.GATE_XPOW, 0, -1, -1, 0.0, t)], [], [0]).ravel()[1])**2)
  ref = Ref(np.array([0, 1 << (n - 1 - 5)]), np.array([1.0 - p1, p1]))
  eng = _engine(n, gates, 0)
  psi = eng.statevector(np.zeros((1, n), np.int8), np.zeros(0, np.float32))
  out = eng.sample(np.zeros((1, n), np.int8), np.zeros(0, np.float32), 2**20, seed=SEED).cpu().numpy()
  _check_shots(_index(out[0]), ref, _delta(psi[0], ref), 0, gpu_ref=_gpu_ref(psi[0]))


def _counts_and_check(eng, bits, params, refs, n_shots, n_programs=1):
  psi = eng.statevector(bits, params)
  deltas = [_delta(psi[r], refs[r]) for r in range(len(refs))]
  got = eng.sample_counts(bits, params, n_shots, seed=SEED, shift_gates=[-1] * n_programs,
                          shifts=[0.0] * n_programs).cpu().numpy()
  dim = 1 << eng.n_qubits
  assert got.shape == (n_programs, bits.shape[0], dim)
  for q in range(n_programs):
    for r, ref in enumerate(refs):
      want, ambiguous = _restated_counts(ref, n_shots, r, q, deltas[r], dim)
      assert got[q, r].sum() == n_shots
      assert not got[q, r][np.setdiff1d(np.arange(dim), ref.support)].any()  # no zero-probability outcome
      off = int(np.abs(got[q, r].astype(np.int64) - want).sum())
      assert off <= 2 * ambiguous, (q, r, off, ambiguous, deltas[r])
      # on the engine's own probabilities: a moved shot counts twice, at most 10^-3 of the shots may move
      own, _ = _restated_counts(_gpu_ref(psi[r]), n_shots, r, q, 0.0, dim)
      assert np.abs(got[q, r].astype(np.int64) - own).sum() <= 2e-3 * n_shots, (q, r)


@pytest.mark.parametrize("n,shots,opts,programs", [
    (1, 65536 + 3, {}, 1), (3, 65535, {"chunk_states": 1}, 3), (9, 2**20, {}, 1), (10, 1, {}, 2),
    (11, 65536 + 3, {"chunk_states": 1}, 3), (13, 65536 + 3, {"tile_qubits": 10}, 1), (16, 2**20, {}, 1),
    (20, 65536 + 3, {}, 1)])
def test_sample_counts_dense_shot_for_shot(n, shots, opts, programs):
  gates, n_params, params, bits, refs = _dense_case(n, 2, seed=100 + n)
  _counts_and_check(_engine(n, gates, n_params, **opts), bits, params, refs, shots, programs)


def test_sample_counts_block_product_and_ghz_24():
  n = 24
  gates, p = _interleaved_product(n, seed=4)
  _counts_and_check(_engine(n, gates, 0), np.zeros((1, n), np.int8), np.zeros(0, np.float32), [Ref.dense(p)],
                    65536 + 3)
  half = Ref(np.array([0, (1 << n) - 1]), np.array([0.5, 0.5]))
  _counts_and_check(_engine(n, _ghz(n), 0), np.zeros((1, n), np.int8), np.zeros(0, np.float32), [half], 65536 + 3)
