"""qhbm_sample_parities / qhbm_sample_parities_states without a device: the symbols, every refusal with its message, the
scratch size, the mirror's switch -- and a self-check of the reference the exact GPU test relies on: on dyadic states a
two-level sampler that adds in other orders (a pairwise tree for the block masses, Hillis-Steele scans for the prefixes)
draws exactly the outcomes of the flat definition."""
import ctypes

import numpy as np
import pytest

from oracle import sampling as S
from qhbmlib_amd import _engine as E
from qhbmlib_amd import inference, ir, models
from tests import sample_parity_ref as R

SEED = 0x9E3779B97F4A7C15


def _err(lib):
  return lib.qhbm_last_error(None).decode()


def test_symbols_are_exported_and_listed():
  lib = E.load_library()
  for name in ("qhbm_sample_parities", "qhbm_sample_parities_scratch_bytes", "qhbm_sample_parities_states"):
    assert name in E.ABI_SYMBOLS
    getattr(lib, name)
  assert lib.qhbm_abi_version() == 5


def test_scratch_bytes_answers():
  # 4096 bytes of masks + per state 2^(n-10) block prefixes and 2^(n-4) sub-block prefixes of 8 bytes
  assert E.sample_parities_scratch_bytes(1, 1, 10) == 4096 + 8 * 2
  assert E.sample_parities_scratch_bytes(3, 10, 0) == 4096 + 3 * 8 * (1 + 64)
  assert E.sample_parities_scratch_bytes(2, 20, 10**6) == 4096 + 2 * 8 * (1024 + 65536)
  assert E.sample_parities_scratch_bytes(1, 31, 2**31 - 1) == 4096 + 8 * (2**21 + 2**27)
  assert E.sample_parities_scratch_bytes(70000, 12, 5) == 4096 + 65535 * 8 * (4 + 256)   # slices of 65535 share it
  lib = E.load_library()
  out = ctypes.c_size_t()
  for args, message in (((0, 5, 1), "M"), ((1, 0, 1), "[1, 31]"), ((1, 32, 1), "[1, 31]"), ((1, 5, -1), "negative"),
                        ((1, 5, 2**31), "too many shots")):
    assert lib.qhbm_sample_parities_scratch_bytes(*args, ctypes.byref(out)) != 0
    assert message in _err(lib), (args, _err(lib))
  assert lib.qhbm_sample_parities_scratch_bytes(1, 5, 1, None) != 0 and "NULL" in _err(lib)


def _states_call(lib, **change):
  """A call with non-NULL aligned fake pointers: every refusal comes before anything touches them."""
  a = dict(d_states=4096, M=2, n=5, masks=np.array([0, 31, 5], np.uint64), T=3, shots=100, seed=1, first_row=0, program=0,
           d_scratch=8192, d_out=12288)
  a.update(change)
  masks = a["masks"]
  return lib.qhbm_sample_parities_states(a["d_states"], a["M"], a["n"], None if masks is None else masks.ctypes.data, a["T"],
                                         a["shots"], a["seed"], a["first_row"], a["program"], a["d_scratch"], a["d_out"], None)


@pytest.mark.parametrize("change,message", [
    (dict(M=0), "M (the number of states) must be positive"), (dict(M=-3), "must be positive"),
    (dict(n=0), "n_qubits must be in [1, 31]"), (dict(n=32), "n_qubits must be in [1, 31]"),
    (dict(T=0), "[1, 1024]"), (dict(T=1025, masks=np.zeros(1025, np.uint64)), "[1, 1024]"),
    (dict(shots=-1), "negative shot count"), (dict(shots=2**31), "too many shots"),
    (dict(masks=None), "masks is NULL"), (dict(d_states=None), "d_states is NULL"), (dict(d_scratch=None), "d_scratch is NULL"),
    (dict(d_out=None), "d_out is NULL"), (dict(d_states=4096 + 8), "d_states must be 16-byte aligned"),
    (dict(d_scratch=8192 + 4), "d_scratch must be 8-byte aligned"), (dict(d_out=12288 + 2), "d_out must be 4-byte aligned"),
    (dict(masks=np.array([0, 32, 5], np.uint64)), "masks[1] has a bit at or above n_qubits = 5"),
    (dict(masks=np.array([0, 1, 1 << 63], np.uint64)), "masks[2] has a bit at or above n_qubits"),
    (dict(first_row=2**32 - 1), "first_row + M exceeds 2^32"),
])
def test_states_entry_refusals(change, message):
  lib = E.load_library()
  assert _states_call(lib, **change) != 0
  assert message in _err(lib), (change, _err(lib))


def _planner():
  eng = E.Engine(None)
  # (kind, q0, q1, param_idx, scalar, offset): gate 0 is parametrised, gate 1 has a constant exponent
  eng.set_circuit(4, [(E.GATE_XPOW, 0, -1, 0, 1.0, 0.0), (E.GATE_XPOW, 1, -1, -1, 0.0, 0.25)], 1)
  return eng


def _engine_call(eng, **change):
  a = dict(U=2, gates=[-1, 0], shifts=[0.0, 0.5], masks=np.array([0, 15], np.uint64), T=2, shots=100, d_out=4096)
  a.update(change)
  sg, sv = np.asarray(a["gates"], np.int32), np.asarray(a["shifts"], np.float32)
  masks = a["masks"]
  rc = eng._lib.qhbm_sample_parities(eng._h, 4096, a["U"], 4096, len(sg), sg.ctypes.data, sv.ctypes.data,
                                     None if masks is None else masks.ctypes.data, a["T"], a["shots"], 1, a["d_out"], None)
  return rc, eng._lib.qhbm_last_error(eng._h).decode()


@pytest.mark.parametrize("change,message", [
    (dict(U=-1), "negative batch size"), (dict(T=0), "[1, 1024]"), (dict(T=1025, masks=np.zeros(1025, np.uint64)), "[1, 1024]"),
    (dict(shots=-5), "negative shot count"), (dict(shots=2**31), "too many shots"), (dict(masks=None), "masks is NULL"),
    (dict(masks=np.array([0, 16], np.uint64)), "masks[1] has a bit at or above n_qubits = 4"),
    (dict(gates=[-1, 2]), "shift_gates entry out of range"),
    (dict(gates=[-1, 1]), "constant exponent"), (dict(d_out=None), "d_out is NULL"),
    (dict(), "without a device"),   # a valid call gets as far as asking for the GPU
])
def test_engine_entry_refusals(change, message):
  rc, err = _engine_call(_planner(), **change)
  assert rc != 0 and message in err, (change, err)


def test_mirror_switch():
  qubits = ir.GridQubit.rect(1, 2)
  circ = models.DirectQuantumCircuit(ir.Circuit(ir.X(q)**ir.Symbol("p") for q in qubits))
  assert inference.SampledQuantumInference(circ, 10)._pauli_route == "outcomes"
  assert inference.SampledQuantumInference(circ, 10, pauli_estimator="parities")._pauli_route == "parities"
  with pytest.raises(ValueError, match="pauli_estimator"):
    inference.SampledQuantumInference(circ, 10, pauli_estimator="bogus")


# ---- the reference's self-check ----

def _pairwise(x):
  """Sum over the last axis in a balanced tree."""
  while x.shape[-1] > 1:
    x = x[..., 0::2] + x[..., 1::2]
  return x[..., 0]


def _hillis_steele(x):
  """Inclusive prefix over the last axis, offsets 1, 2, 4, ..."""
  x = x.copy()
  k = 1
  while k < x.shape[-1]:
    y = x.copy()
    y[..., k:] += x[..., :-k]
    x, k = y, 2 * k
  return x


def _two_level_outcomes(p, u, block):
  """The outcomes of a two-level sampler: blocks of `block` masses added in a pairwise tree, both prefixes by
  Hillis-Steele scans, the remainder r = u * total - (prefix of the blocks before) searched inside the block."""
  rows = p.reshape(-1, block)
  block_cum = _hillis_steele(_pairwise(rows))
  inner = _hillis_steele(rows)
  v = u * block_cum[-1]
  b = np.minimum(np.searchsorted(block_cum, v, side="right"), len(block_cum) - 1)
  r = v - np.where(b > 0, block_cum[np.maximum(b - 1, 0)], 0.0)
  lo, hi = np.zeros(len(u), np.int64), np.full(len(u), block - 1, np.int64)
  while (lo < hi).any():
    mid = (lo + hi) // 2
    up = inner[b, mid] > r
    hi = np.where(up, mid, hi)
    lo = np.where(up, lo, np.minimum(mid + 1, hi))
  return np.minimum(b * block + lo, np.flatnonzero(p > 0)[-1])


@pytest.mark.parametrize("n,shots", [(3, 4099), (10, 65539), (11, 65539), (16, 65539), (20, 2**18)])
def test_dyadic_states_draw_the_same_outcomes_in_every_order(n, shots):
  rng = np.random.default_rng(n)
  p = R.masses(R.dyadic_states(rng, 1, n))[0]
  assert (p * 2.0**24 == np.round(p * 2.0**24)).all() and n + 24 <= 53
  flat = R.restated_outcomes(p, shots, 3, SEED, 1)
  assert (p[flat] > 0).all()
  two = _two_level_outcomes(p, S.engine_uniforms(shots, 3, SEED, 1), min(1024, 1 << n))
  assert (flat == two).all()
  assert len(np.unique(flat)) > 1 or n < 2


def test_restated_sums_edge_cases():
  masks = np.array([0, 1, 2, 3], np.uint64)
  # a basis state |10>: qubit 0 set, qubit 1 clear -> mask bit 0 flips the sign
  assert R.restated_sums([0, 0, 1, 0], masks, 1000, 0, SEED).tolist() == [1000, -1000, 1000, -1000]
  assert R.restated_sums([0, 0, 0, 0], masks, 1000, 0, SEED).tolist() == [0, 0, 0, 0]
  # the sparse form is the dense one
  p = np.zeros(64)
  p[[3, 17, 40]] = [0.25, 1.0, 0.0625]
  m = R.mask_set(np.random.default_rng(0), 6, 5)
  assert (R.restated_sums(p, m, 5000, 2, SEED, 1) ==
          R.restated_sums([0.25, 1.0, 0.0625], m, 5000, 2, SEED, 1, support=[3, 17, 40], n_qubits=6)).all()
