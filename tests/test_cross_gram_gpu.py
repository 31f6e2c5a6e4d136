"""The cross-Gram kernel (csrc/cross_gram.hip) and `inference.ensemble_metrics` / `matrix_elements` on the GPU.

1. `qhbm_cross_gram` through the C ABI, output and scratch pre-filled with NaN, against `tests/cross_gram_ref.cross_gram` on
   the same complex64 states.  Bound, per part, derived and not tuned (gram.hip's, tests/test_state_metrics_gpu.py): every
   product is exact in float64, each of the 2^(n+1) terms of a part meets one rounding per addition on its way through the
   thread's chain, the shuffle tree, the waves and the slices; the reference's own float64 sum is allowed as much:
   |dC| <= 4 (2^n + 4) 2^-53 sum_x |t(x)| |a_i(x)| |b_j(x)|.
2. Exact inputs come out exact: amplitudes whose parts are +-(a power of two) of modulus 2^(-n/2) -- real +-2^-5 at n = 10,
   (+-1 +- i) 2^-7 at n = 13, where 2^(-n/2) itself is no float -- make every product and every partial sum a small integer
   multiple of 2^-n (2^-(n+1)): the overlap count comes out with NO rounding, whatever the order.
3. With bras and kets the same buffer the kernel repeats `qhbm_weighted_gram`'s additions: equal bits on the strict upper
   triangle and the real diagonal.
4. An entry depends neither on M, nor on K, nor on its tile; two calls give the same bits; overlapping views of one buffer
   give the bits of separate copies.
5. Refusals launch nothing.
6. `ensemble_metrics` and `matrix_elements` against the same host formulas on the restatement's matrices, and one use at 20
   qubits.
Every comparison prints its largest error beside its bar before it asserts.
"""
import ctypes
import functools
import importlib

import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir
from tests import cross_gram_ref as X
from tests import state_metrics_ref as R
from tests import thermal_ref as T

EM = importlib.import_module("qhbmlib_amd.inference.ensemble_metrics")

pytestmark = pytest.mark.gpu

QUBITS = [1, 3, 10, 13]  # one 16-byte word; fewer words than threads; one slice; the first n with several slices
SHAPES = [(1, 1), (4, 4), (5, 3), (3, 5), (9, 2), (2, 9), (6, 7)]  # every <TI, TJ> with TI, TJ in 1..4 runs
TABLES = ["none", "signed"]


def _raw_cross(bras, num_a, kets, num_b, n, table=None):
  """qhbm_cross_gram through the C ABI on NaN-filled scratch and output: complex128 numpy [M, K].  `bras` / `kets`:
  tensors or raw device addresses."""
  lib = E.load_library()
  scratch = torch.full((E.cross_gram_scratch_bytes(num_a, num_b, n) // 8,), float("nan"), dtype=torch.float64, device="cuda")
  out = torch.full((num_a, num_b, 2), float("nan"), dtype=torch.float64, device="cuda")
  ptr = lambda t: t.data_ptr() if torch.is_tensor(t) else int(t)
  rc = lib.qhbm_cross_gram(ptr(bras), num_a, ptr(kets), num_b, n, None if table is None else table.data_ptr(), scratch.data_ptr(),
                           out.data_ptr(), torch.cuda.current_stream().cuda_stream)
  assert rc == 0, lib.qhbm_last_error(None).decode()
  got = out.cpu().numpy()
  return got[..., 0] + 1j * got[..., 1]


@functools.lru_cache(maxsize=None)
def _case(n, num_a, num_b):
  """(complex64 bras, complex64 kets, {table name: float32 table or None}) as numpy, one draw per shape."""
  rng = np.random.default_rng(1000 * n + 10 * num_a + num_b)
  dim = 1 << n
  draw = lambda num: ((rng.normal(size=(num, dim)) + 1j * rng.normal(size=(num, dim))) / np.sqrt(2 * dim)).astype(np.complex64)
  bras, kets = draw(num_a), draw(num_b)
  sign = rng.choice([-1.0, 1.0], dim)
  sign[0], sign[-1] = 1.0, -1.0   # (both signs at n = 1 too)
  signed = (sign * np.abs(rng.normal(size=dim)) * 10.0**rng.uniform(-3, 3, dim)).astype(np.float32)  # magnitudes << 1 and >> 1
  return bras, kets, {"none": None, "signed": signed}


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(a, b):
  return np.array_equal(_bits(a.real), _bits(b.real)) and np.array_equal(_bits(a.imag), _bits(b.imag))


def _kernel_bound(n, bras, kets, table=None):
  return 4.0 * ((1 << n) + 4) * X.EPS * X.cross_gram_bound(bras, kets, table)


# ---- 1. the kernel against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("num_a,num_b", SHAPES)
@pytest.mark.parametrize("n", QUBITS)
def test_cross_gram_kernel_matches_the_float64_restatement(n, num_a, num_b, table):
  bras, kets, tables = _case(n, num_a, num_b)
  t = tables[table]
  d_bras, d_kets = torch.from_numpy(bras).cuda(), torch.from_numpy(kets).cuda()
  d_table = None if t is None else torch.from_numpy(t).cuda()
  got = _raw_cross(d_bras, num_a, d_kets, num_b, n, d_table)
  want = X.cross_gram(bras, kets, t)
  bound = _kernel_bound(n, bras, kets, t)
  err_re, err_im = np.abs(got.real - want.real), np.abs(got.imag - want.imag)
  print(f"n={n} M={num_a} K={num_b} {table}: worst re {np.max(err_re / bound):.3g} im {np.max(err_im / bound):.3g} of the bound")
  assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag))
  assert np.all(err_re <= bound) and np.all(err_im <= bound)
  # the binding: same kernel, its own scratch
  bound_call = E.cross_gram(d_bras, d_kets, d_table)
  assert bound_call.dtype == torch.complex128 and tuple(bound_call.shape) == (num_a, num_b)
  assert _same_bits(bound_call.cpu().numpy(), got)
  assert inference.cross_gram is E.cross_gram


# ---- 2. exact inputs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [10, 13])
def test_random_sign_states_give_the_overlap_count_exactly(n):
  rng = np.random.default_rng(n)
  dim, num_a, num_b = 1 << n, 5, 3
  signs = lambda num: rng.integers(0, 2, size=(num, dim)) * 2 - 1
  if n % 2 == 0:   # +-2^(-n/2), real
    unit, scale = 2.0**-(n // 2), float(dim)
    int_a, int_b = signs(num_a).astype(np.complex128), signs(num_b).astype(np.complex128)
  else:            # (+-1 +- i) 2^(-(n+1)/2): modulus 2^(-n/2), both parts powers of two
    unit, scale = 2.0**-((n + 1) // 2), float(2 * dim)
    int_a, int_b = signs(num_a) + 1j * signs(num_a), signs(num_b) + 1j * signs(num_b)
  bras, kets = (int_a * unit).astype(np.complex64), (int_b * unit).astype(np.complex64)
  np.testing.assert_allclose(np.abs(bras), 2.0**(-n / 2), rtol=1e-7, atol=0)   # (the modulus of every amplitude)
  count = int_a.conj() @ int_b.T   # Gaussian integers, exact in float64
  assert np.all(count.real == np.round(count.real)) and np.abs(count).max() > 0
  got = _raw_cross(torch.from_numpy(bras).cuda(), num_a, torch.from_numpy(kets).cuda(), num_b, n)
  print(f"n={n}: counts {count[0].tolist()} got * {scale:g} = {(got[0] * scale).tolist()}")
  assert np.array_equal(got.real * scale, count.real) and np.array_equal(got.imag * scale, count.imag)


# ---- 3. equality with qhbm_weighted_gram ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("n", [3, 10, 13])
def test_same_buffer_repeats_the_weighted_gram_bit_for_bit(n, table):
  num = 6
  states, _, tables = _case(n, num, num)
  t = tables[table]
  d_states = torch.from_numpy(states).cuda()
  d_table = None if t is None else torch.from_numpy(t).cuda()
  gram = E.weighted_gram(d_states, d_table)
  cross = torch.from_numpy(_raw_cross(d_states, num, d_states, num, n, d_table)).cuda()
  upper = torch.triu(torch.ones((num, num), dtype=torch.bool, device="cuda"), diagonal=1)
  assert torch.equal(cross.real[upper], gram.real[upper]) and torch.equal(cross.imag[upper], gram.imag[upper])
  assert torch.equal(cross.real.diagonal(), gram.real.diagonal())
  # what is NOT promised bit for bit: Im C[i, i] and the lower triangle, within the bound of 0 and of G's mirrored conj
  bound = torch.from_numpy(0.5 * _kernel_bound(n, states, states, t)).cuda()   # (the kernel's own: 2 (2^n + 4) 2^-53 sum; two kernel results differ by twice that)
  assert torch.all(cross.imag.diagonal().abs() <= bound.diagonal())
  lower = upper.transpose(0, 1)
  assert torch.all((cross - gram)[lower].real.abs() <= 2 * bound[lower])   # (G[j, i] is the mirrored conj(G[i, j]))
  assert torch.all((cross - gram)[lower].imag.abs() <= 2 * bound[lower])
  print(f"n={n} {table}: largest |Im C[i, i]| {float(cross.imag.diagonal().abs().max()):.3e}")


# ---- 4. independence ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("n", [10, 13])
def test_an_entry_does_not_depend_on_the_company_it_keeps(n, table):
  num_a, num_b = 5, 3
  bras, kets, tables = _case(n, num_a, num_b)
  t = tables[table]
  d_bras, d_kets = torch.from_numpy(bras).cuda(), torch.from_numpy(kets).cuda()
  d_table = None if t is None else torch.from_numpy(t).cuda()
  full = _raw_cross(d_bras, num_a, d_kets, num_b, n, d_table)
  again = _raw_cross(d_bras, num_a, d_kets, num_b, n, d_table)
  assert _same_bits(full, again)
  for i in range(num_a):
    for j in range(num_b):
      pair = _raw_cross(d_bras[i:i + 1], 1, d_kets[j:j + 1], 1, n, d_table)   # a <1, 1> tile of its own
      assert _same_bits(pair[0, 0], full[i, j]), (i, j)
  # the same pairs inside a (9, 7) call, where they fall into other tiles (<4, 4>, <4, 3>, <1, 4>, <1, 3>)
  wide_a, wide_b = np.concatenate([bras[:4], bras]), np.concatenate([kets[2:], kets[:2], kets, kets[:1]])
  wide = _raw_cross(torch.from_numpy(wide_a).cuda(), 9, torch.from_numpy(wide_b).cuda(), 7, n, d_table)
  assert _same_bits(wide[4:9, 3:6], full)


@pytest.mark.parametrize("n", [3, 13])
def test_overlapping_views_of_one_buffer_give_the_bits_of_separate_copies(n):
  states, _, tables = _case(n, 6, 6)
  buffer = torch.from_numpy(states).cuda()
  d_table = torch.from_numpy(tables["signed"]).cuda()
  bras, kets = buffer[0:5], buffer[2:6]   # rows 2, 3 and 4 belong to both
  assert bras.data_ptr() < kets.data_ptr() < bras.data_ptr() + bras.numel() * 8
  shared = _raw_cross(bras, 5, kets, 4, n, d_table)
  apart = _raw_cross(bras.clone(), 5, kets.clone(), 4, n, d_table)
  assert _same_bits(shared, apart)
  assert torch.equal(torch.view_as_real(buffer), torch.view_as_real(torch.from_numpy(states).cuda()))   # only read
  assert _same_bits(E.cross_gram(bras, kets, d_table).cpu().numpy(), shared)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refused_arguments_return_a_status_and_launch_nothing():
  lib = E.load_library()
  bras = torch.ones((4, 64), dtype=torch.complex64, device="cuda")
  kets = torch.ones((3, 64), dtype=torch.complex64, device="cuda")
  table = torch.ones(66, dtype=torch.float32, device="cuda")
  scratch = torch.full((E.cross_gram_scratch_bytes(4, 3, 6) // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")
  out = torch.full((4 * 3 * 2 + 1,), float("nan"), dtype=torch.float64, device="cuda")
  stream = torch.cuda.current_stream().cuda_stream
  good = dict(a=bras.data_ptr(), m=4, b=kets.data_ptr(), k=3, n=6, t=table.data_ptr(), w=scratch.data_ptr(), o=out.data_ptr())
  refused = [dict(m=0), dict(m=-1), dict(m=1025), dict(k=0), dict(k=-1), dict(k=1025), dict(n=0), dict(n=32), dict(a=None),
             dict(b=None), dict(w=None), dict(o=None), dict(a=bras.data_ptr() + 8), dict(b=kets.data_ptr() + 8),
             dict(t=table.data_ptr() + 4), dict(w=scratch.data_ptr() + 4), dict(o=out.data_ptr() + 4)]
  for change in refused:
    c = dict(good, **change)
    rc = lib.qhbm_cross_gram(c["a"], c["m"], c["b"], c["k"], c["n"], c["t"], c["w"], c["o"], stream)
    assert rc != 0, change
    assert lib.qhbm_last_error(None).decode()
  size = ctypes.c_size_t()
  for m, k, n in [(0, 3, 6), (1025, 3, 6), (4, 0, 6), (4, 1025, 6), (4, 3, 0), (4, 3, 32)]:
    assert lib.qhbm_cross_gram_scratch_bytes(m, k, n, ctypes.byref(size)) != 0
  assert lib.qhbm_cross_gram_scratch_bytes(4, 3, 6, None) != 0
  torch.cuda.synchronize()
  assert torch.all(torch.isnan(out)) and torch.all(torch.isnan(scratch))
  with pytest.raises(E.EngineError):
    E.cross_gram(bras.cpu(), kets)
  with pytest.raises(ValueError):
    E.cross_gram(bras, kets[:, :32])      # 64 amplitudes against 32
  with pytest.raises(ValueError):
    E.cross_gram(bras, kets, table)       # 66 entries for 64 amplitudes


# ---- 6. the mirror -----------------------------------------------------------------------------------------------------------
def _ensembles(n, num_a, num_b, seed):
  """Two random weighted ensembles, neither orthogonal nor normalised: complex64 states, float64 weights (numpy)."""
  rng = np.random.default_rng(seed)
  dim = 1 << n
  draw = lambda num: (rng.normal(size=(num, dim)) + 1j * rng.normal(size=(num, dim))) / np.sqrt(2 * dim)
  a = (draw(num_a) * rng.uniform(0.5, 1.5, (num_a, 1))).astype(np.complex64)
  b = (0.6 * draw(num_b) + 0.8 * draw(num_b)[:1] + 0.5 * a[:num_b].astype(np.complex128)).astype(np.complex64)  # (not orthogonal to a)
  return a, rng.uniform(0.1, 0.4, num_a), b, rng.uniform(0.1, 0.4, num_b)


def _nuclear_bar(n, a, w, b, v):
  """min(M, K) ||bound||_F: the kernel's and the restatement's bound on C (both parts: sqrt 2), scaled into X = W^1/2 C V^1/2;
  by Weyl's inequality no singular value of X moves by more than ||dX||_2 <= ||dX||_F, and there are min(M, K) of them."""
  scaled = np.sqrt(2.0) * np.sqrt(np.outer(w, v)) * _kernel_bound(n, a, b)
  return min(len(w), len(v)) * float(np.linalg.norm(scaled))


def test_ensemble_metrics_mirror_the_host_formulas_on_the_restatement():
  n, num_a, num_b = 10, 5, 3
  a, w, b, v = _ensembles(n, num_a, num_b, 77)
  got = inference.ensemble_metrics((torch.from_numpy(a), torch.from_numpy(w)), (torch.from_numpy(b), torch.from_numpy(v)))
  want = EM.metrics_from_grams(R.gram(a), R.gram(b), X.cross_gram(a, b), w, v)
  assert isinstance(got, inference.EnsembleMetrics) and all(isinstance(x, float) for x in (got.fidelity, got.overlap, got.trace_distance))
  delta = _nuclear_bar(n, a, w, b, v)
  bar_fidelity = (2 * np.sqrt(want.fidelity) + delta) * delta
  bar_overlap = (2 * np.sqrt(want.overlap) + delta) * delta
  print(f"fidelity {got.fidelity:.12g} ({abs(got.fidelity - want.fidelity):.2e}, bar {bar_fidelity:.2e}) overlap {got.overlap:.12g} "
        f"({abs(got.overlap - want.overlap):.2e}, bar {bar_overlap:.2e}) distance {got.trace_distance:.12g} "
        f"({abs(got.trace_distance - want.trace_distance):.2e}) traces {got.trace_a:.6g} {got.trace_b:.6g}")
  assert want.fidelity > 1e-3 and want.overlap > 1e-4
  assert abs(got.fidelity - want.fidelity) <= bar_fidelity
  assert abs(got.overlap - want.overlap) <= bar_overlap
  # the same through StateVectorData, its thin calls included
  source_a = data.StateVectorData(torch.from_numpy(a), torch.from_numpy(w))
  source_b = data.StateVectorData(torch.from_numpy(b), torch.from_numpy(v))
  assert inference.ensemble_metrics(source_a, source_b) == got
  assert source_a.fidelity_to(source_b) == got.fidelity and source_a.trace_distance_to(source_b) == got.trace_distance
  with pytest.raises(ValueError, match="qubits"):
    inference.ensemble_metrics(source_a, (torch.from_numpy(b[:, :512]), None))
  named = data.StateVectorData(torch.from_numpy(b), torch.from_numpy(v), qubits=[ir.GridQubit(1, c) for c in range(n)])
  elsewhere = data.StateVectorData(torch.from_numpy(a), torch.from_numpy(w), qubits=[ir.GridQubit(2, c) for c in range(n)])
  with pytest.raises(ValueError, match="qubits"):
    inference.ensemble_metrics(elsewhere, named)


def test_an_ensemble_has_fidelity_trace_squared_to_itself():
  n, num = 10, 5
  a, w, _, _ = _ensembles(n, num, 3, 78)
  pair = (torch.from_numpy(a), torch.from_numpy(w))
  got = inference.ensemble_metrics(pair, pair)
  delta = _nuclear_bar(n, a, w, a, w)
  bar = (2 * got.trace_a + delta) * delta
  print(f"fidelity {got.fidelity:.15g} trace^2 {got.trace_a**2:.15g} ({abs(got.fidelity - got.trace_a**2):.2e}, bar {bar:.2e}) "
        f"distance {got.trace_distance:.3e}")
  assert got.trace_a == got.trace_b and got.purity_a == got.purity_b
  assert abs(got.fidelity - got.trace_a**2) <= bar


def test_matrix_elements_of_a_pauli_sum_match_the_restatement():
  n, num_a, num_b = 10, 3, 2
  qubits = ir.GridQubit.rect(1, n)
  op = ir.as_pauli_sum(0.7 * ir.PX(qubits[0]) * ir.PX(qubits[1]) + (-0.4) * ir.PY(qubits[2]) * ir.PZ(qubits[5]) + 1.1 * ir.PZ(qubits[9]))
  assert len(op.terms) == 3
  masks = [list(op.masks(qubits))]
  bras, kets, _ = _case(n, num_a, num_b)
  got = inference.matrix_elements([op], torch.from_numpy(bras), torch.from_numpy(kets), qubits=qubits).cpu().numpy()
  applied = T.apply_h(n, masks, kets.astype(np.complex128))
  want = X.cross_gram(bras, applied)
  # the kernel's bound on <a|(H b)> plus `qhbm_apply_observables`' own, tests/test_thermal_gpu.py: per amplitude
  # (T + 2) 2^-24 R max |b|, T = 3 terms, summed against |a|
  apply_bar = (3 + 2) * 2.0**-24 * T.radius(n, masks) * np.abs(kets).max(axis=1)
  bar = _kernel_bound(n, bras, applied) + np.abs(bras).astype(np.float64).sum(axis=1)[:, None] * apply_bar[None, :]
  err_re, err_im = np.abs(got.real - want.real), np.abs(got.imag - want.imag)
  print(f"matrix elements: largest |want| {np.abs(want).max():.3e} worst re {np.max(err_re / bar):.3g} im {np.max(err_im / bar):.3g} of the bar")
  assert got.dtype == np.complex128 and got.shape == (num_a, num_b) and np.abs(want).max() > 1e-3
  assert np.all(err_re <= bar) and np.all(err_im <= bar)


def test_chebyshev_and_krylov_thermal_ensembles_at_twenty_qubits():
  """rho_beta of the 57-term XXZ chain from the same two start states by the Chebyshev evolution and by the Krylov space:
  the fidelity of one to the other over the product of their traces is reported and is at most 1.  Nothing tighter is
  asserted: how well the two evolutions agree has not been measured before (scripts/cross_gram_time.py records the value in
  profiles/cross_gram.json)."""
  n, beta = 20, 0.5
  qubits = ir.GridQubit.rect(1, n)
  xxz = ir.PauliSum()
  for a, b in zip(qubits[:-1], qubits[1:]):
    xxz += ir.PX(a) * ir.PX(b) + ir.PY(a) * ir.PY(b) + 0.5 * ir.PZ(a) * ir.PZ(b)
  assert len(xxz.terms) == 57
  chebyshev = inference.thermal_ensemble([xxz], beta, num_vectors=2, seed=5)
  krylov = inference.thermal_sweep([xxz], [beta], num_vectors=2, num_steps=24, seed=5).ensemble(beta)
  got = inference.ensemble_metrics(chebyshev, krylov)
  ratio = got.fidelity / (got.trace_a * got.trace_b)
  print(f"n=20 beta={beta}: fidelity / (tr tr) = {ratio!r} (1 - it: {1 - ratio:.3e}) trace distance {got.trace_distance:.3e} {got}")
  assert ratio <= 1 + 1e-9
