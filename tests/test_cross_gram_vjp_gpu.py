"""`qhbm_cross_gram_vjp` (csrc/cross_gram_vjp.hip) and `ensemble_metrics(..., differentiable=True)` on the GPU,
against the complex128 restatement of tests/cross_gram_vjp_ref.py.

1. The kernels through the C ABI on the same complex64 / float32 inputs, every output and the scratch pre-filled with NaN.
   The bar needs no measurement.  A real or imaginary part of out_s(x) / t(x) = sum_r W[r, s] src_r(x) is a sum of N = 2 R
   real products (the real embedding Re = W_r s_r - W_i s_i, Im = W_r s_i + W_i s_r) made as an f32 fused-multiply-add chain:
   at most N roundings on the way of any product, each relative 2^-24 to a partial sum no larger than
   T_s = sum_r (|Re W_rs| + |Im W_rs|) (|Re src_r| + |Im src_r|), then one more for the table; the second-order term
   N^2 2^-48 / 2 is below 2^-24 for N <= 2048.  So |out - want| <= (2 R + 4) 2^-24 |t(x)| T_s(x) per part in ANY summation
   order, asserted elementwise, R = M for the kets' output and K for the bras'; table_grad, summed exactly in float64 from
   the unscaled f32 c, is held to sum_j (2 M + 4) 2^-24 T_j(x) (|Re b_j| + |Im b_j|).
2. Exact cases: amplitudes (+-1 +- i) 2^-k, Gamma entries in {+-1, +-i}, a table of signed powers of two, at most 16 source
   rows: every partial sum is exact in float32, so the outputs equal the restatement bit for bit.
3. Independence: two calls, calls with outputs left out, single output rows, overlapping views of one buffer.
4. Bras and kets the same buffer against `qhbm_weighted_gram_vjp` with H = Gamma + Gamma^H.
5. Refusals leave outputs and scratch untouched.
6. The autograd node `inference.differentiable_cross_gram` and the mirror `ensemble_metrics(..., differentiable=True)` through
   `final_states_from_states`, against the restatement composed with `tests/final_states_ref.vjp` at the bar of DESIGN.md
   6l / 6n, 1e-4 max(1, ||grad||_inf); the weights' gradients at the float64 bar 1e-7 max(1, ||grad||_inf).
"""
import dataclasses
import functools
import importlib
import warnings

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir, models
from tests import cross_gram_ref as X
from tests import cross_gram_vjp_ref as V
from tests import final_states_ref as F
from tests import from_states_ref as S
from tests import state_metrics_vjp_ref as G
from tests.test_from_states_gpu import _close, _grad_bar
from tests.test_host_api import hea_circuit

pytestmark = pytest.mark.gpu

EM = importlib.import_module("qhbmlib_amd.inference.ensemble_metrics")

# 1: a single word; 5, 6, 7: either side of a 64-amplitude column tile; 10, 11, 12: below, at and above one 1024-word slice
WIDTHS = [1, 2, 5, 6, 7, 10, 11, 12, 13]
# both kernels on both sides (the switch is at 8 | 9 SOURCE rows), ragged stages, ragged and several row tiles
PAIRS = [(1, 1), (3, 5), (8, 9), (9, 8), (5, 17), (17, 5), (16, 16), (15, 33), (33, 15), (3, 65), (65, 3)]
WIDE = [(2, 1024), (1024, 2), (9, 1024), (1024, 9)]  # at n = 7: the W chunks of the vector kernel, sixteen row tiles
TABLES = ["none", "positive", "signed"]
METRICS = ("overlap", "fidelity", "trace_distance")


def _bits32(a):
  return np.ascontiguousarray(a).view(np.int64)


def _bits64(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _raw_vjp(bras, kets, table, gamma, want=(True, True, True)):
  """qhbm_cross_gram_vjp through the C ABI on NaN-filled outputs and scratch: (out_bras [M, 2^n], out_kets [K, 2^n] complex64,
  table_grad [2^n] float64) as numpy."""
  lib = E.load_library()
  num, dim = bras.shape
  num_kets = kets.shape[0]
  n = dim.bit_length() - 1
  nan = float("nan")
  scratch = torch.full((E.cross_gram_vjp_scratch_bytes(num, num_kets, n) // 8,), nan, dtype=torch.float64, device="cuda")
  out_bras = torch.full((num, dim), complex(nan, nan), dtype=torch.complex64, device="cuda")
  out_kets = torch.full((num_kets, dim), complex(nan, nan), dtype=torch.complex64, device="cuda")
  grad = torch.full((dim,), nan, dtype=torch.float64, device="cuda")
  rc = lib.qhbm_cross_gram_vjp(bras.data_ptr(), num, kets.data_ptr(), num_kets, n, None if table is None else table.data_ptr(),
                               gamma.data_ptr(), out_bras.data_ptr() if want[0] else None, out_kets.data_ptr() if want[1] else None,
                               grad.data_ptr() if want[2] else None, scratch.data_ptr(), torch.cuda.current_stream().cuda_stream)
  assert rc == 0, lib.qhbm_last_error(None).decode()
  return out_bras.cpu().numpy(), out_kets.cpu().numpy(), grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(n, num_a, num_b):
  """(complex64 bras, kets, a complex64 Gamma that is not Hermitian, with one zero row and one zero column, {table name:
  float32 table or None}): one draw per shape."""
  rng = np.random.default_rng(10000 * n + 10 * num_a + num_b)
  dim = 1 << n
  bras = ((rng.normal(size=(num_a, dim)) + 1j * rng.normal(size=(num_a, dim))) / np.sqrt(2 * dim)).astype(np.complex64)
  kets = ((rng.normal(size=(num_b, dim)) + 1j * rng.normal(size=(num_b, dim))) / np.sqrt(2 * dim)).astype(np.complex64)
  gamma = rng.normal(size=(num_a, num_b)) + 1j * rng.normal(size=(num_a, num_b))
  if num_a > 1:
    gamma[num_a // 2, :] = 0
  if num_b > 1:
    gamma[:, num_b // 2] = 0
  signed = rng.normal(size=dim) * 10.0**rng.uniform(-3, 3, dim)
  signed[rng.integers(0, dim, max(1, dim // 8))] = 0.0
  tables = {"none": None, "positive": rng.uniform(0.05, 1.0, dim).astype(np.float32), "signed": signed.astype(np.float32)}
  return bras, kets, gamma.astype(np.complex64), tables


def _device(bras, kets, gamma, t):
  return (torch.from_numpy(bras).cuda(), torch.from_numpy(kets).cuda(), None if t is None else torch.from_numpy(t).cuda(),
          torch.from_numpy(gamma).cuda())


def _hold_bound(label, got, want, bars, num_a, num_b):
  """The elementwise bound of this file's head; prints the worst fraction of it before it asserts."""
  eps_bras, eps_kets = (2.0 * num_b + 4.0) * 2.0**-24, (2.0 * num_a + 4.0) * 2.0**-24
  worst = []
  for out, expected, bar, eps in zip(got[:2], want[:2], bars[:2], (eps_bras, eps_kets)):
    err = np.maximum(np.abs(out.real - expected.real), np.abs(out.imag - expected.imag))
    live = bar > 0
    worst.append(float(np.max(err[live] / (eps * bar[live]))) if live.any() else 0.0)
    assert np.all(np.isfinite(out.real)) and np.all(np.isfinite(out.imag)), label
    assert np.all(err <= eps * bar), (label, worst)
  err = np.abs(got[2] - want[2])
  live = bars[2] > 0
  worst.append(float(np.max(err[live] / (eps_kets * bars[2][live]))) if live.any() else 0.0)
  print(f"{label}: worst out_bras {worst[0]:.3g} out_kets {worst[1]:.3g} table_grad {worst[2]:.3g} of the bound")
  assert np.all(np.isfinite(got[2])) and np.all(err <= eps_kets * bars[2]), (label, worst)


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("num_a,num_b", PAIRS)
@pytest.mark.parametrize("n", WIDTHS)
def test_kernel_matches_the_restatement(n, num_a, num_b, table):
  bras, kets, gamma, tables = _case(n, num_a, num_b)
  t = tables[table]
  got = _raw_vjp(*_device(bras, kets, gamma, t))
  _hold_bound(f"n={n} M={num_a} K={num_b} {table}", got, V.vjp(bras, kets, t, gamma), V.vjp_bounds(bras, kets, t, gamma), num_a, num_b)
  assert np.abs(got[0]).max() > 0 and np.abs(got[1]).max() > 0 and np.abs(got[2]).max() > 0


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("num_a,num_b", WIDE)
def test_kernel_matches_the_restatement_at_1024_states(num_a, num_b, table):
  n = 7
  bras, kets, gamma, tables = _case(n, num_a, num_b)
  t = tables[table]
  got = _raw_vjp(*_device(bras, kets, gamma, t))
  _hold_bound(f"n={n} M={num_a} K={num_b} {table}", got, V.vjp(bras, kets, t, gamma), V.vjp_bounds(bras, kets, t, gamma), num_a, num_b)


# ---- 2. exact cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,num_a,num_b", [(1, 1, 1), (6, 3, 5), (5, 16, 16), (7, 16, 9), (11, 8, 16), (12, 12, 7), (13, 9, 2)])
def test_exact_inputs_give_the_restatement_bit_for_bit(n, num_a, num_b):
  rng = np.random.default_rng(31 * n + num_a)
  dim, scale = 1 << n, 2.0**-((n + 1) // 2)
  draw = lambda rows: ((rng.choice([-1.0, 1.0], (rows, dim)) + 1j * rng.choice([-1.0, 1.0], (rows, dim))) * scale).astype(np.complex64)
  bras, kets = draw(num_a), draw(num_b)
  gamma = rng.choice(np.array([1, -1, 1j, -1j]), (num_a, num_b)).astype(np.complex64)
  t = (rng.choice([-1.0, 1.0], dim) * 2.0**rng.integers(-3, 4, dim)).astype(np.float32)
  for table in (None, t):
    got = _raw_vjp(*_device(bras, kets, gamma, table))
    want = V.vjp(bras, kets, table, gamma)
    # (equal as numbers, which for finite values is bit for bit but for the sign of a zero: a sum that cancels)
    assert np.array_equal(got[0].astype(np.complex128), want[0]) and np.array_equal(got[1].astype(np.complex128), want[1])
    assert np.array_equal(got[2], want[2])
    assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0 and np.abs(want[2]).max() > 0


def test_hand_checks_on_the_device():
  """M = K = 1: L = Re C gives gbar_b = t a, gbar_a = t b, tbar = Re(conj(a) b); L = Im C gives i t a and -i t b: one product
  each, so exactly."""
  bras, kets, _, tables = _case(10, 3, 5)
  t = tables["positive"]
  a, b = bras[:1].copy(), kets[:1].copy()
  for gamma, factor in ((1.0, 1.0), (1j, 1j)):
    got = _raw_vjp(*_device(a, b, np.full((1, 1), gamma, dtype=np.complex64), t))
    assert np.array_equal(got[1][0], (factor * a[0]).astype(np.complex64) * t)
    assert np.array_equal(got[0][0], (np.conj(factor) * b[0]).astype(np.complex64) * t)
  a64, b64 = a[0].astype(np.complex128), b[0].astype(np.complex128)
  # (c = i a: tbar = Re(conj(i a) b) = Im(conj(a) b), two exact products and one float64 fma chain: to rounding of the sum)
  np.testing.assert_allclose(got[2], np.imag(np.conj(a64) * b64), rtol=0, atol=2.0**-52 * np.abs(a64 * b64).max())


# ---- 3. independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,num_a,num_b", [(6, 3, 5), (11, 8, 9), (12, 9, 8), (7, 17, 33), (13, 33, 2)])
def test_outputs_do_not_depend_on_the_call_they_share(n, num_a, num_b):
  bras, kets, gamma, tables = _case(n, num_a, num_b)
  t = tables["signed"]
  d_bras, d_kets, d_table, d_gamma = _device(bras, kets, gamma, t)
  full = _raw_vjp(d_bras, d_kets, d_table, d_gamma)
  again = _raw_vjp(d_bras, d_kets, d_table, d_gamma)
  assert all(np.array_equal(_bits32(x), _bits32(y)) for x, y in zip(full[:2], again[:2])) and np.array_equal(_bits64(full[2]), _bits64(again[2]))
  # every subset of the outputs: what is asked for has the bits of the full call, what is not stays NaN
  for want in [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)]:
    part = _raw_vjp(d_bras, d_kets, d_table, d_gamma, want=want)
    for k in range(3):
      bits = _bits32 if k < 2 else _bits64
      if want[k]:
        assert np.array_equal(bits(part[k]), bits(full[k])), (want, k)
      else:
        assert np.all(np.isnan(part[k].real)), (want, k)
  # the binding, with its own scratch
  bound = E.cross_gram_vjp(d_bras, d_kets, d_table, d_gamma)
  assert bound[0].dtype == bound[1].dtype == torch.complex64 and bound[2].dtype == torch.float64
  assert all(np.array_equal(_bits32(x.cpu().numpy()), _bits32(y)) for x, y in zip(bound[:2], full[:2]))
  assert np.array_equal(_bits64(bound[2].cpu().numpy()), _bits64(full[2]))
  only = E.cross_gram_vjp(d_bras, d_kets, d_table, d_gamma, want_kets=False, want_table=False)
  assert only[1] is None and only[2] is None and torch.equal(torch.view_as_real(only[0]), torch.view_as_real(bound[0]))
  # one ket against all bras, one bra against all kets
  for j in sorted({0, num_b // 2, num_b - 1}):
    single = _raw_vjp(d_bras, d_kets[j:j + 1].clone(), d_table, d_gamma[:, j:j + 1].contiguous(), want=(False, True, False))
    assert np.array_equal(_bits32(single[1][0]), _bits32(full[1][j])), j
  for i in sorted({0, num_a // 2, num_a - 1}):
    single = _raw_vjp(d_bras[i:i + 1].clone(), d_kets, d_table, d_gamma[i:i + 1].contiguous(), want=(True, False, False))
    assert np.array_equal(_bits32(single[0][0]), _bits32(full[0][i])), i


@pytest.mark.parametrize("n,total,num_a,num_b,start_b", [(6, 6, 4, 5, 1), (11, 12, 9, 8, 2), (7, 20, 17, 12, 8)])
def test_overlapping_views_of_one_buffer_give_the_bits_of_separate_copies(n, total, num_a, num_b, start_b):
  states, _, _, tables = _case(n, total, 1)
  gamma = _case(n, num_a, num_b)[2]
  buffer = torch.from_numpy(states).cuda()
  d_table, d_gamma = torch.from_numpy(tables["positive"]).cuda(), torch.from_numpy(gamma).cuda()
  view_a, view_b = buffer[:num_a], buffer[start_b:start_b + num_b]
  assert view_b.data_ptr() < view_a.data_ptr() + view_a.numel() * 8  # (they overlap)
  views = _raw_vjp(view_a, view_b, d_table, d_gamma)
  copies = _raw_vjp(view_a.clone(), view_b.clone(), d_table, d_gamma)
  assert all(np.array_equal(_bits32(x), _bits32(y)) for x, y in zip(views[:2], copies[:2])) and np.array_equal(_bits64(views[2]), _bits64(copies[2]))


# ---- 4. the same buffer -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num", [6, 17])
@pytest.mark.parametrize("n", [6, 11])
def test_same_buffer_is_the_weighted_gram_vjp(n, num):
  """out_bras + out_kets against qhbm_weighted_gram_vjp with H = Gamma + Gamma^H: both are f32 chains for one complex128
  value, so they differ by at most the sum of their bounds (the sum of two floats adds one more rounding of the result)."""
  states, _, gamma, tables = _case(n, num, num)
  t = tables["signed"]
  hermitian = (gamma.astype(np.complex128) + gamma.astype(np.complex128).conj().T).astype(np.complex64)
  d_states, _, d_table, d_gamma = _device(states, states, gamma, t)
  out_bras, out_kets, grad = _raw_vjp(d_states, d_states, d_table, d_gamma)
  gram_out, gram_grad = E.weighted_gram_vjp(d_states, d_table, torch.from_numpy(hermitian).cuda())
  gram_out, gram_grad = gram_out.cpu().numpy(), gram_grad.cpu().numpy()
  bar_a, bar_b, bar_t = V.vjp_bounds(states, states, t, gamma)
  gram_bar, gram_bar_t = G.gram_vjp_bounds(states, t, hermitian)
  eps = (2.0 * num + 4.0) * 2.0**-24
  total = out_bras.astype(np.complex128) + out_kets.astype(np.complex128)
  err = np.maximum(np.abs(total.real - gram_out.real), np.abs(total.imag - gram_out.imag))
  # (H was rounded to complex64 once more than Gamma: one 2^-24 of each entry, inside gram_bar's term)
  bar = eps * (bar_a + bar_b) + (eps + 2.0**-24) * gram_bar
  print(f"n={n} M=K={num}: worst {float(np.max(err[bar > 0] / bar[bar > 0])):.3g} of the summed bounds")
  assert np.all(err <= bar)
  assert np.all(np.abs(grad - gram_grad) <= eps * bar_t + (eps + 2.0**-24) * gram_bar_t)
  assert np.abs(gram_out).max() > 0 and np.abs(gram_grad).max() > 0


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_return_a_message_and_launch_nothing():
  lib = E.load_library()
  n, num_a, num_b = 6, 4, 9
  dim = 1 << n
  bras = torch.ones((num_a * dim + 2,), dtype=torch.complex64, device="cuda")
  kets = torch.ones((num_b * dim + 2,), dtype=torch.complex64, device="cuda")
  out_bras = torch.full((num_a * dim + 2,), complex(-7.0, -7.0), dtype=torch.complex64, device="cuda")
  out_kets = torch.full((num_b * dim + 2,), complex(-7.0, -7.0), dtype=torch.complex64, device="cuda")
  table = torch.ones(dim + 2, dtype=torch.float32, device="cuda")
  gamma = torch.ones(num_a * num_b + 1, dtype=torch.complex64, device="cuda")
  grad = torch.full((dim + 1,), -7.0, dtype=torch.float64, device="cuda")
  scratch = torch.zeros(E.cross_gram_vjp_scratch_bytes(num_a, num_b, n) // 8 + 1, dtype=torch.float64, device="cuda")
  stream = torch.cuda.current_stream().cuda_stream
  good = dict(a=bras.data_ptr(), m=num_a, b=kets.data_ptr(), k=num_b, n=n, t=table.data_ptr(), c=gamma.data_ptr(),
              oa=out_bras.data_ptr(), ob=out_kets.data_ptr(), g=grad.data_ptr(), w=scratch.data_ptr())
  refused = [
      (dict(m=0), "M must be in [1, 1024]"), (dict(m=1025), "M must be"), (dict(k=0), "K must be in [1, 1024]"), (dict(k=1025), "K must be"),
      (dict(n=0), "n_qubits must be in [1, 31]"), (dict(n=32), "n_qubits must be"),
      (dict(a=None), "d_bras is NULL"), (dict(b=None), "d_kets is NULL"), (dict(c=None), "d_cotangent is NULL"), (dict(w=None), "d_scratch is NULL"),
      (dict(oa=None, ob=None, g=None), "all NULL"),
      (dict(a=bras.data_ptr() + 8), "d_bras must be 16-byte aligned"), (dict(b=kets.data_ptr() + 8), "d_kets must be 16-byte aligned"),
      (dict(oa=out_bras.data_ptr() + 8), "d_out_bras must be 16-byte aligned"), (dict(ob=out_kets.data_ptr() + 8), "d_out_kets must be 16-byte aligned"),
      (dict(t=table.data_ptr() + 4), "d_table must be 8-byte aligned"), (dict(c=gamma.data_ptr() + 4), "d_cotangent must be 8-byte aligned"),
      (dict(g=grad.data_ptr() + 4), "d_table_grad must be 8-byte aligned"), (dict(w=scratch.data_ptr() + 4), "d_scratch must be 8-byte aligned"),
      (dict(oa=bras.data_ptr()), "d_out_bras overlaps d_bras"), (dict(oa=kets.data_ptr() + 8 * dim * (num_b - 1) + 16), "d_out_bras overlaps d_kets"),
      (dict(ob=kets.data_ptr()), "d_out_kets overlaps d_kets"), (dict(ob=bras.data_ptr() + 8 * dim * (num_a - 1) + 16), "d_out_kets overlaps d_bras"),
      (dict(ob=out_bras.data_ptr() + 16, oa=out_bras.data_ptr()), "d_out_bras overlaps d_out_kets"),
  ]
  for change, message in refused:
    a = dict(good, **change)
    rc = lib.qhbm_cross_gram_vjp(a["a"], a["m"], a["b"], a["k"], a["n"], a["t"], a["c"], a["oa"], a["ob"], a["g"], a["w"], stream)
    assert rc != 0, change
    assert message in lib.qhbm_last_error(None).decode(), (change, lib.qhbm_last_error(None).decode())
  torch.cuda.synchronize()
  assert torch.all(torch.view_as_real(out_bras) == -7.0) and torch.all(torch.view_as_real(out_kets) == -7.0)
  assert torch.all(grad == -7.0) and torch.all(scratch == 0.0)
  # the good call goes through, NULL table included: out_kets = sum of four ones, out_bras = sum of nine, tbar = 9 * 4
  assert lib.qhbm_cross_gram_vjp(good["a"], num_a, good["b"], num_b, n, None, good["c"], good["oa"], good["ob"], good["g"], good["w"], stream) == 0
  torch.cuda.synchronize()
  assert torch.all(torch.view_as_real(out_kets[:num_b * dim]) == 4.0 * torch.tensor([1.0, 0.0], device="cuda"))
  assert torch.all(torch.view_as_real(out_bras[:num_a * dim]) == 9.0 * torch.tensor([1.0, 0.0], device="cuda"))
  assert torch.all(torch.view_as_real(out_kets[num_b * dim:]) == -7.0) and torch.all(torch.view_as_real(out_bras[num_a * dim:]) == -7.0)
  assert torch.all(grad[:dim] == 36.0) and grad[dim] == -7.0


def test_binding_and_mirror_refusals():
  bras = torch.ones((3, 16), dtype=torch.complex64, device="cuda")
  kets = torch.ones((2, 16), dtype=torch.complex64, device="cuda")
  table = torch.ones(16, dtype=torch.float32, device="cuda")
  gamma = torch.ones((3, 2), dtype=torch.complex64)
  with pytest.raises(E.EngineError, match="CUDA kets"):
    E.cross_gram_vjp(bras, kets.cpu(), None, gamma)
  with pytest.raises(ValueError, match="no output"):
    E.cross_gram_vjp(bras, kets, table, gamma, want_bras=False, want_kets=False, want_table=False)
  with pytest.raises(ValueError, match="table must be real and have shape"):
    E.cross_gram_vjp(bras, kets, table[:8], gamma)
  with pytest.raises(E.EngineError, match="table on the states' device"):
    E.cross_gram_vjp(bras, kets, table.cpu(), gamma)
  with pytest.raises(ValueError, match="cotangent must be complex of shape"):
    E.cross_gram_vjp(bras, kets, table, gamma.T)
  with pytest.raises(ValueError, match="cotangent must be complex of shape"):
    E.cross_gram_vjp(bras, kets, table, torch.ones((3, 2)))
  with pytest.raises(ValueError, match="power of two"):
    E.cross_gram_vjp(bras[:, :12], kets[:, :12], None, gamma)
  with pytest.raises(ValueError, match="amplitudes, kets"):
    E.cross_gram_vjp(bras, kets[:, :8], None, gamma)
  with pytest.raises(E.EngineError, match="CUDA bras"):
    inference.differentiable_cross_gram(bras.cpu(), kets)
  with pytest.raises(ValueError, match="table must have shape"):
    inference.differentiable_cross_gram(bras, kets, table[:8])
  with pytest.raises(ValueError, match="real floating-point"):
    inference.differentiable_cross_gram(bras, kets, table.to(torch.complex64))
  # double backward is refused
  leaf = bras.clone().requires_grad_(True)
  (g,) = torch.autograd.grad((inference.differentiable_cross_gram(leaf, kets).abs()**2).sum(), [leaf], create_graph=True)
  with pytest.raises(RuntimeError, match="differentiate twice"):
    g.abs().sum().backward()


# ---- 6. the autograd node ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,num_a,num_b", [(6, 5, 3), (12, 8, 8), (7, 17, 9)])
def test_autograd_node_against_the_restatement(n, num_a, num_b):
  bras, kets, gamma, tables = _case(n, num_a, num_b)
  table = tables["signed" if num_a == 5 else "positive"].astype(np.float64)
  table32 = table.astype(np.float32)
  leaf_a = torch.from_numpy(bras).cuda().requires_grad_(True)
  leaf_b = torch.from_numpy(kets).cuda().requires_grad_(True)
  d_table = torch.from_numpy(table).cuda().requires_grad_(True)
  cross = inference.differentiable_cross_gram(leaf_a, leaf_b, d_table)
  assert cross.dtype == torch.complex128 and cross.requires_grad and tuple(cross.shape) == (num_a, num_b)
  plain = E.cross_gram(leaf_a.detach(), leaf_b.detach(), d_table.detach())
  assert torch.equal(torch.view_as_real(cross.detach()), torch.view_as_real(plain))  # the same forward bits
  assert inference.cross_gram is E.cross_gram
  label = f"n={n} M={num_a} K={num_b}"
  gamma128 = gamma.astype(np.complex128)  # (a complex128 cotangent that is not Hermitian, handed to autograd as it is)
  got = torch.autograd.grad(cross, [leaf_a, leaf_b, d_table], grad_outputs=torch.from_numpy(gamma128).cuda(), retain_graph=True)
  assert got[0].dtype == got[1].dtype == torch.complex64 and got[2].dtype == torch.float64
  want, bars = V.vjp(bras, kets, table32, gamma), V.vjp_bounds(bras, kets, table32, gamma)
  _hold_bound(label + " node", [g.cpu().numpy() for g in got], want, bars, num_a, num_b)
  assert min(np.abs(w).max() for w in want) > 1e-3
  # a loss through torch: sum |C_ij|^2, Gamma = 2 C (rounded to complex64 by the node)
  got = torch.autograd.grad((cross.abs()**2).sum(), [leaf_a, leaf_b, d_table], retain_graph=True)
  want = V.vjp(bras, kets, table32, 2.0 * X.cross_gram(bras, kets, table32))
  for name, g, w in zip(("bras", "kets", "table"), got, want):
    _close(f"{label} sum |C|^2 d/d {name}", g, w, _grad_bar(w))
  # only what requires grad is delivered, and it has the bits of the full backward; no table: ones
  first = torch.autograd.grad(cross, [leaf_a, leaf_b, d_table], grad_outputs=torch.from_numpy(gamma128).cuda(), retain_graph=True)
  node = inference.differentiable_cross_gram(leaf_a, leaf_b.detach(), d_table.detach())
  (only_bras,) = torch.autograd.grad(node, [leaf_a], grad_outputs=torch.from_numpy(gamma128).cuda())
  assert torch.equal(torch.view_as_real(only_bras), torch.view_as_real(first[0]))
  node = inference.differentiable_cross_gram(leaf_a.detach(), leaf_b.detach(), d_table)
  (only_table,) = torch.autograd.grad(node, [d_table], grad_outputs=torch.from_numpy(gamma128).cuda())
  assert torch.equal(only_table, first[2])
  node = inference.differentiable_cross_gram(leaf_a.detach(), leaf_b)
  (only_kets,) = torch.autograd.grad(node, [leaf_b], grad_outputs=torch.from_numpy(gamma128).cuda())
  want = V.vjp(bras, kets, None, gamma)[1]
  _close(f"{label} no table d/d kets", only_kets, want, _grad_bar(want))
  assert not inference.differentiable_cross_gram(leaf_a.detach(), leaf_b.detach()).requires_grad


# ---- 6. gradients through the mirror -------------------------------------------------------------------------------------------------
class _Circuit:
  """Two HEA layers with what the restatement needs: the gate list and the float32 parameter values the model holds."""

  def __init__(self, n):
    self.n = n
    rng = np.random.default_rng(160 + n)
    tag = f"cg{n}"
    self.circ = models.DirectQuantumCircuit(hea_circuit(ir.GridQubit.rect(1, n), 2, tag))
    self.gates, names = O.hea_gates(n, 2, tag)
    assert self.circ.symbol_names == names
    with torch.no_grad():
      self.circ.trainable_variables[0].copy_(torch.as_tensor(rng.uniform(-1, 1, len(names)), dtype=torch.float32))
    self.params = self.circ.trainable_variables[0].detach().double().numpy().copy()
    self.variable = self.circ.trainable_variables[0]
    self.inference = inference.AnalyticQuantumInference(self.circ)


@functools.lru_cache(maxsize=None)
def _circuit(n):
  return _Circuit(n)


def _host_metrics(psi, w, b, v):
  """The host formulas on complex128 Gram matrices of the restatement's kind, in torch on the CPU: (metrics, (G_A, C)) with
  the two matrices that depend on psi retaining their gradients."""
  gram_a, gram_b, cross = psi.conj() @ psi.transpose(0, 1), b.conj() @ b.transpose(0, 1), psi.conj() @ b.transpose(0, 1)
  gram_a.retain_grad()
  cross.retain_grad()
  return EM.differentiable_metrics_from_grams(gram_a, gram_b, cross, w, v), (gram_a, cross)


def _hold_mirror(label, n, inputs, w, targets, v):
  """`ensemble_metrics((final states of `inputs`, w), (targets, v), differentiable=True)`: values against the default path,
  the circuit's gradient against restatement + final_states_ref.vjp, the weights' gradients in float64."""
  c = _circuit(n)
  inputs64 = inputs.astype(np.complex64).astype(np.complex128)  # (as the engine reads them)
  targets64 = targets.astype(np.complex64).astype(np.complex128)
  d_targets = torch.from_numpy(targets.astype(np.complex64)).cuda()
  w_leaf = torch.from_numpy(w.copy()).requires_grad_(True)
  v_leaf = torch.from_numpy(v.copy()).requires_grad_(True)
  psi = c.inference.final_states_from_states(torch.from_numpy(inputs.astype(np.complex64)).cuda())
  assert psi.requires_grad
  got = inference.ensemble_metrics((psi, w_leaf), (d_targets, v_leaf), differentiable=True)
  plain = inference.ensemble_metrics((psi.detach(), w_leaf.detach()), (d_targets, v_leaf.detach()))
  scale = max(plain.trace_a, plain.trace_b)
  for field in dataclasses.fields(plain):
    value = getattr(got, field.name)
    assert isinstance(getattr(plain, field.name), float)  # the default path is as it was
    assert torch.is_tensor(value) and value.dtype == torch.float64 and value.dim() == 0 and value.device.type == "cpu", field.name
    assert abs(float(value.detach()) - getattr(plain, field.name)) <= 1e-12 * scale, field.name
  # the reference: Gamma of G_A and of C from the host formulas in float64, pulled back by the two restatements and the circuit
  finals = S.final_states(n, c.gates, c.params, inputs64)
  for metric in METRICS:
    leaves = [torch.from_numpy(np.ascontiguousarray(t)).requires_grad_(True) for t in (finals, w, targets64, v)]
    ref, (gram_a, cross) = _host_metrics(*leaves)
    getattr(ref, metric).backward()
    # (the overlap does not depend on G_A: no cotangent reaches it)
    gamma_a = np.zeros(gram_a.shape, dtype=np.complex128) if gram_a.grad is None else gram_a.grad.resolve_conj().numpy()
    cot = G.vjp(finals, None, gamma_a)[0] + V.vjp(finals, targets64, None, cross.grad.resolve_conj().numpy())[0]
    np.testing.assert_allclose(cot, leaves[0].grad.resolve_conj().numpy(), atol=1e-12)  # (the two restatements are the chain rule)
    want = F.vjp(n, c.gates, c.params, inputs64, cot)
    field = getattr(got, metric)
    assert field.requires_grad
    grad, grad_w, grad_v = torch.autograd.grad(field, [c.variable, w_leaf, v_leaf], retain_graph=True)
    _close(f"{label} {metric} d/d circuit", grad, want, _grad_bar(want))
    assert np.abs(want).max() > 1e-5  # (the check is not of zeros)
    # the weights: float64 on the host from the device's own Gram matrices, so against the formulas at the DEVICE's final states
    at_device = [torch.from_numpy(np.ascontiguousarray(t)).requires_grad_(True)
                 for t in (psi.detach().cpu().numpy().astype(np.complex128), w, targets64, v)]
    ref_device, _ = _host_metrics(*at_device)
    want_w, want_v = torch.autograd.grad(getattr(ref_device, metric), [at_device[1], at_device[3]])
    for name, g, expected in (("weights a", grad_w, want_w.numpy()), ("weights b", grad_v, want_v.numpy())):
      _close(f"{label} {metric} d/d {name}", g, expected, 1e-7 * max(1.0, float(np.abs(expected).max())))
  return got


@pytest.mark.parametrize("num_a,num_b", [(1, 2), (3, 2), (1, 3), (3, 3)])
@pytest.mark.parametrize("n", [4, 6])
def test_mirror_gradients_through_final_states(n, num_a, num_b):
  inputs, w, targets, v = X.well_conditioned_ensembles(n, num_a, num_b, 7000 * n + 10 * num_a + num_b)
  with warnings.catch_warnings():
    warnings.simplefilter("error")  # (the Cholesky route: no constant-distance warning)
    got = _hold_mirror(f"n={n} M={num_a} K={num_b}", n, inputs, w, targets, v)
  assert got.trace_distance.requires_grad
  # StateVectorData passes the flag on, and is itself a constant
  source = data.StateVectorData(torch.from_numpy(targets), torch.from_numpy(v))
  psi = _circuit(n).inference.final_states_from_states(torch.from_numpy(inputs.astype(np.complex64)).cuda())
  fidelity = source.fidelity_to((psi, torch.from_numpy(w)), differentiable=True)
  distance = source.trace_distance_to((psi, torch.from_numpy(w)), differentiable=True)
  assert fidelity.requires_grad and distance.requires_grad
  assert abs(float(fidelity.detach()) - float(got.fidelity.detach())) <= 1e-12 * float(max(got.trace_a, got.trace_b).detach())
  assert isinstance(source.fidelity_to((psi.detach(), torch.from_numpy(w))), float)
  assert not inference.ensemble_metrics(source, source, differentiable=True).overlap.requires_grad


def test_mirror_gradients_at_twelve_qubits():
  """Nine states against eight: the matrix kernel for the kets' side is not asked for (the targets are constants), the bras'
  cotangent comes from the vector kernel with eight source rows and G_A's from the matrix kernel of gram_vjp.hip."""
  n = 12
  rng = np.random.default_rng(12)
  inputs = S.random_states(9, n, 21) * rng.uniform(0.7, 1.0, (9, 1))
  targets = S.random_states(8, n, 22) * rng.uniform(0.7, 1.0, (8, 1))
  # (random states at 12 qubits overlap by 2^-6: mix the targets into the inputs' images so that fidelity and overlap are O(1))
  c = _circuit(n)
  images = S.final_states(n, c.gates, c.params, inputs.astype(np.complex64).astype(np.complex128))
  targets[:6] = 0.6 * images[:6] + 0.8 * targets[:6]
  _hold_mirror("n=12 M=9 K=8", n, inputs, rng.uniform(0.05, 0.15, 9), targets, rng.uniform(0.05, 0.15, 8))
