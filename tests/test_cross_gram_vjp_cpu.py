"""What needs no GPU of the cross-Gram matrix's VJP and of `ensemble_metrics(..., differentiable=True)`.

1. The complex128 restatement (tests/cross_gram_vjp_ref.py, what the GPU tests compare the engine with) against central
   differences in float64 -- step 1e-5, bar 1e-7 max(1, ||grad||_inf), the bar of tests/test_state_metrics_vjp_cpu.py --, the
   hand checks, and the same-buffer identity with tests/state_metrics_vjp_ref.vjp.
2. The host formulas under torch autograd (`differentiable_metrics_from_grams`), fed with the restatement's Gram matrices,
   against central differences (step 1e-6) of the DENSE route tests/cross_gram_ref.dense_metrics, for the states and the
   weights of both ensembles, at the same bar.  Each case asserts the conditions the bar rests on.
3. Orthogonal supports: the fidelity's gradient is finite and zero to rounding.
4. The entry points without a device: ABI symbols, scratch sizes against the plan header, every refusal, the plan checker
   under ASan / UBSan as a stand-alone program, and the assembly of the translation unit.
"""
import ctypes
import importlib
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import torch

from tests import cross_gram_ref as X
from tests import cross_gram_vjp_ref as V
from tests import state_metrics_ref as R
from tests import state_metrics_vjp_ref as G

EM = importlib.import_module("qhbmlib_amd.inference.ensemble_metrics")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qhbm-library_amd", "csrc")
STEP = 1e-5
PAIRS = [(1, 1), (3, 2), (2, 5), (5, 3)]
METRICS = ("overlap", "fidelity", "trace_distance")


def _bar(grad):
  return 1e-7 * max(1.0, float(np.abs(grad).max()))


def _central_states(f, states, step=STEP):
  """dL/dRe a + i dL/dIm a, amplitude by amplitude."""
  grad = np.zeros(states.shape, dtype=np.complex128)
  for m in range(states.shape[0]):
    for x in range(states.shape[1]):
      for unit in (1.0, 1j):
        hi, lo = states.copy(), states.copy()
        hi[m, x] += step * unit
        lo[m, x] -= step * unit
        grad[m, x] += unit * (f(hi) - f(lo)) / (2 * step)
  return grad


def _central_real(f, vector, step=STEP):
  grad = np.zeros(vector.shape)
  for x in range(vector.size):
    hi, lo = vector.copy(), vector.copy()
    hi[x] += step
    lo[x] -= step
    grad[x] = (f(hi) - f(lo)) / (2 * step)
  return grad


def _hold(label, got, want):
  err = float(np.abs(got - want).max())
  print(f"{label}: error {err:.3e} (bar {_bar(want):.3e}, ||grad|| {np.abs(want).max():.3e})")
  assert err <= _bar(want), label


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_a,num_b", PAIRS)
@pytest.mark.parametrize("n", [3, 4, 5])
def test_vjp_matches_central_differences(n, num_a, num_b):
  """L = Re sum conj(B_ij) C_ij with a B that is not Hermitian and a signed table: Gamma = B."""
  bras, kets, table, b = V.random_case(n, num_a, num_b, 100 * n + 10 * num_a + num_b)
  assert table.min() < 0 < table.max()
  if num_a == num_b and num_a > 1:
    assert np.abs(b - b.conj().T).max() > 0.1
  loss = lambda a_, b_, t_: V.linear_loss(X.cross_gram(a_, b_, t_), b)[0]
  got_bras, got_kets, got_table = V.vjp(bras, kets, table, b)
  want_bras = _central_states(lambda s: loss(s, kets, table), bras)
  want_kets = _central_states(lambda s: loss(bras, s, table), kets)
  want_table = _central_real(lambda t: loss(bras, kets, t), table)
  _hold(f"n={n} M={num_a} K={num_b}: bras", got_bras, want_bras)
  _hold(f"n={n} M={num_a} K={num_b}: kets", got_kets, want_kets)
  _hold(f"n={n} M={num_a} K={num_b}: table", got_table, want_table)
  assert min(np.abs(want_bras).max(), np.abs(want_kets).max()) > 1e-3 and np.abs(want_table).max() > 1e-4  # (not of zeros)
  # no table: ones
  got_bras, got_kets, _ = V.vjp(bras, kets, None, b)
  _hold(f"n={n} M={num_a} K={num_b}: bras, no table", got_bras, _central_states(lambda s: loss(s, kets, None), bras))
  _hold(f"n={n} M={num_a} K={num_b}: kets, no table", got_kets, _central_states(lambda s: loss(bras, s, None), kets))


def test_hand_checks():
  rng = np.random.default_rng(1)
  a = rng.normal(size=(1, 8)) + 1j * rng.normal(size=(1, 8))
  b = rng.normal(size=(1, 8)) + 1j * rng.normal(size=(1, 8))
  t = rng.normal(size=8)
  # M = K = 1, L = Re C: gbar_b = t a, gbar_a = t b, tbar = Re(conj(a) b)
  out_a, out_b, grad = V.vjp(a, b, t, np.ones((1, 1)))
  np.testing.assert_allclose(out_b, t * a, atol=1e-14)
  np.testing.assert_allclose(out_a, t * b, atol=1e-14)
  np.testing.assert_allclose(grad, np.real(np.conj(a[0]) * b[0]), atol=1e-14)
  # L = Im C: gbar_b = i t a, gbar_a = -i t b
  out_a, out_b, grad = V.vjp(a, b, t, 1j * np.ones((1, 1)))
  np.testing.assert_allclose(out_b, 1j * t * a, atol=1e-14)
  np.testing.assert_allclose(out_a, -1j * t * b, atol=1e-14)
  np.testing.assert_allclose(grad, np.imag(np.conj(a[0]) * b[0]), atol=1e-14)
  # the bound terms dominate the outputs they bound
  bras, kets, table, gamma = V.random_case(4, 3, 5, 9)
  outs, bars = V.vjp(bras, kets, table, gamma), V.vjp_bounds(bras, kets, table, gamma)
  for out, bar in zip(outs[:2], bars[:2]):
    assert out.shape == bar.shape and np.all(np.abs(out.real) <= bar + 1e-15) and np.all(np.abs(out.imag) <= bar + 1e-15)
  assert np.all(np.abs(outs[2]) <= bars[2] + 1e-15)


@pytest.mark.parametrize("n,num", [(3, 1), (4, 3), (5, 6)])
def test_same_buffer_is_the_weighted_gram_vjp(n, num):
  """Bras and kets the same buffer: gbar_a + gbar_b is the weighted Gram matrix's cotangent for H = Gamma + Gamma^H, and
  tbar the same table cotangent (1/2 sum_j Re conj(c^H_j) a_j with c^H from H)."""
  states, _, table, gamma = V.random_case(n, num, num, 50 * n + num)
  out_a, out_b, grad = V.vjp(states, states, table, gamma)
  want_states, want_table = G.vjp(states, table, gamma)
  np.testing.assert_allclose(out_a + out_b, want_states, atol=1e-13)
  np.testing.assert_allclose(grad, want_table, atol=1e-13)
  assert np.abs(want_states).max() > 1e-2 and np.abs(want_table).max() > 1e-3


# ---- 2. the metrics' gradients against the dense route ---------------------------------------------------------------------
def _torch_metrics(a, w, b, v):
  """The host formulas under autograd on the restatement's Gram matrices, written as torch ops so that the graph reaches
  the states and the weights (complex128 / float64 leaves)."""
  gram_a, gram_b, cross = a.conj() @ a.transpose(0, 1), b.conj() @ b.transpose(0, 1), a.conj() @ b.transpose(0, 1)
  return EM.differentiable_metrics_from_grams(gram_a, gram_b, cross, w, v), (gram_a, gram_b, cross)


@pytest.mark.parametrize("n,num_a,num_b", [(3, 1, 1), (3, 2, 3), (3, 3, 3), (4, 5, 2), (5, 3, 5)])
def test_metric_gradients_match_the_dense_route(n, num_a, num_b):
  a, w, b, v = X.well_conditioned_ensembles(n, num_a, num_b, 6000 * n + 10 * num_a + num_b)
  label = f"n={n} M={num_a} K={num_b}"
  # the conditions the bar rests on
  joint = X.joint_gram(a, w, b, v)
  cond = np.linalg.cond(joint)
  lam, route = EM.difference_spectrum(torch.from_numpy(joint), num_a)
  singular = np.linalg.svd(np.sqrt(w)[:, None] * X.cross_gram(a, b) * np.sqrt(v)[None, :], compute_uv=False)
  print(f"{label}: cond {cond:.2f} route {route} least relative singular value {singular.min() / singular.max():.3g} "
        f"least |lambda| {float(lam.abs().min()):.3g}")
  assert cond <= 100.0 and route == "cholesky"
  assert singular.min() >= 1e-3 * singular.max() and float(lam.abs().min()) >= 1e-2
  leaves = [torch.from_numpy(np.ascontiguousarray(t)).requires_grad_(True) for t in (a, w, b, v)]
  got, grams = _torch_metrics(*leaves)
  np.testing.assert_allclose(grams[0].detach().numpy(), R.gram(a), atol=1e-14)
  np.testing.assert_allclose(grams[2].detach().numpy(), X.cross_gram(a, b), atol=1e-14)
  plain = EM.metrics_from_grams(R.gram(a), R.gram(b), X.cross_gram(a, b), w, v)
  dense = lambda a_, w_, b_, v_: X.dense_metrics(X.dense(a_, w_), X.dense(b_, v_))
  for metric in METRICS:
    field = getattr(got, metric)
    assert torch.is_tensor(field) and field.dtype == torch.float64 and field.dim() == 0 and field.requires_grad
    np.testing.assert_allclose(float(field.detach()), getattr(plain, metric), rtol=1e-12, atol=1e-15)
    grads = [g.resolve_conj().numpy() for g in torch.autograd.grad(field, leaves, retain_graph=True)]
    want = [_central_states(lambda s: dense(s, w, b, v)[metric], a, 1e-6), _central_real(lambda s: dense(a, s, b, v)[metric], w, 1e-6),
            _central_states(lambda s: dense(a, w, s, v)[metric], b, 1e-6), _central_real(lambda s: dense(a, w, b, s)[metric], v, 1e-6)]
    for name, g, expected in zip(("states a", "weights a", "states b", "weights b"), grads, want):
      _hold(f"{label} {metric} d/d {name}", g, expected)
    assert max(np.abs(e).max() for e in want) > 1e-3  # (the check is not of zeros)
  for name in ("trace_a", "trace_b", "purity_a", "purity_b"):
    np.testing.assert_allclose(float(getattr(got, name).detach()), getattr(plain, name), rtol=1e-12)


# ---- 3. orthogonal supports ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,num_a,num_b", [(3, 1, 1), (3, 2, 3), (5, 3, 5), (5, 5, 2)])
def test_orthogonal_supports_give_a_finite_zero_fidelity_gradient(n, num_a, num_b):
  """X = A^dagger B is zero up to the rounding of the frame's construction, |X_ij| <= 2^n 2^-50 here, so every singular value
  is such a rounded zero.  d fidelity = 2 (sum sigma) sum_i Re(u_i^H dX v_i): with sum sigma <= min(M, K) ||X|| and
  |dX / d state| <= 1 (weights below 1, states of norm below 1.3) the gradient is below 2 min(M, K)^2 2^n 2^-50 1.3 <= 3e-12
  for these shapes -- and above all it is finite: no 1 / sigma appears."""
  a, w, b, v = X.well_conditioned_ensembles(n, num_a, num_b, 4000 * n + 10 * num_a + num_b, orthogonal=True)
  assert np.abs(X.cross_gram(a, b)).max() <= (1 << n) * 2.0**-50
  leaves = [torch.from_numpy(np.ascontiguousarray(t)).requires_grad_(True) for t in (a, w, b, v)]
  got, _ = _torch_metrics(*leaves)
  grads = torch.autograd.grad(got.fidelity, leaves, allow_unused=True)
  for g in grads:
    if g is None:
      continue
    assert bool(torch.isfinite(torch.view_as_real(g.resolve_conj()) if g.is_complex() else g).all())
    assert float(g.abs().max()) <= 3e-12
  assert float(got.fidelity.detach()) <= 64 * X.EPS * (num_a + num_b) * float(max(got.trace_a, got.trace_b).detach())


def test_the_singular_route_returns_a_constant_trace_distance_with_a_warning():
  a, w, b, v = X.well_conditioned_ensembles(4, 3, 2, 77)
  a = a.copy()
  a[2] = a[0]  # a repeated state: Gamma is singular
  leaves = [torch.from_numpy(np.ascontiguousarray(t)).requires_grad_(True) for t in (a, w, b, v)]
  with pytest.warns(UserWarning, match="returned as a constant"):
    got, _ = _torch_metrics(*leaves)
  plain = EM.metrics_from_grams(R.gram(a), R.gram(b), X.cross_gram(a, b), w, v)
  assert not got.trace_distance.requires_grad and float(got.trace_distance.detach()) == pytest.approx(plain.trace_distance, rel=1e-12)
  assert got.fidelity.requires_grad and got.overlap.requires_grad
  assert all(bool(torch.isfinite(torch.view_as_real(g.resolve_conj()) if g.is_complex() else g).all())
             for g in torch.autograd.grad(got.fidelity, leaves))
  # and the Cholesky route warns of nothing
  leaves = [torch.from_numpy(np.ascontiguousarray(t)).requires_grad_(True) for t in X.well_conditioned_ensembles(4, 3, 2, 77)]
  with warnings.catch_warnings():
    warnings.simplefilter("error")
    assert _torch_metrics(*leaves)[0].trace_distance.requires_grad


# ---- 4. the entry points, without a device ---------------------------------------------------------------------------------
NEW_SYMBOLS = ("qhbm_cross_gram_vjp_scratch_bytes", "qhbm_cross_gram_vjp")


def test_abi_symbols_and_version():
  from qhbmlib_amd import _engine as E  # pylint: disable=import-outside-toplevel
  with open(os.path.join(ROOT, "include", "qhbm_engine.h")) as f:
    header = f.read()
  assert int(re.search(r"#define QHBM_ABI_VERSION (\d+)", header).group(1)) == 5 == E.ABI_VERSION
  lib = E.load_library()
  assert lib.qhbm_abi_version() == 5
  for sym in NEW_SYMBOLS:
    assert re.search(r"\bint " + sym + r"\(", header), sym
    assert sym in E.ABI_SYMBOLS
    getattr(lib, sym)
  from qhbmlib_amd import inference  # pylint: disable=import-outside-toplevel
  assert inference.cross_gram is E.cross_gram and inference.differentiable_cross_gram is EM.differentiable_cross_gram


def _planes_bytes(rows, outputs):
  """The plan header's W planes of one side, restated: none up to 8 source rows; above, two float planes of
  16 ceil(R / 16) x Ps, Ps = 16 ceil(S / 16) up to 64 and 64 ceil(S / 64) beyond."""
  if rows <= 8:
    return 0
  s16 = 16 * ((outputs + 15) // 16)
  pitch = s16 if s16 <= 64 else 64 * ((s16 + 63) // 64)
  return 2 * 4 * 16 * ((rows + 15) // 16) * pitch


def test_scratch_size_needs_no_device_and_refuses_bad_shapes():
  from qhbmlib_amd import _engine as E  # pylint: disable=import-outside-toplevel
  for num_a, num_b in [(1, 1), (8, 8), (8, 1024), (9, 8), (8, 9), (9, 9), (16, 17), (32, 2), (2, 32), (33, 15), (65, 3), (3, 65),
                       (64, 65), (1024, 9), (1024, 1024)]:
    want = max(16, _planes_bytes(num_a, num_b) + _planes_bytes(num_b, num_a))
    assert E.cross_gram_vjp_scratch_bytes(num_a, num_b, 3) == E.cross_gram_vjp_scratch_bytes(num_a, num_b, 31) == want, (num_a, num_b)
  assert E.cross_gram_vjp_scratch_bytes(8, 8, 24) == 16 and E.cross_gram_vjp_scratch_bytes(9, 8, 24) == 2 * 4 * 16 * 16
  assert E.cross_gram_vjp_scratch_bytes(1024, 1024, 31) == 2 * (2 * 4 * 1024 * 1024)
  lib = E.load_library()
  out = ctypes.c_size_t()
  for args, text in [((0, 1, 6), "M must be in [1, 1024]"), ((1025, 1, 6), "M must be in"), ((-1, 1, 6), "M must be in"),
                     ((1, 0, 6), "K must be in [1, 1024]"), ((1, 1025, 6), "K must be in"), ((1, -1, 6), "K must be in"),
                     ((1, 1, 0), "n_qubits must be in [1, 31]"), ((1, 1, 32), "n_qubits must be in [1, 31]")]:
    assert lib.qhbm_cross_gram_vjp_scratch_bytes(*args, ctypes.byref(out)) != 0
    assert text in lib.qhbm_last_error(None).decode(), (args, lib.qhbm_last_error(None).decode())
  assert lib.qhbm_cross_gram_vjp_scratch_bytes(1, 1, 6, None) != 0
  assert "out is NULL" in lib.qhbm_last_error(None).decode()


def test_the_call_refuses_before_it_touches_a_device():
  """Every refusal of qhbm_cross_gram_vjp comes before anything is launched, so it can be asked for without a GPU: the
  pointers are never followed."""
  from qhbmlib_amd import _engine as E  # pylint: disable=import-outside-toplevel
  lib = E.load_library()
  n, m, k = 6, 4, 3
  bra_bytes, ket_bytes = m * 8 << n, k * 8 << n  # 2048, 1536
  good = dict(a=0x10000, m=m, b=0x20000, k=k, n=n, t=0x30000, c=0x40000, oa=0x50000, ob=0x60000, g=0x70000, w=0x80000)
  refused = [
      (dict(m=0), "M must be"), (dict(m=1025), "M must be"), (dict(m=-1), "M must be"), (dict(k=0), "K must be"),
      (dict(k=1025), "K must be"), (dict(n=0), "n_qubits"), (dict(n=32), "n_qubits"),
      (dict(a=None), "d_bras is NULL"), (dict(b=None), "d_kets is NULL"), (dict(c=None), "d_cotangent is NULL"),
      (dict(w=None), "d_scratch is NULL"), (dict(oa=None, ob=None, g=None), "all NULL"),
      (dict(a=0x10008), "d_bras must be 16-byte"), (dict(b=0x20008), "d_kets must be 16-byte"),
      (dict(oa=0x50008), "d_out_bras must be 16-byte"), (dict(ob=0x60008), "d_out_kets must be 16-byte"),
      (dict(t=0x30004), "d_table must be 8-byte"), (dict(c=0x40004), "d_cotangent must be 8-byte"),
      (dict(g=0x70004), "d_table_grad must be 8-byte"), (dict(w=0x80004), "d_scratch must be 8-byte"),
      (dict(oa=0x10000), "d_out_bras overlaps d_bras"), (dict(oa=0x10000 + bra_bytes - 16), "d_out_bras overlaps d_bras"),
      (dict(oa=0x20000 - bra_bytes + 16), "d_out_bras overlaps d_kets"), (dict(oa=0x20000 + ket_bytes - 16), "d_out_bras overlaps d_kets"),
      (dict(ob=0x10000 + bra_bytes - 16), "d_out_kets overlaps d_bras"), (dict(ob=0x20000), "d_out_kets overlaps d_kets"),
      (dict(ob=0x20000 - ket_bytes + 16), "d_out_kets overlaps d_kets"),
      (dict(ob=0x50000 + bra_bytes - 16), "d_out_bras overlaps d_out_kets"), (dict(oa=0x60000 + ket_bytes - 16), "d_out_bras overlaps d_out_kets"),
      # bras and kets may alias each other, but then an output overlapping one overlaps both
      (dict(b=0x10000, oa=0x10000 + 16), "d_out_bras overlaps d_bras"),
  ]
  for change, text in refused:
    c = dict(good, **change)
    rc = lib.qhbm_cross_gram_vjp(c["a"], c["m"], c["b"], c["k"], c["n"], c["t"], c["c"], c["oa"], c["ob"], c["g"], c["w"], None)
    assert rc != 0, change
    assert text in lib.qhbm_last_error(None).decode(), (change, lib.qhbm_last_error(None).decode())
  bras = torch.zeros((1, 4), dtype=torch.complex64)
  with pytest.raises(E.EngineError, match="CUDA bras"):
    E.cross_gram_vjp(bras, bras, None, torch.ones((1, 1), dtype=torch.complex64))
  with pytest.raises(E.EngineError, match="CUDA bras"):
    E.cross_gram_vjp(np.zeros((1, 4)), np.zeros((1, 4)), None, np.ones((1, 1)))
  with pytest.raises(E.EngineError, match="CUDA bras"):
    EM.differentiable_cross_gram(bras, bras)


def test_plan_under_asan_and_ubsan(tmp_path):
  """tests/cross_gram_vjp_plan/cross_gram_vjp_plan_check.cpp: both side sweeps of every n <= 13 with (M, K) in
  {1, 3, 8, 9, 16, 17, 33, 65, 1024}^2 and of every M, K <= 40 at n = 7 walked as the kernels walk them -- each output word
  and table_grad entry written once, reads in bounds, LDS entries stored before they are read, the W planes written once
  inside the scratch, the grids within launch limits at 31 qubits and 1024 x 1024 states."""
  cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
  assert cxx, "no host C++ compiler"
  src = os.path.join(ROOT, "tests", "cross_gram_vjp_plan")
  build = subprocess.run(["make", f"CXX={cxx}", f"OUT={tmp_path}"], cwd=src, capture_output=True, text=True, timeout=600)
  assert build.returncode == 0, build.stdout[-2000:] + build.stderr[-2000:]
  env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
  run = subprocess.run([str(tmp_path / "cross_gram_vjp_plan_check")], capture_output=True, text=True, timeout=900, env=env)
  tail = run.stdout[-3000:] + run.stderr[-3000:]
  assert run.returncode == 0, tail
  assert f"cross_gram_vjp_plan_check: {13 * 81 + 40 * 40} shapes" in run.stdout and "cross_gram_vjp_plan_check: 0 failures" in run.stdout, tail
  assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr, tail


def test_translation_unit_compiles_alone_with_matrix_instructions_and_without_atomics_or_scratch():
  """cross_gram_vjp.hip compiles on its own with the product's flags; its gfx950 assembly holds the f32 matrix instruction,
  no floating-point atomic, and no kernel of it uses scratch memory.  It is part of observable.o, and of no other object."""
  hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  assert os.path.exists(hipcc), "no hipcc"
  run = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-mllvm",
                        "-disable-promote-alloca-to-vector=1", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "--cuda-device-only",
                        "-S", "cross_gram_vjp.hip", "-o", "-"], cwd=CSRC, capture_output=True, text=True, timeout=900)
  assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
  asm = run.stdout
  kernels = set(re.findall(r"^(_ZN4qhbm\S*cross_gram_vjp_(?:vector|planes|matrix)_kernel\S*):", asm, flags=re.M))
  assert len(kernels) == 8 + 1 + 4, sorted(kernels)  # R = 1 ... 8, the planes kernel, 1 ... 4 row strips
  code = "\n".join(line.split(";")[0] for line in asm.splitlines())
  assert "v_mfma_f32_16x16x4_f32" in code and "global_load_dwordx4" in code and "v_fma_f64" in code
  assert not re.search(r"\b(?:global|buffer|flat)_atomic_(?:pk_)?add_(?:f16|bf16|f32|f64)\b|\bds_(?:pk_)?add(?:_rtn)?_(?:f16|bf16|f32|f64)\b", code)
  sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
  assert len(sizes) >= 13 and all(v == 0 for v in sizes), sizes
  with open(os.path.join(CSRC, "observable.hip")) as f:
    assert '#include "cross_gram_vjp.hip"' in f.read()
  with open(os.path.join(CSRC, "states.hip")) as f:
    assert "cross_gram" not in f.read()
