"""What needs no GPU of the cross-Gram kernel and of `inference.ensemble_metrics`.

1. The host formulas -- tr(sigma tau) = ||X||_F^2, fidelity = (sum svdvals X)^2, 1/2 ||sigma - tau||_1 from the spectrum of
   J Gamma -- fed with the float64 restatement's Gram matrices (tests/cross_gram_ref.py), against the DENSE route: sigma and
   tau as 2^n x 2^n matrices, sqrt(sigma) by `eigh`, the distance by `eigvalsh`.  n = 3 and 5, M, K in {1, 2, 3, 5}.
   Bars, relative to max(tr sigma, tr tau):
     overlap, fidelity (and traces, purities)  64 2^-53 (M + K), where cond(Gamma) <= 100, which is asserted of the inputs
     trace distance, same inputs               320 2^-53 (M + K)^2: Cholesky's backward error E, |E| <= c (M + K) 2^-53
                                               lambda_max, moves the frame [A B] by |E| / (2 sqrt(lambda_min)), hence each
                                               of the M + K eigenvalues of sigma - tau by sqrt(cond) |E| <= 10 |E|; half their
                                               sum, with the c of the line above (64)
     linearly dependent ensembles              no derived bar: 8 x the error MEASURED here on the CPU against the dense route
                                               (DEPENDENT_MEASURED below, recorded in DESIGN.md 6p) -- a repeated state, more
                                               states than dimensions (n = 3, M = K = 5), and sigma = tau, where the zero
                                               eigenvalue of J Gamma is defective and `eigvals` splits it by ~sqrt(2^-53)
2. The entry points without a device: ABI symbols, scratch size, refusals, and the kernels' translation unit on its own.
"""
import ctypes
import importlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import cross_gram_ref as X
from tests import state_metrics_ref as R

EM = importlib.import_module("qhbmlib_amd.inference.ensemble_metrics")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qhbm-library_amd", "csrc")
SIZES = (1, 2, 3, 5)
FIELDS = ("trace_a", "trace_b", "purity_a", "purity_b", "overlap", "fidelity", "trace_distance")
# worst |formula - dense| / max(tr sigma, tr tau) over the dependent cases of this file, measured on the CPU
DEPENDENT_MEASURED = {"overlap": 2.5e-16, "fidelity": 2.9e-15, "trace_distance": 9.2e-16, "trace_distance_equal": 1.6e-8}


def _both(a, w, b, v):
  """(EnsembleMetrics of the formulas on the restatement's Gram matrices, dense dict, route of the difference spectrum)"""
  got = EM.metrics_from_grams(R.gram(a), R.gram(b), X.cross_gram(a, b), w, v)
  want = X.dense_metrics(X.dense(a, w), X.dense(b, v))
  route = EM.difference_spectrum(torch.from_numpy(X.joint_gram(a, w, b, v)), len(w))[1]
  return got, want, route


def _hold_conditioned(label, a, w, b, v):
  total = len(w) + len(v)
  cond = np.linalg.cond(X.joint_gram(a, w, b, v))
  assert cond <= 100.0, (label, cond)
  got, want, route = _both(a, w, b, v)
  assert route == "cholesky", label
  scale = max(want["trace_a"], want["trace_b"])
  bar = 64 * X.EPS * total * scale
  bar_distance = 320 * X.EPS * total**2 * scale
  errors = {k: abs(getattr(got, k) - want[k]) for k in FIELDS}
  print(f"{label}: cond {cond:.2f} " + " ".join(f"{k} {want[k]:.6g} ({errors[k]:.1e})" for k in FIELDS) +
        f" bars {bar:.1e} {bar_distance:.1e}")
  for k in FIELDS[:-1]:
    assert errors[k] <= bar, (label, k, errors[k], bar)
  assert errors["trace_distance"] <= bar_distance, (label, errors["trace_distance"], bar_distance)
  assert all(isinstance(getattr(got, k), float) for k in FIELDS)
  return got, want


@pytest.mark.parametrize("num_b", SIZES)
@pytest.mark.parametrize("num_a", SIZES)
@pytest.mark.parametrize("n", [3, 5])
def test_formulas_match_the_dense_route(n, num_a, num_b):
  if num_a + num_b > (1 << n):  # n = 3, M = K = 5: ten states in eight dimensions are dependent -- the measured bar
    rng = np.random.default_rng(5)
    a = (rng.normal(size=(num_a, 1 << n)) + 1j * rng.normal(size=(num_a, 1 << n))) / 4
    b = (rng.normal(size=(num_b, 1 << n)) + 1j * rng.normal(size=(num_b, 1 << n))) / 4
    _hold_dependent(f"n={n} M={num_a} K={num_b} overcomplete", a, rng.uniform(0.5, 1, num_a) / num_a, b,
                    rng.uniform(0.5, 1, num_b) / num_b, "trace_distance")
    return
  got, want = _hold_conditioned(f"n={n} M={num_a} K={num_b}",
                                *X.well_conditioned_ensembles(n, num_a, num_b, 1000 * n + 10 * num_a + num_b))
  assert want["overlap"] > 1e-4 and want["trace_distance"] > 1e-2 and want["fidelity"] > 1e-3  # (the check is not of zeros)
  assert got.fidelity <= got.trace_a * got.trace_b * (1 + 1e-12)


@pytest.mark.parametrize("n,num_a,num_b", [(3, 1, 1), (3, 2, 3), (3, 5, 2), (5, 1, 1), (5, 2, 3), (5, 3, 5), (5, 5, 2)])
def test_orthogonal_supports(n, num_a, num_b):
  """fidelity 0, overlap 0, distance 1/2 (tr sigma + tr tau)."""
  a, w, b, v = X.well_conditioned_ensembles(n, num_a, num_b, 4000 * n + 10 * num_a + num_b, orthogonal=True)
  got, want = _hold_conditioned(f"n={n} M={num_a} K={num_b} orthogonal", a, w, b, v)
  scale = max(want["trace_a"], want["trace_b"])
  assert got.fidelity <= 64 * X.EPS * (num_a + num_b) * scale and got.overlap <= 64 * X.EPS * (num_a + num_b) * scale
  assert abs(got.trace_distance - 0.5 * (got.trace_a + got.trace_b)) <= 320 * X.EPS * (num_a + num_b)**2 * scale


def _hold_dependent(label, a, w, b, v, distance_key):
  got, want, route = _both(a, w, b, v)
  assert route == "general", label  # (the singular-Gamma branch runs)
  scale = max(want["trace_a"], want["trace_b"])
  errors = {k: abs(getattr(got, k) - want[k]) / scale for k in ("overlap", "fidelity", "trace_distance")}
  print(f"{label}: " + " ".join(f"{k} {want[k]:.6g} (relative error {e:.2e})" for k, e in errors.items()))
  for k, e in errors.items():
    measured = DEPENDENT_MEASURED[distance_key if k == "trace_distance" else k]
    assert e <= 8 * measured, (label, k, e, measured)
  return got, want


@pytest.mark.parametrize("n,num_a,num_b", [(n, num_a, num_b) for n in (3, 5) for num_a in (2, 3, 5) for num_b in SIZES
                                           if num_a + num_b <= (1 << n)])
def test_a_repeated_state_takes_the_singular_branch(n, num_a, num_b):
  a, w, b, v = X.well_conditioned_ensembles(n, num_a, num_b, 2000 * n + 10 * num_a + num_b)
  a = a.copy()
  a[num_a - 1] = a[0]
  _hold_dependent(f"n={n} M={num_a} K={num_b} repeated state", a, w, b, v, "trace_distance")


@pytest.mark.parametrize("num", SIZES)
@pytest.mark.parametrize("n", [3, 5])
def test_equal_ensembles(n, num):
  """sigma = tau: fidelity (tr sigma)^2, distance 0 -- Gamma = [[G, G], [G, G]] is singular, the general branch runs."""
  a, w, _, _ = X.well_conditioned_ensembles(n, num, 1, 3000 * n + num)
  got, want = _hold_dependent(f"n={n} M={num} sigma = tau", a, w, a, w, "trace_distance_equal")
  scale = want["trace_a"]
  assert abs(got.fidelity - got.trace_a**2) <= 8 * DEPENDENT_MEASURED["fidelity"] * scale
  assert got.trace_distance <= 8 * DEPENDENT_MEASURED["trace_distance_equal"] * scale
  assert abs(got.overlap - got.purity_a) <= 8 * DEPENDENT_MEASURED["overlap"] * scale


def test_restatement_hand_checks():
  rng = np.random.default_rng(2)
  a = rng.normal(size=(3, 8)) + 1j * rng.normal(size=(3, 8))
  b = rng.normal(size=(2, 8)) + 1j * rng.normal(size=(2, 8))
  t = rng.normal(size=8)
  c = X.cross_gram(a, b, t)
  assert c.shape == (3, 2)
  np.testing.assert_allclose(c[1, 0], np.sum(t * np.conj(a[1]) * b[0]), atol=1e-14)
  np.testing.assert_allclose(X.cross_gram(b, a, t), c.conj().T, atol=1e-14)
  np.testing.assert_allclose(X.cross_gram(a, a, t), R.gram(a, t), atol=1e-14)
  np.testing.assert_allclose(X.cross_gram_bound(a, a, t), R.gram_bound(a, t), atol=1e-14)
  assert np.all(np.abs(c.real) <= X.cross_gram_bound(a, b, t) + 1e-15) and np.all(np.abs(c.imag) <= X.cross_gram_bound(a, b, t) + 1e-15)
  # basis states: C picks the table's entry
  eye = np.eye(8)
  np.testing.assert_array_equal(X.cross_gram(eye[:3], eye[1:4], t), np.diag(t[1:3], -1)[:3, :3].astype(np.complex128))
  # one pure state against another: fidelity |<a|b>|^2, distance sqrt(1 - F)
  u, v = a[0] / np.linalg.norm(a[0]), b[0] / np.linalg.norm(b[0])
  got = EM.metrics_from_grams(R.gram(u[None]), R.gram(v[None]), X.cross_gram(u[None], v[None]), [1.0], [1.0])
  fid = abs(np.vdot(u, v))**2
  np.testing.assert_allclose([got.fidelity, got.overlap, got.trace_distance], [fid, fid, np.sqrt(1 - fid)], atol=1e-14)


def test_host_refusals_of_the_metrics():
  g = np.eye(2)
  with pytest.raises(ValueError, match="negative"):
    EM.metrics_from_grams(g, g, g, [0.5, -0.5], [0.5, 0.5])
  with pytest.raises(ValueError, match="do not fit"):
    EM.metrics_from_grams(g, g, np.ones((2, 3)), [0.5, 0.5], [0.5, 0.5])


# ---- the entry points, without a device ------------------------------------------------------------------------------------
NEW_SYMBOLS = ("qhbm_cross_gram_scratch_bytes", "qhbm_cross_gram")


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
  assert inference.cross_gram is E.cross_gram
  for name in ("cross_gram", "ensemble_metrics", "matrix_elements", "EnsembleMetrics"):
    assert name in inference.__all__ and hasattr(inference, name)


def test_scratch_size_needs_no_device_and_refuses_bad_shapes():
  from qhbmlib_amd import _engine as E  # pylint: disable=import-outside-toplevel
  # 16 bytes per pair and slice; gram.hip's slices: 2^n / 2048, at least 1, at most 256
  for num_a, num_b, n, slices in [(1, 1, 1, 1), (5, 3, 10, 1), (5, 3, 11, 1), (5, 3, 12, 2), (5, 3, 13, 4), (8, 8, 19, 256),
                                  (32, 2, 24, 256), (1024, 1024, 31, 256)]:
    assert E.cross_gram_scratch_bytes(num_a, num_b, n) == 16 * num_a * num_b * slices
    assert E.gram_scratch_bytes(num_a, n) == 16 * num_a * num_a * slices  # (the same slices as qhbm_weighted_gram)
  lib = E.load_library()
  out = ctypes.c_size_t()
  for args, text in [((0, 1, 6), "M must be in [1, 1024]"), ((1025, 1, 6), "M must be in"), ((-1, 1, 6), "M must be in"),
                     ((1, 0, 6), "K must be in [1, 1024]"), ((1, 1025, 6), "K must be in"), ((1, -1, 6), "K must be in"),
                     ((1, 1, 0), "n_qubits must be in [1, 31]"), ((1, 1, 32), "n_qubits must be in [1, 31]")]:
    assert lib.qhbm_cross_gram_scratch_bytes(*args, ctypes.byref(out)) != 0
    assert text in lib.qhbm_last_error(None).decode(), (args, lib.qhbm_last_error(None).decode())
  assert lib.qhbm_cross_gram_scratch_bytes(1, 1, 6, None) != 0
  assert "out is NULL" in lib.qhbm_last_error(None).decode()


def test_the_call_refuses_before_it_touches_a_device():
  """Every refusal of qhbm_cross_gram comes before anything is launched, so it can be asked for without a GPU: the
  pointers are never followed."""
  from qhbmlib_amd import _engine as E  # pylint: disable=import-outside-toplevel
  lib = E.load_library()
  good = dict(a=0x10000, m=4, b=0x20000, k=3, n=6, t=0x30000, w=0x40000, o=0x50000)
  refused = [(dict(m=0), "M must be"), (dict(m=1025), "M must be"), (dict(k=0), "K must be"), (dict(k=1025), "K must be"),
             (dict(n=0), "n_qubits"), (dict(n=32), "n_qubits"), (dict(a=None), "d_bras is NULL"), (dict(b=None), "d_kets is NULL"),
             (dict(w=None), "d_scratch is NULL"), (dict(o=None), "d_out is NULL"), (dict(a=0x10008), "d_bras must be 16-byte"),
             (dict(b=0x20008), "d_kets must be 16-byte"), (dict(t=0x30004), "d_table must be 8-byte"),
             (dict(w=0x40004), "d_scratch must be 8-byte"), (dict(o=0x50004), "d_out must be 8-byte")]
  for change, text in refused:
    c = dict(good, **change)
    assert lib.qhbm_cross_gram(c["a"], c["m"], c["b"], c["k"], c["n"], c["t"], c["w"], c["o"], None) != 0, change
    assert text in lib.qhbm_last_error(None).decode(), (change, lib.qhbm_last_error(None).decode())
  with pytest.raises(E.EngineError, match="CUDA bras"):
    E.cross_gram(torch.zeros((1, 4), dtype=torch.complex64), torch.zeros((1, 4), dtype=torch.complex64))
  with pytest.raises(E.EngineError, match="CUDA bras"):
    E.cross_gram(np.zeros((1, 4)), np.zeros((1, 4)))


def test_translation_unit_compiles_alone_without_floating_point_atomics_or_scratch():
  """cross_gram.hip compiles on its own with the product's flags; its gfx950 assembly holds no floating-point atomic and no
  kernel of it uses scratch memory (no spills, no dynamic indexing of the register tiles).  It is part of observable.o, and
  of no other object."""
  hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
  assert os.path.exists(hipcc), "no hipcc"
  run = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-mllvm",
                        "-disable-promote-alloca-to-vector=1", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "--cuda-device-only",
                        "-S", "cross_gram.hip", "-o", "-"], cwd=CSRC, capture_output=True, text=True, timeout=900)
  assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
  asm = run.stdout
  kernels = re.findall(r"^(_ZN4qhbm\S*cross_gram_(?:tile|finish)_kernel\S*):", asm, flags=re.M)
  assert len(set(kernels)) == 33, sorted(set(kernels))  # 4 x 4 tile shapes, with and without a table, and the finish kernel
  assert "v_fma_f64" in asm and "global_load_dwordx4" in asm
  assert not re.search(r"\b(?:global|buffer|flat)_atomic_(?:pk_)?add_(?:f16|bf16|f32|f64)\b|\bds_(?:pk_)?add(?:_rtn)?_(?:f16|bf16|f32|f64)\b",
                       "\n".join(line.split(";")[0] for line in asm.splitlines()))
  sizes = [int(v) for v in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
  assert len(sizes) >= 33 and all(v == 0 for v in sizes), sizes
  with open(os.path.join(CSRC, "observable.hip")) as f:
    assert '#include "cross_gram.hip"' in f.read()
  with open(os.path.join(CSRC, "states.hip")) as f:
    assert "cross_gram" not in f.read()
