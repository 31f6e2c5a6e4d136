"""Streamed Lanczos without a GPU: the two-pass restatement (tests/krylov_stream_ref.py), the byte model of
`qhbm_describe_krylov_stream`, the resource table's rows of the replay kernel and the host logic of `store_basis=False`.

What is checked here and why
  * the algorithm: pass one on three vectors gives, bit for bit, the alpha, beta and lengths of `krylov_ref.lanczos(reorth=
    False)`, in float64 and in its fp32 mode; the replay regenerates, bit for bit, every row of that basis from the recorded
    pairs, and its outputs are the j-ascending sum over those rows.  In the fp32 mode that sum IS `krylov_ref.combine` and the
    outputs equal it exactly.  For a complex128 basis `krylov_ref.combine` is one `numpy.einsum`, whose order of summation is
    not j ascending (its result differs from the j-ascending sum over the SAME stored rows by up to 4.4e-16 on these cases):
    there the outputs equal the j-ascending sum over the stored rows exactly and `combine` within (m + 4) 2^-52 sum_j |c_j|
    max|v_j|, the rounding of two float64 sums of the same m products;
  * the byte model at 20 qubits, 16 states, m = 64, S in {1, 8, 9} against the formulas of DESIGN.md 6o, written out here;
  * `krylov_replay_kernel<SB, FIRST>`, SB = 1 .. 8, is in scripts/kernel_resources.py's table, default-selectable, and has
    no spill and no scratch;
  * `store_basis=False` refuses full reorthogonalisation, and a `StreamedKrylovSpace` answers `ritz()` and `residuals()` as
    a `KrylovSpace` does on the same alpha, beta and lengths."""
import functools
import os

import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd import inference
from qhbmlib_amd.inference import krylov
from tests import krylov_cases as C
from tests import krylov_ref as K
from tests import krylov_stream_ref as S

CASES = [(n, m) for n in (3, 10) for m in (12, 48)]


@functools.lru_cache(maxsize=None)
def streamed(n, m, single):
  """(alpha, beta, lengths, recurrence, norms) of pass one of the restatement on the case of `krylov_cases.run`."""
  return S.tridiagonal(n, C.tfim_parts(n), C.starts(n), m, C.WEIGHTS, np.float32 if single else np.float64)


def _coefficients(n, m, num):
  rng = np.random.default_rng(100 * n + m)
  return rng.normal(size=(num, 3, m)) + 1j * rng.normal(size=(num, 3, m))


# ---- 1. the two-pass restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("n,m", CASES)
def test_pass_one_on_three_vectors_is_the_local_recurrence(n, m, single):
  _, want_alpha, want_beta, want_lengths, want_norms, _ = C.run(n, m, False, single)
  alpha, beta, lengths, recurrence, norms = streamed(n, m, single)
  assert np.array_equal(alpha, want_alpha) and np.array_equal(beta, want_beta)
  assert np.array_equal(lengths, want_lengths) and lengths.dtype == np.int32 and np.array_equal(norms, want_norms)
  assert recurrence.shape == (len(lengths), m, 2) and recurrence.dtype == (np.complex64 if single else np.complex128)
  assert (recurrence[:, 0, 0] == 0).all()  # (the pair of step 0 is (0, c_0))
  # alpha_j is Re c_j before the coefficient was rounded
  assert np.array_equal(recurrence[:, :, 1].real, alpha.astype(recurrence.real.dtype))
  if n == 3:
    assert (lengths < m).all()  # (the case that has breakdowns)


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("n,m", CASES)
def test_the_replay_regenerates_the_basis_and_sums_it(n, m, single):
  dtype = np.float32 if single else np.float64
  basis = C.run(n, m, False, single)[0]
  _, beta, _, recurrence, _ = streamed(n, m, single)
  ops, starts = C.tfim_parts(n), C.starts(n)
  rows = np.stack(list(S.rows(n, ops, starts, beta, recurrence, C.WEIGHTS, dtype)))
  assert rows.dtype == basis.dtype and np.array_equal(rows, basis)
  coef = _coefficients(n, m, basis.shape[1])
  out = S.replay(n, ops, starts, beta, recurrence, coef, C.WEIGHTS, dtype)
  want = K.combine(basis, coef)
  assert out.shape == want.shape and out.dtype == want.dtype
  if single:
    assert np.array_equal(out, want)
    return
  ascending = np.zeros_like(want)
  for j in range(m):
    ascending = ascending + coef[:, :, j, None] * basis[j][:, None, :]
  assert np.array_equal(out, ascending)
  bar = (m + 4) * 2.0**-52 * np.einsum("usj,ju->us", np.abs(coef), np.abs(basis).max(axis=2))[:, :, None]
  err = np.abs(out - want)
  print(f"n={n} m={m} float64 outputs against combine's einsum: max {err.max():.3e}  bar {bar.min():.3e}")
  assert (err <= bar).all()


def test_one_hot_coefficients_pick_single_rows():
  n, m = 3, 12
  basis = C.run(n, m, False, True)[0]
  _, beta, _, recurrence, _ = streamed(n, m, True)
  coef = np.zeros((basis.shape[1], 4, m), np.complex64)
  picks = (0, 1, 2, m - 1)
  for s, j in enumerate(picks):
    coef[:, s, j] = 1
  out = S.replay(n, C.tfim_parts(n), C.starts(n), beta, recurrence, coef, C.WEIGHTS, np.float32)
  for s, j in enumerate(picks):
    assert np.array_equal(out[:, s], basis[j])


# ---- 2. the byte model (needs the built library, no device) ---------------------------------------------------------------------------
def _tridiagonal_sweeps(m):
  """The import 3; step 0 projects and subtracts one row (2 + 3), every later step two rows in one launch (3 + 4); the
  normalised write 2 except after the last step: the launches of the stored local route, on ring slots."""
  return 3 + 5 + (m - 1) * 7 + (m - 1) * 2


def _replay_sweeps(m, num_outputs):
  """Per group of sb <= 8 outputs: the import 3; step 0 subtracts one row (3), the scaled copy reads w and v_0 and writes v_1
  and the outputs (3 + sb); every later step subtracts two rows (4), the scaled copy reads w and the outputs and writes
  v_{j+1} and the outputs (2 + 2 sb)."""
  total = 0
  for s0 in range(0, num_outputs, 8):
    sb = min(8, num_outputs - s0)
    total += 3 + (6 + sb) + (m - 2) * (6 + 2 * sb)
  return total


@pytest.mark.skipif(not os.path.exists(E.LIB_PATH), reason="engine library not built (run __graft_entry__.build())")
def test_describe_krylov_stream_needs_no_device():
  eng = E.Engine(None)
  eng.set_circuit(20, [], 0)
  eng.set_observables(C.tfim_parts(20))
  state, m = 8.0 * 2**20, 64
  assert eng.describe_krylov(16, m, False)["krylov_bytes_per_state"] == _tridiagonal_sweeps(m) * state
  for num_outputs in (1, 8, 9):
    got = eng.describe_krylov_stream(16, m, num_outputs)
    assert set(got) == {"workspace_bytes", "chunk_states", "tridiagonal_applications", "replay_applications",
                        "tridiagonal_bytes_per_state", "replay_bytes_per_state"}
    assert got["tridiagonal_applications"] == m and got["replay_applications"] == (m - 1) * -(-num_outputs // 8)
    assert got["tridiagonal_bytes_per_state"] == _tridiagonal_sweeps(m) * state
    assert got["replay_bytes_per_state"] == _replay_sweeps(m, num_outputs) * state
    assert got["workspace_bytes"] == 5 * got["chunk_states"] * state and got["chunk_states"] == 16
  assert _replay_sweeps(m, 1) == 3 + 7 + 62 * 8 and _replay_sweeps(m, 9) == _replay_sweeps(m, 8) + _replay_sweeps(m, 1)
  # per step 6 + 2 SB sweeps where subtract, scaled copy and accumulate apart would take 7 + 2 SB
  assert _replay_sweeps(m, 8) - _replay_sweeps(m - 1, 8) == 6 + 2 * 8
  assert eng.describe_krylov_stream(16, 8)["workspace_bytes"] == eng.describe_krylov_stream(16, 1024)["workspace_bytes"]
  assert eng.describe_krylov_stream(16, 1, 9)["replay_bytes_per_state"] == (3 + 2 + 9) * state
  for bad, text in (((16, 0, 1), "m must be in"), ((16, 1025, 1), "m must be in"), ((0, 8, 1), "U must be positive"),
                    ((16, 8, 0), "S must be at least 1")):
    with pytest.raises(E.EngineError, match=text):
      eng.describe_krylov_stream(*bad)
  start = torch.zeros((1, 1 << 20), dtype=torch.complex64)
  with pytest.raises(E.EngineError, match="no device"):
    eng.krylov_tridiagonal(start, 4)
  with pytest.raises(E.EngineError, match="no device"):
    eng.krylov_replay(start, torch.ones((1, 4), dtype=torch.float64), torch.full((1,), 4, dtype=torch.int32),
                      torch.zeros((1, 4, 2), dtype=torch.complex64), torch.ones((1, 1, 4), dtype=torch.complex64))
  for sym in ("qhbm_krylov_tridiagonal", "qhbm_krylov_replay", "qhbm_describe_krylov_stream"):
    assert sym in E.ABI_SYMBOLS and hasattr(E.load_library(), sym), sym


# ---- 3. the resource table ---------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_replay_kernels_are_in_the_resource_table_and_do_not_spill():
  import importlib.util
  spec = importlib.util.spec_from_file_location(
      "kernel_resources", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "kernel_resources.py"))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  rows = {r["name"]: r for r in module.resource_rows() if "krylov_replay_kernel" in r["name"]}
  assert set(rows) == {f"krylov_replay_kernel<{count}u, {first}>" for count in range(1, 9) for first in ("true", "false")}, sorted(rows)
  for name, row in rows.items():
    assert module.default_selectable(name) and row.get("VGPRs Spill", 0) == 0 and row.get("SGPRs Spill", 0) == 0, (name, row)
    assert row.get("ScratchSize", 0) == 0 and row.get("LDS Size", 0) == 0, (name, row)


# ---- 4. host logic -----------------------------------------------------------------------------------------------------------------------
def test_store_basis_false_refuses_full_reorthogonalisation():
  # (the refusal comes before any engine is opened: no device needed)
  for call in (lambda: inference.krylov_space([], store_basis=False, reorthogonalise=True),
               lambda: inference.thermal_sweep([], [1.0], store_basis=False, reorthogonalise=True),
               lambda: inference.ground_state([], store_basis=False, reorthogonalise=True),
               lambda: inference.spectrum_extremes([], store_basis=False, reorthogonalise=True)):
    with pytest.raises(ValueError, match="full reorthogonalisation"):
      call()
  assert krylov._reorthogonalise(None, True) is True and krylov._reorthogonalise(None, False) is False  # pylint: disable=protected-access
  assert krylov._reorthogonalise(False, True) is False and krylov._reorthogonalise(False, False) is False  # pylint: disable=protected-access


def test_a_streamed_space_answers_from_t_as_a_stored_one():
  n, m = 10, 12
  basis, alpha, beta, lengths, norms, _ = C.run(n, m, False, True)
  lengths = lengths.copy()
  lengths[1] = 7  # (a breakdown, as the device would report it: beta and alpha zero from there)
  alpha, beta = alpha.copy(), beta.copy()
  alpha[1, 7:], beta[1, 6:] = 0, 0
  tensors = [torch.from_numpy(a) for a in (alpha, beta, lengths, norms)]
  stored = inference.KrylovSpace(None, None, list(range(n)), torch.from_numpy(basis), *tensors, 17.0)
  space = inference.StreamedKrylovSpace(None, None, list(range(n)), None, tensors[0], tensors[1], tensors[2], None, tensors[3], 17.0)
  assert isinstance(space, inference.KrylovSpace) and space.basis is None and space.replays == 0
  assert space.num_steps == stored.num_steps == m and space.num_vectors == stored.num_vectors == 3 and space.num_qubits == n
  assert space.radius == 17.0 and np.array_equal(space.alpha, alpha) and np.array_equal(space.beta, beta)
  assert np.array_equal(space.lengths, lengths) and np.array_equal(space.norms, norms)
  for (theta, s), (want_theta, want_s) in zip(space.ritz(), stored.ritz()):
    assert np.array_equal(theta, want_theta) and np.array_equal(s, want_s)
  assert [len(theta) for theta, _ in space.ritz()] == [12, 7, 12]
  for got, want in zip(space.residuals(), stored.residuals()):
    assert np.array_equal(got, want)
  sweep, want_sweep = krylov.ThermalSweep(space, C.BETAS, "random"), krylov.ThermalSweep(stored, C.BETAS, "random")
  assert np.array_equal(sweep.log_partition(), want_sweep.log_partition()) and np.array_equal(sweep.energy(), want_sweep.energy())
  assert np.array_equal(sweep.entropy(), want_sweep.entropy()) and space.replays == 0
