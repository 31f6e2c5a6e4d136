"""The Krylov restatement (tests/krylov_ref.py) and the host side of `inference.krylov` against `eigh`, without a GPU.

What is checked here and why
  * the algorithm itself in float64: lengths, Ritz values, finite-temperature Lanczos, both evolutions (1e-12 .. 1e-9);
  * the product's host functions (`krylov.ritz`, `evolution_coefficients`, `ftlm_*`) on the restatement's (alpha, beta);
  * the conditions the GPU cases rest on: in the fp32 arithmetic no ||w|| / R of any case lies in [2^-19, 0.1], so the
    breakdown rule (<= 2^-16 R) decides the same way whatever the summation order.  Measured: legitimate steps >= 0.159
    (n = 3), exhausted steps <= 6.3e-7 (n = 3, local mode);
  * the bars of tests/test_krylov_gpu.py: fp32 restatement against its float64 run, the larger of the two modes,
        n = 3,  m = 8    alpha 4.4e-7   beta 3.3e-7   basis 5.6e-7
        n = 10, m = 12   alpha 5.9e-7   beta 4.7e-7   basis 1.0e-7
        n = 13, m = 8    alpha 2.5e-7   beta 3.3e-7   basis 5.8e-8
    and against `eigh` at n = 10, m = 48 (full / local): theta_min 1.4e-7 / 9.1e-8, theta_max 6.6e-8 / 1.0e-7, ground
    vector 1.5e-7 / 1.7e-7, e^{-beta H} states 1.0e-7 / 1.4e-7, log norms 5.9e-7 / 5.9e-7, e^{-itH} 1.1e-7 / 7.5e-8,
    |V^dagger V - I| 3.8e-8 (full).  Over 48 steps alpha and beta of the two precisions agree only to 1e-3 even with
    full reorthogonalisation (Lanczos coefficients stop being comparable once Ritz values converge): they are compared
    element-wise over 12 steps only;
  * the bars of the `thermal_sweep` tests: the fp32 restatement's finite-temperature Lanczos on those tests' own start
    vectors against `eigh`, the larger of the two modes and of beta = 0.5, 4,
        n = 3, all basis states          l_m 4.4e-7  log Z 3.5e-7  <H> 9.2e-8  S 2.1e-8  states 7.0e-8  ensemble <H> 1.7e-7
        n = 10, 4 vectors of seed 77     l_m 8.4e-7  log Z 5.2e-7  <H> 4.2e-7  S 2.8e-7  states 1.3e-7  ensemble <H> 2.3e-7
    while the float64 restatement is within 1e-12 of `eigh` on both.
Every comparison prints its figure beside its bar."""
import os

import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd.inference import krylov
from tests import krylov_cases as C
from tests import krylov_ref as K
from tests import thermal_ref as T


def _close(what, got, want, bar):
  err = float(np.max(np.abs(np.asarray(got) - np.asarray(want)), initial=0.0))
  print(f"{what}: max error {err:.3e}  bar {bar:.3e}")
  assert np.isfinite(np.asarray(got)).all() and err <= bar, (what, err, bar)


# ---- n = 3: exhausted spaces are exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorth", [True, False])
def test_n3_basis_starts_lengths_ritz_values_and_ftlm(reorth):
  n, m = 3, 8
  basis, alpha, beta, lengths, norms, _ = C.run(n, m, reorth, False)
  assert lengths.tolist() == [4, 6, 6, 6, 6, 6, 6, 4]
  d = C.dense(n)
  pairs = [krylov.ritz(alpha[u], beta[u], lengths[u]) for u in range(8)]
  for u, (theta, s) in enumerate(pairs):
    assert len(theta) == lengths[u] and np.allclose(theta, K.ritz(alpha[u], beta[u], lengths[u])[0], atol=0, rtol=0)
    _close(f"state {u} Ritz values against eigh", np.abs(theta[:, None] - d.evals[None, :]).min(axis=1), 0.0, 1e-12)
    assert (basis[lengths[u]:, u] == 0).all() and (alpha[u, lengths[u]:] == 0).all() and (beta[u, lengths[u] - 1:] == 0).all()
  lw = krylov.ftlm_log_weights(pairs, norms, C.BETAS)
  log_z = krylov.ftlm_log_partition(lw, n, "basis")
  energy = krylov.ftlm_energy(pairs, norms, C.BETAS)
  for b, value in enumerate(C.BETAS):
    _close(f"beta={value} log Z", log_z[b], d.log_partition(value), 1e-10)
    _close(f"beta={value} <H>", energy[b], d.energy(value), 1e-10)
    _close(f"beta={value} S", value * energy[b] + log_z[b], d.entropy(value), 1e-10)
  _close("log weights against the restatement's", lw, K.sweep_log_weights(alpha, beta, lengths, norms, C.BETAS), 1e-12)


# ---- n = 10, m = 48, float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorth", [True, False])
def test_n10_float64_ground_energy_and_both_evolutions(reorth):
  n, m = 10, 48
  basis, alpha, beta, lengths, norms, _ = C.run(n, m, reorth, False)
  d = C.dense(n)
  given = C.starts(n).astype(np.complex128)
  assert lengths.tolist() == [m] * 3
  pairs = [krylov.ritz(alpha[u], beta[u], lengths[u]) for u in range(3)]
  _close("E_0", [theta[0] for theta, _ in pairs], d.evals[0], 1e-9)
  for tau in C.BETAS:
    want, want_log = d.evolve(given, tau, 0)
    coef = np.zeros((3, 1, m), np.complex128)
    logs = np.zeros(3)
    for u, (theta, s) in enumerate(pairs):
      coef[u, 0], log_norm = krylov.evolution_coefficients(theta, s, tau, 0, m)
      logs[u] = log_norm + np.log(norms[u])
    got = K.combine(basis, coef)[:, 0]
    got /= np.linalg.norm(got, axis=1, keepdims=True)
    _close(f"tau={tau} states", got, want, 1e-9)
    _close(f"tau={tau} log norms", logs, want_log, 1e-9)
    _close(f"tau={tau} the restatement's evolve", K.evolve(basis, alpha, beta, lengths, norms, tau, 0)[0], want, 1e-9)
  for t in C.TIMES:
    want = d.evolve(given, t, 1)[0]
    coef = np.stack([krylov.evolution_coefficients(theta, s, t, 1, m)[0] * norms[u] for u, (theta, s) in enumerate(pairs)])[:, None]
    _close(f"t={t} states", K.combine(basis, coef)[:, 0], want, 1e-9)


# ---- what the GPU cases rest on -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reorth", [True, False])
@pytest.mark.parametrize("n,m", C.BASIS_CASES + ((10, 48),))
def test_no_step_of_a_gpu_case_is_near_the_breakdown_threshold(n, m, reorth):
  raw = C.run(n, m, reorth, True)[5] / T.radius(n, C.tfim_parts(n), C.WEIGHTS)
  lengths = C.run(n, m, reorth, True)[3]
  assert np.array_equal(lengths, C.run(n, m, reorth, False)[3])
  live = np.array([[j < lengths[u] for u in range(raw.shape[1])] for j in range(m)])  # (steps taken before the space ended)
  print(f"n={n} m={m} reorth={reorth}: smallest / largest ||w|| / R of live steps outside the gap:",
        raw[live & (raw >= 0.1)].min(initial=np.inf), raw[live & (raw < 2.0**-19)].max(initial=0.0))
  assert not ((raw[live] >= 2.0**-19) & (raw[live] <= 0.1)).any()


def test_the_bars_are_the_documented_ones():
  documented = {(3, 8): (4.4e-7, 3.3e-7, 5.6e-7), (10, 12): (5.9e-7, 4.7e-7, 1.0e-7), (13, 8): (2.5e-7, 3.3e-7, 5.8e-8)}
  for (n, m), want in documented.items():
    got = np.maximum(C.elementwise_errors(n, m, True), C.elementwise_errors(n, m, False))
    print(f"n={n} m={m}: fp32 restatement against float64 (alpha, beta, basis) {got}  documented {want}")
    assert (got > 0.5 * np.array(want)).all() and (got < 2.0 * np.array(want)).all()
  long_run = float(np.abs(C.run(10, 48, True, True)[1] - C.run(10, 48, True, False)[1]).max())
  print(f"48 steps, full reorthogonalisation: alpha of the two precisions differs by {long_run:.2e}")
  assert 1e-5 < long_run < 1e-1
  documented = {True: dict(theta_min=1.4e-7, theta_max=6.6e-8, ground=1.5e-7, states=1.0e-7, log_norms=5.9e-7, real_time=1.1e-7, gram=3.8e-8),
                False: dict(theta_min=9.1e-8, theta_max=1.0e-7, ground=1.7e-7, states=1.4e-7, log_norms=5.9e-7, real_time=7.5e-8)}
  for reorth, want in documented.items():
    got = C.derived_errors(reorth)
    print(f"reorth={reorth}: fp32 restatement against eigh {got}")
    for key, value in want.items():
      assert 0.4 * value < got[key] < 2.5 * value, (reorth, key, got[key], value)


# ---- the byte model (needs the built library, no device) ----------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(E.LIB_PATH), reason="engine library not built (run __graft_entry__.build())")
def test_describe_krylov_needs_no_device():
  eng = E.Engine(None)
  eng.set_circuit(20, [], 0)
  eng.set_observables(C.tfim_parts(20))
  full, local = eng.describe_krylov(16, 64, True), eng.describe_krylov(16, 64, False)
  state = 8.0 * 2**20
  assert full["basis_bytes"] == local["basis_bytes"] == 64 * 16 * state == 2.0**33 and full["applications"] == 64
  # local: steps 1 .. 63 are one block of two rows (3 + 4 sweeps), step 0 of one (3 + 2), 63 normalised writes, the import
  assert local["krylov_bytes_per_state"] == (3 + 5 + 63 * 7 + 63 * 2) * state
  blocks = sum(-(-(j + 1) // 8) for j in range(64))
  assert full["krylov_bytes_per_state"] == (3 + 2 * (3 * blocks + 2 * sum(range(1, 65))) + 63 * 2) * state
  assert full["workspace_bytes"] == 2 * full["chunk_states"] * state
  with pytest.raises(E.EngineError, match="no device"):
    eng.krylov_basis(torch.zeros((1, 1 << 20), dtype=torch.complex64), 4)


def test_the_sweep_bars_are_the_documented_ones():
  documented = {"basis": dict(log_weights=4.4e-7, log_z=3.5e-7, energy=9.2e-8, entropy=2.1e-8, states=7.0e-8, ensemble_energy=1.7e-7),
                "random": dict(log_weights=8.4e-7, log_z=5.2e-7, energy=4.2e-7, entropy=2.8e-7, states=1.3e-7, ensemble_energy=2.3e-7)}
  for start, want in documented.items():
    got = C.sweep_errors(start)
    print(f"start={start}: fp32 restatement of the sweep against eigh {got}")
    for key, value in want.items():
      assert 0.4 * value < got[key] < 2.5 * value, (start, key, got[key], value)
    exact = C.sweep_exact(start)
    for reorth in (True, False):
      double = C.sweep_run(start, reorth, False)
      for name, a, b in zip(("l_m", "log Z", "<H>", "S", "states"), double, exact):
        _close(f"start={start} reorth={reorth} float64 {name}", a, b, 1e-12)
      _close(f"start={start} reorth={reorth} float64 ensemble <H>", double[5], exact[2], 1e-12)


def test_a_sweep_without_a_live_vector_has_no_energy():
  pairs, norms = [krylov.ritz(np.zeros(4), np.zeros(4), 0)] * 2, np.zeros(2)
  assert np.isnan(krylov.ftlm_energy(pairs, norms, C.BETAS)).all()
  assert (krylov.ftlm_log_partition(krylov.ftlm_log_weights(pairs, norms, C.BETAS), 3, "random") == -np.inf).all()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_new_kernels_are_in_the_resource_table_and_do_not_spill():
  import importlib.util
  spec = importlib.util.spec_from_file_location(
      "kernel_resources", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "kernel_resources.py"))
  module = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(module)
  rows = {r["name"]: r for r in module.resource_rows() if "krylov_" in r["name"]}
  names = set(rows)
  for count in range(1, 9):
    assert {f"krylov_project_kernel<{count}u>", f"krylov_subtract_kernel<{count}u, true>", f"krylov_subtract_kernel<{count}u, false>",
            f"krylov_combine_kernel<{count}u>"} <= names, sorted(names)
  assert sum(1 for name in names if name.endswith(("krylov_coef_kernel", "krylov_norm_kernel", "krylov_init_kernel"))) == 3
  for name, row in rows.items():
    assert module.default_selectable(name) and row.get("VGPRs Spill", 0) == 0 and row.get("ScratchSize", 0) == 0, (name, row)
