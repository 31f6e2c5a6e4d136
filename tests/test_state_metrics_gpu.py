"""The weighted Gram kernel (csrc/gram.hip) and `inference.state_metrics` on the GPU.

1. `qhbm_weighted_gram` against `tests/state_metrics_ref.gram` on the same complex64 states, with the scratch pre-filled
   with NaN.  Bound, per part, derived and not tuned: every product is exact in float64 (24 x 24 bits, the table's 24 more
   go into the column operand first: 48), so each of the 2^(n+1) terms of a part meets one rounding per addition on its
   way through the thread's chain, the shuffle tree, the waves and the slices -- at most 2^(n+1) + a few of them, each
   relative 2^-53 to a partial sum no larger than sum_x |t| |s_i| |s_j|.  The reference's own float64 sum is allowed as
   much: |dG| <= 4 (2^n + 4) 2^-53 sum_x |t(x)| |s_i(x)| |s_j(x)|.
2. `state_metrics` against the dense route at n = 4 and 6: fidelity rtol 1e-4 (the project's and the reference's
   close_rtol) against `inference.fidelity` and the oracle's direct sqrtm formula; cross and relative entropy against the
   complex128 restatement within the project's expectation tolerance with max |E| as the operator norm, 1e-5 max |E|;
   entropy, purity and trace, which depend on the data alone, 1e-6 absolute.
3. `table="transform"` against `"terms"`, same tolerances (the tables differ by float32 roundings).
4. One use at 20 qubits: internal consistency only.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import data, inference, ir, models
from tests import energy_table_ref
from tests import state_metrics_ref as R
from tests.test_host_api import hea_circuit

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 3), (5, 4), (10, 5), (11, 9), (12, 8), (13, 17)]
TABLES = ["none", "positive", "signed"]


def _raw_gram(states, table=None):
  """qhbm_weighted_gram through the C ABI on a NaN-filled scratch: complex128 numpy [M, M]."""
  lib = E.load_library()
  num, dim = states.shape
  n = dim.bit_length() - 1
  scratch = torch.full((E.gram_scratch_bytes(num, n) // 8,), float("nan"), dtype=torch.float64, device="cuda")
  out = torch.full((num, num, 2), float("nan"), dtype=torch.float64, device="cuda")
  rc = lib.qhbm_weighted_gram(states.data_ptr(), num, n, None if table is None else table.data_ptr(), scratch.data_ptr(),
                              out.data_ptr(), torch.cuda.current_stream().cuda_stream)
  assert rc == 0, lib.qhbm_last_error(None).decode()
  got = out.cpu().numpy()
  return got[..., 0] + 1j * got[..., 1]


@functools.lru_cache(maxsize=None)
def _case(n, num):
  """(complex64 states, {table name: float32 table or None}) as numpy, one draw per shape."""
  rng = np.random.default_rng(100 * n + num)
  dim = 1 << n
  states = ((rng.normal(size=(num, dim)) + 1j * rng.normal(size=(num, dim))) / np.sqrt(2 * dim)).astype(np.complex64)
  signed = rng.normal(size=dim) * 10.0**rng.uniform(-6, 6, dim)   # both magnitudes << 1 and >> 1, both signs
  return states, {"none": None, "positive": rng.uniform(0.05, 1.0, dim).astype(np.float32), "signed": signed.astype(np.float32)}


def _bits(a):
  return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("n,num", SHAPES)
def test_gram_kernel_matches_the_float64_restatement(n, num, table):
  states, tables = _case(n, num)
  t = tables[table]
  d_states = torch.from_numpy(states).cuda()
  d_table = None if t is None else torch.from_numpy(t).cuda()
  got = _raw_gram(d_states, d_table)
  want = R.gram(states, t)
  bound = 4.0 * ((1 << n) + 4) * 2.0**-53 * R.gram_bound(states, t)
  err_re, err_im = np.abs(got.real - want.real), np.abs(got.imag - want.imag)
  print(f"n={n} M={num} {table}: worst re {np.max(err_re / bound):.3g} im {np.max(err_im / bound):.3g} of the bound")
  assert np.all(np.isfinite(got.real)) and np.all(np.isfinite(got.imag))
  assert np.all(err_re <= bound) and np.all(err_im <= bound)
  # Hermitian bit for bit, the diagonal exactly real, and the same bits from a second call
  assert np.array_equal(_bits(got.real), _bits(got.real.T))
  assert np.all(np.diagonal(got).imag == 0.0)
  off = ~np.eye(num, dtype=bool)
  assert np.array_equal(_bits(got.imag[off]), _bits((-got.imag.T)[off]))
  again = _raw_gram(d_states, d_table)
  assert np.array_equal(_bits(got.real), _bits(again.real)) and np.array_equal(_bits(got.imag), _bits(again.imag))
  # the binding: same kernel, its own scratch
  bound_call = E.weighted_gram(d_states, d_table).cpu().numpy()
  assert bound_call.dtype == np.complex128
  assert np.array_equal(_bits(bound_call.real), _bits(got.real)) and np.array_equal(_bits(bound_call.imag), _bits(got.imag))


@pytest.mark.parametrize("table", TABLES)
def test_an_entry_does_not_depend_on_the_company_it_keeps(table):
  """G[2, 6] of eight states (a full 4 x 4 tile off the diagonal) = G[0, 1] of those two alone (a 2 x 2 tail tile)."""
  states, tables = _case(12, 8)
  t = tables[table]
  d_table = None if t is None else torch.from_numpy(t).cuda()
  full = _raw_gram(torch.from_numpy(states).cuda(), d_table)
  pair = _raw_gram(torch.from_numpy(np.ascontiguousarray(states[[2, 6]])).cuda(), d_table)
  assert _bits(full[2, 6].real) == _bits(pair[0, 1].real) and _bits(full[2, 6].imag) == _bits(pair[0, 1].imag)
  assert _bits(full[2, 2].real) == _bits(pair[0, 0].real) and _bits(full[6, 6].real) == _bits(pair[1, 1].real)


@pytest.mark.parametrize("n", [20, 21])
def test_random_sign_states_have_an_exact_norm(n):
  """Every part of `random_states` is +-mag, mag = float32(2^-(n+1)/2), so each float64 product is mag^2 exactly and
  every partial sum k mag^2 on the way is representable: G_1[i, i] = 2^(n+1) mag^2 with NO rounding.  At n = 21 mag is a
  power of two and that is 1.0; at n = 20 mag = float32(sqrt(1/2)) 2^-10 and it is (2 float32(sqrt(1/2))^2), 6e-8
  below 1 -- the exact value either way.  Off-diagonals against float64 torch on the device, within the kernel's bound."""
  states = E.random_states(4, n, 11)
  got = E.weighted_gram(states)
  mag = float(np.float32(np.sqrt(0.5) if n % 2 == 0 else 1.0)) * 2.0**-((n + 1) // 2)
  assert abs(float(states[0, 0].real)) == mag
  exact = 2.0**(n + 1) * (mag * mag)
  if n % 2:
    assert exact == 1.0
  diag = got.diagonal().cpu()
  print(f"n={n}: diagonal {diag.real.tolist()} exact {exact!r}")
  assert torch.all(diag.real == exact) and torch.all(diag.imag == 0.0)
  wide = states.to(torch.complex128)
  want = wide.conj() @ wide.transpose(0, 1)
  magnitudes = states.abs().to(torch.float64)
  bound = 4.0 * ((1 << n) + 4) * 2.0**-53 * (magnitudes @ magnitudes.transpose(0, 1))
  assert torch.all((got.real - want.real).abs() <= bound) and torch.all((got.imag - want.imag).abs() <= bound)


def test_refused_arguments_return_a_status_and_launch_nothing():
  lib = E.load_library()
  states = torch.ones((4, 64), dtype=torch.complex64, device="cuda")
  table = torch.ones(66, dtype=torch.float32, device="cuda")
  scratch = torch.zeros(E.gram_scratch_bytes(4, 6) // 8 + 1, dtype=torch.float64, device="cuda")
  out = torch.full((4 * 4 * 2 + 1,), -7.0, dtype=torch.float64, device="cuda")
  stream = torch.cuda.current_stream().cuda_stream
  good = dict(s=states.data_ptr(), m=4, n=6, t=table.data_ptr(), w=scratch.data_ptr(), g=out.data_ptr())
  refused = [dict(m=0), dict(m=-1), dict(m=1025), dict(n=0), dict(n=32), dict(s=None), dict(w=None), dict(g=None),
             dict(s=states.data_ptr() + 8), dict(t=table.data_ptr() + 4), dict(w=scratch.data_ptr() + 4),
             dict(g=out.data_ptr() + 4)]
  for change in refused:
    a = dict(good, **change)
    rc = lib.qhbm_weighted_gram(a["s"], a["m"], a["n"], a["t"], a["w"], a["g"], stream)
    assert rc != 0, change
    assert lib.qhbm_last_error(None).decode()
  size = ctypes.c_size_t()
  for m, n in [(0, 6), (1025, 6), (4, 0), (4, 32)]:
    assert lib.qhbm_gram_scratch_bytes(m, n, ctypes.byref(size)) != 0
  assert lib.qhbm_gram_scratch_bytes(4, 6, None) != 0
  torch.cuda.synchronize()
  assert torch.all(out == -7.0) and torch.all(scratch == 0.0)
  with pytest.raises(E.EngineError):
    E.weighted_gram(states.cpu())
  with pytest.raises(ValueError):
    E.weighted_gram(states, table)   # 66 entries for 64 amplitudes


# ---- state_metrics against the dense route ----------------------------------------------------------------------------
def _set(param, values):
  with torch.no_grad():
    param.copy_(torch.as_tensor(np.asarray(values), dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _model(n, kind, device="cpu"):
  """(Hamiltonian, oracle unitary complex128, float64 energies): an HEA circuit and an energy without bit-reversal or
  bit-flip symmetry, so that a bit-order mistake shows.  The energy's variables on `device` (the dense route evaluates
  the energy on the CPU, the transform table needs them on the GPU)."""
  qubits = ir.GridQubit.rect(1, n)
  rng = np.random.default_rng(40 + n)
  raw = hea_circuit(qubits, 2, f"sm{n}{kind}")
  circ = models.DirectQuantumCircuit(raw)
  phis = rng.uniform(-1, 1, len(circ.symbol_names))
  _set(circ.trainable_variables[0], phis)
  unitary = O.unitary(n, raw.flat_gates(circ.qubits, circ.symbol_names), phis)
  if kind == "kobe":
    energy = models.KOBE(list(range(n)), 2)
    energy.build([None, n])
    thetas = rng.uniform(-1, 1, energy.trainable_variables[0].shape)
    _set(energy.trainable_variables[0], thetas)
    energies = O.kobe_energy(O.all_bitstrings(n), thetas, 2)
  else:
    # (energies of shape [2^n], as the dense route's `probabilities` takes them)
    energy = models.BitstringEnergy(list(range(n)), energy_table_ref.mlp_layers(n, 5, 7 + n) + [torch.nn.Flatten(0)])
    energies = energy_table_ref.mlp_table_f64(energy, n)[0].detach().numpy()
  energy.to(device)
  return models.Hamiltonian(energy, circ), unitary, np.asarray(energies, dtype=np.float64).reshape(-1)


def _sigma(n, rank, seed):
  rng = np.random.default_rng(seed)
  a = rng.normal(size=(1 << n, rank)) + 1j * rng.normal(size=(1 << n, rank))
  sigma = a @ a.conj().T
  return sigma / np.trace(sigma).real


def _datasets(n):
  """name -> (StateVectorData, dense sigma complex128)"""
  rng = np.random.default_rng(70 + n)
  out = {}
  for name, rank in (("full_rank", 1 << n), ("rank_3", 3)):
    sigma = _sigma(n, rank, 3 * n + rank)
    out[name] = (data.StateVectorData.from_density_matrix(torch.from_numpy(sigma)), sigma)
  # neither orthogonal nor normalised, with weights; norms and weights keep tr sigma below 1
  states = rng.normal(size=(5, 1 << n)) + 1j * rng.normal(size=(5, 1 << n))
  states *= rng.uniform(0.5, 1.0, (5, 1)) / np.linalg.norm(states, axis=1, keepdims=True)
  weights = rng.uniform(0.05, 0.2, 5)
  out["weighted"] = (data.StateVectorData(torch.from_numpy(states), torch.from_numpy(weights)), R.dense_sigma(states, weights))
  return out


def _hold(got, want, e_max, label):
  energy_bar = 1e-5 * e_max
  print(f"{label}: " + " ".join(f"{k} {getattr(got, k):.9g} ({getattr(got, k) - want[k]:+.2g})" for k in want))
  np.testing.assert_allclose(got.cross_entropy, want["cross_entropy"], rtol=0, atol=energy_bar)
  np.testing.assert_allclose(got.relative_entropy, want["relative_entropy"], rtol=0, atol=energy_bar)
  for key in ("entropy", "purity", "trace"):
    np.testing.assert_allclose(getattr(got, key), want[key], rtol=0, atol=1e-6)
  np.testing.assert_allclose(got.log_partition, want["log_partition"], rtol=0, atol=energy_bar)
  np.testing.assert_allclose(got.overlap, want["overlap"], rtol=1e-4)


@pytest.mark.parametrize("kind", ["kobe", "mlp"])
@pytest.mark.parametrize("n", [4, 6])
def test_state_metrics_match_the_dense_route(n, kind):
  model, unitary, energies = _model(n, kind)
  e_max = float(np.abs(energies).max())
  p = np.exp(-energies - np.max(-energies))
  rho = (unitary * (p / p.sum())[None, :]) @ unitary.conj().T
  for name, (source, sigma) in _datasets(n).items():
    got = inference.state_metrics(model, source)
    assert all(isinstance(v, float) for v in (got.trace, got.purity, got.entropy, got.overlap, got.fidelity,
                                              got.log_partition, got.cross_entropy, got.relative_entropy))
    want = R.metrics(unitary, energies, source.states.numpy(), source.weights.numpy())
    _hold(got, want, e_max, f"n={n} {kind} {name}")
    direct = O.fidelity_direct(rho, sigma)
    dense = float(inference.fidelity(model, torch.from_numpy(sigma)).detach())
    print(f"  fidelity {got.fidelity:.9g} direct {direct:.9g} dense route {dense:.9g}")
    np.testing.assert_allclose(got.fidelity, direct, rtol=1e-4)
    np.testing.assert_allclose(got.fidelity, dense, rtol=1e-4)
    assert source.fidelity(model) == got.fidelity and source.relative_entropy(model) == got.relative_entropy
    assert source.entropy() == got.entropy
  if kind == "mlp":  # (what the cross entropy is for: the engine's expectation refuses a general energy)
    with pytest.raises(TypeError):
      source.expectation(model)


@pytest.mark.parametrize("n", [4, 6])
def test_the_models_own_eigen_ensemble_has_fidelity_one_and_no_relative_entropy(n):
  model, _, energies = _model(n, "kobe")
  source = data.StateVectorData.from_density_matrix(inference.density_matrix(model).detach().cpu())
  got = inference.state_metrics(model, source)
  print(f"n={n}: fidelity {got.fidelity!r} relative entropy {got.relative_entropy!r}")
  np.testing.assert_allclose(got.fidelity, 1.0, rtol=0, atol=1e-4)
  np.testing.assert_allclose(got.relative_entropy, 0.0, rtol=0, atol=1e-5 * float(np.abs(energies).max()))


@pytest.mark.parametrize("n", [4, 6])
def test_transform_table_gives_the_same_metrics_as_terms(n):
  model, _, energies = _model(n, "kobe", "cuda")
  e_max = float(np.abs(energies).max())
  for name, (source, _) in _datasets(n).items():
    terms = inference.state_metrics(model, source, table="terms")
    transform = inference.state_metrics(model, source, table="transform")
    want = {k: getattr(terms, k) for k in ("trace", "purity", "entropy", "overlap", "log_partition", "cross_entropy",
                                           "relative_entropy")}
    _hold(transform, want, e_max, f"n={n} {name} transform - terms")
    np.testing.assert_allclose(transform.fidelity, terms.fidelity, rtol=1e-4)


def test_state_metrics_refuse_what_does_not_fit():
  model, _, _ = _model(4, "kobe")
  states = torch.ones((2, 32), dtype=torch.complex64)
  with pytest.raises(ValueError, match="qubits"):
    inference.state_metrics(model, data.StateVectorData(states))
  elsewhere = [ir.GridQubit(1, c) for c in range(4)]
  with pytest.raises(ValueError, match="qubits"):
    inference.state_metrics(model, data.StateVectorData(states[:, :16], qubits=elsewhere))
  with pytest.raises(ValueError, match="max_qubits"):
    inference.state_metrics(model, data.StateVectorData(states[:, :16]), max_qubits=3)


def test_ground_state_data_at_twenty_qubits():
  """Internal consistency where no matrix can be formed: one state, so fidelity = overlap and S(sigma) = 0."""
  n = 20
  qubits = ir.GridQubit.rect(1, n)
  zz = ir.PZ(qubits[0]) * ir.PZ(qubits[1])
  for a, b in zip(qubits[1:-1], qubits[2:]):
    zz = zz + ir.PZ(a) * ir.PZ(b)
  xs = ir.PX(qubits[0])
  for q in qubits[1:]:
    xs = xs + ir.PX(q)
  source = data.StateVectorData.ground_state([zz, xs], weights=[-1.0, -1.0], num_steps=8, max_restarts=0, seed=3)
  rng = np.random.default_rng(20)
  energy = models.BernoulliEnergy(list(range(n)))
  energy.build([None, n])
  _set(energy.trainable_variables[0], rng.uniform(-0.3, 0.3, n))
  energy.to("cuda")
  circ = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "sm20"))
  _set(circ.trainable_variables[0], rng.uniform(-0.2, 0.2, len(circ.symbol_names)))
  got = inference.state_metrics(models.Hamiltonian(energy, circ), source)
  print(got)
  assert got.fidelity > 0.0
  np.testing.assert_allclose(got.fidelity, got.overlap, rtol=1e-6)
  np.testing.assert_allclose(got.entropy, 0.0, rtol=0, atol=1e-6)
  assert got.relative_entropy >= -1e-5
