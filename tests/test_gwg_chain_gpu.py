"""qhbm_gwg_sample -- whole Gibbs-With-Gradients chains of a spin-parity energy inside one wave -- against the numpy
restatement tests/gwg_ref.py, and GibbsWithGradientsInference(chain="device") on top of it.

The exact cases use dyadic theta, so every h_j is exact in fp32, and seeds for which the restatement has no step within
delta of a decision boundary (tests/gwg_ref.py derives delta; tests/test_gwg_ref_cpu.py asserts the condition): every
sample, every final state and every accepted count must EQUAL the restatement's.  The invariances (cutting a run into
calls, the number of chains launched, repeats) hold bit for bit for any theta."""
import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd import inference, ir, models
from tests import gwg_ref as R
from tests.test_host_api import hea_circuit

pytestmark = pytest.mark.gpu


def _i64(a):
  return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def _run(states, n_bits, masks, thetas, seed, step0, n_steps, write=True):
  """(samples or None, final states uint64, accepted) of one call."""
  st = _i64(states)
  out, acc = E.gwg_sample(st, n_bits, _i64(masks), torch.from_numpy(np.asarray(thetas, np.float32)).cuda(), seed, step0,
                          n_steps, write_samples=write, count_accepted=True)
  return (None if out is None else out.cpu().numpy()), st.cpu().numpy().view(np.uint64), acc.cpu().numpy()


@pytest.mark.parametrize("name", sorted(R.EXACT_SEEDS))
def test_exact_cases_equal_the_restatement(name):
  c = R.exact_case(name)
  want = R.run(c["states"], c["n_bits"], c["masks"], c["thetas"], c["seed"], 0, c["n_steps"])
  assert int(want["ambiguous"].sum()) == 0
  got, states, accepted = _run(c["states"], c["n_bits"], c["masks"], c["thetas"], c["seed"], 0, c["n_steps"])
  assert got.shape == want["samples"].shape and got.dtype == np.int8
  np.testing.assert_array_equal(got, want["samples"])
  np.testing.assert_array_equal(states, want["states"])
  np.testing.assert_array_equal(accepted, want["accepted"])
  if name == "theta0_n7":            # every proposal accepted: a pure index walk
    assert np.all(accepted == c["n_steps"])
  if name == "theta128_n5":          # from the highest-energy state down to the ground state, and no step out of it
    assert np.all(states == 31) and np.all(accepted == 5)
    assert np.all(got[5:] == 1) and set(np.unique(got)) <= {0, 1}


def _random_problem(n, order, chains, seed):
  rng = np.random.default_rng(seed)
  masks = R.kobe_masks(n, order)
  thetas = rng.normal(size=masks.size).astype(np.float32) * 0.3
  states = rng.integers(0, 2**63, size=chains, dtype=np.uint64) & np.uint64(2**n - 1)
  return masks, thetas, states


@pytest.mark.parametrize("first_written", [True, False])
def test_one_call_equals_two_calls_chained_by_step0(first_written):
  n, t1, t2 = 20, 100, 156
  masks, thetas, states = _random_problem(n, 2, 5, seed=2)
  whole, s_whole, a_whole = _run(states, n, masks, thetas, 77, 1000, t1 + t2)
  first, s_mid, a1 = _run(states, n, masks, thetas, 77, 1000, t1, write=first_written)
  assert (first is None) == (not first_written)
  second, s_end, a2 = _run(s_mid, n, masks, thetas, 77, 1000 + t1, t2)
  if first_written:
    assert first.tobytes() == whole[:t1].tobytes()
  assert second.tobytes() == whole[t1:].tobytes()
  np.testing.assert_array_equal(s_end, s_whole)
  np.testing.assert_array_equal(a1 + a2, a_whole)
  np.testing.assert_array_equal(R.pack(whole[-1]), s_whole)      # the last row IS the final state


def test_a_run_longer_than_a_launch_slice_equals_its_pieces():
  """65 536 steps per launch: 65 536 + 700 steps in one call (two launches) against 40 000 unwritten + the rest."""
  n, total, t1 = 5, 65536 + 700, 40000
  masks, thetas, states = _random_problem(n, 2, 2, seed=3)
  whole, s_whole, a_whole = _run(states, n, masks, thetas, 5, 2**32 - 3000, total)   # (the step counter's high word too)
  _, s_mid, a1 = _run(states, n, masks, thetas, 5, 2**32 - 3000, t1, write=False)
  rest, s_end, a2 = _run(s_mid, n, masks, thetas, 5, 2**32 - 3000 + t1, total - t1)
  assert rest.tobytes() == whole[t1:].tobytes()
  np.testing.assert_array_equal(s_end, s_whole)
  np.testing.assert_array_equal(a1 + a2, a_whole)
  assert 0 < a_whole.min() and a_whole.max() < total


def test_a_chain_does_not_depend_on_how_many_are_launched():
  n, steps = 12, 64
  masks, thetas, states = _random_problem(n, 2, 130, seed=4)
  many, s_many, a_many = _run(states, n, masks, thetas, 9, 0, steps)
  few, s_few, a_few = _run(states[:3], n, masks, thetas, 9, 0, steps)
  assert few.tobytes() == np.ascontiguousarray(many[:, :3]).tobytes()
  np.testing.assert_array_equal(s_few, s_many[:3])
  np.testing.assert_array_equal(a_few, a_many[:3])
  assert len({s.tobytes() for s in many.transpose(1, 0, 2)}) > 100   # (the chains differ from each other)


def test_identical_calls_return_identical_bytes():
  n = 28
  masks, thetas, states = _random_problem(n, 3, 4, seed=5)           # 3682 terms: the 28-bit KOBE-3 fits
  a = _run(states, n, masks, thetas, 1, 0, 32)
  b = _run(states, n, masks, thetas, 1, 0, 32)
  for x, y in zip(a, b):
    assert x.tobytes() == y.tobytes()
  assert a[2].min() > 0


def test_device_chain_meets_the_reference_criteria():
  """The 4-bit criteria of ebm_test.py:879-947 with the counts of the CPU check: 2e4 samples after 2e3 burn-in."""
  n, masks, thetas = R.stats_case()
  n_samples, n_burn = int(2e4), int(2e3)
  got, _, _ = _run(np.array([0], np.uint64), n, masks, thetas, 5, 0, n_burn + n_samples)
  R.check_statistics(got[n_burn:, 0, :], n, masks, thetas)


def _mirror(num_chains, samples=40):
  n, masks, thetas, seed, states = R.mirror_case(num_chains)
  energy = models.KOBE(list(range(n)), 2)
  with torch.no_grad():
    energy.post_process[0].kernel.copy_(torch.as_tensor(thetas, dtype=torch.float32))
  energy = energy.to("cuda")
  layer = inference.GibbsWithGradientsInference(energy, samples, R.MIRROR_BURNIN, initial_seed=seed, chain="device",
                                                num_chains=num_chains)
  return layer, energy, (n, masks, thetas, seed, states)


def test_inference_device_chain_equals_the_restatement():
  layer, energy, (n, masks, thetas, seed, states) = _mirror(1)
  assert layer.device_chain and layer.chain_step == 0 and layer.chain_seed == seed
  exposed = layer.chain_states
  assert exposed.is_cuda and exposed.dtype == torch.int64
  np.testing.assert_array_equal(exposed.cpu().numpy().view(np.uint64), states)
  got = layer.sample(40)
  assert got.is_cuda and got.dtype == torch.int8 and got.shape == (40, n)
  want = R.run(states, n, masks, thetas, seed, 0, R.MIRROR_BURNIN + 40)
  np.testing.assert_array_equal(got.cpu().numpy(), want["samples"][R.MIRROR_BURNIN:, 0, :])
  np.testing.assert_array_equal(layer.chain_states.cpu().numpy().view(np.uint64), want["states"])
  assert layer.chain_step == R.MIRROR_BURNIN + 40
  exposed.zero_()                                                    # a copy: the chain is not ours to write
  np.testing.assert_array_equal(layer.chain_states.cpu().numpy().view(np.uint64), want["states"])
  with torch.no_grad():                                              # a variable update: burn in again, then one step
    energy.post_process[0].kernel.mul_(-0.5)
  assert layer.variables_updated
  assert layer.sample(1).shape == (1, n)
  assert layer.chain_step == 2 * R.MIRROR_BURNIN + 41 and not layer.variables_updated
  auto = inference.GibbsWithGradientsInference(energy, 40, R.MIRROR_BURNIN, initial_seed=seed, chain="auto")
  assert auto.device_chain


def test_inference_with_three_chains_returns_step_major_rows():
  layer, _, (n, masks, thetas, seed, states) = _mirror(3)
  assert layer.num_chains == 3
  np.testing.assert_array_equal(layer.chain_states.cpu().numpy().view(np.uint64), states)
  got = layer.sample(10)
  assert got.shape == (10, n) and layer.chain_step == R.MIRROR_BURNIN + 4
  want = R.run(states, n, masks, thetas, seed, 0, R.MIRROR_BURNIN + 4)
  np.testing.assert_array_equal(got.cpu().numpy(), want["samples"][R.MIRROR_BURNIN:].reshape(12, n)[:10])


def test_vqt_with_the_device_chain_has_finite_gradients():
  n = 4
  qubits = ir.GridQubit.rect(1, n)
  ebm = models.KOBE(list(range(n)), 2).to("cuda")
  with torch.no_grad():
    ebm.post_process[0].kernel.uniform_(-0.3, 0.3)
  circuit = models.DirectQuantumCircuit(hea_circuit(qubits, 2, "v"))
  e_inf = inference.GibbsWithGradientsInference(ebm, 256, 100, initial_seed=3, chain="device", num_chains=4)
  qhbm = inference.QHBM(e_inf, inference.AnalyticQuantumInference(circuit))
  zz = ir.PauliSum()
  for a, b in zip(qubits, qubits[1:]):
    zz += ir.PZ(a) * ir.PZ(b) + 0.5 * ir.PX(a)
  loss = inference.vqt(qhbm, [zz], 1.0)
  loss.backward()
  assert np.isfinite(float(loss.detach()))
  grads = [ebm.post_process[0].kernel.grad] + [p.grad for p in circuit.trainable_variables]
  assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
  assert float(grads[0].abs().sum()) > 0 and e_inf.chain_step > 100


def test_abi_error_paths():
  n, masks, thetas, states = 5, R.kobe_masks(5, 2), np.ones(15, np.float32), np.zeros(2, np.uint64)
  st, m, th = _i64(states), _i64(masks), torch.from_numpy(thetas).cuda()
  for bad_bits in (0, 65, -1):
    with pytest.raises(E.EngineError, match="n_bits"):
      E.gwg_sample(st, bad_bits, m, th, 1, 0, 4, write_samples=False)
  with pytest.raises(E.EngineError, match="negative"):
    E.gwg_sample(st, n, m, th, 1, 0, -1, write_samples=False)
  lib = E.load_library()
  stream = torch.cuda.current_stream().cuda_stream
  assert lib.qhbm_gwg_sample(None, 2, n, m.data_ptr(), th.data_ptr(), 15, 1, 0, 4, None, None, stream) != 0
  assert b"NULL" in lib.qhbm_last_error(None)
  assert lib.qhbm_gwg_sample(st.data_ptr(), 2, n, None, th.data_ptr(), 15, 1, 0, 4, None, None, stream) != 0
  assert lib.qhbm_gwg_sample(st.data_ptr(), 2, n, m.data_ptr(), None, 15, 1, 0, 4, None, None, stream) != 0
  assert lib.qhbm_gwg_sample(st.data_ptr(), -2, n, m.data_ptr(), th.data_ptr(), 15, 1, 0, 4, None, None, stream) != 0
  assert lib.qhbm_gwg_sample(st.data_ptr(), 2, n, m.data_ptr(), th.data_ptr(), -15, 1, 0, 4, None, None, stream) != 0
  # no-ops: nothing is read, nothing moves
  assert lib.qhbm_gwg_sample(None, 0, n, None, None, 0, 1, 0, 4, None, None, stream) == 0
  out, acc = E.gwg_sample(st, n, m, th, 1, 0, 0, count_accepted=True)
  assert out.shape == (0, 2, n) and st.cpu().tolist() == [0, 0]
  # terms that do not fit in LDS are an error, not a slower path: the largest count that fits runs, 32 more do not
  fit = max(t for t in range(32, 20000, 32) if E.gwg_lds_bytes(64, t) <= E.GWG_LDS_MAX)
  assert E.gwg_lds_bytes(64, fit + 32) > E.GWG_LDS_MAX
  rng = np.random.default_rng(0)
  big = rng.integers(0, 2**63, size=fit + 32, dtype=np.uint64)
  big_th = torch.from_numpy(rng.integers(-64, 65, size=fit + 32) / 4096.0).cuda()
  wide = _i64(np.array([3], np.uint64))
  with pytest.raises(E.EngineError, match="LDS"):
    E.gwg_sample(wide, 64, _i64(big), big_th, 1, 0, 1)
  assert wide.cpu().tolist() == [3]
  want = R.run(np.array([3], np.uint64), 64, big[:fit], big_th[:fit].cpu().numpy(), 1, 0, 2)
  out, _ = E.gwg_sample(wide, 64, _i64(big[:fit]), big_th[:fit], 1, 0, 2)
  assert not want["ambiguous"].any()                                 # (theta in multiples of 2^-12, |h| < 1: exact in fp32)
  np.testing.assert_array_equal(out.cpu().numpy(), want["samples"])
  with pytest.raises(ValueError, match="fit in LDS"):
    inference.GibbsWithGradientsInference(models.KOBE(list(range(40)), 3).to("cuda"), 10, 10, chain="device")
