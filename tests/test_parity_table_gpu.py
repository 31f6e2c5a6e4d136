"""Spin-parity energy tables by a Walsh-Hadamard transform on the MI355X: qhbm_walsh_hadamard,
qhbm_parity_table and qhbm_parity_table_vjp against the numpy restatement (tests/parity_table_ref.py), today's term-by-term
path (qhbm_parity_energy over the bitstring table) and closed forms, and the mirror's opt-in routes
(`energy_table(method="transform")`, `AnalyticEnergyInference(table="transform")`,
`AnalyticQuantumInference(parity_tables="transform")`).

Pass constants of the launcher (csrc/parity_table.hip): a tile of 2^K = 2^14 floats is one launch, every further pass adds
9 index bits: n2 = 15 and n3 = 24 are the smallest sizes with 2 and 3 passes; 30 bits take 3.

Error bounds (u = 2^-24, the unit roundoff of fp32): an output of the transform is the root of a binary tree of n levels
of fp32 additions over inputs x, so its error is at most ((1 + u)^n - 1) sum |x| = n u sum |x| to first order; the tests
allow 2 n u sum |x|.  A table adds the scatter's roundings, one per duplicate of a mask: 2 (n + d) u sum |theta|."""
import ctypes

import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd import inference, ir, models, utils
from qhbmlib_amd.models import energy_utils
from tests import energy_table_ref as TR
from tests import parity_table_ref as R
from tests.test_host_api import hea_circuit

pytestmark = pytest.mark.gpu

K, N2, N3 = R.TILE_BITS, R.N2, R.N3
U = 2.0 ** -24


def _masks_t(masks):
  return torch.from_numpy(np.asarray(masks, dtype=np.uint64).view(np.int64).copy()).cuda()


def _set(param, values):
  with torch.no_grad():
    param.copy_(torch.as_tensor(np.asarray(values), dtype=torch.float32))


def _kobe(n, order, thetas=None, rng=None, scale=64):
  """A KOBE on the GPU with dyadic thetas (multiples of 2^-6 in [-scale/64, scale/64]) unless `thetas` is given."""
  energy = models.KOBE(list(range(n)), order)
  kernel = energy.post_process[0].kernel
  if thetas is None:
    thetas = rng.integers(-scale, scale + 1, kernel.numel()).astype(np.float64) / 64.0
  _set(kernel, thetas)
  return energy.to("cuda")


def _stream():
  return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- 1. raw transform, exact ----------------------------------------------------------------------------------------
def test_constants_are_the_launcher_s():
  assert (K, N2, N3) == (14, 15, 24) == (E.WHT_TILE_BITS, E.WHT_TILE_BITS + 1, E.WHT_TILE_BITS + E.WHT_ROW_BITS + 1)
  assert [E.walsh_hadamard_passes(n) for n in (K, N2, N3 - 1, N3, 30)] == [1, 2, 2, 3, 3]


@pytest.mark.parametrize("n", R.raw_sizes())
def test_raw_transform_is_exact_and_repeatable(n):
  positions, values = R.raw_case(n)
  if positions is None:   # dense, the whole output
    x = torch.from_numpy(values.astype(np.float32)).cuda()
    first = E.walsh_hadamard_(x.clone())
    second = E.walsh_hadamard_(x.clone())
    got = first.cpu().numpy()
    assert np.array_equal(got.astype(np.int64), R.wht_i64(values)) and np.array_equal(got, np.round(got))
  else:                   # sparse: single outputs against the sparse evaluation on the host
    x = torch.zeros(1 << n, dtype=torch.float32, device="cuda")
    x[torch.from_numpy(positions.astype(np.int64)).cuda()] = torch.from_numpy(values.astype(np.float32)).cuda()
    first = E.walsh_hadamard_(x.clone())
    second = E.walsh_hadamard_(x)
    ys = R.raw_outputs(n)
    assert ys.size >= 4096
    got = first[torch.from_numpy(ys.astype(np.int64)).cuda()].cpu().numpy()
    want = R.sparse_eval(positions, values, ys)
    assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, np.round(got))
  assert torch.equal(first, second)


# ---- 2. tables, exact -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 3])
@pytest.mark.parametrize("n", R.TABLE_BITS)
def test_dyadic_kobe_table_equals_the_term_by_term_table(n, order):
  energy = _kobe(n, order, rng=np.random.default_rng(100 * n + order))
  kernel = energy.post_process[0].kernel
  want = energy(energy_utils.all_bitstrings(n, "cuda"))   # today's path: qhbm_parity_energy over the bitstring table
  got = E.parity_table(kernel, energy._parity_masks(kernel.device), n)   # pylint: disable=protected-access
  assert got.shape == (1 << n,) and got.dtype == torch.float32 and got.is_cuda
  assert torch.equal(got, want)
  assert torch.equal(energy_utils.energy_table(energy, n, method="transform"), energy_utils.energy_table(energy, n))


def test_dyadic_bernoulli_table_at_20_bits():
  n = 20
  energy = models.BernoulliEnergy(list(range(n)))
  _set(energy.post_process[0].kernel, R.dyadic_thetas(n, np.random.default_rng(20)))
  energy = energy.to("cuda")
  assert torch.equal(energy_utils.energy_table(energy, n, method="transform"), energy_utils.energy_table(energy, n))


@pytest.mark.parametrize("n", [7, N2])
def test_hand_made_term_lists(n):
  bits = energy_utils.all_bitstrings(n, "cuda")
  for name, (masks, thetas) in R.hand_made_terms(n).items():
    th = torch.from_numpy(np.asarray(thetas, np.float32)).cuda()
    got = E.parity_table(th, _masks_t(masks), n)
    want = R.table(masks, thetas, n)   # dyadic thetas: exact in fp64 and in fp32
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want), name
    assert torch.equal(got, E.parity_energy(th, bits, _masks_t(masks))), name
  assert not E.parity_table(torch.zeros(0, device="cuda"), _masks_t([]), n).any()
  # the bit-order canary: one term on column 0 flips sign exactly at y >= 2^(n-1)
  canary = E.parity_table(torch.ones(1, device="cuda"), _masks_t([1]), n)
  y = torch.arange(1 << n, device="cuda")
  assert torch.equal(canary, torch.where(y >= (1 << (n - 1)), -1.0, 1.0))


# ---- 3. VJP ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.VJP_EXACT_BITS)
def test_vjp_with_integer_weights_equals_the_term_by_term_vjp(n):
  energy = _kobe(n, 2, rng=np.random.default_rng(n))
  kernel = energy.post_process[0].kernel
  w = torch.from_numpy(R.integer_weights(n)).cuda()
  table = E.parity_table(kernel, energy._parity_masks(kernel.device), n)   # pylint: disable=protected-access
  (got,) = torch.autograd.grad((table * w).sum(), kernel)
  (want,) = torch.autograd.grad((energy(energy_utils.all_bitstrings(n, "cuda")) * w).sum(), kernel)   # _ParityEnergyFunction
  assert got.device == kernel.device and torch.equal(got, want)
  assert float(want.abs().max()) > 0


@pytest.mark.parametrize("n", [12, N2, N2 + 1])
def test_vjp_with_positive_weights_against_float64(n):
  rng = np.random.default_rng(7 * n)
  sets = R.kobe_index_sets(n, 2)
  masks = R.masks_of(sets)
  w = rng.uniform(0.1, 1.0, 1 << n).astype(np.float32)
  thetas = torch.zeros(len(sets), device="cuda", requires_grad=True)
  table = E.parity_table(thetas, _masks_t(masks), n)
  (got,) = torch.autograd.grad((table * torch.from_numpy(w).cuda()).sum(), thetas)
  want = R.vjp(masks, w.astype(np.float64), n)
  err, bound = np.abs(got.cpu().numpy() - want).max(), 2 * n * U * np.abs(w.astype(np.float64)).sum()
  print(f"n={n}: max |vjp - float64| = {err:.3e}, bound {bound:.3e}")
  assert err <= bound


@pytest.mark.parametrize("n", [12, N2, N2 + 1])
def test_tables_with_non_dyadic_thetas_against_float64(n):
  rng = np.random.default_rng(11 * n)
  sets = R.kobe_index_sets(n, 3)
  masks = np.concatenate([R.masks_of(sets), R.masks_of(sets[:5]), R.masks_of(sets[:2])])   # multiplicities up to 3
  thetas = rng.uniform(-1, 1, masks.size).astype(np.float32)
  d = R.multiplicity(masks, n)
  assert d == 3
  got = E.parity_table(torch.from_numpy(thetas).cuda(), _masks_t(masks), n).cpu().numpy()
  want = R.table(masks, thetas.astype(np.float64), n)
  err, bound = np.abs(got - want).max(), 2 * (n + d) * U * np.abs(thetas.astype(np.float64)).sum()
  print(f"n={n}: max |table - float64| = {err:.3e}, bound {bound:.3e}")
  assert err <= bound


@pytest.mark.parametrize("n", [9, N2 + 1])
def test_vjp_call_leaves_the_weights_alone(n):
  lib = E.load_library()
  masks = _masks_t(R.masks_of(R.kobe_index_sets(n, 2)))
  w = torch.from_numpy(np.random.default_rng(n).normal(size=1 << n).astype(np.float32)).cuda()
  kept = w.clone()
  scratch = torch.empty_like(w)
  grad = torch.empty(masks.numel(), device="cuda")
  assert lib.qhbm_parity_table_vjp(masks.data_ptr(), masks.numel(), n, w.data_ptr(), scratch.data_ptr(), grad.data_ptr(),
                                   _stream()) == 0
  torch.cuda.synchronize()
  assert torch.equal(w, kept)
  assert torch.equal(scratch, E.walsh_hadamard_(kept.clone()))
  # the scratch may not be the weights
  assert lib.qhbm_parity_table_vjp(masks.data_ptr(), masks.numel(), n, w.data_ptr(), w.data_ptr(), grad.data_ptr(),
                                   _stream()) != 0
  assert torch.equal(w, kept)


# ---- 4. AnalyticEnergyInference(table="transform") against the default ------------------------------------------------
class _LeafTable(inference.AnalyticEnergyInference):
  """The inference's own formulas on a GIVEN table: their gradient with respect to it is the upstream w of the VJP."""
  leaf = None

  @property
  def all_energies(self):
    return self.leaf


@pytest.mark.parametrize("n", [12, N2])
def test_analytic_inference_by_transform_against_the_default(n):
  """Values: the two tables are bit-identical (dyadic thetas), everything after them is the same torch code.
  Gradients: both paths hand the SAME upstream w = d f / d table (same bits in, same torch kernels) to their VJP.  The
  default, qhbm_parity_energy_vjp, sums in fp64 and rounds once: its error is at most u |g_k| <= u sum |w|.  The transform's
  is at most 2 n u sum |w| (module docstring).  So the two gradients differ by at most (2 n + 1) u sum |w|, with sum |w|
  taken from the fp32 upstream itself (`_LeafTable`)."""
  energy = _kobe(n, 2, rng=np.random.default_rng(n), scale=16)
  kernel = energy.post_process[0].kernel
  default = inference.AnalyticEnergyInference(energy, 1000, initial_seed=5)
  by_transform = inference.AnalyticEnergyInference(energy, 1000, initial_seed=5, table="transform")
  assert by_transform.table == "transform" and by_transform._all_bitstrings is None   # pylint: disable=protected-access
  assert torch.equal(by_transform.all_energies, default.all_energies)
  assert torch.equal(by_transform.log_partition(), default.log_partition())
  assert torch.equal(by_transform.entropy(), default.entropy())
  drawn = by_transform.sample(1000)
  assert drawn.dtype == torch.int8 and drawn.shape == (1000, n) and torch.equal(drawn, default.sample(1000))
  assert torch.equal(by_transform.distribution.logits, default.distribution.logits)
  assert by_transform._all_bitstrings is None   # pylint: disable=protected-access  (nothing above needed the bitstring table)
  probe = _LeafTable(energy, 10, initial_seed=5, table="transform")
  for name in ("log_partition", "entropy"):
    (got,) = torch.autograd.grad(getattr(by_transform, name)(), kernel)
    (want,) = torch.autograd.grad(getattr(default, name)(), kernel)
    probe.leaf = default.all_energies.detach().clone().requires_grad_(True)
    with probe.device_only():
      (w,) = torch.autograd.grad(getattr(probe, name)(), probe.leaf)
    err, bound = float((got - want).abs().max()), (2 * n + 1) * U * float(w.double().abs().sum())
    print(f"n={n} {name}: max |grad difference| = {err:.3e}, bound {bound:.3e}, max |grad| = {float(want.abs().max()):.3e}")
    assert err <= bound
  assert torch.equal(by_transform.all_bitstrings, default.all_bitstrings)   # built when somebody asks


def _tfim(qubits):
  ham = ir.PauliSum()
  for i, q in enumerate(qubits):
    ham += -1.0 * ir.PX(q)
    ham += -1.0 * ir.PZ(q) * ir.PZ(qubits[(i + 1) % len(qubits)])
  return ham


def test_captured_vqt_step_with_the_transform_table_replays_the_eager_bits():
  n, layers, samples = N2, 2, 256
  qubits = ir.GridQubit.rect(1, n)
  torch.manual_seed(15)
  circuit = models.DirectQuantumCircuit(hea_circuit(qubits, layers, "pt"), tfq_compat_bit_order=False).to("cuda")
  energy = models.KOBE(list(range(n)), 2).to("cuda")
  with torch.no_grad():
    circuit.trainable_variables[0].uniform_(-1, 1)
    energy.post_process[0].kernel.uniform_(-0.4, 0.4)
  e_inf = inference.AnalyticEnergyInference(energy, samples, initial_seed=15, table="transform")
  qhbm = inference.QHBM(e_inf, inference.AnalyticQuantumInference(circuit))
  variables = list(energy.parameters()) + circuit.trainable_variables
  ham = _tfim(qubits)
  step = inference.CapturedLoss(lambda: inference.vqt(qhbm, [ham], 0.7), [e_inf], variables)
  with torch.no_grad():
    drawn = e_inf.sample(samples).cuda()
  rows, _, counts = utils.unique_bitstrings_with_counts(drawn)
  want_loss = step.eager([(rows, counts)]).clone()
  want = [v.grad.detach().clone() for v in variables]
  for _ in range(3):
    got = step([(rows, counts)])
    torch.cuda.synchronize()
    assert step.captured and torch.equal(got, want_loss)
    assert all(torch.equal(v.grad, w) for v, w in zip(variables, want))
  assert all(float(w.abs().max()) > 0 for w in want)
  assert e_inf._all_bitstrings is None   # pylint: disable=protected-access


# ---- 5. beyond the bitstring table, against closed forms in float64 ---------------------------------------------------
def _reduce_f64(table):
  """(log Z, entropy) of a table reduced on the device in float64."""
  logits = -table.double()
  log_z = torch.logsumexp(logits, 0)
  logp = logits - log_z
  return log_z, -(logp.exp() * logp).sum()


def test_bernoulli_at_26_bits_against_its_closed_form():
  n = 26
  rng = np.random.default_rng(26)
  thetas = rng.uniform(-0.6, 0.6, n)
  energy = models.BernoulliEnergy(list(range(n)))
  _set(energy.post_process[0].kernel, thetas)
  energy = energy.to("cuda")
  kernel = energy.post_process[0].kernel
  th64 = kernel.detach().cpu().double().numpy()   # (the fp32 values the kernel sees)
  table = energy_utils.energy_table(energy, n, max_qubits=n, method="transform")
  log_z, _ = _reduce_f64(table)
  want = np.log(2.0 * np.cosh(th64)).sum()
  table_bound = 2 * (n + 1) * U * np.abs(th64).sum()   # every entry within it, and log Z is 1-Lipschitz in the sup norm
  print(f"log Z = {float(log_z.detach()):.9f}, closed form {want:.9f}, |difference| {abs(float(log_z.detach()) - want):.3e}, bound {table_bound:.3e}")
  assert abs(float(log_z.detach()) - want) <= table_bound
  (grad,) = torch.autograd.grad(log_z, kernel)
  # upstream w = -p: sum |w| = 1
  err, vjp_bound = np.abs(grad.cpu().numpy() - np.tanh(th64)).max(), 2 * n * U * 1.0
  print(f"max |d log Z / d theta - tanh theta| = {err:.3e}, bound {vjp_bound:.3e}")
  assert err <= vjp_bound


def test_open_ising_chain_at_26_bits_against_its_closed_forms():
  """KOBE order 2 with only the chain couplings J_i (bits i, i + 1) non-zero: with bond variables b_i = s_i s_(i+1) the
  weights factorise, Z = 2 prod 2 cosh J_i, <b_i> = -tanh J_i.  A perturbation of every energy by at most eps moves every
  log p by at most 2 eps, so S = -sum p log p moves by at most 2 eps sum p |log p| = 2 eps S to first order."""
  n = 26
  rng = np.random.default_rng(27)
  sets = R.kobe_index_sets(n, 2)
  coupling = rng.uniform(-0.8, 0.8, n - 1)
  thetas = np.zeros(len(sets))
  for i in range(n - 1):
    thetas[sets.index((i, i + 1))] = coupling[i]
  energy = _kobe(n, 2, thetas=thetas)
  kernel = energy.post_process[0].kernel
  chain = [sets.index((i, i + 1)) for i in range(n - 1)]
  j64 = kernel.detach().cpu().double().numpy()[chain]
  inf = inference.AnalyticEnergyInference(energy, 10, initial_seed=1, table="transform")
  log_z, entropy = _reduce_f64(inf.all_energies)
  want_log_z = n * np.log(2.0) + np.log(np.cosh(j64)).sum()
  want_entropy = want_log_z - (j64 * np.tanh(j64)).sum()
  table_bound = 2 * (n + 1) * U * np.abs(j64).sum()
  lz, ent = float(log_z.detach()), float(entropy.detach())
  print(f"log Z = {lz:.9f} (closed form {want_log_z:.9f}, bound {table_bound:.3e}), "
        f"S = {ent:.9f} (closed form {want_entropy:.9f}, bound {2.02 * table_bound * want_entropy:.3e})")
  assert abs(lz - want_log_z) <= table_bound
  assert abs(ent - want_entropy) <= 2.02 * table_bound * want_entropy
  (grad,) = torch.autograd.grad(log_z, kernel)
  grad = grad.cpu().numpy()
  # d log Z / d theta_S = -<s_S>: a single spin averages to zero, a pair (i, j) is the product of the bonds between them,
  # <s_i s_j> = prod_(i <= k < j) (-tanh J_k) -- for a bond itself d log Z / dJ_i = tanh J_i
  want_grad = np.asarray([0.0 if len(ix) == 1 else -np.prod(-np.tanh(j64[ix[0]:ix[1]])) for ix in sets])
  assert np.array_equal(want_grad[chain], np.tanh(j64))
  err, vjp_bound = np.abs(grad - want_grad).max(), 2 * n * U * 1.0   # (upstream w = -p: sum |w| = 1)
  print(f"max |d log Z / d theta - closed form| = {err:.3e} (bonds: {np.abs(grad[chain] - np.tanh(j64)).max():.3e}), "
        f"bound {vjp_bound:.3e}")
  assert err <= vjp_bound
  # the inference's own fp32 reductions, held to the float64 reduction of the same table (tolerances of test_ebm_gpu.py)
  with torch.no_grad(), inf.device_only():
    np.testing.assert_allclose(float(inf.log_partition()), lz, rtol=1e-5)
    np.testing.assert_allclose(float(inf.entropy()), ent, rtol=1e-4)
  del log_z, entropy
  # beyond 2^24 categories the sampler draws by the inverse CDF and unpacks the indices: rows of bits, no bitstring table
  drawn = inf.sample(64)
  assert drawn.shape == (64, n) and drawn.dtype == torch.int8 and int(drawn.min()) >= 0 and int(drawn.max()) <= 1
  assert inf._all_bitstrings is None   # pylint: disable=protected-access
  with pytest.raises(ValueError, match="24 bits"):
    inf.all_bitstrings   # pylint: disable=pointless-statement


def test_thirty_bits_construct_for_free_and_match_the_closed_form():
  n = 30
  thetas = np.random.default_rng(30).uniform(-0.5, 0.5, n)
  energy = models.BernoulliEnergy(list(range(n)))
  _set(energy.post_process[0].kernel, thetas)
  energy = energy.to("cuda")
  torch.cuda.synchronize()
  before = torch.cuda.memory_allocated()
  inf = inference.AnalyticEnergyInference(energy, 10, initial_seed=3, table="transform")
  assert torch.cuda.memory_allocated() == before
  th64 = energy.post_process[0].kernel.detach().cpu().double().numpy()
  with torch.no_grad():
    log_z = float(inf.log_partition())
  want = np.log(2.0 * np.cosh(th64)).sum()
  print(f"30 bits: log Z = {log_z:.7f}, closed form {want:.7f}")
  np.testing.assert_allclose(log_z, want, rtol=1e-5)   # (the tolerance test_ebm_gpu.py holds an fp32 log partition to)
  del inf
  torch.cuda.empty_cache()


# ---- 6. quantum side --------------------------------------------------------------------------------------------------
def test_quantum_inference_builds_its_table_by_transform():
  n = N2
  qubits = ir.GridQubit.rect(1, n)
  states = torch.from_numpy(np.random.default_rng(6).integers(0, 2, (12, n)).astype(np.int8))

  def run(parity_tables):
    torch.manual_seed(12)
    circ = models.DirectQuantumCircuit(hea_circuit(qubits, 2, "m"), tfq_compat_bit_order=False).to("cuda")
    circ_h = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "h"), tfq_compat_bit_order=False).to("cuda")
    with torch.no_grad():
      circ.trainable_variables[0].uniform_(-1, 1)
      circ_h.trainable_variables[0].uniform_(-1, 1)
    energy = _kobe(n, 3, rng=np.random.default_rng(3), scale=16)
    q = inference.AnalyticQuantumInference(circ, energy_tables="all", parity_tables=parity_tables)
    vals = q.expectation(states, models.Hamiltonian(energy, circ_h))
    vals.sum().backward()
    grads = [energy.post_process[0].kernel.grad, circ.trainable_variables[0].grad, circ_h.trainable_variables[0].grad]
    return vals.detach().cpu().numpy(), [g.cpu().numpy() for g in grads]

  v_terms, g_terms = run("terms")
  v_transform, g_transform = run("transform")
  assert np.array_equal(v_transform, v_terms) and np.abs(v_terms).max() > 0
  for a, b in zip(g_transform, g_terms):   # (tests/test_energy_table_gpu.py's tolerance for a gradient block)
    print(f"max |gradient block difference| = {np.abs(a - b).max():.3e} of {np.abs(b).max():.3e}")
    np.testing.assert_allclose(a, b, atol=1e-4 * max(1.0, np.abs(b).max()))
    assert np.abs(b).max() > 0


def test_a_general_energy_is_untouched_by_parity_tables():
  n = 4
  qubits = ir.GridQubit.rect(1, n)
  states = torch.tensor([[0, 1, 1, 0], [1, 0, 0, 1], [1, 1, 1, 0]], dtype=torch.int8)

  def run(parity_tables):
    torch.manual_seed(3)
    circ = models.DirectQuantumCircuit(hea_circuit(qubits, 2, "m"))
    circ_h = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "h"))
    with torch.no_grad():
      circ.trainable_variables[0].uniform_(-1, 1)
      circ_h.trainable_variables[0].uniform_(-1, 1)
    energy = models.BitstringEnergy(list(range(n)), TR.mlp_layers(n, 6, 4))
    q = inference.AnalyticQuantumInference(circ, energy_tables="general", parity_tables=parity_tables)
    vals = q.expectation(states, models.Hamiltonian(energy, circ_h))
    vals.sum().backward()
    return [vals.detach().cpu()] + [p.grad.cpu() for p in list(energy.parameters()) + circ.trainable_variables]

  for a, b in zip(run("transform"), run("terms")):
    assert torch.equal(a, b)
  with pytest.raises(ValueError, match="parity_tables"):
    inference.AnalyticQuantumInference(models.DirectQuantumCircuit(hea_circuit(qubits, 1, "x")), parity_tables="fwht")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
  lib = E.load_library()
  small = torch.zeros(4, device="cuda")
  masks = _masks_t([1])
  for rc in (lib.qhbm_walsh_hadamard(small.data_ptr(), 31, _stream()),
             lib.qhbm_walsh_hadamard(small.data_ptr(), 0, _stream()),
             lib.qhbm_parity_table(masks.data_ptr(), small.data_ptr(), 1, 31, small.data_ptr(), _stream()),
             lib.qhbm_parity_table_vjp(masks.data_ptr(), 1, 31, small.data_ptr(), small.data_ptr(), small.data_ptr(), _stream())):
    assert rc != 0 and b"[1, 30]" in lib.qhbm_last_error(None)
  assert lib.qhbm_walsh_hadamard(None, 2, _stream()) != 0 and b"NULL" in lib.qhbm_last_error(None)
  assert lib.qhbm_parity_table(masks.data_ptr(), small.data_ptr(), -1, 2, small.data_ptr(), _stream()) != 0
  assert lib.qhbm_parity_table(None, small.data_ptr(), 1, 2, small.data_ptr(), _stream()) != 0
  assert lib.qhbm_parity_table(masks.data_ptr(), small.data_ptr(), 1, 2, None, _stream()) != 0
  assert lib.qhbm_parity_table_vjp(masks.data_ptr(), -1, 2, small.data_ptr(), small.data_ptr(), small.data_ptr(), _stream()) != 0
  torch.cuda.synchronize()
  assert not small.any()   # nothing ran
  with pytest.raises(E.EngineError, match=r"\[1, 30\]"):
    E.parity_table(torch.zeros(1, device="cuda"), masks, 31)
  with pytest.raises(E.EngineError, match="2\\^n"):
    E.walsh_hadamard_(torch.zeros(6, device="cuda"))
  with pytest.raises(E.EngineError, match="CUDA"):
    E.walsh_hadamard_(torch.zeros(8))
  wide = models.BernoulliEnergy(list(range(31))).to("cuda")
  with pytest.raises(ValueError, match="at most 30 bits"):
    energy_utils.energy_table(wide, 31, max_qubits=31, method="transform")
  with pytest.raises(ValueError, match="at most 30 bits"):
    inference.AnalyticEnergyInference(wide, 10, table="transform")
  general = models.BitstringEnergy([0, 1, 2], [models.SpinsFromBitstrings(), torch.nn.Linear(3, 1)]).to("cuda")
  with pytest.raises(ValueError, match="PauliMixin"):
    inference.AnalyticEnergyInference(general, 10, table="transform")
  host = models.KOBE(list(range(5)), 2)
  with pytest.raises(ValueError, match="CUDA"):
    energy_utils.energy_table(host, 5, method="transform")
