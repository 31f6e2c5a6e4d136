"""The float64 loss reference (tests/loss_ref.py) checked against central differences, the conditions its cases
(tests/loss_cases.py) must meet so that the GPU bars of tests/test_losses_hamiltonian_gpu.py cannot hide a failure, and
the caller-level contract of the mirror that needs no engine: `QHBM.circuits` and the samplers' seed handling."""
import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import inference, ir, models
from tests import loss_cases as L
from tests import loss_ref as R
from tests.test_host_api import hea_circuit

STEP = 1e-5   # step and bar of the plan emulator's own oracle self-test (tests/sanitize/plan_fuzz.cpp)


def _central(fn, x):
  x = np.asarray(x, dtype=np.float64)
  out = np.zeros_like(x)
  for i in range(x.size):
    hi, lo = x.copy(), x.copy()
    hi[i] += STEP
    lo[i] -= STEP
    out[i] = (fn(hi) - fn(lo)) / (2 * STEP)
  return out


def _assert_block(got, want, what):
  assert got.shape == want.shape, what
  err = np.abs(got - want)
  assert (err <= 1e-8 * np.maximum(1.0, np.abs(want))).all(), (what, float(err.max()))


def _exact(name):
  """The case over ALL 8 bitstrings; the weights are set by the caller."""
  c = dict(L.case(name))
  c["bits"] = O.all_bitstrings(c["n"])
  return c


@pytest.mark.parametrize("name", ["n3", "n3_bernoulli"])
def test_vqt_blocks_equal_central_differences_of_the_exact_expected_loss(name):
  """With w = p_theta over all 8 bitstrings the multiset loss is the exact expected loss.  phi, psi, vartheta: the loss
  itself at fixed weights.  theta: the function whose gradient the estimator estimates -- p_theta varies, the E_theta
  inside f and log Z are constants (vqt_loss.py:46-55, ebm.py:262-329)."""
  c = _exact(name)
  n, a, b = c["n"], c["a"], c["b"]
  p = L.energy(a, n).probabilities()
  base = L.vqt_reference(c, weights=p)
  loss = lambda **kw: L.vqt_reference(c, weights=p, circuit_gradients=False, **kw)["loss"]
  _assert_block(base["phi"], _central(lambda v: loss(phi=v), a["values"]), "phi")
  _assert_block(base["psi"], _central(lambda v: loss(psi=v), b["values"]), "psi")
  _assert_block(base["vartheta"], _central(lambda v: loss(target_energy=L.energy(b, n).with_thetas(v)), b["thetas"]),
                "vartheta")
  _assert_block(base["theta"], _central(lambda v: L.energy(a, n).with_thetas(v).probabilities() @ base["f"], a["thetas"]),
                "theta")


@pytest.mark.parametrize("name", ["n3", "n3_bernoulli"])
def test_qmhl_blocks_equal_central_differences_of_the_exact_expected_loss(name):
  """With w = p_thetad (the data QHBM's exact distribution): theta, phi, phid differentiate the loss at fixed weights
  (log Z_theta included); thetad differentiates sum_x p_thetad(x) g(x) (qmhl_loss.py:33-34, qhbm_data.py:26-38)."""
  c = _exact(name)
  n, a, b = c["n"], c["a"], c["b"]
  p = L.energy(b, n).probabilities()
  base = L.qmhl_reference(c, weights=p)
  loss = lambda **kw: L.qmhl_reference(c, weights=p, circuit_gradients=False, **kw)["loss"]
  _assert_block(base["theta"], _central(lambda v: loss(model_energy=L.energy(a, n).with_thetas(v)), a["thetas"]), "theta")
  _assert_block(base["phi"], _central(lambda v: loss(phi=v), a["values"]), "phi")
  _assert_block(base["phid"], _central(lambda v: loss(phid=v), b["values"]), "phid")
  _assert_block(base["thetad"], _central(lambda v: L.energy(b, n).with_thetas(v).probabilities() @ base["g"], b["thetas"]),
                "thetad")


def test_exact_log_partition_forms_agree():
  """The Bernoulli closed forms equal the enumeration a first-order KOBE gives for the same weights."""
  thetas = np.array([0.3, -1.1, 0.7, 0.05])
  closed, enumerated = R.SpinEnergy(4, thetas), R.SpinEnergy(4, thetas, order=1)
  np.testing.assert_allclose(closed.log_partition(), enumerated.log_partition(), rtol=1e-14)
  np.testing.assert_allclose(closed.log_partition_grad(), enumerated.log_partition_grad(), atol=1e-14)
  np.testing.assert_allclose(enumerated.log_partition(), O.log_partition_exact(enumerated.energy, 4), rtol=1e-14)


# ---- conditions on the cases -------------------------------------------------------------------------------------------
def _assert_visible(blocks, what):
  for key, want in blocks.items():
    mag = np.abs(np.asarray(want))
    assert mag.max() >= 1e-2, (what, key, float(mag.max()))
    assert np.mean(mag < 1e-3) <= 0.25, (what, key, float(np.mean(mag < 1e-3)))


@pytest.mark.parametrize("name", L.LOSS_CASES + ["n12_compat"])
def test_every_expected_gradient_block_stands_clear_of_the_absolute_floors(name):
  """The GPU bars have absolute floors (1e-4, 2e-4, 5e-5 beta): a block of near-zero entries would pass with any
  engine.  Every block has |want|_inf >= 1e-2 and at most a quarter of its entries below 1e-3."""
  c = L.case(name)
  assert len(c["bits"]) <= 8 and len(set(c["counts"].tolist())) == len(c["counts"]) and 1 in c["counts"]
  assert len(np.unique(c["bits"], axis=0)) == len(c["bits"])
  v = L.expected_vqt(name)
  _assert_visible({k: v[k] for k in ("theta", "phi", "vartheta", "psi")}, name + " vqt")
  if not c["compat"]:
    q = L.expected_qmhl(name)
    _assert_visible({k: q[k] for k in ("theta", "phi", "thetad", "phid")}, name + " qmhl")


def test_self_case_copies_the_model_and_its_sampling_error_is_a_fifth_of_the_bar():
  """qmhl_loss_test.py:48-80: the data part is the model part under other symbol names.  The total circuit is then the
  identity, so the circuit blocks vanish on ANY multiset; the theta blocks do not.  The loss bar of the sampled leg,
  2e-3 at 2 10^5 samples, is at least 5 standard deviations of the sample average."""
  c = L.case(L.SELF_CASE)
  assert c["b"]["name"] != c["a"]["name"]
  assert all(np.array_equal(c["a"][k], c["b"][k]) for k in ("thetas", "values"))
  q = L.expected_qmhl(L.SELF_CASE)
  _assert_visible({k: q[k] for k in ("theta", "thetad")}, "self qmhl")
  assert max(np.abs(q["phi"]).max(), np.abs(q["phid"]).max()) < 1e-12
  assert 5 * L.self_sampling_sigma() <= 2e-3


def _far(a, b, bar):
  return float(np.abs(np.asarray(a) - np.asarray(b)).max()) > 2.0 * bar


@pytest.mark.parametrize("name", L.LOSS_CASES)
def test_each_wrong_expected_side_is_farther_than_two_bars_from_the_right_one(name):
  """What a comparison within one bar can tell apart: beta lost, the phi / psi split taken at the wrong place, the
  log Z gradient dropped, equal weights instead of counts.  Each moves the expected side by more than two bars."""
  c = L.case(name)
  a, b, beta = c["a"], c["b"], c["beta"]
  v, q = L.expected_vqt(name), L.expected_qmhl(name)
  # beta -> 1
  v1 = L.vqt_reference(c, beta=1.0)
  assert _far(v["loss"], v1["loss"], L.loss_bar(beta, b["thetas"]))
  assert _far(v["phi"], v1["phi"], L.circuit_bar(v["phi"])) and _far(v["psi"], v1["psi"], L.circuit_bar(v["psi"]))
  assert _far(v["vartheta"], v1["vartheta"], L.shard_bar(beta)) and _far(v["theta"], v1["theta"], L.SCORE_BAR)
  # the two halves of the circuit gradient handed to the wrong circuit
  swapped = np.concatenate([v["psi"], v["phi"]])
  assert _far(swapped[:len(a["values"])], v["phi"], L.circuit_bar(v["phi"]))
  assert _far(swapped[len(a["values"]):], v["psi"], L.circuit_bar(v["psi"]))
  # log Z gradient dropped from the QMHL theta block
  assert _far(q["theta"] - L.energy(a, c["n"]).log_partition_grad(), q["theta"], L.shard_bar(1.0))
  # equal weights
  ve, qe = L.vqt_reference(c, weights=np.ones(len(c["counts"]))), L.qmhl_reference(c, weights=np.ones(len(c["counts"])))
  assert _far(v["loss"], ve["loss"], L.loss_bar(beta, b["thetas"])) and _far(q["loss"], qe["loss"], L.loss_bar(1.0, a["thetas"]))
  for key, bar in (("phi", L.circuit_bar(v["phi"])), ("psi", L.circuit_bar(v["psi"])), ("vartheta", L.shard_bar(beta)),
                   ("theta", L.SCORE_BAR)):
    assert _far(v[key], ve[key], bar), key
  for key, bar in (("phi", L.circuit_bar(q["phi"])), ("phid", L.circuit_bar(q["phid"])), ("theta", L.shard_bar(1.0)),
                   ("thetad", L.SCORE_BAR)):
    assert _far(q[key], qe[key], bar), key


@pytest.mark.parametrize("name", L.COMPAT_CASES)
def test_bit_order_cases_tell_both_wrong_behaviours_apart(name):
  """circuit.py:59-62,131-134 against energy.py:165-167,205-206: the flag permutes the injector columns and NOT the
  shards.  On every row the right value differs from "injector not permuted" and from "injector and shards permuted"
  by at least 100 value bars."""
  c = L.case(name)
  bar = L.loss_bar(1.0, c["b"]["thetas"])
  right = L.expected_modular(name)
  assert (np.abs(right - L.expected_modular(name, injector=False)) >= 100 * bar).all()
  assert (np.abs(right - L.expected_modular(name, shards=True)) >= 100 * bar).all()


def test_bit_order_vqt_case_tells_both_wrong_behaviours_apart():
  name = "n12_compat"
  c = L.case(name)
  n, b = c["n"], c["b"]
  bar = L.loss_bar(c["beta"], b["thetas"])
  right = L.expected_vqt(name)
  unpermuted = L.vqt_reference(c, tfq_compat=False)
  ham = L.energy(b, n)
  shards_too = L.vqt_reference(c, target_energy=R.SpinEnergy(n, ham.thetas, ham.order, L.permuted_shards(b, n)))
  for wrong in (unpermuted, shards_too):
    assert abs(right["loss"] - wrong["loss"]) >= 100 * bar
    for key in ("phi", "psi"):
      assert np.abs(right[key] - wrong[key]).max() >= 100 * L.circuit_bar(right[key])
    assert np.abs(right["vartheta"] - wrong["vartheta"]).max() >= 100 * L.shard_bar(c["beta"])
    assert np.abs(right["theta"] - wrong["theta"]).max() >= 100 * L.SCORE_BAR


# ---- the mirror's caller-level contract that needs no engine ------------------------------------------------------------
def _set(param, values):
  with torch.no_grad():
    param.copy_(torch.as_tensor(np.asarray(values), dtype=torch.float32))


def test_qhbm_circuits_follow_the_energy():
  """qhbm_test.py:73-148: a Bernoulli energy pinned with +-1000 gives exactly one state with all the samples, the other
  pin the other state; one free bit gives the two states with about equal counts; the circuit handed back is the
  quantum inference's own."""
  num_bits, num_samples = 2, 4000
  energy = models.BernoulliEnergy(list(range(num_bits)))
  e_infer = inference.BernoulliEnergyInference(energy, num_samples, initial_seed=11)
  qubits = ir.GridQubit.rect(1, num_bits)
  circuit = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "c"))
  qhbm = inference.QHBM(e_infer, inference.AnalyticQuantumInference(circuit))
  _set(energy.post_process[0].kernel, [-1000.0, 1000.0])               # pinned to [0, 1]
  states, counts = qhbm.circuits(num_samples)
  assert states[1] is qhbm.q_inference.circuit and states[1] is circuit
  assert states[0].tolist() == [[0, 1]] and counts.tolist() == [num_samples]
  _set(energy.post_process[0].kernel, [1000.0, -1000.0])               # pinned to [1, 0]
  states, counts = qhbm.circuits(num_samples)
  assert states[0].tolist() == [[1, 0]] and counts.tolist() == [num_samples]
  _set(energy.post_process[0].kernel, [-1000.0, 0.0])                  # one free bit
  states, counts = qhbm.circuits(num_samples)
  assert sorted(states[0].tolist()) == [[0, 0], [0, 1]]
  assert int(counts.sum()) == num_samples
  assert abs(int(counts[0]) - int(counts[1])) <= 5 * np.sqrt(num_samples)   # 5 sigma of the difference of the two counts
  again, again_counts = qhbm.circuits(num_samples)                     # explicit seed: the same draw
  assert torch.equal(again[0], states[0]) and torch.equal(again_counts, counts)


@pytest.mark.parametrize("kind", ["analytic", "bernoulli"])
def test_sampler_seed_contract(kind):
  """ebm_test.py:281-297, 677-693: an explicit seed gives the same draw twice, `seed = None` lets draws change, an
  explicit seed set again restores equality."""
  num_bits, num_samples = 5, 200
  rng = np.random.default_rng(5)
  if kind == "analytic":
    energy = models.KOBE(list(range(num_bits)), 2)
    layer = inference.AnalyticEnergyInference(energy, num_samples, initial_seed=17)
  else:
    energy = models.BernoulliEnergy(list(range(num_bits)))
    layer = inference.BernoulliEnergyInference(energy, num_samples, initial_seed=17)
  _set(energy.post_process[0].kernel, rng.uniform(-0.5, 0.5, energy.post_process[0].kernel.numel()))
  first, second = layer.sample(num_samples), layer.sample(num_samples)
  assert first.shape == (num_samples, num_bits) and torch.equal(first, second)
  layer.seed = None
  assert not torch.equal(layer.sample(num_samples), layer.sample(num_samples))
  layer.seed = 17
  assert torch.equal(layer.sample(num_samples), layer.sample(num_samples))
  assert torch.equal(layer.sample(num_samples), first)


def test_gibbs_with_gradients_seed_contract():
  """The chain of ebm.py:749-760 persists between calls, so two draws from ONE inference are consecutive stretches of
  the chain and differ whatever the seed; the seed fixes the chain itself.  Two inferences built with the same explicit
  seed return identical draws, two built with `initial_seed=None` do not, and the explicit seed again restores the
  first draw."""
  num_bits, num_samples, burnin = 4, 40, 10
  thetas = np.random.default_rng(6).uniform(-0.5, 0.5, num_bits + num_bits * (num_bits - 1) // 2)

  def draws(seed):
    energy = models.KOBE(list(range(num_bits)), 2)
    _set(energy.post_process[0].kernel, thetas)
    layer = inference.GibbsWithGradientsInference(energy, num_samples, burnin, initial_seed=seed)
    return layer.sample(num_samples), layer.sample(num_samples)

  seeded, seeded_next = draws(23)
  assert torch.equal(draws(23)[0], seeded)
  assert not torch.equal(seeded, seeded_next)
  assert not torch.equal(draws(None)[0], draws(None)[0])
  again, again_next = draws(23)
  assert torch.equal(again, seeded) and torch.equal(again_next, seeded_next)
