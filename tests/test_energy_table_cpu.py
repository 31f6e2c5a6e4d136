"""Energy tables (a general BitstringEnergy measured exactly): everything that needs no GPU.

Table order against the energy itself and AnalyticEnergyInference, the `energy_tables` option and its errors (raised
before any device work), the C ABI declarations, the kernel's register budget, and the two restatements the GPU tests
use (the Walsh form of a table through O.expectation_jacobian and the diagonal adjoint) against each other."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from oracle import qhbm_oracle as O
from qhbmlib_amd import _engine as E
from qhbmlib_amd import inference, ir, models
from qhbmlib_amd.models import energy_utils
from tests import energy_table_ref as R
from tests.test_host_api import hea_circuit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("qhbm_table_expectation", "qhbm_table_expectation_retain", "qhbm_table_expectation_vjp",
                "qhbm_table_expectation_vjp_retained")


def _mlp(n, seed=3):
  return models.BitstringEnergy(list(range(n)), R.mlp_layers(n, 5, seed))


@pytest.mark.parametrize("kind", ["mlp", "kobe2"])
def test_table_row_y_is_the_energy_of_bitstring_y(kind):
  n = 6
  energy = _mlp(n) if kind == "mlp" else models.KOBE(list(range(n)), 2)
  table = energy_utils.energy_table(energy, n)
  assert table.shape == (1 << n,) and table.dtype == torch.float32
  rows = energy_utils.all_bitstrings(n)
  for y in (0, 1, 5, 34, 63):
    bits = [(y >> (n - 1 - j)) & 1 for j in range(n)]
    assert rows[y].tolist() == bits
    want = float(energy(torch.tensor([bits], dtype=torch.int8)).reshape(-1)[0].detach())
    assert abs(float(table[y].detach()) - want) <= 1e-6 * max(1.0, abs(want))   # (a batch of one may round otherwise)
  if kind == "kobe2":
    thetas = energy.post_process[0].kernel.detach().numpy()
    np.testing.assert_allclose(table.detach().numpy(), R.kobe2_table(n, thetas), rtol=1e-5, atol=1e-6)


def test_table_matches_analytic_energy_inference_order():
  n = 5
  energy = _mlp(n, 7)
  e_inf = inference.AnalyticEnergyInference(energy, 8, initial_seed=1)
  assert torch.equal(energy_utils.energy_table(energy, n), e_inf.all_energies.reshape(-1).to(torch.float32))
  assert torch.equal(energy_utils.all_bitstrings(n), e_inf.all_bitstrings)
  assert energy_utils.all_bitstrings(n) is energy_utils.all_bitstrings(n)   # cached per (n, device)


def test_table_keeps_the_graph_to_the_energy_variables():
  energy = _mlp(4)
  table = energy_utils.energy_table(energy, 4)
  (table * torch.arange(16.0)).sum().backward()
  assert all(p.grad is not None and float(p.grad.abs().sum()) > 0 for p in energy.parameters())


def test_energy_output_of_the_wrong_shape_is_refused():
  class Wide(torch.nn.Module):
    def forward(self, x):
      return torch.cat([x.float(), x.float()], 1)
  with pytest.raises(ValueError, match=r"\[8\] or \[8, 1\]"):
    energy_utils.energy_table(models.BitstringEnergy([0, 1, 2], [Wide()]), 3)


def _setup(n, **kwargs):
  qubits = ir.GridQubit.rect(1, n)
  circ = models.DirectQuantumCircuit(hea_circuit(qubits, 1, "t"))
  ham = models.Hamiltonian(_mlp(n), models.DirectQuantumCircuit(hea_circuit(qubits, 1, "h")))
  return circ, ham


def test_energy_tables_option_is_validated():
  circ, _ = _setup(2)
  with pytest.raises(ValueError, match="energy_tables"):
    inference.AnalyticQuantumInference(circ, energy_tables="yes")
  for ok in ("off", "general", "all"):
    assert inference.AnalyticQuantumInference(circ, energy_tables=ok).energy_tables == ok


def test_off_keeps_the_type_error_for_a_general_energy():
  circ, ham = _setup(2)
  with pytest.raises(TypeError, match="General Hamiltonians not accepted"):
    inference.AnalyticQuantumInference(circ).expectation(torch.zeros((1, 2), dtype=torch.int8), ham)


def test_errors_of_the_table_route_come_before_any_device_work(monkeypatch):
  def no_engine(*args, **kwargs):
    raise AssertionError("an engine was created")
  monkeypatch.setattr(E, "Engine", no_engine)
  monkeypatch.setattr(energy_utils, "energy_table", no_engine)
  circ, ham = _setup(4)
  states = torch.zeros((2, 4), dtype=torch.int8)
  with pytest.raises(ValueError, match="max_table_qubits=3"):
    inference.AnalyticQuantumInference(circ, energy_tables="general", max_table_qubits=3).expectation(states, ham)
  with pytest.raises(ValueError, match="parameter-shift"):
    inference.AnalyticQuantumInference(circ, energy_tables="general",
                                       gradient_method=E.GRAD_PARAMETER_SHIFT).expectation(states, ham)


def test_header_declares_the_entry_points_and_the_binding_lists_them():
  with open(os.path.join(ROOT, "include", "qhbm_engine.h")) as f:
    header = f.read()
  assert "#define QHBM_ABI_VERSION 5" in header
  for name in ENTRY_POINTS:
    assert re.search(r"\bint " + name + r"\(", header), name
    assert name in E.ABI_SYMBOLS


def test_energy_table_kernels_compile_without_register_spills():
  hipcc = "/opt/rocm/bin/hipcc"
  if not shutil.which(hipcc):
    pytest.skip("no hipcc")
  csrc = os.path.join(ROOT, "qhbm-library_amd", "csrc")
  out = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-disable-promote-alloca-to-vector=1",
                        "-mllvm", "-amdgpu-sched-strategy=max-ilp", "--cuda-device-only", "-c", "energy_table.hip", "-o",
                        os.devnull, "-Rpass-analysis=kernel-resource-usage"], cwd=csrc, capture_output=True, text=True,
                       timeout=600).stderr
  blocks = re.split(r"remark: Function Name: ", out)[1:]
  names = [b.split()[0] for b in blocks]
  assert sum("energy_table_kernel" in s for s in names) == 3 and len(blocks) == 5, names
  for b in blocks:
    field = lambda name: int(re.search(name + r"[^:]*: (\d+)", b).group(1))  # noqa: E731
    assert field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0 and field("ScratchSize") == 0, b[:400]
    assert field("Occupancy") >= 4, b[:400]


def test_energy_table_kernel_uses_16_byte_loads_and_stores():
  hipcc = "/opt/rocm/bin/hipcc"
  if not shutil.which(hipcc):
    pytest.skip("no hipcc")
  csrc = os.path.join(ROOT, "qhbm-library_amd", "csrc")
  asm = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-disable-promote-alloca-to-vector=1",
                        "-mllvm", "-amdgpu-sched-strategy=max-ilp", "--cuda-device-only", "-S", "energy_table.hip", "-o", "-"],
                       cwd=csrc, capture_output=True, text=True, timeout=600).stdout
  body = asm.split("energy_table_kernelILb1ELb1", 1)[1].split(".Lfunc_end", 1)[0]
  assert "global_load_dwordx4" in body and "global_store_dwordx4" in body
  assert "global_atomic" not in asm and "flat_atomic" not in asm


@pytest.mark.parametrize("n,seed", [(3, 0), (4, 1)])
def test_walsh_form_and_diagonal_adjoint_agree(n, seed):
  rng = np.random.default_rng(seed)
  gates, names = O.hea_gates(n, 2)
  params = rng.uniform(-1, 1, len(names))
  bits = rng.integers(0, 2, (3, n))
  table = R.random_table(n, rng)
  up = rng.normal(size=3)
  vals, grad, tgrad = R.oracle_vjp(n, gates, params, bits, table, up)
  dvals, djac, probs = R.diag_vjp(n, gates, params, bits, table)
  np.testing.assert_allclose(dvals, vals, atol=1e-9 * np.abs(table).max())
  np.testing.assert_allclose(up @ djac, grad, atol=1e-9 * np.abs(table).max())
  np.testing.assert_allclose(up @ probs, tgrad, atol=1e-12)
  np.testing.assert_allclose(probs @ table.astype(np.float64), vals, atol=1e-9 * np.abs(table).max())
