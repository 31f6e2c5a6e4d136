"""Parity tables by a Walsh-Hadamard transform, the part that needs no GPU: the numpy restatement
(tests/parity_table_ref.py) against the definition of the energies, the exactness conditions of the GPU tests' bit-for-bit
cases, the new kernels' resources, the C symbols, and what the mirror refuses."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from qhbmlib_amd import _engine as E
from qhbmlib_amd import inference, models
from qhbmlib_amd.models import energy_utils
from tests import parity_table_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("qhbm_walsh_hadamard", "qhbm_parity_table", "qhbm_parity_table_vjp")


@pytest.mark.parametrize("n,order", [(1, 1), (2, 2), (3, 3), (5, 2), (7, 3), (10, 1), (10, 2), (10, 3)])
def test_restatement_is_the_sum_of_spin_products_in_all_bitstrings_order(n, order):
  rng = np.random.default_rng(10 * n + order)
  sets = R.kobe_index_sets(n, order)
  thetas = rng.uniform(-1, 1, len(sets))
  masks = R.masks_of(sets)
  want = R.table_by_terms(sets, thetas, n)
  np.testing.assert_allclose(R.table(masks, thetas, n), want, atol=1e-12 * len(sets))
  # ... in the row order of the mirror's bitstring table, through the mirror's own layers
  energy = models.KOBE(list(range(n)), order)
  with torch.no_grad():
    energy.post_process[0].kernel.copy_(torch.from_numpy(thetas).float())
  layers = energy(energy_utils.all_bitstrings(n)).detach().numpy()
  np.testing.assert_allclose(R.table(masks, thetas, n), layers, atol=1e-5 * max(1.0, np.abs(thetas).sum()))
  # the VJP: sum_y w[y] parity_k(y)
  w = rng.normal(size=1 << n)
  parities = np.stack([R.table_by_terms([ix], [1.0], n) for ix in sets])
  np.testing.assert_allclose(R.vjp(masks, w, n), parities @ w, atol=1e-12 * np.abs(w).sum())


def test_restatement_pieces():
  assert R.rev_n(np.asarray([0b0011, 0b1000, 0b10110], np.uint64), 4).tolist() == [0b1100, 0b0001, 0b0110]
  masks, thetas = R.hand_made_terms(7)["three equal masks"]
  c = R.scatter(masks, thetas, 7)
  assert c[int(R.rev_n(np.uint64(5), 7))] == 0.5 + 0.25 - 0.015625 and R.multiplicity(masks, 7) == 3
  masks, thetas = R.hand_made_terms(7)["bits at or above n"]
  assert R.table(masks, thetas, 7)[0] == 0.75 and R.multiplicity(masks, 7) == 1
  assert not R.table(*R.hand_made_terms(7)["no terms"], 7).any()
  # int64 and float64 transforms agree, and single outputs by the sparse evaluation are the transform's
  x = np.random.default_rng(1).integers(-7, 8, 1 << 9)
  full = R.wht_i64(x)
  assert np.array_equal(full, R.wht_f64(x).astype(np.int64))
  support = np.flatnonzero(x).astype(np.uint64)
  ys = np.asarray([0, 1, 255, 256, 511, 77], np.uint64)
  assert np.array_equal(R.sparse_eval(support, x[support.astype(np.int64)], ys), full[ys.astype(np.int64)])
  # single term on column 0: the sign flips exactly at y >= 2^(n-1)
  t = R.table(np.asarray([1], np.uint64), [1.0], 6)
  assert np.array_equal(t, np.where(np.arange(64) >= 32, -1.0, 1.0))


def test_pass_counts_restate_the_binding_s():
  assert (R.TILE_BITS, R.ROW_BITS, R.MAX_BITS) == (E.WHT_TILE_BITS, E.WHT_ROW_BITS, E.WHT_MAX_BITS)
  for n in range(1, R.MAX_BITS + 1):
    assert R.num_passes(n) == E.walsh_hadamard_passes(n)
  assert R.num_passes(R.N2 - 1) == 1 and R.num_passes(R.N2) == 2 and R.num_passes(R.N3 - 1) == 2
  assert R.num_passes(R.N3) == 3 and R.num_passes(R.MAX_BITS) == 3
  with open(os.path.join(ROOT, "qhbm-library_amd", "csrc", "parity_table.hip")) as f:
    src = f.read()
  assert int(re.search(r"kWhtTileBits = (\d+);", src).group(1)) == R.TILE_BITS
  assert int(re.search(r"kWhtCarrierBits = (\d+);", src).group(1)) == R.TILE_BITS - R.ROW_BITS
  assert int(re.search(r"kWhtMaxBits = (\d+);", src).group(1)) == R.MAX_BITS
  assert R.raw_sizes() == list(range(1, 17)) + [23, 24, 25, 29, 30]


def test_every_exact_case_meets_its_exactness_condition():
  assert R.exactness_violations() == []
  for n in (23, 30):
    positions, values = R.raw_case(n)
    assert positions.size >= 1 << 12 and np.all(values != 0) and positions.max() < 1 << n
    assert np.isin(R.structured_indices(n), positions).all() and R.raw_outputs(n).size >= 4096
    for b in R.boundaries(n):   # a pair of bits on either side of every boundary is in the support
      assert np.isin(np.uint64((1 << (b - 1)) | (1 << b)), positions)


def test_the_new_kernels_have_no_spill_and_no_scratch():
  spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "scripts", "kernel_resources.py"))
  mod = importlib.util.module_from_spec(spec)
  spec.loader.exec_module(mod)
  rows = {r["name"].replace("qhbm::", ""): r for r in mod.resource_rows()}
  for name in ("wht_pass_kernel", "wht_small_kernel", "parity_scatter_kernel", "parity_gather_kernel"):
    assert name in rows, sorted(rows)
    row = rows[name]
    print(row)
    assert row["VGPRs Spill"] == 0 and row["SGPRs Spill"] == 0 and row["ScratchSize"] == 0, row
  # two workgroups of the pass kernel per CU: 512 threads at 4 waves per SIMD, 66 KiB of the 160 KiB of LDS each
  assert rows["wht_pass_kernel"]["Occupancy"] >= 4 and 2 * rows["wht_pass_kernel"]["LDS Size"] <= 160 * 1024


def test_the_three_symbols_are_in_the_header_the_binding_and_the_library():
  with open(os.path.join(ROOT, "include", "qhbm_engine.h")) as f:
    header = f.read()
  for sym in SYMBOLS:
    assert re.search(r"\bint " + sym + r"\(", header), sym
    assert sym in E.ABI_SYMBOLS
  assert int(re.search(r"#define QHBM_ABI_VERSION (\d+)", header).group(1)) == 5 == E.ABI_VERSION
  if not os.path.exists(E.LIB_PATH):
    pytest.skip("engine library not built")
  lib = ctypes.CDLL(E.LIB_PATH)
  for sym in SYMBOLS:
    assert hasattr(lib, sym), sym


def test_transform_refuses_what_it_cannot_run_and_defaults_are_unchanged():
  kobe = models.KOBE(list(range(5)), 2)   # variables on the host
  with pytest.raises(ValueError, match="CUDA"):
    energy_utils.energy_table(kobe, 5, method="transform")
  with pytest.raises(ValueError, match="CUDA"):
    inference.AnalyticEnergyInference(kobe, 10, table="transform")
  general = models.BitstringEnergy([0, 1, 2], [models.SpinsFromBitstrings(), torch.nn.Linear(3, 1)])
  with pytest.raises(ValueError, match="PauliMixin"):
    inference.AnalyticEnergyInference(general, 10, table="transform")
  with pytest.raises(ValueError, match="PauliMixin"):
    energy_utils.energy_table(general, 3, method="transform")
  with pytest.raises(ValueError, match="method must be"):
    energy_utils.energy_table(kobe, 5, method="fft")
  with pytest.raises(ValueError, match="table must be"):
    inference.AnalyticEnergyInference(kobe, 10, table="fwht")
  wide = models.BernoulliEnergy(list(range(31)))
  with pytest.raises(ValueError, match="at most 30 bits"):
    energy_utils.energy_table(wide, 31, max_qubits=31, method="transform")
  with pytest.raises(ValueError, match="6 bits"):
    energy_utils.energy_table(kobe, 6, method="transform")
  with pytest.raises(E.EngineError, match=r"\[1, 30\]"):
    E.parity_table(torch.zeros(1), torch.zeros(1, dtype=torch.int64), 31)
  # the defaults: today's table, today's bitstring table
  assert torch.equal(energy_utils.energy_table(kobe, 5), energy_utils.energy_table(kobe, 5, method="terms"))
  inf = inference.AnalyticEnergyInference(kobe, 10, initial_seed=1)
  assert inf.table == "bitstrings" and torch.equal(inf.all_bitstrings, energy_utils.all_bitstrings(5))
