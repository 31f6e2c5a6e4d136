"""Utilities for the energy module (reference: qhbmlib/models/energy_utils.py)."""
import itertools
from typing import List

import torch


def check_bits(bits: List[int]) -> List[int]:
  """energy_utils.py:23-27."""
  if len(set(bits)) != len(bits):
    raise ValueError("All entries of `bits` must be unique.")
  return bits


def check_order(order: int) -> int:
  """energy_utils.py:30-36."""
  if not isinstance(order, int):
    raise TypeError("`order` must be an integer.")
  if order <= 0:
    raise ValueError("`order` must be greater than zero.")
  return order


class SpinsFromBitstrings(torch.nn.Module):
  """|0> -> +1, |1> -> -1 (energy_utils.py:39-52)."""

  def forward(self, inputs):
    return (1 - 2 * inputs).to(torch.float32)


class VariableDot(torch.nn.Module):
  """Dot product with a same-sized trainable kernel (energy_utils.py:55-81)."""

  def __init__(self, initializer=None):
    super().__init__()
    self._initializer = initializer
    self.kernel = None

  def build(self, input_shape):
    if self.kernel is None:
      n = int(input_shape[-1])
      init = self._initializer or (lambda shape: torch.empty(shape).uniform_(-0.05, 0.05))
      self.kernel = torch.nn.Parameter(torch.as_tensor(init([n]), dtype=torch.float32).clone())

  def compute_output_shape(self, input_shape):
    self.build(input_shape)
    return list(input_shape[:-1])

  def forward(self, inputs):
    self.build(inputs.shape)
    return torch.sum(inputs * self.kernel.to(inputs.device), -1)


class Parity(torch.nn.Module):
  """Parities of all bit groups of size 1..order, in itertools.combinations order
  (energy_utils.py:84-110)."""

  def __init__(self, bits: List[int], order: int):
    super().__init__()
    bits = check_bits(bits)
    order = check_order(order)
    indices_list = []
    for i in range(1, order + 1):
      indices_list.extend(list(itertools.combinations(range(len(bits)), i)))
    self.indices = indices_list
    self.num_terms = len(indices_list)

  def compute_output_shape(self, input_shape):
    return list(input_shape[:-1]) + [self.num_terms]

  def forward(self, inputs):
    cols = [torch.prod(inputs[..., list(ix)], dim=-1) for ix in self.indices]
    return torch.stack(cols, dim=-1)


_ALL_BITSTRINGS = {}


def all_bitstrings(n: int, device=None) -> torch.Tensor:
  """int8 [2^n, n]: row y holds the bits of y read big-endian (column j = bit n-1-j of y), the order of
  `itertools.product([0, 1], repeat=n)` (ebm.py:445-447) and of a state vector's amplitudes.  Cached per (n, device)."""
  device = torch.device("cpu") if device is None else torch.device(device)
  key = (int(n), device)
  rows = _ALL_BITSTRINGS.get(key)
  if rows is None:
    index = torch.arange(1 << n, dtype=torch.int64, device=device).unsqueeze(1)
    shifts = torch.arange(n - 1, -1, -1, dtype=torch.int64, device=device).unsqueeze(0)
    rows = ((index >> shifts) & 1).to(torch.int8)
    if len(_ALL_BITSTRINGS) >= 8:
      _ALL_BITSTRINGS.clear()
    _ALL_BITSTRINGS[key] = rows
  return rows


ENERGY_TABLE_METHODS = ("terms", "transform")


def parity_transform_missing(input_energy, n: int) -> List[str]:
  """What `energy_table(..., method="transform")` lacks for this energy (strings; empty: it can run): the transform is a
  HIP kernel over the parity masks of a spin-parity energy and has no CPU fallback."""
  from qhbmlib_amd import _engine  # pylint: disable=import-outside-toplevel
  missing, sets = [], None
  if hasattr(input_energy, "_parity_index_sets") and hasattr(input_energy, "post_process"):
    try:
      sets = list(input_energy._parity_index_sets())   # pylint: disable=protected-access
    except NotImplementedError:
      sets = None
  if sets is None:
    missing.append("a PauliMixin energy with parity masks (_parity_index_sets); this one is a " +
                   type(input_energy).__name__)
  device = next(iter(input_energy.parameters()), torch.zeros(())).device
  if device.type != "cuda":
    missing.append(f"the energy's variables on a CUDA device (they are on {device})")
  if input_energy.num_bits != n:
    missing.append(f"an energy over the table's {n} bits (it has {input_energy.num_bits})")
  if n > _engine.WHT_MAX_BITS:
    missing.append(f"at most {_engine.WHT_MAX_BITS} bits (the table has {n})")
  return missing


def parity_transform_table(input_energy, n: int) -> torch.Tensor:
  """float32 [2^n] energies of a spin-parity energy in `all_bitstrings(n)` order by `_engine.parity_table`."""
  from qhbmlib_amd import _engine  # pylint: disable=import-outside-toplevel
  missing = parity_transform_missing(input_energy, n)
  if missing:
    raise ValueError("an energy table by the Walsh-Hadamard transform needs " + "; ".join(missing))
  kernel = input_energy.post_process[0].kernel
  return _engine.parity_table(kernel, input_energy._parity_masks(kernel.device), n)   # pylint: disable=protected-access


def energy_table(input_energy, n: int, max_qubits: int = 24, method: str = "terms") -> torch.Tensor:
  """float32 [2^n]: E[y] = input_energy(row y of `all_bitstrings(n)`), the diagonal of the energy's operator in the
  computational basis, evaluated on the device of the energy's variables and differentiable with respect to them.
  `method`: "terms" (default) evaluates the energy on the bitstring table; "transform" builds the table of a spin-parity
  energy (`BernoulliEnergy`, `KOBE`) by a Walsh-Hadamard transform of its coefficients -- it needs a
  `PauliMixin` energy with parity masks, CUDA variables and `num_bits == n <= 30`, and raises `ValueError` otherwise."""
  if method not in ENERGY_TABLE_METHODS:
    raise ValueError(f"method must be one of {ENERGY_TABLE_METHODS}, got {method!r}")
  if n > max_qubits:
    raise ValueError(f"an energy table over {n} qubits has 2^{n} entries: above max_table_qubits = {max_qubits}")
  if method == "transform":
    return parity_transform_table(input_energy, n)
  device = next(iter(input_energy.parameters()), torch.zeros(())).device
  e = input_energy(all_bitstrings(n, device))
  if e.numel() != 1 << n or not (e.dim() == 1 or (e.dim() == 2 and e.shape[1] == 1)):
    raise ValueError(f"the energy of {1 << n} bitstrings must have shape [{1 << n}] or [{1 << n}, 1], "
                     f"got {tuple(e.shape)}")
  return e.reshape(-1).to(torch.float32)
