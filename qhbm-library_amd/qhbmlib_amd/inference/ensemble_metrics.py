"""Overlap, fidelity and trace distance of two state-vector ensembles, and transition elements, matrix-free.

For sigma = sum_m w_m |a_m><a_m| and tau = sum_k v_k |b_k><b_k| given as M and K state vectors, every number here is a
function of three small matrices: the ensembles' own Gram matrices G_A [M, M] and G_B [K, K] (`_engine.weighted_gram`) and
the cross-Gram matrix C[i, j] = <a_i|b_j> [M, K] (`_engine.cross_gram`), all summed in float64 in one fixed order by the
HIP engine from the states where they lie.  With A = [sqrt(w_m) a_m] and B = [sqrt(v_k) b_k] as columns and
X = A^dagger B = W^1/2 C V^1/2:

    tr(sigma tau) = ||X||_F^2
    (tr sqrt(sqrt(sigma) tau sqrt(sigma)))^2 = (sum of the singular values of X)^2
        (sigma = A A^dagger gives A = sqrt(sigma) times a partial isometry, so A^dagger B and sqrt(sigma) sqrt(tau) have one
        nuclear norm)
    the non-zero spectrum of sigma - tau = [A B] J [A B]^dagger is that of J Gamma, Gamma = [A B]^dagger [A B] (blocks
        W^1/2 G_A W^1/2, X, X^dagger, V^1/2 G_B V^1/2), J = diag(1_M, -1_K)

Everything after the three kernel calls is float64 on the host on matrices of M + K rows.  Nothing here is differentiable
and nothing is sharded over ranks; the relative entropy of two ensembles is not offered (their supports need not nest).
"""
import dataclasses

import torch

from qhbmlib_amd import _engine
from qhbmlib_amd.inference import reduced
from qhbmlib_amd.inference import thermal

# Gamma = R^dagger R by Cholesky is used while the smallest pivot of Gamma is above this fraction of its largest diagonal
# entry (sqrt of the float64 epsilon: the Hermitian route's error grows like 2^-53 sqrt(cond Gamma)); below it
# Gamma is singular to working precision and the spectrum comes from J Gamma itself.
SINGULAR_PIVOT = 2.0**-26


@dataclasses.dataclass(frozen=True)
class EnsembleMetrics:
  """What `ensemble_metrics` returns; python floats (float64), nothing normalised: sigma and tau as given, `trace_a` and
  `trace_b` say what they sum to."""
  trace_a: float         # tr sigma
  trace_b: float         # tr tau
  purity_a: float        # tr sigma^2
  purity_b: float        # tr tau^2
  overlap: float         # tr(sigma tau)
  fidelity: float        # (tr sqrt(sqrt(sigma) tau sqrt(sigma)))^2
  trace_distance: float  # 1/2 ||sigma - tau||_1


def _scaled(gram, left, right):
  return left.unsqueeze(1) * gram * right.unsqueeze(0)


def difference_spectrum(gamma, num_a):
  """(the non-zero eigenvalues of sigma - tau, padded with rounded zeros, as a float64 tensor of M + K entries; which route
  gave them: "cholesky" or "general").  `gamma`: the complex128 Gram matrix of [A B] on the host, `num_a` = M.

  Gamma = R^dagger R (Cholesky) turns J Gamma into the Hermitian R J R^dagger with the same spectrum: `eigvalsh`.  Where
  the factorisation fails or a pivot falls below SINGULAR_PIVOT of the largest diagonal entry -- linearly dependent states,
  sigma = tau -- no root of a near-null Gamma is taken: the eigenvalues are those of the general matrix J Gamma (`eigvals`),
  whose real parts are returned."""
  size = gamma.shape[0]
  sign = torch.ones(size, dtype=torch.float64)
  sign[num_a:] = -1.0
  gamma = 0.5 * (gamma + gamma.conj().transpose(0, 1))
  top = float(gamma.diagonal().real.max())
  if top > 0.0:
    lower, info = torch.linalg.cholesky_ex(gamma)
    if int(info) == 0 and float(lower.diagonal().real.min())**2 > SINGULAR_PIVOT * top:
      upper = lower.conj().transpose(0, 1)  # R
      middle = (upper * sign.unsqueeze(0).to(torch.complex128)) @ lower  # R J R^dagger
      return torch.linalg.eigvalsh(0.5 * (middle + middle.conj().transpose(0, 1))), "cholesky"
  return torch.linalg.eigvals(sign.unsqueeze(1).to(torch.complex128) * gamma).real, "general"


def metrics_from_grams(gram_a, gram_b, cross, weights_a, weights_b):
  """`EnsembleMetrics` from G_A [M, M], G_B [K, K], C [M, K] (complex128) and the weights (float64 [M], [K]), on the host:
  the formulas of this module without a kernel call."""
  gram_a, gram_b, cross = (torch.as_tensor(g).detach().to(device="cpu", dtype=torch.complex128) for g in (gram_a, gram_b, cross))
  w = torch.as_tensor(weights_a).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
  v = torch.as_tensor(weights_b).detach().to(device="cpu", dtype=torch.float64).reshape(-1)
  num_a, num_b = int(w.shape[0]), int(v.shape[0])
  if tuple(gram_a.shape) != (num_a, num_a) or tuple(gram_b.shape) != (num_b, num_b) or tuple(cross.shape) != (num_a, num_b):
    raise ValueError(f"Gram matrices {tuple(gram_a.shape)}, {tuple(gram_b.shape)}, {tuple(cross.shape)} do not fit "
                     f"{num_a} and {num_b} weights")
  if bool((w < 0).any()) or bool((v < 0).any()):
    raise ValueError("the weights of a mixture are not negative")
  root_w, root_v = torch.sqrt(w).to(torch.complex128), torch.sqrt(v).to(torch.complex128)
  block_a, block_b, x = _scaled(gram_a, root_w, root_w), _scaled(gram_b, root_v, root_v), _scaled(cross, root_w, root_v)
  gamma = torch.cat([torch.cat([block_a, x], 1), torch.cat([x.conj().transpose(0, 1), block_b], 1)], 0)
  lam, _ = difference_spectrum(gamma, num_a)
  return EnsembleMetrics(
      trace_a=float(block_a.diagonal().real.sum()), trace_b=float(block_b.diagonal().real.sum()),
      purity_a=float(torch.sum(block_a.real**2 + block_a.imag**2)), purity_b=float(torch.sum(block_b.real**2 + block_b.imag**2)),
      overlap=float(torch.sum(x.real**2 + x.imag**2)), fidelity=float(torch.sum(torch.linalg.svdvals(x))**2),
      trace_distance=float(0.5 * torch.sum(torch.abs(lam))))


def _weights(weights, num):
  if weights is None:
    return torch.ones(num, dtype=torch.float64)
  return weights.detach().to(device="cpu", dtype=torch.float64).reshape(-1)


def ensemble_metrics(a, b) -> EnsembleMetrics:
  """Metrics of sigma = sum_m w_m |a_m><a_m| against tau = sum_k v_k |b_k><b_k|, two ensembles of state vectors on the same
  qubits, matrix-free.  `a`, `b`: sources of the kind `reduced_density_matrix` takes -- `StateVectorData`, a `ThermalEnsemble`
  (through `.data()`), or a `(states, weights)` pair ([M, 2^n] complex, [M] or None for ones).  The states are neither
  orthogonal nor normalised by assumption.

  The values are for the operators AS GIVEN, not normalised (`StateMetrics`' convention): `trace_a`, `trace_b` say what
  sigma and tau sum to; `overlap` = tr(sigma tau), `fidelity` = (tr sqrt(sqrt(sigma) tau sqrt(sigma)))^2 (divide by
  trace_a trace_b for that of the normalised operators), `trace_distance` = 1/2 ||sigma - tau||_1.

  Three kernel calls in the HIP engine -- G_A, G_B (`weighted_gram`) and the cross-Gram matrix C (`cross_gram`), float64 in
  a fixed order --, then host float64 on (M + K)-sized matrices: the fidelity from `svdvals(X)`, the trace distance from the
  eigenvalues of R J R^dagger with Gamma = R^dagger R, or of J Gamma itself where Gamma is singular to working precision
  (`difference_spectrum`).  Sources on different qubit lists or of different widths are refused.  Not differentiable."""
  states_a, w, qubits_a, n_a = reduced._source(a)  # pylint: disable=protected-access
  states_b, v, qubits_b, n_b = reduced._source(b)  # pylint: disable=protected-access
  if n_a != n_b:
    raise ValueError(f"the ensembles live on {n_a} and {n_b} qubits")
  if qubits_a is not None and qubits_b is not None and list(qubits_a) != list(qubits_b):
    raise ValueError("the ensembles' qubits are not the same")
  if states_a.device != states_b.device:
    raise ValueError("the ensembles' states are on different devices")
  w, v = _weights(w, states_a.shape[0]), _weights(v, states_b.shape[0])
  with torch.no_grad():
    gram_a = _engine.weighted_gram(states_a)
    gram_b = _engine.weighted_gram(states_b)
    cross = _engine.cross_gram(states_a, states_b)
  return metrics_from_grams(gram_a, gram_b, cross, w, v)


def matrix_elements(operators, bras, kets, weights=None, qubits=None):
  """complex128 [M, K] on the device: <a_i| sum_t weights[t] operators[t] |b_j> for bras [M, 2^n] and kets [K, 2^n]
  (complex, amplitude index = the bitstring read big-endian over the sorted qubits; default weights: ones).  One
  `qhbm_apply_observables` on the kets (float32, K more states resident), then one `cross_gram`.  Transition elements, and
  with bras = kets the Rayleigh matrix of a subspace.  Not differentiable."""
  operators = thermal._operator_list(operators)  # pylint: disable=protected-access
  qubits = thermal._qubits_of(operators, qubits)  # pylint: disable=protected-access
  n = len(qubits)
  bras = thermal._check_states(bras, n)  # pylint: disable=protected-access
  kets = thermal._check_states(kets, n)  # pylint: disable=protected-access
  eng = thermal._engine_for(operators, qubits)  # pylint: disable=protected-access
  with torch.no_grad():
    applied = eng.apply_observables(kets.detach(), weights)
    bras = bras.detach().to(device=applied.device, dtype=torch.complex64)
    out = _engine.cross_gram(bras, applied)
  eng.close()
  return out
