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

Everything after the three kernel calls is float64 on the host on matrices of M + K rows.  Nothing is sharded over ranks;
the relative entropy of two ensembles is not offered (their supports need not nest).

With `differentiable=True` the same numbers are autograd nodes over the states and weights of `(states, weights)` sources
(DESIGN.md 6q): G_A and G_B go through `inference.weighted_gram`, C through `differentiable_cross_gram`, whose backward is one
`_engine.cross_gram_vjp` from the cotangent of C to those of bras, kets and table, and the host formulas run as torch float64
ops under autograd.
"""
import dataclasses
import warnings

import torch

from qhbmlib_amd import _engine
from qhbmlib_amd.inference import reduced
from qhbmlib_amd.inference import state_metrics
from qhbmlib_amd.inference import thermal

# Gamma = R^dagger R by Cholesky is used while the smallest pivot of Gamma is above this fraction of its largest diagonal
# entry (sqrt of the float64 epsilon: the Hermitian route's error grows like 2^-53 sqrt(cond Gamma)); below it
# Gamma is singular to working precision and the spectrum comes from J Gamma itself.
SINGULAR_PIVOT = 2.0**-26


@dataclasses.dataclass(frozen=True)
class EnsembleMetrics:
  """What `ensemble_metrics` returns; python floats (float64; 0-dim float64 tensors with `differentiable=True`), nothing
  normalised: sigma and tau as given, `trace_a` and `trace_b` say what they sum to."""
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
  top = float(gamma.detach().diagonal().real.max())
  if top > 0.0:
    lower, info = torch.linalg.cholesky_ex(gamma)
    if int(info) == 0 and float(lower.detach().diagonal().real.min())**2 > SINGULAR_PIVOT * top:
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


class _CrossGramFunction(torch.autograd.Function):
  """C of (bras [M, 2^n], kets [K, 2^n] complex on the device, table [2^n] real or None) as an autograd node.  Forward is
  `_engine.cross_gram`; backward one `_engine.cross_gram_vjp` of the cotangent as given.  Bras, kets and the
  table stay resident for backward.  Once differentiable only: the backward is a kernel call without a graph of its own."""

  @staticmethod
  def forward(ctx, bras, kets, table):
    ctx.has_table = table is not None
    ctx.save_for_backward(*((bras, kets, table) if ctx.has_table else (bras, kets)))
    return _engine.cross_gram(bras, kets, table)

  @staticmethod
  @torch.autograd.function.once_differentiable
  def backward(ctx, gamma):
    bras, kets = ctx.saved_tensors[0], ctx.saved_tensors[1]
    table = ctx.saved_tensors[2] if ctx.has_table else None
    need_bras, need_kets = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    need_table = ctx.has_table and ctx.needs_input_grad[2]
    if not (need_bras or need_kets or need_table):
      return None, None, None
    out_bras, out_kets, grad = _engine.cross_gram_vjp(bras, kets, table, gamma.to(torch.complex64), want_bras=need_bras,
                                                      want_kets=need_kets, want_table=need_table)
    return (out_bras.to(bras.dtype) if need_bras else None, out_kets.to(kets.dtype) if need_kets else None,
            grad.to(table.dtype) if need_table else None)


def differentiable_cross_gram(bras, kets, table=None):
  """C[i, j] = sum_x table[x] conj(bras[i, x]) kets[j, x] (table None: ones) of M bras [M, 2^n] and K kets [K, 2^n] on the
  device: complex128 [M, K] with the bits of `_engine.cross_gram`, as an autograd node over `bras`, `kets` and `table`,
  whichever require grad.  The table is a real tensor on the states' device (float32 in the kernel: a float64
  table is cast, its gradient comes back in its own dtype); the states are used as complex64.  For a real loss with cotangent
  Gamma of C, backward casts Gamma to complex64 and makes one engine call that computes only what is asked for: the kets
  receive table * c_j with c_j = sum_i Gamma[i, j] bras[i], the bras table * sum_j conj(Gamma[i, j]) kets[j], the table
  sum_j Re(conj(c_j) kets[j]).  Double backward is refused.  (`inference.cross_gram` stays the plain engine call.)"""
  for name, states in (("bras", bras), ("kets", kets)):
    if not (torch.is_tensor(states) and states.is_cuda and states.dim() == 2 and states.is_complex()):
      raise _engine.EngineError(f"differentiable_cross_gram needs complex CUDA {name} [M, 2^n]: the engine has no CPU fallback")
  if table is not None:
    if not (torch.is_tensor(table) and table.is_cuda and table.device == bras.device):
      raise _engine.EngineError("differentiable_cross_gram needs the table on the states' device")
    if table.is_complex() or not table.is_floating_point():
      raise ValueError(f"table must be a real floating-point tensor, got {table.dtype}")
    if tuple(table.shape) != (bras.shape[1],):
      raise ValueError(f"table must have shape [{bras.shape[1]}], got {tuple(table.shape)}")
  return _CrossGramFunction.apply(bras, kets, table)


def differentiable_metrics_from_grams(gram_a, gram_b, cross, weights_a, weights_b):
  """`metrics_from_grams` as torch float64 ops on the host under autograd: the same formulas, 0-dim float64 tensors.  In the
  fidelity, singular values of X at or below SINGULAR_PIVOT of the largest -- rounded zeros of a rank-deficient X, where the
  nuclear norm has no derivative -- contribute nothing and carry no gradient.  The trace distance carries a gradient on the
  Cholesky route only; where `difference_spectrum` takes the general route its value is a constant, with a warning."""
  gram_a, gram_b, cross = (g.to(device="cpu", dtype=torch.complex128) for g in (gram_a, gram_b, cross))
  w = weights_a.to(device="cpu", dtype=torch.float64).reshape(-1)
  v = weights_b.to(device="cpu", dtype=torch.float64).reshape(-1)
  num_a, num_b = int(w.shape[0]), int(v.shape[0])
  if tuple(gram_a.shape) != (num_a, num_a) or tuple(gram_b.shape) != (num_b, num_b) or tuple(cross.shape) != (num_a, num_b):
    raise ValueError(f"Gram matrices {tuple(gram_a.shape)}, {tuple(gram_b.shape)}, {tuple(cross.shape)} do not fit "
                     f"{num_a} and {num_b} weights")
  if bool((w < 0).any()) or bool((v < 0).any()):
    raise ValueError("the weights of a mixture are not negative")
  root_w, root_v = torch.sqrt(w).to(torch.complex128), torch.sqrt(v).to(torch.complex128)
  block_a, block_b, x = _scaled(gram_a, root_w, root_w), _scaled(gram_b, root_v, root_v), _scaled(cross, root_w, root_v)
  gamma = torch.cat([torch.cat([block_a, x], 1), torch.cat([x.conj().transpose(0, 1), block_b], 1)], 0)
  singular = torch.linalg.svdvals(x)
  top = singular.detach().max()
  fidelity = torch.sum(singular[singular.detach() > SINGULAR_PIVOT * top])**2
  lam, route = difference_spectrum(gamma, num_a)
  distance = 0.5 * torch.sum(torch.abs(lam))
  if route != "cholesky":
    distance = distance.detach()
    if gamma.requires_grad:
      warnings.warn("ensemble_metrics: the joint Gram matrix is singular to working precision, so the trace distance comes "
                    "from the general eigenvalue route and is returned as a constant without a gradient")
  return EnsembleMetrics(
      trace_a=block_a.diagonal().real.sum(), trace_b=block_b.diagonal().real.sum(),
      purity_a=torch.sum(block_a.real**2 + block_a.imag**2), purity_b=torch.sum(block_b.real**2 + block_b.imag**2),
      overlap=torch.sum(x.real**2 + x.imag**2), fidelity=fidelity, trace_distance=distance)


def _weights(weights, num):
  if weights is None:
    return torch.ones(num, dtype=torch.float64)
  return weights.detach().to(device="cpu", dtype=torch.float64).reshape(-1)


def _source(source, differentiable):
  """`reduced._source`; with `differentiable`, a `(states, weights)` pair keeps its graph on the way to the device (complex64
  states, float64 weights), and every other source is a constant as before."""
  found = reduced._source(source)  # pylint: disable=protected-access  (validates, detached)
  if not (differentiable and isinstance(source, (tuple, list))):
    return found
  states, weights = source
  if torch.is_tensor(states) and states.requires_grad:
    found = (states.to(device=found[0].device, dtype=torch.complex64),) + tuple(found[1:])
  if torch.is_tensor(weights) and weights.requires_grad:
    found = (found[0], weights.to(torch.float64).reshape(-1)) + tuple(found[2:])
  return found


def _differentiable_weights(weights, num):
  if weights is None:
    return torch.ones(num, dtype=torch.float64)
  return weights.to(device="cpu", dtype=torch.float64).reshape(-1)


def _gram_node(states):
  """G of one ensemble: the autograd node where the states carry a graph, the plain engine call (the same bits) otherwise."""
  if states.requires_grad:
    return state_metrics.weighted_gram(states)
  with torch.no_grad():
    return _engine.weighted_gram(states)


def ensemble_metrics(a, b, differentiable: bool = False) -> EnsembleMetrics:
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
  (`difference_spectrum`).  Sources on different qubit lists or of different widths are refused.
  `differentiable=False` (default): reported numbers, python floats, no graph.

  `differentiable=True`: the same `EnsembleMetrics` with 0-dim float64 tensors (on the host), autograd nodes over the states
  and weights of `(states, weights)` sources that require grad -- the output of `final_states_from_states`, say, against a
  fixed target; `StateVectorData` and `ThermalEnsemble` sources are constants.  The three matrices have the
  bits of the default path: G_A and G_B through `inference.weighted_gram`, C through `differentiable_cross_gram`, one fused
  kernel call each in backward.  In the fidelity, singular values of X at or below 2^-26 of the largest contribute nothing
  and carry no gradient.  The trace distance carries a gradient on the Cholesky route only: where Gamma is singular to
  working precision its value is the default path's, a constant, and a warning says so.  The states and their cotangents are
  resident together until backward; double backward is refused."""
  states_a, w, qubits_a, n_a = _source(a, differentiable)
  states_b, v, qubits_b, n_b = _source(b, differentiable)
  if n_a != n_b:
    raise ValueError(f"the ensembles live on {n_a} and {n_b} qubits")
  if qubits_a is not None and qubits_b is not None and list(qubits_a) != list(qubits_b):
    raise ValueError("the ensembles' qubits are not the same")
  if states_a.device != states_b.device:
    raise ValueError("the ensembles' states are on different devices")
  if differentiable:
    w, v = _differentiable_weights(w, states_a.shape[0]), _differentiable_weights(v, states_b.shape[0])
    if states_a.requires_grad or states_b.requires_grad:
      cross = differentiable_cross_gram(states_a, states_b)
    else:
      with torch.no_grad():
        cross = _engine.cross_gram(states_a, states_b)
    return differentiable_metrics_from_grams(_gram_node(states_a), _gram_node(states_b), cross, w, v)
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
