"""A complex128 numpy restatement of `qhbm_subsystem_apply` and of the VJP of the reduced density matrix.

    apply:  out_m(a, b) = scale_m sum_a' A[a, a'] phi_m(a', b),     dots_m = <phi_m|(A (x) 1)|phi_m>   (before scaling)
    vjp:    for rho_A = sum_m w_m Phi_m Phi_m^H (Phi_m: phi_m as a 2^k x 2^(n-k) matrix) and a real loss L with torch's cotangent
            Gamma = dL/dRe rho + i dL/dIm rho, so that dL = Re tr(Gamma^H drho),
              grad_states_m  = w_m (Gamma + Gamma^H) Phi_m       (torch's convention again: dL = sum_m Re<grad_m|dphi_m>)
              grad_weights_m = Re tr(Gamma^H Phi_m Phi_m^H) = 1/2 <phi_m|((Gamma + Gamma^H) (x) 1)|phi_m>

Index conventions are those of tests/reduced_density_ref.py (qubit 0 is the most significant bit of an amplitude index; a
reads the kept qubits big-endian in ascending order, b the others): numpy's axis bookkeeping, no bit masks, nothing of the
engine.  Three losses of rho_A, each as (value, Gamma):
  (a) trace_loss       Re tr(rho B)                 Gamma = B^H            (B Hermitian: Gamma = B)
  (b) purity_loss      tr(rho rho^H)                Gamma = 2 rho
  (c) frobenius_loss   ||rho - tau||_F^2            Gamma = 2 (rho - tau)
and `linear_loss`, Re tr(Gamma^H rho) for ANY complex Gamma, whose cotangent is that Gamma.
"""
import numpy as np

from tests import reduced_density_ref as R


def _axes(n, kept):
  kept = sorted(int(q) for q in kept)
  env = [q for q in range(n) if q not in kept]
  return kept, env


def to_panels(states, kept):
  """[M, 2^k, 2^(n-k)] complex128 copy of the states, kept qubits first."""
  return np.ascontiguousarray(R._panels(states, kept)).astype(np.complex128)  # pylint: disable=protected-access


def from_panels(panels, n, kept):
  """The inverse of `to_panels`: [M, 2^n]."""
  kept, env = _axes(n, kept)
  num = panels.shape[0]
  order = [1 + q for q in kept] + [1 + q for q in env]  # axis j of the panel view is axis order[j] of the state
  inverse = np.argsort([0] + order)
  return panels.reshape([num] + [2] * n).transpose(inverse).reshape(num, 1 << n)


def apply(states, kept, operator, scale=None):
  """(out [M, 2^n], dots [M], out_bound [M, 2^n], dots_bound [M]): the bounds are (|Re A| + |Im A|) (|Re phi| + |Im phi|)
  per output, times |scale_m|, and the same summed against |Re phi| + |Im phi| -- what the rounding error of a sum of
  the products in any order is proportional to."""
  states = np.asarray(states)
  num, dim = states.shape
  n = dim.bit_length() - 1
  panels = to_panels(states, kept)
  operator = np.asarray(operator).astype(np.complex128)
  s = np.ones(num) if scale is None else np.asarray(scale, dtype=np.float64).reshape(num)
  applied = np.einsum("ac,mcb->mab", operator, panels)
  dots = np.einsum("mab,mab->m", panels.conj(), applied)
  a_bar = np.abs(operator.real) + np.abs(operator.imag)
  p_bar = np.abs(panels.real) + np.abs(panels.imag)
  applied_bar = np.einsum("ac,mcb->mab", a_bar, p_bar)
  dots_bar = np.einsum("mab,mab->m", p_bar, applied_bar)
  out = from_panels(applied * s[:, None, None], n, kept)
  out_bar = from_panels(applied_bar * np.abs(s)[:, None, None], n, kept)
  return out, dots, out_bar.real, dots_bar


def vjp(states, weights, kept, gamma):
  """(grad_states [M, 2^n] complex128, grad_weights [M] float64) of rho_A = `reduced_density_ref.reduced(states, kept, weights)`
  for the cotangent `gamma`; written from the derivation, not through `apply`."""
  states = np.asarray(states)
  num, dim = states.shape
  n = dim.bit_length() - 1
  panels = to_panels(states, kept)
  w = np.ones(num) if weights is None else np.asarray(weights, dtype=np.float64).reshape(num)
  gamma = np.asarray(gamma).astype(np.complex128)
  hermitian = gamma + gamma.conj().T
  grad_panels = w[:, None, None] * np.einsum("ac,mcb->mab", hermitian, panels)
  grad_weights = np.real(np.einsum("ca,mcb,mab->m", gamma.conj(), panels, panels.conj()))  # Re tr(Gamma^H Phi Phi^H)
  return from_panels(grad_panels, n, kept), grad_weights


def trace_loss(rho, b):
  return float(np.real(np.trace(rho @ b))), np.asarray(b).conj().T.astype(np.complex128)


def purity_loss(rho):
  return float(np.real(np.sum(rho * rho.conj()))), 2.0 * rho


def frobenius_loss(rho, tau):
  return float(np.sum(np.abs(rho - tau)**2)), 2.0 * (rho - tau)


def linear_loss(rho, gamma):
  return float(np.real(np.sum(np.conj(gamma) * rho))), np.asarray(gamma).astype(np.complex128)


def loss_of(kind, rho, aux):
  return {"a": trace_loss, "b": purity_loss, "c": frobenius_loss, "lin": linear_loss}[kind](rho, *aux)


def loss_aux(kind, k, seed):
  """Seeded auxiliary data of a loss on k kept qubits: (B,) Hermitian, (), (tau,) a density matrix, (Gamma,) general."""
  rng = np.random.default_rng(seed)
  dim = 1 << k
  g = rng.normal(size=(dim, dim)) + 1j * rng.normal(size=(dim, dim))
  if kind == "a":
    return (0.5 * (g + g.conj().T),)
  if kind == "b":
    return ()
  if kind == "c":
    tau = g @ g.conj().T
    return (tau / np.trace(tau).real,)
  return (g,)


def random_states(num, n, seed):
  rng = np.random.default_rng(seed)
  states = rng.normal(size=(num, 1 << n)) + 1j * rng.normal(size=(num, 1 << n))
  return states / np.linalg.norm(states, axis=1, keepdims=True)
