"""complex128 numpy restatement of the cross-Gram matrix's VJP, on the conventions of tests/cross_gram_ref.py
and tests/state_metrics_vjp_ref.py.  No GPU, no engine; written from the formulas, not from the kernel.

Convention (torch's for a complex tensor): for a real loss L of C the cotangent is Gamma = dL/dRe C + i dL/dIm C, [M, K], so
that dL = Re sum_ij conj(Gamma_ij) dC_ij; the cotangent of a state is g = dL/dRe a + i dL/dIm a.  With
C[i, j] = sum_x t(x) conj(a_i(x)) b_j(x) and Gamma used as given:

    c_j(x) = sum_i Gamma[i, j] a_i(x),    gbar_b_j(x) = t(x) c_j(x),    gbar_a_i(x) = t(x) sum_j conj(Gamma[i, j]) b_j(x),
    tbar(x) = Re sum_j conj(c_j(x)) b_j(x).
"""
import numpy as np


def _inputs(bras, kets, table, gamma):
  a = np.asarray(bras).astype(np.complex128)
  b = np.asarray(kets).astype(np.complex128)
  g = np.asarray(gamma).astype(np.complex128)
  assert g.shape == (a.shape[0], b.shape[0]) and a.shape[1] == b.shape[1]
  t = np.ones(a.shape[1]) if table is None else np.asarray(table).astype(np.float64)
  return a, b, t, g


def vjp(bras, kets, table, gamma):
  """(cotangent of the bras [M, 2^n], of the kets [K, 2^n] complex128, of the table [2^n] float64) for torch's cotangent
  `gamma` [M, K] of C; `table` None: ones."""
  a, b, t, g = _inputs(bras, kets, table, gamma)
  c = g.T @ a
  return t[None, :] * (g.conj() @ b), t[None, :] * c, np.real(np.sum(c.conj() * b, axis=0))


def vjp_bounds(bras, kets, table, gamma):
  """The elementwise terms the kernel's error bound is a multiple of: |t(x)| T_s(x) for the bras' and the kets' outputs,
  T_s(x) = sum_r (|Re W_rs| + |Im W_rs|) (|Re src_r(x)| + |Im src_r(x)|) over the source rows of the side, and for the table
  sum_j T_j(x) (|Re b_j(x)| + |Im b_j(x)|) with the kets' T (no t)."""
  a, b, t, g = _inputs(bras, kets, table, gamma)
  abar, bbar = np.abs(a.real) + np.abs(a.imag), np.abs(b.real) + np.abs(b.imag)
  gbar = np.abs(g.real) + np.abs(g.imag)
  cbar = gbar.T @ abar
  return np.abs(t)[None, :] * (gbar @ bbar), np.abs(t)[None, :] * cbar, np.sum(cbar * bbar, axis=0)


def linear_loss(c, b):
  """Re sum_ij conj(B_ij) C_ij: Gamma = B, for any B."""
  return float(np.real(np.sum(np.conj(b) * c))), np.asarray(b, dtype=np.complex128)


def random_case(n, num_a, num_b, seed):
  """(bras [M, 2^n], kets [K, 2^n] complex128 seeded Gaussians with norms around 1, a signed table [2^n], a non-Hermitian
  complex B [M, K])."""
  rng = np.random.default_rng(seed)
  dim = 1 << n
  bras = (rng.normal(size=(num_a, dim)) + 1j * rng.normal(size=(num_a, dim))) / np.sqrt(2 * dim)
  kets = (rng.normal(size=(num_b, dim)) + 1j * rng.normal(size=(num_b, dim))) / np.sqrt(2 * dim)
  return bras, kets, rng.normal(size=dim), rng.normal(size=(num_a, num_b)) + 1j * rng.normal(size=(num_a, num_b))
