"""complex128 numpy restatement of the weighted Gram matrix's VJP and of the gradients of the state metrics,
on the conventions of tests/state_metrics_ref.py.  No GPU, no engine; written from the formulas, not from the kernel.

Convention (torch's for a complex tensor): for a real loss L of G the cotangent is Gamma = dL/dRe G + i dL/dIm G, so that
dL = Re sum_ij conj(Gamma_ij) dG_ij; the cotangent of a state is g = dL/dRe a + i dL/dIm a.  With
G[i, j] = sum_x t(x) conj(a_i(x)) a_j(x) and H = Gamma + Gamma^H:

    c_j(x) = sum_i H[i, j] a_i(x),    g_j(x) = t(x) c_j(x),    tbar(x) = 1/2 sum_j Re(conj(c_j(x)) a_j(x)).
"""
import numpy as np

from tests import state_metrics_ref as R


def gram_vjp(states, table, hermitian):
  """(out [M, 2^n] complex128, table_grad [2^n] float64) for H = `hermitian` used as given; `table` None: ones."""
  a = np.asarray(states).astype(np.complex128)
  h = np.asarray(hermitian).astype(np.complex128)
  t = np.ones(a.shape[1]) if table is None else np.asarray(table).astype(np.float64)
  c = h.T @ a
  return t[None, :] * c, 0.5 * np.real(np.sum(c.conj() * a, axis=0))


def gram_vjp_bounds(states, table, hermitian):
  """The elementwise terms the kernel's error bound is a multiple of:
  out_bar[j, x] = |t(x)| sum_i (|Re H_ij| + |Im H_ij|) (|Re a_i(x)| + |Im a_i(x)|) and
  grad_bar[x] = 1/2 sum_j (the same sum without t) (|Re a_j(x)| + |Im a_j(x)|)."""
  a = np.asarray(states).astype(np.complex128)
  h = np.asarray(hermitian).astype(np.complex128)
  t = np.ones(a.shape[1]) if table is None else np.abs(np.asarray(table).astype(np.float64))
  abar = np.abs(a.real) + np.abs(a.imag)
  cbar = (np.abs(h.real) + np.abs(h.imag)).T @ abar
  return t[None, :] * cbar, 0.5 * np.sum(cbar * abar, axis=0)


def vjp(states, table, gamma):
  """(cotangent of the states, cotangent of the table) for torch's cotangent Gamma of G, Hermitian or not."""
  gamma = np.asarray(gamma).astype(np.complex128)
  return gram_vjp(states, table, gamma + gamma.conj().T)


# ---- real losses of a Gram matrix: (value, Gamma) -------------------------------------------------------------------------
def linear_loss(g, b):
  """Re sum_ij conj(B_ij) G_ij: Gamma = B, for any B."""
  return float(np.real(np.sum(np.conj(b) * g))), np.asarray(b, dtype=np.complex128)


def quadratic_loss(g, w):
  """Re tr(W G W G), W = diag(w): d = Re 2 tr(W G W dG) = Re sum_ij 2 (W G W)_ji dG_ij, so Gamma = 2 (W G W)^H."""
  wgw = w[:, None] * g * w[None, :]
  return float(np.real(np.trace(wgw @ g))), 2.0 * wgw.conj().T


def fidelity_loss(g, w):
  """(sum_k sqrt(lambda_k))^2 over the positive eigenvalues of B = W^1/2 (G + G^H) / 2 W^1/2: d lambda_k = v_k^H dB v_k, so
  Gamma_B = sum_k (S / sqrt(lambda_k)) v_k v_k^H with S = sum sqrt(lambda), and Gamma_G = W^1/2 Gamma_B W^1/2.  Eigenvalues
  at or below 0 contribute nothing and carry no gradient."""
  root = np.sqrt(np.asarray(w, dtype=np.float64))
  b = root[:, None] * g * root[None, :]
  lam, vec = np.linalg.eigh((b + b.conj().T) / 2)
  keep = lam > 0
  total = float(np.sum(np.sqrt(lam[keep])))
  slope = np.zeros_like(lam)
  slope[keep] = total / np.sqrt(lam[keep])
  gamma_b = (vec * slope[None, :]) @ vec.conj().T
  return total**2, root[:, None] * gamma_b * root[None, :]


def loss_of(kind, g, aux):
  return {"lin": linear_loss, "quad": quadratic_loss, "fid": fidelity_loss}[kind](g, aux)


def loss_aux(kind, num, seed):
  rng = np.random.default_rng(seed)
  if kind == "lin":
    return rng.normal(size=(num, num)) + 1j * rng.normal(size=(num, num))
  return rng.uniform(0.2, 1.0, num)


# ---- the metrics as functions of (a, E) and their gradients ---------------------------------------------------------------
def _softmax(energies):
  e = np.asarray(energies, dtype=np.float64)
  shift = (-e).max()
  log_z = shift + np.log(np.sum(np.exp(-e - shift)))
  return log_z, np.exp(-e - log_z)


def data_constants(states, weights):
  """(tr sigma, S(sigma)) of the data: U drops out of G_1, so they are constants of the model."""
  w = np.asarray(weights, dtype=np.float64)
  g1 = R.gram(np.asarray(states).astype(np.complex128))
  lam = R._spectrum(g1, w)  # pylint: disable=protected-access
  pos = lam[lam > 0]
  return float(np.sum(w * np.diag(g1).real)), float(-np.sum(pos * np.log(pos)))


def metric_values(amplitudes, energies, weights, constants=None):
  """dict of overlap, fidelity, cross_entropy, relative_entropy of sigma = sum_m w_m |phi_m><phi_m| against
  rho = U diag(softmax(-E)) U^dagger, from a_m = U^dagger phi_m (`amplitudes`) -- tests/state_metrics_ref.metrics with the
  unitary already applied.  `constants`: `data_constants` of the data, where the amplitudes are varied freely (a
  perturbed a is not a unitary image of the data; the metrics take tr sigma and S(sigma) from the data as given)."""
  a = np.asarray(amplitudes).astype(np.complex128)
  w = np.asarray(weights, dtype=np.float64)
  e = np.asarray(energies, dtype=np.float64)
  log_z, p = _softmax(e)
  gp, ge = R.gram(a, p), R.gram(a, e)
  trace, entropy = data_constants(a, w) if constants is None else constants
  cross = float(np.sum(w * np.diag(ge).real) + log_z * trace)
  return {"overlap": float(np.sum(w * np.diag(gp).real)), "fidelity": fidelity_loss(gp, w)[0], "cross_entropy": cross,
          "relative_entropy": cross - entropy}


def metric_gradients(amplitudes, energies, weights):
  """name -> (cotangent of the amplitudes [M, 2^n] complex128, gradient of the energies [2^n]) for overlap, fidelity,
  cross_entropy and relative_entropy.  Through p = softmax(-E): dp_x / dE_y = -p_x (delta_xy - p_y), so a cotangent pbar
  of p gives Ebar_y = -p_y (pbar_y - sum_x p_x pbar_x); d log Z / dE_y = -p_y.  The entropy of sigma and its trace do not
  depend on the model: they are `data_constants`."""
  a = np.asarray(amplitudes).astype(np.complex128)
  w = np.asarray(weights, dtype=np.float64)
  e = np.asarray(energies, dtype=np.float64)
  _, p = _softmax(e)
  trace = data_constants(a, w)[0]
  out = {}
  for name, gamma in (("overlap", np.diag(w).astype(np.complex128)), ("fidelity", fidelity_loss(R.gram(a, p), w)[1])):
    cot, pbar = vjp(a, p, gamma)
    out[name] = (cot, -p * (pbar - np.sum(p * pbar)))
  cot, ebar = vjp(a, e, np.diag(w).astype(np.complex128))
  out["cross_entropy"] = (cot, ebar - trace * p)
  out["relative_entropy"] = out["cross_entropy"]
  return out


def random_states(num, n, seed):
  """[num, 2^n] complex128 seeded complex Gaussians, neither orthogonal nor normalised (norms around 1)."""
  rng = np.random.default_rng(seed)
  return (rng.normal(size=(num, 1 << n)) + 1j * rng.normal(size=(num, 1 << n))) / np.sqrt(2 << n)
