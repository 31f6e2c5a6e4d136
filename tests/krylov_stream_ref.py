"""Two-pass restatement of the streamed Lanczos routines (include/qhbm_engine.h qhbm_krylov_tridiagonal, qhbm_krylov_replay;
DESIGN.md 6o), for the tests.  The product never imports it.  Built on `krylov_ref` and `thermal_ref.apply_h`.

Pass one (`tridiagonal`) is `krylov_ref.lanczos(reorth=False)` on a ring of THREE vectors: it keeps alpha, beta, the
lengths and the pair of coefficients (c_{j-1}, c_j) each step subtracted, (0, c_0) for j = 0, rounded as they were used.
Pass two (`replay`) regenerates every v_j from the start states, beta and those pairs with no inner product,
  v_0 = phi / ||phi||;  v_{j+1} = (H v_j - c_{j-1} v_{j-1} - c_j v_j) * (1 / beta_j, or 0 where beta_j = 0),
and adds coef[u, s, j] v_j into the outputs as it passes, j ascending: never more than three vectors and the outputs.
`dtype=np.float32` is `krylov_ref.lanczos`'s fp32 mode: the arithmetic of the device."""
import numpy as np

from tests import krylov_ref as K
from tests import thermal_ref as T

RING = 3


def _import(starts, cdtype):
  norms = np.linalg.norm(starts.astype(np.complex128), axis=1)
  scale = np.where(norms > 0, 1.0 / np.where(norms > 0, norms, 1.0), 0.0)
  return (starts.astype(np.complex128) * scale[:, None]).astype(cdtype), norms


def tridiagonal(n, ops, starts, m, weights=None, dtype=np.float64):
  """(alpha [U, m], beta [U, m], lengths [U] int32, recurrence [U, m, 2], start norms [U]) as `Engine.krylov_tridiagonal`."""
  cdtype = np.complex64 if dtype == np.float32 else np.complex128
  starts = np.asarray(starts, cdtype)
  num = starts.shape[0]
  threshold = K.BREAKDOWN * T.radius(n, ops, weights)
  ring = [None] * RING
  ring[0], norms = _import(starts, cdtype)
  alpha, beta = np.zeros((num, m)), np.zeros((num, m))
  recurrence = np.zeros((num, m, 2), cdtype)
  lengths = np.where(norms > 0, m, 0).astype(np.int32)
  live = norms > 0
  for j in range(m):
    w = T.apply_h(n, ops, ring[j % RING], weights, dtype).astype(cdtype)
    lo = max(0, j - 1)
    rows = np.stack([ring[i % RING] for i in range(lo, j + 1)]).astype(np.complex128)
    coef = np.einsum("iud,ud->iu", rows.conj(), w.astype(np.complex128))
    alpha[:, j] += coef[j - lo].real
    coef = coef.astype(cdtype)
    recurrence[:, j, 2 - len(coef):] = coef.T
    for i in range(lo, j + 1):
      w = (w - coef[i - lo][:, None] * ring[i % RING]).astype(cdtype)
    norm = np.linalg.norm(w.astype(np.complex128), axis=1)
    broke = live & (norm <= threshold)
    lengths[broke] = j + 1
    live = live & ~broke
    beta[:, j] = np.where(live, norm, 0.0)
    scale = np.where(live, 1.0 / np.where(live, norm, 1.0), 0.0)
    if j + 1 < m:
      ring[(j + 1) % RING] = (w.astype(np.complex128) * scale[:, None]).astype(cdtype)
  return alpha, beta, lengths, recurrence, norms


def rows(n, ops, starts, beta, recurrence, weights=None, dtype=np.float64):
  """Yields v_0, v_1, ..., v_{m-1} ([U, 2^n] each), regenerated from the recorded recurrence: two vectors are alive."""
  cdtype = np.complex64 if dtype == np.float32 else np.complex128
  m = beta.shape[1]
  cur, _ = _import(np.asarray(starts, cdtype), cdtype)
  prev = None
  recurrence = np.asarray(recurrence, cdtype)
  for j in range(m):
    yield cur
    if j + 1 == m:
      return
    w = T.apply_h(n, ops, cur, weights, dtype).astype(cdtype)
    if j > 0:
      w = (w - recurrence[:, j, 0][:, None] * prev).astype(cdtype)
    w = (w - recurrence[:, j, 1][:, None] * cur).astype(cdtype)
    live = beta[:, j] != 0
    scale = np.where(live, 1.0 / np.where(live, beta[:, j], 1.0), 0.0)
    prev, cur = cur, (w.astype(np.complex128) * scale[:, None]).astype(cdtype)


def replay(n, ops, starts, beta, recurrence, coef, weights=None, dtype=np.float64):
  """out[u, s] = sum_j coef[u, s, j] v_j(u), j ascending: `krylov_ref.combine` over a basis that is never stored."""
  cdtype = np.complex64 if dtype == np.float32 else np.complex128
  coef = np.asarray(coef).astype(cdtype)
  out = None
  for j, v in enumerate(rows(n, ops, starts, beta, recurrence, weights, dtype)):
    if out is None:
      out = np.zeros(coef.shape[:2] + v.shape[1:], cdtype)
    out = (out + coef[:, :, j, None] * v[:, None, :]).astype(cdtype)
  return out
