"""Complex128 restatement of `qhbm_statevector_vjp_from_states`: the VJP of the final states psi_u = C(params) phi_u --
cirq's global phase included, nothing normalised -- for a caller's cotangent, on tests/from_states_ref.py
(`apply_circuit`, `final_states`) and the oracle's gate matrices, which carry every gate's phase:
  G**t = sum_k exp(i pi t (e_k + global_shift)) P_k            (cirq EigenGate; X, Y: e = 0, 1, so X**t =
                                                                 e^{i pi t / 2} (cos(pi t / 2) I - i sin(pi t / 2) X))
Nothing of the engine is used here.

Convention (torch's for a complex tensor): for a real loss L the cotangent is g_u = dL/dRe psi_u + i dL/dIm psi_u, so that
dL = sum_u Re<g_u|dpsi_u>, and `vjp` returns grad[p] = sum_u Re<g_u| d psi_u / d params[p]>.

Three losses, each as (value, cotangent) of given final states:
  (A) overlap_loss        sum_u c_u |<t_u|psi_u>|^2                  blind to the global phase
  (B) linear_loss         sum_u Re(z_u <t_u|psi_u>), z_u complex     sensitive to it
  (C) table_loss          sum_u w_u sum_y E[y] |psi_u[y]|^2          an energy table
"""
import math

import numpy as np

from oracle import qhbm_oracle as O
from tests import from_states_ref as R


def vjp(n, gates, params, states, cotangent):
  """grad [P] = sum_u Re<g_u| d(C(params) phi_u) / d params>, by the reverse recursion: lambda starts as g and is pulled
  back gate by gate, psi is un-applied beside it."""
  params = np.asarray(params, dtype=np.float64)
  grad = np.zeros(len(params))
  for s, g_u in zip(np.asarray(states), np.asarray(cotangent)):
    psi = R.apply_circuit(n, gates, params, s)
    lam = np.asarray(g_u, dtype=np.complex128).reshape((2,) * n)
    for g in reversed(gates):
      kind, pidx, scalar = g[0], g[3], g[4]
      shift = O.gate_global_shift(g)
      t_g = O.gate_exponent(g, params)
      qs = R._gate_qubits(g)  # pylint: disable=protected-access
      u_dag = O.gate_matrix(kind, t_g, shift).conj().T
      psi = O._apply_matrix(psi, u_dag, qs)  # pylint: disable=protected-access
      if pidx >= 0:
        dpsi = O._apply_matrix(psi, O.gate_matrix_derivative(kind, t_g, shift), qs)  # pylint: disable=protected-access
        grad[pidx] += scalar * float(np.real(np.vdot(lam.ravel(), dpsi.ravel())))
      lam = O._apply_matrix(lam, u_dag, qs)  # pylint: disable=protected-access
  return grad


def documented_phase_slope(gates, n_params):
  """d theta / d params of the phase the gate documentation writes IN FRONT of the rotations: pi t / 2 per X**t and Y**t,
  pi t global_shift per gate with a shift (t = scalar * param + offset).  A simulator that applies
  cos(pi t / 2) I - i sin(pi t / 2) G for those gates and ignores the shifts has left out exactly this phase."""
  slope = np.zeros(n_params)
  for g in gates:
    kind, pidx, scalar = g[0], g[3], g[4]
    if pidx < 0:
      continue
    if kind in (O.GATE_XPOW, O.GATE_YPOW):
      slope[pidx] += math.pi * 0.5 * scalar
    slope[pidx] += math.pi * O.gate_global_shift(g) * scalar
  return slope


def phase_term(gates, n_params, finals, cotangent):
  """The share of `vjp` that comes through that phase alone: -(d theta / d p) sum_u Im<g_u|psi_u>."""
  s = sum(float(np.imag(np.vdot(g_u, psi_u))) for g_u, psi_u in zip(np.asarray(cotangent), np.asarray(finals)))
  return -documented_phase_slope(gates, n_params) * s


def overlap_loss(finals, targets, c):
  """(A): (sum_u c_u |<t_u|psi_u>|^2, cotangent [M, 2^n]); d|a|^2 = 2 Re(conj(a) <t|dpsi>) = Re<2 a t|dpsi>, a = <t|psi>: g = 2 c a t."""
  finals, targets = np.asarray(finals, dtype=np.complex128), np.asarray(targets, dtype=np.complex128)
  a = np.einsum("uy,uy->u", targets.conj(), finals)
  value = float(np.sum(np.asarray(c) * np.abs(a)**2))
  return value, (2.0 * np.asarray(c) * a)[:, None] * targets


def linear_loss(finals, targets, z):
  """(B): (sum_u Re(z_u <t_u|psi_u>), cotangent); Re(z <t|dpsi>) = Re<conj(z) t|dpsi>: g = conj(z) t."""
  finals, targets = np.asarray(finals, dtype=np.complex128), np.asarray(targets, dtype=np.complex128)
  z = np.asarray(z, dtype=np.complex128)
  a = np.einsum("uy,uy->u", targets.conj(), finals)
  return float(np.real(np.sum(z * a))), np.conj(z)[:, None] * targets


def table_loss(finals, table, w):
  """(C): (sum_u w_u sum_y E[y] |psi_u[y]|^2, cotangent); g = 2 w E psi."""
  finals = np.asarray(finals, dtype=np.complex128)
  table, w = np.asarray(table, dtype=np.float64), np.asarray(w, dtype=np.float64)
  value = float(np.sum(w[:, None] * table[None, :] * np.abs(finals)**2))
  return value, 2.0 * w[:, None] * table[None, :] * finals


def loss_of(kind, finals, aux):
  return {"A": overlap_loss, "B": linear_loss, "C": table_loss}[kind](finals, *aux)


def loss_aux(kind, num, n, seed):
  """Seeded auxiliary data of a loss: (targets, c), (targets, z) or (table, w)."""
  rng = np.random.default_rng(seed)
  if kind == "A":
    return R.random_states(num, n, seed + 1), rng.uniform(0.5, 1.5, num)
  if kind == "B":
    return R.random_states(num, n, seed + 1), rng.normal(size=num) + 1j * rng.normal(size=num)
  return rng.normal(size=1 << n), rng.uniform(0.5, 1.5, num)


def with_rotation_shifts(gates):
  """Every second single-qubit X, Y or Z power of a gate list in its rotation form rx / ry / rz: global_shift -0.5."""
  out, k = [], 0
  for g in gates:
    g = tuple(g[:6])
    if g[0] in (O.GATE_XPOW, O.GATE_YPOW, O.GATE_ZPOW):
      k += 1
      if k % 2 == 0:
        g = g + (-0.5,)
    out.append(g)
  return out


def case(name, num=3, layers=2):
  """(n, gates, params, states) of a named test circuit: "hea<n>" (the hardware-efficient ansatz, `layers` layers) or
  "all_kinds" (tests/golden/all_kinds_n5.npz with rotation-form shifts); `num` seeded states of norms 0.5, 1, 3, 0.5, ...,
  rounded to complex64 -- what an engine is given."""
  from tests import golden_util as G  # pylint: disable=import-outside-toplevel
  if name == "all_kinds":
    g = G.load("all_kinds_n5.npz")
    n, gates, params = int(g["n"]), with_rotation_shifts(G.gates_of(g["gates"])), np.asarray(g["params"], dtype=np.float64)
  else:
    n = int(name[3:])
    gates, names = O.hea_gates(n, layers, "fv")
    params = np.random.default_rng(900 + n).uniform(-1, 1, len(names))
  scale = np.array([0.5, 1.0, 3.0])[np.arange(num) % 3]
  states = (R.random_states(num, n, 910 + n) * scale[:, None]).astype(np.complex64).astype(np.complex128)
  return n, gates, params, states


# Seeds of `loss_aux` per circuit under which loss (B)'s phase term is at least 10 % of ||grad||_inf
# (tests/test_final_states_cpu.py asserts it; where a seed missed the share, the next one was taken).
AUX_SEEDS = {"all_kinds": 939, "hea12": 933}  # (hea12 with five states: 932 gives 8 %)


def aux_seed(name):
  return AUX_SEEDS[name] if name in AUX_SEEDS else 920 + int(name[3:])
