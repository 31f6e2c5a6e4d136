// plan_emulate.cpp -- see plan_emulate.h.  Host C++ only; built with the sanitizers of tests/sanitize/Makefile, so the
// emulator's own indexing into a plan's tables is checked too.
#include "plan_emulate.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

using namespace qhbm;

namespace emu {

namespace {

const double kPi = 3.14159265358979323846;

// sin, cos of pi x with the argument reduced exactly (x - 2 rint(x / 2) is exact in binary floating point)
void sincospi_d(double x, double* s, double* c) {
  const double r = x - 2.0 * std::rint(0.5 * x);
  *s = std::sin(kPi * r);
  *c = std::cos(kPi * r);
}
inline cd cmul(cd a, cd b) { return cd(a.real() * b.real() - a.imag() * b.imag(), a.real() * b.imag() + a.imag() * b.real()); }
inline double im_conj(cd l, cd p) { return l.real() * p.imag() - l.imag() * p.real(); }  // Im(conj(l) p)
inline int popc(uint32_t v) { return __builtin_popcount(v); }
const double kNaN = std::numeric_limits<double>::quiet_NaN();

}  // namespace

// =====================================================================================================================
// Oracle
// =====================================================================================================================
int oracle_gate(int kind, double t, double shift, cd U[16], cd A[16]) {
  const int nq = kind >= QHBM_GATE_CZPOW ? 2 : 1, d = nq == 1 ? 2 : 4;
  for (int i = 0; i < 16; ++i) { U[i] = 0.0; A[i] = 0.0; }
  if (kind == QHBM_GATE_ISWAPPOW) {
    // eigen-exponents 0 on |00>, |11>, +1/2 on (|01> + |10>) / sqrt 2, -1/2 on (|01> - |10>) / sqrt 2
    double sh, ch;
    sincospi_d(0.5 * t, &sh, &ch);
    U[0] = 1.0; U[15] = 1.0;
    U[5] = ch; U[10] = ch;
    U[6] = cd(0.0, sh); U[9] = cd(0.0, sh);
    A[6] = 0.5; A[9] = 0.5;
  } else {
    // an involution G: eigen-exponent 0 on its +1 space, 1 on its -1 space
    cd G[16];
    for (int i = 0; i < 16; ++i) G[i] = 0.0;
    const double r = std::sqrt(0.5);
    switch (kind) {
      case QHBM_GATE_I: G[0] = 1.0; G[3] = 1.0; break;
      case QHBM_GATE_XPOW: G[1] = 1.0; G[2] = 1.0; break;
      case QHBM_GATE_YPOW: G[1] = cd(0.0, -1.0); G[2] = cd(0.0, 1.0); break;
      case QHBM_GATE_ZPOW: G[0] = 1.0; G[3] = -1.0; break;
      case QHBM_GATE_HPOW: G[0] = r; G[1] = r; G[2] = r; G[3] = -r; break;
      case QHBM_GATE_CZPOW: G[0] = 1.0; G[5] = 1.0; G[10] = 1.0; G[15] = -1.0; break;
      case QHBM_GATE_CNOTPOW: G[0] = 1.0; G[5] = 1.0; G[11] = 1.0; G[14] = 1.0; break;
      case QHBM_GATE_SWAPPOW: G[0] = 1.0; G[6] = 1.0; G[9] = 1.0; G[15] = 1.0; break;
      case QHBM_GATE_XXPOW: G[3] = 1.0; G[6] = 1.0; G[9] = 1.0; G[12] = 1.0; break;
      case QHBM_GATE_YYPOW: G[3] = -1.0; G[6] = 1.0; G[9] = 1.0; G[12] = -1.0; break;
      case QHBM_GATE_ZZPOW: G[0] = 1.0; G[5] = -1.0; G[10] = -1.0; G[15] = 1.0; break;
      default: break;
    }
    double s, c;
    sincospi_d(t, &s, &c);
    const cd e(c, s), a = 0.5 * (1.0 + e), b = 0.5 * (1.0 - e);
    for (int i = 0; i < d; ++i)
      for (int j = 0; j < d; ++j) {
        const double id = i == j ? 1.0 : 0.0;
        U[i * d + j] = a * id + b * G[i * d + j];
        A[i * d + j] = 0.5 * (id - G[i * d + j]);
      }
  }
  if (shift != 0.0) {
    double s, c;
    sincospi_d(t * shift, &s, &c);
    for (int i = 0; i < d * d; ++i) U[i] = cmul(U[i], cd(c, s));
  }
  return nq;
}

double oracle_exponent(const Gate& g, const std::vector<double>& params) {
  double t = double(g.offset);
  if (g.param_idx >= 0) t += double(g.scalar) * params[size_t(g.param_idx)];
  return t;
}

namespace {

// M (d x d, row-major) on the index bits b0 (matrix bit 1) and b1 (matrix bit 0); one-qubit: b1 < 0
void apply_matrix(std::vector<cd>& s, int nq, const cd* M, int b0, int b1, bool dagger) {
  const size_t N = s.size();
  if (nq == 1) {
    cd m[4] = {M[0], M[1], M[2], M[3]};
    if (dagger) { m[0] = std::conj(M[0]); m[1] = std::conj(M[2]); m[2] = std::conj(M[1]); m[3] = std::conj(M[3]); }
    const size_t mask = size_t(1) << b0;
    for (size_t i = 0; i < N; ++i) {
      if (i & mask) continue;
      const cd x0 = s[i], x1 = s[i | mask];
      s[i] = cmul(m[0], x0) + cmul(m[1], x1);
      s[i | mask] = cmul(m[2], x0) + cmul(m[3], x1);
    }
    return;
  }
  cd m[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) m[i * 4 + j] = dagger ? std::conj(M[j * 4 + i]) : M[i * 4 + j];
  const size_t m0 = size_t(1) << b0, m1 = size_t(1) << b1;
  for (size_t i = 0; i < N; ++i) {
    if (i & (m0 | m1)) continue;
    const size_t ix[4] = {i, i | m1, i | m0, i | m0 | m1};
    cd x[4], y[4];
    for (int j = 0; j < 4; ++j) x[j] = s[ix[j]];
    for (int r = 0; r < 4; ++r) {
      cd acc = 0.0;
      for (int j = 0; j < 4; ++j) acc += cmul(m[r * 4 + j], x[j]);
      y[r] = acc;
    }
    for (int j = 0; j < 4; ++j) s[ix[j]] = y[j];
  }
}

// Im <lam| A |psi>
double im_lam_a_psi(const std::vector<cd>& lam, const std::vector<cd>& psi, int nq, const cd* A, int b0, int b1) {
  const size_t N = psi.size();
  double acc = 0.0;
  if (nq == 1) {
    const size_t mask = size_t(1) << b0;
    for (size_t i = 0; i < N; ++i) {
      if (i & mask) continue;
      const cd x0 = psi[i], x1 = psi[i | mask];
      acc += im_conj(lam[i], cmul(A[0], x0) + cmul(A[1], x1)) + im_conj(lam[i | mask], cmul(A[2], x0) + cmul(A[3], x1));
    }
    return acc;
  }
  const size_t m0 = size_t(1) << b0, m1 = size_t(1) << b1;
  for (size_t i = 0; i < N; ++i) {
    if (i & (m0 | m1)) continue;
    const size_t ix[4] = {i, i | m1, i | m0, i | m0 | m1};
    for (int r = 0; r < 4; ++r) {
      cd y = 0.0;
      for (int j = 0; j < 4; ++j) y += cmul(A[r * 4 + j], psi[ix[j]]);
      acc += im_conj(lam[ix[r]], y);
    }
  }
  return acc;
}

// P |g> = i^ny (-1)^popc(g & z) |g ^ x>
inline cd pauli_phase(uint32_t g, uint32_t z, int ny) {
  static const cd ipow[4] = {cd(1, 0), cd(0, 1), cd(-1, 0), cd(0, -1)};
  const cd ph = ipow[ny & 3];
  return (popc(g & z) & 1) ? -ph : ph;
}

}  // namespace

std::vector<cd> oracle_state(const Model& m, const std::vector<double>& params, uint32_t basis) {
  std::vector<cd> s(size_t(1) << m.n, cd(0.0, 0.0));
  s[basis] = 1.0;
  cd U[16], A[16];
  for (const Gate& g : m.gates) {
    const int nq = oracle_gate(g.kind, oracle_exponent(g, params), double(g.global_shift), U, A);
    apply_matrix(s, nq, U, m.n - 1 - g.q0, nq == 2 ? m.n - 1 - g.q1 : -1, false);
  }
  return s;
}

std::vector<double> oracle_values(const Model& m, const std::vector<cd>& psi) {
  std::vector<double> v(size_t(m.n_ops), 0.0);
  for (const PauliTerm& t : m.terms) {
    const int ny = popc(t.x & t.z);
    cd acc = 0.0;
    for (size_t g = 0; g < psi.size(); ++g) acc += cmul(std::conj(psi[g ^ t.x]), cmul(pauli_phase(uint32_t(g), t.z, ny), psi[g]));
    v[size_t(t.op)] += double(t.coeff) * acc.real();
  }
  return v;
}

std::vector<cd> oracle_apply_observables(const Model& m, const std::vector<cd>& psi, const std::vector<double>& up) {
  std::vector<cd> lam(psi.size(), cd(0.0, 0.0));
  for (const PauliTerm& t : m.terms) {
    const int ny = popc(t.x & t.z);
    const double w = up[size_t(t.op)] * double(t.coeff);
    for (size_t g = 0; g < psi.size(); ++g) lam[g ^ t.x] += w * cmul(pauli_phase(uint32_t(g), t.z, ny), psi[g]);
  }
  return lam;
}

std::vector<double> oracle_gradient(const Model& m, const std::vector<double>& params, uint32_t basis,
                                    const std::vector<double>& up) {
  std::vector<cd> psi = oracle_state(m, params, basis);
  std::vector<cd> lam = oracle_apply_observables(m, psi, up);
  std::vector<double> grad(size_t(m.n_params), 0.0);
  cd U[16], A[16];
  for (size_t gi = m.gates.size(); gi-- > 0;) {
    const Gate& g = m.gates[gi];
    const int nq = oracle_gate(g.kind, oracle_exponent(g, params), double(g.global_shift), U, A);
    const int b0 = m.n - 1 - g.q0, b1 = nq == 2 ? m.n - 1 - g.q1 : -1;
    // E = <psi|O|psi>, d psi / dt = i pi (A + shift) psi after the gate: dE/dt = 2 Re <lam| i pi A |psi> = -2 pi Im <lam|A|psi>
    // (the shift term is i pi shift <psi|O|psi>: imaginary, gone with the real part)
    if (g.param_idx >= 0 && g.kind != QHBM_GATE_I)
      grad[size_t(g.param_idx)] += double(g.scalar) * (-2.0 * kPi) * im_lam_a_psi(lam, psi, nq, A, b0, b1);
    apply_matrix(psi, nq, U, b0, b1, true);
    apply_matrix(lam, nq, U, b0, b1, true);
  }
  return grad;
}

// =====================================================================================================================
// Emulator
// =====================================================================================================================
void emu_prepare(const Model& m, const Plan& plan, const std::vector<double>& params, Emulation* e) {
  e->m = &m;
  e->plan = &plan;
  e->err.clear();
  fill_args(plan, m, &e->args, &e->prog, &e->tables);
  e->cf.assign(plan.coef_init.size() + 64, 0.0);
  // ---- prep_coefs_kernel, in double and with X**t kept as (cos, sin) of pi t / 2 ----
  for (const CoefJob& jb : plan.jobs) {
    double t = double(jb.offset) + double(jb.add_offset);
    if (jb.param_idx >= 0) t += double(jb.scalar) * params[size_t(jb.param_idx)];
    const size_t need = jb.mop == MOP_MAT2 ? (jb.dagger ? 64 : 32) : jb.mop == MOP_MAT1 ? (jb.dagger ? 16 : 8) : 2;
    if (jb.out_off < 0 || size_t(jb.out_off) + need > e->cf.size()) { e->err = "coefficient job writes outside the buffer"; return; }
    double* o = &e->cf[size_t(jb.out_off)];
    if (jb.mop == MOP_PHASE) {
      double sn, cs;
      sincospi_d(double(jb.mult) * t, &sn, &cs);
      o[0] = cs;
      o[1] = jb.dagger ? -sn : sn;
      continue;
    }
    if (jb.mop == MOP_X) {  // c I - i s X, theta = pi t / 2 with t reduced to one period (a global sign otherwise)
      t *= double(jb.mult);
      const double tr = t - 2.0 * std::rint(0.5 * t);
      double s2, c2;
      sincospi_d(0.5 * tr, &s2, &c2);
      o[0] = c2;
      o[1] = jb.dagger ? -s2 : s2;
      continue;
    }
    double sh, ch;
    sincospi_d(0.5 * t, &sh, &ch);
    if (jb.mop == MOP_Y) {
      o[0] = ch;
      o[1] = jb.dagger ? -sh : sh;
      continue;
    }
    double sp, cp;
    sincospi_d(t, &sp, &cp);
    const cd A(0.5 * (1.0 + cp), 0.5 * sp), B(0.5 * (1.0 - cp), -0.5 * sp);
    if (jb.mop == MOP_MAT1) {  // H**t = A I + B H
      const double r = std::sqrt(0.5);
      const cd U[4] = {A + B * r, B * r, B * r, A - B * r};
      for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 2; ++k) {
          const cd u = jb.dagger ? std::conj(U[k * 2 + i]) : U[i * 2 + k];
          o[(i * 2 + k) * 2] = u.real();
          o[(i * 2 + k) * 2 + 1] = u.imag();
        }
      if (jb.dagger) {
        const double g[4] = {r, r, r, -r};
        for (int i = 0; i < 4; ++i) { o[8 + 2 * i] = kPi * g[i]; o[8 + 2 * i + 1] = 0.0; }
      }
      continue;
    }
    // MOP_MAT2
    cd U[16], Gm[16];
    for (int i = 0; i < 16; ++i) { U[i] = 0.0; Gm[i] = 0.0; }
    if (jb.op_kind == QHBM_GATE_ISWAPPOW) {
      U[0] = 1.0; U[15] = 1.0;
      U[5] = ch; U[10] = ch;
      U[6] = cd(0.0, sh); U[9] = cd(0.0, sh);
      Gm[6] = -kPi; Gm[9] = -kPi;
    } else {
      int perm[4] = {0, 1, 2, 3};
      double ph[4] = {1.0, 1.0, 1.0, 1.0};
      switch (jb.op_kind) {
        case QHBM_GATE_CNOTPOW: perm[2] = 3; perm[3] = 2; break;
        case QHBM_GATE_SWAPPOW: perm[1] = 2; perm[2] = 1; break;
        case QHBM_GATE_XXPOW: perm[0] = 3; perm[1] = 2; perm[2] = 1; perm[3] = 0; break;
        case QHBM_GATE_YYPOW: perm[0] = 3; perm[1] = 2; perm[2] = 1; perm[3] = 0; ph[0] = -1.0; ph[3] = -1.0; break;
        default: break;
      }
      for (int i = 0; i < 4; ++i) {
        U[i * 4 + i] += A;
        U[i * 4 + perm[i]] += B * ph[i];
        Gm[i * 4 + perm[i]] += kPi * ph[i];
      }
    }
    auto idx = [&](int i) { return jb.swap ? ((i & 1) << 1) | (i >> 1) : i; };
    for (int i = 0; i < 4; ++i)
      for (int k = 0; k < 4; ++k) {
        const cd u = jb.dagger ? std::conj(U[idx(k) * 4 + idx(i)]) : U[idx(i) * 4 + idx(k)];
        o[(i * 4 + k) * 2] = u.real();
        o[(i * 4 + k) * 2 + 1] = u.imag();
        if (jb.dagger) {
          const cd g = Gm[idx(i) * 4 + idx(k)];
          o[32 + (i * 4 + k) * 2] = g.real();
          o[32 + (i * 4 + k) * 2 + 1] = g.imag();
        }
      }
  }
  // ---- combine_diag_kernel: FULL[m - 1] = product of the record's PH1 / PH2 inputs contained in register value m ----
  const RecordLayout L(4, false);
  for (uint32_t off : plan.record_offsets) {
    if (size_t(off) + 128 > plan.coef_init.size()) { e->err = "record outside the coefficient buffer"; return; }
    const uint32_t h0 = plan.coef_init[off], h1 = plan.coef_init[off + 1];
    if (!(h1 & kFullDiagFlag)) continue;
    for (int mm = 1; mm <= 15; ++mm) {
      cd c(1.0, 0.0);
      for (int j = 0; j < 4; ++j)
        if (((mm >> j) & 1) && ((h0 >> (4 + j)) & 1u)) c = cmul(c, cd(e->cf[off + size_t(L.in_ph1(j))], e->cf[off + size_t(L.in_ph1(j)) + 1]));
      for (int jb = 1; jb < 4; ++jb)
        for (int ja = 0; ja < jb; ++ja)
          if (((mm >> ja) & 1) && ((mm >> jb) & 1) && ((h0 >> (24 + pair_index(ja, jb))) & 1u))
            c = cmul(c, cd(e->cf[off + size_t(L.in_ph2(pair_index(ja, jb)))], e->cf[off + size_t(L.in_ph2(pair_index(ja, jb))) + 1]));
      e->cf[off + size_t(L.full(mm))] = c.real();
      e->cf[off + size_t(L.full(mm)) + 1] = c.imag();
    }
  }
}

namespace {

#define EMU_REQUIRE(cond, msg)                                   \
  do {                                                           \
    if (!(cond)) {                                               \
      if (e->err.empty()) e->err = std::string(msg) + " [" #cond "]"; \
      return false;                                              \
    }                                                            \
  } while (0)

// What a workgroup derives from its block index, the pass arguments and the input bitstring (kernels.hip input_index,
// local_bits, launched_tile, tile_base_of, tile_offset, the row / thread offsets of prefetch_tile and store_tile).
struct Geometry {
  const PassArgs* a;
  const uint32_t* spread;
  size_t spread_n;
  int K;
  uint32_t idx, in_local;
  bool rows8;  // index bit 0 is not local: the odd amplitude of a pair sits at tile_offset(1), not at the next address

  uint32_t tile_offset(uint32_t l) const {
    const uint32_t cmask = (1u << a->c) - 1u, hi = l >> a->c;
    if (a->spread_shift != 0xffffffffu) return (l & cmask) | (hi << a->spread_shift);
    return (l & cmask) | (hi < spread_n ? spread[hi] : 0xffffffffu);
  }
  void input(uint32_t logical) {
    idx = 0;
    for (uint32_t p = 0; p < a->n && p < 32; ++p)
      if ((logical >> a->log_of[p]) & 1u) idx |= 1u << p;
    in_local = 0;
    for (int k = 0; k < K; ++k)
      if ((idx >> a->local_pos[k]) & 1u) in_local |= 1u << k;
  }
  uint32_t launched_tile(uint32_t block) const {
    const uint32_t live = block & ((1u << a->n_free) - 1u);
    uint32_t id = 0, rank = 0;
    for (uint32_t L = 0; L < a->n_nonlocal; ++L) {
      const uint32_t pos = a->nonlocal_pos[L];
      const bool fixed = (a->zero_mask >> pos) & 1u;
      const uint32_t bit = fixed ? (idx >> pos) & 1u : (live >> rank) & 1u;
      if (!fixed) ++rank;
      id |= bit << L;
    }
    return id;
  }
  uint32_t tile_base_of(uint32_t tile_id) const {
    uint32_t base = 0, rank = 0;
    for (uint32_t p = 0; p < 32; ++p)
      if ((a->nonlocal_mask >> p) & 1u) { base |= ((tile_id >> rank) & 1u) << p; ++rank; }
    return base;
  }
  // address of local index l: row I = l >> (K - 3) through PassArgs::row_off, the thread's own offset added to it
  size_t addr(uint32_t tile_base, uint32_t l) const {
    const uint32_t I = l >> (K - 3), rest = l & ((1u << (K - 3)) - 1u);
    const uint32_t g0 = tile_offset(rest & ~1u);
    const uint32_t g = (rest & 1u) ? (rows8 ? (g0 | tile_offset(1u)) : g0 + 1u) : g0;
    return size_t(tile_base | a->row_off[I]) + size_t(g);
  }
};

struct Record {
  const uint32_t* w;  // static words
  const double* c;    // coefficients
  cd cs(int off) const { return cd(c[off], c[off + 1]); }
};

inline void op_x(cd* a, int J, cd cs) {  // c I - i s X
  const double c = cs.real(), s = cs.imag();
  for (int m = 0; m < 16; ++m) {
    if (m >> J & 1) continue;
    const cd a0 = a[m], a1 = a[m | (1 << J)];
    a[m] = cd(c * a0.real() + s * a1.imag(), c * a0.imag() - s * a1.real());
    a[m | (1 << J)] = cd(c * a1.real() + s * a0.imag(), c * a1.imag() - s * a0.real());
  }
}
inline void op_y(cd* a, int J, cd cs) {  // c I - i s Y = [[c, -s], [s, c]]
  const double c = cs.real(), s = cs.imag();
  for (int m = 0; m < 16; ++m) {
    if (m >> J & 1) continue;
    const cd a0 = a[m], a1 = a[m | (1 << J)];
    a[m] = c * a0 - s * a1;
    a[m | (1 << J)] = s * a0 + c * a1;
  }
}
inline void op_dense(cd* a, int J, const double* u) {
  const cd u00(u[0], u[1]), u01(u[2], u[3]), u10(u[4], u[5]), u11(u[6], u[7]);
  for (int m = 0; m < 16; ++m) {
    if (m >> J & 1) continue;
    const cd a0 = a[m], a1 = a[m | (1 << J)];
    a[m] = cmul(u00, a0) + cmul(u01, a1);
    a[m | (1 << J)] = cmul(u10, a0) + cmul(u11, a1);
  }
}
inline void op_ph1(cd* a, int J, cd cs) {
  for (int m = 0; m < 16; ++m)
    if (m >> J & 1) a[m] = cmul(a[m], cs);
}
inline void op_ph2(cd* a, int JA, int JB, cd cs) {
  for (int m = 0; m < 16; ++m)
    if ((m >> JA & 1) && (m >> JB & 1)) a[m] = cmul(a[m], cs);
}
inline double sum_w1(const cd* p, const cd* l, int J) {
  double g = 0.0;
  for (int m = 0; m < 16; ++m)
    if (m >> J & 1) g += im_conj(l[m], p[m]);
  return g;
}
inline double sum_w2(const cd* p, const cd* l, int JA, int JB) {
  double g = 0.0;
  for (int m = 0; m < 16; ++m)
    if ((m >> JA & 1) && (m >> JB & 1)) g += im_conj(l[m], p[m]);
  return g;
}

// instance_fwd
void instance_fwd(const Record& r, cd* a, uint32_t tlx, bool general) {
  const RecordLayout L(4, false);
  const uint32_t h0 = r.w[0], h1 = r.w[1];
  for (int J = 0; J < 4; ++J)
    if ((h0 >> J) & 1u) op_x(a, J, r.cs(L.x(J)));
  if (general) {  // (the lean kernel variant does not look at these bits)
    for (int J = 0; J < 4; ++J)
      if ((h1 >> (16 + J)) & 1u) op_y(a, J, r.cs(L.y(J)));
    for (int J = 0; J < 4; ++J)
      if ((h1 >> (24 + J)) & 1u) op_dense(a, J, r.c + L.dense(J));
  }
  if (h1 & kFullDiagFlag)
    for (int m = 1; m < 16; ++m) a[m] = cmul(a[m], r.cs(L.full(m)));
  for (int J = 0; J < 4; ++J)
    if ((h0 >> (8 + J)) & 1u) op_ph1(a, J, r.cs(L.ph1(J)));
  for (int JB = 1; JB < 4; ++JB)
    for (int JA = 0; JA < JB; ++JA)
      if ((h0 >> (16 + pair_index(JA, JB))) & 1u) op_ph2(a, JA, JB, r.cs(L.ph2(pair_index(JA, JB))));
  for (int k = 0; k < 8; ++k)
    if ((h1 >> k) & 1u) {
      const uint32_t pred = r.w[L.pred(k)];
      if ((tlx >> (pred & 0x1fu)) & 1u) op_ph1(a, k >> 1, r.cs(L.cph(k)));
    }
}

// instance_adj: the gradient partials Im <lam|A|psi> into the slots the record names, then U^dagger on both.
// `slots`: the pass's slot row (n_slots entries).  A partial the kernel would not have computed is NaN.
bool instance_adj(Emulation* e, const Record& r, cd* p, cd* l, uint32_t tlx, bool general, double* slots, uint32_t n_slots) {
  const RecordLayout L(4, true);
  const uint32_t h0 = r.w[0], h1 = r.w[1];
  auto store8 = [&](int g8, const double* g) -> bool {
    for (int v = 0; v < 8; ++v) {
      const uint32_t s = r.w[L.slot_lane8(g8, v)];
      if (s == 0xffffffffu) continue;
      EMU_REQUIRE(s < n_slots, "gradient slot outside the pass's row");
      slots[s] += g[v];
    }
    return true;
  };
  if (h1 & 0xffu) {
    double g[8] = {kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN};
    for (int k = 0; k < 8; ++k)
      if ((h1 >> k) & 1u) {
        const uint32_t pred = r.w[L.pred(k)];
        g[k] = 0.0;
        if ((tlx >> (pred & 0x1fu)) & 1u) {
          g[k] = sum_w1(p, l, k >> 1);
          op_ph1(p, k >> 1, r.cs(L.cph(k)));
          op_ph1(l, k >> 1, r.cs(L.cph(k)));
        }
      }
    if (!store8(2, g)) return false;
  }
  double g0[8] = {kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN};  // X[4] then PH1[4]
  if (h1 & kFullDiagFlag) {
    double g2[8] = {0, 0, 0, 0, 0, 0, kNaN, kNaN};
    double dm[16];  // full_partials: d[m] = Im(conj(lam_m) psi_m), summed over the register values that contain a term's bits
    for (int m = 0; m < 16; ++m) dm[m] = im_conj(l[m], p[m]);
    for (int J = 0; J < 4; ++J) {
      double g = 0.0;
      for (int m = 0; m < 16; ++m) if (m >> J & 1) g += dm[m];
      g0[4 + J] = g;
    }
    for (int JB = 1; JB < 4; ++JB)
      for (int JA = 0; JA < JB; ++JA) {
        double g = 0.0;
        for (int m = 0; m < 16; ++m) if ((m >> JA & 1) && (m >> JB & 1)) g += dm[m];
        g2[pair_index(JA, JB)] = g;
      }
    if ((h0 >> 24) & 0x3fu)
      if (!store8(1, g2)) return false;
    for (int m = 1; m < 16; ++m) { p[m] = cmul(p[m], r.cs(L.full(m))); l[m] = cmul(l[m], r.cs(L.full(m))); }
  }
  if ((h0 >> 16) & 0x3fu) {
    double g[8] = {kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN, kNaN};
    for (int JB = 1; JB < 4; ++JB)
      for (int JA = 0; JA < JB; ++JA)
        if ((h0 >> (16 + pair_index(JA, JB))) & 1u) {
          const cd cs = r.cs(L.ph2(pair_index(JA, JB)));
          g[pair_index(JA, JB)] = sum_w2(p, l, JA, JB);
          op_ph2(p, JA, JB, cs);
          op_ph2(l, JA, JB, cs);
        }
    if (!store8(1, g)) return false;
  }
  for (int J = 0; J < 4; ++J)
    if ((h0 >> (8 + J)) & 1u) {
      const cd cs = r.cs(L.ph1(J));
      g0[4 + J] = sum_w1(p, l, J);
      op_ph1(p, J, cs);
      op_ph1(l, J, cs);
    }
  for (int J = 0; J < 4; ++J)
    if ((h0 >> J) & 1u) {
      if ((h0 >> (12 + J)) & 1u) {
        double g = 0.0;
        for (int m = 0; m < 16; ++m) g += im_conj(l[m], p[m ^ (1 << J)]);
        g0[J] = g;
      }
      op_x(p, J, r.cs(L.x(J)));
      op_x(l, J, r.cs(L.x(J)));
    }
  if (((h0 >> 12) & 0xfu) | ((((h0 >> 8) | (h0 >> 4)) & 0xfu) << 4))
    if (!store8(0, g0)) return false;
  if (general && ((h1 >> 16) & 0xf0fu)) {
    double g[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int J = 0; J < 4; ++J)
      if ((h1 >> (16 + J)) & 1u) {
        if (r.w[L.slot_y(J)] != 0xffffffffu)
          for (int m = 0; m < 16; ++m) {  // (Y psi)_0 = -i psi_1, (Y psi)_1 = i psi_0
            if (m >> J & 1) continue;
            const int m1 = m | (1 << J);
            g[J] += im_conj(l[m], cmul(cd(0, -1), p[m1])) + im_conj(l[m1], cmul(cd(0, 1), p[m]));
          }
        op_y(p, J, r.cs(L.y(J)));
        op_y(l, J, r.cs(L.y(J)));
      }
    for (int J = 0; J < 4; ++J)
      if ((h1 >> (24 + J)) & 1u) {
        const double* u = r.c + L.dense(J);
        if (r.w[L.slot_dense(J)] != 0xffffffffu) {
          const cd g00(u[8], u[9]), g01(u[10], u[11]), g10(u[12], u[13]), g11(u[14], u[15]);
          for (int m = 0; m < 16; ++m) {
            if (m >> J & 1) continue;
            const int m1 = m | (1 << J);
            g[4 + J] += im_conj(l[m], cmul(g00, p[m]) + cmul(g01, p[m1])) + im_conj(l[m1], cmul(g10, p[m]) + cmul(g11, p[m1]));
          }
        }
        op_dense(p, J, u);
        op_dense(l, J, u);
      }
    if (!store8(3, g)) return false;
  }
  return true;
}

inline void quad_indices(uint32_t q, uint32_t pos0, uint32_t pos1, uint32_t* ix) {
  const uint32_t pa = pos0 < pos1 ? pos0 : pos1, pb = pos0 < pos1 ? pos1 : pos0;
  uint32_t l = ((q >> pa) << (pa + 1)) | (q & ((1u << pa) - 1u));
  l = ((l >> pb) << (pb + 1)) | (l & ((1u << pb) - 1u));
  for (int j = 0; j < 4; ++j) ix[j] = l | (uint32_t(j >> 1) << pos0) | (uint32_t(j & 1) << pos1);
}
inline void mat4_apply(const double* u, const cd* x, cd* y) {
  for (int i = 0; i < 4; ++i) {
    cd acc = 0.0;
    for (int j = 0; j < 4; ++j) acc += cmul(cd(u[(i * 4 + j) * 2], u[(i * 4 + j) * 2 + 1]), x[j]);
    y[i] = acc;
  }
}

struct Round {
  uint32_t n_inst, regmask, first, tl, dead;
  int rb[4];
  uint32_t dep[16];  // register value m deposited on the register bits
};
bool parse_round(Emulation* e, const uint32_t* prog, size_t left, int K, bool adjoint, Round* r) {
  EMU_REQUIRE(left >= size_t(kRoundWords), "round runs past the program");
  r->n_inst = (prog[0] & ~kRoundNoBarrier) >> 8;
  r->regmask = prog[1];
  r->first = prog[2];
  r->tl = prog[3];
  r->dead = prog[4];
  EMU_REQUIRE(popc(r->regmask) == 4 && (r->regmask >> K) == 0, "register mask");
  uint32_t mk = r->regmask;
  for (int j = 0; j < 4; ++j) { r->rb[j] = __builtin_ctz(mk); mk &= mk - 1; }
  for (int m = 0; m < 16; ++m) {
    r->dep[m] = 0;
    for (int j = 0; j < 4; ++j) r->dep[m] |= uint32_t((m >> j) & 1) << r->rb[j];
  }
  const RecordLayout L(4, adjoint);
  EMU_REQUIRE(size_t(r->first) + size_t(r->n_inst) * size_t(L.words()) <= e->plan->coef_init.size(), "records outside the buffer");
  return true;
}
inline uint32_t deposit(const Round& r, int m) { return r.dep[m]; }

void wht_inplace(std::vector<double>& w) {
  for (size_t h = 1; h < w.size(); h <<= 1)
    for (size_t i = 0; i < w.size(); i += h << 1)
      for (size_t j = i; j < i + h; ++j) { const double x = w[j], y = w[j + h]; w[j] = x + y; w[j + h] = x - y; }
}

}  // namespace

bool emu_forward(Emulation* e, uint32_t basis, bool skip_measure, ForwardResult* out) {
  if (!e->err.empty()) return false;
  const Plan& plan = *e->plan;
  const Model& m = *e->m;
  EMU_REQUIRE(!plan.adjoint && plan.n_eff <= 20, "forward plan");
  const size_t N = size_t(1) << plan.n_eff;
  std::vector<cd> st(N, cd(kNaN, kNaN));  // dirty memory: nothing is zero unless a pass wrote a zero
  out->values.assign(size_t(m.n_ops), 0.0);
  out->have_final = false;
  const RecordLayout L(4, false);
  std::vector<cd> tile;
  std::vector<size_t> ad;  // the tile's addresses
  std::vector<double> wbuf;
  for (size_t pi = 0; pi < plan.passes.size(); ++pi) {
    const Pass& p = plan.passes[pi];
    if (skip_measure && p.is_measure_only) continue;
    const PassArgs& a = e->args[pi];
    // engine.cpp run_forward_chunk (keep_state: the final state is wanted)
    uint32_t flags = p.flags & (PASS_INIT_BASIS | PASS_GENERAL | PASS_NO_ZERO_FILL);
    if (skip_measure) flags |= PASS_SKIP_MEASURE;
    if (!p.is_measure_only) flags |= PASS_STORE;
    const bool general = flags & PASS_GENERAL;
    const int K = p.K;
    EMU_REQUIRE(K >= kMinTileBits && K <= kMaxTileBits && a.c <= uint32_t(K) && a.n_free <= a.n_nonlocal && a.n_nonlocal + uint32_t(K) == a.n, "pass geometry");
    const uint32_t NT = 1u << (K - 4), TS = 1u << K;
    EMU_REQUIRE(size_t(a.spread_off) + (size_t(1) << (K - a.c)) <= e->tables.size(), "spread table");
    Geometry g{&a, &e->tables[a.spread_off], size_t(1) << (K - a.c), K, 0, 0, false};
    g.input(basis);
    EMU_REQUIRE(size_t(a.prog_off) < e->prog.size(), "program offset");
    const uint32_t* prog = &e->prog[a.prog_off];
    const size_t prog_n = e->prog.size() - a.prog_off;
    tile.assign(TS, cd(0.0, 0.0));
    ad.assign(TS, 0);
    for (uint32_t block = 0; block < (1u << a.n_free); ++block) {
      const uint32_t tile_id = g.launched_tile(block), tile_base = g.tile_base_of(tile_id);
      const uint32_t tile_hi = tile_id << K;
      for (uint32_t l = 0; l < TS; ++l) {
        ad[l] = g.addr(tile_base, l);
        EMU_REQUIRE(ad[l] < N, "tile address outside the state");
      }
      if (flags & PASS_INIT_BASIS) {
        if ((g.idx & a.nonlocal_mask) != tile_base) {
          if ((flags & PASS_STORE) && !(flags & PASS_NO_ZERO_FILL))
            for (uint32_t l = 0; l < TS; ++l) st[ad[l]] = cd(0.0, 0.0);
          continue;
        }
        for (uint32_t l = 0; l < TS; ++l) tile[l] = cd(0.0, 0.0);
        tile[g.in_local] = cd(1.0, 0.0);
      } else {
        for (uint32_t l = 0; l < TS; ++l) tile[l] = st[ad[l]];
        if (a.frozen_old_local)
          for (uint32_t l = 0; l < TS; ++l)
            if ((l ^ g.in_local) & a.frozen_old_local) tile[l] = cd(0.0, 0.0);
      }
      size_t pc = 0;
      for (;;) {
        EMU_REQUIRE(pc < prog_n, "program runs past its end");
        const uint32_t w0 = prog[pc], opc = w0 & 0xffu;
        if (opc == OP_END) break;
        if (opc == OP_ROUND) {
          Round r;
          if (!parse_round(e, prog + pc, prog_n - pc, K, false, &r)) return false;
          EMU_REQUIRE(size_t(a.tl_off) + size_t(r.tl) + NT <= e->tables.size(), "thread table");
          const uint32_t* TLt = &e->tables[size_t(a.tl_off) + r.tl];
          for (uint32_t tid = 0; tid < NT; ++tid) {
            const uint32_t TL = TLt[tid];
            EMU_REQUIRE((TL >> K) == 0, "thread table entry outside the tile");
            cd amp[16];
            for (int mm = 0; mm < 16; ++mm) amp[mm] = tile[TL | deposit(r, mm)];
            for (uint32_t i = 0; i < r.n_inst; ++i) {
              const size_t ro = size_t(r.first) + size_t(i) * size_t(L.words());
              instance_fwd(Record{&plan.coef_init[ro], &e->cf[ro]}, amp, TL | tile_hi, general);
            }
            for (int mm = 0; mm < 16; ++mm) tile[TL | deposit(r, mm)] = amp[mm];
          }
          pc += kRoundWords;
        } else if (opc == OP_GATE2) {
          EMU_REQUIRE(pc + kGate2Words <= prog_n, "gate2 words");
          if (general) {  // (the lean kernel variant steps over it)
            const uint32_t pw = prog[pc + 1], pos0 = pw & 0xffu, pos1 = (pw >> 8) & 0xffu;
            EMU_REQUIRE(pos0 < uint32_t(K) && pos1 < uint32_t(K) && pos0 != pos1, "gate2 bits");
            EMU_REQUIRE(size_t(prog[pc + 2]) + 32 <= e->cf.size(), "gate2 coefficients");
            const double* u = &e->cf[prog[pc + 2]];
            for (uint32_t q = 0; q < (1u << (K - 2)); ++q) {
              uint32_t ix[4];
              quad_indices(q, pos0, pos1, ix);
              cd x[4], y[4];
              for (int j = 0; j < 4; ++j) x[j] = tile[ix[j]];
              mat4_apply(u, x, y);
              for (int j = 0; j < 4; ++j) tile[ix[j]] = y[j];
            }
          }
          pc += kGate2Words;
        } else if (opc == OP_MEASURE_WHT) {
          const size_t n_terms = w0 >> 8;
          EMU_REQUIRE(pc + kWhtHeaderWords + n_terms * kMeasTermWords <= prog_n, "wht words");
          const uint32_t* class_end = prog + pc + 1;
          const uint32_t* terms = prog + pc + kWhtHeaderWords;
          pc += size_t(kWhtHeaderWords) + n_terms * kMeasTermWords;
          if (flags & PASS_SKIP_MEASURE) continue;
          // |psi|^2 through a Walsh-Hadamard transform over ALL local bits: the kernel transforms register and lane bits and
          // adds the waves with the parity of the term's wave bits, which is the same sum; the REGISTER part of the
          // coefficient it reads is the class the term sits in, not the term's own mask
          wbuf.resize(TS);
          for (uint32_t l = 0; l < TS; ++l) wbuf[l] = std::norm(tile[l]);
          wht_inplace(wbuf);
          uint32_t begin = 0;
          for (uint32_t c = 0; c < 16; ++c) {
            const uint32_t end = class_end[c];
            for (uint32_t k = begin; k < end; ++k) {  // (begin >= end: the kernel's loop does not run either)
              EMU_REQUIRE(k < n_terms, "class table runs past the terms");
              const uint32_t* tw = terms + size_t(k) * kMeasTermWords;
              const uint32_t zl = tw[0], zn = tw[1], op = tw[3];
              float cf;
              std::memcpy(&cf, &tw[2], 4);
              EMU_REQUIRE(op < uint32_t(m.n_ops), "wht operator index");
              const uint32_t zeff = (c << (K - 4)) | (zl & (NT - 1u));
              const double v = double(cf) * wbuf[zeff];
              out->values[op] += (popc(tile_base & zn) & 1) ? -v : v;
            }
            begin = end;
          }
        } else if (opc == OP_MEASURE) {
          const uint32_t n_groups = w0 >> 8;
          ++pc;
          for (uint32_t gi = 0; gi < n_groups; ++gi) {
            EMU_REQUIRE(pc + 2 <= prog_n, "measure group words");
            const uint32_t xl = prog[pc], n_terms = prog[pc + 1];
            pc += 2;
            EMU_REQUIRE(pc + size_t(n_terms) * kMeasTermWords <= prog_n, "measure term words");
            if (flags & PASS_SKIP_MEASURE) { pc += size_t(n_terms) * kMeasTermWords; continue; }
            EMU_REQUIRE((xl >> K) == 0, "measure x mask outside the tile");
            for (uint32_t k = 0; k < n_terms; ++k, pc += kMeasTermWords) {
              const uint32_t zl = prog[pc] & (TS - 1u), zn = prog[pc + 1], ow = prog[pc + 3];
              float cf;
              std::memcpy(&cf, &prog[pc + 2], 4);
              const uint32_t op = ow & 0xffffffu, ny = ow >> 24;
              EMU_REQUIRE(op < uint32_t(m.n_ops), "operator index");
              double sum = 0.0;  // Re(i^ny (-1)^popc(l & z) conj(psi[l ^ x]) psi[l]): ny = 0: wr, 1: -wi, 2: -wr, 3: wi
              for (uint32_t l = 0; l < TS; ++l) {
                const cd q = tile[l ^ xl], pp = tile[l];
                const double v = (ny & 1u) ? q.real() * pp.imag() - q.imag() * pp.real() : q.real() * pp.real() + q.imag() * pp.imag();
                sum += (popc(l & zl) & 1) ? -v : v;
              }
              double sfac = (ny == 1 || ny == 2) ? -double(cf) : double(cf);
              if (popc(tile_base & zn) & 1) sfac = -sfac;
              out->values[op] += sfac * sum;
            }
          }
        } else {
          EMU_REQUIRE(false, "unknown opcode");
        }
      }
      if (flags & PASS_STORE)
        for (uint32_t l = 0; l < TS; ++l) st[ad[l]] = tile[l];
    }
    if (p.completes_circuit) {
      out->final_state.assign(N, cd(0.0, 0.0));
      for (size_t i = 0; i < N; ++i) {
        size_t phys = 0;
        for (int b = 0; b < plan.n_eff; ++b)
          if (i >> b & 1) phys |= size_t(1) << a.phys_of[b];
        EMU_REQUIRE(phys < N, "phys_of");
        out->final_state[i] = st[phys];
      }
      out->have_final = true;
    }
  }
  if (!skip_measure)  // measure_global_kernel on the final state in memory (forward plans: logical = physical addresses)
    for (int ti : plan.global_terms) {
      EMU_REQUIRE(ti >= 0 && size_t(ti) < m.terms.size(), "global term index");
      const PauliTerm& t = m.terms[size_t(ti)];
      EMU_REQUIRE(size_t(t.x) < N, "global term x mask");
      const uint32_t ny = uint32_t(t.ny) & 3u;  // (DevTerm::ny is the number of Y factors; the kernel reduces it)
      double acc = 0.0;
      for (size_t j = 0; j < N; ++j) {
        const cd q = st[j ^ t.x], own = st[j];
        const double wr = q.real() * own.real() + q.imag() * own.imag(), wi = q.real() * own.imag() - q.imag() * own.real();
        double v = (ny & 1u) ? wi : wr;
        if (ny == 1u || ny == 2u) v = -v;
        acc += (popc(uint32_t(j) & t.z) & 1) ? -v : v;
      }
      out->values[size_t(t.op)] += acc * double(t.coeff);
    }
  return true;
}

bool emu_adjoint(Emulation* e, uint32_t basis, const std::vector<cd>& psi, const std::vector<cd>& lam, AdjointResult* out) {
  if (!e->err.empty()) return false;
  const Plan& plan = *e->plan;
  const Model& m = *e->m;
  EMU_REQUIRE(plan.adjoint && plan.n_eff <= 20, "adjoint plan");
  const size_t N = size_t(1) << plan.n_eff;
  EMU_REQUIRE(psi.size() == N && lam.size() == N, "state size");
  const size_t n_slots_total = plan.slot_gate.size();
  out->slots.assign(n_slots_total, 0.0);
  out->grad.assign(size_t(m.n_params), 0.0);
  out->bar.assign(size_t(m.n_params), 1e-10);
  std::vector<cd> sp(N), sl(N);
  if (!plan.passes.empty()) {  // the pair in the layout the first backward pass loads
    const PassArgs& a0 = e->args[0];
    for (size_t i = 0; i < N; ++i) {
      size_t phys = 0;
      for (int b = 0; b < plan.n_eff; ++b)
        if (i >> b & 1) phys |= size_t(1) << a0.phys_of[b];
      EMU_REQUIRE(phys < N, "phys_of");
      sp[phys] = psi[i];
      sl[phys] = lam[i];
    }
  }
  const RecordLayout L(4, true);
  const int K = plan.K;  // (engine.cpp run_adjoint_chunk launches every pass with the PLAN's tile size)
  const uint32_t NT = 1u << (K - 4), TS = 1u << K;
  std::vector<cd> tp(TS), tl(TS);
  std::vector<size_t> ad(TS);           // the tile's addresses
  std::vector<char> written(N, 0);      // by the relabeling store of the tile at hand
  std::vector<size_t> wrote;
  for (size_t pi = 0; pi < plan.passes.size(); ++pi) {
    const Pass& p = plan.passes[pi];
    const PassArgs& a = e->args[pi];
    const uint32_t flags = a.flags;
    const bool general = flags & PASS_GENERAL;
    EMU_REQUIRE(p.K == K, "an adjoint pass with a tile size of its own");
    EMU_REQUIRE(a.c <= uint32_t(K) && a.n_free <= a.n_nonlocal && a.n_nonlocal + uint32_t(K) == a.n, "pass geometry");
    EMU_REQUIRE(size_t(a.spread_off) + (size_t(1) << (K - a.c)) <= e->tables.size(), "spread table");
    EMU_REQUIRE(size_t(a.slot_base) + a.n_slots <= n_slots_total, "slot range of the pass");
    Geometry g{&a, &e->tables[a.spread_off], size_t(1) << (K - a.c), K, 0, 0, a.c == 0};
    g.input(basis);
    EMU_REQUIRE(size_t(a.prog_off) < e->prog.size(), "program offset");
    const uint32_t* prog = &e->prog[a.prog_off];
    const size_t prog_n = e->prog.size() - a.prog_off;
    double* slots = out->slots.data() + a.slot_base;
    for (uint32_t block = 0; block < (1u << a.n_free); ++block) {
      const uint32_t tile_id = g.launched_tile(block), tile_base = g.tile_base_of(tile_id);
      const uint32_t tile_hi = tile_id << K;
      // the exchange-layout kernel (lean passes) returns at once on a program that does not begin with a round
      if (!general && (prog[0] & 0xffu) != OP_ROUND) continue;
      for (uint32_t l = 0; l < TS; ++l) {
        ad[l] = g.addr(tile_base, l);
        EMU_REQUIRE(ad[l] < N, "tile address outside the state");
        tp[l] = sp[ad[l]];
        tl[l] = sl[ad[l]];
      }
      if (!general && a.frozen_old_local)  // (the two-tile kernel of general passes has no such step)
        for (uint32_t l = 0; l < TS; ++l)
          if ((l ^ g.in_local) & a.frozen_old_local) { tp[l] = cd(0.0, 0.0); tl[l] = cd(0.0, 0.0); }
      size_t pc = 0;
      for (;;) {
        EMU_REQUIRE(pc < prog_n, "program runs past its end");
        const uint32_t w0 = prog[pc], opc = w0 & 0xffu;
        if (opc == OP_ROUND) {
          Round r;
          if (!parse_round(e, prog + pc, prog_n - pc, K, true, &r)) return false;
          EMU_REQUIRE(size_t(a.tl_off) + size_t(r.tl) + NT <= e->tables.size(), "thread table");
          const uint32_t* TLt = &e->tables[size_t(a.tl_off) + r.tl];
          for (uint32_t tid = 0; tid < NT; ++tid) {
            const uint32_t TL = TLt[tid];
            EMU_REQUIRE((TL >> K) == 0, "thread table entry outside the tile");
            if (!general && ((TL ^ g.in_local) & r.dead)) continue;  // a dead wave skips the instances, its amplitudes stay
            cd pp[16], ll[16];
            for (int mm = 0; mm < 16; ++mm) { pp[mm] = tp[TL | deposit(r, mm)]; ll[mm] = tl[TL | deposit(r, mm)]; }
            for (uint32_t i = 0; i < r.n_inst; ++i) {
              const size_t ro = size_t(r.first) + size_t(i) * size_t(L.words());
              if (!instance_adj(e, Record{&plan.coef_init[ro], &e->cf[ro]}, pp, ll, TL | tile_hi, general, slots, a.n_slots)) return false;
            }
            for (int mm = 0; mm < 16; ++mm) { tp[TL | deposit(r, mm)] = pp[mm]; tl[TL | deposit(r, mm)] = ll[mm]; }
          }
          pc += kRoundWords;
          continue;
        }
        if (!general) {  // the exchange kernel's loop ends at the first word that is no round
          EMU_REQUIRE(opc == OP_END, "a lean adjoint pass holds an op its kernel does not execute");
          break;
        }
        if (opc == OP_END) break;
        EMU_REQUIRE(opc == OP_GATE2 && pc + kGate2Words <= prog_n, "adjoint opcode");
        {
          const uint32_t pw = prog[pc + 1], pos0 = pw & 0xffu, pos1 = (pw >> 8) & 0xffu, slot = prog[pc + 3];
          EMU_REQUIRE(pos0 < uint32_t(K) && pos1 < uint32_t(K) && pos0 != pos1, "gate2 bits");
          EMU_REQUIRE(size_t(prog[pc + 2]) + 64 <= e->cf.size(), "gate2 coefficients");
          EMU_REQUIRE(slot == 0xffffffffu || slot < a.n_slots, "gate2 slot");
          const double* u = &e->cf[prog[pc + 2]];
          double gacc = 0.0;
          for (uint32_t q = 0; q < (1u << (K - 2)); ++q) {
            uint32_t ix[4];
            quad_indices(q, pos0, pos1, ix);
            cd x[4], lv[4], y[4];
            for (int j = 0; j < 4; ++j) { x[j] = tp[ix[j]]; lv[j] = tl[ix[j]]; }
            if (slot != 0xffffffffu) {
              mat4_apply(u + 32, x, y);
              for (int j = 0; j < 4; ++j) gacc += im_conj(lv[j], y[j]);
            }
            mat4_apply(u, x, y);
            for (int j = 0; j < 4; ++j) tp[ix[j]] = y[j];
            mat4_apply(u, lv, y);
            for (int j = 0; j < 4; ++j) tl[ix[j]] = y[j];
          }
          if (slot != 0xffffffffu) slots[slot] += gacc;
          pc += kGate2Words;
        }
      }
      if (!general && (flags & PASS_RELABEL)) {
        // store_tile_relabeled: only the amplitudes whose newly finished bits equal the input, at their new addresses
        EMU_REQUIRE(a.n_fz <= uint32_t(K), "finished bits");
        const uint32_t n_live = uint32_t(K) - a.n_fz;
        EMU_REQUIRE(!a.relabel_pairs || n_live >= 1, "relabel pairs without a live bit");
        const uint32_t count = a.relabel_pairs ? 1u << (n_live - 1u) : 1u << n_live;
        EMU_REQUIRE(size_t(a.relabel_off) + (size_t(2) << n_live) <= e->tables.size(), "relabel table");
        uint32_t fz_addr = 0;
        for (uint32_t pos = 0; pos < 32; ++pos) {
          const uint32_t src = a.fz_src[pos];
          if (src != 0xffu && ((g.in_local >> (src & 31u)) & 1u)) fz_addr |= 1u << pos;
        }
        const uint32_t fz_local = g.in_local & a.frozen_new_local;
        const size_t sb = size_t(tile_base | fz_addr);
        auto put = [&](size_t at, uint32_t l) -> bool {
          EMU_REQUIRE(at < N && l < TS, "relabeling store outside the state or the tile");
          sp[at] = tp[l];
          sl[at] = tl[l];
          written[at] = 1;
          wrote.push_back(at);
          return true;
        };
        for (uint32_t tid = 0; tid < NT; ++tid) {
          const uint32_t mine = std::min(tid, count - 1u) << (a.relabel_pairs ? 1 : 0);
          const uint32_t l_mine = e->tables[a.relabel_off + 2u * mine], off_mine = e->tables[a.relabel_off + 2u * mine + 1u];
          for (uint32_t i = 0; i < (a.relabel_pairs ? 8u : 16u); ++i) {
            if (!(i < a.relabel_iters && tid + i * NT < count)) continue;
            const uint32_t l0 = l_mine | a.relabel_hi[i][0] | fz_local;
            const size_t at = sb + size_t(off_mine | a.relabel_hi[i][1]);
            if (!put(at, l0)) return false;
            if (a.relabel_pairs && !put(at + 1, l0 | a.relabel_l1)) return false;
          }
        }
        // dirty memory: what the tile owned and the store did not write holds nothing a later pass may use
        for (uint32_t l = 0; l < TS; ++l)
          if (!written[ad[l]]) { sp[ad[l]] = cd(kNaN, kNaN); sl[ad[l]] = cd(kNaN, kNaN); }
        for (size_t at : wrote) written[at] = 0;
        wrote.clear();
      } else if (flags & PASS_STORE) {
        for (uint32_t l = 0; l < TS; ++l) { sp[ad[l]] = tp[l]; sl[ad[l]] = tl[l]; }
      }
    }
  }
  for (size_t s = 0; s < n_slots_total; ++s) {
    const int gate = plan.slot_gate[s];
    EMU_REQUIRE(gate >= 0 && size_t(gate) < m.gates.size(), "slot gate");
    const int prm = m.gates[size_t(gate)].param_idx;
    EMU_REQUIRE(prm >= 0 && prm < m.n_params, "slot of a gate without a parameter");
    const double v = double(plan.slot_factor[s]) * out->slots[s];
    out->grad[size_t(prm)] += v;
    out->bar[size_t(prm)] += 4.0 * std::ldexp(1.0, -24) * std::fabs(v);
  }
  return true;
}

}  // namespace emu
