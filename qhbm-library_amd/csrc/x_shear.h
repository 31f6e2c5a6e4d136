// x_shear.h -- coefficient arithmetic of the X**t micro-op, shared by prep_coefs_kernel, combine_diag_kernel and
// the host (tests/x_shear/x_shear_check.cpp checks it against the closed-form matrices in double).
//
// X**t core c*I - i*s*X, theta = pi t / 2 with t reduced to one period, c = cos(theta), s = sin(theta).
//
//   three shears   [[c, -is], [-is, c]] = T(tan(theta/2)) S(sin(theta)) T(tan(theta/2))
//                  T(w) = [[1, -iw], [0, 1]] (a0 += -i w a1),  S(w) = [[1, 0], [-iw, 1]] (a1 += -i w a0)
//   two shears     [[c, -is], [-is, c]] = D S(s c) T(tan(theta)),  D = diag(c, 1/c)              (forward: D LAST)
//                  [[c,  is], [ is, c]] = S(-tan(theta)) T(-s c) D                               (adjoint: D FIRST)
//
// D is a real diagonal on the gate's register bit.  In an instance with a FULL diagonal table the table sits on D's
// side of the X gates in both sweeps (forward: X then table, adjoint: table then X), so combine_diag_kernel multiplies
// D into the table entries and the kernels run two packed FMAs per pair instead of three.  Both sweeps run T on the slot's
// first float and S on the second, so the adjoint slot holds (-s c, -tan(theta)).
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QHBM_HD __host__ __device__
#else
#define QHBM_HD
#endif

namespace qhbm {

// A gate takes the two-shear form when |theta| <= theta_max = pi / 3, i.e. |reduced exponent| <= 2/3.  The second
// shear forms c^2 a1 = a1 - (s c)(tan(theta) a1) by cancellation, and the table then divides by c: an absolute
// rounding error of the shears reaches the amplitude amplified by 1 / c, at most 2 at pi / 3, and |tan(theta)| stays
// below 1.74, against the 1 of tan(theta / 2).  Towards pi / 2 the factor 1 / c is unbounded (2.8 at 1.2 rad).
// Two thirds of a uniform exponent range qualify.
constexpr double kXTwoShearMaxExponent = 2.0 / 3.0;

struct XShearCoefs {
  double tr;       // reduced exponent in [-1, 1]
  double c, s;     // cos, sin of theta = pi tr / 2
  bool two_shear;  // the form `first`, `second` are written in
  double first, second;  // T coefficient, S coefficient (already negated / swapped for the adjoint)
  double d0, d1;   // D factors of register bit clear / set (1, 1 for three shears)
};

QHBM_HD inline double x_reduced_exponent(double t) { return t - 2.0 * rint(0.5 * t); }

// sin, cos of pi x for |x| <= 1/2
QHBM_HD inline void x_sincospi(double x, double* s, double* c) {
#if defined(__HIP_DEVICE_COMPILE__)
  sincospi(x, s, c);
#else
  const double kPi = 3.14159265358979323846;
  *s = sin(kPi * x);
  *c = x == 0.5 || x == -0.5 ? 0.0 : cos(kPi * x);
#endif
}

QHBM_HD inline bool x_two_shear_ok(double tr) { return fabs(tr) <= kXTwoShearMaxExponent; }

// The two forms for a reduced exponent whose c, s are set.  Both are valid for every angle short of +-pi / 2 (two
// shears: c != 0); which one runs is a matter of rounding error and of where the gate sits.
QHBM_HD inline void x_three_shear_form(XShearCoefs* k, bool dagger) {
  const double sgn = dagger ? -1.0 : 1.0;
  k->two_shear = false;
  k->first = sgn * k->s / (1.0 + k->c);  // tan(theta / 2), |.| <= 1
  k->second = sgn * k->s;
  k->d0 = k->d1 = 1.0;
}
QHBM_HD inline void x_two_shear_form(XShearCoefs* k, bool dagger) {
  const double tn = k->s / k->c, sc = k->s * k->c;
  k->two_shear = true;
  k->first = dagger ? -sc : tn;
  k->second = dagger ? -tn : sc;
  k->d0 = k->c;
  k->d1 = 1.0 / k->c;
}

// `t`: the gate's exponent (any size), `eligible`: the micro-op sits in a FULL instance and the option is on,
// `dagger`: the adjoint sweep un-applies the gate.
QHBM_HD inline XShearCoefs x_shear_coefs(double t, bool eligible, bool dagger) {
  XShearCoefs k;
  k.tr = x_reduced_exponent(t);
  x_sincospi(0.5 * k.tr, &k.s, &k.c);
  if (eligible && x_two_shear_ok(k.tr)) x_two_shear_form(&k, dagger);
  else x_three_shear_form(&k, dagger);
  return k;
}

// D factors of a two-shear gate from its reduced exponent alone (combine_diag_kernel reads the exponent that
// prep_coefs_kernel left in the record, in double).
QHBM_HD inline void x_two_shear_d(double tr, double* d0, double* d1) {
  double s, c;
  x_sincospi(0.5 * tr, &s, &c);
  *d0 = c;
  *d1 = 1.0 / c;
}

// One FULL table: entry m (0..15) = product of the instance's PH1 / PH2 phases contained in register value m, times
// the D factors of its two-shear X bits.  ph1[j] / ph2[pair] = (cos, sin) pairs; masks as in the record header;
// two_mask = register bits with a two-shear X, tr[j] their reduced exponents.  Entry 0 is real (out[0], out[1] = 0).
QHBM_HD inline void x_full_entry(int m, unsigned ph1_mask, unsigned ph2_mask, const double (*ph1)[2], const double (*ph2)[2],
                                 unsigned two_mask, const double* tr, double* re, double* im) {
  double cr = 1.0, ci = 0.0;
  for (int j = 0; j < 4; ++j)
    if (((m >> j) & 1) && ((ph1_mask >> j) & 1u)) {
      const double a = ph1[j][0], b = ph1[j][1], nr = cr * a - ci * b, ni = cr * b + ci * a;
      cr = nr;
      ci = ni;
    }
  for (int jb = 1; jb < 4; ++jb)
    for (int ja = 0; ja < jb; ++ja) {
      const int pi = jb * (jb - 1) / 2 + ja;
      if (((m >> ja) & 1) && ((m >> jb) & 1) && ((ph2_mask >> pi) & 1u)) {
        const double a = ph2[pi][0], b = ph2[pi][1], nr = cr * a - ci * b, ni = cr * b + ci * a;
        cr = nr;
        ci = ni;
      }
    }
  double d = 1.0;
  for (int j = 0; j < 4; ++j)
    if ((two_mask >> j) & 1u) {
      double d0, d1;
      x_two_shear_d(tr[j], &d0, &d1);
      d *= ((m >> j) & 1) ? d1 : d0;
    }
  *re = cr * d;
  *im = ci * d;
}

}  // namespace qhbm
