// Host check of csrc/x_shear.h, the coefficient arithmetic prep_coefs_kernel and combine_diag_kernel call: built with
// -fsanitize=address,undefined and run by tests/test_x_two_shear_cpu.py.
//
//   1. For 10^4 exponents (random over several periods, +-theta_max and its neighbours one ulp either side, 0, +-1
//      (theta = +-pi / 2), exponents far outside one period) the composed shears equal the closed-form matrix of
//      X**t, c I - i s X (forward) and c I + i s X (adjoint), in double: three shears T S T, two shears D S T
//      (forward) and S T D (adjoint).  Within one ulp of the flag boundary BOTH forms must hold.
//   2. The coefficients rounded to float, as the records hold them, still compose to the matrix within the
//      rounding of three factors amplified by 1 / c <= 2.
//   3. The FULL table of an instance with up to four X bits and random PH1 / PH2 phases equals the product of the
//      phases and the D factors, entry 0 included.
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../qhbm-library_amd/csrc/x_shear.h"

using cd = std::complex<double>;
using namespace qhbm;

namespace {

struct M2 { cd m[2][2]; };
M2 mul(const M2& a, const M2& b) {
  M2 r;
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j];
  return r;
}
M2 shear_t(double w) { return M2{{{1.0, cd(0.0, -w)}, {0.0, 1.0}}}; }  // a0 += -i w a1
M2 shear_s(double w) { return M2{{{1.0, 0.0}, {cd(0.0, -w), 1.0}}}; }  // a1 += -i w a0
M2 diag(double d0, double d1) { return M2{{{d0, 0.0}, {0.0, d1}}}; }

// the matrix the kernels' sequence composes to: T(first) then S(second) (then T(first) again), D on the table's side
M2 composed(const XShearCoefs& k, bool dagger, bool as_float) {
  const double f = as_float ? double(float(k.first)) : k.first, s = as_float ? double(float(k.second)) : k.second;
  const double d0 = as_float ? double(float(k.d0)) : k.d0, d1 = as_float ? double(float(k.d1)) : k.d1;
  M2 u = mul(shear_s(s), shear_t(f));
  if (!k.two_shear) return mul(shear_t(f), u);
  return dagger ? mul(u, diag(d0, d1)) : mul(diag(d0, d1), u);
}

// closed form, from an independent reduction of the exponent
M2 closed_form(double t, bool dagger) {
  const double tr = std::remainder(t, 2.0);
  const double th = 1.5707963267948966192 * tr;
  const double c = std::cos(th), s = dagger ? -std::sin(th) : std::sin(th);
  return M2{{{c, cd(0.0, -s)}, {cd(0.0, -s), c}}};
}
double dist(const M2& a, const M2& b) {
  double d = 0.0;
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) d = std::fmax(d, std::abs(a.m[i][j] - b.m[i][j]));
  return d;
}

int failures = 0;
void fail(const char* what, double t, double err) {
  if (++failures <= 20) std::printf("FAIL %s at t = %.17g: %.3g\n", what, t, err);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261017);
  std::uniform_real_distribution<double> uni(-4.0, 4.0);
  std::vector<double> ts;
  const double m = kXTwoShearMaxExponent;
  for (double sg : {1.0, -1.0}) {
    ts.push_back(sg * m);
    ts.push_back(sg * std::nextafter(m, 0.0));
    ts.push_back(sg * std::nextafter(m, 1.0));
    ts.push_back(sg * 1.0);
    ts.push_back(sg * std::nextafter(1.0, 0.0));
    for (double far : {1e6 + 0.3, 12345.678, 4e9 + 0.59375, 1e15 + 0.625, 2.0 + m, 1e6 + 1.0})
      ts.push_back(sg * far);
  }
  ts.push_back(0.0);
  while (ts.size() < 10000) ts.push_back(uni(rng));
  int n_two = 0, n_three = 0;
  double worst_d = 0.0, worst_f = 0.0;
  for (double t : ts) {
    for (int dagger = 0; dagger < 2; ++dagger) {
      const M2 want = closed_form(t, dagger != 0);
      for (int eligible = 0; eligible < 2; ++eligible) {
        const XShearCoefs k = x_shear_coefs(t, eligible != 0, dagger != 0);
        if (!eligible && k.two_shear) fail("two shears outside a FULL instance", t, 0.0);
        if (k.two_shear != (eligible && std::fabs(k.tr) <= m)) fail("flag", t, k.tr);
        if (k.two_shear && (k.d1 > 2.0 * (1.0 + 1e-15) || k.d0 < 0.5 * (1.0 - 1e-15))) fail("1 / c above 2 under the flag", t, k.d1);
        if (!k.two_shear && std::fabs(k.first) > 1.0) fail("tan(theta / 2) above 1", t, k.first);
        (k.two_shear ? n_two : n_three) += 1;
        // far exponents: the reduction t - 2 rint(t / 2) is exact in double, so the same bar holds there
        const double ed = dist(composed(k, dagger != 0, false), want);
        if (!(ed <= 1e-14)) fail(k.two_shear ? "two shears, double" : "three shears, double", t, ed);
        worst_d = std::fmax(worst_d, ed);
        // float coefficients: three factors, each off by 2^-24 relative, products bounded by (1 / c) (1 + tan^2) <= 8
        const double ef = dist(composed(k, dagger != 0, true), want);
        if (!(ef <= 8.0 * 3.0 * 5.97e-8)) fail("float coefficients", t, ef);
        worst_f = std::fmax(worst_f, ef);
      }
      // within an ulp of the boundary both forms hold (the choice there is free)
      XShearCoefs k;
      k.tr = x_reduced_exponent(t);
      x_sincospi(0.5 * k.tr, &k.s, &k.c);
      if (std::fabs(std::fabs(k.tr) - m) <= 4e-16 || std::fabs(k.tr) < 0.95) {
        x_two_shear_form(&k, dagger != 0);
        const double e2 = dist(composed(k, dagger != 0, false), want);
        x_three_shear_form(&k, dagger != 0);
        const double e3 = dist(composed(k, dagger != 0, false), want);
        if (!(e2 <= 2e-13 && e3 <= 1e-14)) fail("both forms", t, std::fmax(e2, e3));
      }
    }
  }
  std::printf("x_shear_check: %zu exponents, %d two-shear and %d three-shear forms, worst error %.3g (double) %.3g (float coefficients)\n",
              ts.size(), n_two, n_three, worst_d, worst_f);

  // ---- the FULL table with D folded in ----
  std::uniform_real_distribution<double> ang(-3.14159265358979, 3.14159265358979), ex(-m, m);
  int tables = 0;
  for (int it = 0; it < 2000; ++it) {
    const unsigned ph1_mask = unsigned(rng() & 15u), ph2_mask = unsigned(rng() & 63u), two_mask = unsigned(it < 16 ? it : rng() & 15u);
    double ph1[4][2], ph2[6][2], tr[4];
    cd z1[4], z2[6];
    for (int j = 0; j < 4; ++j) { const double a = ang(rng); ph1[j][0] = std::cos(a); ph1[j][1] = std::sin(a); z1[j] = cd(ph1[j][0], ph1[j][1]); tr[j] = ex(rng); }
    for (int p = 0; p < 6; ++p) { const double a = ang(rng); ph2[p][0] = std::cos(a); ph2[p][1] = std::sin(a); z2[p] = cd(ph2[p][0], ph2[p][1]); }
    for (int mm = 0; mm < 16; ++mm) {
      cd want(1.0, 0.0);
      for (int j = 0; j < 4; ++j) if ((mm >> j & 1) && (ph1_mask >> j & 1u)) want *= z1[j];
      int p = 0;
      for (int jb = 1; jb < 4; ++jb)
        for (int ja = 0; ja < jb; ++ja, ++p)
          if ((mm >> ja & 1) && (mm >> jb & 1) && (ph2_mask >> p & 1u)) want *= z2[p];
      for (int j = 0; j < 4; ++j)
        if (two_mask >> j & 1u) {
          const double c = std::cos(1.5707963267948966192 * tr[j]);
          want *= (mm >> j & 1) ? 1.0 / c : c;
        }
      double re, im;
      x_full_entry(mm, ph1_mask, ph2_mask, ph1, ph2, two_mask, tr, &re, &im);
      const double e = std::abs(cd(re, im) - want);
      if (!(e <= 1e-13)) fail("table entry", double(mm), e);  // |entry| <= 2^4
      if (mm == 0 && im != 0.0) fail("entry 0 not real", 0.0, im);
      if (two_mask == 0 && mm == 0 && !(re == 1.0)) fail("entry 0 without two-shear gates", 0.0, re);
    }
    ++tables;
  }
  std::printf("x_shear_check: %d tables\n", tables);
  std::printf("x_shear_check: %d failures\n", failures);
  return failures ? 1 : 0;
}
