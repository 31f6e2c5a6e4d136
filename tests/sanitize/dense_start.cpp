// dense_start.cpp -- the dense-start plans of the from-states calls (schedule.h Model::dense_input) on the CPU.
//
// Test infrastructure, not product (tests/test_dense_start_emulated_cpu.py builds and runs it, host only, with
// AddressSanitizer + UBSan like plan_fuzz).  plan_emulate.h's forward emulation starts from a bitstring and cannot be
// handed a state, so two things are checked here:
//   * structure -- no forward pass writes a basis state or counts on zeros (flags, zero_mask, frozen_old_local of the
//     arguments fill_args derives), no adjoint pass prunes, relabels or declares a wave dead, while the basis-state
//     plans of the same model do some of this (the case is one that prunes);
//   * the BACKWARD dense-start plan executed by the emulator from psi = C phi for a random, dense phi, lambda = sum_k
//     up_k O_k psi, against central differences (step 1e-5, bar 1e-7 ||grad||_inf) of sum_k up_k <phi|C^dagger O_k C|phi>
//     evaluated gate by gate from plan_emulate.h's oracle matrices -- with gradient masks, stopping early or not.
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "plan_emulate.h"

using namespace qhbm;
typedef emu::cd cd;

namespace {

int g_failures = 0;
void expect(bool ok, const std::string& what) {
  if (!ok) { std::printf("dense_start: FAILED %s\n", what.c_str()); ++g_failures; }
}

// U on index bits (n - 1 - q0[, n - 1 - q1]); matrix index of a two-qubit gate = (bit of q0) << 1 | (bit of q1)
void apply(std::vector<cd>& s, int n, const Gate& g, int nq, const cd* U) {
  const size_t N = size_t(1) << n, b0 = size_t(1) << (n - 1 - g.q0), b1 = nq == 2 ? size_t(1) << (n - 1 - g.q1) : 0;
  for (size_t i = 0; i < N; ++i) {
    if (i & (b0 | b1)) continue;
    if (nq == 1) {
      const cd a = s[i], b = s[i | b0];
      s[i] = U[0] * a + U[1] * b;
      s[i | b0] = U[2] * a + U[3] * b;
    } else {
      const size_t idx[4] = {i, i | b1, i | b0, i | b0 | b1};
      cd v[4];
      for (int r = 0; r < 4; ++r) { v[r] = 0; for (int c = 0; c < 4; ++c) v[r] += U[4 * r + c] * s[idx[c]]; }
      for (int r = 0; r < 4; ++r) s[idx[r]] = v[r];
    }
  }
}

std::vector<cd> run_circuit(const Model& m, const std::vector<double>& params, std::vector<cd> s) {
  for (const Gate& g : m.gates) {
    cd U[16], A[16];
    const int nq = emu::oracle_gate(g.kind, emu::oracle_exponent(g, params), double(g.global_shift), U, A);
    apply(s, m.n, g, nq, U);
  }
  return s;
}

double objective(const Model& m, const std::vector<double>& params, const std::vector<cd>& phi, const std::vector<double>& up) {
  const std::vector<double> v = emu::oracle_values(m, run_circuit(m, params, phi));
  double e = 0.0;
  for (size_t k = 0; k < v.size(); ++k) e += up[k] * v[k];
  return e;
}

Model make_model(int n, int layers, int idle, int diagonal, std::mt19937_64& rng) {
  Model m;
  m.n = n;
  int p = 0;
  for (int l = 0; l < layers; ++l) {
    for (int q = 0; q < n; ++q) {
      if (q == idle) continue;
      if (q != diagonal) m.gates.push_back(Gate{QHBM_GATE_XPOW, q, -1, p++, 1.f, 0.f, 0.f});
      m.gates.push_back(Gate{QHBM_GATE_ZPOW, q, -1, p++, 1.f, 0.f, 0.f});
    }
    for (int start = 0; start < 2; ++start)
      for (int q = start; q + 1 < n; q += 2)
        if (q != idle && q + 1 != idle) m.gates.push_back(Gate{QHBM_GATE_CZPOW, q, q + 1, p++, 1.f, 0.f, 0.f});
  }
  m.n_params = p;
  m.n_ops = 2;
  std::uniform_real_distribution<float> C(-1.f, 1.f);
  for (int q = 0; q < n; ++q) {  // a transverse-field ring and a few random strings
    m.terms.push_back(PauliTerm{C(rng), 0u, (1u << q) | (1u << ((q + 1) % n)), 0, 0});
    m.terms.push_back(PauliTerm{C(rng), 1u << q, 0u, 0, 0});
  }
  for (int t = 0; t < 8; ++t) {
    const uint32_t x = uint32_t(rng()) & ((1u << n) - 1u), z = uint32_t(rng()) & ((1u << n) - 1u);
    m.terms.push_back(PauliTerm{C(rng), x, z, __builtin_popcount(x & z), 1});
  }
  return m;
}

// forward, or adjoint and relabeling
PlanOptions options(int tile, bool adjoint) {
  PlanOptions o;
  o.tile_bits = tile;
  o.adjoint = adjoint;
  o.relabel = adjoint;
  return o;
}

void check_structure(const Model& dense, int tile) {
  Model basis = dense;
  basis.dense_input = false;
  std::string err;
  for (int adjoint = 0; adjoint < 2; ++adjoint) {
    Plan pd, pb;
    expect(build_plan(dense, options(tile, adjoint != 0), &pd, &err), "dense plan builds: " + err);
    expect(build_plan(basis, options(tile, adjoint != 0), &pb, &err), "basis plan builds: " + err);
    std::vector<PassArgs> ad, ab;
    std::vector<uint32_t> prog, tables;
    fill_args(pd, dense, &ad, &prog, &tables);
    fill_args(pb, basis, &ab, &prog, &tables);
    expect(pd.passes.size() > 1, "the case has several passes");
    bool basis_prunes = false;
    for (size_t i = 0; i < ab.size(); ++i)
      basis_prunes |= ab[i].zero_mask != 0 || ab[i].frozen_old_local != 0 || (pb.passes[i].flags & (PASS_INIT_BASIS | PASS_RELABEL)) != 0;
    expect(basis_prunes, "the basis-state plan of the case prunes somewhere");
    for (size_t i = 0; i < ad.size(); ++i) {
      const Pass& q = pd.passes[i];
      expect(!(q.flags & (PASS_INIT_BASIS | PASS_NO_ZERO_FILL | PASS_RELABEL)), "dense pass without basis / relabel flags");
      expect(ad[i].zero_mask == 0 && ad[i].n_free == ad[i].n_nonlocal, "dense pass launches every tile");
      expect(ad[i].frozen_old_local == 0 && q.frozen_new_local == 0, "dense pass clears and moves nothing");
      for (uint32_t w : q.round_words) expect(!adjoint || q.prog[w + 4] == 0u, "no dead wave in a dense adjoint round");
    }
    if (adjoint) expect(pd.dense_tail, "dense adjoint plan is a dense-tail plan");
  }
}

void check_gradient(const Model& m, int tile, std::mt19937_64& rng, const char* what) {
  std::string err;
  Plan plan;
  if (!build_plan(m, options(tile, true), &plan, &err)) { expect(false, std::string(what) + ": " + err); return; }
  std::uniform_real_distribution<float> P(-1.f, 1.f);
  std::normal_distribution<double> G;
  std::vector<double> params, up;
  for (int i = 0; i < m.n_params; ++i) params.push_back(double(P(rng)));
  for (int k = 0; k < m.n_ops; ++k) up.push_back(double(P(rng)));
  std::vector<cd> phi(size_t(1) << m.n);
  double norm = 0.0;
  for (cd& a : phi) { a = cd(G(rng), G(rng)); norm += std::norm(a); }
  for (cd& a : phi) a /= std::sqrt(norm);
  std::vector<cd> psi = run_circuit(m, params, phi);
  std::vector<cd> lam = emu::oracle_apply_observables(m, psi, up);
  const size_t n_eff = size_t(std::max(m.n, int(kMinTileBits)));  // padding qubits are the high index bits, |0>
  psi.resize(size_t(1) << n_eff, cd(0.0, 0.0));
  lam.resize(size_t(1) << n_eff, cd(0.0, 0.0));
  emu::Emulation e;
  emu::emu_prepare(m, plan, params, &e);
  expect(e.err.empty(), std::string(what) + " prepare: " + e.err);
  emu::AdjointResult ar;
  // (the bitstring the kernels are handed is all zeros; any other must give the same, nothing reads it)
  if (!emu::emu_adjoint(&e, 0u, psi, lam, &ar)) { expect(false, std::string(what) + " adjoint: " + e.err); return; }
  emu::AdjointResult other;
  expect(emu::emu_adjoint(&e, (1u << m.n) - 1u, psi, lam, &other) && other.grad == ar.grad, std::string(what) + ": independent of the bitstring");
  std::vector<double> want(size_t(m.n_params), 0.0);
  double scale = 0.0;
  for (int p = 0; p < m.n_params; ++p) {
    if (m.frozen(p)) continue;
    std::vector<double> hi = params, lo = params;
    hi[size_t(p)] += 1e-5;
    lo[size_t(p)] -= 1e-5;
    want[size_t(p)] = (objective(m, hi, phi, up) - objective(m, lo, phi, up)) / 2e-5;
    scale = std::max(scale, std::fabs(want[size_t(p)]));
  }
  double worst = 0.0;
  for (int p = 0; p < m.n_params; ++p) {
    if (m.frozen(p)) { expect(ar.grad[size_t(p)] == 0.0, std::string(what) + ": frozen parameter without gradient"); continue; }
    worst = std::max(worst, std::fabs(ar.grad[size_t(p)] - want[size_t(p)]));
  }
  std::printf("dense_start: %s: %zu passes, max gradient error %.3g (bar %.3g)\n", what, plan.passes.size(), worst, 1e-7 * scale);
  expect(scale > 1e-2 && worst <= 1e-7 * scale, std::string(what) + ": gradient against central differences");
}

}  // namespace

int main() {
  std::mt19937_64 rng(20261018);
  for (int sub = 0; sub < 2; ++sub) {
    const int n = 12, idle = sub ? n - 1 : 0, diagonal = sub ? 0 : n - 1;
    Model m = make_model(n, 3, idle, diagonal, rng);
    m.dense_input = true;
    check_structure(m, 10);
    check_gradient(m, 10, rng, sub ? "idle low bit" : "idle high bit");
    Model masked = m;  // the first layer frozen: the sweep stops at the first live gate, or runs to the start
    masked.param_frozen.assign(size_t(m.n_params), 0);
    int first_layer = 0;
    for (const Gate& g : m.gates) { if (g.kind == QHBM_GATE_CZPOW && g.q0 == (idle == 0 ? 1 : 0)) break; ++first_layer; }
    for (int i = 0; i < first_layer; ++i) masked.param_frozen[size_t(m.gates[size_t(i)].param_idx)] = 1;
    check_gradient(masked, 10, rng, "masked, stops early");
    masked.stop_at_first_live_gate = false;
    check_gradient(masked, 10, rng, "masked, whole sweep");
  }
  {  // padding: n < kMinTileBits, one tile
    Model m = make_model(6, 2, -1, -1, rng);
    m.dense_input = true;
    check_gradient(m, 0, rng, "n = 6 (padded)");
  }
  std::printf("dense_start: %d failures\n", g_failures);
  return g_failures ? 1 : 0;
}
