// moved_plan_check.cpp -- forward plans that move the low index bits, executed on the CPU against the dense oracle.
//
// Test infrastructure, not product (tests/test_forward_low_bits_emulated_cpu.py builds and runs it: host only, with
// AddressSanitizer + UBSan, nothing loaded into Python).  The plan emulator of tests/sanitize/ stores every tile in
// place and keeps covering the plans without the freedom; moved_forward.inc is its forward executor with the moving
// store, driven by the same PassArgs (fill_args).  Random hardware-efficient circuits and inverted ones (U, then U's
// inverse with parameters of its own) on 13..16 qubits, depth 2..6, a few basis states each: the final state (bar 1e-10
// per amplitude) and the values of an XXZ chain and a TFIM ring (bar 1e-10 max(1, sum |c_k|)), as plan_fuzz holds them.
// Every case must hold at least one pass that permutes, else it would test nothing.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../sanitize/plan_emulate.cpp"

namespace emu {
#include "moved_forward.inc"
}  // namespace emu

using namespace qhbm;
typedef emu::cd cd;

namespace {

int g_failures = 0;
void expect(bool ok, const std::string& what) {
  if (!ok) { std::printf("moved_plan_check: FAILED %s\n", what.c_str()); ++g_failures; }
}

Gate gate(int kind, int q0, int q1, int param, float scalar) {
  Gate g{};
  g.kind = kind;
  g.q0 = q0;
  g.q1 = q1;
  g.param_idx = param;
  g.scalar = scalar;
  g.offset = 0.f;
  g.global_shift = 0.f;
  return g;
}

// X**t, Z**t on every qubit, CZ**t on pairs (0,1),(2,3).. then (1,2),(3,4)..: one parameter per gate
void hea(Model* m, int layers) {
  for (int l = 0; l < layers; ++l) {
    for (int q = 0; q < m->n; ++q) {
      m->gates.push_back(gate(QHBM_GATE_XPOW, q, -1, m->n_params++, 1.f));
      m->gates.push_back(gate(QHBM_GATE_ZPOW, q, -1, m->n_params++, 1.f));
    }
    for (int q = 0; q + 1 < m->n; q += 2) m->gates.push_back(gate(QHBM_GATE_CZPOW, q, q + 1, m->n_params++, 1.f));
    for (int q = 1; q + 1 < m->n; q += 2) m->gates.push_back(gate(QHBM_GATE_CZPOW, q, q + 1, m->n_params++, 1.f));
  }
}

void observables(Model* m) {
  const int n = m->n;
  auto bit = [&](int q) { return 1u << (n - 1 - q); };
  m->n_ops = 2;
  for (int q = 0; q + 1 < n; ++q) {  // XXZ chain: XX + YY + 0.5 ZZ
    m->terms.push_back(PauliTerm{1.f, bit(q) | bit(q + 1), 0u, 0, 0});
    m->terms.push_back(PauliTerm{1.f, bit(q) | bit(q + 1), bit(q) | bit(q + 1), 2, 0});
    m->terms.push_back(PauliTerm{0.5f, 0u, bit(q) | bit(q + 1), 0, 0});
  }
  for (int q = 0; q < n; ++q) {  // TFIM ring: - X_q - Z_q Z_{q+1}
    m->terms.push_back(PauliTerm{-1.f, bit(q), 0u, 0, 1});
    m->terms.push_back(PauliTerm{-1.f, 0u, bit(q) | bit((q + 1) % n), 0, 1});
  }
}

void run_case(std::mt19937_64& rng, int n, int layers, bool inverted, int tile) {
  Model m;
  m.n = n;
  hea(&m, layers);
  if (inverted) {  // U, then U's inverse with parameters of its own
    const std::vector<Gate> fwd = m.gates;
    for (size_t i = fwd.size(); i-- > 0;) {
      Gate g = fwd[i];
      g.param_idx = m.n_params++;
      g.scalar = -g.scalar;
      m.gates.push_back(g);
    }
  }
  observables(&m);
  char name[96];
  std::snprintf(name, sizeof name, "n=%d layers=%d%s tile=%d", n, layers, inverted ? " inverted" : "", tile);
  Plan plain, moved;
  std::string err;
  PlanOptions o;
  o.tile_bits = tile;
  expect(build_plan(m, o, &plain, &err), std::string(name) + ": plain plan: " + err);
  o.move_low_bits = 2;
  expect(build_plan(m, o, &moved, &err), std::string(name) + ": moving plan: " + err);
  if (g_failures) return;
  for (const Pass& p : plain.passes) expect(!(p.flags & PASS_RELABEL), std::string(name) + ": the default plan moves");
  int flagged = 0;
  for (const Pass& p : moved.passes) flagged += (p.flags & PASS_RELABEL) != 0;
  expect(flagged >= 1, std::string(name) + ": no pass of the moving plan permutes");
  std::vector<double> params(size_t(m.n_params));
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  for (double& p : params) p = u(rng);
  std::vector<double> op_norm(size_t(m.n_ops), 0.0);
  for (const PauliTerm& t : m.terms) op_norm[size_t(t.op)] += std::fabs(double(t.coeff));
  emu::Emulation e;
  emu::emu_prepare(m, moved, params, &e);
  double worst_state = 0.0, worst_value = 0.0;
  for (int b = 0; b < 3; ++b) {
    const uint32_t basis = uint32_t(rng()) & ((1u << n) - 1u);
    const std::vector<cd> want = emu::oracle_state(m, params, basis);
    const std::vector<double> want_values = emu::oracle_values(m, want);
    for (int skip = 0; skip < 2; ++skip) {  // the values measured in the passes, and the measurement-free sweep
      emu::ForwardResult fr;
      int n_moving = 0;
      const bool ok = emu::emu_forward_moved(&e, basis, skip != 0, &fr, &n_moving);
      expect(ok && e.err.empty(), std::string(name) + ": emulation: " + e.err);
      if (!ok) return;
      expect(n_moving == flagged, std::string(name) + ": not every flagged pass stored through its table");
      expect(fr.have_final && fr.final_state.size() >= want.size(), std::string(name) + ": no final state");
      if (!fr.have_final) return;
      // (up to the global phase the X**t micro-ops leave to the export, as plan_fuzz compares)
      cd ip(0.0, 0.0);
      for (size_t i = 0; i < want.size(); ++i) ip += std::conj(want[i]) * fr.final_state[i];
      expect(std::abs(ip) > 0.5, std::string(name) + ": overlap with the oracle's state " + std::to_string(std::abs(ip)));
      const cd ph = std::abs(ip) > 0.5 ? ip / std::abs(ip) : cd(1.0, 0.0);
      for (size_t i = 0; i < want.size(); ++i) {
        const double d = std::abs(fr.final_state[i] - ph * want[i]);
        worst_state = std::max(worst_state, std::isfinite(d) ? d : 1.0);
      }
      if (!skip)
        for (int k = 0; k < m.n_ops; ++k) {
          const double d = std::fabs(fr.values[size_t(k)] - want_values[size_t(k)]) / std::max(1.0, op_norm[size_t(k)]);
          worst_value = std::max(worst_value, std::isfinite(d) ? d : 1.0);
        }
    }
  }
  expect(worst_state <= 1e-10, std::string(name) + ": final state off by " + std::to_string(worst_state / 1e-10) + " of its bar 1e-10");
  expect(worst_value <= 1e-10, std::string(name) + ": values off by " + std::to_string(worst_value / 1e-10) + " of their bar");
  std::printf("moved_plan_check: %s: %zu passes (%d moving), state error %.3g, value error %.3g of its bar\n", name,
              moved.passes.size(), flagged, worst_state, worst_value / 1e-10);
}

}  // namespace

int main() {
  std::mt19937_64 rng(20);
  // (n <= 14 is a single tile unless the tile size is given; 15 and 16 qubits take the scheduler's own 2^12)
  const int cases[][4] = {{13, 2, 0, 10}, {13, 4, 1, 10}, {14, 3, 0, 10}, {14, 6, 0, 11}, {15, 5, 0, 0}, {15, 3, 1, 0},
                          {16, 6, 0, 0}, {16, 2, 1, 0}, {16, 4, 0, 12}};
  for (const auto& c : cases) run_case(rng, c[0], c[1], c[2] != 0, c[3]);
  std::printf("moved_plan_check: %d failures\n", g_failures);
  return g_failures ? 1 : 0;
}
