// subsystem_plan_check -- the launch plan of a dense operator on k qubits (csrc/subsystem_plan.h) on the CPU.
//
// For every register of n <= 12 qubits, every keep mask with 1 <= k <= min(n, 10) and one or three states, the kernels of
// subsystem_apply.hip are walked workgroup by workgroup and thread by thread through the header's own helpers:
//   1. every amplitude of every state is written exactly once, at the index rdm_amp_index gives for its (row, environment
//      value), and every read of the states stays inside the state it belongs to;
//   2. vector kernel (k <= 3): the OR of the deposits of a thread's low bits and the slice's high bits is the deposit of
//      their sum;
//   3. matrix kernel (k >= 4): a stage's loads store every element of the two LDS tiles exactly once inside the planes'
//      pitch, read only entries of the transposed operator, and the fragments the waves read were all stored; the
//      accumulator map covers the tile's rows and columns exactly once;
//   4. every partial of the dot products is written once, inside scratch_bytes and behind the operator planes, and the
//      finish kernel reads only written partials;
//   5. at the interface's limits (31 qubits, 65536 states) the grid stays inside what a launch accepts.
// Its own main; built with -fsanitize=address,undefined by its makefile.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "subsystem_plan.h"

using namespace qhbm;

static long failures = 0;
#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      if (++failures <= 20) {              \
        std::printf("FAIL %s: ", #cond);   \
        std::printf(__VA_ARGS__);          \
        std::printf("\n");                 \
      }                                    \
    }                                      \
  } while (0)

static long vector_plans = 0, matrix_plans = 0, padded_tiles = 0;

static void check_mask(int n, uint64_t keep_mask, int M) {
  const SubPlan p = sub_plan(n, keep_mask, M);
  const uint32_t D = 1u << p.k, E = 1u << (p.n - p.k), N = 1u << n;
  CHECK(p.env_values == E && p.matrix == (p.k > uint32_t(kSubVectorMaxKeep)), "plan of n %d mask %llx", n,
        (unsigned long long)keep_mask);
  CHECK(uint64_t(p.grid_y) * p.grid_z >= uint64_t(M) && p.grid_y <= kSubGridY, "grid of %d states", M);
  std::vector<uint8_t> written(size_t(M) * N, 0);
  for (uint32_t z = 0; z < p.grid_z; ++z)
    for (uint32_t y = 0; y < p.grid_y; ++y) {
      const uint32_t m = z * kSubGridY + y;
      if (m >= uint32_t(M)) continue;  // (the kernels return)
      for (uint32_t t = 0; t < p.slices; ++t) {
        if (!p.matrix) {
          for (uint32_t tid = 0; tid < kSubThreads; ++tid)
            for (uint32_t j = 0; j < kSubVecValues; ++j) {
              const uint32_t high = sub_vec_high(t, j);
              if (high + tid >= E) continue;
              const uint32_t idx = rdm_deposit(high, p.masks.env) | rdm_deposit(tid, p.masks.env);
              CHECK(idx == rdm_deposit(high + tid, p.masks.env), "deposit of %u + %u", high, tid);
              for (uint32_t r = 0; r < D; ++r) {
                const uint32_t at = idx | rdm_deposit(r, p.masks.keep);
                CHECK(at < N && at == rdm_amp_index(p.masks, r, high + tid), "amplitude (%u, %u)", r, high + tid);
                if (at < N) ++written[size_t(m) * N + at];
              }
            }
          continue;
        }
        uint32_t row0, col0;
        sub_tile_of(p.row_tiles, p.tm, t, &row0, &col0);
        CHECK(row0 + p.tm <= D && col0 < E, "tile %u at (%u, %u)", t, row0, col0);
        if (col0 + kSubTileCols > E) ++padded_tiles;
        const uint32_t PA = sub_lds_pitch(p.tm), PB = sub_lds_pitch(kSubTileCols);
        const uint32_t NB = p.tk * kSubTileCols / kSubThreads, NA = p.tm * p.tk / kSubThreads;
        CHECK(NB * kSubThreads == p.tk * kSubTileCols && NA * kSubThreads == p.tm * p.tk && NA >= 1, "stage loads of k %u", p.k);
        for (uint32_t k0 = 0; k0 < D; k0 += p.tk) {
          std::vector<uint8_t> lds_a(size_t(p.tk) * PA, 0), lds_b(size_t(p.tk) * PB, 0);
          for (uint32_t tid = 0; tid < kSubThreads; ++tid) {
            for (uint32_t i = 0; i < NB; ++i) {
              uint32_t kk, c;
              sub_panel_element(tid, i, &kk, &c);
              CHECK(kk < p.tk && c < kSubTileCols && k0 + kk < D, "panel element of thread %u pass %u", tid, i);
              if (kk >= p.tk || c >= kSubTileCols) continue;
              ++lds_b[kk * PB + c];
              if (col0 + c >= E) continue;  // (a zero goes to LDS)
              const uint32_t at = rdm_deposit(k0 + kk, p.masks.keep) | rdm_deposit(col0 + c, p.masks.env);
              CHECK(at < N && at == rdm_amp_index(p.masks, k0 + kk, col0 + c), "gather of (%u, %u)", k0 + kk, col0 + c);
            }
            for (uint32_t i = 0; i < NA; ++i) {
              uint32_t kk, r;
              sub_operator_element(p.tm, tid, i, &kk, &r);
              CHECK(kk < p.tk && r < p.tm, "operator element of thread %u pass %u", tid, i);
              if (kk >= p.tk || r >= p.tm) continue;
              ++lds_a[kk * PA + r];
              const uint64_t at = (uint64_t(k0 + kk) << p.k) + row0 + r;
              CHECK(at < (uint64_t(1) << (2 * p.k)) && 2 * ((uint64_t(1) << (2 * p.k))) == p.operator_floats, "operator plane entry");
            }
          }
          for (uint32_t wave = 0; wave < 4; ++wave)
            for (uint32_t lane = 0; lane < 64; ++lane)
              for (uint32_t q = 0; q < p.tk / 4; ++q) {
                const uint32_t kq = 4 * q + (lane >> 4);
                CHECK(lds_b[kq * PB + 16 * wave + (lane & 15)] == 1, "B fragment of wave %u lane %u", wave, lane);
                for (uint32_t s = 0; s < p.tm / 16; ++s)
                  CHECK(lds_a[kq * PA + 16 * s + (lane & 15)] == 1, "A fragment of strip %u lane %u", s, lane);
              }
        }
        std::vector<uint8_t> tile(size_t(p.tm) * kSubTileCols, 0);
        for (uint32_t wave = 0; wave < 4; ++wave)
          for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t s = 0; s < p.tm / 16; ++s)
              for (uint32_t g = 0; g < 4; ++g) {
                uint32_t r, c;
                sub_result_element(wave, lane, s, g, &r, &c);
                CHECK(r < p.tm && c < kSubTileCols, "result element (%u, %u)", r, c);
                if (r >= p.tm || c >= kSubTileCols) continue;
                ++tile[r * kSubTileCols + c];
                if (col0 + c >= E) continue;
                const uint32_t at = rdm_deposit(row0 + r, p.masks.keep) | rdm_deposit(col0 + c, p.masks.env);
                CHECK(at < N && at == rdm_amp_index(p.masks, row0 + r, col0 + c), "result (%u, %u)", row0 + r, col0 + c);
                if (at < N) ++written[size_t(m) * N + at];
              }
        for (size_t i = 0; i < tile.size(); ++i) CHECK(tile[i] == 1, "tile entry %zu held %d times", i, int(tile[i]));
      }
    }
  for (size_t i = 0; i < written.size(); ++i) CHECK(written[i] == 1, "n %d mask %llx: amplitude %zu written %d times", n,
                                                    (unsigned long long)keep_mask, i, int(written[i]));
  // 4
  CHECK(p.parts_offset % sizeof(double) == 0 && p.parts_offset == p.operator_floats * sizeof(float), "partials at %zu", p.parts_offset);
  CHECK(p.scratch_bytes >= p.parts_offset && (p.scratch_bytes - p.parts_offset) % sizeof(double) == 0, "scratch");
  const size_t doubles = (p.scratch_bytes - p.parts_offset) / sizeof(double);
  std::vector<uint8_t> parts(doubles, 0);
  for (uint32_t m = 0; m < uint32_t(M); ++m)
    for (uint32_t t = 0; t < p.slices; ++t)
      for (uint32_t comp = 0; comp < 2; ++comp) {
        const size_t at = (size_t(m) * 2 + comp) * p.slices + t;
        CHECK(at < doubles, "partial %zu of %zu", at, doubles);
        if (at < doubles) ++parts[at];
      }
  for (size_t i = 0; i < doubles; ++i) CHECK(parts[i] == 1, "partial %zu written %d times", i, int(parts[i]));  // (= the finish's reads)
  ++(p.matrix ? matrix_plans : vector_plans);
}

int main() {
  long masks = 0;
  for (int n = 1; n <= 12; ++n)
    for (uint64_t mask = 1; mask < (uint64_t(1) << n); ++mask) {
      const int k = rdm_popcount(mask);
      if (k > 10) {
        CHECK(rdm_check(n, mask) == 3, "k = %d accepted", k);
        continue;
      }
      ++masks;
      check_mask(n, mask, 1);
      if ((mask % 7) == 0) check_mask(n, mask, 3);
    }
  CHECK(vector_plans > 500 && matrix_plans > 3000 && padded_tiles > 1000, "%ld vector plans, %ld matrix plans, %ld padded tiles",
        vector_plans, matrix_plans, padded_tiles);
  // 5
  for (uint64_t mask : {uint64_t(1), uint64_t(1) << 30, uint64_t(0x3ff), uint64_t(0x3ff) << 21, uint64_t(0xf) << 13}) {
    const SubPlan p = sub_plan(31, mask, kRdmMaxStates);
    CHECK(rdm_check(31, mask) == 0, "31 qubits");
    CHECK(p.slices >= 1 && p.slices <= 0x7fffffffu && p.grid_y <= 65535u && p.grid_z <= 65535u, "grid at 31 qubits");
    CHECK(uint64_t(p.grid_y) * p.grid_z >= uint64_t(kRdmMaxStates), "states at 31 qubits");
    CHECK(sub_vec_high(p.slices - 1, kSubVecValues - 1) < (uint64_t(1) << 31), "environment values at 31 qubits");
    CHECK(p.scratch_bytes == p.parts_offset + size_t(kRdmMaxStates) * 2 * p.slices * sizeof(double), "scratch at 31 qubits");
  }
  std::printf("subsystem_plan_check: %ld masks, %ld vector plans, %ld matrix plans, %ld padded tiles\n", masks, vector_plans,
              matrix_plans, padded_tiles);
  std::printf("subsystem_plan_check: %ld failures\n", failures);
  return failures ? 1 : 0;
}
