// gram_vjp_plan_check -- the launch plan of the weighted Gram matrix's VJP (csrc/gram_vjp_plan.h) on the CPU.
//
// For every register of n <= 13 qubits and M in {1, 3, 4, 5, 8, 15, 16, 17, 33, 64, 1024} the kernels of gram_vjp.hip are
// walked workgroup by workgroup and thread by thread through the header's own helpers:
//   1. every 16-byte word of every output state and every table_grad entry is written exactly once;
//   2. every read of the states lies inside [M, 2^n], every read of the table inside [2^n], every read of H inside [M, M];
//   3. matrix kernel (M >= 9): the planes kernel writes every entry of both H planes once, inside scratch_bytes; a stage's
//      loads store every element of the LDS tiles exactly once inside the planes' pitch and read only written plane
//      entries; the fragments the waves read were all stored; the accumulator map stores every entry of the result planes
//      that the epilogue reads, and the epilogue reads inside them;
//   4. at the interface's limits (31 qubits, 1024 states) the grid stays inside what a launch accepts.
// Its own main; built with -fsanitize=address,undefined by its makefile.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gram_vjp_plan.h"

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

static long vector_plans = 0, matrix_plans = 0, padded_tiles = 0, ragged_rows = 0;

static void check_vector(const GvPlan& p, std::vector<uint8_t>& out_words, std::vector<uint8_t>& grads) {
  const uint32_t V = gv_vec_words(p.M);
  CHECK((kGvSliceWords / kGvThreads) % V == 0, "%u words at a time", V);
  CHECK(p.scratch_bytes == kGvMinScratch && p.grid_y == 1 && p.grid_x == p.slices, "vector plan of M %u", p.M);
  for (uint32_t s = 0; s < p.grid_x; ++s)
    for (uint32_t tid = 0; tid < kGvThreads; ++tid)
      for (uint32_t k0 = 0; k0 < kGvSliceWords / kGvThreads; k0 += V)
        for (uint32_t v = 0; v < V; ++v) {
          const uint64_t w = gv_vec_word(s, k0 + v, tid);
          if (w >= p.words) continue;  // (no load, no store)
          for (uint32_t i = 0; i < p.M; ++i) {
            const uint64_t at = i * p.words + w;  // (states as words)
            CHECK(at < p.M * p.words, "state word %llu", (unsigned long long)at);
            if (at < p.M * p.words) ++out_words[at];  // (out[j] at the same place)
          }
          CHECK(2 * w + 1 < p.amps, "table word %llu", (unsigned long long)w);
          if (2 * w + 1 < p.amps) {
            ++grads[2 * w];
            ++grads[2 * w + 1];
          }
        }
  ++vector_plans;
}

static void check_matrix(const GvPlan& p, std::vector<uint8_t>& out_words, std::vector<uint8_t>& grads) {
  const uint32_t TM = p.tm, TK = kGvStage, PA = gv_lds_pitch(TM), PB = gv_lds_pitch(kGvTileCols), PC = kGvResultPitch;
  const uint32_t NB = TK * kGvTileCols / kGvThreads, NA = TM * TK / kGvThreads, NS = TM * (kGvTileCols / 2) / kGvThreads;
  CHECK(p.m16 % 16 == 0 && p.m16 >= p.M && p.m16 < p.M + 16 && TM % 16 == 0 && TM >= 16 && TM <= kGvMaxTileRows, "rows of M %u", p.M);
  CHECK(p.P == p.row_tiles * TM && p.P >= p.m16 && p.P < p.m16 + TM, "pitch %u of M %u", p.P, p.M);
  CHECK(NB * kGvThreads == TK * kGvTileCols && NA * kGvThreads == TM * TK && NS * kGvThreads == TM * (kGvTileCols / 2), "loads of tm %u", TM);
  CHECK(uint64_t(p.col_tiles) * kGvTileCols >= p.amps && uint64_t(p.col_tiles - 1) * kGvTileCols < p.amps, "column tiles");
  CHECK(uint64_t(p.grid_x) * p.grid_y >= p.col_tiles && p.grid_x <= kGvGridX, "grid of %u tiles", p.col_tiles);
  // the planes kernel
  CHECK(p.plane_floats == size_t(2) * p.P * p.P && p.scratch_bytes == p.plane_floats * sizeof(float), "scratch of M %u", p.M);
  std::vector<uint8_t> planes(p.scratch_bytes / sizeof(float), 0);
  const uint32_t entries = p.P * p.P, groups = (entries + kGvThreads - 1) / kGvThreads;
  for (uint32_t e = 0; e < groups * kGvThreads; ++e) {
    if (e >= entries) continue;  // (the kernel returns)
    uint32_t i, j;
    gv_plane_element(p.P, e, &i, &j);
    CHECK(i < p.P && j < p.P, "plane entry %u", e);
    if (i < p.M && j < p.M) CHECK(size_t(i) * p.M + j < size_t(p.M) * p.M, "H[%u, %u]", i, j);
    const size_t re = e, im = size_t(p.P) * p.P + e;
    CHECK(im < planes.size(), "plane entry %zu of %zu", im, planes.size());
    if (im < planes.size()) {
      ++planes[re];
      ++planes[im];
    }
  }
  for (size_t i = 0; i < planes.size(); ++i) CHECK(planes[i] == 1, "plane float %zu written %d times", i, int(planes[i]));

  for (uint32_t by = 0; by < p.grid_y; ++by)
    for (uint32_t bx = 0; bx < p.grid_x; ++bx) {
      const uint32_t tile = by * kGvGridX + bx;
      if (tile >= p.col_tiles) continue;  // (the kernel returns)
      const uint64_t col0 = uint64_t(tile) * kGvTileCols;
      if (col0 + kGvTileCols > p.amps) ++padded_tiles;
      for (uint32_t rt = 0; rt < p.row_tiles; ++rt) {
        const uint32_t row0 = rt * TM, strips = gv_live_strips(p.m16, TM, rt);
        CHECK(strips >= 1 && strips <= TM / 16 && row0 + 16 * strips >= (p.M < row0 + TM ? p.M : row0 + TM), "strips of row tile %u", rt);
        for (uint32_t i0 = 0; i0 < p.m16; i0 += TK) {
          std::vector<uint8_t> lds_a(size_t(TK) * PA, 0), lds_b(size_t(TK) * PB, 0);
          for (uint32_t tid = 0; tid < kGvThreads; ++tid) {
            for (uint32_t i = 0; i < NB; ++i) {
              uint32_t kk, c;
              gv_panel_element(tid, i, &kk, &c);
              CHECK(kk < TK && c < kGvTileCols, "panel element of thread %u pass %u", tid, i);
              if (kk >= TK || c >= kGvTileCols) continue;
              ++lds_b[kk * PB + c];
              if (col0 + c >= p.amps || i0 + kk >= p.M) continue;  // (a zero goes to LDS)
              CHECK(uint64_t(i0 + kk) * p.amps + col0 + c < p.M * p.amps, "panel read");
            }
            for (uint32_t i = 0; i < NA; ++i) {
              uint32_t kk, r;
              gv_operator_element(TM, tid, i, &kk, &r);
              CHECK(kk < TK && r < TM, "operator element of thread %u pass %u", tid, i);
              if (kk >= TK || r >= TM) continue;
              ++lds_a[kk * PA + r];
              const size_t at = size_t(i0 + kk) * p.P + row0 + r;
              CHECK(at < size_t(p.P) * p.P && planes[at] == 1, "plane read %zu", at);
            }
          }
          for (uint32_t wave = 0; wave < 4; ++wave)
            for (uint32_t lane = 0; lane < 64; ++lane)
              for (uint32_t q = 0; q < TK / 4; ++q) {
                const uint32_t kq = 4 * q + (lane >> 4);
                CHECK(lds_b[kq * PB + 16 * wave + (lane & 15)] == 1, "B fragment of wave %u lane %u", wave, lane);
                for (uint32_t s = 0; s < strips; ++s) CHECK(lds_a[kq * PA + 16 * s + (lane & 15)] == 1, "A fragment of strip %u lane %u", s, lane);
              }
        }
        std::vector<uint8_t> result(size_t(TM) * PC, 0);
        for (uint32_t wave = 0; wave < 4; ++wave)
          for (uint32_t lane = 0; lane < 64; ++lane)
            for (uint32_t s = 0; s < TM / 16; ++s)
              for (uint32_t g = 0; g < 4; ++g) {
                uint32_t r, c;
                gv_result_element(wave, lane, s, g, &r, &c);
                CHECK(r < TM && c < kGvTileCols, "result element (%u, %u)", r, c);
                if (r < TM && c < kGvTileCols) ++result[r * PC + c];
              }
        // the epilogue: words of out rows ...
        for (uint32_t tid = 0; tid < kGvThreads; ++tid)
          for (uint32_t q = 0; q < NS; ++q) {
            uint32_t r, w;
            gv_store_element(tid, q, &r, &w);
            CHECK(r < TM && w < kGvTileCols / 2, "store element of thread %u pass %u", tid, q);
            if (r >= TM || w >= kGvTileCols / 2) continue;
            const uint64_t x = col0 + 2 * w;
            if (x >= p.amps || row0 + r >= p.M) {
              if (row0 + r >= p.M) ++ragged_rows;
              continue;
            }
            CHECK(x + 1 < p.amps, "table word at %llu", (unsigned long long)x);
            CHECK(result[r * PC + 2 * w] == 1 && result[r * PC + 2 * w + 1] == 1, "result word (%u, %u)", r, w);
            const uint64_t at = (uint64_t(row0 + r) * p.amps + x) / 2;
            CHECK(at < p.M * p.words, "out word %llu", (unsigned long long)at);
            if (at < p.M * p.words) ++out_words[at];
          }
        // ... and wave 0, a lane per column, over the tile's rows
        for (uint32_t tid = 0; tid < kGvTileCols; ++tid) {
          const uint64_t x = col0 + tid;
          if (x >= p.amps) continue;
          const uint32_t rows = p.M - row0 < TM ? p.M - row0 : TM;
          for (uint32_t r = 0; r < rows; ++r) {
            CHECK(result[r * PC + tid] == 1, "result (%u, %u)", r, tid);
            CHECK(uint64_t(row0 + r) * p.amps + x < p.M * p.amps, "a_j read");
          }
          if (rt + 1 == p.row_tiles) ++grads[x];
        }
      }
    }
  ++matrix_plans;
}

static void check_shape(int n, int M) {
  const GvPlan p = gv_plan(n, M);
  CHECK(p.amps == (uint64_t(1) << n) && p.words * 2 == p.amps && p.matrix == (uint32_t(M) > kGvVectorMaxStates), "plan of n %d M %d", n, M);
  std::vector<uint8_t> out_words(size_t(M) * p.words, 0), grads(p.amps, 0);
  if (p.matrix)
    check_matrix(p, out_words, grads);
  else
    check_vector(p, out_words, grads);
  for (size_t i = 0; i < out_words.size(); ++i) CHECK(out_words[i] == 1, "n %d M %d: out word %zu written %d times", n, M, i, int(out_words[i]));
  for (size_t i = 0; i < grads.size(); ++i) CHECK(grads[i] == 1, "n %d M %d: table_grad %zu written %d times", n, M, i, int(grads[i]));
}

int main() {
  long shapes = 0;
  for (int n = 1; n <= 13; ++n)
    for (int M : {1, 3, 4, 5, 8, 15, 16, 17, 33, 64, 1024}) {
      check_shape(n, M);
      ++shapes;
    }
  for (int M = 1; M <= 130; ++M) check_shape(7, M);  // every ragged M around the tile sizes
  CHECK(vector_plans > 60 && matrix_plans > 100 && padded_tiles > 20 && ragged_rows > 1000,
        "%ld vector plans, %ld matrix plans, %ld padded tiles, %ld ragged rows", vector_plans, matrix_plans, padded_tiles, ragged_rows);
  // 4
  for (int M : {1, 8, 9, 1024}) {
    const GvPlan p = gv_plan(31, M);
    CHECK(p.grid_x >= 1 && p.grid_y >= 1 && p.grid_y <= 65535u && uint64_t(p.grid_x) * kGvThreads < (uint64_t(1) << 32), "grid at 31 qubits, M %d", M);
    if (p.matrix)
      CHECK(uint64_t(p.grid_x) * p.grid_y >= p.col_tiles && p.col_tiles == (1u << 25), "column tiles at 31 qubits");
    else
      CHECK(p.slices == (1u << 20) && gv_vec_word(p.slices - 1, 3, kGvThreads - 1) == p.words - 1, "slices at 31 qubits");
    CHECK(p.scratch_bytes <= size_t(8) * 1024 * 1024 && p.scratch_bytes >= kGvMinScratch, "scratch at M %d", M);
  }
  std::printf("gram_vjp_plan_check: %ld shapes, %ld vector plans, %ld matrix plans, %ld padded tiles, %ld ragged rows\n", shapes,
              vector_plans, matrix_plans, padded_tiles, ragged_rows);
  std::printf("gram_vjp_plan_check: %ld failures\n", failures);
  return failures ? 1 : 0;
}
