// cross_gram_vjp_plan_check -- the launch plan of the cross-Gram matrix's VJP (csrc/cross_gram_vjp_plan.h) on the CPU.
//
// For every register of n <= 13 qubits and (M, K) in {1, 3, 8, 9, 16, 17, 33, 65, 1024}^2, and for every M, K <= 40 at n = 7,
// both side sweeps of cross_gram_vjp.hip (ket side: R = M source rows, S = K output rows, with table_grad; bra side: R = K,
// S = M) are walked workgroup by workgroup and thread by thread through the header's own helpers:
//   1. every 16-byte word of every output row and (ket side) every table_grad entry is written exactly once;
//   2. every read of the source rows lies inside [R, 2^n], of the partner rows inside [S, 2^n], of the table inside [2^n], of
//      the cotangent inside [M, K];
//   3. vector kernel (R <= 8): the k0 loop and the chunk loop are walked as the kernel runs them, a chunk restaged where the
//      kernel restages it (every k0 with several chunks, once with one); a staging stores each entry once inside the LDS
//      array, and every W entry an output row reads was last stored by that row's own chunk;
//   4. matrix kernel (R >= 9): the planes kernel writes every entry of both W planes of the side once, inside its part of
//      scratch_bytes, and the two sides' parts do not meet; a stage's loads store every element of the LDS tiles exactly
//      once inside the planes' pitch and read only written plane entries; the fragments the waves read were all stored; the
//      accumulator map stores every entry of the result planes that the epilogue reads, and the epilogue reads inside them
//      (the LDS walk of a stage does not depend on the column tile but for the columns beyond 2^n, so it is made for the
//      first and the last column tile; the stores and the table_grad entries are counted for every tile);
//   5. at the interface's limits (31 qubits, 1024 x 1024 states) the grids stay inside what a launch accepts.
// Its own main; built with -fsanitize=address,undefined by its makefile.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cross_gram_vjp_plan.h"

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

static long vector_sweeps = 0, matrix_sweeps = 0, padded_tiles = 0, ragged_rows = 0, chunked_sweeps = 0;

// the cotangent entry that W[r, s] of a side reads, inside [M, K]
static void check_cotangent(const CgvSide& p, bool bra_side, uint32_t r, uint32_t s) {
  const uint32_t M = bra_side ? p.S : p.R, K = bra_side ? p.R : p.S;
  const size_t at = cgv_cotangent_index(bra_side, p.R, p.S, r, s);
  const uint32_t i = bra_side ? s : r, j = bra_side ? r : s;
  CHECK(at == size_t(i) * K + j && at < size_t(M) * K, "cotangent entry (%u, %u) of R %u S %u", r, s, p.R, p.S);
}

static void check_vector(const CgvSide& p, bool bra_side, bool sums, std::vector<uint8_t>& out_words, std::vector<uint8_t>& grads) {
  const uint32_t V = gv_vec_words(p.R);
  CHECK((kGvSliceWords / kGvThreads) % V == 0, "%u words at a time", V);
  CHECK(p.plane_floats == 0 && p.grid_y == 1 && p.grid_x == p.slices && p.chunks == (p.S + kCgvChunk - 1) / kCgvChunk,
        "vector plan of R %u S %u", p.R, p.S);
  if (p.chunks > 1) ++chunked_sweeps;
  // 3: the LDS array as the kernel's loops leave it (the same for every workgroup): k0 outside, the chunks inside, a chunk
  // restaged where the kernel restages it -- `chunks > 1 || k0 == 0` -- between its two barriers; every entry carries the
  // chunk that stored it last, and a read must find its own chunk there
  uint32_t covered = 0;
  std::vector<int32_t> lds(size_t(p.R) * kCgvChunk, -1);
  for (uint32_t k0 = 0; k0 < kGvSliceWords / kGvThreads; k0 += V)
    for (uint32_t chunk = 0; chunk < p.chunks; ++chunk) {
      const uint32_t live = cgv_chunk_rows(p.S, chunk), s0 = chunk * kCgvChunk;
      CHECK(live >= 1 && live <= kCgvChunk && s0 + live <= p.S, "chunk %u of S %u", chunk, p.S);
      if (p.chunks > 1 || k0 == 0) {
        std::vector<uint8_t> stores(lds.size(), 0);
        for (uint32_t tid = 0; tid < kGvThreads; ++tid)
          for (uint32_t e = tid; e < p.R * live; e += kGvThreads) {
            const uint32_t r = e / live, sl = e - r * live;
            CHECK(r < p.R && sl < live, "chunk element %u", e);
            check_cotangent(p, bra_side, r, s0 + sl);
            const size_t at = size_t(r) * kCgvChunk + sl;
            CHECK(at < lds.size(), "LDS entry %zu", at);
            if (at < lds.size()) {
              lds[at] = int32_t(chunk);
              ++stores[at];
            }
          }
        for (size_t at = 0; at < stores.size(); ++at) CHECK(stores[at] <= 1, "LDS entry %zu stored %d times in one staging", at, int(stores[at]));
      }
      for (uint32_t sl = 0; sl < live; ++sl)
        for (uint32_t r = 0; r < p.R; ++r)
          CHECK(lds[size_t(r) * kCgvChunk + sl] == int32_t(chunk), "W[%u, %u] read from LDS at k0 %u", r, s0 + sl, k0);
      if (k0 == 0) covered += live;
    }
  CHECK(covered == p.S, "chunks cover %u of %u output rows", covered, p.S);
  for (uint32_t s = 0; s < p.grid_x; ++s)
    for (uint32_t tid = 0; tid < kGvThreads; ++tid)
      for (uint32_t k0 = 0; k0 < kGvSliceWords / kGvThreads; k0 += V)
        for (uint32_t v = 0; v < V; ++v) {
          const uint64_t w = gv_vec_word(s, k0 + v, tid);
          if (w >= p.words) continue;  // (no load, no store)
          CHECK(uint64_t(p.R - 1) * p.words + w < p.R * p.words, "source word %llu", (unsigned long long)w);
          for (uint32_t j = 0; j < p.S; ++j) {
            const uint64_t at = j * p.words + w;  // (out[j] and partner[j] as words)
            CHECK(at < p.S * p.words, "out word %llu", (unsigned long long)at);
            if (at < p.S * p.words) ++out_words[at];
          }
          CHECK(2 * w + 1 < p.amps, "table word %llu", (unsigned long long)w);
          if (sums && 2 * w + 1 < p.amps) {
            ++grads[2 * w];
            ++grads[2 * w + 1];
          }
        }
  ++vector_sweeps;
}

static void check_matrix(const CgvSide& p, bool bra_side, bool sums, size_t plane_offset, size_t scratch_floats,
                         std::vector<uint8_t>& scratch, std::vector<uint8_t>& out_words, std::vector<uint8_t>& grads) {
  const uint32_t TM = p.tm, TK = kGvStage, PA = gv_lds_pitch(TM), PB = gv_lds_pitch(kGvTileCols), PC = kGvResultPitch;
  const uint32_t NB = TK * kGvTileCols / kGvThreads, NA = TM * TK / kGvThreads, NS = TM * (kGvTileCols / 2) / kGvThreads;
  CHECK(p.r16 % 16 == 0 && p.r16 >= p.R && p.r16 < p.R + 16, "stages of R %u", p.R);
  CHECK(p.s16 % 16 == 0 && p.s16 >= p.S && p.s16 < p.S + 16 && TM % 16 == 0 && TM >= 16 && TM <= kGvMaxTileRows, "rows of S %u", p.S);
  CHECK(p.P == p.row_tiles * TM && p.P >= p.s16 && p.P < p.s16 + TM, "pitch %u of S %u", p.P, p.S);
  CHECK(NB * kGvThreads == TK * kGvTileCols && NA * kGvThreads == TM * TK && NS * kGvThreads == TM * (kGvTileCols / 2), "loads of tm %u", TM);
  CHECK(uint64_t(p.col_tiles) * kGvTileCols >= p.amps && uint64_t(p.col_tiles - 1) * kGvTileCols < p.amps, "column tiles");
  CHECK(uint64_t(p.grid_x) * p.grid_y >= p.col_tiles && p.grid_x <= kGvGridX, "grid of %u tiles", p.col_tiles);
  // the planes kernel, into the side's part of the scratch
  CHECK(p.plane_floats == size_t(2) * p.r16 * p.P && plane_offset + p.plane_floats <= scratch_floats, "planes of R %u S %u", p.R, p.S);
  const size_t plane = size_t(p.r16) * p.P;
  const uint32_t entries = p.r16 * p.P, groups = (entries + kGvThreads - 1) / kGvThreads;
  for (uint32_t e = 0; e < groups * kGvThreads; ++e) {
    if (e >= entries) continue;  // (the kernel returns)
    uint32_t r, s;
    cgv_plane_element(p.P, e, &r, &s);
    CHECK(r < p.r16 && s < p.P, "plane entry %u", e);
    if (r < p.R && s < p.S) check_cotangent(p, bra_side, r, s);
    const size_t re = plane_offset + e, im = plane_offset + plane + e;
    CHECK(im < scratch.size(), "plane entry %zu of %zu", im, scratch.size());
    if (im < scratch.size()) {
      ++scratch[re];
      ++scratch[im];
    }
  }
  for (size_t i = 0; i < p.plane_floats; ++i)
    CHECK(scratch[plane_offset + i] == 1, "plane float %zu written %d times", i, int(scratch[plane_offset + i]));

  for (uint32_t by = 0; by < p.grid_y; ++by)
    for (uint32_t bx = 0; bx < p.grid_x; ++bx) {
      const uint32_t tile = by * kGvGridX + bx;
      if (tile >= p.col_tiles) continue;  // (the kernel returns)
      const uint64_t col0 = uint64_t(tile) * kGvTileCols;
      if (col0 + kGvTileCols > p.amps) ++padded_tiles;
      const bool walk_lds = tile == 0 || tile + 1 == p.col_tiles;
      for (uint32_t rt = 0; rt < p.row_tiles; ++rt) {
        const uint32_t row0 = rt * TM, strips = gv_live_strips(p.s16, TM, rt);
        CHECK(strips >= 1 && strips <= TM / 16 && row0 + 16 * strips >= (p.S < row0 + TM ? p.S : row0 + TM), "strips of row tile %u", rt);
        for (uint32_t i0 = 0; walk_lds && i0 < p.r16; i0 += TK) {
          std::vector<uint8_t> lds_a(size_t(TK) * PA, 0), lds_b(size_t(TK) * PB, 0);
          for (uint32_t tid = 0; tid < kGvThreads; ++tid) {
            for (uint32_t i = 0; i < NB; ++i) {
              uint32_t kk, c;
              gv_panel_element(tid, i, &kk, &c);
              CHECK(kk < TK && c < kGvTileCols, "panel element of thread %u pass %u", tid, i);
              if (kk >= TK || c >= kGvTileCols) continue;
              ++lds_b[kk * PB + c];
              if (col0 + c >= p.amps || i0 + kk >= p.R) continue;  // (a zero goes to LDS)
              CHECK(uint64_t(i0 + kk) * p.amps + col0 + c < p.R * p.amps, "panel read");
            }
            for (uint32_t i = 0; i < NA; ++i) {
              uint32_t kk, r;
              gv_operator_element(TM, tid, i, &kk, &r);
              CHECK(kk < TK && r < TM, "operator element of thread %u pass %u", tid, i);
              if (kk >= TK || r >= TM) continue;
              ++lds_a[kk * PA + r];
              const size_t at = size_t(i0 + kk) * p.P + row0 + r;
              CHECK(at < plane && scratch[plane_offset + at] == 1 && scratch[plane_offset + plane + at] == 1, "plane read %zu", at);
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
            if (x >= p.amps || row0 + r >= p.S) {
              if (row0 + r >= p.S) ++ragged_rows;
              continue;
            }
            CHECK(x + 1 < p.amps, "table word at %llu", (unsigned long long)x);
            CHECK(result[r * PC + 2 * w] == 1 && result[r * PC + 2 * w + 1] == 1, "result word (%u, %u)", r, w);
            const uint64_t at = (uint64_t(row0 + r) * p.amps + x) / 2;
            CHECK(at < p.S * p.words, "out word %llu", (unsigned long long)at);
            if (at < p.S * p.words) ++out_words[at];
          }
        // ... and wave 0, a lane per column, over the tile's rows against the partner rows
        for (uint32_t tid = 0; sums && tid < kGvTileCols; ++tid) {
          const uint64_t x = col0 + tid;
          if (x >= p.amps) continue;
          const uint32_t rows = p.S - row0 < TM ? p.S - row0 : TM;
          for (uint32_t r = 0; r < rows; ++r) {
            CHECK(result[r * PC + tid] == 1, "result (%u, %u)", r, tid);
            CHECK(uint64_t(row0 + r) * p.amps + x < p.S * p.amps, "partner read");
          }
          if (rt + 1 == p.row_tiles) ++grads[x];
        }
      }
    }
  ++matrix_sweeps;
}

static void check_side(const CgvSide& p, int n, int R, int S, bool bra_side, size_t plane_offset, size_t scratch_floats,
                       std::vector<uint8_t>& scratch) {
  CHECK(p.n == uint32_t(n) && p.R == uint32_t(R) && p.S == uint32_t(S) && p.amps == (uint64_t(1) << n) && p.words * 2 == p.amps &&
            p.matrix == (uint32_t(R) > kGvVectorMaxStates),
        "side of n %d R %d S %d", n, R, S);
  const bool sums = !bra_side;
  std::vector<uint8_t> out_words(size_t(S) * p.words, 0), grads(p.amps, 0);
  if (p.matrix)
    check_matrix(p, bra_side, sums, plane_offset, scratch_floats, scratch, out_words, grads);
  else
    check_vector(p, bra_side, sums, out_words, grads);
  for (size_t i = 0; i < out_words.size(); ++i)
    CHECK(out_words[i] == 1, "n %d R %d S %d: out word %zu written %d times", n, R, S, i, int(out_words[i]));
  for (size_t i = 0; i < grads.size(); ++i)
    CHECK(grads[i] == (sums ? 1 : 0), "n %d R %d S %d: table_grad %zu written %d times", n, R, S, i, int(grads[i]));
}

static void check_shape(int n, int M, int K) {
  const CgvPlan p = cgv_plan(n, M, K);
  CHECK(p.scratch_bytes >= kGvMinScratch && p.scratch_bytes >= (p.ket.plane_floats + p.bra.plane_floats) * sizeof(float) &&
            p.bra_plane_offset == p.ket.plane_floats && p.scratch_bytes % 8 == 0 && (p.bra_plane_offset * sizeof(float)) % 8 == 0,
        "scratch of n %d M %d K %d", n, M, K);
  const size_t scratch_floats = p.scratch_bytes / sizeof(float);
  std::vector<uint8_t> scratch(scratch_floats, 0);
  check_side(p.ket, n, M, K, false, 0, scratch_floats, scratch);
  check_side(p.bra, n, K, M, true, p.bra_plane_offset, scratch_floats, scratch);
  // (the two sides' planes do not meet: no float of the scratch was written twice)
  for (size_t i = 0; i < scratch.size(); ++i) CHECK(scratch[i] <= 1, "scratch float %zu written %d times", i, int(scratch[i]));
}

int main() {
  long shapes = 0;
  const int counts[] = {1, 3, 8, 9, 16, 17, 33, 65, 1024};
  for (int n = 1; n <= 13; ++n)
    for (int M : counts)
      for (int K : counts) {
        check_shape(n, M, K);
        ++shapes;
      }
  for (int M = 1; M <= 40; ++M)
    for (int K = 1; K <= 40; ++K) {
      check_shape(7, M, K);  // every ragged pair around the switch and the tile sizes
      ++shapes;
    }
  CHECK(vector_sweeps > 1000 && matrix_sweeps > 1000 && padded_tiles > 100 && ragged_rows > 10000 && chunked_sweeps > 50,
        "%ld vector sweeps, %ld matrix sweeps, %ld padded tiles, %ld ragged rows, %ld chunked sweeps", vector_sweeps, matrix_sweeps,
        padded_tiles, ragged_rows, chunked_sweeps);
  // 5
  for (int M : {1, 8, 9, 1024})
    for (int K : {1, 8, 9, 1024}) {
      const CgvPlan plan = cgv_plan(31, M, K);
      for (const CgvSide* p : {&plan.ket, &plan.bra}) {
        CHECK(p->grid_x >= 1 && p->grid_y >= 1 && p->grid_y <= 65535u && uint64_t(p->grid_x) * kGvThreads < (uint64_t(1) << 32),
              "grid at 31 qubits, M %d K %d", M, K);
        if (p->matrix) {
          CHECK(uint64_t(p->grid_x) * p->grid_y >= p->col_tiles && p->col_tiles == (1u << 25), "column tiles at 31 qubits");
          CHECK((uint64_t(p->r16) * p->P + kGvThreads - 1) / kGvThreads <= 65535u * 64u, "planes grid of R %u S %u", p->R, p->S);
        } else {
          CHECK(p->slices == (1u << 20) && gv_vec_word(p->slices - 1, 3, kGvThreads - 1) == p->words - 1, "slices at 31 qubits");
        }
      }
      CHECK(plan.scratch_bytes <= size_t(16) * 1024 * 1024 + 2 * 16 * 1024 * 4 && plan.scratch_bytes >= kGvMinScratch, "scratch at M %d K %d",
            M, K);
    }
  std::printf("cross_gram_vjp_plan_check: %ld shapes, %ld vector sweeps, %ld matrix sweeps, %ld padded tiles, %ld ragged rows, %ld chunked sweeps\n",
              shapes, vector_sweeps, matrix_sweeps, padded_tiles, ragged_rows, chunked_sweeps);
  std::printf("cross_gram_vjp_plan_check: %ld failures\n", failures);
  return failures ? 1 : 0;
}
