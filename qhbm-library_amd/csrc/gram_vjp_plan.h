// gram_vjp_plan.h -- launch plan and index arithmetic of the weighted Gram matrix's VJP, shared by gram_vjp.hip's kernels
// and the host (tests/gram_vjp_plan/gram_vjp_plan_check.cpp walks it on the CPU).
//
//   c_j(x) = sum_i H[i, j] a_i(x),   out_j(x) = t(x) c_j(x),   table_grad(x) = 1/2 sum_j Re(conj(c_j(x)) a_j(x))
//                                                                        (include/qhbm_engine.h qhbm_weighted_gram_vjp)
//
// The plan (a function of n and M alone).  One workgroup owns a range of x and ALL M output states of it, so table_grad(x)
// is finished where it is begun: no partials, no atomics.
//   M <= 8  "vector": state_sweep.h's shape.  The 2^(n-1) words (two amplitudes, 16 bytes) are cut into slices of 1024;
//           thread t of slice s takes the words 1024 s + 256 k + t, k < 4, gv_vec_words(M) of them at a time with all M
//           input rows of each in registers.
//   M >= 9  "matrix": the x axis is cut into column tiles of 64 amplitudes; a workgroup of four waves owns one (wave w its
//           columns 16 w .. 16 w + 15) and walks the output states in row tiles of tm = min(16 ceil(M / 16), 64) and, per
//           row tile, the input states in stages of 16.  H is read from two float planes [P][P], P = row_tiles tm, zero
//           beyond M, which a small kernel writes to the head of the scratch first; rows of the state panel beyond M and
//           columns beyond 2^n are zeros in LDS and are never read from memory.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QHBM_GV_HD __host__ __device__
#else
#define QHBM_GV_HD
#endif

namespace qhbm {

constexpr uint32_t kGvVectorMaxStates = 8;   // up to here the vector kernel; above, the matrix instructions
constexpr uint32_t kGvThreads = 256;
constexpr uint32_t kGvSliceWords = 1024;     // vector kernel: words of a slice (state_sweep.h's kSweepSliceWords)
constexpr uint32_t kGvTileCols = 64;         // matrix kernel: amplitudes of a column tile
constexpr uint32_t kGvMaxTileRows = 64;
constexpr uint32_t kGvStage = 16;            // matrix kernel: input states per stage
constexpr uint32_t kGvGridX = 32768;         // matrix kernel: column tile = blockIdx.y * kGvGridX + blockIdx.x
constexpr size_t kGvMinScratch = 16;         // the vector kernel uses none; the size call never answers 0

struct GvPlan {
  uint32_t n, M;
  bool matrix;
  uint64_t amps, words;       // 2^n, 2^(n-1)
  uint32_t slices;            // vector: workgroups
  uint32_t m16;               // matrix: M rounded up to 16 = the stages' bound
  uint32_t tm, row_tiles, P;  // matrix: rows of a row tile, row tiles, pitch of the H planes (row_tiles tm)
  uint32_t col_tiles;         // matrix: workgroups
  uint32_t grid_x, grid_y;
  size_t plane_floats;        // matrix: 2 P^2
  size_t scratch_bytes;
};

QHBM_GV_HD inline GvPlan gv_plan(int n, int M) {
  GvPlan p;
  p.n = uint32_t(n);
  p.M = uint32_t(M);
  p.matrix = p.M > kGvVectorMaxStates;
  p.amps = uint64_t(1) << n;
  p.words = p.amps >> 1;
  if (p.matrix) {
    p.slices = 0;
    p.m16 = (p.M + 15u) & ~15u;
    p.tm = p.m16 < kGvMaxTileRows ? p.m16 : kGvMaxTileRows;
    p.row_tiles = (p.m16 + p.tm - 1u) / p.tm;
    p.P = p.row_tiles * p.tm;
    p.col_tiles = uint32_t((p.amps + kGvTileCols - 1u) / kGvTileCols);
    p.grid_x = p.col_tiles < kGvGridX ? p.col_tiles : kGvGridX;
    p.grid_y = (p.col_tiles + kGvGridX - 1u) / kGvGridX;
    p.plane_floats = size_t(2) * p.P * p.P;
    p.scratch_bytes = p.plane_floats * sizeof(float);
  } else {
    p.slices = uint32_t((p.words + kGvSliceWords - 1u) / kGvSliceWords);
    p.m16 = p.tm = p.row_tiles = p.P = p.col_tiles = 0;
    p.grid_x = p.slices;
    p.grid_y = 1;
    p.plane_floats = 0;
    p.scratch_bytes = kGvMinScratch;
  }
  return p;
}

// vector kernel: words a thread holds at once (all M rows of each), so that a thread of few states still has loads in flight
QHBM_GV_HD constexpr uint32_t gv_vec_words(uint32_t M) { return M <= 2 ? 4u : M <= 4 ? 2u : 1u; }
// ... and word k < 4 of thread tid of slice s (the caller drops words >= 2^(n-1))
QHBM_GV_HD inline uint64_t gv_vec_word(uint32_t s, uint32_t k, uint32_t tid) {
  return uint64_t(s) * kGvSliceWords + k * kGvThreads + tid;
}

// planes kernel: entry e < P^2 of either plane holds H[e / P, e % P], or 0 where a coordinate is >= M
QHBM_GV_HD inline void gv_plane_element(uint32_t P, uint32_t e, uint32_t* i, uint32_t* j) {
  *i = e / P;
  *j = e % P;
}
// matrix kernel, a stage's loads, pass p of thread tid: the state panel element (input state i0 + *kk, column col0 + *c),
// p < kGvStage kGvTileCols / kGvThreads = 4 ...
QHBM_GV_HD inline void gv_panel_element(uint32_t tid, uint32_t p, uint32_t* kk, uint32_t* c) {
  *kk = tid / kGvTileCols + (kGvThreads / kGvTileCols) * p;
  *c = tid % kGvTileCols;
}
// ... and the H element (input state i0 + *kk, output state row0 + *r), p < tm kGvStage / kGvThreads = tm / 16, read from the
// planes at (i0 + kk) P + row0 + r
QHBM_GV_HD inline void gv_operator_element(uint32_t tm, uint32_t tid, uint32_t p, uint32_t* kk, uint32_t* r) {
  const uint32_t e = tid + kGvThreads * p;
  *kk = e / tm;
  *r = e % tm;
}
// where a lane's accumulator register g of row strip s lies in the tile (the C/D map of v_mfma_f32_16x16x4_f32)
QHBM_GV_HD inline void gv_result_element(uint32_t wave, uint32_t lane, uint32_t s, uint32_t g, uint32_t* r, uint32_t* c) {
  *r = 16u * s + 4u * (lane >> 4) + g;
  *c = 16u * wave + (lane & 15u);
}
// the strips of row tile rt that hold an output state at all (the others are skipped, workgroup-uniformly)
QHBM_GV_HD inline uint32_t gv_live_strips(uint32_t m16, uint32_t tm, uint32_t rt) {
  const uint32_t left = (m16 - rt * tm) / 16u;
  return left < tm / 16u ? left : tm / 16u;
}
// epilogue: pass p of thread tid stores the word (two columns) *w of row *r of the tile, p < tm / 8
QHBM_GV_HD inline void gv_store_element(uint32_t tid, uint32_t p, uint32_t* r, uint32_t* w) {
  *r = tid / (kGvTileCols / 2u) + (kGvThreads / (kGvTileCols / 2u)) * p;
  *w = tid % (kGvTileCols / 2u);
}
// LDS pitches, in floats: a stage's planes [input state][row or column] with 16 floats of padding, so that the four input
// states a wave reads at once (lane >> 4) start 16 banks apart; the result planes [row][column] with 4, which keeps a word's
// two columns 8-byte aligned
QHBM_GV_HD constexpr uint32_t gv_lds_pitch(uint32_t width) { return width + 16u; }
constexpr uint32_t kGvResultPitch = kGvTileCols + 4u;

}  // namespace qhbm
