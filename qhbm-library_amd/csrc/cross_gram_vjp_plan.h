// cross_gram_vjp_plan.h -- launch plan and index arithmetic of the cross-Gram matrix's VJP, shared by cross_gram_vjp.hip's
// kernels and the host (tests/cross_gram_vjp_plan/cross_gram_vjp_plan_check.cpp walks it on the CPU).
//
// For C[i, j] = sum_x t(x) conj(a_i(x)) b_j(x) and a cotangent Gamma [M, K] of C (include/qhbm_engine.h qhbm_cross_gram_vjp)
//   out_kets_j(x) = t(x) c_j(x),  c_j(x) = sum_i Gamma[i, j] a_i(x);   out_bras_i(x) = t(x) sum_j conj(Gamma[i, j]) b_j(x);
//   table_grad(x) = sum_j Re(conj(c_j(x)) b_j(x)).
// Both state outputs are one SIDE SWEEP  out_s(x) = t(x) sum_r W[r, s] src_r(x)  of R source rows and S output rows:
//   ket side  src = bras, R = M, S = K, W[r, s] = Gamma[r, s]         (it also sums table_grad, with the kets as partner rows)
//   bra side  src = kets, R = K, S = M, W[r, s] = conj(Gamma[s, r])
//
// The plan of a side (a function of n, R and S alone; the kernel depends on R, the SOURCE side's row count, only).  One
// workgroup owns a range of x and ALL S output rows of it, so table_grad(x) is finished where it is begun: no partials, no
// atomics.  The index helpers are gram_vjp_plan.h's, which this file only reads:
//   R <= 8  "vector": state_sweep.h's shape, slices of 1024 words; thread t of slice s takes the words 1024 s + 256 k + t,
//           k < 4, gv_vec_words(R) of them at a time with all R source rows of each in registers.  W goes through LDS in
//           chunks of kCgvChunk output rows, so its footprint does not grow with S.
//   R >= 9  "matrix": column tiles of 64 amplitudes, row tiles of tm = min(16 ceil(S / 16), 64) OUTPUT rows and stages of 16
//           SOURCE rows.  W is read from two float planes [Pr][Ps], Pr = 16 ceil(R / 16), Ps = row_tiles tm, zero beyond
//           (R, S), which a small kernel writes to the scratch first; source rows beyond R and columns beyond 2^n are zeros in
//           LDS and are never read from memory.
// The scratch holds the ket side's planes at its head and the bra side's after them.
#pragma once
#include "gram_vjp_plan.h"

namespace qhbm {

constexpr uint32_t kCgvChunk = 64;  // vector kernel: output rows whose W entries sit in LDS at once

struct CgvSide {
  uint32_t n, R, S;
  bool matrix;
  uint64_t amps, words;       // 2^n, 2^(n-1)
  uint32_t slices;            // vector: workgroups
  uint32_t chunks;            // vector: ceil(S / kCgvChunk)
  uint32_t r16;               // matrix: R rounded up to 16 = the stages' bound = rows of a W plane (Pr)
  uint32_t s16;               // matrix: S rounded up to 16
  uint32_t tm, row_tiles, P;  // matrix: output rows of a row tile, row tiles, pitch of a W plane (Ps = row_tiles tm)
  uint32_t col_tiles;         // matrix: workgroups
  uint32_t grid_x, grid_y;
  size_t plane_floats;        // matrix: 2 Pr Ps
};

QHBM_GV_HD inline CgvSide cgv_side(int n, int R, int S) {
  CgvSide p;
  p.n = uint32_t(n);
  p.R = uint32_t(R);
  p.S = uint32_t(S);
  p.matrix = p.R > kGvVectorMaxStates;
  p.amps = uint64_t(1) << n;
  p.words = p.amps >> 1;
  if (p.matrix) {
    p.slices = p.chunks = 0;
    p.r16 = (p.R + 15u) & ~15u;
    p.s16 = (p.S + 15u) & ~15u;
    p.tm = p.s16 < kGvMaxTileRows ? p.s16 : kGvMaxTileRows;
    p.row_tiles = (p.s16 + p.tm - 1u) / p.tm;
    p.P = p.row_tiles * p.tm;
    p.col_tiles = uint32_t((p.amps + kGvTileCols - 1u) / kGvTileCols);
    p.grid_x = p.col_tiles < kGvGridX ? p.col_tiles : kGvGridX;
    p.grid_y = (p.col_tiles + kGvGridX - 1u) / kGvGridX;
    p.plane_floats = size_t(2) * p.r16 * p.P;
  } else {
    p.slices = uint32_t((p.words + kGvSliceWords - 1u) / kGvSliceWords);
    p.chunks = (p.S + kCgvChunk - 1u) / kCgvChunk;
    p.r16 = p.s16 = p.tm = p.row_tiles = p.P = p.col_tiles = 0;
    p.grid_x = p.slices;
    p.grid_y = 1;
    p.plane_floats = 0;
  }
  return p;
}

struct CgvPlan {
  CgvSide ket;              // src = bras: R = M, S = K
  CgvSide bra;              // src = kets: R = K, S = M
  size_t bra_plane_offset;  // floats from the head of the scratch to the bra side's planes
  size_t scratch_bytes;
};

QHBM_GV_HD inline CgvPlan cgv_plan(int n, int M, int K) {
  CgvPlan p;
  p.ket = cgv_side(n, M, K);
  p.bra = cgv_side(n, K, M);
  p.bra_plane_offset = p.ket.plane_floats;
  const size_t bytes = (p.ket.plane_floats + p.bra.plane_floats) * sizeof(float);
  p.scratch_bytes = bytes < kGvMinScratch ? kGvMinScratch : bytes;
  return p;
}

// Where W[r, s] of a side lies in the cotangent Gamma [M, K], row-major: the ket side reads Gamma[r, s] as it is (S = K), the
// bra side Gamma[s, r] (R = K) and conjugates it.
QHBM_GV_HD inline size_t cgv_cotangent_index(bool bra_side, uint32_t R, uint32_t S, uint32_t r, uint32_t s) {
  return bra_side ? size_t(s) * R + r : size_t(r) * S + s;
}

// vector kernel: entry e < R * live of a chunk's LDS image holds W[e / live, s0 + e % live], live = the chunk's output rows
QHBM_GV_HD inline uint32_t cgv_chunk_rows(uint32_t S, uint32_t chunk) {
  const uint32_t left = S - chunk * kCgvChunk;
  return left < kCgvChunk ? left : kCgvChunk;
}

// planes kernel: entry e < Pr Ps of either plane holds W[e / Ps, e % Ps], or 0 where r >= R or s >= S
QHBM_GV_HD inline void cgv_plane_element(uint32_t Ps, uint32_t e, uint32_t* r, uint32_t* s) {
  *r = e / Ps;
  *s = e % Ps;
}

}  // namespace qhbm
