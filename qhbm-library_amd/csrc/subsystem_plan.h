// subsystem_plan.h -- launch plan and index arithmetic of a dense operator on k arbitrary qubits of M states, shared by
// subsystem_apply.hip's kernels and the host (tests/subsystem_plan/subsystem_plan_check.cpp walks it on the CPU for every
// register of up to 12 qubits and every mask).
//
//   out_m(a, b) = scale_m sum_a' A[a, a'] phi_m(a', b)                          (include/qhbm_engine.h qhbm_subsystem_apply)
//
// Conventions, masks and the deposit / extract helpers are rdm_index.h's: amplitude (a, b) sits at index
// rdm_deposit(a, keep) | rdm_deposit(b, env).  A deposit is bitwise, so the deposit of a sum of values with disjoint bits
// is the OR of their deposits: a thread deposits its own low bits once and the workgroup's high bits are scalar.
//
// The plan (a function of n, keep_mask and M alone).
//   k <= 3  "vector": the state (blockIdx.y/z) is cut into slices of 1024 environment values; thread t of slice s takes the
//           values b = (4 s + j) 256 + t, j < 4, with all 2^k rows of each in registers.
//   k >= 4  "matrix": the output of one state is cut into tiles of tm = min(2^k, 64) rows by 64 environment values; a
//           workgroup of four waves owns a tile, wave w its columns 16 w .. 16 w + 15, and walks a' in steps of
//           tk = min(2^k, 32).  Tile t of a state: row tile t % row_tiles (fastest, so that the workgroups that gather the same
//           columns run together), column tile t / row_tiles.
// Either way slice / tile t of state m leaves one partial of the dot product at parts[(2 m + re/im) slices + t].
#pragma once
#include "rdm_index.h"

namespace qhbm {

constexpr int kSubVectorMaxKeep = 3;       // up to here the vector kernel; above, the matrix instructions
constexpr uint32_t kSubThreads = 256;
constexpr uint32_t kSubVecValues = 4;      // environment values per thread of the vector kernel
constexpr uint32_t kSubTileCols = 64;      // environment values of a matrix tile
constexpr uint32_t kSubMaxTileRows = 64;
constexpr uint32_t kSubMaxTileK = 32;
constexpr uint32_t kSubGridY = 32768;      // states per grid.z layer: state m = blockIdx.z * kSubGridY + blockIdx.y

struct SubPlan {
  uint32_t n, k, M;
  RdmMasks masks;
  bool matrix;
  uint32_t env_values;        // 2^(n - k)
  uint32_t tm, tk;            // matrix: rows of a tile, a' per stage (0 for the vector kernel)
  uint32_t row_tiles, col_tiles;
  uint32_t slices;            // workgroups per state = partials per state and component
  uint32_t grid_y, grid_z;
  size_t operator_floats;     // matrix: the operator transposed into two planes, 2 * 4^k floats at the head of the scratch
  size_t parts_offset;        // bytes: where the partials begin
  size_t scratch_bytes;
};

QHBM_RDM_HD inline SubPlan sub_plan(int n, uint64_t keep_mask, int M) {
  SubPlan p;
  p.n = uint32_t(n);
  p.k = uint32_t(rdm_popcount(keep_mask));
  p.M = uint32_t(M);
  p.masks = rdm_masks(n, keep_mask);
  p.matrix = p.k > uint32_t(kSubVectorMaxKeep);
  p.env_values = 1u << (p.n - p.k);
  if (p.matrix) {
    const uint32_t dim = 1u << p.k;
    p.tm = dim < kSubMaxTileRows ? dim : kSubMaxTileRows;
    p.tk = dim < kSubMaxTileK ? dim : kSubMaxTileK;
    p.row_tiles = dim / p.tm;
    p.col_tiles = (p.env_values + kSubTileCols - 1u) / kSubTileCols;
    p.slices = p.row_tiles * p.col_tiles;
    p.operator_floats = size_t(2) << (2u * p.k);
  } else {
    p.tm = p.tk = 0;
    p.row_tiles = 1;
    p.col_tiles = (p.env_values + kSubVecValues * kSubThreads - 1u) / (kSubVecValues * kSubThreads);
    p.slices = p.col_tiles;
    p.operator_floats = 0;
  }
  p.grid_y = p.M < kSubGridY ? p.M : kSubGridY;
  p.grid_z = (p.M + kSubGridY - 1u) / kSubGridY;
  p.parts_offset = p.operator_floats * sizeof(float);  // (a multiple of 8)
  p.scratch_bytes = p.parts_offset + size_t(p.M) * 2 * p.slices * sizeof(double);
  return p;
}

// vector kernel: the environment value of thread tid, value j of slice s (the caller drops values >= env_values)
QHBM_RDM_HD inline uint32_t sub_vec_high(uint32_t s, uint32_t j) { return (s * kSubVecValues + j) * kSubThreads; }

// matrix kernel: tile t of a state -> first row and first environment value
QHBM_RDM_HD inline void sub_tile_of(uint32_t row_tiles, uint32_t tm, uint32_t t, uint32_t* row0, uint32_t* col0) {
  *row0 = (t % row_tiles) * tm;
  *col0 = (t / row_tiles) * kSubTileCols;
}
// the stage's loads, pass i of thread tid: the state panel element (a' = k0 + *kk, column col0 + *c) ...
QHBM_RDM_HD inline void sub_panel_element(uint32_t tid, uint32_t i, uint32_t* kk, uint32_t* c) {
  *kk = tid / kSubTileCols + (kSubThreads / kSubTileCols) * i;
  *c = tid % kSubTileCols;
}
// ... and the operator element (row row0 + *r, a' = k0 + *kk), read from the transposed planes at (k0 + kk) 2^k + row0 + r
QHBM_RDM_HD inline void sub_operator_element(uint32_t tm, uint32_t tid, uint32_t i, uint32_t* kk, uint32_t* r) {
  *kk = tid / tm + (kSubThreads / tm) * i;
  *r = tid % tm;
}
// where a lane's accumulator register g of row strip s lies in the tile (the C/D map of v_mfma_f32_16x16x4_f32)
QHBM_RDM_HD inline void sub_result_element(uint32_t wave, uint32_t lane, uint32_t s, uint32_t g, uint32_t* r, uint32_t* c) {
  *r = 16u * s + 4u * (lane >> 4) + g;
  *c = 16u * wave + (lane & 15u);
}
// LDS pitch of a stage's planes, in floats: [a'][row or column], 16 floats of padding, so that the four a' a wave reads at
// once (lane >> 4) start 16 banks apart
QHBM_RDM_HD constexpr uint32_t sub_lds_pitch(uint32_t width) { return width + 16u; }

}  // namespace qhbm
