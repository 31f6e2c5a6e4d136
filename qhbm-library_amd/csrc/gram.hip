// gram.hip -- the weighted Gram matrix of M device-resident states (gfx950).
//
// qhbm_weighted_gram forms G[i, j] = sum_x t(x) conj(s_i(x)) s_j(x) for M complex64 states of 2^n amplitudes and a real
// float32 table t over the bitstrings (NULL: t = 1) -- the M x M matrix that fidelity, entropy, overlap and cross entropy
// of a state-vector ensemble against a QHBM reduce to (engine.cpp).  What is here:
//   gram_tile_kernel<TI, TJ, TABLE>  part[i0 + k, j0 + l, re / im, slice] = the slice's share of G, k < TI, l < TJ, complex
//                                    fp64: one sweep reads TI + TJ rows and the table's words once for TI TJ outputs held
//                                    in registers                                              TI + TJ (+ 1/2) reads
//   gram_finish_kernel               G[i, j] = its partials in slice order for j >= i; G[j, i] = conj(G[i, j]) written from
//                                    the same registers, Im G[i, i] = 0: Hermitian bit for bit
// The (i, j) plane is cut into tiles of 4 x 4 pairs and only tiles with j0 >= i0 are launched; a ragged M runs its last
// tile row / column through smaller instantiations (<4, r>, <r, r>, r = M mod 4) instead of a test per word.
//
// Shape (state_sweep.h): 16-byte words, 256 threads striding over the words, blockIdx.y = a slice, blockIdx.x = the tile:
// the tiles of one slice are dispatched together, so a row that several tiles read comes from HBM once and from the L2
// for the others (with the slice in blockIdx.x, 32 states at 24 qubits took 5.56 ms instead of 4.76, one run each).
// The slices are sweep_slices' (1024 words each) up to kGramSlices of them, beyond which a thread takes more words: every
// slice ends in a reduction of 2 TI TJ doubles over the workgroup, which four words per thread do not pay for.  The grid
// is a function of n alone.  A thread adds its words in word order -- per word and pair eight fused multiply-adds,
// spelled out so that no instantiation contracts them differently --, a wave's 64 lanes meet in sweep_wave_sum's shuffle
// tree, the four waves in wave order, the slices in slice order through sweep_row_sum(2): no floating-point atomics, and
// G[i, j] depends neither on M, nor on the tile (i, j) falls into, nor on which other states share the call.
// Products are float x float in double (exact), the column operand times t in double (exact as well: 24 + 24 bits), so
// every rounding is one of the additions' -- |dG[i, j]| <= 2 (2^n + 4) 2^-53 sum_x |t| |s_i| |s_j| per part to first order.
//
// (a translation unit of its own in the source tree, compiled as part of states.hip; it uses no name of another .hip file)
#include "kernels.h"
#include "state_sweep.h"

namespace qhbm {
namespace {

constexpr uint32_t kGramTile = 4;           // state pairs along one edge of a full tile
constexpr uint32_t kGramTriangle = ~0u;     // j_fixed: blockIdx.x counts the tiles j0 >= i0 of `tile_rows` tile rows
// (the slice count is state_sweep.h's gram_slices: at most kGramSlices, shared with cross_gram.hip)

// states [M, words]; tile row r of the launch starts at state i_first + 4 r; its column at j_fixed, or (kGramTriangle)
// the launch covers the upper triangle of tile_rows x tile_rows tiles that starts at (i_first, i_first), row-major;
// part [M, M, 2, gridDim.y]
template <uint32_t TI, uint32_t TJ, bool TABLE>
__global__ __launch_bounds__(kSweepThreads) void gram_tile_kernel(const float4* __restrict__ states, uint64_t words,
                                                                  const float2* __restrict__ table, uint32_t M, uint32_t i_first,
                                                                  uint32_t j_fixed, uint32_t tile_rows, double* __restrict__ part) {
  __shared__ double sh[kSweepThreads / 64][2 * TI * TJ];
  uint32_t ti = blockIdx.x, tj = 0;
  if (j_fixed == kGramTriangle) {  // (wave-uniform: scalar arithmetic, at most tile_rows turns)
    uint32_t rest = blockIdx.x;
    ti = 0;
    while (rest >= tile_rows - ti) {
      rest -= tile_rows - ti;
      ++ti;
    }
    tj = ti + rest;
  }
  const uint32_t i0 = i_first + kGramTile * ti, j0 = j_fixed == kGramTriangle ? i_first + kGramTile * tj : j_fixed;
  const float4* ri = states + uint64_t(i0) * words;
  const float4* rj = states + uint64_t(j0) * words;
  double re[TI * TJ], im[TI * TJ];
#pragma unroll
  for (uint32_t p = 0; p < TI * TJ; ++p) re[p] = im[p] = 0.0;
  for (uint64_t i = uint64_t(blockIdx.y) * kSweepThreads + threadIdx.x; i < words; i += uint64_t(gridDim.y) * kSweepThreads) {
    float4 v[TI], a[TJ];
#pragma unroll
    for (uint32_t k = 0; k < TI; ++k) v[k] = ri[uint64_t(k) * words + i];
#pragma unroll
    for (uint32_t l = 0; l < TJ; ++l) a[l] = rj[uint64_t(l) * words + i];
    double t0 = 1.0, t1 = 1.0;
    if (TABLE) {
      const float2 t = table[i];
      t0 = double(t.x);
      t1 = double(t.y);
    }
#pragma unroll
    for (uint32_t l = 0; l < TJ; ++l) {
      // t times the column operand, once per word
      const double cx = TABLE ? double(a[l].x) * t0 : double(a[l].x), cy = TABLE ? double(a[l].y) * t0 : double(a[l].y);
      const double cz = TABLE ? double(a[l].z) * t1 : double(a[l].z), cw = TABLE ? double(a[l].w) * t1 : double(a[l].w);
#pragma unroll
      for (uint32_t k = 0; k < TI; ++k) {
        const double vx = double(v[k].x), vy = double(v[k].y), vz = double(v[k].z), vw = double(v[k].w);
        double r = re[k * TJ + l], s = im[k * TJ + l];
        r = __builtin_fma(vx, cx, r);
        r = __builtin_fma(vy, cy, r);
        r = __builtin_fma(vz, cz, r);
        r = __builtin_fma(vw, cw, r);
        s = __builtin_fma(vx, cy, s);
        s = __builtin_fma(-vy, cx, s);
        s = __builtin_fma(vz, cw, s);
        s = __builtin_fma(-vw, cz, s);
        re[k * TJ + l] = r;
        im[k * TJ + l] = s;
      }
    }
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t p = 0; p < TI * TJ; ++p) {
    const double r = sweep_wave_sum(re[p]), s = sweep_wave_sum(im[p]);
    if (lane == 0) {
      sh[wave][2 * p] = r;
      sh[wave][2 * p + 1] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * TI * TJ) {
    double total = sh[0][threadIdx.x];
    for (uint32_t w = 1; w < kSweepThreads / 64; ++w) total += sh[w][threadIdx.x];
    const uint32_t p = threadIdx.x >> 1, i = i0 + p / TJ, j = j0 + p % TJ;
    part[((uint64_t(i) * M + j) * 2 + (threadIdx.x & 1u)) * gridDim.y + blockIdx.y] = total;
  }
}

// One workgroup per pair (blockIdx.y, blockIdx.x) = (i, j); those with j < i have nothing to do.  gram [M, M, 2]
__global__ __launch_bounds__(kSweepThreads) void gram_finish_kernel(const double* __restrict__ part, uint32_t slices, uint32_t M,
                                                                    double* __restrict__ gram) {
  __shared__ double sh[kSweepThreads];
  const uint32_t i = blockIdx.y, j = blockIdx.x;
  if (j < i) return;
  const double2 g = sweep_row_sum2(part + (uint64_t(i) * M + j) * 2 * slices, slices, sh);
  const double re = g.x, im = g.y;
  if (threadIdx.x == 0) {
    double* up = gram + (uint64_t(i) * M + j) * 2;
    up[0] = re;
    up[1] = i == j ? 0.0 : im;
    if (i != j) {
      double* lo = gram + (uint64_t(j) * M + i) * 2;
      lo[0] = re;
      lo[1] = -im;
    }
  }
}

template <uint32_t TI, uint32_t TJ>
void gram_launch_tiles(dim3 grid, hipStream_t stream, const float4* states, uint64_t words, const float2* table, uint32_t M,
                       uint32_t i_first, uint32_t j_fixed, uint32_t tile_rows, double* part) {
  if (table)
    hipLaunchKernelGGL((gram_tile_kernel<TI, TJ, true>), grid, dim3(kSweepThreads), 0, stream, states, words, table, M, i_first,
                       j_fixed, tile_rows, part);
  else
    hipLaunchKernelGGL((gram_tile_kernel<TI, TJ, false>), grid, dim3(kSweepThreads), 0, stream, states, words, table, M, i_first,
                       j_fixed, tile_rows, part);
}

}  // namespace

size_t gram_parts_count(uint32_t n, uint32_t M) { return size_t(M) * M * 2 * gram_slices(uint64_t(1) << (n - 1)); }

hipError_t launch_weighted_gram(const float2* states, uint32_t M, uint32_t n, const float* table, double* parts, double* gram,
                                hipStream_t stream) {
  // (256 tile rows: 32896 tiles in grid.x, at most 256 slices in grid.y)
  if (n < 1 || n > 31 || M < 1 || M > uint32_t(kGramMaxStates)) return hipErrorInvalidValue;
  const uint64_t words = uint64_t(1) << (n - 1);
  const uint32_t slices = gram_slices(words), full = M / kGramTile, tail = M % kGramTile, j_tail = full * kGramTile;
  const float4* s4 = reinterpret_cast<const float4*>(states);
  const float2* t2 = reinterpret_cast<const float2*>(table);
  if (full)
    gram_launch_tiles<4, 4>(dim3(full * (full + 1) / 2, slices), stream, s4, words, t2, M, 0, kGramTriangle, full, parts);
#define GRAM_TAIL(R)                                                                                        \
  case R:                                                                                                   \
    if (full) gram_launch_tiles<4, R>(dim3(full, slices), stream, s4, words, t2, M, 0, j_tail, full, parts); \
    gram_launch_tiles<R, R>(dim3(1, slices), stream, s4, words, t2, M, j_tail, j_tail, 1, parts);           \
    break;
  switch (tail) {
    GRAM_TAIL(1)
    GRAM_TAIL(2)
    GRAM_TAIL(3)
    default: break;
  }
#undef GRAM_TAIL
  hipLaunchKernelGGL(gram_finish_kernel, dim3(M, M), dim3(kSweepThreads), 0, stream, parts, slices, M, gram);
  return hipGetLastError();
}

}  // namespace qhbm
