// cross_gram.hip -- the cross-Gram matrix of two ensembles of device-resident states (gfx950).
//
// qhbm_cross_gram forms C[i, j] = sum_x t(x) conj(a_i(x)) b_j(x) for M complex64 bras a_i and K complex64 kets b_j of 2^n
// amplitudes, in two separate buffers, and a real float32 table t over the bitstrings (NULL: t = 1) -- the M x K matrix
// that overlap, fidelity and trace distance of two state-vector ensembles, transition elements and Loschmidt echoes reduce
// to (engine.cpp).  What is here:
//   cross_gram_tile_kernel<TI, TJ, TABLE>  part[i0 + k, j0 + l, re / im, slice] = the slice's share of C, k < TI, l < TJ,
//                                          complex fp64: one sweep reads TI bra rows, TJ ket rows and the table's words
//                                          once for TI TJ outputs held in registers
//   cross_gram_finish_kernel               C[i, j] = its partials in slice order, for every (i, j): nothing is mirrored and
//                                          nothing is forced to zero
// The (i, j) plane is cut into tiles of 4 x 4 pairs and every tile is launched; ragged M and K run their last tile row,
// column and corner through smaller instantiations (<r, 4>, <4, r'>, <r, r'>, r = M mod 4, r' = K mod 4) instead of a test
// per word.
//
// Shape and order of additions are gram.hip's own (state_sweep.h): 16-byte words, 256 threads striding over the words,
// blockIdx.y = a slice, blockIdx.x = the tile, gram_slices' slice count (a function of n alone).  A thread adds its words
// in word order -- per word and pair the same eight fused multiply-adds, spelled out so that no instantiation contracts
// them differently, the column operand b_j times t first --, a wave's 64 lanes meet in sweep_wave_sum's shuffle tree, the
// four waves in wave order, the slices in slice order through sweep_row_sum2: no floating-point atomics, and C[i, j]
// depends neither on M, nor on K, nor on the tile (i, j) falls into.  So with bras and kets the same buffer C[i, j] has
// the bits of qhbm_weighted_gram's G[i, j] for j > i, and Re C[i, i] those of Re G[i, i]; Im C[i, i] is what the roundings
// of x y - y x leave (G writes 0 there) and C[j, i] is summed on its own (G mirrors it).  The error bound is gram.hip's:
// |dC[i, j]| <= 2 (2^n + 4) 2^-53 sum_x |t| |a_i| |b_j| per part to first order.  Both buffers are only read: they may
// alias or overlap.
//
// (a translation unit of its own in the source tree, compiled as part of observable.hip with the flags states.hip has; it uses
// no name of another .hip file: what it shares with gram.hip is state_sweep.h)
#include "kernels.h"
#include "state_sweep.h"

namespace qhbm {
namespace {

constexpr uint32_t kCrossTile = 4;  // bras / kets along the edges of a full tile

// bras [M, words], kets [K, words]; the launch covers a rectangle of tiles, tile_cols of them per tile row, that starts at
// (i_first, j_first): tile blockIdx.x is (blockIdx.x / tile_cols, blockIdx.x % tile_cols); part [M, K, 2, gridDim.y]
template <uint32_t TI, uint32_t TJ, bool TABLE>
__global__ __launch_bounds__(kSweepThreads) void cross_gram_tile_kernel(const float4* __restrict__ bras, const float4* __restrict__ kets,
                                                                        uint64_t words, const float2* __restrict__ table, uint32_t K,
                                                                        uint32_t i_first, uint32_t j_first, uint32_t tile_cols,
                                                                        double* __restrict__ part) {
  __shared__ double sh[kSweepThreads / 64][2 * TI * TJ];
  const uint32_t ti = blockIdx.x / tile_cols, tj = blockIdx.x - ti * tile_cols;
  const uint32_t i0 = i_first + kCrossTile * ti, j0 = j_first + kCrossTile * tj;
  const float4* ri = bras + uint64_t(i0) * words;
  const float4* rj = kets + uint64_t(j0) * words;
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
    part[((uint64_t(i) * K + j) * 2 + (threadIdx.x & 1u)) * gridDim.y + blockIdx.y] = total;
  }
}

// One workgroup per pair (blockIdx.y, blockIdx.x) = (i, j).  out [M, K, 2]
__global__ __launch_bounds__(kSweepThreads) void cross_gram_finish_kernel(const double* __restrict__ part, uint32_t slices, uint32_t K,
                                                                          double* __restrict__ out) {
  __shared__ double sh[kSweepThreads];
  const uint64_t pair = uint64_t(blockIdx.y) * K + blockIdx.x;
  const double2 c = sweep_row_sum2(part + pair * 2 * slices, slices, sh);
  if (threadIdx.x == 0) {
    out[pair * 2] = c.x;
    out[pair * 2 + 1] = c.y;
  }
}

struct CrossArgs {
  const float4* bras;
  const float4* kets;
  uint64_t words;
  const float2* table;
  uint32_t K, slices;
  double* part;
  hipStream_t stream;
};

// tile_rows x tile_cols tiles of TI x TJ pairs from (i_first, j_first) on
template <uint32_t TI, uint32_t TJ>
void cross_launch_tiles(const CrossArgs& a, uint32_t i_first, uint32_t j_first, uint32_t tile_rows, uint32_t tile_cols) {
  if (!tile_rows || !tile_cols) return;
  const dim3 grid(tile_rows * tile_cols, a.slices);
  if (a.table)
    hipLaunchKernelGGL((cross_gram_tile_kernel<TI, TJ, true>), grid, dim3(kSweepThreads), 0, a.stream, a.bras, a.kets, a.words,
                       a.table, a.K, i_first, j_first, tile_cols, a.part);
  else
    hipLaunchKernelGGL((cross_gram_tile_kernel<TI, TJ, false>), grid, dim3(kSweepThreads), 0, a.stream, a.bras, a.kets, a.words,
                       a.table, a.K, i_first, j_first, tile_cols, a.part);
}

// tile_rows tile rows of TI bras from i_first on, against all the kets: the full tile columns, then the ragged one
template <uint32_t TI>
void cross_launch_rows(const CrossArgs& a, uint32_t i_first, uint32_t tile_rows) {
  const uint32_t full = a.K / kCrossTile, j_tail = full * kCrossTile;
  cross_launch_tiles<TI, 4>(a, i_first, 0, tile_rows, full);
  switch (a.K % kCrossTile) {
    case 1: cross_launch_tiles<TI, 1>(a, i_first, j_tail, tile_rows, 1); break;
    case 2: cross_launch_tiles<TI, 2>(a, i_first, j_tail, tile_rows, 1); break;
    case 3: cross_launch_tiles<TI, 3>(a, i_first, j_tail, tile_rows, 1); break;
    default: break;
  }
}

}  // namespace

size_t cross_gram_parts_count(uint32_t n, uint32_t M, uint32_t K) { return size_t(M) * K * 2 * gram_slices(uint64_t(1) << (n - 1)); }

hipError_t launch_cross_gram(const float2* bras, uint32_t M, const float2* kets, uint32_t K, uint32_t n, const float* table,
                             double* parts, double* out, hipStream_t stream) {
  // (256 x 256 tiles at most in grid.x, at most 256 slices in grid.y)
  if (n < 1 || n > 31 || M < 1 || M > uint32_t(kGramMaxStates) || K < 1 || K > uint32_t(kGramMaxStates)) return hipErrorInvalidValue;
  const uint64_t words = uint64_t(1) << (n - 1);
  const uint32_t slices = gram_slices(words), full = M / kCrossTile;
  const CrossArgs a{reinterpret_cast<const float4*>(bras), reinterpret_cast<const float4*>(kets), words,
                    reinterpret_cast<const float2*>(table), K, slices, parts, stream};
  cross_launch_rows<4>(a, 0, full);
  switch (M % kCrossTile) {
    case 1: cross_launch_rows<1>(a, full * kCrossTile, 1); break;
    case 2: cross_launch_rows<2>(a, full * kCrossTile, 1); break;
    case 3: cross_launch_rows<3>(a, full * kCrossTile, 1); break;
    default: break;
  }
  hipLaunchKernelGGL(cross_gram_finish_kernel, dim3(K, M), dim3(kSweepThreads), 0, stream, parts, slices, K, out);
  return hipGetLastError();
}

}  // namespace qhbm
