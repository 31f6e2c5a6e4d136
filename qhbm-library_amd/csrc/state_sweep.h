// state_sweep.h -- the one shape of the kernels that sweep whole state vectors, and the order in which their sums meet.
//
// import_states.hip, thermal.hip, krylov.hip and gram.hip stream states as 16-byte words (two complex64 amplitudes):
// 256 threads on consecutive words, a SLICE of 1024 words per workgroup, the state (or the slice) in blockIdx.y, so the
// grid is a function of n alone.  Every sum over a state is float64 and made in two steps: a partial per workgroup, then
// a small kernel of one workgroup per result that adds the partials in slice order.  The additions always meet the
// same way -- a thread's own words in word order; the 64 lanes of a wave in sweep_wave_sum's shuffle tree and the four
// waves in wave order, or the 256 threads in sweep_block_sum's LDS tree; the slices through sweep_row_sum -- which is
// what makes these results reproducible bit for bit: no floating-point atomics, and nothing depends on chunk_states or
// on which other states share the call.  A change to a tree here changes result bits of every feature built on it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qhbm {

constexpr uint32_t kSweepThreads = 256;
constexpr uint32_t kSweepSliceWords = 4 * kSweepThreads;

inline uint32_t sweep_slices(uint64_t words) { return uint32_t((words + kSweepSliceWords - 1) / kSweepSliceWords); }

// The slices of the Gram kernels (gram.hip, cross_gram.hip): sweep_slices' up to kGramSlices of them, beyond which a thread
// takes more words (from n = 20 on more than 4).  Both kernels use this one count, which is what makes their sums meet the
// same way.
constexpr uint32_t kGramSlices = 256;
inline uint32_t gram_slices(uint64_t words) {
  const uint32_t slices = sweep_slices(words);
  return slices < kGramSlices ? slices : kGramSlices;
}

// Sum over the workgroup's 256 threads (every thread gets it); sh: 256 doubles of LDS.  A second call on the same sh
// needs a barrier in between: a fast thread's store would race a slow thread's read of sh[0].
__device__ __forceinline__ double sweep_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t s = kSweepThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

// Sum over the 64 lanes of a wave; lane 0 holds it.
__device__ __forceinline__ double sweep_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// Sum of a row of `slices` partials: thread t adds the entries t, t + 256, ... in that order, then the block tree.
__device__ __forceinline__ double sweep_row_sum(const double* __restrict__ row, uint32_t slices, double* sh) {
  double acc = 0.0;
  for (uint32_t i = threadIdx.x; i < slices; i += kSweepThreads) acc += row[i];
  return sweep_block_sum(acc, sh);
}

// The same for a complex row -- `slices` real parts, then `slices` imaginary parts -- as (re, im).  One loop reads both, so
// that their loads are in flight together: read one row after the other, a Krylov basis with full reorthogonalisation
// (one such sum per basis row, round and step) took 1.2 % longer at 20 qubits.
__device__ __forceinline__ double2 sweep_row_sum2(const double* __restrict__ row, uint32_t slices, double* sh) {
  double re = 0.0, im = 0.0;
  for (uint32_t i = threadIdx.x; i < slices; i += kSweepThreads) {
    re += row[i];
    im += row[slices + i];
  }
  re = sweep_block_sum(re, sh);
  __syncthreads();
  im = sweep_block_sum(im, sh);
  return make_double2(re, im);
}

// |a_0|^2 + |a_1|^2 of a word's two amplitudes, in double
__device__ __forceinline__ double word_norm2(float4 v) {
  return (double(v.x) * double(v.x) + double(v.y) * double(v.y)) + (double(v.z) * double(v.z) + double(v.w) * double(v.w));
}

// c * (two amplitudes)
__device__ __forceinline__ float4 sweep_cmul(float2 c, float4 t) {
  return make_float4(c.x * t.x - c.y * t.y, c.x * t.y + c.y * t.x, c.x * t.z - c.y * t.w, c.x * t.w + c.y * t.z);
}

}  // namespace qhbm
