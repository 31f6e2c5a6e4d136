// import_states.hip -- caller-supplied start states into the engine's workspace (gfx950).
//
// qhbm_*_from_states take states as [U, 2^n] complex64, interleaved (re, im), amplitude index = the bitstring read
// big-endian: the layout qhbm_statevector writes.  The workspace holds a state at a pitch of 2^n_eff amplitudes
// (n_eff = max(n, 10): idle padding qubits are the high index bits and stay |0>), and the expectation values accumulate
// in fixed point on the premise ||psi|| = 1 (program.h kValueFracBits).  Per chunk of c states:
//   1. import_norm_parts   part[i, slice] = sum over the slice of |phi_i[y]|^2, fp64            (reads the input once)
//   2. import_norm_finish  norm2[s0 + i]  = sum of the state's slices, in slice order, fp64
//   3. import_copy         psi_i = phi_i / ||phi_i|| at the workspace pitch, zeros in the padding (reads it a second time)
// A state of norm 0 is imported as zeros (factor 0, never 1 / 0).  The squared norms stay on the device: the callers
// multiply values and upstream rows by norm2 and exported states by its root, so every output is the plain quadratic
// (or linear) function of the states as given.
//
// Shape: streaming kernels, one 16-byte word (two amplitudes) per access.  blockIdx.y is the state, blockIdx.x a SLICE of
// 2^10 words (256 threads x 4 words, consecutive threads on consecutive words): one state of 20 qubits is 512
// workgroups, two per CU, whatever U.
//
// Determinism (no floating-point atomics; nothing depends on chunk_states): a thread adds its 4 words in word order, the
// 256 threads of a slice meet in a fixed LDS tree, import_norm_finish gives thread t the slices t, t + 256, ... in
// order and uses the same tree (state_sweep.h).  The slicing depends on n alone.
//
// The way back is here too: scale_copy_kernel takes rows between the workspace's pitch and the caller's, times a
// per-state factor -- the export of qhbm_statevector_from_states (times ||phi||), the staging of qhbm_apply_observables,
// the last sweep of the evolution and v_{j+1} = w / beta_j of the Krylov basis.
//
// (a translation unit of its own in the source tree, compiled as part of states.hip; it uses no name of another .hip file)
#include "kernels.h"
#include "state_sweep.h"

namespace qhbm {
namespace {

constexpr uint32_t kImpWordsPerThread = kSweepSliceWords / kSweepThreads;

// words: 16-byte words of one input state (2^(n - 1)); part [c, gridDim.x]
__global__ __launch_bounds__(kSweepThreads) void import_norm_parts(const float4* __restrict__ src, uint64_t words, uint32_t s0,
                                                                   double* __restrict__ part) {
  __shared__ double sh[kSweepThreads];
  const float4* st = src + (uint64_t(s0) + blockIdx.y) * words;
  const uint64_t w0 = uint64_t(blockIdx.x) * kSweepSliceWords + threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (uint32_t k = 0; k < kImpWordsPerThread; ++k) {
    const uint64_t w = w0 + uint64_t(k) * kSweepThreads;
    if (w < words) acc += word_norm2(st[w]);
  }
  const double total = sweep_block_sum(acc, sh);
  if (threadIdx.x == 0) part[uint64_t(blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(kSweepThreads) void import_norm_finish(const double* __restrict__ part, uint32_t slices, uint32_t s0,
                                                                    double* __restrict__ norm2) {
  __shared__ double sh[kSweepThreads];
  const double total = sweep_row_sum(part + uint64_t(blockIdx.x) * slices, slices, sh);
  if (threadIdx.x == 0) norm2[s0 + blockIdx.x] = total;
}

// words_in = 2^(n - 1), words_out = 2^(n_eff - 1) >= words_in; psi: the chunk's states, element 0 first
__global__ __launch_bounds__(kSweepThreads) void import_copy(const float4* __restrict__ src, uint64_t words_in, uint64_t words_out,
                                                             uint32_t s0, const double* __restrict__ norm2, float4* __restrict__ psi) {
  const float4* st = src + (uint64_t(s0) + blockIdx.y) * words_in;
  float4* out = psi + uint64_t(blockIdx.y) * words_out;
  const double n2 = norm2[s0 + blockIdx.y];
  const double inv = n2 > 0.0 ? 1.0 / sqrt(n2) : 0.0;
  const uint64_t w0 = uint64_t(blockIdx.x) * kSweepSliceWords + threadIdx.x;
#pragma unroll
  for (uint32_t k = 0; k < kImpWordsPerThread; ++k) {
    const uint64_t w = w0 + uint64_t(k) * kSweepThreads;
    if (w >= words_out) continue;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (w < words_in && inv != 0.0) {
      const float4 a = st[w];
      v = make_float4(float(double(a.x) * inv), float(double(a.y) * inv), float(double(a.z) * inv), float(double(a.w) * inv));
    }
    out[w] = v;
  }
}

// out[r, k] = in[r, k] * norm2[r]
__global__ __launch_bounds__(256) void scale_by_norm2_kernel(const float* __restrict__ in, float* __restrict__ out, uint64_t count,
                                                             uint32_t width, const double* __restrict__ norm2) {
  const uint64_t i = uint64_t(blockIdx.x) * 256u + threadIdx.x;
  if (i < count) out[i] = float(double(in[i]) * norm2[i / width]);
}

// dst row r (dst_pitch words) = src row r (src_pitch words) * f_r for the first words_copy words, zeros behind them;
// f_r = scale[r] (or 1) * sqrt(norm2[r]) (or 1)
__global__ __launch_bounds__(kSweepThreads) void scale_copy_kernel(const float4* __restrict__ src, uint64_t src_pitch,
                                                                   float4* __restrict__ dst, uint64_t dst_pitch, uint64_t words_copy,
                                                                   const double* __restrict__ scale, const double* __restrict__ norm2) {
  const float4* in = src + uint64_t(blockIdx.y) * src_pitch;
  float4* out = dst + uint64_t(blockIdx.y) * dst_pitch;
  const bool scaled = scale || norm2;
  const double f = (scale ? scale[blockIdx.y] : 1.0) * (norm2 ? sqrt(norm2[blockIdx.y]) : 1.0);
  for (uint64_t i = uint64_t(blockIdx.x) * kSweepThreads + threadIdx.x; i < dst_pitch; i += uint64_t(gridDim.x) * kSweepThreads) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < words_copy) {
      v = in[i];
      if (scaled) v = make_float4(float(double(v.x) * f), float(double(v.y) * f), float(double(v.z) * f), float(double(v.w) * f));
    }
    out[i] = v;
  }
}

}  // namespace

size_t state_norm_parts_count(uint32_t n, uint32_t c) { return size_t(c) * sweep_slices(uint64_t(1) << (n - 1)); }

hipError_t launch_import_states(const float2* src, uint32_t n, uint32_t n_eff, uint32_t c, uint32_t s0, float2* psi,
                                double* parts, double* norm2, hipStream_t stream) {
  if (n < 1 || n_eff < n || c == 0 || c > 65535u) return hipErrorInvalidValue;
  const uint64_t words_in = uint64_t(1) << (n - 1), words_out = uint64_t(1) << (n_eff - 1);
  const uint32_t slices_in = sweep_slices(words_in), slices_out = sweep_slices(words_out);
  hipLaunchKernelGGL(import_norm_parts, dim3(slices_in, c), dim3(kSweepThreads), 0, stream,
                     reinterpret_cast<const float4*>(src), words_in, s0, parts);
  hipLaunchKernelGGL(import_norm_finish, dim3(c), dim3(kSweepThreads), 0, stream, parts, slices_in, s0, norm2);
  hipLaunchKernelGGL(import_copy, dim3(slices_out, c), dim3(kSweepThreads), 0, stream, reinterpret_cast<const float4*>(src),
                     words_in, words_out, s0, norm2, reinterpret_cast<float4*>(psi));
  return hipGetLastError();
}

hipError_t launch_scale_by_norm2(const float* in, float* out, uint32_t rows, uint32_t width, const double* norm2,
                                 hipStream_t stream) {
  const uint64_t count = uint64_t(rows) * width;
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(scale_by_norm2_kernel, dim3(unsigned((count + 255) / 256)), dim3(256), 0, stream, in, out, count, width,
                     norm2);
  return hipGetLastError();
}

hipError_t launch_scale_copy_states(const float2* src, uint32_t n_src, float2* dst, uint32_t n_dst, uint32_t n_copy, uint32_t c,
                                    const double* scale, const double* norm2, hipStream_t stream) {
  if (!c) return hipSuccess;
  if (n_copy < 1 || n_copy > n_src || n_copy > n_dst || c > 65535u) return hipErrorInvalidValue;
  const uint64_t dst_pitch = uint64_t(1) << (n_dst - 1);
  hipLaunchKernelGGL(scale_copy_kernel, dim3(sweep_slices(dst_pitch), c), dim3(kSweepThreads), 0, stream,
                     reinterpret_cast<const float4*>(src), uint64_t(1) << (n_src - 1), reinterpret_cast<float4*>(dst), dst_pitch,
                     uint64_t(1) << (n_copy - 1), scale, norm2);
  return hipGetLastError();
}

}  // namespace qhbm
