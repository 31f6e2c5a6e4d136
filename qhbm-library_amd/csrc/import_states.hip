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
// order and uses the same tree.  The slicing depends on n alone.
#include "kernels.h"

namespace qhbm {
namespace {

constexpr uint32_t kImpThreads = 256;
constexpr uint32_t kImpWordsPerThread = 4;
constexpr uint32_t kImpSliceWords = kImpThreads * kImpWordsPerThread;

__device__ __forceinline__ double imp_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (uint32_t s = kImpThreads / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  return sh[0];
}

uint32_t imp_slices(uint64_t words) { return uint32_t((words + kImpSliceWords - 1) / kImpSliceWords); }

// words: 16-byte words of one input state (2^(n - 1)); part [c, gridDim.x]
__global__ __launch_bounds__(kImpThreads) void import_norm_parts(const float4* __restrict__ src, uint64_t words, uint32_t s0,
                                                                 double* __restrict__ part) {
  __shared__ double sh[kImpThreads];
  const float4* st = src + (uint64_t(s0) + blockIdx.y) * words;
  const uint64_t w0 = uint64_t(blockIdx.x) * kImpSliceWords + threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (uint32_t k = 0; k < kImpWordsPerThread; ++k) {
    const uint64_t w = w0 + uint64_t(k) * kImpThreads;
    if (w < words) {
      const float4 v = st[w];
      acc += (double(v.x) * double(v.x) + double(v.y) * double(v.y)) + (double(v.z) * double(v.z) + double(v.w) * double(v.w));
    }
  }
  const double total = imp_block_sum(acc, sh);
  if (threadIdx.x == 0) part[uint64_t(blockIdx.y) * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(kImpThreads) void import_norm_finish(const double* __restrict__ part, uint32_t slices, uint32_t s0,
                                                                  double* __restrict__ norm2) {
  __shared__ double sh[kImpThreads];
  const double* row = part + uint64_t(blockIdx.x) * slices;
  double acc = 0.0;
  for (uint32_t i = threadIdx.x; i < slices; i += kImpThreads) acc += row[i];
  const double total = imp_block_sum(acc, sh);
  if (threadIdx.x == 0) norm2[s0 + blockIdx.x] = total;
}

// words_in = 2^(n - 1), words_out = 2^(n_eff - 1) >= words_in; psi: the chunk's states, element 0 first
__global__ __launch_bounds__(kImpThreads) void import_copy(const float4* __restrict__ src, uint64_t words_in, uint64_t words_out,
                                                           uint32_t s0, const double* __restrict__ norm2, float4* __restrict__ psi) {
  const float4* st = src + (uint64_t(s0) + blockIdx.y) * words_in;
  float4* out = psi + uint64_t(blockIdx.y) * words_out;
  const double n2 = norm2[s0 + blockIdx.y];
  const double inv = n2 > 0.0 ? 1.0 / sqrt(n2) : 0.0;
  const uint64_t w0 = uint64_t(blockIdx.x) * kImpSliceWords + threadIdx.x;
#pragma unroll
  for (uint32_t k = 0; k < kImpWordsPerThread; ++k) {
    const uint64_t w = w0 + uint64_t(k) * kImpThreads;
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

// st[r, :] *= sqrt(norm2[r]); words = 16-byte words per row
__global__ __launch_bounds__(kImpThreads) void scale_state_rows_kernel(float4* __restrict__ st, uint64_t words,
                                                                       const double* __restrict__ norm2) {
  float4* row = st + uint64_t(blockIdx.y) * words;
  const double f = sqrt(norm2[blockIdx.y]);
  const uint64_t w0 = uint64_t(blockIdx.x) * kImpSliceWords + threadIdx.x;
#pragma unroll
  for (uint32_t k = 0; k < kImpWordsPerThread; ++k) {
    const uint64_t w = w0 + uint64_t(k) * kImpThreads;
    if (w >= words) continue;
    const float4 a = row[w];
    row[w] = make_float4(float(double(a.x) * f), float(double(a.y) * f), float(double(a.z) * f), float(double(a.w) * f));
  }
}

}  // namespace

size_t import_norm_parts_count(uint32_t n, uint32_t c) { return size_t(c) * imp_slices(uint64_t(1) << (n - 1)); }

hipError_t launch_import_states(const float2* src, uint32_t n, uint32_t n_eff, uint32_t c, uint32_t s0, float2* psi,
                                double* parts, double* norm2, hipStream_t stream) {
  if (n < 1 || n_eff < n || c == 0 || c > 65535u) return hipErrorInvalidValue;
  const uint64_t words_in = uint64_t(1) << (n - 1), words_out = uint64_t(1) << (n_eff - 1);
  const uint32_t slices_in = imp_slices(words_in), slices_out = imp_slices(words_out);
  hipLaunchKernelGGL(import_norm_parts, dim3(slices_in, c), dim3(kImpThreads), 0, stream,
                     reinterpret_cast<const float4*>(src), words_in, s0, parts);
  hipLaunchKernelGGL(import_norm_finish, dim3(c), dim3(kImpThreads), 0, stream, parts, slices_in, s0, norm2);
  hipLaunchKernelGGL(import_copy, dim3(slices_out, c), dim3(kImpThreads), 0, stream, reinterpret_cast<const float4*>(src),
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

hipError_t launch_scale_state_rows(float2* st, uint32_t rows, uint32_t n, const double* norm2, hipStream_t stream) {
  if (!rows) return hipSuccess;
  if (n < 1 || rows > 65535u) return hipErrorInvalidValue;
  const uint64_t words = uint64_t(1) << (n - 1);
  hipLaunchKernelGGL(scale_state_rows_kernel, dim3(imp_slices(words), rows), dim3(kImpThreads), 0, stream,
                     reinterpret_cast<float4*>(st), words, norm2);
  return hipGetLastError();
}

}  // namespace qhbm
