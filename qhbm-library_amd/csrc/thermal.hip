// thermal.hip -- Chebyshev evolution of caller-supplied states under H = sum_k w_k O_k (gfx950).
//
// qhbm_evolve_states forms e^{-tau H} phi (normalised, with log ||e^{-tau H} phi||) or e^{-i tau H} phi as a sum of
// Chebyshev polynomials of H~ = H / R, R = sum_k |w_k| sum_j |c_kj| >= ||H||, in steps of argument x = delta R (engine.cpp
// evolve_states).  H t comes from the observable kernels (run_observable_chunk with the scale 1 / R or
// 2 / R folded into the upstream weights); what is here is everything around them:
//   cheb_step_kernel     t_{k+1} = w - t_{k-1} over t_{k-1}, acc += c_{k+1} t_{k+1}  (w = (2 / R) H t_k)       3 reads, 2 writes
//     <FIRST>            t_0 = acc * scale over t_{k-1}, acc = c_0 t_0 + c_1 w       (w = (1 / R) H (acc * scale): the
//                        rescale of the previous step's sum is fused here and into the upstream row of that launch)
//     <., NORM>          ... and part[state, workgroup] = sum |acc|^2 of the workgroup's words, fp64
//   finish_step_kernel   norm = sqrt(sum of the state's partials, in index order); log_norm += log(norm) + x;
//                        scale = 1 / norm (0 for norm 0: zeros and -inf); the state's upstream row (w_k / R) * scale
//   evolve_init_kernel   scale = 1, log_norm = log ||phi|| from the import's squared norms, the upstream rows
//   random_states_kernel random-sign states from Philox4x32-10, reproducible bit for bit (tests/thermal_ref.py)
// The rows go back to the caller's pitch (2^n), times 1 / norm or ||phi||, through import_states.hip's
// launch_scale_copy_states.
//
// Shape (state_sweep.h): streaming kernels, 16-byte words (two amplitudes), blockIdx.y = the state, blockIdx.x strides
// over the state's words with gridDim.x = words / 1024 workgroups of 256 threads (four words per thread, consecutive
// threads on consecutive words).  The grid depends on n alone, every state is summed by itself, the partials meet in a
// fixed LDS tree and are added in index order: no floating-point atomics, and nothing depends on chunk_states or on
// which other states share the call.
//
// (a translation unit of its own in the source tree, compiled as part of states.hip; it uses no name of another .hip file)
#include <algorithm>
#include <cmath>

#include "device_common.h"
#include "kernels.h"
#include "state_sweep.h"

namespace qhbm {
namespace {

// words = 2^(n_eff - 1): 16-byte words of one state in the workspace; w, tprev, acc: the chunk's states, element 0 first
template <bool FIRST, bool NORM>
__global__ __launch_bounds__(kSweepThreads) void cheb_step_kernel(const float4* __restrict__ w, float4* __restrict__ tprev,
                                                                  float4* __restrict__ acc, uint64_t words, float2 c0, float2 c,
                                                                  const double* __restrict__ scale, double* __restrict__ part) {
  __shared__ double sh[NORM ? kSweepThreads : 1];
  const uint64_t base = uint64_t(blockIdx.y) * words;
  const double sc = FIRST ? scale[blockIdx.y] : 1.0;
  double sum = 0.0;
  for (uint64_t i = uint64_t(blockIdx.x) * kSweepThreads + threadIdx.x; i < words; i += uint64_t(gridDim.x) * kSweepThreads) {
    const float4 wv = w[base + i];
    float4 t, a;
    if (FIRST) {
      const float4 s = acc[base + i];
      const float4 t0 = make_float4(float(double(s.x) * sc), float(double(s.y) * sc), float(double(s.z) * sc), float(double(s.w) * sc));
      const float4 a0 = sweep_cmul(c0, t0), a1 = sweep_cmul(c, wv);
      t = t0;
      a = make_float4(a0.x + a1.x, a0.y + a1.y, a0.z + a1.z, a0.w + a1.w);
    } else {
      const float4 p = tprev[base + i], s = acc[base + i];
      t = make_float4(wv.x - p.x, wv.y - p.y, wv.z - p.z, wv.w - p.w);
      const float4 d = sweep_cmul(c, t);
      a = make_float4(s.x + d.x, s.y + d.y, s.z + d.z, s.w + d.w);
    }
    tprev[base + i] = t;
    acc[base + i] = a;
    if (NORM) sum += word_norm2(a);
  }
  if (NORM) {
    const double total = sweep_block_sum(sum, sh);
    if (threadIdx.x == 0) part[uint64_t(blockIdx.y) * gridDim.x + blockIdx.x] = total;
  }
}

// One workgroup per state of the chunk.  wr [n_ops]: w_k / R; up1 [c, n_ops]: the upstream rows of the next step's first term.
__global__ __launch_bounds__(kSweepThreads) void finish_step_kernel(const double* __restrict__ part, uint32_t slices, double x,
                                                                    double* __restrict__ log_norm, double* __restrict__ scale,
                                                                    const double* __restrict__ wr, uint32_t n_ops,
                                                                    float* __restrict__ up1) {
  __shared__ double sh[kSweepThreads];
  const double norm = sqrt(sweep_row_sum(part + uint64_t(blockIdx.x) * slices, slices, sh));
  const double sc = norm > 0.0 ? 1.0 / norm : 0.0;
  if (threadIdx.x == 0) {
    scale[blockIdx.x] = sc;
    log_norm[blockIdx.x] += log(norm) + x;  // (norm 0: -inf, and it stays there)
  }
  for (uint32_t k = threadIdx.x; k < n_ops; k += kSweepThreads) up1[uint64_t(blockIdx.x) * n_ops + k] = float(wr[k] * sc);
}

// scale [c] = 1; log_norm [c] (or null) = log ||phi|| from norm2 [c]; up1 [c, n_ops] = wr, up2 [c, n_ops] (or null) = 2 wr
__global__ __launch_bounds__(kSweepThreads) void evolve_init_kernel(uint32_t c, const double* __restrict__ norm2,
                                                                    double* __restrict__ log_norm, double* __restrict__ scale,
                                                                    const double* __restrict__ wr, uint32_t n_ops,
                                                                    float* __restrict__ up1, float* __restrict__ up2) {
  const uint64_t i = uint64_t(blockIdx.x) * kSweepThreads + threadIdx.x;
  if (i < c) {
    if (scale) scale[i] = 1.0;
    if (log_norm) log_norm[i] = 0.5 * log(norm2[i]);
  }
  if (i < uint64_t(c) * n_ops) {
    const double v = wr[i % n_ops];
    if (up1) up1[i] = float(v);
    if (up2) up2[i] = float(2.0 * v);
  }
}

constexpr uint32_t kRandomStatesTag = 0x54505153u;

// One thread per 16-byte word (amplitudes 2 i and 2 i + 1) of one state; words = 2^(n - 1)
__global__ __launch_bounds__(kSweepThreads) void random_states_kernel(float4* __restrict__ out, uint64_t words, uint64_t seed,
                                                                      uint32_t first_state, float mag) {
  float4* row = out + uint64_t(blockIdx.y) * words;
  for (uint64_t i = uint64_t(blockIdx.x) * kSweepThreads + threadIdx.x; i < words; i += uint64_t(gridDim.x) * kSweepThreads) {
    const uint64_t j = 2 * i, g = j >> 6;
    uint32_t c[4] = {uint32_t(g), uint32_t(g >> 32), first_state + blockIdx.y, kRandomStatesTag};
    philox4x32_10(c, uint32_t(seed), uint32_t(seed >> 32));
    const uint32_t b = 2u * uint32_t(j & 63u);          // four consecutive bits of the 128, inside one word (b % 4 == 0)
    const uint32_t bits = c[b >> 5] >> (b & 31u);
    row[i] = make_float4(bits & 1u ? -mag : mag, bits & 2u ? -mag : mag, bits & 4u ? -mag : mag, bits & 8u ? -mag : mag);
  }
}

}  // namespace

hipError_t launch_cheb_step(bool first, bool with_norm, const float2* w, float2* tprev, float2* acc, uint32_t n_eff, uint32_t c,
                            float2 c0, float2 coef, const double* scale, double* parts, hipStream_t stream) {
  if (n_eff < 1 || c == 0 || c > 65535u || (first && !scale) || (with_norm && !parts)) return hipErrorInvalidValue;
  const uint64_t words = uint64_t(1) << (n_eff - 1);
  const dim3 grid(sweep_slices(words), c), block(kSweepThreads);
  const float4* w4 = reinterpret_cast<const float4*>(w);
  float4 *t4 = reinterpret_cast<float4*>(tprev), *a4 = reinterpret_cast<float4*>(acc);
  if (first && with_norm) hipLaunchKernelGGL((cheb_step_kernel<true, true>), grid, block, 0, stream, w4, t4, a4, words, c0, coef, scale, parts);
  else if (first) hipLaunchKernelGGL((cheb_step_kernel<true, false>), grid, block, 0, stream, w4, t4, a4, words, c0, coef, scale, parts);
  else if (with_norm) hipLaunchKernelGGL((cheb_step_kernel<false, true>), grid, block, 0, stream, w4, t4, a4, words, c0, coef, scale, parts);
  else hipLaunchKernelGGL((cheb_step_kernel<false, false>), grid, block, 0, stream, w4, t4, a4, words, c0, coef, scale, parts);
  return hipGetLastError();
}

hipError_t launch_finish_step(const double* parts, uint32_t n_eff, uint32_t c, double x, double* log_norm, double* scale,
                              const double* wr, uint32_t n_ops, float* up1, hipStream_t stream) {
  if (n_eff < 1 || c == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(finish_step_kernel, dim3(c), dim3(kSweepThreads), 0, stream, parts, sweep_slices(uint64_t(1) << (n_eff - 1)), x,
                     log_norm, scale, wr, n_ops, up1);
  return hipGetLastError();
}

hipError_t launch_evolve_init(uint32_t c, const double* norm2, double* log_norm, double* scale, const double* wr, uint32_t n_ops,
                              float* up1, float* up2, hipStream_t stream) {
  const uint64_t count = std::max<uint64_t>(c, uint64_t(c) * n_ops);
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(evolve_init_kernel, dim3(unsigned((count + kSweepThreads - 1) / kSweepThreads)), dim3(kSweepThreads), 0, stream, c,
                     norm2, log_norm, scale, wr, n_ops, up1, up2);
  return hipGetLastError();
}

hipError_t launch_random_states(float2* out, uint32_t n_states, uint32_t n, uint64_t seed, uint32_t first_state,
                                hipStream_t stream) {
  if (n < 1 || n > 40) return hipErrorInvalidValue;
  // each part: 2^{-(n + 1) / 2}, from exact powers of two and one correctly rounded square root
  const float mag = float(std::ldexp((n + 1) % 2 ? std::sqrt(0.5) : 1.0, -int((n + 1) / 2)));
  const uint64_t words = uint64_t(1) << (n - 1);
  for (uint32_t r0 = 0; r0 < n_states; r0 += 65535u) {  // (the state is a grid dimension)
    const uint32_t rows = std::min<uint32_t>(65535u, n_states - r0);
    hipLaunchKernelGGL(random_states_kernel, dim3(sweep_slices(words), rows), dim3(kSweepThreads), 0, stream,
                       reinterpret_cast<float4*>(out) + uint64_t(r0) * words, words, seed, first_state + r0, mag);
  }
  return hipGetLastError();
}

}  // namespace qhbm
