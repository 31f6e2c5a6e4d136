// cotangent.hip -- a caller's cotangent of the final states as the lambda of the backward sweep (gfx950).
//
// qhbm_statevector_vjp_from_states differentiates a real loss L of the states psi_u = ||phi_u|| e^{i theta(p)} chi_u that
// qhbm_statevector_from_states returns, where chi_u is what the forward sweep leaves in the workspace (phi_u / ||phi_u||
// through the circuit, without the global phase) and g_u = dL/dRe psi_u + i dL/dIm psi_u is the caller's cotangent:
//   dL = sum_u Re<g_u|dpsi_u> = sum_u 2 Re<lambda_u|dchi_u> - dtheta sum_u Im<g_u|psi_u>,   lambda_u = 1/2 ||phi_u|| e^{-i theta} g_u.
// The first term is the backward sweep's on lambda (as on lambda = O psi); the second needs theta's constant slope
// (engine.cpp upload_model) and one number.  Per chunk of c states:
//   1. cotangent_import   lambda_i = 1/2 ||phi|| e^{-i theta} g at the workspace pitch, ZEROS in the padding whatever the
//                         workspace held; part[i, re / im, slice] = the slice's share of <g|chi>, fp64   (16 B read, 8 B written
//                         per amplitude: one streaming pass, HBM-bound)
//   2. cotangent_finish   dot[s0 + i] = <g|chi>, its slices in slice order
// and once per call, after launch_reduce_grad:
//   3. cotangent_phase_grad   S = sum_u ||phi_u|| Im(e^{i theta} <g_u|chi_u>) in state order, grad[p] -= slope[p] S
// The phase (cos, sin as float: the pair the exported states were multiplied by) and the squared norms are read on the
// device: no host synchronisation, a captured step stays capturable.
//
// Shape (state_sweep.h): 16-byte words, blockIdx.y the state, blockIdx.x a slice of 1024 words of the workspace row,
// consecutive threads on consecutive words.  Sums: a thread's four words in word order, the lanes of a wave in
// sweep_wave_sum's tree, the four waves in wave order, the slices through sweep_row_sum2, the states in state order by
// one thread: no floating-point atomics, nothing depends on chunk_states.  The products are float x float in double.
//
// (a translation unit of its own in the source tree, compiled as part of observable.hip beside the other producers of
// lambda; it uses no name of another .hip file)
#include "kernels.h"
#include "state_sweep.h"

namespace qhbm {
namespace {

constexpr uint32_t kCotWordsPerThread = kSweepSliceWords / kSweepThreads;

// words_in = 2^(n - 1), words_out = 2^(n_eff - 1) >= words_in; chi, lam: the chunk's states, element 0 first;
// part [c, 2, slices_in] (the slices behind the input hold padding only and have no partial)
__global__ __launch_bounds__(kSweepThreads) void cotangent_import(const float4* __restrict__ cot, const float4* __restrict__ chi,
                                                                  uint64_t words_in, uint64_t words_out, uint32_t s0,
                                                                  uint32_t slices_in, const double* __restrict__ norm2,
                                                                  const float* __restrict__ phase_cs, float4* __restrict__ lam,
                                                                  double* __restrict__ part) {
  __shared__ double sh[kSweepThreads / 64][2];
  const float4* g = cot + (uint64_t(s0) + blockIdx.y) * words_in;
  const float4* x = chi + uint64_t(blockIdx.y) * words_out;
  float4* out = lam + uint64_t(blockIdx.y) * words_out;
  const double f = 0.5 * sqrt(norm2[s0 + blockIdx.y]);
  const float2 z = make_float2(float(f * double(phase_cs[0])), float(-f * double(phase_cs[1])));  // 1/2 ||phi|| e^{-i theta}
  const uint64_t w0 = uint64_t(blockIdx.x) * kSweepSliceWords + threadIdx.x;
  float4 gv[kCotWordsPerThread], xv[kCotWordsPerThread];
#pragma unroll
  for (uint32_t k = 0; k < kCotWordsPerThread; ++k) {  // (every load in flight before the first use)
    const uint64_t w = w0 + uint64_t(k) * kSweepThreads;
    gv[k] = xv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (w < words_in) {
      gv[k] = g[w];
      xv[k] = x[w];
    }
  }
  double re = 0.0, im = 0.0;
#pragma unroll
  for (uint32_t k = 0; k < kCotWordsPerThread; ++k) {
    const uint64_t w = w0 + uint64_t(k) * kSweepThreads;
    if (w >= words_out) continue;
    out[w] = sweep_cmul(z, gv[k]);  // (zeros behind the input: gv is zero there)
    const double gx = double(gv[k].x), gy = double(gv[k].y), gz = double(gv[k].z), gw = double(gv[k].w);
    const double cx = double(xv[k].x), cy = double(xv[k].y), cz = double(xv[k].z), cw = double(xv[k].w);
    re = __builtin_fma(gx, cx, re);  // conj(g) chi
    re = __builtin_fma(gy, cy, re);
    re = __builtin_fma(gz, cz, re);
    re = __builtin_fma(gw, cw, re);
    im = __builtin_fma(gx, cy, im);
    im = __builtin_fma(-gy, cx, im);
    im = __builtin_fma(gz, cw, im);
    im = __builtin_fma(-gw, cz, im);
  }
  if (blockIdx.x >= slices_in) return;  // (workgroup-uniform: a slice of padding)
  re = sweep_wave_sum(re);
  im = sweep_wave_sum(im);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh[wave][0] = re;
    sh[wave][1] = im;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double total = sh[0][threadIdx.x];
    for (uint32_t w = 1; w < kSweepThreads / 64; ++w) total += sh[w][threadIdx.x];
    part[(uint64_t(blockIdx.y) * 2 + threadIdx.x) * slices_in + blockIdx.x] = total;
  }
}

// dot [U, 2]: <g_u|chi_u> of the chunk's states
__global__ __launch_bounds__(kSweepThreads) void cotangent_finish(const double* __restrict__ part, uint32_t slices, uint32_t s0,
                                                                  double* __restrict__ dot) {
  __shared__ double sh[kSweepThreads];
  const double2 d = sweep_row_sum2(part + uint64_t(blockIdx.x) * 2 * slices, slices, sh);
  if (threadIdx.x == 0) {
    dot[2 * (uint64_t(s0) + blockIdx.x)] = d.x;
    dot[2 * (uint64_t(s0) + blockIdx.x) + 1] = d.y;
  }
}

// grad[p] -= slope[p] sum_u Im<g_u|psi_u>, psi_u = ||phi_u|| e^{i theta} chi_u; the sum by every thread for itself, in
// state order (U is a batch size: a few thousand additions at most)
__global__ __launch_bounds__(256) void cotangent_phase_grad(const double* __restrict__ dot, const double* __restrict__ norm2, uint32_t U,
                                                            const float* __restrict__ phase_cs, const float* __restrict__ slope,
                                                            float* __restrict__ grad, uint32_t n_params) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= n_params) return;
  const float sl = slope[p];
  if (sl == 0.f) return;  // (no phase through this parameter, or switched off by the gradient mask: the entry keeps its bits)
  const double c = double(phase_cs[0]), s = double(phase_cs[1]);
  double total = 0.0;
  for (uint32_t u = 0; u < U; ++u) total += sqrt(norm2[u]) * (c * dot[2 * u + 1] + s * dot[2 * u]);
  grad[p] = float(double(grad[p]) - double(sl) * total);
}

}  // namespace

size_t cotangent_parts_count(uint32_t n, uint32_t c) { return size_t(c) * 2 * sweep_slices(uint64_t(1) << (n - 1)); }

hipError_t launch_cotangent_import(const float2* cot, const float2* chi, uint32_t n, uint32_t n_eff, uint32_t c, uint32_t s0,
                                   const double* norm2, const float* phase_cs, float2* lam, double* parts, double* dot,
                                   hipStream_t stream) {
  if (n < 1 || n_eff < n || c == 0 || c > 65535u) return hipErrorInvalidValue;
  const uint64_t words_in = uint64_t(1) << (n - 1), words_out = uint64_t(1) << (n_eff - 1);
  const uint32_t slices_in = sweep_slices(words_in), slices_out = sweep_slices(words_out);
  hipLaunchKernelGGL(cotangent_import, dim3(slices_out, c), dim3(kSweepThreads), 0, stream, reinterpret_cast<const float4*>(cot),
                     reinterpret_cast<const float4*>(chi), words_in, words_out, s0, slices_in, norm2, phase_cs,
                     reinterpret_cast<float4*>(lam), parts);
  hipLaunchKernelGGL(cotangent_finish, dim3(c), dim3(kSweepThreads), 0, stream, parts, slices_in, s0, dot);
  return hipGetLastError();
}

hipError_t launch_cotangent_phase_grad(const double* dot, const double* norm2, uint32_t U, const float* phase_cs, const float* slope,
                                       float* grad, uint32_t n_params, hipStream_t stream) {
  if (!n_params || !U) return hipSuccess;
  hipLaunchKernelGGL(cotangent_phase_grad, dim3((n_params + 255u) / 256u), dim3(256), 0, stream, dot, norm2, U, phase_cs, slope, grad,
                     n_params);
  return hipGetLastError();
}

}  // namespace qhbm
