// krylov.hip -- Lanczos bases of caller-supplied states under H = sum_k w_k O_k, and sums over a stored basis (gfx950).
//
// qhbm_krylov_basis builds, per start state phi, v_0 = phi / ||phi||, and for j = 0 .. m - 1 (engine.cpp)
//   w = H v_j                                      (the observable kernels, run_observable_chunk)
//   c_i = <v_i, w>, i in [lo, j];  w -= sum_i c_i v_i   (one round; full reorthogonalisation: lo = 0, two rounds)
//   alpha_j = sum over rounds of Re c_j,  beta_j = ||w||,  v_{j+1} = w / beta_j
// into a STEP-MAJOR basis [m, U, 2^n]: row j of a chunk of consecutive states is contiguous.  What is here:
//   krylov_project_kernel<NB>    part[state, k, slice] = sum over the slice of conj(v_{i0+k}) w, k < NB <= 8, complex fp64:
//                                one sweep over w serves NB rows                                       1 + NB reads
//   krylov_coef_kernel           c_k = the state's partials in slice order; complex64 into coef[state, i0 + k - lo];
//                                alpha_j += Re c_j where row j is in the block
//   krylov_subtract_kernel<NB>   w -= sum_k c_k v_{i0+k}, k ascending, fp32                            1 + NB reads, 1 write
//     <NB, true>                 ... and part[state, slice] = sum |w|^2 of the slice, fp64 (last block of the last round)
//   krylov_norm_kernel           beta_j = sqrt(partials in slice order); beta_j <= threshold: the space is exhausted --
//                                length = j + 1, beta_j = 0, scale = 0, and scale 0 is sticky: every later w is H 0 = 0,
//                                every later row, alpha and beta an exact zero; else scale = 1 / beta_j
//   krylov_init_kernel           scale = 1, length = m (norm 0: scale 0, length 0) from the import's squared norms
//   krylov_combine_kernel<SB>    out[u, s0 + s] = sum_j coef[u, s0 + s, j] basis[j, u], j ascending, fp32, s < SB <= 8:
//                                every basis word is read once for SB outputs held in registers        m reads, SB writes
//   krylov_replay_kernel<SB, FIRST>  the scaled copy of a step of qhbm_krylov_replay, which also accumulates:
//                                v_{j+1} = w * scale over v_{j-1}, w as krylov_subtract_kernel left it from RECORDED
//                                coefficients, and out_s += coef[s, j + 1] v_{j+1}, SB <= 8 outputs  1 + SB reads, 1 + SB writes
// v_{j+1} = w * scale is import_states.hip's launch_scale_copy_states (1 read, 1 write), which also takes w from the
// workspace's pitch to the caller's.
//
// Shape (state_sweep.h): 16-byte words, blockIdx.y = the state, blockIdx.x = a slice of 1024 words, 256 threads x 4 words,
// the grid a function of n alone.  A thread adds its words in word order, a wave's 64 lanes meet in a fixed shuffle tree,
// the four waves in wave order, the slices in slice order through sweep_row_sum(2): no floating-point atomics, and nothing
// depends on chunk_states or on which other states share the call.
//
// (a translation unit of its own in the source tree, compiled as part of states.hip; it uses no name of another .hip file)
#include <algorithm>

#include "kernels.h"
#include "state_sweep.h"

namespace qhbm {
namespace {

// w: the chunk's states at a pitch of w_pitch words; rows: basis row i0 of the chunk's first state, `row_stride` words
// from one basis row to the next, `words` words per state; part [c, 8, 2, gridDim.x]
template <uint32_t NB>
__global__ __launch_bounds__(kSweepThreads) void krylov_project_kernel(const float4* __restrict__ w, uint64_t w_pitch,
                                                                       const float4* __restrict__ rows, uint64_t row_stride,
                                                                       uint64_t words, double* __restrict__ part) {
  __shared__ double sh[kSweepThreads / 64][2 * NB];
  const float4* wr = w + uint64_t(blockIdx.y) * w_pitch;
  const float4* vr = rows + uint64_t(blockIdx.y) * words;
  double re[NB], im[NB];
#pragma unroll
  for (uint32_t k = 0; k < NB; ++k) re[k] = im[k] = 0.0;
  for (uint64_t i = uint64_t(blockIdx.x) * kSweepThreads + threadIdx.x; i < words; i += uint64_t(gridDim.x) * kSweepThreads) {
    const float4 a = wr[i];
#pragma unroll
    for (uint32_t k = 0; k < NB; ++k) {
      const float4 v = vr[uint64_t(k) * row_stride + i];
      re[k] += (double(v.x) * double(a.x) + double(v.y) * double(a.y)) + (double(v.z) * double(a.z) + double(v.w) * double(a.w));
      im[k] += (double(v.x) * double(a.y) - double(v.y) * double(a.x)) + (double(v.z) * double(a.w) - double(v.w) * double(a.z));
    }
  }
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (uint32_t k = 0; k < NB; ++k) {
    const double r = sweep_wave_sum(re[k]), s = sweep_wave_sum(im[k]);
    if (lane == 0) {
      sh[wave][2 * k] = r;
      sh[wave][2 * k + 1] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x < 2 * NB) {
    double total = sh[0][threadIdx.x];
    for (uint32_t v = 1; v < kSweepThreads / 64; ++v) total += sh[v][threadIdx.x];
    part[(uint64_t(blockIdx.y) * 2 * kKrylovBlock + threadIdx.x) * gridDim.x + blockIdx.x] = total;
  }
}

// One workgroup per state of the chunk.  coef [c, coef_pitch]: the round's coefficients, row i at i - lo; the block's
// rows are first .. first + nb.  alpha_at >= 0: the block's row alpha_at is row j -- alpha[state] += Re c_j.
__global__ __launch_bounds__(kSweepThreads) void krylov_coef_kernel(const double* __restrict__ part, uint32_t slices, uint32_t nb,
                                                                    float2* __restrict__ coef, uint32_t coef_pitch, uint32_t first,
                                                                    int alpha_at, double* __restrict__ alpha, uint64_t alpha_pitch) {
  __shared__ double sh[kSweepThreads];
  for (uint32_t k = 0; k < nb; ++k) {
    const double2 c = sweep_row_sum2(part + (uint64_t(blockIdx.x) * 2 * kKrylovBlock + 2 * k) * slices, slices, sh);
    __syncthreads();
    if (threadIdx.x == 0) {
      coef[uint64_t(blockIdx.x) * coef_pitch + first + k] = make_float2(float(c.x), float(c.y));
      if (int(k) == alpha_at) alpha[uint64_t(blockIdx.x) * alpha_pitch] += c.x;
    }
  }
}

// coef: the state's coefficients of the block's rows (coef_pitch float2 per state); norm_part [c, gridDim.x]
template <uint32_t NB, bool NORM>
__global__ __launch_bounds__(kSweepThreads) void krylov_subtract_kernel(float4* __restrict__ w, uint64_t w_pitch,
                                                                        const float4* __restrict__ rows, uint64_t row_stride,
                                                                        uint64_t words, const float2* __restrict__ coef,
                                                                        uint32_t coef_pitch, double* __restrict__ norm_part) {
  __shared__ double sh[NORM ? kSweepThreads : 1];
  float4* wr = w + uint64_t(blockIdx.y) * w_pitch;
  const float4* vr = rows + uint64_t(blockIdx.y) * words;
  float2 c[NB];
#pragma unroll
  for (uint32_t k = 0; k < NB; ++k) c[k] = coef[uint64_t(blockIdx.y) * coef_pitch + k];
  double sum = 0.0;
  for (uint64_t i = uint64_t(blockIdx.x) * kSweepThreads + threadIdx.x; i < words; i += uint64_t(gridDim.x) * kSweepThreads) {
    float4 a = wr[i];
#pragma unroll
    for (uint32_t k = 0; k < NB; ++k) {
      const float4 d = sweep_cmul(c[k], vr[uint64_t(k) * row_stride + i]);
      a = make_float4(a.x - d.x, a.y - d.y, a.z - d.z, a.w - d.w);
    }
    wr[i] = a;
    if (NORM) sum += word_norm2(a);
  }
  if (NORM) {
    const double total = sweep_block_sum(sum, sh);
    if (threadIdx.x == 0) norm_part[uint64_t(blockIdx.y) * gridDim.x + blockIdx.x] = total;
  }
}

// One workgroup per state of the chunk; beta, lengths: the chunk's first state, beta at step j of a row of beta_pitch.
__global__ __launch_bounds__(kSweepThreads) void krylov_norm_kernel(const double* __restrict__ norm_part, uint32_t slices,
                                                                    double threshold, int j, double* __restrict__ beta,
                                                                    uint64_t beta_pitch, int32_t* __restrict__ lengths,
                                                                    double* __restrict__ scale) {
  __shared__ double sh[kSweepThreads];
  const double norm = sqrt(sweep_row_sum(norm_part + uint64_t(blockIdx.x) * slices, slices, sh));
  if (threadIdx.x == 0) {
    double b = 0.0, sc = 0.0;
    if (scale[blockIdx.x] != 0.0) {  // (0: exhausted at an earlier step, or a start state of norm 0)
      if (norm <= threshold) {
        lengths[blockIdx.x] = j + 1;
      } else {
        b = norm;
        sc = 1.0 / norm;
      }
    }
    beta[uint64_t(blockIdx.x) * beta_pitch + uint64_t(j)] = b;
    scale[blockIdx.x] = sc;
  }
}

__global__ __launch_bounds__(kSweepThreads) void krylov_init_kernel(uint32_t c, const double* __restrict__ norm2, int m,
                                                                    int32_t* __restrict__ lengths, double* __restrict__ scale) {
  const uint32_t i = blockIdx.x * kSweepThreads + threadIdx.x;
  if (i < c) {
    const bool live = norm2[i] > 0.0;
    scale[i] = live ? 1.0 : 0.0;
    lengths[i] = live ? m : 0;
  }
}

// basis: row 0 of state u0 (blockIdx.y = u - u0), row_stride words between rows; coef: [., S, m] at state u0, output s0;
// out: [., S, words] at state u0, output s0
template <uint32_t SB>
__global__ __launch_bounds__(kSweepThreads) void krylov_combine_kernel(const float4* __restrict__ basis, uint64_t row_stride,
                                                                       uint64_t words, uint32_t m, const float2* __restrict__ coef,
                                                                       uint32_t S, float4* __restrict__ out) {
  const float4* vr = basis + uint64_t(blockIdx.y) * words;
  const float2* cf = coef + uint64_t(blockIdx.y) * S * m;
  float4* o = out + uint64_t(blockIdx.y) * S * words;
#pragma unroll 1
  for (uint64_t i = uint64_t(blockIdx.x) * kSweepThreads + threadIdx.x; i < words; i += uint64_t(gridDim.x) * kSweepThreads) {
    float4 acc[SB];
#pragma unroll
    for (uint32_t s = 0; s < SB; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 2
    for (uint32_t j = 0; j < m; ++j) {
      const float4 v = vr[uint64_t(j) * row_stride + i];
#pragma unroll
      for (uint32_t s = 0; s < SB; ++s) {
        const float4 d = sweep_cmul(cf[uint64_t(s) * m + j], v);
        acc[s] = make_float4(acc[s].x + d.x, acc[s].y + d.y, acc[s].z + d.z, acc[s].w + d.w);
      }
    }
#pragma unroll
    for (uint32_t s = 0; s < SB; ++s) o[uint64_t(s) * words + i] = acc[s];
  }
}

// The scaled copy of a replayed step (qhbm_krylov_replay), which also accumulates: w = H v_j - c_{j-1} v_{j-1} - c_j v_j as
// krylov_subtract_kernel left it, vnext (v_{j-1} on entry) and, FIRST only, vcur = v_0, all at a pitch of `pitch` words, the
// first `words` of them the state; beta: the step's beta_j of the chunk's first state; cf: coef[., s0, 0] and o:
// out[., s0, 0] of the chunk's first state.
//   vnext = v_{j+1} = float(double(w) f), f = 1 / beta_j or 0 where beta_j = 0 (krylov_norm_kernel's scale; the expression
//   is scale_copy_kernel's); zeros in the padding;  out_s += coef[s, j + 1] v_{j+1}, s < SB          1 + SB reads, 1 + SB writes
// FIRST (j = 0): out_s starts as coef[s, 0] v_0 + coef[s, 1] v_1 -- no zero fill                      2 reads, 1 + SB writes
template <uint32_t SB, bool FIRST>
__global__ __launch_bounds__(kSweepThreads) void krylov_replay_kernel(const float4* __restrict__ w, const float4* __restrict__ vcur,
                                                                      float4* __restrict__ vnext, uint64_t pitch, uint64_t words,
                                                                      const double* __restrict__ beta, uint64_t beta_pitch,
                                                                      const float2* __restrict__ coef, uint32_t m, uint32_t S,
                                                                      uint32_t j, float4* __restrict__ out) {
  const float4* wr = w + uint64_t(blockIdx.y) * pitch;
  const float4* vc = vcur + uint64_t(blockIdx.y) * pitch;
  float4* vn = vnext + uint64_t(blockIdx.y) * pitch;
  const float2* cf = coef + uint64_t(blockIdx.y) * S * m;
  float4* o = out + uint64_t(blockIdx.y) * S * words;
  const double b = beta[uint64_t(blockIdx.y) * beta_pitch];
  const double f = b != 0.0 ? 1.0 / b : 0.0;
  float2 t0[SB], t1[SB];
#pragma unroll
  for (uint32_t s = 0; s < SB; ++s) {
    t0[s] = cf[uint64_t(s) * m];  // (FIRST only)
    t1[s] = cf[uint64_t(s) * m + j + 1];
  }
  for (uint64_t i = uint64_t(blockIdx.x) * kSweepThreads + threadIdx.x; i < pitch; i += uint64_t(gridDim.x) * kSweepThreads) {
    if (i >= words) {  // (the workspace's padding: idle qubits stay |0>)
      vn[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const float4 a = wr[i];
    const float4 v = make_float4(float(double(a.x) * f), float(double(a.y) * f), float(double(a.z) * f), float(double(a.w) * f));
    vn[i] = v;
    float4 v0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (FIRST) v0 = vc[i];
#pragma unroll
    for (uint32_t s = 0; s < SB; ++s) {
      float4 acc;
      if (FIRST) {
        const float4 d = sweep_cmul(t0[s], v0);
        acc = make_float4(0.f + d.x, 0.f + d.y, 0.f + d.z, 0.f + d.w);  // (krylov_combine_kernel starts its sum at zero)
      } else {
        acc = o[uint64_t(s) * words + i];
      }
      const float4 d = sweep_cmul(t1[s], v);
      o[uint64_t(s) * words + i] = make_float4(acc.x + d.x, acc.y + d.y, acc.z + d.z, acc.w + d.w);
    }
  }
}

template <uint32_t NB>
void kry_launch_project(dim3 grid, hipStream_t stream, const float4* w, uint64_t w_pitch, const float4* rows, uint64_t row_stride,
                        uint64_t words, double* part) {
  hipLaunchKernelGGL((krylov_project_kernel<NB>), grid, dim3(kSweepThreads), 0, stream, w, w_pitch, rows, row_stride, words, part);
}

template <uint32_t NB>
void kry_launch_subtract(bool norm, dim3 grid, hipStream_t stream, float4* w, uint64_t w_pitch, const float4* rows,
                         uint64_t row_stride, uint64_t words, const float2* coef, uint32_t coef_pitch, double* norm_part) {
  if (norm)
    hipLaunchKernelGGL((krylov_subtract_kernel<NB, true>), grid, dim3(kSweepThreads), 0, stream, w, w_pitch, rows, row_stride, words,
                       coef, coef_pitch, norm_part);
  else
    hipLaunchKernelGGL((krylov_subtract_kernel<NB, false>), grid, dim3(kSweepThreads), 0, stream, w, w_pitch, rows, row_stride, words,
                       coef, coef_pitch, norm_part);
}

template <uint32_t SB>
void kry_launch_combine(dim3 grid, hipStream_t stream, const float4* basis, uint64_t row_stride, uint64_t words, uint32_t m,
                        const float2* coef, uint32_t S, float4* out) {
  hipLaunchKernelGGL((krylov_combine_kernel<SB>), grid, dim3(kSweepThreads), 0, stream, basis, row_stride, words, m, coef, S, out);
}

template <uint32_t SB>
void kry_launch_replay(bool first, dim3 grid, hipStream_t stream, const float4* w, const float4* vcur, float4* vnext, uint64_t pitch,
                       uint64_t words, const double* beta, uint64_t beta_pitch, const float2* coef, uint32_t m, uint32_t S, uint32_t j,
                       float4* out) {
  if (first)
    hipLaunchKernelGGL((krylov_replay_kernel<SB, true>), grid, dim3(kSweepThreads), 0, stream, w, vcur, vnext, pitch, words, beta,
                       beta_pitch, coef, m, S, j, out);
  else
    hipLaunchKernelGGL((krylov_replay_kernel<SB, false>), grid, dim3(kSweepThreads), 0, stream, w, vcur, vnext, pitch, words, beta,
                       beta_pitch, coef, m, S, j, out);
}

#define KRY_DISPATCH(count, call) \
  switch (count) {                \
    case 1: call(1); break;       \
    case 2: call(2); break;       \
    case 3: call(3); break;       \
    case 4: call(4); break;       \
    case 5: call(5); break;       \
    case 6: call(6); break;       \
    case 7: call(7); break;       \
    case 8: call(8); break;       \
    default: return hipErrorInvalidValue; \
  }

}  // namespace

size_t krylov_coef_parts_count(uint32_t n, uint32_t c) { return size_t(c) * 2 * kKrylovBlock * sweep_slices(uint64_t(1) << (n - 1)); }

hipError_t launch_krylov_init(uint32_t c, const double* norm2, int m, int32_t* lengths, double* scale, hipStream_t stream) {
  if (!c) return hipSuccess;
  hipLaunchKernelGGL(krylov_init_kernel, dim3((c + kSweepThreads - 1) / kSweepThreads), dim3(kSweepThreads), 0, stream, c, norm2, m, lengths,
                     scale);
  return hipGetLastError();
}

hipError_t launch_krylov_project(const float2* w, uint32_t n_w, const float2* rows, int64_t row_stride_amps, uint32_t n, uint32_t c,
                                 uint32_t nb, double* parts, float2* coef, uint32_t coef_pitch, uint32_t first, int alpha_at,
                                 double* alpha, uint64_t alpha_pitch, hipStream_t stream) {
  if (n < 1 || n_w < n || c == 0 || c > 65535u || nb < 1 || nb > kKrylovBlock || first + nb > coef_pitch) return hipErrorInvalidValue;
  const uint64_t words = uint64_t(1) << (n - 1), w_pitch = uint64_t(1) << (n_w - 1);
  const uint32_t slices = sweep_slices(words);
  const dim3 grid(slices, c);
  const float4 *w4 = reinterpret_cast<const float4*>(w), *r4 = reinterpret_cast<const float4*>(rows);
#define KRY_CALL(NB) kry_launch_project<NB>(grid, stream, w4, w_pitch, r4, uint64_t(row_stride_amps / 2), words, parts)
  KRY_DISPATCH(nb, KRY_CALL)
#undef KRY_CALL
  hipLaunchKernelGGL(krylov_coef_kernel, dim3(c), dim3(kSweepThreads), 0, stream, parts, slices, nb, coef, coef_pitch, first, alpha_at,
                     alpha, alpha_pitch);
  return hipGetLastError();
}

hipError_t launch_krylov_subtract(float2* w, uint32_t n_w, const float2* rows, int64_t row_stride_amps, uint32_t n, uint32_t c,
                                  uint32_t nb, const float2* coef, uint32_t coef_pitch, double* norm_parts, hipStream_t stream) {
  if (n < 1 || n_w < n || c == 0 || c > 65535u || nb < 1 || nb > kKrylovBlock) return hipErrorInvalidValue;
  const uint64_t words = uint64_t(1) << (n - 1), w_pitch = uint64_t(1) << (n_w - 1);
  const dim3 grid(sweep_slices(words), c);
  float4* w4 = reinterpret_cast<float4*>(w);
  const float4* r4 = reinterpret_cast<const float4*>(rows);
#define KRY_CALL(NB) kry_launch_subtract<NB>(norm_parts != nullptr, grid, stream, w4, w_pitch, r4, uint64_t(row_stride_amps / 2), words, coef, coef_pitch, norm_parts)
  KRY_DISPATCH(nb, KRY_CALL)
#undef KRY_CALL
  return hipGetLastError();
}

hipError_t launch_krylov_norm(const double* norm_parts, uint32_t n, uint32_t c, double threshold, int j, double* beta,
                              uint64_t beta_pitch, int32_t* lengths, double* scale, hipStream_t stream) {
  if (n < 1 || c == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(krylov_norm_kernel, dim3(c), dim3(kSweepThreads), 0, stream, norm_parts, sweep_slices(uint64_t(1) << (n - 1)),
                     threshold, j, beta, beta_pitch, lengths, scale);
  return hipGetLastError();
}

hipError_t launch_krylov_combine(const float2* basis, uint32_t m, uint32_t U, uint32_t n, const float2* coef, uint32_t S,
                                 float2* out, hipStream_t stream) {
  if (n < 1 || n > 40 || m < 1 || U < 1 || S < 1) return hipErrorInvalidValue;
  const uint64_t words = uint64_t(1) << (n - 1);
  const float4* b4 = reinterpret_cast<const float4*>(basis);
  float4* o4 = reinterpret_cast<float4*>(out);
  for (uint32_t u0 = 0; u0 < U; u0 += 65535u) {  // (the state is a grid dimension)
    const dim3 grid(sweep_slices(words), std::min<uint32_t>(65535u, U - u0));
    for (uint32_t s0 = 0; s0 < S; s0 += kKrylovBlock) {
      const uint32_t sb = std::min<uint32_t>(kKrylovBlock, S - s0);
#define KRY_CALL(SB) kry_launch_combine<SB>(grid, stream, b4 + uint64_t(u0) * words, uint64_t(U) * words, words, m, \
                                            coef + (uint64_t(u0) * S + s0) * m, S, o4 + (uint64_t(u0) * S + s0) * words)
      KRY_DISPATCH(sb, KRY_CALL)
#undef KRY_CALL
    }
  }
  return hipGetLastError();
}

hipError_t launch_krylov_replay(uint32_t j, const float2* w, const float2* vcur, float2* vnext, uint32_t n, uint32_t n_eff,
                                uint32_t c, const double* beta, uint64_t beta_pitch, const float2* coef, uint32_t m, uint32_t S, uint32_t sb,
                                float2* out, hipStream_t stream) {
  if (n < 1 || n_eff < n || n_eff > 40 || c == 0 || c > 65535u || m < 2 || j + 1 >= m || sb < 1 || sb > S) return hipErrorInvalidValue;
  const uint64_t words = uint64_t(1) << (n - 1), pitch = uint64_t(1) << (n_eff - 1);
  const dim3 grid(sweep_slices(pitch), c);
  const float4 *w4 = reinterpret_cast<const float4*>(w), *c4 = reinterpret_cast<const float4*>(vcur);
  float4 *n4 = reinterpret_cast<float4*>(vnext), *o4 = reinterpret_cast<float4*>(out);
#define KRY_CALL(SB) kry_launch_replay<SB>(j == 0, grid, stream, w4, c4, n4, pitch, words, beta, beta_pitch, coef, m, S, j, o4)
  KRY_DISPATCH(sb, KRY_CALL)
#undef KRY_CALL
  return hipGetLastError();
}

#undef KRY_DISPATCH

}  // namespace qhbm
