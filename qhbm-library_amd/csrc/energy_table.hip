// energy_table.hip -- a diagonal observable given as a TABLE of energies, E = sum_y E[y] |y><y| (gfx950).
//
// A general BitstringEnergy (an MLP on the bits, qhbmlib/models/energy.py) is no Pauli sum; its modular Hamiltonian is
// still diagonal, and over the final states in the workspace it needs one streaming pass:
//   VALUES      v_u = sum_y E[y] |psi_u[y]|^2                                   (nothing stored)
//   LAMBDA      lambda_u[y] = up_u E[y] psi_u[y] into the engine's lambda buffer, v_u from the same launch
//   TABLE_GRAD  g[y] += sum_u up_u |psi_u[y]|^2 (with LAMBDA), fp64 across chunks, in an order fixed by global state index
//
// Shape: a 2-D grid.  blockIdx.x is a y-BLOCK of 2^10 amplitudes (256 threads x 4: two 16-byte loads of two amplitudes
// each, y = 2 t + {0, 1} + 512 k); blockIdx.y is a GROUP of 2^gb consecutive GLOBAL state indices (gb from n_eff only,
// table_group_bits) intersected with the chunk.  The block reads its 1024 table entries once into registers and walks the
// states of its group.  Small n still fills the chip: n = 12 with 1024 states is 4 y-blocks x 128 groups.
//
// Determinism (no floating-point atomics; nothing depends on chunk_states):
//  * v_u: per thread an fp64 sum over its 4 amplitudes, a fixed xor butterfly over the wave, the 4 waves of the block in
//    order -> part[u, y-block]; table_values_finish adds the y-blocks of a state in order.  The y-decomposition depends
//    on n_eff alone.
//  * g[y]: within a group a left fold over its states in state order, in fp64, starting from 0 -- or, for a group a
//    chunk boundary cut, from the carry its earlier part left; table_grad_finish adds every COMPLETE group's fold to the
//    running fp64 sum in group order and keeps an incomplete one as the carry.  So g = sum over groups (in order) of
//    folds (in state order) whatever the chunks.
// Padding (n < 10: n_eff = 10): indices y >= 2^n read no table entry, add nothing, and get lambda = 0 -- the backward
// sweep reads the whole padded state and the workspace may hold another call's amplitudes there.
#include "kernels.h"

namespace qhbm {
namespace {

constexpr int kTabThreads = 256;
constexpr int kTabBlockBits = 10;       // amplitudes per y-block
constexpr int kTabMaxGroupBits = 6;     // states per group <= 64 (the per-state wave partials sit in LDS)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);  // every lane ends with the same bits (a + b == b + a)
  return v;
}

template <bool kLambda, bool kGrad>
__global__ __launch_bounds__(kTabThreads) void energy_table_kernel(
    const float2* __restrict__ psi, float2* __restrict__ lam, const float* __restrict__ table, uint32_t n,
    uint32_t n_eff, uint32_t c, uint32_t s0, uint32_t gb, const float* __restrict__ upstream,
    double* __restrict__ vpart, double* __restrict__ gpart, const double* __restrict__ carry) {
  __shared__ double wpart[1 << kTabMaxGroupBits][kTabThreads / 64];
  const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
  const uint32_t yb = blockIdx.x, nb = gridDim.x;
  const uint32_t j = (s0 >> gb) + blockIdx.y;  // global group index
  const uint32_t u_begin = max(j << gb, s0), u_end = min((j + 1u) << gb, s0 + c);
  const size_t dim = size_t(1) << n;
  const size_t y0 = (size_t(yb) << kTabBlockBits) + 2u * t;  // amplitudes y0, y0 + 1 and y0 + 512, y0 + 513
  bool ok[4];
  float e[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const size_t y = y0 + size_t(k >> 1) * 512u + size_t(k & 1);
    ok[k] = y < dim;
    e[k] = ok[k] ? table[y] : 0.f;
  }
  double g[4] = {0.0, 0.0, 0.0, 0.0};
  if (kGrad && u_begin > (j << gb)) {  // the group began in an earlier chunk: continue its fold
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (ok[k]) g[k] = carry[y0 + size_t(k >> 1) * 512u + size_t(k & 1)];
  }
  const size_t blk = size_t(yb) << (kTabBlockBits - 1);  // y-block offset in float4 (two amplitudes) units
  auto step = [&](uint32_t u, float4 a, float4 b) {
    float4 v4[2] = {a, b};
    float p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float re = (k & 1) ? v4[k >> 1].z : v4[k >> 1].x, im = (k & 1) ? v4[k >> 1].w : v4[k >> 1].y;
      re = ok[k] ? re : 0.f;
      im = ok[k] ? im : 0.f;
      if (k & 1) { v4[k >> 1].z = re; v4[k >> 1].w = im; } else { v4[k >> 1].x = re; v4[k >> 1].y = im; }
      p[k] = fmaf(re, re, im * im);
    }
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v = fma(double(e[k]), double(p[k]), v);
    v = wave_sum_f64(v);
    if (lane == 0) wpart[u - u_begin][wave] = v;
    if (kLambda) {
      const float w = upstream[u];
      float f[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) f[k] = w * e[k];
      float4* dst = reinterpret_cast<float4*>(lam + (size_t(u - s0) << n_eff)) + blk;
      dst[t] = make_float4(v4[0].x * f[0], v4[0].y * f[0], v4[0].z * f[1], v4[0].w * f[1]);
      dst[t + 256] = make_float4(v4[1].x * f[2], v4[1].y * f[2], v4[1].z * f[3], v4[1].w * f[3]);
      if (kGrad) {
        const double wd = double(w);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = fma(wd, double(p[k]), g[k]);
      }
    }
  };
  // four states' loads in flight before the first is used
  uint32_t u = u_begin;
  for (; u + 4 <= u_end; u += 4) {
    float4 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4* src = reinterpret_cast<const float4*>(psi + (size_t(u + i - s0) << n_eff)) + blk;
      a[i] = src[t];
      b[i] = src[t + 256];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) step(u + i, a[i], b[i]);
  }
  for (; u < u_end; ++u) {
    const float4* src = reinterpret_cast<const float4*>(psi + (size_t(u - s0) << n_eff)) + blk;
    step(u, src[t], src[t + 256]);
  }
  if (kGrad) {
    double* dst = gpart + size_t(blockIdx.y) * dim;
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
      const size_t y = y0 + size_t(k >> 1) * 512u;
      if (ok[k] && ok[k + 1]) *reinterpret_cast<double2*>(dst + y) = make_double2(g[k], g[k + 1]);
      else if (ok[k]) dst[y] = g[k];
    }
  }
  __syncthreads();
  if (t < u_end - u_begin) {
    double v = wpart[t][0];
#pragma unroll
    for (int w = 1; w < kTabThreads / 64; ++w) v += wpart[t][w];
    vpart[size_t(u_begin + t - s0) * nb + yb] = v;
  }
}

// out[s0 + i] = sum over the y-blocks (in order) of state i's partials: one wave per state.
__global__ __launch_bounds__(256) void table_values_finish_kernel(const double* __restrict__ vpart, uint32_t nb, uint32_t c,
                                                                  uint32_t s0, float* __restrict__ out) {
  const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  if (i >= c) return;
  double v = 0.0;
  for (uint32_t b = lane; b < nb; b += 64u) v += vpart[size_t(i) * nb + b];
  v = wave_sum_f64(v);
  if (lane == 0) out[s0 + i] = float(v);
}

// Every group of the chunk whose states all lie in [0, s0 + c) (or [0, U)) is complete: its fold goes onto the running
// sum, in group order; the last group of a chunk that ends inside it is kept as the carry of the next chunk.
__global__ __launch_bounds__(256) void table_grad_finish_kernel(const double* __restrict__ gpart, uint32_t n_groups, size_t dim,
                                                                uint32_t s0, uint32_t c, uint32_t U, uint32_t gb,
                                                                double* __restrict__ gsum, double* __restrict__ carry) {
  const size_t y = size_t(blockIdx.x) * 256u + threadIdx.x;
  if (y >= dim) return;
  double acc = gsum[y];
  for (uint32_t jl = 0; jl < n_groups; ++jl) {
    const uint32_t j = (s0 >> gb) + jl;
    const uint32_t end = min((j + 1u) << gb, U);
    const double part = gpart[size_t(jl) * dim + y];
    if (end <= s0 + c) acc += part;
    else carry[y] = part;
  }
  gsum[y] = acc;
}

}  // namespace

uint32_t table_group_bits(uint32_t n_eff) {
  // 4 states per group at n_eff = 10 up to 64 from 15: enough groups to fill the chip at small n, few partial folds
  // (2/2^gb of the state traffic in TABLE_GRAD mode) at large n
  return std::min<uint32_t>(kTabMaxGroupBits, std::max<uint32_t>(2u, n_eff - 8u));
}

uint32_t table_groups(uint32_t s0, uint32_t c, uint32_t n_eff) {
  const uint32_t gb = table_group_bits(n_eff);
  return c ? ((s0 + c - 1u) >> gb) - (s0 >> gb) + 1u : 0u;
}

hipError_t launch_energy_table(int mode, const float2* psi, float2* lam, const float* table, uint32_t n, uint32_t n_eff,
                               uint32_t c, uint32_t s0, uint32_t U, const float* upstream, double* vpart, float* d_out,
                               double* gpart, double* carry, double* gsum, hipStream_t stream) {
  if (!c) return hipSuccess;
  if (n_eff < uint32_t(kTabBlockBits) || n > n_eff) return hipErrorInvalidValue;
  const uint32_t gb = table_group_bits(n_eff), nb = 1u << (n_eff - kTabBlockBits);
  const dim3 grid(nb, table_groups(s0, c, n_eff));
  if (grid.y > 65535u) return hipErrorInvalidValue;
  if (mode == TABLE_VALUES)
    hipLaunchKernelGGL((energy_table_kernel<false, false>), grid, dim3(kTabThreads), 0, stream, psi, lam, table, n, n_eff, c,
                       s0, gb, upstream, vpart, gpart, carry);
  else if (mode == TABLE_LAMBDA)
    hipLaunchKernelGGL((energy_table_kernel<true, false>), grid, dim3(kTabThreads), 0, stream, psi, lam, table, n, n_eff, c,
                       s0, gb, upstream, vpart, gpart, carry);
  else if (mode == TABLE_LAMBDA_GRAD)
    hipLaunchKernelGGL((energy_table_kernel<true, true>), grid, dim3(kTabThreads), 0, stream, psi, lam, table, n, n_eff, c,
                       s0, gb, upstream, vpart, gpart, carry);
  else
    return hipErrorInvalidValue;
  if (hipError_t e = hipGetLastError()) return e;
  if (d_out) {
    hipLaunchKernelGGL(table_values_finish_kernel, dim3((c + 3u) / 4u), dim3(256), 0, stream, vpart, nb, c, s0, d_out);
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (mode == TABLE_LAMBDA_GRAD) {
    const size_t dim = size_t(1) << n;
    hipLaunchKernelGGL(table_grad_finish_kernel, dim3(unsigned((dim + 255) / 256)), dim3(256), 0, stream, gpart, grid.y, dim,
                       s0, c, U, gb, gsum, carry);
    if (hipError_t e = hipGetLastError()) return e;
  }
  return hipSuccess;
}

}  // namespace qhbm
