// subsystem_apply.hip -- a dense 2^k x 2^k operator on k arbitrary qubits of every state of an ensemble (gfx950).
//
// qhbm_subsystem_apply writes out_m = scale_m (A (x) 1_env) phi_m for M complex64 states of 2^n amplitudes, a row-major
// complex64 operator A on the kept qubits of keep_mask (k <= 10) and float64 scales (NULL: 1), and optionally
// dots_m = <phi_m|(A (x) 1)|phi_m> taken before scaling -- engine.cpp, DESIGN.md 6m.  It is the cotangent of the states of a
// reduced density matrix (A = Gamma + Gamma^H, scale = the weights) and the weights' cotangent (1/2 Re dots).  The masks and
// deposits are rdm_index.h's, the launch plan subsystem_plan.h's.  What is here:
//   subsys_vector_kernel<K>        k <= 3: a thread holds all 2^k rows of four environment values in registers, the operator
//                                  sits in LDS and is read as broadcasts, once per four values; fmaf chains in a' order.
//                                  One streaming pass: 16 B per amplitude.
//   subsys_transpose_kernel        k >= 4: the operator into two float planes [a'][a] at the head of the scratch, so that
//                                  a stage's operator tile is read along a (coalesced) and stored to LDS without conflicts
//   subsys_matrix_kernel<STRIPS, TK>  k >= 4: a workgroup owns a tile of 16 STRIPS rows by 64 environment values of one
//                                  state and walks a' in stages of TK: the operator tile and the gathered state panel go to
//                                  LDS as re / im planes [a'][row], [a'][column] (the next stage's words are in registers
//                                  while this one is multiplied), and wave w multiplies its 16 columns by every row strip on
//                                  v_mfma_f32_16x16x4_f32 in the real embedding Re = A_r phi_r - A_i phi_i,
//                                  Im = A_r phi_i + A_i phi_r: four instructions per strip and four a'.  Neither operand is
//                                  resident: per stage a workgroup reads 16 TK (STRIPS + 4) complex numbers for
//                                  64 STRIPS TK 64 flop.  The state panel is re-read 2^k / (16 STRIPS) times (once per
//                                  row tile), the operator once per column tile and state.
//   subsys_dots_finish             dots[m] = its partials in slice order
// Order of additions.  An output is an f32 fused-multiply-add chain over a' ascending (the matrix instruction is bit for bit
// such a chain): per a', A_r phi_r then -A_i phi_i for the real part (vector kernel), or per four a' the four products of
// A_r phi_r then the four of -A_i phi_i (matrix kernel); the imaginary part likewise.  dots: conj(phi) times the unscaled
// f32 output, float x float in double (exact), a thread's elements in the order it produces them (rows ascending), the 64
// lanes of a wave in sweep_wave_sum's tree, the four waves in wave order, the slices through sweep_row_sum2: no
// floating-point atomics, and the grid is a function of (n, keep_mask, M) alone.
//
// (a translation unit of its own in the source tree, compiled as part of observable.hip beside cotangent.hip, whose consumer
// it feeds; it uses no name of another .hip file)
#include "kernels.h"
#include "state_sweep.h"
#include "subsystem_plan.h"

namespace qhbm {
namespace {

typedef float sub_f32x4 __attribute__((ext_vector_type(4)));

struct SubArgs {
  uint32_t n, k, M, env_values, row_tiles, slices;
  uint32_t keep, env;
};

// conj(phi) v into (re, im), float x float in double
__device__ __forceinline__ void sub_dot_add(float2 phi, float vr, float vi, double* re, double* im) {
  *re = __builtin_fma(double(phi.x), double(vr), *re);
  *re = __builtin_fma(double(phi.y), double(vi), *re);
  *im = __builtin_fma(double(phi.x), double(vi), *im);
  *im = __builtin_fma(-double(phi.y), double(vr), *im);
}

// the workgroup's share of <phi|A phi>: lanes, then waves in wave order; red: [4][2] doubles of LDS
__device__ __forceinline__ void sub_store_partial(double re, double im, double (*red)[2], uint32_t m, uint32_t slices,
                                                  uint32_t slice, double* __restrict__ part) {
  re = sweep_wave_sum(re);
  im = sweep_wave_sum(im);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = re;
    red[wave][1] = im;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double total = red[0][threadIdx.x];
    for (uint32_t w = 1; w < kSubThreads / 64; ++w) total += red[w][threadIdx.x];
    part[(uint64_t(m) * 2 + threadIdx.x) * slices + slice] = total;
  }
}

template <uint32_t K>
__global__ __launch_bounds__(kSubThreads) void subsys_vector_kernel(const float2* __restrict__ states, const float2* __restrict__ op,
                                                                   const double* __restrict__ scale, SubArgs a,
                                                                   float2* __restrict__ out, double* __restrict__ part) {
  constexpr uint32_t D = 1u << K, V = kSubVecValues;
  __shared__ float2 sop[D * D];
  __shared__ double red[kSubThreads / 64][2];
  const uint32_t tid = threadIdx.x;
  const uint32_t m = blockIdx.z * kSubGridY + blockIdx.y;
  if (m >= a.M) return;  // (workgroup-uniform)
  for (uint32_t i = tid; i < D * D; i += kSubThreads) sop[i] = op[i];
  uint32_t rowdep[D];
#pragma unroll
  for (uint32_t r = 0; r < D; ++r) rowdep[r] = rdm_deposit(r, a.keep);
  const uint32_t tdep = rdm_deposit(tid, a.env);
  const float2* st = states + (uint64_t(m) << a.n);
  float2* dst = out + (uint64_t(m) << a.n);
  uint32_t idx[V];
  bool valid[V];
  float2 x[V][D];
#pragma unroll
  for (uint32_t j = 0; j < V; ++j) {  // (every load in flight before the first use)
    const uint32_t high = sub_vec_high(blockIdx.x, j);
    valid[j] = high + tid < a.env_values;
    idx[j] = rdm_deposit(high, a.env) | tdep;
#pragma unroll
    for (uint32_t r = 0; r < D; ++r) x[j][r] = valid[j] ? st[idx[j] | rowdep[r]] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  const double sc = scale ? scale[m] : 1.0;
  double dre = 0.0, dim = 0.0;
#pragma unroll
  for (uint32_t r = 0; r < D; ++r) {
    float vr[V], vi[V];
#pragma unroll
    for (uint32_t j = 0; j < V; ++j) vr[j] = vi[j] = 0.f;
#pragma unroll
    for (uint32_t c = 0; c < D; ++c) {
      const float2 o = sop[r * D + c];
#pragma unroll
      for (uint32_t j = 0; j < V; ++j) {
        vr[j] = fmaf(o.x, x[j][c].x, vr[j]);
        vr[j] = fmaf(-o.y, x[j][c].y, vr[j]);
        vi[j] = fmaf(o.x, x[j][c].y, vi[j]);
        vi[j] = fmaf(o.y, x[j][c].x, vi[j]);
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < V; ++j)
      if (valid[j]) {
        dst[idx[j] | rowdep[r]] = make_float2(float(double(vr[j]) * sc), float(double(vi[j]) * sc));
        sub_dot_add(x[j][r], vr[j], vi[j], &dre, &dim);
      }
  }
  if (part) sub_store_partial(dre, dim, red, m, a.slices, blockIdx.x, part);
}

// planes[0][a' 2^k + a] = Re A[a, a'], planes[1][...] = Im A[a, a']
__global__ __launch_bounds__(kSubThreads) void subsys_transpose_kernel(const float2* __restrict__ op, uint32_t k, float* __restrict__ planes) {
  const uint32_t e = blockIdx.x * kSubThreads + threadIdx.x, dim = 1u << k;
  if (e >= dim * dim) return;
  const uint32_t ap = e >> k, r = e & (dim - 1u);
  const float2 v = op[(r << k) | ap];
  planes[e] = v.x;
  planes[(size_t(1) << (2u * k)) + e] = v.y;
}

template <uint32_t STRIPS, uint32_t TK>
__global__ __launch_bounds__(kSubThreads) void subsys_matrix_kernel(const float2* __restrict__ states, const float* __restrict__ planes,
                                                                   const double* __restrict__ scale, SubArgs a,
                                                                   float2* __restrict__ out, double* __restrict__ part) {
  constexpr uint32_t TM = 16u * STRIPS, PA = sub_lds_pitch(TM), PB = sub_lds_pitch(kSubTileCols);
  constexpr uint32_t NB = TK * kSubTileCols / kSubThreads, NA = TM * TK / kSubThreads;
  static_assert(NB >= 1 && NA >= 1 && kSubThreads % TM == 0, "a stage's loads divide among 256 threads");
  __shared__ float s_ar[TK * PA], s_ai[TK * PA], s_br[TK * PB], s_bi[TK * PB];
  __shared__ uint32_t rowdep[1u << kRdmMaxKeep];
  __shared__ double red[kSubThreads / 64][2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t m = blockIdx.z * kSubGridY + blockIdx.y;
  if (m >= a.M) return;  // (workgroup-uniform)
  const uint32_t dim = 1u << a.k;
  uint32_t row0, col0;
  sub_tile_of(a.row_tiles, TM, blockIdx.x, &row0, &col0);
  for (uint32_t r = tid; r < dim; r += kSubThreads) rowdep[r] = rdm_deposit(r, a.keep);
  // the column this thread gathers, and the column of its results
  uint32_t kk_b[NB], c_b, kk_a[NA], r_a;
#pragma unroll
  for (uint32_t i = 0; i < NB; ++i) sub_panel_element(tid, i, &kk_b[i], &c_b);
#pragma unroll
  for (uint32_t i = 0; i < NA; ++i) sub_operator_element(TM, tid, i, &kk_a[i], &r_a);
  const bool gather = col0 + c_b < a.env_values;
  const uint32_t gdep = rdm_deposit(col0 + c_b, a.env);
  const float2* st = states + (uint64_t(m) << a.n);
  const float* plane_r = planes + row0 + r_a;
  const float* plane_i = plane_r + (size_t(1) << (2u * a.k));
  __syncthreads();

  float2 bv[NB];
  float av_r[NA], av_i[NA];
#define SUB_FETCH(k0)                                                                                      \
  {                                                                                                        \
    _Pragma("unroll") for (uint32_t i = 0; i < NB; ++i)                                                    \
      bv[i] = gather ? st[rowdep[(k0) + kk_b[i]] | gdep] : make_float2(0.f, 0.f);                          \
    _Pragma("unroll") for (uint32_t i = 0; i < NA; ++i) {                                                  \
      av_r[i] = plane_r[size_t((k0) + kk_a[i]) << a.k];                                                    \
      av_i[i] = plane_i[size_t((k0) + kk_a[i]) << a.k];                                                    \
    }                                                                                                      \
  }
  SUB_FETCH(0u)
  sub_f32x4 acc_r[STRIPS], acc_i[STRIPS];
#pragma unroll
  for (uint32_t s = 0; s < STRIPS; ++s) acc_r[s] = acc_i[s] = sub_f32x4{0.f, 0.f, 0.f, 0.f};
  const uint32_t quad = lane >> 4, l16 = lane & 15u;
  for (uint32_t k0 = 0; k0 < dim; k0 += TK) {
#pragma unroll
    for (uint32_t i = 0; i < NB; ++i) {
      s_br[kk_b[i] * PB + c_b] = bv[i].x;
      s_bi[kk_b[i] * PB + c_b] = bv[i].y;
    }
#pragma unroll
    for (uint32_t i = 0; i < NA; ++i) {
      s_ar[kk_a[i] * PA + r_a] = av_r[i];
      s_ai[kk_a[i] * PA + r_a] = av_i[i];
    }
    __syncthreads();
    if (k0 + TK < dim) SUB_FETCH(k0 + TK)
#pragma unroll
    for (uint32_t q = 0; q < TK / 4u; ++q) {
      const uint32_t kq = 4u * q + quad;  // A[l16][k = quad], B[k = quad][l16]
      const float br = s_br[kq * PB + 16u * wave + l16], bi = s_bi[kq * PB + 16u * wave + l16];
#pragma unroll
      for (uint32_t s = 0; s < STRIPS; ++s) {
        const float ar = s_ar[kq * PA + 16u * s + l16], ai = s_ai[kq * PA + 16u * s + l16];
        acc_r[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, br, acc_r[s], 0, 0, 0);
        acc_r[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(-ai, bi, acc_r[s], 0, 0, 0);
        acc_i[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, bi, acc_i[s], 0, 0, 0);
        acc_i[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, br, acc_i[s], 0, 0, 0);
      }
    }
    __syncthreads();
  }
#undef SUB_FETCH

  const double sc = scale ? scale[m] : 1.0;
  float2* dst = out + (uint64_t(m) << a.n);
  double dre = 0.0, dim_ = 0.0;
#pragma unroll
  for (uint32_t s = 0; s < STRIPS; ++s)
#pragma unroll
    for (uint32_t g = 0; g < 4; ++g) {
      uint32_t r, c;
      sub_result_element(wave, lane, s, g, &r, &c);
      if (col0 + c < a.env_values) {
        const uint32_t at = rowdep[row0 + r] | rdm_deposit(col0 + c, a.env);
        const float vr = acc_r[s][g], vi = acc_i[s][g];
        dst[at] = make_float2(float(double(vr) * sc), float(double(vi) * sc));
        if (part) sub_dot_add(st[at], vr, vi, &dre, &dim_);
      }
    }
  if (part) sub_store_partial(dre, dim_, red, m, a.slices, blockIdx.x, part);
}

// dots [M, 2]
__global__ __launch_bounds__(kSweepThreads) void subsys_dots_finish(const double* __restrict__ part, uint32_t slices,
                                                                    double* __restrict__ dots) {
  __shared__ double sh[kSweepThreads];
  const double2 d = sweep_row_sum2(part + uint64_t(blockIdx.x) * 2 * slices, slices, sh);
  if (threadIdx.x == 0) {
    dots[2 * uint64_t(blockIdx.x)] = d.x;
    dots[2 * uint64_t(blockIdx.x) + 1] = d.y;
  }
}

}  // namespace

hipError_t launch_subsystem_apply(const float2* states, uint32_t M, uint32_t n, uint64_t keep_mask, const float2* op,
                                  const double* scale, float2* out, double* dots, void* scratch, hipStream_t stream) {
  if (rdm_check(int(n), keep_mask) != 0 || M < 1 || M > uint32_t(kRdmMaxStates)) return hipErrorInvalidValue;
  const SubPlan p = sub_plan(int(n), keep_mask, int(M));
  SubArgs a;
  a.n = p.n;
  a.k = p.k;
  a.M = p.M;
  a.env_values = p.env_values;
  a.row_tiles = p.row_tiles;
  a.slices = p.slices;
  a.keep = p.masks.keep;
  a.env = p.masks.env;
  double* part = dots ? reinterpret_cast<double*>(static_cast<char*>(scratch) + p.parts_offset) : nullptr;
  const dim3 grid(p.slices, p.grid_y, p.grid_z), block(kSubThreads);
  if (!p.matrix) {
    switch (p.k) {
      case 1: hipLaunchKernelGGL(subsys_vector_kernel<1>, grid, block, 0, stream, states, op, scale, a, out, part); break;
      case 2: hipLaunchKernelGGL(subsys_vector_kernel<2>, grid, block, 0, stream, states, op, scale, a, out, part); break;
      case 3: hipLaunchKernelGGL(subsys_vector_kernel<3>, grid, block, 0, stream, states, op, scale, a, out, part); break;
      default: return hipErrorInvalidValue;
    }
  } else {
    float* planes = static_cast<float*>(scratch);
    const uint32_t entries = 1u << (2u * p.k);
    hipLaunchKernelGGL(subsys_transpose_kernel, dim3((entries + kSubThreads - 1u) / kSubThreads), block, 0, stream, op, p.k, planes);
    if (p.k == 4)
      hipLaunchKernelGGL((subsys_matrix_kernel<1, 16>), grid, block, 0, stream, states, planes, scale, a, out, part);
    else if (p.k == 5)
      hipLaunchKernelGGL((subsys_matrix_kernel<2, 32>), grid, block, 0, stream, states, planes, scale, a, out, part);
    else
      hipLaunchKernelGGL((subsys_matrix_kernel<4, 32>), grid, block, 0, stream, states, planes, scale, a, out, part);
  }
  if (dots) hipLaunchKernelGGL(subsys_dots_finish, dim3(M), dim3(kSweepThreads), 0, stream, part, p.slices, dots);
  return hipGetLastError();
}

}  // namespace qhbm
