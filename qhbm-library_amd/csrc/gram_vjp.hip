// gram_vjp.hip -- the vector-Jacobian product of the weighted Gram matrix of M device-resident states (gfx950).
//
// For G[i, j] = sum_x t(x) conj(a_i(x)) a_j(x) (gram.hip) and H = Gamma + Gamma^H of a cotangent Gamma of G,
// qhbm_weighted_gram_vjp writes, in one pass over the states,
//     c_j(x) = sum_i H[i, j] a_i(x),   out_j(x) = t(x) c_j(x),   table_grad(x) = 1/2 sum_j Re(conj(c_j(x)) a_j(x))
// -- the cotangents of the states and of the table (engine.cpp).  H is used as given (complex64 [M, M],
// row-major); either output may be absent.  The launch plan is gram_vjp_plan.h's.  What is here:
//   gram_vjp_vector_kernel<M>     M <= 8: a thread holds all M input rows of its words in registers, H sits in LDS and is
//                                 read as broadcasts, the output states are produced one after the other.  One streaming
//                                 pass: 8 M + 4 bytes read and 8 M + 8 written per amplitude.
//   gram_vjp_planes_kernel        M >= 9: H into two float planes [P][P], zero beyond M, at the head of the scratch
//   gram_vjp_matrix_kernel<STRIPS>  M >= 9: a workgroup owns 64 columns (amplitudes) and walks the output states in row
//                                 tiles of 16 STRIPS and the input states in stages of 16: the H tile and the state panel go
//                                 to LDS as re / im planes [input state][row], [input state][column] (the next stage's words
//                                 are in registers while this one is multiplied), wave w multiplies its 16 columns by every
//                                 row strip on v_mfma_f32_16x16x4_f32 in the real embedding Re = H_r a_r - H_i a_i,
//                                 Im = H_r a_i + H_i a_r.  The unscaled results pass through LDS: every thread stores
//                                 words of out rows (t applied), and wave 0 -- one lane per column -- continues the
//                                 column's table_grad sum over the tile's rows in ascending order.
// Order of additions.  c_j(x) is an f32 fused-multiply-add chain over i ascending (the matrix instruction is bit for bit such
// a chain): per i, H_r a_r then -H_i a_i for the real part (vector kernel), or per four i the four products of H_r a_r then
// the four of -H_i a_i (matrix kernel); the imaginary part likewise with H_r a_i, H_i a_r.  out = t c, one rounding per part.
// table_grad(x): float x float in double (exact), Re c Re a then Im c Im a, j ascending, in one register from j = 0 to
// j = M - 1; halved at the end (exact).  No partials, no atomics: a result depends on (n, M) and the inputs alone.
//
// (a translation unit of its own in the source tree, compiled as part of observable.hip beside subsystem_apply.hip, whose
// matrix kernel is its closest relative; it uses no name of another .hip file)
#include "gram_vjp_plan.h"
#include "kernels.h"

namespace qhbm {
namespace {

typedef float gv_f32x4 __attribute__((ext_vector_type(4)));

template <uint32_t M>
__global__ __launch_bounds__(kGvThreads) void gram_vjp_vector_kernel(const float4* __restrict__ states, uint64_t words,
                                                                    const float2* __restrict__ table, const float2* __restrict__ H,
                                                                    float4* __restrict__ out, double* __restrict__ table_grad) {
  constexpr uint32_t V = gv_vec_words(M);
  __shared__ float2 sh[M * M];
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < M * M; i += kGvThreads) sh[i] = H[i];
  __syncthreads();
#pragma unroll 1
  for (uint32_t k0 = 0; k0 < kGvSliceWords / kGvThreads; k0 += V) {
    uint64_t w[V];
    bool valid[V];
    float4 a[V][M];
    float2 t[V];
#pragma unroll
    for (uint32_t v = 0; v < V; ++v) {  // (every load in flight before the first use)
      w[v] = gv_vec_word(blockIdx.x, k0 + v, tid);
      valid[v] = w[v] < words;
#pragma unroll
      for (uint32_t i = 0; i < M; ++i) a[v][i] = valid[v] ? states[i * words + w[v]] : make_float4(0.f, 0.f, 0.f, 0.f);
      t[v] = (table && valid[v]) ? table[w[v]] : make_float2(1.f, 1.f);
    }
    double g0[V], g1[V];
#pragma unroll
    for (uint32_t v = 0; v < V; ++v) g0[v] = g1[v] = 0.0;
#pragma unroll
    for (uint32_t j = 0; j < M; ++j) {
      float4 c[V];
#pragma unroll
      for (uint32_t v = 0; v < V; ++v) c[v] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (uint32_t i = 0; i < M; ++i) {
        const float2 h = sh[i * M + j];
#pragma unroll
        for (uint32_t v = 0; v < V; ++v) {
          c[v].x = fmaf(h.x, a[v][i].x, c[v].x);
          c[v].x = fmaf(-h.y, a[v][i].y, c[v].x);
          c[v].y = fmaf(h.x, a[v][i].y, c[v].y);
          c[v].y = fmaf(h.y, a[v][i].x, c[v].y);
          c[v].z = fmaf(h.x, a[v][i].z, c[v].z);
          c[v].z = fmaf(-h.y, a[v][i].w, c[v].z);
          c[v].w = fmaf(h.x, a[v][i].w, c[v].w);
          c[v].w = fmaf(h.y, a[v][i].z, c[v].w);
        }
      }
#pragma unroll
      for (uint32_t v = 0; v < V; ++v) {
        if (out && valid[v])
          out[j * words + w[v]] = table ? make_float4(t[v].x * c[v].x, t[v].x * c[v].y, t[v].y * c[v].z, t[v].y * c[v].w) : c[v];
        g0[v] = __builtin_fma(double(c[v].x), double(a[v][j].x), g0[v]);
        g0[v] = __builtin_fma(double(c[v].y), double(a[v][j].y), g0[v]);
        g1[v] = __builtin_fma(double(c[v].z), double(a[v][j].z), g1[v]);
        g1[v] = __builtin_fma(double(c[v].w), double(a[v][j].w), g1[v]);
      }
      // (one output state at a time: left to interleave the M chains, the max-ILP scheduler keeps every c_j and its
      // float64 copies live and the kernel falls to one wave per SIMD)
      __builtin_amdgcn_sched_barrier(0);
    }
    if (table_grad) {
#pragma unroll
      for (uint32_t v = 0; v < V; ++v)
        if (valid[v]) {
          table_grad[2 * w[v]] = 0.5 * g0[v];
          table_grad[2 * w[v] + 1] = 0.5 * g1[v];
        }
    }
  }
}

// planes[0][i P + j] = Re H[i, j], planes[1][...] = Im H[i, j]; zero where i or j >= M
__global__ __launch_bounds__(kGvThreads) void gram_vjp_planes_kernel(const float2* __restrict__ H, uint32_t M, uint32_t P,
                                                                    float* __restrict__ planes) {
  const uint32_t e = blockIdx.x * kGvThreads + threadIdx.x;
  if (e >= P * P) return;
  uint32_t i, j;
  gv_plane_element(P, e, &i, &j);
  const float2 v = (i < M && j < M) ? H[i * M + j] : make_float2(0.f, 0.f);
  planes[e] = v.x;
  planes[size_t(P) * P + e] = v.y;
}

struct GvArgs {
  uint32_t M, m16, row_tiles, P, col_tiles;
  uint64_t amps;
};

template <uint32_t STRIPS>
__global__ __launch_bounds__(kGvThreads) void gram_vjp_matrix_kernel(const float2* __restrict__ states, const float* __restrict__ planes,
                                                                    const float* __restrict__ table, GvArgs a,
                                                                    float2* __restrict__ out, double* __restrict__ table_grad) {
  constexpr uint32_t TM = 16u * STRIPS, TK = kGvStage, PA = gv_lds_pitch(TM), PB = gv_lds_pitch(kGvTileCols), PC = kGvResultPitch;
  constexpr uint32_t NB = TK * kGvTileCols / kGvThreads, NA = TM * TK / kGvThreads, NS = TM * (kGvTileCols / 2u) / kGvThreads;
  static_assert(NB * kGvThreads == TK * kGvTileCols && NA * kGvThreads == TM * TK && NS * kGvThreads == TM * (kGvTileCols / 2u),
                "a stage's loads and the epilogue's stores divide among 256 threads");
  __shared__ float s_ar[TK * PA], s_ai[TK * PA], s_br[TK * PB], s_bi[TK * PB];
  __shared__ __attribute__((aligned(8))) float s_cr[TM * PC], s_ci[TM * PC];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = blockIdx.y * kGvGridX + blockIdx.x;
  if (tile >= a.col_tiles) return;  // (workgroup-uniform)
  const uint64_t col0 = uint64_t(tile) * kGvTileCols;
  uint32_t kk_b[NB], c_b, kk_a[NA], r_a[NA];
#pragma unroll
  for (uint32_t i = 0; i < NB; ++i) gv_panel_element(tid, i, &kk_b[i], &c_b);
#pragma unroll
  for (uint32_t i = 0; i < NA; ++i) gv_operator_element(TM, tid, i, &kk_a[i], &r_a[i]);
  const bool in_cols = col0 + c_b < a.amps;
  const float2* st = states + col0 + c_b;  // (dereferenced only where in_cols)
  const size_t plane = size_t(a.P) * a.P;
  const uint32_t quad = lane >> 4, l16 = lane & 15u;
  // the epilogue's word of this thread, its table entries, and the column's running table_grad (wave 0)
  uint32_t r_s0, w_s;
  gv_store_element(tid, 0, &r_s0, &w_s);
  const uint64_t x_s = col0 + 2u * w_s;
  const bool store_cols = x_s < a.amps;
  float2 t_s = make_float2(1.f, 1.f);
  if (table && store_cols) t_s = *reinterpret_cast<const float2*>(table + x_s);
  const uint64_t x_g = col0 + tid;
  const bool sums = table_grad && tid < kGvTileCols && x_g < a.amps;
  double grad = 0.0;

  for (uint32_t rt = 0; rt < a.row_tiles; ++rt) {
    const uint32_t row0 = rt * TM;
    const uint32_t strips = gv_live_strips(a.m16, TM, rt);
    const float* plane_r = planes + row0;
    float2 bv[NB];
    float av_r[NA], av_i[NA];
#define GV_FETCH(i0)                                                                                          \
  {                                                                                                           \
    _Pragma("unroll") for (uint32_t i = 0; i < NB; ++i)                                                       \
      bv[i] = (in_cols && (i0) + kk_b[i] < a.M) ? st[uint64_t((i0) + kk_b[i]) * a.amps] : make_float2(0.f, 0.f); \
    _Pragma("unroll") for (uint32_t i = 0; i < NA; ++i) {                                                     \
      av_r[i] = plane_r[size_t((i0) + kk_a[i]) * a.P + r_a[i]];                                               \
      av_i[i] = plane_r[plane + size_t((i0) + kk_a[i]) * a.P + r_a[i]];                                       \
    }                                                                                                         \
  }
    GV_FETCH(0u)
    gv_f32x4 acc_r[STRIPS], acc_i[STRIPS];
#pragma unroll
    for (uint32_t s = 0; s < STRIPS; ++s) acc_r[s] = acc_i[s] = gv_f32x4{0.f, 0.f, 0.f, 0.f};
    for (uint32_t i0 = 0; i0 < a.m16; i0 += TK) {
#pragma unroll
      for (uint32_t i = 0; i < NB; ++i) {
        s_br[kk_b[i] * PB + c_b] = bv[i].x;
        s_bi[kk_b[i] * PB + c_b] = bv[i].y;
      }
#pragma unroll
      for (uint32_t i = 0; i < NA; ++i) {
        s_ar[kk_a[i] * PA + r_a[i]] = av_r[i];
        s_ai[kk_a[i] * PA + r_a[i]] = av_i[i];
      }
      __syncthreads();
      if (i0 + TK < a.m16) GV_FETCH(i0 + TK)
#pragma unroll
      for (uint32_t q = 0; q < TK / 4u; ++q) {
        const uint32_t kq = 4u * q + quad;  // A[l16][k = quad], B[k = quad][l16]
        const float br = s_br[kq * PB + 16u * wave + l16], bi = s_bi[kq * PB + 16u * wave + l16];
#pragma unroll
        for (uint32_t s = 0; s < STRIPS; ++s)
          if (s < strips) {
            const float ar = s_ar[kq * PA + 16u * s + l16], ai = s_ai[kq * PA + 16u * s + l16];
            acc_r[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, br, acc_r[s], 0, 0, 0);
            acc_r[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(-ai, bi, acc_r[s], 0, 0, 0);
            acc_i[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(ar, bi, acc_i[s], 0, 0, 0);
            acc_i[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(ai, br, acc_i[s], 0, 0, 0);
          }
      }
      __syncthreads();
    }
#undef GV_FETCH
    // (the previous row tile's readers of s_cr / s_ci have all passed the stage loop's barriers)
#pragma unroll
    for (uint32_t s = 0; s < STRIPS; ++s)
#pragma unroll
      for (uint32_t g = 0; g < 4; ++g) {
        uint32_t r, c;
        gv_result_element(wave, lane, s, g, &r, &c);
        s_cr[r * PC + c] = acc_r[s][g];
        s_ci[r * PC + c] = acc_i[s][g];
      }
    __syncthreads();
    if (out && store_cols) {
#pragma unroll
      for (uint32_t p = 0; p < NS; ++p) {
        uint32_t r, w;
        gv_store_element(tid, p, &r, &w);
        if (row0 + r < a.M) {
          const float2 cr = *reinterpret_cast<const float2*>(&s_cr[r * PC + 2u * w]);
          const float2 ci = *reinterpret_cast<const float2*>(&s_ci[r * PC + 2u * w]);
          const float4 v = table ? make_float4(t_s.x * cr.x, t_s.x * ci.x, t_s.y * cr.y, t_s.y * ci.y) : make_float4(cr.x, ci.x, cr.y, ci.y);
          *reinterpret_cast<float4*>(out + uint64_t(row0 + r) * a.amps + x_s) = v;
        }
      }
    }
    if (sums) {
      const uint32_t rows = a.M - row0 < TM ? a.M - row0 : TM;
      const float2* aj = states + uint64_t(row0) * a.amps + x_g;
#pragma unroll 4
      for (uint32_t r = 0; r < rows; ++r) {
        const float2 v = aj[uint64_t(r) * a.amps];
        grad = __builtin_fma(double(s_cr[r * PC + tid]), double(v.x), grad);
        grad = __builtin_fma(double(s_ci[r * PC + tid]), double(v.y), grad);
      }
    }
  }
  if (sums) table_grad[x_g] = 0.5 * grad;
}

template <uint32_t M>
void gv_launch_vector(const GvPlan& p, const float2* states, const float* table, const float2* H, float2* out, double* table_grad,
                      hipStream_t stream) {
  hipLaunchKernelGGL(gram_vjp_vector_kernel<M>, dim3(p.grid_x), dim3(kGvThreads), 0, stream, reinterpret_cast<const float4*>(states),
                     p.words, reinterpret_cast<const float2*>(table), H, reinterpret_cast<float4*>(out), table_grad);
}

}  // namespace

hipError_t launch_gram_vjp(const float2* states, uint32_t M, uint32_t n, const float* table, const float2* H, float2* out,
                           double* table_grad, void* scratch, hipStream_t stream) {
  if (n < 1 || n > 31 || M < 1 || M > uint32_t(kGramMaxStates) || (!out && !table_grad)) return hipErrorInvalidValue;
  const GvPlan p = gv_plan(int(n), int(M));
  if (!p.matrix) {
    switch (M) {
      case 1: gv_launch_vector<1>(p, states, table, H, out, table_grad, stream); break;
      case 2: gv_launch_vector<2>(p, states, table, H, out, table_grad, stream); break;
      case 3: gv_launch_vector<3>(p, states, table, H, out, table_grad, stream); break;
      case 4: gv_launch_vector<4>(p, states, table, H, out, table_grad, stream); break;
      case 5: gv_launch_vector<5>(p, states, table, H, out, table_grad, stream); break;
      case 6: gv_launch_vector<6>(p, states, table, H, out, table_grad, stream); break;
      case 7: gv_launch_vector<7>(p, states, table, H, out, table_grad, stream); break;
      case 8: gv_launch_vector<8>(p, states, table, H, out, table_grad, stream); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
  float* planes = static_cast<float*>(scratch);
  const uint32_t entries = p.P * p.P;
  hipLaunchKernelGGL(gram_vjp_planes_kernel, dim3((entries + kGvThreads - 1u) / kGvThreads), dim3(kGvThreads), 0, stream, H, M, p.P,
                     planes);
  GvArgs a;
  a.M = p.M;
  a.m16 = p.m16;
  a.row_tiles = p.row_tiles;
  a.P = p.P;
  a.col_tiles = p.col_tiles;
  a.amps = p.amps;
  const dim3 grid(p.grid_x, p.grid_y), block(kGvThreads);
  switch (p.tm / 16u) {
    case 1: hipLaunchKernelGGL(gram_vjp_matrix_kernel<1>, grid, block, 0, stream, states, planes, table, a, out, table_grad); break;
    case 2: hipLaunchKernelGGL(gram_vjp_matrix_kernel<2>, grid, block, 0, stream, states, planes, table, a, out, table_grad); break;
    case 3: hipLaunchKernelGGL(gram_vjp_matrix_kernel<3>, grid, block, 0, stream, states, planes, table, a, out, table_grad); break;
    default: hipLaunchKernelGGL(gram_vjp_matrix_kernel<4>, grid, block, 0, stream, states, planes, table, a, out, table_grad); break;
  }
  return hipGetLastError();
}

}  // namespace qhbm
