// cross_gram_vjp.hip -- the vector-Jacobian product of the cross-Gram matrix of two ensembles of device-resident states (gfx950).
//
// For C[i, j] = sum_x t(x) conj(a_i(x)) b_j(x) (cross_gram.hip) and a cotangent Gamma [M, K] of C, used as given,
// qhbm_cross_gram_vjp writes
//     out_kets_j(x) = t(x) c_j(x),  c_j(x) = sum_i Gamma[i, j] a_i(x)      out_bras_i(x) = t(x) sum_j conj(Gamma[i, j]) b_j(x)
//     table_grad(x) = sum_j Re(conj(c_j(x)) b_j(x))
// -- the cotangents of the kets, of the bras and of the table (engine.cpp); each output may be absent.  Both
// state outputs are one side sweep  out_s(x) = t(x) sum_r W[r, s] src_r(x)  of R source rows and S output rows, run once per
// side (cross_gram_vjp_plan.h): the ket side with src = bras and W = Gamma, which also sums table_grad against the kets as
// partner rows, and the bra side with src = kets and W[r, s] = conj(Gamma[s, r]).  What is here:
//   cross_gram_vjp_vector_kernel<R>       R <= 8: a thread holds all R source rows of its words in registers, W sits in LDS
//                                         in chunks of 64 output rows and is read as broadcasts, the output rows are
//                                         produced one after the other
//   cross_gram_vjp_planes_kernel          R >= 9: W into two float planes [Pr][Ps], zero beyond (R, S), in the scratch
//   cross_gram_vjp_matrix_kernel<STRIPS>  R >= 9: gram_vjp.hip's matrix kernel with a rectangular W: a workgroup owns 64
//                                         columns (amplitudes) and walks the output rows in row tiles of 16 STRIPS and the
//                                         source rows in stages of 16 on v_mfma_f32_16x16x4_f32, in the real embedding
//                                         Re = W_r s_r - W_i s_i, Im = W_r s_i + W_i s_r; the unscaled results pass through
//                                         LDS, every thread stores words of out rows (t applied), and wave 0 -- one lane per
//                                         column -- continues the column's table_grad sum over the tile's rows
// Which kernel runs depends on R, the source side's row count, alone: a call with M = 32 and K = 2 runs the matrix kernel for
// the kets' cotangent and the vector kernel for the bras'.
// Order of additions.  out_s(x) / t(x) is an f32 fused-multiply-add chain over r ascending (the matrix instruction is bit for
// bit such a chain): per r, W_r s_r then -W_i s_i for the real part (vector kernel), or per four r the four products of
// W_r s_r then the four of -W_i s_i (matrix kernel); the imaginary part likewise with W_r s_i, W_i s_r.  out = t c, one
// rounding per part.  table_grad(x): float x float in double (exact), Re c Re b then Im c Im b, j ascending, in one register
// from j = 0 to j = K - 1.  No partials, no atomics: a result depends on (n, M, K) and the inputs alone.
//
// (a translation unit of its own in the source tree, compiled as part of observable.hip beside gram_vjp.hip, whose plan
// helpers it reads; it uses no name of another .hip file)
#include "cross_gram_vjp_plan.h"
#include "kernels.h"

namespace qhbm {
namespace {

typedef float cgv_f32x4 __attribute__((ext_vector_type(4)));

// src [R, words], out [S, words] or NULL, partner [S, words] and table_grad [2 words] or both NULL; gamma [M, K]
template <uint32_t R>
__global__ __launch_bounds__(kGvThreads) void cross_gram_vjp_vector_kernel(const float4* __restrict__ src, uint64_t words,
                                                                          const float2* __restrict__ table,
                                                                          const float2* __restrict__ gamma, uint32_t S,
                                                                          uint32_t bra_side, float4* __restrict__ out,
                                                                          const float4* __restrict__ partner,
                                                                          double* __restrict__ table_grad) {
  constexpr uint32_t V = gv_vec_words(R);
  __shared__ float2 sh[R * kCgvChunk];
  const uint32_t tid = threadIdx.x;
  const uint32_t chunks = (S + kCgvChunk - 1u) / kCgvChunk;
#pragma unroll 1
  for (uint32_t k0 = 0; k0 < kGvSliceWords / kGvThreads; k0 += V) {
    uint64_t w[V];
    bool valid[V];
    float4 a[V][R];
    float2 t[V];
#pragma unroll
    for (uint32_t v = 0; v < V; ++v) {  // (every load in flight before the first use)
      w[v] = gv_vec_word(blockIdx.x, k0 + v, tid);
      valid[v] = w[v] < words;
#pragma unroll
      for (uint32_t r = 0; r < R; ++r) a[v][r] = valid[v] ? src[r * words + w[v]] : make_float4(0.f, 0.f, 0.f, 0.f);
      t[v] = (table && valid[v]) ? table[w[v]] : make_float2(1.f, 1.f);
    }
    double g0[V], g1[V];
#pragma unroll
    for (uint32_t v = 0; v < V; ++v) g0[v] = g1[v] = 0.0;
#pragma unroll 1
    for (uint32_t chunk = 0; chunk < chunks; ++chunk) {
      const uint32_t live = cgv_chunk_rows(S, chunk), s0 = chunk * kCgvChunk;
      if (chunks > 1u || k0 == 0u) {  // (workgroup-uniform; a single chunk stays in LDS for every k0)
        __syncthreads();              // (the previous chunk's readers are done)
        for (uint32_t e = tid; e < R * live; e += kGvThreads) {
          const uint32_t r = e / live, sl = e - r * live;
          const float2 g = gamma[cgv_cotangent_index(bra_side != 0u, R, S, r, s0 + sl)];
          sh[r * kCgvChunk + sl] = bra_side ? make_float2(g.x, -g.y) : g;
        }
        __syncthreads();
      }
#pragma unroll 1
      for (uint32_t sl = 0; sl < live; ++sl) {
        const uint64_t row = uint64_t(s0 + sl) * words;
        float4 b[V];
        if (table_grad) {
#pragma unroll
          for (uint32_t v = 0; v < V; ++v) b[v] = valid[v] ? partner[row + w[v]] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float4 c[V];
#pragma unroll
        for (uint32_t v = 0; v < V; ++v) c[v] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (uint32_t r = 0; r < R; ++r) {
          const float2 h = sh[r * kCgvChunk + sl];
#pragma unroll
          for (uint32_t v = 0; v < V; ++v) {
            c[v].x = fmaf(h.x, a[v][r].x, c[v].x);
            c[v].x = fmaf(-h.y, a[v][r].y, c[v].x);
            c[v].y = fmaf(h.x, a[v][r].y, c[v].y);
            c[v].y = fmaf(h.y, a[v][r].x, c[v].y);
            c[v].z = fmaf(h.x, a[v][r].z, c[v].z);
            c[v].z = fmaf(-h.y, a[v][r].w, c[v].z);
            c[v].w = fmaf(h.x, a[v][r].w, c[v].w);
            c[v].w = fmaf(h.y, a[v][r].z, c[v].w);
          }
        }
#pragma unroll
        for (uint32_t v = 0; v < V; ++v) {
          if (out && valid[v])
            out[row + w[v]] = table ? make_float4(t[v].x * c[v].x, t[v].x * c[v].y, t[v].y * c[v].z, t[v].y * c[v].w) : c[v];
          if (table_grad) {
            g0[v] = __builtin_fma(double(c[v].x), double(b[v].x), g0[v]);
            g0[v] = __builtin_fma(double(c[v].y), double(b[v].y), g0[v]);
            g1[v] = __builtin_fma(double(c[v].z), double(b[v].z), g1[v]);
            g1[v] = __builtin_fma(double(c[v].w), double(b[v].w), g1[v]);
          }
        }
      }
    }
    if (table_grad) {
#pragma unroll
      for (uint32_t v = 0; v < V; ++v)
        if (valid[v]) {
          table_grad[2 * w[v]] = g0[v];
          table_grad[2 * w[v] + 1] = g1[v];
        }
    }
  }
}

// planes[0][r Ps + s] = Re W[r, s], planes[1][...] = Im W[r, s]; zero where r >= R or s >= S
__global__ __launch_bounds__(kGvThreads) void cross_gram_vjp_planes_kernel(const float2* __restrict__ gamma, uint32_t R, uint32_t S,
                                                                          uint32_t bra_side, uint32_t Pr, uint32_t Ps,
                                                                          float* __restrict__ planes) {
  const uint32_t e = blockIdx.x * kGvThreads + threadIdx.x;
  if (e >= Pr * Ps) return;
  uint32_t r, s;
  cgv_plane_element(Ps, e, &r, &s);
  float2 v = make_float2(0.f, 0.f);
  if (r < R && s < S) {
    v = gamma[cgv_cotangent_index(bra_side != 0u, R, S, r, s)];
    if (bra_side) v.y = -v.y;
  }
  planes[e] = v.x;
  planes[size_t(Pr) * Ps + e] = v.y;
}

struct CgvArgs {
  uint32_t R, S, r16, s16, row_tiles, P, col_tiles;
  uint64_t amps;
};

// src [R, amps], out [S, amps] or NULL, partner [S, amps] and table_grad [amps] or both NULL
template <uint32_t STRIPS>
__global__ __launch_bounds__(kGvThreads) void cross_gram_vjp_matrix_kernel(const float2* __restrict__ src, const float* __restrict__ planes,
                                                                          const float* __restrict__ table, CgvArgs a,
                                                                          float2* __restrict__ out, const float2* __restrict__ partner,
                                                                          double* __restrict__ table_grad) {
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
  const float2* st = src + col0 + c_b;  // (dereferenced only where in_cols)
  const size_t plane = size_t(a.r16) * a.P;
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
    const uint32_t strips = gv_live_strips(a.s16, TM, rt);
    const float* plane_r = planes + row0;
    float2 bv[NB];
    float av_r[NA], av_i[NA];
#define CGV_FETCH(i0)                                                                                         \
  {                                                                                                           \
    _Pragma("unroll") for (uint32_t i = 0; i < NB; ++i)                                                       \
      bv[i] = (in_cols && (i0) + kk_b[i] < a.R) ? st[uint64_t((i0) + kk_b[i]) * a.amps] : make_float2(0.f, 0.f); \
    _Pragma("unroll") for (uint32_t i = 0; i < NA; ++i) {                                                     \
      av_r[i] = plane_r[size_t((i0) + kk_a[i]) * a.P + r_a[i]];                                               \
      av_i[i] = plane_r[plane + size_t((i0) + kk_a[i]) * a.P + r_a[i]];                                       \
    }                                                                                                         \
  }
    CGV_FETCH(0u)
    cgv_f32x4 acc_r[STRIPS], acc_i[STRIPS];
#pragma unroll
    for (uint32_t s = 0; s < STRIPS; ++s) acc_r[s] = acc_i[s] = cgv_f32x4{0.f, 0.f, 0.f, 0.f};
    for (uint32_t i0 = 0; i0 < a.r16; i0 += TK) {
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
      if (i0 + TK < a.r16) CGV_FETCH(i0 + TK)
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
#undef CGV_FETCH
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
        if (row0 + r < a.S) {
          const float2 cr = *reinterpret_cast<const float2*>(&s_cr[r * PC + 2u * w]);
          const float2 ci = *reinterpret_cast<const float2*>(&s_ci[r * PC + 2u * w]);
          const float4 v = table ? make_float4(t_s.x * cr.x, t_s.x * ci.x, t_s.y * cr.y, t_s.y * ci.y) : make_float4(cr.x, ci.x, cr.y, ci.y);
          *reinterpret_cast<float4*>(out + uint64_t(row0 + r) * a.amps + x_s) = v;
        }
      }
    }
    if (sums) {
      const uint32_t rows = a.S - row0 < TM ? a.S - row0 : TM;
      const float2* bj = partner + uint64_t(row0) * a.amps + x_g;
#pragma unroll 4
      for (uint32_t r = 0; r < rows; ++r) {
        const float2 v = bj[uint64_t(r) * a.amps];
        grad = __builtin_fma(double(s_cr[r * PC + tid]), double(v.x), grad);
        grad = __builtin_fma(double(s_ci[r * PC + tid]), double(v.y), grad);
      }
    }
  }
  if (sums) table_grad[x_g] = grad;
}

struct CgvSweep {
  const float2* src;      // [R, 2^n]
  const float* table;     // [2^n] or NULL
  const float2* gamma;    // [M, K]
  bool bra_side;
  float2* out;            // [S, 2^n] or NULL
  const float2* partner;  // [S, 2^n] with table_grad, else NULL
  double* table_grad;     // [2^n] or NULL
  float* planes;          // the side's planes in the scratch
  hipStream_t stream;
};

template <uint32_t R>
void cgv_launch_vector(const CgvSide& p, const CgvSweep& s) {
  hipLaunchKernelGGL(cross_gram_vjp_vector_kernel<R>, dim3(p.grid_x), dim3(kGvThreads), 0, s.stream,
                     reinterpret_cast<const float4*>(s.src), p.words, reinterpret_cast<const float2*>(s.table), s.gamma, p.S,
                     uint32_t(s.bra_side), reinterpret_cast<float4*>(s.out), reinterpret_cast<const float4*>(s.partner), s.table_grad);
}

// out_s(x) = t(x) sum_r W[r, s] src_r(x) for one side, with table_grad where the sweep carries partner rows
hipError_t cgv_side_sweep(const CgvSide& p, const CgvSweep& s) {
  if (!p.matrix) {
    switch (p.R) {
      case 1: cgv_launch_vector<1>(p, s); break;
      case 2: cgv_launch_vector<2>(p, s); break;
      case 3: cgv_launch_vector<3>(p, s); break;
      case 4: cgv_launch_vector<4>(p, s); break;
      case 5: cgv_launch_vector<5>(p, s); break;
      case 6: cgv_launch_vector<6>(p, s); break;
      case 7: cgv_launch_vector<7>(p, s); break;
      case 8: cgv_launch_vector<8>(p, s); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
  const uint32_t entries = p.r16 * p.P;
  hipLaunchKernelGGL(cross_gram_vjp_planes_kernel, dim3((entries + kGvThreads - 1u) / kGvThreads), dim3(kGvThreads), 0, s.stream,
                     s.gamma, p.R, p.S, uint32_t(s.bra_side), p.r16, p.P, s.planes);
  CgvArgs a;
  a.R = p.R;
  a.S = p.S;
  a.r16 = p.r16;
  a.s16 = p.s16;
  a.row_tiles = p.row_tiles;
  a.P = p.P;
  a.col_tiles = p.col_tiles;
  a.amps = p.amps;
  const dim3 grid(p.grid_x, p.grid_y), block(kGvThreads);
#define CGV_MATRIX(STRIPS)                                                                                                  \
  hipLaunchKernelGGL(cross_gram_vjp_matrix_kernel<STRIPS>, grid, block, 0, s.stream, s.src, s.planes, s.table, a, s.out, s.partner, \
                     s.table_grad)
  switch (p.tm / 16u) {
    case 1: CGV_MATRIX(1); break;
    case 2: CGV_MATRIX(2); break;
    case 3: CGV_MATRIX(3); break;
    default: CGV_MATRIX(4); break;
  }
#undef CGV_MATRIX
  return hipGetLastError();
}

}  // namespace

hipError_t launch_cross_gram_vjp(const float2* bras, uint32_t M, const float2* kets, uint32_t K, uint32_t n, const float* table,
                                 const float2* gamma, float2* out_bras, float2* out_kets, double* table_grad, void* scratch,
                                 hipStream_t stream) {
  if (n < 1 || n > 31 || M < 1 || M > uint32_t(kGramMaxStates) || K < 1 || K > uint32_t(kGramMaxStates) ||
      (!out_bras && !out_kets && !table_grad))
    return hipErrorInvalidValue;
  const CgvPlan p = cgv_plan(int(n), int(M), int(K));
  float* planes = static_cast<float*>(scratch);
  if (out_kets || table_grad) {
    const CgvSweep s{bras, table, gamma, false, out_kets, table_grad ? kets : nullptr, table_grad, planes, stream};
    if (hipError_t e = cgv_side_sweep(p.ket, s)) return e;
  }
  if (out_bras) {
    const CgvSweep s{kets, table, gamma, true, out_bras, nullptr, nullptr, planes + p.bra_plane_offset, stream};
    if (hipError_t e = cgv_side_sweep(p.bra, s)) return e;
  }
  return hipSuccess;
}

}  // namespace qhbm
