// reduced.hip -- the reduced density matrix of an ensemble of device-resident states (gfx950).
//
// qhbm_reduced_density forms rho_A[a, a'] = sum_m w_m sum_b phi_m(a, b) conj(phi_m(a', b)) for M complex64 states of 2^n
// amplitudes, an arbitrary subset A of k <= 10 kept qubits and float64 weights (NULL: 1) -- engine.cpp, DESIGN.md 6j.
// The index arithmetic and the launch plan are rdm_index.h's.  What is here:
//   rdm_tile_kernel<KT, WEIGHTED>  part[tile, slice, r, c, re / im] = the slice's share of one tile (I, J), J >= I, of edge
//                                  2^KT.  Per block of the environment the workgroup gathers the panel of the tile's rows
//                                  I (and J, off the diagonal) into LDS in 16-byte words -- two environment values of one row
//                                  or two rows, whichever index bit 0 is; slots swizzled by rdm_lds_slot so that the lanes of a
//                                  store spread over the banks for every mask -- the next block's words in flight while this
//                                  one is summed.  A thread owns a register block of min(2^KT, 4)^2 outputs; the (2^KT / 4)^2
//                                  threads of a group share an environment value, the 256 / group groups take the block's
//                                  values in turn: from KT = 6 on a workgroup is one group and nothing crosses lanes.
//   rdm_finish_kernel              rho[a, a'] = its partials in slice order for a' >= a; rho[a', a] = conj(rho[a, a']) written
//                                  from the same registers, Im rho[a, a] = 0: Hermitian bit for bit
// Order of additions: a thread adds its environment values in ascending (m, b) order, per value and output four fused
// multiply-adds, spelled out; the groups of a wave meet in a fixed shuffle tree, the waves in wave order, the slices in
// slice order: no floating-point atomics, and the grid is a function of (n, keep_mask, M) alone.  Products are
// float x float in double (exact); the column operand times w_m in double is the one rounding that is not an addition's.
//
// (a translation unit of its own in the source tree, compiled as part of states.hip; it uses no name of another .hip file.
// Its shape is its own -- panels in LDS, not state_sweep.h's streamed slices)
#include "kernels.h"
#include "rdm_index.h"

namespace qhbm {
namespace {

struct RdmArgs {
  uint32_t n, le, nv, tile_rows, slices;
  uint32_t keep, env_hi;
  uint64_t blocks_per_state, blocks;
  uint64_t gpos, lpos;  // RdmPlan's packed tables
};

constexpr uint32_t kRdmWords = (1u << kRdmPanelBits) / 2 / kRdmThreads;  // 16-byte words of a panel per thread: 4

struct RdmWords {
  float4 v[kRdmWords];
};

template <uint32_t KT, bool WEIGHTED>
__global__ __launch_bounds__(kRdmThreads) void rdm_tile_kernel(const float2* __restrict__ states,
                                                              const double* __restrict__ weights, RdmArgs a,
                                                              double* __restrict__ part) {
  constexpr uint32_t TE = 1u << KT, RB = KT < 2 ? TE : 4u, TB = TE / RB, G = TB * TB, NG = kRdmThreads / G;
  constexpr uint32_t GW = G < 64 ? G : 64;  // lanes of a wave that end up with distinct outputs
  constexpr uint32_t NO = RB * RB;
  __shared__ __attribute__((aligned(16))) float2 panel[2][1u << kRdmPanelBits];
  const uint32_t tid = threadIdx.x;
  uint32_t ti, tj;  // (wave-uniform: scalar arithmetic)
  rdm_tile_of(a.tile_rows, blockIdx.x, &ti, &tj);
  const bool diag = ti == tj;
  const uint32_t base_i = rdm_deposit(ti << KT, a.keep), base_j = rdm_deposit(tj << KT, a.keep);

  // This thread's words of a panel: elements L = 2 (tid + 256 w) and L + 1, w < 4.  Both maps are bitwise, so the part of
  // tid is computed once and the part of w is the same for every thread.
  const uint32_t pairs = 1u << (a.nv - 1u);
  uint32_t goff, slot;
  rdm_thread_part(a.gpos, a.lpos, a.nv, tid, &goff, &slot);
  uint32_t gw[kRdmWords], sw[kRdmWords];
#pragma unroll
  for (uint32_t w = 0; w < kRdmWords; ++w) rdm_word_part(a.gpos, a.lpos, a.nv, w, &gw[w], &sw[w]);
  const uint32_t slot1 = 1u << rdm_packed(a.lpos, 0);  // (index bit 0 is always a panel bit: rdm_index.h)

  uint64_t begin, end;
  rdm_slice_blocks(a.blocks, a.slices, blockIdx.y, &begin, &end);
  uint64_t m = begin / a.blocks_per_state;
  uint32_t hi = rdm_deposit(uint32_t(begin % a.blocks_per_state), a.env_hi);

  const uint32_t g = tid / G, pos = tid % G, bi = pos / TB, bj = pos % TB;
  const uint32_t env_block = 1u << a.le;
  double re[NO], im[NO];
#pragma unroll
  for (uint32_t p = 0; p < NO; ++p) re[p] = im[p] = 0.0;

  RdmWords wi, wj;
#define RDM_FETCH()                                                                                          \
  {                                                                                                          \
    const float2* st = states + (m << a.n);                                                                  \
    _Pragma("unroll") for (uint32_t w = 0; w < kRdmWords; ++w) if (tid + kRdmThreads * w < pairs) {          \
      wi.v[w] = *reinterpret_cast<const float4*>(st + (base_i | hi | goff | gw[w]));                         \
      if (!diag) wj.v[w] = *reinterpret_cast<const float4*>(st + (base_j | hi | goff | gw[w]));              \
    }                                                                                                        \
  }
  RDM_FETCH()
  for (uint64_t blk = begin; blk < end; ++blk) {
    const double wm = WEIGHTED ? weights[m] : 1.0;
#pragma unroll
    for (uint32_t w = 0; w < kRdmWords; ++w)
      if (tid + kRdmThreads * w < pairs) {
        const uint32_t s0 = rdm_lds_slot(KT, slot | sw[w]), s1 = rdm_lds_slot(KT, slot | sw[w] | slot1);
        panel[0][s0] = make_float2(wi.v[w].x, wi.v[w].y);
        panel[0][s1] = make_float2(wi.v[w].z, wi.v[w].w);
        if (!diag) {
          panel[1][s0] = make_float2(wj.v[w].x, wj.v[w].y);
          panel[1][s1] = make_float2(wj.v[w].z, wj.v[w].w);
        }
      }
    __syncthreads();
    hi = rdm_masked_inc(hi, a.env_hi);
    if (hi == 0u) ++m;
    if (blk + 1 < end) RDM_FETCH()
    const float2* rows = panel[0];
    const float2* cols = diag ? panel[0] : panel[1];
    for (uint32_t e = g; e < env_block; e += NG) {
      float4 x4[RB / 2], y4[RB / 2];
#pragma unroll
      for (uint32_t h = 0; h < RB / 2; ++h) {
        x4[h] = *reinterpret_cast<const float4*>(rows + rdm_lds_slot(KT, e * TE + bi * RB) + 2u * h);
        y4[h] = *reinterpret_cast<const float4*>(cols + rdm_lds_slot(KT, e * TE + bj * RB) + 2u * h);
      }
      double xr[RB], xi[RB], yr[RB], yi[RB];
#pragma unroll
      for (uint32_t h = 0; h < RB / 2; ++h) {
        xr[2 * h] = double(x4[h].x);
        xi[2 * h] = double(x4[h].y);
        xr[2 * h + 1] = double(x4[h].z);
        xi[2 * h + 1] = double(x4[h].w);
        // w_m times the column operand, once per amplitude
        yr[2 * h] = WEIGHTED ? double(y4[h].x) * wm : double(y4[h].x);
        yi[2 * h] = WEIGHTED ? double(y4[h].y) * wm : double(y4[h].y);
        yr[2 * h + 1] = WEIGHTED ? double(y4[h].z) * wm : double(y4[h].z);
        yi[2 * h + 1] = WEIGHTED ? double(y4[h].w) * wm : double(y4[h].w);
      }
#pragma unroll
      for (uint32_t r = 0; r < RB; ++r)
#pragma unroll
        for (uint32_t c = 0; c < RB; ++c) {
          double s = re[r * RB + c], t = im[r * RB + c];
          s = __builtin_fma(xr[r], yr[c], s);
          s = __builtin_fma(xi[r], yi[c], s);
          t = __builtin_fma(xi[r], yr[c], t);
          t = __builtin_fma(-xr[r], yi[c], t);
          re[r * RB + c] = s;
          im[r * RB + c] = t;
        }
    }
    __syncthreads();
  }
#undef RDM_FETCH

  // the groups of a wave in a fixed shuffle tree (lanes below GW hold the sums), then the waves in wave order
  if (G < 64) {
#pragma unroll
    for (uint32_t p = 0; p < NO; ++p)
#pragma unroll
      for (uint32_t off = 32; off >= G; off >>= 1) {
        re[p] += __shfl_down(re[p], off, 64);
        im[p] += __shfl_down(im[p], off, 64);
      }
  }
  double* out = part + ((uint64_t(blockIdx.x) * a.slices + blockIdx.y) << (2u * KT + 1u));
  const uint32_t lane = tid & 63u, wave = tid >> 6;
  double* red = reinterpret_cast<double*>(&panel[0][0]);  // [4 waves][GW][2] (the loop ended in a barrier)
#pragma unroll
  for (uint32_t p = 0; p < NO; ++p) {
    double r = re[p], s = im[p];
    if (G < kRdmThreads) {
      if (lane < GW) {
        red[(wave * GW + lane) * 2u] = r;
        red[(wave * GW + lane) * 2u + 1u] = s;
      }
      __syncthreads();
      if (tid < GW) {
        r = red[tid * 2u];
        s = red[tid * 2u + 1u];
        for (uint32_t w = 1; w < kRdmThreads / 64; ++w) {
          r += red[(w * GW + tid) * 2u];
          s += red[(w * GW + tid) * 2u + 1u];
        }
      }
    }
    if (G == kRdmThreads || tid < GW) {
      const uint32_t row = bi * RB + p / RB, col = bj * RB + p % RB;
      out[(row * TE + col) * 2u] = r;
      out[(row * TE + col) * 2u + 1u] = s;
    }
    if (G < kRdmThreads) __syncthreads();
  }
}

// One thread per entry of a tile (blockIdx.y = the tile); the entries below the diagonal have nothing to do.
// part [tiles, slices, 4^kt, 2], rho [2^k, 2^k, 2]
__global__ __launch_bounds__(kRdmThreads) void rdm_finish_kernel(const double* __restrict__ part, uint32_t kt, uint32_t k,
                                                                uint32_t tile_rows, uint32_t slices, double* __restrict__ rho) {
  const uint32_t entry = blockIdx.x * kRdmThreads + threadIdx.x, edge = 1u << kt;
  if (entry >= edge * edge) return;
  uint32_t ti, tj;
  rdm_tile_of(tile_rows, blockIdx.y, &ti, &tj);
  const uint32_t r = entry >> kt, c = entry & (edge - 1u);
  const uint64_t row = (uint64_t(ti) << kt) | r, col = (uint64_t(tj) << kt) | c;
  if (col < row) return;
  const double* p = part + ((uint64_t(blockIdx.y) * slices) << (2u * kt + 1u)) + 2u * entry;
  double re = 0.0, im = 0.0;
#pragma unroll 4
  for (uint32_t s = 0; s < slices; ++s) {
    re += p[uint64_t(s) << (2u * kt + 1u)];
    im += p[(uint64_t(s) << (2u * kt + 1u)) + 1u];
  }
  double* up = rho + ((row << k) + col) * 2u;
  up[0] = re;
  up[1] = row == col ? 0.0 : im;
  if (row != col) {
    double* lo = rho + ((col << k) + row) * 2u;
    lo[0] = re;
    lo[1] = -im;
  }
}

template <uint32_t KT>
void rdm_launch_tiles(dim3 grid, hipStream_t stream, const float2* states, const double* weights, const RdmArgs& a,
                      double* part) {
  if (weights)
    hipLaunchKernelGGL((rdm_tile_kernel<KT, true>), grid, dim3(kRdmThreads), 0, stream, states, weights, a, part);
  else
    hipLaunchKernelGGL((rdm_tile_kernel<KT, false>), grid, dim3(kRdmThreads), 0, stream, states, weights, a, part);
}

}  // namespace

hipError_t launch_reduced_density(const float2* states, uint32_t M, uint32_t n, uint64_t keep_mask, const double* weights,
                                  double* parts, double* rho, hipStream_t stream) {
  if (rdm_check(int(n), keep_mask) != 0 || M < 1 || M > uint32_t(kRdmMaxStates)) return hipErrorInvalidValue;
  const RdmPlan p = rdm_plan(int(n), keep_mask, int(M));
  RdmArgs a;
  a.n = p.n;
  a.le = p.le;
  a.nv = p.nv;
  a.tile_rows = p.tile_rows;
  a.slices = p.slices;
  a.keep = p.masks.keep;
  a.env_hi = p.env_hi;
  a.blocks_per_state = p.blocks_per_state;
  a.blocks = p.blocks;
  a.gpos = p.gpos_packed;
  a.lpos = p.lpos_packed;
  const dim3 grid(p.tiles, p.slices);
  switch (p.kt) {
    case 1: rdm_launch_tiles<1>(grid, stream, states, weights, a, parts); break;
    case 2: rdm_launch_tiles<2>(grid, stream, states, weights, a, parts); break;
    case 3: rdm_launch_tiles<3>(grid, stream, states, weights, a, parts); break;
    case 4: rdm_launch_tiles<4>(grid, stream, states, weights, a, parts); break;
    case 5: rdm_launch_tiles<5>(grid, stream, states, weights, a, parts); break;
    case 6: rdm_launch_tiles<6>(grid, stream, states, weights, a, parts); break;
    default: return hipErrorInvalidValue;
  }
  const uint32_t entries = 1u << (2u * p.kt);
  hipLaunchKernelGGL(rdm_finish_kernel, dim3((entries + kRdmThreads - 1u) / kRdmThreads, p.tiles), dim3(kRdmThreads), 0,
                     stream, parts, p.kt, p.k, p.tile_rows, p.slices, rho);
  return hipGetLastError();
}

}  // namespace qhbm
