// Spin-parity energy tables by a fast Walsh-Hadamard transform; part of kernels.hip's translation unit
// (#include "parity_table.hip" after gwg.hip, inside namespace qhbm).
//
// E(x) = sum_k theta_k (-1)^popcount(x & mask_k) over ALL 2^n bitstrings is the unnormalised Walsh-Hadamard transform
//   H[y] = sum_m c[m] (-1)^popcount(y & m)
// of the coefficient vector c that holds theta_k at index mask_k, and the VJP sum_y w[y] parity_k(y) is entry mask_k of
// the transform of w: n 2^n additions either way instead of T 2^n parity evaluations, and no bitstring table.
//
// Pass structure (the shape of the pass kernels): a workgroup of 512 threads keeps a tile of 2^14 floats on chip for a
// whole pass, 32 per thread.  A tile index t has 5 CARRIER bits (t & 31 = index bits 0..4: one 128-byte line) and 9 ROW
// bits that sit at index bits s..s+8; the workgroup number supplies the rest.  Pass 0 has s = 5 (a contiguous tile) and
// butterflies all 14 bits; a later pass takes its 9 row bits strided and butterflies only those the earlier passes have
// not done (`active`, a mask over tile bits).  Inside a pass the 32 registers of a thread take three geometries:
//   round 1  registers = tile bits 9..13   (global load: lanes run over bits 0..8, two whole lines per wave instruction)
//   round 2  registers = tile bits 0..4    (pass 0 only)
//   round 3  registers = tile bits 5..8,13 (global store: lanes run over bits 0..4 and 9..12, two whole lines again)
// with the butterflies of the register bits in registers and the geometry changes through LDS, padded by one float per 32
// so that every exchange is free of bank conflicts.  n < 14 is one launch of one workgroup that transforms in LDS.
// The butterfly order is a function of n alone: results are bit-identical from call to call.  No atomics.

constexpr int kWhtTileBits = 14;   // floats of a tile, log2: n <= kWhtTileBits is a single launch
constexpr int kWhtCarrierBits = 5; // low index bits every pass keeps: 32 floats = one 128-byte line
constexpr int kWhtRowBits = kWhtTileBits - kWhtCarrierBits;  // new index bits of a later pass
constexpr int kWhtThreads = 512, kWhtRegs = 32;
constexpr int kWhtMaxBits = 30;

int wht_num_passes(int n_bits) {
  return n_bits <= kWhtTileBits ? 1 : 1 + (n_bits - kWhtTileBits + kWhtRowBits - 1) / kWhtRowBits;
}

// Butterflies over the register-index bits [0, BITS) whose flag in `on` (bit b = register bit b) is set.
template <int BITS>
__device__ __forceinline__ void wht_registers(float (&v)[kWhtRegs], uint32_t on) {
#pragma unroll
  for (int b = 0; b < BITS; ++b) {
    if ((on >> b) & 1u) {
#pragma unroll
      for (int j = 0; j < kWhtRegs; ++j) {
        if (!(j & (1 << b))) {
          const float lo = v[j], hi = v[j | (1 << b)];
          v[j] = lo + hi;
          v[j | (1 << b)] = lo - hi;
        }
      }
    }
  }
}

// LDS image of tile index t: one float of padding per 32, so that every geometry of a pass puts the 32 lanes of a bank
// group on 32 banks (lane strides 1 and 33) and every register's address is the thread's plus a constant.
__device__ __forceinline__ uint32_t wht_pad(uint32_t t) { return t + (t >> 5); }
constexpr int kWhtLdsFloats = (1 << kWhtTileBits) + (1 << (kWhtTileBits - 5));  // 66 KiB: two workgroups per CU

// One pass over a tile.  `s`: index position of the tile's row bits; `active`: tile bits to butterfly; `low`: pass 0,
// whose carriers are butterflied too.  src == dst (in place: no __restrict__) or disjoint.
// (two workgroups per CU, as the 66 KiB of LDS allow: at most 128 VGPRs)
__global__ __launch_bounds__(kWhtThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void wht_pass_kernel(const float* src, float* dst,
                                                               int s, uint32_t active, int low) {
  __shared__ float tile[kWhtLdsFloats];
  const uint32_t t = threadIdx.x, wg = blockIdx.x;
  const uint32_t wg_lo = wg & ((1u << (s - kWhtCarrierBits)) - 1u), wg_hi = wg >> (s - kWhtCarrierBits);
  const size_t base = (size_t(wg_lo) << kWhtCarrierBits) | (size_t(wg_hi) << (s + kWhtRowBits));
  float v[kWhtRegs];
  // Addresses are a wave-uniform 64-bit part (the workgroup's base and the register's rows: scalar registers) plus a
  // 32-bit offset of the thread (below 2^29 floats): byte offsets pass 2^32 at n = 30.
  const uint32_t t_lo = t & 31u, t_hi = t >> 5;
  const uint32_t off1 = t_lo + (t_hi << s);        // round 1: rows (j << 4) | t_hi
  const uint32_t off3 = t_lo + (t_hi << (s + 4));  // round 3: rows ((j >> 4) << 8) | (t_hi << 4) | (j & 15)

  // round 1: register j = tile bits 9..13, thread = tile bits 0..8
#pragma unroll
  for (int j = 0; j < kWhtRegs; ++j) v[j] = (src + base + (size_t(j) << (s + 4)))[off1];
  wht_registers<5>(v, active >> 9);
  const uint32_t mid = (active >> 5) & 15u;
  if (!low && !mid) {  // (a last pass with at most 5 new bits) the load geometry stores whole lines as well
#pragma unroll
    for (int j = 0; j < kWhtRegs; ++j) (dst + base + (size_t(j) << (s + 4)))[off1] = v[j];
    return;
  }
#pragma unroll
  for (int j = 0; j < kWhtRegs; ++j) tile[wht_pad((uint32_t(j) << 9) | t)] = v[j];
  __syncthreads();

  if (low) {  // round 2: register j = tile bits 0..4, thread = tile bits 5..13 (each thread rewrites what it read)
#pragma unroll
    for (int j = 0; j < kWhtRegs; ++j) v[j] = tile[t * 33u + uint32_t(j)];
    wht_registers<5>(v, active & 31u);
#pragma unroll
    for (int j = 0; j < kWhtRegs; ++j) tile[t * 33u + uint32_t(j)] = v[j];
    __syncthreads();
  }

  // round 3: register j = tile bits 5..8 (j & 15) and 13 (j >> 4), thread = tile bits 0..4 and 9..12
#pragma unroll
  for (int j = 0; j < kWhtRegs; ++j) {
    const uint32_t idx = (uint32_t(j >> 4) << 13) | (t_hi << 9) | (uint32_t(j & 15) << 5) | t_lo;
    v[j] = tile[wht_pad(idx)];
  }
  wht_registers<4>(v, mid);
#pragma unroll
  for (int j = 0; j < kWhtRegs; ++j)
    (dst + base + (size_t((uint32_t(j >> 4) << 8) | uint32_t(j & 15)) << s))[off3] = v[j];
}

// n < kWhtTileBits: one workgroup, the whole array in LDS, one level per barrier.
__global__ __launch_bounds__(256) void wht_small_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
  __shared__ float a[1 << (kWhtTileBits - 1)];
  const uint32_t size = 1u << n, tid = threadIdx.x;
  for (uint32_t i = tid; i < size; i += 256u) a[i] = src[i];
  for (int b = 0; b < n; ++b) {
    __syncthreads();
    for (uint32_t p = tid; p < size / 2u; p += 256u) {
      const uint32_t i = ((p >> b) << (b + 1)) | (p & ((1u << b) - 1u));
      const float lo = a[i], hi = a[i | (1u << b)];
      a[i] = lo + hi;
      a[i | (1u << b)] = lo - hi;
    }
  }
  __syncthreads();
  for (uint32_t i = tid; i < size; i += 256u) dst[i] = a[i];
}

__device__ __forceinline__ uint64_t wht_table_index(uint64_t mask, int n) {
  // column q of a bitstring is mask bit q; table index y holds column q at bit n-1-q (all_bitstrings, qhbm_statevector)
  return __brevll(mask & ((1ull << n) - 1ull)) >> (64 - n);   // mask bits at or above n are ignored (1 <= n <= 30)
}

// c[rev_n(mask_k)] += theta_k on a zeroed c.  One thread per term; the first occurrence of a mask adds its duplicates in
// ascending term order and is the only writer of its entry.
__global__ __launch_bounds__(256) void parity_scatter_kernel(const uint64_t* __restrict__ masks,
                                                             const float* __restrict__ thetas, int n_terms, int n,
                                                             float* __restrict__ c) {
  const int k = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (k >= n_terms) return;
  const uint64_t live = (1ull << n) - 1ull, m = masks[k] & live;
  for (int j = 0; j < k; ++j)
    if ((masks[j] & live) == m) return;
  float sum = thetas[k];
  for (int j = k + 1; j < n_terms; ++j)
    if ((masks[j] & live) == m) sum += thetas[j];
  c[wht_table_index(m, n)] = sum;
}

__global__ __launch_bounds__(256) void parity_gather_kernel(const uint64_t* __restrict__ masks, int n_terms, int n,
                                                            const float* __restrict__ buf, float* __restrict__ grad) {
  const int k = int(blockIdx.x) * 256 + int(threadIdx.x);
  if (k < n_terms) grad[k] = buf[wht_table_index(masks[k], n)];
}

// dst = WHT(src); src == dst transforms in place, otherwise src is only read (the first pass moves the data).
hipError_t launch_walsh_hadamard(const float* src, float* dst, int n_bits, hipStream_t stream) {
  if (n_bits < 1 || n_bits > kWhtMaxBits) return hipErrorInvalidValue;
  if (n_bits < kWhtTileBits) {
    hipLaunchKernelGGL(wht_small_kernel, dim3(1), dim3(256), 0, stream, src, dst, n_bits);
    return hipGetLastError();
  }
  const uint32_t grid = 1u << (n_bits - kWhtTileBits);
  hipLaunchKernelGGL(wht_pass_kernel, dim3(grid), dim3(kWhtThreads), 0, stream, src, dst, kWhtCarrierBits,
                     (1u << kWhtTileBits) - 1u, 1);
  // later passes: 9 row bits each from `done` on; the last one is moved down so that its rows end at bit n - 1 and
  // butterflies only the bits from `done` up
  for (int done = kWhtTileBits; done < n_bits; done += kWhtRowBits) {
    const int s = std::min(done, n_bits - kWhtRowBits);
    const int fresh = std::min(kWhtRowBits, n_bits - done);
    const uint32_t rows_on = ((1u << fresh) - 1u) << (done - s);
    hipLaunchKernelGGL(wht_pass_kernel, dim3(grid), dim3(kWhtThreads), 0, stream, dst, dst, s,
                       rows_on << kWhtCarrierBits, 0);
  }
  return hipGetLastError();
}

hipError_t launch_parity_table(const uint64_t* masks, const float* thetas, int n_terms, int n_bits, float* table,
                               hipStream_t stream) {
  if (n_bits < 1 || n_bits > kWhtMaxBits) return hipErrorInvalidValue;
  if (hipError_t e = launch_zero_fill(table, sizeof(float) << n_bits, stream); e != hipSuccess) return e;
  if (n_terms == 0) return hipSuccess;
  hipLaunchKernelGGL(parity_scatter_kernel, dim3(unsigned((n_terms + 255) / 256)), dim3(256), 0, stream, masks, thetas,
                     n_terms, n_bits, table);
  return launch_walsh_hadamard(table, table, n_bits, stream);
}

hipError_t launch_parity_table_vjp(const uint64_t* masks, int n_terms, int n_bits, const float* weights, float* scratch,
                                   float* grad, hipStream_t stream) {
  if (n_bits < 1 || n_bits > kWhtMaxBits) return hipErrorInvalidValue;
  if (n_terms == 0) return hipSuccess;
  if (hipError_t e = launch_walsh_hadamard(weights, scratch, n_bits, stream); e != hipSuccess) return e;
  hipLaunchKernelGGL(parity_gather_kernel, dim3(unsigned((n_terms + 255) / 256)), dim3(256), 0, stream, masks, n_terms,
                     n_bits, scratch, grad);
  return hipGetLastError();
}
