// Gibbs-With-Gradients chains for spin-parity energies; part of kernels.hip's
// translation unit (#include "gwg.hip" after the parity kernels, inside namespace qhbm).
//
// For E(x) = sum_k theta_k prod_{q in S_k} (1 - 2 x_q) -- BernoulliEnergy / KOBE, the form parity_energy_kernel computes
// -- the energy is multilinear in x, so the sampler's Taylor estimate (qhbmlib/inference/ebm.py:618-650) is exact:
//   d_j(x) = (2 x_j - 1) dE/dx_j = E(x) - E(x ^ e_j) = 2 h_j(x),   h_j(x) = sum_{k : j in S_k} theta_k s_k(x),
// s_k(x) = (-1)^popcount(x & mask_k).  With L(x) = logsumexp_j h_j(x) the index proposal is q(j | x) = exp(h_j(x) - L(x))
// and the Metropolis-Hastings acceptance exp(E(x) - E(x')) q(i | x') / q(i | x) of ebm.py:674-678 equals exp(L(x) - L(x'))
// (h_i(x') = -h_i(x)).  A chain is a pure function of (theta, masks, x_0, random stream).
//
// One workgroup of ONE wave per chain; lane j owns bit j (n_bits <= 64); the state is one wave-uniform uint64 with
// column q in bit q (pack_bits).  LDS holds the term table (mask 8 B + theta 4 B per term) and, per bit, a MEMBERSHIP
// BITMAP over the terms (word w of bit j at memb[w * n_bits + j]: consecutive lanes, consecutive banks).  Lane j walks the
// set bits of its bitmap in ascending term order.  The bitmap takes the place of index lists because its size is a
// function of (n_terms, n_bits) alone: the host decides whether the terms fit without reading the device-resident masks
// (no synchronisation), and it is the smaller of the two whenever more than one term in sixteen holds a given bit.
//
// Random stream: Philox4x32-10 (philox4x32_10 of the shot sampler), key = seed, counter = {step low, step high,
// kGwgCounterTag, chain} with the ABSOLUTE step index; output words 0,1 -> u1 (index pick), 2,3 -> u2 (acceptance), each
// c_a 2^-32 + c_b 2^-64 in fp64 as the shot sampler forms its uniform.  Nothing depends on the grid, on how the steps are
// cut into launches, or on whether the samples are written.  No atomics, no spin loops: the only loop bounds are n_steps
// and the term lists.

constexpr uint32_t kGwgCounterTag = 0x47574731u;  // "GWG1"; the shot sampler's third counter word is 0x51b0c6a1
constexpr int64_t kGwgStepSlice = 65536;          // steps per launch (the absolute step counter makes the cut invisible)

size_t gwg_lds_bytes(int n_bits, int n_terms) {
  const size_t words = (size_t(n_terms) + 31u) / 32u;
  return (12u * size_t(n_terms) + 4u * words * size_t(n_bits) + 15u) & ~size_t(15);
}

// h_j(x) of this lane's bit, the inclusive lane-order prefix of p_j = exp(h_j - max h) and L(x) = max h + log(sum p).
__device__ __forceinline__ void gwg_evaluate(uint64_t x, int lane, int n_bits, int n_words, const uint64_t* sm,
                                             const float* st, const uint32_t* memb, float& incl, float& total,
                                             float& log_norm) {
  const bool live = lane < n_bits;
  float h = 0.f;
  for (int w = 0; w < n_words; ++w) {
    uint32_t m = live ? memb[w * n_bits + lane] : 0u;
    while (m) {
      const int k = w * 32 + __builtin_ctz(m);
      m &= m - 1u;
      const float th = st[k];
      h += (__popcll(x & sm[k]) & 1) ? -th : th;
    }
  }
  if (!live) h = -INFINITY;
  float top = h;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) top = fmaxf(top, __shfl_xor(top, off));
  incl = live ? expf(h - top) : 0.f;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const float t = __shfl_up(incl, k);
    if (lane >= k) incl += t;
  }
  total = __shfl(incl, 63);
  log_norm = top + logf(total);
}

__global__ __launch_bounds__(64) void gwg_chain_kernel(uint64_t* __restrict__ states, int n_chains, int n_bits,
                                                       const uint64_t* __restrict__ masks,
                                                       const float* __restrict__ thetas, int n_terms, uint64_t seed,
                                                       uint64_t step0, int n_steps, int8_t* __restrict__ out,
                                                       int32_t* __restrict__ accepted, int add_accepted) {
  extern __shared__ __attribute__((aligned(16))) unsigned char gwg_lds[];
  uint64_t* sm = reinterpret_cast<uint64_t*>(gwg_lds);
  float* st = reinterpret_cast<float*>(gwg_lds + 8u * size_t(n_terms));
  uint32_t* memb = reinterpret_cast<uint32_t*>(gwg_lds + 12u * size_t(n_terms));
  const int lane = int(threadIdx.x), n_words = (n_terms + 31) / 32;
  const uint32_t chain = blockIdx.x;
  const uint64_t live_bits = n_bits == 64 ? ~0ull : (1ull << n_bits) - 1ull;

  for (int k = lane; k < n_terms; k += 64) {
    sm[k] = masks[k] & live_bits;  // bits at or above n_bits never match, as in parity_energy_kernel
    st[k] = thetas[k];
  }
  __syncthreads();
  if (lane < n_bits)
    for (int w = 0; w < n_words; ++w) {
      uint32_t m = 0;
      const int kn = min(32, n_terms - w * 32);
      for (int t = 0; t < kn; ++t) m |= uint32_t((sm[w * 32 + t] >> lane) & 1ull) << t;
      memb[w * n_bits + lane] = m;
    }
  __syncthreads();

  uint64_t x = states[chain] & live_bits;
  float incl, total, log_norm;
  gwg_evaluate(x, lane, n_bits, n_words, sm, st, memb, incl, total, log_norm);
  int n_accepted = 0;
  for (int t = 0; t < n_steps; ++t) {
    const uint64_t step = step0 + uint64_t(t);
    uint32_t c[4] = {uint32_t(step), uint32_t(step >> 32), kGwgCounterTag, chain};
    philox4x32_10(c, uint32_t(seed), uint32_t(seed >> 32));
    const double u1 = double(c[0]) * 0x1p-32 + double(c[1]) * 0x1p-64;
    const double u2 = double(c[2]) * 0x1p-32 + double(c[3]) * 0x1p-64;
    // the first bit whose inclusive prefix exceeds u1 * sum; the last bit if rounding leaves none
    const uint64_t over = __ballot(lane < n_bits && double(incl) > u1 * double(total));
    const int pick = over ? __builtin_ctzll(over) : n_bits - 1;
    const uint64_t y = x ^ (1ull << pick);
    float incl_y, total_y, log_norm_y;
    gwg_evaluate(y, lane, n_bits, n_words, sm, st, memb, incl_y, total_y, log_norm_y);
    if (u2 <= double(expf(fminf(0.f, log_norm - log_norm_y)))) {
      x = y;
      incl = incl_y;
      total = total_y;
      log_norm = log_norm_y;
      ++n_accepted;
    }
    if (out && lane < n_bits) out[(int64_t(t) * n_chains + chain) * n_bits + lane] = int8_t((x >> lane) & 1ull);
  }
  if (lane == 0) {
    states[chain] = x;
    if (accepted) accepted[chain] = (add_accepted ? accepted[chain] : 0) + n_accepted;
  }
}

hipError_t launch_gwg_sample(uint64_t* states, int n_chains, int n_bits, const uint64_t* masks, const float* thetas,
                             int n_terms, uint64_t seed, uint64_t step0, int64_t n_steps, int8_t* out, int32_t* accepted,
                             hipStream_t stream) {
  if (n_chains == 0 || n_steps == 0) return hipSuccess;
  const size_t lds = gwg_lds_bytes(n_bits, n_terms);
  if (lds > kGwgLdsMax) return hipErrorInvalidValue;  // (qhbm_gwg_sample reports it before it gets here)
  static bool attr_done[kMaxDevices] = {};
  if (lds > 64u * 1024u)
    if (hipError_t e = opt_in_lds(gwg_chain_kernel, attr_done, kGwgLdsMax); e != hipSuccess) return e;
  for (int64_t t0 = 0; t0 < n_steps; t0 += kGwgStepSlice) {
    const int steps = int(std::min(kGwgStepSlice, n_steps - t0));
    hipLaunchKernelGGL(gwg_chain_kernel, dim3(unsigned(n_chains)), dim3(64), lds, stream, states, n_chains, n_bits, masks,
                       thetas, n_terms, seed, step0 + uint64_t(t0), steps,
                       out ? out + t0 * int64_t(n_chains) * n_bits : nullptr, accepted, t0 ? 1 : 0);
  }
  return hipGetLastError();
}
