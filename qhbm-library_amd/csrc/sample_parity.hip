// sample_parity.hip -- signed shot sums of Pauli-Z strings, drawn and reduced on the device (gfx950).  Part of the
// kernels.hip translation unit (#include "sample_parity.hip" after parity_table.hip, inside namespace qhbm).
//
// For element (program q, state row s) and T masks, out[q, s, t] = sum over shots j of (-1)^popcount(x_j & m_t), where
// x_j is drawn from |psi|^2 with the uniform of qhbm_sample_counts (Philox4x32-10, counter {j, s, 0x51b0c6a1, q}).  Neither
// the shots nor a counter per outcome are stored: qhbm_sample_parities, qhbm_sample_parities_states (engine.cpp),
// DESIGN.md 6k.
//
// The cumulative distribution is a three-level table in float64, built in ONE pass over the amplitudes:
//   sub-block   16 consecutive amplitudes (2^n when n < 4): mass = p_0 + p_1 + ... in index order, p = re^2 + im^2 with
//               both products exact in float64 and one rounding in their sum;
//   block       1024 amplitudes = 64 sub-blocks (2^n amplitudes when n < 10): sub_cum[b][s] = inclusive prefix of the
//               sub-block masses, a Hillis-Steele scan over the lanes of one wave (offsets 1, 2, 4, ...);
//   state       block_cum[b] = inclusive prefix of the block masses sub_cum[b][last] by block_scan_kernel; total = its
//               last entry.
// A shot with u * total = v (one float64 multiply) takes the first block b with block_cum[b] > v, r = v - block_cum[b - 1],
// the first sub-block s with sub_cum[b][s] > r, and the first amplitude of s at which sub_cum[b][s - 1] + p_0 + p_1 + ...
// (added in index order) exceeds r.  Where rounding leaves no such entry at a level -- u rounds to 1, or a scanned prefix
// and the sequential one differ in the last place -- the shot takes the LAST outcome of non-zero mass at or before the
// place the search reached: an outcome of zero mass is never drawn.  On states whose partial sums are exact in float64
// every order of additions gives the same table, and the outcome is that of the flat definition
// searchsorted(cumsum(p), u * total, side="right").
//
// shot_parity_draw_kernel: a LANE owns a shot.  A workgroup draws 4096 shots of one element (16 per lane; per shot
// n - 10 + 6 eight-byte reads of the tables and one 128-byte line of amplitudes), parks the outcomes in LDS, then every
// wave walks the masks: per mask and 64 shots one ballot of the parity bit and one scalar population count, added per
// workgroup in LDS and once per mask with an integer atomicAdd into `out`.  Integer atomics only: the sums do not depend
// on the order of the shots, the workgroups or the launch sets.

constexpr uint32_t kSpBlockBits = 10, kSpSubBits = 4;
constexpr uint32_t kSpThreads = 256, kSpShotsPerLane = 16, kSpShotsPerGroup = kSpThreads * kSpShotsPerLane;
constexpr uint32_t kSpMaskWords = 512;  // masks per staging launch: 2 KiB of kernel arguments

struct ShotParityMaskWords {
  uint32_t m[kSpMaskWords];
};

// The masks arrive as kernel arguments (the caller's array is in HOST memory and was validated there): no copy, nothing to
// synchronise with, capturable.
__global__ __launch_bounds__(kSpThreads) void shot_parity_masks_kernel(ShotParityMaskWords w, uint32_t count,
                                                                      uint32_t* __restrict__ dst) {
  for (uint32_t i = threadIdx.x; i < count; i += kSpThreads) dst[i] = w.m[i];
}

__device__ __forceinline__ double sp_mass(float re, float im) {
  return double(re) * double(re) + double(im) * double(im);
}

// grid (blocks of a state, elements), one wave: lane l sums sub-block l.  row_bits: amplitudes between two elements.
__global__ __launch_bounds__(64) void shot_parity_cdf_kernel(const float2* __restrict__ psi, uint32_t row_bits, uint32_t lb,
                                                             uint32_t ls, double* __restrict__ block_mass,
                                                             double* __restrict__ sub_cum) {
  const uint32_t lane = threadIdx.x, b = blockIdx.x, e = blockIdx.y;
  const uint32_t subs = 1u << (lb - ls), nb = 1u << (row_bits - lb);
  double mine = 0.0;
  if (lane < subs) {
    const float4* p = reinterpret_cast<const float4*>(psi + (size_t(e) << row_bits) + (size_t(b) << lb) + (size_t(lane) << ls));
    for (uint32_t k = 0; k < (1u << ls) / 2u; ++k) {
      const float4 v = p[k];
      mine += sp_mass(v.x, v.y);
      mine += sp_mass(v.z, v.w);
    }
  }
  double incl = mine;
#pragma unroll
  for (int k = 1; k < 64; k <<= 1) {
    const double t = __shfl_up(incl, k);
    if (int(lane) >= k) incl += t;
  }
  const size_t blk = size_t(e) * nb + b;
  if (lane < subs) sub_cum[(blk << (lb - ls)) + lane] = incl;
  if (lane == subs - 1u) block_mass[blk] = incl;
}

struct ShotParityArgs {
  const float2* psi;
  const double* block_cum;  // [elements, blocks]
  const double* sub_cum;    // [elements, blocks, sub-blocks]
  const uint32_t* masks;    // [T] in INDEX space
  int* out;                 // [programs, n_states_total, T]
  uint64_t seed;
  uint32_t row_bits, lb, ls, idx_mask, T, n_shots, prog_states, prog0, state0, n_states_total;
  uint32_t ctr_state, ctr_prog;  // added to the state row / program for the counter words alone
};

// grid (ceil(n_shots / 4096), elements)
__global__ __launch_bounds__(kSpThreads) void shot_parity_draw_kernel(ShotParityArgs a) {
  __shared__ int odd[1024];
  __shared__ uint32_t xs[kSpShotsPerGroup];
  const uint32_t tid = threadIdx.x, e = blockIdx.y;
  const uint32_t q = a.prog0 + e / a.prog_states, srow = a.state0 + e % a.prog_states;
  const uint32_t nb = 1u << (a.row_bits - a.lb), sb = a.lb - a.ls, subs = 1u << sb, pairs = (1u << a.ls) / 2u;
  const double* cum = a.block_cum + size_t(e) * nb;
  const double* sub = a.sub_cum + ((size_t(e) * nb) << sb);
  const float2* st = a.psi + (size_t(e) << a.row_bits);
  const double total = cum[nb - 1u];
  if (!(total > 0.0)) return;  // a state of no mass draws nothing (the same for the whole workgroup)
  for (uint32_t t = tid; t < a.T; t += kSpThreads) odd[t] = 0;
  const uint32_t shot0 = blockIdx.x * kSpShotsPerGroup;
  const double inf = __builtin_huge_val();

  for (uint32_t i = 0; i < kSpShotsPerLane; ++i) {
    const uint32_t shot = shot0 + i * kSpThreads + tid;
    uint32_t x = 0u;  // a shot past the end: even parity under every mask, taken out again below
    if (shot < a.n_shots) {
      uint32_t c[4] = {shot, a.ctr_state + srow, 0x51b0c6a1u, a.ctr_prog + q};
      philox4x32_10(c, uint32_t(a.seed), uint32_t(a.seed >> 32));
      const double v = (double(c[0]) * 0x1p-32 + double(c[1]) * 0x1p-64) * total;
      uint32_t lo = 0u, hi = nb - 1u;  // the first block whose inclusive prefix exceeds v
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (cum[mid] > v) hi = mid; else lo = mid + 1u;
      }
      uint32_t b = lo;
      double r;
      if (cum[b] > v && sub[(size_t(b) << sb) + subs - 1u] > 0.0) {
        r = v - (b ? cum[b - 1u] : 0.0);
      } else {  // nothing exceeds v, or rounding chose a block of no mass: the last outcome of the last block with mass
        while (b > 0u && !(sub[(size_t(b) << sb) + subs - 1u] > 0.0)) --b;
        r = inf;
      }
      const double* sc = sub + (size_t(b) << sb);
      lo = 0u, hi = subs - 1u;
      while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sc[mid] > r) hi = mid; else lo = mid + 1u;
      }
      uint32_t s = lo;
      if (!(sc[s] > r)) r = inf;
      int pick;
      for (;;) {
        const float4* p = reinterpret_cast<const float4*>(st + (size_t(b) << a.lb) + (size_t(s) << a.ls));
        double acc = s ? sc[s - 1u] : 0.0;
        int last = -1;
        pick = -1;
        for (uint32_t k = 0; k < pairs; ++k) {
          const float4 w = p[k];
          const double w0 = sp_mass(w.x, w.y), w1 = sp_mass(w.z, w.w);
          acc += w0;
          if (w0 > 0.0) {
            last = int(2u * k);
            if (pick < 0 && acc > r) pick = last;
          }
          acc += w1;
          if (w1 > 0.0) {
            last = int(2u * k + 1u);
            if (pick < 0 && acc > r) pick = last;
          }
        }
        if (pick < 0) pick = last;
        if (pick >= 0 || s == 0u) break;
        --s;  // a sub-block of no mass: the last outcome with mass before it
        r = inf;
      }
      if (pick < 0) pick = 0;
      x = ((b << a.lb) + (s << a.ls) + uint32_t(pick)) & a.idx_mask;
    }
    xs[i * kSpThreads + tid] = x;
  }
  __syncthreads();  // (odd[] is zeroed; each thread reads back its own outcomes)
  uint32_t x[kSpShotsPerLane];
#pragma unroll
  for (uint32_t i = 0; i < kSpShotsPerLane; ++i) x[i] = xs[i * kSpThreads + tid];
  for (uint32_t t = 0; t < a.T; ++t) {
    const uint32_t m = a.masks[t];
    int cnt = 0;
#pragma unroll
    for (uint32_t i = 0; i < kSpShotsPerLane; ++i) cnt += __popcll(__ballot((__popc(x[i] & m) & 1) != 0));
    if ((tid & 63u) == 0u && cnt) atomicAdd(&odd[t], cnt);
  }
  __syncthreads();
  const int drawn = int(min(kSpShotsPerGroup, a.n_shots - shot0));
  int* o = a.out + (size_t(q) * a.n_states_total + srow) * a.T;
  for (uint32_t t = tid; t < a.T; t += kSpThreads) {
    const int sum = drawn - 2 * odd[t];
    if (sum) atomicAdd(&o[t], sum);
  }
}

size_t shot_parity_table_doubles(uint32_t row_bits, size_t n_elements) {
  const uint32_t lb = std::min(row_bits, kSpBlockBits), ls = std::min(row_bits, kSpSubBits);
  return n_elements * ((size_t(1) << (row_bits - lb)) + (size_t(1) << (row_bits - ls)));
}

hipError_t launch_shot_parity_masks(const uint32_t* host_masks, uint32_t T, uint32_t* d_masks, hipStream_t stream) {
  for (uint32_t t0 = 0; t0 < T; t0 += kSpMaskWords) {
    ShotParityMaskWords w;
    const uint32_t count = std::min(kSpMaskWords, T - t0);
    memcpy(w.m, host_masks + t0, count * sizeof(uint32_t));
    memset(w.m + count, 0, (kSpMaskWords - count) * sizeof(uint32_t));
    hipLaunchKernelGGL(shot_parity_masks_kernel, dim3(1), dim3(kSpThreads), 0, stream, w, count, d_masks + t0);
  }
  return hipGetLastError();
}

hipError_t launch_shot_parities(const float2* psi, uint32_t row_bits, int n_user, uint32_t n_elements, uint32_t prog_states,
                                uint32_t prog0, double* tables, const uint32_t* d_masks, uint32_t T, uint32_t n_shots,
                                uint64_t seed, uint32_t state0, uint32_t n_states_total, uint32_t ctr_state, uint32_t ctr_prog, int* out,
                                hipStream_t stream) {
  if (!n_elements || !n_shots) return hipSuccess;
  if (n_elements > 65535u || T < 1u || T > 1024u || row_bits < 1u || row_bits > 31u || n_user < 1 || uint32_t(n_user) > row_bits)
    return hipErrorInvalidValue;
  const uint32_t lb = std::min(row_bits, kSpBlockBits), ls = std::min(row_bits, kSpSubBits), nb = 1u << (row_bits - lb);
  double* block_cum = tables;
  double* sub_cum = tables + size_t(n_elements) * nb;
  hipLaunchKernelGGL(shot_parity_cdf_kernel, dim3(nb, n_elements), dim3(64), 0, stream, psi, row_bits, lb, ls, block_cum,
                     sub_cum);
  hipLaunchKernelGGL(block_scan_kernel, dim3(n_elements), dim3(256), 0, stream, block_cum, nb);
  ShotParityArgs a;
  a.psi = psi;
  a.block_cum = block_cum;
  a.sub_cum = sub_cum;
  a.masks = d_masks;
  a.out = out;
  a.seed = seed;
  a.row_bits = row_bits;
  a.lb = lb;
  a.ls = ls;
  a.idx_mask = uint32_t((uint64_t(1) << n_user) - 1u);
  a.T = T;
  a.n_shots = n_shots;
  a.prog_states = prog_states;
  a.prog0 = prog0;
  a.state0 = state0;
  a.n_states_total = n_states_total;
  a.ctr_state = ctr_state;
  a.ctr_prog = ctr_prog;
  const uint32_t groups = uint32_t((uint64_t(n_shots) + kSpShotsPerGroup - 1u) / kSpShotsPerGroup);
  hipLaunchKernelGGL(shot_parity_draw_kernel, dim3(groups, n_elements), dim3(kSpThreads), 0, stream, a);
  return hipGetLastError();
}
