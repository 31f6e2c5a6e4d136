// rdm_index.h -- index arithmetic and launch plan of the reduced density matrix, shared by reduced.hip's kernels and the
// host (tests/rdm_index/rdm_index_check.cpp checks it on the CPU for every register of up to 12 qubits and every mask).
//
//   rho_A[a, a'] = sum_m w_m sum_b phi_m(a, b) conj(phi_m(a', b))            (include/qhbm_engine.h qhbm_reduced_density)
//
// Conventions (the header's): qubit 0 is the MOST significant bit of an amplitude index, so qubit q sits on index bit
// n - 1 - q.  `keep_mask` is in QUBIT space (bit q set <=> qubit q is kept); RdmMasks holds it in INDEX space.  Row index a
// of rho_A is the kept qubits' bits read big-endian in ascending qubit order -- bit j of a is the j-th lowest kept index
// bit -- and b is the same for the environment: (a, b) -> index is two bit deposits, index -> (a, b) two extracts.
//
// The plan (a function of n, keep_mask and M alone).  rho_A is cut into tiles of edge 2^kt, kt = min(k, 6); only tiles
// with j0 >= i0 are launched.  The environment (m, b) of M 2^(n - k) values is cut into blocks of 2^le values of one state
// that share b's high bits, le = min(n - k, 11 - kt): a block's panel -- a tile row's 2^kt rows at the block's 2^le
// environment values -- is at most 2048 amplitudes, and its amplitudes differ in the index bits `gpos`: the kt lowest kept
// and the le lowest environment bits.  Index bit 0 is always one of them, so a panel is read in 16-byte words whichever
// kind bit 0 is.  Panel element L (its bits deposited on gpos in ascending order) is row r, environment value e of the
// block, and has slot e 2^kt + r -- bit i of L moves the slot by 2^lpos[i] -- which rdm_lds_slot places in LDS.  The blocks are dealt to `slices`
// workgroups per tile in contiguous, ascending runs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define QHBM_RDM_HD __host__ __device__
#else
#define QHBM_RDM_HD
#endif

namespace qhbm {

constexpr int kRdmMaxKeep = 10;          // rho_A has at most 2^10 rows
constexpr int kRdmMaxQubits = 31;
constexpr int kRdmMaxStates = 65536;
constexpr int kRdmMaxTileBits = 6;       // tile edge 64: 256 threads x (4 x 4) outputs
constexpr int kRdmPanelBits = 11;        // a panel holds at most 2048 amplitudes (16 KiB)
constexpr uint32_t kRdmThreads = 256;
constexpr uint32_t kRdmMaxSlices = 512;
constexpr uint32_t kRdmTargetGroups = 1024;  // tiles x slices aims at this many workgroups

QHBM_RDM_HD inline int rdm_popcount(uint64_t v) {
  int c = 0;
  for (; v; v &= v - 1) ++c;
  return c;
}
// bits of v on the set bits of mask, lowest first / the bits of idx under mask, packed
QHBM_RDM_HD inline uint32_t rdm_deposit(uint32_t v, uint32_t mask) {
  uint32_t out = 0;
  for (uint32_t bit = 1; mask; bit <<= 1) {
    const uint32_t low = mask & (0u - mask);
    if (v & bit) out |= low;
    mask &= mask - 1;
  }
  return out;
}
QHBM_RDM_HD inline uint32_t rdm_extract(uint32_t idx, uint32_t mask) {
  uint32_t out = 0;
  for (uint32_t bit = 1; mask; bit <<= 1) {
    const uint32_t low = mask & (0u - mask);
    if (idx & low) out |= bit;
    mask &= mask - 1;
  }
  return out;
}
// the successor of `cur` among the values whose bits lie in mask (wraps to 0)
QHBM_RDM_HD inline uint32_t rdm_masked_inc(uint32_t cur, uint32_t mask) { return ((cur | ~mask) + 1u) & mask; }

struct RdmMasks {
  uint32_t keep;  // INDEX space: bit n - 1 - q for every kept qubit q
  uint32_t env;   // the other bits below 2^n
};

// 0, or why (n_qubits, keep_mask) is refused: 1 n_qubits, 2 a mask bit at or above n_qubits, 3 the number of kept qubits
QHBM_RDM_HD inline int rdm_check(int n, uint64_t keep_mask) {
  if (n < 1 || n > kRdmMaxQubits) return 1;
  if (keep_mask >> n) return 2;
  const int k = rdm_popcount(keep_mask);
  if (k < 1 || k > (n < kRdmMaxKeep ? n : kRdmMaxKeep)) return 3;
  return 0;
}

QHBM_RDM_HD inline RdmMasks rdm_masks(int n, uint64_t keep_mask) {
  RdmMasks m;
  m.keep = 0;
  for (int q = 0; q < n; ++q)
    if ((keep_mask >> q) & 1u) m.keep |= 1u << (n - 1 - q);
  m.env = uint32_t((uint64_t(1) << n) - 1u) & ~m.keep;
  return m;
}
QHBM_RDM_HD inline uint32_t rdm_amp_index(const RdmMasks& m, uint32_t a, uint32_t b) {
  return rdm_deposit(a, m.keep) | rdm_deposit(b, m.env);
}
QHBM_RDM_HD inline void rdm_split_index(const RdmMasks& m, uint32_t idx, uint32_t* a, uint32_t* b) {
  *a = rdm_extract(idx, m.keep);
  *b = rdm_extract(idx, m.env);
}

struct RdmPlan {
  uint32_t n, k, M;
  RdmMasks masks;
  uint32_t kt;               // log2 of the tile edge
  uint32_t le;               // log2 of the environment values of one block
  uint32_t rb;               // edge of a thread's register block: min(2^kt, 4)
  uint32_t group;            // threads that share one environment value: (2^kt / rb)^2
  uint32_t tile_rows, tiles; // tiles along an edge; tiles with j0 >= i0
  uint32_t env_hi;           // INDEX space: the environment bits above a block's
  uint64_t blocks_per_state, blocks;
  uint32_t slices;
  uint32_t nv;               // kt + le: bits of a panel element
  uint8_t gpos[kRdmPanelBits];  // bit i of a panel element -> index bit gpos[i]
  uint8_t lpos[kRdmPanelBits];  // ... -> LDS slot bit lpos[i]
  uint64_t gpos_packed, lpos_packed;  // the same tables, five bits an entry (what the kernel takes: rdm_packed)
  size_t scratch_bytes;      // tiles * slices * 4^kt * 2 doubles
};

QHBM_RDM_HD inline uint32_t rdm_packed(uint64_t packed, uint32_t i) { return uint32_t(packed >> (5u * i)) & 31u; }

// How rdm_tile_kernel's threads share a panel: thread tid takes the 16-byte words of elements L = 2 (tid + 256 w) and
// L + 1, w < 4, while tid + 256 w < 2^(nv - 1).  Both maps of rdm_panel_offsets are bitwise, so the offsets of L are the OR
// of a part that depends on tid alone (bits 1..8 of L) and a part that depends on w alone (bits 9, 10); element L + 1 adds
// index offset 1 and slot bit lpos[0].
QHBM_RDM_HD inline void rdm_thread_part(uint64_t gpos, uint64_t lpos, uint32_t nv, uint32_t tid, uint32_t* goff,
                                        uint32_t* slot) {
  uint32_t g = 0, s = 0;
  for (uint32_t i = 1; i < nv && i <= 8u; ++i)
    if ((tid >> (i - 1u)) & 1u) {
      g |= 1u << rdm_packed(gpos, i);
      s |= 1u << rdm_packed(lpos, i);
    }
  *goff = g;
  *slot = s;
}
QHBM_RDM_HD inline void rdm_word_part(uint64_t gpos, uint64_t lpos, uint32_t nv, uint32_t w, uint32_t* goff,
                                      uint32_t* slot) {
  uint32_t g = 0, s = 0;
  if ((w & 1u) && nv > 9u) {
    g |= 1u << rdm_packed(gpos, 9);
    s |= 1u << rdm_packed(lpos, 9);
  }
  if ((w & 2u) && nv > 10u) {
    g |= 1u << rdm_packed(gpos, 10);
    s |= 1u << rdm_packed(lpos, 10);
  }
  *goff = g;
  *slot = s;
}

// Where slot s = e 2^kt + r of a panel lives in LDS.  From kt = 3 on, bits 2.. of r are XOR-ed with the low bits of e: when
// the lanes of a wave store one row at consecutive environment values (the "high" masks: a lane stride of 2^kt slots, one
// bank for every lane) they now spread over 2^(kt - 2) bank groups.  A thread's register block reads 4 consecutive rows
// from a multiple of 4, which the swizzle keeps together; e and the two low bits of r are untouched.
QHBM_RDM_HD inline uint32_t rdm_lds_slot(uint32_t kt, uint32_t s) {
  if (kt < 3u) return s;
  return s ^ (((s >> kt) & ((1u << (kt - 2u)) - 1u)) << 2);
}

QHBM_RDM_HD inline RdmPlan rdm_plan(int n, uint64_t keep_mask, int M) {
  RdmPlan p;
  p.n = uint32_t(n);
  p.k = uint32_t(rdm_popcount(keep_mask));
  p.M = uint32_t(M);
  p.masks = rdm_masks(n, keep_mask);
  p.kt = p.k < uint32_t(kRdmMaxTileBits) ? p.k : uint32_t(kRdmMaxTileBits);
  const uint32_t room = uint32_t(kRdmPanelBits) - p.kt;
  p.le = p.n - p.k < room ? p.n - p.k : room;
  p.rb = p.kt < 2 ? (1u << p.kt) : 4u;
  p.group = ((1u << p.kt) / p.rb) * ((1u << p.kt) / p.rb);
  p.tile_rows = 1u << (p.k - p.kt);
  p.tiles = p.tile_rows * (p.tile_rows + 1u) / 2u;
  const uint32_t keep_lo = rdm_deposit((1u << p.kt) - 1u, p.masks.keep);
  const uint32_t env_lo = rdm_deposit((1u << p.le) - 1u, p.masks.env);
  p.env_hi = p.masks.env & ~env_lo;
  p.blocks_per_state = uint64_t(1) << (p.n - p.k - p.le);
  p.blocks = p.blocks_per_state * p.M;
  uint32_t want = 1;
  while (want * p.tiles < kRdmTargetGroups && want < kRdmMaxSlices) want <<= 1;
  p.slices = p.blocks < want ? uint32_t(p.blocks) : want;
  p.nv = p.kt + p.le;
  uint32_t v = keep_lo | env_lo, nk = 0, ne = 0;
  for (uint32_t i = 0; i < uint32_t(kRdmPanelBits); ++i) p.gpos[i] = p.lpos[i] = 0;
  for (uint32_t i = 0; v; ++i, v &= v - 1) {
    const uint32_t low = v & (0u - v);
    uint32_t pos = 0;
    while (!((low >> pos) & 1u)) ++pos;
    p.gpos[i] = uint8_t(pos);
    p.lpos[i] = uint8_t((low & keep_lo) ? nk++ : p.kt + ne++);
  }
  p.gpos_packed = p.lpos_packed = 0;
  for (uint32_t i = 0; i < p.nv; ++i) {
    p.gpos_packed |= uint64_t(p.gpos[i]) << (5u * i);
    p.lpos_packed |= uint64_t(p.lpos[i]) << (5u * i);
  }
  p.scratch_bytes = size_t(p.tiles) * p.slices * (size_t(1) << (2 * p.kt)) * 2 * sizeof(double);
  return p;
}

// tile t of the launch (row-major over the upper triangle of tile_rows x tile_rows tiles) -> its tile row and column
QHBM_RDM_HD inline void rdm_tile_of(uint32_t tile_rows, uint32_t t, uint32_t* ti, uint32_t* tj) {
  uint32_t i = 0;
  while (t >= tile_rows - i) {
    t -= tile_rows - i;
    ++i;
  }
  *ti = i;
  *tj = i + t;
}
// the blocks [*begin, *end) of slice s
QHBM_RDM_HD inline void rdm_slice_blocks(uint64_t blocks, uint32_t slices, uint32_t s, uint64_t* begin, uint64_t* end) {
  const uint64_t q = blocks / slices, r = blocks % slices;
  *begin = q * s + (s < r ? s : r);
  *end = *begin + q + (s < r ? 1u : 0u);
}
// panel element L -> its offset from the panel's first amplitude (index space) and its LDS slot
QHBM_RDM_HD inline void rdm_panel_offsets(const RdmPlan& p, uint32_t L, uint32_t* goff, uint32_t* slot) {
  uint32_t g = 0, s = 0;
  for (uint32_t i = 0; i < p.nv; ++i)
    if ((L >> i) & 1u) {
      g |= 1u << p.gpos[i];
      s |= 1u << p.lpos[i];
    }
  *goff = g;
  *slot = s;
}

}  // namespace qhbm
