// rdm_index_check -- the index arithmetic and launch plan of the reduced density matrix (csrc/rdm_index.h) on the CPU.
//
// For every register of n <= 12 qubits and every keep mask with 1 <= k <= min(n, 10):
//   1. (a, b) -> index is a bijection onto [0, 2^n), and index -> (a, b) inverts it;
//   2. (a, b) -> index agrees with the convention restated here bit by bit: qubit 0 is the most significant index bit, a
//      reads the kept qubits big-endian in ascending qubit order, b the others;
//   3. the plan's tiles cover the upper triangle of rho_A exactly once (entries of a diagonal tile below the diagonal
//      are the ones the finish kernel skips);
//   4. the plan's slices -- walked as rdm_tile_kernel walks them: rdm_slice_blocks, a deposit for the first block, the
//      masked increment and the carry into the next state for the following ones, the panel's words dealt to 256 threads
//      by rdm_thread_part / rdm_word_part (held to rdm_panel_offsets element by element), stored at rdm_lds_slot and read
//      back as the register blocks read them -- cover every (m, b) exactly once for every row of a tile row, read only
//      amplitudes of the right state, 16-byte aligned, and store every LDS slot below the panel's 2048 once.  With one
//      or three states every slice is a single block at these sizes, so plans with 1500 states (n <= 4) and 700 states
//      (n = 12, k <= 2, where a state has several blocks) are walked too: the program counts the blocks it reached through
//      the increment and the state boundaries it crossed inside a slice, and fails if there were none;
//   5. scratch_bytes equals the highest byte the tile kernel writes, every partial is written once, and the finish
//      kernel reads only written partials.
// Its own main; built with -fsanitize=address,undefined by its makefile.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "rdm_index.h"

using namespace qhbm;

static long failures = 0;
static long carried_blocks = 0, state_crossings = 0;  // blocks reached by the masked increment / by ++m inside a slice
#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      if (++failures <= 20) {              \
        std::printf("FAIL %s: ", #cond);   \
        std::printf(__VA_ARGS__);          \
        std::printf("\n");                 \
      }                                    \
    }                                      \
  } while (0)

// the convention, restated without the header's helpers
static uint32_t restated_index(int n, uint64_t keep_mask, uint32_t a, uint32_t b) {
  int k = 0;
  for (int q = 0; q < n; ++q) k += int((keep_mask >> q) & 1u);
  uint32_t idx = 0;
  int ia = 0, ib = 0;  // kept / environment qubits seen so far, in ascending qubit order
  for (int q = 0; q < n; ++q) {
    uint32_t bit;
    if ((keep_mask >> q) & 1u) {
      bit = (a >> (k - 1 - ia)) & 1u;  // big-endian: the first kept qubit is a's most significant bit
      ++ia;
    } else {
      bit = (b >> (n - k - 1 - ib)) & 1u;
      ++ib;
    }
    idx |= bit << (n - 1 - q);  // qubit 0 is the most significant index bit
  }
  return idx;
}

static void check_mask(int n, uint64_t keep_mask, int M, bool walk) {
  CHECK(rdm_check(n, keep_mask) == 0, "n %d mask %llx", n, (unsigned long long)keep_mask);
  const RdmPlan p = rdm_plan(n, keep_mask, M);
  const uint32_t D = 1u << p.k, E = 1u << (p.n - p.k), N = 1u << n;
  // 1, 2
  std::vector<uint8_t> seen(N, 0);
  for (uint32_t a = 0; a < D; ++a)
    for (uint32_t b = 0; b < E; ++b) {
      const uint32_t idx = rdm_amp_index(p.masks, a, b);
      CHECK(idx < N, "index %u of 2^%d", idx, n);
      if (idx >= N) continue;
      CHECK(idx == restated_index(n, keep_mask, a, b), "n %d mask %llx a %u b %u", n, (unsigned long long)keep_mask, a, b);
      ++seen[idx];
      uint32_t a2, b2;
      rdm_split_index(p.masks, idx, &a2, &b2);
      CHECK(a2 == a && b2 == b, "split of %u", idx);
    }
  for (uint32_t i = 0; i < N; ++i) CHECK(seen[i] == 1, "index %u hit %d times", i, int(seen[i]));
  if (!walk) return;

  // 3
  const uint32_t TE = 1u << p.kt;
  CHECK(p.tile_rows * TE == D && p.tiles == p.tile_rows * (p.tile_rows + 1) / 2, "tiles of n %d k %u", n, p.k);
  CHECK(p.rb * p.rb * p.group == TE * TE && p.group <= kRdmThreads && kRdmThreads % p.group == 0, "register blocks");
  std::vector<uint8_t> upper(size_t(D) * D, 0);
  for (uint32_t t = 0; t < p.tiles; ++t) {
    uint32_t ti, tj;
    rdm_tile_of(p.tile_rows, t, &ti, &tj);
    CHECK(ti <= tj && tj < p.tile_rows, "tile %u -> (%u, %u)", t, ti, tj);
    for (uint32_t r = 0; r < TE; ++r)
      for (uint32_t c = 0; c < TE; ++c) {
        const uint32_t row = ti * TE + r, col = tj * TE + c;
        if (col < row) continue;  // (rdm_finish_kernel returns)
        if (row < D && col < D) ++upper[size_t(row) * D + col];
      }
  }
  for (uint32_t r = 0; r < D; ++r)
    for (uint32_t c = 0; c < D; ++c) CHECK(upper[size_t(r) * D + c] == (c >= r ? 1 : 0), "entry (%u, %u)", r, c);

  // 4: one tile row is enough for the environment walk (the tile only moves base_i); take the last
  CHECK(p.nv == p.kt + p.le && p.nv >= 1 && p.nv <= uint32_t(kRdmPanelBits) && p.gpos[0] == 0, "panel bits");
  CHECK(p.slices >= 1 && p.slices <= kRdmMaxSlices && p.slices <= p.blocks, "slices %u of %llu blocks", p.slices,
        (unsigned long long)p.blocks);
  CHECK(p.blocks == (uint64_t(M) << (p.n - p.k - p.le)), "blocks");
  const uint32_t ti = p.tile_rows - 1, base_i = rdm_deposit(ti << p.kt, p.masks.keep);
  std::vector<uint8_t> env_seen(size_t(M) * E * TE, 0);
  uint64_t expect_begin = 0;
  for (uint32_t s = 0; s < p.slices; ++s) {
    uint64_t begin, end;
    rdm_slice_blocks(p.blocks, p.slices, s, &begin, &end);
    CHECK(begin == expect_begin && end > begin, "slice %u", s);
    expect_begin = end;
    uint64_t m = begin / p.blocks_per_state;
    uint32_t hi = rdm_deposit(uint32_t(begin % p.blocks_per_state), p.env_hi);
    for (uint64_t blk = begin; blk < end; ++blk) {
      CHECK(m < uint64_t(M), "state %llu", (unsigned long long)m);
      CHECK(hi == rdm_deposit(uint32_t(blk % p.blocks_per_state), p.env_hi), "increment at block %llu", (unsigned long long)blk);
      // the panel as the kernel's 256 threads store it: thread tid, word w -> elements 2 (tid + 256 w) and the next one
      std::vector<uint32_t> lds(size_t(1) << p.nv, ~0u);
      const uint32_t pairs = 1u << (p.nv - 1), slot1 = 1u << rdm_packed(p.lpos_packed, 0);
      for (uint32_t tid = 0; tid < kRdmThreads; ++tid) {
        uint32_t goff_t, slot_t;
        rdm_thread_part(p.gpos_packed, p.lpos_packed, p.nv, tid, &goff_t, &slot_t);
        for (uint32_t w = 0; w < 4; ++w) {
          if (tid + kRdmThreads * w >= pairs) continue;
          uint32_t goff_w, slot_w;
          rdm_word_part(p.gpos_packed, p.lpos_packed, p.nv, w, &goff_w, &slot_w);
          for (uint32_t second = 0; second < 2; ++second) {
            const uint32_t L = 2 * (tid + kRdmThreads * w) + second;
            const uint32_t goff = (goff_t | goff_w) + second, slot = slot_t | slot_w | (second ? slot1 : 0u);
            uint32_t goff_ref, slot_ref;
            rdm_panel_offsets(p, L, &goff_ref, &slot_ref);
            CHECK(goff == goff_ref && slot == slot_ref, "thread %u word %u: (%u, %u) against element %u's (%u, %u)", tid, w,
                  goff, slot, L, goff_ref, slot_ref);
            const uint32_t idx = base_i | hi | goff;
            CHECK((base_i & hi) == 0 && ((base_i | hi) & (goff_t | goff_w)) == 0, "overlapping parts");
            CHECK(idx < N && slot < (1u << p.nv), "panel element %u", L);
            if (!second) CHECK((idx & 1u) == 0, "word of element %u is not 16-byte aligned", L);
            const uint32_t at = rdm_lds_slot(p.kt, slot);
            CHECK(at < (1u << p.nv), "LDS slot %u of element %u", at, L);
            if (at < (1u << p.nv)) {
              CHECK(lds[at] == ~0u, "LDS slot %u stored twice", at);
              lds[at] = idx;
            }
          }
        }
      }
      // ... and as the register blocks read it: rows 4 j .. 4 j + 3 (2 j, 2 j + 1 at kt = 1) of value e, from one swizzled base
      for (uint32_t e = 0; e < (1u << p.le); ++e)
        for (uint32_t r = 0; r < TE; ++r) {
          const uint32_t at = rdm_lds_slot(p.kt, e * TE + (r / p.rb) * p.rb) + r % p.rb;
          CHECK(at < (1u << p.nv) && lds[at] != ~0u, "read of (r %u, e %u) at slot %u", r, e, at);
          if (at >= (1u << p.nv) || lds[at] == ~0u) continue;
          uint32_t a, b;
          rdm_split_index(p.masks, lds[at], &a, &b);
          CHECK(a == ti * TE + r, "row at (r %u, e %u): %u", r, e, a);
          CHECK((b & ((1u << p.le) - 1u)) == e && rdm_deposit(b >> p.le, p.env_hi) == hi, "environment value at (r %u, e %u)", r, e);
          if (m < uint64_t(M) && b < E) ++env_seen[(size_t(m) * E + b) * TE + r];
        }
      if (blk > begin) {
        ++carried_blocks;
        if (hi == 0) ++state_crossings;
      }
      hi = rdm_masked_inc(hi, p.env_hi);
      if (hi == 0) ++m;
    }
  }
  CHECK(expect_begin == p.blocks, "slices end at %llu", (unsigned long long)expect_begin);
  for (size_t i = 0; i < env_seen.size(); ++i) CHECK(env_seen[i] == 1, "(m, b, r) %zu read %d times", i, int(env_seen[i]));

  // 5: the tile kernel's writes (per tile, slice, thread position, register) against scratch_bytes and the finish's reads
  const size_t doubles = p.scratch_bytes / sizeof(double);
  std::vector<uint8_t> written(doubles, 0);
  size_t highest = 0;
  const uint32_t TB = TE / p.rb;
  for (uint32_t t = 0; t < p.tiles; ++t)
    for (uint32_t s = 0; s < p.slices; ++s) {
      const size_t out = (size_t(t) * p.slices + s) << (2 * p.kt + 1);
      for (uint32_t pos = 0; pos < p.group; ++pos)
        for (uint32_t q = 0; q < p.rb * p.rb; ++q) {
          const uint32_t row = (pos / TB) * p.rb + q / p.rb, col = (pos % TB) * p.rb + q % p.rb;
          for (uint32_t part = 0; part < 2; ++part) {
            const size_t at = out + (size_t(row) * TE + col) * 2 + part;
            if (at < doubles) ++written[at];
            if (at + 1 > highest) highest = at + 1;
          }
        }
    }
  CHECK(highest * sizeof(double) == p.scratch_bytes, "scratch %zu, written %zu", p.scratch_bytes, highest * sizeof(double));
  for (size_t i = 0; i < doubles; ++i) CHECK(written[i] == 1, "partial %zu written %d times", i, int(written[i]));
}

int main() {
  long masks = 0;
  for (int n = 1; n <= 12; ++n)
    for (uint64_t mask = 1; mask < (uint64_t(1) << n); ++mask) {
      const int k = rdm_popcount(mask);
      if (k > 10) {
        CHECK(rdm_check(n, mask) == 3, "k = %d accepted", k);
        continue;
      }
      ++masks;
      check_mask(n, mask, 1, true);
      if ((mask % 7) == 0) check_mask(n, mask, 3, true);
      // more blocks than slices: a slice then walks the masked increment and carries m from one state into the next
      if (n <= 4 || (n == 12 && k <= 2 && (mask % 5) == 0)) check_mask(n, mask, n <= 4 ? 1500 : 700, true);
    }
  CHECK(carried_blocks > 10000 && state_crossings > 5000, "the walk carried %ld blocks and crossed %ld states", carried_blocks,
        state_crossings);
  // refusals, and plans that must stay in range at the interface's limits
  CHECK(rdm_check(0, 1) == 1 && rdm_check(32, 1) == 1, "n outside [1, 31]");
  CHECK(rdm_check(4, 0) == 3 && rdm_check(12, 0x7ff) == 3, "k outside [1, 10]");
  CHECK(rdm_check(4, 0x10) == 2, "mask bit at n");
  for (uint64_t mask : {uint64_t(1), uint64_t(1) << 30, uint64_t(0x3ff), uint64_t(0x3ff) << 21, uint64_t(0x15555555) & 0x3ffff}) {
    const RdmPlan p = rdm_plan(31, mask, kRdmMaxStates);
    CHECK(rdm_check(31, mask) == 0, "31 qubits");
    CHECK((p.masks.keep | p.masks.env) == 0x7fffffffu && (p.masks.keep & p.masks.env) == 0, "masks at 31 qubits");
    CHECK(p.blocks == (uint64_t(kRdmMaxStates) << (31 - p.k - p.le)) && p.slices <= kRdmMaxSlices, "blocks at 31 qubits");
    uint64_t begin, end;
    rdm_slice_blocks(p.blocks, p.slices, p.slices - 1, &begin, &end);
    CHECK(end == p.blocks, "last slice at 31 qubits");
  }
  std::printf("rdm_index_check: %ld masks\n", masks);
  std::printf("rdm_index_check: %ld blocks reached by the increment inside a slice, %ld of them in the next state\n", carried_blocks,
              state_crossings);
  std::printf("rdm_index_check: %ld failures\n", failures);
  return failures ? 1 : 0;
}
