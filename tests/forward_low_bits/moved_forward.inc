// moved_forward.inc -- plan_emulate.cpp's forward executor with the store of forward plans that move the low index bits
// (schedule.h PlanOptions::move_low_bits): a pass flagged PASS_RELABEL stores its tile through its relabel table, and the
// final state is read at logical = physical addresses.  Included by moved_plan_check.cpp inside namespace emu, after
// plan_emulate.cpp (whose helpers it uses); everything else is that executor, statement for statement.
bool emu_forward_moved(Emulation* e, uint32_t basis, bool skip_measure, ForwardResult* out, int* n_moving) {
  if (!e->err.empty()) return false;
  const Plan& plan = *e->plan;
  const Model& m = *e->m;
  EMU_REQUIRE(!plan.adjoint && plan.n_eff <= 20, "forward plan");
  const size_t N = size_t(1) << plan.n_eff;
  std::vector<cd> st(N, cd(kNaN, kNaN));  // dirty memory: nothing is zero unless a pass wrote a zero
  out->values.assign(size_t(m.n_ops), 0.0);
  out->have_final = false;
  const RecordLayout L(4, false);
  std::vector<cd> tile;
  std::vector<size_t> ad;  // the tile's addresses
  std::vector<double> wbuf;
  std::vector<char> written;
  std::vector<size_t> dest;
  *n_moving = 0;
  for (size_t pi = 0; pi < plan.passes.size(); ++pi) {
    const Pass& p = plan.passes[pi];
    if (skip_measure && p.is_measure_only) continue;
    const PassArgs& a = e->args[pi];
    // engine.cpp run_forward_chunk (keep_state: the final state is wanted)
    uint32_t flags = p.flags & (PASS_INIT_BASIS | PASS_GENERAL | PASS_NO_ZERO_FILL | PASS_RELABEL);  // engine.cpp forward_pass_args
    if (skip_measure) flags |= PASS_SKIP_MEASURE;
    if (!p.is_measure_only) flags |= PASS_STORE;
    const bool general = flags & PASS_GENERAL;
    const int K = p.K;
    EMU_REQUIRE(K >= kMinTileBits && K <= kMaxTileBits && a.c <= uint32_t(K) && a.n_free <= a.n_nonlocal && a.n_nonlocal + uint32_t(K) == a.n, "pass geometry");
    const uint32_t NT = 1u << (K - 4), TS = 1u << K;
    EMU_REQUIRE(size_t(a.spread_off) + (size_t(1) << (K - a.c)) <= e->tables.size(), "spread table");
    Geometry g{&a, &e->tables[a.spread_off], size_t(1) << (K - a.c), K, 0, 0, false};
    g.input(basis);
    EMU_REQUIRE(size_t(a.prog_off) < e->prog.size(), "program offset");
    const uint32_t* prog = &e->prog[a.prog_off];
    const size_t prog_n = e->prog.size() - a.prog_off;
    tile.assign(TS, cd(0.0, 0.0));
    ad.assign(TS, 0);
    for (uint32_t block = 0; block < (1u << a.n_free); ++block) {
      const uint32_t tile_id = g.launched_tile(block), tile_base = g.tile_base_of(tile_id);
      const uint32_t tile_hi = tile_id << K;
      for (uint32_t l = 0; l < TS; ++l) {
        ad[l] = g.addr(tile_base, l);
        EMU_REQUIRE(ad[l] < N, "tile address outside the state");
      }
      if (flags & PASS_INIT_BASIS) {
        if ((g.idx & a.nonlocal_mask) != tile_base) {
          if ((flags & PASS_STORE) && !(flags & PASS_NO_ZERO_FILL))
            for (uint32_t l = 0; l < TS; ++l) st[ad[l]] = cd(0.0, 0.0);
          continue;
        }
        for (uint32_t l = 0; l < TS; ++l) tile[l] = cd(0.0, 0.0);
        tile[g.in_local] = cd(1.0, 0.0);
      } else {
        for (uint32_t l = 0; l < TS; ++l) tile[l] = st[ad[l]];
        if (a.frozen_old_local)
          for (uint32_t l = 0; l < TS; ++l)
            if ((l ^ g.in_local) & a.frozen_old_local) tile[l] = cd(0.0, 0.0);
      }
      size_t pc = 0;
      for (;;) {
        EMU_REQUIRE(pc < prog_n, "program runs past its end");
        const uint32_t w0 = prog[pc], opc = w0 & 0xffu;
        if (opc == OP_END) break;
        if (opc == OP_ROUND) {
          Round r;
          if (!parse_round(e, prog + pc, prog_n - pc, K, false, &r)) return false;
          EMU_REQUIRE(size_t(a.tl_off) + size_t(r.tl) + NT <= e->tables.size(), "thread table");
          const uint32_t* TLt = &e->tables[size_t(a.tl_off) + r.tl];
          for (uint32_t tid = 0; tid < NT; ++tid) {
            const uint32_t TL = TLt[tid];
            EMU_REQUIRE((TL >> K) == 0, "thread table entry outside the tile");
            cd amp[16];
            for (int mm = 0; mm < 16; ++mm) amp[mm] = tile[TL | deposit(r, mm)];
            for (uint32_t i = 0; i < r.n_inst; ++i) {
              const size_t ro = size_t(r.first) + size_t(i) * size_t(L.words());
              instance_fwd(Record{&plan.coef_init[ro], &e->cf[ro]}, amp, TL | tile_hi, general);
            }
            for (int mm = 0; mm < 16; ++mm) tile[TL | deposit(r, mm)] = amp[mm];
          }
          pc += kRoundWords;
        } else if (opc == OP_GATE2) {
          EMU_REQUIRE(pc + kGate2Words <= prog_n, "gate2 words");
          if (general) {  // (the lean kernel variant steps over it)
            const uint32_t pw = prog[pc + 1], pos0 = pw & 0xffu, pos1 = (pw >> 8) & 0xffu;
            EMU_REQUIRE(pos0 < uint32_t(K) && pos1 < uint32_t(K) && pos0 != pos1, "gate2 bits");
            EMU_REQUIRE(size_t(prog[pc + 2]) + 32 <= e->cf.size(), "gate2 coefficients");
            const double* u = &e->cf[prog[pc + 2]];
            for (uint32_t q = 0; q < (1u << (K - 2)); ++q) {
              uint32_t ix[4];
              quad_indices(q, pos0, pos1, ix);
              cd x[4], y[4];
              for (int j = 0; j < 4; ++j) x[j] = tile[ix[j]];
              mat4_apply(u, x, y);
              for (int j = 0; j < 4; ++j) tile[ix[j]] = y[j];
            }
          }
          pc += kGate2Words;
        } else if (opc == OP_MEASURE_WHT) {
          const size_t n_terms = w0 >> 8;
          EMU_REQUIRE(pc + kWhtHeaderWords + n_terms * kMeasTermWords <= prog_n, "wht words");
          const uint32_t* class_end = prog + pc + 1;
          const uint32_t* terms = prog + pc + kWhtHeaderWords;
          pc += size_t(kWhtHeaderWords) + n_terms * kMeasTermWords;
          if (flags & PASS_SKIP_MEASURE) continue;
          // |psi|^2 through a Walsh-Hadamard transform over ALL local bits: the kernel transforms register and lane bits and
          // adds the waves with the parity of the term's wave bits, which is the same sum; the REGISTER part of the
          // coefficient it reads is the class the term sits in, not the term's own mask
          wbuf.resize(TS);
          for (uint32_t l = 0; l < TS; ++l) wbuf[l] = std::norm(tile[l]);
          wht_inplace(wbuf);
          uint32_t begin = 0;
          for (uint32_t c = 0; c < 16; ++c) {
            const uint32_t end = class_end[c];
            for (uint32_t k = begin; k < end; ++k) {  // (begin >= end: the kernel's loop does not run either)
              EMU_REQUIRE(k < n_terms, "class table runs past the terms");
              const uint32_t* tw = terms + size_t(k) * kMeasTermWords;
              const uint32_t zl = tw[0], zn = tw[1], op = tw[3];
              float cf;
              std::memcpy(&cf, &tw[2], 4);
              EMU_REQUIRE(op < uint32_t(m.n_ops), "wht operator index");
              const uint32_t zeff = (c << (K - 4)) | (zl & (NT - 1u));
              const double v = double(cf) * wbuf[zeff];
              out->values[op] += (popc(tile_base & zn) & 1) ? -v : v;
            }
            begin = end;
          }
        } else if (opc == OP_MEASURE) {
          const uint32_t n_groups = w0 >> 8;
          ++pc;
          for (uint32_t gi = 0; gi < n_groups; ++gi) {
            EMU_REQUIRE(pc + 2 <= prog_n, "measure group words");
            const uint32_t xl = prog[pc], n_terms = prog[pc + 1];
            pc += 2;
            EMU_REQUIRE(pc + size_t(n_terms) * kMeasTermWords <= prog_n, "measure term words");
            if (flags & PASS_SKIP_MEASURE) { pc += size_t(n_terms) * kMeasTermWords; continue; }
            EMU_REQUIRE((xl >> K) == 0, "measure x mask outside the tile");
            for (uint32_t k = 0; k < n_terms; ++k, pc += kMeasTermWords) {
              const uint32_t zl = prog[pc] & (TS - 1u), zn = prog[pc + 1], ow = prog[pc + 3];
              float cf;
              std::memcpy(&cf, &prog[pc + 2], 4);
              const uint32_t op = ow & 0xffffffu, ny = ow >> 24;
              EMU_REQUIRE(op < uint32_t(m.n_ops), "operator index");
              double sum = 0.0;  // Re(i^ny (-1)^popc(l & z) conj(psi[l ^ x]) psi[l]): ny = 0: wr, 1: -wi, 2: -wr, 3: wi
              for (uint32_t l = 0; l < TS; ++l) {
                const cd q = tile[l ^ xl], pp = tile[l];
                const double v = (ny & 1u) ? q.real() * pp.imag() - q.imag() * pp.real() : q.real() * pp.real() + q.imag() * pp.imag();
                sum += (popc(l & zl) & 1) ? -v : v;
              }
              double sfac = (ny == 1 || ny == 2) ? -double(cf) : double(cf);
              if (popc(tile_base & zn) & 1) sfac = -sfac;
              out->values[op] += sfac * sum;
            }
          }
        } else {
          EMU_REQUIRE(false, "unknown opcode");
        }
      }
      if ((flags & PASS_STORE) && (flags & PASS_RELABEL)) {
        // kernels.hip store_tile_moved: out-index o -> tables[relabel_off + 2 o] = (local index, offset in the state), pairs of
        // consecutive o in one 16-byte store, the odd one's local index = the even one's | relabel_l1
        EMU_REQUIRE(a.n_fz == 0 && a.frozen_new_local == 0 && a.relabel_pairs == 1, "a forward moving store has no finished bit");
        EMU_REQUIRE(size_t(a.relabel_off) + 2 * size_t(TS) <= e->tables.size() && a.relabel_off % 4 == 0, "moving-store table");
        const uint32_t* tab = &e->tables[a.relabel_off];
        written.assign(TS, 0);
        for (uint32_t o = 0; o < TS; o += 2) {
          const uint32_t l = tab[2 * o], off = tab[2 * o + 1];
          for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t lh = h ? (l | a.relabel_l1) : l;
            const size_t at = size_t(tile_base | off) + h;
            EMU_REQUIRE(lh < TS && at < N && (off & 1u) == 0, "moving store outside the tile or the state");
            EMU_REQUIRE(tab[2 * (o + h)] == lh && size_t(tile_base | tab[2 * (o + h) + 1]) == at, "moving-store table is not made of pairs");
            EMU_REQUIRE(!written[lh], "moving store reads a tile amplitude twice");
            written[lh] = 1;
            dest.push_back(at);
            st[at] = tile[lh];
          }
        }
        // in place: the addresses written are the addresses the tile was loaded from
        std::vector<size_t> from(ad.begin(), ad.end());
        std::sort(from.begin(), from.end());
        std::sort(dest.begin(), dest.end());
        EMU_REQUIRE(from == dest, "moving store is not a permutation of the tile's own addresses");
        dest.clear();
        if (block == 0) ++*n_moving;
      } else if (flags & PASS_STORE) {
        for (uint32_t l = 0; l < TS; ++l) st[ad[l]] = tile[l];
      }
    }
    if (p.completes_circuit) {  // every consumer of final states reads logical = physical addresses
      out->final_state.assign(st.begin(), st.end());
      out->have_final = true;
    }
  }
  if (!skip_measure)  // measure_global_kernel on the final state in memory (forward plans: logical = physical addresses)
    for (int ti : plan.global_terms) {
      EMU_REQUIRE(ti >= 0 && size_t(ti) < m.terms.size(), "global term index");
      const PauliTerm& t = m.terms[size_t(ti)];
      EMU_REQUIRE(size_t(t.x) < N, "global term x mask");
      const uint32_t ny = uint32_t(t.ny) & 3u;  // (DevTerm::ny is the number of Y factors; the kernel reduces it)
      double acc = 0.0;
      for (size_t j = 0; j < N; ++j) {
        const cd q = st[j ^ t.x], own = st[j];
        const double wr = q.real() * own.real() + q.imag() * own.imag(), wi = q.real() * own.imag() - q.imag() * own.real();
        double v = (ny & 1u) ? wi : wr;
        if (ny == 1u || ny == 2u) v = -v;
        acc += (popc(uint32_t(j) & t.z) & 1) ? -v : v;
      }
      out->values[size_t(t.op)] += acc * double(t.coeff);
    }
  return true;
}
