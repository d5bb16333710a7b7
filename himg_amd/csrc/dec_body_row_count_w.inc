  // (Also included under a SHADOWED blockIdx -- k_stream_count / k_stream_count_w give a list entry's stream as
  // .y and 0 as .x: this body may read blockIdx.x and blockIdx.y only, never blockIdx.z or gridDim.)
  __shared__ __attribute__((aligned(16))) uint32_t gyx[2 * kTabEntries];
  __shared__ uint32_t nd[kMaxNodes + 1];
  __shared__ __attribute__((aligned(16))) uint32_t s_stage[kCountRowsW * (NQ > 1 ? kLaneAlloc : kStageAlloc)];
  __shared__ int s_flag;
  uint32_t *gy = gyx, *gx = gyx + kTabEntries;
  const int f = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  DecFrame *df = ws.frames + f;
  if (tid == 0) {
    // The row walk ran beside k_dec_parse: its verdict counts if the parse passed.
    const int w = df->parse_status == 0 ? df->walk_status : 0;
    if (w && blockIdx.x == 0) atomicMax(&df->status, w);
    s_flag = df->status | w;
  }
  __syncthreads();
  const int failed = s_flag;
  if (!failed) {   // load_dec_tables with the count-only step words next to the long-code descriptors
    const uint32_t *nodes = ws.nodes + ((size_t)f * 2 + 1) * (kMaxNodes + 1);
    const int nn = df->s[1].num_nodes;
    for (int k = tid; k < nn; k += kDecThreads) nd[k] = nodes[k];
    const uint4 *gg = reinterpret_cast<const uint4 *>(ws.grp + ((size_t)f * 2 + 1) * (1u << kLutBits));
    for (int k = tid; k < (1 << kLutBits) / 2; k += kDecThreads) {
      const uint4 q = gg[k];
      reinterpret_cast<uint2 *>(gx)[k] = make_uint2(q.x, q.z);   // bytes / long-code descriptors
      // The step words of the WRITE pass's groups (at most four output bytes), not the
      // count-only ones: a row kernel that walks those groups from a lane's recorded start
      // follows exactly this kernel's chain and lands on the next lane's start -- no
      // token-by-token tail there (1.3 % more steps here than with the longer groups).
      reinterpret_cast<uint2 *>(gy)[k] = make_uint2(q.y, q.w);
    }
    const uint4 *gs = reinterpret_cast<const uint4 *>(ws.sub + ((size_t)f * 2 + 1) * kSubEntries);
    for (int k = tid; k < kSubEntries / 2; k += kDecThreads) {
      const uint4 q = gs[k];
      reinterpret_cast<uint2 *>(gx + (1 << kLutBits))[k] = make_uint2(q.x, q.z);
      reinterpret_cast<uint2 *>(gy + (1 << kLutBits))[k] = make_uint2(q.y, q.w);
    }
  }
  __syncthreads();
  GrpTables tb;
  tb.grp = nullptr; tb.gx = gx; tb.gy = gy; tb.nd = nd;
  const int r = r0 + (int)blockIdx.x * kCountRowsW + (tid >> 6);
  if (r >= r1) return;
  const uint8_t *p = packed + (size_t)f * in_stride;
  uint32_t *l_start = ws.lane_start + ((size_t)f * g.rows + r) * kDecThreads;
  uint32_t *l_off = ws.lane_off + ((size_t)f * g.rows + r) * (kDecThreads + kRecHdr);
  if (lane == 0) l_off[kDecThreads + 2] = 0;   // not usable until proven otherwise
  const uint32_t pay_off = ws.row_off[(size_t)f * g.rows + r], pay_len = ws.row_len[(size_t)f * g.rows + r];
  const unsigned long long rem64 = 8ull * pay_len;
  uint32_t sb = (uint32_t)((rem64 + kDecThreads - 1) / kDecThreads);
  sb = (sb + 31u) & ~31u;
  sb = sb < kMinSubBits ? kMinSubBits : sb;
  // More than one chunk, or nothing to do: the row kernels do it all (k_row_count's rule).
  if (failed || sb > (uint32_t)g.max_sub || rem64 == 0 || g.row_block >= (1 << 22)) return;
  const uint32_t rem = (uint32_t)rem64;
  GReader rd;
  const uint32_t rel0 = rd.attach(p, sizes[f], 8ull * pay_off);
  const uint32_t rel_end = rel0 + rem;
  const uint32_t lead = (uint32_t)g.lead_bits;
  uint32_t first = rel0;   // where the phase's first lane starts: exact
  uint32_t base = 0;       // symbols in front of the phase
  uint32_t rounds = 0;
  uint32_t *stage = s_stage + (tid >> 6) * (NQ > 1 ? kLaneAlloc : kStageAlloc);
  LdsBits bits;
  bits.base = lds_addr(stage);
  auto phases = [&](auto staged_c) {
  constexpr bool STAGED = decltype(staged_c)::value;
#pragma unroll 1
  for (int j = 0; j < kDecThreads / 64; ++j) {
    const int v = 64 * j + lane;
    const SubGrid q = sub_grid(rel0, rem, sb, v);
    const bool active = q.active;
    const uint32_t pb0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)q.b0);   // the phase's first lane: its nominal start
    if (pb0 >= rel_end) {   // a phase beyond the payload: its lanes own nothing
      l_start[v] = rem;
      l_off[v] = base;
      continue;
    }
    // STAGED: positions below are relative to the dword `w0` of the reader's window, the
    // first one staged: the one that holds the first bit of the phase's first lane.
    uint32_t shift = 0;
    if constexpr (STAGED) {
      const uint32_t w0 = pb0 >> 5;
      shift = 32u * w0;
      wave_lds_sync();   // the walks of the phase before are done with the buffer
      for (uint32_t k = (uint32_t)lane; 4u * k < kStageWords; k += 64u) {
        const uint32_t w = w0 + 4u * k;
        uint4 x;
        if (w + 3u <= rd.jmax) {
          const PackedU4 u = *reinterpret_cast<const PackedU4 *>(rd.w + w);
          x.x = u.x; x.y = u.y; x.z = u.z; x.w = u.w;
        } else {
          x.x = rd.ld(w); x.y = rd.ld(w + 1u); x.z = rd.ld(w + 2u); x.w = rd.ld(w + 3u);
        }
        // Blocks of 33 (see LdsBits): four dwords of one block, and the block's first dword
        // once more behind the block before it.
        uint32_t *d = stage + 4u * k + (k >> 3);
        d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w;
        if ((k & 7u) == 0u && k) d[-1] = x.x;
      }
      wave_lds_sync();
    }
    auto walk = [&](uint32_t from, uint32_t to, uint32_t *e, uint32_t *c, bool cont) {
      if constexpr (STAGED) { (void)cont; grp_count_lds(bits, tb, from, to, e, c); }
      else lean_count<true, GReader, true>(rd, tb, from, to, e, c, cont);
    };
    const uint32_t b0 = q.b0 - shift, lim = q.lim - shift, lo0 = rel0 - shift, fst = first - shift;
    uint32_t start = active ? b0 : rel_end - shift;
    if (lane == 0 && active) start = fst;
    // Lead-in (see lean_fixpoint): a boundary of the token chain at or past the nominal
    // start, found from lead_bits in front of it.
    bool at_start = false;   // the reader stands at `start`
    if (lane > 0 && active && lead) {
      uint32_t from = start - lo0 > lead ? start - lead : lo0;
      if (from < pb0 - shift) from = pb0 - shift;   // (a lead-in longer than a sub-sequence: not in front of the phase)
      uint32_t guess, none;
      walk(from, start, &guess, &none, false);
      start = guess;
      at_start = true;
    }
    uint32_t endpos = start, cnt = 0;
    bool dirty = active;
    // Re-join (see lean_fixpoint): the walk is cut at T = nominal start + kJoinBits; a lane
    // whose start moves in a later round walks up to T again, and if it arrives at the
    // same boundary everything behind is what it already has.  A round after the first
    // then costs the wavefront kJoinBits instead of a whole sub-sequence.
    uint32_t T = (active ? b0 : rel_end - shift) + kJoinBits;
    if (T > lim || T < b0) T = lim;
    uint32_t posT = ~0u, cT = 0;
    for (;;) {
      if (dirty) {
        uint32_t p1, c1;
        walk(start, T, &p1, &c1, at_start);
        if (p1 == posT) {
          cnt = c1 + (cnt - cT);
        } else {
          uint32_t c2;
          walk(p1, lim, &endpos, &c2, start < T || at_start);
          cnt = c1 + c2;
        }
        posT = p1;
        cT = c1;
        at_start = false;
      }
      // The chain: a lane starts where its left neighbour ended (one DPP move).
      const uint32_t ns = wave_shr1_dpp(fst, endpos);
      dirty = active && ns != start;
      if (active) start = ns;
      ++rounds;
      if (!__any(dirty ? 1 : 0)) break;
    }
    // Exclusive prefix of the counts (k_row_count's clamp: see row_count_one).
    const uint32_t c = min(cnt, 0x3fffffu);
    const uint32_t incl = wave_scan_add_dpp(c);
    l_start[v] = start + shift - rel0;
    l_off[v] = base + incl - c;
    if (v == q.last_active) l_off[kDecThreads + 1] = endpos + shift - rel0;
    base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    // The next phase starts where this one's last lane ended (a phase of inactive lanes: nowhere).
    first = (uint32_t)__builtin_amdgcn_readlane((int)(active ? endpos + shift : rel_end), 63);
  }
  };
  // ---- NQ > 1: a lane owns a STRETCH of NQ consecutive sub-sequences -------------------------
  // Lane l of phase j walks sub-sequences (64 j + l) NQ .. + NQ - 1 as one continuous chain, so a
  // row takes 16 / NQ phases and only the 64 stretch boundaries of a phase are speculative: one
  // lead-in and one re-join per stretch where the form above pays them per sub-sequence.  The
  // records are the same: the chain is the same chain, cut at the same nominal boundaries (every
  // walk below ends where the walk of a lane of the form above ends: at the first boundary of a
  // group at or past the sub-sequence's limit, a long code completed).
  // The wavefront goes through a stretch in NQ sub-steps.  Before each, every walking lane copies
  // the kLaneWords dwords from the dword of its CURRENT position to its own piece of the staging
  // buffer (LaneBits) -- the pieces of the lanes of a sub-step lie NQ sub-sequences apart, so
  // there is no contiguous range to stage.  A lane's boundaries inside its stretch (its marks) and
  // the symbols of each of its sub-sequences wait in the phase's own 64 NQ records, TRANSPOSED --
  // sub-step k of lane l at 64 k + l, so that a wave's store is one run of 64 dwords (at l NQ + k,
  // where the record belongs, it is 64 pieces NQ dwords apart: measured, 3.2 ms for NQ = 8).
  // Each word is written and read back by the same lane only.  When the phase's chain stands,
  // marks and offsets go through the (then idle) staging buffer into their places.
  // Re-join: a lane whose start moves walks to T again (as above); if it arrives where it did
  // before, everything behind stands and only the first count changes.  If not it walks on,
  // replacing marks and counts, until it meets one of its earlier marks or reaches the end of
  // the stretch.  Exact by induction from the phase's first lane, as above.
  auto stretches = [&]() {
    uint32_t *piece = stage + (uint32_t)lane * kLaneWords;
    LaneBits lb;
    lb.base = 0;
    // Lanes that are `on` copy their piece: the dwords from the one that holds bit `pos`.
    auto stage_at = [&](uint32_t pos, bool on) {
      wave_lds_sync();   // (the walks before are done with the pieces)
      if (on) {
        const uint32_t w0 = pos >> 5;
        if (w0 + kLaneWords - 1u <= rd.jmax) {
#pragma unroll
          for (uint32_t i = 0; i + 4u <= kLaneWords; i += 4u) {
            const PackedU4 u = *reinterpret_cast<const PackedU4 *>(rd.w + w0 + i);
            piece[i] = u.x; piece[i + 1u] = u.y; piece[i + 2u] = u.z; piece[i + 3u] = u.w;
          }
#pragma unroll
          for (uint32_t i = kLaneWords & ~3u; i < kLaneWords; ++i) piece[i] = rd.w[w0 + i];
        } else {   // the stream ends inside the piece: clamped, as the reader in place clamps
#pragma unroll 1
          for (uint32_t i = 0; i < kLaneWords; ++i) piece[i] = rd.ld(w0 + i);
        }
        lb.base = lds_addr(piece) - 4u * w0;
      }
      wave_lds_sync();
    };
    // sub_grid's boundaries, from the row's S (the grid is moved left so that the last active
    // sub-sequence is kTailBits long: see sub_grid).
    const uint32_t la = (rem - 1u) / sb, L = rem - la * sb;
    const uint32_t S = (L > kTailBits && la + 1u < (uint32_t)kDecThreads) ? sb - (L - kTailBits) : 0u;
    const uint32_t last_active = (rem - 1u + S) / sb;
    auto nom_b0 = [&](uint32_t v) { return v ? rel0 + v * sb - S : rel0; };
    auto nom_lim = [&](uint32_t v) { const uint32_t x = rel0 + (v + 1u) * sb - S; return x > rel_end ? rel_end : x; };
    const uint32_t lead_in = lead < 256u ? lead : 256u;   // (a piece holds a lead-in of up to 311 bits)
#pragma unroll 1
    for (int j = 0; j < kDecThreads / (64 * NQ); ++j) {
      const uint32_t v0 = (uint32_t)(64 * j + lane) * (uint32_t)NQ;
      const uint32_t b0 = nom_b0(v0);
      // sub-step k's word of this lane while the phase is walked: [64 k] of these
      uint32_t *t_start = l_start + 64 * NQ * j + lane, *t_off = l_off + 64 * NQ * j + lane;
      const bool active = b0 < rel_end;
      const uint32_t pb0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
      if (pb0 >= rel_end) {   // a phase beyond the payload: its lanes own nothing
#pragma unroll
        for (int k = 0; k < NQ; ++k) { t_start[64 * k] = rem; t_off[64 * k] = base; }
        continue;
      }
      uint32_t start = active ? b0 : rel_end;
      if (lane == 0) start = first;
      if (lead_in) {   // lead-in, as above
        const bool on = lane > 0 && active;
        const uint32_t from = start - rel0 > lead_in ? start - lead_in : rel0;
        stage_at(from, on);
        if (on) {
          uint32_t guess, none;
          grp_count_lds(lb, tb, from, start, &guess, &none);
          start = guess;
        }
      }
      uint32_t endpos = start, cnt0 = 0;
      bool dirty = active;
      uint32_t T = b0 + kJoinBits;
      { const uint32_t lim0 = nom_lim(v0); if (T > lim0 || T < b0) T = lim0; }
      uint32_t posT = ~0u, cT = 0;
      bool again = false;   // a round after the first: the lanes that walk have marks from before
      for (;;) {
        bool walking = dirty;
        uint32_t pos = start;
#pragma unroll 1
        for (int k = 0; k < NQ; ++k) {
          if (!__any(walking ? 1 : 0)) break;
          const uint32_t lim = nom_lim(v0 + (uint32_t)k);
          stage_at(pos, walking);
          if (walking) {
            uint32_t np = pos, c;
            if (k == 0) {
              uint32_t p1, c1;
              grp_count_lds(lb, tb, pos, T, &p1, &c1);
              if (p1 == posT) {
                c = c1 + (cnt0 - cT);
                walking = false;
              } else {
                uint32_t c2;
                grp_count_lds(lb, tb, p1, lim, &np, &c2);
                c = c1 + c2;
              }
              posT = p1;
              cT = c1;
              cnt0 = c;
            } else {
              grp_count_lds(lb, tb, pos, lim, &np, &c);
            }
            t_off[64 * k] = c;
            if (walking) {
              if (k + 1 < NQ) {
                uint32_t *m = t_start + 64 * (k + 1);
                if (again && *m == np - rel0) walking = false;   // met an earlier mark: the rest stands
                else *m = np - rel0;
              } else {
                endpos = np;
              }
              pos = np;
            }
          }
        }
        // The chain: a lane starts where its left neighbour's stretch ended (one DPP move).
        const uint32_t ns = wave_shr1_dpp(first, endpos);
        dirty = active && ns != start;
        if (active) start = ns;
        ++rounds;
        again = true;
        if (!__any(dirty ? 1 : 0)) break;
      }
      // Offsets: one scan over the lanes' stretch totals, then the partial sums inside a lane
      // (each count clamped like k_row_count's: see row_count_one).
      uint32_t tot = 0;
      if (active) {
#pragma unroll
        for (int k = 0; k < NQ; ++k) tot += min(t_off[64 * k], 0x3fffffu);
      }
      const uint32_t incl = wave_scan_add_dpp(tot);
      // Into place through the staging buffer, the starts and then the offsets: every lane's
      // words are in LDS before the first store lands on another lane's.
      wave_lds_sync();
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        const uint32_t v = v0 + (uint32_t)k;
        const bool a = nom_b0(v) < rel_end;
        if (v == last_active) l_off[kDecThreads + 1] = k + 1 < NQ ? t_start[64 * (k + 1)] : endpos - rel0;
        // (k = 0 of a lane with no sub-sequence of its own: rel_end, i.e. rem)
        stage[(uint32_t)lane * NQ + k] = k == 0 ? start - rel0 : (a ? t_start[64 * k] : rem);
      }
      wave_lds_sync();
#pragma unroll
      for (int k = 0; k < NQ; ++k) t_start[64 * k] = stage[64 * k + lane];
      wave_lds_sync();
      uint32_t off = base + incl - tot;
#pragma unroll
      for (int k = 0; k < NQ; ++k) {
        const bool a = nom_b0(v0 + (uint32_t)k) < rel_end;
        stage[(uint32_t)lane * NQ + k] = off;
        off += a ? min(t_off[64 * k], 0x3fffffu) : 0u;
      }
      wave_lds_sync();
#pragma unroll
      for (int k = 0; k < NQ; ++k) t_off[64 * k] = stage[64 * k + lane];
      base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
      first = (uint32_t)__builtin_amdgcn_readlane((int)(active ? endpos : rel_end), 63);
    }
  };
  if constexpr (NQ > 1) {
    if (sb <= kStageSubBits) stretches();
    else phases(std::false_type{});
  } else {
    if (sb <= kStageSubBits) phases(std::true_type{});
    else phases(std::false_type{});
  }
  if (lane == 0) {
    l_off[kDecThreads] = base;
    l_off[kDecThreads + 3] = rounds;
    l_off[kDecThreads + 4] = 0;   // one record per lane (no boundaries inside the lanes' ranges)
    l_off[kDecThreads + 2] = 3;   // boundaries of the write pass's chain of groups (no fence: the consumer is a later kernel)
  }
