  __shared__ __attribute__((aligned(16))) uint32_t gyx[2 * kTabEntries];
  __shared__ uint32_t nd[kMaxNodes + 1];
  __shared__ __attribute__((aligned(16))) uint32_t s_stage[kCountRowsW * kStageAlloc];
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
  uint32_t *stage = s_stage + (tid >> 6) * kStageAlloc;
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
  if (sb <= kStageSubBits) phases(std::true_type{});
  else phases(std::false_type{});
  if (lane == 0) {
    l_off[kDecThreads] = base;
    l_off[kDecThreads + 3] = rounds;
    l_off[kDecThreads + 4] = 0;   // one record per lane (no boundaries inside the lanes' ranges)
    l_off[kDecThreads + 2] = 3;   // boundaries of the write pass's chain of groups (no fence: the consumer is a later kernel)
  }
