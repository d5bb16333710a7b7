  // (Also included under a SHADOWED blockIdx -- k_stream_count / k_stream_count_w give a list entry's stream as
  // .y and 0 as .x: this body may read blockIdx.x and blockIdx.y only, never blockIdx.z or gridDim.)
  // Both tables as two arrays: the step words (gy), then their .x words (gx).
  __shared__ __attribute__((aligned(16))) uint32_t gyx[2 * kTabEntries];
  __shared__ __attribute__((aligned(16))) uint32_t s_pay[LDSPAY ? kPayWords : 4];   // the row's payload
  __shared__ uint32_t nd[kMaxNodes + 1];
  uint32_t *gy = gyx, *gx = gyx + kTabEntries;
  __shared__ uint32_t sm32[kDecThreads / 64];
  __shared__ StreamShared sh;
  const int f = blockIdx.y, tid = threadIdx.x;
  DecFrame *df = ws.frames + f;
  // One read for the whole workgroup: the LRES kernels run concurrently on the
  // other stream and may flag the frame while this kernel starts.
  if (tid == 0) {
    // The row walk ran beside k_dec_parse: its verdict counts if the parse passed.
    const int w = df->parse_status == 0 ? df->walk_status : 0;
    if (w && blockIdx.x == 0) atomicMax(&df->status, w);
    sh.flag = df->status | w;
  }
  __syncthreads();
  const int failed = sh.flag;
  if (!failed) {   // load_dec_tables with the count-only step words next to the long-code descriptors
    const uint32_t *nodes = ws.nodes + ((size_t)f * 2 + 1) * (kMaxNodes + 1);
    const int nn = df->s[1].num_nodes;
    for (int k = tid; k < nn; k += kDecThreads) nd[k] = nodes[k];
    const uint4 *gg = reinterpret_cast<const uint4 *>(ws.grp + ((size_t)f * 2 + 1) * (1u << kLutBits));
    const uint2 *gc = reinterpret_cast<const uint2 *>(ws.gyc + ((size_t)f * 2 + 1) * (1u << kLutBits));
    for (int k = tid; k < (1 << kLutBits) / 2; k += kDecThreads) {
      const uint4 q = gg[k];
      reinterpret_cast<uint2 *>(gx)[k] = make_uint2(q.x, q.z);   // long-code descriptors
      reinterpret_cast<uint2 *>(gy)[k] = gc[k];                  // count-only step words
    }
    const uint4 *gs = reinterpret_cast<const uint4 *>(ws.sub + ((size_t)f * 2 + 1) * kSubEntries);
    for (int k = tid; k < kSubEntries / 2; k += kDecThreads) {
      const uint4 q = gs[k];
      reinterpret_cast<uint2 *>(gx + (1 << kLutBits))[k] = make_uint2(q.x, q.z);
      reinterpret_cast<uint2 *>(gy + (1 << kLutBits))[k] = make_uint2(q.y, q.w);
    }
  }
  GrpTables tb;
  tb.grp = nullptr; tb.gx = gx; tb.gy = gy; tb.nd = nd;
  const uint8_t *p = packed + (size_t)f * in_stride;
  const int rb = r0 + (int)blockIdx.x * rows_per_wg;
  for (int r = rb; r < min(rb + rows_per_wg, r1); ++r) {
    const long long c_in = clock64();
    uint32_t *l_start = ws.lane_start + ((size_t)f * g.rows + r) * kDecThreads;
    uint32_t *l_off = ws.lane_off + ((size_t)f * g.rows + r) * (kDecThreads + kRecHdr);
    uint32_t *rc = ws.rc_stats ? ws.rc_stats + ((size_t)f * g.rows + r) * 8 : nullptr;
    if (tid == 0) { l_off[kDecThreads + 2] = 0; sh.dbg[0] = sh.dbg[1] = 0; }   // not usable until proven otherwise
    if (tid >= kRecWin && tid < kRecHdr) l_off[kDecThreads + tid] = ~0u;            // no window index yet (k_row_window checks what it finds)
    const uint32_t pay_off = ws.row_off[(size_t)f * g.rows + r], pay_len = ws.row_len[(size_t)f * g.rows + r];
    const unsigned long long rem = 8ull * pay_len;
    uint32_t sb = (uint32_t)((rem + kDecThreads - 1) / kDecThreads);
    sb = (sb + 31u) & ~31u;
    sb = sb < kMinSubBits ? kMinSubBits : sb;
    // More than one chunk: the fused kernel does it all.
    if (failed || sb > (uint32_t)g.max_sub || rem == 0 || g.row_block >= (1 << 22)) continue;
    GReader rd;
    const uint32_t rel0 = rd.attach(p, sizes[f], 8ull * pay_off);
    if (LDSPAY) {
      const uint32_t nd = (rel0 + (uint32_t)rem + 31u) / 32u;   // dwords that hold payload bits
      // A payload beyond the staging buffer is left to the row kernels, like a row of
      // several chunks.
      if (nd + kPayPad > (uint32_t)kPayWords) continue;
      __syncthreads();   // the previous row's readers are done with s_pay (and the tables are in)
      stage_payload(rd, s_pay, nd + kPayPad);
      __syncthreads();
      LReader lr;
      lr.w = (const __attribute__((address_space(3))) uint32_t *)s_pay;
      lr.jmax = nd + kPayPad - 1u;
      row_count_one(lr, tb, &sh, sm32, rel0, (uint32_t)rem, sb, (uint32_t)g.lead_bits, l_start, l_off, rc, c_in);
    } else {
      __syncthreads();   // the tables are in / the previous row is done with the exchange slots
      if (ws.lane_q)     // rows that go through windows: four records per lane
        row_count_one<GReader, true>(rd, tb, &sh, sm32, rel0, (uint32_t)rem, sb, (uint32_t)g.lead_bits, l_start, l_off, rc, c_in,
                                     ws.lane_q + ((size_t)f * g.rows + r) * (6 * kDecThreads), (uint32_t)g.row_block, kRowWindow);
      else
        row_count_one(rd, tb, &sh, sm32, rel0, (uint32_t)rem, sb, (uint32_t)g.lead_bits, l_start, l_off, rc, c_in);
    }
  }
